// lupin_lightmap.hpp -- lightmap baking, included once by lupin_hip.hip after lupin_rays.hpp.
//
// lupin_hip_bake_lightmap turns a scene and a UV layout into an atlas of irradiance: the charts' triangles are rasterised
// into texels, every owned texel becomes a mode-1 ray record on the surface point its centre maps to, the records are
// path-traced by the radiance query (lupin_rays.hpp) and the result is scattered back and dilated into the gutters.
//
//   k_lm_raster    one wave64 per (chart, triangle) pair; lanes stride the texels of the triangle's clamped bounding box;
//                  atomicMin of the pair's key on a u32 owner plane (the smallest key owns a centre: no scheduling shows)
//   k_lm_count     owned texels per block of LP_BLOCK texels (ballot + popcount per wave)
//   k_lm_scan      one block: exclusive scan of the block totals in place, the grand total beside them
//   k_lm_emit      order-preserving compaction: the record and the texel index of every owned texel, ascending
//   (lupin_hip_pathtrace_rays on the compacted device records)
//   k_lm_scatter   pi * mean radiance and alpha 1 to the texel, the record to its place in the record plane if asked
//   k_lm_dilate    one gutter pass, ping-pong
//   k_lm_ao_scatter  lupin_hip_bake_lightmap_ao's k_lm_scatter: visibility and bent normal from the bent-normal query's sums
//   (lupin_hip_bake_lightmap_directional's resolve and scatter kernels are in lupin_lightmap_directional.hpp)
//
// Geometry is read from plain global memory (GeoGlobal): every triangle is fetched once per wave in the raster and once per
// owned texel in the emit, neighbouring texels share it through the cache, and nothing here iterates over a hierarchy --
// staging the scene in LDS would cost more than the reads it saves.
// Every operation is f32 without contraction (-ffp-contract=off), IEEE division and sqrt; tests/lightmap_ref.py restates
// the rasterisation rule, the records and the dilation operation for operation.
#pragma once

#include "lupin_rays.hpp"

constexpr uint32_t LP_LM_NO_OWNER = 0xFFFFFFFFu;
constexpr uint32_t LP_LM_SMOOTH_NORMALS = 1u;   // LUPIN_LIGHTMAP_SMOOTH_NORMALS
constexpr uint32_t LP_LM_SCAN_THREADS = 1024;

// one chart on the device: the instance, the key of its first triangle, its place in the atlas, and the lightmap UV set of
// the instance's mesh (lupin_hip_scene_set_lightmap_uvs: one float2 per triangle corner, the mesh's first corner first), or
// nullptr: the chart reads the mesh's texcoords
struct LmChartDev
{
    uint32_t inst, key_base, tri_count, pad;
    float scale_u, scale_v, offset_u, offset_v;
    const float2 *lm_uvs;
};

struct LmTri   // a triangle in texel space
{
    float x0, y0, x1, y1, x2, y2;
    float area2;      // edge(t0, t1, t2) as computed (its sign: the chart's orientation)
    bool ok;          // finite UVs, area2 finite and not zero
    uint32_t gtri;    // global triangle
    MeshDev mesh;
    uint32_t i0, i1, i2;
};

LP_DEV float lm_edge(float ax, float ay, float bx, float by, float px, float py)
{
    return (bx - ax) * (py - ay) - (by - ay) * (px - ax);
}

// the chart a key belongs to: the last chart whose key_base is <= key (charts without triangles share their successor's base)
LP_DEV uint32_t lm_chart_of(const LmChartDev *__restrict__ charts, uint32_t num_charts, uint32_t key)
{
    uint32_t lo = 0, hi = num_charts - 1;
    while (lo < hi)
    {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (charts[mid].key_base <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}

LP_DEV LmTri lm_triangle(const SceneDev &sc, const LmChartDev &ch, uint32_t tri, float Wf, float Hf)
{
    LmTri t;
    t.mesh = sc.inst_meshes[ch.inst];
    t.gtri = t.mesh.tri_offset + tri;
    t.i0 = sc.tri_indices[(size_t)t.gtri * 3 + 0];
    t.i1 = sc.tri_indices[(size_t)t.gtri * 3 + 1];
    t.i2 = sc.tri_indices[(size_t)t.gtri * 3 + 2];
    const float2 a = ch.lm_uvs ? ch.lm_uvs[(size_t)tri * 3 + 0] : sc.texcoords[t.mesh.texcoords_base + t.i0];
    const float2 b = ch.lm_uvs ? ch.lm_uvs[(size_t)tri * 3 + 1] : sc.texcoords[t.mesh.texcoords_base + t.i1];
    const float2 c = ch.lm_uvs ? ch.lm_uvs[(size_t)tri * 3 + 2] : sc.texcoords[t.mesh.texcoords_base + t.i2];
    t.x0 = (a.x * ch.scale_u + ch.offset_u) * Wf; t.y0 = (a.y * ch.scale_v + ch.offset_v) * Hf;
    t.x1 = (b.x * ch.scale_u + ch.offset_u) * Wf; t.y1 = (b.y * ch.scale_v + ch.offset_v) * Hf;
    t.x2 = (c.x * ch.scale_u + ch.offset_u) * Wf; t.y2 = (c.y * ch.scale_v + ch.offset_v) * Hf;
    t.area2 = lm_edge(t.x0, t.y0, t.x1, t.y1, t.x2, t.y2);
    t.ok = ray_component_finite(a.x) && ray_component_finite(a.y) && ray_component_finite(b.x) && ray_component_finite(b.y) &&
           ray_component_finite(c.x) && ray_component_finite(c.y) && ray_component_finite(t.area2) && t.area2 != 0.0f;
    return t;
}

// the three edge values at a centre, oriented so that inside is >= 0; `area2` comes back oriented the same way
LP_DEV bool lm_covers(const LmTri &t, float cx, float cy, float &e1, float &e2, float &area2)
{
    float e0 = lm_edge(t.x1, t.y1, t.x2, t.y2, cx, cy);
    e1 = lm_edge(t.x2, t.y2, t.x0, t.y0, cx, cy);
    e2 = lm_edge(t.x0, t.y0, t.x1, t.y1, cx, cy);
    area2 = t.area2;
    if (t.area2 < 0.0f) { e0 = -e0; e1 = -e1; e2 = -e2; area2 = -area2; }
    return e0 >= 0.0f && e1 >= 0.0f && e2 >= 0.0f;
}

// texel columns (or rows) floor(lo) .. floor(hi) of a span, clamped to [0, size] IN FLOAT first: a coordinate of 1e30 or
// below zero never reaches an integer conversion.  first > last: nothing inside.
LP_DEV void lm_span(float a, float b, float c, float sizef, uint32_t size, uint32_t &first, uint32_t &last)
{
    const float lo = clampf(minf(minf(a, b), c), 0.0f, sizef), hi = clampf(maxf(maxf(a, b), c), 0.0f, sizef);
    first = f2u_sat(floorf(lo));
    last = f2u_sat(floorf(hi));
    if (last > size - 1u) last = size - 1u;
}

__global__ void __launch_bounds__(LP_BLOCK) k_lm_raster(SceneDev sc, const LmChartDev *__restrict__ charts, uint32_t num_charts, uint32_t total_keys,
                                                        uint32_t W, uint32_t H, uint32_t *__restrict__ owner)
{
    const uint32_t key = blockIdx.x * (LP_BLOCK / 64u) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (key >= total_keys) return;
    const LmChartDev ch = charts[lm_chart_of(charts, num_charts, key)];
    const float Wf = (float)W, Hf = (float)H;
    const LmTri t = lm_triangle(sc, ch, key - ch.key_base, Wf, Hf);
    if (!t.ok) return;
    uint32_t x0, x1, y0, y1;
    lm_span(t.x0, t.x1, t.x2, Wf, W, x0, x1);
    lm_span(t.y0, t.y1, t.y2, Hf, H, y0, y1);
    if (x0 > x1 || y0 > y1) return;
    const uint32_t bw = x1 - x0 + 1u, count = bw * (y1 - y0 + 1u);   // <= 16384^2
    for (uint32_t i = lane; i < count; i += 64u)
    {
        const uint32_t ry = i / bw;
        const uint32_t x = x0 + (i - ry * bw), y = y0 + ry;   // x <= x1 < W, y <= y1 < H
        float e1, e2, area2;
        if (lm_covers(t, (float)x + 0.5f, (float)y + 0.5f, e1, e2, area2)) atomicMin(&owner[(size_t)y * W + x], key);
    }
}

// owned texels of this thread's block before this thread (`before`) and in the whole block (`total`)
LP_DEV void lm_block_rank(bool owned, uint32_t *lds_wave, uint32_t &before, uint32_t &total)
{
    const unsigned long long mask = __ballot(owned);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) lds_wave[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    before = (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
    total = 0u;
    for (uint32_t w = 0; w < LP_BLOCK / 64u; w++)
    {
        if (w < wave) before += lds_wave[w];
        total += lds_wave[w];
    }
}

__global__ void __launch_bounds__(LP_BLOCK) k_lm_count(const uint32_t *__restrict__ owner, uint32_t texels, uint32_t *__restrict__ block_totals)
{
    __shared__ uint32_t lds_wave[LP_BLOCK / 64u];
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    const bool owned = i < texels && owner[i] != LP_LM_NO_OWNER;
    uint32_t before, total;
    lm_block_rank(owned, lds_wave, before, total);
    if (threadIdx.x == 0u) block_totals[blockIdx.x] = total;
}

// one block: totals[0 .. n) become their exclusive prefix sums, totals[n] the grand total (<= 2^28: texels)
__global__ void __launch_bounds__(LP_LM_SCAN_THREADS) k_lm_scan(uint32_t *__restrict__ totals, uint32_t n)
{
    __shared__ uint32_t lds[LP_LM_SCAN_THREADS];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0u) carry = 0u;
    __syncthreads();
    for (uint32_t first = 0; first < n; first += LP_LM_SCAN_THREADS)
    {
        const uint32_t i = first + threadIdx.x;
        const uint32_t mine = i < n ? totals[i] : 0u;
        lds[threadIdx.x] = mine;
        __syncthreads();
        for (uint32_t d = 1; d < LP_LM_SCAN_THREADS; d <<= 1)   // Hillis-Steele, inclusive
        {
            const uint32_t add_ = threadIdx.x >= d ? lds[threadIdx.x - d] : 0u;
            __syncthreads();
            lds[threadIdx.x] += add_;
            __syncthreads();
        }
        const uint32_t base = carry;
        if (i < n) totals[i] = base + lds[threadIdx.x] - mine;
        __syncthreads();
        if (threadIdx.x == LP_LM_SCAN_THREADS - 1u) carry = base + lds[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0u) totals[n] = carry;
}

// local -> world of a point: the inverse of the instance's stored world -> local affine, operation for operation what
// lights_sample does (mat4x3f_inverse, pathtracer.wgsl:2790-2802)
LP_DEV f3 lm_local_to_world(const InstanceDev &in, f3 lp)
{
    f3 a0 = mk3(in.r0.x, in.r1.x, in.r2.x), a1 = mk3(in.r0.y, in.r1.y, in.r2.y);
    f3 a2 = mk3(in.r0.z, in.r1.z, in.r2.z), a3 = mk3(in.r0.w, in.r1.w, in.r2.w);
    f3 cyz = cross3(a1, a2), czx = cross3(a2, a0), cxy = cross3(a0, a1);
    float idet = 1.0f / dot3(a0, cyz);
    f3 m0 = scale(mk3(cyz.x, czx.x, cxy.x), idet);
    f3 m1 = scale(mk3(cyz.y, czx.y, cxy.y), idet);
    f3 m2 = scale(mk3(cyz.z, czx.z, cxy.z), idet);
    f3 m3 = neg(mat3_mul(m0, m1, m2, a3));
    return add(add(add(scale(m0, lp.x), scale(m1, lp.y)), scale(m2, lp.z)), scale(m3, 1.0f));
}

// The bake normal at barycentrics (u, v) of global triangle gtri (vertex ids i0, i1, i2) of an instance: the geometric normal
// `ng`, or with LP_LM_SMOOTH_NORMALS on a mesh that has normals the interpolated vertex normal in world space, turned to
// ng's side.  k_lm_emit writes it into the record; the directional lightmapped view (lupin_lightmapped_view.hpp) computes it
// again at a pixel's hit: both go through here.
template <typename Geo>
LP_DEV f3 lm_bake_normal(const Geo &geo, const SceneDev &sc, const InstanceDev &in, const MeshDev &mesh, uint32_t gtri, uint32_t i0, uint32_t i1,
                         uint32_t i2, float u, float v, uint32_t flags, f3 &ng)
{
    ng = geometric_normal(geo, in, gtri);
    f3 n = ng;
    if ((flags & LP_LM_SMOOTH_NORMALS) && mesh.normals_base != LUPIN_SENTINEL_IDX)
    {
        const float w = 1.0f - u - v;
        const f3 n0 = xyz(sc.normals[mesh.normals_base + i0]);
        const f3 n1 = xyz(sc.normals[mesh.normals_base + i1]);
        const f3 n2 = xyz(sc.normals[mesh.normals_base + i2]);
        n = normal_to_world(in, normalize3(add(add(scale(n0, w), scale(n1, u)), scale(n2, v))));
        if (dot3(n, ng) < 0.0f) n = neg(n);
    }
    return n;
}

__global__ void __launch_bounds__(LP_BLOCK) k_lm_emit(SceneDev sc, const LmChartDev *__restrict__ charts, uint32_t num_charts, uint32_t W, uint32_t H,
                                                      const uint32_t *__restrict__ owner, const uint32_t *__restrict__ block_offsets, uint32_t flags,
                                                      uint32_t counter, float surface_offset, float4 *__restrict__ records,
                                                      uint32_t *__restrict__ texel_of)
{
    __shared__ uint32_t lds_wave[LP_BLOCK / 64u];
    const uint32_t texels = W * H;
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    const uint32_t key = i < texels ? owner[i] : LP_LM_NO_OWNER;
    const bool owned = key != LP_LM_NO_OWNER;
    uint32_t before, total;
    lm_block_rank(owned, lds_wave, before, total);
    if (!owned) return;
    const uint32_t slot = block_offsets[blockIdx.x] + before;

    const LmChartDev ch = charts[lm_chart_of(charts, num_charts, key)];
    const LmTri t = lm_triangle(sc, ch, key - ch.key_base, (float)W, (float)H);
    const uint32_t y = i / W, x = i - y * W;
    float e1, e2, area2;
    lm_covers(t, (float)x + 0.5f, (float)y + 0.5f, e1, e2, area2);
    const float u = e1 / area2, v = e2 / area2;
    const float w = 1.0f - u - v;

    const auto geo = geo_global(sc);
    const InstanceDev in = sc.instances[ch.inst];
    const TriVerts tv = geo.tri_fetch(t.gtri);
    const f3 lp = add(add(scale(xyz(tv.v0), w), scale(xyz(tv.v1), u)), scale(xyz(tv.v2), v));
    const f3 wp = lm_local_to_world(in, lp);
    f3 ng;
    const f3 n = lm_bake_normal(geo, sc, in, t.mesh, t.gtri, t.i0, t.i1, t.i2, u, v, flags, ng);
    const f3 o = add(wp, scale(ng, surface_offset));
    records[2 * (size_t)slot] = make_float4(o.x, o.y, o.z, __uint_as_float(rng_seed_for(i, counter)));
    records[2 * (size_t)slot + 1] = make_float4(n.x, n.y, n.z, __uint_as_float(LP_RAY_COSINE_HEMISPHERE));
    texel_of[slot] = i;
}

// one thread per covered texel: rgba (cleared before) gets pi * mean and alpha 1, `filled` 1; the record plane its record
__global__ void __launch_bounds__(LP_BLOCK) k_lm_scatter(uint32_t n, const uint32_t *__restrict__ texel_of, const float4 *__restrict__ mean,
                                                         const float4 *__restrict__ records, float4 *__restrict__ rgba, uint8_t *__restrict__ filled,
                                                         float4 *__restrict__ record_plane)
{
    const uint32_t j = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t texel = texel_of[j];
    const float4 m = mean[j];
    rgba[texel] = make_float4(LP_PI * m.x, LP_PI * m.y, LP_PI * m.z, 1.0f);
    filled[texel] = 1u;
    if (record_plane)
    {
        record_plane[2 * (size_t)texel] = records[2 * (size_t)j];
        record_plane[2 * (size_t)texel + 1] = records[2 * (size_t)j + 1];
    }
}

// One gutter pass: a texel not filled yet takes the f32 mean of its filled 8-neighbours (summed dy -1..1 outer, dx -1..1
// inner, from zero, then divided by their count) and counts as filled in the next pass; its alpha stays 0.
__global__ void __launch_bounds__(LP_BLOCK) k_lm_dilate(uint32_t W, uint32_t H, const float4 *__restrict__ src, const uint8_t *__restrict__ src_filled,
                                                        float4 *__restrict__ dst, uint8_t *__restrict__ dst_filled)
{
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i >= W * H) return;
    float4 c = src[i];
    uint8_t f = src_filled[i];
    if (!f)
    {
        const int32_t y = (int32_t)(i / W), x = (int32_t)(i - (uint32_t)y * W);
        f3 sum = splat(0.0f);
        uint32_t count = 0u;
        for (int32_t dy = -1; dy <= 1; dy++)
            for (int32_t dx = -1; dx <= 1; dx++)
            {
                const int32_t nx = x + dx, ny = y + dy;
                if ((dx == 0 && dy == 0) || nx < 0 || ny < 0 || nx >= (int32_t)W || ny >= (int32_t)H) continue;
                const size_t j = (size_t)ny * W + (uint32_t)nx;
                if (!src_filled[j]) continue;
                const float4 s = src[j];
                sum = add(sum, mk3(s.x, s.y, s.z));
                count++;
            }
        if (count)
        {
            const float cf = (float)count;
            c = make_float4(sum.x / cf, sum.y / cf, sum.z / cf, 0.0f);
            f = 1u;
        }
    }
    dst[i] = c;
    dst_filled[i] = f;
}

// lupin_hip_bake_lightmap_ao, one thread per covered texel (planes cleared before), from the sums of
// k_bent_normal (lupin_bent_normal.hpp).  With a = sums[j]: v = a.w / samples_f; ao texel = (v, v, v, 1);
// len = sqrtf((a.x*a.x + a.y*a.y) + a.z*a.z);  bent texel = (a.x / len, a.y / len, a.z / len, 1), or the record's bake
// normal where len == 0;  `filled` 1;  the record plane its record.  bent and record_plane may be null.
__global__ void __launch_bounds__(LP_BLOCK) k_lm_ao_scatter(uint32_t n, const uint32_t *__restrict__ texel_of, const float4 *__restrict__ sums,
                                                            const float4 *__restrict__ records, float samples_f, float4 *__restrict__ ao,
                                                            float4 *__restrict__ bent, uint8_t *__restrict__ filled, float4 *__restrict__ record_plane)
{
    const uint32_t j = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t texel = texel_of[j];
    const float4 a = sums[j];
    const float4 r0 = records[2 * (size_t)j], r1 = records[2 * (size_t)j + 1];
    const float v = a.w / samples_f;
    ao[texel] = make_float4(v, v, v, 1.0f);
    if (bent)
    {
        const float len = sqrtf((a.x * a.x + a.y * a.y) + a.z * a.z);
        bent[texel] = len == 0.0f ? make_float4(r1.x, r1.y, r1.z, 1.0f) : make_float4(a.x / len, a.y / len, a.z / len, 1.0f);
    }
    filled[texel] = 1u;
    if (record_plane)
    {
        record_plane[2 * (size_t)texel] = r0;
        record_plane[2 * (size_t)texel + 1] = r1;
    }
}
