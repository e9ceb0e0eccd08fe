// lupin_lightmap_stitch.hpp -- lightmap seam stitching, included once by lupin_hip.hip after
// lupin_lightmapped_view.hpp.
//
// lupin_hip_stitch_lightmap pulls the two sides of every chart border of a baked atlas together: the seam edges of the
// charts' meshes are found, sampled, every sample becomes a row of eight (texel, weight) entries -- the view's
// ownership-aware bilinear fetch on side A minus the same fetch on side B -- and (A^T A + lambda I) d = -A^T (A x0) is solved
// by plain conjugate gradients over the texels the rows touch.  The rule is in include/lupin_hip.h; tests/lightmap_stitch_ref.py
// restates it.  In order of use:
//
//   k_st_keys      one thread per half-edge h = 3 * triangle + k: the key (min vertex index << 32 | max) and the value h
//   (hipCUB's stable radix sort by key, then, with more than one chart, by chart: runs of equal (chart, min, max); the sorts
//    and the scan are in lupin_stitch_sort.hip)
//   k_st_chart_keys  between the two sorts: the chart of every sorted half-edge
//   k_st_runs      one thread per sorted place: at the start of a run of exactly two, the seam test; partner[hA] = hB.
//                  Runs of three or more are counted (one integer atomicAdd each).
//   (k_lm_count, k_lm_scan of lupin_lightmap.hpp on the partner plane: seam edges in ascending hA)
//   k_st_edges     order-preserving compaction: the edge's four end points in texel space and its sample count n_e
//   (hipCUB's exclusive sum of the counts)
//   k_st_pairs     one thread per sample pair: the two footprints (st_footprint: the view's fetch arithmetic, lmv_axis of
//                  lupin_lightmapped_view.hpp), the row's eight entries, and the incidence keys (texel, 8 * pair + entry)
//   (hipCUB's stable radix sort of the incidence keys by texel)
//   k_st_heads     the first place of every texel's run in the sorted incidence list, and the number of live entries
//   (k_lm_count, k_lm_scan on the head plane)
//   k_st_active    order-preserving compaction: per active texel its texel index and the start of its incidence list
//   k_st_columns   one thread per active texel: col[8 * pair + entry] = the texel's active number; x0 from the atlas
//   k_st_apply     s = A v, one thread per pair, eight entries in entry order; with ENERGY the block partials of s * s
//   k_st_adjoint   one thread per active texel over its incidence list in ascending (pair, entry) order:
//                  INIT: r = -(A^T s), p = r, d = 0, partials of r * r;   otherwise q = A^T s + lambda * p, partials of p * q
//   k_st_scalars   one wave: the partials summed in ascending block order, then alpha, beta or an energy, on the device
//   k_st_update    d = d + alpha * p, r = r - alpha * q, partials of r * r
//   k_st_direction p = r + beta * p
//   k_st_result    x = x0 + d per active texel, and (k_st_scatter) its rgb into the output atlas
//
// Sums.  A block of LP_BLOCK elements (zeros past the last) is summed by the xor butterfly 32, 16, .., 1 in each wave64 and
// the four wave sums are added in ascending wave order; one wave then adds the block sums lane-strided (lane l: blocks l,
// l + 64, .. ascending, from 0.0f) and runs the same butterfly.  The order depends on the element count alone.  No float
// atomics.  Every float operation is f32 without contraction (-ffp-contract=off), IEEE division and sqrt.
#pragma once

#include "lupin_lightmapped_view.hpp"

constexpr uint32_t LP_ST_MAX_EDGE_SAMPLES = 65536u;   // LUPIN_LIGHTMAP_STITCH_MAX_EDGE_SAMPLES
// the integer counters of a call, on the device
constexpr uint32_t LP_ST_NON_MANIFOLD = 0u, LP_ST_DROPPED = 1u, LP_ST_LIVE_ENTRIES = 2u, LP_ST_COUNTERS = 4u;

struct StScalars   // the solver's scalars, per channel in x, y, z
{
    float4 rr, alpha, beta, before, after;
    uint32_t stopped[4];
};
constexpr uint32_t LP_ST_INIT = 0u, LP_ST_ALPHA = 1u, LP_ST_BETA = 2u, LP_ST_AFTER = 3u;   // k_st_scalars' modes

// the chart and the two vertex indices of half-edge h (corner k to corner (k + 1) % 3 of triangle h / 3)
LP_DEV void st_half_edge(const SceneDev &sc, const LmChartDev *__restrict__ charts, uint32_t num_charts, uint32_t h, uint32_t &chart, uint32_t &va,
                         uint32_t &vb)
{
    const uint32_t key = h / 3u, k = h - 3u * key;
    chart = lm_chart_of(charts, num_charts, key);
    const LmChartDev ch = charts[chart];
    const size_t gtri = (size_t)sc.inst_meshes[ch.inst].tri_offset + (key - ch.key_base);
    va = sc.tri_indices[gtri * 3 + k];
    vb = sc.tri_indices[gtri * 3 + (k + 1u) % 3u];
}

__global__ void __launch_bounds__(LP_BLOCK) k_st_keys(SceneDev sc, const LmChartDev *__restrict__ charts, uint32_t num_charts, uint32_t n,
                                                      unsigned long long *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t h = blockIdx.x * LP_BLOCK + threadIdx.x;   // n <= 2^32 - 2: the last block's last lane is 2^32 - 1 at most
    if (h >= n) return;
    uint32_t c, va, vb;
    st_half_edge(sc, charts, num_charts, h, c, va, vb);
    keys[h] = ((unsigned long long)min(va, vb) << 32) | (unsigned long long)max(va, vb);
    vals[h] = h;
}

__global__ void __launch_bounds__(LP_BLOCK) k_st_chart_keys(const LmChartDev *__restrict__ charts, uint32_t num_charts, uint32_t n,
                                                            const uint32_t *__restrict__ vals, uint32_t *__restrict__ chart_keys)
{
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i >= n) return;
    chart_keys[i] = lm_chart_of(charts, num_charts, vals[i] / 3u);
}

// corner k of triangle `tri` of a chart in texel space, formed as lm_triangle forms it; v: the corner's vertex index
LP_DEV float2 st_corner(const SceneDev &sc, const LmChartDev &ch, const MeshDev &mesh, uint32_t tri, uint32_t k, uint32_t v, float Wf, float Hf)
{
    const float2 a = ch.lm_uvs ? ch.lm_uvs[(size_t)tri * 3 + k] : sc.texcoords[mesh.texcoords_base + v];
    return make_float2((a.x * ch.scale_u + ch.offset_u) * Wf, (a.y * ch.scale_v + ch.offset_v) * Hf);
}

// The two sides of the edge that half-edges hA and hB share, in texel space, the vertex hA starts at first on both sides:
// a0, a1 and b0, b1.
LP_DEV void st_sides(const SceneDev &sc, const LmChartDev *__restrict__ charts, uint32_t num_charts, uint32_t hA, uint32_t hB, float Wf, float Hf,
                     float2 &a0, float2 &a1, float2 &b0, float2 &b1)
{
    const uint32_t keyA = hA / 3u, kA = hA - 3u * keyA, keyB = hB / 3u, kB = hB - 3u * keyB;
    const LmChartDev ch = charts[lm_chart_of(charts, num_charts, keyA)];   // (hB is of the same chart)
    const MeshDev mesh = sc.inst_meshes[ch.inst];
    const uint32_t tA = keyA - ch.key_base, tB = keyB - ch.key_base, kA1 = (kA + 1u) % 3u, kB1 = (kB + 1u) % 3u;
    const size_t iA = ((size_t)mesh.tri_offset + tA) * 3, iB = ((size_t)mesh.tri_offset + tB) * 3;
    const uint32_t vA0 = sc.tri_indices[iA + kA], vA1 = sc.tri_indices[iA + kA1], vB0 = sc.tri_indices[iB + kB], vB1 = sc.tri_indices[iB + kB1];
    a0 = st_corner(sc, ch, mesh, tA, kA, vA0, Wf, Hf);
    a1 = st_corner(sc, ch, mesh, tA, kA1, vA1, Wf, Hf);
    const float2 p = st_corner(sc, ch, mesh, tB, kB, vB0, Wf, Hf), q = st_corner(sc, ch, mesh, tB, kB1, vB1, Wf, Hf);
    const bool same = vB0 == vA0;
    b0 = same ? p : q;
    b1 = same ? q : p;
}

// vals: the half-edges sorted by (chart, min, max), equal keys in ascending half-edge.  partner: n words, 0xFF-filled before.
__global__ void __launch_bounds__(LP_BLOCK) k_st_runs(SceneDev sc, const LmChartDev *__restrict__ charts, uint32_t num_charts, uint32_t n,
                                                      const uint32_t *__restrict__ vals, float Wf, float Hf, uint32_t *__restrict__ partner,
                                                      uint32_t *__restrict__ counters)
{
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t hA = vals[i];
    uint32_t c, va, vb, c2, va2, vb2;
    st_half_edge(sc, charts, num_charts, hA, c, va, vb);
    if (va == vb) return;   // a half-edge with equal indices (its key meets only its like)
    const uint32_t lo = min(va, vb), hi = max(va, vb);
    auto same = [&](uint32_t j) {
        st_half_edge(sc, charts, num_charts, vals[j], c2, va2, vb2);
        return c2 == c && min(va2, vb2) == lo && max(va2, vb2) == hi;
    };
    if (i > 0u && same(i - 1u)) return;                 // not the start of a run
    if (!(i + 1u < n && same(i + 1u))) return;          // one holder: a boundary
    if (i + 2u < n && same(i + 2u)) { atomicAdd(&counters[LP_ST_NON_MANIFOLD], 1u); return; }
    const uint32_t hB = vals[i + 1u];                   // hA < hB: the sorts are stable
    float2 a0, a1, b0, b1;
    st_sides(sc, charts, num_charts, hA, hB, Wf, Hf, a0, a1, b0, b1);
    const bool seam = __float_as_uint(a0.x) != __float_as_uint(b0.x) || __float_as_uint(a0.y) != __float_as_uint(b0.y) ||
                      __float_as_uint(a1.x) != __float_as_uint(b1.x) || __float_as_uint(a1.y) != __float_as_uint(b1.y);
    if (seam) partner[hA] = hB;
}

LP_DEV float st_length(float2 p, float2 q)
{
    const float dx = q.x - p.x, dy = q.y - p.y;
    return sqrtf(dx * dx + dy * dy);
}

// order-preserving compaction of the partner plane (block_offsets: k_lm_count's totals after k_lm_scan): edge e, the e-th
// seam in ascending hA, gets (a0, a1) (b0, b1) and counts[e] = n_e
__global__ void __launch_bounds__(LP_BLOCK) k_st_edges(SceneDev sc, const LmChartDev *__restrict__ charts, uint32_t num_charts, uint32_t n,
                                                       const uint32_t *__restrict__ partner, const uint32_t *__restrict__ block_offsets, float Wf, float Hf,
                                                       float samples_per_texel, float4 *__restrict__ edges, unsigned long long *__restrict__ counts)
{
    __shared__ uint32_t lds_wave[LP_BLOCK / 64u];
    const uint32_t h = blockIdx.x * LP_BLOCK + threadIdx.x;
    const uint32_t hB = h < n ? partner[h] : LP_LM_NO_OWNER;
    const bool seam = hB != LP_LM_NO_OWNER;
    uint32_t before, total;
    lm_block_rank(seam, lds_wave, before, total);
    if (!seam) return;
    const uint32_t e = block_offsets[blockIdx.x] + before;
    float2 a0, a1, b0, b1;
    st_sides(sc, charts, num_charts, h, hB, Wf, Hf, a0, a1, b0, b1);
    const float m = ceilf(fmaxf(st_length(a0, a1), st_length(b0, b1)) * samples_per_texel);
    uint32_t ne = 1u;                                    // (also what a length that is not a number gives)
    if (m >= (float)LP_ST_MAX_EDGE_SAMPLES) ne = LP_ST_MAX_EDGE_SAMPLES;
    else if (m >= 1.0f) ne = (uint32_t)m;
    edges[2 * (size_t)e] = make_float4(a0.x, a0.y, a1.x, a1.y);
    edges[2 * (size_t)e + 1] = make_float4(b0.x, b0.y, b1.x, b1.y);
    counts[e] = ne;
}

// The footprint of the point (px, py) of texel space: the four taps of the view's fetch at (px - 0.5, py - 0.5) in tap order
// 00, 10, 01, 11, `cov` over the taps whose input alpha != 0, an owned tap weighted w / cov and every other 0.
// false: a coordinate that is not finite, or cov == 0.
LP_DEV bool st_footprint(const float4 *__restrict__ rgba, uint32_t W, uint32_t H, float px, float py, uint32_t tex[4], float wgt[4])
{
    const float cx = px - 0.5f, cy = py - 0.5f;
    if (!(isfinite(cx) && isfinite(cy))) return false;
    uint32_t x0, x1, y0, y1;
    float fx, fy;
    lmv_axis(cx, W, x0, x1, fx);
    lmv_axis(cy, H, y0, y1, fy);
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const float wt[4] = {gx * gy, fx * gy, gx * fy, fx * fy};
    tex[0] = y0 * W + x0; tex[1] = y0 * W + x1; tex[2] = y1 * W + x0; tex[3] = y1 * W + x1;   // < W * H <= 2^28
    bool owned[4];
    float cov = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; k++)
    {
        owned[k] = rgba[tex[k]].w != 0.0f;
        if (owned[k]) cov = cov + wt[k];
    }
    if (!(cov > 0.0f)) return false;
#pragma unroll
    for (int k = 0; k < 4; k++) wgt[k] = owned[k] ? wt[k] / cov : 0.0f;
    return true;
}

// offsets: the exclusive sums of the edges' counts, num_edges + 1 of them.  Pair p = offsets[e] + j is sample j of edge e.
// row_wgt: 8 weights a pair; inc_keys / inc_vals: what the incidence sort takes (the texel, or `texels` for an entry without
// weight; 8 * p + entry).
__global__ void __launch_bounds__(LP_BLOCK) k_st_pairs(const float4 *__restrict__ rgba, uint32_t W, uint32_t H, const float4 *__restrict__ edges,
                                                       const unsigned long long *__restrict__ offsets, uint32_t num_edges, uint32_t num_pairs,
                                                       float *__restrict__ row_wgt, uint32_t *__restrict__ inc_keys, uint32_t *__restrict__ inc_vals,
                                                       uint32_t *__restrict__ counters)
{
    const uint32_t p = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (p >= num_pairs) return;
    uint32_t lo = 0u, hi = num_edges - 1u;   // the last edge whose offset is <= p (every edge has a sample)
    while (lo < hi)
    {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (offsets[mid] <= (unsigned long long)p) lo = mid; else hi = mid - 1u;
    }
    const uint32_t j = p - (uint32_t)offsets[lo], ne = (uint32_t)(offsets[lo + 1u] - offsets[lo]);
    const float4 ea = edges[2 * (size_t)lo], eb = edges[2 * (size_t)lo + 1];
    const float t = ((float)j + 0.5f) / (float)ne;
    const float ax = ea.x + (ea.z - ea.x) * t, ay = ea.y + (ea.w - ea.y) * t;
    const float bx = eb.x + (eb.z - eb.x) * t, by = eb.y + (eb.w - eb.y) * t;
    uint32_t tex[8];
    float wgt[8];
    const bool keptA = st_footprint(rgba, W, H, ax, ay, tex, wgt);
    const bool keptB = st_footprint(rgba, W, H, bx, by, tex + 4, wgt + 4);
    const bool kept = keptA && keptB;
    if (!kept) atomicAdd(&counters[LP_ST_DROPPED], 1u);
    const uint32_t texels = W * H;
#pragma unroll
    for (uint32_t k = 0; k < 8u; k++)
    {
        const float w = kept ? (k < 4u ? wgt[k] : -wgt[k]) : 0.0f;
        const uint32_t tx = kept ? tex[k] : 0u;
        const size_t at = 8 * (size_t)p + k;
        row_wgt[at] = w;
        inc_keys[at] = w != 0.0f ? tx : texels;
        inc_vals[at] = (uint32_t)at;
    }
}

// keys: the sorted incidence keys, n of them.  heads[i] = i at the first place of a texel's run, LP_LM_NO_OWNER elsewhere;
// counters[LP_ST_LIVE_ENTRIES] (zero before) = the number of entries that carry a weight (one writer).
__global__ void __launch_bounds__(LP_BLOCK) k_st_heads(const uint32_t *__restrict__ keys, uint32_t n, uint32_t texels, uint32_t *__restrict__ heads,
                                                       uint32_t *__restrict__ counters)
{
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t key = keys[i];
    const bool live = key < texels;
    heads[i] = (live && (i == 0u || keys[i - 1u] != key)) ? i : LP_LM_NO_OWNER;
    if (live && (i + 1u == n || keys[i + 1u] >= texels)) counters[LP_ST_LIVE_ENTRIES] = i + 1u;
}

__global__ void __launch_bounds__(LP_BLOCK) k_st_active(const uint32_t *__restrict__ keys, uint32_t n, const uint32_t *__restrict__ heads,
                                                        const uint32_t *__restrict__ block_offsets, uint32_t *__restrict__ act_texel,
                                                        uint32_t *__restrict__ act_start)
{
    __shared__ uint32_t lds_wave[LP_BLOCK / 64u];
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    const bool head = i < n && heads[i] != LP_LM_NO_OWNER;
    uint32_t before, total;
    lm_block_rank(head, lds_wave, before, total);
    if (!head) return;
    const uint32_t a = block_offsets[blockIdx.x] + before;
    act_texel[a] = keys[i];
    act_start[a] = i;
}

// the places [first, last) of active texel a in the sorted incidence list
LP_DEV void st_list(const uint32_t *__restrict__ act_start, uint32_t num_active, const uint32_t *__restrict__ counters, uint32_t a, uint32_t &first,
                    uint32_t &last)
{
    first = act_start[a];
    last = a + 1u < num_active ? act_start[a + 1u] : counters[LP_ST_LIVE_ENTRIES];
}

// col (8 entries a pair, zero before): the active number of every entry that carries a weight.  x0: the atlas at the texel.
__global__ void __launch_bounds__(LP_BLOCK) k_st_columns(const float4 *__restrict__ rgba, const uint32_t *__restrict__ act_texel,
                                                         const uint32_t *__restrict__ act_start, uint32_t num_active, const uint32_t *__restrict__ counters,
                                                         const uint32_t *__restrict__ inc_vals, uint32_t *__restrict__ col, float4 *__restrict__ x0)
{
    const uint32_t a = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (a >= num_active) return;
    uint32_t first, last;
    st_list(act_start, num_active, counters, a, first, last);
    for (uint32_t i = first; i < last; i++) col[inc_vals[i]] = a;
    const float4 t = rgba[act_texel[a]];
    x0[a] = make_float4(t.x, t.y, t.z, 0.0f);
}

LP_DEV float st_butterfly(float a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a = a + __shfl_xor(a, off);
    return a;
}

// The block's sum of v per channel, in the order of the header comment; every thread of the block calls it, thread 0 writes
// the sum to partials[blockIdx.x].
LP_DEV void st_block_sum(float4 v, float4 *lds_wave, float4 *__restrict__ partials)
{
    v.x = st_butterfly(v.x); v.y = st_butterfly(v.y); v.z = st_butterfly(v.z);
    if ((threadIdx.x & 63u) == 0u) lds_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0u)
    {
        float4 s = lds_wave[0];
        for (uint32_t w = 1; w < LP_BLOCK / 64u; w++) { s.x = s.x + lds_wave[w].x; s.y = s.y + lds_wave[w].y; s.z = s.z + lds_wave[w].z; }
        partials[blockIdx.x] = make_float4(s.x, s.y, s.z, 0.0f);
    }
}

// s = A v: per pair the eight entries in entry order from zero, an entry without weight adding 0.0f.  ENERGY: the block
// partials of s * s.
template <bool ENERGY>
__global__ void __launch_bounds__(LP_BLOCK) k_st_apply(uint32_t num_pairs, const float *__restrict__ row_wgt, const uint32_t *__restrict__ col,
                                                       const float4 *__restrict__ v, float4 *__restrict__ s, float4 *__restrict__ partials)
{
    __shared__ float4 lds_wave[LP_BLOCK / 64u];
    const uint32_t p = blockIdx.x * LP_BLOCK + threadIdx.x;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p < num_pairs)
    {
        const float4 w0 = reinterpret_cast<const float4 *>(row_wgt)[2 * (size_t)p], w1 = reinterpret_cast<const float4 *>(row_wgt)[2 * (size_t)p + 1];
        const uint4 c0 = reinterpret_cast<const uint4 *>(col)[2 * (size_t)p], c1 = reinterpret_cast<const uint4 *>(col)[2 * (size_t)p + 1];
        const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
        const uint32_t c[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
#pragma unroll
        for (int k = 0; k < 8; k++)
        {
            float4 x = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (w[k] != 0.0f) { const float4 t = v[c[k]]; x = make_float4(w[k] * t.x, w[k] * t.y, w[k] * t.z, 0.0f); }
            acc.x = acc.x + x.x; acc.y = acc.y + x.y; acc.z = acc.z + x.z;
        }
        s[p] = acc;
    }
    if constexpr (ENERGY) st_block_sum(make_float4(acc.x * acc.x, acc.y * acc.y, acc.z * acc.z, 0.0f), lds_wave, partials);
}

// t = A^T s at an active texel: its incidence list in ascending (pair, entry) order, from zero.
// INIT: r = -t, p = r, d = 0, the block partials of r * r.  Otherwise: q = t + lambda * p, the block partials of p * q.
template <bool INIT>
__global__ void __launch_bounds__(LP_BLOCK) k_st_adjoint(uint32_t num_active, const uint32_t *__restrict__ act_start, const uint32_t *__restrict__ counters,
                                                         const uint32_t *__restrict__ inc_vals, const float *__restrict__ row_wgt,
                                                         const float4 *__restrict__ s, float lambda, float4 *__restrict__ r, float4 *__restrict__ p,
                                                         float4 *__restrict__ d, float4 *__restrict__ q, float4 *__restrict__ partials)
{
    __shared__ float4 lds_wave[LP_BLOCK / 64u];
    const uint32_t a = blockIdx.x * LP_BLOCK + threadIdx.x;
    float4 dot = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a < num_active)
    {
        uint32_t first, last;
        st_list(act_start, num_active, counters, a, first, last);
        float4 t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (uint32_t i = first; i < last; i++)
        {
            const uint32_t at = inc_vals[i];
            const float w = row_wgt[at];
            const float4 sp = s[at >> 3];
            t.x = t.x + w * sp.x; t.y = t.y + w * sp.y; t.z = t.z + w * sp.z;
        }
        if constexpr (INIT)
        {
            const float4 rv = make_float4(-t.x, -t.y, -t.z, 0.0f);
            r[a] = rv; p[a] = rv;
            d[a] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            dot = make_float4(rv.x * rv.x, rv.y * rv.y, rv.z * rv.z, 0.0f);
        }
        else
        {
            const float4 pv = p[a];
            const float4 qv = make_float4(t.x + lambda * pv.x, t.y + lambda * pv.y, t.z + lambda * pv.z, 0.0f);
            q[a] = qv;
            dot = make_float4(pv.x * qv.x, pv.y * qv.y, pv.z * qv.z, 0.0f);
        }
    }
    st_block_sum(dot, lds_wave, partials);
}

// one wave: the sum of n block sums, lane-strided from 0.0f, then the butterfly (every lane holds it)
LP_DEV float4 st_total(const float4 *__restrict__ partials, uint32_t n)
{
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t b = threadIdx.x; b < n; b += 64u) { const float4 v = partials[b]; acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z; }
    return make_float4(st_butterfly(acc.x), st_butterfly(acc.y), st_butterfly(acc.z), 0.0f);
}

// LP_ST_INIT:  before = total(pair partials), rr = total(active partials), nothing stopped
// LP_ST_ALPHA: pq = total(active partials); a channel whose pq is zero or not finite stops: alpha = 0 from then on;
//              otherwise alpha = rr / pq
// LP_ST_BETA:  rr' = total(active partials); beta = rr' / rr (0 for a stopped channel); rr = rr'
// LP_ST_AFTER: after = total(pair partials)
__global__ void __launch_bounds__(64) k_st_scalars(uint32_t mode, const float4 *__restrict__ pair_partials, uint32_t pair_blocks,
                                                   const float4 *__restrict__ active_partials, uint32_t active_blocks, StScalars *__restrict__ sc)
{
    if (mode == LP_ST_INIT || mode == LP_ST_AFTER)
    {
        const float4 e = st_total(pair_partials, pair_blocks);
        if (threadIdx.x == 0u) { if (mode == LP_ST_INIT) sc->before = e; else sc->after = e; }
        if (mode == LP_ST_AFTER) return;
    }
    const float4 tot = st_total(active_partials, active_blocks);
    if (threadIdx.x != 0u) return;
    const float t[3] = {tot.x, tot.y, tot.z};
    float rr[3] = {sc->rr.x, sc->rr.y, sc->rr.z}, out[3];
    for (int c = 0; c < 3; c++)
    {
        if (mode == LP_ST_INIT) { rr[c] = t[c]; sc->stopped[c] = 0u; out[c] = 0.0f; }
        else if (mode == LP_ST_ALPHA)
        {
            if (!(t[c] != 0.0f && isfinite(t[c]))) sc->stopped[c] = 1u;
            out[c] = sc->stopped[c] ? 0.0f : rr[c] / t[c];
        }
        else
        {
            out[c] = sc->stopped[c] ? 0.0f : t[c] / rr[c];
            rr[c] = t[c];
        }
    }
    sc->rr = make_float4(rr[0], rr[1], rr[2], 0.0f);
    if (mode == LP_ST_ALPHA) sc->alpha = make_float4(out[0], out[1], out[2], 0.0f);
    if (mode == LP_ST_BETA) sc->beta = make_float4(out[0], out[1], out[2], 0.0f);
}

__global__ void __launch_bounds__(LP_BLOCK) k_st_update(uint32_t num_active, const StScalars *__restrict__ sc, const float4 *__restrict__ p,
                                                        const float4 *__restrict__ q, float4 *__restrict__ d, float4 *__restrict__ r,
                                                        float4 *__restrict__ partials)
{
    __shared__ float4 lds_wave[LP_BLOCK / 64u];
    const uint32_t a = blockIdx.x * LP_BLOCK + threadIdx.x;
    float4 dot = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a < num_active)
    {
        const float4 al = sc->alpha, pv = p[a], qv = q[a], dv = d[a], rv = r[a];
        d[a] = make_float4(dv.x + al.x * pv.x, dv.y + al.y * pv.y, dv.z + al.z * pv.z, 0.0f);
        const float4 rn = make_float4(rv.x - al.x * qv.x, rv.y - al.y * qv.y, rv.z - al.z * qv.z, 0.0f);
        r[a] = rn;
        dot = make_float4(rn.x * rn.x, rn.y * rn.y, rn.z * rn.z, 0.0f);
    }
    st_block_sum(dot, lds_wave, partials);
}

__global__ void __launch_bounds__(LP_BLOCK) k_st_direction(uint32_t num_active, const StScalars *__restrict__ sc, const float4 *__restrict__ r,
                                                           float4 *__restrict__ p)
{
    const uint32_t a = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (a >= num_active) return;
    const float4 be = sc->beta, rv = r[a], pv = p[a];
    p[a] = make_float4(rv.x + be.x * pv.x, rv.y + be.y * pv.y, rv.z + be.z * pv.z, 0.0f);
}

// x = x0 + d
__global__ void __launch_bounds__(LP_BLOCK) k_st_result(uint32_t num_active, const float4 *__restrict__ x0, const float4 *__restrict__ d,
                                                        float4 *__restrict__ x)
{
    const uint32_t a = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (a >= num_active) return;
    const float4 v = x0[a], dv = d[a];
    x[a] = make_float4(v.x + dv.x, v.y + dv.y, v.z + dv.z, 0.0f);
}

// rgb of x into the output atlas at the active texels (12 bytes each: the alpha beside them is not written)
__global__ void __launch_bounds__(LP_BLOCK) k_st_scatter(uint32_t num_active, const uint32_t *__restrict__ act_texel, const float4 *__restrict__ x,
                                                         float *__restrict__ out)
{
    const uint32_t a = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (a >= num_active) return;
    const float4 v = x[a];
    float *__restrict__ o = out + 4 * (size_t)act_texel[a];
    o[0] = v.x; o[1] = v.y; o[2] = v.z;
}
