// lupin_unwrap.hpp -- lightmap UV generation, included once by lupin_hip.hip after lupin_lightmap.hpp.
//
// lupin_hip_unwrap_lightmap_uvs gives one mesh a non-overlapping UV set of its own: triangles are sorted into six buckets by
// the dominant axis of their normal, the connected components of a bucket (over shared vertex indices) are the charts, a
// chart is projected on its bucket's plane, and the charts' bounding rectangles are shelf-packed (on the host, between two
// device phases: include/lupin_pack.hpp).  The rule is in include/lupin_hip.h; tests/lightmap_unwrap_ref.py restates it.
// One thread per triangle everywhere:
//
//   k_uw_classify   the bucket of a triangle (LP_UW_NONE: degenerate), parent[t] = t, and atomicMin of t on the
//                   (bucket, vertex) table of 6 * V words: the smallest triangle that touches a vertex in a bucket
//   k_uw_union      a triangle unites itself with the table's entry of each of its three vertices: lock-free union-find, the
//                   larger root is always hooked under the smaller (one atomicCAS on a root), paths halved with atomicMin
//   k_uw_flatten    label[t] = the root of t (the smallest triangle of its component, whatever the scheduling was), the
//                   root plane (t where label[t] == t, LP_LM_NO_OWNER elsewhere), and the chart's box: atomicMin / atomicMax
//                   on order-preserving integer images of the plane coordinates, at the label's place
//   (k_lm_count, k_lm_scan of lupin_lightmap.hpp on the root plane: the charts' dense numbers are ranks of labels)
//   k_uw_compact    per chart, in ascending label: its label and its box as floats; per root its dense number
//   (the host computes the rectangles, packs them and uploads each chart's origin)
//   k_uw_uvs        the three UVs of a triangle and its chart's dense number
//
// parent[] only ever decreases and parent[x] is always in x's component, so a racing reader sees a valid forest at every
// moment; the final roots depend on the triangles alone.  Every float operation is f32 without contraction.
#pragma once

#include "lupin_lightmap.hpp"

constexpr uint32_t LP_UW_NONE = 0xFFFFFFFFu;   // LUPIN_UNWRAP_NO_CHART: a degenerate triangle's bucket, label and chart

// the bucket 2 * axis + (negative ? 1 : 0) of the dominant axis of n = cross(p1 - p0, p2 - p0), or LP_UW_NONE
LP_DEV uint32_t uw_bucket(f3 p0, f3 p1, f3 p2)
{
    const f3 a = sub(p1, p0), b = sub(p2, p0);
    const float nx = a.y * b.z - a.z * b.y, ny = a.z * b.x - a.x * b.z, nz = a.x * b.y - a.y * b.x;
    if (!(isfinite(nx) && isfinite(ny) && isfinite(nz)) || (nx == 0.0f && ny == 0.0f && nz == 0.0f)) return LP_UW_NONE;
    uint32_t k = 0u;
    float best = fabsf(nx), nk = nx;
    if (fabsf(ny) > best) { k = 1u; best = fabsf(ny); nk = ny; }
    if (fabsf(nz) > best) { k = 2u; nk = nz; }
    return 2u * k + (nk >= 0.0f ? 0u : 1u);
}

LP_DEV float uw_axis(f3 p, uint32_t k) { return k == 0u ? p.x : (k == 1u ? p.y : p.z); }

// plane coordinates of a point in a bucket: (p[(k+1)%3], p[(k+2)%3]), swapped for a negative bucket; + 0.0f makes -0 a +0
LP_DEV void uw_project(f3 p, uint32_t bucket, float &s, float &t)
{
    const uint32_t k = bucket >> 1;
    const float a = uw_axis(p, (k + 1u) % 3u) + 0.0f, b = uw_axis(p, (k + 2u) % 3u) + 0.0f;
    if (bucket & 1u) { s = b; t = a; } else { s = a; t = b; }
}

// an unsigned image of a float that keeps the order of finite floats, and back
LP_DEV uint32_t uw_ordered(float f)
{
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
LP_DEV float uw_unordered(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

LP_DEV uint32_t uw_load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// the root of x as the forest stands; every node passed gets its grandparent (atomicMin: parents only decrease)
LP_DEV uint32_t uw_find(uint32_t *parent, uint32_t x)
{
    for (;;)
    {
        const uint32_t p = uw_load(parent + x);
        if (p == x) return x;
        const uint32_t g = uw_load(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = g;
    }
}

LP_DEV void uw_unite(uint32_t *parent, uint32_t a, uint32_t b)
{
    for (;;)
    {
        a = uw_find(parent, a);
        b = uw_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t s = a; a = b; b = s; }      // a is the larger root: it goes under b
        if (atomicCAS(parent + a, a, b) == a) return;           // a was still a root; otherwise find again
    }
}

// `tris` and `indices` point at the mesh's first triangle; table has 6 * V words (0xFF-filled before)
__global__ void __launch_bounds__(LP_BLOCK) k_uw_classify(const TriVerts *__restrict__ tris, const uint32_t *__restrict__ indices, uint32_t T, uint32_t V,
                                                          uint32_t *__restrict__ bucket, uint32_t *__restrict__ parent, uint32_t *__restrict__ table)
{
    const uint32_t t = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (t >= T) return;
    const TriVerts tv = tris[t];
    const uint32_t b = uw_bucket(xyz(tv.v0), xyz(tv.v1), xyz(tv.v2));
    bucket[t] = b;
    parent[t] = t;
    if (b == LP_UW_NONE) return;
    for (uint32_t k = 0; k < 3u; k++)
    {
        const uint32_t v = indices[(size_t)t * 3 + k];
        if (v < V) atomicMin(table + (size_t)b * V + v, t);     // (scene creation has refused an index >= V)
    }
}

__global__ void __launch_bounds__(LP_BLOCK) k_uw_union(const uint32_t *__restrict__ indices, uint32_t T, uint32_t V, const uint32_t *__restrict__ bucket,
                                                       const uint32_t *__restrict__ table, uint32_t *parent)
{
    const uint32_t t = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (t >= T) return;
    const uint32_t b = bucket[t];
    if (b == LP_UW_NONE) return;
    for (uint32_t k = 0; k < 3u; k++)
    {
        const uint32_t v = indices[(size_t)t * 3 + k];
        if (v >= V) continue;
        const uint32_t other = table[(size_t)b * V + v];        // <= t < T: t itself has touched this entry
        if (other < T && other != t) uw_unite(parent, t, other);
    }
}

// box_min (2 words a triangle, 0xFF-filled before) and box_max (2 words, zero-filled before) are used at the labels' places
__global__ void __launch_bounds__(LP_BLOCK) k_uw_flatten(const TriVerts *__restrict__ tris, uint32_t T, const uint32_t *__restrict__ bucket, uint32_t *parent,
                                                         uint32_t *__restrict__ label, uint32_t *__restrict__ roots, uint32_t *__restrict__ box_min,
                                                         uint32_t *__restrict__ box_max)
{
    const uint32_t t = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (t >= T) return;
    const uint32_t b = bucket[t];
    uint32_t l = LP_UW_NONE;
    if (b != LP_UW_NONE)
    {
        l = uw_find(parent, t);
        const TriVerts tv = tris[t];
        const f3 p[3] = {xyz(tv.v0), xyz(tv.v1), xyz(tv.v2)};
        for (uint32_t k = 0; k < 3u; k++)
        {
            float s, q;
            uw_project(p[k], b, s, q);
            atomicMin(box_min + 2 * (size_t)l, uw_ordered(s)); atomicMin(box_min + 2 * (size_t)l + 1, uw_ordered(q));
            atomicMax(box_max + 2 * (size_t)l, uw_ordered(s)); atomicMax(box_max + 2 * (size_t)l + 1, uw_ordered(q));
        }
    }
    label[t] = l;
    roots[t] = l == t ? t : LP_LM_NO_OWNER;
}

// order-preserving compaction of the roots (block_offsets: k_lm_count's totals after k_lm_scan): chart c, the c-th root in
// ascending order, gets its label and its box (min s, min t, max s, max t); dense[root] = c
__global__ void __launch_bounds__(LP_BLOCK) k_uw_compact(uint32_t T, const uint32_t *__restrict__ roots, const uint32_t *__restrict__ block_offsets,
                                                         const uint32_t *__restrict__ box_min, const uint32_t *__restrict__ box_max,
                                                         uint32_t *__restrict__ chart_label, float4 *__restrict__ chart_box, uint32_t *__restrict__ dense)
{
    __shared__ uint32_t lds_wave[LP_BLOCK / 64u];
    const uint32_t t = blockIdx.x * LP_BLOCK + threadIdx.x;
    const bool root = t < T && roots[t] != LP_LM_NO_OWNER;
    uint32_t before, total;
    lm_block_rank(root, lds_wave, before, total);
    if (!root) return;
    const uint32_t c = block_offsets[blockIdx.x] + before;
    chart_label[c] = t;
    chart_box[c] = make_float4(uw_unordered(box_min[2 * (size_t)t]), uw_unordered(box_min[2 * (size_t)t + 1]), uw_unordered(box_max[2 * (size_t)t]),
                               uw_unordered(box_max[2 * (size_t)t + 1]));
    dense[t] = c;
}

// chart_origin: per chart ((float)(rect.x + padding), (float)(rect.y + padding)).  uvs: 3 float2 a triangle.
__global__ void __launch_bounds__(LP_BLOCK) k_uw_uvs(const TriVerts *__restrict__ tris, uint32_t T, const uint32_t *__restrict__ bucket,
                                                     const uint32_t *__restrict__ label, const uint32_t *__restrict__ dense,
                                                     const float4 *__restrict__ chart_box, const float2 *__restrict__ chart_origin, float texel_size,
                                                     float2 *__restrict__ uvs, uint32_t *__restrict__ chart_of_tri)
{
    const uint32_t t = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (t >= T) return;
    const uint32_t b = bucket[t];
    float2 uv[3] = {make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f), make_float2(0.0f, 0.0f)};
    uint32_t c = LP_UW_NONE;
    if (b != LP_UW_NONE)
    {
        c = dense[label[t]];
        const float4 box = chart_box[c];
        const float2 o = chart_origin[c];
        const TriVerts tv = tris[t];
        const f3 p[3] = {xyz(tv.v0), xyz(tv.v1), xyz(tv.v2)};
        for (uint32_t k = 0; k < 3u; k++)
        {
            float s, q;
            uw_project(p[k], b, s, q);
            uv[k] = make_float2(o.x + (s - box.x) / texel_size, o.y + (q - box.y) / texel_size);
        }
    }
    uvs[3 * (size_t)t] = uv[0]; uvs[3 * (size_t)t + 1] = uv[1]; uvs[3 * (size_t)t + 2] = uv[2];
    chart_of_tri[t] = c;
}
