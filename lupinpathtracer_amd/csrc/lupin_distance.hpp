// lupin_distance.hpp -- distance queries, included once by lupin_hip.hip after lupin_occlusion.hpp.
//
// lupin_hip_distance_points and lupin_hip_bake_distance_grid answer "how far is the nearest surface, where is it and which
// side of it am I on?" for points: a nearest-point traversal of the binary hierarchy whose pruning bound is the squared
// distance from the query point to a box, and whose leaf test is the closest point on a triangle.
//
// DEFINITION.  A query is (p, rmax).  Over every triangle of every instance, taken in WORLD space (its vertices through the
// instance's local -> world rows, the f32 inverse lupin_mat3x4_inverse gives of the world -> local rows), c* is the nearest
// point of the surface; found = |p - c*| < rmax.  A triangle whose world-space cross product (v1 - v0) x (v2 - v0) has a
// squared length of zero in f32 is SKIPPED, and so is every triangle of an instance whose rows have no finite inverse.
// Material opacity is not consulted.
//
//   k_validate_records<DistanceRecordRule>   device records only: counts the records the host check would refuse
//   k_distance<LDSGEO>     one lane per record; three float4 stores per result
//   k_distance_grid<LDSGEO> one lane per voxel, x fastest: centre = origin + (i + 0.5) * spacing per axis, one float per voxel
//
// Every float operation is f32 without contraction (-ffp-contract=off), as everywhere in the library.  No inline assembly.
#pragma once

#include "lupin_occlusion.hpp"

constexpr uint32_t LP_DISTANCE_GRID_SIGNED = 2u;   // LUPIN_DISTANCE_GRID_SIGNED (include/lupin_hip.h)
constexpr uint32_t LP_DISTANCE_AUX_WORDS = 4u;     // float4 per instance: local -> world rows 0..2, then (c_i, 0, 0, 0)

// What the distance entry points refuse in a record: a non-finite point, an rmax that is NaN or <= 0 (+inf is "unbounded").
// The host check and DistanceRecordRule share this function.
__host__ __device__ inline bool distance_record_ok(float px, float py, float pz, float rmax)
{
    const float s = (px - px) + (py - py) + (pz - pz);   // 0 for finite components, NaN otherwise
    return s == 0.0f && rmax > 0.0f;                     // (NaN > 0 is false)
}

struct DistanceRecordRule   // the record format (lupin_rays.hpp says what a Rule is)
{
    static constexpr uint32_t FLOATS = LUPIN_DISTANCE_RECORD_FLOATS;
    static constexpr const char *NOUN = "record", *WHY = "non-finite point, or rmax NaN or not positive";
    static bool host_ok(const float *r) { return distance_record_ok(r[0], r[1], r[2], r[3]); }
    static __device__ bool ok(const float4 *__restrict__ records, unsigned long long i)
    {
        const float4 a = records[i];
        return distance_record_ok(a.x, a.y, a.z, a.w);
    }
};

// The flag word of a node (WideNode.d.z: bit 0 / 1 = the left / right child's stored box does not bound its triangles), read
// beside node() so that NodeRegs and every kernel that uses it stay what they were.  0 in a TLAS node.
LP_DEV uint32_t node_flags(const GeoGlobal &g, uint32_t i) { return g.blas[i].d.z; }
LP_DEV uint32_t node_flags(const GeoLds &g, uint32_t i) { return __float_as_uint(g.base[i * LP_GEO_LDS_STRIDE + 3u].z); }

// squared distance from p to the box [lo, hi], per axis max(lo - p, p - hi, 0): zero inside.  A NaN bound gives NaN, which
// is not below any bound: such a child is not entered (the empty slots of a degenerate node).
LP_DEV float box_dst2(f3 p, float lox, float loy, float loz, float hix, float hiy, float hiz)
{
    const float dx = maxf(maxf(lox - p.x, p.x - hix), 0.0f);
    const float dy = maxf(maxf(loy - p.y, p.y - hiy), 0.0f);
    const float dz = maxf(maxf(loz - p.z, p.z - hiz), 0.0f);
    return dx * dx + dy * dy + dz * dz;
}

// Closest point of the triangle (a, b, c) to p by Voronoi-region classification (Ericson, Real-Time Collision Detection
// 5.1.5): dot products only, the two divisions are the final barycentrics.  The point is a + (b - a) u + (c - a) v.
struct TriNear { float d2, u, v; };
LP_DEV f3 tri_point(f3 a, f3 b, f3 c, float u, float v)
{
    const f3 ab = sub(b, a), ac = sub(c, a);
    return mk3(a.x + ab.x * u + ac.x * v, a.y + ab.y * u + ac.y * v, a.z + ab.z * u + ac.z * v);
}
LP_DEV TriNear tri_nearest(f3 p, f3 a, f3 b, f3 c)
{
    const f3 ab = sub(b, a), ac = sub(c, a);
    const f3 ap = sub(p, a), bp = sub(p, b), cp = sub(p, c);
    const float d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    const float d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    const float d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float e43 = d4 - d3, e56 = d5 - d6;
    // the regions in reverse order of precedence, so that the earlier one of Ericson's sequence wins
    float nu = vb, nv = vc, den = (va + vb) + vc;                                                     // face
    if (va <= 0.0f && e43 >= 0.0f && e56 >= 0.0f) { nu = e56; nv = e43; den = e43 + e56; }            // edge bc
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { nu = 0.0f; nv = d2; den = d2 - d6; }                // edge ac
    if (d6 >= 0.0f && d5 <= d6) { nu = 0.0f; nv = 1.0f; den = 1.0f; }                                 // vertex c
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { nu = d1; nv = 0.0f; den = d1 - d3; }                // edge ab
    if (d3 >= 0.0f && d4 <= d3) { nu = 1.0f; nv = 0.0f; den = 1.0f; }                                 // vertex b
    if (d1 <= 0.0f && d2 <= 0.0f) { nu = 0.0f; nv = 0.0f; den = 1.0f; }                               // vertex a
    TriNear r;
    r.u = nu / den; r.v = nv / den;
    const f3 q = sub(p, tri_point(a, b, c, r.u, r.v));
    r.d2 = dot3(q, q);
    const f3 n = cross3(ab, ac);
    if (dot3(n, n) == 0.0f) r.d2 = LP_F32_MAX * 2.0f;   // zero area: skipped (+inf is below no bound)
    return r;
}

// local -> world of a vertex, the expression of the TLAS builder's box corners (lupin_internal_tlas_leaves): being the same
// monotone f32 expression of the same matrix, it puts every vertex of the mesh inside the instance's TLAS box exactly
LP_DEV f3 to_world(float4 m0, float4 m1, float4 m2, float4 v)
{
    return mk3(m0.x * v.x + m0.y * v.y + m0.z * v.z + m0.w * 1.0f,
               m1.x * v.x + m1.y * v.y + m1.z * v.z + m1.w * 1.0f,
               m2.x * v.x + m2.y * v.y + m2.z * v.z + m2.w * 1.0f);
}

struct NearestHit
{
    float d2;            // squared distance of the best triangle; the starting bound when nothing was accepted
    float u, v;
    uint32_t tri, inst;  // global triangle index; 0xFFFFFFFF = nothing accepted
};

// scene_closest's single convergent two-level loop (lupin_device.hpp) with the per-lane LDS stack, over the binary
// hierarchy only.  What differs from scene_any_hit:
//   * the bound `best` is a squared distance that starts at `bound2` and shrinks with every accepted triangle;
//   * a child's key is box_dst2 of the query point (world at the TLAS level, pl = R p + t inside an instance) times the
//     level's scale (1, or c_i^2 with c_i <= 1 / sigma_max(R): a lower bound of the world distance); a child whose flag bit
//     is set (its box does not bound its triangles) has key 0; the nearer child is visited first, the farther one pushed if
//     its key < best;
//   * the stack holds (reference, key) PAIRS, entry e of lane t at stack[(2 e) * LP_BLOCK + t] and [(2 e + 1) * LP_BLOCK + t]
//     (the wide tracer's layout): a popped entry whose key is no longer < best is dropped without a fetch.  The depth bound
//     is scene->stack_entries entries, 2 * stack_entries * LP_BLOCK words.
//   * a leaf tests every triangle in world space and accepts d2 < best.
// aux: LP_DISTANCE_AUX_WORDS float4 per instance (local -> world rows, c_i; c_i < 0: the instance is skipped).
template <typename Geo>
LP_DEV NearestHit scene_nearest(const Geo &geo, const SceneDev &sc, uint32_t *stack, f3 p, float bound2, const float4 *__restrict__ aux)
{
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t REF_DONE = 0xFFFFFFFFu;   // not a valid leaf reference (leaf payloads are < 2^31 - 1)
    NearestHit best;
    best.d2 = bound2; best.u = 0.0f; best.v = 0.0f; best.tri = 0xFFFFFFFFu; best.inst = 0xFFFFFFFFu;
    if (sc.num_instances == 0) return best;

    f3 cp = p;                             // query point of the current level (world, or instance-local)
    float kscale = 1.0f;                   // key = box_dst2 * kscale
    float4 m0 = make_float4(0, 0, 0, 0), m1 = m0, m2 = m0;   // local -> world rows of the current instance
    uint32_t cur_inst = 0;
    uint32_t sp = 0;
    uint32_t blas_base = 0xFFFFFFFFu;      // stack height at instance entry; all-ones = at TLAS level
    uint32_t cur = sc.tlas_root;

    auto pop = [&]() {
        for (;;)
        {
            if (sp == blas_base) { blas_base = 0xFFFFFFFFu; cp = p; kscale = 1.0f; }
            if (sp == 0) { cur = REF_DONE; return; }
            sp--;
            const float key = __uint_as_float(stack[(2u * sp + 1u) * LP_BLOCK + tid]);
            if (key < best.d2) { cur = stack[(2u * sp) * LP_BLOCK + tid]; return; }   // the bound has moved since the push
        }
    };

    for (;;)
    {
        // ---- phase 1: internal nodes of either level ----
        while (!(cur & REF_LEAF))
        {
            const NodeRegs nd = geo.node(blas_base != 0xFFFFFFFFu, cur);
            const uint32_t fl = node_flags(geo, cur);
            float lk = box_dst2(cp, LP_NODE_LEFT(nd)) * kscale;
            float rk = box_dst2(cp, LP_NODE_RIGHT(nd)) * kscale;
            if (fl & 1u) lk = 0.0f;
            if (fl & 2u) rk = 0.0f;
            const bool left_first = lk <= rk;
            const bool push_l = lk < best.d2, push_r = rk < best.d2;
            const uint32_t near_ref = left_first ? nd.left : nd.right;
            const uint32_t far_ref = left_first ? nd.right : nd.left;
            const float far_key = left_first ? rk : lk;
            const bool push_near = left_first ? push_l : push_r;
            const bool push_far = left_first ? push_r : push_l;
            if (push_far)
            {
                stack[(2u * sp) * LP_BLOCK + tid] = far_ref;
                stack[(2u * sp + 1u) * LP_BLOCK + tid] = __float_as_uint(far_key);
                sp++;
            }
            if (push_near) cur = near_ref; else pop();
        }
        if (cur == REF_DONE) return best;

        // ---- phase 2: leaves ----
        if (blas_base == 0xFFFFFFFFu)
        {
            // TLAS leaf: enter the instance
            cur_inst = cur & ~REF_LEAF;
            const InstanceDev in = geo.inst(cur_inst);
            const float4 a3 = aux[LP_DISTANCE_AUX_WORDS * cur_inst + 3u];
            if (a3.x < 0.0f) { pop(); continue; }   // no finite inverse: the instance contributes nothing
            m0 = aux[LP_DISTANCE_AUX_WORDS * cur_inst]; m1 = aux[LP_DISTANCE_AUX_WORDS * cur_inst + 1u]; m2 = aux[LP_DISTANCE_AUX_WORDS * cur_inst + 2u];
            cp = mk3(p.x * in.r0.x + p.y * in.r0.y + p.z * in.r0.z + 1.0f * in.r0.w,
                     p.x * in.r1.x + p.y * in.r1.y + p.z * in.r1.z + 1.0f * in.r1.w,
                     p.x * in.r2.x + p.y * in.r2.y + p.z * in.r2.z + 1.0f * in.r2.w);
            kscale = a3.x * a3.x;
            blas_base = sp;
            cur = in.blas_root;
        }
        else
        {
            // BLAS leaf: every triangle, in world space
            uint32_t ti = cur & ~REF_LEAF;
            for (;;)
            {
                const TriVerts tv = geo.tri(ti);
                const TriNear h = tri_nearest(p, to_world(m0, m1, m2, tv.v0), to_world(m0, m1, m2, tv.v1), to_world(m0, m1, m2, tv.v2));
                if (h.d2 < best.d2) { best.d2 = h.d2; best.u = h.u; best.v = h.v; best.tri = ti; best.inst = cur_inst; }
                if (__float_as_uint(tv.v0.w) & LEAF_END_BITS) break;
                ti++;
            }
            pop();
        }
    }
}

// The starting bound of a query: rmax^2 widened by a few ulps, so that the squared comparison of the traversal never refuses
// what the final comparison sqrt(d2) < rmax accepts.  rmax >= 2^64 squares to +inf: unbounded.  A tiny rmax squares to a
// denormal or to 0: the bound is at least the smallest normal float, so that a point ON the surface (d2 == 0 < bound) is
// still accepted and then judged by sqrt(d2) < rmax like every other.
LP_DEV float distance_bound2(float rmax)
{
    const float r2 = rmax * rmax;
    return maxf(r2 + r2 * 0x1p-21f, 1.17549435e-38f);
}

struct DistanceResult
{
    bool found;
    float distance;
    f3 point;
    float u, v;
    uint32_t inst, tri;   // tri: mesh-local, as lupin_hip_trace_rays reports it
    float side;           // +1, -1 or 0: the sign of dot(p - point, (v1 - v0) x (v2 - v0)) of that triangle in world space
};

// The winner's triangle is fetched again and its point recomputed by tri_nearest's own expression.
template <typename Geo>
LP_DEV DistanceResult distance_query(const Geo &geo, const SceneDev &sc, uint32_t *stack, f3 p, float rmax, const float4 *__restrict__ aux)
{
    const NearestHit h = scene_nearest(geo, sc, stack, p, distance_bound2(rmax), aux);
    DistanceResult r;
    r.found = false; r.distance = rmax; r.point = mk3(0.0f, 0.0f, 0.0f); r.u = 0.0f; r.v = 0.0f; r.inst = 0u; r.tri = 0u; r.side = 0.0f;
    if (h.tri == 0xFFFFFFFFu) return r;
    const float d = sqrtf(h.d2);
    if (!(d < rmax)) return r;
    const float4 m0 = aux[LP_DISTANCE_AUX_WORDS * h.inst], m1 = aux[LP_DISTANCE_AUX_WORDS * h.inst + 1u], m2 = aux[LP_DISTANCE_AUX_WORDS * h.inst + 2u];
    const TriVerts tv = geo.tri_fetch(h.tri);
    const f3 a = to_world(m0, m1, m2, tv.v0), b = to_world(m0, m1, m2, tv.v1), c = to_world(m0, m1, m2, tv.v2);
    r.found = true; r.distance = d; r.u = h.u; r.v = h.v; r.inst = h.inst;
    r.point = tri_point(a, b, c, h.u, h.v);
    r.tri = h.tri - sc.inst_meshes[h.inst].tri_offset;
    const float s = dot3(sub(p, r.point), cross3(sub(b, a), sub(c, a)));
    r.side = s > 0.0f ? 1.0f : (s < 0.0f ? -1.0f : 0.0f);
    return r;
}

// `records` and `out` point at the chunk's first record; n = the chunk's records, below 2^31.  Whole blocks run (make_geo<true>
// has a barrier); lanes past n write nothing.  Result i: three float4,
//   [found (bits) | distance | point.x | point.y]  [point.z | u | v | instance (bits)]  [tri (bits) | side | 0 | 0]
template <bool LDSGEO>
__global__ void __launch_bounds__(LP_BLOCK) k_distance(SceneDev sc, uint32_t n, const float4 *__restrict__ records, const float4 *__restrict__ aux,
                                                       float4 *__restrict__ out, uint32_t stack_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const auto geo = make_geo<LDSGEO>(sc, lds_stack, stack_words);
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 rec = records[i];
    const float rmax = __builtin_fminf(rec.w, LP_F32_MAX);   // +inf: unbounded
    const DistanceResult r = distance_query(geo, sc, lds_stack, mk3(rec.x, rec.y, rec.z), rmax, aux);
    float4 *o = out + 3 * (size_t)i;
    o[0] = make_float4(__uint_as_float(r.found ? 1u : 0u), r.found ? r.distance : 0.0f, r.point.x, r.point.y);
    o[1] = make_float4(r.point.z, r.u, r.v, __uint_as_float(r.inst));
    o[2] = make_float4(__uint_as_float(r.tri), r.side, 0.0f, 0.0f);
}

struct DistanceGrid
{
    float ox, oy, oz, sx, sy, sz;
    uint32_t nx, ny;       // voxel = ix + nx * (iy + ny * iz)
    float rmax;            // already clamped to LP_F32_MAX
    uint32_t flags;
};

// The centre of a voxel along one axis, in this order: (float(i) + 0.5f) * spacing, then origin + that.  i < 2^24 is exact.
LP_DEV float voxel_centre(float origin, uint32_t i, float spacing) { return origin + ((float)i + 0.5f) * spacing; }

// one lane per voxel of the chunk [first, first + n), x fastest: the lanes of a wave query neighbouring points
template <bool LDSGEO>
__global__ void __launch_bounds__(LP_BLOCK) k_distance_grid(SceneDev sc, unsigned long long first, uint32_t n, DistanceGrid g, const float4 *__restrict__ aux,
                                                            float *__restrict__ out, uint32_t stack_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const auto geo = make_geo<LDSGEO>(sc, lds_stack, stack_words);
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const unsigned long long voxel = first + i;
    const unsigned long long row = voxel / g.nx;
    const uint32_t ix = (uint32_t)(voxel - row * g.nx), iy = (uint32_t)(row % g.ny), iz = (uint32_t)(row / g.ny);
    const f3 p = mk3(voxel_centre(g.ox, ix, g.sx), voxel_centre(g.oy, iy, g.sy), voxel_centre(g.oz, iz, g.sz));
    const DistanceResult r = distance_query(geo, sc, lds_stack, p, g.rmax, aux);
    float v = r.distance;                                     // rmax where nothing was found
    if ((g.flags & LP_DISTANCE_GRID_SIGNED) && r.found) v = r.side == 0.0f ? 0.0f : v * r.side;
    out[i] = v;
}
