// lupin_transmittance.hpp -- transmittance queries, included once by lupin_hip.hip after lupin_occlusion.hpp.
//
// lupin_hip_transmittance_rays answers "how much gets through?" for caller-supplied segments: occlusion's records, modes and
// slots (slot = i * samples + s, one lane each), but the traversal does not stop at the first triangle.  It multiplies what
// each surface of the segment lets through and stops only when nothing is left.  The result is, per record, the SUM over its
// slots of the slot's transmittance T; the caller divides.
//
// DEFINITION.  T starts at 1.  Each triangle the traversal tests with eps <= t < tmax (t: tri_dst's value) contributes one
// factor, in the order the traversal meets them:
//   instance flag bit 0 clear ("opacity is exactly 1", set at upload)   T = 0, the query ends, no material is read
//   otherwise  a = surface_opacity(sc, resolve_surface(sc, inst, tri, u, v))
//              !(a < 1.0f)  (this includes NaN)                          T = 0, the query ends
//              else                                                       T = T * (1.0f - fmaxf(a, 0.0f))
// For a in [0, 1), 1 - a is the probability that the integrators' stochastic skip (trace_alpha: rnd(rng) >= a) lets a path
// through, so T is the EXPECTATION of that skip over the surfaces of one segment.  It is not a replay of trace_alpha, which
// restarts the ray at every skipped surface with a fresh ray_epsilon and gives up after 128 skips.  Colour is not consulted:
// a refractive or transparent material type with opacity 1 blocks.  The visited set is scene_any_hit's: the nodes whose slab
// distance is below the CONSTANT tmax, binary hierarchy only.
//
//   (device records are checked by occlusion's k_validate_records<OcclusionRecordRule>: one rule, one kernel)
//   k_transmittance<LDSGEO>    one lane per slot: direction exactly as k_occlusion derives it, scene_transmittance, T stored
//                              to out[slot] (direction mode: the caller's array; hemisphere mode: the context's slot plane)
//   k_transmittance_resolve    one wave per record: lane l adds slots l, l + 64, ... in ascending order, an xor butterfly
//                              (offsets 32, 16, .. 1) adds the 64 partial sums, lane 0 stores the sum
//
// The order of every addition is fixed and restated in numpy (tests/transmittance_ref.py); no float atomics.
// Every float operation is f32 without contraction (-ffp-contract=off), as everywhere in the library.
#pragma once

#include "lupin_occlusion.hpp"

// scene_any_hit's loop (lupin_occlusion.hpp): the same stack, near / far choice, instance entry arithmetic, slab_dst, tri_dst
// and constant pruning bound, tracking the current instance and its flags as scene_closest tracks the instance.  At a BLAS
// leaf an accepted triangle of a flag-clear instance ends the query with 0.  An accepted triangle of an alpha-capable
// instance leaves the triangle loop carrying (tri, u, v) only: the opacity (a texture fetch, three texcoords, three vertex
// colours) is evaluated between two runs of the triangle loop, where no node or triangle registers are alive, and only
// by the lanes that hit such a triangle.  Each triangle of a visited leaf is tested once.
template <typename Geo>
LP_DEV float scene_transmittance(const Geo &geo, const SceneDev &sc, uint32_t *stack, f3 o, f3 d, float eps, float tmax)
{
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t REF_DONE = 0xFFFFFFFFu;   // not a valid leaf reference (leaf payloads are < 2^31 - 1)
    float T = 1.0f;
    if (sc.num_instances == 0) return T;
    const f3 inv_d = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);

    f3 co = o, cd = d, cinv = inv_d;       // ray of the current level (world, or instance-local)
    uint32_t sp = 0;
    uint32_t blas_base = 0xFFFFFFFFu;      // stack height at instance entry; all-ones = at TLAS level
    uint32_t cur_inst = 0, cur_flags = 0;
    uint32_t cur = sc.tlas_root;

    auto pop = [&]() {
        if (sp == blas_base) { blas_base = 0xFFFFFFFFu; co = o; cd = d; cinv = inv_d; }
        if (sp == 0) { cur = REF_DONE; return; }
        sp--;
        cur = stack[sp * LP_BLOCK + tid];
    };

    for (;;)
    {
        // ---- phase 1: internal nodes of either level ----
        while (!(cur & REF_LEAF))
        {
            const NodeRegs nd = geo.node(blas_base != 0xFFFFFFFFu, cur);
            float ld = slab_dst(co, cinv, LP_NODE_LEFT(nd));
            float rd = slab_dst(co, cinv, LP_NODE_RIGHT(nd));
            bool left_first = ld <= rd;
            bool push_l = ld < tmax, push_r = rd < tmax;
            uint32_t near_ref = left_first ? nd.left : nd.right;
            uint32_t far_ref = left_first ? nd.right : nd.left;
            bool push_near = left_first ? push_l : push_r;
            bool push_far = left_first ? push_r : push_l;
            if (push_far) { stack[sp * LP_BLOCK + tid] = far_ref; sp++; }
            if (push_near) cur = near_ref; else pop();
        }
        if (cur == REF_DONE) return T;

        // ---- phase 2: leaves ----
        if (blas_base == 0xFFFFFFFFu)
        {
            // TLAS leaf: enter the instance
            cur_inst = cur & ~REF_LEAF;
            const InstanceDev in = geo.inst(cur_inst);
            cur_flags = in.flags;
            co = mk3(o.x * in.r0.x + o.y * in.r0.y + o.z * in.r0.z + 1.0f * in.r0.w,
                     o.x * in.r1.x + o.y * in.r1.y + o.z * in.r1.z + 1.0f * in.r1.w,
                     o.x * in.r2.x + o.y * in.r2.y + o.z * in.r2.z + 1.0f * in.r2.w);
            cd = mk3(d.x * in.r0.x + d.y * in.r0.y + d.z * in.r0.z + 0.0f * in.r0.w,
                     d.x * in.r1.x + d.y * in.r1.y + d.z * in.r1.z + 0.0f * in.r1.w,
                     d.x * in.r2.x + d.y * in.r2.y + d.z * in.r2.z + 0.0f * in.r2.w);
            if (!(in.blas_root & REF_LEAF)) cinv = mk3(1.0f / cd.x, 1.0f / cd.y, 1.0f / cd.z);
            blas_base = sp;
            cur = in.blas_root;
        }
        else
        {
            // BLAS leaf: every triangle below tmax contributes its factor, in leaf order
            uint32_t ti = cur & ~REF_LEAF;
            bool more = true;
            while (more)
            {
                bool pending = false;
                uint32_t hit_tri = 0;
                float hit_u = 0.0f, hit_v = 0.0f;
                for (;;)
                {
                    const TriVerts tv = geo.tri(ti);
                    const TriHit h = tri_dst(co, cd, xyz(tv.v0), xyz(tv.v1), xyz(tv.v2), eps);
                    const bool last = (__float_as_uint(tv.v0.w) & LEAF_END_BITS) != 0u;
                    more = !last;
                    if (h.t < tmax)
                    {
                        if (!(cur_flags & 1u)) return 0.0f;   // opacity is exactly 1 there: no material is read
                        pending = true; hit_tri = ti; hit_u = h.u; hit_v = h.v;
                        ti++;
                        break;
                    }
                    if (last) break;
                    ti++;
                }
                if (pending)
                {
                    const float a = surface_opacity(sc, resolve_surface(sc, cur_inst, hit_tri, hit_u, hit_v));
                    if (!(a < 1.0f)) return 0.0f;             // (NaN ends here too)
                    T = T * (1.0f - __builtin_fmaxf(a, 0.0f));
                    if (T == 0.0f) return 0.0f;
                }
            }
            pop();
        }
    }
}

// `records` and `out` point at the chunk's first record / slot; n = the chunk's slots (records * samples), below 2^31.  Whole
// blocks run (make_geo<true> has a barrier); lanes past n test nothing and store nothing.  out[slot] = T: with samples == 1
// that is the record's result, otherwise the slot plane k_transmittance_resolve sums.
template <bool LDSGEO>
__global__ void __launch_bounds__(LP_BLOCK) k_transmittance(SceneDev sc, uint32_t n, const float4 *__restrict__ records, uint32_t samples, uint32_t mode,
                                                            float eps, float *__restrict__ out, uint32_t stack_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const auto geo = make_geo<LDSGEO>(sc, lds_stack, stack_words);
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (slot >= n) return;
    const uint32_t rec = slot / samples;
    const uint32_t s = slot - rec * samples;
    const float4 a = records[2 * (size_t)rec], b = records[2 * (size_t)rec + 1];
    f3 d = mk3(b.x, b.y, b.z);
    if (mode == LP_OCCLUSION_COSINE_HEMISPHERE)
    {
        // the slot's state and direction as k_begin_rays derives them for LUPIN_RAY_COSINE_HEMISPHERE (and k_occlusion)
        uint32_t rng = __float_as_uint(a.w);
        if (s != 0u) rng = hash_u32(rng + s * LP_RAY_SAMPLE_STRIDE);
        const float r0 = rnd(rng), r1 = rnd(rng);
        d = sample_cos_hemisphere(d, r0, r1);
    }
    const float tmax = __builtin_fminf(b.w, LP_F32_MAX);   // +inf: unbounded
    out[slot] = scene_transmittance(geo, sc, lds_stack, mk3(a.x, a.y, a.z), d, eps, tmax);
}

// One wave per record of the chunk, LP_BLOCK / 64 records per block.  Lane l adds the record's slots l, l + 64, ... to a
// zero in ascending order; the xor butterfly (offsets 32, 16, 8, 4, 2, 1: acc = acc + the partner's acc) leaves the same sum
// in every lane (f32 addition is commutative); lane 0 stores it.  Consecutive lanes read consecutive slots.
constexpr uint32_t LP_TRANSMITTANCE_RECORDS_PER_BLOCK = LP_BLOCK / 64u;
__global__ void __launch_bounds__(LP_BLOCK) k_transmittance_resolve(const float *__restrict__ plane, uint32_t num_records, uint32_t samples,
                                                                    float *__restrict__ out)
{
    const uint32_t rec = blockIdx.x * LP_TRANSMITTANCE_RECORDS_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (rec >= num_records) return;   // whole waves leave: the shuffles below see 64 lanes
    const size_t first = (size_t)rec * samples;
    float acc = 0.0f;
    for (uint32_t s = lane; s < samples; s += 64u) acc = acc + plane[first + s];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (lane == 0u) out[rec] = acc;
}
