// lupin_occlusion.hpp -- occlusion queries, included once by lupin_hip.hip after lupin_probes.hpp.
//
// lupin_hip_occlusion_rays answers "is anything in the way?" for caller-supplied segments: an any-hit traversal of the
// binary hierarchy that stops at the first triangle it accepts.  Record i expands into `samples` slots,
// slot = i * samples + s, one lane each; the result is, per record, the number of its slots that are blocked.
//
// DEFINITION.  A segment (o, d, eps, tmax) is blocked iff some triangle the traversal tests has eps <= t < tmax, where t is
// tri_dst's value for that triangle (tri_dst already turns t < eps into a miss, LP_F32_MAX).  The traversal visits the nodes
// whose slab distance is below the CONSTANT tmax: the bound never shrinks, so the visited set depends on tmax alone.
// Material opacity is not consulted: this is geometric visibility.
//
//   k_validate_records<OcclusionRecordRule>   device records only: counts the records the host check would refuse (the
//                          host reads the count before the first launch)
//   k_occlusion<LDSGEO>    one lane per slot: direction (as given, or cosine-weighted about the normal exactly as a mode-1
//                          radiance query derives it), scene_any_hit, then the lanes of a wave that share a record are
//                          combined by ballot / popcount and their first lane adds the count with one atomicAdd
//
// Counts are integers: the order of the additions cannot matter.
// Every float operation is f32 without contraction (-ffp-contract=off), as everywhere in the library.
#pragma once

#include "lupin_rays.hpp"

constexpr uint32_t LP_OCCLUSION_DIRECTION = 0u, LP_OCCLUSION_COSINE_HEMISPHERE = 1u;   // LUPIN_OCCLUSION_* (include/lupin_hip.h)

// What lupin_hip_occlusion_rays refuses in a record: what a mode-0 radiance query refuses (a non-finite origin, direction or
// normal, a squared length further than LP_RAY_UNIT_TOLERANCE from 1), and a tmax that is NaN or <= 0 (+inf is "unbounded").
// The host check and OcclusionRecordRule share this function.
__host__ __device__ inline bool occlusion_record_ok(float ox, float oy, float oz, float dx, float dy, float dz, float tmax)
{
    return ray_record_ok(ox, oy, oz, dx, dy, dz, LP_RAY_DIRECTION) && tmax > 0.0f;   // (NaN > 0 is false)
}

// the record format (lupin_rays.hpp says what a Rule is); transmittance queries share it
struct OcclusionRecordRule
{
    static constexpr uint32_t FLOATS = LUPIN_OCCLUSION_RECORD_FLOATS;
    static constexpr const char *NOUN = "record", *WHY = "non-finite component, direction or normal not of unit length, or tmax NaN or not positive";
    static bool host_ok(const float *r) { return occlusion_record_ok(r[0], r[1], r[2], r[4], r[5], r[6], r[7]); }
    static __device__ bool ok(const float4 *__restrict__ records, unsigned long long i)
    {
        const float4 a = records[2 * i], b = records[2 * i + 1];
        return occlusion_record_ok(a.x, a.y, a.z, b.x, b.y, b.z, b.w);
    }
};

// scene_closest's single convergent two-level loop (lupin_device.hpp), with the same per-lane LDS stack, near / far choice
// (ld <= rd), instance entry arithmetic (the direction is not re-normalised: t stays in world units), slab_dst and tri_dst.
// It differs in exactly two ways: the pruning bound is the constant tmax (ld < tmax, rd < tmax), and the function returns
// true at the first triangle whose tri_dst(...).t < tmax.  Binary hierarchy only (DESIGN.md 18 says why).
template <typename Geo>
LP_DEV bool scene_any_hit(const Geo &geo, const SceneDev &sc, uint32_t *stack, f3 o, f3 d, float eps, float tmax)
{
    const uint32_t tid = threadIdx.x;
    constexpr uint32_t REF_DONE = 0xFFFFFFFFu;   // not a valid leaf reference (leaf payloads are < 2^31 - 1)
    if (sc.num_instances == 0) return false;
    const f3 inv_d = mk3(1.0f / d.x, 1.0f / d.y, 1.0f / d.z);

    f3 co = o, cd = d, cinv = inv_d;       // ray of the current level (world, or instance-local)
    uint32_t sp = 0;
    uint32_t blas_base = 0xFFFFFFFFu;      // stack height at instance entry; all-ones = at TLAS level
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
        if (cur == REF_DONE) return false;

        // ---- phase 2: leaves ----
        if (blas_base == 0xFFFFFFFFu)
        {
            // TLAS leaf: enter the instance
            const InstanceDev in = geo.inst(cur & ~REF_LEAF);
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
            // BLAS leaf: the first triangle below tmax ends the query
            uint32_t ti = cur & ~REF_LEAF;
            for (;;)
            {
                const TriVerts tv = geo.tri(ti);
                const TriHit h = tri_dst(co, cd, xyz(tv.v0), xyz(tv.v1), xyz(tv.v2), eps);
                if (h.t < tmax) return true;
                if (__float_as_uint(tv.v0.w) & LEAF_END_BITS) break;
                ti++;
            }
            pop();
        }
    }
}

// `records` and `out` point at the chunk's first record; n = the chunk's slots (records * samples), below 2^31.  Whole blocks
// run (make_geo<true> has a barrier, and the ballots below see 64 lanes); lanes past n test nothing and count nothing.
// Slots ascend with the lane, so the lanes of a wave that share a record are contiguous: the first of them (its left
// neighbour has another record) counts the blocked lanes up to the next such lane and adds them to the zero-initialised
// counter.  With samples >= 64 that is one atomic per wave at most; a segment without a blocked lane adds nothing.
template <bool LDSGEO>
__global__ void __launch_bounds__(LP_BLOCK) k_occlusion(SceneDev sc, uint32_t n, const float4 *__restrict__ records, uint32_t samples, uint32_t mode,
                                                        float eps, uint32_t *__restrict__ out, uint32_t stack_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const auto geo = make_geo<LDSGEO>(sc, lds_stack, stack_words);
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x, lane = threadIdx.x & 63u;
    const bool live = slot < n;
    uint32_t rec = 0xFFFFFFFFu;   // no record: a lane past n is a segment of its own
    bool blocked = false;
    if (live)
    {
        rec = slot / samples;
        const uint32_t s = slot - rec * samples;
        const float4 a = records[2 * (size_t)rec], b = records[2 * (size_t)rec + 1];
        f3 d = mk3(b.x, b.y, b.z);
        if (mode == LP_OCCLUSION_COSINE_HEMISPHERE)
        {
            // the slot's state and direction as k_begin_rays derives them for LUPIN_RAY_COSINE_HEMISPHERE
            uint32_t rng = __float_as_uint(a.w);
            if (s != 0u) rng = hash_u32(rng + s * LP_RAY_SAMPLE_STRIDE);
            const float r0 = rnd(rng), r1 = rnd(rng);
            d = sample_cos_hemisphere(d, r0, r1);
        }
        const float tmax = __builtin_fminf(b.w, LP_F32_MAX);   // +inf: unbounded
        blocked = scene_any_hit(geo, sc, lds_stack, mk3(a.x, a.y, a.z), d, eps, tmax);
    }
    const uint32_t left = __shfl_up(rec, 1);
    const bool first = lane == 0u || left != rec;
    const unsigned long long firsts = __ballot(first), hits = __ballot(blocked);
    if (first && live)
    {
        const unsigned long long from = ~0ull << lane;                           // this lane and those above it
        const unsigned long long above = firsts & ~((2ull << lane) - 1ull);      // the segments that start above this lane
        const unsigned long long upto = above ? (1ull << (__ffsll((long long)above) - 1)) - 1ull : ~0ull;
        const uint32_t count = (uint32_t)__popcll(hits & from & upto);
        if (count) atomicAdd(&out[rec], count);
    }
}
