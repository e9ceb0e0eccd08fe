// lupin_bent_normal.hpp -- bent-normal queries, included once by lupin_hip.hip after lupin_transmittance.hpp.
//
// lupin_hip_bent_normal_rays answers "how much of the hemisphere is open, and which way does the open part point?" for
// caller-supplied surface records: the hemisphere-mode records and slots of lupin_hip_occlusion_rays (slot s of a record has
// that mode's RNG state and direction d_s, bit for bit), a weight T_s per slot -- 1.0f / 0.0f from scene_any_hit, or
// scene_transmittance's T with LUPIN_BENT_NORMAL_OPACITY -- and, per record, the four sums
//     (sum T_s * d_s.x,  sum T_s * d_s.y,  sum T_s * d_s.z,  sum T_s)
// The caller divides the last by `samples` (ambient-occlusion visibility) and normalises the first three (the
// cosine-weighted bent normal).
//
//   (device records are checked by k_validate_records: OcclusionRecordRule for the query, RayRecordRule for the atlas bake)
//   k_bent_normal<LDSGEO, OPACITY>   one wave per record, LP_BLOCK / 64 records per block: lane l traces the record's slots
//                                    l, l + 64, ... in ascending order and adds each to four registers that start at +0
//                                    (acc.x = acc.x + T * d.x, .y, .z alike, acc.w = acc.w + T); an xor butterfly (offsets
//                                    32, 16, .. 1: acc = acc + the partner's acc, per component) adds the 64 partial sums;
//                                    lane 0 stores one float4.  No slot plane, no second kernel.
//   (lupin_hip_bake_lightmap_ao runs this kernel on the rasteriser's records; its per-texel formulas: k_lm_ao_scatter, lupin_lightmap.hpp)
//
// The order of every addition is k_transmittance_resolve's, per component, so .w is that kernel's word when the weights are
// the same; it is restated in numpy (tests/bent_normal_ref.py).  No float atomics.  A record is never split between waves
// or launches, so the words do not depend on how the host cuts the batch.  Records are not packed several to a wave for
// small `samples`: lanes without a slot hold +0 and the butterfly adds them, which leaves the words of the definition.
// Every float operation is f32 without contraction (-ffp-contract=off), as everywhere in the library.
#pragma once

#include "lupin_transmittance.hpp"

constexpr uint32_t LP_BENT_NORMAL_RECORDS_PER_BLOCK = LP_BLOCK / 64u;

// `records` and `out` point at the chunk's first record; num_records * 64 lanes stay below 2^32.  Whole blocks run
// (make_geo<true> has a barrier): the waves of records past num_records leave after it, as whole waves, so the shuffles
// below see 64 lanes; a lane whose slot loop is empty (samples < 64) takes part in them holding +0.  fixed_tmax != 0: every
// slot's tmax is `tmax_all` and the records' word [7] is not read as a float (the atlas bake's records carry the radiance
// query's mode there).
template <bool LDSGEO, bool OPACITY>
__global__ void __launch_bounds__(LP_BLOCK) k_bent_normal(SceneDev sc, uint32_t num_records, const float4 *__restrict__ records, uint32_t samples,
                                                          float eps, uint32_t fixed_tmax, float tmax_all, float4 *__restrict__ out,
                                                          uint32_t stack_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const auto geo = make_geo<LDSGEO>(sc, lds_stack, stack_words);
    const uint32_t rec = blockIdx.x * LP_BENT_NORMAL_RECORDS_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (rec >= num_records) return;
    const float4 a = records[2 * (size_t)rec], b = records[2 * (size_t)rec + 1];
    const f3 o = mk3(a.x, a.y, a.z), nrm = mk3(b.x, b.y, b.z);
    const float tmax = __builtin_fminf(fixed_tmax ? tmax_all : b.w, LP_F32_MAX);   // +inf: unbounded
    float ax = 0.0f, ay = 0.0f, az = 0.0f, aw = 0.0f;
    for (uint32_t s = lane; s < samples; s += 64u)
    {
        // the slot's state and direction as k_begin_rays derives them for LUPIN_RAY_COSINE_HEMISPHERE (and k_occlusion)
        uint32_t rng = __float_as_uint(a.w);
        if (s != 0u) rng = hash_u32(rng + s * LP_RAY_SAMPLE_STRIDE);
        const float r0 = rnd(rng), r1 = rnd(rng);
        const f3 d = sample_cos_hemisphere(nrm, r0, r1);
        float T;
        if (OPACITY) T = scene_transmittance(geo, sc, lds_stack, o, d, eps, tmax);
        else T = scene_any_hit(geo, sc, lds_stack, o, d, eps, tmax) ? 0.0f : 1.0f;
        ax = ax + T * d.x;
        ay = ay + T * d.y;
        az = az + T * d.z;
        aw = aw + T;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
    {
        ax = ax + __shfl_xor(ax, off);
        ay = ay + __shfl_xor(ay, off);
        az = az + __shfl_xor(az, off);
        aw = aw + __shfl_xor(aw, off);
    }
    if (lane == 0u) out[rec] = make_float4(ax, ay, az, aw);
}
