// lupin_lightmap_adaptive.hpp -- adaptive lightmap baking, included once by lupin_hip.hip after
// lupin_lightmap.hpp and lupin_adaptive.hpp.
//
// lupin_hip_bake_lightmap_adaptive is lupin_hip_bake_lightmap in rounds of `samples` paths per texel: the records are the
// lightmap's (lightmap_emit_records), every round traces only the records that still want samples, and a texel stops once
// the relative standard error of its luminance (adaptive_pixel_error, lupin_adaptive.hpp) is below the threshold and no
// atlas neighbour still wants samples.  lupin_hip_pathtrace_rays_moments is the radiance query with the round's resolve.
//
//   k_resolve_moments   one wave per record, two passes over its slots' `color`: the mean radiance and the mean luminance,
//                       then the sum of squared deviations of the luminance from that mean (M2); lane l takes slots l, l + 64,
//                       ... in ascending order, an xor butterfly adds the 64 partial sums
//   k_lm_ad_count       active records per block of LP_BLOCK records (lm_block_rank: ballot + popcount per wave)
//   (k_lm_scan          UNCHANGED, on the block totals)
//   k_lm_ad_emit        order-preserving compaction: the index of every active record, ascending, and its record with the
//                       round's RNG word
//   (the radiance query's wavefront on the round's records, k_resolve_moments after it)
//   k_lm_ad_merge       one thread per active record: the round's moments into the record's (Chan's pairwise update), its
//                       error, whether it wants more samples -> a byte at its texel
//   k_lm_ad_mask        one thread per record: active = not at the cap and (wants, or an atlas neighbour wants)
//   (k_lm_scatter, k_lm_dilate   UNCHANGED: the irradiance plane from the records' means)
//   k_lm_ad_stats       one thread per record: the four statistics of its texel, the counts of converged and capped texels
//
// The second moment is taken in two passes on purpose: sum l^2 - S * ml^2 cancels in f32 exactly where the samples agree
// with each other, which is where a texel converges first.  The order of every sum is part of the contract
// (include/lupin_hip.h) and restated in tests/lightmap_adaptive_ref.py.  Every operation is f32 without contraction
// (-ffp-contract=off), IEEE division and sqrt.
#pragma once

#include "lupin_lightmap.hpp"
#include "lupin_adaptive.hpp"

constexpr uint32_t LP_LM_AD_RECORDS_PER_BLOCK = LP_BLOCK / 64;
constexpr uint32_t LP_LM_AD_ROUND_STRIDE = 0x85EBCA6Bu;   // RNG word of round r > 0: hash_u32(word + r * stride); not LP_RAY_SAMPLE_STRIDE

// per owned record, for the length of one call; all zero at its start
struct LmAdaptiveDev
{
    uint32_t *samples;   // n_i
    uint32_t *rounds;    // rounds_i
    float4 *mean;        // (mean_r, mean_g, mean_b, ml_i): k_lm_scatter reads the first three
    float *m2;           // M2_i
};

LP_DEV uint32_t lm_ad_round_word(uint32_t word, uint32_t round)
{
    return round == 0u ? word : hash_u32(word + round * LP_LM_AD_ROUND_STRIDE);
}

// the sum of a value over the wave's 64 lanes, in every lane
LP_DEV float lm_ad_butterfly(float a)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a = a + __shfl_xor(a, off);
    return a;
}

// One wave per record of the chunk, LP_LM_AD_RECORDS_PER_BLOCK records per block; out: (mean_r, mean_g, mean_b, 1) and
// (ml, M2, samples, 0) per record.  The slots are read twice from `color`, never kept: `samples` has no bound.
__global__ void __launch_bounds__(LP_BLOCK) k_resolve_moments(PathBuffers pb, uint32_t num_records, uint32_t samples, float4 *__restrict__ out)
{
    const uint32_t rec = blockIdx.x * LP_LM_AD_RECORDS_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (rec >= num_records) return;   // whole waves leave: the shuffles below see 64 lanes
    const size_t first = (size_t)rec * samples;
    const float count = (float)samples;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sl = 0.0f;
    for (uint32_t s = lane; s < samples; s += 64u)
    {
        const float4 c = pb.color[first + s];
        const float lum = adaptive_luminance(c.x, c.y, c.z);
        sr += c.x;
        sg += c.y;
        sb += c.z;
        sl += lum;
    }
    sr = lm_ad_butterfly(sr);
    sg = lm_ad_butterfly(sg);
    sb = lm_ad_butterfly(sb);
    sl = lm_ad_butterfly(sl);
    const float ml = sl / count;
    float q = 0.0f;
    for (uint32_t s = lane; s < samples; s += 64u)
    {
        const float4 c = pb.color[first + s];
        const float lum = adaptive_luminance(c.x, c.y, c.z);
        q += (lum - ml) * (lum - ml);
    }
    q = lm_ad_butterfly(q);
    if (lane == 0u)
    {
        out[2 * (size_t)rec] = make_float4(sr / count, sg / count, sb / count, 1.0f);
        out[2 * (size_t)rec + 1] = make_float4(ml, q, count, 0.0f);
    }
}

__global__ void __launch_bounds__(LP_BLOCK) k_lm_ad_count(const uint8_t *__restrict__ active, uint32_t n, uint32_t *__restrict__ block_totals)
{
    __shared__ uint32_t lds_wave[LP_BLOCK / 64u];
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    const bool on = i < n && active[i] != 0u;
    uint32_t before, total;
    lm_block_rank(on, lds_wave, before, total);
    if (threadIdx.x == 0u) block_totals[blockIdx.x] = total;
}

// block_offsets: k_lm_scan's of k_lm_ad_count's totals.  Active record i becomes the round's record j (ascending in i).
__global__ void __launch_bounds__(LP_BLOCK) k_lm_ad_emit(const uint8_t *__restrict__ active, uint32_t n, const uint32_t *__restrict__ block_offsets,
                                                         const float4 *__restrict__ records, uint32_t round, float4 *__restrict__ round_records,
                                                         uint32_t *__restrict__ index_of)
{
    __shared__ uint32_t lds_wave[LP_BLOCK / 64u];
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    const bool on = i < n && active[i] != 0u;
    uint32_t before, total;
    lm_block_rank(on, lds_wave, before, total);
    if (!on) return;
    const uint32_t j = block_offsets[blockIdx.x] + before;   // < the grand total <= n
    const float4 a = records[2 * (size_t)i];
    round_records[2 * (size_t)j] = make_float4(a.x, a.y, a.z, __uint_as_float(lm_ad_round_word(__float_as_uint(a.w), round)));
    round_records[2 * (size_t)j + 1] = records[2 * (size_t)i + 1];
    index_of[j] = i;
}

// one thread per active record j of the round: `moments` is k_resolve_moments' pair for it
__global__ void __launch_bounds__(LP_BLOCK) k_lm_ad_merge(uint32_t n_active, const uint32_t *__restrict__ index_of, const float4 *__restrict__ moments,
                                                          uint32_t samples, LmAdaptiveDev st, const uint32_t *__restrict__ texel_of, float threshold,
                                                          uint32_t min_rounds, uint32_t max_rounds, uint8_t *__restrict__ want)
{
    const uint32_t j = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (j >= n_active) return;
    const uint32_t i = index_of[j];
    const float4 rm = moments[2 * (size_t)j], rq = moments[2 * (size_t)j + 1];
    const uint32_t n0 = st.samples[i];
    float4 m = make_float4(rm.x, rm.y, rm.z, rq.x);
    float m2 = rq.y;
    if (n0 != 0u)
    {
        const float4 m0 = st.mean[i];
        const float nA = (float)n0, nB = (float)samples;
        const float w = nB / (nA + nB);
        const float delta = rq.x - m0.w;
        m = make_float4(m0.x + (rm.x - m0.x) * w, m0.y + (rm.y - m0.y) * w, m0.z + (rm.z - m0.z) * w, m0.w + delta * w);
        m2 = (st.m2[i] + rq.y) + ((delta * delta) * nA) * w;
    }
    const uint32_t n1 = n0 + samples, r1 = st.rounds[i] + 1u;
    st.mean[i] = m;
    st.m2[i] = m2;
    st.samples[i] = n1;
    st.rounds[i] = r1;
    const float e = adaptive_pixel_error(n1, m.w, m2);
    want[texel_of[i]] = (r1 < max_rounds && (r1 < min_rounds || !(e < threshold))) ? 1u : 0u;
}

// one thread per record: the dilation of adaptive sampling's block mask (k_adaptive_mask), in atlas space
__global__ void __launch_bounds__(LP_BLOCK) k_lm_ad_mask(uint32_t n, const uint32_t *__restrict__ texel_of, uint32_t W, uint32_t H,
                                                         const uint8_t *__restrict__ want, const uint32_t *__restrict__ rounds, uint32_t max_rounds,
                                                         uint8_t *__restrict__ active)
{
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t texel = texel_of[i];
    const int32_t y = (int32_t)(texel / W), x = (int32_t)(texel - (uint32_t)y * W);
    bool open = false;
    for (int32_t dy = -1; dy <= 1; dy++)
        for (int32_t dx = -1; dx <= 1; dx++)
        {
            const int32_t nx = x + dx, ny = y + dy;
            if (nx < 0 || ny < 0 || nx >= (int32_t)W || ny >= (int32_t)H) continue;
            open = open || want[(size_t)ny * W + (uint32_t)nx] != 0u;
        }
    active[i] = (rounds[i] < max_rounds && open) ? 1u : 0u;
}

// one thread per record, after the last round: the texel of the statistics plane (cleared before), and the counts of texels
// that converged (counts[0]) and that the cap stopped (counts[1]), one atomic per wave and count
__global__ void __launch_bounds__(LP_BLOCK) k_lm_ad_stats(uint32_t n, const uint32_t *__restrict__ texel_of, LmAdaptiveDev st, float threshold,
                                                          uint32_t min_rounds, uint32_t max_rounds, float4 *__restrict__ stats,
                                                          unsigned long long *__restrict__ counts)
{
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    bool converged = false, capped = false;
    if (i < n)
    {
        const uint32_t ni = st.samples[i], ri = st.rounds[i];
        const float ml = st.mean[i].w, m2 = st.m2[i];
        const float e = adaptive_pixel_error(ni, ml, m2);
        const float nf = (float)ni;
        const float se = ni < 2u ? 0.0f : LP_PI * sqrtf(m2 / (nf * (nf - 1.0f)));
        converged = ri >= min_rounds && e < threshold;
        capped = !converged && ri >= max_rounds;
        if (stats) stats[texel_of[i]] = make_float4(nf, e, se, converged ? 1.0f : 0.0f);
    }
    const unsigned long long mc = __ballot(converged), mk = __ballot(capped);
    if ((threadIdx.x & 63u) == 0u)
    {
        if (mc) atomicAdd(&counts[0], (unsigned long long)__popcll(mc));
        if (mk) atomicAdd(&counts[1], (unsigned long long)__popcll(mk));
    }
}
