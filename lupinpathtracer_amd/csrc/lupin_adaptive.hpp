// lupin_adaptive.hpp -- adaptive sampling, included once by lupin_hip.hip after lupin_stages.hpp.
//
// Per-pixel state: frames taken since the reset n_p (u32) and f32 Welford moments (mean_p, M2_p) of the frame
// luminance; per 8x8 block: the error E_b, a flags byte, the active byte and (sum, max) of n_p.  One call of
// lupin_hip_pathtrace_scene_adaptive runs
//
//   k_begin_adaptive     k_begin (begin_paths<true>): only pixels of active blocks start a path; seed with base + n_p
//   (the ordinary iterations: inactive pixels were never queued, so they cost nothing)
//   k_resolve_adaptive   active pixels: k_resolve's blend with counter base + n_p, then n_p += 1 and the moments
//                        inactive pixels: prev's texel (and f32 accumulator) copied bit for bit
//   k_adaptive_update    one wave64 per block, lane = pixel: e_p, E_b = max, min / max / sum of n_p -> flags, counts
//   k_adaptive_mask      one thread per block: active = (itself or a neighbour not converged) and not capped; the
//                        statistics, one atomic per wave of 64 blocks (one per block wave would serialise ~130 k
//                        same-address atomics at 4K: 3 ms measured)
//
// Every operation is f32 without contraction (the Makefile builds with -ffp-contract=off), so tests/adaptive_ref.py
// restates the rule exactly.
#pragma once

#include "lupin_stages.hpp"

constexpr uint32_t LP_AD_BLOCK = 8;            // block edge in pixels: one block = one wave64
constexpr uint8_t LP_AD_CONVERGED = 1u;        // block_flags bit: E_b < threshold and every n_p >= min_frames
constexpr uint8_t LP_AD_CAPPED = 2u;           // block_flags bit: every n_p >= max_frames (max_frames > 0)
constexpr float LP_AD_MEAN_FLOOR = 1e-3f;      // absolute floor of the relative error's denominator

struct AdaptiveDev
{
    uint32_t *frames;              // n_p, W*H
    float2 *moments;               // (mean_p, M2_p), W*H
    float *block_error;            // E_b (+inf: no estimate yet)
    uint8_t *block_flags;          // LP_AD_CONVERGED | LP_AD_CAPPED
    uint8_t *block_active;         // 1: the next call renders the block
    uint2 *block_count;            // (sum, max) of n_p over the block's in-image pixels, for the statistics
    unsigned long long *stats;     // [0] in-image pixels of active blocks, [1] sum of n_p, [2] max n_p
    uint32_t width, height, blocks_x, blocks_y;
    float threshold;
    uint32_t min_frames, max_frames;
};

__device__ __forceinline__ float adaptive_luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// e_p: relative standard error of the mean with an absolute floor; +inf while there is no estimate
__device__ __forceinline__ float adaptive_pixel_error(uint32_t n, float mean, float m2)
{
    if (n < 2u || !__builtin_isfinite(mean) || !__builtin_isfinite(m2)) return __builtin_inff();
    const float nf = (float)n;
    return sqrtf(m2 / (nf * (nf - 1.0f))) / (mean + LP_AD_MEAN_FLOOR);
}

__global__ void __launch_bounds__(LP_BLOCK) k_begin_adaptive(const FrameParams *__restrict__ fpp, PathBuffers pb, uint32_t n,
                                                             const uint8_t *__restrict__ block_active, const uint32_t *__restrict__ frames,
                                                             uint32_t blocks_x)
{
    begin_paths<true>(fpp, pb, n, block_active, frames, blocks_x);
}

// k_resolve for one frame (count == 1) with a per-pixel counter; the blend is k_resolve's, expression for expression
__global__ void __launch_bounds__(LP_BLOCK) k_resolve_adaptive(FrameParams fp, PathBuffers pb, uint32_t n, AdaptiveDev ad, __half *target,
                                                               const __half *prev, const float4 *prev32, float4 *out32)
{
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (slot >= n) return;
    uint32_t gx, gy;
    slot_to_pixel(fp, slot, gx, gy);
    if (gx >= fp.width || gy >= fp.height) return;
    const size_t px = (size_t)gy * fp.width + gx;
    if (!ad.block_active[(gy >> 3) * ad.blocks_x + (gx >> 3)])
    {
        // the pixel took no frame: the target keeps what prev holds, bit for bit
        const uint2 w = reinterpret_cast<const uint2 *>(prev)[px];
        reinterpret_cast<uint2 *>(target)[px] = w;
        if (out32)
            out32[px] = prev32 ? prev32[px]
                               : make_float4(half_bits_to_float(w.x & 0xFFFFu), half_bits_to_float(w.x >> 16),
                                             half_bits_to_float(w.y & 0xFFFFu), half_bits_to_float(w.y >> 16));
        return;
    }
    const float spp = (float)fp.spp;
    const bool rne = fp.store_rne != 0;
    const uint32_t taken = ad.frames[px];
    const uint32_t counter = fp.pc.accum_counter + taken;
    const float4 c4 = pb.color[slot];
    const f3 v = mk3(maxf(c4.x / spp, 0.0f), maxf(c4.y / spp, 0.0f), maxf(c4.z / spp, 0.0f));   // this frame's value
    f3 c = v;
    if (counter != 0)
    {
        const float w = 1.0f / (float)counter;
        f3 pc;
        if (prev32) { const float4 p = prev32[px]; pc = mk3(p.x, p.y, p.z); }
        else pc = load_rgb16f(prev, px);
        c = mk3(maxf(pc.x * (1.0f - w) + c.x * w, 0.0f), maxf(pc.y * (1.0f - w) + c.y * w, 0.0f), maxf(pc.z * (1.0f - w) + c.z * w, 0.0f));
    }
    if (out32) out32[px] = make_float4(c.x, c.y, c.z, 1.0f);
    store_rgba16f(target, px, c, rne);
    // Welford over the frame values' luminance
    const float l = adaptive_luminance(v.x, v.y, v.z);
    float2 m = ad.moments[px];
    const uint32_t n1 = taken + 1u;
    const float d = l - m.x;
    m.x = m.x + d / (float)n1;
    m.y = m.y + d * (l - m.x);
    ad.moments[px] = m;
    ad.frames[px] = n1;
}

// One wave64 per 8x8 block (four blocks per workgroup), lane = pixel (lane & 7, lane >> 3).  Lanes outside the image
// contribute the neutral element of every reduction.
__global__ void __launch_bounds__(LP_BLOCK) k_adaptive_update(AdaptiveDev ad)
{
    const uint32_t b = blockIdx.x * (LP_BLOCK / 64u) + (threadIdx.x >> 6);
    if (b >= ad.blocks_x * ad.blocks_y) return;   // whole waves leave together
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gx = (b % ad.blocks_x) * LP_AD_BLOCK + (lane & 7u), gy = (b / ad.blocks_x) * LP_AD_BLOCK + (lane >> 3);
    float e = -__builtin_inff();
    uint32_t nmin = 0xFFFFFFFFu, nmax = 0u, nsum = 0u;
    if (gx < ad.width && gy < ad.height)
    {
        const size_t px = (size_t)gy * ad.width + gx;
        const uint32_t nf = ad.frames[px];
        const float2 m = ad.moments[px];
        e = adaptive_pixel_error(nf, m.x, m.y);
        nmin = nmax = nsum = nf;
    }
    for (int off = 32; off > 0; off >>= 1)
    {
        e = fmaxf(e, __shfl_xor(e, off));
        nmin = min(nmin, (uint32_t)__shfl_xor((int)nmin, off));
        nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, off));
        nsum += (uint32_t)__shfl_xor((int)nsum, off);   // 64 counts below 2^26 each: no overflow
    }
    if (lane == 0)
    {
        // lane 0's pixel is always inside the image, so e is a pixel's error
        const bool converged = e < ad.threshold && nmin >= ad.min_frames;
        const bool capped = ad.max_frames != 0u && nmin >= ad.max_frames;
        ad.block_error[b] = e;
        ad.block_flags[b] = (converged ? LP_AD_CONVERGED : 0u) | (capped ? LP_AD_CAPPED : 0u);
        ad.block_count[b] = make_uint2(nsum, nmax);
    }
}

// After k_adaptive_update (same stream): a block is active when it or one of its 8 neighbours has not converged, and
// it is not capped.  One thread per block; one atomic per wave and statistic.
__global__ void __launch_bounds__(LP_BLOCK) k_adaptive_mask(AdaptiveDev ad)
{
    const uint32_t b = blockIdx.x * LP_BLOCK + threadIdx.x;
    uint32_t px_active = 0u, nmax = 0u;
    unsigned long long nsum = 0ull;
    if (b < ad.blocks_x * ad.blocks_y)
    {
        const uint2 cnt = ad.block_count[b];
        nsum = cnt.x;
        nmax = cnt.y;
        const int bx = (int)(b % ad.blocks_x), by = (int)(b / ad.blocks_x);
        bool open = false;
        for (int dy = -1; dy <= 1; dy++)
            for (int dx = -1; dx <= 1; dx++)
            {
                const int x = bx + dx, y = by + dy;
                if (x >= 0 && y >= 0 && x < (int)ad.blocks_x && y < (int)ad.blocks_y)
                    open = open || (ad.block_flags[(uint32_t)y * ad.blocks_x + (uint32_t)x] & LP_AD_CONVERGED) == 0u;
            }
        const bool active = open && (ad.block_flags[b] & LP_AD_CAPPED) == 0u;
        ad.block_active[b] = active ? 1u : 0u;
        if (active)
            px_active = min(LP_AD_BLOCK, ad.width - (uint32_t)bx * LP_AD_BLOCK) * min(LP_AD_BLOCK, ad.height - (uint32_t)by * LP_AD_BLOCK);
    }
    for (int off = 32; off > 0; off >>= 1)
    {
        px_active += (uint32_t)__shfl_xor((int)px_active, off);
        nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, off));
        nsum += (unsigned long long)__shfl_xor((long long)nsum, off);
    }
    if ((threadIdx.x & 63u) == 0u)
    {
        if (px_active) atomicAdd(&ad.stats[0], (unsigned long long)px_active);
        if (nsum) atomicAdd(&ad.stats[1], nsum);
        if (nmax) atomicMax(&ad.stats[2], (unsigned long long)nmax);
    }
}

// lupin_hip_adaptive_reset: counts and moments 0, every block active with no error estimate
__global__ void __launch_bounds__(LP_BLOCK) k_adaptive_reset(AdaptiveDev ad)
{
    const size_t i = (size_t)blockIdx.x * LP_BLOCK + threadIdx.x;
    const size_t pixels = (size_t)ad.width * ad.height;
    if (i < pixels)
    {
        ad.frames[i] = 0u;
        ad.moments[i] = make_float2(0.0f, 0.0f);
    }
    if (i < (size_t)ad.blocks_x * ad.blocks_y)
    {
        ad.block_error[i] = __builtin_inff();
        ad.block_flags[i] = 0u;
        ad.block_active[i] = 1u;
        ad.block_count[i] = make_uint2(0u, 0u);
    }
    if (i == 0)
    {
        ad.stats[0] = (unsigned long long)pixels;
        ad.stats[1] = 0ull;
        ad.stats[2] = 0ull;
    }
}
