// lupin_lightmap_directional.hpp -- directional lightmaps, included once by lupin_hip.hip after
// lupin_lightmap.hpp and lupin_probes.hpp.
//
// lupin_hip_bake_lightmap_directional is lupin_hip_bake_lightmap with four coefficient planes in place of one irradiance
// plane: the records are the lightmap's (lightmap_emit_records), their paths run through the radiance query's wavefront
// (k_begin_rays, the ordinary iterations), and instead of k_resolve_rays
//
//   k_resolve_lightmap_sh   one wave per record: lane l takes slots l, l + 64, ... in ascending order, derives the slot's first
//                           direction again (ray_first_direction: what k_begin_rays traced) and adds radiance * Y_j(direction)
//                           for the four L0 / L1 basis values of probe_sh_basis; an xor butterfly adds the 64 partial sums,
//                           lanes 0..3 store (sum * pi) / samples of one coefficient each
//   k_lm_sh_scatter         one thread per record: its four coefficients to the texel of the four planes, `filled` 1, the
//                           record to its place in the record plane if asked
//   k_lm_dilate             UNCHANGED, per plane (the planes share the filled bytes)
//
// Coefficient j estimates the integral of L(w) (w . n)+ Y_j(w) over the sphere: the L1 projection of the cosine-weighted
// incident radiance.  The order of every sum is part of the contract (include/lupin_hip.h) and restated in
// tests/lightmap_directional_ref.py.  Every operation is f32 without contraction (-ffp-contract=off).
#pragma once

#include "lupin_lightmap.hpp"
#include "lupin_probes.hpp"

constexpr uint32_t LP_LM_SH = 4;   // LUPIN_LIGHTMAP_DIRECTIONAL_PLANES: the first LP_LM_SH values of probe_sh_basis
constexpr uint32_t LP_LM_SH_RECORDS_PER_BLOCK = LP_BLOCK / 64;

// One wave per record of the chunk, LP_LM_SH_RECORDS_PER_BLOCK records per block; `records` points at the chunk's first
// record, out: 4 x (r, g, b, 1) per record.  Consecutive lanes read consecutive slots' `color` (num_records * samples of
// them).  The accumulators are indexed by unrolled constants only: they stay in registers.
__global__ void __launch_bounds__(LP_BLOCK) k_resolve_lightmap_sh(PathBuffers pb, uint32_t num_records, const float4 *__restrict__ records,
                                                                  uint32_t samples, float4 *__restrict__ out)
{
    const uint32_t rec = blockIdx.x * LP_LM_SH_RECORDS_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (rec >= num_records) return;   // whole waves leave: the shuffles below see 64 lanes
    const float4 a = records[2 * (size_t)rec], b = records[2 * (size_t)rec + 1];
    const size_t first = (size_t)rec * samples;
    float acc[LP_LM_SH][3];
#pragma unroll
    for (uint32_t j = 0; j < LP_LM_SH; j++)
        acc[j][0] = acc[j][1] = acc[j][2] = 0.0f;
    for (uint32_t s = lane; s < samples; s += 64u)
    {
        uint32_t rng;
        const f3 d = ray_first_direction(a, b, s, rng);
        float Y[LP_PROBE_SH];
        probe_sh_basis(d, Y);   // (only Y[0..3] are read: the band-2 values are never computed)
        const float4 L = pb.color[first + s];
#pragma unroll
        for (uint32_t j = 0; j < LP_LM_SH; j++)
        {
            acc[j][0] += L.x * Y[j];
            acc[j][1] += L.y * Y[j];
            acc[j][2] += L.z * Y[j];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (uint32_t j = 0; j < LP_LM_SH; j++)
#pragma unroll
            for (uint32_t c = 0; c < 3; c++) acc[j][c] = acc[j][c] + __shfl_xor(acc[j][c], off);
    const float count = (float)samples;
#pragma unroll
    for (uint32_t j = 0; j < LP_LM_SH; j++)
        if (lane == j)
            out[(size_t)rec * LP_LM_SH + j] = make_float4((acc[j][0] * LP_PI) / count, (acc[j][1] * LP_PI) / count, (acc[j][2] * LP_PI) / count, 1.0f);
}

// one thread per covered texel: plane j (of `texels` texels each, cleared before) gets coefficient j, `filled` 1; the record
// plane its record
__global__ void __launch_bounds__(LP_BLOCK) k_lm_sh_scatter(uint32_t n, const uint32_t *__restrict__ texel_of, const float4 *__restrict__ coef,
                                                            const float4 *__restrict__ records, uint32_t texels, float4 *__restrict__ planes,
                                                            uint8_t *__restrict__ filled, float4 *__restrict__ record_plane)
{
    const uint32_t j = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t texel = texel_of[j];
#pragma unroll
    for (uint32_t k = 0; k < LP_LM_SH; k++) planes[(size_t)k * texels + texel] = coef[LP_LM_SH * (size_t)j + k];
    filled[texel] = 1u;
    if (record_plane)
    {
        record_plane[2 * (size_t)texel] = records[2 * (size_t)j];
        record_plane[2 * (size_t)texel + 1] = records[2 * (size_t)j + 1];
    }
}
