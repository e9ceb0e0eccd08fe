// lupin_lightmap_denoise.hpp -- the kernels of lupin_hip_denoise_lightmap (gfx950), included once by
// lupin_hip.hip after lupin_denoise.hpp and lupin_lightmap.hpp.
//
// An edge-avoiding a-trous filter in atlas space.  lp::denoise (lupin_denoise.hpp) filters a screen: f16 textures, an
// albedo to demodulate by, camera-space normals, and no notion of a chart.  A lightmap is f32 irradiance, and what guides
// its filter is the record plane lupin_hip_bake_lightmap writes: per owned texel the world-space surface point and the bake
// normal.  A tap counts only if it is a neighbour in space as well as in the atlas, which is what stops the filter at a
// chart border, at a gutter and at a fold.
//
//   k_lmd_prep   rgba + records -> (irradiance, 3 x 3 luminance variance over guided texels), the packed guide, the footprint
//   k_lmd_pass   one 5 x 5 B3-spline pass at tap spacing 2^i; its FINAL instantiation writes the output texel (and, when
//                gutter passes follow, the `filled` byte k_lm_dilate reads)
//   (k_lm_dilate of lupin_lightmap.hpp, unchanged, for the gutter passes)
//
// The guide of a texel is 24 bytes in two planes: (x, y, z, n.x) and (n.y, n.z); a texel that is not guided has x = NaN, so
// the distance test refuses it without a flag of its own.  A tap reads the first 16 bytes, and the other 8 and the 16 of
// (irradiance, variance) only when the distance test passes: 40 bytes for a tap that counts, 16 for one that does not.
// Every value is f32 under the library's flags (-ffp-contract=off, IEEE div / sqrt), every sum in a fixed order (dy outer,
// dx inner, -2..2); the exponential is dn_exp_neg and the luminance dn_lum of lupin_denoise.hpp, guidedness is
// ray_record_ok of lupin_rays.hpp.  tests/lightmap_denoise_ref.py restates these kernels operation for operation.
// The passes read only what the prep pass wrote and the rgba texel of their own thread, so the output may alias the input.
#pragma once

#include "lupin_denoise.hpp"
#include "lupin_lightmap.hpp"

// alpha != 0 (a NaN alpha owns its texel: it is not zero)
__device__ __forceinline__ bool lmd_owned(float alpha) { return alpha != 0.0f; }

// the texel's record is read only when the texel is owned
__device__ __forceinline__ bool lmd_guided(const float4 *__restrict__ records, uint32_t q, float alpha, float4 &pos, float4 &nrm)
{
    if (!lmd_owned(alpha)) return false;
    pos = records[2 * (size_t)q];
    nrm = records[2 * (size_t)q + 1];
    return ray_record_ok(pos.x, pos.y, pos.z, nrm.x, nrm.y, nrm.z, LP_RAY_DIRECTION);
}

// iv[p] = (c_p, var_0); guide; foot[p] = the smallest squared distance to a guided 4-neighbour (0: none).
// A texel that is not guided: (c_p, 0), x = NaN, footprint 0.
__global__ void __launch_bounds__(LP_DN_BX * LP_DN_BY) k_lmd_prep(const float4 *__restrict__ rgba, const float4 *__restrict__ records,
                                                                  float4 *__restrict__ iv, float4 *__restrict__ g0, float2 *__restrict__ g1,
                                                                  float *__restrict__ foot, uint32_t W, uint32_t H)
{
    const uint32_t x = blockIdx.x * LP_DN_BX + threadIdx.x, y = blockIdx.y * LP_DN_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const uint32_t p = y * W + x;
    const float4 cp = rgba[p];
    const float3 c = make_float3(dn_finite_or_zero(cp.x), dn_finite_or_zero(cp.y), dn_finite_or_zero(cp.z));
    float4 xp, np;
    if (!lmd_guided(records, p, cp.w, xp, np))
    {
        iv[p] = make_float4(c.x, c.y, c.z, 0.0f);
        g0[p] = make_float4(__builtin_nanf(""), 0.0f, 0.0f, 0.0f);
        g1[p] = make_float2(0.0f, 0.0f);
        foot[p] = 0.0f;
        return;
    }
    float s1 = 0.0f, s2 = 0.0f, cnt = 0.0f, f = 0.0f;
    bool has_f = false;
    for (int dy = -1; dy <= 1; dy++)
    {
        const int qy = (int)y + dy;
        if (qy < 0 || qy >= (int)H) continue;
        for (int dx = -1; dx <= 1; dx++)
        {
            const int qx = (int)x + dx;
            if (qx < 0 || qx >= (int)W) continue;
            float l;
            if (dx == 0 && dy == 0) l = dn_lum(c.x, c.y, c.z);
            else
            {
                const uint32_t q = (uint32_t)qy * W + (uint32_t)qx;
                const float4 cq = rgba[q];
                float4 xq, nq;
                if (!lmd_guided(records, q, cq.w, xq, nq)) continue;
                l = dn_lum(dn_finite_or_zero(cq.x), dn_finite_or_zero(cq.y), dn_finite_or_zero(cq.z));
                if (dx == 0 || dy == 0)   // a 4-neighbour
                {
                    const float ex = xq.x - xp.x, ey = xq.y - xp.y, ez = xq.z - xp.z;
                    const float d2 = (ex * ex + ey * ey) + ez * ez;
                    f = has_f ? fminf(f, d2) : d2;
                    has_f = true;
                }
            }
            s1 += l;
            s2 += l * l;
            cnt += 1.0f;
        }
    }
    const float mean = s1 / cnt;
    iv[p] = make_float4(c.x, c.y, c.z, fmaxf(s2 / cnt - mean * mean, 0.0f));
    g0[p] = make_float4(xp.x, xp.y, xp.z, np.x);
    g1[p] = make_float2(np.y, np.z);
    foot[p] = f;
}

// One a-trous pass over a guided texel p: taps q at k * step (k = -2..2 per axis) with h = (1,4,6,4,1)/16.  A tap counts if
// it is inside the atlas, guided, and, for q != p, |x_q - x_p|^2 <= (stretch * (kx^2 + ky^2)) * f_p, where the host hands
// in stretch = (max_stretch * max_stretch) * 4^i.
//   w = ((h_x h_y) * w_n) * exp(-(|l_p - l_q| * s_p)),  s_p = 1 / (4 sqrt(var_p) + 1e-4)
//   w_n = max(0, n_p . n_q) squared `squarings` times
// irr' = sum w c_q / sum w, var' = sum w^2 var_q / (sum w)^2.  (The centre tap always counts and its weight is not 0.)
// A texel that is not guided keeps (c_p, var_p).
// FINAL: out[p] = (irr', the input's alpha) on owned texels; on the others the input texel (GUTTER false) or zeros, and
// filled[p] = owned (GUTTER true: k_lm_dilate fills them next).  `out` may be `rgba`.
template <bool FINAL, bool GUTTER>
__global__ void __launch_bounds__(LP_DN_BX * LP_DN_BY) k_lmd_pass(const float4 *__restrict__ src, float4 *__restrict__ dst,
                                                                  const float4 *__restrict__ g0, const float2 *__restrict__ g1,
                                                                  const float *__restrict__ foot, const float4 *rgba, float4 *out,
                                                                  uint8_t *__restrict__ filled, uint32_t W, uint32_t H, int step, float stretch,
                                                                  uint32_t squarings)
{
    const uint32_t x = blockIdx.x * LP_DN_BX + threadIdx.x, y = blockIdx.y * LP_DN_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const uint32_t p = y * W + x;
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float4 cp = src[p];
    const float4 gp = g0[p];
    float4 res = cp;
    if (!__builtin_isnan(gp.x))
    {
        const float2 gp1 = g1[p];
        const float fp = foot[p];
        const float lp = dn_lum(cp.x, cp.y, cp.z);
        const float inv_sig = 1.0f / (4.0f * sqrtf(cp.w) + 1e-4f);
        float wsum = 0.0f, w2v = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
        for (int ky = 0; ky < 5; ky++)
        {
            const int qy = (int)y + (ky - 2) * step;
            if (qy < 0 || qy >= (int)H) continue;
#pragma unroll
            for (int kx = 0; kx < 5; kx++)
            {
                const int qx = (int)x + (kx - 2) * step;
                if (qx < 0 || qx >= (int)W) continue;
                const uint32_t q = (uint32_t)qy * W + (uint32_t)qx;
                const float4 gq = g0[q];
                if (kx != 2 || ky != 2)
                {
                    const float ex = gq.x - gp.x, ey = gq.y - gp.y, ez = gq.z - gp.z;
                    const float d2 = (ex * ex + ey * ey) + ez * ez;   // NaN for a tap that is not guided
                    const float limit = (stretch * (float)((kx - 2) * (kx - 2) + (ky - 2) * (ky - 2))) * fp;
                    if (!(d2 <= limit)) continue;
                }
                const float2 gq1 = g1[q];
                const float4 cq = src[q];
                float t = fmaxf((gp.w * gq.w + gp1.x * gq1.x) + gp1.y * gq1.y, 0.0f);
                for (uint32_t s = 0; s < squarings; s++) t *= t;
                const float dl = fabsf(lp - dn_lum(cq.x, cq.y, cq.z));
                const float w = ((h[kx] * h[ky]) * t) * dn_exp_neg(-(dl * inv_sig));
                wsum += w;
                sr += w * cq.x;
                sg += w * cq.y;
                sb += w * cq.z;
                w2v += (w * w) * cq.w;
            }
        }
        res = make_float4(sr / wsum, sg / wsum, sb / wsum, w2v / (wsum * wsum));
    }
    if (!FINAL)
    {
        dst[p] = res;
        return;
    }
    const float4 in = rgba[p];   // read before the write below: `out` may be `rgba`
    const bool owned = lmd_owned(in.w);
    if (owned) out[p] = make_float4(res.x, res.y, res.z, in.w);
    else out[p] = GUTTER ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : in;
    if (GUTTER) filled[p] = owned ? 1u : 0u;
}
