// lupin_denoise.hpp -- the kernels of lupin_hip_denoise (gfx950), included once by lupin_hip.hip.
//
// The reference denoises with OIDN (denoising.rs:83-306), a third-party ML filter whose library and weights are not part
// of this project.  In its place: a G-buffer-guided edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) with
// SVGF-style luminance edge stopping (variance estimated spatially, not temporally) and albedo demodulation.  DESIGN.md 9
// gives the algorithm and its constants; tests/denoise_ref.py restates these kernels operation for operation in float32.
//
//   k_denoise_prep   colour / albedo / normals (f16) -> demodulated irradiance + 3x3 luminance variance, guides
//   k_denoise_iter   one 5x5 B3-spline pass at tap spacing 2^i; the last pass remodulates and stores f16 (RNE)
//
// Every value is f32 under the library's flags (-ffp-contract=off, IEEE div / sqrt), every sum in a fixed order (dy outer,
// dx inner, -2..2), so the result depends only on the inputs.  Taps outside the frame are skipped.  The kernels read
// only the scratch the prep pass wrote and the colour texel of their own pixel (alpha), so the output may alias any input.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#define LP_DN_BX 16   // 2-D blocks of 16 x 16 threads: four wave64s, each covering 16 x 4 pixels
#define LP_DN_BY 16

struct DenoiseGuide
{
    float4 n;      // normalised normal (xyz; 0 = none), w unused
    uint2 albedo;  // albedo rgb as f16 (non-finite -> 0; 0 without an albedo texture), alpha slot 0
};

// exp(x) for x <= 0 in f32 operations only: 2^k * p(r), k = rint(x log2 e), r = x - k ln2 (ln2 split in
// two, the high part exact for |k| < 128), p = degree-7 Taylor (|r| <= 0.35: relative error ~ 1e-8 before rounding);
// 0 below -80 (e^-80 ~ 2e-35: no weight).  Every step is one rounded f32 operation, so numpy reproduces it bit for bit.
// A quarter of the instructions of lpm_expf (double precision), which bounded the a-trous pass: 25 exps per pixel.
__device__ __forceinline__ float dn_exp_neg(float x)
{
    if (!(x > -80.0f)) return 0.0f;
    const float k = rintf(x * 1.44269504f);
    const float r = (x - k * 0.693145751953125f) - k * 1.42860677e-06f;
    float p = 1.0f / 5040.0f;
    p = p * r + 1.0f / 720.0f;
    p = p * r + 1.0f / 120.0f;
    p = p * r + 1.0f / 24.0f;
    p = p * r + 1.0f / 6.0f;
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    return ldexpf(p, (int)k);
}
__device__ __forceinline__ float dn_finite_or_zero(float v) { return __builtin_isfinite(v) ? v : 0.0f; }
__device__ __forceinline__ float dn_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ float dn_demod_factor(float a) { return a >= 1e-3f ? a : 1.0f; }
__device__ __forceinline__ float4 dn_load_h4(const uint2 *tex, uint32_t i)
{
    const uint2 v = tex[i];
    return make_float4(__half2float(__ushort_as_half((unsigned short)(v.x & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(v.x >> 16))),
                       __half2float(__ushort_as_half((unsigned short)(v.y & 0xFFFFu))), __half2float(__ushort_as_half((unsigned short)(v.y >> 16))));
}
__device__ __forceinline__ uint32_t dn_pack2(float a, float b)
{
    return (uint32_t)__half_as_ushort(__float2half_rn(a)) | ((uint32_t)__half_as_ushort(__float2half_rn(b)) << 16);
}

// Irradiance of pixel i: colour (non-finite components -> 0) / a' with a' = albedo >= 1e-3 ? albedo : 1 per channel.
__device__ __forceinline__ float3 dn_irradiance(const uint2 *color, const uint2 *albedo, uint32_t i, float3 *alb_out)
{
    const float4 c = dn_load_h4(color, i);
    float3 a = make_float3(0.0f, 0.0f, 0.0f);
    if (albedo)
    {
        const float4 av = dn_load_h4(albedo, i);
        a = make_float3(dn_finite_or_zero(av.x), dn_finite_or_zero(av.y), dn_finite_or_zero(av.z));
    }
    if (alb_out) *alb_out = a;
    return make_float3(dn_finite_or_zero(c.x) / dn_demod_factor(a.x), dn_finite_or_zero(c.y) / dn_demod_factor(a.y),
                       dn_finite_or_zero(c.z) / dn_demod_factor(a.z));
}

// iv[p] = (irradiance rgb, var_0) with var_0 = E[l^2] - E[l]^2 (>= 0) over the in-bounds 3x3 neighbourhood; guides.
__global__ void __launch_bounds__(LP_DN_BX * LP_DN_BY) k_denoise_prep(const uint2 *__restrict__ color, const uint2 *__restrict__ albedo,
                                                                      const uint2 *__restrict__ normals, float4 *__restrict__ iv,
                                                                      DenoiseGuide *__restrict__ guide, uint32_t W, uint32_t H)
{
    const uint32_t x = blockIdx.x * LP_DN_BX + threadIdx.x, y = blockIdx.y * LP_DN_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const uint32_t p = y * W + x;
    float3 a;
    const float3 irr = dn_irradiance(color, albedo, p, &a);
    float s1 = 0.0f, s2 = 0.0f, cnt = 0.0f;
    for (int dy = -1; dy <= 1; dy++)
    {
        const int qy = (int)y + dy;
        if (qy < 0 || qy >= (int)H) continue;
        for (int dx = -1; dx <= 1; dx++)
        {
            const int qx = (int)x + dx;
            if (qx < 0 || qx >= (int)W) continue;
            const float3 q = (dx == 0 && dy == 0) ? irr : dn_irradiance(color, albedo, (uint32_t)qy * W + (uint32_t)qx, nullptr);
            const float l = dn_lum(q.x, q.y, q.z);
            s1 += l;
            s2 += l * l;
            cnt += 1.0f;
        }
    }
    const float mean = s1 / cnt;
    const float var = fmaxf(s2 / cnt - mean * mean, 0.0f);
    iv[p] = make_float4(irr.x, irr.y, irr.z, var);

    float3 n = make_float3(0.0f, 0.0f, 0.0f);
    if (normals)
    {
        const float4 nv = dn_load_h4(normals, p);
        const float nx = dn_finite_or_zero(nv.x), ny = dn_finite_or_zero(nv.y), nz = dn_finite_or_zero(nv.z);
        const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
        if (len > 1e-6f) n = make_float3(nx / len, ny / len, nz / len);
    }
    DenoiseGuide g;
    g.n = make_float4(n.x, n.y, n.z, 0.0f);
    g.albedo = make_uint2(dn_pack2(a.x, a.y), dn_pack2(a.z, 0.0f));
    guide[p] = g;
}

// One a-trous pass: taps at k * step (k = -2..2) with h = (1,4,6,4,1)/16 per axis and
//   w = h_x h_y * w_n * exp(-(|A_p - A_q|^2 * 100 + |l_p - l_q| * s_p)),  s_p = 1 / (4 sqrt(var_p) + 1e-4)
//   w_n = max(0, n_p . n_q)^128 (seven squarings); 1 when both normals are 0
// (the albedo and luminance terms share one exp: exp(-a) exp(-b) = exp(-(a + b)); 1/0.1^2 = 100).
// irr' = sum w irr_q / sum w, var' = sum w^2 var_q / (sum w)^2.  FINAL: out = irr' * a' as f16 (RNE), alpha = colour's.
// HAS_N / HAS_A: the guide is present (without it w_n = 1 / the albedo term is 0).
template <bool FINAL, bool HAS_N, bool HAS_A>
__global__ void __launch_bounds__(LP_DN_BX * LP_DN_BY) k_denoise_iter(const float4 *__restrict__ src, float4 *__restrict__ dst,
                                                                      const DenoiseGuide *__restrict__ guide, const uint2 *color,
                                                                      uint2 *out, uint32_t W, uint32_t H, int step)
{
    const uint32_t x = blockIdx.x * LP_DN_BX + threadIdx.x, y = blockIdx.y * LP_DN_BY + threadIdx.y;
    if (x >= W || y >= H) return;
    const uint32_t p = y * W + x;
    const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const float4 cp = src[p];
    const float lp = dn_lum(cp.x, cp.y, cp.z);
    const float inv_sig = 1.0f / (4.0f * sqrtf(cp.w) + 1e-4f);
    float4 np = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    float4 ap = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (HAS_N) np = guide[p].n;
    if (HAS_A || FINAL) ap = dn_load_h4(&guide[p].albedo, 0);
    const bool np_zero = np.x == 0.0f && np.y == 0.0f && np.z == 0.0f;
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
            const float4 cq = src[q];
            float wn = 1.0f;
            if (HAS_N)
            {
                const float4 nq = guide[q].n;
                const bool nq_zero = nq.x == 0.0f && nq.y == 0.0f && nq.z == 0.0f;
                if (!(np_zero && nq_zero))
                {
                    float t = fmaxf((np.x * nq.x + np.y * nq.y) + np.z * nq.z, 0.0f);
                    t *= t; t *= t; t *= t; t *= t; t *= t; t *= t; t *= t;
                    wn = t;
                }
            }
            float da2 = 0.0f;
            if (HAS_A)
            {
                const float4 aq = dn_load_h4(&guide[q].albedo, 0);
                const float dr = ap.x - aq.x, dg = ap.y - aq.y, db = ap.z - aq.z;
                da2 = (dr * dr + dg * dg) + db * db;
            }
            const float dl = fabsf(lp - dn_lum(cq.x, cq.y, cq.z));
            const float w = ((h[kx] * h[ky]) * wn) * dn_exp_neg(-(da2 * 100.0f + dl * inv_sig));
            wsum += w;
            sr += w * cq.x;
            sg += w * cq.y;
            sb += w * cq.z;
            w2v += (w * w) * cq.w;
        }
    }
    const float r = sr / wsum, g = sg / wsum, b = sb / wsum;
    if (!FINAL)
    {
        dst[p] = make_float4(r, g, b, w2v / (wsum * wsum));
        return;
    }
    const uint2 c = color[p];   // read before the write below: `out` may be `color`
    out[p] = make_uint2(dn_pack2(r * dn_demod_factor(ap.x), g * dn_demod_factor(ap.y)),
                        (uint32_t)__half_as_ushort(__float2half_rn(b * dn_demod_factor(ap.z))) | (c.y & 0xFFFF0000u));
}
