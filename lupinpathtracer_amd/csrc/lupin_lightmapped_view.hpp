// lupin_lightmapped_view.hpp -- lightmapped view, included once by lupin_hip.hip after lupin_baked_view.hpp.
//
// lupin_hip_render_lightmapped draws a camera view of baked lighting: one primary hit per pixel, then
// emission + albedo / pi * E, with E fetched from a lightmap atlas where the hit instance has a chart and from an irradiance
// volume (or `ambient`) where it has none.  A launch of at most max_slots pixels runs two or three kernels:
//
//   k_lightmapped_gbuffer<LDSGEO>   ONE LANE PER PIXEL.  baked_primary (lupin_baked_view.hpp: the body k_baked_gbuffer runs),
//                          then the chart of the hit instance from chart_of_instance, interp_texcoords and the atlas
//                          coordinate.  It writes, per slot, the lookup's record (8 words), the compose record (8 words, as
//                          k_baked_gbuffer's), the lightmap record (x, y | chart | source) and, where asked, the G-buffer's
//                          20 words.
//   k_probe_grid / k_probe_grid_depth   UNCHANGED, over the records; launched only with a volume.
//   k_lightmapped_compose  one lane per pixel: the ownership-aware bilinear fetch (four float4 loads), or the lookup's answer,
//                          or ambient; the shading, the f16 store, and G-buffer words [11] and [19].
//
// lupin_hip_render_lightmapped_directional runs k_lightmapped_gbuffer_directional and
// k_lightmapped_compose_directional: the first also writes, per LIGHTMAP slot, the turned shading normal n', the bake normal
// n_b (lm_bake_normal: the record emitter's own function) and the back-face bit; the second, a template variant of the compose
// body, fetches the four coefficient planes by the scalar fetch's taps and scales E by max(num, 0) / den.  The kernels of
// lupin_hip_render_lightmapped are instruction for instruction what they were.
//
// Only an uncharted hit whose record the lookups accept asks the lookup; every other slot gets the harmless record of
// lupin_baked_view.hpp.  The order of every operation is the contract (include/lupin_hip.h), restated in
// tests/lightmapped_view_ref.py.  Whole blocks run in k_lightmapped_gbuffer (make_geo<true> has a barrier): lanes past the
// last slot trace nothing and store nothing, and there is no return before the barrier.  Neither kernel has a shuffle or a
// ballot.  Every float operation is f32 without contraction (-ffp-contract=off).
#pragma once

#include "lupin_baked_view.hpp"
#include "lupin_lightmap.hpp"

constexpr uint32_t LP_LMV_MISS = 0u, LP_LMV_LIGHTMAP = 1u, LP_LMV_PROBES = 2u, LP_LMV_AMBIENT = 3u;   // LUPIN_LIGHTMAPPED_SOURCE_*
constexpr uint32_t LP_LMV_NO_CHART = 0xFFFFFFFFu;   // chart_of_instance's sentinel, and G-buffer word [18] of an uncharted pixel
// G-buffer word [23] of lupin_hip_render_lightmapped_directional (LUPIN_LIGHTMAPPED_DIRECTIONAL_*)
constexpr uint32_t LP_LMV_DIR_APPLIED = 1u, LP_LMV_DIR_BACK_FACE = 2u, LP_LMV_DIR_DEN_NOT_POSITIVE = 4u, LP_LMV_DIR_NOT_FINITE = 8u;

struct LightmappedViewDev   // what of LupinLightmappedViewDesc and the context the kernels take
{
    BakedViewDev view;
    uint32_t width, height;   // the atlas, texels
    uint32_t volume;          // sh != NULL: an uncharted hit asks the lookup
};

// The coordinate a chart places in the atlas: interp_texcoords on the mesh's texcoords, or, where the hit instance's mesh has
// a lightmap UV set (lm_uvs != nullptr: one float2 per triangle corner, the mesh's first corner first), the same weighted
// sum over the hit triangle's three corners of that set.
LP_DEV void lmv_atlas_uv(const SceneDev &sc, const Surface &s, const float2 *__restrict__ lm_uvs, float &tu, float &tv)
{
    if (!lm_uvs) { interp_texcoords(sc, s, tu, tv); return; }
    const size_t corner = (size_t)(s.gtri - s.mesh.tri_offset) * 3;
    const float2 a = lm_uvs[corner], b = lm_uvs[corner + 1], c = lm_uvs[corner + 2];
    const float w = 1.0f - s.u - s.v;
    tu = a.x * w + b.x * s.u + c.x * s.v;
    tv = a.y * w + b.y * s.u + c.y * s.v;
}

// `records`, `aux` (2 float4 a slot each), `lm` (1 float4 a slot) and `gbuffer` (nullptr, or 5 float4 a slot) point at the
// launch's first slot.  chart_of_instance: per instance the lowest chart that names it, or LP_LMV_NO_CHART; charts: per
// chart (scale_u, scale_v, offset_u, offset_v); chart_lm_uvs: per chart the lightmap UV set of its instance's mesh, or nullptr.
template <bool LDSGEO>
__global__ void __launch_bounds__(LP_BLOCK) k_lightmapped_gbuffer(SceneDev sc, FrameParams fp, LightmappedViewDev v, unsigned long long first, uint32_t n,
                                                                  float eps, const uint32_t *__restrict__ chart_of_instance,
                                                                  const float4 *__restrict__ charts, float4 *__restrict__ records,
                                                                  float4 *__restrict__ aux, float4 *__restrict__ lm, float4 *__restrict__ gbuffer,
                                                                  uint32_t stack_words, const float2 *const *__restrict__ chart_lm_uvs)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const auto geo = make_geo<LDSGEO>(sc, lds_stack, stack_words);
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (slot < n)   // (every lane of the block has passed the barrier)
    {
        const BakedPrimary r = baked_primary(geo, sc, fp, lds_stack, first + slot, eps);
        float x = 0.0f, y = 0.0f;
        uint32_t chart = LP_LMV_NO_CHART, source = LP_LMV_MISS;
        if (r.hit)
        {
            const uint32_t c = chart_of_instance[r.inst];
            if (c != LP_LMV_NO_CHART)   // (the host has seen that a charted instance's mesh has texcoords or a lightmap UV set)
            {
                float tu, tv;
                lmv_atlas_uv(sc, r.s, chart_lm_uvs[c], tu, tv);
                const float4 k = charts[c];
                const float au = tu * k.x + k.z, av = tv * k.y + k.w;
                const float cx = au * (float)v.width - 0.5f, cy = av * (float)v.height - 0.5f;
                if (isfinite(cx) && isfinite(cy)) { x = cx; y = cy; chart = c; source = LP_LMV_LIGHTMAP; }
            }
            if (source != LP_LMV_LIGHTMAP) source = (v.volume != 0u && r.state == LP_BAKED_LOOKUP) ? LP_LMV_PROBES : LP_LMV_AMBIENT;
        }
        baked_store_record(r, source == LP_LMV_PROBES, records, slot);
        aux[2 * (size_t)slot] = make_float4(r.color.x, r.color.y, r.color.z, __uint_as_float(r.state));
        aux[2 * (size_t)slot + 1] = make_float4(r.glow.x, r.glow.y, r.glow.z, r.dst);
        const float4 rec = make_float4(x, y, __uint_as_float(chart), __uint_as_float(source));
        lm[slot] = rec;
        if (gbuffer)
        {
            float4 *__restrict__ g = gbuffer + 5 * (size_t)slot;
            baked_store_gbuffer(r, g);
            g[4] = rec;   // [19] is k_lightmapped_compose's to settle: PROBES becomes AMBIENT where the lookup answers w == 0
        }
    }
}

// lupin_hip_render_lightmapped_directional's k_lightmapped_gbuffer.  It has a body of its own, the one above statement for
// statement plus what is marked DIRECTIONAL: routing both kernels through one templated body moved instructions in the kernel
// above, and that kernel's code is to stay what it was.  The G-buffer has 6 float4 a slot, and `dir` (2 float4
// a slot) takes what the ratio needs of a LIGHTMAP pixel, (n' | back-face bit) (n_b | 0), and zeros of every other pixel.
template <bool LDSGEO>
__global__ void __launch_bounds__(LP_BLOCK) k_lightmapped_gbuffer_directional(SceneDev sc, FrameParams fp, LightmappedViewDev v, unsigned long long first,
                                                                              uint32_t n, float eps, const uint32_t *__restrict__ chart_of_instance,
                                                                              const float4 *__restrict__ charts, float4 *__restrict__ records,
                                                                              float4 *__restrict__ aux, float4 *__restrict__ lm,
                                                                              float4 *__restrict__ gbuffer, uint32_t stack_words, uint32_t bake_flags,
                                                                              float4 *__restrict__ dir, const float2 *const *__restrict__ chart_lm_uvs)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const auto geo = make_geo<LDSGEO>(sc, lds_stack, stack_words);
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (slot < n)   // (every lane of the block has passed the barrier)
    {
        const BakedPrimary r = baked_primary(geo, sc, fp, lds_stack, first + slot, eps);
        float x = 0.0f, y = 0.0f;
        uint32_t chart = LP_LMV_NO_CHART, source = LP_LMV_MISS;
        if (r.hit)
        {
            const uint32_t c = chart_of_instance[r.inst];
            if (c != LP_LMV_NO_CHART)
            {
                float tu, tv;
                lmv_atlas_uv(sc, r.s, chart_lm_uvs[c], tu, tv);
                const float4 k = charts[c];
                const float au = tu * k.x + k.z, av = tv * k.y + k.w;
                const float cx = au * (float)v.width - 0.5f, cy = av * (float)v.height - 0.5f;
                if (isfinite(cx) && isfinite(cy)) { x = cx; y = cy; chart = c; source = LP_LMV_LIGHTMAP; }
            }
            if (source != LP_LMV_LIGHTMAP) source = (v.volume != 0u && r.state == LP_BAKED_LOOKUP) ? LP_LMV_PROBES : LP_LMV_AMBIENT;
        }
        baked_store_record(r, source == LP_LMV_PROBES, records, slot);
        aux[2 * (size_t)slot] = make_float4(r.color.x, r.color.y, r.color.z, __uint_as_float(r.state));
        aux[2 * (size_t)slot + 1] = make_float4(r.glow.x, r.glow.y, r.glow.z, r.dst);
        const float4 rec = make_float4(x, y, __uint_as_float(chart), __uint_as_float(source));
        lm[slot] = rec;
        if (gbuffer)
        {
            float4 *__restrict__ g = gbuffer + 6 * (size_t)slot;   // DIRECTIONAL: 24 words; [20..23] are the compose kernel's
            baked_store_gbuffer(r, g);
            g[4] = rec;
        }
        // DIRECTIONAL: the ratio's record
        float4 d0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), d1 = d0;
        if (source == LP_LMV_LIGHTMAP)
        {
            f3 ng;
            const f3 nb = lm_bake_normal(geo, sc, r.s.in, r.s.mesh, r.s.gtri, r.s.i0, r.s.i1, r.s.i2, r.s.u, r.s.v, bake_flags, ng);
            f3 o, d;
            baked_primary_ray(fp, first + slot, o, d);   // (BakedPrimary does not carry the ray: the same function gives it again)
            const bool back = ((d.x * ng.x + d.y * ng.y) + d.z * ng.z) > 0.0f;
            d0 = make_float4(r.nrm.x, r.nrm.y, r.nrm.z, __uint_as_float(back ? 1u : 0u));
            d1 = make_float4(nb.x, nb.y, nb.z, 0.0f);
        }
        dir[2 * (size_t)slot] = d0;
        dir[2 * (size_t)slot + 1] = d1;
    }
}

// One clamped axis of the fetch: the two texels and the weight of the second.
LP_DEV void lmv_axis(float x, uint32_t size, uint32_t &i0, uint32_t &i1, float &f)
{
    const float xf = fminf(fmaxf(x, 0.0f), (float)(size - 1u));   // clamped in float before any conversion to integer
    const float fl = floorf(xf);
    i0 = (uint32_t)fl;
    i1 = min(i0 + 1u, size - 1u);
    f = xf - fl;
}

// `aux`, `lm`, `results` (the lookup's, one float4 a slot; not read without a volume) and `gbuffer` point at the launch's first
// slot; `atlas` at the lightmap's first texel, `texels` at the image's (4 halves each).
// DIRECTIONAL: `directional` points at the first texel of the first of the four coefficient planes, `dir` at the launch's
// first slot (k_lightmapped_gbuffer_directional's), and the G-buffer has 6 float4 a slot.
template <bool DIRECTIONAL>
LP_DEV void lightmapped_compose(const LightmappedViewDev &v, unsigned long long first, uint32_t n, const float4 *__restrict__ aux,
                                const float4 *__restrict__ lm, const float4 *__restrict__ results, const float4 *__restrict__ atlas,
                                __half *__restrict__ texels, float4 *__restrict__ gbuffer, const float4 *__restrict__ directional,
                                const float4 *__restrict__ dir)
{
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (slot >= n) return;
    float ratio[3] = {1.0f, 1.0f, 1.0f};
    uint32_t ratio_bits = 0u;
    const float4 a = aux[2 * (size_t)slot], b = aux[2 * (size_t)slot + 1], l = lm[slot];
    uint32_t source = __float_as_uint(l.w);
    float r = b.x, g = b.y, bl = b.z, w = 0.0f;
    if (source != LP_LMV_MISS)
    {
        float er = v.view.ar, eg = v.view.ag, eb = v.view.ab;
        if (source == LP_LMV_LIGHTMAP)
        {
            uint32_t x0, x1, y0, y1;
            float fx, fy;
            lmv_axis(l.x, v.width, x0, x1, fx);
            lmv_axis(l.y, v.height, y0, y1, fy);
            const float gx = 1.0f - fx, gy = 1.0f - fy;
            const float wt[4] = {gx * gy, fx * gy, gx * fy, fx * fy};   // taps 00, 10, 01, 11
            const size_t row0 = (size_t)y0 * v.width, row1 = (size_t)y1 * v.width;
            const float4 t[4] = {atlas[row0 + x0], atlas[row0 + x1], atlas[row1 + x0], atlas[row1 + x1]};
            float cov = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, pr = 0.0f, pg = 0.0f, pb = 0.0f;
#pragma unroll
            for (int k = 0; k < 4; k++)
            {
                const float cr = wt[k] * t[k].x, cg = wt[k] * t[k].y, cb = wt[k] * t[k].z;
                pr = pr + cr; pg = pg + cg; pb = pb + cb;   // the plain sum, over all four
                if (t[k].w != 0.0f) { cov = cov + wt[k]; sr = sr + cr; sg = sg + cg; sb = sb + cb; }   // an OWNED tap
            }
            if (cov > 0.0f) { er = sr / cov; eg = sg / cov; eb = sb / cov; }
            else { er = pr; eg = pg; eb = pb; }
            w = cov;
            if constexpr (DIRECTIONAL)
            {
                // C0..C3 by the same taps, weights, ownership (the scalar lightmap's alpha) and branch
                const size_t plane = (size_t)v.width * v.height;
                float C[4][3];
#pragma unroll
                for (int j = 0; j < 4; j++)
                {
                    const float4 *__restrict__ p = directional + (size_t)j * plane;
                    const float4 q[4] = {p[row0 + x0], p[row0 + x1], p[row1 + x0], p[row1 + x1]};
                    float s3[3] = {0.0f, 0.0f, 0.0f}, p3[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int k = 0; k < 4; k++)
                    {
                        const float cr = wt[k] * q[k].x, cg = wt[k] * q[k].y, cb = wt[k] * q[k].z;
                        p3[0] = p3[0] + cr; p3[1] = p3[1] + cg; p3[2] = p3[2] + cb;
                        if (t[k].w != 0.0f) { s3[0] = s3[0] + cr; s3[1] = s3[1] + cg; s3[2] = s3[2] + cb; }
                    }
#pragma unroll
                    for (int c = 0; c < 3; c++) C[j][c] = cov > 0.0f ? s3[c] / cov : p3[c];
                }
                const float4 d0 = dir[2 * (size_t)slot], d1 = dir[2 * (size_t)slot + 1];
                float Yn[LP_PROBE_SH], Yb[LP_PROBE_SH];   // (only [0..3] are read)
                probe_sh_basis(mk3(d0.x, d0.y, d0.z), Yn);
                probe_sh_basis(mk3(d1.x, d1.y, d1.z), Yb);
                const bool back = __float_as_uint(d0.w) != 0u;
                if (back) ratio_bits |= LP_LMV_DIR_BACK_FACE;
#pragma unroll
                for (int c = 0; c < 3; c++)
                {
                    const float num = ((C[0][c] * Yn[0] + C[1][c] * Yn[1]) + C[2][c] * Yn[2]) + C[3][c] * Yn[3];
                    const float den = ((C[0][c] * Yb[0] + C[1][c] * Yb[1]) + C[2][c] * Yb[2]) + C[3][c] * Yb[3];
                    if (back) continue;
                    const bool finite = isfinite(num) && isfinite(den);
                    if (den <= 0.0f) ratio_bits |= LP_LMV_DIR_DEN_NOT_POSITIVE;
                    if (!finite) ratio_bits |= LP_LMV_DIR_NOT_FINITE;
                    if (finite && !(den <= 0.0f))
                    {
                        ratio[c] = (num > 0.0f ? num : 0.0f) / den;
                        ratio_bits |= LP_LMV_DIR_APPLIED;
                    }
                }
                er = er * ratio[0]; eg = eg * ratio[1]; eb = eb * ratio[2];
            }
        }
        else if (source == LP_LMV_PROBES)
        {
            const float4 e = results[slot];
            w = e.w;
            if (!(e.w == 0.0f)) { er = e.x; eg = e.y; eb = e.z; }
            else source = LP_LMV_AMBIENT;
        }
        r = b.x + (a.x * er) * LP_BAKED_INV_PI;
        g = b.y + (a.y * eg) * LP_BAKED_INV_PI;
        bl = b.z + (a.z * eb) * LP_BAKED_INV_PI;
    }
    store_rgba16f(texels, (size_t)(first + slot), mk3(r, g, bl), v.view.store_rne != 0u);
    if (gbuffer)
    {
        float *__restrict__ gw = reinterpret_cast<float *>(gbuffer + (DIRECTIONAL ? 6u : 5u) * (size_t)slot);
        gw[11] = w;
        gw[19] = __uint_as_float(source);
        if constexpr (DIRECTIONAL)
        {
            gw[20] = ratio[0]; gw[21] = ratio[1]; gw[22] = ratio[2];
            gw[23] = __uint_as_float(ratio_bits);
        }
    }
}

__global__ void __launch_bounds__(LP_BLOCK) k_lightmapped_compose(LightmappedViewDev v, unsigned long long first, uint32_t n,
                                                                  const float4 *__restrict__ aux, const float4 *__restrict__ lm,
                                                                  const float4 *__restrict__ results, const float4 *__restrict__ atlas,
                                                                  __half *__restrict__ texels, float4 *__restrict__ gbuffer)
{
    lightmapped_compose<false>(v, first, n, aux, lm, results, atlas, texels, gbuffer, nullptr, nullptr);
}

__global__ void __launch_bounds__(LP_BLOCK) k_lightmapped_compose_directional(LightmappedViewDev v, unsigned long long first, uint32_t n,
                                                                              const float4 *__restrict__ aux, const float4 *__restrict__ lm,
                                                                              const float4 *__restrict__ results, const float4 *__restrict__ atlas,
                                                                              __half *__restrict__ texels, float4 *__restrict__ gbuffer,
                                                                              const float4 *__restrict__ directional, const float4 *__restrict__ dir)
{
    lightmapped_compose<true>(v, first, n, aux, lm, results, atlas, texels, gbuffer, directional, dir);
}
