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
// Only an uncharted hit whose record the lookups accept asks the lookup; every other slot gets the harmless record of
// lupin_baked_view.hpp.  The order of every operation is the contract (include/lupin_hip.h), restated in
// tests/lightmapped_view_ref.py.  Whole blocks run in k_lightmapped_gbuffer (make_geo<true> has a barrier): lanes past the
// last slot trace nothing and store nothing, and there is no return before the barrier.  Neither kernel has a shuffle or a
// ballot.  Every float operation is f32 without contraction (-ffp-contract=off).
#pragma once

#include "lupin_baked_view.hpp"

constexpr uint32_t LP_LMV_MISS = 0u, LP_LMV_LIGHTMAP = 1u, LP_LMV_PROBES = 2u, LP_LMV_AMBIENT = 3u;   // LUPIN_LIGHTMAPPED_SOURCE_*
constexpr uint32_t LP_LMV_NO_CHART = 0xFFFFFFFFu;   // chart_of_instance's sentinel, and G-buffer word [18] of an uncharted pixel

struct LightmappedViewDev   // what of LupinLightmappedViewDesc and the context the kernels take
{
    BakedViewDev view;
    uint32_t width, height;   // the atlas, texels
    uint32_t volume;          // sh != NULL: an uncharted hit asks the lookup
};

// `records`, `aux` (2 float4 a slot each), `lm` (1 float4 a slot) and `gbuffer` (nullptr, or 5 float4 a slot) point at the
// launch's first slot.  chart_of_instance: per instance the lowest chart that names it, or LP_LMV_NO_CHART; charts: per
// chart (scale_u, scale_v, offset_u, offset_v).
template <bool LDSGEO>
__global__ void __launch_bounds__(LP_BLOCK) k_lightmapped_gbuffer(SceneDev sc, FrameParams fp, LightmappedViewDev v, unsigned long long first, uint32_t n,
                                                                  float eps, const uint32_t *__restrict__ chart_of_instance,
                                                                  const float4 *__restrict__ charts, float4 *__restrict__ records,
                                                                  float4 *__restrict__ aux, float4 *__restrict__ lm, float4 *__restrict__ gbuffer,
                                                                  uint32_t stack_words)
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
            if (c != LP_LMV_NO_CHART)   // (the host has seen that a charted instance's mesh has texcoords)
            {
                float tu, tv;
                interp_texcoords(sc, r.s, tu, tv);
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
__global__ void __launch_bounds__(LP_BLOCK) k_lightmapped_compose(LightmappedViewDev v, unsigned long long first, uint32_t n,
                                                                  const float4 *__restrict__ aux, const float4 *__restrict__ lm,
                                                                  const float4 *__restrict__ results, const float4 *__restrict__ atlas,
                                                                  __half *__restrict__ texels, float4 *__restrict__ gbuffer)
{
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (slot >= n) return;
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
        float *__restrict__ gw = reinterpret_cast<float *>(gbuffer + 5 * (size_t)slot);
        gw[11] = w;
        gw[19] = __uint_as_float(source);
    }
}
