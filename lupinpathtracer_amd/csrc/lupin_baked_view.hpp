// lupin_baked_view.hpp -- baked-lighting view, included once by lupin_hip.hip after lupin_probe_depth.hpp.
//
// lupin_hip_render_baked draws a camera view of a baked irradiance volume: one primary hit per pixel, then
// emission + albedo / pi * E(p, n) with E from the volume.  A launch of at most max_slots pixels runs three kernels:
//
//   k_baked_gbuffer<LDSGEO>   ONE LANE PER PIXEL.  camera_ray_centre, scene_closest, and at a hit the shading normal (turned
//                          to the viewer's side) and material_point<false>; at a miss environment_radiance.  It writes, per
//                          slot, the lookup's record (8 words), what the compose kernel needs (8 words: color | state,
//                          emission or environment | dst) and, where the caller asked for one, the G-buffer's 16 words.
//   k_probe_grid / k_probe_grid_depth   UNCHANGED, over the records.
//   k_baked_compose        one lane per pixel: ambient where the lookup was not asked or answered w == 0, step 6, the f16
//                          store, and G-buffer word [11].
//
// The record of a pixel whose lookup is not asked (a miss; a hit whose p or n the lookups would refuse) is a harmless one,
// (0, 0, 0 | instance) (0, 0, 1 | tri): the lookup kernels run over whole launches and its result for that slot is not read.
// The order of every operation is the contract (include/lupin_hip.h) and restated in tests/baked_view_ref.py.
// Whole blocks run in k_baked_gbuffer (make_geo<true> has a barrier): lanes past the last slot trace nothing and store
// nothing, and there is no return before the barrier.  Neither kernel has a shuffle or a ballot.
// Every float operation is f32 without contraction (-ffp-contract=off).
#pragma once

#include "lupin_probe_depth.hpp"

constexpr uint32_t LP_BAKED_VIEW_DEVICE_POINTERS = 1u;   // LUPIN_BAKED_VIEW_DEVICE_POINTERS
constexpr uint32_t LP_BAKED_MISS = 0u, LP_BAKED_LOOKUP = 1u, LP_BAKED_NO_LOOKUP = 2u;   // a slot's state, word 3 of its compose record
constexpr float LP_BAKED_INV_PI = 0.31830988f;           // the literal of include/lupin_hip.h

struct BakedViewDev   // what of LupinBakedViewDesc and the context the compose kernel takes
{
    float ar, ag, ab;     // ambient
    uint32_t store_rne;   // FrameParams::store_rne
};

// `records` (2 float4 a slot), `aux` (2 float4 a slot) and `gbuffer` (nullptr, or 4 float4 a slot) point at the launch's first
// slot; first = the launch's first pixel (y * W + x), n = the launch's slots.
template <bool LDSGEO>
__global__ void __launch_bounds__(LP_BLOCK) k_baked_gbuffer(SceneDev sc, FrameParams fp, unsigned long long first, uint32_t n, float eps,
                                                            float4 *__restrict__ records, float4 *__restrict__ aux, float4 *__restrict__ gbuffer,
                                                            uint32_t stack_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const auto geo = make_geo<LDSGEO>(sc, lds_stack, stack_words);
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (slot < n)   // (every lane of the block has passed the barrier)
    {
        const unsigned long long pixel = first + slot;
        const uint32_t gy = (uint32_t)(pixel / fp.width), gx = (uint32_t)(pixel - (unsigned long long)gy * fp.width);
        f3 o, d;
        camera_ray_centre(fp, gx, gy, o, d);
        const Closest c = scene_closest(geo, sc, lds_stack, o, d, eps);
        const bool hit = c.t != LP_F32_MAX;
        f3 p = splat(0.0f), nrm = splat(0.0f), color = splat(0.0f), glow;
        uint32_t inst = HIT_MISS, tri = 0u, state = LP_BAKED_MISS;
        float dst = 0.0f;
        if (hit)
        {
            inst = c.inst;
            dst = c.t;
            const Surface s = resolve_surface(sc, c.inst, c.tri, c.u, c.v);
            tri = c.tri - s.mesh.tri_offset;
            p = mk3(o.x + d.x * dst, o.y + d.y * dst, o.z + d.z * dst);
            const f3 ns = shading_normal(geo, sc, s);
            const float cs = (d.x * ns.x + d.y * ns.y) + d.z * ns.z;
            nrm = cs > 0.0f ? mk3(-ns.x, -ns.y, -ns.z) : ns;
            const MatPoint m = material_point<false>(sc, s);
            color = m.color;
            glow = m.emission;
            state = ray_record_ok(p.x, p.y, p.z, nrm.x, nrm.y, nrm.z, LP_RAY_DIRECTION) ? LP_BAKED_LOOKUP : LP_BAKED_NO_LOOKUP;
        }
        else glow = environment_radiance(sc, d);
        const bool ask = state == LP_BAKED_LOOKUP;
        records[2 * (size_t)slot] = ask ? make_float4(p.x, p.y, p.z, __uint_as_float(inst)) : make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(inst));
        records[2 * (size_t)slot + 1] = ask ? make_float4(nrm.x, nrm.y, nrm.z, __uint_as_float(tri)) : make_float4(0.0f, 0.0f, 1.0f, __uint_as_float(tri));
        aux[2 * (size_t)slot] = make_float4(color.x, color.y, color.z, __uint_as_float(state));
        aux[2 * (size_t)slot + 1] = make_float4(glow.x, glow.y, glow.z, dst);
        if (gbuffer)
        {
            float4 *__restrict__ g = gbuffer + 4 * (size_t)slot;
            g[0] = make_float4(p.x, p.y, p.z, __uint_as_float(inst));
            g[1] = make_float4(nrm.x, nrm.y, nrm.z, __uint_as_float(tri));
            g[2] = make_float4(color.x, color.y, color.z, 0.0f);   // [11] is k_baked_compose's
            g[3] = make_float4(glow.x, glow.y, glow.z, dst);
        }
    }
}

// `aux`, `results` (the lookup's, one float4 a slot) and `gbuffer` point at the launch's first slot; `texels` at the image's
// first texel (4 halves each).
__global__ void __launch_bounds__(LP_BLOCK) k_baked_compose(BakedViewDev v, unsigned long long first, uint32_t n, const float4 *__restrict__ aux,
                                                            const float4 *__restrict__ results, __half *__restrict__ texels, float4 *__restrict__ gbuffer)
{
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (slot >= n) return;
    const float4 a = aux[2 * (size_t)slot], b = aux[2 * (size_t)slot + 1];
    const uint32_t state = __float_as_uint(a.w);
    float r = b.x, g = b.y, bl = b.z, w = 0.0f;
    if (state != LP_BAKED_MISS)
    {
        float er = v.ar, eg = v.ag, eb = v.ab;
        if (state == LP_BAKED_LOOKUP)
        {
            const float4 e = results[slot];
            w = e.w;
            if (!(e.w == 0.0f)) { er = e.x; eg = e.y; eb = e.z; }
        }
        r = b.x + (a.x * er) * LP_BAKED_INV_PI;
        g = b.y + (a.y * eg) * LP_BAKED_INV_PI;
        bl = b.z + (a.z * eb) * LP_BAKED_INV_PI;
    }
    store_rgba16f(texels, (size_t)(first + slot), mk3(r, g, bl), v.store_rne != 0u);   // the renders' own store: one 8-byte word, alpha 1.0
    if (gbuffer) reinterpret_cast<float *>(gbuffer + 4 * (size_t)slot)[11] = w;
}
