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

// A pixel's primary hit, resolved once: what k_baked_gbuffer writes, and what the lightmapped view (lupin_lightmapped_view.hpp)
// goes on from.  `s` is the hit's surface where hit, and not set otherwise.
struct BakedPrimary
{
    Surface s;
    f3 p, nrm, color, glow;
    uint32_t inst, tri, state;
    float dst;
    bool hit;
};

// Step 1 of the contract: the centre ray of pixel `pixel` (y * W + x).  baked_primary traces it; the directional lightmapped
// view asks for it again where it needs the direction.
LP_DEV void baked_primary_ray(const FrameParams &fp, unsigned long long pixel, f3 &o, f3 &d)
{
    const uint32_t gy = (uint32_t)(pixel / fp.width), gx = (uint32_t)(pixel - (unsigned long long)gy * fp.width);
    camera_ray_centre(fp, gx, gy, o, d);
}

// Steps 1 to 4 of the contract for pixel first + slot; the lane has passed make_geo's barrier.
template <typename Geo>
LP_DEV BakedPrimary baked_primary(const Geo &geo, const SceneDev &sc, const FrameParams &fp, uint32_t *lds_stack, unsigned long long pixel, float eps)
{
    f3 o, d;
    baked_primary_ray(fp, pixel, o, d);
    const Closest c = scene_closest(geo, sc, lds_stack, o, d, eps);
    BakedPrimary r;
    r.hit = c.t != LP_F32_MAX;
    r.p = splat(0.0f); r.nrm = splat(0.0f); r.color = splat(0.0f);
    r.inst = HIT_MISS; r.tri = 0u; r.state = LP_BAKED_MISS;
    r.dst = 0.0f;
    if (r.hit)
    {
        r.inst = c.inst;
        r.dst = c.t;
        r.s = resolve_surface(sc, c.inst, c.tri, c.u, c.v);
        r.tri = c.tri - r.s.mesh.tri_offset;
        r.p = mk3(o.x + d.x * r.dst, o.y + d.y * r.dst, o.z + d.z * r.dst);
        const f3 ns = shading_normal(geo, sc, r.s);
        const float cs = (d.x * ns.x + d.y * ns.y) + d.z * ns.z;
        r.nrm = cs > 0.0f ? mk3(-ns.x, -ns.y, -ns.z) : ns;
        const MatPoint m = material_point<false>(sc, r.s);
        r.color = m.color;
        r.glow = m.emission;
        r.state = ray_record_ok(r.p.x, r.p.y, r.p.z, r.nrm.x, r.nrm.y, r.nrm.z, LP_RAY_DIRECTION) ? LP_BAKED_LOOKUP : LP_BAKED_NO_LOOKUP;
    }
    else r.glow = environment_radiance(sc, d);
    return r;
}

// The lookup's record of a pixel (see the head of this file), and the G-buffer's 16 words.
LP_DEV void baked_store_record(const BakedPrimary &r, bool ask, float4 *__restrict__ records, size_t slot)
{
    records[2 * slot] = ask ? make_float4(r.p.x, r.p.y, r.p.z, __uint_as_float(r.inst)) : make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(r.inst));
    records[2 * slot + 1] = ask ? make_float4(r.nrm.x, r.nrm.y, r.nrm.z, __uint_as_float(r.tri)) : make_float4(0.0f, 0.0f, 1.0f, __uint_as_float(r.tri));
}

LP_DEV void baked_store_gbuffer(const BakedPrimary &r, float4 *__restrict__ g)
{
    g[0] = make_float4(r.p.x, r.p.y, r.p.z, __uint_as_float(r.inst));
    g[1] = make_float4(r.nrm.x, r.nrm.y, r.nrm.z, __uint_as_float(r.tri));
    g[2] = make_float4(r.color.x, r.color.y, r.color.z, 0.0f);   // [11] is the compose kernel's
    g[3] = make_float4(r.glow.x, r.glow.y, r.glow.z, r.dst);
}

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
        const BakedPrimary r = baked_primary(geo, sc, fp, lds_stack, first + slot, eps);
        baked_store_record(r, r.state == LP_BAKED_LOOKUP, records, slot);
        aux[2 * (size_t)slot] = make_float4(r.color.x, r.color.y, r.color.z, __uint_as_float(r.state));
        aux[2 * (size_t)slot + 1] = make_float4(r.glow.x, r.glow.y, r.glow.z, r.dst);
        if (gbuffer) baked_store_gbuffer(r, gbuffer + 4 * (size_t)slot);
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
