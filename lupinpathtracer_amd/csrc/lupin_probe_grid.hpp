// lupin_probe_grid.hpp -- irradiance volume lookup, included once by lupin_hip.hip after lupin_distance.hpp.
//
// lupin_hip_sample_probe_grid goes from (point, normal) to irradiance over a regular grid of baked probes
// (lupin_hip_bake_probes' coefficients): the cell, the trilinear weights of its eight probes, the probes the caller marked
// invalid dropped, the probes behind a wall dropped (the any-hit segment of lupin_occlusion.hpp, point -> probe), the
// backface weight, the clamped cosine's irradiance at the normal, and the normalisation -- one kernel, nothing on the host.
//
//   k_validate_records<ProbeGridRecordRule>   device records only: counts the records the host check would refuse
//   k_probe_grid<LDSGEO, VIS>   EIGHT ADJACENT LANES PER RECORD, one per corner of the cell: a wave holds eight records.
//                          Lane c computes its corner's weight t and irradiance E (and, with VIS, runs the corner's segment
//                          through scene_any_hit); then every lane of the group fetches the eight (t, E) by shuffle and
//                          adds the ones in use in ascending c from +0; the group's first lane stores.
//
// The order of every operation is the contract (include/lupin_hip.h) and restated in tests/probe_grid_ref.py: the result
// does not depend on the eight-lane shape.  What follows a corner's visibility is written once, for this kernel and for
// k_probe_grid_depth (lupin_probe_depth.hpp): probe_grid_irradiance and probe_grid_fold_store, below.  The corner itself
// (steps 1 to 4) and, here, the irradiance stay in the kernels: as force-inlined functions they changed the kernels'
// registers (DESIGN.md 23 "One fold, two corners").
// VIS = false reserves no traversal stack and stages no geometry: the launch has no dynamic LDS.
// Every float operation is f32 without contraction (-ffp-contract=off), division and square root correctly rounded.
#pragma once

#include "lupin_occlusion.hpp"

constexpr uint32_t LP_PROBE_GRID_DEVICE_POINTERS = 1u, LP_PROBE_GRID_VISIBILITY = 2u, LP_PROBE_GRID_BACKFACE = 4u;   // LUPIN_PROBE_GRID_*
constexpr uint32_t LP_PROBE_GRID_LANES = 8u;                                  // lanes per record: the corners of a cell
constexpr uint32_t LP_PROBE_GRID_RECORDS_PER_BLOCK = LP_BLOCK / LP_PROBE_GRID_LANES;
// the clamped cosine's band factors pi, 2 pi / 3, pi / 4: the literals of include/lupin_hip.h
constexpr float LP_SH_A0 = 3.14159265f, LP_SH_A1 = 2.09439510f, LP_SH_A2 = 0.78539816f;

// What lupin_hip_sample_probe_grid refuses in a record: a non-finite point or normal, a normal whose squared length is
// further than LP_RAY_UNIT_TOLERANCE from 1 -- a direction-mode ray record's rule.  Floats 3 and 7 are not looked at.
struct ProbeGridRecordRule   // the record format (lupin_rays.hpp says what a Rule is)
{
    static constexpr uint32_t FLOATS = LUPIN_PROBE_GRID_RECORD_FLOATS;
    static constexpr const char *NOUN = "record", *WHY = "non-finite point or normal, or normal not of unit length";
    static bool host_ok(const float *r) { return ray_record_ok(r[0], r[1], r[2], r[4], r[5], r[6], LP_RAY_DIRECTION); }
    static __device__ bool ok(const float4 *__restrict__ records, unsigned long long i)
    {
        const float4 a = records[2 * i], b = records[2 * i + 1];
        return ray_record_ok(a.x, a.y, a.z, b.x, b.y, b.z, LP_RAY_DIRECTION);
    }
};

struct ProbeGridDev   // LupinProbeGridDesc as the kernel takes it
{
    float ox, oy, oz, sx, sy, sz;
    uint32_t nx, ny, nz, flags;
    float eps, bias;
};

// one axis of step 2: the cell index and the fraction within it
LP_DEV void probe_grid_axis(float o, float origin, float spacing, uint32_t dim, uint32_t &i, float &f)
{
    float g = (o - origin) / spacing;
    g = __builtin_fminf(__builtin_fmaxf(g, 0.0f), (float)(dim - 1u));
    i = dim > 1u ? min((uint32_t)g, dim - 2u) : 0u;
    f = g - (float)i;
}

// ---- what k_probe_grid and k_probe_grid_depth share once a corner's visibility is known ----
// A corner that is skipped (zero trilinear weight, invalid, not visible) is NOT added: adding 0 * E would turn a NaN
// coefficient of a skipped probe into the result.  Which corners are in use travels as a ballot, not as t == 0: a weight
// that underflows to 0 after the backface factor is still added.
// Every lane of a wave reaches the ballot and every shuffle, so probe_grid_fold_store stands outside every branch: lanes of
// records past n, of skipped corners and of traversals that ended early leave only the traversal, never the kernel.

// the clamped cosine's irradiance of probe `index` at nrm, added to (er, eg, eb) term by term from band 0
LP_DEV void probe_grid_irradiance(const float4 *__restrict__ sh, uint32_t index, f3 nrm, float &er, float &eg, float &eb)
{
    float Y[LP_PROBE_SH];
    probe_sh_basis(nrm, Y);
    const float4 *__restrict__ s = sh + (size_t)index * LP_PROBE_SH;
#pragma unroll
    for (uint32_t j = 0; j < LP_PROBE_SH; j++)
    {
        const float B = (j == 0 ? LP_SH_A0 : j < 4 ? LP_SH_A1 : LP_SH_A2) * Y[j];
        const float4 v = s[j];
        er = er + B * v.x;
        eg = eg + B * v.y;
        eb = eb + B * v.z;
    }
}

// EVERY LANE OF THE WAVE CALLS THIS: the group's (t, E) in use added in ascending c from +0, stored normalised where `store`
LP_DEV void probe_grid_fold_store(bool use, float t, float er, float eg, float eb, bool store, float4 *__restrict__ out, uint32_t rec)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t used = (uint32_t)(__ballot(use) >> (lane & ~(LP_PROBE_GRID_LANES - 1u))) & 0xFFu;
    float ar = 0.0f, ag = 0.0f, ab = 0.0f, aw = 0.0f;
#pragma unroll
    for (uint32_t k = 0; k < LP_PROBE_GRID_LANES; k++)
    {
        const float tk = __shfl(t, (int)k, (int)LP_PROBE_GRID_LANES), rk = __shfl(er, (int)k, (int)LP_PROBE_GRID_LANES),
                    gk = __shfl(eg, (int)k, (int)LP_PROBE_GRID_LANES), bk = __shfl(eb, (int)k, (int)LP_PROBE_GRID_LANES);
        if (used & (1u << k))
        {
            ar = ar + tk * rk;
            ag = ag + tk * gk;
            ab = ab + tk * bk;
            aw = aw + tk;
        }
    }
    if (store) out[rec] = aw > 0.0f ? make_float4(ar / aw, ag / aw, ab / aw, aw) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// `records` and `out` point at the chunk's first record; n = the chunk's records, at most 2^27 (n * 8 lanes fit 32 bits).
// Whole blocks run (make_geo<true> has a barrier; the ballot and the shuffles see 64 lanes).
template <bool LDSGEO, bool VIS>
__global__ void __launch_bounds__(LP_BLOCK) k_probe_grid(SceneDev sc, uint32_t n, ProbeGridDev g, const float4 *__restrict__ sh,
                                                         const uint8_t *__restrict__ valid, const float4 *__restrict__ records,
                                                         float4 *__restrict__ out, uint32_t stack_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    const uint32_t rec = slot / LP_PROBE_GRID_LANES, c = slot % LP_PROBE_GRID_LANES;
    const bool live = rec < n;
    bool use = false;
    float t = 0.0f, er = 0.0f, eg = 0.0f, eb = 0.0f;
    f3 o = mk3(0.0f, 0.0f, 0.0f), nrm = mk3(0.0f, 0.0f, 1.0f), dir = nrm;
    float len = 0.0f;
    uint32_t index = 0u;
    if (live)
    {
        const float4 a = records[2 * (size_t)rec], b = records[2 * (size_t)rec + 1];
        nrm = mk3(b.x, b.y, b.z);
        o = mk3(a.x + nrm.x * g.bias, a.y + nrm.y * g.bias, a.z + nrm.z * g.bias);
        uint32_t ix, iy, iz;
        float fx, fy, fz;
        probe_grid_axis(o.x, g.ox, g.sx, g.nx, ix, fx);
        probe_grid_axis(o.y, g.oy, g.sy, g.ny, iy, fy);
        probe_grid_axis(o.z, g.oz, g.sz, g.nz, iz, fz);
        const uint32_t bx = c & 1u, by = (c >> 1) & 1u, bz = c >> 2;
        const float wx = bx ? fx : 1.0f - fx, wy = by ? fy : 1.0f - fy, wz = bz ? fz : 1.0f - fz;
        t = (wx * wy) * wz;
        use = t != 0.0f;   // (a zero weight's corner may lie outside the grid: nothing of it is read)
        if (use)
        {
            ix += bx; iy += by; iz += bz;
            index = ix + g.nx * (iy + g.ny * iz);
            if (valid && valid[index] == 0) use = false;
        }
        if (use)
        {
            const f3 q = mk3(g.ox + (float)ix * g.sx, g.oy + (float)iy * g.sy, g.oz + (float)iz * g.sz);
            const f3 d = mk3(q.x - o.x, q.y - o.y, q.z - o.z);
            len = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
            dir = len == 0.0f ? nrm : mk3(d.x / len, d.y / len, d.z / len);
            if (g.flags & LP_PROBE_GRID_BACKFACE)
            {
                const float bf = (((dir.x * nrm.x + dir.y * nrm.y) + dir.z * nrm.z) + 1.0f) * 0.5f;
                t = t * (bf * bf + 0.2f);
            }
        }
    }
    if constexpr (VIS)
    {
        const auto geo = make_geo<LDSGEO>(sc, lds_stack, stack_words);   // (its barrier: every lane of the block is here)
        if (use && len > 2.0f * g.eps)
            if (scene_any_hit(geo, sc, lds_stack, o, dir, g.eps, len - g.eps)) use = false;
    }
    if (use)   // probe_grid_irradiance, restated: the call costs this kernel three SGPRs and moves its VGPRs
    {
        float Y[LP_PROBE_SH];
        probe_sh_basis(nrm, Y);
        const float4 *__restrict__ s = sh + (size_t)index * LP_PROBE_SH;
#pragma unroll
        for (uint32_t j = 0; j < LP_PROBE_SH; j++)
        {
            const float B = (j == 0 ? LP_SH_A0 : j < 4 ? LP_SH_A1 : LP_SH_A2) * Y[j];
            const float4 v = s[j];
            er = er + B * v.x;
            eg = eg + B * v.y;
            eb = eb + B * v.z;
        }
    }
    probe_grid_fold_store(use, t, er, eg, eb, live && c == 0u, out, rec);
}
