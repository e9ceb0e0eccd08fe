// lupin_probe_depth.hpp -- probe depth maps, included once by lupin_hip.hip after lupin_probe_grid.hpp.
//
// What a probe sees, as distances per direction: lupin_hip_bake_probe_depth bakes, per probe, an octahedral map of the first
// two moments of the distance to the nearest surface; lupin_hip_sample_probe_grid_depth is the irradiance volume lookup of
// lupin_probe_grid.hpp with the any-hit segment of a corner replaced by a Chebyshev test against that map: no traversal,
// and no scene geometry at all.
//
//   k_validate_records<ProbeDepthPositionRule>   device positions only: counts the positions the host check would refuse
//   k_probe_depth_stats_init   one thread per probe: rays, 0, 0, all-ones
//   k_probe_depth<LDSGEO, STATS>   ONE LANE PER RAY.  slot = ((probe * R * R + ty * R + tx) * K * K) + sy * K + sx: the K * K rays
//                          of a texel are adjacent lanes of one wave (K * K divides 64 and launches start at multiples of 64).
//                          Lane: octahedral direction of its sub-sample, scene_closest, d = the capped distance; then the
//                          lanes of the texel add (d, d * d) by xor-shuffles, offset K * K / 2 .. 1, every lane ending with
//                          the same sum; the texel's first lane divides and stores the texel and, where the texel lies on
//                          the map's edge, the border texels it is the source of.
//   k_probe_grid_depth     k_probe_grid's shape (eight adjacent lanes per record, one per corner) with the depth test in the
//                          segment's place, and k_probe_grid's own probe_grid_irradiance and probe_grid_fold_store (the
//                          ballot of the corners in use; the ascending sum by every lane).  No SceneDev, no LDS.
//
// The order of every operation is the contract (include/lupin_hip.h) and restated in tests/probe_depth_ref.py.  The sum of
// a texel is a butterfly: lane l adds lane l ^ offset, so every lane computes the same tree whatever K; the restatement
// builds that tree.
// Every lane of a wave reaches every shuffle and the ballot: lanes past the last slot trace nothing, hold d = 0 and store
// nothing; since slots come in whole texels a texel is never half alive.  Whole blocks run (make_geo<true> has a barrier).
// Stats are integer atomics (add, and an unsigned min on the bits of a distance that is never negative): the words do not
// depend on the order or on how the slots were cut into launches.
// Every float operation is f32 without contraction (-ffp-contract=off), division and square root correctly rounded.
#pragma once

#include "lupin_probe_grid.hpp"

constexpr uint32_t LP_PROBE_DEPTH_DEVICE_POINTERS = 1u;   // LUPIN_PROBE_DEPTH_DEVICE_POINTERS
constexpr uint32_t LP_PROBE_DEPTH_STATS = 4u;             // LUPIN_PROBE_DEPTH_STATS_WORDS

// What lupin_hip_bake_probe_depth refuses in a position: a non-finite coordinate.  Float 3 is not looked at.
struct ProbeDepthPositionRule   // the record format (lupin_rays.hpp says what a Rule is)
{
    static constexpr uint32_t FLOATS = 4;
    static constexpr const char *NOUN = "position", *WHY = "non-finite coordinate";
    static bool host_ok(const float *r) { return ray_component_finite(r[0]) && ray_component_finite(r[1]) && ray_component_finite(r[2]); }
    static __device__ bool ok(const float4 *__restrict__ records, unsigned long long i)
    {
        const float4 a = records[i];
        return ray_component_finite(a.x) && ray_component_finite(a.y) && ray_component_finite(a.z);
    }
};

LP_DEV float probe_depth_sgn(float x) { return x < 0.0f ? -1.0f : 1.0f; }   // sgn(0) = +1

// the octahedral decode of the header: (u, v) in [-1, 1]^2 -> unit vector
LP_DEV f3 probe_depth_decode(float u, float v)
{
    const float au = __builtin_fabsf(u), av = __builtin_fabsf(v);
    const float z = (1.0f - au) - av;
    float x = u, y = v;
    if (z < 0.0f)
    {
        x = (1.0f - av) * probe_depth_sgn(u);
        y = (1.0f - au) * probe_depth_sgn(v);
    }
    const float len = sqrtf((x * x + y * y) + z * z);
    return mk3(x / len, y / len, z / len);
}

// n probes, 4 words each
__global__ void __launch_bounds__(LP_BLOCK) k_probe_depth_stats_init(uint32_t n, uint32_t rays, uint4 *__restrict__ stats)
{
    const uint32_t i = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (i < n) stats[i] = make_uint4(rays, 0u, 0u, 0xFFFFFFFFu);
}

// `positions`, `out` and `stats` point at the batch's first probe; first = the launch's first slot within the batch (a
// multiple of 64), n = the launch's slots, below 2^31.  R in 2 .. 64, K in {1, 2, 4, 8}.
template <bool LDSGEO, bool STATS>
__global__ void __launch_bounds__(LP_BLOCK) k_probe_depth(SceneDev sc, unsigned long long first, uint32_t n, uint32_t R, uint32_t K, float eps, float maxd,
                                                          const float4 *__restrict__ positions, float2 *__restrict__ out, uint32_t *__restrict__ stats,
                                                          uint32_t stack_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const auto geo = make_geo<LDSGEO>(sc, lds_stack, stack_words);
    const uint32_t local = blockIdx.x * LP_BLOCK + threadIdx.x;
    const bool live = local < n;
    const uint32_t KK = K * K;
    float d = 0.0f;
    uint32_t hits = 0u, backs = 0u, dmin = 0xFFFFFFFFu;
    unsigned long long probe = 0;
    uint32_t tx = 0, ty = 0, sub = 0;
    if (live)
    {
        const unsigned long long slot = first + local, texel = slot / KK;
        sub = (uint32_t)(slot - texel * KK);
        probe = texel / (R * R);
        const uint32_t rem = (uint32_t)(texel - probe * (R * R));
        ty = rem / R; tx = rem - ty * R;
        const uint32_t sy = sub / K, sx = sub - sy * K;
        const float a = ((float)(tx * K + sx) + 0.5f) / (float)(R * K), b = ((float)(ty * K + sy) + 0.5f) / (float)(R * K);
        const f3 w = probe_depth_decode(2.0f * a - 1.0f, 2.0f * b - 1.0f);
        const float4 p = positions[probe];
        const Closest c = scene_closest(geo, sc, lds_stack, mk3(p.x, p.y, p.z), w, eps);
        const bool hit = c.t != LP_F32_MAX;
        d = hit ? __builtin_fminf(c.t, maxd) : maxd;
        if constexpr (STATS)
        {
            dmin = __float_as_uint(d);
            if (hit)
            {
                hits = 1u;
                const f3 g = geometric_normal(geo, sc.instances[c.inst], c.tri);   // what k_surface_probe reports in NORMAL mode [3..5]
                backs = ((w.x * g.x + w.y * g.y) + w.z * g.z) > 0.0f ? 1u : 0u;
            }
        }
    }
    // every lane of the wave is here
    float m1 = d, m2 = d * d;
    for (uint32_t offset = KK >> 1; offset != 0u; offset >>= 1)
    {
        m1 = m1 + __shfl_xor(m1, (int)offset);
        m2 = m2 + __shfl_xor(m2, (int)offset);
        if constexpr (STATS)
        {
            hits += __shfl_xor(hits, (int)offset);
            backs += __shfl_xor(backs, (int)offset);
            dmin = min(dmin, (uint32_t)__shfl_xor((int)dmin, (int)offset));
        }
    }
    if (!live || sub != 0u) return;
    const float2 m = make_float2(m1 / (float)KK, m2 / (float)KK);
    const uint32_t S = R + 2u;
    float2 *__restrict__ map = out + (size_t)probe * S * S;
    map[(ty + 1u) * S + (tx + 1u)] = m;
    // the border texels whose source this texel is: the edge mirrored, the corner from the opposite corner
    const bool ex = tx == 0u || tx == R - 1u, ey = ty == 0u || ty == R - 1u;
    const uint32_t bx = tx == 0u ? 0u : R + 1u, by = ty == 0u ? 0u : R + 1u;   // the border column / row beside this texel, in map coordinates
    if (ex) map[(R - ty) * S + bx] = m;                       // (bx, R - 1 - ty) + 1
    if (ey) map[by * S + (R - tx)] = m;
    if (ex && ey) map[(ty == 0u ? R + 1u : 0u) * S + (tx == 0u ? R + 1u : 0u)] = m;
    if constexpr (STATS)
    {
        uint32_t *__restrict__ s = stats + (size_t)probe * LP_PROBE_DEPTH_STATS;
        if (hits) atomicAdd(&s[1], hits);
        if (backs) atomicAdd(&s[2], backs);
        atomicMin(&s[3], dmin);
    }
}

// one axis of the texel address: px in [-1, 1] -> the left texel of the bordered map and the fraction
LP_DEV void probe_depth_axis(float px, uint32_t R, uint32_t &i, float &f)
{
    float a = px * 0.5f;
    a = a + 0.5f;
    a = a * (float)R;
    a = a + 0.5f;
    i = min((uint32_t)a, R);   // (the conversion saturates: a NaN or negative a is texel 0; i + 1 <= R + 1 whatever a)
    f = a - (float)i;
}

// `records` and `out` point at the chunk's first record; n = the chunk's records, at most 2^27 (n * 8 lanes fit 32 bits).
// Whole blocks run: the ballot and the shuffles see 64 lanes.  Steps 1 to 4 restate k_probe_grid's, line for line, with the
// depth test in its VIS block's place; then its irradiance and its fold (lupin_probe_grid.hpp, which also says why a skipped
// corner is not added and why the fold stands outside every branch).
__global__ void __launch_bounds__(LP_BLOCK) k_probe_grid_depth(uint32_t n, ProbeGridDev g, uint32_t R, float maxd, const float4 *__restrict__ sh,
                                                               const float2 *__restrict__ depth, const uint8_t *__restrict__ valid,
                                                               const float4 *__restrict__ records, float4 *__restrict__ out)
{
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    const uint32_t rec = slot / LP_PROBE_GRID_LANES, c = slot % LP_PROBE_GRID_LANES;
    const bool live = rec < n;
    bool use = false;
    float t = 0.0f, er = 0.0f, eg = 0.0f, eb = 0.0f;
    f3 nrm = mk3(0.0f, 0.0f, 1.0f);
    uint32_t index = 0u;
    if (live)
    {
        const float4 a = records[2 * (size_t)rec], b = records[2 * (size_t)rec + 1];
        nrm = mk3(b.x, b.y, b.z);
        const f3 o = mk3(a.x + nrm.x * g.bias, a.y + nrm.y * g.bias, a.z + nrm.z * g.bias);
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
            const float len = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
            const f3 dir = len == 0.0f ? nrm : mk3(d.x / len, d.y / len, d.z / len);
            if (g.flags & LP_PROBE_GRID_BACKFACE)
            {
                const float bf = (((dir.x * nrm.x + dir.y * nrm.y) + dir.z * nrm.z) + 1.0f) * 0.5f;
                t = t * (bf * bf + 0.2f);
            }
            if (len != 0.0f)
            {
                // the probe looks at the point: e = -dir, encoded
                const f3 e = mk3(-dir.x, -dir.y, -dir.z);
                const float s = (__builtin_fabsf(e.x) + __builtin_fabsf(e.y)) + __builtin_fabsf(e.z);
                float px = e.x / s, py = e.y / s;
                if (e.z < 0.0f)
                {
                    const float qx = (1.0f - __builtin_fabsf(py)) * probe_depth_sgn(px), qy = (1.0f - __builtin_fabsf(px)) * probe_depth_sgn(py);
                    px = qx; py = qy;
                }
                uint32_t jx, jy;
                float gx, gy;
                probe_depth_axis(px, R, jx, gx);
                probe_depth_axis(py, R, jy, gy);
                const uint32_t S = R + 2u;
                const float2 *__restrict__ map = depth + (size_t)index * S * S + (size_t)jy * S + jx;
                const float2 m00 = map[0], m10 = map[1], m01 = map[S], m11 = map[S + 1u];
                const float top1 = m00.x + gx * (m10.x - m00.x), bot1 = m01.x + gx * (m11.x - m01.x), m1 = top1 + gy * (bot1 - top1);
                const float top2 = m00.y + gx * (m10.y - m00.y), bot2 = m01.y + gx * (m11.y - m01.y), m2 = top2 + gy * (bot2 - top2);
                const float r = __builtin_fminf(len, maxd);
                if (r > m1)   // (false for a NaN m1: the corner counts as visible)
                {
                    const float x = m2 - m1 * m1, var = x > 0.0f ? x : 0.0f;   // (a NaN is 0)
                    const float dd = r - m1;
                    const float cc = var / (var + dd * dd);
                    const float vis = (cc * cc) * cc;
                    t = t * vis;
                    if (vis == 0.0f) use = false;
                }
            }
        }
    }
    if (use) probe_grid_irradiance(sh, index, nrm, er, eg, eb);
    probe_grid_fold_store(use, t, er, eg, eb, live && c == 0u, out, rec);   // (every lane of the wave is here)
}
