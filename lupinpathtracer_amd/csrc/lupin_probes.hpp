// lupin_probes.hpp -- light-probe baking, included once by lupin_hip.hip after lupin_rays.hpp.
//
// lupin_hip_bake_probes path-traces `samples` uniformly distributed directions from every probe position and projects the
// radiance onto the nine real spherical harmonics of bands 0..2.  Probe i expands into `samples` paths, slot = i * samples + s,
// seeded as a radiance query seeds them.  One chunk of probes runs
//
//   k_validate_records<ProbeRule>   device positions only: counts the probes the host check would refuse (the host reads
//                        the count before the first wavefront)
//   k_begin_probes       k_begin_rays for probes: seeding, the sphere sampler, every plane k_begin_rays initialises, the queue
//                        append per shard; optionally the first ray of every slot as a mode-0 record (out_rays)
//   (the ordinary iterations, unchanged)
//   k_resolve_probes     one wave per probe: lane l sums samples l, l + 64, ... in ascending order, an xor butterfly adds
//                        the 64 partial sums, lanes 0..8 store one coefficient each
//
// The order of every sum is part of the contract (include/lupin_hip.h) and restated in tests/probe_ref.py.
// Every operation is f32 without contraction (-ffp-contract=off), as everywhere in the library.
#pragma once

#include "lupin_rays.hpp"

constexpr uint32_t LP_PROBE_SH = 9;           // LUPIN_PROBE_SH_COEFFS
constexpr uint32_t LP_PROBES_PER_BLOCK = LP_BLOCK / 64;

// Real spherical harmonics, bands 0..2, of the unit vector w in world x, y, z: literals and order of operations as in
// include/lupin_hip.h
LP_DEV void probe_sh_basis(f3 w, float (&Y)[LP_PROBE_SH])
{
    constexpr float k0 = 0.28209479f, k1 = 0.48860251f, k2 = 1.09254843f, k3 = 0.31539157f, k4 = 0.54627422f;
    Y[0] = k0;
    Y[1] = k1 * w.y;
    Y[2] = k1 * w.z;
    Y[3] = k1 * w.x;
    Y[4] = (k2 * w.x) * w.y;
    Y[5] = (k2 * w.y) * w.z;
    Y[6] = k3 * ((3.0f * w.z) * w.z - 1.0f);
    Y[7] = (k2 * w.x) * w.z;
    Y[8] = k4 * (w.x * w.x - w.y * w.y);
}

// RNG state of path s of a probe (the query's rule) and its direction: two draws, then the sphere sampler.  k_begin_probes
// hands the direction out, k_resolve_probes computes it again from the same word: both go through here.
LP_DEV f3 probe_direction(uint32_t word, uint32_t s, uint32_t &rng)
{
    rng = word;
    if (s != 0u) rng = hash_u32(rng + s * LP_RAY_SAMPLE_STRIDE);
    const float r0 = rnd(rng), r1 = rnd(rng);
    return sample_uniform_sphere(r0, r1);
}

// What lupin_hip_bake_probes refuses in a probe: a non-finite position.  (The RNG word is bits: any pattern is a state.)
__host__ __device__ inline bool probe_position_ok(float x, float y, float z)
{
    return ray_component_finite(x) && ray_component_finite(y) && ray_component_finite(z);
}

struct ProbeRule   // the probe as a record format (lupin_rays.hpp says what a Rule is)
{
    static constexpr uint32_t FLOATS = LUPIN_PROBE_FLOATS;
    static constexpr const char *NOUN = "probe", *WHY = "non-finite position";
    static bool host_ok(const float *p) { return probe_position_ok(p[0], p[1], p[2]); }
    static __device__ bool ok(const float4 *__restrict__ probes, unsigned long long i)
    {
        const float4 p = probes[i];
        return probe_position_ok(p.x, p.y, p.z);
    }
};

// `probes` and `out_rays` point at the chunk's first probe / first slot; n = the chunk's slots (probes * samples)
__global__ void __launch_bounds__(LP_BLOCK) k_begin_probes(PathBuffers pb, uint32_t n, const float4 *__restrict__ probes, uint32_t samples,
                                                           float4 *__restrict__ out_rays)
{
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    const bool live = slot < n;
    const uint32_t shard = blockIdx.x % LP_SHARDS;
    queue_append(live, slot, pb.queue[0] + (size_t)shard * pb.shard_cap, &pb.counts[shard]);
    if (!live) return;
    const uint32_t probe = slot / samples, s = slot - probe * samples;
    const float4 p = probes[probe];
    uint32_t rng;
    const f3 d = probe_direction(__float_as_uint(p.w), s, rng);
    const float4 orr = make_float4(p.x, p.y, p.z, __uint_as_float(rng));
    pb.ori_rng[slot] = orr;
    pb.dir_meta[slot] = make_float4(d.x, d.y, d.z, __uint_as_float(META_NEXT_EMISSION));
    pb.weight[slot] = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    pb.radiance[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    pb.color[slot] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    pb.next_hit[slot] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(HIT_MISS));
    pb.next_tri[slot] = 0u;
    if (out_rays)
    {
        out_rays[2 * (size_t)slot] = orr;
        out_rays[2 * (size_t)slot + 1] = make_float4(d.x, d.y, d.z, __uint_as_float(LP_RAY_DIRECTION));
    }
}

// One wave per probe of the chunk, LP_PROBES_PER_BLOCK probes per block; out: 9 x (r, g, b, w) per probe.  Consecutive
// lanes read consecutive slots' `color`.  The accumulators are indexed by unrolled constants only: they stay in registers.
__global__ void __launch_bounds__(LP_BLOCK) k_resolve_probes(PathBuffers pb, uint32_t num_probes, const float4 *__restrict__ probes,
                                                             uint32_t samples, float4 *__restrict__ out)
{
    const uint32_t probe = blockIdx.x * LP_PROBES_PER_BLOCK + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (probe >= num_probes) return;   // whole waves leave: the shuffles below see 64 lanes
    const uint32_t word = __float_as_uint(probes[probe].w);
    const size_t first = (size_t)probe * samples;
    float acc[LP_PROBE_SH][4];
#pragma unroll
    for (uint32_t j = 0; j < LP_PROBE_SH; j++)
        acc[j][0] = acc[j][1] = acc[j][2] = acc[j][3] = 0.0f;
    for (uint32_t s = lane; s < samples; s += 64u)
    {
        uint32_t rng;
        const f3 w = probe_direction(word, s, rng);
        float Y[LP_PROBE_SH];
        probe_sh_basis(w, Y);
        const float4 L = pb.color[first + s];
#pragma unroll
        for (uint32_t j = 0; j < LP_PROBE_SH; j++)
        {
            acc[j][0] += L.x * Y[j];
            acc[j][1] += L.y * Y[j];
            acc[j][2] += L.z * Y[j];
            acc[j][3] += Y[j];
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
        for (uint32_t j = 0; j < LP_PROBE_SH; j++)
#pragma unroll
            for (uint32_t c = 0; c < 4; c++) acc[j][c] = acc[j][c] + __shfl_xor(acc[j][c], off);
    const float scale = 4.0f * LP_PI, count = (float)samples;
#pragma unroll
    for (uint32_t j = 0; j < LP_PROBE_SH; j++)
        if (lane == j)
            out[(size_t)probe * LP_PROBE_SH + j] = make_float4((acc[j][0] * scale) / count, (acc[j][1] * scale) / count,
                                                               (acc[j][2] * scale) / count, (acc[j][3] * scale) / count);
}
