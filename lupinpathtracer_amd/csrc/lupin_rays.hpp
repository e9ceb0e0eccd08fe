// lupin_rays.hpp -- radiance queries, included once by lupin_hip.hip after lupin_stages.hpp.
//
// lupin_hip_pathtrace_rays path-traces caller-supplied rays: a second way into the wavefront and a second way out of it.
// A record is the ori_rng / dir_meta pair of a path (origin | RNG state, direction or normal | mode); record i expands
// into `samples` paths, slot = i * samples + s.  One chunk of records runs
//
//   k_validate_records<RayRecordRule>   device records only: counts the records the host check would refuse (the host
//                        reads the count before the first wavefront)
//   k_begin_rays         k_begin for records: seeding, hemisphere sampling, every plane begin_paths initialises, the queue
//                        append per shard; optionally the first ray of every slot as a mode-0 record (out_rays)
//   (the ordinary iterations, unchanged: the stage kernels only ever see slots; with fp.spp == 1 path_epilogue never
//   starts a camera sample)
//   k_resolve_rays       one thread per record: the f32 sum of its slots' `color` in sample order, / samples
//
// Every operation is f32 without contraction (-ffp-contract=off), as everywhere in the library.
#pragma once

#include "lupin_stages.hpp"

constexpr uint32_t LP_RAY_DIRECTION = 0u, LP_RAY_COSINE_HEMISPHERE = 1u;   // LUPIN_RAY_* (include/lupin_hip.h)
constexpr uint32_t LP_RAY_SAMPLE_STRIDE = 0x9E3779B9u;                     // RNG state of path s > 0: hash_u32(word + s * stride)
constexpr float LP_RAY_UNIT_TOLERANCE = 1e-4f;                              // | |d|^2 - 1 | a record's direction or normal may have

// What lupin_hip_pathtrace_rays refuses in a record: a non-finite origin or direction / normal, a squared length further
// than LP_RAY_UNIT_TOLERANCE from 1, an unknown mode.  (The RNG word is bits: any pattern is a state.)  The host check
// and RayRecordRule share this function.
__host__ __device__ inline bool ray_component_finite(float v)
{
    uint32_t u;
    memcpy(&u, &v, 4);
    return (u & 0x7F800000u) != 0x7F800000u;
}
__host__ __device__ inline bool ray_record_ok(float ox, float oy, float oz, float dx, float dy, float dz, uint32_t mode)
{
    if (!(ray_component_finite(ox) && ray_component_finite(oy) && ray_component_finite(oz) && ray_component_finite(dx) &&
          ray_component_finite(dy) && ray_component_finite(dz)))
        return false;
    if (mode > LP_RAY_COSINE_HEMISPHERE) return false;
    const float off = ((dx * dx + dy * dy) + dz * dz) - 1.0f;
    return off <= LP_RAY_UNIT_TOLERANCE && off >= -LP_RAY_UNIT_TOLERANCE;   // (an overflowed length is +inf: refused)
}

// A Rule is one record format of a scene query (RayRecordRule here; ProbeRule, OcclusionRecordRule and DistanceRecordRule
// beside their formats): its size, how a refusal names it, the host's look at one record (host_ok) and the same look on
// the device (ok).  Device records of every query are checked by this one kernel: one thread per record; a wave that found
// something adds its count with one atomic.
template <typename Rule>
__global__ void __launch_bounds__(LP_BLOCK) k_validate_records(const float4 *__restrict__ records, unsigned long long n, unsigned long long *bad_count)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * LP_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < n) bad = !Rule::ok(records, i);
    const unsigned long long mask = __ballot(bad);
    if (mask && (threadIdx.x & 63u) == (uint32_t)(__ffsll((long long)mask) - 1)) atomicAdd(bad_count, (unsigned long long)__popcll(mask));
}

struct RayRecordRule
{
    static constexpr uint32_t FLOATS = LUPIN_RAY_RECORD_FLOATS;
    static constexpr const char *NOUN = "record", *WHY = "non-finite component, direction or normal not of unit length, or unknown mode";
    static bool host_ok(const float *r)
    {
        uint32_t mode;
        memcpy(&mode, &r[7], 4);
        return ray_record_ok(r[0], r[1], r[2], r[4], r[5], r[6], mode);
    }
    static __device__ bool ok(const float4 *__restrict__ records, unsigned long long i)
    {
        const float4 a = records[2 * i], b = records[2 * i + 1];
        return ray_record_ok(a.x, a.y, a.z, b.x, b.y, b.z, __float_as_uint(b.w));
    }
};

// RNG state of path s of the record (a, b) (the query's rule) and the path's first direction: the record's own in mode 0; in
// mode 1 two draws, then the matte BSDF's sampler (sample_cos_hemisphere) about the record's normal.  k_begin_rays hands the
// direction out, k_resolve_lightmap_sh (lupin_lightmap_directional.hpp) computes it again from the same record: both go
// through here.
LP_DEV f3 ray_first_direction(float4 a, float4 b, uint32_t s, uint32_t &rng)
{
    rng = __float_as_uint(a.w);
    if (s != 0u) rng = hash_u32(rng + s * LP_RAY_SAMPLE_STRIDE);
    f3 d = mk3(b.x, b.y, b.z);
    if (__float_as_uint(b.w) == LP_RAY_COSINE_HEMISPHERE)
    {
        const float r0 = rnd(rng), r1 = rnd(rng);
        d = sample_cos_hemisphere(d, r0, r1);
    }
    return d;
}

// `records` and `out_rays` point at the chunk's first record / first slot; n = the chunk's slots (records * samples)
__global__ void __launch_bounds__(LP_BLOCK) k_begin_rays(PathBuffers pb, uint32_t n, const float4 *__restrict__ records, uint32_t samples,
                                                         float4 *__restrict__ out_rays)
{
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    const bool live = slot < n;
    const uint32_t shard = blockIdx.x % LP_SHARDS;
    queue_append(live, slot, pb.queue[0] + (size_t)shard * pb.shard_cap, &pb.counts[shard]);
    if (!live) return;
    const uint32_t rec = slot / samples, s = slot - rec * samples;
    const float4 a = records[2 * (size_t)rec], b = records[2 * (size_t)rec + 1];
    uint32_t rng;
    const f3 d = ray_first_direction(a, b, s, rng);
    const float4 orr = make_float4(a.x, a.y, a.z, __uint_as_float(rng));
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

// one thread per record of the chunk: r, g, b, 1
__global__ void __launch_bounds__(LP_BLOCK) k_resolve_rays(PathBuffers pb, uint32_t num_records, uint32_t samples, float4 *__restrict__ out)
{
    const uint32_t rec = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (rec >= num_records) return;
    f3 sum = splat(0.0f);
    const size_t first = (size_t)rec * samples;
    for (uint32_t s = 0; s < samples; s++)
    {
        const float4 c = pb.color[first + s];
        sum = add(sum, mk3(c.x, c.y, c.z));
    }
    const float count = (float)samples;
    out[rec] = make_float4(sum.x / count, sum.y / count, sum.z / count, 1.0f);
}
