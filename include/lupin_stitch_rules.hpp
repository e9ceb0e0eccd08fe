// lupin_stitch_rules.hpp -- the host-side rules of lightmap seam stitching that need no device.
// Host only, no HIP header: the library (lupin_hip_stitch_lightmap) and tests/stitch_rules_main.cpp, which runs this file
// under the sanitizers, read the same functions.
#pragma once
#include <cmath>
#include <cstdint>

namespace lupin_stitch {

constexpr uint32_t MAX_SIZE = 16384u;             // LUPIN_LIGHTMAP_MAX_SIZE
constexpr uint32_t MAX_ITERATIONS = 1024u;        // LUPIN_LIGHTMAP_STITCH_MAX_ITERATIONS
constexpr uint32_t DEVICE_POINTERS = 1u;          // LUPIN_LIGHTMAP_STITCH_DEVICE_POINTERS
constexpr uint64_t MAX_COUNT = 0xFFFFFFFEull;     // half-edges, pairs and incidence entries: 2^32 - 2 at most

// What lupin_hip_stitch_lightmap refuses in its descriptor, in the order it looks; nullptr when it is fine.
inline const char *desc_refusal(uint32_t width, uint32_t height, uint32_t iterations, float samples_per_texel, float lambda, uint32_t flags,
                                uint32_t reserved)
{
    if (width == 0 || height == 0 || width > MAX_SIZE || height > MAX_SIZE) return "width and height must be in [1, 16384]";
    if (iterations > MAX_ITERATIONS) return "iterations must be <= 1024";
    if (!(std::isfinite(samples_per_texel) && samples_per_texel > 0.0f)) return "samples_per_texel must be finite and positive";
    if (!(std::isfinite(lambda) && lambda > 0.0f)) return "lambda must be finite and positive";
    if (flags & ~DEVICE_POINTERS) return "unknown flag";
    if (reserved != 0) return "reserved must be 0";
    return nullptr;
}

// The number of bits that hold every value 0 .. v (at least 1): the radix sorts' end bit for keys up to v.
inline int bits_for(uint64_t v)
{
    int b = 1;
    while (b < 64 && (v >> b) != 0) b++;
    return b;
}

// Whether `triangles` triangles give a half-edge count the call takes, and whether `pairs` sample pairs give an incidence
// count it takes (8 entries a pair).
inline bool half_edges_ok(uint64_t triangles) { return triangles <= MAX_COUNT / 3; }
inline bool pairs_ok(uint64_t pairs) { return pairs <= MAX_COUNT / 8; }

}   // namespace lupin_stitch
