// lupin_pack.hpp -- the shelf packer and the descriptor checks of the lightmap unwrap (include/lupin_hip.h).
// Host only, no HIP header: the library (lupin_hip_unwrap_lightmap_uvs), the C++ host mirror (include/lupin_unwrap.hpp) and
// tests/unwrap_pack_main.cpp (under the sanitizers) all compile this one file.  Everything is integer arithmetic except
// lupin_pack::extent_texels, whose three f32 operations are separately rounded (-ffp-contract=off).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace lupin_pack {

constexpr uint32_t MAX_SIZE = 16384u;      // LUPIN_LIGHTMAP_MAX_SIZE
constexpr uint32_t MAX_PADDING = 16u;      // LUPIN_UNWRAP_MAX_PADDING

struct Rect
{
    uint32_t w, h;       // in: the rectangle, texels
    uint32_t label;      // in: the last sort key (unique among the rectangles of a call)
    uint32_t x, y;       // out: its place
};

// the smallest r with r * r >= n
inline uint64_t isqrt_ceil(uint64_t n)
{
    if (n == 0) return 0;
    uint64_t r = (uint64_t)std::sqrt((double)n);
    while (r * r >= n && r > 0) r--;       // now r * r < n ...
    while (r * r < n) r++;                 // ... and r is the first with r * r >= n (r <= 2^32: no overflow for n <= 2^63)
    return r;
}

// One shelf packer: sort by height descending, then width descending, then label ascending; the atlas is
// max(widest rectangle, isqrt_ceil(sum of areas)) wide; rectangles go left to right, a new shelf opens when the next one
// would cross the width; the height is the bottom of the last shelf.  `rects` comes back in the sorted order, placed.
inline void shelf_pack(std::vector<Rect> &rects, uint64_t *width, uint64_t *height)
{
    std::sort(rects.begin(), rects.end(), [](const Rect &a, const Rect &b) {
        if (a.h != b.h) return a.h > b.h;
        if (a.w != b.w) return a.w > b.w;
        return a.label < b.label;
    });
    uint64_t area = 0, widest = 0;
    for (const Rect &r : rects)
    {
        area += (uint64_t)r.w * r.h;
        widest = std::max<uint64_t>(widest, r.w);
    }
    const uint64_t W = std::max(widest, isqrt_ceil(area));
    uint64_t x = 0, y = 0, shelf = 0;
    for (Rect &r : rects)
    {
        if (x + r.w > W) { y += shelf; x = 0; shelf = 0; }
        r.x = (uint32_t)x;
        r.y = (uint32_t)y;
        x += r.w;
        shelf = std::max<uint64_t>(shelf, r.h);
    }
    *width = W;
    *height = y + shelf;
}

// What lupin_hip_unwrap_lightmap_uvs refuses in its descriptor; nullptr when it is fine.
inline const char *unwrap_desc_refusal(float texel_size, uint32_t padding, uint32_t flags)
{
    if (!(std::isfinite(texel_size) && texel_size > 0.0f)) return "texel_size must be finite and positive";
    if (padding > MAX_PADDING) return "padding must be <= 16";
    if (flags != 0u) return "unknown flag";
    return nullptr;
}

// A chart's extent along one plane axis, texels: ceil((hi - lo) / texel_size), at least 1.  false when it is above
// MAX_SIZE or not a number (hi - lo overflowed): the atlas would be refused anyway.
inline bool extent_texels(float lo, float hi, float texel_size, uint32_t *out)
{
    const float d = hi - lo;
    const float q = d / texel_size;
    const float c = std::ceil(q);
    if (!(c <= (float)MAX_SIZE)) return false;
    *out = c < 1.0f ? 1u : (uint32_t)c;
    return true;
}

// A placed instance's rectangle side: ceil(size * multiplier) + 2 * gutter, with the product one f32 operation.  false when
// the multiplier is not finite and positive, the size is 0 or the side is above MAX_SIZE.
inline bool instance_side(uint32_t size, float multiplier, uint32_t gutter, uint32_t *out)
{
    if (!(std::isfinite(multiplier) && multiplier > 0.0f) || size == 0u || size > MAX_SIZE || gutter > MAX_SIZE) return false;
    const float p = (float)size * multiplier;
    const float c = std::ceil(p);
    if (!(c <= (float)MAX_SIZE)) return false;
    const uint32_t side = (c < 1.0f ? 1u : (uint32_t)c) + 2u * gutter;
    if (side > MAX_SIZE) return false;
    *out = side;
    return true;
}

}  // namespace lupin_pack
