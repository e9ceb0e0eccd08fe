// lupin_stitch.hpp -- the C++ host mirror of lightmap seam stitching (include/lupin_hip.h).
// tests/stitch_mirror_probe.cpp runs it against the Python host, word for word.
#pragma once

#include <vector>

#include "lupin.hpp"

namespace lp {

struct StitchDesc
{
    uint32_t width = 0, height = 0;      // the atlas, texels
    uint32_t iterations = 32;            // conjugate-gradient steps; 0: the counts and energies only
    float samples_per_texel = 2.0f;      // seam samples per texel of edge length
    float lambda = 0.1f;                 // the weight that keeps a texel near its baked value
    uint32_t flags = 0;                  // LUPIN_LIGHTMAP_STITCH_DEVICE_POINTERS
};

struct StitchResult
{
    std::vector<float> rgba;             // height x width x 4 (empty with LUPIN_LIGHTMAP_STITCH_DEVICE_POINTERS: out_rgba has it)
    LupinLightmapStitchInfo info{};
};

// lupin_hip_stitch_lightmap on host arrays: `rgba` is height x width x 4 floats, the atlas `charts` was baked with.
inline StitchResult stitch_lightmap(const Device &d, const Scene &scene, const StitchDesc &desc, const LightmapChart *charts, uint32_t num_charts,
                                    const float *rgba, float *out_rgba = nullptr)
{
    LupinLightmapStitchDesc c{};
    c.width = desc.width;
    c.height = desc.height;
    c.iterations = desc.iterations;
    c.samples_per_texel = desc.samples_per_texel;
    c.lambda = desc.lambda;
    c.flags = desc.flags;
    c.reserved = 0;
    const std::vector<LupinLightmapChart> cc = detail::charts_c(charts, num_charts);
    StitchResult r;
    if (!out_rgba)
    {
        if (desc.flags & LUPIN_LIGHTMAP_STITCH_DEVICE_POINTERS) throw Error(LUPIN_ERR_INVALID_ARGUMENT, "lp::stitch_lightmap: device pointers need an out_rgba");
        const bool sized = desc.width != 0 && desc.height != 0 && desc.width <= LUPIN_LIGHTMAP_MAX_SIZE && desc.height <= LUPIN_LIGHTMAP_MAX_SIZE;
        r.rgba.assign(sized ? (size_t)desc.width * desc.height * 4 : 4, 0.0f);      // a refused size: the library says so
        out_rgba = r.rgba.data();
    }
    check(lupin_hip_stitch_lightmap(d.raw(), scene.raw(), &c, cc.data(), num_charts, rgba, out_rgba, &r.info));
    return r;
}

inline LupinLightmapStitchStats lightmap_stitch_stats()
{
    LupinLightmapStitchStats s{};
    check(lupin_hip_lightmap_stitch_stats(&s));
    return s;
}

}  // namespace lp
