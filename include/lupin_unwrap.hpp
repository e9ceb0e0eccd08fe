// lupin_unwrap.hpp -- the C++ host mirror of the lightmap UV sets (include/lupin_hip.h): generating a set on the
// device and placing instances in one atlas.  Scene::set_lightmap_uvs is in lupin.hpp.  tests/unwrap_mirror_probe.cpp runs
// both functions against the Python host, word for word.
#pragma once

#include <utility>
#include <vector>

#include "lupin.hpp"
#include "lupin_pack.hpp"

namespace lp {

struct UnwrapDesc
{
    float texel_size = 0.0f;     // local units per texel; the caller chooses (> 0)
    uint32_t padding = 2;        // texels around every chart
};

struct UnwrapResult
{
    std::vector<float> uvs;                // 6 floats a triangle: (u, v) of its three corners, in texels of the mesh's own atlas
    std::vector<uint32_t> chart_of_tri;    // LUPIN_UNWRAP_NO_CHART for a degenerate triangle
    LupinUnwrapInfo info{};
};

// lupin_hip_unwrap_lightmap_uvs; the outputs are sized by the scene's own triangle count of the mesh
// (lupin_hip_scene_mesh_triangle_count).  It does not attach the set (Scene::set_lightmap_uvs does).
inline UnwrapResult unwrap_lightmap_uvs(const Device &d, const Scene &scene, uint32_t mesh_idx, const UnwrapDesc &desc)
{
    const int64_t count = lupin_hip_scene_mesh_triangle_count(scene.raw(), mesh_idx);
    if (count < 0) check((int)count);
    const uint32_t num_tris = (uint32_t)count;
    LupinUnwrapDesc c{};
    c.texel_size = desc.texel_size;
    c.padding = desc.padding;
    c.flags = 0;
    UnwrapResult r;
    r.uvs.assign((size_t)num_tris * 6, 0.0f);
    r.chart_of_tri.assign(num_tris, 0u);
    check(lupin_hip_unwrap_lightmap_uvs(d.raw(), scene.raw(), mesh_idx, &c, r.uvs.data(), r.chart_of_tri.data(), &r.info));
    return r;
}

// Places instances in one atlas, on the host.  sizes: per entry the (width, height) in texels of its mesh's own atlas
// (UnwrapResult::info); multipliers: per entry the resolution m relative to that atlas; gutter: texels kept free around every
// entry.  Entry i gets the rectangle ceil(size * m) + 2 * gutter per side, the rectangles go through the shelf packer of
// lupin_pack.hpp, and its chart is instance_idx = i, scale = (m / W, m / H), offset = ((x + gutter) / W, (y + gutter) / H),
// each one f32 division.  Throws LUPIN_ERR_INVALID_ARGUMENT for a multiplier that is not finite and positive, a size of 0, or
// a rectangle or an atlas above LUPIN_LIGHTMAP_MAX_SIZE.
inline std::vector<LightmapChart> pack_lightmap_instances(const std::vector<std::pair<uint32_t, uint32_t>> &sizes, const std::vector<float> &multipliers,
                                                          uint32_t gutter, uint32_t *out_width, uint32_t *out_height)
{
    if (sizes.size() != multipliers.size()) throw Error(LUPIN_ERR_INVALID_ARGUMENT, "lp::pack_lightmap_instances: one multiplier per size");
    std::vector<lupin_pack::Rect> rects(sizes.size());
    for (size_t i = 0; i < sizes.size(); i++)
    {
        uint32_t w = 0, h = 0;
        if (!lupin_pack::instance_side(sizes[i].first, multipliers[i], gutter, &w) || !lupin_pack::instance_side(sizes[i].second, multipliers[i], gutter, &h))
            throw Error(LUPIN_ERR_INVALID_ARGUMENT, "lp::pack_lightmap_instances: entry " + std::to_string(i) + " has no size, a bad multiplier, or is larger than 16384 texels");
        rects[i] = lupin_pack::Rect{w, h, (uint32_t)i, 0u, 0u};
    }
    uint64_t W = 0, H = 0;
    lupin_pack::shelf_pack(rects, &W, &H);
    if (W > LUPIN_LIGHTMAP_MAX_SIZE || H > LUPIN_LIGHTMAP_MAX_SIZE) throw Error(LUPIN_ERR_INVALID_ARGUMENT, "lp::pack_lightmap_instances: the atlas is larger than 16384 texels");
    std::vector<LightmapChart> charts(sizes.size());
    const float Wf = (float)W, Hf = (float)H;
    for (const lupin_pack::Rect &r : rects)
    {
        const float m = multipliers[r.label];
        LightmapChart &c = charts[r.label];
        c.instance_idx = r.label;
        c.scale_u = m / Wf;
        c.scale_v = m / Hf;
        c.offset_u = (float)(r.x + gutter) / Wf;
        c.offset_v = (float)(r.y + gutter) / Hf;
    }
    *out_width = (uint32_t)W;
    *out_height = (uint32_t)H;
    return charts;
}

}  // namespace lp
