// cpp_mirror_probe.cpp -- runs every entry point of the C++ host mirror (include/lupin.hpp) that no example calls, on inputs
// read from a blob, and writes every output to a blob; tests/test_cpp_mirror.py makes the same calls through the Python
// host and compares the words.  No RNG here and no arithmetic of its own: what is compared is the header's.
//
//   cpp_mirror_probe <inputs.bin> <outputs.bin> [section ...]     no section names: every section
//   cpp_mirror_probe --list                                       one line per section: its name, then the lp:: names it runs
//
// A blob is a flat list of named arrays: u32 name length, name bytes, u32 dtype code (0 f32, 1 u32, 2 u8, 3 u16), u32 ndim,
// u64 dims, raw bytes (tests/cpp_mirror.py is the Python twin).  A scalar is an array of one element.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <iostream>
#include <memory>

#include "lupin_loader.hpp"

namespace {

enum Dtype : uint32_t { F32 = 0, U32 = 1, U8 = 2, U16 = 3 };
const size_t DTYPE_SIZE[4] = {4, 4, 1, 2};
struct Array { uint32_t dtype = F32; std::vector<uint64_t> dims; std::vector<uint8_t> bytes; };

struct Blob
{
    std::vector<std::pair<std::string, Array>> items;
    static Blob read(const std::string &path)
    {
        Blob b;
        FILE *f = std::fopen(path.c_str(), "rb");
        if (!f) throw std::runtime_error("cannot open " + path);
        auto get = [&](void *dst, size_t n) { if (n && std::fread(dst, 1, n, f) != n) throw std::runtime_error(path + ": truncated"); };
        uint32_t len;
        while (std::fread(&len, 1, 4, f) == 4)
        {
            std::string name(len, '\0');
            get(&name[0], len);
            Array a;
            uint32_t ndim;
            get(&a.dtype, 4); get(&ndim, 4);
            if (a.dtype > U16) throw std::runtime_error(path + ": unknown dtype");
            a.dims.resize(ndim);
            get(a.dims.data(), 8 * (size_t)ndim);
            size_t count = 1;
            for (uint64_t d : a.dims) count *= (size_t)d;
            a.bytes.resize(count * DTYPE_SIZE[a.dtype]);
            get(a.bytes.data(), a.bytes.size());
            b.items.emplace_back(std::move(name), std::move(a));
        }
        std::fclose(f);
        return b;
    }
    void write(const std::string &path) const
    {
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) throw std::runtime_error("cannot open " + path);
        for (const auto &it : items)
        {
            const uint32_t len = (uint32_t)it.first.size(), ndim = (uint32_t)it.second.dims.size();
            std::fwrite(&len, 4, 1, f); std::fwrite(it.first.data(), 1, len, f);
            std::fwrite(&it.second.dtype, 4, 1, f); std::fwrite(&ndim, 4, 1, f);
            std::fwrite(it.second.dims.data(), 8, ndim, f);
            std::fwrite(it.second.bytes.data(), 1, it.second.bytes.size(), f);
        }
        if (std::fclose(f) != 0) throw std::runtime_error("cannot write " + path);
    }
    const Array &at(const std::string &name, uint32_t dtype) const
    {
        for (const auto &it : items)
            if (it.first == name)
            {
                if (it.second.dtype != dtype) throw std::runtime_error("input " + name + " has another dtype");
                return it.second;
            }
        throw std::runtime_error("input " + name + " is missing");
    }
    void put(const std::string &name, uint32_t dtype, std::vector<uint64_t> dims, const void *data)
    {
        Array a;
        a.dtype = dtype;
        a.dims = std::move(dims);
        size_t count = 1;
        for (uint64_t d : a.dims) count *= (size_t)d;
        a.bytes.assign((const uint8_t *)data, (const uint8_t *)data + count * DTYPE_SIZE[dtype]);
        items.emplace_back(name, std::move(a));
    }
};

Blob in, out;

const float *f32(const std::string &name) { return (const float *)in.at(name, F32).bytes.data(); }
const uint32_t *u32(const std::string &name) { return (const uint32_t *)in.at(name, U32).bytes.data(); }
const uint8_t *u8(const std::string &name) { return in.at(name, U8).bytes.data(); }
float F(const std::string &name) { return f32(name)[0]; }
uint32_t U(const std::string &name) { return u32(name)[0]; }
uint64_t rows(const std::string &name, uint32_t dtype) { return in.at(name, dtype).dims.at(0); }
std::array<float, 3> f3(const std::string &name) { const float *p = f32(name); return {{p[0], p[1], p[2]}}; }
std::array<uint32_t, 3> u3(const std::string &name) { const uint32_t *p = u32(name); return {{p[0], p[1], p[2]}}; }
void put_f(const std::string &name, std::vector<uint64_t> dims, const float *p) { out.put(name, F32, std::move(dims), p); }
void put_u(const std::string &name, std::vector<uint64_t> dims, const uint32_t *p) { out.put(name, U32, std::move(dims), p); }
void put_scalar(const std::string &name, float v) { out.put(name, F32, {1}, &v); }
void put_scalar(const std::string &name, uint32_t v) { out.put(name, U32, {1}, &v); }
void put_texture(const std::string &name, lp::TextureRef t)
{
    const std::vector<uint16_t> px = t.download();
    out.put(name, U16, {t.height(), t.width(), 4}, px.data());
}

lp::CameraParams camera_params(const std::string &k)
{
    lp::CameraParams c;
    c.is_orthographic = U(k + ".is_orthographic") != 0;
    c.lens = F(k + ".lens"); c.film = F(k + ".film"); c.aspect = F(k + ".aspect"); c.focus = F(k + ".focus"); c.aperture = F(k + ".aperture");
    return c;
}
lp::Mat3x4 mat3x4(const std::string &name)
{
    lp::Mat3x4 m;
    std::memcpy(&m, f32(name), sizeof m);
    return m;
}
lp::AdvancedParams advanced(const std::string &k)
{
    lp::AdvancedParams a;
    a.max_radiance = F(k + ".max_radiance"); a.rng_seed = U(k + ".rng_seed"); a.ray_epsilon = F(k + ".ray_epsilon");
    return a;
}
// every field of a PathtraceDesc from the blob; accum_params and tile_params are the section's
lp::PathtraceDesc pathtrace_desc(const std::string &k)
{
    lp::PathtraceDesc d;
    d.accum_params.reset();
    d.tile_params.reset();
    d.camera_params = camera_params(k + ".camera");
    d.camera_transform = mat3x4(k + ".camera_transform");
    d.force_software_bvh = U(k + ".force_software_bvh") != 0;
    d.advanced = advanced(k + ".advanced");
    return d;
}
lp::BakedPathtraceParams baked_params(const std::string &k)
{
    lp::BakedPathtraceParams p;
    p.with_runtime_checks = U(k + ".with_runtime_checks") != 0; p.max_bounces = U(k + ".max_bounces"); p.samples_per_pixel = U(k + ".samples_per_pixel");
    return p;
}
lp::RayQueryDesc ray_query_desc(const std::string &k)
{
    lp::RayQueryDesc d;
    d.pathtrace_type = (lp::PathtraceType)U(k + ".pathtrace_type"); d.max_bounces = U(k + ".max_bounces"); d.samples = U(k + ".samples");
    d.flags = U(k + ".flags"); d.max_slots = U(k + ".max_slots"); d.advanced = advanced(k + ".advanced");
    return d;
}
lp::LightmapDesc lightmap_desc(const std::string &k)
{
    lp::LightmapDesc d;
    d.width = U(k + ".width"); d.height = U(k + ".height"); d.pathtrace_type = (lp::PathtraceType)U(k + ".pathtrace_type");
    d.max_bounces = U(k + ".max_bounces"); d.samples = U(k + ".samples"); d.max_slots = U(k + ".max_slots"); d.flags = U(k + ".flags");
    d.dilate = U(k + ".dilate"); d.counter = U(k + ".counter"); d.surface_offset = F(k + ".surface_offset"); d.advanced = advanced(k + ".advanced");
    return d;
}
std::vector<lp::LightmapChart> charts(const std::string &k)
{
    const uint32_t *inst = u32(k + ".instance_idx");
    const float *v = f32(k + ".scale_offset");   // per chart: scale_u, scale_v, offset_u, offset_v
    std::vector<lp::LightmapChart> c(rows(k + ".instance_idx", U32));
    for (size_t i = 0; i < c.size(); i++)
    {
        c[i].instance_idx = inst[i];
        c[i].scale_u = v[4 * i]; c[i].scale_v = v[4 * i + 1]; c[i].offset_u = v[4 * i + 2]; c[i].offset_v = v[4 * i + 3];
    }
    return c;
}
std::vector<LupinLightmapChart> charts_c(const std::vector<lp::LightmapChart> &c)
{
    std::vector<LupinLightmapChart> cc(c.size());
    for (size_t i = 0; i < c.size(); i++)
    {
        cc[i].instance_idx = c[i].instance_idx;
        cc[i].scale_u = c[i].scale_u; cc[i].scale_v = c[i].scale_v; cc[i].offset_u = c[i].offset_u; cc[i].offset_v = c[i].offset_v;
    }
    return cc;
}
lp::ProbeGridDesc probe_grid_desc(const std::string &k)
{
    lp::ProbeGridDesc g;
    g.origin = f3(k + ".origin"); g.spacing = f3(k + ".spacing"); g.dims = u3(k + ".dims");
    g.flags = U(k + ".flags"); g.ray_epsilon = F(k + ".ray_epsilon"); g.normal_bias = F(k + ".normal_bias");
    return g;
}
lp::ProbeDepthDesc probe_depth_desc(const std::string &k)
{
    lp::ProbeDepthDesc d;
    d.resolution = U(k + ".resolution"); d.subsamples = U(k + ".subsamples"); d.flags = U(k + ".flags"); d.max_slots = U(k + ".max_slots");
    d.ray_epsilon = F(k + ".ray_epsilon"); d.max_distance = F(k + ".max_distance");
    return d;
}
lp::BakedViewDesc baked_view_desc(const std::string &k)
{
    lp::BakedViewDesc v;
    const lp::CameraParams cp = camera_params(k + ".camera");
    v.camera_params.is_orthographic = cp.is_orthographic ? 1u : 0u;
    v.camera_params.lens = cp.lens; v.camera_params.film = cp.film; v.camera_params.aspect = cp.aspect; v.camera_params.focus = cp.focus;
    v.camera_params.aperture = cp.aperture;
    v.camera_transform = mat3x4(k + ".camera_transform");
    v.grid = probe_grid_desc(k + ".grid");
    v.resolution = U(k + ".resolution"); v.max_distance = F(k + ".max_distance"); v.ray_epsilon = F(k + ".ray_epsilon");
    v.ambient = f3(k + ".ambient"); v.flags = U(k + ".flags"); v.max_slots = U(k + ".max_slots");
    return v;
}
lp::OcclusionDesc occlusion_desc(const std::string &k)
{
    lp::OcclusionDesc d;
    d.mode = (lp::OcclusionMode)U(k + ".mode"); d.samples = U(k + ".samples"); d.flags = U(k + ".flags"); d.ray_epsilon = F(k + ".ray_epsilon");
    return d;
}

// the device, and the two scenes, made when a section first asks for them
struct World
{
    std::unique_ptr<lp::Device> device;
    std::unique_ptr<lp::Scene> cornell, fixture;
    lp::Device &dev()
    {
        if (!device) device.reset(new lp::Device(0));
        return *device;
    }
    lp::Scene &cornell_box()
    {
        if (!cornell) cornell.reset(new lp::Scene(lpl::build_scene_cornell_box(dev()).first));
        return *cornell;
    }
    lp::Scene &fixture_scene()   // texcoords on every mesh, one material of opacity 0.2
    {
        if (!fixture)
        {
            const Array &p = in.at("fixture.path", U8), &a = in.at("fixture.asset_dir", U8);
            fixture.reset(new lp::Scene(lpl::load_scene_yoctogl_v24(std::string(p.bytes.begin(), p.bytes.end()), dev(), true,
                                                                    {std::string(a.bytes.begin(), a.bytes.end())}).first));
        }
        return *fixture;
    }
} world;

// ---- the sections ----------------------------------------------------------------------------------------------

void section_tiles()
{
    const std::string k = "pathtrace_scene_tiles";
    lp::Device &d = world.dev();
    lp::PathtraceResources res = lp::build_pathtrace_resources(d, baked_params(k + ".baked"));
    // tile_size counts 4 x 4 pixel workgroups: `tile_size` covers the whole frame with one tile, `small_tile_size` cuts it into
    // a grid with edge tiles
    for (const char *which : {"tile_size", "small_tile_size"})
    {
        lp::DoubleBufferedTexture tex(d, U(k + ".width"), U(k + ".height"));
        lp::PathtraceDesc desc = pathtrace_desc(k + ".desc");
        desc.accum_params = lp::AccumulationParams{tex.back(), U(k + ".accum_counter")};
        lp::pathtrace_scene_tiles(d, res, world.cornell_box(), tex.front(), (lp::PathtraceType)U(k + ".pathtrace_type"), desc, U(k + "." + which), U(k + ".rank"),
                                  U(k + ".world"));
        put_texture(k + ".image." + which, tex.front());
    }
}

void falsecolor_into(lp::TextureRef target, uint32_t type)
{
    const std::string k = "pathtrace_scene_falsecolor";
    lp::PathtraceResources res = lp::build_pathtrace_resources(world.dev(), baked_params(k + ".baked"));
    lp::pathtrace_scene_falsecolor(world.dev(), res, world.cornell_box(), target, (lp::FalsecolorType)type, pathtrace_desc(k + ".desc"));
}

void section_falsecolor()
{
    const std::string k = "pathtrace_scene_falsecolor";
    lp::DoubleBufferedTexture tex(world.dev(), U(k + ".width"), U(k + ".height"));
    falsecolor_into(tex.front(), U(k + ".type_a"));
    falsecolor_into(tex.back(), U(k + ".type_b"));
    put_texture(k + ".image_a", tex.front());
    put_texture(k + ".image_b", tex.back());
}

void section_debug()
{
    const std::string k = "pathtrace_scene_debug";
    lp::Device &d = world.dev();
    lp::PathtraceResources res = lp::build_pathtrace_resources(d, baked_params(k + ".baked"));
    lp::DoubleBufferedTexture tex(d, U(k + ".width"), U(k + ".height"));
    lp::DebugVizDesc dd;
    dd.viz_type = (lp::DebugVizType)U(k + ".viz_type"); dd.heatmap_min = F(k + ".heatmap_min"); dd.heatmap_max = F(k + ".heatmap_max");
    dd.first_hit_only = U(k + ".first_hit_only") != 0;
    lp::pathtrace_scene_debug(d, res, world.cornell_box(), tex.front(), dd, pathtrace_desc(k + ".desc"));
    put_texture(k + ".image", tex.front());
}

void section_denoise()
{
    const std::string k = "denoise", fk = "pathtrace_scene_falsecolor";
    lp::Device &d = world.dev();
    const uint32_t W = U(fk + ".width"), H = U(fk + ".height");
    lp::PathtraceResources res = lp::build_pathtrace_resources(d, baked_params(k + ".baked"));
    lp::DoubleBufferedTexture color(d, W, H), guides(d, W, H), result(d, W, H);
    for (uint32_t f = 0; f < U(k + ".frames"); f++)
    {
        lp::PathtraceDesc desc = pathtrace_desc(k + ".desc");
        desc.accum_params = lp::AccumulationParams{color.back(), f};
        lp::pathtrace_scene(d, res, world.cornell_box(), color.front(), (lp::PathtraceType)U(k + ".pathtrace_type"), desc);
        color.flip();
    }
    color.flip();
    falsecolor_into(guides.front(), U(fk + ".type_a"));   // Albedo
    falsecolor_into(guides.back(), U(fk + ".type_b"));    // Normals
    lp::DenoiseResources dres = lp::build_denoise_resources(d, W, H);
    lp::DenoiseDesc dd;
    dd.pathtrace_output = color.front();
    dd.albedo = guides.front();
    dd.normals = guides.back();
    dd.denoise_output = result.front();
    dd.quality = (lp::DenoiseQuality)U(k + ".quality");
    lp::denoise(d, dres, dd);
    put_texture(k + ".noisy", color.front());
    put_texture(k + ".image", result.front());
}

void put_adaptive_state(const std::string &k, const lp::AdaptiveResources &ares, uint32_t W, uint32_t H)
{
    const uint32_t bx = (W + 7) / 8, by = (H + 7) / 8;
    std::vector<uint32_t> frames((size_t)W * H);
    std::vector<float> moments((size_t)W * H * 2), err((size_t)bx * by);
    std::vector<uint8_t> active((size_t)bx * by);
    ares.download(frames.data(), moments.data(), err.data(), active.data());
    put_u(k + ".frames", {H, W}, frames.data());
    put_f(k + ".moments", {H, W, 2}, moments.data());
    put_f(k + ".block_error", {by, bx}, err.data());
    out.put(k + ".block_active", U8, {by, bx}, active.data());
    const LupinAdaptiveStats s = ares.stats();
    const uint32_t words[4] = {(uint32_t)s.active_pixels, (uint32_t)s.pixel_frames, s.calls, s.max_frames_taken};
    put_u(k + ".stats", {4}, words);
}

// the first reprojection fixes the view, `calls` adaptive frames follow; with `reproject` the history then moves to the second view
void adaptive_sequence(const std::string &k, bool reproject)
{
    const std::string a = "pathtrace_scene_adaptive", r = "adaptive_reproject";
    lp::Device &d = world.dev();
    const uint32_t W = U(a + ".width"), H = U(a + ".height");
    lp::PathtraceResources res = lp::build_pathtrace_resources(d, baked_params(a + ".baked"));
    lp::AdaptiveResources ares = lp::build_adaptive_resources(d, W, H);
    lp::ReprojectResources rres = lp::build_reproject_resources(d, W, H);
    lp::DoubleBufferedTexture tex(d, W, H);
    lp::AdaptiveParams params;
    params.threshold = F(a + ".threshold"); params.min_frames = U(a + ".min_frames"); params.max_frames = U(a + ".max_frames");
    auto reproject_to = [&](const std::string &view) {
        lp::ReprojectDesc rd;
        rd.camera_params = camera_params(view + ".camera");
        rd.camera_transform = mat3x4(view + ".camera_transform");
        rd.ray_epsilon = F(r + ".ray_epsilon"); rd.depth_tolerance = F(r + ".depth_tolerance"); rd.max_history = U(r + ".max_history");
        const LupinMat4x3 *t = (const LupinMat4x3 *)f32(r + ".prev_instance_transforms");
        rd.prev_instance_transforms.assign(t, t + rows(r + ".prev_instance_transforms", F32));
        lp::adaptive_reproject(d, ares, rres, world.cornell_box(), rd, tex.back(), tex.front());
        tex.flip();
    };
    if (reproject) reproject_to(a + ".desc");
    for (uint32_t call = 0; call < U(a + ".calls"); call++)
    {
        lp::PathtraceDesc desc = pathtrace_desc(a + ".desc");
        desc.accum_params = lp::AccumulationParams{tex.back(), U(a + ".accum_counter")};
        lp::pathtrace_scene_adaptive(d, res, world.cornell_box(), tex.front(), (lp::PathtraceType)U(a + ".pathtrace_type"), desc, ares, params);
        tex.flip();
    }
    if (reproject)
    {
        reproject_to(r + ".view");
        std::vector<uint32_t> inst((size_t)W * H), tri((size_t)W * H);
        std::vector<float> uv((size_t)W * H * 2), depth((size_t)W * H);
        rres.download(0, inst.data(), tri.data(), uv.data(), depth.data());
        put_u(k + ".inst", {H, W}, inst.data());
        put_u(k + ".tri", {H, W}, tri.data());
        put_f(k + ".uv", {H, W, 2}, uv.data());
        put_f(k + ".depth", {H, W}, depth.data());
    }
    put_texture(k + ".image", tex.back());
    put_adaptive_state(k, ares, W, H);
}

void section_rays()
{
    const std::string k = "pathtrace_rays";
    const lp::RayQueryDesc desc = ray_query_desc(k + ".desc");
    const uint64_t n = rows(k + ".records", F32);
    std::vector<float> result(n * LUPIN_RAY_RESULT_FLOATS), rays(n * desc.samples * LUPIN_RAY_RECORD_FLOATS);
    lp::pathtrace_rays(world.dev(), world.cornell_box(), desc, n, f32(k + ".records"), result.data(), rays.data());
    put_f(k + ".out", {n, LUPIN_RAY_RESULT_FLOATS}, result.data());
    put_f(k + ".out_rays", {n * desc.samples, LUPIN_RAY_RECORD_FLOATS}, rays.data());
}

void section_rays_moments()
{
    const std::string k = "pathtrace_rays_moments";
    const uint64_t n = rows(k + ".records", F32);
    std::vector<float> result(n * LUPIN_RAY_MOMENTS_FLOATS);
    lp::pathtrace_rays_moments(world.dev(), world.cornell_box(), ray_query_desc(k + ".desc"), n, f32(k + ".records"), result.data());
    put_f(k + ".out", {n, LUPIN_RAY_MOMENTS_FLOATS}, result.data());
}

struct Baked { std::vector<float> rgba, records; uint64_t covered = 0; };
Baked bake_lightmap_of(const std::string &k)
{
    const lp::LightmapDesc desc = lightmap_desc(k + ".desc");
    const std::vector<lp::LightmapChart> c = charts(k + ".charts");
    Baked b;
    b.rgba.resize((size_t)desc.width * desc.height * 4);
    b.records.resize((size_t)desc.width * desc.height * LUPIN_RAY_RECORD_FLOATS);
    b.covered = lp::bake_lightmap(world.dev(), world.fixture_scene(), desc, c.data(), (uint32_t)c.size(), b.rgba.data(), b.records.data());
    return b;
}

void section_bake_lightmap()
{
    const std::string k = "bake_lightmap";
    const Baked b = bake_lightmap_of(k);
    const uint64_t W = U(k + ".desc.width"), H = U(k + ".desc.height");
    put_f(k + ".rgba", {H, W, 4}, b.rgba.data());
    put_f(k + ".records", {H, W, LUPIN_RAY_RECORD_FLOATS}, b.records.data());
    put_scalar(k + ".covered", (uint32_t)b.covered);
}

std::vector<float> bake_directional_of(const std::string &k, std::vector<float> *records, uint64_t *covered)
{
    const lp::LightmapDesc desc = lightmap_desc(k + ".desc");
    const std::vector<lp::LightmapChart> c = charts(k + ".charts");
    std::vector<float> sh((size_t)LUPIN_LIGHTMAP_DIRECTIONAL_PLANES * desc.width * desc.height * 4);
    records->resize((size_t)desc.width * desc.height * LUPIN_RAY_RECORD_FLOATS);
    *covered = lp::bake_lightmap_directional(world.dev(), world.fixture_scene(), desc, c.data(), (uint32_t)c.size(), sh.data(), records->data());
    return sh;
}

void section_bake_lightmap_directional()
{
    const std::string k = "bake_lightmap_directional";
    std::vector<float> records;
    uint64_t covered = 0;
    const std::vector<float> sh = bake_directional_of(k, &records, &covered);
    const uint64_t W = U(k + ".desc.width"), H = U(k + ".desc.height");
    put_f(k + ".sh", {LUPIN_LIGHTMAP_DIRECTIONAL_PLANES, H, W, 4}, sh.data());
    put_f(k + ".records", {H, W, LUPIN_RAY_RECORD_FLOATS}, records.data());
    put_scalar(k + ".covered", (uint32_t)covered);
}

void section_bake_lightmap_adaptive()
{
    const std::string k = "bake_lightmap_adaptive";
    const lp::LightmapDesc desc = lightmap_desc(k + ".desc");
    const std::vector<lp::LightmapChart> c = charts(k + ".charts");
    lp::LightmapAdaptiveDesc ad;
    ad.threshold = F(k + ".threshold"); ad.min_rounds = U(k + ".min_rounds"); ad.max_rounds = U(k + ".max_rounds");
    const uint64_t W = desc.width, H = desc.height;
    std::vector<float> rgba(W * H * 4), stats(W * H * LUPIN_LIGHTMAP_ADAPTIVE_STATS_FLOATS), records(W * H * LUPIN_RAY_RECORD_FLOATS);
    const uint64_t covered = lp::bake_lightmap_adaptive(world.dev(), world.fixture_scene(), desc, ad, c.data(), (uint32_t)c.size(), rgba.data(), stats.data(),
                                                        records.data());
    put_f(k + ".rgba", {H, W, 4}, rgba.data());
    put_f(k + ".stats", {H, W, LUPIN_LIGHTMAP_ADAPTIVE_STATS_FLOATS}, stats.data());
    put_f(k + ".records", {H, W, LUPIN_RAY_RECORD_FLOATS}, records.data());
    put_scalar(k + ".covered", (uint32_t)covered);
    const LupinLightmapAdaptiveStats s = lp::lightmap_adaptive_stats();
    const uint32_t totals[6] = {(uint32_t)s.covered_texels, (uint32_t)s.rounds, (uint32_t)s.paths, (uint32_t)s.converged_texels, (uint32_t)s.capped_texels,
                                (uint32_t)s.keys};
    put_u(k + ".totals", {6}, totals);
}

void section_bake_lightmap_ao()
{
    const std::string k = "bake_lightmap_ao";
    lp::LightmapAoDesc desc;
    desc.width = U(k + ".desc.width"); desc.height = U(k + ".desc.height"); desc.samples = U(k + ".desc.samples"); desc.max_slots = U(k + ".desc.max_slots");
    desc.flags = U(k + ".desc.flags"); desc.dilate = U(k + ".desc.dilate"); desc.counter = U(k + ".desc.counter");
    desc.surface_offset = F(k + ".desc.surface_offset"); desc.max_distance = F(k + ".desc.max_distance"); desc.ray_epsilon = F(k + ".desc.ray_epsilon");
    const std::vector<lp::LightmapChart> c = charts(k + ".charts");
    const uint64_t W = desc.width, H = desc.height;
    std::vector<float> ao(W * H * 4), bent(W * H * 4), records(W * H * LUPIN_RAY_RECORD_FLOATS);
    const uint64_t covered = lp::bake_lightmap_ao(world.dev(), world.fixture_scene(), desc, c.data(), (uint32_t)c.size(), ao.data(), bent.data(), records.data());
    put_f(k + ".ao", {H, W, 4}, ao.data());
    put_f(k + ".bent", {H, W, 4}, bent.data());
    put_f(k + ".records", {H, W, LUPIN_RAY_RECORD_FLOATS}, records.data());
    put_scalar(k + ".covered", (uint32_t)covered);
}

void section_denoise_lightmap()
{
    const std::string k = "denoise_lightmap";
    const Baked b = bake_lightmap_of("bake_lightmap");
    lp::LightmapDenoiseDesc desc;
    desc.width = U(k + ".width"); desc.height = U(k + ".height"); desc.passes = U(k + ".passes"); desc.normal_squarings = U(k + ".normal_squarings");
    desc.dilate = U(k + ".dilate"); desc.flags = U(k + ".flags"); desc.max_stretch = F(k + ".max_stretch");
    std::vector<float> result(b.rgba.size());
    lp::denoise_lightmap(world.dev(), desc, b.rgba.data(), b.records.data(), result.data());
    put_f(k + ".rgba", {desc.height, desc.width, 4}, result.data());
}

void section_bake_probes()
{
    const std::string k = "bake_probes";
    lp::ProbeDesc desc;
    desc.pathtrace_type = (lp::PathtraceType)U(k + ".desc.pathtrace_type"); desc.max_bounces = U(k + ".desc.max_bounces"); desc.samples = U(k + ".desc.samples");
    desc.flags = U(k + ".desc.flags"); desc.max_slots = U(k + ".desc.max_slots"); desc.advanced = advanced(k + ".desc.advanced");
    const uint64_t n = rows(k + ".probes", F32);
    std::vector<float> sh(n * LUPIN_PROBE_RESULT_FLOATS), rays(n * desc.samples * LUPIN_RAY_RECORD_FLOATS);
    lp::bake_probes(world.dev(), world.cornell_box(), desc, n, f32(k + ".probes"), sh.data(), rays.data());
    put_f(k + ".sh", {n, LUPIN_PROBE_SH_COEFFS, 4}, sh.data());
    put_f(k + ".rays", {n * desc.samples, LUPIN_RAY_RECORD_FLOATS}, rays.data());
}

void section_occlusion_rays()
{
    const std::string k = "occlusion_rays";
    const uint64_t n = rows(k + ".records", F32);
    std::vector<uint32_t> blocked(n);
    lp::occlusion_rays(world.dev(), world.cornell_box(), occlusion_desc(k + ".desc"), n, f32(k + ".records"), blocked.data());
    put_u(k + ".blocked", {n}, blocked.data());
}

void section_visible()
{
    const std::string k = "visible";
    const uint64_t n = rows(k + ".p", F32);
    const std::vector<uint8_t> v = lp::visible(world.dev(), world.cornell_box(), n, f32(k + ".p"), f32(k + ".q"), F(k + ".ray_epsilon"));
    out.put(k + ".visible", U8, {n}, v.data());
}

void section_ambient_occlusion()
{
    const std::string k = "ambient_occlusion";
    const uint64_t n = rows(k + ".origins", F32);
    const std::vector<float> ao = lp::ambient_occlusion(world.dev(), world.cornell_box(), n, f32(k + ".origins"), f32(k + ".normals"), u32(k + ".rng_words"),
                                                        F(k + ".radius"), U(k + ".samples"), F(k + ".ray_epsilon"));
    put_f(k + ".ao", {n}, ao.data());
}

void section_transmittance_rays()
{
    const std::string k = "transmittance_rays";
    const uint64_t n = rows(k + ".records", F32);
    std::vector<float> sum(n);
    lp::transmittance_rays(world.dev(), world.fixture_scene(), occlusion_desc(k + ".desc"), n, f32(k + ".records"), sum.data());
    put_f(k + ".sum", {n}, sum.data());
}

void section_transmittance()
{
    const std::string k = "transmittance";
    const uint64_t n = rows(k + ".p", F32);
    const std::vector<float> t = lp::transmittance(world.dev(), world.fixture_scene(), n, f32(k + ".p"), f32(k + ".q"), F(k + ".ray_epsilon"));
    put_f(k + ".t", {n}, t.data());
}

void section_bent_normal_rays()
{
    const std::string k = "bent_normal_rays";
    lp::BentNormalDesc desc;
    desc.samples = U(k + ".desc.samples"); desc.flags = U(k + ".desc.flags"); desc.max_slots = U(k + ".desc.max_slots"); desc.ray_epsilon = F(k + ".desc.ray_epsilon");
    const uint64_t n = rows(k + ".records", F32);
    std::vector<float> sums(n * LUPIN_BENT_NORMAL_RESULT_FLOATS);
    lp::bent_normal_rays(world.dev(), world.fixture_scene(), desc, n, f32(k + ".records"), sums.data());
    put_f(k + ".sums", {n, LUPIN_BENT_NORMAL_RESULT_FLOATS}, sums.data());
}

void section_distance_points()
{
    const std::string k = "distance_points";
    const uint64_t n = rows(k + ".records", F32);
    std::vector<lp::DistanceResult> r(n);
    lp::distance_points(world.dev(), world.cornell_box(), n, f32(k + ".records"), r.data(), U(k + ".flags"));
    std::vector<uint32_t> found(n), instance(n), tri(n);
    std::vector<float> distance(n), point(n * 3), u(n), v(n), side(n);
    for (uint64_t i = 0; i < n; i++)
    {
        found[i] = r[i].found; distance[i] = r[i].distance; u[i] = r[i].u; v[i] = r[i].v; instance[i] = r[i].instance; tri[i] = r[i].tri; side[i] = r[i].side;
        for (int c = 0; c < 3; c++) point[3 * i + c] = r[i].point[c];
    }
    put_u(k + ".found", {n}, found.data()); put_f(k + ".distance", {n}, distance.data()); put_f(k + ".point", {n, 3}, point.data());
    put_f(k + ".u", {n}, u.data()); put_f(k + ".v", {n}, v.data()); put_u(k + ".instance", {n}, instance.data()); put_u(k + ".tri", {n}, tri.data());
    put_f(k + ".side", {n}, side.data());
}

void section_bake_distance_grid()
{
    const std::string k = "bake_distance_grid";
    const std::array<uint32_t, 3> dims = u3(k + ".dims");
    for (int is_signed = 0; is_signed < 2; is_signed++)
    {
        const std::vector<float> g = lp::bake_distance_grid(world.dev(), world.cornell_box(), f3(k + ".origin"), f3(k + ".spacing"), dims, F(k + ".rmax"), is_signed != 0);
        if (g.size() != (size_t)dims[0] * dims[1] * dims[2]) throw std::runtime_error("bake_distance_grid sized its output wrongly");
        put_f(k + (is_signed ? ".signed" : ".unsigned"), {dims[2], dims[1], dims[0]}, g.data());
    }
}

void section_sample_probe_grid()
{
    const std::string k = "sample_probe_grid";
    const uint64_t n = rows(k + ".records", F32);
    std::vector<float> result(n * LUPIN_PROBE_GRID_RESULT_FLOATS);
    lp::sample_probe_grid(world.dev(), world.cornell_box(), probe_grid_desc(k + ".grid"), f32("volume.sh"), u8("volume.valid"), n, f32(k + ".records"), result.data());
    put_f(k + ".out", {n, LUPIN_PROBE_GRID_RESULT_FLOATS}, result.data());
}

// the grid's probes by the descriptor `desc_of` carries: bake_probe_depth's own, or view_depth's for the lookup and the view
std::vector<float> bake_probe_depth_of(std::vector<uint32_t> *stats, const std::string &desc_of = "bake_probe_depth")
{
    const std::string k = "bake_probe_depth";
    const lp::ProbeDepthDesc desc = probe_depth_desc(desc_of + ".desc");
    const uint64_t n = rows(k + ".positions", F32), side = desc.resolution + 2;
    std::vector<float> depth(n * side * side * 2);
    stats->resize(n * LUPIN_PROBE_DEPTH_STATS_WORDS);
    lp::bake_probe_depth(world.dev(), world.cornell_box(), desc, n, f32(k + ".positions"), depth.data(), stats->data());
    return depth;
}

void section_bake_probe_depth()
{
    const std::string k = "bake_probe_depth";
    std::vector<uint32_t> stats;
    const std::vector<float> depth = bake_probe_depth_of(&stats);
    const uint64_t n = rows(k + ".positions", F32), side = U(k + ".desc.resolution") + 2;
    put_f(k + ".depth", {n, side, side, 2}, depth.data());
    put_u(k + ".stats", {n, LUPIN_PROBE_DEPTH_STATS_WORDS}, stats.data());
}

void section_sample_probe_grid_depth()
{
    const std::string k = "sample_probe_grid_depth";
    std::vector<uint32_t> stats;
    const std::vector<float> depth = bake_probe_depth_of(&stats, "view_depth");
    const uint64_t n = rows(k + ".records", F32);
    std::vector<float> result(n * LUPIN_PROBE_GRID_RESULT_FLOATS);
    lp::sample_probe_grid_depth(world.dev(), world.cornell_box(), probe_grid_desc(k + ".grid"), U(k + ".resolution"), F(k + ".max_distance"), f32("volume.sh"),
                                depth.data(), u8("volume.valid"), n, f32(k + ".records"), result.data());
    put_f(k + ".out", {n, LUPIN_PROBE_GRID_RESULT_FLOATS}, result.data());
}

void section_baked_view_desc_c()   // no device: the words of the C descriptor
{
    const std::string k = "baked_view_desc_c";
    const LupinBakedViewDesc c = lp::baked_view_desc_c(baked_view_desc("render_baked.view"));
    static_assert(sizeof c % 4 == 0, "LupinBakedViewDesc is whole words");
    put_u(k + ".words", {sizeof c / 4}, (const uint32_t *)&c);
}

void section_render_baked()
{
    const std::string k = "render_baked";
    lp::Device &d = world.dev();
    std::vector<uint32_t> stats;
    const std::vector<float> depth = bake_probe_depth_of(&stats, "view_depth");
    const uint32_t W = U(k + ".width"), H = U(k + ".height");
    lp::DoubleBufferedTexture tex(d, W, H);
    std::vector<float> gbuffer((size_t)W * H * LUPIN_BAKED_VIEW_GBUFFER_FLOATS);
    lp::render_baked(d, world.cornell_box(), tex.front(), baked_view_desc(k + ".view"), f32("volume.sh"), depth.data(), u8("volume.valid"), gbuffer.data());
    put_texture(k + ".image", tex.front());
    put_f(k + ".gbuffer", {H, W, LUPIN_BAKED_VIEW_GBUFFER_FLOATS}, gbuffer.data());
}

void section_render_lightmapped()
{
    const std::string k = "render_lightmapped";
    lp::Device &d = world.dev();
    const Baked b = bake_lightmap_of("bake_lightmap");
    const uint32_t W = U(k + ".width"), H = U(k + ".height");
    lp::DoubleBufferedTexture tex(d, W, H);
    std::vector<float> gbuffer((size_t)W * H * LUPIN_LIGHTMAPPED_VIEW_GBUFFER_FLOATS);
    lp::render_lightmapped(d, world.fixture_scene(), tex.front(), baked_view_desc(k + ".view"), charts_c(charts("bake_lightmap.charts")), b.rgba.data(),
                           U(k + ".lightmap_width"), U(k + ".lightmap_height"), nullptr, nullptr, nullptr, gbuffer.data());
    put_texture(k + ".image", tex.front());
    put_f(k + ".gbuffer", {H, W, LUPIN_LIGHTMAPPED_VIEW_GBUFFER_FLOATS}, gbuffer.data());
}

void section_render_lightmapped_directional()
{
    const std::string k = "render_lightmapped_directional";
    lp::Device &d = world.dev();
    const Baked b = bake_lightmap_of("bake_lightmap_directional");
    std::vector<float> records;
    uint64_t covered = 0;
    const std::vector<float> planes = bake_directional_of("bake_lightmap_directional", &records, &covered);
    const uint32_t W = U(k + ".width"), H = U(k + ".height");
    lp::DoubleBufferedTexture tex(d, W, H);
    std::vector<float> gbuffer((size_t)W * H * LUPIN_LIGHTMAPPED_DIRECTIONAL_GBUFFER_FLOATS);
    lp::render_lightmapped_directional(d, world.fixture_scene(), tex.front(), baked_view_desc(k + ".view"), charts_c(charts("bake_lightmap_directional.charts")),
                                       b.rgba.data(), planes.data(), U(k + ".lightmap_width"), U(k + ".lightmap_height"), U(k + ".bake_flags"), nullptr, nullptr,
                                       nullptr, gbuffer.data());
    put_texture(k + ".image", tex.front());
    put_f(k + ".gbuffer", {H, W, LUPIN_LIGHTMAPPED_DIRECTIONAL_GBUFFER_FLOATS}, gbuffer.data());
}

void section_update_instances()   // a scene of its own: it is changed in place
{
    const std::string k = "update_instances";
    lp::Device &d = world.dev();
    lp::Scene scene = lpl::build_scene_cornell_box(d).first;
    const LupinMat4x3 *t = (const LupinMat4x3 *)f32(k + ".transforms");
    scene.update_instances(std::vector<LupinMat4x3>(t, t + rows(k + ".transforms", F32)), U(k + ".device_tlas") != 0);
    const uint64_t n = rows(k + ".records", F32);
    std::vector<lp::DistanceResult> r(n);
    lp::distance_points(d, scene, n, f32(k + ".records"), r.data(), 0);
    put_u(k + ".results", {n, LUPIN_DISTANCE_RESULT_FLOATS}, (const uint32_t *)r.data());
}

template <class Fn> uint32_t throws_invalid_argument(Fn fn)
{
    try { fn(); }
    catch (const std::invalid_argument &) { return 1; }
    return 0;
}
template <class Fn> uint32_t throws_error(Fn fn)
{
    try { fn(); }
    catch (const lp::Error &e) { return e.code == LUPIN_ERR_INVALID_ARGUMENT ? 1 : 2; }
    return 0;
}

void section_host_only()   // no device
{
    const std::string k = "host_only";
    const std::vector<float> pos = lp::probe_grid_positions(f3(k + ".grid.origin"), f3(k + ".grid.spacing"), u3(k + ".grid.dims"));
    put_f(k + ".probe_grid_positions", {pos.size() / 3, 3}, pos.data());

    const uint64_t n = rows(k + ".sh.normals", F32);
    const float *coeffs = f32(k + ".sh.coeffs"), *normals = f32(k + ".sh.normals");
    std::vector<float> e(n * 3);
    for (uint64_t i = 0; i < n; i++)
    {
        const std::array<float, 3> v = lp::sh_irradiance(coeffs + i * LUPIN_PROBE_RESULT_FLOATS, normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
        for (int c = 0; c < 3; c++) e[3 * i + c] = v[c];
    }
    put_f(k + ".sh_irradiance", {n, 3}, e.data());

    const uint32_t *tiles = u32(k + ".get_num_tiles");   // rows of (tile_size, width, height)
    std::vector<uint32_t> num(rows(k + ".get_num_tiles", U32));
    for (size_t i = 0; i < num.size(); i++) num[i] = lp::get_num_tiles(tiles[3 * i], tiles[3 * i + 1], tiles[3 * i + 2]);
    put_u(k + ".num_tiles", {num.size()}, num.data());

    // validate_scene: one triangle that is valid, and the same with each of its parts broken in turn
    auto triangle = [] {
        lp::SceneCPU s;
        s.mesh_infos.push_back(lp::default_mesh_info());
        s.verts_pos_array.push_back({{0, 0, 0, 0}, {1, 0, 0, 0}, {0, 1, 0, 0}});
        s.indices_array.push_back({0, 1, 2});
        s.materials.push_back(lp::default_material());
        lp::Instance inst = lp::default_instance();
        inst.mesh_idx = 0; inst.mat_idx = 0;
        s.instances.push_back(inst);
        return s;
    };
    std::vector<uint32_t> refused;
    { lp::SceneCPU s = triangle(); refused.push_back(throws_error([&] { lp::validate_scene(s, 0, 0); })); }                                 // valid: 0
    { lp::SceneCPU s = triangle(); s.indices_array[0][2] = 3; refused.push_back(throws_error([&] { lp::validate_scene(s, 0, 0); })); }      // index out of range
    { lp::SceneCPU s = triangle(); s.instances[0].mat_idx = 1; refused.push_back(throws_error([&] { lp::validate_scene(s, 0, 0); })); }     // no such material
    { lp::SceneCPU s = triangle(); s.materials[0].color_tex_idx = 0; refused.push_back(throws_error([&] { lp::validate_scene(s, 0, 0); })); }   // no such texture
    { lp::SceneCPU s = triangle(); refused.push_back(throws_error([&] { lp::validate_scene(s, 1, 0); })); }                                 // textures != samplers
    { lp::SceneCPU s = triangle(); s.mesh_infos[0].normals_buf_idx = 0; refused.push_back(throws_error([&] { lp::validate_scene(s, 0, 0); })); }   // no such normals
    put_u(k + ".validate_scene", {refused.size()}, refused.data());

    // the segments: the records word for word, and the refusal at exactly 2 * ray_epsilon before anything touches the device
    const float eps = F(k + ".segments.ray_epsilon");
    const uint64_t ns = rows(k + ".segments.p", F32);
    const std::vector<float> rec = lp::segment_records(ns, f32(k + ".segments.p"), f32(k + ".segments.q"), eps);
    put_f(k + ".segment_records", {ns, LUPIN_OCCLUSION_RECORD_FLOATS}, rec.data());
    const lp::Device no_device(nullptr);
    const lp::Scene no_scene;
    const float *sp = f32(k + ".short.p"), *sq = f32(k + ".short.q");
    const uint64_t nshort = rows(k + ".short.p", F32);
    const uint32_t short_refused[3] = {throws_invalid_argument([&] { lp::segment_records(nshort, sp, sq, eps); }),
                                       throws_invalid_argument([&] { lp::visible(no_device, no_scene, nshort, sp, sq, eps); }),
                                       throws_invalid_argument([&] { lp::transmittance(no_device, no_scene, nshort, sp, sq, eps); })};
    put_u(k + ".short_refused", {3}, short_refused);
}

void section_defaults()   // no device: every field of every default-constructed descriptor
{
    auto camera = [](const std::string &k, const lp::CameraParams &c) {
        put_scalar(k + ".is_orthographic", (uint32_t)c.is_orthographic); put_scalar(k + ".lens", c.lens); put_scalar(k + ".film", c.film);
        put_scalar(k + ".aspect", c.aspect); put_scalar(k + ".focus", c.focus); put_scalar(k + ".aperture", c.aperture);
    };
    auto adv = [](const std::string &k, const lp::AdvancedParams &a) {
        put_scalar(k + ".max_radiance", a.max_radiance); put_scalar(k + ".rng_seed", a.rng_seed); put_scalar(k + ".ray_epsilon", a.ray_epsilon);
    };
    auto grid = [](const std::string &k, const lp::ProbeGridDesc &g) {
        put_f(k + ".origin", {3}, g.origin.data()); put_f(k + ".spacing", {3}, g.spacing.data()); put_u(k + ".dims", {3}, g.dims.data());
        put_scalar(k + ".flags", g.flags); put_scalar(k + ".ray_epsilon", g.ray_epsilon); put_scalar(k + ".normal_bias", g.normal_bias);
    };
    { lp::BakedPathtraceParams p; put_scalar("BakedPathtraceParams.with_runtime_checks", (uint32_t)p.with_runtime_checks);
      put_scalar("BakedPathtraceParams.max_bounces", p.max_bounces); put_scalar("BakedPathtraceParams.samples_per_pixel", p.samples_per_pixel); }
    camera("CameraParams", lp::CameraParams());
    adv("AdvancedParams", lp::AdvancedParams());
    { lp::TileParams t; put_scalar("TileParams.tile_size", t.tile_size); put_scalar("TileParams.tile_idx", t.tile_idx); }
    { lp::PathtraceDesc d; put_scalar("PathtraceDesc.accum_params", (uint32_t)d.accum_params.has_value());
      put_scalar("PathtraceDesc.tile_params", (uint32_t)d.tile_params.has_value()); camera("PathtraceDesc.camera_params", d.camera_params);
      put_f("PathtraceDesc.camera_transform", {4, 3}, &d.camera_transform.m[0][0]); put_scalar("PathtraceDesc.force_software_bvh", (uint32_t)d.force_software_bvh);
      adv("PathtraceDesc.advanced", d.advanced); }
    { lp::DebugVizDesc d; put_scalar("DebugVizDesc.viz_type", (uint32_t)d.viz_type); put_scalar("DebugVizDesc.heatmap_min", d.heatmap_min);
      put_scalar("DebugVizDesc.heatmap_max", d.heatmap_max); put_scalar("DebugVizDesc.first_hit_only", (uint32_t)d.first_hit_only); }
    { lp::TonemapDesc d; put_scalar("TonemapDesc.viewport", (uint32_t)d.viewport.has_value()); put_scalar("TonemapDesc.exposure", d.exposure);
      put_scalar("TonemapDesc.filmic", (uint32_t)d.filmic); put_scalar("TonemapDesc.srgb", (uint32_t)d.srgb); put_scalar("TonemapDesc.clear", (uint32_t)d.clear); }
    { lp::Viewport v; put_scalar("Viewport.x", v.x); put_scalar("Viewport.y", v.y); put_scalar("Viewport.w", v.w); put_scalar("Viewport.h", v.h); }
    { lp::DenoiseDesc d; put_scalar("DenoiseDesc.albedo", (uint32_t)d.albedo.has_value()); put_scalar("DenoiseDesc.normals", (uint32_t)d.normals.has_value());
      put_scalar("DenoiseDesc.quality", (uint32_t)d.quality); }
    { lp::AdaptiveParams p; put_scalar("AdaptiveParams.threshold", p.threshold); put_scalar("AdaptiveParams.min_frames", p.min_frames);
      put_scalar("AdaptiveParams.max_frames", p.max_frames); }
    { lp::ReprojectDesc d; camera("ReprojectDesc.camera_params", d.camera_params); put_f("ReprojectDesc.camera_transform", {4, 3}, &d.camera_transform.m[0][0]);
      put_scalar("ReprojectDesc.ray_epsilon", d.ray_epsilon); put_scalar("ReprojectDesc.depth_tolerance", d.depth_tolerance);
      put_scalar("ReprojectDesc.max_history", d.max_history); put_scalar("ReprojectDesc.prev_instance_transforms", (uint32_t)d.prev_instance_transforms.size()); }
    { lp::RayQueryDesc d; put_scalar("RayQueryDesc.pathtrace_type", (uint32_t)d.pathtrace_type); put_scalar("RayQueryDesc.max_bounces", d.max_bounces);
      put_scalar("RayQueryDesc.samples", d.samples); put_scalar("RayQueryDesc.flags", d.flags); put_scalar("RayQueryDesc.max_slots", d.max_slots);
      adv("RayQueryDesc.advanced", d.advanced); }
    { lp::LightmapChart c; put_scalar("LightmapChart.instance_idx", c.instance_idx); put_scalar("LightmapChart.scale_u", c.scale_u);
      put_scalar("LightmapChart.scale_v", c.scale_v); put_scalar("LightmapChart.offset_u", c.offset_u); put_scalar("LightmapChart.offset_v", c.offset_v); }
    { lp::LightmapDesc d; put_scalar("LightmapDesc.width", d.width); put_scalar("LightmapDesc.height", d.height);
      put_scalar("LightmapDesc.pathtrace_type", (uint32_t)d.pathtrace_type); put_scalar("LightmapDesc.max_bounces", d.max_bounces);
      put_scalar("LightmapDesc.samples", d.samples); put_scalar("LightmapDesc.max_slots", d.max_slots); put_scalar("LightmapDesc.flags", d.flags);
      put_scalar("LightmapDesc.dilate", d.dilate); put_scalar("LightmapDesc.counter", d.counter); put_scalar("LightmapDesc.surface_offset", d.surface_offset);
      adv("LightmapDesc.advanced", d.advanced); }
    { lp::LightmapAdaptiveDesc d; put_scalar("LightmapAdaptiveDesc.threshold", d.threshold); put_scalar("LightmapAdaptiveDesc.min_rounds", d.min_rounds);
      put_scalar("LightmapAdaptiveDesc.max_rounds", d.max_rounds); }
    { lp::LightmapAoDesc d; put_scalar("LightmapAoDesc.width", d.width); put_scalar("LightmapAoDesc.height", d.height); put_scalar("LightmapAoDesc.samples", d.samples);
      put_scalar("LightmapAoDesc.max_slots", d.max_slots); put_scalar("LightmapAoDesc.flags", d.flags); put_scalar("LightmapAoDesc.dilate", d.dilate);
      put_scalar("LightmapAoDesc.counter", d.counter); put_scalar("LightmapAoDesc.surface_offset", d.surface_offset);
      put_scalar("LightmapAoDesc.max_distance", d.max_distance); put_scalar("LightmapAoDesc.ray_epsilon", d.ray_epsilon); }
    { lp::LightmapDenoiseDesc d; put_scalar("LightmapDenoiseDesc.width", d.width); put_scalar("LightmapDenoiseDesc.height", d.height);
      put_scalar("LightmapDenoiseDesc.passes", d.passes); put_scalar("LightmapDenoiseDesc.normal_squarings", d.normal_squarings);
      put_scalar("LightmapDenoiseDesc.dilate", d.dilate); put_scalar("LightmapDenoiseDesc.flags", d.flags); put_scalar("LightmapDenoiseDesc.max_stretch", d.max_stretch); }
    { lp::ProbeDesc d; put_scalar("ProbeDesc.pathtrace_type", (uint32_t)d.pathtrace_type); put_scalar("ProbeDesc.max_bounces", d.max_bounces);
      put_scalar("ProbeDesc.samples", d.samples); put_scalar("ProbeDesc.flags", d.flags); put_scalar("ProbeDesc.max_slots", d.max_slots);
      adv("ProbeDesc.advanced", d.advanced); }
    { lp::OcclusionDesc d; put_scalar("OcclusionDesc.mode", (uint32_t)d.mode); put_scalar("OcclusionDesc.samples", d.samples); put_scalar("OcclusionDesc.flags", d.flags);
      put_scalar("OcclusionDesc.ray_epsilon", d.ray_epsilon); }
    { lp::BentNormalDesc d; put_scalar("BentNormalDesc.samples", d.samples); put_scalar("BentNormalDesc.flags", d.flags); put_scalar("BentNormalDesc.max_slots", d.max_slots);
      put_scalar("BentNormalDesc.ray_epsilon", d.ray_epsilon); }
    grid("ProbeGridDesc", lp::ProbeGridDesc());
    { lp::ProbeDepthDesc d; put_scalar("ProbeDepthDesc.resolution", d.resolution); put_scalar("ProbeDepthDesc.subsamples", d.subsamples);
      put_scalar("ProbeDepthDesc.flags", d.flags); put_scalar("ProbeDepthDesc.max_slots", d.max_slots); put_scalar("ProbeDepthDesc.ray_epsilon", d.ray_epsilon);
      put_scalar("ProbeDepthDesc.max_distance", d.max_distance); }
    { lp::BakedViewDesc d; lp::CameraParams c; c.is_orthographic = d.camera_params.is_orthographic != 0; c.lens = d.camera_params.lens; c.film = d.camera_params.film;
      c.aspect = d.camera_params.aspect; c.focus = d.camera_params.focus; c.aperture = d.camera_params.aperture;
      camera("BakedViewDesc.camera_params", c); put_f("BakedViewDesc.camera_transform", {4, 3}, &d.camera_transform.m[0][0]); grid("BakedViewDesc.grid", d.grid);
      put_scalar("BakedViewDesc.resolution", d.resolution); put_scalar("BakedViewDesc.max_distance", d.max_distance); put_scalar("BakedViewDesc.ray_epsilon", d.ray_epsilon);
      put_f("BakedViewDesc.ambient", {3}, d.ambient.data()); put_scalar("BakedViewDesc.flags", d.flags); put_scalar("BakedViewDesc.max_slots", d.max_slots); }
}

struct Section { const char *name; const char *covers; std::function<void()> run; };
const std::vector<Section> SECTIONS = {
    {"host_only", "sh_irradiance probe_grid_positions get_num_tiles validate_scene segment_records visible transmittance", section_host_only},
    {"defaults", "", section_defaults},
    {"baked_view_desc_c", "baked_view_desc_c", section_baked_view_desc_c},
    {"pathtrace_scene_tiles", "pathtrace_scene_tiles", section_tiles},
    {"pathtrace_scene_falsecolor", "pathtrace_scene_falsecolor", section_falsecolor},
    {"pathtrace_scene_debug", "pathtrace_scene_debug", section_debug},
    {"denoise", "denoise build_denoise_resources", section_denoise},
    {"pathtrace_scene_adaptive", "pathtrace_scene_adaptive build_adaptive_resources", [] { adaptive_sequence("pathtrace_scene_adaptive", false); }},
    {"adaptive_reproject", "adaptive_reproject build_reproject_resources", [] { adaptive_sequence("adaptive_reproject", true); }},
    {"pathtrace_rays", "pathtrace_rays", section_rays},
    {"pathtrace_rays_moments", "pathtrace_rays_moments", section_rays_moments},
    {"bake_probes", "bake_probes", section_bake_probes},
    {"occlusion_rays", "occlusion_rays", section_occlusion_rays},
    {"visible", "visible segment_records", section_visible},
    {"ambient_occlusion", "ambient_occlusion", section_ambient_occlusion},
    {"bent_normal_rays", "bent_normal_rays", section_bent_normal_rays},
    {"distance_points", "distance_points", section_distance_points},
    {"bake_distance_grid", "bake_distance_grid", section_bake_distance_grid},
    {"sample_probe_grid", "sample_probe_grid", section_sample_probe_grid},
    {"bake_probe_depth", "bake_probe_depth", section_bake_probe_depth},
    {"sample_probe_grid_depth", "sample_probe_grid_depth", section_sample_probe_grid_depth},
    {"render_baked", "render_baked baked_view_desc_c", section_render_baked},
    {"update_instances", "update_instances", section_update_instances},
    {"transmittance_rays", "transmittance_rays", section_transmittance_rays},
    {"transmittance", "transmittance segment_records", section_transmittance},
    {"bake_lightmap", "bake_lightmap", section_bake_lightmap},
    {"bake_lightmap_directional", "bake_lightmap_directional", section_bake_lightmap_directional},
    {"bake_lightmap_adaptive", "bake_lightmap_adaptive lightmap_adaptive_stats", section_bake_lightmap_adaptive},
    {"bake_lightmap_ao", "bake_lightmap_ao", section_bake_lightmap_ao},
    {"denoise_lightmap", "denoise_lightmap", section_denoise_lightmap},
    {"render_lightmapped", "render_lightmapped", section_render_lightmapped},
    {"render_lightmapped_directional", "render_lightmapped_directional", section_render_lightmapped_directional},
};

}  // namespace

int main(int argc, char **argv)
{
    if (argc == 2 && std::string(argv[1]) == "--list")
    {
        for (const Section &s : SECTIONS) std::cout << s.name << ": " << s.covers << "\n";
        return 0;
    }
    if (argc < 3) { std::cerr << "usage: cpp_mirror_probe <inputs.bin> <outputs.bin> [section ...] | --list\n"; return 2; }
    std::string running = "reading the inputs";
    try
    {
        in = Blob::read(argv[1]);
        for (const Section &s : SECTIONS)
        {
            bool wanted = argc == 3;
            for (int i = 3; i < argc; i++) wanted = wanted || s.name == std::string(argv[i]);
            if (!wanted) continue;
            running = s.name;
            s.run();
            uint32_t done = 1;
            out.put(std::string("done.") + s.name, U32, {1}, &done);
        }
        for (int i = 3; i < argc; i++)
        {
            bool known = false;
            for (const Section &s : SECTIONS) known = known || s.name == std::string(argv[i]);
            if (!known) throw std::runtime_error(std::string("no section named ") + argv[i]);
        }
        running = "writing the outputs";
        world.fixture.reset(); world.cornell.reset(); world.device.reset();
        out.write(argv[2]);
    }
    catch (const std::exception &e)
    {
        std::cerr << "cpp_mirror_probe: " << running << ": " << e.what() << "\n";
        return 1;
    }
    return 0;
}
