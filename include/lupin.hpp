// lupin.hpp -- C++ host-side mirror of the reference's Rust call surface (crate `lupin_pt`, namespace `lp::`,
// and the parts of `lupin_loader`, `lpl::`, that the canonical example needs) on top of the C ABI in lupin_hip.h.
//
// Same names, defaults and error behaviour as the reference:
//   lp::BakedPathtraceParams / build_pathtrace_resources      lupin/src/renderer.rs:451-642
//   lp::PathtraceDesc, AccumulationParams, TileParams, CameraParams, AdvancedParams, PathtraceType
//                                                             renderer.rs:644-766
//   lp::pathtrace_scene                                       renderer.rs:768-842
//   lp::get_num_tiles                                         renderer.rs:675-681
//   lp::DoubleBufferedTexture                                 lupin/src/wgpu_utils.rs:279-348
//   lp::SceneCPU, validate_scene, build_accel_structures_and_upload   renderer.rs:62-76, data_structures.rs:696-928
//   lpl::build_scene_cornell_box, lpl::save_texture (.hdr)    lupin_loader/src/loader.rs:14-207, :1775-1879
//
// Where the reference panics (assert! / panic!), these throw lp::Error.  Header-only; link with -llupin_hip.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <array>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "lupin_hip.h"

namespace lp {

struct Error : std::runtime_error
{
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc)
{
    if (rc != LUPIN_OK) throw Error(rc, lupin_hip_last_error());
}

constexpr uint32_t SENTINEL_IDX = LUPIN_SENTINEL_IDX;
using Mat3x4 = LupinMat3x4;
using MeshInfo = LupinMeshInfo;
using Instance = LupinInstance;
using Material = LupinMaterial;
using Environment = LupinEnvironment;
using Light = LupinLight;
using AliasBin = LupinAliasBin;
using BvhNode = LupinBvhNode;
using TlasNode = LupinTlasNode;
struct Vec4 { float x = 0, y = 0, z = 0, w = 0; };

inline Mat3x4 mat3x4_identity() { return Mat3x4{{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 0, 0}}}; }
inline MeshInfo default_mesh_info() { return MeshInfo{SENTINEL_IDX, SENTINEL_IDX, SENTINEL_IDX}; }   // renderer.rs:102-113
inline Instance default_instance()
{
    Instance i{};
    i.transpose_inverse_transform = LupinMat4x3{{{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}}};
    return i;
}
inline Material default_material()   // renderer.rs:163-185
{
    Material m{};
    m.color[3] = 1.0f;
    m.ior = 1.5f;
    m.tr_depth = 0.01f;
    m.color_tex_idx = m.emission_tex_idx = m.roughness_tex_idx = m.scattering_tex_idx = m.normal_tex_idx = SENTINEL_IDX;
    return m;
}

enum class PathtraceType : uint32_t { Standard = 0, MIS = 1, Naive = 2, Direct = 3 };   // renderer.rs:711-729
enum class FalsecolorType : uint32_t { Albedo = 0, Normals, NormalsUnsigned, FrontFacing, Emission, Roughness, Metallic, Opacity, MatType, IsDelta, Instance, Tri };   // renderer.rs:843-870

struct BakedPathtraceParams   // renderer.rs:451-468
{
    bool with_runtime_checks = false;
    uint32_t max_bounces = 8;
    uint32_t samples_per_pixel = 5;
};
struct CameraParams   // renderer.rs:683-708
{
    bool is_orthographic = false;
    float lens = 0.050f, film = 0.036f, aspect = 1.5f, focus = 10000.0f, aperture = 0.0f;
};
struct AdvancedParams { float max_radiance = 100.0f; uint32_t rng_seed = 0; float ray_epsilon = 0.001f; };   // :731-749
struct TileParams { uint32_t tile_size = 100; uint32_t tile_idx = 0; };                                      // :651-670

inline uint32_t get_num_tiles(uint32_t tile_size, uint32_t width, uint32_t height) { return lupin_hip_get_num_tiles(tile_size, width, height); }

// ---- device objects (RAII over the opaque handles) ----

class Device   // the reference's (wgpu::Device, wgpu::Queue) pair
{
  public:
    explicit Device(int ordinal = 0) { check(lupin_hip_create_context(ordinal, &ctx_)); }
    // no context: what the host-side entry points and refusals need on a machine without a device; every device call fails
    explicit Device(std::nullptr_t) {}
    ~Device() { lupin_hip_destroy_context(ctx_); }
    Device(const Device &) = delete;
    Device &operator=(const Device &) = delete;
    LupinContext *raw() const { return ctx_; }
    void poll_wait() const { check(lupin_hip_sync(ctx_)); }   // device.poll(wait_indefinitely)
    // pathtracer.wgsl:275-289 re-quantises the running mean to f16 every frame (default, LUPIN_ACCUM_F16_RUNNING_AVERAGE);
    // LUPIN_ACCUM_F32 runs the same recurrence on an f32 shadow of each texture and stores the rounded f16 view
    void set_accumulation_mode(int mode) const { check(lupin_hip_set_accumulation_mode(ctx_, mode)); }
    // path state of every frame in flight allocated now instead of at each lane's first pathtrace call
    void reserve_path_state(uint64_t pixels, uint32_t max_bounces, uint32_t samples_per_pixel) const { check(lupin_hip_reserve_path_state(ctx_, pixels, max_bounces, samples_per_pixel)); }
    // calls per wavefront (1..16; 0 = by dispatch size, the default) and the hierarchy the tracer walks (LUPIN_TRAVERSAL_BINARY / _WIDE)
    void set_batch_frames(uint32_t frames) const { check(lupin_hip_set_batch_frames(ctx_, frames)); }
    void set_traversal(int mode) const { check(lupin_hip_set_traversal(ctx_, mode)); }
  private:
    LupinContext *ctx_ = nullptr;
};

class PathtraceResources
{
  public:
    PathtraceResources(const Device &d, const BakedPathtraceParams &p)
    {
        LupinBakedPathtraceParams c{};
        c.with_runtime_checks = p.with_runtime_checks ? 1u : 0u;
        c.max_bounces = p.max_bounces;
        c.samples_per_pixel = p.samples_per_pixel;
        check(lupin_hip_build_pathtrace_resources(d.raw(), &c, &res_));
    }
    ~PathtraceResources() { lupin_hip_destroy_pathtrace_resources(res_); }
    PathtraceResources(const PathtraceResources &) = delete;
    LupinPathtraceResources *raw() const { return res_; }
  private:
    LupinPathtraceResources *res_ = nullptr;
};
inline PathtraceResources build_pathtrace_resources(const Device &d, const BakedPathtraceParams &p) { return PathtraceResources(d, p); }

class TextureRef   // a borrowed Rgba16Float render target (wgpu::Texture)
{
  public:
    explicit TextureRef(LupinTexture *t = nullptr) : t_(t) {}
    LupinTexture *raw() const { return t_; }
    uint32_t width() const { return lupin_hip_texture_width(t_); }
    uint32_t height() const { return lupin_hip_texture_height(t_); }
    std::vector<uint16_t> download() const   // synchronises
    {
        std::vector<uint16_t> px((size_t)width() * height() * 4);
        check(lupin_hip_texture_download_rgba16f(t_, px.data()));
        return px;
    }
    std::vector<float> download_f32() const   // the f32 accumulator (LUPIN_ACCUM_F32 frames only)
    {
        std::vector<float> px((size_t)width() * height() * 4);
        check(lupin_hip_texture_download_rgba32f(t_, px.data()));
        return px;
    }
  private:
    LupinTexture *t_;
};

class DoubleBufferedTexture   // wgpu_utils.rs:279-348
{
  public:
    static DoubleBufferedTexture create(const Device &d, uint32_t width, uint32_t height) { return DoubleBufferedTexture(d, width, height); }
    DoubleBufferedTexture(const Device &d, uint32_t w, uint32_t h) { check(lupin_hip_dbuf_create(d.raw(), w, h, &t_)); }
    DoubleBufferedTexture(DoubleBufferedTexture &&o) noexcept : t_(o.t_) { o.t_ = nullptr; }
    DoubleBufferedTexture(const DoubleBufferedTexture &) = delete;
    ~DoubleBufferedTexture() { if (t_) lupin_hip_dbuf_destroy(t_); }
    TextureRef front() const { return TextureRef(lupin_hip_dbuf_front(t_)); }
    TextureRef back() const { return TextureRef(lupin_hip_dbuf_back(t_)); }
    void copy_front_to_back() { check(lupin_hip_dbuf_copy_front_to_back(t_)); }
    void flip() { lupin_hip_dbuf_flip(t_); }
    void resize(uint32_t w, uint32_t h) { check(lupin_hip_dbuf_resize(t_, w, h)); }
  private:
    LupinDoubleBufferedTexture *t_ = nullptr;
};

struct AccumulationParams { TextureRef prev_frame; uint32_t accum_counter = 0; };   // renderer.rs:644-649

struct PathtraceDesc   // renderer.rs:751-766
{
    std::optional<AccumulationParams> accum_params;
    std::optional<TileParams> tile_params;
    CameraParams camera_params;
    Mat3x4 camera_transform = mat3x4_identity();
    bool force_software_bvh = false;
    AdvancedParams advanced;
};

// ---- scene ----

struct TextureCPU { uint32_t width = 0, height = 0; uint32_t format = LUPIN_TEX_RGBA8_UNORM; std::vector<uint8_t> pixels; };
struct EnvMapInfo { std::vector<Vec4> data; uint32_t width = 0, height = 0; };   // data_structures.rs:13-19

struct SceneCPU   // renderer.rs:62-76
{
    std::vector<MeshInfo> mesh_infos;
    std::vector<std::vector<Vec4>> verts_pos_array, verts_normal_array, verts_color_array;
    std::vector<std::vector<float>> verts_texcoord_array;   // 2 floats per vertex
    std::vector<std::vector<uint32_t>> indices_array;
    std::vector<Instance> instances;
    std::vector<Material> materials;
    std::vector<Environment> environments;
};

inline void validate_scene(const SceneCPU &s, uint32_t num_textures, uint32_t num_samplers)   // data_structures.rs:876-928
{
    auto require = [](bool ok, const char *what) { if (!ok) throw Error(LUPIN_ERR_INVALID_ARGUMENT, std::string("validate_scene: ") + what); };
    require(s.verts_pos_array.size() == s.mesh_infos.size(), "verts_pos_array / mesh_infos size mismatch");
    require(num_textures == num_samplers, "textures / samplers mismatch");
    for (size_t i = 0; i < s.mesh_infos.size(); i++)
    {
        const MeshInfo &m = s.mesh_infos[i];
        if (m.normals_buf_idx != SENTINEL_IDX) require(m.normals_buf_idx < s.verts_normal_array.size() && s.verts_normal_array[m.normals_buf_idx].size() == s.verts_pos_array[i].size(), "normals");
        if (m.texcoords_buf_idx != SENTINEL_IDX) require(m.texcoords_buf_idx < s.verts_texcoord_array.size() && s.verts_texcoord_array[m.texcoords_buf_idx].size() == 2 * s.verts_pos_array[i].size(), "texcoords");
        if (m.colors_buf_idx != SENTINEL_IDX) require(m.colors_buf_idx < s.verts_color_array.size() && s.verts_color_array[m.colors_buf_idx].size() == s.verts_pos_array[i].size(), "colors");
    }
    for (size_t i = 0; i < s.indices_array.size(); i++)
        for (uint32_t idx : s.indices_array[i]) require(idx < s.verts_pos_array[i].size(), "vertex index out of range");
    for (const Instance &in : s.instances) require(in.mesh_idx < s.mesh_infos.size() && in.mat_idx < s.materials.size(), "instance indices");
    auto tex_ok = [&](uint32_t t) { return t == SENTINEL_IDX || t < num_textures; };
    for (const Material &m : s.materials) require(tex_ok(m.color_tex_idx) && tex_ok(m.emission_tex_idx) && tex_ok(m.roughness_tex_idx) && tex_ok(m.scattering_tex_idx) && tex_ok(m.normal_tex_idx), "material texture index");
    for (const Environment &e : s.environments) require(e.emission[0] >= 0 && e.emission[1] >= 0 && e.emission[2] >= 0 && tex_ok(e.emission_tex_idx), "environment");
}

class Scene   // lp::Scene, software-BVH configuration (renderer.rs:17-60)
{
  public:
    Scene() = default;
    Scene(Scene &&o) noexcept : scene_(o.scene_) { o.scene_ = nullptr; }
    Scene(const Scene &) = delete;
    ~Scene() { if (scene_) lupin_hip_scene_destroy(scene_); }
    LupinScene *raw() const { return scene_; }
    // Moves the instances in place (lupin_hip_scene_update_instances): one transpose_inverse_transform per instance, in
    // instance order; the TLAS is rebuilt on the device (or by lupin_build_tlas), nothing else is uploaded again.
    void update_instances(const std::vector<LupinMat4x3> &transpose_inverse_transforms, bool device_tlas = true)
    {
        check(lupin_hip_scene_update_instances(scene_, transpose_inverse_transforms.data(), (uint32_t)transpose_inverse_transforms.size(), device_tlas ? 1 : 0));
    }
    // Gives a mesh a lightmap UV set (lupin_hip_scene_set_lightmap_uvs): one (u, v) per triangle corner in the
    // scene's own triangle order, 6 floats a triangle; nullptr removes it.  lp::unwrap_lightmap_uvs (lupin_unwrap.hpp) makes one.
    void set_lightmap_uvs(uint32_t mesh_idx, const float *uvs, uint64_t num_corners) { check(lupin_hip_scene_set_lightmap_uvs(scene_, mesh_idx, uvs, num_corners)); }
    LupinScene *scene_ = nullptr;
};

// Which builder produces the BLASes: the reference's CPU builder restated (lupin_build_bvh) or the same tree built on the GPU.
enum class BlasBuilder { Cpu, Device };

// lp::build_accel_structures_and_upload (data_structures.rs:696-872): BLAS over a clone of each index buffer,
// TLAS over the instances, lights + alias tables from the ORIGINAL triangle order, then upload.
inline Scene build_accel_structures_and_upload(const Device &d, const SceneCPU &s, const std::vector<TextureCPU> &textures,
                                               const std::vector<EnvMapInfo> &envs_info, bool /*build_sw_and_hw*/ = true,
                                               BlasBuilder blas_builder = BlasBuilder::Cpu)
{
    if (s.environments.size() != envs_info.size()) throw Error(LUPIN_ERR_INVALID_ARGUMENT, "Mismatching sizes for environment data!");
    const size_t nm = s.verts_pos_array.size();
    std::vector<std::vector<uint32_t>> reordered(nm);
    std::vector<std::vector<BvhNode>> bvhs(nm);
    std::vector<float> aabbs(nm * 6);
    std::vector<LupinMeshDesc> meshes(nm);
    for (size_t m = 0; m < nm; m++)
    {
        const auto &v = s.verts_pos_array[m];
        reordered[m] = s.indices_array[m];
        const float *vp = v.empty() ? nullptr : &v[0].x;
        static const float dummy[4] = {0, 0, 0, 0};
        if (!vp) vp = dummy;
        // 2 * triangles - 1 nodes always suffice; BlasBuilder::Device builds the same tree on the GPU (csrc/sahbvh.hip)
        const size_t num_tris = reordered[m].size() / 3;
        bvhs[m].resize(num_tris ? 2 * num_tris - 1 : 1);
        const bool on_device = blas_builder == BlasBuilder::Device && num_tris >= 64;
        const int64_t n = on_device
            ? lupin_hip_build_bvh_sah_device(d.raw(), vp, (uint32_t)v.size(), reordered[m].data(), (uint32_t)reordered[m].size(), bvhs[m].data(), (uint64_t)bvhs[m].size())
            : lupin_build_bvh(vp, (uint32_t)v.size(), reordered[m].data(), (uint32_t)reordered[m].size(), bvhs[m].data(), (uint64_t)bvhs[m].size());
        if (n < 0) throw Error((int)n, "build_bvh failed");
        bvhs[m].resize((size_t)n);
        float lo[3] = {3.402823466e38f, 3.402823466e38f, 3.402823466e38f}, hi[3] = {-3.402823466e38f, -3.402823466e38f, -3.402823466e38f};
        for (const Vec4 &p : v) { lo[0] = std::fmin(lo[0], p.x); lo[1] = std::fmin(lo[1], p.y); lo[2] = std::fmin(lo[2], p.z); hi[0] = std::fmax(hi[0], p.x); hi[1] = std::fmax(hi[1], p.y); hi[2] = std::fmax(hi[2], p.z); }
        for (int k = 0; k < 3; k++) { aabbs[m * 6 + k] = lo[k]; aabbs[m * 6 + 3 + k] = hi[k]; }
        meshes[m] = LupinMeshDesc{vp, (uint32_t)v.size(), reordered[m].data(), (uint32_t)reordered[m].size(), bvhs[m].data(), (uint32_t)bvhs[m].size()};
    }
    std::vector<TlasNode> tlas(2 * s.instances.size() + 1);
    int64_t nt = lupin_build_tlas(s.instances.data(), (uint32_t)s.instances.size(), aabbs.data(), (uint32_t)nm, tlas.data());
    if (nt < 0) throw Error((int)nt, "build_tlas failed");
    tlas.resize((size_t)nt);

    // build_lights (data_structures.rs:20-113)
    std::vector<Light> lights;
    std::vector<std::vector<AliasBin>> alias_tables, env_alias_tables;
    for (size_t i = 0; i < s.instances.size(); i++)
    {
        const Instance &in = s.instances[i];
        const Material &mat = s.materials[in.mat_idx];
        const auto &idx = s.indices_array[in.mesh_idx];
        if (mat.emission[0] == 0 && mat.emission[1] == 0 && mat.emission[2] == 0 && mat.emission[3] == 0) continue;
        if (idx.empty()) continue;
        std::vector<float> w(idx.size() / 3);
        float total = lupin_mesh_light_weights(&s.verts_pos_array[in.mesh_idx][0].x, idx.data(), (uint32_t)idx.size(), w.data());
        if (total <= 0.0f) continue;
        std::vector<AliasBin> bins(w.size());
        int64_t nb = lupin_build_alias_table(w.data(), w.size(), bins.data());
        bins.resize((size_t)std::max<int64_t>(nb, 0));
        if (bins.empty()) continue;
        lights.push_back(Light{(uint32_t)i, total});
        alias_tables.push_back(std::move(bins));
    }
    for (size_t i = 0; i < s.environments.size(); i++)
    {
        const EnvMapInfo &e = envs_info[i];
        std::vector<float> w((size_t)e.width * e.height);
        lupin_env_light_weights(&e.data[0].x, e.width, e.height, s.environments[i].emission, w.data());
        std::vector<AliasBin> bins(w.size());
        int64_t nb = lupin_build_alias_table(w.data(), w.size(), bins.data());
        bins.resize((size_t)std::max<int64_t>(nb, 0));
        env_alias_tables.push_back(std::move(bins));
    }

    auto vbufs = [](const std::vector<std::vector<Vec4>> &a) {
        std::vector<LupinVertexBufferDesc> out;
        for (const auto &v : a) out.push_back(LupinVertexBufferDesc{v.empty() ? nullptr : &v[0].x, (uint32_t)v.size()});
        return out;
    };
    std::vector<LupinVertexBufferDesc> nrm = vbufs(s.verts_normal_array), col = vbufs(s.verts_color_array), uvs;
    for (const auto &v : s.verts_texcoord_array) uvs.push_back(LupinVertexBufferDesc{v.data(), (uint32_t)(v.size() / 2)});
    std::vector<LupinTextureDesc> tex;
    for (const TextureCPU &t : textures) tex.push_back(LupinTextureDesc{t.width, t.height, t.format, t.pixels.data()});
    std::vector<LupinAliasTableDesc> at, eat;
    for (const auto &t : alias_tables) at.push_back(LupinAliasTableDesc{t.data(), (uint32_t)t.size()});
    for (const auto &t : env_alias_tables) eat.push_back(LupinAliasTableDesc{t.data(), (uint32_t)t.size()});

    LupinSceneDesc desc{};
    desc.mesh_infos = s.mesh_infos.data(); desc.meshes = meshes.data(); desc.num_meshes = (uint32_t)nm;
    desc.verts_normal_array = nrm.data(); desc.num_normal_buffers = (uint32_t)nrm.size();
    desc.verts_texcoord_array = uvs.data(); desc.num_texcoord_buffers = (uint32_t)uvs.size();
    desc.verts_color_array = col.data(); desc.num_color_buffers = (uint32_t)col.size();
    desc.instances = s.instances.data(); desc.num_instances = (uint32_t)s.instances.size();
    desc.materials = s.materials.data(); desc.num_materials = (uint32_t)s.materials.size();
    desc.textures = tex.data(); desc.num_textures = (uint32_t)tex.size();
    desc.environments = s.environments.data(); desc.num_environments = (uint32_t)s.environments.size();
    desc.tlas_nodes = tlas.data(); desc.num_tlas_nodes = (uint32_t)tlas.size();
    desc.lights = lights.data(); desc.num_lights = (uint32_t)lights.size();
    desc.alias_tables = at.data(); desc.env_alias_tables = eat.data();
    Scene out;
    check(lupin_hip_scene_create(d.raw(), &desc, &out.scene_));
    return out;
}

// The C descriptors are filled member by member, by name: their fields are mostly uint32_t, and a positional initialiser
// that falls out of step with include/lupin_hip.h would still compile.
namespace detail {
inline LupinCameraParams camera_params_c(const CameraParams &p)
{
    LupinCameraParams c{};
    c.is_orthographic = p.is_orthographic ? 1u : 0u;
    c.lens = p.lens; c.film = p.film; c.aspect = p.aspect; c.focus = p.focus; c.aperture = p.aperture;
    return c;
}
inline LupinAdvancedParams advanced_c(const AdvancedParams &a)
{
    LupinAdvancedParams c{};
    c.max_radiance = a.max_radiance; c.rng_seed = a.rng_seed; c.ray_epsilon = a.ray_epsilon;
    return c;
}
inline void fill_desc(const PathtraceDesc &desc, LupinAccumulationParams &ap, LupinTileParams &tp, LupinPathtraceDesc &c)
{
    if (desc.accum_params) { ap.prev_frame = desc.accum_params->prev_frame.raw(); ap.accum_counter = desc.accum_params->accum_counter; c.accum_params = &ap; }
    if (desc.tile_params) { tp.tile_size = desc.tile_params->tile_size; tp.tile_idx = desc.tile_params->tile_idx; c.tile_params = &tp; }
    c.camera_params = camera_params_c(desc.camera_params);
    c.camera_transform = desc.camera_transform;
    c.force_software_bvh = desc.force_software_bvh ? 1u : 0u;
    c.advanced = advanced_c(desc.advanced);
}
}  // namespace detail

// lp::pathtrace_scene (renderer.rs:768-842): enqueues one accumulation frame (or one tile) and returns.
inline void pathtrace_scene(const Device &d, const PathtraceResources &res, const Scene &scene, TextureRef render_target,
                            PathtraceType type, const PathtraceDesc &desc)
{
    LupinAccumulationParams ap{};
    LupinTileParams tp{};
    LupinPathtraceDesc c{};
    detail::fill_desc(desc, ap, tp, c);
    check(lupin_hip_pathtrace_scene(d.raw(), res.raw(), scene.raw(), render_target.raw(), (uint32_t)type, &c));
}

// ---- multi-GPU extension (no counterpart in the reference, which is single-device; tile mathematics renderer.rs:807-829) ----

// All tiles of the frame owned by `rank` (include/lupin_tiles.h) in one launch; desc.tile_params is ignored.
inline void pathtrace_scene_tiles(const Device &d, const PathtraceResources &res, const Scene &scene, TextureRef render_target,
                                  PathtraceType type, const PathtraceDesc &desc, uint32_t tile_size, uint32_t rank, uint32_t world)
{
    LupinAccumulationParams ap{};
    LupinTileParams tp{};
    LupinPathtraceDesc c{};
    detail::fill_desc(desc, ap, tp, c);
    check(lupin_hip_pathtrace_scene_tiles(d.raw(), res.raw(), scene.raw(), render_target.raw(), (uint32_t)type, &c, tile_size, rank, world));
}

// RCCL communicator of one Device; gather_framebuffer = pack own tiles -> ncclAllGather -> scatter the others' tiles.
class Comm
{
  public:
    static std::array<uint8_t, LUPIN_COMM_ID_BYTES> unique_id() { std::array<uint8_t, LUPIN_COMM_ID_BYTES> id{}; check(lupin_hip_comm_get_unique_id(id.data())); return id; }
    Comm(const Device &d, const std::array<uint8_t, LUPIN_COMM_ID_BYTES> &id, uint32_t rank, uint32_t world) { check(lupin_hip_comm_init_rank(d.raw(), id.data(), rank, world, &c_)); }
    explicit Comm(LupinComm *adopted) : c_(adopted) {}
    Comm(Comm &&o) noexcept : c_(o.c_) { o.c_ = nullptr; }
    Comm(const Comm &) = delete;
    ~Comm() { if (c_) lupin_hip_comm_destroy(c_); }
    // one process driving several devices (one context per GPU)
    static std::vector<Comm> init_all(const std::vector<const Device *> &devices)
    {
        std::vector<LupinContext *> ctxs;
        for (const Device *d : devices) ctxs.push_back(d->raw());
        std::vector<LupinComm *> raw(devices.size(), nullptr);
        check(lupin_hip_comm_init_all(ctxs.data(), (uint32_t)ctxs.size(), raw.data()));
        std::vector<Comm> out;
        for (LupinComm *c : raw) out.emplace_back(c);
        return out;
    }
    void gather_framebuffer(TextureRef tex, uint32_t tile_size) const { check(lupin_hip_gather_framebuffer(c_, tex.raw(), tile_size)); }
    // readback form: only `root` receives the other ranks' tiles
    void gather_framebuffer_to(TextureRef tex, uint32_t tile_size, uint32_t root) const { check(lupin_hip_gather_framebuffer_to(c_, tex.raw(), tile_size, root)); }
    void barrier() const { check(lupin_hip_comm_barrier(c_)); }
    uint32_t rank() const { return lupin_hip_comm_rank(c_); }
    uint32_t world() const { return lupin_hip_comm_world(c_); }
    LupinComm *raw() const { return c_; }
  private:
    LupinComm *c_ = nullptr;
};
inline void gather_framebuffer_all(const std::vector<Comm> &comms, const std::vector<TextureRef> &texs, uint32_t tile_size)
{
    std::vector<LupinComm *> c;
    std::vector<LupinTexture *> t;
    for (const Comm &x : comms) c.push_back(x.raw());
    for (const TextureRef &x : texs) t.push_back(x.raw());
    check(lupin_hip_gather_framebuffer_all(c.data(), t.data(), (uint32_t)c.size(), tile_size));
}

// lp::pathtrace_scene_falsecolor (renderer.rs:872-948)
inline void pathtrace_scene_falsecolor(const Device &d, const PathtraceResources &res, const Scene &scene, TextureRef render_target,
                                       FalsecolorType type, const PathtraceDesc &desc)
{
    LupinAccumulationParams ap{};
    LupinTileParams tp{};
    LupinPathtraceDesc c{};
    detail::fill_desc(desc, ap, tp, c);
    check(lupin_hip_pathtrace_scene_falsecolor(d.raw(), res.raw(), scene.raw(), render_target.raw(), (uint32_t)type, &c));
}

// lp::DebugVizType / DebugVizDesc / pathtrace_scene_debug (renderer.rs:950-1041)
enum class DebugVizType : uint32_t { BVHAABBChecks = 0, BVHTriChecks = 1, NumBounces = 2 };
struct DebugVizDesc { DebugVizType viz_type = DebugVizType::BVHAABBChecks; float heatmap_min = 0.0f, heatmap_max = 100.0f; bool first_hit_only = false; };
inline void pathtrace_scene_debug(const Device &d, const PathtraceResources &res, const Scene &scene, TextureRef render_target,
                                  const DebugVizDesc &debug_desc, const PathtraceDesc &desc)
{
    LupinAccumulationParams ap{};
    LupinTileParams tp{};
    LupinPathtraceDesc c{};
    detail::fill_desc(desc, ap, tp, c);
    LupinDebugVizDesc dd{};
    dd.viz_type = (uint32_t)debug_desc.viz_type;
    dd.heatmap_min = debug_desc.heatmap_min;
    dd.heatmap_max = debug_desc.heatmap_max;
    dd.first_hit_only = debug_desc.first_hit_only ? 1u : 0u;
    check(lupin_hip_pathtrace_scene_debug(d.raw(), res.raw(), scene.raw(), render_target.raw(), &dd, &c));
}

// lp::Viewport / TonemapDesc / tonemap_and_fit_aspect (tonemapping.rs:106-224); the Rgba8Unorm target is a host image
struct Viewport { float x = 0, y = 0, w = 0, h = 0; };
struct TonemapDesc { std::optional<Viewport> viewport; float exposure = 0.0f; bool filmic = false; bool srgb = true; bool clear = true; };
inline void tonemap_and_fit_aspect(const Device &d, TextureRef src, std::vector<uint8_t> &dst_rgba8, uint32_t dst_width, uint32_t dst_height,
                                   const TonemapDesc &desc = TonemapDesc())
{
    dst_rgba8.resize((size_t)dst_width * dst_height * 4);
    LupinTonemapDesc c{};
    if (desc.viewport) { c.has_viewport = 1; c.viewport_x = desc.viewport->x; c.viewport_y = desc.viewport->y; c.viewport_w = desc.viewport->w; c.viewport_h = desc.viewport->h; }
    c.exposure = desc.exposure; c.filmic = desc.filmic ? 1u : 0u; c.srgb = desc.srgb ? 1u : 0u; c.clear = desc.clear ? 1u : 0u;
    check(lupin_hip_tonemap_and_fit_aspect(d.raw(), src.raw(), dst_rgba8.data(), dst_width, dst_height, &c));
}

// lp::DenoiseResources / build_denoise_resources / DenoiseQuality / DenoiseDesc / denoise (denoising.rs:56-306): the
// filter is the library's own a-trous denoiser, not OIDN; the Device plays the role of the DenoiseDevice
class DenoiseResources
{
  public:
    DenoiseResources(const Device &d, uint32_t width, uint32_t height) { check(lupin_hip_build_denoise_resources(d.raw(), width, height, &res_)); }
    DenoiseResources(DenoiseResources &&o) noexcept : res_(o.res_) { o.res_ = nullptr; }
    DenoiseResources(const DenoiseResources &) = delete;
    ~DenoiseResources() { if (res_) lupin_hip_destroy_denoise_resources(res_); }
    LupinDenoiseResources *raw() const { return res_; }
  private:
    LupinDenoiseResources *res_ = nullptr;
};
inline DenoiseResources build_denoise_resources(const Device &d, uint32_t width, uint32_t height) { return DenoiseResources(d, width, height); }
enum class DenoiseQuality : uint32_t { Low = LUPIN_DENOISE_LOW, Medium = LUPIN_DENOISE_MEDIUM, High = LUPIN_DENOISE_HIGH };
struct DenoiseDesc
{
    TextureRef pathtrace_output;
    std::optional<TextureRef> albedo;
    std::optional<TextureRef> normals;
    TextureRef denoise_output;   // may be pathtrace_output: in place
    DenoiseQuality quality = DenoiseQuality::High;
};
inline void denoise(const Device &d, DenoiseResources &res, const DenoiseDesc &desc)
{
    LupinDenoiseDesc c{};
    c.pathtrace_output = desc.pathtrace_output.raw();
    c.albedo = desc.albedo ? desc.albedo->raw() : nullptr;
    c.normals = desc.normals ? desc.normals->raw() : nullptr;
    c.denoise_output = desc.denoise_output.raw();
    c.quality = (uint32_t)desc.quality;
    check(lupin_hip_denoise(d.raw(), res.raw(), &c));
}

// Adaptive sampling (no reference counterpart): renders only the 8x8 blocks that have not converged
struct AdaptiveParams
{
    float threshold = 0.01f;   // relative standard error of the mean a block must fall below; 0 = never converge
    uint32_t min_frames = 8;
    uint32_t max_frames = 0;   // 0 = no cap
};
class AdaptiveResources
{
  public:
    AdaptiveResources(const Device &d, uint32_t width, uint32_t height) : ctx_(d.raw()) { check(lupin_hip_build_adaptive_resources(ctx_, width, height, &res_)); }
    AdaptiveResources(AdaptiveResources &&o) noexcept : ctx_(o.ctx_), res_(o.res_) { o.res_ = nullptr; }
    AdaptiveResources(const AdaptiveResources &) = delete;
    ~AdaptiveResources() { if (res_) lupin_hip_destroy_adaptive_resources(res_); }
    LupinAdaptiveResources *raw() const { return res_; }
    // where accum_counter goes back to 0 (camera or scene changed)
    void reset() { check(lupin_hip_adaptive_reset(ctx_, res_)); }
    LupinAdaptiveStats stats() const { LupinAdaptiveStats s{}; check(lupin_hip_adaptive_stats(ctx_, res_, &s)); return s; }
    // any pointer may be null; frames W*H, moments W*H*2 (mean, M2), block_error / block_active ceil(W/8)*ceil(H/8)
    void download(uint32_t *frames, float *moments, float *block_error, uint8_t *block_active) const
    {
        check(lupin_hip_adaptive_download(ctx_, res_, frames, moments, block_error, block_active));
    }
  private:
    LupinContext *ctx_ = nullptr;
    LupinAdaptiveResources *res_ = nullptr;
};
inline AdaptiveResources build_adaptive_resources(const Device &d, uint32_t width, uint32_t height) { return AdaptiveResources(d, width, height); }
// desc.accum_params (with its prev_frame) is required; desc.tile_params must be empty
inline void pathtrace_scene_adaptive(const Device &d, const PathtraceResources &res, const Scene &scene, TextureRef render_target,
                                     PathtraceType type, const PathtraceDesc &desc, AdaptiveResources &ares, const AdaptiveParams &params = {})
{
    LupinAccumulationParams ap{};
    LupinTileParams tp{};
    LupinPathtraceDesc c{};
    detail::fill_desc(desc, ap, tp, c);
    LupinAdaptiveParams p{};
    p.threshold = params.threshold;
    p.min_frames = params.min_frames;
    p.max_frames = params.max_frames;
    check(lupin_hip_pathtrace_scene_adaptive(d.raw(), res.raw(), scene.raw(), render_target.raw(), (uint32_t)type, &c, ares.raw(), &p));
}

// Reprojection of the adaptive history (no reference counterpart): when the camera or instances move, carry the
// accumulated image, the per-pixel frame counts and the moments over to the new view instead of resetting them
struct ReprojectDesc
{
    CameraParams camera_params;   // the NEW view
    Mat3x4 camera_transform = mat3x4_identity();
    float ray_epsilon = 0.001f;
    float depth_tolerance = 0.02f;   // relative
    uint32_t max_history = 0;        // 0 = no cap
    // empty = no instance moved; else one transpose_inverse_transform per instance: what the scene held when history_in was rendered
    std::vector<LupinMat4x3> prev_instance_transforms;
};
class ReprojectResources
{
  public:
    ReprojectResources(const Device &d, uint32_t width, uint32_t height) : ctx_(d.raw()) { check(lupin_hip_build_reproject_resources(ctx_, width, height, &res_)); }
    ReprojectResources(ReprojectResources &&o) noexcept : ctx_(o.ctx_), res_(o.res_) { o.res_ = nullptr; }
    ReprojectResources(const ReprojectResources &) = delete;
    ~ReprojectResources() { if (res_) lupin_hip_destroy_reproject_resources(res_); }
    LupinReprojectResources *raw() const { return res_; }
    // forget the previous view: wherever AdaptiveResources::reset is called
    void invalidate() { check(lupin_hip_reproject_invalidate(ctx_, res_)); }
    // device milliseconds of the latest call's trace and gather kernels; needs lupin_hip_stats_reset(ctx, LUPIN_STATS_KERNEL_TIMING)
    void timings(float &trace_ms, float &gather_ms) const { check(lupin_hip_reproject_timings(ctx_, res_, &trace_ms, &gather_ms)); }
    // which: 0 the latest call's view, 1 the one before; any pointer may be null; inst / tri / depth W*H, uv W*H*2
    void download(int which, uint32_t *inst, uint32_t *tri, float *uv, float *depth) const
    {
        check(lupin_hip_reproject_download(ctx_, res_, which, inst, tri, uv, depth));
    }
  private:
    LupinContext *ctx_ = nullptr;
    LupinReprojectResources *res_ = nullptr;
};
inline ReprojectResources build_reproject_resources(const Device &d, uint32_t width, uint32_t height) { return ReprojectResources(d, width, height); }
inline void adaptive_reproject(const Device &d, AdaptiveResources &ares, ReprojectResources &res, const Scene &scene, const ReprojectDesc &desc,
                               TextureRef history_in, TextureRef history_out)
{
    LupinReprojectDesc c{};
    c.camera_params = detail::camera_params_c(desc.camera_params);
    c.camera_transform = desc.camera_transform;
    c.ray_epsilon = desc.ray_epsilon;
    c.depth_tolerance = desc.depth_tolerance;
    c.max_history = desc.max_history;
    c.prev_instance_transforms = desc.prev_instance_transforms.empty() ? nullptr : desc.prev_instance_transforms.data();
    c.num_instances = (uint32_t)desc.prev_instance_transforms.size();
    check(lupin_hip_adaptive_reproject(d.raw(), ares.raw(), res.raw(), scene.raw(), &c, history_in.raw(), history_out.raw()));
}


// radiance queries (no reference counterpart): the integrators over caller-supplied rays
enum class RayMode : uint32_t { Direction = LUPIN_RAY_DIRECTION, CosineHemisphere = LUPIN_RAY_COSINE_HEMISPHERE };
struct RayQueryDesc
{
    PathtraceType pathtrace_type = PathtraceType::Standard;
    uint32_t max_bounces = 8;
    uint32_t samples = 1;
    uint32_t flags = 0;            // LUPIN_RAYS_DEVICE_POINTERS: records, out and out_rays are device memory
    uint32_t max_slots = 0;        // paths per wavefront; 0 = the library's default
    AdvancedParams advanced;
};
namespace detail {
inline LupinRayQueryDesc ray_query_desc_c(const RayQueryDesc &desc)
{
    LupinRayQueryDesc c{};
    c.pathtrace_type = (uint32_t)desc.pathtrace_type;
    c.max_bounces = desc.max_bounces;
    c.samples = desc.samples;
    c.flags = desc.flags;
    c.max_slots = desc.max_slots;
    c.advanced = advanced_c(desc.advanced);
    return c;
}
}  // namespace detail
// records: n x 8 floats (origin | RNG bits, direction or normal | mode bits); out: n x 4; out_rays: nullptr or n * samples x 8
inline void pathtrace_rays(const Device &d, const Scene &scene, const RayQueryDesc &desc, uint64_t n, const float *records, float *out,
                           float *out_rays = nullptr)
{
    const LupinRayQueryDesc c = detail::ray_query_desc_c(desc);
    check(lupin_hip_pathtrace_rays(d.raw(), scene.raw(), &c, n, records, out, out_rays));
}

// lightmap baking (no reference counterpart): the charts' triangles rasterised to texels, every owned texel
// path-traced over its hemisphere
struct LightmapChart
{
    uint32_t instance_idx = 0;
    float scale_u = 1.0f, scale_v = 1.0f, offset_u = 0.0f, offset_v = 0.0f;   // atlas uv = mesh uv * scale + offset
};
struct LightmapDesc
{
    uint32_t width = 0, height = 0;
    PathtraceType pathtrace_type = PathtraceType::Standard;
    uint32_t max_bounces = 8;
    uint32_t samples = 64;
    uint32_t max_slots = 0;
    uint32_t flags = 0;            // LUPIN_LIGHTMAP_SMOOTH_NORMALS
    uint32_t dilate = 0;           // gutter passes
    uint32_t counter = 0;
    float surface_offset = 0.0f;   // world units along the geometric normal; the caller chooses (> 0)
    AdvancedParams advanced;
};
namespace detail {
inline LupinLightmapDesc lightmap_desc_c(const LightmapDesc &desc)
{
    LupinLightmapDesc c{};
    c.width = desc.width;
    c.height = desc.height;
    c.pathtrace_type = (uint32_t)desc.pathtrace_type;
    c.max_bounces = desc.max_bounces;
    c.samples = desc.samples;
    c.max_slots = desc.max_slots;
    c.flags = desc.flags;
    c.dilate = desc.dilate;
    c.counter = desc.counter;
    c.surface_offset = desc.surface_offset;
    c.advanced = advanced_c(desc.advanced);
    return c;
}
inline std::vector<LupinLightmapChart> charts_c(const LightmapChart *charts, uint32_t num_charts)
{
    std::vector<LupinLightmapChart> cc(num_charts);
    for (uint32_t k = 0; k < num_charts; k++)
    {
        cc[k].instance_idx = charts[k].instance_idx;
        cc[k].scale_u = charts[k].scale_u; cc[k].scale_v = charts[k].scale_v;
        cc[k].offset_u = charts[k].offset_u; cc[k].offset_v = charts[k].offset_v;
    }
    return cc;
}
}  // namespace detail
// out_rgba: height x width x 4 floats; out_records: nullptr or height x width x 8; returns the number of owned texels
inline uint64_t bake_lightmap(const Device &d, const Scene &scene, const LightmapDesc &desc, const LightmapChart *charts, uint32_t num_charts,
                              float *out_rgba, float *out_records = nullptr)
{
    const LupinLightmapDesc c = detail::lightmap_desc_c(desc);
    const std::vector<LupinLightmapChart> cc = detail::charts_c(charts, num_charts);
    uint64_t covered = 0;
    check(lupin_hip_bake_lightmap(d.raw(), scene.raw(), &c, cc.data(), num_charts, out_rgba, out_records, &covered));
    return covered;
}

// directional lightmaps (no reference counterpart): bake_lightmap's texels, records and paths, resolved into the
// four L0 / L1 coefficient planes of the cosine-weighted incident radiance that render_lightmapped_directional shades normal
// maps from.  out_sh: 4 x height x width x 4 floats, plane j first; out_records: nullptr or height x width x 8; returns the
// number of owned texels.
inline uint64_t bake_lightmap_directional(const Device &d, const Scene &scene, const LightmapDesc &desc, const LightmapChart *charts,
                                          uint32_t num_charts, float *out_sh, float *out_records = nullptr)
{
    const LupinLightmapDesc c = detail::lightmap_desc_c(desc);
    const std::vector<LupinLightmapChart> cc = detail::charts_c(charts, num_charts);
    uint64_t covered = 0;
    check(lupin_hip_bake_lightmap_directional(d.raw(), scene.raw(), &c, cc.data(), num_charts, out_sh, out_records, &covered));
    return covered;
}

// adaptive lightmap baking (no reference counterpart).  pathtrace_rays_moments is pathtrace_rays with the moments
// of every record's paths: out n x 8 floats (mean r, g, b, 1, the mean luminance, M2 about it, samples, 0).
inline void pathtrace_rays_moments(const Device &d, const Scene &scene, const RayQueryDesc &desc, uint64_t n, const float *records, float *out)
{
    const LupinRayQueryDesc c = detail::ray_query_desc_c(desc);
    check(lupin_hip_pathtrace_rays_moments(d.raw(), scene.raw(), &c, n, records, out));
}
// bake_lightmap in rounds of desc.samples paths per texel: a texel stops once the relative standard error of its luminance is
// below the threshold and no atlas neighbour wants samples.  out_rgba: height x width x 4 floats; out_stats: nullptr or the
// same shape (paths taken, relative error, standard error of the irradiance's luminance, converged); out_records: nullptr or
// height x width x 8; returns the number of owned texels.
struct LightmapAdaptiveDesc
{
    float threshold = 0.05f;
    uint32_t min_rounds = 2;
    uint32_t max_rounds = 64;      // <= LUPIN_LIGHTMAP_ADAPTIVE_MAX_ROUNDS; samples * max_rounds <= 2^24
};
inline uint64_t bake_lightmap_adaptive(const Device &d, const Scene &scene, const LightmapDesc &desc, const LightmapAdaptiveDesc &adaptive,
                                       const LightmapChart *charts, uint32_t num_charts, float *out_rgba, float *out_stats = nullptr,
                                       float *out_records = nullptr)
{
    const LupinLightmapDesc c = detail::lightmap_desc_c(desc);
    LupinLightmapAdaptiveDesc a{};
    a.threshold = adaptive.threshold;
    a.min_rounds = adaptive.min_rounds;
    a.max_rounds = adaptive.max_rounds;
    a.flags = 0u;
    const std::vector<LupinLightmapChart> cc = detail::charts_c(charts, num_charts);
    uint64_t covered = 0;
    check(lupin_hip_bake_lightmap_adaptive(d.raw(), scene.raw(), &c, &a, cc.data(), num_charts, out_rgba, out_stats, out_records, &covered));
    return covered;
}
inline LupinLightmapAdaptiveStats lightmap_adaptive_stats()
{
    LupinLightmapAdaptiveStats s;
    lupin_hip_lightmap_adaptive_stats(&s);
    return s;
}

// ambient-occlusion and bent-normal atlases (no reference counterpart): bake_lightmap's texels and records,
// every owned texel queried by the bent-normal kernel up to max_distance
struct LightmapAoDesc
{
    uint32_t width = 0, height = 0;
    uint32_t samples = 64;
    uint32_t max_slots = 0;
    uint32_t flags = 0;            // LUPIN_LIGHTMAP_SMOOTH_NORMALS | LUPIN_LIGHTMAP_AO_OPACITY
    uint32_t dilate = 0;           // gutter passes
    uint32_t counter = 0;
    float surface_offset = 0.0f;   // world units along the geometric normal; the caller chooses (> 0)
    float max_distance = std::numeric_limits<float>::infinity();
    float ray_epsilon = 0.001f;
};
// out_ao: height x width x 4 floats (visibility, alpha = ownership); out_bent: nullptr or height x width x 4 (unit bent
// normal); out_records: nullptr or height x width x 8; returns the number of owned texels
inline uint64_t bake_lightmap_ao(const Device &d, const Scene &scene, const LightmapAoDesc &desc, const LightmapChart *charts, uint32_t num_charts,
                                 float *out_ao, float *out_bent = nullptr, float *out_records = nullptr)
{
    LupinLightmapAoDesc c{};
    c.width = desc.width;
    c.height = desc.height;
    c.samples = desc.samples;
    c.max_slots = desc.max_slots;
    c.flags = desc.flags;
    c.dilate = desc.dilate;
    c.counter = desc.counter;
    c.surface_offset = desc.surface_offset;
    c.max_distance = desc.max_distance;
    c.ray_epsilon = desc.ray_epsilon;
    const std::vector<LupinLightmapChart> cc = detail::charts_c(charts, num_charts);
    uint64_t covered = 0;
    check(lupin_hip_bake_lightmap_ao(d.raw(), scene.raw(), &c, cc.data(), num_charts, out_ao, out_bent, out_records, &covered));
    return covered;
}

// lightmap denoising (no reference counterpart): an edge-avoiding a-trous filter in atlas space, guided by the
// records of the bake; `out_rgba` may be `rgba`
struct LightmapDenoiseDesc
{
    uint32_t width = 0, height = 0;
    uint32_t passes = 5;              // pass i taps at step 2^i
    uint32_t normal_squarings = 5;    // w_n = max(0, n_p . n_q)^32
    uint32_t dilate = 0;              // gutter passes after the filter
    uint32_t flags = 0;               // LUPIN_LIGHTMAP_DENOISE_DEVICE_POINTERS
    float max_stretch = 4.0f;
};
inline void denoise_lightmap(const Device &d, const LightmapDenoiseDesc &desc, const float *rgba, const float *records, float *out_rgba)
{
    LupinLightmapDenoiseDesc c{};
    c.width = desc.width;
    c.height = desc.height;
    c.passes = desc.passes;
    c.normal_squarings = desc.normal_squarings;
    c.dilate = desc.dilate;
    c.flags = desc.flags;
    c.max_stretch = desc.max_stretch;
    check(lupin_hip_denoise_lightmap(d.raw(), &c, rgba, records, out_rgba));
}

// light-probe baking (no reference counterpart): radiance over the sphere at points in space, as L2 SH
struct ProbeDesc
{
    PathtraceType pathtrace_type = PathtraceType::Standard;
    uint32_t max_bounces = 8;
    uint32_t samples = 1024;
    uint32_t flags = 0;            // LUPIN_PROBES_DEVICE_POINTERS: probes, out_sh and out_rays are device memory
    uint32_t max_slots = 0;        // paths per wavefront; 0 = the library's default
    AdvancedParams advanced;
};
// probes: n x 4 floats (position | RNG bits); out_sh: n x 9 x 4 (r, g, b, w per coefficient); out_rays: nullptr or n * samples x 8
inline void bake_probes(const Device &d, const Scene &scene, const ProbeDesc &desc, uint64_t n, const float *probes, float *out_sh,
                        float *out_rays = nullptr)
{
    LupinProbeDesc c{};
    c.pathtrace_type = (uint32_t)desc.pathtrace_type;
    c.max_bounces = desc.max_bounces;
    c.samples = desc.samples;
    c.flags = desc.flags;
    c.max_slots = desc.max_slots;
    c.advanced = detail::advanced_c(desc.advanced);
    check(lupin_hip_bake_probes(d.raw(), scene.raw(), &c, n, probes, out_sh, out_rays));
}
// Irradiance (r, g, b) at a surface with unit normal n from one probe's 9 x 4 coefficients: Ramamoorthi-Hanrahan, the clamped
// cosine's band factors pi, 2 pi / 3, pi / 4 on the basis of include/lupin_hip.h evaluated at n
inline std::array<float, 3> sh_irradiance(const float *coeffs, float nx, float ny, float nz)
{
    const float k0 = 0.28209479f, k1 = 0.48860251f, k2 = 1.09254843f, k3 = 0.31539157f, k4 = 0.54627422f;
    const float pi = 3.14159265358979323846f, a0 = pi, a1 = 2.0f * pi / 3.0f, a2 = pi / 4.0f;
    const float y[LUPIN_PROBE_SH_COEFFS] = {a0 * k0, a1 * (k1 * ny), a1 * (k1 * nz), a1 * (k1 * nx), a2 * ((k2 * nx) * ny), a2 * ((k2 * ny) * nz),
                                            a2 * (k3 * ((3.0f * nz) * nz - 1.0f)), a2 * ((k2 * nx) * nz), a2 * (k4 * (nx * nx - ny * ny))};
    std::array<float, 3> e{0.0f, 0.0f, 0.0f};
    for (int j = 0; j < LUPIN_PROBE_SH_COEFFS; j++)
        for (int c = 0; c < 3; c++) e[c] += coeffs[4 * j + c] * y[j];
    return e;
}

// occlusion queries (no reference counterpart): any-hit segment tests and ambient occlusion.  Geometric
// visibility: material opacity is not consulted.
enum class OcclusionMode : uint32_t { Direction = LUPIN_OCCLUSION_DIRECTION, CosineHemisphere = LUPIN_OCCLUSION_COSINE_HEMISPHERE };
struct OcclusionDesc
{
    OcclusionMode mode = OcclusionMode::Direction;
    uint32_t samples = 1;          // slots per record; 1 in direction mode
    uint32_t flags = 0;            // LUPIN_OCCLUSION_DEVICE_POINTERS: records and out_blocked are device memory
    float ray_epsilon = 0.001f;
};
namespace detail {
inline LupinOcclusionDesc occlusion_desc_c(const OcclusionDesc &desc)
{
    LupinOcclusionDesc c{};
    c.mode = (uint32_t)desc.mode;
    c.samples = desc.samples;
    c.flags = desc.flags;
    c.ray_epsilon = desc.ray_epsilon;
    return c;
}
}  // namespace detail
// records: n x 8 floats (origin | RNG bits, unit direction or normal | tmax); out_blocked: n counts of blocked slots
inline void occlusion_rays(const Device &d, const Scene &scene, const OcclusionDesc &desc, uint64_t n, const float *records, uint32_t *out_blocked)
{
    const LupinOcclusionDesc c = detail::occlusion_desc_c(desc);
    check(lupin_hip_occlusion_rays(d.raw(), scene.raw(), &c, n, records, out_blocked));
}
// Direction-mode records of the segments p[i] -> q[i] (n x 3 floats each), in f32: d = q - p, len = sqrt((dx dx + dy dy) + dz dz),
// dir = d / len, tmax = len - ray_epsilon (the far end point's own surface does not block).  A pair no further apart than
// 2 * ray_epsilon is refused (std::invalid_argument, `who` names the caller) before anything touches the device.
inline std::vector<float> segment_records(uint64_t n, const float *p, const float *q, float ray_epsilon, const char *who = "lp::segment_records")
{
    std::vector<float> rec(n * LUPIN_OCCLUSION_RECORD_FLOATS, 0.0f);
    for (uint64_t i = 0; i < n; i++)
    {
        const float dx = q[3 * i] - p[3 * i], dy = q[3 * i + 1] - p[3 * i + 1], dz = q[3 * i + 2] - p[3 * i + 2];
        const float len = std::sqrt((dx * dx + dy * dy) + dz * dz);
        if (!(len > 2.0f * ray_epsilon)) throw std::invalid_argument(std::string(who) + ": a segment is not longer than 2 * ray_epsilon");
        float *r = &rec[i * LUPIN_OCCLUSION_RECORD_FLOATS];
        r[0] = p[3 * i]; r[1] = p[3 * i + 1]; r[2] = p[3 * i + 2];
        r[4] = dx / len; r[5] = dy / len; r[6] = dz / len;
        r[7] = len - ray_epsilon;
    }
    return rec;
}
// Whether nothing lies between p[i] and q[i] (n x 3 floats each); the segments are segment_records'.
inline std::vector<uint8_t> visible(const Device &d, const Scene &scene, uint64_t n, const float *p, const float *q, float ray_epsilon = 0.001f)
{
    const std::vector<float> rec = segment_records(n, p, q, ray_epsilon, "lp::visible");
    std::vector<uint32_t> blocked(n, 0u);
    OcclusionDesc desc;
    desc.mode = OcclusionMode::Direction;
    desc.samples = 1;
    desc.flags = 0;
    desc.ray_epsilon = ray_epsilon;
    occlusion_rays(d, scene, desc, n, rec.data(), blocked.data());
    std::vector<uint8_t> out(n);
    for (uint64_t i = 0; i < n; i++) out[i] = blocked[i] == 0u;
    return out;
}
// 1 - blocked / samples over `samples` cosine-weighted directions of length `radius` about normals[i], from origins[i] (n x 3
// floats each; the caller has moved the origins off the surface); rng_words: n RNG states, one per point
inline std::vector<float> ambient_occlusion(const Device &d, const Scene &scene, uint64_t n, const float *origins, const float *normals,
                                            const uint32_t *rng_words, float radius, uint32_t samples = 64, float ray_epsilon = 0.001f)
{
    std::vector<float> rec(n * LUPIN_OCCLUSION_RECORD_FLOATS, 0.0f);
    for (uint64_t i = 0; i < n; i++)
    {
        float *r = &rec[i * LUPIN_OCCLUSION_RECORD_FLOATS];
        r[0] = origins[3 * i]; r[1] = origins[3 * i + 1]; r[2] = origins[3 * i + 2];
        std::memcpy(&r[3], &rng_words[i], 4);
        r[4] = normals[3 * i]; r[5] = normals[3 * i + 1]; r[6] = normals[3 * i + 2];
        r[7] = radius;
    }
    std::vector<uint32_t> blocked(n, 0u);
    OcclusionDesc desc;
    desc.mode = OcclusionMode::CosineHemisphere;
    desc.samples = samples;
    desc.flags = 0;
    desc.ray_epsilon = ray_epsilon;
    occlusion_rays(d, scene, desc, n, rec.data(), blocked.data());
    std::vector<float> out(n);
    for (uint64_t i = 0; i < n; i++) out[i] = 1.0f - (float)blocked[i] / (float)samples;
    return out;
}

// transmittance queries (no reference counterpart): occlusion_rays' records and desc; out_sum: per record, the
// sum over its slots of the product of 1 - opacity over the surfaces at ray_epsilon <= t < tmax (0 once an opacity of 1 is
// met): the expected result of the integrators' stochastic alpha skip.  The caller divides by samples.
inline void transmittance_rays(const Device &d, const Scene &scene, const OcclusionDesc &desc, uint64_t n, const float *records, float *out_sum)
{
    const LupinOcclusionDesc c = detail::occlusion_desc_c(desc);
    check(lupin_hip_transmittance_rays(d.raw(), scene.raw(), &c, n, records, out_sum));
}
// bent-normal queries (no reference counterpart): hemisphere-mode occlusion records; out: n x 4 floats, per
// record (sum T d.x, sum T d.y, sum T d.z, sum T) over its cosine-weighted slots, T = 1 / 0 (open / blocked) or, with
// LUPIN_BENT_NORMAL_OPACITY, the slot's transmittance.  The caller divides .w by samples and normalises .xyz.
struct BentNormalDesc
{
    uint32_t samples = 64;
    uint32_t flags = 0;        // LUPIN_BENT_NORMAL_DEVICE_POINTERS | LUPIN_BENT_NORMAL_OPACITY
    uint32_t max_slots = 0;    // 0: the library's default
    float ray_epsilon = 0.001f;
};
inline void bent_normal_rays(const Device &d, const Scene &scene, const BentNormalDesc &desc, uint64_t n, const float *records, float *out)
{
    LupinBentNormalDesc c{};
    c.samples = desc.samples;
    c.flags = desc.flags;
    c.max_slots = desc.max_slots;
    c.ray_epsilon = desc.ray_epsilon;
    check(lupin_hip_bent_normal_rays(d.raw(), scene.raw(), &c, n, records, out));
}
// The transmittance between p[i] and q[i] (n x 3 floats each); the segments are segment_records'.
inline std::vector<float> transmittance(const Device &d, const Scene &scene, uint64_t n, const float *p, const float *q, float ray_epsilon = 0.001f)
{
    const std::vector<float> rec = segment_records(n, p, q, ray_epsilon, "lp::transmittance");
    std::vector<float> out(n, 0.0f);
    OcclusionDesc desc;
    desc.mode = OcclusionMode::Direction;
    desc.samples = 1;
    desc.flags = 0;
    desc.ray_epsilon = ray_epsilon;
    transmittance_rays(d, scene, desc, n, rec.data(), out.data());
    return out;
}

// distance queries (no reference counterpart): the nearest surface point of points in world space.
// `side` is the side of the REPORTED triangle (sign of dot(p - point, (v1 - v0) x (v2 - v0))), not inside / outside.
struct DistanceResult   // the twelve words of LUPIN_DISTANCE_RESULT_FLOATS
{
    uint32_t found;
    float distance;
    float point[3];
    float u, v;
    uint32_t instance, tri;
    float side;
    uint32_t pad[2];
};
static_assert(sizeof(DistanceResult) == 4 * LUPIN_DISTANCE_RESULT_FLOATS, "DistanceResult mirrors the result words");
// records: n x 4 floats (point | rmax); flags: LUPIN_DISTANCE_DEVICE_POINTERS or 0
inline void distance_points(const Device &d, const Scene &scene, uint64_t n, const float *records, DistanceResult *out_results, uint32_t flags = 0)
{
    check(lupin_hip_distance_points(d.raw(), scene.raw(), flags, n, records, reinterpret_cast<float *>(out_results)));
}
// dims[0] x dims[1] x dims[2] distances, x fastest, at origin + (i + 0.5) * spacing; rmax where nothing lies within rmax
inline std::vector<float> bake_distance_grid(const Device &d, const Scene &scene, const std::array<float, 3> &origin, const std::array<float, 3> &spacing,
                                             const std::array<uint32_t, 3> &dims, float rmax = std::numeric_limits<float>::infinity(), bool is_signed = false)
{
    std::vector<float> out((size_t)dims[0] * dims[1] * dims[2]);
    const uint32_t flags = is_signed ? (uint32_t)LUPIN_DISTANCE_GRID_SIGNED : 0u;
    check(lupin_hip_bake_distance_grid(d.raw(), scene.raw(), flags, origin.data(), spacing.data(), dims.data(), rmax, out.data()));
    return out;
}

// irradiance volume lookup (no reference counterpart): irradiance at (point, normal) from a regular grid of
// bake_probes' coefficients -- trilinear over the cell's eight probes, less the probes marked invalid and the probes the
// scene hides from the point; lupin_hip.h states the arithmetic.
struct ProbeGridDesc
{
    std::array<float, 3> origin{{0.0f, 0.0f, 0.0f}}, spacing{{1.0f, 1.0f, 1.0f}};
    std::array<uint32_t, 3> dims{{1u, 1u, 1u}};
    uint32_t flags = LUPIN_PROBE_GRID_VISIBILITY | LUPIN_PROBE_GRID_BACKFACE;   // | LUPIN_PROBE_GRID_DEVICE_POINTERS
    float ray_epsilon = 0.001f;
    float normal_bias = 0.0f;   // world units; the Python mirror's default is 1e-4 of the scene's extent
};
// the probe positions in index order (x fastest), n x 3 floats: origin + (float)i * spacing per axis
inline std::vector<float> probe_grid_positions(const std::array<float, 3> &origin, const std::array<float, 3> &spacing, const std::array<uint32_t, 3> &dims)
{
    std::vector<float> out;
    out.reserve((size_t)dims[0] * dims[1] * dims[2] * 3);
    for (uint32_t iz = 0; iz < dims[2]; iz++)
        for (uint32_t iy = 0; iy < dims[1]; iy++)
            for (uint32_t ix = 0; ix < dims[0]; ix++)
            {
                const float px = (float)ix * spacing[0], py = (float)iy * spacing[1], pz = (float)iz * spacing[2];   // the product first
                out.push_back(origin[0] + px);
                out.push_back(origin[1] + py);
                out.push_back(origin[2] + pz);
            }
    return out;
}
// sh: P x 9 x 4 floats; valid: nullptr or P bytes; records: n x 8 floats (point | -, unit normal | -); out: n x (r, g, b, w)
inline void sample_probe_grid(const Device &d, const Scene &scene, const ProbeGridDesc &desc, const float *sh, const uint8_t *valid, uint64_t n,
                              const float *records, float *out)
{
    LupinProbeGridDesc c;
    for (int k = 0; k < 3; k++) { c.origin[k] = desc.origin[k]; c.spacing[k] = desc.spacing[k]; c.dims[k] = desc.dims[k]; }
    c.flags = desc.flags;
    c.ray_epsilon = desc.ray_epsilon;
    c.normal_bias = desc.normal_bias;
    check(lupin_hip_sample_probe_grid(d.raw(), scene.raw(), &c, sh, valid, n, records, out));
}

// probe depth maps (no reference counterpart): per probe an octahedral map of the mean and mean square of the
// distance to the nearest surface, and the irradiance volume lookup that takes a corner's visibility from those maps
// instead of the scene; lupin_hip.h states the arithmetic.
struct ProbeDepthDesc
{
    uint32_t resolution = 16;     // R: interior texels per side, 2 .. 64
    uint32_t subsamples = 4;      // K: 1, 2, 4 or 8; K * K rays per texel
    uint32_t flags = 0;           // LUPIN_PROBE_DEPTH_DEVICE_POINTERS
    uint32_t max_slots = 0;       // rays per launch; 0 = the library's default
    float ray_epsilon = 0.001f;
    float max_distance = 1.0f;    // the cap; for a grid, 1.5 |spacing| is the Python mirror's default
};
// positions: n x 4 floats ([3] ignored); out_depth: n x (R + 2) x (R + 2) x 2; out_stats: nullptr or n x 4 words
inline void bake_probe_depth(const Device &d, const Scene &scene, const ProbeDepthDesc &desc, uint64_t n, const float *positions, float *out_depth,
                             uint32_t *out_stats = nullptr)
{
    LupinProbeDepthDesc c;
    c.resolution = desc.resolution;
    c.subsamples = desc.subsamples;
    c.flags = desc.flags;
    c.max_slots = desc.max_slots;
    c.ray_epsilon = desc.ray_epsilon;
    c.max_distance = desc.max_distance;
    check(lupin_hip_bake_probe_depth(d.raw(), scene.raw(), &c, n, positions, out_depth, out_stats));
}
// desc.flags: LUPIN_PROBE_GRID_BACKFACE | LUPIN_PROBE_GRID_DEVICE_POINTERS (LUPIN_PROBE_GRID_VISIBILITY, ProbeGridDesc's default, is
// refused: clear it); depth: P x (R + 2) x (R + 2) x 2, bake_probe_depth's maps at the grid's positions; max_distance: the bake's
inline void sample_probe_grid_depth(const Device &d, const Scene &scene, const ProbeGridDesc &desc, uint32_t resolution, float max_distance, const float *sh,
                                    const float *depth, const uint8_t *valid, uint64_t n, const float *records, float *out)
{
    LupinProbeGridDepthDesc c;
    for (int k = 0; k < 3; k++) { c.grid.origin[k] = desc.origin[k]; c.grid.spacing[k] = desc.spacing[k]; c.grid.dims[k] = desc.dims[k]; }
    c.grid.flags = desc.flags;
    c.grid.ray_epsilon = desc.ray_epsilon;
    c.grid.normal_bias = desc.normal_bias;
    c.resolution = resolution;
    c.max_distance = max_distance;
    check(lupin_hip_sample_probe_grid_depth(d.raw(), scene.raw(), &c, sh, depth, valid, n, records, out));
}

// baked-lighting view (no reference counterpart): a camera view of a baked irradiance volume -- one primary hit
// per pixel, then emission + color / pi * E(p, n) with E from sample_probe_grid's lookup (depth == nullptr) or from
// sample_probe_grid_depth's; every material is drawn as a matte surface of its color; lupin_hip.h states the arithmetic.
struct BakedViewDesc
{
    LupinCameraParams camera_params{0u, 0.050f, 0.036f, 1.5f, 10000.0f, 0.0f};
    LupinMat3x4 camera_transform{{{1.0f, 0.0f, 0.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}, {0.0f, 0.0f, 0.0f}}};
    ProbeGridDesc grid;             // flags: LUPIN_PROBE_GRID_BACKFACE, and without maps LUPIN_PROBE_GRID_VISIBILITY (clear it with maps)
    uint32_t resolution = 16;       // of the maps; with depth only
    float max_distance = 1.0f;      // the maps' bake's; with depth only
    float ray_epsilon = 0.001f;     // the primary ray's
    std::array<float, 3> ambient{{0.0f, 0.0f, 0.0f}};   // E where no probe answers
    uint32_t flags = 0;             // LUPIN_BAKED_VIEW_DEVICE_POINTERS: sh, depth, valid and out_gbuffer are device memory
    uint32_t max_slots = 0;         // pixels per launch; 0 = the library's default
};
inline LupinBakedViewDesc baked_view_desc_c(const BakedViewDesc &desc)
{
    LupinBakedViewDesc c;
    c.camera_params = desc.camera_params;
    c.camera_transform = desc.camera_transform;
    for (int k = 0; k < 3; k++) { c.grid.origin[k] = desc.grid.origin[k]; c.grid.spacing[k] = desc.grid.spacing[k]; c.grid.dims[k] = desc.grid.dims[k]; c.ambient[k] = desc.ambient[k]; }
    c.grid.flags = desc.grid.flags;
    c.grid.ray_epsilon = desc.grid.ray_epsilon;
    c.grid.normal_bias = desc.grid.normal_bias;
    c.resolution = desc.resolution;
    c.max_distance = desc.max_distance;
    c.ray_epsilon = desc.ray_epsilon;
    c.flags = desc.flags;
    c.max_slots = desc.max_slots;
    return c;
}
// sh: P x 9 x 4; depth: nullptr or P x (R + 2) x (R + 2) x 2; valid: nullptr or P; out_gbuffer: nullptr or W x H x 16 floats
inline void render_baked(const Device &d, const Scene &scene, TextureRef render_target, const BakedViewDesc &desc, const float *sh,
                         const float *depth = nullptr, const uint8_t *valid = nullptr, float *out_gbuffer = nullptr)
{
    const LupinBakedViewDesc c = baked_view_desc_c(desc);
    check(lupin_hip_render_baked(d.raw(), scene.raw(), render_target.raw(), &c, sh, depth, valid, out_gbuffer));
}

// lightmapped view (no reference counterpart): render_baked with a lightmap atlas as the irradiance source on
// every instance that has a chart -- an ownership-aware bilinear fetch at the hit's texcoords -- and the volume (sh != nullptr)
// or `view.ambient` on the rest; lupin_hip.h states the arithmetic.  `charts` are the bake's, `lightmap` is
// lightmap_height x lightmap_width x 4 floats (bake_lightmap's or denoise_lightmap's atlas); view.grid, resolution and
// max_distance are read only with sh; out_gbuffer: nullptr or W x H x 20 floats.
inline void render_lightmapped(const Device &d, const Scene &scene, TextureRef render_target, const BakedViewDesc &view,
                               const std::vector<LupinLightmapChart> &charts, const float *lightmap, uint32_t lightmap_width, uint32_t lightmap_height,
                               const float *sh = nullptr, const float *depth = nullptr, const uint8_t *valid = nullptr, float *out_gbuffer = nullptr)
{
    LupinLightmappedViewDesc c{};
    c.view = baked_view_desc_c(view);
    c.lightmap_width = lightmap_width;
    c.lightmap_height = lightmap_height;
    c.num_charts = (uint32_t)charts.size();
    c.reserved = 0u;
    check(lupin_hip_render_lightmapped(d.raw(), scene.raw(), render_target.raw(), &c, charts.empty() ? nullptr : charts.data(), lightmap, sh, depth, valid,
                                       out_gbuffer));
}

// ... with a directional lightmap: `directional` is bake_lightmap_directional's 4 x lightmap_height x
// lightmap_width x 4 floats for the same atlas and charts, bake_flags that bake's flags; a lightmapped pixel's irradiance is
// scaled by what its shading normal receives against what the bake normal did.  out_gbuffer: nullptr or W x H x 24 floats.
inline void render_lightmapped_directional(const Device &d, const Scene &scene, TextureRef render_target, const BakedViewDesc &view,
                                           const std::vector<LupinLightmapChart> &charts, const float *lightmap, const float *directional,
                                           uint32_t lightmap_width, uint32_t lightmap_height, uint32_t bake_flags = 0, const float *sh = nullptr,
                                           const float *depth = nullptr, const uint8_t *valid = nullptr, float *out_gbuffer = nullptr)
{
    LupinLightmappedDirectionalDesc c{};
    c.base.view = baked_view_desc_c(view);
    c.base.lightmap_width = lightmap_width;
    c.base.lightmap_height = lightmap_height;
    c.base.num_charts = (uint32_t)charts.size();
    c.base.reserved = 0u;
    c.bake_flags = bake_flags;
    check(lupin_hip_render_lightmapped_directional(d.raw(), scene.raw(), render_target.raw(), &c, charts.empty() ? nullptr : charts.data(), lightmap,
                                                   directional, sh, depth, valid, out_gbuffer));
}

}  // namespace lp

namespace lpl {

struct SceneCamera { lp::Mat3x4 transform = lp::mat3x4_identity(); lp::CameraParams params; };   // loader.rs:303-308

// lpl::build_scene_cornell_box (loader.rs:14-207): 8 meshes / instances, 4 materials, values from Yocto/GL.
inline std::pair<lp::Scene, std::vector<SceneCamera>> build_scene_cornell_box(const lp::Device &d, bool build_sw_and_hw = true)
{
    using lp::Vec4;
    lp::SceneCPU s;
    auto mat = [&](float r, float g, float b, float er, float eg, float eb) {
        lp::Material m = lp::default_material();
        if (r >= 0) { m.color[0] = r; m.color[1] = g; m.color[2] = b; m.color[3] = 1.0f; }
        m.emission[0] = er; m.emission[1] = eg; m.emission[2] = eb;
        s.materials.push_back(m);
    };
    mat(0.725f, 0.71f, 0.68f, 0, 0, 0);      // white
    mat(0.63f, 0.065f, 0.05f, 0, 0, 0);      // red
    mat(0.14f, 0.45f, 0.091f, 0, 0, 0);      // green
    mat(-1, 0, 0, 17.0f, 12.0f, 4.0f);       // emissive
    auto mesh = [&](std::vector<Vec4> v, std::vector<uint32_t> idx, uint32_t m) {
        s.mesh_infos.push_back(lp::default_mesh_info());
        s.verts_pos_array.push_back(std::move(v));
        s.indices_array.push_back(std::move(idx));
        lp::Instance in = lp::default_instance();
        in.mesh_idx = (uint32_t)s.mesh_infos.size() - 1;
        in.mat_idx = m;
        s.instances.push_back(in);
    };
    const std::vector<uint32_t> quad = {0, 1, 2, 2, 3, 0}, quad2 = {0, 2, 1, 2, 0, 3};
    const std::vector<uint32_t> box = {0, 2, 1, 2, 0, 3, 4, 6, 5, 6, 4, 7, 8, 10, 9, 10, 8, 11, 12, 14, 13, 14, 12, 15, 16, 18, 17, 18, 16, 19, 20, 22, 21, 22, 20, 23};
    mesh({{-1, 0, 1}, {1, 0, 1}, {1, 0, -1}, {-1, 0, -1}}, quad, 0);                       // floor
    mesh({{-1, 2, 1}, {-1, 2, -1}, {1, 2, -1}, {1, 2, 1}}, quad, 0);                       // ceiling
    mesh({{-1, 0, 1}, {1, 0, 1}, {1, 2, 1}, {-1, 2, 1}}, quad2, 0);                        // back wall
    mesh({{1, 0, -1}, {1, 0, 1}, {1, 2, 1}, {1, 2, -1}}, quad, 2);                         // right wall
    mesh({{-1, 0, 1}, {-1, 0, -1}, {-1, 2, -1}, {-1, 2, 1}}, quad, 1);                     // left wall
    mesh({{0.53f, 0.6f, -0.75f}, {0.7f, 0.6f, -0.17f}, {0.13f, 0.6f, -0.0f}, {-0.05f, 0.6f, -0.57f}, {-0.05f, 0.0f, -0.57f}, {-0.05f, 0.6f, -0.57f},
          {0.13f, 0.6f, -0.0f}, {0.13f, 0.0f, -0.0f}, {0.53f, 0.0f, -0.75f}, {0.53f, 0.6f, -0.75f}, {-0.05f, 0.6f, -0.57f}, {-0.05f, 0.0f, -0.57f},
          {0.7f, 0.0f, -0.17f}, {0.7f, 0.6f, -0.17f}, {0.53f, 0.6f, -0.75f}, {0.53f, 0.0f, -0.75f}, {0.13f, 0.0f, -0.0f}, {0.13f, 0.6f, -0.0f},
          {0.7f, 0.6f, -0.17f}, {0.7f, 0.0f, -0.17f}, {0.53f, 0.0f, -0.75f}, {0.7f, 0.0f, -0.17f}, {0.13f, 0.0f, -0.0f}, {-0.05f, 0.0f, -0.57f}}, box, 0);   // short box
    mesh({{-0.53f, 1.2f, -0.09f}, {0.04f, 1.2f, 0.09f}, {-0.14f, 1.2f, 0.67f}, {-0.71f, 1.2f, 0.49f}, {-0.53f, 0.0f, -0.09f}, {-0.53f, 1.2f, -0.09f},
          {-0.71f, 1.2f, 0.49f}, {-0.71f, 0.0f, 0.49f}, {-0.71f, 0.0f, 0.49f}, {-0.71f, 1.2f, 0.49f}, {-0.14f, 1.2f, 0.67f}, {-0.14f, 0.0f, 0.67f},
          {-0.14f, 0.0f, 0.67f}, {-0.14f, 1.2f, 0.67f}, {0.04f, 1.2f, 0.09f}, {0.04f, 0.0f, 0.09f}, {0.04f, 0.0f, 0.09f}, {0.04f, 1.2f, 0.09f},
          {-0.53f, 1.2f, -0.09f}, {-0.53f, 0.0f, -0.09f}, {-0.53f, 0.0f, -0.09f}, {0.04f, 0.0f, 0.09f}, {-0.14f, 0.0f, 0.67f}, {-0.71f, 0.0f, 0.49f}}, box, 0);   // tall box
    mesh({{-0.25f, 1.99f, -0.25f}, {-0.25f, 1.99f, 0.25f}, {0.25f, 1.99f, 0.25f}, {0.25f, 1.99f, -0.25f}}, quad2, 3);   // light
    lp::validate_scene(s, 0, 0);
    SceneCamera cam;
    cam.transform = lp::Mat3x4{{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0, 1, -3.9f}}};
    cam.params.is_orthographic = false; cam.params.lens = 0.035f; cam.params.aperture = 0.0f;
    cam.params.focus = 3.9f; cam.params.film = 0.024f; cam.params.aspect = 1.0f;
    return {lp::build_accel_structures_and_upload(d, s, {}, {}, build_sw_and_hw), {cam}};
}

// f16 -> f32 for readback
inline float half_to_float(uint16_t h)
{
    uint32_t sign = (uint32_t)(h & 0x8000u) << 16, exp = (h >> 10) & 0x1F, man = h & 0x3FFu, u;
    if (exp == 0) { if (!man) u = sign; else { int e = -1; do { man <<= 1; e++; } while (!(man & 0x400u)); man &= 0x3FFu; u = sign | ((uint32_t)(127 - 15 - e) << 23) | (man << 13); } }
    else if (exp == 31) u = sign | 0x7F800000u | (man << 13);
    else u = sign | ((exp + 112) << 23) | (man << 13);
    float f; std::memcpy(&f, &u, 4); return f;
}

// 8-bit preview of a tonemapped target (lp::tonemap_and_fit_aspect output) as binary PPM; the reference saves Rgba8Unorm
// textures as RGB8 through the `image` crate (loader.rs:1823-1851), PPM keeps this header dependency-free
inline void save_rgba8_ppm(const std::string &path, const std::vector<uint8_t> &rgba8, uint32_t w, uint32_t h)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw lp::Error(LUPIN_ERR_INVALID_ARGUMENT, "cannot open " + path);
    std::fprintf(f, "P6\n%u %u\n255\n", w, h);
    for (size_t i = 0; i < (size_t)w * h; i++) std::fwrite(&rgba8[i * 4], 1, 3, f);
    std::fclose(f);
}

// lpl::save_texture for `.hdr` (loader.rs:1775-1879; alpha dropped): flat RGBE, pixel rule of the `image` crate's encoder
inline void save_texture(const std::string &path, lp::TextureRef tex)
{
    const uint32_t w = tex.width(), h = tex.height();
    const std::vector<uint16_t> px = tex.download();
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) throw lp::Error(LUPIN_ERR_INVALID_ARGUMENT, "cannot open " + path);
    std::fprintf(f, "#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %u +X %u\n", h, w);
    std::vector<uint8_t> row((size_t)w * 4);
    for (uint32_t y = 0; y < h; y++)
    {
        for (uint32_t x = 0; x < w; x++)
        {
            const uint16_t *p = &px[((size_t)y * w + x) * 4];
            float c[3] = {half_to_float(p[0]), half_to_float(p[1]), half_to_float(p[2])};
            float mx = std::fmax(c[0], std::fmax(c[1], c[2]));
            uint8_t *o = &row[(size_t)x * 4];
            if (!(mx > 0.0f)) { o[0] = o[1] = o[2] = o[3] = 0; continue; }
            int e = (int)std::floor(std::log2(mx)) + 1;
            float mul = std::ldexp(1.0f, e);
            for (int k = 0; k < 3; k++) { float v = std::trunc(c[k] / mul * 256.0f); o[k] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }
            o[3] = (uint8_t)(e + 128);
        }
        std::fwrite(row.data(), 1, row.size(), f);
    }
    std::fclose(f);
}

}  // namespace lpl
