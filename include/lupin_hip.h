/*
 * lupin_hip.h -- C ABI of the MI355X (gfx950) software-BVH path tracer that stands in for
 * LupinPathTracer's `lp::pathtrace_scene()` hot path.
 *
 * Every struct below is byte-identical to the `#[repr(C)]` type the reference uploads to its
 * WGSL megakernel, and every entry point names the reference interface it replaces
 * (paths are relative to the reference checkout, `lupin/src/...`).
 *
 * Conventions (reference: renderer.rs:754-766, :768-842):
 *   - handles are opaque, not thread-safe, one context per GPU;
 *   - `lupin_hip_pathtrace_scene` ENQUEUES on the context's HIP stream and returns (the
 *     reference does `queue.submit` and returns, renderer.rs:841); `lupin_hip_sync` or any
 *     download is the sync point;
 *   - no panics across the ABI: every call returns LUPIN_OK or a negative error code and
 *     `lupin_hip_last_error()` holds the message (the reference asserts / panics instead,
 *     renderer.rs:770,776,814);
 *   - matrices are column-major f32, little-endian, exactly as base.rs:500-800 lays them out.
 */
#ifndef LUPIN_HIP_H
#define LUPIN_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------
 * Scene record layouts (renderer.rs:94-250 == pathtracer.wgsl:88-178)
 * ---------------------------------------------------------------------------------------- */

#define LUPIN_SENTINEL_IDX 0xFFFFFFFFu /* renderer.rs SENTINEL_IDX / pathtracer.wgsl:66 */

/* base.rs:634  Mat3x4 { m: [[f32;3];4] }  -- 4 columns x 3 rows, last column = translation */
typedef struct LupinMat3x4 { float m[4][3]; } LupinMat3x4;
/* base.rs:763  Mat4x3 { m: [[f32;4];3] }  -- 3 columns x 4 rows */
typedef struct LupinMat4x3 { float m[3][4]; } LupinMat4x3;
/* base.rs:505  Mat4 { m: [[f32;4];4] } column-major */
typedef struct LupinMat4 { float m[4][4]; } LupinMat4;

/* renderer.rs:94-100 */
typedef struct LupinMeshInfo {
    uint32_t normals_buf_idx;
    uint32_t texcoords_buf_idx;
    uint32_t colors_buf_idx;
} LupinMeshInfo;

/* renderer.rs:115-124 ; 64 bytes. transpose_inverse_transform = rows of the world->local affine. */
typedef struct LupinInstance {
    LupinMat4x3 transpose_inverse_transform;
    uint32_t mesh_idx;
    uint32_t mat_idx;
    float _padding0;
    float _padding1;
} LupinInstance;

/* renderer.rs:126-139 */
enum LupinMaterialType {
    LUPIN_MAT_MATTE = 0,
    LUPIN_MAT_GLOSSY = 1,
    LUPIN_MAT_REFLECTIVE = 2,
    LUPIN_MAT_TRANSPARENT = 3,
    LUPIN_MAT_REFRACTIVE = 4,
    LUPIN_MAT_SUBSURFACE = 5,
    LUPIN_MAT_VOLUMETRIC = 6,
    LUPIN_MAT_GLTFPBR = 7
};

/* renderer.rs:141-161 ; 96 bytes */
typedef struct LupinMaterial {
    float color[4];      /* w = opacity */
    float emission[4];
    float scattering[4];
    uint32_t mat_type;
    float roughness;
    float metallic;
    float ior;
    float sc_anisotropy;
    float tr_depth;
    uint32_t color_tex_idx;
    uint32_t emission_tex_idx;
    uint32_t roughness_tex_idx;
    uint32_t scattering_tex_idx;
    uint32_t normal_tex_idx;
    uint32_t padding0;
} LupinMaterial;

/* renderer.rs:187-194 ; 80 bytes */
typedef struct LupinEnvironment {
    float emission[3];
    uint32_t emission_tex_idx;
    LupinMat4 transform;
} LupinEnvironment;

/* renderer.rs:208-214 */
typedef struct LupinLight {
    uint32_t instance_idx;
    float area;
} LupinLight;

/* renderer.rs:216-223 */
typedef struct LupinAliasBin {
    float prob;
    float alias_threshold;
    uint32_t alias;
} LupinAliasBin;

/* renderer.rs:228-238 ; 32 bytes. tri_count == 0 => internal node, children at first_child, +1 */
typedef struct LupinBvhNode {
    float aabb_min[3];
    uint32_t tri_begin_or_first_child;
    float aabb_max[3];
    uint32_t tri_count;
} LupinBvhNode;

/* renderer.rs:240-250 ; 48 bytes. left == 0 => leaf */
typedef struct LupinTlasNode {
    float aabb_min[3];
    uint32_t left;
    float aabb_max[3];
    uint32_t instance_idx;
    uint32_t right;
    float _padding0[3];
} LupinTlasNode;

/* renderer.rs:252-280 ; 128 bytes. Exposed because the oracle and the kernels consume exactly
 * this record; hosts normally never build it (lupin_hip_pathtrace_scene does, like
 * get_push_constants{,_tiled}, renderer.rs:1426-1506). */
typedef struct LupinPushConstants {
    LupinMat4 camera_transform;
    float camera_lens;
    float camera_film;
    float camera_aspect;
    float camera_focus;
    float camera_aperture;
    uint32_t flags;
    uint32_t id_offset[2];
    uint32_t accum_counter;
    float heatmap_min;
    float heatmap_max;
    uint32_t falsecolor_type;
    uint32_t pathtrace_type;
    float max_radiance;
    uint32_t rng_seed;   /* never read by the shader (pathtracer.wgsl:1565) -- kept for layout */
    float ray_epsilon;
} LupinPushConstants;

/* renderer.rs:284-291 */
#define LUPIN_FLAG_CAMERA_ORTHO         (1u << 0)
#define LUPIN_FLAG_ENVS_EMPTY           (1u << 1)
#define LUPIN_FLAG_LIGHTS_EMPTY         (1u << 2)
#define LUPIN_FLAG_DEBUG_TRI_CHECKS     (1u << 3)
#define LUPIN_FLAG_DEBUG_AABB_CHECKS    (1u << 4)
#define LUPIN_FLAG_DEBUG_NUM_BOUNCES    (1u << 5)
#define LUPIN_FLAG_DEBUG_FIRST_HIT_ONLY (1u << 6)
#define LUPIN_FLAG_INSTANCES_EMPTY      (1u << 7)

/* renderer.rs:294-305 */
#define LUPIN_BVH_MAX_DEPTH   25
#define LUPIN_TLAS_MAX_DEPTH  50
#define LUPIN_WORKGROUP_SIZE  4   /* tile_size is counted in 4x4-pixel workgroups */
#define LUPIN_MAX_ENVS        10

/* Texture formats the loader produces (lupin_loader/src/loader.rs:227-231): LDR = Rgba8Unorm
 * (never ...Srgb, decode happens in the shader), HDR = Rgba16Float. One mip, bilinear, Repeat
 * in u and v (wgpu_utils.rs:244-256). */
enum LupinTextureFormat {
    LUPIN_TEX_RGBA8_UNORM = 0,
    LUPIN_TEX_RGBA16_FLOAT = 1
};

typedef struct LupinTextureDesc {
    uint32_t width;
    uint32_t height;
    uint32_t format;       /* LupinTextureFormat */
    const void *pixels;    /* host pointer, row-major, 4 B or 8 B per texel */
} LupinTextureDesc;

/* One mesh = the per-mesh storage buffers of lp::Scene in its software-BVH configuration
 * (renderer.rs:17-60): positions (Vec4, stride 16), BVH-reordered indices, BLAS nodes. */
typedef struct LupinMeshDesc {
    const float *verts_pos;          /* num_verts * 4 floats (w ignored) */
    uint32_t num_verts;
    const uint32_t *indices;         /* num_indices u32, triangles in BLAS leaf order */
    uint32_t num_indices;
    const LupinBvhNode *bvh_nodes;
    uint32_t num_bvh_nodes;
} LupinMeshDesc;

typedef struct LupinVertexBufferDesc {
    const float *data;               /* normals/colours: 4 floats per vertex; texcoords: 2 */
    uint32_t num_verts;
} LupinVertexBufferDesc;

typedef struct LupinAliasTableDesc {
    const LupinAliasBin *bins;
    uint32_t num_bins;
} LupinAliasTableDesc;

/* Flat restatement of lp::Scene (renderer.rs:17-60) for the software-BVH pipeline. All pointers
 * are host pointers, copied during lupin_hip_scene_create. */
typedef struct LupinSceneDesc {
    const LupinMeshInfo *mesh_infos;         /* num_meshes entries */
    const LupinMeshDesc *meshes;
    uint32_t num_meshes;

    const LupinVertexBufferDesc *verts_normal_array;
    uint32_t num_normal_buffers;
    const LupinVertexBufferDesc *verts_texcoord_array;
    uint32_t num_texcoord_buffers;
    const LupinVertexBufferDesc *verts_color_array;
    uint32_t num_color_buffers;

    const LupinInstance *instances;
    uint32_t num_instances;
    const LupinMaterial *materials;
    uint32_t num_materials;
    const LupinTextureDesc *textures;
    uint32_t num_textures;
    const LupinEnvironment *environments;
    uint32_t num_environments;

    const LupinTlasNode *tlas_nodes;
    uint32_t num_tlas_nodes;

    const LupinLight *lights;
    uint32_t num_lights;
    const LupinAliasTableDesc *alias_tables;      /* num_lights tables */
    const LupinAliasTableDesc *env_alias_tables;  /* num_environments tables */
} LupinSceneDesc;

/* ------------------------------------------------------------------------------------------
 * Call-surface structs (renderer.rs:451-468, :644-766)
 * ---------------------------------------------------------------------------------------- */

/* renderer.rs:451-468 (defaults false, 8, 5) */
typedef struct LupinBakedPathtraceParams {
    uint32_t with_runtime_checks;   /* accepted, no effect: HIP kernels have no naga bounds checks */
    uint32_t max_bounces;
    uint32_t samples_per_pixel;
} LupinBakedPathtraceParams;

/* renderer.rs:683-708 (defaults 0, .050, .036, 1.5, 10000, 0) */
typedef struct LupinCameraParams {
    uint32_t is_orthographic;
    float lens;
    float film;
    float aspect;
    float focus;
    float aperture;
} LupinCameraParams;

/* renderer.rs:711-729 */
enum LupinPathtraceType {
    LUPIN_PATHTRACE_STANDARD = 0,
    LUPIN_PATHTRACE_MIS = 1,
    LUPIN_PATHTRACE_NAIVE = 2,
    LUPIN_PATHTRACE_DIRECT = 3
};

/* renderer.rs:731-749 (defaults 100, 0, 0.001) */
typedef struct LupinAdvancedParams {
    float max_radiance;
    uint32_t rng_seed;
    float ray_epsilon;
} LupinAdvancedParams;

/* renderer.rs:651-670 (defaults 100, 0) */
typedef struct LupinTileParams {
    uint32_t tile_size;   /* in 4-pixel workgroups */
    uint32_t tile_idx;
} LupinTileParams;

typedef struct LupinContext LupinContext;
typedef struct LupinPathtraceResources LupinPathtraceResources;
typedef struct LupinScene LupinScene;
typedef struct LupinTexture LupinTexture;                     /* one Rgba16Float render target */
typedef struct LupinDoubleBufferedTexture LupinDoubleBufferedTexture;
typedef struct LupinComm LupinComm;                           /* RCCL communicator of one context (multi-GPU gather) */

/* renderer.rs:644-649 */
typedef struct LupinAccumulationParams {
    const LupinTexture *prev_frame;
    uint32_t accum_counter;
} LupinAccumulationParams;

/* renderer.rs:751-766. Option<> fields become nullable pointers. */
typedef struct LupinPathtraceDesc {
    const LupinAccumulationParams *accum_params;   /* NULL = None */
    const LupinTileParams *tile_params;            /* NULL = None (full-screen dispatch) */
    LupinCameraParams camera_params;
    LupinMat3x4 camera_transform;
    uint32_t force_software_bvh;                   /* both values select the software BVH here */
    LupinAdvancedParams advanced;
} LupinPathtraceDesc;

enum LupinStatus {
    LUPIN_OK = 0,
    LUPIN_ERR_INVALID_ARGUMENT = -1,
    LUPIN_ERR_NO_DEVICE = -2,        /* no HIP device / extension unusable: there is NO CPU fallback */
    LUPIN_ERR_HIP = -3,
    LUPIN_ERR_NO_SW_BVH = -4,        /* renderer.rs:774-777 */
    LUPIN_ERR_TILE_OUT_OF_RANGE = -5,/* renderer.rs:814 */
    LUPIN_ERR_SAME_TARGET = -6,      /* render_target == prev_frame, renderer.rs:754-755 */
    LUPIN_ERR_OUT_OF_MEMORY = -7,
    LUPIN_ERR_RCCL = -8              /* librccl missing or a collective failed (multi-GPU gather only) */
};

/* ------------------------------------------------------------------------------------------
 * Entry points
 * ---------------------------------------------------------------------------------------- */

const char *lupin_hip_last_error(void);
/* number of visible HIP devices; 0 when none (never initialises a context) */
int lupin_hip_device_count(void);

/* wgpu device/queue acquisition (wgpu_utils.rs:20-120, renderer.rs:307-330) -> one HIP device + its streams.
 * Like a wgpu queue, the context orders work in call order: consecutive pathtrace_scene calls may overlap on the
 * device (they run on alternating internal streams), but each call sees the textures exactly as the calls before it
 * left them; uploads, downloads, copies and lupin_hip_sync wait for everything submitted earlier. */
int lupin_hip_create_context(int device_ordinal, LupinContext **out_ctx);
/* Destroying a context twice is a no-op.  Textures, scenes and communicators may be destroyed after their context (their
 * device memory is freed then); every other use of an object whose context is gone returns LUPIN_ERR_INVALID_ARGUMENT
 * instead of touching freed memory. */
void lupin_hip_destroy_context(LupinContext *ctx);
/* device.poll(wait_indefinitely) (loader.rs:1692,1825) */
int lupin_hip_sync(LupinContext *ctx);

/* f32 -> f16 rounding of the Rgba16Float store (pathtracer.wgsl:288).  WGSL leaves it to the device;
 * the reference's golden renders are reproduced by round-toward-zero, which is the
 * default.  mode: 0 = toward zero, 1 = nearest even. */
#define LUPIN_STORE_ROUND_TOWARD_ZERO 0
#define LUPIN_STORE_ROUND_NEAREST_EVEN 1
int lupin_hip_set_f16_store_rounding(LupinContext *ctx, int mode);

/* Frames per wavefront.  pathtrace_scene is enqueue-and-return like the reference's queue.submit
 * (renderer.rs:841); consecutive calls that differ only in camera and accum_counter and chain their textures (each call's
 * prev_frame is the previous call's render_target -- the reference's front / back / flip loop) are recorded and executed
 * as ONE wavefront of up to `frames` calls: the stage kernels see `frames` times as many paths per launch, the resolve
 * applies the calls' blends per pixel in call order.  Same texels as one wavefront per call, bit for bit.  A batch runs
 * when it is full or as soon as anything needs its result: lupin_hip_sync, texture download / upload / copy, tonemap, pack /
 * gather, falsecolor / debug calls, statistics, a call that cannot join (other scene / integrator / size / parameters /
 * texture chain), a mode setter, teardown of any object.  An error of a recorded call is reported by the call that runs the
 * batch, with its own code and message; that call then does none of its own work (its outputs are untouched), the batch is
 * dropped, and the same call repeated succeeds.  Teardown has nobody to report to and drops a failing batch silently.
 * frames in [1, 16] (LUPIN_BATCH), or 0 = chosen by dispatch size, the default: sixteen for dispatches of up to 4 M
 * pixels, eight above; 1 = every call is its own wavefront.  f32 accumulation and work
 * counting run unbatched (kernel timing keeps the batches: its launches are the production launches, one lane). */
int lupin_hip_set_batch_frames(LupinContext *ctx, uint32_t frames);

/* Which hierarchy the persistent tracer walks on scenes traversed from global memory (DESIGN.md 5 "Wide traversal").
 * BINARY (default): the reference's own visiting order for every query.  WIDE: the four-wide collapse of the reference's
 * trees with an exactness certificate; queries it cannot certify are re-traced in the reference's order
 * (LupinStats.wide_queries / wide_retraced).  Same images either way; the wide form needs 40 % fewer memory requests
 * per ray and is measured NOT to be faster on MI355X (the tracer is not request-bound), so it is the opt-in.
 * LUPIN_TRAVERSAL=wide sets it at context creation.  Takes effect with the next pathtrace call. */
enum LupinTraversalMode { LUPIN_TRAVERSAL_BINARY = 0, LUPIN_TRAVERSAL_WIDE = 1 };
int lupin_hip_set_traversal(LupinContext *ctx, int mode);

/* lp::build_pathtrace_resources (renderer.rs:470-642): bakes max_bounces / samples_per_pixel */
/* pathtracer.wgsl:275-289 accumulates into an Rgba16Float texture: the running mean is re-quantised to f16 every frame
 * (and stalls once 1/k drops under half an ulp).  LUPIN_ACCUM_F16_RUNNING_AVERAGE reproduces that bit for bit
 * (default); LUPIN_ACCUM_F32 runs the same recurrence on an f32 shadow of each texture (16 B per pixel, allocated on first
 * use) and stores the rounded f16 view, so lupin_hip_texture_download_rgba16f keeps working and
 * lupin_hip_texture_download_rgba32f returns the unquantised mean.  The multi-GPU gather moves the f16 view only. */
enum LupinAccumulationMode { LUPIN_ACCUM_F16_RUNNING_AVERAGE = 0, LUPIN_ACCUM_F32 = 1 };
int lupin_hip_set_accumulation_mode(LupinContext *ctx, int mode);
/* Optional: allocate the path state of every frame in flight up front (dispatches of up to `pixels` pixels, baked
 * max_bounces / samples_per_pixel as in lupin_hip_build_pathtrace_resources).  Without it each of the context's lanes
 * allocates at its first pathtrace call, i.e. inside the first frames of the host's loop.  No counterpart in the reference
 * (wgpu allocates its storage buffers in build_pathtrace_resources, renderer.rs:451-640). */
int lupin_hip_reserve_path_state(LupinContext *ctx, uint64_t pixels, uint32_t max_bounces, uint32_t samples_per_pixel);


int lupin_hip_build_pathtrace_resources(LupinContext *ctx, const LupinBakedPathtraceParams *params,
                                        LupinPathtraceResources **out_res);
void lupin_hip_destroy_pathtrace_resources(LupinPathtraceResources *res);

/* upload half of lp::build_accel_structures_and_upload (data_structures.rs:696-872) */
int lupin_hip_scene_create(LupinContext *ctx, const LupinSceneDesc *desc, LupinScene **out_scene);
/* Moves the instances of a scene in place (no counterpart in the reference, whose Scene is immutable once
 * build_accel_structures_and_upload, data_structures.rs:696-872, has returned): instance i's transform becomes
 * transpose_inverse_transforms[i] (the Instance field of renderer.rs:115-124), the TLAS is rebuilt over the model boxes
 * kept from creation -- tlas_builder 0: lupin_build_tlas, 1: lupin_hip_build_tlas_device, the same tree -- and written over
 * the old one together with the instance rows, the traversal-stack depth and the lights' cull spheres.  mesh_idx, mat_idx,
 * the instance count, materials, textures and environments stay, and with them the light list and every alias table.
 * Ordering: pathtrace calls recorded before the update run first and render the old transforms; the call returns once the
 * new ones are in place.  Errors leave the scene exactly as it was: LUPIN_ERR_INVALID_ARGUMENT for a count other than the
 * scene's, a transform that gives a non-finite world box, a builder error or a tree too deep for the LDS traversal stack;
 * LUPIN_ERR_NO_SW_BVH for a scene created without TLAS; whatever a recorded call fails with.
 * The four-wide hierarchy (lupin_hip_set_traversal) is not rebuilt: after an update, rendering this scene with the wide
 * traversal selected and lupin_hip_trace_rays_wide return LUPIN_ERR_INVALID_ARGUMENT until the scene is created anew. */
int lupin_hip_scene_update_instances(LupinScene *scene, const LupinMat4x3 *transpose_inverse_transforms /* num_instances */,
                                     uint32_t num_instances, int tlas_builder /* 0 = CPU, 1 = device */);
/* The TLAS the scene is traversed with, in lupin_build_tlas' format (what creation was given, or what the latest update
 * built): returns the node count (2 * instances; out_nodes may be NULL to query it) or LUPIN_ERR_INVALID_ARGUMENT when
 * capacity is smaller. */
int64_t lupin_hip_scene_get_tlas(const LupinScene *scene, LupinTlasNode *out_nodes, uint64_t capacity);
void lupin_hip_scene_destroy(LupinScene *scene);

/* Rgba16Float render targets + lp::DoubleBufferedTexture (wgpu_utils.rs:279-348) */
int lupin_hip_texture_create(LupinContext *ctx, uint32_t width, uint32_t height, LupinTexture **out_tex);
void lupin_hip_texture_destroy(LupinTexture *tex);
uint32_t lupin_hip_texture_width(const LupinTexture *tex);
uint32_t lupin_hip_texture_height(const LupinTexture *tex);
/* raw device pointer of the W*H*4 half-float payload (row-major, row 0 = top) for zero-copy
 * wrapping by the host (e.g. RCCL gather of tile payloads) */
void *lupin_hip_texture_device_ptr(const LupinTexture *tex);
int lupin_hip_texture_upload_rgba16f(LupinTexture *tex, const uint16_t *pixels);
/* readback (loader.rs:1775-1879 download path); synchronises the stream */
/* (H, W, 4) f32 of the texture's f32 accumulator; fails unless the last frame rendered into it used LUPIN_ACCUM_F32 */
int lupin_hip_texture_download_rgba32f(const LupinTexture *tex, float *out_pixels);
int lupin_hip_texture_download_rgba16f(const LupinTexture *tex, uint16_t *out_pixels);

int lupin_hip_dbuf_create(LupinContext *ctx, uint32_t width, uint32_t height,
                          LupinDoubleBufferedTexture **out);          /* wgpu_utils.rs:289 */
void lupin_hip_dbuf_destroy(LupinDoubleBufferedTexture *t);
LupinTexture *lupin_hip_dbuf_front(LupinDoubleBufferedTexture *t);    /* :301 */
LupinTexture *lupin_hip_dbuf_back(LupinDoubleBufferedTexture *t);     /* :306 */
int lupin_hip_dbuf_copy_front_to_back(LupinDoubleBufferedTexture *t); /* :321 */
void lupin_hip_dbuf_flip(LupinDoubleBufferedTexture *t);              /* :334 */
int lupin_hip_dbuf_resize(LupinDoubleBufferedTexture *t, uint32_t width, uint32_t height); /* :341 */

/* lp::get_num_tiles (renderer.rs:675-681) */
uint32_t lupin_hip_get_num_tiles(uint32_t tile_size, uint32_t width, uint32_t height);

/* lp::pathtrace_scene (renderer.rs:768-842): enqueues one accumulation frame (or one tile of it) and returns, like
 * queue.submit (:841).  render_target must differ from accum_params->prev_frame (:754-755). */
int lupin_hip_pathtrace_scene(LupinContext *ctx, const LupinPathtraceResources *res,
                              const LupinScene *scene, LupinTexture *render_target,
                              uint32_t pathtrace_type, const LupinPathtraceDesc *desc);

/* renderer.rs:843-870 FalsecolorType */
enum LupinFalsecolorType {
    LUPIN_FALSECOLOR_ALBEDO = 0, LUPIN_FALSECOLOR_NORMALS = 1, LUPIN_FALSECOLOR_NORMALS_UNSIGNED = 2,
    LUPIN_FALSECOLOR_FRONT_FACING = 3, LUPIN_FALSECOLOR_EMISSION = 4, LUPIN_FALSECOLOR_ROUGHNESS = 5,
    LUPIN_FALSECOLOR_METALLIC = 6, LUPIN_FALSECOLOR_OPACITY = 7, LUPIN_FALSECOLOR_MAT_TYPE = 8,
    LUPIN_FALSECOLOR_IS_DELTA = 9, LUPIN_FALSECOLOR_INSTANCE = 10, LUPIN_FALSECOLOR_TRI = 11
};
/* lp::pathtrace_scene_falsecolor (renderer.rs:872-948; shader entry pathtrace_falsecolor_main,
 * pathtracer.wgsl:296-452): G-buffers for denoisers and visual debugging.  Same dispatch / tiling / accumulation
 * rules as lupin_hip_pathtrace_scene. */
int lupin_hip_pathtrace_scene_falsecolor(LupinContext *ctx, const LupinPathtraceResources *res,
                                         const LupinScene *scene, LupinTexture *render_target,
                                         uint32_t falsecolor_type, const LupinPathtraceDesc *desc);

/* renderer.rs:951-964  DebugVizType / DebugVizDesc */
enum LupinDebugVizType { LUPIN_DEBUG_VIZ_BVH_AABB_CHECKS = 0, LUPIN_DEBUG_VIZ_BVH_TRI_CHECKS = 1, LUPIN_DEBUG_VIZ_NUM_BOUNCES = 2 };
typedef struct LupinDebugVizDesc
{
    uint32_t viz_type;        /* LupinDebugVizType */
    float    heatmap_min;
    float    heatmap_max;
    uint32_t first_hit_only;  /* bool */
} LupinDebugVizDesc;

/* renderer.rs:966-1041  lp::pathtrace_scene_debug(device, queue, resources, scene, render_target, debug_desc, desc):
 * pathtrace_debug_main (pathtracer.wgsl:457-503) -- per pixel ONE sample of the first closest-hit query (first_hit_only,
 * except for NumBounces) or of the whole Standard path; the number of box tests / triangle tests / surface hits becomes
 * a heat-map colour (get_heatmap_color, :2806-2872).  Same tiling, accumulation and error rules as pathtrace_scene;
 * baked samples_per_pixel is ignored as in the reference. */
int lupin_hip_pathtrace_scene_debug(LupinContext *ctx, const LupinPathtraceResources *res, const LupinScene *scene,
                                    LupinTexture *render_target, const LupinDebugVizDesc *debug_desc,
                                    const LupinPathtraceDesc *desc);

/* Tile-sharded variant for multi-GPU rendering (extension; the reference renders tiles one
 * sub-dispatch at a time on one device, renderer.rs:807-829): renders, in ONE wavefront launch,
 * every tile t of the frame that lupin_tile_owner(t, tiles_x, world) of include/lupin_tiles.h gives to `rank`
 * (round-robin t % world; rows rotated when a row holds a multiple of `world` tiles) (tiles of tile_size*4 pixels, numbered
 * row-major as renderer.rs:816-817).  Edge tiles cover all in-bounds pixels, so the union over
 * ranks equals the full-screen dispatch bit for bit.  desc->tile_params is ignored. */
int lupin_hip_pathtrace_scene_tiles(LupinContext *ctx, const LupinPathtraceResources *res,
                                    const LupinScene *scene, LupinTexture *render_target,
                                    uint32_t pathtrace_type, const LupinPathtraceDesc *desc,
                                    uint32_t tile_size, uint32_t rank, uint32_t world);

/* ---- denoising (denoising.rs:83-306; the context plays the role of the reference's DenoiseDevice) ----
 * The reference runs OIDN; this library runs a G-buffer-guided edge-avoiding a-trous wavelet filter of its own, in HIP
 * (DESIGN.md 9): albedo demodulation, normal / albedo / luminance-variance edge stopping, 3 / 4 / 5 passes. */

/* denoising.rs:208-218 DenoiseQuality (default High) */
enum LupinDenoiseQuality { LUPIN_DENOISE_LOW = 0, LUPIN_DENOISE_MEDIUM = 1, LUPIN_DENOISE_HIGH = 2 };

/* denoising.rs:193-206 DenoiseDesc.  Every texture is Rgba16Float of the resources' size. */
typedef struct LupinDenoiseDesc {
    const LupinTexture *pathtrace_output;   /* linear colour (required) */
    const LupinTexture *albedo;             /* NULL = None; FalsecolorType Albedo */
    const LupinTexture *normals;            /* NULL = None; FalsecolorType Normals (signed; 0 = background) */
    LupinTexture       *denoise_output;     /* required; may be pathtrace_output (in place, same bits as out of place) */
    uint32_t            quality;            /* LupinDenoiseQuality */
} LupinDenoiseDesc;

typedef struct LupinDenoiseResources LupinDenoiseResources;

/* lp::build_denoise_resources (denoising.rs:83-191): the ping-pong scratch and guides of one width x height
 * (64 bytes per pixel), reusable for any number of denoise calls of that size. */
int lupin_hip_build_denoise_resources(LupinContext *ctx, uint32_t width, uint32_t height, LupinDenoiseResources **out);
/* Drop for DenoiseResources (denoising.rs:71-81): waits for the context's work, then frees the scratch. */
void lupin_hip_destroy_denoise_resources(LupinDenoiseResources *res);
/* lp::denoise (denoising.rs:220-306).  Checks what the reference asserts (:226-237: every given texture has the
 * resources' size) plus NULL colour / output textures, quality > 2 and objects of another or a destroyed context:
 * LUPIN_ERR_INVALID_ARGUMENT, nothing written.  Recorded pathtrace calls run first (their targets may be the inputs); the
 * filter is enqueued on the context's primary stream after every frame enqueued so far and the call returns without a
 * host stall (the reference stalls, :258).  Output: f16 rounded to nearest even, alpha copied from pathtrace_output; the
 * output's f32 accumulator becomes invalid (lupin_hip_texture_download_rgba32f of it fails). */
int lupin_hip_denoise(LupinContext *ctx, LupinDenoiseResources *res, const LupinDenoiseDesc *desc);

/* ---- adaptive sampling (no reference counterpart) ----
 * Renders only the pixels of active 8x8 blocks.  Per pixel p the resources keep n_p, the frames p has taken since the
 * latest reset, and f32 Welford moments (mean_p, M2_p) of the frame luminance (0.2126 r + 0.7152 g) + 0.0722 b.
 * For one call with accum_params {prev, base}:
 *   active p:   exactly what lupin_hip_pathtrace_scene with accum_counter = base + n_p renders at p (same seed, blend,
 *               f16 rounding / f32 accumulator); then n_p += 1 and the moments take the frame's clamped spp-average
 *   inactive p: prev's texel copied bit for bit (f32 mode: prev's f32 value if valid, else its f16 texel widened)
 * After the frame, on the device: e_p = +inf if n_p < 2 or a moment is not finite, else
 * sqrt(M2_p / (n_p (n_p - 1))) / (mean_p + 1e-3); E_b = max e_p over the block's in-image pixels; a block converged when
 * E_b < threshold and every n_p >= min_frames; it is active for the next call when it or one of its 8 neighbours has
 * not converged, and not every n_p has reached max_frames (0 = no cap).  threshold 0: nothing converges.
 * Ping-ponging a double-buffered texture therefore gives, at every pixel, the ordinary sequence's image at that
 * pixel's own frame count.  Memory: 12 B per pixel + 14 B per block. */
typedef struct LupinAdaptiveParams {
    float    threshold;     /* relative standard error a block must fall below (>= 0; 0 = never converge) */
    uint32_t min_frames;    /* frames every pixel of a block takes before it may stop */
    uint32_t max_frames;    /* 0 = no cap */
} LupinAdaptiveParams;

typedef struct LupinAdaptiveStats {
    uint64_t active_pixels;     /* in-image pixels of the blocks the next call renders */
    uint64_t pixel_frames;      /* sum of n_p: pixel-frames rendered since the latest reset */
    uint32_t calls;             /* adaptive calls since the latest reset */
    uint32_t max_frames_taken;  /* max n_p */
} LupinAdaptiveStats;

typedef struct LupinAdaptiveResources LupinAdaptiveResources;

/* State for one width x height, reset (every block active, counts and moments 0). */
int lupin_hip_build_adaptive_resources(LupinContext *ctx, uint32_t width, uint32_t height, LupinAdaptiveResources **out);
/* Waits for the context's work, then frees the state. */
void lupin_hip_destroy_adaptive_resources(LupinAdaptiveResources *res);
/* Counts and moments 0, every block active: call it where accum_counter goes back to 0 (camera or scene changed).
 * Enqueued after every frame so far. */
int lupin_hip_adaptive_reset(LupinContext *ctx, LupinAdaptiveResources *res);
/* One adaptive frame.  LUPIN_ERR_INVALID_ARGUMENT, nothing written, for: a NULL argument, accum_params or its prev_frame
 * missing, tile_params given, render_target / prev_frame / resources of different sizes, objects of another context,
 * a NaN or negative threshold, an unknown pathtrace_type.  prev_frame == render_target: LUPIN_ERR_SAME_TARGET.
 * Recorded pathtrace calls run first; the call is one wavefront of its own, ordered after the previous call's update. */
int lupin_hip_pathtrace_scene_adaptive(LupinContext *ctx, const LupinPathtraceResources *res, const LupinScene *scene,
                                       LupinTexture *render_target, uint32_t pathtrace_type, const LupinPathtraceDesc *desc,
                                       LupinAdaptiveResources *ares, const LupinAdaptiveParams *params);
/* Synchronises. */
int lupin_hip_adaptive_stats(LupinContext *ctx, const LupinAdaptiveResources *ares, LupinAdaptiveStats *out);
/* Any pointer may be NULL; synchronises.  frames: W*H u32; moments: W*H*2 f32 (mean, M2); block_error (f32, +inf = no
 * estimate) and block_active (u8): ceil(W/8) * ceil(H/8), row-major. */
int lupin_hip_adaptive_download(LupinContext *ctx, const LupinAdaptiveResources *ares, uint32_t *frames, float *moments,
                                float *block_error, uint8_t *block_active);

/* ---- reprojection of the adaptive history (no reference counterpart) ----
 * When the camera or an instance moves, lupin_hip_adaptive_reproject rewrites the accumulated image and the adaptive state
 * for the new view, so that the next lupin_hip_pathtrace_scene_adaptive call continues every pixel from the history of the
 * surface point it now shows instead of from zero samples (the alternative: lupin_hip_adaptive_reset).  One call
 *   1. traces the pinhole ray through every pixel centre of the new view (camera_ray with zero jitter and zero aperture;
 *      opacity is not consulted: cut-outs count as opaque) and records instance | global triangle | u, v | camera-space z;
 *   2. per hit pixel: local point v0 (1 - u - v) + v1 u + v2 v -> world as the instance stood when history_in was rendered
 *      (prev_instance_transforms, or the scene's current rows) -> the previous call's camera space -> its continuous
 *      pixel coordinates, snapped to 1/64 pixel -> bilinear 2 x 2 taps of history_in and the adaptive state.  A tap counts
 *      when it lies inside the image with a bilinear weight > 0, its n_q >= 1, the previous view saw the same instance
 *      there and |z_prev[q] - z| <= depth_tolerance * z.  With W the sum of the counting weights:
 *        colour = sum w c_q / W,  n = min n_q (capped at max_history),  mean = sum w mean_q / W,
 *        M2 = sum w s_q / W with s_q = M2_q where n_q == n, else (M2_q / n_q) n.
 *      A pixel whose ray missed, whose point lies behind the previous camera or with W == 0 (disoccluded), and every pixel
 *      of the first call after the resources were built or invalidated, takes n = 0, zero moments and texel (0, 0, 0, 1);
 *   3. the adaptive resources' counts and moments take the gathered values, every block becomes active with no error
 *      estimate and cleared flags, the statistics are recomputed (active pixels = W H, sum and max of n_p), and the new
 *      view's visibility and camera become the previous ones.
 * Colour is read from history_in's f32 accumulator when that is valid, else from its f16 texel, and stored to history_out
 * as f16 rounded to nearest even whatever lupin_hip_set_store_rounding says (toward zero would darken the image by up to
 * 2^-11 per call); in f32 accumulation mode it also goes to history_out's accumulator, which becomes valid (otherwise
 * invalid).  An unmoved view copies history_in, n_p and the moments exactly at every hit pixel.
 * Memory: two visibility buffers of 20 B per pixel and 12 B per pixel of gather output: 52 B per pixel, plus 48 B per
 * instance on the device and twice that in pinned host memory.
 * Out of scope: tiles and multi-GPU (whole frames of one device only); reprojection of background pixels (a miss starts
 * afresh); motion of anything but the camera and instance transforms (deforming meshes, materials, lights, environments:
 * invalidate or reset); depth of field in the reprojection itself (both views are taken as pinhole views). */
typedef struct LupinReprojectResources LupinReprojectResources;

typedef struct LupinReprojectDesc {
    LupinCameraParams camera_params;      /* the NEW view */
    LupinMat3x4       camera_transform;
    float             ray_epsilon;        /* as advanced.ray_epsilon */
    float             depth_tolerance;    /* relative; finite, >= 0 */
    uint32_t          max_history;        /* 0 = no cap; else n_p <= max_history after the call */
    const LupinMat4x3 *prev_instance_transforms;  /* NULL = no instance moved; else num_instances entries in
                                                     lupin_hip_scene_update_instances' format: what the scene held
                                                     when history_in was rendered */
    uint32_t          num_instances;
} LupinReprojectDesc;

/* State for one width x height; no previous view yet. */
int lupin_hip_build_reproject_resources(LupinContext *ctx, uint32_t width, uint32_t height, LupinReprojectResources **out);
/* Waits for the context's work, then frees the state. */
void lupin_hip_destroy_reproject_resources(LupinReprojectResources *res);
/* Forgets the previous view: the next lupin_hip_adaptive_reproject gives n = 0 everywhere.  Call it wherever
 * lupin_hip_adaptive_reset is called. */
int lupin_hip_reproject_invalidate(LupinContext *ctx, LupinReprojectResources *res);
/* LUPIN_ERR_INVALID_ARGUMENT, nothing written, for: a NULL argument, textures or resources of different sizes, objects of
 * another context, a non-finite or negative depth_tolerance, num_instances other than the scene's when transforms are
 * given, a previous transform whose inverse is not finite.  history_in == history_out: LUPIN_ERR_SAME_TARGET.  A scene
 * without TLAS would give LUPIN_ERR_NO_SW_BVH as in the other entry points; lupin_hip_scene_create makes no such scene.
 * Recorded pathtrace calls run first (their target may be history_in); the work is enqueued on the context's primary
 * stream after every frame enqueued so far and the call returns without waiting for the device, with two exceptions: a
 * call whose scene has more instances than any earlier call's on these resources reallocates the instance rows and waits
 * for the stream, and a third call in flight waits for the first one's copy of them.  The host inverts one 3x4 matrix per
 * instance in every call. */
int lupin_hip_adaptive_reproject(LupinContext *ctx, LupinAdaptiveResources *ares, LupinReprojectResources *res, const LupinScene *scene,
                                 const LupinReprojectDesc *desc, const LupinTexture *history_in, LupinTexture *history_out);
/* Device time in milliseconds of the latest call's trace kernel and gather kernel (hipEvents around each launch), when that
 * call ran after lupin_hip_stats_reset(ctx, LUPIN_STATS_KERNEL_TIMING); LUPIN_ERR_INVALID_ARGUMENT otherwise.  Waits for
 * the gather. */
int lupin_hip_reproject_timings(LupinContext *ctx, const LupinReprojectResources *res, float *trace_ms, float *gather_ms);
/* The visibility buffer of the latest call's view (which = 0) or of the call before it (1); any pointer may be NULL;
 * synchronises.  inst (HIT_MISS = 0xFFFFFFFF), tri (global triangle: the scene's meshes' triangles in order) and depth:
 * W*H each; uv: W*H*2. */
int lupin_hip_reproject_download(LupinContext *ctx, const LupinReprojectResources *res, int which, uint32_t *inst, uint32_t *tri, float *uv,
                                 float *depth);

/* ---- measurement hooks (no reference counterpart; the reference exposes none) ---- */

typedef struct LupinStats {
    uint64_t path_bounces;      /* integrator iterations that issued a closest-hit query (metric unit) */
    uint64_t paths;             /* camera samples started */
    uint64_t extend_launches;   /* launches of the dominant (extend) kernel */
    double extend_ms;           /* summed hipEvent duration of those launches (0 unless timing on) */
    double shade_ms;
    double total_ms;            /* whole pathtrace_scene device time (timing on) */
    /* LUPIN_STATS_WORK_COUNTERS: work done by the tracing kernels in this build's layout, per tracing mode
     * [0] closest hit of the integrator loop, [1] MIS / Direct shadow rays, [2] light-pdf marching:
     * internal-node visits (= the oracle's box tests / 2; one 64-byte node fetch each), triangle tests (one 48-byte
     * record each), instance entries (64 bytes) */
    uint64_t node_visits[3];
    uint64_t tri_tests[3];
    uint64_t instance_entries[3];
    uint64_t wide_node_visits[3];   /* visits of four-wide nodes (one 128-byte fetch each) */
    /* how the persistent tracer's waves spent their scheduling rounds (closest-hit mode, first pass): refill rounds | node
     * rounds, node steps, lanes summed over the node steps | triangle rounds, lanes | instance rounds, lanes | end-of-
     * traversal rounds, lanes.  lanes / (64 x steps or rounds) = lane utilisation of that phase. */
    uint64_t tracer_rounds[10];
    /* shader-clock cycles (s_memtime, summed over the waves) spent in refill | node | triangle | instance | end-of-traversal
     * rounds and in the whole scheduling loop (the work-counting build waits for each round's loads before reading the clock) */
    uint64_t tracer_cycles[6];
    /* The first pass of a two-pass tracer (always counted) -- the four-wide tracer, or the binary tracer on its short stack:
     * queries it took, and how many of them it handed to the full-stack binary tracer (uncertified wide results; stack
     * overflows) -- the fallback rate is wide_retraced / wide_queries. */
    uint64_t wide_queries;
    uint64_t wide_retraced;
    /* LUPIN_VERIFY_WIDE=1: every query also run binary-vs-wide on the device, one ray per lane: rays checked, rays the wide
     * traversal flagged, unflagged rays whose result differed (must be 0), rays that differed flag or not */
    uint64_t verify_checked, verify_flagged, verify_mismatches, verify_raw_mismatches;
    uint64_t verify_reasons[4];     /* flagged rays by reason: second hit within the margin | ill-conditioned hit | triangle outside a box above it | stack bound */
    uint32_t frames_in_flight;      /* lanes the latest pathtrace call could use */
    uint32_t wide_traversal;        /* 1 = the latest pathtrace call ran the four-wide tracer */
    uint32_t frames_per_wavefront;  /* recorded calls the latest wavefront carried (lupin_hip_set_batch_frames) */
    uint32_t short_stack_entries;   /* stack entries per lane of the binary tracer's first pass in the latest wavefront; 0 = one pass on the full stack */
} LupinStats;
enum LupinStatsMode {
    LUPIN_STATS_PLAIN = 0,           /* path-bounce / path counters only (always on) */
    LUPIN_STATS_KERNEL_TIMING = 1,   /* + hipEvents around every extend / shade launch (frames run one at a time) */
    LUPIN_STATS_WORK_COUNTERS = 2    /* + the work-counting instantiation of the tracing kernels */
};
/* reset the counters and choose the mode for the calls that follow */
int lupin_hip_stats_reset(LupinContext *ctx, int mode);
/* synchronises, then reports totals since the last reset */
int lupin_hip_stats_get(LupinContext *ctx, LupinStats *out);

/* Device-to-device copy of `bytes` bytes, `reps` times, on the context's stream: (bytes read + bytes written) / time in
 * GB/s -- the measured HBM peak that bench.py reports next to the nominal 8 TB/s.  Synchronous. */
int lupin_hip_measure_copy_bandwidth(LupinContext *ctx, uint64_t bytes, uint32_t reps, double *out_gb_per_s);

/* Which HIP runtime serves this process: the version the library was built against (HIP_VERSION), the version of the
 * libamdhip64 that is bound, and every distinct libamdhip64 mapped (a PyTorch wheel bundles its own; two in one process
 * make lupin_hip_create_context fail, and LUPIN_GRAPH=1 additionally requires build and runtime major.minor to agree). */
typedef struct LupinRuntimeInfo {
    int32_t  build_hip_version;
    int32_t  runtime_hip_version;
    uint32_t num_hip_runtimes_mapped;
    char     hip_runtime_paths[1012];   /* ';'-separated */
} LupinRuntimeInfo;
int lupin_hip_runtime_info(LupinRuntimeInfo *out);

/* Standalone closest-hit probe over a ray batch: the traversal kernel alone
 * (bvh_custom.wgsl:7-110). Host arrays; n rays; outputs hit(0/1), dst, u, v, instance, tri. */
int lupin_hip_trace_rays(LupinContext *ctx, const LupinScene *scene, uint32_t n,
                         const float *ori_xyz, const float *dir_xyz, float ray_epsilon,
                         uint32_t *out_hit, float *out_dst, float *out_uv,
                         uint32_t *out_instance, uint32_t *out_tri);

/* The same probe through the four-wide traversal the persistent tracer runs by default on scenes traversed from global
 * memory (DESIGN.md 5 "Wide traversal"): out_needs_retrace[i] = 1 when the traversal could not certify that ray's result
 * (the pipeline re-traces such a query with the binary kernel; the other outputs of that ray are then unspecified);
 * every other ray's outputs equal lupin_hip_trace_rays' bit for bit.  Scenes staged in LDS have no wide hierarchy
 * (LUPIN_ERR_INVALID_ARGUMENT). */
int lupin_hip_trace_rays_wide(LupinContext *ctx, const LupinScene *scene, uint32_t n,
                              const float *ori_xyz, const float *dir_xyz, float ray_epsilon,
                              uint32_t *out_hit, float *out_dst, float *out_uv,
                              uint32_t *out_instance, uint32_t *out_tri, uint32_t *out_needs_retrace);

/* Evaluates one function of include/lupin_detmath.h (fn: 0 sin, 1 cos, 2 atan, 3 atan2(x,y), 4 acos,
 * 5 exp, 6 log, 7 pow(x,y), 8 x/y, 9 sqrt) on the device over host arrays; the tests require the
 * result to be bit-identical to the host build of the same header. */
int lupin_hip_detmath_probe(LupinContext *ctx, int fn, uint32_t n, const float *x, const float *y, float *out);

/* Scattering-function probe: evaluates the device BSDF, delta-lobe, phase-function and homogeneous-medium functions
 * (pathtracer.wgsl:1789-1949 sample_*, :1951-2095 eval_*, :2097-2229 *_pdf, :2231-2422 delta / scattering /
 * transmittance) over n host records.  The tests require the result to be bit-identical to oracle_scatter_probe.
 *
 * Input record, LUPIN_SCATTER_IN_FLOATS floats:
 *   [0] material type (LupinMatType, as a float)   [1] mode (LupinScatterMode, as a float)
 *   [2..4] color  [5] roughness (as the material point stores it: already squared)  [6] metallic  [7] ior
 *   [8..10] density  [11..13] scattering  [14] anisotropy
 *   [15..17] normal  [18..20] outgoing  [21..23] incoming  [24] rnl  [25..26] rn  [27] max distance
 * Output record, LUPIN_SCATTER_OUT_FLOATS floats: [0..2] direction  [3..5] eval  [6] pdf  [7] 0.
 * Modes:
 *   BSDF_SAMPLE   direction = sample_delta(rnl) when the material is delta, else sample_bsdfcos(rnl, rn); eval and pdf
 *                 of the same family (eval_delta / sample_delta_pdf, eval_bsdfcos / sample_bsdfcos_pdf) at it
 *   BSDF_EVAL     the same eval and pdf at the given incoming; direction = incoming
 *   PHASE_SAMPLE  direction = sample_scattering(rn); eval = eval_scattering, pdf = sample_scattering_pdf at it
 *   PHASE_EVAL    the same at the given incoming
 *   MEDIUM_SAMPLE direction = (d, 0, 0) with d = sample_transmittance(density, max distance, rnl, rn[0]);
 *                 eval = eval_transmittance(density, d), pdf = sample_transmittance_pdf(density, d, max distance)
 *   MEDIUM_EVAL   the same with d = incoming[0]
 * Any other mode writes zeros.  Types and modes must be small non-negative integers. */
#define LUPIN_SCATTER_IN_FLOATS 28
#define LUPIN_SCATTER_OUT_FLOATS 8
typedef enum LupinScatterMode
{
    LUPIN_SCATTER_BSDF_SAMPLE = 0,
    LUPIN_SCATTER_BSDF_EVAL = 1,
    LUPIN_SCATTER_PHASE_SAMPLE = 2,
    LUPIN_SCATTER_PHASE_EVAL = 3,
    LUPIN_SCATTER_MEDIUM_SAMPLE = 4,
    LUPIN_SCATTER_MEDIUM_EVAL = 5
} LupinScatterMode;
int lupin_hip_scatter_probe(LupinContext *ctx, uint32_t n, const float *records, float *out);

/* Light-sampling probe: sample_lights (pathtracer.wgsl:2468-2514) and sample_lights_pdf (:2516-2549 with
 * compute_instance_lights_pdf, bvh_custom.wgsl:112-152) of the device over n host records on `scene`, through the
 * geometry accessor the scene's kernels use (staged in LDS, or global memory).  Host arrays in and out; synchronous;
 * calls recorded on the context run first.  The tests require the result to be bit-identical to oracle_light_probe.
 *
 * Input record, LUPIN_LIGHT_IN_FLOATS floats:
 *   [0] mode (LupinLightMode, as a float)  [1..3] pos  [4..6] incoming  [7] ray epsilon
 *   [8] RNG state: the u32's bits stored in the float's place (not a float value)   [9..11] unused
 * Output record, LUPIN_LIGHT_OUT_FLOATS floats:
 *   [0..2] direction  [3] pdf  [4] RNG state afterwards (bits, as in the input)  [5..7] 0.
 * Modes:
 *   SAMPLE  direction = sample_lights(pos) drawn from the record's RNG state; pdf = sample_lights_pdf(pos, direction)
 *   PDF     pdf = sample_lights_pdf(pos, incoming) at the given incoming, which need not have unit length;
 *           direction = incoming, RNG state unchanged
 * Any other mode writes a zero direction and pdf and returns the RNG state unchanged. */
#define LUPIN_LIGHT_IN_FLOATS 12
#define LUPIN_LIGHT_OUT_FLOATS 8
typedef enum LupinLightMode
{
    LUPIN_LIGHT_SAMPLE = 0,
    LUPIN_LIGHT_PDF = 1
} LupinLightMode;
int lupin_hip_light_probe(LupinContext *ctx, const LupinScene *scene, uint32_t n, const float *records, float *out);

/* Surface probe: what runs between a hit and the scattering functions -- sample_texture (pathtracer.wgsl:1413-1416 with
 * the linear / Repeat sampler of wgpu_utils.rs:244-256), get_material_point (:1265-1342) with vec3f_srgb_to_linear (:2729)
 * and get_vert_color (:1757-1770), compute_shading_normal (:1344-1384) with get_vert_normal (:1730-1755) and
 * compute_tangents_from_uv (:1699-1727), compute_tri_geom_normal (:2561-2576), sample_environments (:1386-1410) with
 * dir_to_env_uv (:2579-2587) -- of the device over n host records on `scene`, through the geometry accessor the scene's
 * kernels use (staged in LDS, or global memory).  Host arrays in and out; synchronous; calls recorded on the context run
 * first.  The tests require the result to be bit-identical to oracle_surface_probe.
 *
 * Input record, LUPIN_SURFACE_IN_FLOATS floats ("bits": the u32's bits stored in the float's place, not a float value):
 *   [0] mode (LupinSurfaceMode, as a float)
 *   [1] instance index (bits), in TEXTURE mode the texture index (bits)
 *   [2] triangle index within the instance's mesh (bits): the numbering lupin_hip_trace_rays returns
 *   [3..4] barycentric u, v of the hit (weights: 1 - u - v, u, v), in TEXTURE mode the texture coordinates u, v
 *   [5..7] direction (ENVIRONMENT mode; it need not have unit length)
 * Output record, LUPIN_SURFACE_OUT_FLOATS floats; what a mode does not name is 0:
 *   TEXTURE          [0..3] sample_texture(texture, (u, v)) rgba, as sampled (no sRGB decode)
 *   MATERIAL         get_material_point: [0] mat_type (bits)  [1..3] emission  [4..6] color  [7] opacity  [8] roughness
 *                    [9] metallic  [10] ior  [11..13] density  [14..16] scattering  [17] sc_anisotropy
 *   MATERIAL_SIMPLE  the same layout from the specialisation the shade kernel uses on a scene of untextured matte
 *                    materials without vertex colours or environments; any other scene: LUPIN_ERR_INVALID_ARGUMENT
 *   OPACITY          [0] the material point's opacity as the tracer's alpha test computes it on its own
 *   NORMAL           [0..2] compute_shading_normal  [3..5] compute_tri_geom_normal
 *   ENVIRONMENT      [0..2] sample_environments(direction)  [3..4] dir_to_env_uv(direction, 0) (0 without environments)
 * Any other mode writes zeros.  An instance, triangle or texture index outside the scene fails the whole call with
 * LUPIN_ERR_INVALID_ARGUMENT before anything is launched. */
#define LUPIN_SURFACE_IN_FLOATS 8
#define LUPIN_SURFACE_OUT_FLOATS 20
typedef enum LupinSurfaceMode
{
    LUPIN_SURFACE_TEXTURE = 0,
    LUPIN_SURFACE_MATERIAL = 1,
    LUPIN_SURFACE_MATERIAL_SIMPLE = 2,
    LUPIN_SURFACE_OPACITY = 3,
    LUPIN_SURFACE_NORMAL = 4,
    LUPIN_SURFACE_ENVIRONMENT = 5
} LupinSurfaceMode;
int lupin_hip_surface_probe(LupinContext *ctx, const LupinScene *scene, uint32_t n, const float *records, float *out);

/* Camera probe: compute_camera_ray (pathtracer.wgsl:505-542) with random_in_disk (:1623-1629) and transform_ray
 * (:2662-2669) of the device over n host records, for an image of width x height pixels.  The camera enters the frame
 * parameters through the code lupin_hip_pathtrace_scene fills them with; camera_transform's first three rows are the
 * LupinMat3x4 a render takes, and its last row, (0, 0, 0, 1) in every render, is passed on as given: the ray does not
 * depend on it (transform_point divides by no w).  Host arrays in and out; synchronous; calls recorded on the context run
 * first.  The tests hold the result to tests/camera_ref.py in float64.
 *
 * Input record, LUPIN_CAMERA_IN_WORDS uint32:  [0] pixel x  [1] pixel y  [2] RNG state  [3] mode (LupinCameraMode)
 * Output record, LUPIN_CAMERA_OUT_FLOATS floats:
 *   [0..2] origin  [3..5] direction  [6] RNG state afterwards (the u32's bits stored in the float's place)  [7] 0.
 * Modes:
 *   RAY         the ray a sample of that pixel starts with: four numbers are drawn from the record's RNG state, two for the
 *               pixel offset, then two for the lens (also at aperture 0)
 *   RAY_CENTRE  the pinhole ray through the pixel centre the reprojection traces: nothing is drawn, aperture 0
 * Any other mode writes zeros and returns the RNG state unchanged.  Pixels need not lie inside the image. */
#define LUPIN_CAMERA_IN_WORDS 4
#define LUPIN_CAMERA_OUT_FLOATS 8
typedef enum LupinCameraMode
{
    LUPIN_CAMERA_RAY = 0,
    LUPIN_CAMERA_RAY_CENTRE = 1
} LupinCameraMode;
int lupin_hip_camera_probe(LupinContext *ctx, uint32_t width, uint32_t height, const LupinCameraParams *camera_params,
                           const LupinMat4 *camera_transform, uint32_t n, const uint32_t *records, float *out);

/* ---- radiance queries (no reference counterpart) ----
 * The full integrators over caller-supplied rays: the radiance arriving along each ray, or at a surface point over its
 * cosine-weighted hemisphere, instead of a camera pixel's texel.
 *
 * Record, LUPIN_RAY_RECORD_FLOATS floats ("bits": the u32's bits stored in the float's place, not a float value):
 *   [0..2] origin   [3] RNG state (bits)   [4..6] unit direction (mode 0) or unit surface normal (mode 1)   [7] mode (bits)
 * Result, LUPIN_RAY_RESULT_FLOATS floats: r, g, b, 1.0f -- the mean of the `samples` per-path radiances, each clamped at
 * advanced.max_radiance as a pixel's samples are, summed in f32 in sample order from zero and divided by (float)samples.
 * Path s of record i is slot i * samples + s.  Its RNG state is the record's word for s == 0 and
 * hash_u32(word + s * 0x9E3779B9) otherwise; it starts at bounce 0, outside any medium, exactly as a camera path does.
 *   LUPIN_RAY_DIRECTION          the direction as given
 *   LUPIN_RAY_COSINE_HEMISPHERE  two numbers drawn from the slot's RNG state, then the matte BSDF's cosine-weighted
 *                                direction about the normal; the origin is the record's (offset it off the surface)
 * out_rays (NULL, or n * samples records): every slot's first ray and its RNG state after the ray's generation, as a mode-0
 * record; querying such a record with samples = 1 replays that one path.
 *
 * The call runs the calls recorded on the context first (and returns their error, if any), then its own wavefronts one
 * after another, and returns when `out` is complete.  (The recorded calls run once the descriptor and the pointers have
 * passed their checks and before the records, the hierarchy's depth and device pointers' contents are looked at: a call
 * refused for those has still run them, one refused for its descriptor or a null pointer has not.)  A wavefront carries at
 * most desc->max_slots paths (0: LUPIN_RAYS_DEFAULT_MAX_SLOTS), rounded down to whole records, at least one record; the path state is sized for that, not for
 * n * samples.  Frames rendered before and after are what they would be without the call.
 *
 * With LUPIN_RAYS_DEVICE_POINTERS in desc->flags, records, out and out_rays are device memory of the context's device,
 * 16-byte aligned, and the caller has finished writing the records; nothing is copied to or from the host.
 *
 * LUPIN_ERR_INVALID_ARGUMENT, nothing traced and `out` untouched, for: a NULL argument; an unknown pathtrace_type, flag or
 * record mode; samples == 0 or above 2^27; max_bounces >= 4095; n * samples above 2^38; a scene of another or of a destroyed
 * context; a record with a non-finite origin, direction or normal; a direction or normal whose squared length is further
 * than 1e-4 from 1; a hierarchy too deep for the traversal stack (as a render).  Host records are checked on the host,
 * device records by a kernel whose count the host reads before the first wavefront.  n == 0: LUPIN_OK, nothing touched.
 * Without a HIP device: LUPIN_ERR_NO_DEVICE. */
#define LUPIN_RAY_RECORD_FLOATS 8
#define LUPIN_RAY_RESULT_FLOATS 4
#define LUPIN_RAYS_DEFAULT_MAX_SLOTS 4194304u   /* paths per wavefront when desc.max_slots is 0: 1.3 GB of path state */
enum { LUPIN_RAY_DIRECTION = 0, LUPIN_RAY_COSINE_HEMISPHERE = 1 };      /* record mode */
enum { LUPIN_RAYS_DEVICE_POINTERS = 1u };                               /* desc.flags  */
typedef struct LupinRayQueryDesc {
    uint32_t pathtrace_type;        /* LupinPathtraceType, all four */
    uint32_t max_bounces;           /* not taken from LupinPathtraceResources: no resources object is needed */
    uint32_t samples;               /* S >= 1 paths per record */
    uint32_t flags;
    uint32_t max_slots;             /* 0 = library default; paths per wavefront */
    LupinAdvancedParams advanced;   /* max_radiance, ray_epsilon as in pathtrace_scene */
} LupinRayQueryDesc;
int lupin_hip_pathtrace_rays(LupinContext *ctx, const LupinScene *scene, const LupinRayQueryDesc *desc,
                             uint64_t n, const float *records /* n x 8 */, float *out /* n x 4 */,
                             float *out_rays /* NULL, or n*S x 8 */);

/* ---- moments of a record's paths (no reference counterpart) ----
 * lupin_hip_pathtrace_rays with another resolve and without out_rays: the descriptor, the flags
 * (LUPIN_RAYS_DEVICE_POINTERS), the records, their validation, the chunks of max_slots paths (whole records), the ordering and
 * every refusal are that call's; the paths traced are the same paths.  Result, LUPIN_RAY_MOMENTS_FLOATS floats per record:
 *   [0..2] mean r, g, b    [3] 1.0f    [4] ml, the mean luminance    [5] M2 = sum over the paths of (lum - ml)^2
 *   [6] (float)samples     [7] 0.0f
 * With c_s the clamped radiance of slot s (what the query with samples == 1 returns for the path), S = samples and
 * lum(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b, every operation one rounded f32 operation without contraction,
 * in this order:
 *   Pass 1.  Lane l = 0..63 takes slots s = l, l + 64, ... in ascending order and adds c_s.r, c_s.g, c_s.b and lum(c_s) to
 *   four partial sums that start from +0.0f.  Each of the four is then summed over the lanes by an xor butterfly over lane
 *   offsets 32, 16, 8, 4, 2, 1: at each offset every lane's value becomes its own plus that of lane ^ offset.
 *   mean_c = sum_c / (float)S,  ml = sum_lum / (float)S.
 *   Pass 2.  The same slots in the same order: q += (lum(c_s) - ml) * (lum(c_s) - ml) from +0.0f, the same butterfly: M2.
 * The mean is therefore lupin_hip_pathtrace_rays' mean summed in another order (the same words for S <= 2).  M2 is taken
 * about the mean in a second pass, not as sum lum^2 - S * ml^2: that difference cancels in f32 exactly where the paths
 * agree.  A record is never split between waves or launches: the words do not depend on max_slots. */
#define LUPIN_RAY_MOMENTS_FLOATS 8
int lupin_hip_pathtrace_rays_moments(LupinContext *ctx, const LupinScene *scene, const LupinRayQueryDesc *desc,
                                     uint64_t n, const float *records /* n x 8 */, float *out /* n x 8 */);

/* ---- lightmap baking (no reference counterpart) ----
 * Irradiance on the scene's surfaces, laid out by the meshes' texcoords: every chart places one instance's UVs in the atlas
 * (atlas uv = mesh uv * scale + offset), its triangles are rasterised to texels, and every owned texel is path-traced over
 * the cosine-weighted hemisphere of the surface point its centre maps to, with `samples` paths, by the radiance query above.
 *
 * Rasterisation, every operation one rounded f32 operation (no contraction).  Vertex k of a triangle in texel space is
 * t_k = ((u_k * scale_u + offset_u) * W, (v_k * scale_v + offset_v) * H); texel (x, y) has the centre c = (x + 0.5, y + 0.5),
 * row 0 is v in [0, 1/H) (no flip).  edge(a, b, p) = (b.x-a.x)*(p.y-a.y) - (b.y-a.y)*(p.x-a.x); area2 = edge(t0, t1, t2);
 * a triangle with a non-finite UV or with area2 zero or not finite is skipped.  e0 = edge(t1, t2, c), e1 = edge(t2, t0, c),
 * e2 = edge(t0, t1, c), all four negated when area2 < 0; the centre is covered when e0, e1, e2 >= 0; u = e1 / area2,
 * v = e2 / area2, weights 1-u-v, u, v.  Only the texels of the triangle's bounding box are looked at: columns
 * floor(clamp(min x, 0, W)) .. min(floor(clamp(max x, 0, W)), W - 1), rows alike -- clamped in float, so UVs of 1e30 or
 * below zero cover nothing inside and never reach an integer.  A covered centre belongs to the smallest key among the
 * triangles covering it; the key of triangle t of chart c is the sum of the triangle counts of the charts before c, plus t
 * (t in the scene's own triangle order: that of the indices handed to lupin_hip_scene_create).
 *
 * The record of an owned texel (a mode-1 record of the query): local point v0*w + v1*u + v2*v, to world through the inverse
 * of the instance's world -> local affine as light sampling computes it; n_g = the geometric normal, reference winding;
 * n = n_g, or with LUPIN_LIGHTMAP_SMOOTH_NORMALS on a mesh with normals the interpolated vertex normal in world space,
 * negated if n . n_g < 0 (normal maps are not applied); origin = world + n_g * surface_offset; RNG word =
 * rng_seed_for(y * W + x, counter).  Records are traced in ascending texel order, empty texels cost no paths.
 *
 * out_rgba (H x W x 4, host): pi * the query's mean radiance and alpha 1.0f on owned texels, zeros elsewhere; then
 * `dilate` gutter passes: a texel not filled yet takes the f32 mean of its filled 8-neighbours (summed dy -1..1 outer,
 * dx -1..1 inner, divided by their count) and counts as filled from the next pass on; its alpha stays 0.
 * out_records (NULL, or H x W x 8, host): every owned texel's record at its place, zeros elsewhere.
 * out_num_covered (NULL ok): the number of owned texels.
 *
 * Ordering as lupin_hip_pathtrace_rays: recorded calls run first (their error is returned), the call returns when out_rgba
 * is complete, frames before and after are unchanged.  LUPIN_ERR_INVALID_ARGUMENT with the outputs untouched for: a NULL
 * argument (out_records and out_num_covered may be NULL); width or height 0 or above LUPIN_LIGHTMAP_MAX_SIZE;
 * num_charts == 0; an instance index out of range; a mesh without texcoords; a non-finite scale or offset; surface_offset not
 * finite and positive; an unknown flag; dilate above LUPIN_LIGHTMAP_MAX_DILATE; 2^32 - 1 or more (chart, triangle) pairs;
 * everything the query refuses (among it a record whose normal is not finite: a triangle with UV area but without area in
 * space).  An atlas without an owned texel: LUPIN_OK, all zeros.  Without a HIP device: LUPIN_ERR_NO_DEVICE. */
#define LUPIN_LIGHTMAP_MAX_SIZE 16384u
#define LUPIN_LIGHTMAP_MAX_DILATE 64u
enum { LUPIN_LIGHTMAP_SMOOTH_NORMALS = 1u };                            /* desc.flags */
typedef struct LupinLightmapChart {     /* one instance's place in the atlas */
    uint32_t instance_idx;
    float scale_u;
    float scale_v;
    float offset_u;
    float offset_v;
} LupinLightmapChart;
typedef struct LupinLightmapDesc {
    uint32_t width;                 /* atlas texels, 1 .. LUPIN_LIGHTMAP_MAX_SIZE */
    uint32_t height;
    uint32_t pathtrace_type;        /* as LupinRayQueryDesc */
    uint32_t max_bounces;
    uint32_t samples;
    uint32_t max_slots;
    uint32_t flags;
    uint32_t dilate;                /* gutter passes, 0 .. LUPIN_LIGHTMAP_MAX_DILATE */
    uint32_t counter;               /* seeds: rng_seed_for(texel linear index, counter) */
    float surface_offset;           /* world units along the geometric normal; finite, > 0 */
    LupinAdvancedParams advanced;
} LupinLightmapDesc;
int lupin_hip_bake_lightmap(LupinContext *ctx, const LupinScene *scene, const LupinLightmapDesc *desc,
                            const LupinLightmapChart *charts, uint32_t num_charts, float *out_rgba /* H*W*4 */,
                            float *out_records /* NULL, or H*W*8 */, uint64_t *out_num_covered /* NULL ok */);
/* The calling thread's latest successful bake, host-clock milliseconds of its phases (each ends synchronised). */
typedef struct LupinLightmapStats {
    uint64_t covered_texels;
    uint32_t keys;                  /* (chart, triangle) pairs rasterised */
    float raster_ms;
    float compact_ms;               /* count, scan, emit */
    float trace_ms;                 /* the radiance query */
    float scatter_dilate_ms;
    float download_ms;
} LupinLightmapStats;
void lupin_hip_lightmap_stats(LupinLightmapStats *out);

/* ---- ambient-occlusion and bent-normal atlases (no reference counterpart) ----
 * Two more channels in the lightmap's atlas.  Rasterisation, ownership, record emission and out_records are
 * lupin_hip_bake_lightmap's, word for word, for the same charts, flags (LUPIN_LIGHTMAP_SMOOTH_NORMALS), counter and
 * surface_offset: the same kernels run.  Every owned texel's record is then queried by lupin_hip_bent_normal_rays' kernel
 * (below) with `samples` slots, ray_epsilon, LUPIN_LIGHTMAP_AO_OPACITY as its OPACITY flag, and max_distance as the tmax of
 * every slot (the record's word [7] stays the radiance query's mode).  With a = the query's four floats for the texel, each
 * operation one rounded f32 operation:
 *   v = a.w / (float)samples                       out_ao texel   = (v, v, v, 1.0f)
 *   len = sqrtf((a.x*a.x + a.y*a.y) + a.z*a.z)     out_bent texel = (a.x / len, a.y / len, a.z / len, 1.0f),
 *                                                  or (n.x, n.y, n.z, 1.0f) with n the record's bake normal where len == 0
 * Texels that are not owned hold zeros in both planes.  Then both planes get `dilate` gutter passes exactly as
 * lupin_hip_bake_lightmap's (the same kernel; gutter alpha stays 0; dilated bent normals are not renormalised).
 * Intermediates stay on the device; only the outputs cross the bus.
 *
 * out_ao (with out_records) is a valid input to lupin_hip_denoise_lightmap, and a valid `lightmap` for
 * lupin_hip_render_lightmapped: both take any H x W x 4 plane with alpha as ownership.
 *
 * Ordering as lupin_hip_bake_lightmap.  LUPIN_ERR_INVALID_ARGUMENT with the outputs untouched for what
 * lupin_hip_bake_lightmap refuses in the atlas, the charts and the records (out_bent, out_records and out_num_covered may be
 * NULL), an unknown flag, samples == 0 or above 2^20, a ray_epsilon that is not finite or is negative, and a max_distance
 * that is NaN or <= 0.  An atlas without an owned texel: LUPIN_OK, all zeros.  Without a HIP device: LUPIN_ERR_NO_DEVICE. */
enum { LUPIN_LIGHTMAP_AO_OPACITY = 2u };                                /* desc.flags, with LUPIN_LIGHTMAP_SMOOTH_NORMALS */
typedef struct LupinLightmapAoDesc {
    uint32_t width;                 /* atlas texels, 1 .. LUPIN_LIGHTMAP_MAX_SIZE */
    uint32_t height;
    uint32_t samples;               /* 1 .. 2^20 slots per texel */
    uint32_t max_slots;             /* as LupinBentNormalDesc */
    uint32_t flags;
    uint32_t dilate;                /* gutter passes, 0 .. LUPIN_LIGHTMAP_MAX_DILATE */
    uint32_t counter;               /* seeds: rng_seed_for(texel linear index, counter) */
    float surface_offset;           /* as LupinLightmapDesc */
    float max_distance;             /* tmax of every slot: > 0; +inf = unbounded; NaN or <= 0 refused */
    float ray_epsilon;              /* finite, >= 0 */
} LupinLightmapAoDesc;
int lupin_hip_bake_lightmap_ao(LupinContext *ctx, const LupinScene *scene, const LupinLightmapAoDesc *desc,
                               const LupinLightmapChart *charts, uint32_t num_charts, float *out_ao /* H*W*4 */,
                               float *out_bent /* NULL, or H*W*4 */, float *out_records /* NULL, or H*W*8 */,
                               uint64_t *out_num_covered /* NULL ok */);

/* ---- directional lightmaps (no reference counterpart) ----
 * lupin_hip_bake_lightmap with four coefficient planes in place of one irradiance plane, so that the lightmapped view can
 * shade a normal map (lupin_hip_render_lightmapped_directional).  Rasterisation, ownership, record emission, out_records and
 * out_num_covered are lupin_hip_bake_lightmap's, word for word, for the same charts, flags (LUPIN_LIGHTMAP_SMOOTH_NORMALS),
 * counter and surface_offset: the same kernels run.  The owned texels' records run through the radiance query's wavefront
 * with `samples` paths each, exactly as lupin_hip_pathtrace_rays runs mode-1 records (pathtrace_type, max_bounces, max_slots
 * and advanced are the query's).  The resolve is this one, per record, with d_s the FIRST direction of slot s (what the
 * query reports in out_rays) and L_s the slot's clamped path radiance (what the query with samples == 1 would return for it):
 *
 *   Y0 = 0.28209479f;  Y1 = 0.48860251f * d.y;  Y2 = 0.48860251f * d.z;  Y3 = 0.48860251f * d.x   (the first four values of
 *   lupin_hip_bake_probes' basis, its literals).  Lane l = 0..63 takes slots s = l, l + 64, ... in ascending order and adds,
 *   from +0.0f, acc[j][c] += L_s[c] * Yj(d_s) for j = 0..3 and c in r, g, b (the product rounded, then the sum).  The 64 lanes'
 *   accumulators are added by an xor butterfly over lane offsets 32, 16, 8, 4, 2, 1: at each offset every lane's value becomes
 *   its own plus that of lane ^ offset.  Coefficient j, channel c = (acc[j][c] * 3.14159265f) / (float)samples, with w = 1.0f.
 *   Every operation is one rounded f32 operation without contraction.  A record is never split between waves or launches:
 *   the words do not depend on max_slots.
 *
 * Coefficient j estimates the integral of L(w) (w . n)+ Yj(w) over the sphere, the L1 projection of the cosine-weighted
 * incident radiance: coefficient 0 / 0.28209479 is lupin_hip_bake_lightmap's irradiance (the same terms, summed in another
 * order), coefficients 1..3 / 0.48860251 are that irradiance times its mean direction's y, z, x.
 *
 * out_sh (LUPIN_LIGHTMAP_DIRECTIONAL_PLANES x H x W x 4, host; plane j first): on owned texels coefficient j's rgb and alpha
 * 1.0f, zeros elsewhere; then `dilate` gutter passes of lupin_hip_bake_lightmap's on each plane (gutter alpha stays 0).
 * Alpha is ownership in every plane, so each is a valid input to lupin_hip_denoise_lightmap.  Intermediates stay on the
 * device.
 *
 * Ordering, refusals (LUPIN_ERR_INVALID_ARGUMENT with the outputs untouched; out_records and out_num_covered may be NULL),
 * the atlas without an owned texel (LUPIN_OK, all zeros) and LUPIN_ERR_NO_DEVICE are lupin_hip_bake_lightmap's.
 * LUPIN_ERR_OUT_OF_MEMORY, outputs untouched, when the planes (64 bytes per texel, twice that with gutter passes) cannot be
 * allocated. */
#define LUPIN_LIGHTMAP_DIRECTIONAL_PLANES 4
int lupin_hip_bake_lightmap_directional(LupinContext *ctx, const LupinScene *scene, const LupinLightmapDesc *desc,
                                        const LupinLightmapChart *charts, uint32_t num_charts, float *out_sh /* 4*H*W*4 */,
                                        float *out_records /* NULL, or H*W*8 */, uint64_t *out_num_covered /* NULL ok */);

/* ---- adaptive lightmap baking (no reference counterpart) ----
 * lupin_hip_bake_lightmap in rounds: desc->samples is S, the paths per texel PER ROUND; a texel stops taking rounds once the
 * relative standard error of its luminance is below ad->threshold and no atlas neighbour wants samples either.
 * Rasterisation, ownership, record emission, out_records, out_num_covered and the `dilate` gutter passes are
 * lupin_hip_bake_lightmap's, word for word, for the same charts, flags, counter and surface_offset: the same kernels run.
 * Record i below is the i-th owned texel in ascending texel order.
 *
 * State per record, zero at the start of the call: n_i (u32 paths), rounds_i (u32), mean_i (r, g, b), ml_i, M2_i.
 * Round r = 0, 1, ... (every operation one rounded f32 operation without contraction):
 *   1. The active records (round 0: all) are compacted in ascending i.  Active record i becomes record j of the round: its
 *      own record with the RNG word replaced by word_r = word for r == 0, else hash_u32(word + r * 0x85EBCA6B) (r is the
 *      round of the call, not rounds_i).  No active record: the loop ends.
 *   2. lupin_hip_pathtrace_rays_moments' query on the round's records with S samples (pathtrace_type, max_bounces, max_slots
 *      and advanced are the query's).  Every round pays that query's validation of its records and its synchronisation.
 *   3. Merge, with (round_c, ml_round, M2_round) the query's result for j and i its record.  n_i == 0: the state becomes
 *      the round's.  Otherwise  nA = (float)n_i;  nB = (float)S;  w = nB / (nA + nB);  delta = ml_round - ml_i;
 *        mean_c = mean_c + (round_c - mean_c) * w  per channel;   ml = ml_i + delta * w;
 *        M2 = (M2_i + M2_round) + ((delta * delta) * nA) * w.
 *      Then n_i += S, rounds_i += 1,
 *        e_i = +inf if n_i < 2 or ml_i or M2_i is not finite, else sqrtf(M2_i / (nf * (nf - 1.0f))) / (ml_i + 1e-3f), nf = (float)n_i
 *      (lupin_hip_pathtrace_scene_adaptive's per-pixel error), and
 *        want_i = rounds_i < max_rounds && (rounds_i < min_rounds || !(e_i < threshold)).
 *   4. Mask: active_i = rounds_i < max_rounds && (want_i || want of any of the texel's eight atlas neighbours inside the
 *      atlas).  Texels that are not owned never want; a neighbour at max_rounds has want == 0 and keeps nobody alive.  (A texel
 *      whose first rounds all returned zero has M2 == 0 and would stop at min_rounds beside a neighbour still finding the light.)
 * Every round adds one to rounds_i of the records it traces and none is active at max_rounds, so the loop ends; a texel that
 * a neighbour woke late is behind the call's round r, so the call may run more than max_rounds rounds.
 *
 * out_rgba (H x W x 4, host): 3.14159265f * mean_c and alpha 1.0f on owned texels, zeros elsewhere, then the gutter passes.
 * out_stats (NULL, or H x W x 4, host; not dilated, zeros where not owned):
 *   [0] (float)n_i   [1] e_i   [2] 3.14159265f * sqrtf(M2_i / (nf * (nf - 1.0f))), the standard error of the irradiance's
 *   luminance, 0.0f when n_i < 2   [3] 1.0f if rounds_i >= min_rounds && e_i < threshold, else 0.0f.
 * With threshold == 0 and min_rounds == max_rounds == R every texel takes R * S paths.
 *
 * Ordering as lupin_hip_bake_lightmap.  LUPIN_ERR_INVALID_ARGUMENT with the outputs untouched for everything
 * lupin_hip_bake_lightmap refuses (out_stats, out_records and out_num_covered may be NULL), a NULL ad, a threshold that is
 * negative or not finite, min_rounds == 0, max_rounds below min_rounds or above LUPIN_LIGHTMAP_ADAPTIVE_MAX_ROUNDS,
 * samples * max_rounds above 2^24 ((float)n_i must be exact), a non-zero ad->flags.  LUPIN_ERR_OUT_OF_MEMORY, outputs
 * untouched and nothing launched, when the atlas planes cannot be allocated.  An atlas without an owned texel: LUPIN_OK, all
 * zeros.  Without a HIP device: LUPIN_ERR_NO_DEVICE. */
#define LUPIN_LIGHTMAP_ADAPTIVE_MAX_ROUNDS 4096u
#define LUPIN_LIGHTMAP_ADAPTIVE_STATS_FLOATS 4
typedef struct LupinLightmapAdaptiveDesc {
    float threshold;                /* finite, >= 0: a texel wants no more samples once its relative standard error is < threshold */
    uint32_t min_rounds;            /* >= 1 */
    uint32_t max_rounds;            /* >= min_rounds, <= LUPIN_LIGHTMAP_ADAPTIVE_MAX_ROUNDS; desc->samples * max_rounds <= 2^24 */
    uint32_t flags;                 /* 0 */
} LupinLightmapAdaptiveDesc;
int lupin_hip_bake_lightmap_adaptive(LupinContext *ctx, const LupinScene *scene, const LupinLightmapDesc *desc,
                                     const LupinLightmapAdaptiveDesc *ad, const LupinLightmapChart *charts, uint32_t num_charts,
                                     float *out_rgba /* H*W*4 */, float *out_stats /* NULL, or H*W*4 */,
                                     float *out_records /* NULL, or H*W*8 */, uint64_t *out_num_covered /* NULL ok */);
/* The calling thread's latest successful adaptive bake; host-clock milliseconds, summed over the rounds (each phase ends
 * synchronised). */
typedef struct LupinLightmapAdaptiveStats {
    uint64_t covered_texels;
    uint64_t paths;                 /* paths traced: S * the sum of the rounds' active records */
    uint64_t converged_texels;      /* out_stats [3] == 1 */
    uint64_t capped_texels;         /* stopped by max_rounds without [3] == 1 */
    uint32_t rounds;                /* rounds that traced */
    uint32_t keys;                  /* (chart, triangle) pairs rasterised */
    float raster_ms;
    float compact_ms;               /* the records' count, scan, emit, and every round's */
    float trace_ms;                 /* the rounds' queries */
    float merge_mask_ms;
    float scatter_dilate_ms;        /* with the statistics plane */
    float download_ms;
} LupinLightmapAdaptiveStats;
void lupin_hip_lightmap_adaptive_stats(LupinLightmapAdaptiveStats *out);

/* ---- lightmap UV sets: a second UV set per mesh, and its generation (no reference counterpart) ----
 * A mesh may carry a LIGHTMAP UV SET beside its material texcoords: one UV per triangle CORNER (3 * triangles float pairs, in
 * the scene's own triangle order), per corner because a vertex on a chart seam needs two coordinates and vertices are not
 * split.  Where the mesh of a chart's instance has a set, every lightmap consumer (lupin_hip_bake_lightmap and its _ao,
 * _directional and _adaptive variants, lupin_hip_render_lightmapped and its _directional variant) takes corner k of
 * triangle t from lm_uvs[3 * t + k] in place of texcoords[index_k]; nothing else about rasterisation, ownership, records, the
 * view's fetch or a chart's scale and offset changes, and material evaluation (albedo, normal maps, opacity) keeps reading
 * the material texcoords.  "A mesh without texcoords" is refused only for a mesh that has neither.
 *
 * lupin_hip_scene_set_lightmap_uvs copies num_corners float pairs to the device (uvs == NULL removes the mesh's set;
 * num_corners is then not looked at).  Non-finite values are allowed: the rasteriser's rule skips such triangles.  Ordering as
 * lupin_hip_scene_update_instances: recorded calls run first and see the previous set.  LUPIN_ERR_INVALID_ARGUMENT, the
 * scene untouched, for a NULL scene, a mesh index out of range, a num_corners that is not three times the mesh's triangle
 * count. */
int lupin_hip_scene_set_lightmap_uvs(LupinScene *scene, uint32_t mesh_idx, const float *uvs /* num_corners x 2, or NULL */,
                                     uint64_t num_corners);
/* The triangle count of a mesh, as the scene holds it: what sizes a lightmap UV set and lupin_hip_unwrap_lightmap_uvs' outputs.
 * LUPIN_ERR_INVALID_ARGUMENT for a NULL scene or a mesh index out of range.  Needs no device. */
int64_t lupin_hip_scene_mesh_triangle_count(const LupinScene *scene, uint32_t mesh_idx);

/* lupin_hip_unwrap_lightmap_uvs generates such a set on the device, from the mesh's local positions and indices where they
 * already live in device memory, and writes host arrays; it does not attach the result.  The unit of the UVs is the texel of
 * the mesh's own atlas of out_info->width x height texels, so a chart with scale = m / W and offset = X / W places the mesh
 * at texel X of a W-wide atlas at m times the resolution.  Every float operation is one rounded f32 operation without
 * contraction, IEEE division; tests/lightmap_unwrap_ref.py restates the rule.
 *
 * Classify.  With p0, p1, p2 the triangle's local positions, a = p1 - p0, b = p2 - p0,
 *   n = (a.y*b.z - a.z*b.y,  a.z*b.x - a.x*b.z,  a.x*b.y - a.y*b.x).
 * The bucket is the axis k of the largest |n_k|, a tie going to the lower axis (x before y before z), with sign + when
 * n_k >= 0: six buckets.  A triangle whose n has a non-finite component or is all zero is DEGENERATE: its chart is
 * LUPIN_UNWRAP_NO_CHART, its UVs are 0 (the rasteriser skips zero area), and it is counted in degenerate_tris.
 *
 * Charts.  Two triangles are linked when they are in the same bucket and share a vertex INDEX; a chart is a connected
 * component.  Its label is the smallest triangle index in it, its dense number (out_chart_of_tri) the rank of its label.
 * (Device: atomicMin of the triangle index on a (bucket, vertex) table of 6 * V words, then a lock-free union-find that
 * always hooks the larger root under the smaller, then a flatten pass: the labels do not depend on scheduling.)
 *
 * Project.  For axis k the plane coordinates of a point p are (s, t) = (p[(k+1)%3] + 0.0f, p[(k+2)%3] + 0.0f), swapped for a
 * negative bucket: every non-degenerate triangle has positive area in the plane, no chart is mirrored.  (+ 0.0f: -0 is +0.)
 *
 * Rectangles.  Per chart the exact min and max of s and of t over its corners; extent = ceilf((max - min) / texel_size), at
 * least 1, per axis; the chart's rectangle is extent + 2 * padding on each side.
 *
 * Pack (host, integers; include/lupin_pack.hpp).  Charts sorted by rectangle height descending, then width descending, then
 * label ascending.  Atlas width = max(widest rectangle, isqrt_ceil(sum of rectangle areas)); rectangles are placed left to
 * right, a new shelf opens when the next rectangle would cross the width; the height is the bottom of the last shelf.
 *
 * UVs.  Corner uv = ((float)(rect.x + padding) + (s - min_s) / texel_size,  (float)(rect.y + padding) + (t - min_t) / texel_size).
 *
 * Known limits.  A chart is a height field over its plane only locally: a helicoid-like patch can overlap itself, and the
 * rasteriser's smallest-key rule then decides who owns the texel.  A mesh with duplicated vertices per face falls into one
 * chart per face.  Stretch reaches sqrt(3) in area at a (1,1,1) normal.  Non-uniform instance scale distorts density.
 *
 * Ordering as lupin_hip_pathtrace_rays: recorded calls run first, the call returns when the outputs are complete.
 * LUPIN_ERR_INVALID_ARGUMENT with the outputs untouched for: a NULL argument (out_chart_of_tri may be NULL); a mesh index out
 * of range; a texel_size that is not finite and positive; padding above LUPIN_UNWRAP_MAX_PADDING; a non-zero flags; an atlas
 * wider or higher than LUPIN_LIGHTMAP_MAX_SIZE.  A mesh without a non-degenerate triangle: LUPIN_OK, 0 charts, 0 x 0.
 * Without a HIP device: LUPIN_ERR_NO_DEVICE. */
#define LUPIN_UNWRAP_MAX_PADDING 16u
#define LUPIN_UNWRAP_NO_CHART 0xFFFFFFFFu
typedef struct LupinUnwrapDesc {
    float texel_size;               /* local units per texel; finite, > 0 */
    uint32_t padding;               /* texels around every chart, 0 .. LUPIN_UNWRAP_MAX_PADDING */
    uint32_t flags;                 /* 0 */
} LupinUnwrapDesc;
typedef struct LupinUnwrapInfo {
    uint32_t num_charts;
    uint32_t width;                 /* the mesh's own atlas, texels */
    uint32_t height;
    uint32_t degenerate_tris;
    float charts_ms;                /* host-clock milliseconds (each phase ends synchronised): classify, union, flatten */
    float rects_ms;                 /* count, scan, compact, and the charts' boxes to the host */
    float pack_ms;                  /* the host's rectangles and shelf packer */
    float uvs_ms;                   /* the origins to the device, the UVs, and the results to the host */
} LupinUnwrapInfo;
int lupin_hip_unwrap_lightmap_uvs(LupinContext *ctx, const LupinScene *scene, uint32_t mesh_idx, const LupinUnwrapDesc *desc,
                                  float *out_uvs /* tris*3*2 */, uint32_t *out_chart_of_tri /* NULL, or tris */,
                                  LupinUnwrapInfo *out_info);

/* ---- lightmap denoising (no reference counterpart) ----
 * An edge-avoiding a-trous filter in atlas space for what lupin_hip_bake_lightmap writes: `rgba` is its out_rgba (or several
 * bakes with different `counter`, averaged by the caller), `records` its out_records.  No scene is needed.  Texel p is
 * OWNED when its alpha != 0.  Its record gives the world-space surface point x_p (floats 0..2) and the bake normal n_p
 * (floats 4..6); the record of a texel that is not owned is never read.  Every float operation below is one rounded f32
 * operation (no contraction, IEEE division and sqrt); sums run dy outer, dx inner.
 *
 * 1. Prep.  p is GUIDED when it is owned, x_p and n_p are finite and | ((nx*nx + ny*ny) + nz*nz) - 1 | <= 1e-4 (the
 *    radiance query's tolerance).  c_p = rgb with non-finite components set to 0.  Luminance l = (0.2126 r + 0.7152 g) +
 *    0.0722 b.  var_p = max(0, s2 / cnt - (s1 / cnt) * (s1 / cnt)) with s1 = sum l_q, s2 = sum l_q * l_q, cnt the count, over
 *    the guided texels q of the in-bounds 3 x 3 neighbourhood of a guided p (dy, dx = -1..1).  The footprint f_p = the
 *    smallest |x_q - x_p|^2 = (ex*ex + ey*ey) + ez*ez, e = x_q - x_p, over the guided 4-neighbours q of p, or 0 without one.
 *
 * 2. `passes` passes, ping-pong; pass i = 0, 1, .. has step 2^i.  For a guided p the taps are q = p + (kx, ky) * 2^i with
 *    kx, ky = -2..2 and h = (1, 4, 6, 4, 1) / 16.  A tap counts only if it is inside the atlas, guided, and, for q != p,
 *      |x_q - x_p|^2 <= (K_i * (kx*kx + ky*ky)) * f_p,   K_i = (max_stretch * max_stretch) * 4^i
 *    -- a neighbour in the atlas that is not a neighbour in space (another chart, across a gutter, behind a fold) is further
 *    away than the texel spacing allows.  Its weight is
 *      w = ((h_kx * h_ky) * w_n) * exp_neg(-(|l_p - l_q| * s_p)),   s_p = 1 / (4 * sqrt(var_p) + 1e-4),
 *      w_n = max((n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z, 0) squared normal_squarings times (the exponent 2^k),
 *    exp_neg being the f32 exponential of lupin_hip_denoise, l of the pass's input.  Then
 *      c'_p = (sum w * c_q) / sum w per channel,   var'_p = (sum (w * w) * var_q) / ((sum w) * (sum w)).
 *    The centre tap always counts, so sum w > 0.  A texel that is not guided keeps c_p through every pass.
 *
 * 3. out_rgba: on owned texels rgb of the last pass and the input's alpha.  On the others, with dilate == 0, the input texel
 *    as it is; with dilate > 0, zeros, then `dilate` gutter passes exactly as lupin_hip_bake_lightmap's, in which the owned
 *    texels count as filled and nothing else does (whatever the bake's own gutter passes left there does not survive); a
 *    filled gutter texel has alpha 0.  out_rgba may be the same memory as rgba.
 *
 * Ordering as lupin_hip_bake_lightmap: recorded calls run first (their error is returned), the call returns when out_rgba
 * is complete, frames before and after are unchanged.  LUPIN_ERR_INVALID_ARGUMENT with out_rgba untouched for: a NULL
 * argument; width or height 0 or above LUPIN_LIGHTMAP_MAX_SIZE; passes 0 or above LUPIN_LIGHTMAP_DENOISE_MAX_PASSES;
 * normal_squarings above LUPIN_LIGHTMAP_DENOISE_MAX_SQUARINGS; dilate above LUPIN_LIGHTMAP_MAX_DILATE; an unknown flag;
 * max_stretch not finite or not positive; a destroyed context; with LUPIN_LIGHTMAP_DENOISE_DEVICE_POINTERS a pointer that
 * is not 16-byte aligned.  LUPIN_ERR_OUT_OF_MEMORY when the scratch (60 bytes per texel, 2 more with gutter passes, 48 more for
 * host arrays) cannot be allocated.  Without a HIP device: LUPIN_ERR_NO_DEVICE.
 * With LUPIN_LIGHTMAP_DENOISE_DEVICE_POINTERS all three pointers are device memory of the context's device and nothing
 * crosses the bus; otherwise they are host arrays.  The scratch stays with the context from call to call. */
#define LUPIN_LIGHTMAP_DENOISE_MAX_PASSES 8u
#define LUPIN_LIGHTMAP_DENOISE_MAX_SQUARINGS 7u
enum { LUPIN_LIGHTMAP_DENOISE_DEVICE_POINTERS = 1u };                   /* desc.flags */
typedef struct LupinLightmapDenoiseDesc {
    uint32_t width;                 /* atlas texels, 1 .. LUPIN_LIGHTMAP_MAX_SIZE */
    uint32_t height;
    uint32_t passes;                /* 1 .. LUPIN_LIGHTMAP_DENOISE_MAX_PASSES; pass i taps at step 2^i */
    uint32_t normal_squarings;      /* 0 .. 7: w_n = max(0, n_p . n_q)^(2^k) */
    uint32_t dilate;                /* 0 .. LUPIN_LIGHTMAP_MAX_DILATE gutter passes after the filter */
    uint32_t flags;
    float max_stretch;              /* finite, > 0 */
} LupinLightmapDenoiseDesc;
int lupin_hip_denoise_lightmap(LupinContext *ctx, const LupinLightmapDenoiseDesc *desc, const float *rgba /* H*W*4 */,
                               const float *records /* H*W*8 */, float *out_rgba /* H*W*4 */);
/* The calling thread's latest successful lupin_hip_denoise_lightmap: device-event milliseconds of its kernels (pass_ms[i]
 * for i < passes, zeros beyond; dilate_ms: all gutter passes) and host-clock milliseconds of the call after its refusals. */
typedef struct LupinLightmapDenoiseStats {
    float prep_ms;
    float pass_ms[8];
    float dilate_ms;
    float call_ms;
} LupinLightmapDenoiseStats;
void lupin_hip_lightmap_denoise_stats(LupinLightmapDenoiseStats *out);

/* ---- lightmap seam stitching (no reference counterpart) ----
 * lupin_hip_stitch_lightmap takes a baked (or denoised) atlas and the charts it was baked with, finds the edges along which a
 * mesh's lightmap UVs are cut, and moves the texels beside them so that what lupin_hip_render_lightmapped fetches on one side
 * of a cut agrees with what it fetches on the other, while every texel stays near its baked value: a least-squares problem
 * solved by conjugate gradients on the device.  `rgba` is H x W x 4 floats, alpha != 0 marking an owned texel, exactly what
 * the view takes.  Every float operation below is one rounded f32 operation in the written order (no contraction, IEEE
 * division and sqrt); tests/lightmap_stitch_ref.py restates the rule.
 *
 * 1. Seam edges.  Every chart on its own.  With T the triangle count of the chart's instance's mesh, half-edge h = 3 t + k
 *    runs from corner k to corner (k + 1) % 3 of triangle t; its key is (min, max) of its two vertex indices.  A half-edge
 *    with equal indices is skipped.  A key with one holder is a boundary and ignored; with three or more it is NON-MANIFOLD,
 *    skipped and counted once; with exactly two, hA < hB, it is an interior edge.  A corner's atlas coordinate is
 *    ((u * scale_u + offset_u) * (float)W, (v * scale_v + offset_v) * (float)H), (u, v) being the corner's lightmap UV (the
 *    mesh's lightmap UV set, or its texcoords), as the bake's rasteriser forms it.  Side A is hA from a0 to a1; side B is the
 *    same two VERTICES (matched by index) in hB's triangle, b0 at the vertex of a0.  The edge is a SEAM when a0 != b0 or
 *    a1 != b1 in any bit of x or y.  Seams are numbered over all charts in ascending (chart, hA).  Matching is by index only:
 *    vertices duplicated per face share no edge and give no seam, and no seam joins two instances.
 *    (Device: a stable radix sort of the keys with h as the value, then of the charts; runs of exactly two.)
 *
 * 2. Sample pairs.  len(p, q) = sqrtf(dx * dx + dy * dy), d = q - p.  m = ceilf(max(len(a0, a1), len(b0, b1)) *
 *    samples_per_texel); n_e = LUPIN_LIGHTMAP_STITCH_MAX_EDGE_SAMPLES if m >= that, (uint32)m if m >= 1, else 1.  Sample j
 *    of edge e has t = ((float)j + 0.5f) / (float)n_e and the points A = a0 + (a1 - a0) * t, B = b0 + (b1 - b0) * t per
 *    component.  Pairs are numbered edge by edge, j ascending.  The FOOTPRINT of a point P is the view's fetch (step 7 of
 *    lupin_hip_render_lightmapped) at (x, y) = (P.x - 0.5f, P.y - 0.5f): the clamp in float, x0 = (uint32)floorf, x1 =
 *    min(x0 + 1, W - 1), f = xf - floorf(xf), likewise y; the taps 00, 10, 01, 11 with weights (1-fx)(1-fy), fx(1-fy),
 *    (1-fx)fy, fx fy; cov = the sum, in tap order from 0, of the weights of the taps whose input alpha != 0; an owned tap
 *    gets weight w / cov, every other tap 0.  A pair one of whose four coordinates x, y is not finite, or with cov == 0 (not
 *    > 0) on either side, is DROPPED: counted, its eight weights 0.  A pair is a row of eight (texel, weight) entries: the
 *    four taps of A with their weights, then the four taps of B with their weights negated.
 *
 * 3. The problem.  A texel is ACTIVE when an entry with weight != 0 names it; the active texels are numbered in ascending
 *    texel index.  x0 = the input rgb at the active texels.  Per channel, minimise sum_p (sum_i w_pi x[t_pi])^2 +
 *    lambda * sum_t (x_t - x0_t)^2 by `iterations` steps of plain conjugate gradients on (A^T A + lambda I) d = -A^T (A x0)
 *    from d = 0; the three channels are three independent solves with their own scalars:
 *      s = A x0; E_before = sum(s * s); r = -(A^T s); p = r; d = 0; rr = sum(r * r);
 *      each step: s = A p; q = A^T s + lambda * p; pq = sum(p * q); a channel whose pq is 0 or not finite STOPS: its alpha
 *      and beta are 0 from then on; otherwise alpha = rr / pq; d = d + alpha * p; r = r - alpha * q; rr' = sum(r * r);
 *      beta = rr' / rr; rr = rr'; p = r + beta * p;
 *      at the end x = x0 + d; s = A x; E_after = sum(s * s).
 *    (A v)_p adds its eight entries w * v[t] in entry order from 0.0f, an entry with weight 0 adding 0.0f.  (A^T s)_t adds
 *    w * s_p over the entries that name t, in ascending (pair, entry) order, from 0.0f.
 *    A sum over n elements: elements are taken in blocks of 256 (zeros past the last); in a block, each run of 64 is summed
 *    by v[i] = v[i] + v[i ^ m] for m = 32, 16, 8, 4, 2, 1, and the four results are added in ascending order; the block
 *    sums b_0, b_1, .. are then added lane-strided, lane l = 0..63 adding b_l, b_(l+64), .. in ascending order from 0.0f, and
 *    the 64 lane sums by the same six steps.  The order depends on n alone: no launch shape, no scheduling, no float atomic.
 *    The scalars stay on the device; there is no host round trip per step.
 *
 * 4. Output.  out_rgba rgb = x at the active texels when iterations > 0; every other texel's rgb, every alpha, and the
 *    whole atlas when iterations == 0, is the input's bit for bit.  Gutter texels that are not active are NOT re-dilated:
 *    they keep what the bake's or the denoiser's gutter passes left.  out_rgba may be the same memory as rgba.
 *    out_info (NULL: not wanted) gets the counts and E_before, E_after per channel, the same with iterations == 0.
 *
 * Ordering as lupin_hip_denoise_lightmap and the bakes: recorded calls run first (their error is returned), the call returns
 * when out_rgba is complete; the scene's hierarchies are not read, so a scene moved by lupin_hip_scene_update_instances
 * stitches to the same words.  Host arrays are staged in device buffers that live for the call.
 * LUPIN_ERR_INVALID_ARGUMENT with out_rgba and out_info untouched for: a NULL argument (out_info may be NULL); num_charts ==
 * 0; width or height 0 or above LUPIN_LIGHTMAP_MAX_SIZE; iterations above LUPIN_LIGHTMAP_STITCH_MAX_ITERATIONS;
 * samples_per_texel or lambda not finite and positive; an unknown flag; reserved != 0; with
 * LUPIN_LIGHTMAP_STITCH_DEVICE_POINTERS a pointer that is not 16-byte aligned; a chart whose instance is out of range, whose
 * mesh has neither a lightmap UV set nor texcoords, or whose scale or offset is not finite; more than 2^32 - 2 half-edges,
 * sample pairs or incidence entries (8 a pair).  An atlas without a seam: LUPIN_OK, out = in.  Without a HIP device:
 * LUPIN_ERR_NO_DEVICE.
 * Known limits and out of scope: seams between instances or meshes; welding by position; re-dilating gutters; stopping by a
 * tolerance; preconditioning.  A directional plane or an AO plane can be passed as `rgba` one at a time. */
#define LUPIN_LIGHTMAP_STITCH_MAX_ITERATIONS 1024u
#define LUPIN_LIGHTMAP_STITCH_MAX_EDGE_SAMPLES 65536u
enum { LUPIN_LIGHTMAP_STITCH_DEVICE_POINTERS = 1u };                    /* desc.flags: rgba and out_rgba are device memory */
typedef struct LupinLightmapStitchDesc {
    uint32_t width;                 /* atlas texels, 1 .. LUPIN_LIGHTMAP_MAX_SIZE */
    uint32_t height;
    uint32_t iterations;            /* 0 .. LUPIN_LIGHTMAP_STITCH_MAX_ITERATIONS; 0: out = in, the counts and energies only */
    float samples_per_texel;        /* seam samples per texel of edge length; finite, > 0 */
    float lambda;                   /* the weight that keeps a texel near its baked value; finite, > 0 */
    uint32_t flags;
    uint32_t reserved;              /* 0 */
} LupinLightmapStitchDesc;
typedef struct LupinLightmapStitchInfo {
    uint32_t seam_edges;
    uint32_t non_manifold_edges;    /* keys with three or more holders */
    uint32_t sample_pairs;          /* emitted, the dropped ones among them */
    uint32_t dropped_pairs;
    uint32_t active_texels;
    uint32_t iterations;            /* steps run */
    float energy_before[3];         /* sum_p (A x0)_p^2 per channel, by the solver's own sum */
    float energy_after[3];          /* the same of x */
} LupinLightmapStitchInfo;
int lupin_hip_stitch_lightmap(LupinContext *ctx, const LupinScene *scene, const LupinLightmapStitchDesc *desc,
                              const LupinLightmapChart *charts, uint32_t num_charts, const float *rgba /* H*W*4 */,
                              float *out_rgba /* H*W*4 */, LupinLightmapStitchInfo *out_info /* NULL ok */);
/* The calling thread's latest successful lupin_hip_stitch_lightmap: host-clock milliseconds per phase (each ends
 * synchronised) and of the call after its refusals.  LUPIN_ERR_INVALID_ARGUMENT for NULL. */
typedef struct LupinLightmapStitchStats {
    float edges_ms;                 /* keys, sorts, runs, the seam edges' count */
    float samples_ms;               /* edges, counts, scan, pairs */
    float incidence_ms;             /* the incidence sort, the active texels, the columns */
    float solve_ms;                 /* all steps, the energies and the output */
    float call_ms;
} LupinLightmapStitchStats;
int lupin_hip_lightmap_stitch_stats(LupinLightmapStitchStats *out);

/* ---- light-probe baking (no reference counterpart) ----
 * The radiance arriving at points in space from every direction, projected onto the nine real spherical harmonics of bands
 * 0..2: what lights everything a lightmap cannot cover.  Every probe is path-traced along `samples` uniformly distributed
 * directions by the integrators of the radiance query above, and reduced on the device.  Every float operation below is
 * one rounded f32 operation (no contraction).
 *
 * Probe, LUPIN_PROBE_FLOATS floats: [0..2] position   [3] RNG word (bits).
 * Path s of probe i is slot i * samples + s.  Its RNG state is the query's: the probe's word for s == 0 and
 * hash_u32(word + s * 0x9E3779B9) otherwise; it starts at bounce 0, outside any medium, exactly as a query path does.
 * Direction: two numbers r0, r1 drawn from the slot's state, then
 *   z = 1.0f - 2.0f * r1;  rad = sqrtf(max(0.0f, 1.0f - z * z));  (s, c) = sincos(2.0f * pi * r0);  w = (rad * c, rad * s, z)
 * in world axes (sincos: the library's lpm_sincosf, lupin_detmath.h).
 * out_rays (NULL, or n * samples records of the query): the probe's position, the state after the two draws, w and mode 0;
 * querying such a record with samples = 1 replays that one path.
 *
 * Basis, w = (x, y, z) in world axes, k0 = 0.28209479f, k1 = 0.48860251f, k2 = 1.09254843f, k3 = 0.31539157f,
 * k4 = 0.54627422f:
 *   Y0 = k0          Y1 = k1*y        Y2 = k1*z                        Y3 = k1*x        Y4 = (k2*x)*y
 *   Y5 = (k2*y)*z    Y6 = k3*((3.0f*z)*z - 1.0f)                       Y7 = (k2*x)*z    Y8 = k4*(x*x - y*y)
 *
 * Reduction, per probe, as one wave of 64 lanes: lane l takes the samples s = l, l + 64, l + 128, ... < samples in ascending
 * order and adds, from +0.0f, acc[j][c] += L_s[c] * Yj(w_s) for c in r, g, b and acc[j][3] += Yj(w_s); L_s is the path's
 * radiance, clamped at advanced.max_radiance as a pixel's samples are, w_s the direction above.  Then for offset = 32, 16, 8,
 * 4, 2, 1: acc = acc + acc of lane (l xor offset).  The result is (acc * (4.0f * pi)) / (float)samples.
 *
 * out_sh (n x LUPIN_PROBE_SH_COEFFS x 4): coefficient j of probe i is (r, g, b, w); L(w) ~ sum_j out_sh[i][j].rgb * Yj(w).
 * The w channel is the projection of the sample pattern itself (2 sqrt(pi), 0, ..., 0 for perfect sampling): it does not
 * depend on the scene, and a caller who wants ratio estimates divides by it.
 *
 * Chunks, ordering and failure are lupin_hip_pathtrace_rays': recorded calls run first (their error is returned; they have
 * run once the descriptor and the pointers have passed their checks), a wavefront holds whole probes, at most
 * desc->max_slots paths (0: LUPIN_RAYS_DEFAULT_MAX_SLOTS), at least one probe; the call returns when out_sh is complete;
 * frames rendered before and after are what they would be without the call.  With LUPIN_PROBES_DEVICE_POINTERS in
 * desc->flags, probes, out_sh and out_rays are device memory of the context's device, 16-byte aligned, and nothing is copied
 * to or from the host.
 *
 * LUPIN_ERR_INVALID_ARGUMENT, nothing traced and the outputs untouched, for: a NULL argument (out_rays may be NULL); an unknown
 * pathtrace_type or flag; samples == 0 or above 2^27; max_bounces >= 4095; n * samples above 2^38; a scene of another or of a
 * destroyed context; a probe with a non-finite position (host probes are checked on the host, device probes by a kernel
 * whose count the host reads before the first wavefront); device pointers not 16-byte aligned; a hierarchy too deep for the
 * traversal stack (as a render).  n == 0: LUPIN_OK, nothing touched.  Without a HIP device: LUPIN_ERR_NO_DEVICE. */
#define LUPIN_PROBE_FLOATS 4
#define LUPIN_PROBE_SH_COEFFS 9
#define LUPIN_PROBE_RESULT_FLOATS 36
enum { LUPIN_PROBES_DEVICE_POINTERS = 1u };                             /* desc.flags */
typedef struct LupinProbeDesc {
    uint32_t pathtrace_type;        /* as LupinRayQueryDesc */
    uint32_t max_bounces;
    uint32_t samples;               /* S >= 1 paths per probe */
    uint32_t flags;
    uint32_t max_slots;             /* 0 = library default; paths per wavefront */
    LupinAdvancedParams advanced;
} LupinProbeDesc;
int lupin_hip_bake_probes(LupinContext *ctx, const LupinScene *scene, const LupinProbeDesc *desc,
                          uint64_t n, const float *probes /* n x 4 */, float *out_sh /* n x 9 x 4 */,
                          float *out_rays /* NULL, or n*S x 8 */);

/* ---- occlusion queries (no reference counterpart) ----
 * "Is anything in the way?": line of sight, ambient occlusion, probe validity, a caller's own shadow terms.  An any-hit
 * traversal of the binary hierarchy that stops at the first triangle it accepts.
 *
 * Record, LUPIN_OCCLUSION_RECORD_FLOATS floats ("bits": the u32's bits stored in the float's place):
 *   [0..2] origin   [3] RNG state (bits; ignored in direction mode)   [4..6] unit direction (mode 0) or unit surface normal
 *   (mode 1)   [7] tmax (a float; +inf or any value >= FLT_MAX: unbounded)
 * A segment (origin o, direction d, ray_epsilon, tmax) is BLOCKED iff some triangle the traversal tests is hit at a ray
 * parameter t with ray_epsilon <= t < tmax, t in world units along d as lupin_hip_trace_rays reports it.  The traversal
 * enters every node whose box the ray reaches below tmax; with tmax unbounded the answer is lupin_hip_trace_rays' `hit`,
 * ray for ray, and a segment blocked at tmax is blocked at every larger tmax.
 * Material opacity is NOT consulted: this is geometric visibility.  Emissive, transparent and alpha-textured surfaces block
 * like any other; the stochastic alpha skip belongs to the integrators.
 *
 * Record i expands into desc->samples slots, slot = i * samples + s:
 *   LUPIN_OCCLUSION_DIRECTION          the direction as given; samples must be 1
 *   LUPIN_OCCLUSION_COSINE_HEMISPHERE  the slot's RNG state and direction exactly as LUPIN_RAY_COSINE_HEMISPHERE derives them
 *                                      in a radiance query: the record's word for s == 0, hash_u32(word + s * 0x9E3779B9)
 *                                      otherwise, two numbers drawn, the matte BSDF's cosine-weighted direction about the
 *                                      normal -- bit for bit the out_rays of lupin_hip_pathtrace_rays on the same record
 * out_blocked[i]: the number of record i's slots that are blocked, 0 .. samples.
 *
 * The call runs the calls recorded on the context first (and returns their error, if any), then its own launches, and
 * returns when out_blocked is complete; frames rendered before and after are what they would be without the call.  Large
 * batches run as successive launches of at most 2^30 slots.  With LUPIN_OCCLUSION_DEVICE_POINTERS in desc->flags, records
 * (16-byte aligned) and out_blocked (4-byte aligned) are device memory of the context's device and nothing is copied to or
 * from the host; host arrays go through staging buffers the context keeps and reuses from call to call.  It works on a
 * scene whose four-wide hierarchy is stale after lupin_hip_scene_update_instances: only the binary hierarchy is read.
 *
 * LUPIN_ERR_INVALID_ARGUMENT, nothing traced and out_blocked untouched, for: a NULL argument; an unknown mode or flag;
 * samples == 0 or above 2^27; direction mode with samples != 1; n * samples above 2^38; a scene of another or of a destroyed
 * context; a record with a non-finite origin, direction or normal; a direction or normal whose squared length is further
 * than 1e-4 from 1; a tmax that is NaN or <= 0; a ray_epsilon that is not finite or is negative; misaligned device pointers;
 * a hierarchy too deep for the traversal stack (as a render).  Host records are checked on the host, device records by a
 * kernel whose count the host reads before the first launch.  n == 0: LUPIN_OK, nothing touched.
 * Without a HIP device: LUPIN_ERR_NO_DEVICE. */
#define LUPIN_OCCLUSION_RECORD_FLOATS 8
enum { LUPIN_OCCLUSION_DIRECTION = 0, LUPIN_OCCLUSION_COSINE_HEMISPHERE = 1 };   /* desc.mode  */
enum { LUPIN_OCCLUSION_DEVICE_POINTERS = 1u };                                   /* desc.flags */
typedef struct LupinOcclusionDesc {
    uint32_t mode;
    uint32_t samples;               /* S >= 1 slots per record; 1 in direction mode */
    uint32_t flags;
    float ray_epsilon;              /* finite, >= 0; hits below it are ignored, as in pathtrace_scene */
} LupinOcclusionDesc;
int lupin_hip_occlusion_rays(LupinContext *ctx, const LupinScene *scene, const LupinOcclusionDesc *desc,
                             uint64_t n, const float *records /* n x 8 */, uint32_t *out_blocked /* n */);

/* ---- transmittance queries (no reference counterpart) ----
 * "How much gets through?": opacity-aware visibility for the callers of lupin_hip_occlusion_rays -- alpha-textured leaf
 * cards, cut-out fences, half-transparent panes.  The records, modes, slots, flags and LupinOcclusionDesc are those of
 * lupin_hip_occlusion_rays; the traversal does not stop at the first triangle.
 *
 * A slot's segment (o, d, ray_epsilon, tmax) starts with T = 1.  Each triangle the traversal tests that is hit at
 * ray_epsilon <= t < tmax contributes one factor, in the order the traversal meets them:
 *   - its instance cannot have an opacity other than 1 (material colour alpha == 1, no colour texture on a mesh with
 *     texcoords, no vertex colours: decided at upload): T = 0 and the query ends; no material is read.
 *   - otherwise a = texture alpha * material colour alpha * vertex colour alpha at the hit (LUPIN_SURFACE_OPACITY of
 *     lupin_hip_surface_probe).  If !(a < 1) (this includes NaN): T = 0 and the query ends.  Otherwise
 *     T = T * (1 - max(a, 0)).
 * f32, no contraction, one multiplication per accepted triangle.  For a in [0, 1), 1 - a is the probability with which the
 * integrators' stochastic alpha skip lets a path through that surface, so T is the EXPECTED result of that skip over the
 * surfaces of one segment.  It is NOT a replay of the integrators' loop: that loop restarts the ray at every skipped surface
 * with a fresh ray_epsilon and gives up after 128 skips.  Colour is not consulted: a refractive or transparent MATERIAL
 * TYPE with opacity 1 blocks -- this is alpha, not BSDF transmission.  The visited nodes are those of
 * lupin_hip_occlusion_rays (slab distance below the constant tmax, binary hierarchy only: it works after
 * lupin_hip_scene_update_instances), each triangle of a visited leaf is tested once, and T(tmax) never grows with tmax.
 * On a scene without an alpha-capable instance T == 1 - blocked of lupin_hip_occlusion_rays, bit for bit.
 *
 * out_sum[i]: the SUM of T over record i's slots (direction mode: T itself); the caller divides by samples.  The sum's
 * order is fixed: 64 partial sums p[l] = T[l] + T[l + 64] + ... (ascending, from 0), then for off = 32, 16, 8, 4, 2, 1:
 * p[l] = p[l] + p[l ^ off]; the result is p[0].  No float atomics: the same records give the same words.
 *
 * The call behaves as lupin_hip_occlusion_rays does: recorded calls run first, the work runs on the primary stream, host
 * arrays go through the context's staging buffers, LUPIN_OCCLUSION_DEVICE_POINTERS takes device memory in place (records
 * 16-byte, out_sum 4-byte aligned), launches cover whole records, and the same refusals apply (LUPIN_ERR_INVALID_ARGUMENT,
 * out_sum untouched) with one tighter limit: samples must not exceed 2^20.  With samples > 1 the slots' T go through a
 * plane of floats the context owns and reuses; launches are sized so that it stays within 2^24 slots (64 MB).
 * n == 0: LUPIN_OK, nothing touched.  Without a HIP device: LUPIN_ERR_NO_DEVICE. */
int lupin_hip_transmittance_rays(LupinContext *ctx, const LupinScene *scene, const LupinOcclusionDesc *desc,
                                 uint64_t n, const float *records /* n x 8 */, float *out_sum /* n */);

/* ---- bent-normal queries (no reference counterpart) ----
 * "How much of the hemisphere is open, and which way does the open part point?": ambient occlusion and the cosine-weighted
 * bent normal of surface points, in one launch per batch.
 *
 * Records are lupin_hip_occlusion_rays' records read in LUPIN_OCCLUSION_COSINE_HEMISPHERE mode: [0..2] origin, [3] RNG word
 * (bits), [4..6] unit surface normal, [7] tmax.  Slot s of record i (s < samples) has the RNG state and direction d_s of
 * that mode, bit for bit -- the out_rays of lupin_hip_pathtrace_rays on the same record.
 *
 * Weight per slot, for the segment (o, d_s, ray_epsilon, tmax):
 *   without LUPIN_BENT_NORMAL_OPACITY   T_s = 1.0f if the segment is not BLOCKED in lupin_hip_occlusion_rays' sense, else 0.0f
 *   with LUPIN_BENT_NORMAL_OPACITY      T_s = lupin_hip_transmittance_rays' T for that segment, word for word
 *
 * out[i], LUPIN_BENT_NORMAL_RESULT_FLOATS floats, is summed as one wave of 64 lanes; every float operation is one rounded
 * f32 operation, no contraction:
 *   1. lane l takes slots s = l, l + 64, ... in ascending order;
 *   2. it adds them to acc = (+0, +0, +0, +0):  acc.x = acc.x + T_s * d_s.x,  acc.y = acc.y + T_s * d_s.y,
 *      acc.z = acc.z + T_s * d_s.z,  acc.w = acc.w + T_s;
 *   3. for off = 32, 16, 8, 4, 2, 1:  acc = acc + acc of lane (l xor off), component by component;
 *   4. out[i] = acc of lane 0.
 * Lanes without a slot (samples < 64) hold +0 and take part in step 3.  No float atomics, no per-slot plane in memory, no
 * second kernel; the same records give the same words, whatever max_slots is and however the batch is cut into launches.
 * out[i].w / samples is the ambient-occlusion visibility; out[i].xyz, normalised, is the cosine-weighted bent normal (its
 * expectation per slot is E[T d]: (0, 0, 2/3) about a normal +z under an open sky).  The caller divides and normalises.
 *   - With LUPIN_BENT_NORMAL_OPACITY, out[i].w is lupin_hip_transmittance_rays' out_sum for the same records, bit for bit.
 *   - Without it, out[i].w is exactly (float)(samples - blocked) of lupin_hip_occlusion_rays: every partial sum is an integer
 *     of at most 2^20, which f32 holds exactly.
 *
 * The call behaves as lupin_hip_transmittance_rays does: recorded calls run first (their error is returned), the work runs
 * on the primary stream, host arrays go through staging buffers the context keeps, and LUPIN_BENT_NORMAL_DEVICE_POINTERS
 * takes device memory of the context's device in place (records and out 16-byte aligned).  A launch holds whole records:
 * max_slots / samples of them, at least one, and never more than 2^25.  Only the binary hierarchy is read: it works after
 * lupin_hip_scene_update_instances.
 *
 * LUPIN_ERR_INVALID_ARGUMENT, nothing traced and `out` untouched, for everything lupin_hip_transmittance_rays refuses in
 * hemisphere mode (a NULL argument; n * samples above 2^38; a scene of another or of a destroyed context; a record with a
 * non-finite origin or normal, a normal whose squared length is further than 1e-4 from 1, a tmax that is NaN or <= 0; a
 * ray_epsilon that is not finite or is negative; a hierarchy too deep for the traversal stack), an unknown flag, samples
 * == 0 or above 2^20, and misaligned device pointers.  n == 0: LUPIN_OK, nothing touched.
 * Without a HIP device: LUPIN_ERR_NO_DEVICE. */
#define LUPIN_BENT_NORMAL_RESULT_FLOATS 4
enum { LUPIN_BENT_NORMAL_DEVICE_POINTERS = 1u, LUPIN_BENT_NORMAL_OPACITY = 2u };   /* desc.flags */
typedef struct LupinBentNormalDesc {
    uint32_t samples;               /* S: 1 .. 2^20 slots per record */
    uint32_t flags;
    uint32_t max_slots;             /* 0 = library default (2^30); slots per launch; a launch holds whole records, at least one */
    float ray_epsilon;              /* finite, >= 0 */
} LupinBentNormalDesc;
int lupin_hip_bent_normal_rays(LupinContext *ctx, const LupinScene *scene, const LupinBentNormalDesc *desc,
                               uint64_t n, const float *records /* n x 8 */, float *out /* n x 4 */);

/* ---- distance queries (no reference counterpart) ----
 * "How far is the nearest surface, where is it, and which side of it am I on?" for POINTS: clearances for bake offsets, probe
 * validity, a distance volume for collision, sphere tracing or leak checks.  A nearest-point traversal of the binary
 * hierarchy, pruned by the distance from the point to a node's box.
 *
 * Record, LUPIN_DISTANCE_RECORD_FLOATS floats:   [0..2] point p (finite)   [3] rmax, the search radius (> 0; +inf or any
 * value >= FLT_MAX: unbounded, clamped to FLT_MAX)
 * Over every triangle of every instance, taken in WORLD space (its vertices through the instance's local -> world
 * transform, the f32 inverse lupin_mat3x4_inverse gives of the world -> local rows: non-uniform scale and shear are
 * measured as they appear in the world), c* is the point of the surface nearest to p, and  found = |p - c*| < rmax.
 * Contributing nothing: an instance whose rows have no finite inverse, and a triangle whose world-space cross product
 * (v1 - v0) x (v2 - v0) has squared length 0 in f32 (zero area).  Material opacity is NOT consulted.  Triangles at equal
 * distance: either may be reported.  A surface further than about 1.8e19 units away (its squared distance is not a finite
 * float) is not found.
 *
 * Result, LUPIN_DISTANCE_RESULT_FLOATS floats, 48 bytes ("bits": the u32's bits stored in the float's place):
 *   [0] found (bits: 1 or 0)   [1] distance |p - c*|   [2..4] point c*   [5] u   [6] v   [7] instance (bits)
 *   [8] tri (bits): the triangle index lupin_hip_trace_rays reports (within the instance's mesh, in the scene's order)
 *   [9] side: +1.0, -1.0 or 0.0   [10] 0   [11] 0
 * c* = v0 + (v1 - v0) u + (v2 - v0) v with the triangle's world-space vertices.  Words 1 .. 9 are 0 when nothing was found.
 * side is the sign of dot(p - c*, n) with n = (v1 - v0) x (v2 - v0) of THE REPORTED TRIANGLE in world space.  It is a
 * statement about that one triangle.  It is NOT an inside / outside classification: where c* lies on an edge or a vertex
 * that several triangles share, it is the side of whichever of them was reported, and two of them can disagree.
 *
 * lupin_hip_bake_distance_grid fills a regular grid of dims[0] x dims[1] x dims[2] voxels, x fastest:
 * voxel = ix + dims[0] * (iy + dims[1] * iz), centre, per axis and in this order in f32,
 *   c = origin + ((float)i + 0.5f) * spacing
 * out_volume[voxel] = the distance from the centre, or rmax (clamped to FLT_MAX) where nothing lies within rmax.  With
 * LUPIN_DISTANCE_GRID_SIGNED a found distance is multiplied by side, and where side is 0 the value is 0.  The same
 * centres given to lupin_hip_distance_points give the same floats.
 *
 * Both calls run the calls recorded on the context first (and return their error, if any), then their own launches on the
 * primary stream, and return when the output is complete.  Large batches run as successive launches of at most 2^30 records
 * or voxels.  With LUPIN_DISTANCE_DEVICE_POINTERS records and out_results (16-byte aligned) or out_volume (4-byte aligned)
 * are device memory of the context's device and nothing is copied to or from the host; host arrays go through staging
 * buffers the context keeps and reuses from call to call.  origin, spacing and dims are host memory always.  Both work on
 * a scene whose four-wide hierarchy is stale after lupin_hip_scene_update_instances: only the binary hierarchy is read,
 * and the transforms are the scene's current ones.
 *
 * LUPIN_ERR_INVALID_ARGUMENT, nothing computed and the output untouched, for: a NULL argument; an unknown flag (GRID_SIGNED
 * is unknown to distance_points); a scene of another or of a destroyed context; a record with a non-finite point or an
 * rmax that is NaN or <= 0; n above 2^38; a non-finite origin; a spacing that is not finite or not positive; a zero
 * dimension; more than 2^36 voxels; a grid whose last centre is not finite; misaligned device pointers; a hierarchy too
 * deep for the traversal stack (which holds two words per entry here).  Host records are checked on the host, device
 * records by a kernel whose count the host reads before the first launch.  n == 0: LUPIN_OK, nothing touched.
 * Without a HIP device: LUPIN_ERR_NO_DEVICE. */
#define LUPIN_DISTANCE_RECORD_FLOATS 4
#define LUPIN_DISTANCE_RESULT_FLOATS 12
enum { LUPIN_DISTANCE_DEVICE_POINTERS = 1u, LUPIN_DISTANCE_GRID_SIGNED = 2u };   /* flags */
int lupin_hip_distance_points(LupinContext *ctx, const LupinScene *scene, uint32_t flags, uint64_t n,
                              const float *records /* n x 4 */, float *out_results /* n x 12 */);
int lupin_hip_bake_distance_grid(LupinContext *ctx, const LupinScene *scene, uint32_t flags, const float *origin /* 3 */,
                                 const float *spacing /* 3 */, const uint32_t *dims /* 3 */, float rmax,
                                 float *out_volume /* dims[0] * dims[1] * dims[2] */);

/* ---- irradiance volume lookup (no reference counterpart) ----
 * "What light arrives at this point with this normal?" from a regular grid of baked probes: what lights everything a
 * lightmap does not cover.  The consumer of lupin_hip_bake_probes: per shading point the cell, the trilinear weights of its
 * eight probes, the probes the caller marked invalid and the probes behind a wall dropped, the clamped cosine's irradiance
 * at the normal, and the normalisation, in one kernel.  Every float operation below is one rounded f32 operation (no
 * contraction; division and square root correctly rounded), in the order written.
 *
 * Probes.  Probe (ix, iy, iz) has index ix + dims[0] * (iy + dims[1] * iz); its position is, per axis,
 *   origin + (float)i * spacing        (the product first)
 * These are probe POSITIONS, not voxel centres: there is no + 0.5.  sh is P x LUPIN_PROBE_SH_COEFFS x 4 floats, P =
 * dims[0] * dims[1] * dims[2]: lupin_hip_bake_probes' out_sh for those positions in index order (the w channel is not read).
 * valid is NULL or P bytes; a zero byte marks a probe that must not be used.
 *
 * Record, LUPIN_PROBE_GRID_RECORD_FLOATS floats:   [0..2] point p   [4..6] unit normal nrm   [3], [7] ignored
 *
 * 1. o = p + nrm * normal_bias (the product first), per axis.
 * 2. Per axis k:   g = (o_k - origin_k) / spacing_k;   g = min(max(g, 0.0f), (float)(dims_k - 1));
 *    i_k = dims_k > 1 ? min((uint32_t)g, dims_k - 2) : 0;   f_k = g - (float)i_k.   A point outside the grid is clamped onto
 *    it; an axis with dims_k == 1 has f_k == 0 and ignores that coordinate.
 * 3. Yj(nrm), j = 0 .. 8, by the nine expressions of the light-probe section above;  B_j = A_j * Yj(nrm) with the clamped
 *    cosine's band factors A_0 = 3.14159265f (pi), A_1 = A_2 = A_3 = 2.09439510f (2 pi / 3), A_4 = .. = A_8 = 0.78539816f (pi / 4).
 * 4. The corners c = 0 .. 7 in ascending order; bit 0 of c selects ix + 1, bit 1 iy + 1, bit 2 iz + 1.  acc = (+0, +0, +0, +0).
 *    For each corner:
 *      t = (wx * wy) * wz with w = bit ? f : 1.0f - f.  If t == 0 the corner contributes nothing and casts no ray.
 *      If valid is given and valid[index] == 0 the corner is skipped.
 *      With q the probe's position:  d = q - o;  len = sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z);  dir = d / len per axis; where
 *      len == 0, dir = nrm.
 *      LUPIN_PROBE_GRID_BACKFACE:  b = (((dir.x*nrm.x + dir.y*nrm.y) + dir.z*nrm.z) + 1.0f) * 0.5f;  t = t * (b * b + 0.2f):
 *      probes the surface faces away from count for less, never for nothing.
 *      LUPIN_PROBE_GRID_VISIBILITY:  if len > 2.0f * ray_epsilon, the corner is skipped when the segment (o, dir,
 *      ray_epsilon, tmax = len - ray_epsilon) is BLOCKED in the sense of lupin_hip_occlusion_rays: the same traversal of the
 *      binary hierarchy, material opacity not consulted.  A shorter segment is visible.
 *      E[ch] = sum over j ascending, from +0, of B_j * sh[index][j][ch], for ch in r, g, b.
 *      acc.rgb = acc.rgb + t * E;  acc.w = acc.w + t.
 *    A skipped corner is not added at all (0 * E is not added either: a NaN coefficient of a skipped probe stays out).
 * 5. out = acc.w > 0 ? (acc.r / acc.w, acc.g / acc.w, acc.b / acc.w, acc.w) : (0, 0, 0, 0).
 * out (n x LUPIN_PROBE_GRID_RESULT_FLOATS): irradiance r, g, b and the weight w that survived.  w == 0 means "no probe of this
 * cell may be used"; the fallback is the caller's.  The coefficients are NOT inspected: a NaN or infinite coefficient of a
 * probe that is used reaches the output.
 *
 * The call behaves as the other scene queries do: the calls recorded on the context run first (and their error, if any, is
 * returned), the work runs on the primary stream, host arrays (sh, valid, records, out) go through staging buffers the
 * context keeps and reuses, launches cover at most 2^27 records, and the call returns when out is complete; frames rendered
 * before and after are what they would be without the call.  With LUPIN_PROBE_GRID_DEVICE_POINTERS sh, records and out are
 * device memory of the context's device, 16-byte aligned, valid is device memory of any alignment, and nothing is copied.
 * It works on a scene whose four-wide hierarchy is stale after lupin_hip_scene_update_instances.  Without
 * LUPIN_PROBE_GRID_VISIBILITY the scene's geometry is not read and no traversal stack is reserved.
 *
 * LUPIN_ERR_INVALID_ARGUMENT, nothing traced and out untouched, for: a NULL ctx, scene, desc, sh, records or out; an unknown
 * flag; a non-finite origin; a spacing that is not finite or not positive; a zero dim; more than 2^31 probes; a last probe
 * position that is not finite; a ray_epsilon or normal_bias that is not finite or is negative; n above 2^38; a record with a
 * non-finite point or normal; a normal whose squared length is further than 1e-4 from 1; misaligned device pointers; a scene
 * of another or of a destroyed context; with LUPIN_PROBE_GRID_VISIBILITY, a hierarchy too deep for the traversal stack.  Host
 * records are checked on the host, device records by a kernel whose count the host reads before the first launch.
 * n == 0: LUPIN_OK, nothing touched.  Without a HIP device: LUPIN_ERR_NO_DEVICE. */
#define LUPIN_PROBE_GRID_RECORD_FLOATS 8
#define LUPIN_PROBE_GRID_RESULT_FLOATS 4
enum { LUPIN_PROBE_GRID_DEVICE_POINTERS = 1u, LUPIN_PROBE_GRID_VISIBILITY = 2u, LUPIN_PROBE_GRID_BACKFACE = 4u };   /* desc.flags */
typedef struct LupinProbeGridDesc {
    float    origin[3];      /* position of probe (0,0,0); finite */
    float    spacing[3];     /* finite, > 0 (also on an axis whose dim is 1) */
    uint32_t dims[3];        /* >= 1 each; product <= 2^31 */
    uint32_t flags;
    float    ray_epsilon;    /* finite, >= 0; VISIBILITY only */
    float    normal_bias;    /* finite, >= 0; world units the point is moved along its normal before anything else */
} LupinProbeGridDesc;
int lupin_hip_sample_probe_grid(LupinContext *ctx, const LupinScene *scene, const LupinProbeGridDesc *desc,
                                const float *sh /* P x 9 x 4, bake_probes' out_sh */, const uint8_t *valid /* NULL or P */,
                                uint64_t n, const float *records /* n x 8 */, float *out /* n x 4 */);

/* ---- probe depth maps (no reference counterpart) ----
 * "What does this probe see, as distances, per direction?"  lupin_hip_bake_probe_depth bakes per probe an octahedral map of
 * the mean and the mean square of the distance to the nearest surface; lupin_hip_sample_probe_grid_depth is the irradiance
 * volume lookup above with a corner's any-hit segment replaced by a Chebyshev test against the corner's map, so that a
 * baked volume needs no scene geometry to be looked up.  Every float operation below is one rounded f32 operation (no
 * contraction; division and square root correctly rounded), in the order written.  sgn(x) is -1.0f for x < 0 and +1.0f
 * otherwise (sgn(0) = +1); |x| clears the sign bit.
 *
 * BAKE.  R = resolution, K = subsamples.  positions: n x 4 floats, [3] ignored.  Probe i casts R * R * K * K rays; the ray of
 * texel (tx, ty), sub-sample (sx, sy) is slot ((i * R * R + ty * R + tx) * K * K) + sy * K + sx.
 * Direction (octahedral decode):
 *   a = ((float)(tx * K + sx) + 0.5f) / (float)(R * K);   u = 2.0f * a - 1.0f;   v likewise from ty, sy
 *   z = (1.0f - |u|) - |v|
 *   if z < 0:  x = (1.0f - |v|) * sgn(u),  y = (1.0f - |u|) * sgn(v);   otherwise  x = u,  y = v
 *   len = sqrtf((x * x + y * y) + z * z);   w = (x / len, y / len, z / len)
 * Distance: (hit, dst) is lupin_hip_trace_rays' answer for (position, w, ray_epsilon), bit for bit (the binary hierarchy;
 * material opacity is not consulted);  d = hit ? min(dst, max_distance) : max_distance.
 * Reduction: the K * K rays of a texel hold (d, d * d) in sub-sample order s = sy * K + sx.  For offset = K * K / 2, .., 2, 1:
 * acc[s] = acc[s] + acc[s xor offset], all s at once (a butterfly: every s ends with the same value).  Then
 *   m1 = acc.x / (float)(K * K),   m2 = acc.y / (float)(K * K)
 * Layout: out_depth[i] is a row-major (R + 2) x (R + 2) map of (m1, m2); interior texel (tx, ty) sits at (tx + 1, ty + 1).
 * The one-texel border holds copies, so that plain bilinear filtering is right across the octahedral seams: for border
 * coordinates (bx, by) in -1 .. R, with clamp to 0 .. R - 1,
 *   both out of range:     the source is interior texel (R - 1 - clamp(bx), R - 1 - clamp(by))
 *   only bx out of range:  (clamp(bx), R - 1 - by)
 *   only by out of range:  (R - 1 - bx, clamp(by))
 * Stats (out_stats NULL, or n x LUPIN_PROBE_DEPTH_STATS_WORDS words which the call initialises), per probe:
 *   [0] rays = R * R * K * K     [1] rays that hit anything (before the cap)
 *   [2] hits on a back face: ((w.x * g.x + w.y * g.y) + w.z * g.z) > 0 with g the hit triangle's geometric normal, the value
 *       lupin_hip_surface_probe reports in LUPIN_SURFACE_NORMAL mode at [3..5]
 *   [3] the bits of the smallest d, as an unsigned minimum over the bits
 * None of the words depends on how the rays were cut into launches.
 *
 * The call behaves as the other scene queries do: the calls recorded on the context run first (and their error, if any, is
 * returned), the work runs on the primary stream, host arrays go through device buffers that live for the call (at most
 * 1024 probes at a time), a launch covers at most max_slots rays (0: LUPIN_PROBE_DEPTH_DEFAULT_MAX_SLOTS; rounded down to a
 * multiple of 64, at least 64, at most 2^30), and the call returns when the outputs are complete; frames rendered before and
 * after are what they would be without the call.  With LUPIN_PROBE_DEPTH_DEVICE_POINTERS positions, out_depth and out_stats
 * are device memory of the context's device (positions and out_stats 16-byte aligned, out_depth 8-byte aligned) and nothing
 * is copied.  It works on a scene whose four-wide hierarchy is stale after lupin_hip_scene_update_instances.
 *
 * LUPIN_ERR_INVALID_ARGUMENT, nothing traced and the outputs untouched, for: a NULL ctx, scene, desc, positions or out_depth;
 * an unknown flag; a resolution outside 2 .. 64; subsamples other than 1, 2, 4, 8; a ray_epsilon that is not finite or is
 * negative; a max_distance that is not finite or not positive; n * R * R * K * K above 2^38; misaligned device pointers; a
 * scene of another or of a destroyed context; a position with a non-finite coordinate (host positions are checked on the
 * host, device positions by a kernel whose count the host reads before the first launch); a hierarchy too deep for the
 * traversal stack.  LUPIN_ERR_NO_SW_BVH for a scene without a software BVH.  n == 0: LUPIN_OK, nothing touched.  Without a
 * HIP device: LUPIN_ERR_NO_DEVICE.
 *
 * LOOKUP.  sh, valid, records, out and steps 1 to 5 are lupin_hip_sample_probe_grid's, word for word, with grid.flags of
 * LUPIN_PROBE_GRID_DEVICE_POINTERS and LUPIN_PROBE_GRID_BACKFACE (LUPIN_PROBE_GRID_VISIBILITY is refused: the visibility is
 * the maps'; grid.ray_epsilon is checked and not used).  depth is P x (R + 2) x (R + 2) x 2 floats, the bake's out_depth for
 * the grid's probe positions in index order, R = resolution; max_distance is the bake's.  In step 4, in the place of the
 * LUPIN_PROBE_GRID_VISIBILITY clause, for a corner still in use (after the backface factor):
 *   if len == 0 the corner is visible.  Otherwise, with e = -dir (the probe looks at the point):
 *   s = (|e.x| + |e.y|) + |e.z|;   px = e.x / s;   py = e.y / s
 *   if e.z < 0:  (px, py) = ((1.0f - |py|) * sgn(px), (1.0f - |px|) * sgn(py)), both from the old values
 *   per axis:  a = px * 0.5f;  a = a + 0.5f;  a = a * (float)R;  a = a + 0.5f;  ix = min((uint32_t)a, R);  fx = a - (float)ix
 *   m00, m10, m01, m11 = texels (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) of the probe's bordered map; per moment
 *   top = m00 + fx * (m10 - m00);   bot = m01 + fx * (m11 - m01);   m = top + fy * (bot - top)
 *   r = min(len, max_distance)
 *   if r > m1:  x = m2 - m1 * m1;  var = x > 0 ? x : 0.0f;  dd = r - m1;  c = var / (var + dd * dd);  vis = (c * c) * c;
 *               t = t * vis;  a corner with vis == 0 is skipped like a blocked one (not added at all).
 * The moments are NOT inspected.  A NaN m1 fails r > m1: the corner counts as visible.  A NaN m2 (with r > m1) gives var = 0,
 * hence vis = 0 unless dd * dd underflows to 0 as well, where c = 0 / 0 is NaN and reaches the output, as does any NaN that
 * an infinite moment produces.
 *
 * The scene's geometry is never read and no LDS is reserved: a scene without a software BVH, or with a hierarchy too deep
 * for the stack, is accepted; it still has to belong to the context.  Otherwise the call behaves as
 * lupin_hip_sample_probe_grid does (host arrays go through device buffers that live for the call).  With
 * LUPIN_PROBE_GRID_DEVICE_POINTERS depth is device memory, 8-byte aligned.
 * LUPIN_ERR_INVALID_ARGUMENT, out untouched, for: what lupin_hip_sample_probe_grid refuses without VISIBILITY; a NULL depth;
 * LUPIN_PROBE_GRID_VISIBILITY; a resolution outside 2 .. 64; a max_distance that is not finite or not positive. */
#define LUPIN_PROBE_DEPTH_STATS_WORDS 4
#define LUPIN_PROBE_DEPTH_MIN_RESOLUTION 2
#define LUPIN_PROBE_DEPTH_MAX_RESOLUTION 64
#define LUPIN_PROBE_DEPTH_DEFAULT_MAX_SLOTS (1u << 24)
enum { LUPIN_PROBE_DEPTH_DEVICE_POINTERS = 1u };   /* LupinProbeDepthDesc.flags */
typedef struct LupinProbeDepthDesc {
    uint32_t resolution;    /* R: interior texels per side, 2 .. 64 */
    uint32_t subsamples;    /* K: 1, 2, 4 or 8; K * K rays per texel on a regular sub-grid, no RNG */
    uint32_t flags;         /* LUPIN_PROBE_DEPTH_DEVICE_POINTERS */
    uint32_t max_slots;     /* 0 = library default; rays per launch, rounded down to a multiple of 64, at least 64 */
    float    ray_epsilon;   /* finite, >= 0 */
    float    max_distance;  /* finite, > 0: distances are capped here, misses count as this */
} LupinProbeDepthDesc;
int lupin_hip_bake_probe_depth(LupinContext *ctx, const LupinScene *scene, const LupinProbeDepthDesc *desc, uint64_t n,
                               const float *positions /* n x 4, [3] ignored */, float *out_depth /* n x (R+2) x (R+2) x 2 */,
                               uint32_t *out_stats /* NULL or n x 4 */);
typedef struct LupinProbeGridDepthDesc {
    LupinProbeGridDesc grid;   /* flags: DEVICE_POINTERS, BACKFACE; VISIBILITY is refused here */
    uint32_t resolution;       /* R of the maps */
    float    max_distance;     /* the bake's */
} LupinProbeGridDepthDesc;
int lupin_hip_sample_probe_grid_depth(LupinContext *ctx, const LupinScene *scene, const LupinProbeGridDepthDesc *desc,
                                      const float *sh /* P x 9 x 4 */, const float *depth /* P x (R+2) x (R+2) x 2 */,
                                      const uint8_t *valid /* NULL or P */, uint64_t n, const float *records /* n x 8 */,
                                      float *out /* n x 4 */);

/* ---- baked-lighting view (no reference counterpart) ----
 * "What does this baked volume look like from here?"  One primary hit per pixel, then emission + albedo / pi * E(p, n) with
 * the irradiance E taken from an irradiance volume by one of the two lookups above: a camera view of a baked volume without
 * a path traced, and the cheap frame to show while the path tracer converges.  The call is a composition of contracts
 * stated elsewhere in this header and is held to them bit for bit.  Every float operation below is one rounded f32
 * operation (no contraction), in the order written.
 *
 * render_target gives the image: W x H texels.  depth == NULL selects lupin_hip_sample_probe_grid's lookup (grid.flags may
 * hold LUPIN_PROBE_GRID_VISIBILITY and LUPIN_PROBE_GRID_BACKFACE); depth != NULL selects lupin_hip_sample_probe_grid_depth's
 * with desc.resolution and desc.max_distance (LUPIN_PROBE_GRID_BACKFACE only: VISIBILITY is refused, as that call refuses
 * it).  Where sh, depth, valid and out_gbuffer live is said by desc.flags, not by grid.flags: LUPIN_PROBE_GRID_DEVICE_POINTERS
 * in grid.flags is refused as an unknown flag.  For pixel (x, y), row 0 at the top:
 *
 * 1. (o, d) is lupin_hip_camera_probe's LUPIN_CAMERA_RAY_CENTRE ray for that pixel of a W x H image, bit for bit.  No RNG
 *    number is drawn; the aperture is ignored.
 * 2. (hit, dst, u, v, instance, tri) is lupin_hip_trace_rays' answer for (o, d, ray_epsilon), bit for bit: the binary
 *    hierarchy; material opacity is not consulted, so cut-outs are opaque in this view.
 * 3. On a miss:  rgb = lupin_hip_surface_probe's LUPIN_SURFACE_ENVIRONMENT [0..2] for d;  w = 0.
 * 4. On a hit:   p = o + d * dst per axis (the product first);
 *    ns = lupin_hip_surface_probe's LUPIN_SURFACE_NORMAL [0..2] (the shading normal) for (instance, tri, u, v);
 *    c = (d.x * ns.x + d.y * ns.y) + d.z * ns.z;   n = c > 0 ? -ns : ns   (the surface is lit from the viewer's side);
 *    color = LUPIN_SURFACE_MATERIAL [4..6], emission = LUPIN_SURFACE_MATERIAL [1..3] of the same record.
 *    EVERY MATERIAL TYPE IS DRAWN AS A MATTE SURFACE OF ITS color: glossy, reflective, transparent, refractive and volumetric
 *    materials get no highlights, reflections or transmission here.
 * 5. (E.r, E.g, E.b, w) is the chosen lookup's result for the record (p | -, n | -), word for word (its steps 1 to 5).
 *    The lookup is not asked, and (E, w) = (ambient, 0), where a coordinate of p or n is not finite or |n|^2 = (n.x * n.x +
 *    n.y * n.y) + n.z * n.z is further than 1e-4 from 1: the lookups' own refusals, here per pixel and not per call.
 *    Where the lookup answers w == 0 (no probe of the cell may be used), E = ambient.
 * 6. rgb = emission + (color * E) * 0.31830988f, per channel.
 * 7. The texel is rgb rounded to f16 by the context's store rounding (lupin_hip_set_f16_store_rounding: toward zero unless
 *    nearest-even was selected), alpha 1.0.  Nothing is accumulated, there is no prev_frame, and rgb is not clamped.
 *
 * out_gbuffer is NULL or W x H x LUPIN_BAKED_VIEW_GBUFFER_FLOATS floats, row-major with row 0 at the top ("bits": the u32's
 * bits in the float's place):
 *   [0..2] p    [3] instance bits, or LUPIN_BAKED_VIEW_MISS    [4..6] n    [7] tri bits (within the instance's mesh)
 *   [8..10] color    [11] w    [12..14] emission; on a miss the environment radiance    [15] dst
 * What a miss does not define is 0.  The first eight words of a hit pixel are a LUPIN_PROBE_GRID_RECORD: handed to the
 * chosen lookup they reproduce E and [11] (where step 5 asked the lookup).
 *
 * The image is cut into launches of max_slots pixels (0: LUPIN_BAKED_VIEW_DEFAULT_MAX_SLOTS; rounded down to a multiple of
 * 64, at least 64): per launch a primary-hit kernel writes records into scratch memory of that size, the lookup's own kernel
 * runs over them, and a third kernel composes and stores.  The picture does not depend on max_slots.
 *
 * The call behaves as the other scene queries do: the calls recorded on the context run first (and their error, if any, is
 * returned), the work runs on the primary stream, host arrays (sh, depth, valid, out_gbuffer) go through device buffers
 * that live for the call, and the call returns when the target and out_gbuffer are complete; frames rendered before and
 * after are what they would be without the call.  With LUPIN_BAKED_VIEW_DEVICE_POINTERS sh and out_gbuffer are device memory
 * of the context's device, 16-byte aligned, depth 8-byte aligned, valid of any alignment, and nothing is copied.  It works
 * on a scene whose four-wide hierarchy is stale after lupin_hip_scene_update_instances.
 *
 * LUPIN_ERR_INVALID_ARGUMENT, nothing traced, the target and out_gbuffer untouched, for: a NULL ctx, scene, render_target,
 * desc or sh; a scene or a target of another or of a destroyed context; an unknown flag; a non-finite ambient; a
 * ray_epsilon that is not finite or is negative; what the chosen lookup refuses in its grid (with depth: also a resolution
 * outside 2 .. 64 and a max_distance that is not finite or not positive); misaligned device pointers; a hierarchy too deep
 * for the traversal stack.  (Every LupinTexture is Rgba16Float: there is no other target to refuse.)  LUPIN_ERR_NO_SW_BVH
 * for a scene without a software BVH.  Without a HIP device: LUPIN_ERR_NO_DEVICE. */
#define LUPIN_BAKED_VIEW_GBUFFER_FLOATS 16
#define LUPIN_BAKED_VIEW_MISS 0xFFFFFFFFu
#define LUPIN_BAKED_VIEW_DEFAULT_MAX_SLOTS (1u << 20)
enum { LUPIN_BAKED_VIEW_DEVICE_POINTERS = 1u };   /* LupinBakedViewDesc.flags */
typedef struct LupinBakedViewDesc {
    LupinCameraParams camera_params;   /* as LupinPathtraceDesc carries them */
    LupinMat3x4 camera_transform;
    LupinProbeGridDesc grid;           /* flags: VISIBILITY (depth == NULL only), BACKFACE */
    uint32_t resolution;               /* R of the maps; depth != NULL only */
    float    max_distance;             /* the maps' bake's; depth != NULL only */
    float    ray_epsilon;              /* of the primary ray: finite, >= 0 */
    float    ambient[3];               /* E where no probe answers; finite */
    uint32_t flags;                    /* LUPIN_BAKED_VIEW_DEVICE_POINTERS */
    uint32_t max_slots;                /* 0 = library default; pixels per launch, rounded down to a multiple of 64, at least 64 */
} LupinBakedViewDesc;
int lupin_hip_render_baked(LupinContext *ctx, const LupinScene *scene, LupinTexture *render_target, const LupinBakedViewDesc *desc,
                           const float *sh /* P x 9 x 4 */, const float *depth /* NULL or P x (R+2) x (R+2) x 2 */,
                           const uint8_t *valid /* NULL or P */, float *out_gbuffer /* NULL or W x H x 16 */);

/* ---- lightmapped view (no reference counterpart) ----
 * "What does this baked lightmap look like from here?"  The baked-lighting view above with a lightmap atlas as the
 * irradiance source on every surface that has a chart, and the irradiance volume (or `ambient`) on whatever has none:
 * lightmaps on the static surfaces, probes as the fallback.  `lightmap` is lupin_hip_bake_lightmap's or
 * lupin_hip_denoise_lightmap's out_rgba (H x W x 4 floats, row 0 first; alpha != 0 marks a texel a chart owns), and `charts`
 * is the array the bake was given, unchanged.  desc.view carries the camera, ray_epsilon, ambient, flags and max_slots; its
 * grid, resolution and max_distance are read only when sh != NULL, and then sh, depth and valid select and feed the lookup
 * exactly as in lupin_hip_render_baked.  Every float operation below is one rounded f32 operation (no contraction), in the
 * order written.  For pixel (x, y) of the target, row 0 at the top:
 *
 * 1.-4. lupin_hip_render_baked's steps 1 to 4, bit for bit: the centre ray (o, d), the binary hierarchy's hit
 *    (dst, u, v, instance, tri), on a miss the environment radiance, on a hit p, the turned shading normal n, color, emission.
 * 5. The chart of a hit instance is the chart of LOWEST index whose instance_idx names it; an instance no chart names is
 *    uncharted.
 * 6. For a charted hit, with (a, b, c) the texcoords of the triangle's three vertices:
 *    w = 1 - u - v;   tu = a.x * w + b.x * u + c.x * v;   tv = a.y * w + b.y * u + c.y * v   (summed left to right: what the
 *    material textures are sampled at);   au = tu * scale_u + offset_u;   av = tv * scale_v + offset_v;
 *    X = au * W - 0.5f;   Y = av * H - 0.5f   (W, H the atlas size as floats; texel centres are at +0.5 and row 0 is v in
 *    [0, 1 / H), as the bake rasterises).  If X or Y is not finite the pixel is UNCHARTED from here on, in every respect.
 * 7. The fetch.  xf = min(max(X, 0), W - 1), clamped in float before any conversion to integer;  x0 = floor(xf);
 *    x1 = min(x0 + 1, W - 1);  fx = xf - floor(xf);  y0, y1, fy likewise from Y and H.  The taps, in TAP ORDER, are the texels
 *    (x0, y0), (x1, y0), (x0, y1), (x1, y1) with weights (1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy.  A tap
 *    is OWNED when its alpha != 0.  Every sum starts at 0.0f and adds in tap order.  cov = the sum of the weights of the
 *    owned taps.  If cov > 0:  E = (the sum over the owned taps of weight * rgb) / cov per channel; a tap that is not owned
 *    enters neither sum.  Otherwise E = the sum over all four taps of weight * rgb: what the bake's gutter passes are for.
 *    Lightmap texels are not sanitised.  The pixel's source is LUPIN_LIGHTMAPPED_SOURCE_LIGHTMAP and its G-buffer word [11]
 *    is cov.
 * 8. For an uncharted hit:  with sh != NULL, lupin_hip_render_baked's step 5 with the chosen lookup, its per-pixel refusal
 *    and `ambient` where w == 0 included; the source is LUPIN_LIGHTMAPPED_SOURCE_PROBES, or
 *    LUPIN_LIGHTMAPPED_SOURCE_AMBIENT where ambient was used, and word [11] is the lookup's w (0 where it was not asked).
 *    With sh == NULL:  E = ambient, the source is AMBIENT, word [11] is 0, and no lookup kernel is launched.
 * 9. rgb = emission + (color * E) * 0.31830988f per channel, and the store: lupin_hip_render_baked's steps 6 and 7.
 *
 * out_gbuffer is NULL or W x H x LUPIN_LIGHTMAPPED_VIEW_GBUFFER_FLOATS floats: [0..15] are lupin_hip_render_baked's, with
 * [11] as said in steps 7 and 8;  [16] X  [17] Y of step 6, or 0 when uncharted;  [18] the chart index bits, or
 * LUPIN_BAKED_VIEW_MISS when uncharted;  [19] the source bits (LUPIN_LIGHTMAPPED_SOURCE_MISS on a miss, where [16..18] are
 * 0, 0 and LUPIN_BAKED_VIEW_MISS).
 *
 * Launches, ordering and host arrays are lupin_hip_render_baked's: launches of max_slots pixels, recorded calls first (their
 * error is returned), the primary stream, host arrays (lightmap among them) through device buffers that live for the call;
 * it works on a scene moved by lupin_hip_scene_update_instances.  `charts` is always a host array.  With
 * LUPIN_BAKED_VIEW_DEVICE_POINTERS in view.flags lightmap, sh, depth, valid and out_gbuffer are device memory of the context's
 * device: lightmap 16-byte aligned, the others as lupin_hip_render_baked asks.
 *
 * LUPIN_ERR_INVALID_ARGUMENT, nothing launched, the target and out_gbuffer untouched, for: everything lupin_hip_render_baked
 * refuses (a NULL sh is not refused; what it refuses in the grid, resolution and max_distance only when sh != NULL); depth
 * or valid without sh; a NULL lightmap; charts == NULL with num_charts > 0; an atlas width or height of 0 or above
 * LUPIN_LIGHTMAP_MAX_SIZE; reserved != 0; a chart whose instance is out of range, whose mesh has no texcoords, or whose
 * scale or offset is not finite; a misaligned device lightmap.  LUPIN_ERR_NO_SW_BVH and LUPIN_ERR_NO_DEVICE as
 * lupin_hip_render_baked. */
#define LUPIN_LIGHTMAPPED_VIEW_GBUFFER_FLOATS 20
enum { LUPIN_LIGHTMAPPED_SOURCE_MISS = 0u, LUPIN_LIGHTMAPPED_SOURCE_LIGHTMAP = 1u,
       LUPIN_LIGHTMAPPED_SOURCE_PROBES = 2u, LUPIN_LIGHTMAPPED_SOURCE_AMBIENT = 3u };
typedef struct LupinLightmappedViewDesc {
    LupinBakedViewDesc view;      /* camera, ray_epsilon, ambient, flags, max_slots; grid/resolution/max_distance read only when sh != NULL */
    uint32_t lightmap_width;      /* atlas texels, 1 .. LUPIN_LIGHTMAP_MAX_SIZE */
    uint32_t lightmap_height;
    uint32_t num_charts;          /* may be 0 */
    uint32_t reserved;            /* must be 0 */
} LupinLightmappedViewDesc;
int lupin_hip_render_lightmapped(LupinContext *ctx, const LupinScene *scene, LupinTexture *render_target,
                                 const LupinLightmappedViewDesc *desc,
                                 const LupinLightmapChart *charts /* num_charts, host */,
                                 const float *lightmap /* H x W x 4: bake_lightmap's or denoise_lightmap's out_rgba */,
                                 const float *sh /* NULL: no volume */, const float *depth, const uint8_t *valid,
                                 float *out_gbuffer /* NULL or Wimg x Himg x 20 */);

/* ---- lightmapped view with a directional lightmap (no reference counterpart) ----
 * lupin_hip_render_lightmapped with one more input: `directional`, the four coefficient planes of
 * lupin_hip_bake_lightmap_directional (LUPIN_LIGHTMAP_DIRECTIONAL_PLANES x H x W x 4 floats, plane j first, for the same atlas
 * and charts as `lightmap`), and desc.bake_flags, the flags that bake was given (0 or LUPIN_LIGHTMAP_SMOOTH_NORMALS).  On a
 * charted surface the scalar lightmap's E is scaled by how much more or less light the pixel's shading normal (a normal map, a
 * smooth-shaded mesh) receives than the bake normal did, so the atlas responds to normal detail.  desc.base is
 * lupin_hip_render_lightmapped's descriptor and steps 1 to 9 are that function's, bit for bit.  Between steps 7 and 9, for a
 * pixel whose source is LUPIN_LIGHTMAPPED_SOURCE_LIGHTMAP, every operation one rounded f32 operation in the order written:
 *
 * 7a. C0..C3 (rgb each) are step 7's fetch from the four planes: the same four taps in tap order, the same weights, the same
 *     cov, and OWNED still means that the tap's alpha in `lightmap` (not in the plane) != 0.  If cov > 0, Cj = (the sum over
 *     the owned taps of weight * plane j's rgb) / cov, otherwise the sum over all four taps.
 * 7b. n' = step 4's turned shading normal n.  n_b = the bake normal at the hit: what lupin_hip_bake_lightmap writes into the
 *     record of a texel whose centre maps to (instance, tri, u, v) under bake_flags (the geometric normal g; with
 *     SMOOTH_NORMALS on a mesh with normals the interpolated vertex normal in world space, negated if it points away from g).
 *     With k0 = 0.28209479f, k1 = 0.48860251f, per channel:
 *       num = ((C0 * k0 + C1 * (k1 * n'.y)) + C2 * (k1 * n'.z)) + C3 * (k1 * n'.x)
 *       den = ((C0 * k0 + C1 * (k1 * n_b.y)) + C2 * (k1 * n_b.z)) + C3 * (k1 * n_b.x)
 * 7c. r = 1.0f when the ray meets the triangle's back face, (d.x * g.x + d.y * g.y) + d.z * g.z > 0 with g as
 *     lupin_hip_surface_probe's LUPIN_SURFACE_NORMAL reports it at [3..5] (the bake lit the other side); or when den <= 0; or
 *     when num or den is not finite.  Otherwise r = max(num, 0) / den, the maximum being (num > 0 ? num : +0.0f).
 *     E = E * r per channel, and step 9 follows.
 *
 * With n' == n_b num and den are the same operations on the same numbers, so r == 1.0f and the picture is
 * lupin_hip_render_lightmapped's.  For planes baked from non-negative radiance 0 <= r <= 4 up to rounding and Monte Carlo
 * noise of the fetch: num and den are the radiance integrated against (1 + 3 w . n') / (4 pi) and (1 + 3 w . n_b) / (4 pi)
 * times (w . n_b)+, and on the hemisphere about n_b the first weight lies in [-2, 4] / (4 pi), the second in [1, 4] / (4 pi).
 *
 * out_gbuffer is NULL or W x H x LUPIN_LIGHTMAPPED_DIRECTIONAL_GBUFFER_FLOATS floats: [0..19] are
 * lupin_hip_render_lightmapped's;  [20..22] r per channel, 1.0f wherever no ratio was applied (every pixel that is not
 * LIGHTMAP among them);  [23] bits: LUPIN_LIGHTMAPPED_DIRECTIONAL_APPLIED (r = max(num, 0) / den was taken in at least one
 * channel), _BACK_FACE, _DEN_NOT_POSITIVE (den <= 0 in at least one channel of a front-face pixel), _NOT_FINITE (num or den
 * not finite in at least one channel of a front-face pixel); 0 where the source is not LIGHTMAP.
 *
 * Launches, ordering, host arrays and LUPIN_BAKED_VIEW_DEVICE_POINTERS (in desc.base.view.flags; `directional` is then device
 * memory, 16-byte aligned) are lupin_hip_render_lightmapped's.  LUPIN_ERR_INVALID_ARGUMENT, nothing launched, the target and
 * out_gbuffer untouched, for everything lupin_hip_render_lightmapped refuses and: a NULL directional; a bake_flags bit other
 * than LUPIN_LIGHTMAP_SMOOTH_NORMALS; a misaligned device directional; a non-zero reserved word. */
#define LUPIN_LIGHTMAPPED_DIRECTIONAL_GBUFFER_FLOATS 24
enum { LUPIN_LIGHTMAPPED_DIRECTIONAL_APPLIED = 1u, LUPIN_LIGHTMAPPED_DIRECTIONAL_BACK_FACE = 2u,
       LUPIN_LIGHTMAPPED_DIRECTIONAL_DEN_NOT_POSITIVE = 4u, LUPIN_LIGHTMAPPED_DIRECTIONAL_NOT_FINITE = 8u };
typedef struct LupinLightmappedDirectionalDesc {
    LupinLightmappedViewDesc base;
    uint32_t bake_flags;          /* the directional bake's desc.flags: 0 or LUPIN_LIGHTMAP_SMOOTH_NORMALS */
    uint32_t reserved[3];         /* must be 0 */
} LupinLightmappedDirectionalDesc;
int lupin_hip_render_lightmapped_directional(LupinContext *ctx, const LupinScene *scene, LupinTexture *render_target,
                                             const LupinLightmappedDirectionalDesc *desc,
                                             const LupinLightmapChart *charts /* num_charts, host */,
                                             const float *lightmap /* H x W x 4 */, const float *directional /* 4 x H x W x 4 */,
                                             const float *sh /* NULL: no volume */, const float *depth, const uint8_t *valid,
                                             float *out_gbuffer /* NULL or Wimg x Himg x 24 */);

/* tonemapping.rs:106-132  TonemapDesc (+ Viewport :144-151) */
typedef struct LupinTonemapDesc
{
    uint32_t has_viewport;   /* 0 = None: the whole target */
    float    viewport_x, viewport_y, viewport_w, viewport_h;
    float    exposure;       /* color *= 2^exposure */
    uint32_t filmic;         /* bool, default false */
    uint32_t srgb;           /* bool, default true */
    uint32_t clear;          /* bool, default true: target cleared to (0,0,0,1) first */
} LupinTonemapDesc;

/* tonemapping.rs:155-224  lp::tonemap_and_fit_aspect(device, queue, resources, src, dst, desc) with the Rgba8Unorm
 * target held by the host: `dst_rgba8` (dst_width x dst_height x 4 bytes, row 0 = top) is read when !clear and
 * overwritten with the result.  Synchronous.  The reference rasterises a quad and samples through the hardware
 * sampler, whose sub-texel precision is not specified; this is the same mapping evaluated at pixel centres. */
int lupin_hip_tonemap_and_fit_aspect(LupinContext *ctx, const LupinTexture *src, uint8_t *dst_rgba8,
                                     uint32_t dst_width, uint32_t dst_height, const LupinTonemapDesc *desc);

/* Tile-sharded multi-GPU support: pack the pixels of every tile owned by `rank` (include/lupin_tiles.h) (tiles
 * of tile_size*4 pixels, row-major tile order as renderer.rs:816-817) into a dense device
 * buffer / scatter a packed buffer back. Payload layout: tiles in ascending t, each tile
 * row-major, 8 B per pixel. Returns the number of pixels via out_pixels. */
int lupin_hip_pack_tiles(LupinContext *ctx, const LupinTexture *tex, uint32_t tile_size,
                         uint32_t rank, uint32_t world, void *device_dst, uint64_t *out_pixels);
int lupin_hip_unpack_tiles(LupinContext *ctx, LupinTexture *tex, uint32_t tile_size,
                           uint32_t rank, uint32_t world, const void *device_src);
uint64_t lupin_hip_packed_tile_pixels(uint32_t width, uint32_t height, uint32_t tile_size,
                                      uint32_t rank, uint32_t world);
/* The scatter after an all-gather in ONE launch: `device_gathered` holds `world` payloads of `capacity_pixels` pixels each
 * (rank r's at r * capacity_pixels * 8 bytes, padded); every tile NOT owned by `rank` is written into `tex`.  For hosts that
 * run their own collective; lupin_hip_gather_framebuffer does pack + all-gather + this. */
int lupin_hip_unpack_gathered_tiles(LupinContext *ctx, LupinTexture *tex, uint32_t tile_size, uint32_t rank, uint32_t world,
                                    const void *device_gathered, uint64_t capacity_pixels);

/* ---- the one exchange step of tile-sharded rendering: RCCL gather of per-tile framebuffers over xGMI ----
 * No counterpart in the reference (single device; its TileParams sub-dispatch, renderer.rs:807-829, is what the shards
 * are made of).  A host renders its tiles with lupin_hip_pathtrace_scene_tiles for any number of accumulation frames
 * (no communication) and calls lupin_hip_gather_framebuffer once per readback: every rank then holds the whole frame,
 * bit-identical to the single-GPU render.  librccl is dlopen'ed on first use (LUPIN_RCCL_LIB names the one library to load instead of the default sonames;
 * a library that cannot be loaded makes every communicator call return LUPIN_ERR_RCCL).
 *
 * One process per GPU:  rank 0 calls lupin_hip_comm_get_unique_id and hands the 128 bytes to the other ranks by any
 *                       means (file, socket, MPI); every rank then calls lupin_hip_comm_init_rank.
 * One process, n GPUs:  lupin_hip_comm_init_all over n contexts (one per device), gathers through
 *                       lupin_hip_gather_framebuffer_all (the n all-gathers form one RCCL group).
 * A host that already owns an ncclComm_t for the context's device wraps it with lupin_hip_comm_from_nccl. */
#define LUPIN_COMM_ID_BYTES 128
int lupin_hip_comm_get_unique_id(uint8_t *out_id /* LUPIN_COMM_ID_BYTES */);
int lupin_hip_comm_init_rank(LupinContext *ctx, const uint8_t *id /* LUPIN_COMM_ID_BYTES */, uint32_t rank, uint32_t world,
                             LupinComm **out_comm);
int lupin_hip_comm_init_all(LupinContext *const *ctxs, uint32_t n, LupinComm **out_comms /* n entries */);
int lupin_hip_comm_from_nccl(LupinContext *ctx, void *nccl_comm, uint32_t rank, uint32_t world, LupinComm **out_comm);
void lupin_hip_comm_destroy(LupinComm *comm);
uint32_t lupin_hip_comm_rank(const LupinComm *comm);
uint32_t lupin_hip_comm_world(const LupinComm *comm);
/* pack this rank's tiles of `tex` -> ncclAllGather -> scatter the other ranks' tiles into `tex`; enqueued on the context's
 * stream after every frame enqueued so far (asynchronous like pathtrace_scene; download / lupin_hip_sync waits). */
int lupin_hip_gather_framebuffer(LupinComm *comm, LupinTexture *tex, uint32_t tile_size);
int lupin_hip_gather_framebuffer_all(LupinComm *const *comms, LupinTexture *const *texs, uint32_t n, uint32_t tile_size);
/* the readback form: only `root` receives (one grouped ncclSend per peer / ncclRecv per peer on the root, exact payload
 * sizes), so a 3840 x 2160 readback moves 66 MB once instead of to every rank; the other ranks' textures keep their own
 * tiles only.  Same enqueue semantics as lupin_hip_gather_framebuffer. */
int lupin_hip_gather_framebuffer_to(LupinComm *comm, LupinTexture *tex, uint32_t tile_size, uint32_t root);
/* host-side reductions over the ranks for measurement loops (op 0 = sum, 1 = max); synchronous, and every frame this
 * rank enqueued has completed when they return, so lupin_hip_comm_barrier brackets a timed region */
int lupin_hip_comm_allreduce_f64(LupinComm *comm, double *inout, uint32_t n, uint32_t op);
int lupin_hip_comm_barrier(LupinComm *comm);

/* ------------------------------------------------------------------------------------------
 * CPU-side preprocessing that produces the path's inputs (data_structures.rs:20-641).
 * Pure host code, no device needed.
 * ---------------------------------------------------------------------------------------- */

/* Device BLAS builder ("next" row 8f-1; no counterpart in the reference, whose builder is CPU-only,
 * data_structures.rs:196-475): a linear BVH over Morton-sorted triangles -- a complete binary tree with 1-2 triangles
 * per leaf, depth lupin_hip_lbvh_depth(n) <= 22 -- written in the reference's BvhNode format with the reordered index
 * buffer, i.e. a drop-in alternative to lupin_build_bvh for lupin_hip_scene_create.  Returns the node count
 * (= lupin_hip_lbvh_node_count(num_indices / 3)) or a negative status.  Synchronous. */
uint32_t lupin_hip_lbvh_depth(uint32_t num_tris);
uint64_t lupin_hip_lbvh_node_count(uint32_t num_tris);
int64_t lupin_hip_build_bvh_device(LupinContext *ctx, const float *verts_pos4, uint32_t num_verts, uint32_t *indices,
                                   uint32_t num_indices, LupinBvhNode *out_nodes, uint64_t out_capacity);

/* The reference's own BLAS builder run on the device (csrc/sahbvh.hip): level-synchronous binned SAH that reproduces
 * lp::build_bvh's decisions (data_structures.rs:196-475: 5 bins per axis, half-area x count cost, centroid[axis] <= pos
 * partition, depth cap) from min / max / count reductions, so every node's box, split plane and triangle SET equals
 * lupin_build_bvh's bit for bit.  Only bookkeeping differs: nodes are numbered level by level and both sides of a
 * partition keep their input order.  Same signature and return value as lupin_build_bvh (out_nodes must not be NULL;
 * 2 * triangles - 1 nodes always suffice; vertex positions must be finite).  Synchronous. */
int64_t lupin_hip_build_bvh_sah_device(LupinContext *ctx, const float *verts_pos4, uint32_t num_verts, uint32_t *indices,
                                       uint32_t num_indices, LupinBvhNode *out_nodes, uint64_t out_capacity);

/* build_tlas (data_structures.rs:545-641) on the device (csrc/tlas.hip): lupin_build_tlas' inputs and output, the same
 * tree node for node.  The leaf boxes come from the host code lupin_build_tlas uses; the agglomerative clustering
 * (:572-610), a serial chain of tlas_find_best_match scans (:670-692), runs in one workgroup, each scan a reduction of
 * (area, index) pairs in which the smaller area, then the smaller index wins -- the first minimum of the reference's
 * ascending scan.  Boxes equal lupin_build_tlas' as float values (a zero may differ in sign: fminf(+0, -0)).
 * Returns the node count (2 * num_instances) or a negative status; LUPIN_ERR_INVALID_ARGUMENT, before anything is
 * launched, for an instance whose world box is not finite, and after the kernel stopped itself: at n^2 + 4n scans (no
 * input needs them) or at a scan without candidate (every union area NaN or >= FLT_MAX).  Synchronous. */
int64_t lupin_hip_build_tlas_device(LupinContext *ctx, const LupinInstance *instances, uint32_t num_instances,
                                    const float *model_aabbs, uint32_t num_meshes, LupinTlasNode *out_nodes);
/* the calling thread's latest lupin_hip_build_tlas_device (including the one inside lupin_hip_scene_update_instances) */
typedef struct LupinTlasBuildStats {
    uint32_t num_instances;
    uint32_t state_in_lds;   /* 1: the live-slot state was held in LDS, 0: in global memory (more than 5800 instances) */
    uint64_t scans;          /* tlas_find_best_match scans */
    float kernel_ms;         /* the clustering kernel, between two events */
} LupinTlasBuildStats;
void lupin_hip_tlas_build_stats(LupinTlasBuildStats *out);

/* The four-wide collapse of one mesh's BLAS exactly as lupin_hip_scene_create performs it for the wide tracer (host code,
 * no device needed; DESIGN.md 5 "Wide traversal"): a node's grandchildren are pulled up, largest box first, until it has
 * four children or only leaves; a child whose own children's boxes are not inside its box stays a child.  out_nodes
 * receives 128-byte records of 32 words: lox[4] loy[4] loz[4] hix[4] hiy[4] hiz[4] (f32; NaN in unused slots), ref[4]
 * (u32: bit 31 = leaf, bit 30 = the child's box does not contain every triangle below it (never pruned by distance), low
 * 30 bits = first triangle of the leaf / index into out_nodes; 0xFFFFFFFF = unused slot), 4 zero words.
 * With vertex data (verts_pos4 / indices in BLAS leaf order; may be NULL), out_tri_flags (may be NULL; one byte per
 * triangle) receives bit 0 = last triangle of its leaf, bit 1 = the triangle is not inside every box above it.
 * Returns the node count (out_nodes may be NULL to query it) or < 0; *out_root = the root reference (a single-leaf BLAS
 * has no wide node: the leaf reference passes through). */
int64_t lupin_hip_collapse_bvh4(const LupinBvhNode *nodes, uint32_t num_nodes, const float *verts_pos4, uint32_t num_verts,
                                const uint32_t *indices, uint32_t num_indices, void *out_nodes, uint64_t capacity,
                                uint32_t *out_root, uint8_t *out_tri_flags);

/* build_bvh (data_structures.rs:196-235): reorders `indices` in place; returns node count or <0.
 * out_nodes may be NULL to query the count (indices untouched in that case). */
int64_t lupin_build_bvh(const float *verts_pos4, uint32_t num_verts, uint32_t *indices,
                        uint32_t num_indices, LupinBvhNode *out_nodes, uint64_t out_capacity);
/* build_tlas (data_structures.rs:545-641): out_nodes must hold 2*num_instances entries.
 * model_aabbs: per mesh 6 floats (min xyz, max xyz). */
int64_t lupin_build_tlas(const LupinInstance *instances, uint32_t num_instances,
                         const float *model_aabbs, uint32_t num_meshes, LupinTlasNode *out_nodes);
/* build_alias_table (data_structures.rs:116-193): returns bins written (0 when sum == 0) */
int64_t lupin_build_alias_table(const float *weights, uint64_t n, LupinAliasBin *out_bins);
/* triangle-area weights + total area of build_lights' inner loop (data_structures.rs:40-51,106-112) */
float lupin_mesh_light_weights(const float *verts_pos4, const uint32_t *indices, uint32_t num_indices,
                               float *out_weights);
/* environment texel weights of build_lights (data_structures.rs:65-93); texels = w*h*4 f32 */
void lupin_env_light_weights(const float *texels_rgba_f32, uint32_t width, uint32_t height,
                             const float scale_rgb[3], float *out_weights);
/* Mat3x4 inverse through Mat4::inverse (base.rs:542-578, :708-722) */
void lupin_mat3x4_inverse(const LupinMat3x4 *in, LupinMat3x4 *out);

#ifdef __cplusplus
}
#endif
#endif /* LUPIN_HIP_H */
