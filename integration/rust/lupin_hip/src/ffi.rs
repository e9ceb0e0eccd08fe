//! Raw declarations of include/lupin_hip.h. Every `#[repr(C)]` struct has the byte layout of the C struct of the same
//! name, which in turn equals the reference's own `#[repr(C)]` upload types (lupin/src/renderer.rs:94-280).
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int, c_void};

macro_rules! opaque { ($($n:ident),*) => { $(#[repr(C)] pub struct $n { _p: [u8; 0] })* } }
opaque!(LupinContext, LupinPathtraceResources, LupinScene, LupinTexture, LupinDoubleBufferedTexture, LupinComm, LupinDenoiseResources,
        LupinAdaptiveResources, LupinReprojectResources);

pub const LUPIN_OK: c_int = 0;
pub const LUPIN_SENTINEL_IDX: u32 = 0xFFFF_FFFF;

#[repr(C)] #[derive(Copy, Clone, Default)] pub struct LupinMat3x4 { pub m: [[f32; 3]; 4] }          // base.rs:634-657: 4 columns x 3 rows
#[repr(C)] #[derive(Copy, Clone, Default)] pub struct LupinMat4x3 { pub m: [[f32; 4]; 3] }          // base.rs:763-768
#[repr(C)] #[derive(Copy, Clone, Default)] pub struct LupinMat4 { pub m: [[f32; 4]; 4] }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinMeshInfo { pub normals_buf_idx: u32, pub texcoords_buf_idx: u32, pub colors_buf_idx: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinInstance { pub transpose_inverse_transform: LupinMat4x3, pub mesh_idx: u32, pub mat_idx: u32, pub padding0: f32, pub padding1: f32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinMaterial {
    pub color: [f32; 4], pub emission: [f32; 4], pub scattering: [f32; 4],
    pub mat_type: u32, pub roughness: f32, pub metallic: f32, pub ior: f32, pub sc_anisotropy: f32, pub tr_depth: f32,
    pub color_tex_idx: u32, pub emission_tex_idx: u32, pub roughness_tex_idx: u32, pub scattering_tex_idx: u32, pub normal_tex_idx: u32, pub padding0: u32,
}
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinEnvironment { pub emission: [f32; 3], pub emission_tex_idx: u32, pub transform: LupinMat4 }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinLight { pub instance_idx: u32, pub area: f32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinAliasBin { pub prob: f32, pub alias_threshold: f32, pub alias: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinBvhNode { pub aabb_min: [f32; 3], pub tri_begin_or_first_child: u32, pub aabb_max: [f32; 3], pub tri_count: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinTlasNode { pub aabb_min: [f32; 3], pub left: u32, pub aabb_max: [f32; 3], pub instance_idx: u32, pub right: u32, pub padding: [f32; 3] }

#[repr(C)] pub struct LupinTextureDesc { pub width: u32, pub height: u32, pub format: u32, pub pixels: *const c_void }   // format: 0 Rgba8Unorm, 1 Rgba16Float
#[repr(C)] pub struct LupinMeshDesc { pub verts_pos: *const f32, pub num_verts: u32, pub indices: *const u32, pub num_indices: u32, pub bvh_nodes: *const LupinBvhNode, pub num_bvh_nodes: u32 }
#[repr(C)] pub struct LupinVertexBufferDesc { pub data: *const f32, pub num_verts: u32 }
#[repr(C)] pub struct LupinAliasTableDesc { pub bins: *const LupinAliasBin, pub num_bins: u32 }
#[repr(C)] pub struct LupinSceneDesc {
    pub mesh_infos: *const LupinMeshInfo, pub meshes: *const LupinMeshDesc, pub num_meshes: u32,
    pub verts_normal_array: *const LupinVertexBufferDesc, pub num_normal_buffers: u32,
    pub verts_texcoord_array: *const LupinVertexBufferDesc, pub num_texcoord_buffers: u32,
    pub verts_color_array: *const LupinVertexBufferDesc, pub num_color_buffers: u32,
    pub instances: *const LupinInstance, pub num_instances: u32,
    pub materials: *const LupinMaterial, pub num_materials: u32,
    pub textures: *const LupinTextureDesc, pub num_textures: u32,
    pub environments: *const LupinEnvironment, pub num_environments: u32,
    pub tlas_nodes: *const LupinTlasNode, pub num_tlas_nodes: u32,
    pub lights: *const LupinLight, pub num_lights: u32,
    pub alias_tables: *const LupinAliasTableDesc, pub env_alias_tables: *const LupinAliasTableDesc,
}

#[repr(C)] #[derive(Copy, Clone)] pub struct LupinBakedPathtraceParams { pub with_runtime_checks: u32, pub max_bounces: u32, pub samples_per_pixel: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinCameraParams { pub is_orthographic: u32, pub lens: f32, pub film: f32, pub aspect: f32, pub focus: f32, pub aperture: f32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinAdvancedParams { pub max_radiance: f32, pub rng_seed: u32, pub ray_epsilon: f32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinTileParams { pub tile_size: u32, pub tile_idx: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinAccumulationParams { pub prev_frame: *const LupinTexture, pub accum_counter: u32 }
#[repr(C)] pub struct LupinPathtraceDesc {
    pub accum_params: *const LupinAccumulationParams, pub tile_params: *const LupinTileParams,
    pub camera_params: LupinCameraParams, pub camera_transform: LupinMat3x4, pub force_software_bvh: u32, pub advanced: LupinAdvancedParams,
}
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinDebugVizDesc { pub viz_type: u32, pub heatmap_min: f32, pub heatmap_max: f32, pub first_hit_only: u32 }
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinTonemapDesc {
    pub has_viewport: u32, pub viewport_x: f32, pub viewport_y: f32, pub viewport_w: f32, pub viewport_h: f32,
    pub exposure: f32, pub filmic: u32, pub srgb: u32, pub clear: u32,
}
// denoising.rs:193-218 (quality: 0 Low, 1 Medium, 2 High = the reference's default)
pub const LUPIN_DENOISE_LOW: u32 = 0;
pub const LUPIN_DENOISE_MEDIUM: u32 = 1;
pub const LUPIN_DENOISE_HIGH: u32 = 2;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinDenoiseDesc {
    pub pathtrace_output: *const LupinTexture, pub albedo: *const LupinTexture, pub normals: *const LupinTexture,
    pub denoise_output: *mut LupinTexture, pub quality: u32,
}
// adaptive sampling (no reference counterpart)
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinAdaptiveParams { pub threshold: f32, pub min_frames: u32, pub max_frames: u32 }
#[repr(C)] #[derive(Copy, Clone, Default, Debug)] pub struct LupinAdaptiveStats {
    pub active_pixels: u64, pub pixel_frames: u64, pub calls: u32, pub max_frames_taken: u32,
}
// reprojection of the adaptive history (no reference counterpart)
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinReprojectDesc {
    pub camera_params: LupinCameraParams, pub camera_transform: LupinMat3x4, pub ray_epsilon: f32, pub depth_tolerance: f32, pub max_history: u32,
    pub prev_instance_transforms: *const LupinMat4x3, pub num_instances: u32,
}
// radiance queries (no reference counterpart)
pub const LUPIN_RAY_DIRECTION: u32 = 0;
pub const LUPIN_RAY_COSINE_HEMISPHERE: u32 = 1;
pub const LUPIN_RAYS_DEVICE_POINTERS: u32 = 1;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinRayQueryDesc {
    pub pathtrace_type: u32, pub max_bounces: u32, pub samples: u32, pub flags: u32, pub max_slots: u32, pub advanced: LupinAdvancedParams,
}
// lightmap baking (no reference counterpart)
pub const LUPIN_LIGHTMAP_SMOOTH_NORMALS: u32 = 1;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinLightmapChart {
    pub instance_idx: u32, pub scale_u: f32, pub scale_v: f32, pub offset_u: f32, pub offset_v: f32,
}
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinLightmapDesc {
    pub width: u32, pub height: u32, pub pathtrace_type: u32, pub max_bounces: u32, pub samples: u32, pub max_slots: u32, pub flags: u32,
    pub dilate: u32, pub counter: u32, pub surface_offset: f32, pub advanced: LupinAdvancedParams,
}
#[repr(C)] #[derive(Copy, Clone, Default, Debug)] pub struct LupinLightmapStats {
    pub covered_texels: u64, pub keys: u32, pub raster_ms: f32, pub compact_ms: f32, pub trace_ms: f32, pub scatter_dilate_ms: f32, pub download_ms: f32,
}
// adaptive lightmap baking (no reference counterpart)
pub const LUPIN_RAY_MOMENTS_FLOATS: usize = 8;
pub const LUPIN_LIGHTMAP_ADAPTIVE_MAX_ROUNDS: u32 = 4096;
pub const LUPIN_LIGHTMAP_ADAPTIVE_STATS_FLOATS: usize = 4;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinLightmapAdaptiveDesc {
    pub threshold: f32, pub min_rounds: u32, pub max_rounds: u32, pub flags: u32,
}
#[repr(C)] #[derive(Copy, Clone, Default, Debug)] pub struct LupinLightmapAdaptiveStats {
    pub covered_texels: u64, pub paths: u64, pub converged_texels: u64, pub capped_texels: u64, pub rounds: u32, pub keys: u32,
    pub raster_ms: f32, pub compact_ms: f32, pub trace_ms: f32, pub merge_mask_ms: f32, pub scatter_dilate_ms: f32, pub download_ms: f32,
}
// lightmap UV sets and their generation (no reference counterpart)
pub const LUPIN_UNWRAP_MAX_PADDING: u32 = 16;
pub const LUPIN_UNWRAP_NO_CHART: u32 = 0xFFFF_FFFF;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinUnwrapDesc {
    pub texel_size: f32, pub padding: u32, pub flags: u32,
}
#[repr(C)] #[derive(Copy, Clone, Default, Debug)] pub struct LupinUnwrapInfo {
    pub num_charts: u32, pub width: u32, pub height: u32, pub degenerate_tris: u32,
    pub charts_ms: f32, pub rects_ms: f32, pub pack_ms: f32, pub uvs_ms: f32,
}
// lightmap denoising (no reference counterpart)
pub const LUPIN_LIGHTMAP_DENOISE_DEVICE_POINTERS: u32 = 1;
pub const LUPIN_LIGHTMAP_DENOISE_MAX_PASSES: u32 = 8;
pub const LUPIN_LIGHTMAP_DENOISE_MAX_SQUARINGS: u32 = 7;
// lightmap seam stitching (no reference counterpart)
pub const LUPIN_LIGHTMAP_STITCH_DEVICE_POINTERS: u32 = 1;
pub const LUPIN_LIGHTMAP_STITCH_MAX_ITERATIONS: u32 = 1024;
pub const LUPIN_LIGHTMAP_STITCH_MAX_EDGE_SAMPLES: u32 = 65536;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinLightmapStitchDesc {
    pub width: u32, pub height: u32, pub iterations: u32, pub samples_per_texel: f32, pub lambda: f32, pub flags: u32, pub reserved: u32,
}
#[repr(C)] #[derive(Copy, Clone, Default, Debug)] pub struct LupinLightmapStitchInfo {
    pub seam_edges: u32, pub non_manifold_edges: u32, pub sample_pairs: u32, pub dropped_pairs: u32, pub active_texels: u32, pub iterations: u32,
    pub energy_before: [f32; 3], pub energy_after: [f32; 3],
}
#[repr(C)] #[derive(Copy, Clone, Default, Debug)] pub struct LupinLightmapStitchStats {
    pub edges_ms: f32, pub samples_ms: f32, pub incidence_ms: f32, pub solve_ms: f32, pub call_ms: f32,
}
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinLightmapDenoiseDesc {
    pub width: u32, pub height: u32, pub passes: u32, pub normal_squarings: u32, pub dilate: u32, pub flags: u32, pub max_stretch: f32,
}
#[repr(C)] #[derive(Copy, Clone, Default, Debug)] pub struct LupinLightmapDenoiseStats {
    pub prep_ms: f32, pub pass_ms: [f32; 8], pub dilate_ms: f32, pub call_ms: f32,
}
// light-probe baking (no reference counterpart)
pub const LUPIN_PROBE_FLOATS: usize = 4;
pub const LUPIN_PROBE_SH_COEFFS: usize = 9;
pub const LUPIN_PROBE_RESULT_FLOATS: usize = 36;
pub const LUPIN_PROBES_DEVICE_POINTERS: u32 = 1;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinProbeDesc {
    pub pathtrace_type: u32, pub max_bounces: u32, pub samples: u32, pub flags: u32, pub max_slots: u32, pub advanced: LupinAdvancedParams,
}
// occlusion queries (no reference counterpart)
pub const LUPIN_OCCLUSION_RECORD_FLOATS: usize = 8;
pub const LUPIN_OCCLUSION_DIRECTION: u32 = 0;
pub const LUPIN_OCCLUSION_COSINE_HEMISPHERE: u32 = 1;
pub const LUPIN_OCCLUSION_DEVICE_POINTERS: u32 = 1;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinOcclusionDesc {
    pub mode: u32, pub samples: u32, pub flags: u32, pub ray_epsilon: f32,
}
// bent-normal queries and the ambient-occlusion atlas (no reference counterpart)
pub const LUPIN_BENT_NORMAL_RESULT_FLOATS: usize = 4;
pub const LUPIN_BENT_NORMAL_DEVICE_POINTERS: u32 = 1;
pub const LUPIN_BENT_NORMAL_OPACITY: u32 = 2;
pub const LUPIN_LIGHTMAP_AO_OPACITY: u32 = 2;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinBentNormalDesc {
    pub samples: u32, pub flags: u32, pub max_slots: u32, pub ray_epsilon: f32,
}
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinLightmapAoDesc {
    pub width: u32, pub height: u32, pub samples: u32, pub max_slots: u32, pub flags: u32, pub dilate: u32, pub counter: u32,
    pub surface_offset: f32, pub max_distance: f32, pub ray_epsilon: f32,
}
// distance queries (no reference counterpart)
pub const LUPIN_DISTANCE_RECORD_FLOATS: usize = 4;
pub const LUPIN_DISTANCE_RESULT_FLOATS: usize = 12;
pub const LUPIN_DISTANCE_DEVICE_POINTERS: u32 = 1;
pub const LUPIN_DISTANCE_GRID_SIGNED: u32 = 2;
// irradiance volume lookup (no reference counterpart)
pub const LUPIN_PROBE_GRID_RECORD_FLOATS: usize = 8;
pub const LUPIN_PROBE_GRID_RESULT_FLOATS: usize = 4;
pub const LUPIN_PROBE_GRID_DEVICE_POINTERS: u32 = 1;
pub const LUPIN_PROBE_GRID_VISIBILITY: u32 = 2;
pub const LUPIN_PROBE_GRID_BACKFACE: u32 = 4;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinProbeGridDesc {
    pub origin: [f32; 3], pub spacing: [f32; 3], pub dims: [u32; 3], pub flags: u32, pub ray_epsilon: f32, pub normal_bias: f32,
}
// probe depth maps (no reference counterpart)
pub const LUPIN_PROBE_DEPTH_STATS_WORDS: usize = 4;
pub const LUPIN_PROBE_DEPTH_DEVICE_POINTERS: u32 = 1;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinProbeDepthDesc {
    pub resolution: u32, pub subsamples: u32, pub flags: u32, pub max_slots: u32, pub ray_epsilon: f32, pub max_distance: f32,
}
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinProbeGridDepthDesc {
    pub grid: LupinProbeGridDesc, pub resolution: u32, pub max_distance: f32,
}
// baked-lighting view (no reference counterpart)
pub const LUPIN_BAKED_VIEW_GBUFFER_FLOATS: usize = 16;
pub const LUPIN_BAKED_VIEW_MISS: u32 = 0xFFFF_FFFF;
pub const LUPIN_BAKED_VIEW_DEVICE_POINTERS: u32 = 1;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinBakedViewDesc {
    pub camera_params: LupinCameraParams, pub camera_transform: LupinMat3x4, pub grid: LupinProbeGridDesc, pub resolution: u32, pub max_distance: f32,
    pub ray_epsilon: f32, pub ambient: [f32; 3], pub flags: u32, pub max_slots: u32,
}
pub const LUPIN_LIGHTMAPPED_VIEW_GBUFFER_FLOATS: usize = 20;
pub const LUPIN_LIGHTMAPPED_SOURCE_MISS: u32 = 0;
pub const LUPIN_LIGHTMAPPED_SOURCE_LIGHTMAP: u32 = 1;
pub const LUPIN_LIGHTMAPPED_SOURCE_PROBES: u32 = 2;
pub const LUPIN_LIGHTMAPPED_SOURCE_AMBIENT: u32 = 3;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinLightmappedViewDesc {
    pub view: LupinBakedViewDesc, pub lightmap_width: u32, pub lightmap_height: u32, pub num_charts: u32, pub reserved: u32,
}
// directional lightmaps and their view (no reference counterpart)
pub const LUPIN_LIGHTMAP_DIRECTIONAL_PLANES: usize = 4;
pub const LUPIN_LIGHTMAPPED_DIRECTIONAL_GBUFFER_FLOATS: usize = 24;
pub const LUPIN_LIGHTMAPPED_DIRECTIONAL_APPLIED: u32 = 1;
pub const LUPIN_LIGHTMAPPED_DIRECTIONAL_BACK_FACE: u32 = 2;
pub const LUPIN_LIGHTMAPPED_DIRECTIONAL_DEN_NOT_POSITIVE: u32 = 4;
pub const LUPIN_LIGHTMAPPED_DIRECTIONAL_NOT_FINITE: u32 = 8;
#[repr(C)] #[derive(Copy, Clone)] pub struct LupinLightmappedDirectionalDesc {
    pub base: LupinLightmappedViewDesc, pub bake_flags: u32, pub reserved: [u32; 3],
}

extern "C" {
    pub fn lupin_hip_last_error() -> *const c_char;
    pub fn lupin_hip_device_count() -> c_int;
    pub fn lupin_hip_create_context(device_ordinal: c_int, out: *mut *mut LupinContext) -> c_int;
    pub fn lupin_hip_destroy_context(ctx: *mut LupinContext);
    pub fn lupin_hip_sync(ctx: *mut LupinContext) -> c_int;
    pub fn lupin_hip_build_pathtrace_resources(ctx: *mut LupinContext, p: *const LupinBakedPathtraceParams, out: *mut *mut LupinPathtraceResources) -> c_int;
    pub fn lupin_hip_destroy_pathtrace_resources(res: *mut LupinPathtraceResources);
    pub fn lupin_hip_scene_create(ctx: *mut LupinContext, desc: *const LupinSceneDesc, out: *mut *mut LupinScene) -> c_int;
    pub fn lupin_hip_scene_destroy(scene: *mut LupinScene);
    // moves the instances in place: new transforms, TLAS rebuilt (tlas_builder 0 = lupin_build_tlas, 1 = on the device)
    pub fn lupin_hip_scene_update_instances(scene: *mut LupinScene, transpose_inverse_transforms: *const LupinMat4x3, num_instances: u32, tlas_builder: c_int) -> c_int;
    pub fn lupin_hip_texture_create(ctx: *mut LupinContext, w: u32, h: u32, out: *mut *mut LupinTexture) -> c_int;
    pub fn lupin_hip_texture_destroy(tex: *mut LupinTexture);
    pub fn lupin_hip_texture_width(tex: *const LupinTexture) -> u32;
    pub fn lupin_hip_texture_height(tex: *const LupinTexture) -> u32;
    pub fn lupin_hip_texture_upload_rgba16f(tex: *mut LupinTexture, pixels: *const u16) -> c_int;
    pub fn lupin_hip_texture_download_rgba16f(tex: *const LupinTexture, out_pixels: *mut u16) -> c_int;
    pub fn lupin_hip_dbuf_create(ctx: *mut LupinContext, w: u32, h: u32, out: *mut *mut LupinDoubleBufferedTexture) -> c_int;
    pub fn lupin_hip_dbuf_destroy(t: *mut LupinDoubleBufferedTexture);
    pub fn lupin_hip_dbuf_front(t: *mut LupinDoubleBufferedTexture) -> *mut LupinTexture;
    pub fn lupin_hip_dbuf_back(t: *mut LupinDoubleBufferedTexture) -> *mut LupinTexture;
    pub fn lupin_hip_dbuf_flip(t: *mut LupinDoubleBufferedTexture);
    pub fn lupin_hip_dbuf_copy_front_to_back(t: *mut LupinDoubleBufferedTexture) -> c_int;
    pub fn lupin_hip_dbuf_resize(t: *mut LupinDoubleBufferedTexture, w: u32, h: u32) -> c_int;
    pub fn lupin_hip_get_num_tiles(tile_size: u32, w: u32, h: u32) -> u32;
    pub fn lupin_hip_pathtrace_scene(ctx: *mut LupinContext, res: *const LupinPathtraceResources, scene: *const LupinScene,
                                     target: *mut LupinTexture, pathtrace_type: u32, desc: *const LupinPathtraceDesc) -> c_int;
    pub fn lupin_hip_pathtrace_scene_falsecolor(ctx: *mut LupinContext, res: *const LupinPathtraceResources, scene: *const LupinScene,
                                                target: *mut LupinTexture, falsecolor_type: u32, desc: *const LupinPathtraceDesc) -> c_int;
    pub fn lupin_hip_pathtrace_scene_debug(ctx: *mut LupinContext, res: *const LupinPathtraceResources, scene: *const LupinScene,
                                           target: *mut LupinTexture, debug_desc: *const LupinDebugVizDesc, desc: *const LupinPathtraceDesc) -> c_int;
    pub fn lupin_hip_pathtrace_scene_tiles(ctx: *mut LupinContext, res: *const LupinPathtraceResources, scene: *const LupinScene,
                                           target: *mut LupinTexture, pathtrace_type: u32, desc: *const LupinPathtraceDesc,
                                           tile_size: u32, rank: u32, world: u32) -> c_int;
    // multi-GPU: the one exchange step (RCCL all-gather of tile payloads over xGMI) and its communicators
    pub fn lupin_hip_comm_get_unique_id(out_id: *mut u8) -> c_int;
    pub fn lupin_hip_comm_init_rank(ctx: *mut LupinContext, id: *const u8, rank: u32, world: u32, out: *mut *mut LupinComm) -> c_int;
    pub fn lupin_hip_comm_init_all(ctxs: *const *mut LupinContext, n: u32, out_comms: *mut *mut LupinComm) -> c_int;
    pub fn lupin_hip_comm_from_nccl(ctx: *mut LupinContext, nccl_comm: *mut c_void, rank: u32, world: u32, out: *mut *mut LupinComm) -> c_int;
    pub fn lupin_hip_comm_destroy(comm: *mut LupinComm);
    pub fn lupin_hip_comm_rank(comm: *const LupinComm) -> u32;
    pub fn lupin_hip_comm_world(comm: *const LupinComm) -> u32;
    pub fn lupin_hip_gather_framebuffer(comm: *mut LupinComm, tex: *mut LupinTexture, tile_size: u32) -> c_int;
    pub fn lupin_hip_gather_framebuffer_all(comms: *const *mut LupinComm, texs: *const *mut LupinTexture, n: u32, tile_size: u32) -> c_int;
    pub fn lupin_hip_gather_framebuffer_to(comm: *mut LupinComm, tex: *mut LupinTexture, tile_size: u32, root: u32) -> c_int;
    pub fn lupin_hip_comm_barrier(comm: *mut LupinComm) -> c_int;
    pub fn lupin_hip_comm_allreduce_f64(comm: *mut LupinComm, inout: *mut f64, n: u32, op: u32) -> c_int;
    // accumulation mode (f16 running average = reference, or f32 accumulator) and its readback
    pub fn lupin_hip_set_accumulation_mode(ctx: *mut LupinContext, mode: c_int) -> c_int;
    pub fn lupin_hip_reserve_path_state(ctx: *mut LupinContext, pixels: u64, max_bounces: u32, samples_per_pixel: u32) -> c_int;
    pub fn lupin_hip_set_batch_frames(ctx: *mut LupinContext, frames: u32) -> c_int;
    pub fn lupin_hip_set_traversal(ctx: *mut LupinContext, mode: c_int) -> c_int;
    pub fn lupin_hip_texture_download_rgba32f(tex: *const LupinTexture, out_pixels: *mut f32) -> c_int;
    pub fn lupin_hip_tonemap_and_fit_aspect(ctx: *mut LupinContext, src: *const LupinTexture, dst_rgba8: *mut u8, w: u32, h: u32,
                                            desc: *const LupinTonemapDesc) -> c_int;
    // lp::build_denoise_resources / denoise (denoising.rs:83-306), the library's own a-trous filter in place of OIDN
    pub fn lupin_hip_build_denoise_resources(ctx: *mut LupinContext, width: u32, height: u32, out: *mut *mut LupinDenoiseResources) -> c_int;
    pub fn lupin_hip_destroy_denoise_resources(res: *mut LupinDenoiseResources);
    pub fn lupin_hip_denoise(ctx: *mut LupinContext, res: *mut LupinDenoiseResources, desc: *const LupinDenoiseDesc) -> c_int;
    // adaptive sampling: only 8x8 blocks that have not converged are rendered
    pub fn lupin_hip_build_adaptive_resources(ctx: *mut LupinContext, width: u32, height: u32, out: *mut *mut LupinAdaptiveResources) -> c_int;
    pub fn lupin_hip_destroy_adaptive_resources(res: *mut LupinAdaptiveResources);
    pub fn lupin_hip_adaptive_reset(ctx: *mut LupinContext, res: *mut LupinAdaptiveResources) -> c_int;
    pub fn lupin_hip_pathtrace_scene_adaptive(ctx: *mut LupinContext, res: *const LupinPathtraceResources, scene: *const LupinScene,
                                              render_target: *mut LupinTexture, pathtrace_type: u32, desc: *const LupinPathtraceDesc,
                                              ares: *mut LupinAdaptiveResources, params: *const LupinAdaptiveParams) -> c_int;
    pub fn lupin_hip_adaptive_stats(ctx: *mut LupinContext, ares: *const LupinAdaptiveResources, out: *mut LupinAdaptiveStats) -> c_int;
    pub fn lupin_hip_adaptive_download(ctx: *mut LupinContext, ares: *const LupinAdaptiveResources, frames: *mut u32, moments: *mut f32,
                                       block_error: *mut f32, block_active: *mut u8) -> c_int;
    // reprojection: carries the image and the adaptive state over to a new view (camera or instances moved)
    pub fn lupin_hip_build_reproject_resources(ctx: *mut LupinContext, width: u32, height: u32, out: *mut *mut LupinReprojectResources) -> c_int;
    pub fn lupin_hip_destroy_reproject_resources(res: *mut LupinReprojectResources);
    pub fn lupin_hip_reproject_invalidate(ctx: *mut LupinContext, res: *mut LupinReprojectResources) -> c_int;
    pub fn lupin_hip_adaptive_reproject(ctx: *mut LupinContext, ares: *mut LupinAdaptiveResources, res: *mut LupinReprojectResources, scene: *const LupinScene,
                                        desc: *const LupinReprojectDesc, history_in: *const LupinTexture, history_out: *mut LupinTexture) -> c_int;
    pub fn lupin_hip_reproject_timings(ctx: *mut LupinContext, res: *const LupinReprojectResources, trace_ms: *mut f32, gather_ms: *mut f32) -> c_int;
    pub fn lupin_hip_reproject_download(ctx: *mut LupinContext, res: *const LupinReprojectResources, which: c_int, inst: *mut u32, tri: *mut u32,
                                        uv: *mut f32, depth: *mut f32) -> c_int;
    // radiance queries: the integrators over n caller-supplied rays (records n x 8 f32, out n x 4, out_rays null or n * samples x 8)
    pub fn lupin_hip_pathtrace_rays(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinRayQueryDesc, n: u64,
                                    records: *const f32, out: *mut f32, out_rays: *mut f32) -> c_int;
    // lightmap baking: out_rgba height x width x 4 f32, out_records null or height x width x 8, out_num_covered null ok
    pub fn lupin_hip_bake_lightmap(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinLightmapDesc,
                                   charts: *const LupinLightmapChart, num_charts: u32, out_rgba: *mut f32, out_records: *mut f32,
                                   out_num_covered: *mut u64) -> c_int;
    pub fn lupin_hip_lightmap_stats(out: *mut LupinLightmapStats);
    // lightmap denoising: rgba and out_rgba height x width x 4 f32 (they may be the same), records height x width x 8
    pub fn lupin_hip_denoise_lightmap(ctx: *mut LupinContext, desc: *const LupinLightmapDenoiseDesc, rgba: *const f32, records: *const f32,
                                      out_rgba: *mut f32) -> c_int;
    pub fn lupin_hip_lightmap_denoise_stats(out: *mut LupinLightmapDenoiseStats);
    // lightmap seam stitching: rgba and out_rgba height x width x 4 f32 (they may be the same), out_info null ok
    pub fn lupin_hip_stitch_lightmap(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinLightmapStitchDesc,
                                     charts: *const LupinLightmapChart, num_charts: u32, rgba: *const f32, out_rgba: *mut f32,
                                     out_info: *mut LupinLightmapStitchInfo) -> c_int;
    pub fn lupin_hip_lightmap_stitch_stats(out: *mut LupinLightmapStitchStats) -> c_int;
    // light-probe baking: probes n x 4 f32 (position | RNG word), out_sh n x 9 x 4 (r, g, b, w per L2 SH coefficient), out_rays null or n * samples x 8
    pub fn lupin_hip_bake_probes(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinProbeDesc, n: u64,
                                 probes: *const f32, out_sh: *mut f32, out_rays: *mut f32) -> c_int;
    // occlusion queries: records n x 8 f32 (origin | RNG bits, unit direction or normal | tmax), out_blocked n counts
    pub fn lupin_hip_occlusion_rays(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinOcclusionDesc, n: u64,
                                    records: *const f32, out_blocked: *mut u32) -> c_int;
    pub fn lupin_hip_transmittance_rays(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinOcclusionDesc, n: u64, records: *const f32, out_sum: *mut f32) -> c_int;
    // bent-normal queries: hemisphere-mode occlusion records, out n x 4 f32 (sum T d.xyz | sum T)
    pub fn lupin_hip_bent_normal_rays(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinBentNormalDesc, n: u64, records: *const f32, out: *mut f32) -> c_int;
    // ambient-occlusion atlas: out_ao height x width x 4 f32, out_bent null or the same, out_records null or height x width x 8, out_num_covered null ok
    pub fn lupin_hip_bake_lightmap_ao(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinLightmapAoDesc,
                                      charts: *const LupinLightmapChart, num_charts: u32, out_ao: *mut f32, out_bent: *mut f32,
                                      out_records: *mut f32, out_num_covered: *mut u64) -> c_int;
    // distance queries: records n x 4 f32 (point | rmax), out_results n x 12 f32 words; the grid: x fastest, one f32 per voxel
    pub fn lupin_hip_distance_points(ctx: *mut LupinContext, scene: *const LupinScene, flags: u32, n: u64, records: *const f32, out_results: *mut f32) -> c_int;
    pub fn lupin_hip_bake_distance_grid(ctx: *mut LupinContext, scene: *const LupinScene, flags: u32, origin: *const f32, spacing: *const f32,
                                        dims: *const u32, rmax: f32, out_volume: *mut f32) -> c_int;
    // irradiance volume lookup: sh P x 9 x 4 f32 (bake_probes' out_sh), valid null or P bytes, records n x 8 f32 (point | -, unit normal | -), out n x 4
    pub fn lupin_hip_sample_probe_grid(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinProbeGridDesc, sh: *const f32,
                                       valid: *const u8, n: u64, records: *const f32, out: *mut f32) -> c_int;
    // probe depth maps: positions n x 4 f32, out_depth n x (R + 2) x (R + 2) x 2 f32, out_stats null or n x 4 u32
    pub fn lupin_hip_bake_probe_depth(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinProbeDepthDesc, n: u64, positions: *const f32,
                                      out_depth: *mut f32, out_stats: *mut u32) -> c_int;
    // ... and the lookup that reads them: depth P x (R + 2) x (R + 2) x 2 f32; the rest as lupin_hip_sample_probe_grid
    pub fn lupin_hip_sample_probe_grid_depth(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinProbeGridDepthDesc, sh: *const f32,
                                             depth: *const f32, valid: *const u8, n: u64, records: *const f32, out: *mut f32) -> c_int;
    // baked-lighting view: sh P x 9 x 4 f32, depth null or P x (R + 2) x (R + 2) x 2 f32, valid null or P bytes, out_gbuffer null or W x H x 16 f32
    pub fn lupin_hip_render_baked(ctx: *mut LupinContext, scene: *const LupinScene, render_target: *mut LupinTexture, desc: *const LupinBakedViewDesc,
                                  sh: *const f32, depth: *const f32, valid: *const u8, out_gbuffer: *mut f32) -> c_int;
    // lightmapped view: charts num_charts (host), lightmap height x width x 4 f32, sh null for no volume, out_gbuffer null or W x H x 20
    pub fn lupin_hip_render_lightmapped(ctx: *mut LupinContext, scene: *const LupinScene, render_target: *mut LupinTexture,
                                        desc: *const LupinLightmappedViewDesc, charts: *const LupinLightmapChart, lightmap: *const f32, sh: *const f32,
                                        depth: *const f32, valid: *const u8, out_gbuffer: *mut f32) -> c_int;
    // directional lightmap: out_sh 4 x height x width x 4 f32 (plane j first), out_records null or height x width x 8, out_num_covered null ok
    pub fn lupin_hip_bake_lightmap_directional(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinLightmapDesc,
                                               charts: *const LupinLightmapChart, num_charts: u32, out_sh: *mut f32, out_records: *mut f32,
                                               out_num_covered: *mut u64) -> c_int;
    // ... and the lightmapped view that shades from it: directional 4 x height x width x 4 f32, out_gbuffer null or W x H x 24
    pub fn lupin_hip_render_lightmapped_directional(ctx: *mut LupinContext, scene: *const LupinScene, render_target: *mut LupinTexture,
                                                    desc: *const LupinLightmappedDirectionalDesc, charts: *const LupinLightmapChart,
                                                    lightmap: *const f32, directional: *const f32, sh: *const f32, depth: *const f32,
                                                    valid: *const u8, out_gbuffer: *mut f32) -> c_int;
    // moments of a record's paths: records n x 8 f32, out n x 8 f32 (mean rgb, 1, mean luminance, M2, samples, 0)
    pub fn lupin_hip_pathtrace_rays_moments(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinRayQueryDesc, n: u64,
                                            records: *const f32, out: *mut f32) -> c_int;
    // adaptive lightmap: out_rgba height x width x 4 f32, out_stats null or the same shape, out_records null or height x width x 8
    pub fn lupin_hip_bake_lightmap_adaptive(ctx: *mut LupinContext, scene: *const LupinScene, desc: *const LupinLightmapDesc,
                                            ad: *const LupinLightmapAdaptiveDesc, charts: *const LupinLightmapChart, num_charts: u32,
                                            out_rgba: *mut f32, out_stats: *mut f32, out_records: *mut f32, out_num_covered: *mut u64) -> c_int;
    pub fn lupin_hip_lightmap_adaptive_stats(out: *mut LupinLightmapAdaptiveStats);
    // lightmap UV sets: uvs num_corners x 2 f32 (one per triangle corner) or null to remove the set
    pub fn lupin_hip_scene_set_lightmap_uvs(scene: *mut LupinScene, mesh_idx: u32, uvs: *const f32, num_corners: u64) -> c_int;
    pub fn lupin_hip_scene_mesh_triangle_count(scene: *const LupinScene, mesh_idx: u32) -> i64;
    // out_uvs triangles x 3 x 2 f32 in texels of the mesh's own atlas, out_chart_of_tri null or triangles u32
    pub fn lupin_hip_unwrap_lightmap_uvs(ctx: *mut LupinContext, scene: *const LupinScene, mesh_idx: u32, desc: *const LupinUnwrapDesc,
                                         out_uvs: *mut f32, out_chart_of_tri: *mut u32, out_info: *mut LupinUnwrapInfo) -> c_int;
    // host-side builders with the results of lupin/src/data_structures.rs
    pub fn lupin_build_bvh(verts_pos4: *const f32, num_verts: u32, indices: *mut u32, num_indices: u32, out_nodes: *mut LupinBvhNode, cap: u64) -> i64;
    // the same tree built on the GPU (csrc/sahbvh.hip); cap = 2 * triangles - 1 always suffices
    pub fn lupin_hip_build_bvh_sah_device(ctx: *mut LupinContext, verts_pos4: *const f32, num_verts: u32, indices: *mut u32, num_indices: u32,
                                          out_nodes: *mut LupinBvhNode, cap: u64) -> i64;
    pub fn lupin_build_tlas(instances: *const LupinInstance, n: u32, model_aabbs: *const f32, num_meshes: u32, out: *mut LupinTlasNode) -> i64;
    // the same tree built on the GPU (csrc/tlas.hip)
    pub fn lupin_hip_build_tlas_device(ctx: *mut LupinContext, instances: *const LupinInstance, n: u32, model_aabbs: *const f32, num_meshes: u32,
                                       out: *mut LupinTlasNode) -> i64;
    pub fn lupin_build_alias_table(weights: *const f32, n: u64, out_bins: *mut LupinAliasBin) -> i64;
}
