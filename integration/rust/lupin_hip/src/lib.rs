//! `lupin_hip` -- the reference's public pathtracing surface over the MI355X backend (liblupin_hip.so).
//!
//! SOURCE ONLY: never compiled in this repository (no Rust toolchain in its build environment). It documents,
//! in the reference's own language, how `lp::` maps onto the C ABI of `include/lupin_hip.h`:
//!
//! | reference (crate `lupin_pt`)                         | here                                   |
//! |------------------------------------------------------|----------------------------------------|
//! | `wgpu::Device` + `wgpu::Queue`                       | [`Device`] (one per GPU)               |
//! | `build_pathtrace_resources`, `BakedPathtraceParams`  | [`build_pathtrace_resources`]          |
//! | `Scene`, `build_accel_structures_and_upload`         | [`Scene::upload`] (takes the CPU-built arrays of `SceneCPU` + BVH / TLAS / lights) |
//! | `DoubleBufferedTexture`                              | [`DoubleBufferedTexture`]              |
//! | `pathtrace_scene`, `PathtraceDesc`, `AccumulationParams`, `TileParams` | [`pathtrace_scene`]  |
//! | `pathtrace_scene_falsecolor`, `pathtrace_scene_debug`| [`pathtrace_scene_falsecolor`], [`pathtrace_scene_debug`] |
//! | `tonemap_and_fit_aspect`, `TonemapDesc`              | [`tonemap_and_fit_aspect`]             |
//! | `build_denoise_resources`, `denoise`, `DenoiseDesc`, `DenoiseQuality` | [`build_denoise_resources`], [`denoise`] (own a-trous filter, not OIDN) |
//! | (no counterpart)                                     | [`build_adaptive_resources`], [`pathtrace_scene_adaptive`] (adaptive sampling) |
//! | (no counterpart)                                     | [`build_reproject_resources`], [`adaptive_reproject`] (reprojection of its history) |
//! | (no counterpart: `lp::Scene` is immutable)           | [`Scene::update_instances`] (instance transforms moved in place, device-built TLAS) |
//!
//! Like the reference, failures panic (the reference asserts / panics; the C ABI returns a status + message).
pub mod ffi;
use ffi::*;
use std::ffi::CStr;
use std::ptr;

fn check(rc: i32) {
    if rc != LUPIN_OK {
        let msg = unsafe { CStr::from_ptr(lupin_hip_last_error()) }.to_string_lossy().into_owned();
        panic!("lupin_hip error {}: {}", rc, msg);
    }
}

/// One GPU: HIP context + streams (replaces `wgpu::Device` + `wgpu::Queue`).
pub struct Device { raw: *mut LupinContext }
impl Device {
    pub fn new(ordinal: i32) -> Device { let mut raw = ptr::null_mut(); check(unsafe { lupin_hip_create_context(ordinal, &mut raw) }); Device { raw } }
    /// `device.poll(wait_indefinitely)`
    pub fn sync(&self) { check(unsafe { lupin_hip_sync(self.raw) }); }
}
impl Drop for Device { fn drop(&mut self) { unsafe { lupin_hip_destroy_context(self.raw) } } }

#[derive(Copy, Clone, Debug)] pub struct BakedPathtraceParams { pub with_runtime_checks: bool, pub max_bounces: u32, pub samples_per_pixel: u32 }
impl Default for BakedPathtraceParams { fn default() -> Self { Self { with_runtime_checks: false, max_bounces: 8, samples_per_pixel: 5 } } }   // renderer.rs:458-468
pub struct PathtraceResources { raw: *mut LupinPathtraceResources }
impl Drop for PathtraceResources { fn drop(&mut self) { unsafe { lupin_hip_destroy_pathtrace_resources(self.raw) } } }
pub fn build_pathtrace_resources(device: &Device, p: &BakedPathtraceParams) -> PathtraceResources {
    let c = LupinBakedPathtraceParams { with_runtime_checks: p.with_runtime_checks as u32, max_bounces: p.max_bounces, samples_per_pixel: p.samples_per_pixel };
    let mut raw = ptr::null_mut();
    check(unsafe { lupin_hip_build_pathtrace_resources(device.raw, &c, &mut raw) });
    PathtraceResources { raw }
}

/// Borrowed view of a render target (a `&wgpu::Texture` in the reference).
#[derive(Copy, Clone)] pub struct Texture { raw: *mut LupinTexture }
impl Texture {
    pub fn width(&self) -> u32 { unsafe { lupin_hip_texture_width(self.raw) } }
    pub fn height(&self) -> u32 { unsafe { lupin_hip_texture_height(self.raw) } }
    /// Rgba16Float payload as raw half bits, row 0 = top (`download_texture`, loader.rs:1640-1700); synchronises.
    pub fn download(&self) -> Vec<u16> {
        let mut v = vec![0u16; (self.width() * self.height() * 4) as usize];
        check(unsafe { lupin_hip_texture_download_rgba16f(self.raw, v.as_mut_ptr()) });
        v
    }
}

pub struct DoubleBufferedTexture { raw: *mut LupinDoubleBufferedTexture }   // wgpu_utils.rs:279-348
impl DoubleBufferedTexture {
    pub fn create(device: &Device, width: u32, height: u32) -> Self { let mut raw = ptr::null_mut(); check(unsafe { lupin_hip_dbuf_create(device.raw, width, height, &mut raw) }); Self { raw } }
    pub fn front(&self) -> Texture { Texture { raw: unsafe { lupin_hip_dbuf_front(self.raw) } } }
    pub fn back(&self) -> Texture { Texture { raw: unsafe { lupin_hip_dbuf_back(self.raw) } } }
    pub fn flip(&mut self) { unsafe { lupin_hip_dbuf_flip(self.raw) } }
    pub fn copy_front_to_back(&self) { check(unsafe { lupin_hip_dbuf_copy_front_to_back(self.raw) }); }
    pub fn resize(&mut self, width: u32, height: u32) { check(unsafe { lupin_hip_dbuf_resize(self.raw, width, height) }); }
}
impl Drop for DoubleBufferedTexture { fn drop(&mut self) { unsafe { lupin_hip_dbuf_destroy(self.raw) } } }

/// The arrays `lp::build_accel_structures_and_upload` produces on the CPU before uploading
/// (data_structures.rs:696-872): `SceneCPU`'s vectors plus per-mesh BVH nodes (with the BVH-reordered index
/// buffers), the TLAS and `LightsCPU`. Build them with Lupin's own builders or with `ffi::lupin_build_*`.
pub struct SceneArrays<'a> {
    pub mesh_infos: &'a [LupinMeshInfo],
    pub verts_pos: &'a [Vec<[f32; 4]>], pub indices: &'a [Vec<u32>], pub bvh_nodes: &'a [Vec<LupinBvhNode>],
    pub verts_normal: &'a [Vec<[f32; 4]>], pub verts_texcoord: &'a [Vec<[f32; 2]>], pub verts_color: &'a [Vec<[f32; 4]>],
    pub instances: &'a [LupinInstance], pub materials: &'a [LupinMaterial], pub environments: &'a [LupinEnvironment],
    pub textures: &'a [LupinTextureDesc],
    pub tlas_nodes: &'a [LupinTlasNode], pub lights: &'a [LupinLight],
    pub alias_tables: &'a [Vec<LupinAliasBin>], pub env_alias_tables: &'a [Vec<LupinAliasBin>],
}
pub struct Scene { raw: *mut LupinScene }
impl Scene {
    pub fn upload(device: &Device, s: &SceneArrays) -> Scene {
        let meshes: Vec<LupinMeshDesc> = (0..s.verts_pos.len()).map(|i| LupinMeshDesc {
            verts_pos: s.verts_pos[i].as_ptr() as *const f32, num_verts: s.verts_pos[i].len() as u32,
            indices: s.indices[i].as_ptr(), num_indices: s.indices[i].len() as u32,
            bvh_nodes: s.bvh_nodes[i].as_ptr(), num_bvh_nodes: s.bvh_nodes[i].len() as u32 }).collect();
        let vb4 = |v: &[Vec<[f32; 4]>]| -> Vec<LupinVertexBufferDesc> { v.iter().map(|b| LupinVertexBufferDesc { data: b.as_ptr() as *const f32, num_verts: b.len() as u32 }).collect() };
        let normals = vb4(s.verts_normal);
        let colors = vb4(s.verts_color);
        let uvs: Vec<LupinVertexBufferDesc> = s.verts_texcoord.iter().map(|b| LupinVertexBufferDesc { data: b.as_ptr() as *const f32, num_verts: b.len() as u32 }).collect();
        let tables = |t: &[Vec<LupinAliasBin>]| -> Vec<LupinAliasTableDesc> { t.iter().map(|b| LupinAliasTableDesc { bins: b.as_ptr(), num_bins: b.len() as u32 }).collect() };
        let (alias, env_alias) = (tables(s.alias_tables), tables(s.env_alias_tables));
        let desc = LupinSceneDesc {
            mesh_infos: s.mesh_infos.as_ptr(), meshes: meshes.as_ptr(), num_meshes: meshes.len() as u32,
            verts_normal_array: normals.as_ptr(), num_normal_buffers: normals.len() as u32,
            verts_texcoord_array: uvs.as_ptr(), num_texcoord_buffers: uvs.len() as u32,
            verts_color_array: colors.as_ptr(), num_color_buffers: colors.len() as u32,
            instances: s.instances.as_ptr(), num_instances: s.instances.len() as u32,
            materials: s.materials.as_ptr(), num_materials: s.materials.len() as u32,
            textures: s.textures.as_ptr(), num_textures: s.textures.len() as u32,
            environments: s.environments.as_ptr(), num_environments: s.environments.len() as u32,
            tlas_nodes: s.tlas_nodes.as_ptr(), num_tlas_nodes: s.tlas_nodes.len() as u32,
            lights: s.lights.as_ptr(), num_lights: s.lights.len() as u32,
            alias_tables: alias.as_ptr(), env_alias_tables: env_alias.as_ptr(),
        };
        let mut raw = ptr::null_mut();
        check(unsafe { lupin_hip_scene_create(device.raw, &desc, &mut raw) });
        Scene { raw }
    }
}
impl Scene {
    /// Moves the instances in place (no counterpart in the reference): one `transpose_inverse_transform` per
    /// instance, in instance order; the TLAS is rebuilt on the device (or by `lupin_build_tlas`), nothing else is uploaded again.
    pub fn update_instances(&mut self, transpose_inverse_transforms: &[LupinMat4x3], device_tlas: bool) {
        check(unsafe { lupin_hip_scene_update_instances(self.raw, transpose_inverse_transforms.as_ptr(), transpose_inverse_transforms.len() as u32,
                                                        if device_tlas { 1 } else { 0 }) });
    }
}
impl Drop for Scene { fn drop(&mut self) { unsafe { lupin_hip_scene_destroy(self.raw) } } }

#[repr(u32)] #[derive(Copy, Clone, Debug, PartialEq)] pub enum PathtraceType { Standard = 0, MIS = 1, Naive = 2, Direct = 3 }   // renderer.rs:711-729
#[repr(u32)] #[derive(Copy, Clone, Debug, PartialEq)]
pub enum FalsecolorType { Albedo = 0, Normals, NormalsUnsigned, FrontFacing, Emission, Roughness, Metallic, Opacity, MatType, IsDelta, Instance, Tri }
#[repr(u32)] #[derive(Copy, Clone, Debug, PartialEq)] pub enum DebugVizType { BVHAABBChecks = 0, BVHTriChecks = 1, NumBounces = 2 }
#[derive(Copy, Clone)] pub struct DebugVizDesc { pub viz_type: DebugVizType, pub heatmap_min: f32, pub heatmap_max: f32, pub first_hit_only: bool }

#[derive(Copy, Clone)] pub struct CameraParams { pub is_orthographic: bool, pub lens: f32, pub film: f32, pub aspect: f32, pub focus: f32, pub aperture: f32 }
impl Default for CameraParams { fn default() -> Self { Self { is_orthographic: false, lens: 0.050, film: 0.036, aspect: 1.5, focus: 10000.0, aperture: 0.0 } } }   // renderer.rs:695-707
#[derive(Copy, Clone)] pub struct AdvancedParams { pub max_radiance: f32, pub rng_seed: u32, pub ray_epsilon: f32 }
impl Default for AdvancedParams { fn default() -> Self { Self { max_radiance: 100.0, rng_seed: 0, ray_epsilon: 0.001 } } }   // renderer.rs:739-749
#[derive(Copy, Clone)] pub struct TileParams { pub tile_size: u32, pub tile_idx: u32 }
#[derive(Copy, Clone)] pub struct AccumulationParams { pub prev_frame: Texture, pub accum_counter: u32 }
pub struct PathtraceDesc<'a> {
    pub accum_params: Option<AccumulationParams>, pub tile_params: Option<&'a TileParams>,
    pub camera_params: CameraParams, pub camera_transform: LupinMat3x4, pub force_software_bvh: bool, pub advanced: AdvancedParams,
}

fn with_desc<R>(desc: &PathtraceDesc, f: impl FnOnce(*const LupinPathtraceDesc) -> R) -> R {
    let accum = desc.accum_params.map(|a| LupinAccumulationParams { prev_frame: a.prev_frame.raw, accum_counter: a.accum_counter });
    let tile = desc.tile_params.map(|t| LupinTileParams { tile_size: t.tile_size, tile_idx: t.tile_idx });
    let cp = &desc.camera_params;
    let c = LupinPathtraceDesc {
        accum_params: accum.as_ref().map_or(ptr::null(), |a| a as *const _),
        tile_params: tile.as_ref().map_or(ptr::null(), |t| t as *const _),
        camera_params: LupinCameraParams { is_orthographic: cp.is_orthographic as u32, lens: cp.lens, film: cp.film, aspect: cp.aspect, focus: cp.focus, aperture: cp.aperture },
        camera_transform: desc.camera_transform,
        force_software_bvh: 1,   // the HIP backend is the software-BVH path
        advanced: LupinAdvancedParams { max_radiance: desc.advanced.max_radiance, rng_seed: desc.advanced.rng_seed, ray_epsilon: desc.advanced.ray_epsilon },
    };
    f(&c)
}

pub fn get_num_tiles(tile_size: u32, width: u32, height: u32) -> u32 { unsafe { lupin_hip_get_num_tiles(tile_size, width, height) } }

/// `lp::pathtrace_scene` (renderer.rs:768): enqueues one accumulation frame (or one tile) and returns.
pub fn pathtrace_scene(device: &Device, resources: &PathtraceResources, scene: &Scene, render_target: Texture, pathtrace_type: PathtraceType, desc: &PathtraceDesc) {
    with_desc(desc, |c| check(unsafe { lupin_hip_pathtrace_scene(device.raw, resources.raw, scene.raw, render_target.raw, pathtrace_type as u32, c) }));
}
/// `lp::pathtrace_scene_falsecolor` (renderer.rs:872)
pub fn pathtrace_scene_falsecolor(device: &Device, resources: &PathtraceResources, scene: &Scene, render_target: Texture, falsecolor_type: FalsecolorType, desc: &PathtraceDesc) {
    with_desc(desc, |c| check(unsafe { lupin_hip_pathtrace_scene_falsecolor(device.raw, resources.raw, scene.raw, render_target.raw, falsecolor_type as u32, c) }));
}
/// `lp::pathtrace_scene_debug` (renderer.rs:966)
pub fn pathtrace_scene_debug(device: &Device, resources: &PathtraceResources, scene: &Scene, render_target: Texture, debug_desc: &DebugVizDesc, desc: &PathtraceDesc) {
    let d = LupinDebugVizDesc { viz_type: debug_desc.viz_type as u32, heatmap_min: debug_desc.heatmap_min, heatmap_max: debug_desc.heatmap_max, first_hit_only: debug_desc.first_hit_only as u32 };
    with_desc(desc, |c| check(unsafe { lupin_hip_pathtrace_scene_debug(device.raw, resources.raw, scene.raw, render_target.raw, &d, c) }));
}
/// Multi-GPU extension: every tile `t` with `t % world == rank` of one frame in one launch (one `Device` per GPU).
pub fn pathtrace_scene_tiles(device: &Device, resources: &PathtraceResources, scene: &Scene, render_target: Texture, pathtrace_type: PathtraceType, desc: &PathtraceDesc, tile_size: u32, rank: u32, world: u32) {
    with_desc(desc, |c| check(unsafe { lupin_hip_pathtrace_scene_tiles(device.raw, resources.raw, scene.raw, render_target.raw, pathtrace_type as u32, c, tile_size, rank, world) }));
}

#[derive(Copy, Clone, Default)] pub struct Viewport { pub x: f32, pub y: f32, pub w: f32, pub h: f32 }
#[derive(Copy, Clone)] pub struct TonemapDesc { pub viewport: Option<Viewport>, pub exposure: f32, pub filmic: bool, pub srgb: bool, pub clear: bool }
impl Default for TonemapDesc { fn default() -> Self { Self { viewport: None, exposure: 0.0, filmic: false, srgb: true, clear: true } } }   // tonemapping.rs:120-132
/// `lp::tonemap_and_fit_aspect` (tonemapping.rs:155) into a host Rgba8Unorm image (`dst.len() == w * h * 4`).
pub fn tonemap_and_fit_aspect(device: &Device, src: Texture, dst: &mut [u8], dst_width: u32, dst_height: u32, desc: &TonemapDesc) {
    assert_eq!(dst.len(), (dst_width * dst_height * 4) as usize);
    let v = desc.viewport.unwrap_or_default();
    let c = LupinTonemapDesc { has_viewport: desc.viewport.is_some() as u32, viewport_x: v.x, viewport_y: v.y, viewport_w: v.w, viewport_h: v.h,
                               exposure: desc.exposure, filmic: desc.filmic as u32, srgb: desc.srgb as u32, clear: desc.clear as u32 };
    check(unsafe { lupin_hip_tonemap_and_fit_aspect(device.raw, src.raw, dst.as_mut_ptr(), dst_width, dst_height, &c) });
}

/// `lp::DenoiseResources` (denoising.rs:56): scratch of one width x height.
pub struct DenoiseResources { raw: *mut LupinDenoiseResources }
impl Drop for DenoiseResources { fn drop(&mut self) { unsafe { lupin_hip_destroy_denoise_resources(self.raw) } } }
/// `lp::build_denoise_resources` (denoising.rs:83); the `Device` plays the role of the `DenoiseDevice`.
pub fn build_denoise_resources(device: &Device, width: u32, height: u32) -> DenoiseResources {
    let mut raw = ptr::null_mut();
    check(unsafe { lupin_hip_build_denoise_resources(device.raw, width, height, &mut raw) });
    DenoiseResources { raw }
}
#[derive(Copy, Clone, Debug, Default)] pub enum DenoiseQuality { Low = 0, Medium = 1, #[default] High = 2 }   // denoising.rs:208-218
pub struct DenoiseDesc { pub pathtrace_output: Texture, pub albedo: Option<Texture>, pub normals: Option<Texture>, pub denoise_output: Texture, pub quality: DenoiseQuality }
/// `lp::denoise` (denoising.rs:222): enqueued after every frame so far; returns without a host stall.
pub fn denoise(device: &Device, resources: &mut DenoiseResources, desc: &DenoiseDesc) {
    let c = LupinDenoiseDesc { pathtrace_output: desc.pathtrace_output.raw, albedo: desc.albedo.map_or(ptr::null(), |t| t.raw as *const _),
                               normals: desc.normals.map_or(ptr::null(), |t| t.raw as *const _), denoise_output: desc.denoise_output.raw,
                               quality: desc.quality as u32 };
    check(unsafe { lupin_hip_denoise(device.raw, resources.raw, &c) });
}

/// Adaptive sampling's per-pixel / per-block state (no reference counterpart).
pub struct AdaptiveResources { raw: *mut LupinAdaptiveResources, ctx: *mut LupinContext }
impl Drop for AdaptiveResources { fn drop(&mut self) { unsafe { lupin_hip_destroy_adaptive_resources(self.raw) } } }
impl AdaptiveResources {
    /// Counts and moments to 0, every block active: call it where `accum_counter` goes back to 0.
    pub fn reset(&mut self) { check(unsafe { lupin_hip_adaptive_reset(self.ctx, self.raw) }); }
    pub fn stats(&self) -> LupinAdaptiveStats { let mut s = LupinAdaptiveStats::default(); check(unsafe { lupin_hip_adaptive_stats(self.ctx, self.raw, &mut s) }); s }
}
pub fn build_adaptive_resources(device: &Device, width: u32, height: u32) -> AdaptiveResources {
    let mut raw = ptr::null_mut();
    check(unsafe { lupin_hip_build_adaptive_resources(device.raw, width, height, &mut raw) });
    AdaptiveResources { raw, ctx: device.raw }
}
#[derive(Copy, Clone, Debug)] pub struct AdaptiveParams { pub threshold: f32, pub min_frames: u32, pub max_frames: u32 }
impl Default for AdaptiveParams { fn default() -> Self { Self { threshold: 0.01, min_frames: 8, max_frames: 0 } } }
/// One frame of the blocks that have not converged; `desc.accum_params` is required, `desc.tile_params` must be `None`.
pub fn pathtrace_scene_adaptive(device: &Device, resources: &PathtraceResources, scene: &Scene, render_target: Texture, pathtrace_type: PathtraceType,
                                desc: &PathtraceDesc, adaptive: &mut AdaptiveResources, params: &AdaptiveParams) {
    let p = LupinAdaptiveParams { threshold: params.threshold, min_frames: params.min_frames, max_frames: params.max_frames };
    with_desc(desc, |c| check(unsafe { lupin_hip_pathtrace_scene_adaptive(device.raw, resources.raw, scene.raw, render_target.raw, pathtrace_type as u32, c, adaptive.raw, &p) }));
}

/// Visibility buffers and the previous view of [`adaptive_reproject`] (no reference counterpart).
pub struct ReprojectResources { raw: *mut LupinReprojectResources, ctx: *mut LupinContext, width: u32, height: u32 }
impl Drop for ReprojectResources { fn drop(&mut self) { unsafe { lupin_hip_destroy_reproject_resources(self.raw) } } }
impl ReprojectResources {
    /// Forgets the previous view: call it wherever [`AdaptiveResources::reset`] is called.
    pub fn invalidate(&mut self) { check(unsafe { lupin_hip_reproject_invalidate(self.ctx, self.raw) }); }
    /// Visibility of the latest call's view (`which` = 0) or of the call before it (1); synchronises.  Every slice that is
    /// given must hold width * height entries (`uv`: twice that); `inst` is `u32::MAX` where the ray missed.
    pub fn download(&self, which: i32, inst: Option<&mut [u32]>, tri: Option<&mut [u32]>, uv: Option<&mut [f32]>, depth: Option<&mut [f32]>) {
        let px = (self.width as usize) * (self.height as usize);
        assert!(inst.as_ref().map_or(true, |s| s.len() == px) && tri.as_ref().map_or(true, |s| s.len() == px));
        assert!(uv.as_ref().map_or(true, |s| s.len() == 2 * px) && depth.as_ref().map_or(true, |s| s.len() == px));
        check(unsafe { lupin_hip_reproject_download(self.ctx, self.raw, which, inst.map_or(ptr::null_mut(), |s| s.as_mut_ptr()),
                                                    tri.map_or(ptr::null_mut(), |s| s.as_mut_ptr()), uv.map_or(ptr::null_mut(), |s| s.as_mut_ptr()),
                                                    depth.map_or(ptr::null_mut(), |s| s.as_mut_ptr())) });
    }
    /// Device milliseconds `(trace, gather)` of the latest call's two kernels; the call must have run in the kernel-timing stats mode.
    pub fn timings(&self) -> (f32, f32) {
        let (mut t, mut g) = (0f32, 0f32);
        check(unsafe { lupin_hip_reproject_timings(self.ctx, self.raw, &mut t, &mut g) });
        (t, g)
    }
}
pub fn build_reproject_resources(device: &Device, width: u32, height: u32) -> ReprojectResources {
    let mut raw = ptr::null_mut();
    check(unsafe { lupin_hip_build_reproject_resources(device.raw, width, height, &mut raw) });
    ReprojectResources { raw, ctx: device.raw, width, height }
}
pub struct ReprojectDesc<'a> {
    pub camera_params: CameraParams, pub camera_transform: LupinMat3x4, pub ray_epsilon: f32, pub depth_tolerance: f32, pub max_history: u32,
    /// `None`: no instance moved; else one `transpose_inverse_transform` per instance, as the scene held them when `history_in` was rendered.
    pub prev_instance_transforms: Option<&'a [LupinMat4x3]>,
}
/// Rewrites the accumulated image and the adaptive state for the new view; the next adaptive call continues from them.
pub fn adaptive_reproject(device: &Device, adaptive: &mut AdaptiveResources, resources: &mut ReprojectResources, scene: &Scene, desc: &ReprojectDesc,
                          history_in: Texture, history_out: Texture) {
    let cp = &desc.camera_params;
    let c = LupinReprojectDesc {
        camera_params: LupinCameraParams { is_orthographic: cp.is_orthographic as u32, lens: cp.lens, film: cp.film, aspect: cp.aspect, focus: cp.focus, aperture: cp.aperture },
        camera_transform: desc.camera_transform, ray_epsilon: desc.ray_epsilon, depth_tolerance: desc.depth_tolerance, max_history: desc.max_history,
        prev_instance_transforms: desc.prev_instance_transforms.map_or(ptr::null(), |t| t.as_ptr()),
        num_instances: desc.prev_instance_transforms.map_or(0, |t| t.len() as u32),
    };
    check(unsafe { lupin_hip_adaptive_reproject(device.raw, adaptive.raw, resources.raw, scene.raw, &c, history_in.raw, history_out.raw) });
}

// ---- occlusion queries (no reference counterpart) ----
#[derive(Copy, Clone, PartialEq, Eq)] pub enum OcclusionMode { Direction = 0, CosineHemisphere = 1 }
/// Per record (8 floats: origin | RNG bits, unit direction or normal | tmax), the number of its `samples` slots whose segment is
/// blocked by some triangle at `ray_epsilon <= t < tmax`.  Geometric visibility: material opacity is not consulted.
pub fn occlusion_rays(device: &Device, scene: &Scene, records: &[f32], mode: OcclusionMode, samples: u32, ray_epsilon: f32) -> Vec<u32> {
    assert!(records.len() % LUPIN_OCCLUSION_RECORD_FLOATS == 0);
    let n = records.len() / LUPIN_OCCLUSION_RECORD_FLOATS;
    let mut out = vec![0u32; n];
    let c = LupinOcclusionDesc { mode: mode as u32, samples, flags: 0, ray_epsilon };
    check(unsafe { lupin_hip_occlusion_rays(device.raw, scene.raw, &c, n as u64, records.as_ptr(), out.as_mut_ptr()) });
    out
}

/// Transmittance queries: per record of `occlusion_rays`' layout, the sum over its `samples` slots of the product
/// of `1 - opacity` over the surfaces at `ray_epsilon <= t < tmax` (0 once an opacity of 1 is met).  Divide by `samples`.
pub fn transmittance_rays(device: &Device, scene: &Scene, records: &[f32], mode: OcclusionMode, samples: u32, ray_epsilon: f32) -> Vec<f32> {
    assert!(records.len() % LUPIN_OCCLUSION_RECORD_FLOATS == 0);
    let n = records.len() / LUPIN_OCCLUSION_RECORD_FLOATS;
    let mut out = vec![0f32; n];
    let c = LupinOcclusionDesc { mode: mode as u32, samples, flags: 0, ray_epsilon };
    check(unsafe { lupin_hip_transmittance_rays(device.raw, scene.raw, &c, n as u64, records.as_ptr(), out.as_mut_ptr()) });
    out
}

// ---- bent-normal queries and the ambient-occlusion atlas (no reference counterpart) ----
/// Per hemisphere-mode record of `occlusion_rays`' layout, four sums over its `samples` cosine-weighted slots:
/// `(sum T d.x, sum T d.y, sum T d.z, sum T)`, `T` = 1 / 0 (open / blocked) or with `opacity` the slot's transmittance.
/// `[3] / samples` is the ambient-occlusion visibility, `[0..3]` normalised the bent normal.
pub fn bent_normal_rays(device: &Device, scene: &Scene, records: &[f32], samples: u32, ray_epsilon: f32, opacity: bool) -> Vec<f32> {
    assert!(records.len() % LUPIN_OCCLUSION_RECORD_FLOATS == 0);
    let n = records.len() / LUPIN_OCCLUSION_RECORD_FLOATS;
    let mut out = vec![0f32; n * LUPIN_BENT_NORMAL_RESULT_FLOATS];
    let c = LupinBentNormalDesc { samples, flags: if opacity { LUPIN_BENT_NORMAL_OPACITY } else { 0 }, max_slots: 0, ray_epsilon };
    check(unsafe { lupin_hip_bent_normal_rays(device.raw, scene.raw, &c, n as u64, records.as_ptr(), out.as_mut_ptr()) });
    out
}

/// The ambient-occlusion map and the bent-normal map of `charts` in a `desc.height` x `desc.width` atlas (x 4 floats each,
/// alpha = ownership), laid out as `lupin_hip_bake_lightmap` lays out its lightmap.
pub fn bake_lightmap_ao(device: &Device, scene: &Scene, desc: &LupinLightmapAoDesc, charts: &[LupinLightmapChart]) -> (Vec<f32>, Vec<f32>) {
    let texels = desc.width as usize * desc.height as usize;
    let (mut ao, mut bent) = (vec![0f32; texels * 4], vec![0f32; texels * 4]);
    check(unsafe { lupin_hip_bake_lightmap_ao(device.raw, scene.raw, desc, charts.as_ptr(), charts.len() as u32, ao.as_mut_ptr(), bent.as_mut_ptr(),
                                              std::ptr::null_mut(), std::ptr::null_mut()) });
    (ao, bent)
}

// ---- distance queries (no reference counterpart) ----
/// The twelve words of a result.  `side` is the side of the reported triangle, not an inside / outside classification.
#[repr(C)] #[derive(Copy, Clone, Debug, Default)] pub struct DistanceResult {
    pub found: u32, pub distance: f32, pub point: [f32; 3], pub u: f32, pub v: f32, pub instance: u32, pub tri: u32, pub side: f32, pub pad: [u32; 2],
}
/// Per record (4 floats: point | rmax, `f32::INFINITY` = unbounded), the nearest surface point in world space.
pub fn distance_points(device: &Device, scene: &Scene, records: &[f32]) -> Vec<DistanceResult> {
    assert!(records.len() % LUPIN_DISTANCE_RECORD_FLOATS == 0);
    let n = records.len() / LUPIN_DISTANCE_RECORD_FLOATS;
    let mut out = vec![DistanceResult::default(); n];
    check(unsafe { lupin_hip_distance_points(device.raw, scene.raw, 0, n as u64, records.as_ptr(), out.as_mut_ptr() as *mut f32) });
    out
}
/// dims[0] x dims[1] x dims[2] distances, x fastest, at `origin + (i + 0.5) * spacing`; `rmax` where nothing lies within it.
pub fn bake_distance_grid(device: &Device, scene: &Scene, origin: [f32; 3], spacing: [f32; 3], dims: [u32; 3], rmax: f32, signed: bool) -> Vec<f32> {
    let mut out = vec![0f32; dims[0] as usize * dims[1] as usize * dims[2] as usize];
    let flags = if signed { LUPIN_DISTANCE_GRID_SIGNED } else { 0 };
    check(unsafe { lupin_hip_bake_distance_grid(device.raw, scene.raw, flags, origin.as_ptr(), spacing.as_ptr(), dims.as_ptr(), rmax, out.as_mut_ptr()) });
    out
}

// ---- irradiance volume lookup (no reference counterpart) ----
/// Irradiance `(r, g, b, w)` per record (8 floats: point | -, unit normal | -) from a regular grid of `bake_probes` coefficients
/// (`sh`: P x 9 x 4, probe `(ix, iy, iz)` at `origin + i * spacing`, index `ix + dims[0] * (iy + dims[1] * iz)`): trilinear over the
/// cell's eight probes, less the probes with a zero byte in `valid` and, with `visibility`, the probes the scene hides from the
/// point.  `w == 0`: no probe of the cell may be used.  The point is first moved along its normal by `normal_bias` world units.
#[allow(clippy::too_many_arguments)]
pub fn sample_probe_grid(device: &Device, scene: &Scene, origin: [f32; 3], spacing: [f32; 3], dims: [u32; 3], sh: &[f32], valid: Option<&[u8]>,
                         records: &[f32], visibility: bool, backface: bool, ray_epsilon: f32, normal_bias: f32) -> Vec<f32> {
    let probes = dims[0] as usize * dims[1] as usize * dims[2] as usize;
    assert!(sh.len() == probes * 36 && valid.map_or(true, |v| v.len() == probes));
    assert!(records.len() % LUPIN_PROBE_GRID_RECORD_FLOATS == 0);
    let n = records.len() / LUPIN_PROBE_GRID_RECORD_FLOATS;
    let mut out = vec![0f32; n * LUPIN_PROBE_GRID_RESULT_FLOATS];
    let flags = if visibility { LUPIN_PROBE_GRID_VISIBILITY } else { 0 } | if backface { LUPIN_PROBE_GRID_BACKFACE } else { 0 };
    let c = LupinProbeGridDesc { origin, spacing, dims, flags, ray_epsilon, normal_bias };
    check(unsafe { lupin_hip_sample_probe_grid(device.raw, scene.raw, &c, sh.as_ptr(), valid.map_or(std::ptr::null(), |v| v.as_ptr()), n as u64,
                                               records.as_ptr(), out.as_mut_ptr()) });
    out
}

// ---- probe depth maps (no reference counterpart) ----
/// Octahedral distance moments per probe: `(depth, stats)` with `depth` n x (R + 2) x (R + 2) x 2 floats (mean and mean square of the
/// distance to the nearest surface per texel, capped at `max_distance`, the border repeating the texels across the seams) and
/// `stats` n x 4 words (rays, hits, hits on a back face, the bits of the smallest distance).  `positions`: n x 4 floats, `[3]` ignored.
pub fn bake_probe_depth(device: &Device, scene: &Scene, positions: &[f32], resolution: u32, subsamples: u32, ray_epsilon: f32,
                        max_distance: f32) -> (Vec<f32>, Vec<u32>) {
    assert!(positions.len() % 4 == 0 && (2..=64).contains(&resolution));
    let n = positions.len() / 4;
    let side = resolution as usize + 2;
    let mut depth = vec![0f32; n * side * side * 2];
    let mut stats = vec![0u32; n * LUPIN_PROBE_DEPTH_STATS_WORDS];
    let c = LupinProbeDepthDesc { resolution, subsamples, flags: 0, max_slots: 0, ray_epsilon, max_distance };
    check(unsafe { lupin_hip_bake_probe_depth(device.raw, scene.raw, &c, n as u64, positions.as_ptr(), depth.as_mut_ptr(), stats.as_mut_ptr()) });
    (depth, stats)
}

/// `sample_probe_grid` with a corner's visibility taken from `depth` (`bake_probe_depth` at the grid's probe positions, with the same
/// `resolution` and `max_distance`) instead of the scene's geometry, which is not read.
#[allow(clippy::too_many_arguments)]
pub fn sample_probe_grid_depth(device: &Device, scene: &Scene, origin: [f32; 3], spacing: [f32; 3], dims: [u32; 3], sh: &[f32], depth: &[f32],
                               resolution: u32, max_distance: f32, valid: Option<&[u8]>, records: &[f32], backface: bool, normal_bias: f32) -> Vec<f32> {
    let probes = dims[0] as usize * dims[1] as usize * dims[2] as usize;
    let side = resolution as usize + 2;
    assert!(sh.len() == probes * 36 && depth.len() == probes * side * side * 2 && valid.map_or(true, |v| v.len() == probes));
    assert!(records.len() % LUPIN_PROBE_GRID_RECORD_FLOATS == 0);
    let n = records.len() / LUPIN_PROBE_GRID_RECORD_FLOATS;
    let mut out = vec![0f32; n * LUPIN_PROBE_GRID_RESULT_FLOATS];
    let flags = if backface { LUPIN_PROBE_GRID_BACKFACE } else { 0 };
    let grid = LupinProbeGridDesc { origin, spacing, dims, flags, ray_epsilon: 0.0, normal_bias };
    let c = LupinProbeGridDepthDesc { grid, resolution, max_distance };
    check(unsafe { lupin_hip_sample_probe_grid_depth(device.raw, scene.raw, &c, sh.as_ptr(), depth.as_ptr(), valid.map_or(std::ptr::null(), |v| v.as_ptr()),
                                                     n as u64, records.as_ptr(), out.as_mut_ptr()) });
    out
}

// ---- baked-lighting view (no reference counterpart) ----
/// A camera view of a baked irradiance volume into `target`: per pixel the primary hit through the pixel's centre, then
/// `emission + color / pi * E(p, n)` with `E` from `sample_probe_grid`'s lookup (`depth` = `None`; `visibility` traces the corners'
/// segments) or from `sample_probe_grid_depth`'s (`depth` = the maps, their resolution and their bake's `max_distance`); a miss
/// shows the environment, and where no probe answers `E` is `ambient`.  Every material is drawn as a matte surface of its colour.
/// Returns the G-buffer, width x height x 16 floats (p | instance bits, n | triangle bits, color | w, emission | dst).
#[allow(clippy::too_many_arguments)]
pub fn render_baked(device: &Device, scene: &Scene, target: &Texture, camera_params: LupinCameraParams, camera_transform: LupinMat3x4, origin: [f32; 3],
                    spacing: [f32; 3], dims: [u32; 3], sh: &[f32], depth: Option<(&[f32], u32, f32)>, valid: Option<&[u8]>, ambient: [f32; 3],
                    visibility: bool, backface: bool, ray_epsilon: f32, normal_bias: f32) -> Vec<f32> {
    let probes = dims[0] as usize * dims[1] as usize * dims[2] as usize;
    assert!(sh.len() == probes * 36 && valid.map_or(true, |v| v.len() == probes));
    let (maps, resolution, max_distance) = depth.map_or((std::ptr::null(), 0, 0.0), |(m, r, d)| {
        assert!(m.len() == probes * (r as usize + 2) * (r as usize + 2) * 2);
        (m.as_ptr(), r, d)
    });
    let (width, height) = unsafe { (lupin_hip_texture_width(target.raw) as usize, lupin_hip_texture_height(target.raw) as usize) };
    let mut gbuffer = vec![0f32; width * height * LUPIN_BAKED_VIEW_GBUFFER_FLOATS];
    let flags = (if visibility { LUPIN_PROBE_GRID_VISIBILITY } else { 0 }) | (if backface { LUPIN_PROBE_GRID_BACKFACE } else { 0 });
    let grid = LupinProbeGridDesc { origin, spacing, dims, flags, ray_epsilon, normal_bias };
    let c = LupinBakedViewDesc { camera_params, camera_transform, grid, resolution, max_distance, ray_epsilon, ambient, flags: 0, max_slots: 0 };
    check(unsafe { lupin_hip_render_baked(device.raw, scene.raw, target.raw, &c, sh.as_ptr(), maps, valid.map_or(std::ptr::null(), |v| v.as_ptr()),
                                          gbuffer.as_mut_ptr()) });
    gbuffer
}

// ---- lightmapped view (no reference counterpart) ----
/// `render_baked` with a lightmap as the irradiance source on every instance that has a chart: `charts` are the bake's, `lightmap`
/// is the `lightmap_height` x `lightmap_width` x 4 atlas `bake_lightmap` or `denoise_lightmap` returned.  A hit without a chart takes
/// `ambient`; this thin wrapper passes no volume (call `lupin_hip_render_lightmapped` with `sh` for probes as the fallback).
/// Returns the G-buffer, width x height x 20 floats (`render_baked`'s 16, then atlas x, y, chart bits, source bits).
#[allow(clippy::too_many_arguments)]
pub fn render_lightmapped(device: &Device, scene: &Scene, target: &Texture, camera_params: LupinCameraParams, camera_transform: LupinMat3x4,
                          charts: &[LupinLightmapChart], lightmap: &[f32], lightmap_width: u32, lightmap_height: u32, ambient: [f32; 3],
                          ray_epsilon: f32) -> Vec<f32> {
    assert!(lightmap.len() == lightmap_width as usize * lightmap_height as usize * 4);
    let (width, height) = unsafe { (lupin_hip_texture_width(target.raw) as usize, lupin_hip_texture_height(target.raw) as usize) };
    let mut gbuffer = vec![0f32; width * height * LUPIN_LIGHTMAPPED_VIEW_GBUFFER_FLOATS];
    let grid = LupinProbeGridDesc { origin: [0.0; 3], spacing: [0.0; 3], dims: [0; 3], flags: 0, ray_epsilon: 0.0, normal_bias: 0.0 };
    let view = LupinBakedViewDesc { camera_params, camera_transform, grid, resolution: 0, max_distance: 0.0, ray_epsilon, ambient, flags: 0, max_slots: 0 };
    let c = LupinLightmappedViewDesc { view, lightmap_width, lightmap_height, num_charts: charts.len() as u32, reserved: 0 };
    check(unsafe { lupin_hip_render_lightmapped(device.raw, scene.raw, target.raw, &c, if charts.is_empty() { std::ptr::null() } else { charts.as_ptr() },
                                                lightmap.as_ptr(), std::ptr::null(), std::ptr::null(), std::ptr::null(), gbuffer.as_mut_ptr()) });
    gbuffer
}

/// `lp::stitch_lightmap`: the atlas with its chart borders pulled together, and the call's counts and energies.
pub fn stitch_lightmap(device: &Device, scene: &Scene, desc: &LupinLightmapStitchDesc, charts: &[LupinLightmapChart], rgba: &[f32]) -> (Vec<f32>, LupinLightmapStitchInfo) {
    assert!(rgba.len() == desc.width as usize * desc.height as usize * 4);
    let mut out = vec![0f32; rgba.len()];
    let mut info = LupinLightmapStitchInfo::default();
    check(unsafe { lupin_hip_stitch_lightmap(device.raw, scene.raw, desc, charts.as_ptr(), charts.len() as u32, rgba.as_ptr(), out.as_mut_ptr(), &mut info) });
    (out, info)
}

// ---- directional lightmaps (no reference counterpart) ----
/// `lupin_hip_bake_lightmap`'s texels, records and paths, resolved into four L0 / L1 coefficient planes of the cosine-weighted
/// incident radiance: 4 x `desc.height` x `desc.width` x 4 floats, plane j first, alpha = ownership in every plane.
pub fn bake_lightmap_directional(device: &Device, scene: &Scene, desc: &LupinLightmapDesc, charts: &[LupinLightmapChart]) -> Vec<f32> {
    let texels = desc.width as usize * desc.height as usize;
    let mut planes = vec![0f32; LUPIN_LIGHTMAP_DIRECTIONAL_PLANES * texels * 4];
    check(unsafe { lupin_hip_bake_lightmap_directional(device.raw, scene.raw, desc, charts.as_ptr(), charts.len() as u32, planes.as_mut_ptr(),
                                                       std::ptr::null_mut(), std::ptr::null_mut()) });
    planes
}

/// `render_lightmapped` with `directional`, the planes `bake_lightmap_directional` returned for the same atlas and charts, and
/// `bake_flags`, that bake's flags: a lightmapped pixel's irradiance is scaled by what its shading normal receives against what
/// the bake normal did, so normal maps show.  Returns the G-buffer, width x height x 24 floats (`render_lightmapped`'s 20,
/// then the ratio per channel and the `LUPIN_LIGHTMAPPED_DIRECTIONAL_*` bits).
#[allow(clippy::too_many_arguments)]
pub fn render_lightmapped_directional(device: &Device, scene: &Scene, target: &Texture, camera_params: LupinCameraParams,
                                      camera_transform: LupinMat3x4, charts: &[LupinLightmapChart], lightmap: &[f32], directional: &[f32],
                                      lightmap_width: u32, lightmap_height: u32, bake_flags: u32, ambient: [f32; 3], ray_epsilon: f32) -> Vec<f32> {
    let texels = lightmap_width as usize * lightmap_height as usize;
    assert!(lightmap.len() == texels * 4 && directional.len() == LUPIN_LIGHTMAP_DIRECTIONAL_PLANES * texels * 4);
    let (width, height) = unsafe { (lupin_hip_texture_width(target.raw) as usize, lupin_hip_texture_height(target.raw) as usize) };
    let mut gbuffer = vec![0f32; width * height * LUPIN_LIGHTMAPPED_DIRECTIONAL_GBUFFER_FLOATS];
    let grid = LupinProbeGridDesc { origin: [0.0; 3], spacing: [0.0; 3], dims: [0; 3], flags: 0, ray_epsilon: 0.0, normal_bias: 0.0 };
    let view = LupinBakedViewDesc { camera_params, camera_transform, grid, resolution: 0, max_distance: 0.0, ray_epsilon, ambient, flags: 0, max_slots: 0 };
    let base = LupinLightmappedViewDesc { view, lightmap_width, lightmap_height, num_charts: charts.len() as u32, reserved: 0 };
    let c = LupinLightmappedDirectionalDesc { base, bake_flags, reserved: [0; 3] };
    check(unsafe { lupin_hip_render_lightmapped_directional(device.raw, scene.raw, target.raw, &c,
                                                            if charts.is_empty() { std::ptr::null() } else { charts.as_ptr() }, lightmap.as_ptr(),
                                                            directional.as_ptr(), std::ptr::null(), std::ptr::null(), std::ptr::null(),
                                                            gbuffer.as_mut_ptr()) });
    gbuffer
}
