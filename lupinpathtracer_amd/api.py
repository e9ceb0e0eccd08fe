"""Host-side mirror of the reference's call surface for the hot path (crate `lupin_pt`, `lp::*`).

Same names, argument meaning and error behaviour as lupin/src/renderer.rs, wgpu_utils.rs and
data_structures.rs, on top of the C ABI in include/lupin_hip.h:

    lp::build_pathtrace_resources        renderer.rs:470      -> build_pathtrace_resources
    lp::pathtrace_scene                  renderer.rs:768      -> pathtrace_scene
    lp::PathtraceDesc / AccumulationParams / TileParams / CameraParams / AdvancedParams / PathtraceType
                                         renderer.rs:644-766  -> dataclasses below
    lp::get_num_tiles                    renderer.rs:675      -> get_num_tiles
    lp::DoubleBufferedTexture            wgpu_utils.rs:279    -> DoubleBufferedTexture
    lp::build_denoise_resources / denoise / DenoiseDesc / DenoiseQuality
                                         denoising.rs:83-306  -> build_denoise_resources, denoise (the library's own
                                                                 a-trous filter in HIP, not OIDN: DESIGN.md 9)
    (no reference counterpart)           adaptive sampling   -> AdaptiveParams, build_adaptive_resources,
                                                                 pathtrace_scene_adaptive
    (no reference counterpart)           its reprojection    -> ReprojectDesc, build_reproject_resources,
                                                                 adaptive_reproject
    lp::SceneCPU / validate_scene / build_accel_structures_and_upload
                                         renderer.rs:62-76, data_structures.rs:696-928

Where the reference panics (assert!/panic!), these raise (`LupinError` for ABI errors,
`AssertionError`/`ValueError` for host-side validation).
"""
import ctypes as C
import math
import os
import enum
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import _abi
from ._abi import (ALIAS_BIN_DTYPE, BVH_NODE_DTYPE, ENVIRONMENT_DTYPE, INSTANCE_DTYPE, LIGHT_DTYPE, MATERIAL_DTYPE,
                   MESH_INFO_DTYPE, SENTINEL_IDX, TLAS_NODE_DTYPE, LupinError, check, lib, ptr)

WORKGROUP_SIZE = _abi.WORKGROUP_SIZE


class PathtraceType(enum.IntEnum):  # renderer.rs:711-729
    Standard = 0
    MIS = 1
    Naive = 2
    Direct = 3


class FalsecolorType(enum.IntEnum):  # renderer.rs:843-870
    Albedo = 0
    Normals = 1
    NormalsUnsigned = 2
    FrontFacing = 3
    Emission = 4
    Roughness = 5
    Metallic = 6
    Opacity = 7
    MatType = 8
    IsDelta = 9
    Instance = 10
    Tri = 11


class DebugVizType(enum.IntEnum):  # renderer.rs:950-956
    BVHAABBChecks = 0
    BVHTriChecks = 1
    NumBounces = 2


@dataclass
class DebugVizDesc:  # renderer.rs:958-964
    viz_type: int = DebugVizType.BVHAABBChecks
    heatmap_min: float = 0.0
    heatmap_max: float = 100.0
    first_hit_only: bool = False


@dataclass
class Viewport:  # tonemapping.rs:144-151
    x: float = 0.0
    y: float = 0.0
    w: float = 0.0
    h: float = 0.0


@dataclass
class TonemapDesc:  # tonemapping.rs:106-132
    viewport: Optional[Viewport] = None
    exposure: float = 0.0
    filmic: bool = False
    srgb: bool = True
    clear: bool = True


class MaterialType(enum.IntEnum):  # renderer.rs:126-139
    Matte = 0
    Glossy = 1
    Reflective = 2
    Transparent = 3
    Refractive = 4
    Subsurface = 5
    Volumetric = 6
    GltfPbr = 7


@dataclass
class BakedPathtraceParams:  # renderer.rs:451-468
    with_runtime_checks: bool = False
    max_bounces: int = 8
    samples_per_pixel: int = 5


@dataclass
class CameraParams:  # renderer.rs:683-708
    is_orthographic: bool = False
    lens: float = 0.050
    film: float = 0.036
    aspect: float = 1.500
    focus: float = 10000.0
    aperture: float = 0.0


@dataclass
class AdvancedParams:  # renderer.rs:731-749
    max_radiance: float = 100.0
    rng_seed: int = 0
    ray_epsilon: float = 0.001


@dataclass
class TileParams:  # renderer.rs:651-670
    tile_size: int = 100
    tile_idx: int = 0


@dataclass
class AccumulationParams:  # renderer.rs:644-649
    prev_frame: "Texture"
    accum_counter: int


def identity_mat3x4():
    """Mat3x4::IDENTITY (base.rs:651-660): 4 columns x 3 rows."""
    return np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], dtype=np.float32)


@dataclass
class PathtraceDesc:  # renderer.rs:751-766
    accum_params: Optional[AccumulationParams] = None
    tile_params: Optional[TileParams] = None
    camera_params: CameraParams = field(default_factory=CameraParams)
    camera_transform: np.ndarray = field(default_factory=identity_mat3x4)
    force_software_bvh: bool = False
    advanced: AdvancedParams = field(default_factory=AdvancedParams)


def get_num_tiles(tile_size, width, height):
    """renderer.rs:675-681"""
    return int(lib().lupin_hip_get_num_tiles(tile_size, width, height))


# ------------------------------------------------------------------------------------------------
# Device objects
# ------------------------------------------------------------------------------------------------

class Context:
    """One HIP device + stream (the reference's wgpu Device/Queue pair)."""

    def __init__(self, device_ordinal=0):
        h = C.c_void_p()
        check(lib().lupin_hip_create_context(device_ordinal, C.byref(h)))
        self.handle = h
        self.device_ordinal = device_ordinal

    def sync(self):
        check(lib().lupin_hip_sync(self.handle))

    def set_f16_store_rounding(self, mode):
        """0 = toward zero (what the reference's goldens show; default), 1 = nearest even."""
        check(lib().lupin_hip_set_f16_store_rounding(self.handle, int(mode)))

    def stats_reset(self, mode=0):
        """mode: 0 / False plain counters, 1 / True per-kernel hipEvent timing, 2 work counters of the tracing kernels."""
        check(lib().lupin_hip_stats_reset(self.handle, int(mode)))

    def stats(self):
        s = _abi.StatsC()
        check(lib().lupin_hip_stats_get(self.handle, C.byref(s)))
        def conv(v):
            return [conv(x) for x in v] if hasattr(v, "__len__") else v
        return {k: conv(getattr(s, k)) for k, _ in _abi.StatsC._fields_}

    def reserve_path_state(self, pixels, max_bounces, samples_per_pixel):
        """Allocate the path state of every frame in flight now instead of at each lane's first pathtrace call."""
        check(lib().lupin_hip_reserve_path_state(self.handle, int(pixels), int(max_bounces), int(samples_per_pixel)))

    def set_batch_frames(self, frames):
        """Frames per wavefront: how many consecutive, chained pathtrace_scene calls run as one wavefront (1..16;
        0 = by dispatch size, the default: 16 up to 4 M pixels, 8 above)."""
        check(lib().lupin_hip_set_batch_frames(self.handle, int(frames)))

    def set_traversal(self, mode):
        """"binary" (default: the reference's visiting order) or "wide" (four-wide hierarchy + exactness certificate + re-trace)."""
        check(lib().lupin_hip_set_traversal(self.handle, {"binary": 0, "wide": 1}[mode]))

    def set_accumulation_mode(self, mode):
        """0 = f16 running average (reference-faithful, default), 1 = f32 accumulator per texture (pathtracer.wgsl:275-289)."""
        check(lib().lupin_hip_set_accumulation_mode(self.handle, int(mode)))

    def measure_copy_bandwidth(self, nbytes=1 << 30, reps=10):
        """GB/s (read + written) of a device-to-device copy: the measured HBM peak."""
        out = C.c_double()
        check(lib().lupin_hip_measure_copy_bandwidth(self.handle, nbytes, reps, C.byref(out)))
        return float(out.value)

    def close(self):
        if self.handle:
            lib().lupin_hip_destroy_context(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count():
    return int(lib().lupin_hip_device_count())


def runtime_info():
    """HIP version the library was built against / runs on, and every libamdhip64 mapped into the process."""
    r = _abi.RuntimeInfoC()
    check(lib().lupin_hip_runtime_info(C.byref(r)))
    paths = r.hip_runtime_paths.decode("utf-8", "replace")
    return {"build_hip_version": int(r.build_hip_version), "runtime_hip_version": int(r.runtime_hip_version),
            "num_hip_runtimes_mapped": int(r.num_hip_runtimes_mapped), "hip_runtime_paths": [p for p in paths.split(";") if p]}


class PathtraceResources:
    def __init__(self, ctx, params):
        self.ctx = ctx
        self.params = params
        h = C.c_void_p()
        c = _abi.BakedPathtraceParamsC(1 if params.with_runtime_checks else 0, params.max_bounces, params.samples_per_pixel)
        check(lib().lupin_hip_build_pathtrace_resources(ctx.handle, C.byref(c), C.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if self.handle and self.ctx.handle:   # a closed context has already released the device
                lib().lupin_hip_destroy_pathtrace_resources(self.handle)
            self.handle = None
        except Exception:
            pass


def build_pathtrace_resources(ctx, baked_pathtrace_params):
    """lp::build_pathtrace_resources (renderer.rs:470): max_bounces / samples_per_pixel are baked."""
    return PathtraceResources(ctx, baked_pathtrace_params)


class Texture:
    """An Rgba16Float render target (row 0 = top)."""

    def __init__(self, ctx, width, height, _handle=None):
        self.ctx = ctx
        self._owned = _handle is None
        if _handle is None:
            h = C.c_void_p()
            check(lib().lupin_hip_texture_create(ctx.handle, width, height, C.byref(h)))
            _handle = h
        self.handle = _handle
        self.width = int(lib().lupin_hip_texture_width(self.handle))
        self.height = int(lib().lupin_hip_texture_height(self.handle))

    def format(self):
        return "Rgba16Float"

    def device_ptr(self):
        return int(lib().lupin_hip_texture_device_ptr(self.handle) or 0)

    def upload(self, rgba16f):
        a = np.ascontiguousarray(rgba16f, dtype=np.float16).reshape(self.height, self.width, 4)
        check(lib().lupin_hip_texture_upload_rgba16f(self.handle, ptr(a)))

    def download(self):
        """(H, W, 4) float16; synchronises (loader.rs download_texture)."""
        out = np.empty((self.height, self.width, 4), dtype=np.float16)
        check(lib().lupin_hip_texture_download_rgba16f(self.handle, ptr(out)))
        return out

    def download_f32(self):
        """(H, W, 4) float32 of the f32 accumulator (frames rendered with Context.set_accumulation_mode(1))."""
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        check(lib().lupin_hip_texture_download_rgba32f(self.handle, ptr(out)))
        return out

    def __del__(self):
        try:
            if self._owned and self.handle and self.ctx.handle:
                lib().lupin_hip_texture_destroy(self.handle)
            self.handle = None
        except Exception:
            pass


class DoubleBufferedTexture:
    """lp::DoubleBufferedTexture (wgpu_utils.rs:279-348)."""

    def __init__(self, ctx, width, height):
        self.ctx = ctx
        h = C.c_void_p()
        check(lib().lupin_hip_dbuf_create(ctx.handle, width, height, C.byref(h)))
        self.handle = h

    @classmethod
    def create(cls, ctx, width, height):
        return cls(ctx, width, height)

    def front(self):
        return Texture(self.ctx, 0, 0, _handle=C.c_void_p(lib().lupin_hip_dbuf_front(self.handle)))

    def back(self):
        return Texture(self.ctx, 0, 0, _handle=C.c_void_p(lib().lupin_hip_dbuf_back(self.handle)))

    def copy_front_to_back(self):
        check(lib().lupin_hip_dbuf_copy_front_to_back(self.handle))

    def flip(self):
        lib().lupin_hip_dbuf_flip(self.handle)

    def resize(self, width, height):
        check(lib().lupin_hip_dbuf_resize(self.handle, width, height))

    def __del__(self):
        try:
            if self.handle and self.ctx.handle:
                lib().lupin_hip_dbuf_destroy(self.handle)
            self.handle = None
        except Exception:
            pass


# ------------------------------------------------------------------------------------------------
# Scene: CPU description, preprocessing, upload
# ------------------------------------------------------------------------------------------------

@dataclass
class TextureCPU:
    """One texture as the loader hands it over: Rgba8Unorm (H,W,4 uint8) or Rgba16Float (H,W,4 float16)."""
    pixels: np.ndarray

    @property
    def format(self):
        return _abi.TEX_RGBA8_UNORM if self.pixels.dtype == np.uint8 else _abi.TEX_RGBA16_FLOAT


@dataclass
class EnvMapInfo:  # data_structures.rs:13-19: f32 texels used for the env alias table
    data: np.ndarray   # (H, W, 4) float32
    width: int
    height: int


@dataclass
class SceneCPU:  # renderer.rs:62-76
    mesh_infos: np.ndarray = field(default_factory=lambda: np.zeros(0, MESH_INFO_DTYPE))
    verts_pos_array: List[np.ndarray] = field(default_factory=list)        # (n,4) f32
    verts_normal_array: List[np.ndarray] = field(default_factory=list)     # (n,4) f32
    verts_texcoord_array: List[np.ndarray] = field(default_factory=list)   # (n,2) f32
    verts_color_array: List[np.ndarray] = field(default_factory=list)      # (n,4) f32
    indices_array: List[np.ndarray] = field(default_factory=list)          # (3t,) u32
    instances: np.ndarray = field(default_factory=lambda: np.zeros(0, INSTANCE_DTYPE))
    materials: np.ndarray = field(default_factory=lambda: np.zeros(0, MATERIAL_DTYPE))
    environments: np.ndarray = field(default_factory=lambda: np.zeros(0, ENVIRONMENT_DTYPE))


def default_material():
    """Material::default() (renderer.rs:163-185)."""
    m = np.zeros((), MATERIAL_DTYPE)
    m["color"] = (0.0, 0.0, 0.0, 1.0)
    m["ior"] = 1.5
    m["tr_depth"] = 0.01
    for k in ("color_tex_idx", "emission_tex_idx", "roughness_tex_idx", "scattering_tex_idx", "normal_tex_idx"):
        m[k] = SENTINEL_IDX
    return m


def default_mesh_info():
    return np.array((SENTINEL_IDX, SENTINEL_IDX, SENTINEL_IDX), MESH_INFO_DTYPE)


def default_instance():
    """Instance::default(): identity world->local, mesh 0, material 0."""
    i = np.zeros((), INSTANCE_DTYPE)
    i["transpose_inverse_transform"] = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], np.float32)
    return i


def default_environment():
    e = np.zeros((), ENVIRONMENT_DTYPE)
    e["emission_tex_idx"] = SENTINEL_IDX
    e["transform"] = np.eye(4, dtype=np.float32)
    return e


def mat3x4_inverse(m):
    """Mat3x4::inverse (base.rs:708-722); m is (4,3) column-major."""
    a = _abi.Mat3x4()
    b = _abi.Mat3x4()
    m = np.asarray(m, np.float32)
    for c in range(4):
        for r in range(3):
            a.m[c][r] = float(m[c][r])
    lib().lupin_mat3x4_inverse(C.byref(a), C.byref(b))
    return np.array([[b.m[c][r] for r in range(3)] for c in range(4)], np.float32)


def instance_from_transform(local_to_world, mesh_idx, mat_idx):
    """Instance whose transpose_inverse_transform is transpose(inverse(local_to_world)) (loader.rs:653-654)."""
    inv = mat3x4_inverse(local_to_world)      # (4 cols, 3 rows)
    inst = default_instance()
    inst["transpose_inverse_transform"] = inv.T.copy()   # Mat3x4::transpose -> 3 x 4
    inst["mesh_idx"] = mesh_idx
    inst["mat_idx"] = mat_idx
    return inst


def validate_scene(scene: SceneCPU, num_textures: int, num_samplers: int):
    """lp::validate_scene (data_structures.rs:876-928)."""
    assert len(scene.verts_pos_array) == len(scene.mesh_infos)
    assert num_textures == num_samplers
    for i, info in enumerate(scene.mesh_infos):
        for key, arr in (("normals_buf_idx", scene.verts_normal_array), ("texcoords_buf_idx", scene.verts_texcoord_array),
                         ("colors_buf_idx", scene.verts_color_array)):
            idx = int(info[key])
            if idx != SENTINEL_IDX:
                assert idx < len(arr)
                assert len(arr[idx]) == len(scene.verts_pos_array[i])
    for i, indices in enumerate(scene.indices_array):
        if len(indices):
            assert int(indices.max()) < len(scene.verts_pos_array[i])
    for inst in scene.instances:
        assert int(inst["mesh_idx"]) < len(scene.mesh_infos)
        assert int(inst["mat_idx"]) < len(scene.materials)
    for mat in scene.materials:
        for k in ("color_tex_idx", "emission_tex_idx", "roughness_tex_idx", "scattering_tex_idx", "normal_tex_idx"):
            assert int(mat[k]) < num_textures or int(mat[k]) == SENTINEL_IDX
    for env in scene.environments:
        assert (env["emission"] >= 0).all()
        assert int(env["emission_tex_idx"]) < num_textures or int(env["emission_tex_idx"]) == SENTINEL_IDX


def build_bvh(verts_pos, indices):
    """lp::build_bvh (data_structures.rs:196-235): returns (nodes, reordered indices)."""
    verts = np.ascontiguousarray(verts_pos, np.float32).reshape(-1, 4)
    idx = np.ascontiguousarray(indices, np.uint32).copy()
    count = lib().lupin_build_bvh(ptr(verts), len(verts), ptr(idx), len(idx), None, 0)
    if count < 0:
        raise ValueError("build_bvh: invalid input")
    nodes = np.zeros(count, BVH_NODE_DTYPE)
    n2 = lib().lupin_build_bvh(ptr(verts), len(verts), ptr(idx), len(idx), ptr(nodes), count)
    assert n2 == count
    return nodes, idx


def build_bvh_device(ctx, verts_pos, indices):
    """Device BLAS builder (csrc/lbvh.hip): Morton-sorted complete binary tree in the reference's BvhNode format.
    Returns (nodes, reordered indices) like build_bvh; needs a GPU context."""
    verts = np.ascontiguousarray(verts_pos, np.float32).reshape(-1, 4)
    idx = np.ascontiguousarray(indices, np.uint32).copy()
    count = int(lib().lupin_hip_lbvh_node_count(len(idx) // 3))
    nodes = np.zeros(count, BVH_NODE_DTYPE)
    n2 = lib().lupin_hip_build_bvh_device(ctx.handle, ptr(verts), len(verts), ptr(idx), len(idx), ptr(nodes), count)
    if n2 < 0:
        check(int(n2))
    assert n2 == count
    return nodes, idx


def build_bvh_sah_device(ctx, verts_pos, indices):
    """lp::build_bvh (data_structures.rs:196-235) run on the device (csrc/sahbvh.hip): the same tree as build_bvh -- same
    boxes, split planes and triangle set per node -- numbered level by level.  Returns (nodes, reordered indices)."""
    verts = np.ascontiguousarray(verts_pos, np.float32).reshape(-1, 4)
    idx = np.ascontiguousarray(indices, np.uint32).copy()
    cap = max(2 * (len(idx) // 3) - 1, 1)
    nodes = np.zeros(cap, BVH_NODE_DTYPE)
    n = lib().lupin_hip_build_bvh_sah_device(ctx.handle, ptr(verts), len(verts), ptr(idx), len(idx), ptr(nodes), cap)
    if n < 0:
        check(int(n))
    return nodes[:n].copy(), idx


def build_tlas(instances, model_aabbs):
    """lp::build_tlas (data_structures.rs:545-641). model_aabbs: (num_meshes, 6)."""
    inst = np.ascontiguousarray(instances)
    ab = np.ascontiguousarray(model_aabbs, np.float32).reshape(-1, 6)
    if len(inst) == 0 or len(ab) == 0:
        return np.zeros(0, TLAS_NODE_DTYPE)
    out = np.zeros(2 * len(inst), TLAS_NODE_DTYPE)
    n = lib().lupin_build_tlas(ptr(inst), len(inst), ptr(ab), len(ab), ptr(out))
    if n < 0:
        raise ValueError("build_tlas: invalid input")
    return out[:n]


# Scene.update_instances builds the TLAS on the device from this many instances.  Measured (DESIGN.md 11,
# profiles/scene_update_bench.jsonl): lupin_build_tlas wins at 501 and 2 101 instances, the device builder at 8 101.
UPDATE_DEVICE_MIN_INSTANCES = 4000


def build_tlas_device(ctx, instances, model_aabbs):
    """build_tlas on the device (csrc/tlas.hip): the same tree as build_tlas, node for node.  Needs a GPU context."""
    if ctx is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "the device TLAS builder needs a GPU context")
    inst = np.ascontiguousarray(instances)
    ab = np.ascontiguousarray(model_aabbs, np.float32).reshape(-1, 6)
    if len(inst) == 0 or len(ab) == 0:
        return np.zeros(0, TLAS_NODE_DTYPE)
    out = np.zeros(2 * len(inst), TLAS_NODE_DTYPE)
    n = lib().lupin_hip_build_tlas_device(ctx.handle, ptr(inst), len(inst), ptr(ab), len(ab), ptr(out))
    if n < 0:
        check(int(n))
    return out[:n]


def tlas_build_stats():
    """The calling thread's latest build_tlas_device: instances, best-match scans, where the state lived, kernel time."""
    s = _abi.TlasBuildStatsC()
    lib().lupin_hip_tlas_build_stats(C.byref(s))
    return {"num_instances": int(s.num_instances), "state_in_lds": bool(s.state_in_lds), "scans": int(s.scans), "kernel_ms": float(s.kernel_ms)}


def build_alias_table(weights):
    """lp::build_alias_table (data_structures.rs:116-193)."""
    w = np.ascontiguousarray(weights, np.float32)
    out = np.zeros(len(w), ALIAS_BIN_DTYPE)
    n = lib().lupin_build_alias_table(ptr(w), len(w), ptr(out))
    if n < 0:
        raise ValueError("build_alias_table: invalid input")
    return out[:n]


def build_lights(scene: SceneCPU, envs_info: List[EnvMapInfo]):
    """lp::build_lights (data_structures.rs:20-113): alias tables use the ORIGINAL triangle order."""
    assert len(scene.environments) == len(envs_info), "Mismatching sizes for environment data!"
    lights, alias_tables, env_alias_tables = [], [], []
    for i, inst in enumerate(scene.instances):
        mat = scene.materials[int(inst["mat_idx"])]
        verts = scene.verts_pos_array[int(inst["mesh_idx"])]
        idx = scene.indices_array[int(inst["mesh_idx"])]
        if not np.any(mat["emission"] != 0.0):
            continue
        if len(idx) == 0:
            continue
        verts = np.ascontiguousarray(verts, np.float32)
        idx = np.ascontiguousarray(idx, np.uint32)
        weights = np.zeros(len(idx) // 3, np.float32)
        total = float(lib().lupin_mesh_light_weights(ptr(verts), ptr(idx), len(idx), ptr(weights)))
        if total <= 0.0:
            continue
        table = build_alias_table(weights)
        assert len(table) > 0
        lights.append((i, total))
        alias_tables.append(table)
    for i, env in enumerate(scene.environments):
        info = envs_info[i]
        tex = np.ascontiguousarray(info.data, np.float32).reshape(info.height, info.width, 4)
        if os.environ.get("LUPIN_EXPERIMENT_ENV_F16_WEIGHTS") == "1":   # tools/env_residual.py: weights from the f16 texels the shader samples
            tex = np.ascontiguousarray(tex.astype(np.float16).astype(np.float32))
        scale = np.ascontiguousarray(env["emission"], np.float32)
        weights = np.zeros(info.width * info.height, np.float32)
        lib().lupin_env_light_weights(ptr(tex), info.width, info.height, ptr(scale), ptr(weights))
        table = build_alias_table(weights)
        assert len(table) > 0
        env_alias_tables.append(table)
    return np.array(lights, LIGHT_DTYPE), alias_tables, env_alias_tables


class Scene:
    """lp::Scene in its software-BVH configuration (renderer.rs:17-60): the prepared host arrays, the
    C descriptor that views them, and (when a context is given) the uploaded device scene."""

    def __init__(self):
        self.desc = None
        self.handle = None
        self.ctx = None
        self._keep = []
        self.envs_empty = True
        self.lights_empty = True
        self.instances_empty = True
        self.stats = {}
        self.instances = None      # the instance records and per-mesh model boxes the TLAS was built from
        self.model_aabbs = None

    def update_instances(self, transforms, tlas_builder=None):
        """Move the scene's instances in place (lupin_hip_scene_update_instances): new transforms, a rebuilt TLAS, nothing
        else re-uploaded.  transforms: (n, 3, 4) transpose_inverse_transform matrices (the rows of world -> local), or
        instance records whose mesh_idx / mat_idx equal the scene's.  tlas_builder: "cpu" | "device"; None picks by
        instance count (the CPU builder below UPDATE_DEVICE_MIN_INSTANCES instances).
        Calls recorded before the update render the old transforms.  On an error the scene is unchanged.
        Also refreshes desc.instances, desc.tlas_nodes and .tlas, so the oracle can run on the same object."""
        if self.handle is None:
            raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "scene was built without a device context; there is no CPU fallback")
        if tlas_builder is None:
            tlas_builder = "device" if len(self.instances) >= UPDATE_DEVICE_MIN_INSTANCES else "cpu"
        if tlas_builder not in ("cpu", "device"):
            raise ValueError("tlas_builder must be 'cpu' or 'device'")
        t = np.asarray(transforms)
        if t.dtype == INSTANCE_DTYPE:
            if len(t) == len(self.instances) and not (np.array_equal(t["mesh_idx"], self.instances["mesh_idx"]) and
                                                      np.array_equal(t["mat_idx"], self.instances["mat_idx"])):
                raise ValueError("update_instances changes transforms only: mesh_idx and mat_idx must stay as they are")
            t = t["transpose_inverse_transform"]
        t = np.ascontiguousarray(t, np.float32).reshape(-1, 3, 4)
        check(lib().lupin_hip_scene_update_instances(self.handle, ptr(t), len(t), 1 if tlas_builder == "device" else 0))
        instances = self.instances.copy()
        instances["transpose_inverse_transform"] = t
        tlas = np.zeros(2 * len(instances), TLAS_NODE_DTYPE)
        n = lib().lupin_hip_scene_get_tlas(self.handle, ptr(tlas), len(tlas))
        if n < 0:
            check(int(n))
        tlas = tlas[:n].copy()
        self._keep += [instances, tlas]
        self.instances, self.tlas = instances, tlas
        self.desc.instances = ptr(instances)
        self.desc.tlas_nodes = ptr(tlas) if len(tlas) else None
        self.desc.num_tlas_nodes = len(tlas)

    def mesh_triangle_count(self, mesh_idx):
        """Triangles of mesh `mesh_idx`, from the descriptor the scene was created with."""
        if not 0 <= int(mesh_idx) < int(self.desc.num_meshes):
            raise LupinError(_abi_code("LUPIN_ERR_INVALID_ARGUMENT"), "mesh index out of range")
        return int(self.desc.meshes[int(mesh_idx)].num_indices) // 3

    def set_lightmap_uvs(self, mesh_idx, uvs):
        """Give mesh `mesh_idx` a lightmap UV set (lupin_hip_scene_set_lightmap_uvs): `uvs` holds one UV per
        triangle corner, (3 * triangles, 2) or (triangles, 3, 2) float32, in the scene's own triangle order; None removes
        the set.  Every lightmap bake and the lightmapped views then place the instances of this mesh by the set instead of
        its material texcoords; materials keep reading the texcoords.  Calls recorded before run first.  On an error the
        scene keeps the set it had."""
        if self.handle is None:
            raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "scene was built without a device context; there is no CPU fallback")
        if uvs is None:
            check(lib().lupin_hip_scene_set_lightmap_uvs(self.handle, int(mesh_idx), None, 0))
            return
        a = np.ascontiguousarray(uvs, np.float32)
        if a.size % 2:
            raise ValueError("uvs must hold float pairs")
        check(lib().lupin_hip_scene_set_lightmap_uvs(self.handle, int(mesh_idx), ptr(a), a.size // 2))

    def unwrap_lightmap_uvs(self, mesh_idx, texel_size, padding=2, attach=True, want_charts=False):
        """Generate a lightmap UV set for mesh `mesh_idx` on the device (lupin_hip_unwrap_lightmap_uvs) and, with `attach`,
        give it to the mesh (set_lightmap_uvs).  texel_size: local units per texel; padding: texels around every chart.
        Returns (uvs, info) or (uvs, chart_of_tri, info): uvs (triangles, 3, 2) float32 in texels of the mesh's own atlas of
        info["width"] x info["height"] texels; chart_of_tri uint32 (UNWRAP_NO_CHART for a degenerate triangle)."""
        if self.handle is None or self.ctx is None:
            raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "scene was built without a device context; there is no CPU fallback")
        tris = int(lib().lupin_hip_scene_mesh_triangle_count(self.handle, int(mesh_idx)))      # the scene's own count sizes the outputs
        if tris < 0:
            check(tris)
        uvs = np.zeros((tris, 3, 2), np.float32)
        chart = np.zeros(tris, np.uint32)
        d = _abi.UnwrapDescC(float(texel_size), int(padding), 0)
        info = _abi.UnwrapInfoC()
        check(lib().lupin_hip_unwrap_lightmap_uvs(self.ctx.handle, self.handle, int(mesh_idx), C.byref(d), ptr(uvs), ptr(chart), C.byref(info)))
        if attach:
            self.set_lightmap_uvs(mesh_idx, uvs)
        out = {k: (float if k.endswith("_ms") else int)(getattr(info, k)) for k, _ in _abi.UnwrapInfoC._fields_}
        return (uvs, chart, out) if want_charts else (uvs, out)

    def __del__(self):
        try:
            if self.handle and self.ctx is not None and self.ctx.handle:
                lib().lupin_hip_scene_destroy(self.handle)
            self.handle = None
        except Exception:
            pass


def _array_of(struct, items):
    arr = (struct * max(1, len(items)))()
    for i, it in enumerate(items):
        arr[i] = it
    return arr


def build_accel_structures_and_upload(ctx, scene: SceneCPU, textures: List[TextureCPU], envs_info: List[EnvMapInfo],
                                      build_sw_and_hw: bool = True, blas_builder: str = "sah", tlas_builder: str = "cpu") -> Scene:
    """lp::build_accel_structures_and_upload (data_structures.rs:696-872), software-BVH pipeline.

    ctx may be None: the host-side preprocessing still runs and `Scene.desc` is usable (CPU-only
    tests feed it to the oracle); nothing is uploaded then.
    blas_builder: "sah" = the reference's CPU builder (lupin_build_bvh), "sah_device" = the same tree built on the GPU
    (build_bvh_sah_device; meshes with at least 64 triangles), "lbvh" = the Morton-order device builder
    (build_bvh_device; meshes with at least 64 triangles, smaller ones keep the SAH builder); a callable
    (verts (N,4), indices) -> (nodes, reordered indices) plugs in any other builder that emits the reference's node format.
    tlas_builder: "cpu" = lupin_build_tlas, "device" = the same tree built on the GPU (build_tlas_device).
    """
    if tlas_builder not in ("cpu", "device"):
        raise ValueError("tlas_builder must be 'cpu' or 'device'")
    if tlas_builder == "device" and ctx is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "the device TLAS builder needs a GPU context")
    if not callable(blas_builder) and blas_builder not in ("sah", "sah_device", "lbvh"):
        raise ValueError("blas_builder must be 'sah', 'sah_device', 'lbvh' or a callable (verts, indices) -> (nodes, reordered indices)")
    if blas_builder in ("lbvh", "sah_device") and ctx is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "the device BLAS builder needs a GPU context")
    out = Scene()
    keep = out._keep

    lights, alias_tables, env_alias_tables = build_lights(scene, envs_info)

    # per mesh: BLAS over a CLONE of the indices; the reordered clone is what the path reads (:724-730)
    mesh_descs, model_aabbs = [], []
    total_tris = 0
    for verts, indices in zip(scene.verts_pos_array, scene.indices_array):
        v = np.ascontiguousarray(verts, np.float32).reshape(-1, 4)
        if callable(blas_builder):
            nodes, reordered = blas_builder(v, indices)
            nodes, reordered = np.ascontiguousarray(nodes, BVH_NODE_DTYPE), np.ascontiguousarray(reordered, np.uint32)
        elif blas_builder == "lbvh" and len(indices) >= 3 * 64:
            nodes, reordered = build_bvh_device(ctx, v, indices)
        elif blas_builder == "sah_device" and len(indices) >= 3 * 64:
            nodes, reordered = build_bvh_sah_device(ctx, v, indices)
        else:
            nodes, reordered = build_bvh(v, indices)
        keep += [v, nodes, reordered]
        mesh_descs.append(_abi.MeshDesc(ptr(v), len(v), ptr(reordered), len(reordered), ptr(nodes), len(nodes)))
        total_tris += len(reordered) // 3
        if len(v):
            model_aabbs.append(np.concatenate([v[:, :3].min(axis=0), v[:, :3].max(axis=0)]))
        else:   # Aabb::neutral()
            fm = np.finfo(np.float32).max
            model_aabbs.append(np.array([fm, fm, fm, -fm, -fm, -fm], np.float32))
    model_aabbs = np.array(model_aabbs, np.float32).reshape(-1, 6)
    instances = np.ascontiguousarray(scene.instances)
    tlas = build_tlas_device(ctx, instances, model_aabbs) if tlas_builder == "device" else build_tlas(instances, model_aabbs)

    def vbufs(arrs, comps):
        descs = []
        for a in arrs:
            a = np.ascontiguousarray(a, np.float32).reshape(-1, comps)
            keep.append(a)
            descs.append(_abi.VertexBufferDesc(ptr(a), len(a)))
        return descs

    normal_descs = vbufs(scene.verts_normal_array, 4)
    uv_descs = vbufs(scene.verts_texcoord_array, 2)
    color_descs = vbufs(scene.verts_color_array, 4)

    tex_descs = []
    for t in textures:
        px = np.ascontiguousarray(t.pixels)
        assert px.ndim == 3 and px.shape[2] == 4 and px.dtype in (np.uint8, np.float16)
        keep.append(px)
        tex_descs.append(_abi.TextureDesc(px.shape[1], px.shape[0], t.format, ptr(px)))

    alias_descs = [_abi.AliasTableDesc(ptr(t), len(t)) for t in alias_tables]
    env_alias_descs = [_abi.AliasTableDesc(ptr(t), len(t)) for t in env_alias_tables]
    keep += alias_tables + env_alias_tables

    mesh_infos = np.ascontiguousarray(scene.mesh_infos)
    materials = np.ascontiguousarray(scene.materials)
    environments = np.ascontiguousarray(scene.environments)
    keep += [mesh_infos, materials, environments, instances, tlas, lights]

    c_meshes = _array_of(_abi.MeshDesc, mesh_descs)
    c_normals = _array_of(_abi.VertexBufferDesc, normal_descs)
    c_uvs = _array_of(_abi.VertexBufferDesc, uv_descs)
    c_colors = _array_of(_abi.VertexBufferDesc, color_descs)
    c_tex = _array_of(_abi.TextureDesc, tex_descs)
    c_alias = _array_of(_abi.AliasTableDesc, alias_descs)
    c_env_alias = _array_of(_abi.AliasTableDesc, env_alias_descs)
    keep += [c_meshes, c_normals, c_uvs, c_colors, c_tex, c_alias, c_env_alias]

    d = _abi.SceneDesc()
    d.mesh_infos = ptr(mesh_infos) if len(mesh_infos) else None
    d.meshes = c_meshes
    d.num_meshes = len(mesh_descs)
    d.verts_normal_array = c_normals
    d.num_normal_buffers = len(normal_descs)
    d.verts_texcoord_array = c_uvs
    d.num_texcoord_buffers = len(uv_descs)
    d.verts_color_array = c_colors
    d.num_color_buffers = len(color_descs)
    d.instances = ptr(instances) if len(instances) else None
    d.num_instances = len(instances)
    d.materials = ptr(materials) if len(materials) else None
    d.num_materials = len(materials)
    d.textures = c_tex
    d.num_textures = len(tex_descs)
    d.environments = ptr(environments) if len(environments) else None
    d.num_environments = len(environments)
    d.tlas_nodes = ptr(tlas) if len(tlas) else None
    d.num_tlas_nodes = len(tlas)
    d.lights = ptr(lights) if len(lights) else None
    d.num_lights = len(lights)
    d.alias_tables = c_alias
    d.env_alias_tables = c_env_alias
    out.desc = d
    out.envs_empty = len(envs_info) == 0
    out.lights_empty = len(lights) == 0
    out.instances_empty = len(instances) == 0
    out.tlas = tlas
    out.instances = instances
    out.model_aabbs = model_aabbs
    out.lights = lights
    out.alias_tables = alias_tables
    out.env_alias_tables = env_alias_tables
    out.stats = {"total_tri_count": total_tris, "instances": len(instances), "materials": len(materials),
                 "lights": len(lights), "textures": len(tex_descs)}   # get_scene_stats (data_structures.rs:940-953)

    if ctx is not None:
        h = C.c_void_p()
        check(lib().lupin_hip_scene_create(ctx.handle, C.byref(d), C.byref(h)))
        out.handle = h
        out.ctx = ctx
    return out


def scene_flags(scene: Scene, camera_params: CameraParams):
    """The flag word get_push_constants sets (renderer.rs:1457-1471)."""
    f = 0
    if camera_params.is_orthographic:
        f |= _abi.FLAG_CAMERA_ORTHO
    if scene.envs_empty:
        f |= _abi.FLAG_ENVS_EMPTY
    if scene.lights_empty:
        f |= _abi.FLAG_LIGHTS_EMPTY
    if scene.instances_empty:
        f |= _abi.FLAG_INSTANCES_EMPTY
    return f


def _desc_to_c(desc: PathtraceDesc, keep):
    c = _abi.PathtraceDescC()
    if desc.accum_params is not None:
        ap = _abi.AccumulationParamsC(desc.accum_params.prev_frame.handle, desc.accum_params.accum_counter)
        keep.append(ap)
        c.accum_params = C.pointer(ap)
    if desc.tile_params is not None:
        tp = _abi.TileParamsC(desc.tile_params.tile_size, desc.tile_params.tile_idx)
        keep.append(tp)
        c.tile_params = C.pointer(tp)
    cp = desc.camera_params
    c.camera_params = _abi.CameraParamsC(1 if cp.is_orthographic else 0, cp.lens, cp.film, cp.aspect, cp.focus, cp.aperture)
    m = np.asarray(desc.camera_transform, np.float32).reshape(4, 3)
    for col in range(4):
        for row in range(3):
            c.camera_transform.m[col][row] = float(m[col][row])
    c.force_software_bvh = 1 if desc.force_software_bvh else 0
    c.advanced = _abi.AdvancedParamsC(desc.advanced.max_radiance, desc.advanced.rng_seed, desc.advanced.ray_epsilon)
    return c


def pathtrace_scene(ctx, resources, scene, render_target, pathtrace_type, desc):
    """lp::pathtrace_scene (renderer.rs:768-842): enqueue one accumulation frame (or one tile of it)."""
    assert render_target.format() == "Rgba16Float"
    if scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "scene was built without a device context; there is no CPU fallback")
    keep = []
    c = _desc_to_c(desc, keep)
    check(lib().lupin_hip_pathtrace_scene(ctx.handle, resources.handle, scene.handle, render_target.handle,
                                          int(pathtrace_type), C.byref(c)))


def pathtrace_scene_falsecolor(ctx, resources, scene, render_target, falsecolor_type, desc):
    """lp::pathtrace_scene_falsecolor (renderer.rs:872-948)."""
    assert render_target.format() == "Rgba16Float"
    if scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "scene was built without a device context; there is no CPU fallback")
    keep = []
    c = _desc_to_c(desc, keep)
    check(lib().lupin_hip_pathtrace_scene_falsecolor(ctx.handle, resources.handle, scene.handle, render_target.handle,
                                                     int(falsecolor_type), C.byref(c)))


def pathtrace_scene_debug(ctx, resources, scene, render_target, debug_desc, desc):
    """lp::pathtrace_scene_debug (renderer.rs:966-1041): BVH-cost / bounce-count heat maps."""
    assert render_target.format() == "Rgba16Float"
    if scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "scene was built without a device context; there is no CPU fallback")
    keep = []
    c = _desc_to_c(desc, keep)
    dd = _abi.DebugVizDescC(int(debug_desc.viz_type), float(debug_desc.heatmap_min), float(debug_desc.heatmap_max),
                            1 if debug_desc.first_hit_only else 0)
    check(lib().lupin_hip_pathtrace_scene_debug(ctx.handle, resources.handle, scene.handle, render_target.handle,
                                                C.byref(dd), C.byref(c)))


def tonemap_and_fit_aspect(ctx, src, dst_width, dst_height, desc=None, dst=None):
    """lp::tonemap_and_fit_aspect (tonemapping.rs:155-224): `src` Texture -> (dst_height, dst_width, 4) uint8 (Rgba8Unorm).
    `dst` = previous target contents, used when desc.clear is False."""
    desc = desc or TonemapDesc()
    out = np.zeros((dst_height, dst_width, 4), np.uint8) if dst is None else np.ascontiguousarray(dst, np.uint8).copy()
    assert out.shape == (dst_height, dst_width, 4)
    vp = desc.viewport
    c = _abi.TonemapDescC(0 if vp is None else 1, *( (0.0, 0.0, 0.0, 0.0) if vp is None else (vp.x, vp.y, vp.w, vp.h)),
                          float(desc.exposure), 1 if desc.filmic else 0, 1 if desc.srgb else 0, 1 if desc.clear else 0)
    check(lib().lupin_hip_tonemap_and_fit_aspect(ctx.handle, src.handle, ptr(out), dst_width, dst_height, C.byref(c)))
    return out


class DenoiseQuality(enum.IntEnum):  # denoising.rs:208-218
    Low = 0
    Medium = 1
    High = 2

    @classmethod
    def default(cls):
        return cls.High   # #[default]


@dataclass
class DenoiseDesc:  # denoising.rs:193-206
    pathtrace_output: "Texture"
    denoise_output: "Texture"          # may be pathtrace_output: denoised in place
    albedo: Optional["Texture"] = None   # FalsecolorType.Albedo
    normals: Optional["Texture"] = None  # FalsecolorType.Normals
    quality: DenoiseQuality = DenoiseQuality.High


def _require_device(ctx, what):
    if ctx is None or getattr(ctx, "handle", None) is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), f"{what} needs a device context; there is no CPU fallback")


class DenoiseResources:
    """lp::DenoiseResources (denoising.rs:56-81): the filter's scratch for one width x height."""

    def __init__(self, ctx, width, height):
        _require_device(ctx, "build_denoise_resources")
        self.ctx = ctx
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        check(lib().lupin_hip_build_denoise_resources(ctx.handle, self.width, self.height, C.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if self.handle:   # after its context: only frees the scratch
                lib().lupin_hip_destroy_denoise_resources(self.handle)
            self.handle = None
        except Exception:
            pass


def build_denoise_resources(ctx, width, height):
    """lp::build_denoise_resources (denoising.rs:83): reusable for every denoise of that size."""
    return DenoiseResources(ctx, width, height)


def denoise(ctx, resources, desc: DenoiseDesc):
    """lp::denoise (denoising.rs:222-306): enqueued after every frame so far, returns without a host stall.  The output is
    f16 (nearest even) with the colour's alpha; its f32 accumulator is invalidated (Texture.download_f32 then fails)."""
    _require_device(ctx, "denoise")
    if resources is None or getattr(resources, "handle", None) is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "denoise resources were not built on a device")

    def h(t):
        return None if t is None else t.handle
    c = _abi.DenoiseDescC(h(desc.pathtrace_output), h(desc.albedo), h(desc.normals), h(desc.denoise_output), int(desc.quality))
    check(lib().lupin_hip_denoise(ctx.handle, resources.handle, C.byref(c)))


@dataclass
class AdaptiveParams:  # LupinAdaptiveParams
    threshold: float = 0.01   # relative standard error of the mean a block must fall below; 0 = no block ever converges
    min_frames: int = 8       # frames every pixel of a block takes before the block may stop
    max_frames: int = 0       # 0 = no cap


@dataclass
class AdaptiveStats:  # LupinAdaptiveStats
    active_pixels: int      # in-image pixels of the blocks the next call renders
    pixel_frames: int       # sum of the per-pixel frame counts since the latest reset
    calls: int              # adaptive calls since the latest reset
    max_frames_taken: int   # largest per-pixel frame count


class AdaptiveResources:
    """Adaptive sampling's state for one width x height (12 B per pixel + 14 B per 8x8 block), created reset."""

    def __init__(self, ctx, width, height):
        _require_device(ctx, "build_adaptive_resources")
        self.ctx = ctx
        self.width, self.height = int(width), int(height)
        self.blocks_x, self.blocks_y = (self.width + 7) // 8, (self.height + 7) // 8
        h = C.c_void_p()
        check(lib().lupin_hip_build_adaptive_resources(ctx.handle, self.width, self.height, C.byref(h)))
        self.handle = h

    def reset(self):
        """Counts and moments to 0, every block active: call it where accum_counter goes back to 0."""
        check(lib().lupin_hip_adaptive_reset(self.ctx.handle, self.handle))

    def stats(self):
        s = _abi.AdaptiveStatsC()
        check(lib().lupin_hip_adaptive_stats(self.ctx.handle, self.handle, C.byref(s)))
        return AdaptiveStats(int(s.active_pixels), int(s.pixel_frames), int(s.calls), int(s.max_frames_taken))

    def download(self):
        """(frames (H, W) uint32, moments (H, W, 2) float32 [mean, M2], block_error (by, bx) float32, block_active (by, bx) bool)."""
        frames = np.zeros((self.height, self.width), np.uint32)
        moments = np.zeros((self.height, self.width, 2), np.float32)
        err = np.zeros((self.blocks_y, self.blocks_x), np.float32)
        act = np.zeros((self.blocks_y, self.blocks_x), np.uint8)
        check(lib().lupin_hip_adaptive_download(self.ctx.handle, self.handle, ptr(frames), ptr(moments), ptr(err), ptr(act)))
        return frames, moments, err, act.astype(bool)

    def __del__(self):
        try:
            if self.handle:
                lib().lupin_hip_destroy_adaptive_resources(self.handle)
            self.handle = None
        except Exception:
            pass


def build_adaptive_resources(ctx, width, height):
    return AdaptiveResources(ctx, width, height)


def pathtrace_scene_adaptive(ctx, resources, scene, render_target, pathtrace_type, desc, adaptive_resources,
                             params: Optional[AdaptiveParams] = None):
    """One frame of the pixels whose 8x8 block is active.  desc.accum_params is required: its prev_frame
    supplies the inactive pixels, bit for bit, and an active pixel p renders as pathtrace_scene would with accum_counter =
    accum_params.accum_counter + (frames p has taken since the reset)."""
    assert render_target.format() == "Rgba16Float"
    if scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "scene was built without a device context; there is no CPU fallback")
    params = params or AdaptiveParams()
    keep = []
    c = _desc_to_c(desc, keep)
    p = _abi.AdaptiveParamsC(float(params.threshold), int(params.min_frames), int(params.max_frames))
    check(lib().lupin_hip_pathtrace_scene_adaptive(ctx.handle, resources.handle, scene.handle, render_target.handle,
                                                   int(pathtrace_type), C.byref(c), adaptive_resources.handle, C.byref(p)))


@dataclass
class ReprojectDesc:  # LupinReprojectDesc
    camera_params: CameraParams = field(default_factory=CameraParams)   # the NEW view
    camera_transform: np.ndarray = field(default_factory=identity_mat3x4)
    ray_epsilon: float = 0.001
    depth_tolerance: float = 0.02    # relative to the expected depth
    max_history: int = 0             # 0 = no cap; else every n_p <= max_history after the call
    # None = no instance moved; else (n, 3, 4) transpose_inverse_transform matrices (or instance records): what the scene held
    # when history_in was rendered
    prev_instance_transforms: Optional[np.ndarray] = None


class ReprojectResources:
    """Two visibility buffers, the previous view and the gather's output for one width x height (52 B per pixel)."""

    def __init__(self, ctx, width, height):
        _require_device(ctx, "build_reproject_resources")
        self.ctx = ctx
        self.width, self.height = int(width), int(height)
        h = C.c_void_p()
        check(lib().lupin_hip_build_reproject_resources(ctx.handle, self.width, self.height, C.byref(h)))
        self.handle = h

    def invalidate(self):
        """Forget the previous view (the next adaptive_reproject gives n = 0 everywhere): wherever AdaptiveResources.reset is called."""
        check(lib().lupin_hip_reproject_invalidate(self.ctx.handle, self.handle))

    def timings(self):
        """(trace_ms, gather_ms): device time of the latest call's two kernels; that call must have run after
        Context.stats_reset(1).  Waits for the gather."""
        t, g = C.c_float(), C.c_float()
        check(lib().lupin_hip_reproject_timings(self.ctx.handle, self.handle, C.byref(t), C.byref(g)))
        return float(t.value), float(g.value)

    def download(self, which=0):
        """Visibility of the latest call's view (which = 0) or of the call before it (1): (inst (H, W) uint32 with 0xFFFFFFFF =
        miss, tri (H, W) uint32 global triangle, uv (H, W, 2) float32, depth (H, W) float32 camera-space z)."""
        inst = np.zeros((self.height, self.width), np.uint32)
        tri = np.zeros((self.height, self.width), np.uint32)
        uv = np.zeros((self.height, self.width, 2), np.float32)
        depth = np.zeros((self.height, self.width), np.float32)
        check(lib().lupin_hip_reproject_download(self.ctx.handle, self.handle, int(which), ptr(inst), ptr(tri), ptr(uv), ptr(depth)))
        return inst, tri, uv, depth

    def __del__(self):
        try:
            if self.handle:
                lib().lupin_hip_destroy_reproject_resources(self.handle)
            self.handle = None
        except Exception:
            pass


def build_reproject_resources(ctx, width, height):
    return ReprojectResources(ctx, width, height)


def adaptive_reproject(ctx, adaptive_resources, resources, scene, desc: ReprojectDesc, history_in, history_out):
    """Carry history_in, the per-pixel frame counts and the moments over to desc's view: history_out and the
    adaptive state then hold, per pixel, the history of the surface point the pixel now shows (n = 0 where there is none),
    and the next pathtrace_scene_adaptive call with prev_frame = history_out continues from them."""
    if scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "scene was built without a device context; there is no CPU fallback")
    c = _abi.ReprojectDescC()
    cp = desc.camera_params
    c.camera_params = _abi.CameraParamsC(1 if cp.is_orthographic else 0, cp.lens, cp.film, cp.aspect, cp.focus, cp.aperture)
    m = np.asarray(desc.camera_transform, np.float32).reshape(4, 3)
    for col in range(4):
        for row in range(3):
            c.camera_transform.m[col][row] = float(m[col][row])
    c.ray_epsilon = float(desc.ray_epsilon)
    c.depth_tolerance = float(desc.depth_tolerance)
    c.max_history = int(desc.max_history)
    t = None
    if desc.prev_instance_transforms is not None:
        t = np.asarray(desc.prev_instance_transforms)
        if t.dtype == INSTANCE_DTYPE:
            t = t["transpose_inverse_transform"]
        t = np.ascontiguousarray(t, np.float32).reshape(-1, 3, 4)
        c.prev_instance_transforms = t.ctypes.data
        c.num_instances = len(t)
    check(lib().lupin_hip_adaptive_reproject(ctx.handle, adaptive_resources.handle, resources.handle, scene.handle, C.byref(c),
                                             history_in.handle, history_out.handle))


def pathtrace_scene_tiles(ctx, resources, scene, render_target, pathtrace_type, desc, tile_size, rank, world):
    """Multi-GPU extension: all tiles owned by `rank` (include/lupin_tiles.h: round-robin, rotated rows) of one accumulation frame, in one launch."""
    assert render_target.format() == "Rgba16Float"
    if scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "scene was built without a device context; there is no CPU fallback")
    keep = []
    c = _desc_to_c(desc, keep)
    check(lib().lupin_hip_pathtrace_scene_tiles(ctx.handle, resources.handle, scene.handle, render_target.handle,
                                                int(pathtrace_type), C.byref(c), tile_size, rank, world))


def pack_tiles(ctx, texture, tile_size, rank, world, device_dst_ptr):
    n = C.c_uint64()
    check(lib().lupin_hip_pack_tiles(ctx.handle, texture.handle, tile_size, rank, world, C.c_void_p(device_dst_ptr), C.byref(n)))
    return int(n.value)


def unpack_tiles(ctx, texture, tile_size, rank, world, device_src_ptr):
    check(lib().lupin_hip_unpack_tiles(ctx.handle, texture.handle, tile_size, rank, world, C.c_void_p(device_src_ptr)))


def unpack_gathered_tiles(ctx, texture, tile_size, rank, world, device_gathered_ptr, capacity_pixels):
    """One launch: every tile not owned by `rank` from `world` payloads of `capacity_pixels` pixels each."""
    check(lib().lupin_hip_unpack_gathered_tiles(ctx.handle, texture.handle, tile_size, rank, world, C.c_void_p(device_gathered_ptr), capacity_pixels))


def packed_tile_pixels(width, height, tile_size, rank, world):
    return int(lib().lupin_hip_packed_tile_pixels(width, height, tile_size, rank, world))


class Comm:
    """RCCL communicator of one context (include/lupin_hip.h "the one exchange step"): one per rank / per GPU."""

    def __init__(self, ctx, handle, rank, world):
        self.ctx, self.handle, self.rank, self.world = ctx, handle, rank, world

    @staticmethod
    def unique_id():
        """128 opaque bytes made by rank 0 (ncclGetUniqueId) that every rank passes to `init_rank`."""
        buf = (C.c_uint8 * 128)()
        check(lib().lupin_hip_comm_get_unique_id(C.cast(buf, C.c_void_p)))
        return bytes(buf)

    @classmethod
    def init_rank(cls, ctx, unique_id, rank, world):
        assert len(unique_id) == 128
        h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        check(lib().lupin_hip_comm_init_rank(ctx.handle, C.cast(buf, C.c_void_p), rank, world, C.byref(h)))
        return cls(ctx, h, rank, world)

    @classmethod
    def init_all(cls, ctxs):
        """One process driving len(ctxs) GPUs (one context per device)."""
        n = len(ctxs)
        cin = (C.c_void_p * n)(*[c.handle for c in ctxs])
        cout = (C.c_void_p * n)()
        check(lib().lupin_hip_comm_init_all(cin, n, cout))
        return [cls(ctxs[i], C.c_void_p(cout[i]), i, n) for i in range(n)]

    def gather_framebuffer(self, texture, tile_size):
        """pack own tiles -> all-gather -> scatter the others' tiles; enqueued, `texture.download()` / `ctx.sync()` waits."""
        check(lib().lupin_hip_gather_framebuffer(self.handle, texture.handle, tile_size))

    def gather_framebuffer_to(self, texture, tile_size, root=0):
        """pack own tiles -> grouped ncclSend / ncclRecv -> the root scatters: only `root` ends up with the whole frame."""
        check(lib().lupin_hip_gather_framebuffer_to(self.handle, texture.handle, tile_size, root))

    def allreduce(self, values, op="sum"):
        a = np.ascontiguousarray(values, dtype=np.float64).copy()
        check(lib().lupin_hip_comm_allreduce_f64(self.handle, ptr(a), a.size, {"sum": 0, "max": 1}[op]))
        return a

    def barrier(self):
        """Every rank's enqueued frames have completed when this returns."""
        check(lib().lupin_hip_comm_barrier(self.handle))

    def close(self):
        if self.handle and self.ctx.handle:
            lib().lupin_hip_comm_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gather_framebuffer_all(comms, textures, tile_size):
    n = len(comms)
    check(lib().lupin_hip_gather_framebuffer_all((C.c_void_p * n)(*[c.handle for c in comms]),
                                                 (C.c_void_p * n)(*[t.handle for t in textures]), n, tile_size))


def _abi_code(name):
    return {"LUPIN_ERR_NO_DEVICE": -2}[name]


def trace_rays(ctx, scene, ori, dir_, ray_epsilon=0.001):
    """Closest-hit probe (bvh_custom.wgsl:7-110) on the device: returns hit, dst, uv, instance, tri arrays."""
    ori = np.ascontiguousarray(ori, np.float32).reshape(-1, 3)
    dir_ = np.ascontiguousarray(dir_, np.float32).reshape(-1, 3)
    n = len(ori)
    hit = np.zeros(n, np.uint32)
    dst = np.zeros(n, np.float32)
    uv = np.zeros((n, 2), np.float32)
    inst = np.zeros(n, np.uint32)
    tri = np.zeros(n, np.uint32)
    check(lib().lupin_hip_trace_rays(ctx.handle, scene.handle, n, ptr(ori), ptr(dir_), ray_epsilon,
                                     ptr(hit), ptr(dst), ptr(uv), ptr(inst), ptr(tri)))
    return hit, dst, uv, inst, tri


def trace_rays_wide(ctx, scene, ori, dir_, ray_epsilon=0.001):
    """The same probe through the four-wide traversal: returns hit, dst, uv, instance, tri and `needs_retrace` (1 = the
    traversal could not certify that ray; the pipeline re-traces such queries with the binary kernel)."""
    ori = np.ascontiguousarray(ori, np.float32).reshape(-1, 3)
    dir_ = np.ascontiguousarray(dir_, np.float32).reshape(-1, 3)
    n = len(ori)
    hit = np.zeros(n, np.uint32)
    dst = np.zeros(n, np.float32)
    uv = np.zeros((n, 2), np.float32)
    inst = np.zeros(n, np.uint32)
    tri = np.zeros(n, np.uint32)
    flag = np.zeros(n, np.uint32)
    check(lib().lupin_hip_trace_rays_wide(ctx.handle, scene.handle, n, ptr(ori), ptr(dir_), ray_epsilon,
                                          ptr(hit), ptr(dst), ptr(uv), ptr(inst), ptr(tri), ptr(flag)))
    return hit, dst, uv, inst, tri, flag


# lupin_hip_scatter_probe record layout (include/lupin_hip.h)
SCATTER_IN_FLOATS = 28
SCATTER_OUT_FLOATS = 8


class ScatterMode(enum.IntEnum):
    BSDF_SAMPLE = 0
    BSDF_EVAL = 1
    PHASE_SAMPLE = 2
    PHASE_EVAL = 3
    MEDIUM_SAMPLE = 4
    MEDIUM_EVAL = 5


def scatter_probe(ctx, records):
    """BSDF / delta / phase / medium functions of the device over (n, SCATTER_IN_FLOATS) float32 records; returns the
    (n, SCATTER_OUT_FLOATS) float32 outputs (direction, eval, pdf, 0)."""
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, SCATTER_IN_FLOATS)
    out = np.zeros((len(rec), SCATTER_OUT_FLOATS), np.float32)
    check(lib().lupin_hip_scatter_probe(ctx.handle, len(rec), ptr(rec), ptr(out)))
    return out


# lupin_hip_light_probe record layout (include/lupin_hip.h)
LIGHT_IN_FLOATS = 12
LIGHT_OUT_FLOATS = 8


class LightMode(enum.IntEnum):
    SAMPLE = 0
    PDF = 1


def light_records(mode, pos, incoming=None, ray_epsilon=0.001, rng=0):
    """(n, LIGHT_IN_FLOATS) float32 records for light_probe / oracle.light_probe: `pos` (n, 3), `incoming` (n, 3) or None,
    `ray_epsilon` and `rng` (u32 states, stored as bits) scalars or (n,) arrays."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    rec = np.zeros((len(pos), LIGHT_IN_FLOATS), np.float32)
    rec[:, 0] = np.float32(int(mode))
    rec[:, 1:4] = pos
    if incoming is not None:
        rec[:, 4:7] = np.asarray(incoming, np.float32).reshape(-1, 3)
    rec[:, 7] = np.asarray(ray_epsilon, np.float32)
    rec.view(np.uint32)[:, 8] = np.asarray(rng, np.uint32)
    return rec


def light_probe(ctx, scene, records):
    """sample_lights / sample_lights_pdf of the device on `scene` over (n, LIGHT_IN_FLOATS) float32 records; returns the
    (n, LIGHT_OUT_FLOATS) float32 outputs: direction, pdf, RNG state afterwards (bits; read it with .view(np.uint32)), 0."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "light_probe needs a GPU context and an uploaded scene; there is no CPU fallback")
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, LIGHT_IN_FLOATS)
    out = np.zeros((len(rec), LIGHT_OUT_FLOATS), np.float32)
    check(lib().lupin_hip_light_probe(ctx.handle, scene.handle, len(rec), ptr(rec), ptr(out)))
    return out


# lupin_hip_surface_probe record layout (include/lupin_hip.h)
SURFACE_IN_FLOATS = 8
SURFACE_OUT_FLOATS = 20


class SurfaceMode(enum.IntEnum):
    TEXTURE = 0
    MATERIAL = 1
    MATERIAL_SIMPLE = 2
    OPACITY = 3
    NORMAL = 4
    ENVIRONMENT = 5


def surface_records(mode, index=0, tri=0, uv=None, direction=None, n=None):
    """(n, SURFACE_IN_FLOATS) float32 records for surface_probe / oracle.surface_probe.  `mode` a SurfaceMode or (n,) array
    of them; `index` the instance (TEXTURE mode: the texture) and `tri` the triangle within its mesh, as trace_rays returns
    them (u32, stored as bits); `uv` (n, 2) the hit's barycentrics (TEXTURE mode: the texture coordinates); `direction`
    (n, 3) for ENVIRONMENT mode."""
    for a in (uv, direction, mode, index, tri):
        if n is None and a is not None and np.ndim(a) > 0:
            n = len(a)
    rec = np.zeros((n or 1, SURFACE_IN_FLOATS), np.float32)
    rec[:, 0] = np.asarray(mode, np.float32)
    rec.view(np.uint32)[:, 1] = np.asarray(index, np.uint32)
    rec.view(np.uint32)[:, 2] = np.asarray(tri, np.uint32)
    if uv is not None:
        rec[:, 3:5] = np.asarray(uv, np.float32).reshape(-1, 2)
    if direction is not None:
        rec[:, 5:8] = np.asarray(direction, np.float32).reshape(-1, 3)
    return rec


def surface_probe(ctx, scene, records):
    """sample_texture / material point / opacity / shading and geometric normal / environment radiance of the device on
    `scene` over (n, SURFACE_IN_FLOATS) float32 records; returns the (n, SURFACE_OUT_FLOATS) float32 outputs (layout per
    mode: include/lupin_hip.h; the material type is stored as bits: read it with .view(np.uint32))."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "surface_probe needs a GPU context and an uploaded scene; there is no CPU fallback")
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, SURFACE_IN_FLOATS)
    out = np.zeros((len(rec), SURFACE_OUT_FLOATS), np.float32)
    check(lib().lupin_hip_surface_probe(ctx.handle, scene.handle, len(rec), ptr(rec), ptr(out)))
    return out


# lupin_hip_camera_probe record layout (include/lupin_hip.h)
CAMERA_IN_WORDS = 4
CAMERA_OUT_FLOATS = 8


class CameraMode(enum.IntEnum):
    RAY = 0
    RAY_CENTRE = 1


def camera_transform_mat4(transform):
    """The 4 columns x 4 rows matrix lupin_hip_camera_probe and oracle.camera_probe take, as a (4, 4) float32 array [column][row]:
    from a (4, 3) LupinMat3x4 (the last row becomes the renderer's (0, 0, 0, 1)) or from 16 numbers taken as they are."""
    m = np.asarray(transform, np.float32)
    if m.size == 12:
        m = np.concatenate([m.reshape(4, 3), np.array([[0.0], [0.0], [0.0], [1.0]], np.float32)], axis=1)
    return np.ascontiguousarray(m.reshape(4, 4), np.float32)


def camera_records(gx, gy, rng_state, mode=CameraMode.RAY):
    """(n, CAMERA_IN_WORDS) uint32 records for camera_probe / oracle.camera_probe: pixel, RNG state, CameraMode."""
    gx = np.asarray(gx, np.uint32).reshape(-1)
    rec = np.zeros((len(gx), CAMERA_IN_WORDS), np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = gx, np.asarray(gy, np.uint32), np.asarray(rng_state, np.uint32), np.asarray(mode, np.uint32)
    return rec


def camera_probe(ctx, width, height, camera_params, camera_transform, records):
    """camera_ray / camera_ray_centre of the device for a width x height image over (n, CAMERA_IN_WORDS) uint32 records;
    `camera_transform` as camera_transform_mat4 takes it.  Returns (ori (n, 3) float32, dir (n, 3) float32, RNG state
    afterwards (n,) uint32)."""
    if ctx is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "camera_probe needs a GPU context; there is no CPU fallback")
    rec = np.ascontiguousarray(records, np.uint32).reshape(-1, CAMERA_IN_WORDS)
    out = np.zeros((len(rec), CAMERA_OUT_FLOATS), np.float32)
    cp = camera_params
    c = _abi.CameraParamsC(1 if cp.is_orthographic else 0, cp.lens, cp.film, cp.aspect, cp.focus, cp.aperture)
    m4 = _abi.Mat4()
    C.memmove(C.byref(m4), camera_transform_mat4(camera_transform).ctypes.data, 64)
    check(lib().lupin_hip_camera_probe(ctx.handle, int(width), int(height), C.byref(c), C.byref(m4), len(rec), ptr(rec), ptr(out)))
    return out[:, 0:3].copy(), out[:, 3:6].copy(), out[:, 6].copy().view(np.uint32)


# ---- radiance queries: lupin_hip_pathtrace_rays (include/lupin_hip.h) ----
RAY_RECORD_FLOATS = 8
RAY_RESULT_FLOATS = 4
RAYS_DEVICE_POINTERS = 1
RAYS_DEFAULT_MAX_SLOTS = 1 << 22   # LUPIN_RAYS_DEFAULT_MAX_SLOTS: paths per wavefront when RayQueryDesc.max_slots is 0


class RayMode(enum.IntEnum):
    DIRECTION = 0            # floats 4..6 are the ray's unit direction
    COSINE_HEMISPHERE = 1    # floats 4..6 are a unit surface normal; the direction is cosine-sampled about it


@dataclass
class RayQueryDesc:  # LupinRayQueryDesc
    pathtrace_type: int = PathtraceType.Standard
    max_bounces: int = 8
    samples: int = 1
    flags: int = 0
    max_slots: int = 0       # paths per wavefront; 0 = the library's default
    advanced: AdvancedParams = field(default_factory=AdvancedParams)


def _hash_u32(x):
    """hash_u32 of the device (pathtracer.wgsl:1561-1570) on uint32 arrays."""
    x = np.asarray(x, np.uint32).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint32(17); x *= np.uint32(0xed5ad4bb)
        x ^= x >> np.uint32(11); x *= np.uint32(0xac4c1b51)
        x ^= x >> np.uint32(15); x *= np.uint32(0x31848bab)
        x ^= x >> np.uint32(14)
    return x


def rng_seed_for(index, counter=0):
    """The device's rng_seed_for in numpy: the u32 RNG state a pixel with linear index `index` starts a frame of
    accum_counter `counter` with.  Scalars or arrays; seeds records the way pixels are seeded."""
    index = np.asarray(index, np.uint32)
    counter = np.asarray(counter, np.uint32)
    with np.errstate(over="ignore"):
        return _hash_u32((index * np.uint32(19349663)) ^ (counter * np.uint32(83492791)))


def ray_sample_seed(word, s):
    """RNG state of path `s` of a record whose RNG word is `word`: the word itself for s == 0, hash_u32(word + s * 0x9E3779B9)
    otherwise."""
    word = np.asarray(word, np.uint32)
    s = np.asarray(s, np.uint32)
    with np.errstate(over="ignore"):
        return np.where(s == 0, word, _hash_u32(word + s * np.uint32(0x9E3779B9))).astype(np.uint32)


def ray_records(ori, dir_or_normal, rng=0, mode=RayMode.DIRECTION):
    """(n, RAY_RECORD_FLOATS) float32 records for pathtrace_rays: `ori` (n, 3); `dir_or_normal` (n, 3), the unit direction
    (mode DIRECTION) or the unit surface normal (mode COSINE_HEMISPHERE); `rng` u32 states and `mode`, scalars or (n,)
    arrays, both stored as bits."""
    ori = np.asarray(ori, np.float32).reshape(-1, 3)
    rec = np.zeros((len(ori), RAY_RECORD_FLOATS), np.float32)
    rec[:, 0:3] = ori
    rec[:, 4:7] = np.asarray(dir_or_normal, np.float32).reshape(-1, 3)
    rec.view(np.uint32)[:, 3] = np.asarray(rng, np.uint32)
    rec.view(np.uint32)[:, 7] = np.asarray(mode, np.uint32)
    return rec


def pathtrace_rays(ctx, scene, records, desc: Optional[RayQueryDesc] = None, want_rays=False):
    """The radiance along (or, mode COSINE_HEMISPHERE, arriving at) every record: (n, 4) r, g, b, 1 -- the mean over
    desc.samples paths per record.  `records` is an (n, RAY_RECORD_FLOATS) float32 numpy array (see ray_records), or a
    contiguous float32 torch tensor on the context's device: then torch's current stream is synchronised, the tensors' device
    memory is used in place and tensors are returned.  With want_rays also the (n * samples, RAY_RECORD_FLOATS) first rays,
    as mode-DIRECTION records that replay one path each.  Blocks until the result is complete."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "pathtrace_rays needs a GPU context and an uploaded scene; there is no CPU fallback")
    desc = desc or RayQueryDesc()
    flags = int(desc.flags)
    c = _abi.RayQueryDescC(int(desc.pathtrace_type), int(desc.max_bounces), int(desc.samples), flags, int(desc.max_slots),
                           _abi.AdvancedParamsC(desc.advanced.max_radiance, desc.advanced.rng_seed, desc.advanced.ray_epsilon))
    if hasattr(records, "data_ptr"):   # a torch tensor
        import torch
        t = records
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == RAY_RECORD_FLOATS):
            raise ValueError("records must be a contiguous (n, 8) float32 tensor on the context's device")
        if t.device.index != ctx.device_ordinal:
            raise ValueError("records are on another device than the context")
        n = int(t.shape[0])
        out = torch.zeros((n, RAY_RESULT_FLOATS), dtype=torch.float32, device=t.device)
        rays = torch.zeros((n * int(desc.samples), RAY_RECORD_FLOATS), dtype=torch.float32, device=t.device) if want_rays else None
        torch.cuda.current_stream(t.device).synchronize()   # the records (and the zero fills) are written
        c.flags = flags | RAYS_DEVICE_POINTERS
        check(lib().lupin_hip_pathtrace_rays(ctx.handle, scene.handle, C.byref(c), n, C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()),
                                             C.c_void_p(rays.data_ptr()) if want_rays else None))
        return (out, rays) if want_rays else out
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, RAY_RECORD_FLOATS)
    out = np.zeros((len(rec), RAY_RESULT_FLOATS), np.float32)
    rays = np.zeros((len(rec) * int(desc.samples), RAY_RECORD_FLOATS), np.float32) if want_rays else None
    check(lib().lupin_hip_pathtrace_rays(ctx.handle, scene.handle, C.byref(c), len(rec), ptr(rec), ptr(out), ptr(rays)))
    return (out, rays) if want_rays else out


def bake_irradiance(ctx, scene, points, normals, samples=64, pathtrace_type=PathtraceType.Standard, max_bounces=8, advanced=None,
                    counter=0, max_slots=0):
    """Irradiance (n, 3) at `points` (n, 3) with unit `normals` (n, 3): pi * the mean radiance over `samples` cosine-weighted
    paths per point (mode COSINE_HEMISPHERE records, point i seeded with rng_seed_for(i, counter)).
    The paths start AT the points given: the caller offsets them off the surface (along the normal, by more than
    advanced.ray_epsilon times the scene's scale), or the first ray may hit the surface it starts on."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    rec = ray_records(points, normals, rng_seed_for(np.arange(len(points), dtype=np.uint32), counter), RayMode.COSINE_HEMISPHERE)
    desc = RayQueryDesc(pathtrace_type, max_bounces, samples, 0, max_slots, advanced or AdvancedParams())
    out = pathtrace_rays(ctx, scene, rec, desc)
    return np.float32(np.pi) * out[:, :3]


# ---- lightmap baking: lupin_hip_bake_lightmap (include/lupin_hip.h) ----
LIGHTMAP_SMOOTH_NORMALS = 1
LIGHTMAP_MAX_SIZE = 16384
LIGHTMAP_MAX_DILATE = 64
LIGHTMAP_OFFSET_FRACTION = 1e-4   # default surface_offset: this fraction of the scene's largest world extent


@dataclass
class LightmapChart:  # LupinLightmapChart: atlas uv = mesh uv * scale + offset
    instance_idx: int = 0
    scale_u: float = 1.0
    scale_v: float = 1.0
    offset_u: float = 0.0
    offset_v: float = 0.0


@dataclass
class LightmapDesc:  # LupinLightmapDesc
    width: int = 0
    height: int = 0
    pathtrace_type: int = PathtraceType.Standard
    max_bounces: int = 8
    samples: int = 64
    max_slots: int = 0
    flags: int = 0
    dilate: int = 0
    counter: int = 0
    surface_offset: float = 0.0
    advanced: AdvancedParams = field(default_factory=AdvancedParams)


def scene_world_extent(scene):
    """The largest side of the box around the scene's instances in world space, from the model boxes the TLAS was built
    from: every instance's eight box corners through the inverse of its world -> local affine.  0.0 for an empty scene."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in scene.instances:
        box = np.asarray(scene.model_aabbs[int(inst["mesh_idx"])], np.float64)
        if not np.all(box[:3] <= box[3:]):
            continue   # Aabb::neutral(): a mesh without vertices
        m = np.asarray(inst["transpose_inverse_transform"], np.float64)      # 3 x 4 rows of world -> local
        inv = np.linalg.inv(m[:, :3])
        corners = np.array([[box[0 + 3 * (k & 1)], box[1 + 3 * ((k >> 1) & 1)], box[2 + 3 * ((k >> 2) & 1)]] for k in range(8)])
        world = (corners - m[:, 3]) @ inv.T
        lo, hi = np.minimum(lo, world.min(axis=0)), np.maximum(hi, world.max(axis=0))
    return float((hi - lo).max()) if np.all(np.isfinite(hi - lo)) else 0.0


def lightmap_stats():
    """The calling thread's latest successful bake_lightmap: covered texels, (chart, triangle) pairs, host-clock ms per phase."""
    s = _abi.LightmapStatsC()
    lib().lupin_hip_lightmap_stats(C.byref(s))
    return {"covered_texels": int(s.covered_texels), "keys": int(s.keys), "raster_ms": float(s.raster_ms), "compact_ms": float(s.compact_ms),
            "trace_ms": float(s.trace_ms), "scatter_dilate_ms": float(s.scatter_dilate_ms), "download_ms": float(s.download_ms)}


def bake_lightmap(ctx, scene, charts, width, height, samples=64, pathtrace_type=PathtraceType.Standard, max_bounces=8, advanced=None,
                  counter=0, max_slots=0, smooth_normals=False, dilate=0, surface_offset=None, want_records=False, denoise=False):
    """The scene's irradiance as a lightmap: (height, width, 4) float32, rgb = pi * the mean radiance over `samples`
    cosine-weighted paths from the surface point under each texel centre, alpha 1 on rasterised texels and 0 elsewhere
    (gutter texels filled by `dilate` passes keep alpha 0).  Row 0 is v in [0, 1 / height): no flip.
    `charts`: LightmapChart items (or (instance_idx, scale_u, scale_v, offset_u, offset_v) tuples); the mesh's texcoords times
    the scale plus the offset are the instance's place in the atlas.  Where charts or triangles overlap, the first chart and
    the lowest triangle own the texel.  smooth_normals: hemispheres about the interpolated vertex normals where the mesh has
    them (the origin is still offset along the geometric normal).
    surface_offset (world units along the geometric normal) defaults to LIGHTMAP_OFFSET_FRACTION = 1e-4 times the
    largest world extent of the scene, taken from the instances' model boxes (scene_world_extent), and to 1e-4 for a scene
    without extent.  With want_records also the (height, width, 8) ray records of the owned texels (zeros elsewhere).
    denoise: the atlas is baked without gutter passes, filtered by denoise_lightmap with its defaults, and the `dilate`
    gutter passes run after the filter, from the filtered texels.
    Blocks until the result is complete."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "bake_lightmap needs a GPU context and an uploaded scene; there is no CPU fallback")
    if denoise:
        noisy, rec = bake_lightmap(ctx, scene, charts, width, height, samples, pathtrace_type, max_bounces, advanced, counter, max_slots,
                                   smooth_normals, 0, surface_offset, True)
        out = denoise_lightmap(ctx, noisy, rec, dilate=dilate)
        return (out, rec) if want_records else out
    if surface_offset is None:
        surface_offset = LIGHTMAP_OFFSET_FRACTION * (scene_world_extent(scene) or 1.0)
    adv = advanced or AdvancedParams()
    items = [c if isinstance(c, LightmapChart) else LightmapChart(*c) for c in charts]
    c_charts = (_abi.LightmapChartC * max(1, len(items)))(*[_abi.LightmapChartC(int(c.instance_idx), c.scale_u, c.scale_v, c.offset_u, c.offset_v)
                                                           for c in items])
    d = _abi.LightmapDescC(int(width), int(height), int(pathtrace_type), int(max_bounces), int(samples), int(max_slots),
                           LIGHTMAP_SMOOTH_NORMALS if smooth_normals else 0, int(dilate), int(counter), float(surface_offset),
                           _abi.AdvancedParamsC(adv.max_radiance, adv.rng_seed, adv.ray_epsilon))
    shape_ok = 0 < int(width) <= LIGHTMAP_MAX_SIZE and 0 < int(height) <= LIGHTMAP_MAX_SIZE
    out = np.zeros((int(height), int(width), 4) if shape_ok else (1, 1, 4), np.float32)      # a refused size: the library says so
    rec = np.zeros((int(height), int(width), RAY_RECORD_FLOATS) if shape_ok else (1, 1, RAY_RECORD_FLOATS), np.float32) if want_records else None
    check(lib().lupin_hip_bake_lightmap(ctx.handle, scene.handle, C.byref(d), c_charts, len(items), ptr(out), ptr(rec), None))
    return (out, rec) if want_records else out


# ---- lightmap UV sets: Scene.set_lightmap_uvs, Scene.unwrap_lightmap_uvs, the shelf packer (include/lupin_pack.hpp) ----
UNWRAP_MAX_PADDING = 16
UNWRAP_NO_CHART = 0xFFFFFFFF


def isqrt_ceil(n):
    """The smallest r with r * r >= n."""
    r = math.isqrt(int(n))
    return r if r * r == int(n) else r + 1


def shelf_pack(sizes):
    """include/lupin_pack.hpp's shelf packer, in integers.  sizes: (w, h) per rectangle; its index is its label.
    Rectangles sorted by height descending, then width descending, then label ascending; the atlas is
    max(widest, isqrt_ceil(sum of areas)) wide; placed left to right, a new shelf opens when the next rectangle would cross
    the width; the height is the bottom of the last shelf.  Returns (width, height, [(x, y) per rectangle])."""
    rects = [(int(w), int(h)) for w, h in sizes]
    order = sorted(range(len(rects)), key=lambda i: (-rects[i][1], -rects[i][0], i))
    width = max([w for w, _ in rects] + [isqrt_ceil(sum(w * h for w, h in rects))])
    place = [None] * len(rects)
    x = y = shelf = 0
    for i in order:
        w, h = rects[i]
        if x + w > width:
            y, x, shelf = y + shelf, 0, 0
        place[i] = (x, y)
        x += w
        shelf = max(shelf, h)
    return width, y + shelf, place


def pack_lightmap_instances(sizes, multipliers, gutter=2):
    """Place instances in one atlas, on the host: (width, height, [LightmapChart per entry]).  sizes: per entry the (width,
    height) in texels of its mesh's own atlas (unwrap_lightmap_uvs' info); multipliers: per entry the resolution m relative
    to that atlas; gutter: texels kept free around every entry.  Entry i gets the rectangle ceil(size * m) + 2 * gutter per
    side (the product one f32 operation), the rectangles go through shelf_pack, and its chart is instance_idx = i,
    scale = (m / W, m / H), offset = ((x + gutter) / W, (y + gutter) / H), each one f32 division: the unit of the mesh's
    lightmap UVs is a texel of its own atlas.  ValueError for a multiplier that is not finite and positive, a size of 0, or
    a rectangle or an atlas above LIGHTMAP_MAX_SIZE."""
    f32 = np.float32
    ms = [f32(m) for m in multipliers]
    if len(ms) != len(sizes):
        raise ValueError("one multiplier per size")
    gutter = int(gutter)
    if not 0 <= gutter <= LIGHTMAP_MAX_SIZE:
        raise ValueError("gutter out of range")
    rects = []
    for (w, h), m in zip(sizes, ms):
        side = []
        for s in (int(w), int(h)):
            if not (np.isfinite(m) and m > 0) or not 0 < s <= LIGHTMAP_MAX_SIZE:
                raise ValueError("sizes must be in [1, LIGHTMAP_MAX_SIZE] and multipliers finite and positive")
            c = np.ceil(f32(s) * m)
            if not c <= LIGHTMAP_MAX_SIZE or max(int(c), 1) + 2 * gutter > LIGHTMAP_MAX_SIZE:
                raise ValueError("a placed instance is larger than LIGHTMAP_MAX_SIZE")
            side.append(max(int(c), 1) + 2 * gutter)
        rects.append(tuple(side))
    width, height, place = shelf_pack(rects)
    if width > LIGHTMAP_MAX_SIZE or height > LIGHTMAP_MAX_SIZE:
        raise ValueError("the atlas is larger than LIGHTMAP_MAX_SIZE")
    charts = [LightmapChart(i, float(m / f32(width)), float(m / f32(height)), float(f32(x + gutter) / f32(width)), float(f32(y + gutter) / f32(height)))
              for i, ((x, y), m) in enumerate(zip(place, ms))]
    return width, height, charts


# ---- lightmap denoising: lupin_hip_denoise_lightmap (include/lupin_hip.h) ----
LIGHTMAP_DENOISE_DEVICE_POINTERS = 1
LIGHTMAP_DENOISE_MAX_PASSES = 8
LIGHTMAP_DENOISE_MAX_SQUARINGS = 7


def denoise_lightmap(ctx, rgba, records, passes=5, normal_squarings=5, max_stretch=4.0, dilate=0):
    """A baked lightmap, filtered in atlas space: (height, width, 4) float32.  `rgba` (height, width, 4) and `records`
    (height, width, RAY_RECORD_FLOATS) are what bake_lightmap(..., want_records=True) returns (or several bakes with
    different `counter`, averaged).  An edge-avoiding a-trous filter of `passes` 5 x 5 passes at steps 1, 2, 4, ..: a tap
    counts only if its surface point is as near in space as it is in the atlas (within max_stretch times the texel's own
    footprint per texel of distance), weighted by max(0, n_p . n_q)^(2^normal_squarings) and by the luminance difference
    against the local deviation.  Charts, gutters and folds are never filtered across.  Alpha is the input's; texels of
    alpha 0 are returned as they came, or with dilate > 0 refilled from the filtered texels by that many gutter passes.
    numpy arrays, or contiguous float32 torch tensors on the context's device: then torch's current stream is synchronised,
    the tensors' device memory is used in place and a tensor is returned.  Blocks until the result is complete."""
    if ctx is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "denoise_lightmap needs a GPU context; there is no CPU fallback")
    if hasattr(rgba, "data_ptr") or hasattr(records, "data_ptr"):   # torch tensors
        import torch
        for t, last in ((rgba, 4), (records, RAY_RECORD_FLOATS)):
            if not (hasattr(t, "data_ptr") and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 3 and t.shape[2] == last):
                raise ValueError("rgba and records must be contiguous (height, width, 4) and (height, width, 8) float32 tensors on the context's device")
            if t.device.index != ctx.device_ordinal:
                raise ValueError("rgba and records are on another device than the context")
        if tuple(rgba.shape[:2]) != tuple(records.shape[:2]):
            raise ValueError("rgba and records differ in height or width")
        h, w = int(rgba.shape[0]), int(rgba.shape[1])
        out = torch.zeros((h, w, 4), dtype=torch.float32, device=rgba.device)
        torch.cuda.current_stream(rgba.device).synchronize()   # the inputs (and the zero fill) are written
        d = _abi.LightmapDenoiseDescC(w, h, int(passes), int(normal_squarings), int(dilate), LIGHTMAP_DENOISE_DEVICE_POINTERS, float(max_stretch))
        check(lib().lupin_hip_denoise_lightmap(ctx.handle, C.byref(d), C.c_void_p(rgba.data_ptr()), C.c_void_p(records.data_ptr()),
                                               C.c_void_p(out.data_ptr())))
        return out
    rgba = np.ascontiguousarray(rgba, np.float32)
    records = np.ascontiguousarray(records, np.float32)
    if rgba.ndim != 3 or rgba.shape[2] != 4 or records.shape != rgba.shape[:2] + (RAY_RECORD_FLOATS,):
        raise ValueError("rgba must be (height, width, 4) and records (height, width, 8)")
    h, w = rgba.shape[:2]
    d = _abi.LightmapDenoiseDescC(w, h, int(passes), int(normal_squarings), int(dilate), 0, float(max_stretch))
    out = np.zeros((h, w, 4), np.float32)
    check(lib().lupin_hip_denoise_lightmap(ctx.handle, C.byref(d), ptr(rgba), ptr(records), ptr(out)))
    return out


def lightmap_denoise_stats():
    """The calling thread's latest successful denoise_lightmap: device-event ms of the prep pass, of each filter pass and of
    the gutter passes together, host-clock ms of the call."""
    s = _abi.LightmapDenoiseStatsC()
    lib().lupin_hip_lightmap_denoise_stats(C.byref(s))
    return {"prep_ms": float(s.prep_ms), "pass_ms": [float(v) for v in s.pass_ms], "dilate_ms": float(s.dilate_ms), "call_ms": float(s.call_ms)}


# ---- lightmap seam stitching: lupin_hip_stitch_lightmap (include/lupin_hip.h) ----
LIGHTMAP_STITCH_DEVICE_POINTERS = 1
LIGHTMAP_STITCH_MAX_ITERATIONS = 1024
LIGHTMAP_STITCH_MAX_EDGE_SAMPLES = 65536


def stitch_lightmap(ctx, scene, charts, rgba, iterations=32, samples_per_texel=2.0, lam=0.1, want_info=False):
    """A baked (or denoised) lightmap with its chart borders pulled together: (height, width, 4) float32.  `charts` are the
    LightmapChart items the atlas was baked with.  Every interior edge of a chart's mesh whose two sides have different
    lightmap UVs is a seam; it is sampled `samples_per_texel` times per texel of its length, and `iterations` steps of
    conjugate gradients minimise, per channel, the squared difference of what the lightmapped view fetches on the two sides
    of every sample plus `lam` times the squared distance of every touched texel from its baked value.  Texels no sample
    touches, and every alpha, come back bit for bit; iterations == 0 returns the input and reports the counts.
    want_info: also a dict of the seam edges, non-manifold edges, sample pairs, dropped pairs, active texels, iterations and
    the seam energy per channel before and after.  numpy arrays, or a contiguous float32 torch tensor on the context's device:
    then torch's current stream is synchronised, the tensor's memory is read in place and a tensor is returned.  Blocks
    until the result is complete."""
    if ctx is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "stitch_lightmap needs a GPU context; there is no CPU fallback")
    items = [c if isinstance(c, LightmapChart) else LightmapChart(*c) for c in charts]
    c_charts = (_abi.LightmapChartC * max(1, len(items)))(*[_abi.LightmapChartC(int(c.instance_idx), c.scale_u, c.scale_v, c.offset_u, c.offset_v)
                                                           for c in items])
    info = _abi.LightmapStitchInfoC()
    if hasattr(rgba, "data_ptr"):   # a torch tensor
        import torch
        if not (rgba.is_cuda and rgba.dtype == torch.float32 and rgba.is_contiguous() and rgba.dim() == 3 and rgba.shape[2] == 4):
            raise ValueError("rgba must be a contiguous (height, width, 4) float32 tensor on the context's device")
        if rgba.device.index != ctx.device_ordinal:
            raise ValueError("rgba is on another device than the context")
        h, w = int(rgba.shape[0]), int(rgba.shape[1])
        out = torch.zeros((h, w, 4), dtype=torch.float32, device=rgba.device)
        torch.cuda.current_stream(rgba.device).synchronize()   # the input (and the zero fill) is written
        d = _abi.LightmapStitchDescC(w, h, int(iterations), float(samples_per_texel), float(lam), LIGHTMAP_STITCH_DEVICE_POINTERS, 0)
        check(lib().lupin_hip_stitch_lightmap(ctx.handle, scene.handle, C.byref(d), c_charts, len(items), C.c_void_p(rgba.data_ptr()),
                                              C.c_void_p(out.data_ptr()), C.byref(info)))
    else:
        rgba = np.ascontiguousarray(rgba, np.float32)
        if rgba.ndim != 3 or rgba.shape[2] != 4:
            raise ValueError("rgba must be (height, width, 4)")
        h, w = rgba.shape[:2]
        d = _abi.LightmapStitchDescC(w, h, int(iterations), float(samples_per_texel), float(lam), 0, 0)
        out = np.zeros((h, w, 4), np.float32)
        check(lib().lupin_hip_stitch_lightmap(ctx.handle, scene.handle, C.byref(d), c_charts, len(items), ptr(rgba), ptr(out), C.byref(info)))
    if not want_info:
        return out
    return out, {"seam_edges": int(info.seam_edges), "non_manifold_edges": int(info.non_manifold_edges), "sample_pairs": int(info.sample_pairs),
                 "dropped_pairs": int(info.dropped_pairs), "active_texels": int(info.active_texels), "iterations": int(info.iterations),
                 "energy_before": np.array(list(info.energy_before), np.float32), "energy_after": np.array(list(info.energy_after), np.float32)}


def lightmap_stitch_stats():
    """The calling thread's latest successful stitch_lightmap: host-clock ms of its phases (seam edges, sample pairs, the
    incidence lists, the solve with the output) and of the call."""
    s = _abi.LightmapStitchStatsC()
    check(lib().lupin_hip_lightmap_stitch_stats(C.byref(s)))
    return {k: float(getattr(s, k)) for k, _ in _abi.LightmapStitchStatsC._fields_}


# ---- light-probe baking: lupin_hip_bake_probes (include/lupin_hip.h) ----
PROBE_FLOATS = 4
PROBE_SH_COEFFS = 9
PROBE_RESULT_FLOATS = 36
PROBES_DEVICE_POINTERS = 1
SH_BAND_FACTORS = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)   # the clamped cosine's, per coefficient


@dataclass
class ProbeDesc:  # LupinProbeDesc
    pathtrace_type: int = PathtraceType.Standard
    max_bounces: int = 8
    samples: int = 1024
    flags: int = 0
    max_slots: int = 0       # paths per wavefront; 0 = the library's default
    advanced: AdvancedParams = field(default_factory=AdvancedParams)


def sh_basis(dirs):
    """(..., 9) float64: the real spherical harmonics of bands 0..2 at the unit vectors `dirs` (..., 3), in world x, y, z and
    in the order of include/lupin_hip.h -- 1, y, z, x, xy, yz, 3z^2 - 1, xz, x^2 - y^2, each with its normalisation."""
    d = np.asarray(dirs, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    k0, k1 = 0.5 * np.sqrt(1.0 / np.pi), np.sqrt(3.0 / (4.0 * np.pi))
    k2, k3, k4 = 0.5 * np.sqrt(15.0 / np.pi), 0.25 * np.sqrt(5.0 / np.pi), 0.25 * np.sqrt(15.0 / np.pi)
    return np.stack([np.full_like(x, k0), k1 * y, k1 * z, k1 * x, k2 * x * y, k2 * y * z, k3 * (3.0 * z * z - 1.0), k2 * x * z,
                     k4 * (x * x - y * y)], axis=-1)


def sh_irradiance(coeffs, normals):
    """Irradiance (..., 3) float64 at surfaces with unit `normals` (..., 3) from probe coefficients `coeffs` (..., 9, 3 or 4;
    only r, g, b are read): Ramamoorthi-Hanrahan, sum_j A_j coeffs[j] Y_j(n) with the clamped cosine's band factors
    A = pi, 2 pi / 3, pi / 4.  Exact for radiance that has no bands above 2.  Leading dimensions broadcast."""
    c = np.asarray(coeffs, np.float64)[..., :3]
    return np.einsum("...j,...jc->...c", sh_basis(normals) * SH_BAND_FACTORS, c)


def bake_probes(ctx, scene, positions, samples=1024, pathtrace_type=PathtraceType.Standard, max_bounces=8, advanced=None, counter=0,
                max_slots=0, want_rays=False):
    """Light probes at `positions` (n, 3): (n, 9, 4) float32, coefficient j of probe i as (r, g, b, w) -- the radiance arriving
    at the point over the whole sphere, path-traced along `samples` uniform directions and projected onto sh_basis on the
    device; L(w) ~ sum_j out[i, j, :3] * sh_basis(w)[j].  The w channel is the projection of the sample pattern itself
    (2 sqrt(pi), 0, ... for perfect sampling).  Probe i is seeded with rng_seed_for(i, counter).  With want_rays also the
    (n * samples, RAY_RECORD_FLOATS) first rays as mode-DIRECTION records of pathtrace_rays.  Blocks until complete."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "bake_probes needs a GPU context and an uploaded scene; there is no CPU fallback")
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    probes = np.zeros((len(pos), PROBE_FLOATS), np.float32)
    probes[:, :3] = pos
    probes.view(np.uint32)[:, 3] = rng_seed_for(np.arange(len(pos), dtype=np.uint32), counter)
    adv = advanced or AdvancedParams()
    c = _abi.ProbeDescC(int(pathtrace_type), int(max_bounces), int(samples), 0, int(max_slots),
                        _abi.AdvancedParamsC(adv.max_radiance, adv.rng_seed, adv.ray_epsilon))
    out = np.zeros((len(pos), PROBE_SH_COEFFS, 4), np.float32)
    rays = np.zeros((len(pos) * int(samples), RAY_RECORD_FLOATS), np.float32) if want_rays else None
    check(lib().lupin_hip_bake_probes(ctx.handle, scene.handle, C.byref(c), len(pos), ptr(probes), ptr(out), ptr(rays)))
    return (out, rays) if want_rays else out


# ---- occlusion queries: lupin_hip_occlusion_rays (include/lupin_hip.h) ----
OCCLUSION_RECORD_FLOATS = 8
OCCLUSION_DEVICE_POINTERS = 1


class OcclusionMode(enum.IntEnum):
    DIRECTION = 0            # floats 4..6 are the segment's unit direction; one slot per record
    COSINE_HEMISPHERE = 1    # floats 4..6 are a unit surface normal; `samples` cosine-weighted directions about it


def occlusion_records(ori, dir_or_normal, tmax=np.inf, rng=0):
    """(n, OCCLUSION_RECORD_FLOATS) float32 records for occlusion_rays: `ori` (n, 3); `dir_or_normal` (n, 3), the unit
    direction (mode DIRECTION) or the unit surface normal (mode COSINE_HEMISPHERE); `tmax` floats (inf: unbounded) and `rng`
    u32 states (stored as bits; ignored in direction mode), scalars or (n,) arrays."""
    ori = np.asarray(ori, np.float32).reshape(-1, 3)
    rec = np.zeros((len(ori), OCCLUSION_RECORD_FLOATS), np.float32)
    rec[:, 0:3] = ori
    rec[:, 4:7] = np.asarray(dir_or_normal, np.float32).reshape(-1, 3)
    rec.view(np.uint32)[:, 3] = np.asarray(rng, np.uint32)
    rec[:, 7] = np.asarray(tmax, np.float32)
    return rec


def _segment_query(name, np_dtype, torch_dtype, ctx, scene, records, mode, samples, ray_epsilon):
    """What occlusion_rays and transmittance_rays share: lupin_hip_<name> over numpy records (a `np_dtype` array comes back)
    or over a torch tensor in place (a tensor of torch's dtype named `torch_dtype`)."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), f"{name} needs a GPU context and an uploaded scene; there is no CPU fallback")
    fn = getattr(lib(), "lupin_hip_" + name)
    c = _abi.OcclusionDescC(int(mode), int(samples), 0, float(ray_epsilon))
    if hasattr(records, "data_ptr"):   # a torch tensor
        import torch
        t = records
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == OCCLUSION_RECORD_FLOATS):
            raise ValueError("records must be a contiguous (n, 8) float32 tensor on the context's device")
        if t.device.index != ctx.device_ordinal:
            raise ValueError("records are on another device than the context")
        out = torch.zeros((int(t.shape[0]),), dtype=getattr(torch, torch_dtype), device=t.device)
        torch.cuda.current_stream(t.device).synchronize()   # the records (and the zero fill) are written
        c.flags = OCCLUSION_DEVICE_POINTERS
        check(fn(ctx.handle, scene.handle, C.byref(c), int(t.shape[0]), C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())))
        return out
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, OCCLUSION_RECORD_FLOATS)
    out = np.zeros(len(rec), np_dtype)
    check(fn(ctx.handle, scene.handle, C.byref(c), len(rec), ptr(rec), ptr(out)))
    return out


def occlusion_rays(ctx, scene, records, mode=OcclusionMode.DIRECTION, samples=1, ray_epsilon=0.001):
    """Per record, the number of its `samples` slots whose segment is blocked (some triangle at ray_epsilon <= t < tmax):
    (n,) uint32.  Geometric visibility: opacity is not consulted.  `records` is an (n, OCCLUSION_RECORD_FLOATS) float32 numpy
    array (see occlusion_records), or a contiguous float32 torch tensor on the context's device: then torch's current stream
    is synchronised, the device memory is used in place and an int32 tensor is returned.  Blocks until complete."""
    return _segment_query("occlusion_rays", np.uint32, "int32", ctx, scene, records, mode, samples, ray_epsilon)


def occluded(ctx, scene, ori, dir_, tmax=np.inf, ray_epsilon=0.001):
    """(n,) bool: whether the segment from `ori` (n, 3) along the unit direction `dir_` (n, 3) is blocked before `tmax`."""
    return occlusion_rays(ctx, scene, occlusion_records(ori, dir_, tmax), OcclusionMode.DIRECTION, 1, ray_epsilon) != 0


def segment_records(p, q, ray_epsilon):
    """Direction-mode records of the segments p -> q ((n, 3) each), in float32: d = q - p, len = sqrt(dot(d, d)),
    dir = d / len, tmax = len - ray_epsilon (the far end point's own surface does not block).  ValueError for a pair with
    len <= 2 * ray_epsilon: nothing of such a segment lies between the two epsilons."""
    p, q = np.asarray(p, np.float32).reshape(-1, 3), np.asarray(q, np.float32).reshape(-1, 3)
    eps = np.float32(ray_epsilon)
    d = q - p
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=np.float32)
    if not np.all(length > np.float32(2.0) * eps):
        raise ValueError("segment_records: a segment is not longer than 2 * ray_epsilon")
    return occlusion_records(p, d / length[:, None], length - eps)


def visible(ctx, scene, p, q, ray_epsilon=0.001):
    """(n,) bool: whether nothing lies between the points p and q ((n, 3) each); see segment_records."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "visible needs a GPU context and an uploaded scene; there is no CPU fallback")
    return occlusion_rays(ctx, scene, segment_records(p, q, ray_epsilon), OcclusionMode.DIRECTION, 1, ray_epsilon) == 0


def transmittance_rays(ctx, scene, records, mode=OcclusionMode.DIRECTION, samples=1, ray_epsilon=0.001):
    """Per record, the SUM over its `samples` slots of the slot's transmittance T: (n,) float32; divide by
    `samples` for the mean.  T is the product of 1 - opacity over the surfaces at ray_epsilon <= t < tmax, 0 once a surface
    of opacity 1 is met: the expected result of the integrators' stochastic alpha skip along the segment.  `records` as
    occlusion_rays takes them: an (n, OCCLUSION_RECORD_FLOATS) float32 numpy array, or a contiguous float32 torch tensor on
    the context's device, used in place (a float32 tensor is returned).  Blocks until complete."""
    return _segment_query("transmittance_rays", np.float32, "float32", ctx, scene, records, mode, samples, ray_epsilon)


def transmittance(ctx, scene, p, q, ray_epsilon=0.001):
    """(n,) float32: the transmittance between the points p and q ((n, 3) each); see segment_records and transmittance_rays."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "transmittance needs a GPU context and an uploaded scene; there is no CPU fallback")
    return transmittance_rays(ctx, scene, segment_records(p, q, ray_epsilon), OcclusionMode.DIRECTION, 1, ray_epsilon)


def ambient_occlusion(ctx, scene, points, normals, radius, samples=64, ray_epsilon=0.001, counter=0, surface_offset=None, opacity=False):
    """Ambient occlusion (n,) float32 at `points` (n, 3) with unit `normals` (n, 3): 1 - blocked / samples over `samples`
    cosine-weighted directions per point, each tested up to `radius` (a scalar or (n,) array).  Point i is seeded with
    rng_seed_for(i, counter), as bake_irradiance seeds it.  The origins are the points moved along their normals by
    `surface_offset` world units (default: LIGHTMAP_OFFSET_FRACTION of the scene's extent, bake_lightmap's default).
    opacity=True: the mean transmittance of the same slots instead (transmittance_rays' sum / samples): alpha-textured,
    cut-out and half-transparent surfaces let through what the integrators let through on average."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "ambient_occlusion needs a GPU context and an uploaded scene; there is no CPU fallback")
    points = np.asarray(points, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    if surface_offset is None:
        surface_offset = LIGHTMAP_OFFSET_FRACTION * scene_world_extent(scene)
    rec = occlusion_records(points + normals * np.float32(surface_offset), normals, radius, rng_seed_for(np.arange(len(points), dtype=np.uint32), counter))
    if opacity:
        return transmittance_rays(ctx, scene, rec, OcclusionMode.COSINE_HEMISPHERE, samples, ray_epsilon) / np.float32(samples)
    blocked = occlusion_rays(ctx, scene, rec, OcclusionMode.COSINE_HEMISPHERE, samples, ray_epsilon)
    return np.float32(1.0) - blocked.astype(np.float32) / np.float32(samples)


# ---- bent-normal queries: lupin_hip_bent_normal_rays, lupin_hip_bake_lightmap_ao (include/lupin_hip.h) ----
BENT_NORMAL_RESULT_FLOATS = 4
BENT_NORMAL_DEVICE_POINTERS = 1
BENT_NORMAL_OPACITY = 2
BENT_NORMAL_MAX_SAMPLES = 1 << 20
LIGHTMAP_AO_OPACITY = 2


def bent_normal_rays(ctx, scene, records, samples, ray_epsilon=0.001, opacity=False, max_slots=0):
    """Per record, the four sums over its `samples` cosine-weighted slots (sum T d.x, sum T d.y, sum T d.z, sum T):
    (n, 4) float32.  T is 1 or 0 (the slot's segment is not / is blocked, as occlusion_rays decides), or with opacity=True
    the slot's transmittance (transmittance_rays' T).  [:, 3] / samples is the ambient-occlusion visibility, [:, :3]
    normalised the cosine-weighted bent normal; bent_normal_resolve does both.  `records` are occlusion_records read in
    OcclusionMode.COSINE_HEMISPHERE: an (n, OCCLUSION_RECORD_FLOATS) float32 numpy array, or a contiguous float32 torch
    tensor on the context's device: then torch's current stream is synchronised, the device memory is used in place and
    a float32 tensor is returned.  max_slots: slots per launch (0: the library's default); the words do not depend on it.
    Blocks until complete."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "bent_normal_rays needs a GPU context and an uploaded scene; there is no CPU fallback")
    c = _abi.BentNormalDescC(int(samples), BENT_NORMAL_OPACITY if opacity else 0, int(max_slots), float(ray_epsilon))
    if hasattr(records, "data_ptr"):   # a torch tensor
        import torch
        t = records
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == OCCLUSION_RECORD_FLOATS):
            raise ValueError("records must be a contiguous (n, 8) float32 tensor on the context's device")
        if t.device.index != ctx.device_ordinal:
            raise ValueError("records are on another device than the context")
        out = torch.zeros((int(t.shape[0]), BENT_NORMAL_RESULT_FLOATS), dtype=torch.float32, device=t.device)
        torch.cuda.current_stream(t.device).synchronize()   # the records (and the zero fill) are written
        c.flags |= BENT_NORMAL_DEVICE_POINTERS
        check(lib().lupin_hip_bent_normal_rays(ctx.handle, scene.handle, C.byref(c), int(t.shape[0]), C.c_void_p(t.data_ptr()),
                                               C.c_void_p(out.data_ptr())))
        return out
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, OCCLUSION_RECORD_FLOATS)
    out = np.zeros((len(rec), BENT_NORMAL_RESULT_FLOATS), np.float32)
    check(lib().lupin_hip_bent_normal_rays(ctx.handle, scene.handle, C.byref(c), len(rec), ptr(rec), ptr(out)))
    return out


def bent_normal_resolve(sums, samples, normals):
    """(ao (n,), bent (n, 3)) float32 from bent_normal_rays' sums, by the atlas bake's formulas in float32:
    ao = sums.w / samples;  len = sqrt((x*x + y*y) + z*z);  bent = sums.xyz / len, or the row of `normals` where len == 0."""
    a = np.asarray(sums, np.float32).reshape(-1, BENT_NORMAL_RESULT_FLOATS)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    ao = a[:, 3] / np.float32(samples)
    length = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2], dtype=np.float32)
    zero = length == np.float32(0.0)
    bent = a[:, :3] / np.where(zero, np.float32(1.0), length)[:, None]
    bent[zero] = normals[zero]
    return ao, bent


def bent_normals(ctx, scene, points, normals, radius, samples=64, ray_epsilon=0.001, counter=0, surface_offset=None, opacity=False):
    """(ao (n,), bent (n, 3)) float32 at `points` (n, 3) with unit `normals` (n, 3): the ambient-occlusion visibility
    ambient_occlusion returns, and the cosine-weighted mean unoccluded direction, unit length -- or the point's normal where
    nothing is open.  Seeds, offset default, `radius` and `opacity` are ambient_occlusion's: the two see the same slots."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "bent_normals needs a GPU context and an uploaded scene; there is no CPU fallback")
    points = np.asarray(points, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    if surface_offset is None:
        surface_offset = LIGHTMAP_OFFSET_FRACTION * scene_world_extent(scene)
    rec = occlusion_records(points + normals * np.float32(surface_offset), normals, radius, rng_seed_for(np.arange(len(points), dtype=np.uint32), counter))
    return bent_normal_resolve(bent_normal_rays(ctx, scene, rec, samples, ray_epsilon, opacity), samples, normals)


def bake_lightmap_ao(ctx, scene, charts, width, height, samples=64, max_distance=np.inf, ray_epsilon=0.001, counter=0, max_slots=0,
                     smooth_normals=False, opacity=False, dilate=0, surface_offset=None, want_bent=False, want_records=False, denoise=False):
    """An ambient-occlusion map in bake_lightmap's atlas: (height, width, 4) float32, rgb = the visibility (the share of
    `samples` cosine-weighted directions that are open up to `max_distance`; with opacity=True their mean transmittance),
    alpha 1 on rasterised texels and 0 elsewhere (gutter texels filled by `dilate` passes keep alpha 0).  charts,
    smooth_normals, counter, surface_offset and the records are bake_lightmap's: the same texels, the same records.
    want_bent: also the bent-normal map (height, width, 4): xyz = the cosine-weighted mean open direction, unit length on
    owned texels (the bake normal where nothing is open), not renormalised in the gutters.  want_records: also the
    (height, width, 8) records.  denoise: the visibility's owned texels are filtered by denoise_lightmap with its defaults,
    and its gutters are refilled from the filtered texels by `dilate` passes; the bent normals are not filtered.
    Returns ao, or (ao[, bent][, records]) in that order.  Blocks until the result is complete."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "bake_lightmap_ao needs a GPU context and an uploaded scene; there is no CPU fallback")
    if surface_offset is None:
        surface_offset = LIGHTMAP_OFFSET_FRACTION * (scene_world_extent(scene) or 1.0)
    items = [c if isinstance(c, LightmapChart) else LightmapChart(*c) for c in charts]
    c_charts = (_abi.LightmapChartC * max(1, len(items)))(*[_abi.LightmapChartC(int(c.instance_idx), c.scale_u, c.scale_v, c.offset_u, c.offset_v)
                                                           for c in items])
    flags = (LIGHTMAP_SMOOTH_NORMALS if smooth_normals else 0) | (LIGHTMAP_AO_OPACITY if opacity else 0)
    d = _abi.LightmapAoDescC(int(width), int(height), int(samples), int(max_slots), flags, int(dilate), int(counter), float(surface_offset),
                             float(max_distance), float(ray_epsilon))
    shape_ok = 0 < int(width) <= LIGHTMAP_MAX_SIZE and 0 < int(height) <= LIGHTMAP_MAX_SIZE
    hw = (int(height), int(width)) if shape_ok else (1, 1)      # a refused size: the library says so
    ao = np.zeros(hw + (4,), np.float32)
    bent = np.zeros(hw + (4,), np.float32) if want_bent else None
    rec = np.zeros(hw + (RAY_RECORD_FLOATS,), np.float32) if (want_records or denoise) else None
    check(lib().lupin_hip_bake_lightmap_ao(ctx.handle, scene.handle, C.byref(d), c_charts, len(items), ptr(ao), ptr(bent), ptr(rec), None))
    if denoise:   # (the filter reads owned texels only and refills the gutters itself)
        ao = denoise_lightmap(ctx, ao, rec, dilate=dilate)
    out = (ao,) + ((bent,) if want_bent else ()) + ((rec,) if want_records else ())
    return out if len(out) > 1 else ao


# ---- directional lightmaps: lupin_hip_bake_lightmap_directional (include/lupin_hip.h) ----
LIGHTMAP_DIRECTIONAL_PLANES = 4
SH_K0, SH_K1 = np.float32(0.28209479), np.float32(0.48860251)   # the header's literals for Y0 and Y1..Y3


def bake_lightmap_directional(ctx, scene, charts, width, height, samples=64, pathtrace_type=PathtraceType.Standard, max_bounces=8, advanced=None,
                              counter=0, max_slots=0, smooth_normals=False, dilate=0, surface_offset=None, want_records=False):
    """A directional lightmap in bake_lightmap's atlas: (4, height, width, 4) float32, plane j the L0 / L1 coefficient j
    (basis 1, y, z, x with sh_basis' normalisation) of the cosine-weighted incident radiance under each texel centre, rgb,
    with alpha 1 on rasterised texels and 0 elsewhere (gutter texels filled by `dilate` passes keep alpha 0).  Plane 0 / SH_K0
    is bake_lightmap's irradiance (the same paths, summed in another order); planes 1..3 / SH_K1 are that irradiance times
    the y, z, x of its mean direction.  Every argument is bake_lightmap's: the same texels, the same records, the same paths.
    render_lightmapped(..., directional=planes, bake_flags=...) shades normal maps from it.  With want_records also the
    (height, width, 8) records.  Blocks until the result is complete."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "bake_lightmap_directional needs a GPU context and an uploaded scene; there is no CPU fallback")
    if surface_offset is None:
        surface_offset = LIGHTMAP_OFFSET_FRACTION * (scene_world_extent(scene) or 1.0)
    adv = advanced or AdvancedParams()
    items = [c if isinstance(c, LightmapChart) else LightmapChart(*c) for c in charts]
    c_charts = (_abi.LightmapChartC * max(1, len(items)))(*[_abi.LightmapChartC(int(c.instance_idx), c.scale_u, c.scale_v, c.offset_u, c.offset_v)
                                                           for c in items])
    d = _abi.LightmapDescC(int(width), int(height), int(pathtrace_type), int(max_bounces), int(samples), int(max_slots),
                           LIGHTMAP_SMOOTH_NORMALS if smooth_normals else 0, int(dilate), int(counter), float(surface_offset),
                           _abi.AdvancedParamsC(adv.max_radiance, adv.rng_seed, adv.ray_epsilon))
    shape_ok = 0 < int(width) <= LIGHTMAP_MAX_SIZE and 0 < int(height) <= LIGHTMAP_MAX_SIZE
    hw = (int(height), int(width)) if shape_ok else (1, 1)      # a refused size: the library says so
    out = np.zeros((LIGHTMAP_DIRECTIONAL_PLANES,) + hw + (4,), np.float32)
    rec = np.zeros(hw + (RAY_RECORD_FLOATS,), np.float32) if want_records else None
    check(lib().lupin_hip_bake_lightmap_directional(ctx.handle, scene.handle, C.byref(d), c_charts, len(items), ptr(out), ptr(rec), None))
    return (out, rec) if want_records else out


def lightmap_directional_ratio(coeffs, n_shade, n_bake):
    """The factor render_lightmapped(..., directional=...) scales a lightmapped pixel's irradiance by, in numpy float32 and in
    the header's order of operations: `coeffs` (..., 4, 3 or 4) the fetched coefficients C0..C3 (only r, g, b are read),
    `n_shade` (..., 3) the pixel's shading normal n', `n_bake` (..., 3) the bake normal n_b.  Per channel
    num = ((C0 k0 + C1 (k1 n'.y)) + C2 (k1 n'.z)) + C3 (k1 n'.x), den the same with n_b; the ratio is max(num, 0) / den, and
    1 where den <= 0 or either is not finite.  (..., 3) float32; 0 <= ratio <= 4 for coefficients of non-negative radiance,
    and exactly 1 where n_shade == n_bake.  (The view also returns 1 on a back face, which only it can see.)"""
    c = np.asarray(coeffs, np.float32)[..., :3]
    one = np.float32(1.0)

    def project(n):
        n = np.asarray(n, np.float32)
        y1, y2, y3 = (SH_K1 * n[..., 1])[..., None], (SH_K1 * n[..., 2])[..., None], (SH_K1 * n[..., 0])[..., None]
        return ((c[..., 0, :] * SH_K0 + c[..., 1, :] * y1) + c[..., 2, :] * y2) + c[..., 3, :] * y3

    with np.errstate(all="ignore"):
        num, den = project(n_shade), project(n_bake)
        ok = np.isfinite(num) & np.isfinite(den) & ~(den <= 0)
        return np.where(ok, np.where(num > 0, num, np.float32(0.0)) / np.where(ok, den, one), one).astype(np.float32)


# ---- adaptive lightmap baking: lupin_hip_pathtrace_rays_moments, lupin_hip_bake_lightmap_adaptive (include/lupin_hip.h) ----
RAY_MOMENTS_FLOATS = 8
LIGHTMAP_ADAPTIVE_MAX_ROUNDS = 4096
LIGHTMAP_ADAPTIVE_STATS_FLOATS = 4
LIGHTMAP_ADAPTIVE_ROUND_STRIDE = 0x85EBCA6B


def lightmap_round_word(word, r):
    """RNG word of a lightmap record in round `r` of bake_lightmap_adaptive: the record's own for r == 0,
    hash_u32(word + r * 0x85EBCA6B) otherwise."""
    word = np.asarray(word, np.uint32)
    r = np.asarray(r, np.uint32)
    with np.errstate(over="ignore"):
        return np.where(r == 0, word, _hash_u32(word + r * np.uint32(LIGHTMAP_ADAPTIVE_ROUND_STRIDE))).astype(np.uint32)


def pathtrace_rays_moments(ctx, scene, records, desc: Optional[RayQueryDesc] = None):
    """pathtrace_rays with the moments of every record's desc.samples paths: (n, RAY_MOMENTS_FLOATS) float32 -- mean r, g, b,
    1, the mean luminance ml, M2 = the sum of (luminance - ml)^2 over the paths, float(samples), 0.  The same records, the same
    paths; the mean is summed in another order than pathtrace_rays' (include/lupin_hip.h).  `records` as pathtrace_rays
    takes them: a numpy array, or a contiguous float32 torch tensor on the context's device (then a tensor comes back)."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "pathtrace_rays_moments needs a GPU context and an uploaded scene; there is no CPU fallback")
    desc = desc or RayQueryDesc()
    flags = int(desc.flags)
    c = _abi.RayQueryDescC(int(desc.pathtrace_type), int(desc.max_bounces), int(desc.samples), flags, int(desc.max_slots),
                           _abi.AdvancedParamsC(desc.advanced.max_radiance, desc.advanced.rng_seed, desc.advanced.ray_epsilon))
    if hasattr(records, "data_ptr"):   # a torch tensor
        import torch
        t = records
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == RAY_RECORD_FLOATS):
            raise ValueError("records must be a contiguous (n, 8) float32 tensor on the context's device")
        if t.device.index != ctx.device_ordinal:
            raise ValueError("records are on another device than the context")
        n = int(t.shape[0])
        out = torch.zeros((n, RAY_MOMENTS_FLOATS), dtype=torch.float32, device=t.device)
        torch.cuda.current_stream(t.device).synchronize()   # the records (and the zero fill) are written
        c.flags = flags | RAYS_DEVICE_POINTERS
        check(lib().lupin_hip_pathtrace_rays_moments(ctx.handle, scene.handle, C.byref(c), n, C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())))
        return out
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, RAY_RECORD_FLOATS)
    out = np.zeros((len(rec), RAY_MOMENTS_FLOATS), np.float32)
    check(lib().lupin_hip_pathtrace_rays_moments(ctx.handle, scene.handle, C.byref(c), len(rec), ptr(rec), ptr(out)))
    return out


def lightmap_adaptive_stats():
    """The calling thread's latest successful bake_lightmap_adaptive: covered texels, rounds that traced, paths traced, texels
    that converged and texels the cap stopped, (chart, triangle) pairs, host-clock ms per phase summed over the rounds."""
    s = _abi.LightmapAdaptiveStatsC()
    lib().lupin_hip_lightmap_adaptive_stats(C.byref(s))
    return {"covered_texels": int(s.covered_texels), "rounds": int(s.rounds), "paths": int(s.paths), "converged_texels": int(s.converged_texels),
            "capped_texels": int(s.capped_texels), "keys": int(s.keys), "raster_ms": float(s.raster_ms), "compact_ms": float(s.compact_ms),
            "trace_ms": float(s.trace_ms), "merge_mask_ms": float(s.merge_mask_ms), "scatter_dilate_ms": float(s.scatter_dilate_ms),
            "download_ms": float(s.download_ms)}


def bake_lightmap_adaptive(ctx, scene, charts, width, height, samples_per_round=16, threshold=0.05, min_rounds=2, max_rounds=64,
                           pathtrace_type=PathtraceType.Standard, max_bounces=8, advanced=None, counter=0, max_slots=0, smooth_normals=False,
                           dilate=0, surface_offset=None, want_stats=False, want_records=False):
    """bake_lightmap in rounds of `samples_per_round` paths per texel: a texel takes at least min_rounds and at most max_rounds
    rounds and stops in between once the relative standard error of its luminance is below `threshold` and none of its eight
    atlas neighbours still wants samples.  (height, width, 4) float32 as bake_lightmap returns it; the other arguments are
    bake_lightmap's.  With want_stats also (height, width, 4) per-texel statistics, zeros where not rasterised: [0] the paths
    taken, [1] the relative standard error (+inf without an estimate), [2] the standard error of the irradiance's luminance,
    [3] 1 where the texel converged and 0 where the cap stopped it.  With want_records also the records.  The result is
    (rgba[, stats][, records]).  lightmap_adaptive_stats() has the call's totals.  Blocks until the result is complete."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "bake_lightmap_adaptive needs a GPU context and an uploaded scene; there is no CPU fallback")
    if surface_offset is None:
        surface_offset = LIGHTMAP_OFFSET_FRACTION * (scene_world_extent(scene) or 1.0)
    adv = advanced or AdvancedParams()
    items = [c if isinstance(c, LightmapChart) else LightmapChart(*c) for c in charts]
    c_charts = (_abi.LightmapChartC * max(1, len(items)))(*[_abi.LightmapChartC(int(c.instance_idx), c.scale_u, c.scale_v, c.offset_u, c.offset_v)
                                                           for c in items])
    d = _abi.LightmapDescC(int(width), int(height), int(pathtrace_type), int(max_bounces), int(samples_per_round), int(max_slots),
                           LIGHTMAP_SMOOTH_NORMALS if smooth_normals else 0, int(dilate), int(counter), float(surface_offset),
                           _abi.AdvancedParamsC(adv.max_radiance, adv.rng_seed, adv.ray_epsilon))
    a = _abi.LightmapAdaptiveDescC(float(threshold), int(min_rounds), int(max_rounds), 0)
    shape_ok = 0 < int(width) <= LIGHTMAP_MAX_SIZE and 0 < int(height) <= LIGHTMAP_MAX_SIZE
    hw = (int(height), int(width)) if shape_ok else (1, 1)      # a refused size: the library says so
    out = np.zeros(hw + (4,), np.float32)
    stats = np.zeros(hw + (LIGHTMAP_ADAPTIVE_STATS_FLOATS,), np.float32) if want_stats else None
    rec = np.zeros(hw + (RAY_RECORD_FLOATS,), np.float32) if want_records else None
    check(lib().lupin_hip_bake_lightmap_adaptive(ctx.handle, scene.handle, C.byref(d), C.byref(a), c_charts, len(items), ptr(out), ptr(stats), ptr(rec),
                                                 None))
    result = (out,) + ((stats,) if want_stats else ()) + ((rec,) if want_records else ())
    return result if len(result) > 1 else out


# ---- distance queries: lupin_hip_distance_points, lupin_hip_bake_distance_grid (include/lupin_hip.h) ----
DISTANCE_RECORD_FLOATS = 4
DISTANCE_RESULT_FLOATS = 12
DISTANCE_DEVICE_POINTERS = 1
DISTANCE_GRID_SIGNED = 2
# the twelve words of a result, as the header lists them
DISTANCE_RESULT_DTYPE = np.dtype([("found", np.uint32), ("distance", np.float32), ("point", np.float32, 3), ("u", np.float32), ("v", np.float32),
                                  ("instance", np.uint32), ("tri", np.uint32), ("side", np.float32), ("pad", np.uint32, 2)])
assert DISTANCE_RESULT_DTYPE.itemsize == 4 * DISTANCE_RESULT_FLOATS


def distance_records(points, rmax=np.inf):
    """(n, DISTANCE_RECORD_FLOATS) float32 records for distance_points: `points` (n, 3); `rmax` the search radius, a scalar
    or an (n,) array (inf: unbounded)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    rec = np.zeros((len(points), DISTANCE_RECORD_FLOATS), np.float32)
    rec[:, 0:3] = points
    rec[:, 3] = np.asarray(rmax, np.float32)
    return rec


def distance_points(ctx, scene, records):
    """The nearest surface point of every record (see distance_records): an (n,) array of DISTANCE_RESULT_DTYPE -- found,
    distance, point, the barycentrics u, v, instance, tri (as trace_rays reports it) and side, the sign of dot(p - point, n) for
    the REPORTED triangle's world-space normal (v1 - v0) x (v2 - v0): not an inside / outside classification.  `records` is
    an (n, DISTANCE_RECORD_FLOATS) float32 numpy array, or a contiguous float32 torch tensor on the context's device: then
    torch's current stream is synchronised, the device memory is used in place and an (n, DISTANCE_RESULT_FLOATS) float32
    tensor of the same words is returned.  Blocks until complete."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "distance_points needs a GPU context and an uploaded scene; there is no CPU fallback")
    if hasattr(records, "data_ptr"):   # a torch tensor
        import torch
        t = records
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == DISTANCE_RECORD_FLOATS):
            raise ValueError("records must be a contiguous (n, 4) float32 tensor on the context's device")
        if t.device.index != ctx.device_ordinal:
            raise ValueError("records are on another device than the context")
        out = torch.zeros((int(t.shape[0]), DISTANCE_RESULT_FLOATS), dtype=torch.float32, device=t.device)
        torch.cuda.current_stream(t.device).synchronize()   # the records (and the zero fill) are written
        check(lib().lupin_hip_distance_points(ctx.handle, scene.handle, DISTANCE_DEVICE_POINTERS, int(t.shape[0]), C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())))
        return out
    rec = np.ascontiguousarray(records, np.float32).reshape(-1, DISTANCE_RECORD_FLOATS)
    out = np.zeros((len(rec), DISTANCE_RESULT_FLOATS), np.float32)
    check(lib().lupin_hip_distance_points(ctx.handle, scene.handle, 0, len(rec), ptr(rec), ptr(out)))
    return out.view(DISTANCE_RESULT_DTYPE).reshape(-1)


def nearest_distance(ctx, scene, points, rmax=np.inf):
    """(n,) float32: the distance from `points` (n, 3) to the nearest surface; inf where nothing lies within `rmax`."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "nearest_distance needs a GPU context and an uploaded scene; there is no CPU fallback")
    res = distance_points(ctx, scene, distance_records(points, rmax))
    return np.where(res["found"] != 0, res["distance"], np.float32(np.inf)).astype(np.float32)


def grid_centres(origin, spacing, dims):
    """The voxel centres of bake_distance_grid, (nz, ny, nx, 3) float32, by the stated f32 expression per axis:
    origin + (float32(i) + 0.5) * spacing, the product first."""
    origin, spacing = np.asarray(origin, np.float32).reshape(3), np.asarray(spacing, np.float32).reshape(3)
    axes = [origin[k] + (np.arange(int(dims[k]), dtype=np.float32) + np.float32(0.5)) * spacing[k] for k in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x, y, z], -1).astype(np.float32)


def bake_distance_grid(ctx, scene, origin, spacing, dims, rmax=np.inf, signed=False):
    """A (nz, ny, nx) float32 volume of distances to the nearest surface at the voxel centres of grid_centres(origin,
    spacing, dims) (dims = (nx, ny, nz)), computed on the device; `rmax` (clamped to the largest float) where nothing lies
    within `rmax`.  signed: a found distance is multiplied by distance_points' `side` (0 where side is 0) -- the side of the
    nearest TRIANGLE, not a true signed distance."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "bake_distance_grid needs a GPU context and an uploaded scene; there is no CPU fallback")
    o = (C.c_float * 3)(*[float(x) for x in np.asarray(origin, np.float32).reshape(3)])
    s = (C.c_float * 3)(*[float(x) for x in np.asarray(spacing, np.float32).reshape(3)])
    nx, ny, nz = (int(d) for d in dims)
    d = (C.c_uint32 * 3)(nx, ny, nz)
    out = np.zeros((nz, ny, nx), np.float32)
    check(lib().lupin_hip_bake_distance_grid(ctx.handle, scene.handle, DISTANCE_GRID_SIGNED if signed else 0, o, s, d, float(np.float32(rmax)), ptr(out)))
    return out


def surface_clearance(ctx, scene, points, normals, offset):
    """(n,) float32: the distance to the nearest surface from `points` + `offset` * `normals` ((n, 3) each, float32
    arithmetic; `offset` a scalar or (n,) array) -- what a caller looks at to choose a bake offset locally: a clearance below
    the offset says that another surface is nearer to the moved point than the one it was moved off."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "surface_clearance needs a GPU context and an uploaded scene; there is no CPU fallback")
    points = np.asarray(points, np.float32).reshape(-1, 3)
    normals = np.asarray(normals, np.float32).reshape(-1, 3)
    offset = np.asarray(offset, np.float32).reshape(-1, 1)
    return nearest_distance(ctx, scene, points + normals * offset)


# ---- irradiance volume lookup: lupin_hip_sample_probe_grid (include/lupin_hip.h) ----
PROBE_GRID_RECORD_FLOATS = 8
PROBE_GRID_RESULT_FLOATS = 4
PROBE_GRID_DEVICE_POINTERS = 1
PROBE_GRID_VISIBILITY = 2
PROBE_GRID_BACKFACE = 4


def probe_grid_positions(origin, spacing, dims):
    """The probe positions of a grid, (P, 3) float32 in index order (x fastest: probe (ix, iy, iz) has index
    ix + nx * (iy + ny * iz)), by the stated f32 expression per axis: origin + float32(i) * spacing, the product first.
    Probe positions, not voxel centres: there is no + 0.5."""
    origin, spacing = np.asarray(origin, np.float32).reshape(3), np.asarray(spacing, np.float32).reshape(3)
    axes = [origin[k] + np.arange(int(dims[k]), dtype=np.float32) * spacing[k] for k in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x, y, z], -1).astype(np.float32).reshape(-1, 3)


def bake_probe_grid(ctx, scene, origin, spacing, dims, **bake_probes_kwargs):
    """(positions (P, 3), sh (P, 9, 4)) float32: one bake_probes call at probe_grid_positions(origin, spacing, dims), with
    bake_probes' keyword arguments.  No validity judgement is made: which probes may be used (inside geometry, too close
    to a wall) is the caller's, with occlusion_rays and distance_points to decide it by."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "bake_probe_grid needs a GPU context and an uploaded scene; there is no CPU fallback")
    if bake_probes_kwargs.get("want_rays"):
        raise ValueError("bake_probe_grid returns positions and coefficients only; call bake_probes for the first rays")
    pos = probe_grid_positions(origin, spacing, dims)
    return pos, bake_probes(ctx, scene, pos, **bake_probes_kwargs)


def probe_grid_records(points, normals):
    """(n, PROBE_GRID_RECORD_FLOATS) float32 records for sample_probe_grid: `points` (n, 3) and unit `normals` (n, 3)."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    rec = np.zeros((len(points), PROBE_GRID_RECORD_FLOATS), np.float32)
    rec[:, 0:3] = points
    rec[:, 4:7] = np.asarray(normals, np.float32).reshape(-1, 3)
    return rec


def _probe_grid_arrays(ctx, scene, origin, spacing, dims, flags, ray_epsilon, normal_bias, sh, depth, valid, records=None):
    """What every consumer of a probe grid does alike with the grid itself (the two lookups through _probe_grid_lookup, and
    render_baked): the grid's descriptor, and `sh`, `depth`, `valid` as the entry point takes them -- torch tensors through
    the gate and in place, arrays converted.  `records`: the lookups' batch, which must be a tensor exactly when `sh` is.
    Returns (grid, R, tensors, sh, depth, valid): tensors says that the arguments are device pointers (the caller sets its
    entry point's DEVICE_POINTERS flag, and synchronises torch's current stream once its outputs are allocated).  The
    pointers of converted arrays keep those arrays alive (ndarray.ctypes.data_as does)."""
    if normal_bias is None:
        normal_bias = LIGHTMAP_OFFSET_FRACTION * scene_world_extent(scene)
    nx, ny, nz = (int(d) for d in dims)
    P = nx * ny * nz
    R = None
    if depth is not None:
        if len(depth.shape) != 4 or depth.shape[1] != depth.shape[2] or depth.shape[1] < 3:
            raise ValueError("depth must be (P, R + 2, R + 2, 2)")
        R = int(depth.shape[1]) - 2
    grid = _abi.ProbeGridDescC((C.c_float * 3)(*[float(x) for x in np.asarray(origin, np.float32).reshape(3)]),
                               (C.c_float * 3)(*[float(x) for x in np.asarray(spacing, np.float32).reshape(3)]),
                               (C.c_uint32 * 3)(nx, ny, nz), flags, float(ray_epsilon), float(np.float32(normal_bias)))
    arrays = tuple(x for x in (records, sh, depth) if x is not None)
    if any(hasattr(x, "data_ptr") for x in arrays):   # torch tensors
        import torch
        if not all(hasattr(x, "data_ptr") for x in arrays):
            names = ["sh"] + (["depth"] if depth is not None else []) + (["records"] if records is not None else [])
            raise ValueError(" and ".join(names) + " must all be torch tensors, or none of them")
        if not (sh.is_cuda and sh.dtype == torch.float32 and sh.is_contiguous() and tuple(sh.shape) == (P, PROBE_SH_COEFFS, 4)):
            raise ValueError("sh must be a contiguous (P, 9, 4) float32 tensor on the context's device")
        if depth is not None and not (depth.is_cuda and depth.dtype == torch.float32 and depth.is_contiguous() and
                                      tuple(depth.shape) == (P, R + 2, R + 2, 2)):
            raise ValueError("depth must be a contiguous (P, R + 2, R + 2, 2) float32 tensor on the context's device")
        if valid is not None and not (hasattr(valid, "data_ptr") and valid.is_cuda and valid.dtype in (torch.uint8, torch.bool) and
                                      valid.is_contiguous() and valid.numel() == P):
            raise ValueError("valid must be a contiguous uint8 or bool tensor of P elements on the context's device")
        if any(x.device.index != ctx.device_ordinal for x in arrays + (() if valid is None else (valid,))):
            raise ValueError("a tensor is on another device than the context")
        dev = lambda x: None if x is None else C.c_void_p(x.data_ptr())
        return grid, R, True, dev(sh), dev(depth), dev(valid)
    sh = np.ascontiguousarray(sh, np.float32)
    if sh.shape != (P, PROBE_SH_COEFFS, 4):
        raise ValueError(f"sh must be ({P}, 9, 4) for dims {(nx, ny, nz)}")
    if depth is not None:
        depth = np.ascontiguousarray(depth, np.float32)
        if depth.shape != (P, R + 2, R + 2, 2):
            raise ValueError(f"depth must be ({P}, R + 2, R + 2, 2) for dims {(nx, ny, nz)}")
    v = None
    if valid is not None:
        v = np.ascontiguousarray(np.asarray(valid).reshape(-1) != 0, np.uint8)
        if v.shape != (P,):
            raise ValueError(f"valid must have {P} elements for dims {(nx, ny, nz)}")
    return grid, R, False, ptr(sh), ptr(depth), ptr(v)


def _probe_grid_lookup(ctx, scene, origin, spacing, dims, flags, ray_epsilon, normal_bias, sh, depth, points_or_records, normals, valid, call):
    """What sample_probe_grid and sample_probe_grid_depth (the one with `depth`) do alike, which is all but the entry point:
    _probe_grid_arrays, the records and the output.  call(grid, R, sh, depth, valid, n, records, out) gets the descriptor
    and what the entry point takes for the arrays, and returns its code."""
    t = points_or_records
    if hasattr(t, "data_ptr"):   # torch tensors
        import torch
        if normals is not None:
            raise ValueError("tensor records carry their normals: (n, 8)")
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 2 and t.shape[1] == PROBE_GRID_RECORD_FLOATS):
            raise ValueError("records must be a contiguous (n, 8) float32 tensor on the context's device")
        grid, R, _, d_sh, d_depth, d_valid = _probe_grid_arrays(ctx, scene, origin, spacing, dims, flags, ray_epsilon, normal_bias, sh, depth, valid, t)
        out = torch.zeros((int(t.shape[0]), PROBE_GRID_RESULT_FLOATS), dtype=torch.float32, device=t.device)
        torch.cuda.current_stream(t.device).synchronize()   # the inputs (and the zero fill) are written
        grid.flags |= PROBE_GRID_DEVICE_POINTERS
        check(call(grid, R, d_sh, d_depth, d_valid, int(t.shape[0]), C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr())))
        return out
    if normals is not None:
        rec = probe_grid_records(points_or_records, normals)
    else:
        rec = np.ascontiguousarray(points_or_records, np.float32).reshape(-1, PROBE_GRID_RECORD_FLOATS)
    grid, R, tensors, p_sh, p_depth, p_valid = _probe_grid_arrays(ctx, scene, origin, spacing, dims, flags, ray_epsilon, normal_bias, sh, depth, valid, rec)
    out = np.zeros((len(rec), PROBE_GRID_RESULT_FLOATS), np.float32)
    check(call(grid, R, p_sh, p_depth, p_valid, len(rec), ptr(rec), ptr(out)))
    return out


def sample_probe_grid(ctx, scene, origin, spacing, dims, sh, points_or_records, normals=None, valid=None, visibility=True, backface=True,
                      ray_epsilon=0.001, normal_bias=None):
    """Irradiance from a grid of baked probes: (n, 4) float32, (r, g, b, w) per shading point -- the trilinear blend of the
    cell's eight probes' sh_irradiance at the normal, over the probes that may be used, and the weight w that survived
    (w == 0: none of the cell's probes may be used, r = g = b = 0; the fallback is the caller's).  `sh` is (P, 9, 4), what
    bake_probe_grid returns; `valid` None or (P,) with zeros at the probes not to use; visibility drops the probes the
    scene's geometry hides from the point (light does not leak through walls), backface weighs down the probes behind the
    surface.  The point is first moved along its normal by `normal_bias` world units (None: LIGHTMAP_OFFSET_FRACTION of the
    scene's extent, ambient_occlusion's default).  `points_or_records` is (n, 3) points with `normals` (n, 3), or (n, 8)
    records (see probe_grid_records).  With a contiguous float32 torch tensor on the context's device for `sh` and for the
    records, torch's current stream is synchronised, the device memory is used in place (`valid`, if given, a uint8 or bool
    tensor there) and a tensor is returned.  Blocks until complete."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "sample_probe_grid needs a GPU context and an uploaded scene; there is no CPU fallback")
    flags = (PROBE_GRID_VISIBILITY if visibility else 0) | (PROBE_GRID_BACKFACE if backface else 0)
    fn = lib().lupin_hip_sample_probe_grid
    return _probe_grid_lookup(ctx, scene, origin, spacing, dims, flags, ray_epsilon, normal_bias, sh, None, points_or_records, normals, valid,
                              lambda grid, R, sh, depth, valid, n, rec, out: fn(ctx.handle, scene.handle, C.byref(grid), sh, valid, n, rec, out))


# ---- probe depth maps: lupin_hip_bake_probe_depth, lupin_hip_sample_probe_grid_depth (include/lupin_hip.h) ----
PROBE_DEPTH_DEVICE_POINTERS = 1
PROBE_DEPTH_STATS_WORDS = 4
PROBE_DEPTH_MIN_RESOLUTION, PROBE_DEPTH_MAX_RESOLUTION = 2, 64
PROBE_DEPTH_DEFAULT_MAX_SLOTS = 1 << 24


@dataclass
class ProbeDepthDesc:  # LupinProbeDepthDesc
    resolution: int = 16
    subsamples: int = 4
    flags: int = 0
    max_slots: int = 0       # rays per launch; 0 = the library's default
    ray_epsilon: float = 0.001
    max_distance: float = 1.0


def _oct_sgn(x):
    return np.where(x < 0, np.float32(-1.0), np.float32(1.0))   # sgn(0) = +1


def oct_decode(uv):
    """(..., 3) float32 unit vectors from octahedral coordinates `uv` (..., 2) in [-1, 1]^2, by the header's f32 expressions:
    z = (1 - |u|) - |v|; below the fold (z < 0) x = (1 - |v|) sgn(u), y = (1 - |u|) sgn(v); then the division by the length."""
    uv = np.asarray(uv, np.float32)
    u, v = uv[..., 0], uv[..., 1]
    one = np.float32(1.0)
    z = (one - np.abs(u)) - np.abs(v)
    x = np.where(z < 0, (one - np.abs(v)) * _oct_sgn(u), u)
    y = np.where(z < 0, (one - np.abs(u)) * _oct_sgn(v), v)
    ln = np.sqrt((x * x + y * y) + z * z)
    return np.stack([x / ln, y / ln, z / ln], axis=-1)


def oct_encode(dirs):
    """(..., 2) float32 octahedral coordinates in [-1, 1]^2 of the directions `dirs` (..., 3) (any non-zero length), by the
    header's f32 expressions: the division by the 1-norm, then the fold for z < 0 from the unfolded pair."""
    e = np.asarray(dirs, np.float32)
    one = np.float32(1.0)
    s = (np.abs(e[..., 0]) + np.abs(e[..., 1])) + np.abs(e[..., 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        px, py = e[..., 0] / s, e[..., 1] / s
    fx, fy = (one - np.abs(py)) * _oct_sgn(px), (one - np.abs(px)) * _oct_sgn(py)
    below = e[..., 2] < 0
    return np.stack([np.where(below, fx, px), np.where(below, fy, py)], axis=-1)


def bake_probe_depth(ctx, scene, positions, resolution=16, subsamples=4, *, max_distance, ray_epsilon=0.001, want_stats=False, max_slots=0):
    """Octahedral distance moments of the probes at `positions` (n, 3): (n, R + 2, R + 2, 2) float32, texel [ty + 1, tx + 1] the
    (mean, mean square) over subsamples^2 rays of the distance to the nearest surface in the texel's directions, capped at
    `max_distance` (a miss counts as max_distance); the one-texel border repeats the texels across the octahedral seams, so
    that plain bilinear filtering needs no special case.  With want_stats also (n, 4) uint32: rays, hits, hits on a back
    face, the bits of the smallest distance.  Blocks until complete."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "bake_probe_depth needs a GPU context and an uploaded scene; there is no CPU fallback")
    pos = np.asarray(positions, np.float32).reshape(-1, 3)
    rec = np.zeros((len(pos), 4), np.float32)
    rec[:, :3] = pos
    R = int(resolution)
    c = _abi.ProbeDepthDescC(R, int(subsamples), 0, int(max_slots), float(ray_epsilon), float(np.float32(max_distance)))
    side = max(R, 0) + 2
    out = np.zeros((len(pos), side, side, 2), np.float32)
    stats = np.zeros((len(pos), PROBE_DEPTH_STATS_WORDS), np.uint32) if want_stats else None
    check(lib().lupin_hip_bake_probe_depth(ctx.handle, scene.handle, C.byref(c), len(pos), ptr(rec), ptr(out), ptr(stats)))
    return (out, stats) if want_stats else out


def probe_grid_depth_max_distance(spacing):
    """The default cap of a grid's depth maps, float32: 1.5 |spacing|, the longest segment of a cell plus margin."""
    return np.float32(1.5 * np.linalg.norm(np.asarray(spacing, np.float32).reshape(3).astype(np.float64)))


def bake_probe_grid_depth(ctx, scene, origin, spacing, dims, resolution=16, subsamples=4, max_distance=None, **bake_probe_depth_kwargs):
    """(positions (P, 3), depth (P, R + 2, R + 2, 2), max_distance) -- and the stats with want_stats: one bake_probe_depth call at
    probe_grid_positions(origin, spacing, dims).  max_distance None: probe_grid_depth_max_distance(spacing).  Hand depth and
    max_distance to sample_probe_grid_depth."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "bake_probe_grid_depth needs a GPU context and an uploaded scene; there is no CPU fallback")
    if max_distance is None:
        max_distance = probe_grid_depth_max_distance(spacing)
    max_distance = np.float32(max_distance)
    pos = probe_grid_positions(origin, spacing, dims)
    got = bake_probe_depth(ctx, scene, pos, resolution, subsamples, max_distance=max_distance, **bake_probe_depth_kwargs)
    if bake_probe_depth_kwargs.get("want_stats"):
        return pos, got[0], max_distance, got[1]
    return pos, got, max_distance


def sample_probe_grid_depth(ctx, scene, origin, spacing, dims, sh, depth, points_or_records, normals=None, *, max_distance, valid=None,
                            backface=True, normal_bias=None):
    """sample_probe_grid with the visibility taken from baked depth maps instead of the scene: (n, 4) float32 (r, g, b, w).
    `depth` is (P, R + 2, R + 2, 2), what bake_probe_grid_depth returns, and `max_distance` the bake's.  A corner whose probe
    sees, in the direction of the point, a mean distance shorter than the point's is weighed by the cube of Chebyshev's
    bound var / (var + (r - mean)^2); the scene's geometry is not read.  Everything else is sample_probe_grid's, the torch
    tensor form included (then `depth` is a tensor as well)."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), "sample_probe_grid_depth needs a GPU context and an uploaded scene; there is no CPU fallback")
    fn = lib().lupin_hip_sample_probe_grid_depth
    md = float(np.float32(max_distance))
    return _probe_grid_lookup(ctx, scene, origin, spacing, dims, PROBE_GRID_BACKFACE if backface else 0, 0.0, normal_bias, sh, depth, points_or_records,
                              normals, valid, lambda grid, R, sh, depth, valid, n, rec, out: fn(
                                  ctx.handle, scene.handle, C.byref(_abi.ProbeGridDepthDescC(grid, R, md)), sh, depth, valid, n, rec, out))


# ---- baked-lighting view: lupin_hip_render_baked (include/lupin_hip.h) ----
BAKED_VIEW_GBUFFER_FLOATS = 16
BAKED_VIEW_MISS = 0xFFFFFFFF
BAKED_VIEW_DEVICE_POINTERS = 1
BAKED_VIEW_DEFAULT_MAX_SLOTS = 1 << 20


def render_baked(ctx, scene, render_target, camera_params, camera_transform, origin, spacing, dims, sh, depth=None, max_distance=None, valid=None,
                 ambient=(0.0, 0.0, 0.0), visibility=False, backface=True, ray_epsilon=0.001, normal_bias=None, want_gbuffer=False, max_slots=0):
    """A camera view of a baked irradiance volume into `render_target`: per pixel the primary hit through the pixel's centre,
    then emission + color / pi * E(p, n), with E from sample_probe_grid's lookup (depth None; `visibility` traces the corners'
    segments) or from sample_probe_grid_depth's (`depth` and `max_distance` as bake_probe_grid_depth returns them); a miss
    shows the environment, and where no probe answers E is `ambient`.  Every material is drawn as a matte surface of its
    colour; the normal is turned to the viewer's side.  `camera_transform` is a (4, 3) LupinMat3x4 as PathtraceDesc carries
    it; grid, `sh`, `valid`, `backface` and `normal_bias` are sample_probe_grid's, the torch tensor form included (then
    `depth` is a tensor as well).  `ray_epsilon` is the primary ray's and the segments'.  With want_gbuffer the (H, W, 16)
    float32 G-buffer is returned (p | instance bits, n | triangle bits, color | w, emission | dst; a tensor where `sh` is
    one); otherwise None.  The picture does not depend on `max_slots` (pixels per launch).  Blocks until complete."""
    c, tensors, p_sh, p_depth, p_valid = _baked_view_desc("render_baked", ctx, scene, render_target, camera_params, camera_transform, origin, spacing, dims,
                                                          sh, depth, max_distance, valid, ambient, visibility, backface, ray_epsilon, normal_bias, max_slots)
    gbuffer, gb = _baked_view_gbuffer(render_target, BAKED_VIEW_GBUFFER_FLOATS, want_gbuffer, sh if tensors else None)
    check(lib().lupin_hip_render_baked(ctx.handle, scene.handle, render_target.handle, C.byref(c), p_sh, p_depth, p_valid, gb))
    return gbuffer


def _baked_view_desc(who, ctx, scene, render_target, camera_params, camera_transform, origin, spacing, dims, sh, depth, max_distance, valid, ambient,
                     visibility, backface, ray_epsilon, normal_bias, max_slots):
    """What render_baked and render_lightmapped do alike before their entry points: the no-device and target checks, and the
    LupinBakedViewDesc with the volume's arrays through _probe_grid_arrays.  `sh` None (render_lightmapped only): no volume,
    a zero grid.  Returns (desc, tensors, sh, depth, valid) as _probe_grid_arrays returns them; desc.flags says DEVICE_POINTERS
    where tensors."""
    if ctx is None or scene.handle is None:
        raise LupinError(_abi_code("LUPIN_ERR_NO_DEVICE"), f"{who} needs a GPU context and an uploaded scene; there is no CPU fallback")
    if render_target.format() != "Rgba16Float":
        raise LupinError(-1, f"{who}: the render target must be Rgba16Float")
    if depth is not None and max_distance is None:
        raise ValueError("depth maps come with the max_distance of their bake")
    cp = camera_params
    cam = _abi.CameraParamsC(1 if cp.is_orthographic else 0, cp.lens, cp.film, cp.aspect, cp.focus, cp.aperture)
    mat = _abi.Mat3x4()
    m = np.asarray(camera_transform, np.float32).reshape(4, 3)
    for col in range(4):
        for row in range(3):
            mat.m[col][row] = float(m[col][row])
    amb = (C.c_float * 3)(*[float(x) for x in np.asarray(ambient, np.float32).reshape(3)])
    md = 0.0 if max_distance is None else float(np.float32(max_distance))
    if sh is None:
        if depth is not None or valid is not None:
            raise ValueError("depth and valid belong to a volume: give sh")
        grid, R, tensors, p_sh, p_depth, p_valid = _abi.ProbeGridDescC(), None, False, None, None, None
    else:
        flags = (PROBE_GRID_VISIBILITY if visibility else 0) | (PROBE_GRID_BACKFACE if backface else 0)
        grid, R, tensors, p_sh, p_depth, p_valid = _probe_grid_arrays(ctx, scene, origin, spacing, dims, flags, ray_epsilon, normal_bias, sh, depth, valid)
    c = _abi.BakedViewDescC(cam, mat, grid, R or 0, md, float(ray_epsilon), amb, BAKED_VIEW_DEVICE_POINTERS if tensors else 0, int(max_slots))
    return c, tensors, p_sh, p_depth, p_valid


def _baked_view_gbuffer(render_target, floats, want_gbuffer, tensor):
    """(gbuffer or None, its pointer or None) for a view: zeros of (H, W, floats), a torch tensor beside `tensor` where that
    is one (then torch's current stream is synchronised: the inputs and the zero fill are written), a numpy array otherwise."""
    H, W = render_target.height, render_target.width
    gbuffer, gb = None, None
    if tensor is not None:
        import torch
        if want_gbuffer:
            gbuffer = torch.zeros((H, W, floats), dtype=torch.float32, device=tensor.device)
            gb = C.c_void_p(gbuffer.data_ptr())
        torch.cuda.current_stream(tensor.device).synchronize()
    elif want_gbuffer:
        gbuffer = np.zeros((H, W, floats), np.float32)
        gb = ptr(gbuffer)
    return gbuffer, gb


# ---- lightmapped view: lupin_hip_render_lightmapped (include/lupin_hip.h) ----
LIGHTMAPPED_VIEW_GBUFFER_FLOATS = 20
LIGHTMAPPED_SOURCE_MISS, LIGHTMAPPED_SOURCE_LIGHTMAP, LIGHTMAPPED_SOURCE_PROBES, LIGHTMAPPED_SOURCE_AMBIENT = 0, 1, 2, 3
LIGHTMAPPED_DIRECTIONAL_GBUFFER_FLOATS = 24   # lupin_hip_render_lightmapped_directional
LIGHTMAPPED_DIRECTIONAL_APPLIED, LIGHTMAPPED_DIRECTIONAL_BACK_FACE = 1, 2
LIGHTMAPPED_DIRECTIONAL_DEN_NOT_POSITIVE, LIGHTMAPPED_DIRECTIONAL_NOT_FINITE = 4, 8


def render_lightmapped(ctx, scene, render_target, camera_params, camera_transform, charts, lightmap, *, origin=None, spacing=None, dims=None, sh=None,
                       depth=None, max_distance=None, valid=None, ambient=(0.0, 0.0, 0.0), visibility=False, backface=True, ray_epsilon=0.001,
                       normal_bias=None, want_gbuffer=False, max_slots=0, directional=None, bake_flags=0):
    """A camera view of baked lighting into `render_target`: render_baked with a lightmap as the irradiance source wherever
    the hit instance has a chart, and the irradiance volume (or `ambient`) as the fallback.  `charts` are the LightmapChart
    items the atlas was baked with and `lightmap` is the (height, width, 4) float32 atlas bake_lightmap or denoise_lightmap
    returned: E is its bilinear fetch at the hit's texcoords over the texels a chart owns (alpha != 0), renormalised by
    their coverage, or the plain bilinear fetch where none of the four is owned (the gutter).  A hit without a chart takes
    E from the volume exactly as render_baked does when `sh` is given (with `origin`, `spacing`, `dims`, and `depth`,
    `max_distance`, `valid`, `visibility`, `backface`, `normal_bias` as there), and `ambient` otherwise.  With torch tensors
    `lightmap` is a contiguous float32 tensor on the context's device, and so is `sh` if given.  With want_gbuffer the
    (H, W, 20) float32 G-buffer is returned: render_baked's 16 words ([11]: the owned coverage on a lightmapped pixel, the
    lookup's w on a probe pixel), then the atlas coordinate x, y in texels, the chart index bits (BAKED_VIEW_MISS: none) and
    the LIGHTMAPPED_SOURCE_* bits.  The picture does not depend on `max_slots`.  Blocks until complete.
    With `directional`, the (4, height, width, 4) planes bake_lightmap_directional returned for the same atlas and charts (a
    tensor where `lightmap` is one), and `bake_flags`, that bake's flags (0, or LIGHTMAP_SMOOTH_NORMALS for smooth_normals=True),
    a lightmapped pixel's E is scaled per channel by lightmap_directional_ratio(fetched coefficients, the pixel's shading
    normal, the bake normal at the hit), so normal maps and smooth-shaded meshes show in the baked view; a pixel seen from
    its back face is not scaled.  The G-buffer then has 24 words: [20..22] the ratio (1 where none was applied) and [23] the
    LIGHTMAPPED_DIRECTIONAL_* bits.  Without `directional` the call and its picture are what they were."""
    if sh is not None and (origin is None or spacing is None or dims is None):
        raise ValueError("a volume comes with its origin, spacing and dims")
    c, tensors, p_sh, p_depth, p_valid = _baked_view_desc("render_lightmapped", ctx, scene, render_target, camera_params, camera_transform, origin, spacing,
                                                          dims, sh, depth, max_distance, valid, ambient, visibility, backface, ray_epsilon, normal_bias,
                                                          max_slots)
    items = [k if isinstance(k, LightmapChart) else LightmapChart(*k) for k in charts]
    c_charts = (_abi.LightmapChartC * max(1, len(items)))(*[_abi.LightmapChartC(int(k.instance_idx), k.scale_u, k.scale_v, k.offset_u, k.offset_v)
                                                           for k in items])
    if hasattr(lightmap, "data_ptr"):   # a torch tensor
        import torch
        if sh is not None and not tensors:
            raise ValueError("lightmap and sh must both be torch tensors, or neither")
        if not (lightmap.is_cuda and lightmap.dtype == torch.float32 and lightmap.is_contiguous() and lightmap.dim() == 3 and lightmap.shape[2] == 4):
            raise ValueError("lightmap must be a contiguous (height, width, 4) float32 tensor on the context's device")
        if lightmap.device.index != ctx.device_ordinal:
            raise ValueError("lightmap is on another device than the context")
        c.flags = BAKED_VIEW_DEVICE_POINTERS
        p_lm = C.c_void_p(lightmap.data_ptr())
    else:
        if tensors:
            raise ValueError("lightmap and sh must both be torch tensors, or neither")
        lightmap = np.ascontiguousarray(lightmap, np.float32)
        if lightmap.ndim != 3 or lightmap.shape[2] != 4:
            raise ValueError("lightmap must be (height, width, 4)")
        p_lm = ptr(lightmap)
    d = _abi.LightmappedViewDescC(c, int(lightmap.shape[1]), int(lightmap.shape[0]), len(items), 0)
    if directional is None:
        gbuffer, gb = _baked_view_gbuffer(render_target, LIGHTMAPPED_VIEW_GBUFFER_FLOATS, want_gbuffer, lightmap if hasattr(lightmap, "data_ptr") else None)
        check(lib().lupin_hip_render_lightmapped(ctx.handle, scene.handle, render_target.handle, C.byref(d), c_charts, p_lm, p_sh, p_depth, p_valid, gb))
        return gbuffer
    planes = (LIGHTMAP_DIRECTIONAL_PLANES,) + tuple(int(k) for k in lightmap.shape)
    if hasattr(lightmap, "data_ptr"):
        import torch
        if not (hasattr(directional, "data_ptr") and directional.is_cuda and directional.dtype == torch.float32 and directional.is_contiguous()
                and tuple(directional.shape) == planes and directional.device == lightmap.device):
            raise ValueError("directional must be a contiguous (4, height, width, 4) float32 tensor beside lightmap")
        p_dir = C.c_void_p(directional.data_ptr())
    else:
        if hasattr(directional, "data_ptr"):
            raise ValueError("lightmap and directional must both be torch tensors, or neither")
        directional = np.ascontiguousarray(directional, np.float32)
        if directional.shape != planes:
            raise ValueError("directional must be (4, height, width, 4), the lightmap's atlas four times")
        p_dir = ptr(directional)
    gbuffer, gb = _baked_view_gbuffer(render_target, LIGHTMAPPED_DIRECTIONAL_GBUFFER_FLOATS, want_gbuffer,
                                      lightmap if hasattr(lightmap, "data_ptr") else None)
    dd = _abi.LightmappedDirectionalDescC(d, int(bake_flags), (C.c_uint32 * 3)(0, 0, 0))
    check(lib().lupin_hip_render_lightmapped_directional(ctx.handle, scene.handle, render_target.handle, C.byref(dd), c_charts, p_lm, p_dir, p_sh, p_depth,
                                                         p_valid, gb))
    return gbuffer
