"""The Python side of tests/cpp_mirror_probe.cpp: the blob format, the inputs of every section, and the same calls through
lupinpathtracer_amd.api.  tests/test_cpp_mirror.py compares the two hosts' words.

A blob is a flat list of named arrays: u32 name length, name bytes, u32 dtype code (0 f32, 1 u32, 2 u8, 3 u16), u32 ndim,
u64 dims, raw bytes.  A scalar is an array of one element.

The rule for the inputs: within one descriptor no two scalar fields of the same type carry the same value (`distinct`), so
that a wrapper that swaps two fields, or shifts them by one, cannot give the words of a wrapper that does not."""
import os
import struct

import numpy as np

from lupinpathtracer_amd import api, loader
from tests import util

DTYPES = [np.dtype(np.float32), np.dtype(np.uint32), np.dtype(np.uint8), np.dtype(np.uint16)]
FIXTURE = "materials2"     # texcoords on every mesh, and a material of opacity 0.2 (instances 5 and 10)
N = 65                     # records and points: one full wave and a tail lane
SEED = 20240611


def write_blob(path, arrays):
    with open(path, "wb") as f:
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            if a.ndim == 0:
                a = a.reshape(1)
            code = DTYPES.index(a.dtype)
            raw = name.encode()
            f.write(struct.pack("<I", len(raw)) + raw + struct.pack("<II", code, a.ndim) + struct.pack(f"<{a.ndim}Q", *a.shape))
            f.write(a.tobytes())


def read_blob(path):
    out = {}
    with open(path, "rb") as f:
        data = f.read()
    at = 0
    while at < len(data):
        (n,) = struct.unpack_from("<I", data, at)
        name = data[at + 4:at + 4 + n].decode()
        at += 4 + n
        code, ndim = struct.unpack_from("<II", data, at)
        dims = struct.unpack_from(f"<{ndim}Q", data, at + 8)
        at += 8 + 8 * ndim
        count = int(np.prod(dims, dtype=np.int64)) if ndim else 1
        out[name] = np.frombuffer(data, DTYPES[code], count, at).reshape(dims).copy()
        at += count * DTYPES[code].itemsize
    return out


def distinct(what, same=(), **fields):
    """The rule: the scalar fields of one descriptor, ints among themselves and floats among themselves, all differ.
    `same`: names the Python host fills from one argument, which therefore cannot differ.  Returns the fields."""
    for kind in (int, float):
        seen = {}
        for name, v in fields.items():
            if isinstance(v, bool) or not isinstance(v, kind) or name in same:
                continue
            key = np.float32(v).tobytes() if kind is float else int(v)
            assert key not in seen, f"{what}: {name} and {seen[key]} carry the same value {v}; a swap of the two would go unseen"
            seen[key] = name
    return fields


def flat(prefix, fields):
    """Blob entries of a descriptor's scalars: ints and bools as u32, floats as f32, nested dicts by dotted names."""
    out = {}
    for name, v in fields.items():
        key = f"{prefix}.{name}"
        if isinstance(v, dict):
            out.update(flat(key, v))
        elif isinstance(v, (bool, int, np.integer)):
            out[key] = np.uint32(int(v))
        elif isinstance(v, (float, np.floating)):
            out[key] = np.float32(v)
        else:
            out[key] = np.ascontiguousarray(v)
    return out


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


# ---- what every section is called with --------------------------------------------------------------------------

ADVANCED = distinct("AdvancedParams", max_radiance=10.5, rng_seed=7, ray_epsilon=0.002)
EPS = ADVANCED["ray_epsilon"]
IMAGE = (40, 24)           # falsecolor, debug, denoise, tiles, the baked and lightmapped views
ADAPTIVE_IMAGE = (41, 27)  # no multiple of the 8 x 8 block
ATLAS = (24, 20)


def camera(cam, width, height):
    p = cam.params
    return distinct("CameraParams", is_orthographic=bool(p.is_orthographic), lens=float(p.lens), film=float(p.film), aspect=width / height,
                    focus=float(p.focus), aperture=float(p.aperture))


def camera_of(fields):
    return api.CameraParams(fields["is_orthographic"], fields["lens"], fields["film"], fields["aspect"], fields["focus"], fields["aperture"])


def advanced_of(fields):
    return api.AdvancedParams(fields["max_radiance"], fields["rng_seed"], fields["ray_epsilon"])


def pathtrace_desc(cam, width, height):
    return dict(camera=camera(cam, width, height), camera_transform=np.asarray(cam.transform, np.float32).reshape(4, 3), force_software_bvh=True,
                advanced=dict(ADVANCED))


def pathtrace_desc_of(fields, accum_params=None):
    return api.PathtraceDesc(accum_params=accum_params, tile_params=None, camera_params=camera_of(fields["camera"]), camera_transform=fields["camera_transform"],
                             force_software_bvh=fields["force_software_bvh"], advanced=advanced_of(fields["advanced"]))


def baked(max_bounces=3, samples_per_pixel=4):
    return distinct("BakedPathtraceParams", with_runtime_checks=True, max_bounces=max_bounces, samples_per_pixel=samples_per_pixel)


def baked_of(fields):
    return api.BakedPathtraceParams(fields["with_runtime_checks"], fields["max_bounces"], fields["samples_per_pixel"])


def lightmap_desc(pathtrace_type, flags=0):
    """With flags 0 every u32 of the descriptor differs, so a swap shows.  The only flag a host-pointer bake can set,
    LIGHTMAP_SMOOTH_NORMALS, is 1, and so is the dilate the bakes are to run with: the directional bake sets the flag, so a
    wrapper that drops `flags` shows there, and flags and dilate are then the same on purpose."""
    return distinct("LightmapDesc", same=("flags",) if flags == 1 else (), width=ATLAS[0], height=ATLAS[1], pathtrace_type=pathtrace_type, max_bounces=3, samples=4,
                    max_slots=256, flags=flags, dilate=1, counter=5, surface_offset=0.003, **{"advanced." + k: v for k, v in ADVANCED.items()})


def lightmap_fields(d):
    """lightmap_desc's fields as the blob carries them: the advanced parameters nested."""
    out = {k: v for k, v in d.items() if not k.startswith("advanced.")}
    out["advanced"] = {k[len("advanced."):]: v for k, v in d.items() if k.startswith("advanced.")}
    return out


# the floor (its texcoords run to 20) in the atlas' first quadrant, a half-transparent sphere in its last
CHARTS = [api.LightmapChart(0, 0.023, 0.0215, 0.02, 0.03), api.LightmapChart(5, 0.41, 0.37, 0.52, 0.55)]
for _c in CHARTS:
    distinct("LightmapChart", instance_idx=_c.instance_idx, scale_u=_c.scale_u, scale_v=_c.scale_v, offset_u=_c.offset_u, offset_v=_c.offset_v)


def charts_fields():
    return {"instance_idx": np.array([c.instance_idx for c in CHARTS], np.uint32),
            "scale_offset": np.array([[c.scale_u, c.scale_v, c.offset_u, c.offset_v] for c in CHARTS], np.float32)}


GRID = dict(origin=np.array([-0.7, 0.3, -0.6], np.float32), spacing=np.array([1.3, 1.2, 1.1], np.float32), dims=np.array([2, 2, 2], np.uint32))
NORMAL_BIAS = 0.004
DEPTH = distinct("ProbeDepthDesc", resolution=4, subsamples=2, flags=0, max_slots=64, ray_epsilon=EPS, max_distance=1.3)
# the maps the depth lookup and the baked view read: another resolution than PROBE_GRID_BACKFACE = 4, the grid's flags there
VIEW_DEPTH = distinct("ProbeDepthDesc", resolution=6, subsamples=2, flags=0, max_slots=64, ray_epsilon=EPS, max_distance=1.3)
AMBIENT = np.array([0.11, 0.12, 0.13], np.float32)


def box_points(rng, n):
    """Points inside the Cornell box (x, z in [-1, 1], y in [0, 2]), clear of its walls."""
    return rng.uniform([-0.9, 0.1, -0.9], [0.9, 1.9, 0.9], (n, 3)).astype(np.float32)


def instance_centre(cpu, i):
    """The world-space centre of instance i's model box."""
    inst = cpu.instances[i]
    v = np.asarray(cpu.verts_pos_array[int(inst["mesh_idx"])], np.float64).reshape(-1, 4)[:, :3]
    m = np.asarray(inst["transpose_inverse_transform"], np.float64)      # 3 x 4 rows of world -> local
    return np.linalg.solve(m[:, :3], 0.5 * (v.min(axis=0) + v.max(axis=0)) - m[:, 3])


def host_inputs():
    """The inputs of the sections that need no device."""
    rng = np.random.default_rng(SEED)
    eps = np.float32(EPS)
    p = rng.uniform(-1.0, 1.0, (N, 3)).astype(np.float32)
    q = (p + unit(rng.normal(size=(N, 3))) * rng.uniform(0.01, 2.0, (N, 1))).astype(np.float32)
    # length exactly 2 * ray_epsilon, in f32: along one axis from the origin, so that the squares, the sum and the root are exact
    short_p = np.zeros((1, 3), np.float32)
    short_q = np.array([[0.0, np.float32(2.0) * eps, 0.0]], np.float32)
    return {
        "host_only.grid.origin": np.array([0.1, -0.2, 0.3], np.float32),
        "host_only.grid.spacing": np.array([0.3, 0.7, 1.1], np.float32),      # not dyadic: the sum first would round differently
        "host_only.grid.dims": np.array([3, 2, 4], np.uint32),
        "host_only.sh.coeffs": rng.uniform(-2.0, 2.0, (64, 9, 4)).astype(np.float32),
        "host_only.sh.normals": unit(rng.normal(size=(64, 3))),
        "host_only.get_num_tiles": np.array([[16, 40, 24], [100, 1920, 1080], [1, 5, 3], [8, 64, 64], [7, 33, 17]], np.uint32),
        "host_only.segments.ray_epsilon": eps,
        "host_only.segments.p": p,
        "host_only.segments.q": q,
        "host_only.short.p": short_p,
        "host_only.short.q": short_q,
    }


class Inputs:
    """Every section's arguments, as Python values (`P`) and as the blob's arrays (`blob`)."""

    def __init__(self, adaptive_threshold=0.25):
        rng = np.random.default_rng(SEED + 1)
        _, cams = util.load_scene("cornellbox_builtin", None)
        cornell_cpu, _ = loader.cornell_box_scene_cpu()
        self.fixture_path = os.path.join(util.SCENES, FIXTURE, FIXTURE + ".json")
        fixture_cpu, _, _, fixture_cams = loader.load_scene_cpu_yoctogl_v24(self.fixture_path, [util.SHARED])
        cam, fcam = cams[0], fixture_cams[0]
        P, B = {}, dict(host_inputs())
        B["fixture.path"] = np.frombuffer(self.fixture_path.encode(), np.uint8)
        B["fixture.asset_dir"] = np.frombuffer(util.SHARED.encode(), np.uint8)

        def section(name, **fields):
            P[name] = fields
            B.update(flat(name, fields))
            return fields

        W, H = IMAGE
        section("pathtrace_scene_tiles", baked=baked(), width=W, height=H, desc=pathtrace_desc(cam, W, H), accum_counter=5,
                small_tile_size=distinct("pathtrace_scene_tiles", pathtrace_type=3, tile_size=4, rank=1, world=2)["tile_size"],
                **distinct("pathtrace_scene_tiles", pathtrace_type=3, tile_size=16, rank=1, world=2))
        section("pathtrace_scene_falsecolor", baked=baked(), width=W, height=H, desc=pathtrace_desc(cam, W, H), type_a=int(api.FalsecolorType.Albedo),
                type_b=int(api.FalsecolorType.Normals))
        section("pathtrace_scene_debug", baked=baked(), width=W, height=H, desc=pathtrace_desc(cam, W, H),
                **distinct("DebugVizDesc", viz_type=int(api.DebugVizType.NumBounces), heatmap_min=0.5, heatmap_max=37.0, first_hit_only=True))
        section("denoise", baked=baked(), desc=pathtrace_desc(cam, W, H), frames=2, pathtrace_type=0, quality=int(api.DenoiseQuality.Medium))

        AW, AH = ADAPTIVE_IMAGE
        section("pathtrace_scene_adaptive", baked=baked(), width=AW, height=AH, desc=pathtrace_desc(cam, AW, AH), calls=3, accum_counter=0, pathtrace_type=0,
                **distinct("AdaptiveParams", threshold=float(adaptive_threshold), min_frames=2, max_frames=7))
        moved = np.asarray(cam.transform, np.float32).reshape(4, 3).copy()
        moved[3] += np.array([0.11, 0.05, 0.07], np.float32)
        section("adaptive_reproject", view=dict(camera=camera(cam, AW, AH), camera_transform=moved),
                prev_instance_transforms=np.ascontiguousarray(cornell_cpu.instances["transpose_inverse_transform"], np.float32).reshape(-1, 3, 4),
                **distinct("ReprojectDesc", ray_epsilon=EPS, depth_tolerance=0.03, max_history=2, num_instances=len(cornell_cpu.instances)))

        def ray_query(pathtrace_type, max_slots):
            return distinct("RayQueryDesc", pathtrace_type=pathtrace_type, max_bounces=3, samples=4, flags=0, max_slots=max_slots,
                            **{"advanced." + k: v for k, v in ADVANCED.items()})

        modes = (np.arange(N) % 2).astype(np.uint32)          # direction and cosine-hemisphere records, alternating
        records = api.ray_records(box_points(rng, N), unit(rng.normal(size=(N, 3))), rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32), modes)
        section("pathtrace_rays", desc=lightmap_fields(ray_query(1, 128)), records=records)      # 128 slots: more than one wavefront of paths
        section("pathtrace_rays_moments", desc=lightmap_fields(ray_query(2, 64)), records=records)

        positions = api.probe_grid_positions(GRID["origin"], GRID["spacing"], GRID["dims"])
        probes = np.zeros((len(positions), 4), np.float32)
        probes[:, :3] = positions
        probes.view(np.uint32)[:, 3] = api.rng_seed_for(np.arange(len(positions), dtype=np.uint32), 9)
        section("bake_probes", counter=9, probes=probes, positions=positions,
                desc=lightmap_fields(distinct("ProbeDesc", pathtrace_type=1, max_bounces=3, samples=16, flags=0, max_slots=64,
                                              **{"advanced." + k: v for k, v in ADVANCED.items()})))

        words = rng.integers(0, 2 ** 32, N, dtype=np.uint64).astype(np.uint32)
        hemisphere = api.occlusion_records(box_points(rng, N), unit(rng.normal(size=(N, 3))), 0.6, words)
        section("occlusion_rays", records=hemisphere, desc=distinct("OcclusionDesc", mode=1, samples=4, flags=0, ray_epsilon=EPS))
        section("visible", p=box_points(rng, N), q=box_points(rng, N), ray_epsilon=EPS)
        section("ambient_occlusion", origins=box_points(rng, N), normals=unit(rng.normal(size=(N, 3))), counter=3,
                rng_words=api.rng_seed_for(np.arange(N, dtype=np.uint32), 3), **distinct("ambient_occlusion", radius=0.6, samples=4, ray_epsilon=EPS))

        rmax = np.where(np.arange(N) % 2 == 0, np.float32(np.inf), np.float32(0.3)).astype(np.float32)
        section("distance_points", records=api.distance_records(box_points(rng, N), rmax), flags=0)
        section("bake_distance_grid", origin=np.array([-0.8, 0.2, -0.7], np.float32), spacing=np.array([0.55, 0.65, 0.6], np.float32),
                dims=np.array([3, 2, 2], np.uint32), rmax=0.9)

        valid = np.ones(len(positions), np.uint8)
        valid[5] = 0
        B["volume.sh"] = rng.uniform(0.0, 1.0, (len(positions), 9, 4)).astype(np.float32)
        B["volume.valid"] = valid
        lookups = api.probe_grid_records(rng.uniform(GRID["origin"] - 0.1, GRID["origin"] + GRID["spacing"] + 0.1, (N, 3)).astype(np.float32),
                                         unit(rng.normal(size=(N, 3))))
        section("sample_probe_grid", records=lookups,
                grid=dict(GRID, **distinct("ProbeGridDesc", flags=api.PROBE_GRID_VISIBILITY | api.PROBE_GRID_BACKFACE, ray_epsilon=EPS, normal_bias=NORMAL_BIAS)))
        depth_positions = np.zeros((len(positions), 4), np.float32)
        depth_positions[:, :3] = positions
        section("bake_probe_depth", desc=dict(DEPTH), positions=depth_positions)
        section("view_depth", desc=dict(VIEW_DEPTH))
        distinct("ProbeGridDepthDesc", **{"grid.flags": api.PROBE_GRID_BACKFACE, "grid.ray_epsilon": 0.0, "grid.normal_bias": NORMAL_BIAS},
                 resolution=VIEW_DEPTH["resolution"], max_distance=VIEW_DEPTH["max_distance"])
        section("sample_probe_grid_depth", records=lookups, resolution=VIEW_DEPTH["resolution"], max_distance=VIEW_DEPTH["max_distance"],
                grid=dict(GRID, **distinct("ProbeGridDesc", flags=api.PROBE_GRID_BACKFACE, ray_epsilon=0.0, normal_bias=NORMAL_BIAS)))

        def view(cam):
            """A LupinBakedViewDesc's fields; the Python host fills the grid's ray_epsilon and the view's from one argument."""
            fields = distinct("BakedViewDesc", same=("grid.ray_epsilon",), resolution=VIEW_DEPTH["resolution"], max_distance=VIEW_DEPTH["max_distance"],
                              ray_epsilon=EPS, flags=0, max_slots=128,
                              **{"grid.flags": api.PROBE_GRID_BACKFACE, "grid.ray_epsilon": EPS, "grid.normal_bias": NORMAL_BIAS},
                              **{"camera." + k: v for k, v in camera(cam, W, H).items()})
            out = {k: v for k, v in fields.items() if "." not in k}
            out["camera"] = camera(cam, W, H)
            out["camera_transform"] = np.asarray(cam.transform, np.float32).reshape(4, 3)
            out["grid"] = dict(GRID, **distinct("ProbeGridDesc", flags=api.PROBE_GRID_BACKFACE, ray_epsilon=EPS, normal_bias=NORMAL_BIAS))
            out["ambient"] = AMBIENT
            return out

        section("render_baked", width=W, height=H, view=view(cam))
        # without a volume the Python host passes a zeroed grid, no maps' resolution and no max_distance: so does the probe
        no_volume = view(fcam)
        no_volume.update(resolution=0, max_distance=0.0,
                         grid=dict(origin=np.zeros(3, np.float32), spacing=np.zeros(3, np.float32), dims=np.zeros(3, np.uint32), flags=0, ray_epsilon=0.0, normal_bias=0.0))
        distinct("LightmappedViewDesc", lightmap_width=ATLAS[0], lightmap_height=ATLAS[1], num_charts=len(CHARTS), reserved=0)
        section("render_lightmapped", width=W, height=H, view=no_volume, lightmap_width=ATLAS[0], lightmap_height=ATLAS[1])
        section("render_lightmapped_directional", width=W, height=H, view=no_volume, lightmap_width=ATLAS[0], lightmap_height=ATLAS[1],
                bake_flags=api.LIGHTMAP_SMOOTH_NORMALS)

        transforms = np.ascontiguousarray(cornell_cpu.instances["transpose_inverse_transform"], np.float32).reshape(-1, 3, 4).copy()
        transforms[5, :, 3] += np.array([0.21, 0.0, -0.13], np.float32)       # the short box slides over the floor
        transforms[6, :, 3] += np.array([-0.1, 0.0, 0.17], np.float32)        # and the tall one
        section("update_instances", transforms=transforms, device_tlas=True, records=api.distance_records(box_points(rng, N)))

        # the fixture scene: half of the segments and origins lie about the two instances of opacity 0.2
        centres = np.array([instance_centre(fixture_cpu, 5), instance_centre(fixture_cpu, 10)])
        about = centres[np.arange(N) % 2]
        away = unit(rng.normal(size=(N, 3))) * np.array([0.45, 0.04, 0.45], np.float32)      # nearly level: they stand on an opaque floor
        p = (about + away + rng.uniform(-0.03, 0.03, (N, 3))).astype(np.float32)
        q = (about - away + rng.uniform(-0.03, 0.03, (N, 3))).astype(np.float32)
        section("transmittance", p=p, q=q, ray_epsilon=EPS)
        origins = (about + unit(rng.normal(size=(N, 3))) * rng.uniform(0.2, 0.5, (N, 1))).astype(np.float32)
        section("bent_normal_rays", records=api.occlusion_records(origins, unit(about - origins + rng.normal(size=(N, 3)) * 0.2), 0.9, words),
                desc=distinct("BentNormalDesc", samples=4, flags=api.BENT_NORMAL_OPACITY, max_slots=128, ray_epsilon=EPS))      # on the scene that has opacity
        section("transmittance_rays", records=api.occlusion_records(origins, unit(about - origins + rng.normal(size=(N, 3)) * 0.2), 0.9, words),
                desc=distinct("OcclusionDesc", mode=1, samples=4, flags=0, ray_epsilon=EPS))

        section("bake_lightmap", desc=lightmap_fields(lightmap_desc(2)), charts=charts_fields())
        section("bake_lightmap_directional", desc=lightmap_fields(lightmap_desc(2, api.LIGHTMAP_SMOOTH_NORMALS)), charts=charts_fields())
        section("bake_lightmap_adaptive", desc=lightmap_fields(lightmap_desc(2)), charts=charts_fields(),
                **distinct("LightmapAdaptiveDesc", threshold=0.2, min_rounds=1, max_rounds=3, flags=0))
        section("bake_lightmap_ao", charts=charts_fields(),
                desc=distinct("LightmapAoDesc", width=ATLAS[0], height=ATLAS[1], samples=4, max_slots=256, flags=api.LIGHTMAP_AO_OPACITY, dilate=1, counter=5,
                              surface_offset=0.003, max_distance=0.75, ray_epsilon=EPS))
        section("denoise_lightmap", **distinct("LightmapDenoiseDesc", width=ATLAS[0], height=ATLAS[1], passes=2, normal_squarings=3, dilate=1, flags=0, max_stretch=3.5))
        self.P, self.blob, self.fixture_cam = P, B, fcam

    def set_adaptive_threshold(self, threshold):
        self.P["pathtrace_scene_adaptive"]["threshold"] = float(threshold)
        self.blob["pathtrace_scene_adaptive.threshold"] = np.float32(threshold)


# ---- the same calls through the Python host ---------------------------------------------------------------------

class PythonHost:
    """Every section through lupinpathtracer_amd.api: section(name) returns the arrays the probe writes under that name."""

    def __init__(self, ctx, inputs):
        self.ctx, self.P, self.B = ctx, inputs.P, inputs.blob
        self._cornell = self._fixture = None
        self._cache = {}

    @property
    def cornell(self):
        if self._cornell is None:
            self._cornell = util.load_scene("cornellbox_builtin", self.ctx)[0]
        return self._cornell

    @property
    def fixture(self):
        if self._fixture is None:
            self._fixture = util.load_scene(FIXTURE, self.ctx)[0]
        return self._fixture

    def section(self, name):
        def as_written(v):      # an Rgba16Float image is compared as its f16 words
            v = np.ascontiguousarray(v)
            return v.view(np.uint16) if v.dtype == np.float16 else v
        return {f"{name}.{k}": as_written(v) for k, v in getattr(self, name)().items()}

    def once(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def pathtrace_scene_tiles(self):
        p = self.P["pathtrace_scene_tiles"]
        res = api.build_pathtrace_resources(self.ctx, baked_of(p["baked"]))
        out = {}
        for which in ("tile_size", "small_tile_size"):
            tex = api.DoubleBufferedTexture(self.ctx, p["width"], p["height"])
            desc = pathtrace_desc_of(p["desc"], api.AccumulationParams(tex.back(), p["accum_counter"]))
            api.pathtrace_scene_tiles(self.ctx, res, self.cornell, tex.front(), p["pathtrace_type"], desc, p[which], p["rank"], p["world"])
            out["image." + which] = tex.front().download()
        return out

    def falsecolor(self, falsecolor_type):
        p = self.P["pathtrace_scene_falsecolor"]
        res = api.build_pathtrace_resources(self.ctx, baked_of(p["baked"]))
        tex = api.Texture(self.ctx, p["width"], p["height"])
        api.pathtrace_scene_falsecolor(self.ctx, res, self.cornell, tex, falsecolor_type, pathtrace_desc_of(p["desc"]))
        return tex

    def pathtrace_scene_falsecolor(self):
        p = self.P["pathtrace_scene_falsecolor"]
        return {"image_a": self.falsecolor(p["type_a"]).download(), "image_b": self.falsecolor(p["type_b"]).download()}

    def pathtrace_scene_debug(self):
        p = self.P["pathtrace_scene_debug"]
        res = api.build_pathtrace_resources(self.ctx, baked_of(p["baked"]))
        tex = api.Texture(self.ctx, p["width"], p["height"])
        dd = api.DebugVizDesc(p["viz_type"], p["heatmap_min"], p["heatmap_max"], p["first_hit_only"])
        api.pathtrace_scene_debug(self.ctx, res, self.cornell, tex, dd, pathtrace_desc_of(p["desc"]))
        return {"image": tex.download()}

    def denoise(self):
        p, f = self.P["denoise"], self.P["pathtrace_scene_falsecolor"]
        W, H = f["width"], f["height"]
        res = api.build_pathtrace_resources(self.ctx, baked_of(p["baked"]))
        color = api.DoubleBufferedTexture(self.ctx, W, H)
        for k in range(p["frames"]):
            api.pathtrace_scene(self.ctx, res, self.cornell, color.front(), p["pathtrace_type"], pathtrace_desc_of(p["desc"], api.AccumulationParams(color.back(), k)))
            color.flip()
        color.flip()
        albedo, normals, result = self.falsecolor(f["type_a"]), self.falsecolor(f["type_b"]), api.Texture(self.ctx, W, H)
        api.denoise(self.ctx, api.build_denoise_resources(self.ctx, W, H),
                    api.DenoiseDesc(pathtrace_output=color.front(), denoise_output=result, albedo=albedo, normals=normals, quality=api.DenoiseQuality(p["quality"])))
        return {"noisy": color.front().download(), "image": result.download()}

    def adaptive_sequence(self, reproject, threshold=None, calls=None):
        a, r = self.P["pathtrace_scene_adaptive"], self.P["adaptive_reproject"]
        W, H = a["width"], a["height"]
        res = api.build_pathtrace_resources(self.ctx, baked_of(a["baked"]))
        ares = api.build_adaptive_resources(self.ctx, W, H)
        rres = api.build_reproject_resources(self.ctx, W, H)
        tex = api.DoubleBufferedTexture(self.ctx, W, H)
        params = api.AdaptiveParams(a["threshold"] if threshold is None else threshold, a["min_frames"], a["max_frames"])

        def reproject_to(view):
            rd = api.ReprojectDesc(camera_of(view["camera"]), view["camera_transform"], r["ray_epsilon"], r["depth_tolerance"], r["max_history"],
                                   r["prev_instance_transforms"])
            api.adaptive_reproject(self.ctx, ares, rres, self.cornell, rd, tex.back(), tex.front())
            tex.flip()

        if reproject:
            reproject_to(a["desc"])
        for _ in range(a["calls"] if calls is None else calls):
            desc = pathtrace_desc_of(a["desc"], api.AccumulationParams(tex.back(), a["accum_counter"]))
            api.pathtrace_scene_adaptive(self.ctx, res, self.cornell, tex.front(), a["pathtrace_type"], desc, ares, params)
            tex.flip()
        out = {}
        if reproject:
            reproject_to(r["view"])
            out["inst"], out["tri"], out["uv"], out["depth"] = rres.download(0)
        out["image"] = tex.back().download()
        frames, moments, err, active = ares.download()
        s = ares.stats()
        out.update(frames=frames, moments=moments, block_error=err, block_active=active.astype(np.uint8),
                   stats=np.array([s.active_pixels, s.pixel_frames, s.calls, s.max_frames_taken], np.uint32))
        return out

    def pathtrace_scene_adaptive(self):
        return self.adaptive_sequence(False)

    def adaptive_reproject(self):
        return self.adaptive_sequence(True)

    def pick_adaptive_threshold(self):
        """A threshold under which, after the two frames every block must take, some blocks stop and some go on: from the
        block errors of two frames rendered with threshold 0 (which do not depend on the threshold), by the stated rule -- a
        block is active while it or one of its eight neighbours has not converged."""
        err = self.adaptive_sequence(False, threshold=0.0, calls=2)["block_error"].astype(np.float64)
        values = np.unique(err[np.isfinite(err)])
        for thr in np.float32(0.5 * (values[:-1] + values[1:]))[::-1]:
            waiting = np.pad(~(err < thr), 1, constant_values=False)
            active = np.zeros_like(err, bool)
            for dy in range(3):
                for dx in range(3):
                    active |= waiting[dy:dy + err.shape[0], dx:dx + err.shape[1]]
            if 0 < active.sum() < active.size:
                return float(thr)
        raise AssertionError("no threshold stops some 8 x 8 blocks and not others: the adaptive section's image does not reach that path")

    def ray_query_desc(self, d):
        return api.RayQueryDesc(d["pathtrace_type"], d["max_bounces"], d["samples"], d["flags"], d["max_slots"], advanced_of(d["advanced"]))

    def pathtrace_rays(self):
        p = self.P["pathtrace_rays"]
        out, rays = api.pathtrace_rays(self.ctx, self.cornell, p["records"], self.ray_query_desc(p["desc"]), want_rays=True)
        return {"out": out, "out_rays": rays}

    def pathtrace_rays_moments(self):
        p = self.P["pathtrace_rays_moments"]
        return {"out": api.pathtrace_rays_moments(self.ctx, self.cornell, p["records"], self.ray_query_desc(p["desc"]))}

    def bake_probes(self):
        p = self.P["bake_probes"]
        d = p["desc"]
        sh, rays = api.bake_probes(self.ctx, self.cornell, p["positions"], d["samples"], d["pathtrace_type"], d["max_bounces"], advanced_of(d["advanced"]),
                                   p["counter"], d["max_slots"], want_rays=True)
        return {"sh": sh, "rays": rays}

    def occlusion_rays(self):
        p = self.P["occlusion_rays"]
        d = p["desc"]
        return {"blocked": api.occlusion_rays(self.ctx, self.cornell, p["records"], d["mode"], d["samples"], d["ray_epsilon"])}

    def visible(self):
        p = self.P["visible"]
        return {"visible": api.visible(self.ctx, self.cornell, p["p"], p["q"], p["ray_epsilon"]).astype(np.uint8)}

    def ambient_occlusion(self):
        p = self.P["ambient_occlusion"]
        return {"ao": api.ambient_occlusion(self.ctx, self.cornell, p["origins"], p["normals"], p["radius"], p["samples"], p["ray_epsilon"], p["counter"],
                                            surface_offset=0)}

    def transmittance_rays(self):
        p = self.P["transmittance_rays"]
        d = p["desc"]
        return {"sum": api.transmittance_rays(self.ctx, self.fixture, p["records"], d["mode"], d["samples"], d["ray_epsilon"])}

    def transmittance(self):
        p = self.P["transmittance"]
        return {"t": api.transmittance(self.ctx, self.fixture, p["p"], p["q"], p["ray_epsilon"])}

    def bent_normal_rays(self):
        p = self.P["bent_normal_rays"]
        d = p["desc"]
        return {"sums": api.bent_normal_rays(self.ctx, self.fixture, p["records"], d["samples"], d["ray_epsilon"], opacity=bool(d["flags"] & api.BENT_NORMAL_OPACITY),
                                             max_slots=d["max_slots"])}

    def distance_points(self):
        r = api.distance_points(self.ctx, self.cornell, self.P["distance_points"]["records"])
        return {k: r[k] for k in ("found", "distance", "point", "u", "v", "instance", "tri", "side")}

    def bake_distance_grid(self):
        p = self.P["bake_distance_grid"]
        return {name: api.bake_distance_grid(self.ctx, self.cornell, p["origin"], p["spacing"], p["dims"], p["rmax"], signed=signed)
                for name, signed in (("unsigned", False), ("signed", True))}

    def sample_probe_grid(self):
        p = self.P["sample_probe_grid"]
        g = p["grid"]
        return {"out": api.sample_probe_grid(self.ctx, self.cornell, g["origin"], g["spacing"], g["dims"], self.B["volume.sh"], p["records"], valid=self.B["volume.valid"],
                                             visibility=bool(g["flags"] & api.PROBE_GRID_VISIBILITY), backface=bool(g["flags"] & api.PROBE_GRID_BACKFACE),
                                             ray_epsilon=g["ray_epsilon"], normal_bias=g["normal_bias"])}

    def probe_depth(self, name="bake_probe_depth"):
        """(maps, stats) of the grid's probes by the descriptor of section `name`: bake_probe_depth's own, or view_depth's."""
        positions, d = self.P["bake_probe_depth"]["positions"], self.P[name]["desc"]
        return self.once(name, lambda: api.bake_probe_depth(self.ctx, self.cornell, positions[:, :3], d["resolution"], d["subsamples"],
                                                            max_distance=d["max_distance"], ray_epsilon=d["ray_epsilon"], want_stats=True, max_slots=d["max_slots"]))

    def bake_probe_depth(self):
        depth, stats = self.probe_depth()
        return {"depth": depth, "stats": stats}

    def sample_probe_grid_depth(self):
        p = self.P["sample_probe_grid_depth"]
        g = p["grid"]
        return {"out": api.sample_probe_grid_depth(self.ctx, self.cornell, g["origin"], g["spacing"], g["dims"], self.B["volume.sh"], self.probe_depth("view_depth")[0], p["records"],
                                                   max_distance=p["max_distance"], valid=self.B["volume.valid"], backface=bool(g["flags"] & api.PROBE_GRID_BACKFACE),
                                                   normal_bias=g["normal_bias"])}

    def render_baked_arguments(self):
        v = self.P["render_baked"]["view"]
        g = v["grid"]
        return dict(camera_params=camera_of(v["camera"]), camera_transform=v["camera_transform"], origin=g["origin"], spacing=g["spacing"], dims=g["dims"],
                    sh=self.B["volume.sh"], depth=self.probe_depth("view_depth")[0], max_distance=v["max_distance"], valid=self.B["volume.valid"], ambient=v["ambient"],
                    visibility=bool(g["flags"] & api.PROBE_GRID_VISIBILITY), backface=bool(g["flags"] & api.PROBE_GRID_BACKFACE), ray_epsilon=v["ray_epsilon"],
                    normal_bias=g["normal_bias"], max_slots=v["max_slots"])

    def baked_view_desc_c(self):
        """The words of the LupinBakedViewDesc the Python host hands to lupin_hip_render_baked for render_baked's section."""
        p = self.P["render_baked"]
        tex = api.Texture(self.ctx, p["width"], p["height"])
        a = self.render_baked_arguments()
        c = api._baked_view_desc("render_baked", self.ctx, self.cornell, tex, a["camera_params"], a["camera_transform"], a["origin"], a["spacing"], a["dims"], a["sh"],
                                 a["depth"], a["max_distance"], a["valid"], a["ambient"], a["visibility"], a["backface"], a["ray_epsilon"], a["normal_bias"],
                                 a["max_slots"])[0]
        return {"words": np.frombuffer(bytes(c), np.uint32)}

    def render_baked(self):
        p = self.P["render_baked"]
        tex = api.Texture(self.ctx, p["width"], p["height"])
        gbuffer = api.render_baked(self.ctx, self.cornell, tex, want_gbuffer=True, **self.render_baked_arguments())
        return {"image": tex.download(), "gbuffer": gbuffer}

    def update_instances(self):
        p = self.P["update_instances"]
        scene = loader.build_scene_cornell_box(self.ctx)[0]     # a scene of its own: it is changed in place
        scene.update_instances(p["transforms"], tlas_builder="device" if p["device_tlas"] else "cpu")
        moved = api.distance_points(self.ctx, scene, p["records"])
        still = api.distance_points(self.ctx, self.cornell, p["records"])
        assert int((moved["distance"] != still["distance"]).sum()) > 0, "the move is not visible to these points"
        return {"results": moved.view(np.uint32).reshape(len(moved), api.DISTANCE_RESULT_FLOATS)}

    def lightmap_arguments(self, name):
        d = self.P[name]["desc"]
        assert d["flags"] in (0, api.LIGHTMAP_SMOOTH_NORMALS)
        return dict(charts=CHARTS, width=d["width"], height=d["height"], pathtrace_type=d["pathtrace_type"], max_bounces=d["max_bounces"],
                    advanced=advanced_of(d["advanced"]), counter=d["counter"], max_slots=d["max_slots"], smooth_normals=d["flags"] == api.LIGHTMAP_SMOOTH_NORMALS, dilate=d["dilate"],
                    surface_offset=d["surface_offset"], want_records=True), d["samples"]

    def lightmap(self, name):
        def bake():
            kw, samples = self.lightmap_arguments(name)
            return api.bake_lightmap(self.ctx, self.fixture, samples=samples, **kw)
        return self.once("lightmap." + name, bake)

    def directional(self):
        def bake():
            kw, samples = self.lightmap_arguments("bake_lightmap_directional")
            return api.bake_lightmap_directional(self.ctx, self.fixture, samples=samples, **kw)
        return self.once("directional", bake)

    def bake_lightmap(self):
        rgba, records = self.lightmap("bake_lightmap")
        return {"rgba": rgba, "records": records, "covered": np.uint32((rgba[..., 3] == 1.0).sum())}

    def bake_lightmap_directional(self):
        planes, records = self.directional()
        return {"sh": planes, "records": records, "covered": np.uint32((planes[0, ..., 3] == 1.0).sum())}

    def bake_lightmap_adaptive(self):
        p = self.P["bake_lightmap_adaptive"]
        kw, samples = self.lightmap_arguments("bake_lightmap_adaptive")
        rgba, stats, records = api.bake_lightmap_adaptive(self.ctx, self.fixture, samples_per_round=samples, threshold=p["threshold"], min_rounds=p["min_rounds"],
                                                          max_rounds=p["max_rounds"], want_stats=True, **kw)
        s = api.lightmap_adaptive_stats()
        totals = np.array([s["covered_texels"], s["rounds"], s["paths"], s["converged_texels"], s["capped_texels"], s["keys"]], np.uint32)
        return {"rgba": rgba, "stats": stats, "records": records, "covered": np.uint32((rgba[..., 3] == 1.0).sum()), "totals": totals}

    def bake_lightmap_ao(self):
        d = self.P["bake_lightmap_ao"]["desc"]
        ao, bent, records = api.bake_lightmap_ao(self.ctx, self.fixture, CHARTS, d["width"], d["height"], d["samples"], d["max_distance"], d["ray_epsilon"], d["counter"],
                                                 d["max_slots"], smooth_normals=bool(d["flags"] & api.LIGHTMAP_SMOOTH_NORMALS),
                                                 opacity=bool(d["flags"] & api.LIGHTMAP_AO_OPACITY), dilate=d["dilate"], surface_offset=d["surface_offset"], want_bent=True,
                                                 want_records=True)
        return {"ao": ao, "bent": bent, "records": records, "covered": np.uint32((ao[..., 3] == 1.0).sum())}

    def denoise_lightmap(self):
        p = self.P["denoise_lightmap"]
        rgba, records = self.lightmap("bake_lightmap")
        assert rgba.shape[:2] == (p["height"], p["width"]) and p["flags"] == 0
        return {"rgba": api.denoise_lightmap(self.ctx, rgba, records, p["passes"], p["normal_squarings"], p["max_stretch"], p["dilate"])}

    def lightmapped(self, name, source="bake_lightmap", **directional):
        """`source`: the section whose descriptor the atlas is baked with."""
        p = self.P[name]
        v = p["view"]
        tex = api.Texture(self.ctx, p["width"], p["height"])
        lightmap = self.lightmap(source)[0]
        assert lightmap.shape[:2] == (p["lightmap_height"], p["lightmap_width"])
        gbuffer = api.render_lightmapped(self.ctx, self.fixture, tex, camera_of(v["camera"]), v["camera_transform"], CHARTS, lightmap, ambient=v["ambient"],
                                         ray_epsilon=v["ray_epsilon"], want_gbuffer=True, max_slots=v["max_slots"], **directional)
        return {"image": tex.download(), "gbuffer": gbuffer}

    def render_lightmapped(self):
        return self.lightmapped("render_lightmapped")

    def render_lightmapped_directional(self):
        return self.lightmapped("render_lightmapped_directional", "bake_lightmap_directional", directional=self.directional()[0], bake_flags=self.P["render_lightmapped_directional"]["bake_flags"])
