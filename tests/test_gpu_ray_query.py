"""Radiance queries on the device (lupin_hip_pathtrace_rays): per ray against the oracle bit for bit, slot
independence, samples, chunks, the hemisphere mode, closed-form answers, device pointers, validation, and that frames
rendered around a query do not notice it.  Record layout: include/lupin_hip.h."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api, loader
from tests import stats, util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48
PT = api.PathtraceType
_cache = {}


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_words(got, want, what):
    bad = int((words(got) != words(want)).sum())
    assert bad == 0, f"{what}: {bad} of {words(want).size} f32 words differ"


def pcg_advance(state, draws):
    state = np.asarray(state, np.uint32).copy()
    with np.errstate(over="ignore"):
        for _ in range(draws):
            state = state * np.uint32(747796405) + np.uint32(2891336453)
    return state


def staged_in_lds(ctx, scene):
    """Whether this context's kernels read the scene's geometry from LDS: such a scene has no four-wide hierarchy, and the
    wide probe says so (as tests/test_light_probe.py finds out)."""
    try:
        api.trace_rays_wide(ctx, scene, [[0.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    except api.LupinError as e:
        assert "staged in LDS" in str(e), str(e)
        return True
    return False


def camera_records(scene, cam_params, cam_transform):
    """Every pixel's first ray of a W x H frame with accum_counter 0, as mode-0 records: the oracle's camera rays, and the
    pixel's seed advanced by the camera's four draws."""
    from oracle import oracle
    ori, dir_ = oracle.camera_rays(scene, W, H, cam_params, cam_transform, 0)
    seed = api.rng_seed_for(np.arange(W * H, dtype=np.uint32), 0)
    return api.ray_records(ori.reshape(-1, 3), dir_.reshape(-1, 3), pcg_advance(seed, 4), api.RayMode.DIRECTION)


def oracle_colours(scene, cam_params, cam_transform, ptype, max_bounces=8):
    from oracle import oracle
    _, _, rgb = oracle.pathtrace(scene, W, H, cam_params, cam_transform, max_bounces, 1, int(ptype), accum_counter=0, want_f32=True)
    return rgb.reshape(-1, 3)


def cornell(ctx):
    """The Cornell set shared by the tests: scene, records of the pinhole camera, the oracle's Standard colours."""
    if "cornell" not in _cache:
        scene, cams = util.load_scene("cornellbox_builtin", ctx)
        rec = camera_records(scene, cams[0].params, cams[0].transform)
        _cache["cornell"] = (scene, cams[0], rec, oracle_colours(scene, cams[0].params, cams[0].transform, PT.Standard))
    return _cache["cornell"]


PER_RAY = [("cornellbox_builtin", PT.Standard, False), ("cornellbox_builtin", PT.MIS, False), ("cornellbox_builtin", PT.Naive, False),
           ("cornellbox_builtin", PT.Direct, False), ("cornellbox_builtin", PT.Standard, True), ("cornellbox_builtin", PT.MIS, True),
           ("bistro_class_small", PT.Standard, False), ("bistro_class_small", PT.MIS, False),
           ("features1", PT.Standard, False), ("features1", PT.MIS, False),
           ("materials4", PT.Standard, False), ("materials4", PT.MIS, False)]


@pytest.fixture(scope="module")
def global_ctx(built):
    """A context whose kernels read every scene from global memory (GeoGlobal), as tests/test_light_probe.py makes one."""
    old = os.environ.get("LUPIN_LDS_GEOMETRY")
    os.environ["LUPIN_LDS_GEOMETRY"] = "0"     # read at context creation: small scenes stay in global memory
    try:
        ctx = api.Context(0)
    finally:
        if old is None:
            os.environ.pop("LUPIN_LDS_GEOMETRY", None)
        else:
            os.environ["LUPIN_LDS_GEOMETRY"] = old
    yield ctx
    for key in [k for k in util._scene_cache if k[1] == id(ctx)]:
        del util._scene_cache[key]
    ctx.close()


def bsdf_families(scene):
    """Material types among the scene's instances: from four on, the library sorts the queue into shade order before
    k_shade and keeps the path state as records (lupin_hip_scene_create; LUPIN_SORT_SHADE would override it)."""
    n = int(scene.desc.num_materials)
    mats = np.frombuffer((C.c_char * (n * _abi.MATERIAL_DTYPE.itemsize)).from_address(scene.desc.materials), _abi.MATERIAL_DTYPE)
    return {int(t) & 0xF for t in mats["mat_type"][scene.instances["mat_idx"]]}


# The accessor the default context gives each scene: only the Cornell box (36 triangles) fits a block's LDS; the others
# (156 340 to 432 142 triangles) are read from global memory by the persistent tracer.  The Cornell box also runs on the
# global context, so that both accessors are compared with the oracle on the same records.
STAGED_BY_DEFAULT = {"cornellbox_builtin": True, "bistro_class_small": False, "features1": False, "materials4": False}
# Scenes whose instances show four or more BSDF families: the shade-order sort runs, the path state is kept as records.
SORTED = {"cornellbox_builtin": False, "bistro_class_small": True, "features1": True, "materials4": False}
PER_RAY_LEGS = [(n, t, l, "default") for n, t, l in PER_RAY] + [(n, t, l, "global") for n, t, l in PER_RAY if n == "cornellbox_builtin" and not l]


@pytest.mark.gpu
@pytest.mark.parametrize("name,ptype,thin_lens,leg", PER_RAY_LEGS,
                         ids=[f"{n}-{t.name}{'-thinlens' if l else ''}{'-global' if g == 'global' else ''}" for n, t, l, g in PER_RAY_LEGS])
def test_per_ray_equals_the_oracle_bit_for_bit(gpu_ctx, global_ctx, name, ptype, thin_lens, leg):
    ctx = gpu_ctx if leg == "default" else global_ctx
    scene, cams = util.load_scene(name, ctx)
    cam = cams[0]
    params = cam.params
    if thin_lens:
        params = api.CameraParams(**{**cam.params.__dict__, "aperture": 0.05, "focus": 3.0})
    # the accessor of this leg: GeoLds or GeoGlobal
    assert staged_in_lds(ctx, scene) == (STAGED_BY_DEFAULT[name] and leg == "default"), (name, leg)
    # whether the shade-order sort runs on this scene
    assert os.environ.get("LUPIN_SORT_SHADE") is None and os.environ.get("LUPIN_PATH_RECORDS") is None
    assert (len(bsdf_families(scene)) >= 4) == SORTED[name], (name, bsdf_families(scene))
    rec = camera_records(scene, params, cam.transform)
    if thin_lens:
        assert len(np.unique(rec[:, 0:3], axis=0)) > 100       # the origins are on the lens, not in one point
    want = oracle_colours(scene, params, cam.transform, ptype)
    got = api.pathtrace_rays(ctx, scene, rec, api.RayQueryDesc(ptype, 8, 1))
    assert got.shape == (W * H, 4) and np.all(got[:, 3] == 1.0)
    assert float(want.max()) > 0.0
    assert_same_words(got[:, :3], want, f"{name} / {ptype.name} / {leg}")


@pytest.mark.gpu
def test_a_record_does_not_notice_its_slot(gpu_ctx):
    scene, _, rec, want = cornell(gpu_ctx)
    rng = np.random.default_rng(3)
    assert api.pathtrace_rays(gpu_ctx, scene, rec[:0]).shape == (0, 4)          # n = 0: nothing happens
    for n in (1, 63, 64, 65, 257, 1000):
        pick = rng.permutation(len(rec))[:n]
        got = api.pathtrace_rays(gpu_ctx, scene, rec[pick], api.RayQueryDesc(PT.Standard, 8, 1))
        assert_same_words(got[:, :3], want[pick], f"{n} shuffled records")


def sampled_reference(ctx, scene, rec, S, desc_kw):
    """The f32 sum, in order, of S one-sample queries seeded by the stated recurrence, divided by S."""
    total = np.zeros((len(rec), 3), np.float32)
    for s in range(S):
        r = rec.copy()
        r.view(np.uint32)[:, 3] = api.ray_sample_seed(rec.view(np.uint32)[:, 3], s)
        total = total + api.pathtrace_rays(ctx, scene, r, api.RayQueryDesc(samples=1, **desc_kw))[:, :3]
    return total / np.float32(S)


@pytest.mark.gpu
def test_samples_are_the_ordered_mean_of_single_paths(gpu_ctx):
    scene, _, rec, _ = cornell(gpu_ctx)
    rec = rec[np.random.default_rng(4).permutation(len(rec))[:300]]
    kw = dict(pathtrace_type=PT.Standard, max_bounces=8)
    got = api.pathtrace_rays(gpu_ctx, scene, rec, api.RayQueryDesc(samples=5, **kw))
    assert_same_words(got[:, :3], sampled_reference(gpu_ctx, scene, rec, 5, kw), "S = 5")


@pytest.mark.gpu
def test_chunks_do_not_change_the_result(gpu_ctx):
    scene, _, rec, _ = cornell(gpu_ctx)
    rec = rec[np.random.default_rng(5).permutation(len(rec))[:1000]]
    whole, whole_rays = api.pathtrace_rays(gpu_ctx, scene, rec, api.RayQueryDesc(PT.MIS, 8, 5), want_rays=True)
    for max_slots in (1003, 3):       # 200 whole records per wavefront (not a multiple of 256 slots); below S: one record each
        got, rays = api.pathtrace_rays(gpu_ctx, scene, rec, api.RayQueryDesc(PT.MIS, 8, 5, 0, max_slots), want_rays=True)
        assert_same_words(got, whole, f"max_slots = {max_slots}")
        assert_same_words(rays, whole_rays, f"first rays, max_slots = {max_slots}")


def empty_scene_with_environment(ctx, emission=0.5):
    key = ("env", emission)
    if key not in _cache:
        cpu = api.SceneCPU()
        env = api.default_environment()
        env["emission"] = (emission, emission, emission)
        cpu.environments = np.array([env], _abi.ENVIRONMENT_DTYPE)
        _cache[key] = api.build_accel_structures_and_upload(ctx, cpu, [], [api.EnvMapInfo(np.ones((1, 1, 4), np.float32), 1, 1)], True)
    return _cache[key]


NORMALS = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [1, 2, 3], [-2, 1, -0.5], [1e-3, -1e-3, -1], [0.6, 0, 0.8]], np.float64)
NORMALS /= np.linalg.norm(NORMALS, axis=1, keepdims=True)


def frame_of(n):
    """An orthonormal frame (float64) with z = n."""
    a = np.array([1.0, 0, 0]) if abs(n[0]) < 0.9 else np.array([0, 1.0, 0])
    x = np.cross(a, n)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(n, x), n])


@pytest.mark.gpu
def test_hemisphere_mode_replays_and_is_cosine_weighted(gpu_ctx):
    # (i) replay on the Cornell box: normals = the camera directions, origins = the camera origins
    scene, _, rec, _ = cornell(gpu_ctx)
    rec = rec[np.random.default_rng(6).permutation(len(rec))[:400]].copy()
    rec.view(np.uint32)[:, 7] = int(api.RayMode.COSINE_HEMISPHERE)
    S = 3
    kw = dict(pathtrace_type=PT.Standard, max_bounces=8)
    got, rays = api.pathtrace_rays(gpu_ctx, scene, rec, api.RayQueryDesc(samples=S, **kw), want_rays=True)
    assert rays.shape == (len(rec) * S, 8) and np.all(rays.view(np.uint32)[:, 7] == 0)
    assert_same_words(rays[:, 0:3], np.repeat(rec[:, 0:3], S, axis=0), "origins of the first rays")
    single = api.pathtrace_rays(gpu_ctx, scene, rays, api.RayQueryDesc(samples=1, **kw))[:, :3].reshape(len(rec), S, 3)
    mean = np.zeros((len(rec), 3), np.float32)
    for s in range(S):
        mean = mean + single[:, s]
    assert_same_words(got[:, :3], mean / np.float32(S), "mode-1 result against the replayed paths")
    # the RNG state handed back is the slot's seed advanced by the two draws
    seeds = api.ray_sample_seed(np.repeat(rec.view(np.uint32)[:, 3], S), np.tile(np.arange(S, dtype=np.uint32), len(rec)))
    assert np.array_equal(rays.view(np.uint32)[:, 3], pcg_advance(seeds, 2))

    # (ii) the directions: unit, in the hemisphere, cosine-weighted (and not uniform)
    env = empty_scene_with_environment(gpu_ctx)
    N = 100_000
    qd, qbin, domega = stats.sphere_quadrature()
    nbins = 2 * stats.NC * stats.NPHI
    exp_cos = np.bincount(qbin, np.maximum(qd[:, 2], 0.0) / math.pi * domega, nbins) * N
    exp_uni = np.bincount(qbin, (qd[:, 2] > 0.0) / (2 * math.pi) * domega, nbins) * N
    alpha = 1e-3 / len(NORMALS)
    for k, n in enumerate(NORMALS):
        r = api.ray_records(np.zeros((N, 3)), np.tile(n, (N, 1)), api.rng_seed_for(np.arange(N, dtype=np.uint32), 100 + k), api.RayMode.COSINE_HEMISPHERE)
        _, first = api.pathtrace_rays(gpu_ctx, env, r, api.RayQueryDesc(PT.Naive, 1, 1), want_rays=True)
        d = first[:, 4:7].astype(np.float64)
        assert np.all(np.abs(np.linalg.norm(d, axis=1) - 1.0) <= 1e-6), n
        n32 = r[0, 4:7].astype(np.float64)
        assert np.all(d @ n32 >= -1e-6), n
        local = d @ frame_of(n32 / np.linalg.norm(n32)).T
        obs = np.bincount(stats.sphere_bin(local), minlength=nbins)
        stat, dof, p = stats.chi2_pooled(obs, exp_cos)
        _, _, p_uniform = stats.chi2_pooled(obs, exp_uni)
        print(f"normal {n}: chi2 {stat:.1f} / {dof} dof, p = {p:.3g}; taken for uniform: p = {p_uniform:.3g}")
        assert p > alpha, (n, p)
        assert p_uniform < alpha, (n, p_uniform)


@pytest.mark.gpu
def test_constant_environment_returns_itself(gpu_ctx):
    env = empty_scene_with_environment(gpu_ctx)
    rng = np.random.default_rng(8)
    d = rng.normal(size=(500, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    for mode in (api.RayMode.DIRECTION, api.RayMode.COSINE_HEMISPHERE):
        rec = api.ray_records(rng.uniform(-5, 5, (500, 3)), d, rng.integers(0, 2 ** 32, 500, dtype=np.uint64).astype(np.uint32), mode)
        for S in (1, 7):
            for ptype in (PT.Standard, PT.Naive):
                got = api.pathtrace_rays(gpu_ctx, env, rec, api.RayQueryDesc(ptype, 8, S))
                assert np.all(got[:, :3] == np.float32(0.5)) and np.all(got[:, 3] == 1.0), (mode, S, ptype)


L_EMIT = 3.0


def emitter_scene(ctx):
    """A 2 x 2 emitter of radiance L_EMIT at height 1 above the origin, facing down (the winding of the Cornell box's
    light); its colour is black, so a path that reaches it ends there.  No environment."""
    if "emitter" not in _cache:
        cpu = api.SceneCPU()
        m = api.default_material()
        m["emission"] = (L_EMIT, L_EMIT, L_EMIT, 0.0)
        cpu.materials = np.array([m], _abi.MATERIAL_DTYPE)
        v = np.zeros((4, 4), np.float32)
        v[:, :3] = [(-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1)]
        cpu.verts_pos_array.append(v)
        cpu.indices_array.append(np.array([0, 2, 1, 2, 0, 3], np.uint32))
        cpu.mesh_infos = np.array([api.default_mesh_info()], _abi.MESH_INFO_DTYPE)
        cpu.instances = np.array([api.default_instance()], _abi.INSTANCE_DTYPE)
        api.validate_scene(cpu, 0, 0)
        _cache["emitter"] = api.build_accel_structures_and_upload(ctx, cpu, [], [], True)
    return _cache["emitter"]


def form_factor_quadrature(m=2000):
    """Cosine-weighted fraction of the hemisphere the emitter fills, seen from the origin: the integral of
    cos cos' / (pi r^2) over the square, midpoint rule in float64."""
    x = (np.arange(m) + 0.5) / m * 2.0 - 1.0
    xx, zz = np.meshgrid(x, x)
    return float(np.sum(1.0 / (math.pi * (xx * xx + zz * zz + 1.0) ** 2)) * (2.0 / m) ** 2)


@pytest.mark.gpu
def test_irradiance_under_a_square_emitter(gpu_ctx):
    F = 4.0 * (1.0 / (2.0 * math.pi)) * 2.0 * (1.0 / math.sqrt(2.0)) * math.atan(1.0 / math.sqrt(2.0))
    assert abs(F - 0.5541) < 1e-4 and abs(form_factor_quadrature() - F) < 1e-6
    scene = emitter_scene(gpu_ctx)
    R, S = 16, 4096
    sigma = math.sqrt(F * (1.0 - F) / (R * S))
    points, normals = np.zeros((R, 3), np.float32), np.tile(np.float32([0, 1, 0]), (R, 1))
    rec = api.ray_records(points, normals, api.rng_seed_for(np.arange(R, dtype=np.uint32), 0), api.RayMode.COSINE_HEMISPHERE)
    adv = api.AdvancedParams(max_radiance=2.0 * L_EMIT)
    for ptype in (PT.Naive, PT.Standard):
        got = api.pathtrace_rays(gpu_ctx, scene, rec, api.RayQueryDesc(ptype, 8, S, 0, 0, adv))
        assert np.all(got[:, 0] == got[:, 1]) and np.all(got[:, 1] == got[:, 2])
        ratio = float(got[:, 0].astype(np.float64).mean() / L_EMIT)
        print(f"{ptype.name}: mean / L = {ratio:.5f}, F = {F:.5f}, sigma = {sigma:.5f}")
        assert abs(ratio - F) <= 4.0 * sigma, (ptype, ratio, F, sigma)
        baked = api.bake_irradiance(gpu_ctx, scene, points, normals, S, ptype, 8, adv)
        assert baked.shape == (R, 3)
        assert_same_words(baked, np.float32(np.pi) * got[:, :3], "bake_irradiance = pi * the mean radiance")


class DeviceArray:
    """Device memory of the context without another runtime in the process: the texels of a texture (8 bytes each)."""

    def __init__(self, ctx, nbytes):
        self.rows = max(1, (nbytes + 31) // 32)
        self.tex = api.Texture(ctx, 4, self.rows)
        self.ptr = self.tex.device_ptr()
        assert self.ptr and self.ptr % 16 == 0

    def upload(self, a):
        raw = np.zeros(self.rows * 32, np.uint8)
        b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        raw[:len(b)] = b
        self.tex.upload(raw.view(np.float16).reshape(self.rows, 4, 4))
        return self

    def download(self, dtype, count):
        return self.tex.download().view(np.uint8).reshape(-1)[:count * np.dtype(dtype).itemsize].view(dtype).copy()


def device_query(ctx, scene, rec, desc, want_rays=False, sentinel=None):
    """lupin_hip_pathtrace_rays with LUPIN_RAYS_DEVICE_POINTERS on texture memory: (status, out, rays)."""
    n, S = len(rec), int(desc.samples)
    d_rec = DeviceArray(ctx, rec.nbytes).upload(rec)
    d_out = DeviceArray(ctx, n * 16)
    if sentinel is not None:
        d_out.upload(np.full(n * 4, sentinel, np.float32))
    d_rays = DeviceArray(ctx, n * S * 32) if want_rays else None
    c = _abi.RayQueryDescC(int(desc.pathtrace_type), desc.max_bounces, S, int(desc.flags) | api.RAYS_DEVICE_POINTERS, desc.max_slots,
                           _abi.AdvancedParamsC(desc.advanced.max_radiance, desc.advanced.rng_seed, desc.advanced.ray_epsilon))
    rc = _abi.lib().lupin_hip_pathtrace_rays(ctx.handle, scene.handle, C.byref(c), n, C.c_void_p(d_rec.ptr), C.c_void_p(d_out.ptr),
                                             C.c_void_p(d_rays.ptr) if want_rays else None)
    out = d_out.download(np.float32, n * 4).reshape(n, 4)
    rays = d_rays.download(np.float32, n * S * 8).reshape(n * S, 8) if want_rays else None
    return rc, out, rays


@pytest.mark.gpu
def test_device_pointers_give_the_same_words(gpu_ctx):
    scene, _, rec, _ = cornell(gpu_ctx)
    rec = rec[np.random.default_rng(9).permutation(len(rec))[:777]].copy()
    rec.view(np.uint32)[::2, 7] = int(api.RayMode.COSINE_HEMISPHERE)
    desc = api.RayQueryDesc(PT.MIS, 8, 3, 0, 1000)
    want, want_rays = api.pathtrace_rays(gpu_ctx, scene, rec, desc, want_rays=True)
    rc, got, rays = device_query(gpu_ctx, scene, rec, desc, want_rays=True)
    assert rc == 0, _abi.lib().lupin_hip_last_error()
    assert_same_words(got, want, "device pointers")
    assert_same_words(rays, want_rays, "first rays through device pointers")
    rc, got, _ = device_query(gpu_ctx, scene, rec, desc)
    assert rc == 0
    assert_same_words(got, want, "device pointers without out_rays")


@pytest.mark.gpu
def test_torch_tensors_give_the_same_words(built):
    """Tensors on the device through api.pathtrace_rays, in a process of its own: torch brings its own HIP runtime, and a
    process with two of them cannot create further contexts."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_ray_query_torch_worker.py")], capture_output=True, text=True, timeout=600,
                         cwd=ROOT)
    assert out.returncode == 0 and "RAY QUERY TORCH OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_validation_refuses_before_anything_is_traced(gpu_ctx):
    scene, cam, rec, want = cornell(gpu_ctx)
    rec = rec[:64].copy()
    lib = _abi.lib()
    INVALID = -1

    def raw(ctx_h, scene_h, desc, n, records, out, flags=0, **over):
        f = dict(pathtrace_type=0, max_bounces=8, samples=1, flags=flags, max_slots=0)
        f.update(over)
        c = _abi.RayQueryDescC(f["pathtrace_type"], f["max_bounces"], f["samples"], f["flags"], f["max_slots"], _abi.AdvancedParamsC(100.0, 0, 0.001))
        return lib.lupin_hip_pathtrace_rays(ctx_h, scene_h, C.byref(c) if desc else None, n, _abi.ptr(records), _abi.ptr(out), None)

    def fresh():
        return np.full((len(rec), 4), -7.0, np.float32)

    cases = []
    out = fresh(); cases.append(("null context", raw(None, scene.handle, True, 64, rec, out), out))
    out = fresh(); cases.append(("null scene", raw(gpu_ctx.handle, None, True, 64, rec, out), out))
    out = fresh(); cases.append(("null desc", raw(gpu_ctx.handle, scene.handle, False, 64, rec, out), out))
    out = fresh(); cases.append(("null records", raw(gpu_ctx.handle, scene.handle, True, 64, None, out), out))
    out = fresh(); cases.append(("null out", raw(gpu_ctx.handle, scene.handle, True, 64, rec, None), out))
    out = fresh(); cases.append(("unknown integrator", raw(gpu_ctx.handle, scene.handle, True, 64, rec, out, pathtrace_type=4), out))
    out = fresh(); cases.append(("unknown flag", raw(gpu_ctx.handle, scene.handle, True, 64, rec, out, flags=2), out))
    out = fresh(); cases.append(("samples == 0", raw(gpu_ctx.handle, scene.handle, True, 64, rec, out, samples=0), out))
    out = fresh(); cases.append(("max_bounces == 4095", raw(gpu_ctx.handle, scene.handle, True, 64, rec, out, max_bounces=4095), out))
    out = fresh(); cases.append(("samples above 2^27", raw(gpu_ctx.handle, scene.handle, True, 64, rec, out, samples=(1 << 27) + 1), out))
    out = fresh(); cases.append(("n * samples too large", raw(gpu_ctx.handle, scene.handle, True, (1 << 38) // 4 + 1, rec, out, samples=4), out))
    other = api.Context(0)
    foreign, _ = loader.build_scene_cornell_box(other)
    out = fresh(); cases.append(("scene of another context", raw(gpu_ctx.handle, foreign.handle, True, 64, rec, out), out))
    other.close()
    out = fresh(); cases.append(("scene of a destroyed context", raw(gpu_ctx.handle, foreign.handle, True, 64, rec, out), out))
    bad_records = {}
    for label, col, value in (("NaN origin", 1, np.nan), ("infinite direction", 5, np.inf), ("NaN normal", 6, np.nan)):
        r = rec.copy(); r[17, col] = value
        bad_records[label] = r
    r = rec.copy(); r[40, 4:7] *= np.float32(1.001)
    bad_records["direction too long"] = r
    r = rec.copy(); r[3, 4:7] = 0.0
    bad_records["zero normal"] = r
    r = rec.copy(); r.view(np.uint32)[63, 7] = 2
    bad_records["unknown mode"] = r
    for label, r in bad_records.items():
        out = fresh(); cases.append((label + " (host check)", raw(gpu_ctx.handle, scene.handle, True, 64, r, out), out))
        rc, dout, _ = device_query(gpu_ctx, scene, r, api.RayQueryDesc(), sentinel=-7.0)
        cases.append((label + " (device check)", rc, dout))
    # device pointers that are not 16-byte aligned: each of the three in turn
    d_rec = DeviceArray(gpu_ctx, rec.nbytes + 32).upload(np.concatenate([np.zeros(8, np.float32), rec.reshape(-1)]))
    d_out = DeviceArray(gpu_ctx, 64 * 16 + 32).upload(np.full(64 * 4 + 8, -7.0, np.float32))
    d_rays = DeviceArray(gpu_ctx, 64 * 32 + 32)
    cdev = _abi.RayQueryDescC(0, 8, 1, api.RAYS_DEVICE_POINTERS, 0, _abi.AdvancedParamsC(100.0, 0, 0.001))
    for label, offs in (("records", (8, 0, 0)), ("out", (0, 8, 0)), ("out_rays", (0, 0, 8))):
        rc = lib.lupin_hip_pathtrace_rays(gpu_ctx.handle, scene.handle, C.byref(cdev), 64, C.c_void_p(d_rec.ptr + 32 + offs[0]),
                                          C.c_void_p(d_out.ptr + offs[1]), C.c_void_p(d_rays.ptr + offs[2]))
        cases.append((f"unaligned device pointer: {label}", rc, d_out.download(np.float32, 64 * 4 + 8)))
    for label, rc, out in cases:
        assert rc == INVALID, (label, rc)
        assert lib.lupin_hip_last_error()
        assert np.all(out == -7.0), label
    # a direction within the tolerance passes, and its RNG word may be any bit pattern
    r = rec.copy(); r[40, 4:7] *= np.float32(1.00004); r.view(np.uint32)[5, 3] = 0x7FC00000
    assert raw(gpu_ctx.handle, scene.handle, True, 64, r, fresh()) == 0
    # what follows is unharmed: the same query, and a render against the oracle
    assert_same_words(api.pathtrace_rays(gpu_ctx, scene, rec)[:, :3], want[:64], "query after the refusals")
    got = util.gpu_accumulate(gpu_ctx, scene, cam, W, H, frames=2, spp=2)
    assert util.f16_words_differ(got, util.oracle_accumulate(scene, cam, W, H, frames=2, spp=2)) == 0


def chain_bvh(verts, indices):
    """A BLAS in the reference's node format that is one long chain: inner node k (index 2k) has the leaf of triangle k
    (index 2k + 1) and inner node k + 1 (index 2k + 2) as children; the last inner node ends in two leaves."""
    tris = np.asarray(indices, np.uint32).reshape(-1, 3)
    T = len(tris)
    p = verts[:, :3][tris]                                   # (T, 3, 3)
    lo, hi = p.min(axis=1), p.max(axis=1)
    lo_from, hi_from = np.minimum.accumulate(lo[::-1])[::-1], np.maximum.accumulate(hi[::-1])[::-1]     # bounds of triangles k ..
    nodes = np.zeros(2 * T - 1, _abi.BVH_NODE_DTYPE)

    def leaf(i, t):
        nodes[i] = (lo[t], t, hi[t], 1)
    for k in range(T - 1):
        nodes[2 * k] = (lo_from[k], 2 * k + 1, hi_from[k], 0)
        leaf(2 * k + 1, k)
    leaf(2 * T - 2, T - 1)
    return nodes, tris.reshape(-1).copy()


def deep_chain_scene(ctx):
    """200 triangles in a chain of depth 200: more stack than a block's LDS holds, so every traversal of it is refused."""
    cpu = api.SceneCPU()
    m = api.default_material()
    m["color"] = (0.5, 0.5, 0.5, 1.0)
    cpu.materials = np.array([m], _abi.MATERIAL_DTYPE)
    T = 200
    v = np.zeros((3 * T, 4), np.float32)
    for t in range(T):
        v[3 * t:3 * t + 3, :3] = [(t, 0, 0), (t + 0.9, 0, 0), (t, 0.9, 0)]
    cpu.verts_pos_array.append(v)
    cpu.indices_array.append(np.arange(3 * T, dtype=np.uint32))
    cpu.mesh_infos = np.array([api.default_mesh_info()], _abi.MESH_INFO_DTYPE)
    cpu.instances = np.array([api.default_instance()], _abi.INSTANCE_DTYPE)
    return api.build_accel_structures_and_upload(ctx, cpu, [], [], True, blas_builder=chain_bvh)


@pytest.mark.gpu
def test_a_tree_too_deep_is_refused_as_a_render_refuses_it(gpu_ctx):
    """The query gives the render's error, and so does the call that runs a batch the render was only recorded into."""
    scene = deep_chain_scene(gpu_ctx)
    rec = api.ray_records([[0.2, 0.2, 1.0]], [[0, 0, -1.0]])
    with pytest.raises(api.LupinError) as query:
        api.pathtrace_rays(gpu_ctx, scene, rec)
    res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=2, samples_per_pixel=1))
    target = api.Texture(gpu_ctx, 8, 8)
    gpu_ctx.set_batch_frames(1)           # the render's error at the call itself, not at the flush of a batch
    try:
        with pytest.raises(api.LupinError) as render:
            api.pathtrace_scene(gpu_ctx, res, scene, target, PT.Standard, api.PathtraceDesc())
    finally:
        gpu_ctx.set_batch_frames(0)
    assert query.value.code == render.value.code == -1
    assert "too deep" in str(query.value) and str(query.value) == str(render.value)
    # default batching: the render is recorded and returns; its error is reported by the call that runs the batch
    api.pathtrace_scene(gpu_ctx, res, scene, target, PT.Standard, api.PathtraceDesc())
    with pytest.raises(api.LupinError) as sync:
        gpu_ctx.sync()
    assert sync.value.code == query.value.code and str(sync.value) == str(query.value)
    gpu_ctx.sync()                        # the batch was dropped with its error


@pytest.mark.gpu
def test_frames_around_a_query_do_not_notice_it(gpu_ctx):
    scene, cam, rec, want = cornell(gpu_ctx)

    def chain(query_after):
        res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=8, samples_per_pixel=2))
        out = api.DoubleBufferedTexture(gpu_ctx, W, H)
        for k in range(6):
            desc = api.PathtraceDesc(accum_params=api.AccumulationParams(out.back(), k), camera_params=cam.params, camera_transform=cam.transform)
            api.pathtrace_scene(gpu_ctx, res, scene, out.front(), PT.Standard, desc)
            out.flip()
            if k + 1 == query_after:
                got = api.pathtrace_rays(gpu_ctx, scene, rec, api.RayQueryDesc(PT.MIS, 8, 2))
                assert got.shape == (len(rec), 4)
        out.flip()
        return out.front().download()

    plain = chain(None)
    assert util.f16_words_differ(chain(3), plain) == 0
    assert util.f16_words_differ(plain, util.oracle_accumulate(scene, cam, W, H, frames=6, spp=2)) == 0
    assert_same_words(api.pathtrace_rays(gpu_ctx, scene, rec)[:, :3], want, "query after the frames")


@pytest.mark.gpu
def test_query_after_update_instances_equals_a_fresh_scene(gpu_ctx):
    cpu, cams = loader.cornell_box_scene_cpu()
    a = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], [], True)
    moved_cpu, _ = loader.cornell_box_scene_cpu()
    t = moved_cpu.instances["transpose_inverse_transform"].copy()
    t[5, :, 3] = (0.2, 0.0, 0.1)        # the short box: world -> local subtracts the offset
    t[6, :, 3] = (-0.1, -0.3, 0.0)      # the tall box, lifted
    moved_cpu.instances["transpose_inverse_transform"] = t
    b = api.build_accel_structures_and_upload(gpu_ctx, moved_cpu, [], [], True)
    rec = camera_records(a, cams[0].params, cams[0].transform)
    desc = api.RayQueryDesc(PT.MIS, 8, 2)
    before = api.pathtrace_rays(gpu_ctx, a, rec, desc)
    a.update_instances(t)
    after = api.pathtrace_rays(gpu_ctx, a, rec, desc)
    fresh = api.pathtrace_rays(gpu_ctx, b, rec, desc)
    assert int((words(before) != words(fresh)).sum()) > 100      # the move is visible
    assert_same_words(after, fresh, "updated scene against a freshly created moved scene")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 65])
def test_a_refused_call_names_its_records_and_leaves_recorded_frames_intact(gpu_ctx, S):
    """Frames recorded and not yet run, then a query refused for its records: host arrays name the first bad index, device
    arrays count the bad records, `out` stays untouched, and the frames are what they are without the call.  (What a
    query returns is checked by the tests above; this one is about the refusal.)"""
    scene, cam, rec, _ = cornell(gpu_ctx)
    rec = rec[100:107].copy()
    if S > 1:
        rec.view(np.uint32)[:, 7] = int(api.RayMode.COSINE_HEMISPHERE)
    desc = api.RayQueryDesc(PT.Standard, 4, S)
    alone = api.pathtrace_rays(gpu_ctx, scene, rec, desc)
    bad = rec.copy(); bad[3, 1] = np.nan; bad.view(np.uint32)[5, 7] = 2
    lib = _abi.lib()

    def host_refusal():
        out = np.full((7, 4), -7.0, np.float32)
        c = _abi.RayQueryDescC(int(PT.Standard), 4, S, 0, 0, _abi.AdvancedParamsC(100.0, 0, 0.001))
        assert lib.lupin_hip_pathtrace_rays(gpu_ctx.handle, scene.handle, C.byref(c), 7, _abi.ptr(bad), _abi.ptr(out), None) == -1
        assert lib.lupin_hip_last_error().decode().startswith("record 3: ") and np.all(out == -7.0)

    def device_refusal():
        rc, out, _ = device_query(gpu_ctx, scene, bad, desc, sentinel=-7.0)
        assert rc == -1 and lib.lupin_hip_last_error().decode().startswith("2 record(s): ") and np.all(out == -7.0)

    plain = util.gpu_accumulate(gpu_ctx, scene, cam, 32, 24, frames=4, spp=1)
    for refusal in (host_refusal, device_refusal):
        assert util.f16_words_differ(util.gpu_accumulate(gpu_ctx, scene, cam, 32, 24, frames=4, spp=1, between=refusal), plain) == 0
    assert_same_words(api.pathtrace_rays(gpu_ctx, scene, rec, desc), alone, "the query after the refusals")
