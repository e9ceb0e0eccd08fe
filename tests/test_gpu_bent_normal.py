"""Bent-normal queries on the device (lupin_hip_bent_normal_rays): the four sums are the restated 64-lane
sum of tests/bent_normal_ref.py over the slots' own directions and weights, bit for bit; .w is the existing queries' answer;
the words do not depend on the launch cut, on where the geometry is staged or on how the scene came to its transforms;
the closed forms under an open sky and at the foot of a wall; api.bent_normals; torch tensors; every refusal."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import bent_normal_ref as B
from tests import closest_hit_ref as X
from tests import transmittance_ref as TR
from tests import util
from tests.test_gpu_closest_hit import staged_in_lds
from tests.test_gpu_occlusion import upload
from tests.test_gpu_ray_query import DeviceArray, chain_bvh
from tests.test_gpu_transmittance import device_scene, global_ctx, hemisphere_records   # noqa: F401  (global_ctx is a fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODE = api.OcclusionMode
PT = api.PathtraceType
SENTINEL = 0xABCDABCD
SAMPLES = (1, 2, 63, 64, 65, 129, 1000)
CLOSED_SAMPLES = 65536
DEVICE, OPACITY = api.BENT_NORMAL_DEVICE_POINTERS, api.BENT_NORMAL_OPACITY


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def device_bent(ctx, scene, rec, S, flags=0, eps=1e-3, max_slots=0, sentinel=None):
    """lupin_hip_bent_normal_rays with LUPIN_BENT_NORMAL_DEVICE_POINTERS: (status, (n, 4) u32 words)."""
    n = len(rec)
    d_rec = DeviceArray(ctx, rec.nbytes).upload(rec)
    d_out = DeviceArray(ctx, n * 16)
    if sentinel is not None:
        d_out.upload(np.full(4 * n, sentinel, np.uint32))
    c = _abi.BentNormalDescC(S, flags | DEVICE, max_slots, eps)
    rc = _abi.lib().lupin_hip_bent_normal_rays(ctx.handle, scene.handle, C.byref(c), n, C.c_void_p(d_rec.ptr), C.c_void_p(d_out.ptr))
    return rc, d_out.download(np.uint32, 4 * n).reshape(n, 4)


def slot_weights(ctx, scene, rec, S, opacity):
    """Per record the slots' directions (6, S, 3), from the radiance query, and weights (6, S), from the direction-mode queries."""
    qrec = rec.copy()
    qrec.view(np.uint32)[:, 7] = int(api.RayMode.COSINE_HEMISPHERE)
    _, rays = api.pathtrace_rays(ctx, scene, qrec, api.RayQueryDesc(PT.Naive, 0, S), want_rays=True)
    single = api.occlusion_records(rays[:, 0:3], rays[:, 4:7], np.repeat(rec[:, 7], S))
    if opacity:
        T = api.transmittance_rays(ctx, scene, single, MODE.DIRECTION, 1)
    else:
        T = np.float32(1.0) - api.occlusion_rays(ctx, scene, single, MODE.DIRECTION, 1).astype(np.float32)
    return rays[:, 4:7].reshape(len(rec), S, 3), T.reshape(len(rec), S)


# ---- the restated sum -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("opacity", [False, True])
@pytest.mark.parametrize("S", SAMPLES)
@pytest.mark.parametrize("kind", ["big", "small"])
def test_the_four_sums_are_the_restated_order_over_the_slots_own_rays(gpu_ctx, kind, S, opacity):
    scene, rec = hemisphere_records(gpu_ctx, kind)
    assert staged_in_lds(gpu_ctx, scene) == (kind == "small")
    got = api.bent_normal_rays(gpu_ctx, scene, rec, S, opacity=opacity)
    assert got.shape == (6, 4) and got.dtype == np.float32
    dirs, T = slot_weights(gpu_ctx, scene, rec, S, opacity)
    want = np.stack([B.resolve_f32(T[i], dirs[i]) for i in range(6)])
    assert np.array_equal(words(got), words(want)), (got, want)
    rc, dev = device_bent(gpu_ctx, scene, rec, S, OPACITY if opacity else 0)
    assert rc == 0 and np.array_equal(dev, words(got))
    if S == 1000:
        assert (T == 0).any() and (T == 1).any() and (not opacity or ((T > 0) & (T < 1)).sum() > 100)
        assert not np.array_equal(words(want), words(np.stack([B.sequential_f32(T[i], dirs[i]) for i in range(6)])))     # the order shows here


@pytest.mark.parametrize("S", [2, 65, 1000])
@pytest.mark.parametrize("kind", ["big", "small"])
def test_w_is_the_existing_queries_answer(gpu_ctx, kind, S):
    scene, rec = hemisphere_records(gpu_ctx, kind)
    with_op = api.bent_normal_rays(gpu_ctx, scene, rec, S, opacity=True)
    assert np.array_equal(words(with_op[:, 3]), words(api.transmittance_rays(gpu_ctx, scene, rec, MODE.COSINE_HEMISPHERE, S)))
    plain = api.bent_normal_rays(gpu_ctx, scene, rec, S)
    blocked = api.occlusion_rays(gpu_ctx, scene, rec, MODE.COSINE_HEMISPHERE, S)
    assert np.array_equal(words(plain[:, 3]), words((S - blocked.astype(np.int64)).astype(np.float32)))
    if S == 1000:
        assert 0 < blocked.sum() < 6 * S and (with_op[:, 3] >= plain[:, 3]).all() and (with_op[:, 3] > plain[:, 3]).any()
    opaque = device_scene(gpu_ctx, kind, opaque=True)
    assert np.array_equal(words(api.bent_normal_rays(gpu_ctx, opaque, rec, S, opacity=True)), words(api.bent_normal_rays(gpu_ctx, opaque, rec, S)))


def many_records(ctx, kind, n):
    scene, rec = hemisphere_records(ctx, kind)
    out = np.tile(rec, ((n + 5) // 6, 1))[:n].copy()
    out.view(np.uint32)[:, 3] = api.rng_seed_for(np.arange(n, dtype=np.uint32), 11)
    return scene, out


@pytest.mark.parametrize("opacity", [False, True])
def test_words_do_not_depend_on_the_launch_cut(gpu_ctx, opacity):
    """Four records per block: n around it and a partial last block; max_slots of one slot (a record per launch), one record,
    three records and a slot, and the default."""
    scene, rec = many_records(gpu_ctx, "small", 257)
    for S in (5, 70):
        whole = api.bent_normal_rays(gpu_ctx, scene, rec, S, opacity=opacity)
        assert len(np.unique(words(whole), axis=0)) > 200
        for n in (1, 3, 4, 5, 257):
            if n == 257 and S == 70:
                continue                                        # (257 launches of one record at S = 5 are enough)
            for max_slots in (1, S, 3 * S + 1, 0):
                got = api.bent_normal_rays(gpu_ctx, scene, rec[:n], S, opacity=opacity, max_slots=max_slots)
                assert np.array_equal(words(got), words(whole[:n])), (S, n, max_slots)
            rc, dev = device_bent(gpu_ctx, scene, rec[:n], S, OPACITY if opacity else 0, max_slots=3 * S + 1)
            assert rc == 0 and np.array_equal(dev, words(whole[:n])), (S, n)
    assert api.bent_normal_rays(gpu_ctx, scene, rec[:0], 5).shape == (0, 4)


def test_staged_and_global_geometry_give_the_same_words(gpu_ctx, global_ctx):   # noqa: F811
    staged, unstaged = device_scene(gpu_ctx, "small"), device_scene(global_ctx, "small")
    assert staged_in_lds(gpu_ctx, staged) and not staged_in_lds(global_ctx, unstaged)
    _, rec = hemisphere_records(gpu_ctx, "small")
    for S in (65, 1000):
        for opacity in (False, True):
            assert np.array_equal(words(api.bent_normal_rays(gpu_ctx, staged, rec, S, opacity=opacity)),
                                  words(api.bent_normal_rays(global_ctx, unstaged, rec, S, opacity=opacity))), (S, opacity)


@pytest.mark.parametrize("tlas_builder", ["cpu", "device"])
def test_moved_instances_give_the_words_of_a_fresh_scene(gpu_ctx, tlas_builder):
    """After Scene.update_instances the four-wide hierarchy is stale; the query reads the binary one only."""
    _, rec = hemisphere_records(gpu_ctx, "big")
    moved = X.transforms(X.SEED, moved=True)
    scene = TR.build("big", gpu_ctx)[2]                                  # a scene of its own: it is changed in place
    before = api.bent_normal_rays(gpu_ctx, scene, rec, 129, opacity=True)
    scene.update_instances(np.array(X.instance_records(moved)["transpose_inverse_transform"], np.float32).reshape(-1, 3, 4), tlas_builder=tlas_builder)
    fresh = TR.build("big", gpu_ctx, xf=moved)[2]
    for opacity in (False, True):
        assert np.array_equal(words(api.bent_normal_rays(gpu_ctx, scene, rec, 129, opacity=opacity)),
                              words(api.bent_normal_rays(gpu_ctx, fresh, rec, 129, opacity=opacity)))
    assert not np.array_equal(words(before), words(api.bent_normal_rays(gpu_ctx, scene, rec, 129, opacity=True)))     # the move is visible


# ---- closed forms -----------------------------------------------------------------------------------------------

def quad(corners):
    v = np.zeros((4, 4), np.float32)
    v[:, :3] = corners
    return v, np.array([0, 1, 2, 0, 2, 3], np.uint32)


TMAX = 1.0
FLOOR = quad([(-50, -50, 0), (50, -50, 0), (50, 50, 0), (-50, 50, 0)])
WALL_X = -1e-4       # a direction escapes the wall only with |d.x| < 1e-4 / TMAX: a share of 1e-4 of the blocked half, far inside the band
WALL = quad([(WALL_X, -2, 0), (WALL_X, 2, 0), (WALL_X, 2, 2), (WALL_X, -2, 2)])       # half-width 2 and height 2: above TMAX


@pytest.mark.parametrize("case", ["open_sky", "wall"])
def test_closed_forms_within_five_standard_errors(gpu_ctx, case):
    scene = upload(gpu_ctx, [FLOOR] if case == "open_sky" else [FLOOR, WALL])
    closed, twin = (B.OPEN_SKY, B.OPEN_SKY_UNIFORM) if case == "open_sky" else (B.WALL, B.WALL_UNIFORM)
    rec = api.occlusion_records([[0.0, 0.0, 1e-3]], [[0.0, 0.0, 1.0]], TMAX, api.rng_seed_for(np.arange(1, dtype=np.uint32), 5))
    se = B.standard_errors(closed, CLOSED_SAMPLES)
    for opacity in (False, True):
        got = api.bent_normal_rays(gpu_ctx, scene, rec, CLOSED_SAMPLES, ray_epsilon=0.0, opacity=opacity)[0].astype(np.float64) / CLOSED_SAMPLES
        print(case, "opacity" if opacity else "plain", "mean", got, "closed form", closed["mean"], "standard errors", se)
        assert (np.abs(got - closed["mean"]) <= B.SIGMAS * se).all()
        assert not (np.abs(got - twin) <= B.SIGMAS * se).all()           # a uniform-hemisphere sampler would land elsewhere
    if case == "open_sky":
        assert got[3] == 1.0                                             # nothing is blocked: the sum of ones is exact


# ---- the Python helpers -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["big", "small"])
def test_bent_normals_is_ambient_occlusion_and_a_unit_direction(gpu_ctx, kind):
    scene, rec = hemisphere_records(gpu_ctx, kind)
    p, n = rec[:, 0:3], rec[:, 4:7]
    for samples, radius in ((64, 4.0), (1000, np.inf), (1, 0.01)):
        ao, bent = api.bent_normals(gpu_ctx, scene, p, n, radius, samples=samples, surface_offset=0.0, opacity=True)
        want = api.ambient_occlusion(gpu_ctx, scene, p, n, radius, samples=samples, surface_offset=0.0, opacity=True)
        assert ao.dtype == np.float32 and ao.shape == (6,) and bent.shape == (6, 3) and np.array_equal(words(ao), words(want))
        unit = np.abs(np.linalg.norm(bent.astype(np.float64), axis=1) - 1.0) <= 1e-6
        assert (unit | (words(bent) == words(n)).all(axis=1)).all()
        assert (np.einsum("ij,ij->i", bent, n)[ao > 0] > 0).all()       # an open direction lies in the normal's hemisphere
    ao, bent = api.bent_normals(gpu_ctx, scene, p, n, 4.0, samples=64, surface_offset=0.0)
    assert np.array_equal(words(ao), words(api.ambient_occlusion(gpu_ctx, scene, p, n, 4.0, samples=64, surface_offset=0.0)))    # 64ths are exact


def test_torch_tensors_give_the_same_words():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_bent_normal_torch_worker.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "BENT NORMAL TORCH OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- refusals ---------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_the_output_untouched(gpu_ctx):
    c = TR.case("small")
    scene = device_scene(gpu_ctx, "small")
    rec = api.occlusion_records(c.ori[:64], c.dir[:64], 5.0)
    lib = _abi.lib()
    INVALID = -1

    def raw(ctx_h, scene_h, desc, n, records, out, samples=3, flags=0, eps=1e-3, max_slots=0):
        d = _abi.BentNormalDescC(samples, flags, max_slots, eps)
        return lib.lupin_hip_bent_normal_rays(ctx_h, scene_h, C.byref(d) if desc else None, n, _abi.ptr(records), _abi.ptr(out))

    def fresh():
        return np.full((len(rec), 4), SENTINEL, np.uint32)

    g, s = gpu_ctx.handle, scene.handle
    cases = []
    out = fresh(); cases.append(("null context", raw(None, s, True, 64, rec, out), out))
    out = fresh(); cases.append(("null scene", raw(g, None, True, 64, rec, out), out))
    out = fresh(); cases.append(("null desc", raw(g, s, False, 64, rec, out), out))
    out = fresh(); cases.append(("null records", raw(g, s, True, 64, None, out), out))
    out = fresh(); cases.append(("null out", raw(g, s, True, 64, rec, None), out))
    for flag in (4, 8, 1 << 31):
        out = fresh(); cases.append((f"unknown flag {flag}", raw(g, s, True, 64, rec, out, flags=flag), out))
    out = fresh(); cases.append(("samples == 0", raw(g, s, True, 64, rec, out, samples=0), out))
    out = fresh(); cases.append(("samples above 2^20", raw(g, s, True, 64, rec, out, samples=(1 << 20) + 1), out))
    out = fresh(); cases.append(("n * samples too large", raw(g, s, True, (1 << 38) // 4 + 1, rec, out, samples=4), out))
    for label, eps in (("NaN", np.nan), ("infinite", np.inf), ("negative", -1e-3)):
        out = fresh(); cases.append((f"{label} ray_epsilon", raw(g, s, True, 64, rec, out, eps=eps), out))
    other = api.Context(0)
    foreign = X.build("small", X.SEED, other)
    out = fresh(); cases.append(("scene of another context", raw(g, foreign.handle, True, 64, rec, out), out))
    other.close()
    out = fresh(); cases.append(("scene of a destroyed context", raw(g, foreign.handle, True, 64, rec, out), out))
    bad_records = {}
    for label, row, col, value in (("NaN origin", 17, 1, np.nan), ("infinite normal", 17, 5, np.inf), ("NaN normal", 63, 6, np.nan),
                                   ("NaN tmax", 0, 7, np.nan), ("zero tmax", 31, 7, 0.0), ("negative tmax", 31, 7, -1.0),
                                   ("minus infinite tmax", 5, 7, -np.inf)):
        r = rec.copy(); r[row, col] = value
        bad_records[label] = r
    r = rec.copy(); r[40, 4:7] *= np.float32(1.001)
    bad_records["normal too long"] = r
    r = rec.copy(); r[3, 4:7] = 0.0
    bad_records["zero normal"] = r
    for label, r in bad_records.items():
        for flags in (0, OPACITY):
            out = fresh(); cases.append((f"{label} (host check, flags {flags})", raw(g, s, True, 64, r, out, flags=flags), out))
            rc, dout = device_bent(gpu_ctx, scene, r, 3, flags, sentinel=SENTINEL)
            cases.append((f"{label} (device check, flags {flags})", rc, dout))
    d_rec = DeviceArray(gpu_ctx, rec.nbytes + 32).upload(np.concatenate([np.zeros(8, np.float32), rec.reshape(-1)]))
    d_out = DeviceArray(gpu_ctx, 64 * 16 + 32).upload(np.full(64 * 4 + 8, SENTINEL, np.uint32))
    cdev = _abi.BentNormalDescC(3, DEVICE, 0, 1e-3)
    for label, offs in (("records", (8, 0)), ("out by 4 bytes", (0, 4)), ("out by 8 bytes", (0, 8))):
        rc = lib.lupin_hip_bent_normal_rays(g, s, C.byref(cdev), 64, C.c_void_p(d_rec.ptr + 32 + offs[0]), C.c_void_p(d_out.ptr + offs[1]))
        cases.append((f"misaligned device pointer: {label}", rc, d_out.download(np.uint32, 64 * 4 + 8)))
    # a hierarchy too deep for the stack: 200 triangles in a chain (tests/test_gpu_ray_query.py)
    cpu = api.SceneCPU()
    cpu.materials = np.array([api.default_material()], _abi.MATERIAL_DTYPE)
    T = 200
    v = np.zeros((3 * T, 4), np.float32)
    for t in range(T):
        v[3 * t:3 * t + 3, :3] = [(t, 0, 0), (t + 0.9, 0, 0), (t, 0.9, 0)]
    cpu.verts_pos_array.append(v)
    cpu.indices_array.append(np.arange(3 * T, dtype=np.uint32))
    cpu.mesh_infos = np.array([api.default_mesh_info()], _abi.MESH_INFO_DTYPE)
    cpu.instances = np.array([api.default_instance()], _abi.INSTANCE_DTYPE)
    deep = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], [], True, blas_builder=chain_bvh)
    out = fresh(); cases.append(("hierarchy too deep", raw(g, deep.handle, True, 64, rec, out), out))
    assert "too deep" in lib.lupin_hip_last_error().decode()
    for label, rc, out in cases:
        assert rc == INVALID, (label, rc)
        assert np.all(out == SENTINEL), label
    assert len(cases) >= 50
    # accepted: n == 0 (nothing touched), samples == 2^20 on one record, tmax = +inf, both flags together
    out = fresh()
    assert raw(g, s, True, 0, rec, out) == 0 and np.all(out == SENTINEL)
    out = fresh()
    assert raw(g, s, True, 1, rec, out, samples=1 << 20) == 0 and 0.0 <= out.view(np.float32)[0, 3] <= float(1 << 20) and np.all(out[1:] == SENTINEL)
    r = rec.copy(); r[9, 7] = np.inf
    out = fresh()
    assert raw(g, s, True, 64, r, out, flags=OPACITY) == 0 and np.all(out.view(np.float32)[:, 3] <= 3.0)
    # what follows is unharmed
    assert np.array_equal(words(api.bent_normal_rays(gpu_ctx, scene, rec, 3)), device_bent(gpu_ctx, scene, rec, 3)[1])


# ---- calls between recorded frames ------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 65])
def test_a_refused_call_names_its_records_and_leaves_recorded_frames_intact(gpu_ctx, S):
    """Frames recorded and not yet run, then a call refused for its records (host arrays name the first bad index, device
    arrays count the bad records, the output stays untouched) or a call that succeeds: the frames are what they are
    without the call."""
    W, H = 32, 24
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=(7, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rec = api.occlusion_records(rng.uniform(-0.5, 0.5, (7, 3)) + [0.0, 1.0, 0.0], nrm, 0.7, api.rng_seed_for(np.arange(7, dtype=np.uint32), 0))
    alone = api.bent_normal_rays(gpu_ctx, scene, rec, S)
    bad = rec.copy(); bad[3, 1] = np.nan; bad[5, 7] = 0.0
    lib = _abi.lib()
    between = []

    def host_refusal():
        out = np.full((7, 4), SENTINEL, np.uint32)
        c = _abi.BentNormalDescC(S, 0, 0, 1e-3)
        assert lib.lupin_hip_bent_normal_rays(gpu_ctx.handle, scene.handle, C.byref(c), 7, _abi.ptr(bad), _abi.ptr(out)) == -1
        assert lib.lupin_hip_last_error().decode().startswith("record 3: ") and np.all(out == SENTINEL)

    def device_refusal():
        rc, out = device_bent(gpu_ctx, scene, bad, S, sentinel=SENTINEL)
        assert rc == -1 and lib.lupin_hip_last_error().decode().startswith("2 record(s): ") and np.all(out == SENTINEL)

    def success():
        between.append(api.bent_normal_rays(gpu_ctx, scene, rec, S))

    plain = util.gpu_accumulate(gpu_ctx, scene, cams[0], W, H, frames=4, spp=1)
    for call in (host_refusal, device_refusal, success):
        assert util.f16_words_differ(util.gpu_accumulate(gpu_ctx, scene, cams[0], W, H, frames=4, spp=1, between=call), plain) == 0
    assert len(between) >= 1 and all(np.array_equal(words(b), words(alone)) for b in between)
    assert np.array_equal(words(api.bent_normal_rays(gpu_ctx, scene, rec, S)), words(alone))
