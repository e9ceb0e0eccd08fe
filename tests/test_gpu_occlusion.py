"""Occlusion queries on the device (lupin_hip_occlusion_rays): the exact properties of the any-hit traversal
(unbounded = the closest hit's flag, monotone in tmax, hemisphere counts = sums over the radiance query's first rays, the same
words from LDS-staged and global geometry), the float64 judgement of tests/occlusion_ref.py at 0.5 t and 2 t over every
builder and after instances moved, the batch shapes of the wave-level combine, closed forms, line of sight, every refusal,
and that frames rendered around a call do not notice it.

The rays are closest_hit_ref's families, less the three whose directions are not of unit length (in_plane, short, long): a
record with such a direction is refused, and the refusal is tested below."""
import ctypes as C
import os

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import closest_hit_ref as X
from tests import occlusion_ref as R
from tests import util
from tests.test_gpu_closest_hit import device_scene, staged_in_lds
from tests.test_gpu_ray_query import DeviceArray, chain_bvh
from tests.test_occlusion_cpu import AO_SAMPLES, AO_SIGMAS, check_inputs

pytestmark = pytest.mark.gpu

MODE = api.OcclusionMode
PT = api.PathtraceType
SENTINEL = 0xABCDABCD
_cache = {}


def usable_rays(kind, moved=False):
    c = X.case(kind, moved)
    keep = R.usable(c)
    return c, keep, c.ori[keep], c.dir[keep]


@pytest.fixture(scope="module")
def global_ctx(built):
    """A context whose kernels read every scene from global memory, as tests/test_light_probe.py makes one."""
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
    ctx.close()


def device_occlusion(ctx, scene, rec, mode=MODE.DIRECTION, samples=1, eps=1e-3, sentinel=None):
    """lupin_hip_occlusion_rays with LUPIN_OCCLUSION_DEVICE_POINTERS on texture memory: (status, counts)."""
    n = len(rec)
    d_rec = DeviceArray(ctx, rec.nbytes).upload(rec)
    d_out = DeviceArray(ctx, n * 4)
    if sentinel is not None:
        d_out.upload(np.full(n, sentinel, np.uint32))
    c = _abi.OcclusionDescC(int(mode), samples, api.OCCLUSION_DEVICE_POINTERS, eps)
    rc = _abi.lib().lupin_hip_occlusion_rays(ctx.handle, scene.handle, C.byref(c), n, C.c_void_p(d_rec.ptr), C.c_void_p(d_out.ptr))
    return rc, d_out.download(np.uint32, n)


# ---- the exact properties ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", X.EPSILONS)
@pytest.mark.parametrize("kind", ["big", "small"])
def test_unbounded_equals_the_closest_hit_flag(gpu_ctx, kind, eps):
    """Property 1: zero differing, against the device's closest hit and against the oracle's."""
    from oracle import oracle
    c, keep, ori, d = usable_rays(kind)
    scene = device_scene(gpu_ctx, kind)
    assert staged_in_lds(gpu_ctx, scene) == (kind == "small")
    got = api.occluded(gpu_ctx, scene, ori, d, np.inf, eps)
    assert got.dtype == bool and got.shape == (len(ori),) and 0.3 < got.mean() < 0.8
    hit = api.trace_rays(gpu_ctx, scene, ori, d, eps)[0] != 0
    assert int((got != hit).sum()) == 0
    assert int((got != (oracle.trace_rays(c.scene, ori, d, eps)[0] != 0)).sum()) == 0
    # any tmax >= FLT_MAX is unbounded
    assert np.array_equal(api.occluded(gpu_ctx, scene, ori, d, np.finfo(np.float32).max, eps), got)


@pytest.mark.parametrize("kind", ["big", "small"])
def test_monotone_in_tmax(gpu_ctx, kind):
    """Property 2: no ray goes from blocked to unblocked as tmax grows."""
    _, _, ori, d = usable_rays(kind)
    scene = device_scene(gpu_ctx, kind)
    hit, dst, _, _, _ = api.trace_rays(gpu_ctx, scene, ori, d, 1e-3)
    base = np.where(hit != 0, dst, np.float32(5.0)).astype(np.float32)
    steps = [api.occluded(gpu_ctx, scene, ori, d, np.float32(f) * base, 1e-3) for f in (0.25, 0.5, 1.0, 2.0, 4.0)]
    steps.append(api.occluded(gpu_ctx, scene, ori, d, np.inf, 1e-3))
    for a, b in zip(steps, steps[1:]):
        assert int((a & ~b).sum()) == 0
    assert steps[0].sum() < steps[3].sum() <= steps[-1].sum()       # and the bound is looked at


def judge(ctx, scene, ref, ori, d, eps, per_instance=None):
    rep = R.report(ref, lambda tmax: api.occluded(ctx, scene, ori, d, tmax, eps))
    print({k: v for k, v in rep.items() if k != "per_instance"}, rep["per_instance"])
    check_inputs(rep) if per_instance is None else check_inputs(rep, per_instance)
    assert rep["disagree"] == 0, rep


@pytest.mark.parametrize("eps", X.EPSILONS)
@pytest.mark.parametrize("kind", ["big", "small"])
def test_float64_judgement(gpu_ctx, kind, eps):
    c, keep, ori, d = usable_rays(kind)
    judge(gpu_ctx, device_scene(gpu_ctx, kind), c.refs[eps].take(keep), ori, d, eps)


@pytest.mark.parametrize("tlas_builder", ["cpu", "device"])
@pytest.mark.parametrize("blas_builder", ["sah", "sah_device", "lbvh"])
def test_float64_judgement_on_every_builder(gpu_ctx, blas_builder, tlas_builder):
    c, keep, ori, d = usable_rays("big")
    scene = device_scene(gpu_ctx, "big", blas_builder=blas_builder, tlas_builder=tlas_builder)
    judge(gpu_ctx, scene, c.refs[1e-3].take(keep), ori, d, 1e-3)


@pytest.mark.parametrize("tlas_builder", ["cpu", "device"])
def test_moved_instances_give_the_answers_of_a_fresh_scene(gpu_ctx, tlas_builder):
    """After Scene.update_instances the four-wide hierarchy is stale; the query reads the binary one only."""
    c, keep, ori, d = usable_rays("big", moved=True)
    moved = X.transforms(X.SEED, moved=True)
    scene = X.build("big", X.SEED, gpu_ctx)                              # a scene of its own: it is changed in place
    before = api.occluded(gpu_ctx, scene, ori, d, np.inf, 1e-3)
    scene.update_instances(X.instance_records(moved), tlas_builder=tlas_builder)
    fresh = X.build("big", X.SEED, gpu_ctx, xf=moved)
    judge(gpu_ctx, scene, c.refs[1e-3].take(keep), ori, d, 1e-3, per_instance=15)   # a third of the main batch's rays
    ref = c.refs[1e-3].take(keep)
    for scale in (0.5, 2.0):
        tmax, _ = R.judgement(ref, scale)
        assert np.array_equal(api.occluded(gpu_ctx, scene, ori, d, tmax, 1e-3), api.occluded(gpu_ctx, fresh, ori, d, tmax, 1e-3))
    after = api.occluded(gpu_ctx, scene, ori, d, np.inf, 1e-3)
    assert np.array_equal(after, api.occluded(gpu_ctx, fresh, ori, d, np.inf, 1e-3))
    assert int((before != after).sum()) > 100                           # the move is visible to these rays


# ---- batch shapes: the wave-level combine and the record / slot indexing ----------------------------------------

@pytest.mark.parametrize("kind", ["big", "small"])
def test_small_batches(gpu_ctx, kind):
    _, _, ori, d = usable_rays(kind)
    scene = device_scene(gpu_ctx, kind)
    hit, dst, _, _, _ = api.trace_rays(gpu_ctx, scene, ori[:257], d[:257], 1e-3)
    tmax = np.where(hit != 0, np.float32(2.0) * dst, np.float32(5.0)).astype(np.float32)
    tmax[::3] = np.inf
    whole = api.occlusion_rays(gpu_ctx, scene, api.occlusion_records(ori[:257], d[:257], tmax))
    assert whole.dtype == np.uint32 and (whole <= 1).all()
    assert np.array_equal(whole[::3], hit[::3]) and 0 < whole.sum() < 257      # unbounded: the closest hit's flag
    for n in (1, 63, 64, 65, 257):
        first = 257 - n                                                  # a batch does not notice where it starts
        rec = api.occlusion_records(ori[first:257], d[first:257], tmax[first:257])
        assert np.array_equal(api.occlusion_rays(gpu_ctx, scene, rec), whole[first:]), n
        rc, dev = device_occlusion(gpu_ctx, scene, rec)
        assert rc == 0 and np.array_equal(dev, whole[first:]), n
    assert api.occlusion_rays(gpu_ctx, scene, api.occlusion_records(ori[:0], d[:0])).shape == (0,)


def hemisphere_records(ctx, kind):
    """Five records: origins and normals of rays of which the device's closest hit blocks three nearby and misses two."""
    _, _, ori, d = usable_rays(kind)
    scene = device_scene(ctx, kind)
    hit, dst, _, _, _ = api.trace_rays(ctx, scene, ori, d, 1e-3)
    near, free = np.nonzero((hit != 0) & (dst > 0.5) & (dst < 3.0))[0][:3], np.nonzero(hit == 0)[0][:2]
    pick = np.concatenate([near, free])
    assert len(pick) == 5
    return scene, api.occlusion_records(ori[pick], d[pick], np.float32([6.0, np.inf, 4.0, 6.0, 8.0]),
                                        api.rng_seed_for(np.arange(5, dtype=np.uint32), 3))


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 129, 1000])
@pytest.mark.parametrize("kind", ["big", "small"])
def test_hemisphere_count_is_the_sum_over_the_radiance_query_first_rays(gpu_ctx, kind, S):
    """Property 3: integers, equal; the same words through host and device pointers."""
    scene, rec = hemisphere_records(gpu_ctx, kind)
    got = api.occlusion_rays(gpu_ctx, scene, rec, MODE.COSINE_HEMISPHERE, S)
    assert got.shape == (5,) and (got <= S).all()
    qrec = rec.copy()
    qrec.view(np.uint32)[:, 7] = int(api.RayMode.COSINE_HEMISPHERE)
    _, rays = api.pathtrace_rays(gpu_ctx, scene, qrec, api.RayQueryDesc(PT.Naive, 0, S), want_rays=True)
    assert rays.shape == (5 * S, 8)
    single = api.occlusion_rays(gpu_ctx, scene, api.occlusion_records(rays[:, 0:3], rays[:, 4:7], np.repeat(rec[:, 7], S)))
    assert np.array_equal(got, single.reshape(5, S).sum(axis=1).astype(np.uint32)), (got, single.reshape(5, S).sum(axis=1))
    rc, dev = device_occlusion(gpu_ctx, scene, rec, MODE.COSINE_HEMISPHERE, S)
    assert rc == 0 and np.array_equal(dev, got)
    if S == 1000:
        assert 0 < int(got.sum()) < 5 * S, got                          # both answers occur


def test_staged_and_global_geometry_give_the_same_words(gpu_ctx, global_ctx):
    """Property 4."""
    _, _, ori, d = usable_rays("small")
    staged, unstaged = device_scene(gpu_ctx, "small"), X.build("small", X.SEED, global_ctx)
    assert staged_in_lds(gpu_ctx, staged) and not staged_in_lds(global_ctx, unstaged)
    hit, dst, _, _, _ = api.trace_rays(gpu_ctx, staged, ori, d, 1e-3)
    for f in (0.5, 1.0, 2.0, np.inf):
        tmax = np.where(hit != 0, np.float32(f) * np.where(hit != 0, dst, np.float32(1.0)), np.float32(5.0)).astype(np.float32)
        assert np.array_equal(api.occluded(gpu_ctx, staged, ori, d, tmax, 1e-3), api.occluded(global_ctx, unstaged, ori, d, tmax, 1e-3)), f
    _, rec = hemisphere_records(gpu_ctx, "small")
    for S in (65, 1000):
        assert np.array_equal(api.occlusion_rays(gpu_ctx, staged, rec, MODE.COSINE_HEMISPHERE, S),
                              api.occlusion_rays(global_ctx, unstaged, rec, MODE.COSINE_HEMISPHERE, S)), S


# ---- closed forms -----------------------------------------------------------------------------------------------

H_CEILING = 1.0


def quad_y(y, half, flip=False):
    v = np.zeros((4, 4), np.float32)
    v[:, :3] = [(-half, y, -half), (-half, y, half), (half, y, half), (half, y, -half)]
    return v, np.array([0, 1, 2, 0, 2, 3] if flip else [0, 2, 1, 2, 0, 3], np.uint32)


def upload(ctx, meshes):
    cpu = api.SceneCPU()
    cpu.materials = np.array([api.default_material()], _abi.MATERIAL_DTYPE)
    for v, idx in meshes:
        cpu.verts_pos_array.append(v)
        cpu.indices_array.append(idx)
    cpu.mesh_infos = np.array([api.default_mesh_info() for _ in meshes], _abi.MESH_INFO_DTYPE)
    cpu.instances = np.array([api.default_instance() for _ in meshes], _abi.INSTANCE_DTYPE)
    cpu.instances["mesh_idx"] = np.arange(len(meshes))
    api.validate_scene(cpu, 0, 0)
    return api.build_accel_structures_and_upload(ctx, cpu, [], [], True)


def room(ctx):
    """A floor at y = 0 under a ceiling at y = H_CEILING, both 20 H wide: the ceiling's edge is 10 H away, outside any radius
    used here."""
    if "room" not in _cache:
        _cache["room"] = upload(ctx, [quad_y(0.0, 10.0 * H_CEILING, flip=True), quad_y(H_CEILING, 10.0 * H_CEILING)])
    return _cache["room"]


def closed_box(ctx):
    if "box" not in _cache:
        v = np.zeros((8, 4), np.float32)
        v[:, :3] = [(x, y, z) for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]
        idx = [0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3]
        _cache["box"] = upload(ctx, [(v, np.array(idx, np.uint32))])
    return _cache["box"]


def test_ambient_occlusion_under_a_ceiling_is_the_cosine_weighted_closed_form(gpu_ctx):
    scene = room(gpu_ctx)
    point, normal = [[0.3, 0.0, -0.2]], [[0.0, 1.0, 0.0]]
    radius = 2.0 * H_CEILING
    ao = api.ambient_occlusion(gpu_ctx, scene, point, normal, radius, samples=AO_SAMPLES, surface_offset=0.0)
    assert ao.dtype == np.float32 and ao.shape == (1,)
    blocked = 1.0 - float(ao[0])
    want, twin = R.ceiling_blocked_fraction(H_CEILING, radius), R.ceiling_blocked_fraction_uniform_twin(H_CEILING, radius)
    print(f"blocked fraction {blocked:.5f}, closed form {want}, sigma {R.binomial_sigma(want, AO_SAMPLES):.5f}")
    assert abs(blocked - want) <= AO_SIGMAS * R.binomial_sigma(want, AO_SAMPLES)
    assert not abs(blocked - twin) <= AO_SIGMAS * R.binomial_sigma(twin, AO_SAMPLES)      # uniform weighting would fail
    # below the ceiling nothing is in reach: exactly none
    assert api.ambient_occlusion(gpu_ctx, scene, point, normal, 0.9 * H_CEILING, samples=AO_SAMPLES, surface_offset=0.0)[0] == 1.0
    # the default offset moves the origin off the floor by 1e-4 of the scene's extent: the same closed form within the band
    ao = api.ambient_occlusion(gpu_ctx, scene, point, normal, radius, samples=AO_SAMPLES, counter=1)
    assert abs((1.0 - float(ao[0])) - want) <= AO_SIGMAS * R.binomial_sigma(want, AO_SAMPLES) + 2e-3


def test_inside_a_closed_box_every_slot_is_blocked(gpu_ctx):
    scene = closed_box(gpu_ctx)
    points = np.float32([[0.0, 0.0, 0.0], [0.5, -0.7, 0.2], [-0.9, 0.9, -0.9]])
    normals = np.float32([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.6, 0.0, 0.8]])
    S = 4096
    rec = api.occlusion_records(points, normals, 4.0, api.rng_seed_for(np.arange(3, dtype=np.uint32), 0))    # the diagonal is 3.47
    assert np.array_equal(api.occlusion_rays(gpu_ctx, scene, rec, MODE.COSINE_HEMISPHERE, S), np.full(3, S, np.uint32))
    assert np.array_equal(api.ambient_occlusion(gpu_ctx, scene, points, normals, 4.0, samples=S, surface_offset=0.0), np.zeros(3, np.float32))


def test_visible(gpu_ctx):
    scene = room(gpu_ctx)
    h = H_CEILING
    p = np.float32([[0.0, 0.5 * h, 0.0], [0.0, 0.2 * h, 0.0], [0.0, 0.01, 0.0], [0.0, 0.0, 0.0], [2.0, 1.5 * h, 1.0]])
    q = np.float32([[0.0, 1.5 * h, 0.0], [3.0, 0.6 * h, 1.0], [1.0, h - 0.01, 0.5], [1.0, h, 0.5], [-4.0, 3.0 * h, 0.0]])
    # either side of the ceiling | free space | facing surfaces, offset by their normals | the same without the offset: the
    # end points' own surfaces lie below ray_epsilon and at tmax + ray_epsilon | free space above the ceiling
    assert api.visible(gpu_ctx, scene, p, q).tolist() == [False, True, True, True, True]
    assert api.visible(gpu_ctx, scene, q, p).tolist() == [False, True, True, True, True]
    with pytest.raises(ValueError):
        api.visible(gpu_ctx, scene, p, p)


# ---- refusals ---------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_the_output_untouched(gpu_ctx):
    _, _, ori, d = usable_rays("small")
    scene = device_scene(gpu_ctx, "small")
    rec = api.occlusion_records(ori[:64], d[:64], 5.0)
    lib = _abi.lib()
    INVALID = -1

    def raw(ctx_h, scene_h, desc, n, records, out, mode=0, samples=1, flags=0, eps=1e-3):
        c = _abi.OcclusionDescC(mode, samples, flags, eps)
        return lib.lupin_hip_occlusion_rays(ctx_h, scene_h, C.byref(c) if desc else None, n, _abi.ptr(records), _abi.ptr(out))

    def fresh():
        return np.full(len(rec), SENTINEL, np.uint32)

    g, s = gpu_ctx.handle, scene.handle
    cases = []
    out = fresh(); cases.append(("null context", raw(None, s, True, 64, rec, out), out))
    out = fresh(); cases.append(("null scene", raw(g, None, True, 64, rec, out), out))
    out = fresh(); cases.append(("null desc", raw(g, s, False, 64, rec, out), out))
    out = fresh(); cases.append(("null records", raw(g, s, True, 64, None, out), out))
    out = fresh(); cases.append(("null out", raw(g, s, True, 64, rec, None), out))
    out = fresh(); cases.append(("unknown mode", raw(g, s, True, 64, rec, out, mode=2), out))
    out = fresh(); cases.append(("unknown flag", raw(g, s, True, 64, rec, out, flags=2), out))
    out = fresh(); cases.append(("samples == 0", raw(g, s, True, 64, rec, out, mode=1, samples=0), out))
    out = fresh(); cases.append(("samples above 2^27", raw(g, s, True, 64, rec, out, mode=1, samples=(1 << 27) + 1), out))
    out = fresh(); cases.append(("direction mode with two samples", raw(g, s, True, 64, rec, out, samples=2), out))
    out = fresh(); cases.append(("n * samples too large", raw(g, s, True, (1 << 38) // 4 + 1, rec, out, mode=1, samples=4), out))
    for label, eps in (("NaN", np.nan), ("infinite", np.inf), ("negative", -1e-3)):
        out = fresh(); cases.append((f"{label} ray_epsilon", raw(g, s, True, 64, rec, out, eps=eps), out))
    other = api.Context(0)
    foreign = X.build("small", X.SEED, other)
    out = fresh(); cases.append(("scene of another context", raw(g, foreign.handle, True, 64, rec, out), out))
    other.close()
    out = fresh(); cases.append(("scene of a destroyed context", raw(g, foreign.handle, True, 64, rec, out), out))
    bad_records = {}
    for label, row, col, value in (("NaN origin", 17, 1, np.nan), ("infinite direction", 17, 5, np.inf), ("NaN normal", 63, 6, np.nan),
                                   ("NaN tmax", 0, 7, np.nan), ("zero tmax", 31, 7, 0.0), ("negative tmax", 31, 7, -1.0),
                                   ("minus infinite tmax", 5, 7, -np.inf)):
        r = rec.copy(); r[row, col] = value
        bad_records[label] = r
    r = rec.copy(); r[40, 4:7] *= np.float32(1.001)
    bad_records["direction too long"] = r
    r = rec.copy(); r[3, 4:7] = 0.0
    bad_records["zero normal"] = r
    for label, r in bad_records.items():
        for mode, S in ((0, 1), (1, 3)):
            out = fresh(); cases.append((f"{label} (host check, mode {mode})", raw(g, s, True, 64, r, out, mode=mode, samples=S), out))
            rc, dout = device_occlusion(gpu_ctx, scene, r, mode, S, sentinel=SENTINEL)
            cases.append((f"{label} (device check, mode {mode})", rc, dout))
    # misaligned device pointers
    d_rec = DeviceArray(gpu_ctx, rec.nbytes + 32).upload(np.concatenate([np.zeros(8, np.float32), rec.reshape(-1)]))
    d_out = DeviceArray(gpu_ctx, 64 * 4 + 32).upload(np.full(64 + 8, SENTINEL, np.uint32))
    cdev = _abi.OcclusionDescC(0, 1, api.OCCLUSION_DEVICE_POINTERS, 1e-3)
    for label, offs in (("records", (8, 0)), ("out_blocked", (0, 2))):
        rc = lib.lupin_hip_occlusion_rays(g, s, C.byref(cdev), 64, C.c_void_p(d_rec.ptr + 32 + offs[0]), C.c_void_p(d_out.ptr + offs[1]))
        cases.append((f"misaligned device pointer: {label}", rc, d_out.download(np.uint32, 64 + 8)))
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
    # accepted: n == 0 (nothing touched), a direction within the tolerance, any bit pattern as the RNG word, tmax = +inf
    out = fresh()
    assert raw(g, s, True, 0, rec, out) == 0 and np.all(out == SENTINEL)
    r = rec.copy(); r[40, 4:7] *= np.float32(1.00004); r.view(np.uint32)[5, 3] = 0x7FC00000; r[9, 7] = np.inf
    out = fresh()
    assert raw(g, s, True, 64, r, out) == 0 and np.all(out <= 1)
    # what follows is unharmed
    hit = api.trace_rays(gpu_ctx, scene, ori[:64], d[:64], 1e-3)[0]
    assert np.array_equal(api.occlusion_rays(gpu_ctx, scene, api.occlusion_records(ori[:64], d[:64])), hit)


# ---- frames around a call ---------------------------------------------------------------------------------------

def test_frames_around_an_occlusion_call_do_not_notice_it(gpu_ctx):
    W, H = 64, 48
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cam = cams[0]
    rng = np.random.default_rng(2)
    n = rng.normal(size=(300, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    rec = api.occlusion_records(rng.uniform(-0.5, 0.5, (300, 3)) + [0.0, 1.0, 0.0], n, 0.7, api.rng_seed_for(np.arange(300, dtype=np.uint32), 0))
    alone = api.occlusion_rays(gpu_ctx, scene, rec, MODE.COSINE_HEMISPHERE, 16)

    def chain(call_after):
        res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=8, samples_per_pixel=2))
        out = api.DoubleBufferedTexture(gpu_ctx, W, H)
        for k in range(6):
            desc = api.PathtraceDesc(accum_params=api.AccumulationParams(out.back(), k), camera_params=cam.params, camera_transform=cam.transform)
            api.pathtrace_scene(gpu_ctx, res, scene, out.front(), PT.Standard, desc)
            out.flip()
            if k + 1 == call_after:
                assert np.array_equal(api.occlusion_rays(gpu_ctx, scene, rec, MODE.COSINE_HEMISPHERE, 16), alone)
        out.flip()
        return out.front().download()

    plain = chain(None)
    assert util.f16_words_differ(chain(3), plain) == 0
    assert util.f16_words_differ(plain, util.oracle_accumulate(scene, cam, W, H, frames=6, spp=2)) == 0
    assert 0 < int(alone.sum()) < 300 * 16


# ---- a refused call between recorded frames -----------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 65])
def test_a_refused_call_names_its_records_and_leaves_recorded_frames_intact(gpu_ctx, S):
    """Frames recorded and not yet run, then a call refused for its records: host arrays name the first bad index, device
    arrays count the bad records, the output stays untouched, and the frames are what they are without the call.  65 slots
    per record make a record straddle a wave in the combine; that the 65-slot counts are right is property 3's business
    (test_hemisphere_count_is_the_sum_over_the_radiance_query_first_rays, S = 65 among its cases)."""
    W, H = 32, 24
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    mode = MODE.DIRECTION if S == 1 else MODE.COSINE_HEMISPHERE
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=(7, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rec = api.occlusion_records(rng.uniform(-0.5, 0.5, (7, 3)) + [0.0, 1.0, 0.0], nrm, 0.7, api.rng_seed_for(np.arange(7, dtype=np.uint32), 0))
    alone = api.occlusion_rays(gpu_ctx, scene, rec, mode, S)
    bad = rec.copy(); bad[3, 1] = np.nan; bad[5, 7] = 0.0
    lib = _abi.lib()

    def host_refusal():
        out = np.full(7, SENTINEL, np.uint32)
        c = _abi.OcclusionDescC(int(mode), S, 0, 1e-3)
        assert lib.lupin_hip_occlusion_rays(gpu_ctx.handle, scene.handle, C.byref(c), 7, _abi.ptr(bad), _abi.ptr(out)) == -1
        assert lib.lupin_hip_last_error().decode().startswith("record 3: ") and np.all(out == SENTINEL)

    def device_refusal():
        rc, out = device_occlusion(gpu_ctx, scene, bad, mode, S, sentinel=SENTINEL)
        assert rc == -1 and lib.lupin_hip_last_error().decode().startswith("2 record(s): ") and np.all(out == SENTINEL)

    plain = util.gpu_accumulate(gpu_ctx, scene, cams[0], W, H, frames=4, spp=1)
    for refusal in (host_refusal, device_refusal):
        assert util.f16_words_differ(util.gpu_accumulate(gpu_ctx, scene, cams[0], W, H, frames=4, spp=1, between=refusal), plain) == 0
    assert np.array_equal(api.occlusion_rays(gpu_ctx, scene, rec, mode, S), alone)
