"""Transmittance queries on the device (lupin_hip_transmittance_rays): the float64 judgement of
tests/transmittance_ref.py (zero disagreements on `small` and `big` at three epsilons and three tmax settings, and after
instances moved), the exact properties (an opaque scene is 1 - blocked, LDS = global, monotone in tmax, a single crossing is
1 - opacity of the surface probe, the hemisphere sum is the restated resolve order, host = device pointers), exact small
cases on stacked quads, the closed form under a half-transparent ceiling, and every refusal."""
import ctypes as C
import os

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import closest_hit_ref as X
from tests import occlusion_ref as R
from tests import transmittance_ref as TR
from tests import util
from tests.test_gpu_closest_hit import staged_in_lds
from tests.test_gpu_ray_query import DeviceArray, chain_bvh

pytestmark = pytest.mark.gpu

MODE = api.OcclusionMode
PT = api.PathtraceType
SENTINEL = 0xABCDABCD
AO_SAMPLES = 65536
AO_SIGMAS = 5.0
_scenes = {}


def device_scene(ctx, kind, opaque=False):
    key = (id(ctx), kind, opaque)
    if key not in _scenes:
        _scenes[key] = TR.build(kind, ctx, opaque=opaque)[2]
    return _scenes[key]


@pytest.fixture(scope="module")
def global_ctx(built):
    """A context whose kernels read every scene from global memory, as tests/test_gpu_occlusion.py makes one."""
    old = os.environ.get("LUPIN_LDS_GEOMETRY")
    os.environ["LUPIN_LDS_GEOMETRY"] = "0"
    try:
        ctx = api.Context(0)
    finally:
        if old is None:
            os.environ.pop("LUPIN_LDS_GEOMETRY", None)
        else:
            os.environ["LUPIN_LDS_GEOMETRY"] = old
    yield ctx
    ctx.close()


def direct(ctx, scene, ori, d, tmax, eps=1e-3):
    return api.transmittance_rays(ctx, scene, api.occlusion_records(ori, d, tmax), MODE.DIRECTION, 1, eps)


def device_transmittance(ctx, scene, rec, mode=MODE.DIRECTION, samples=1, eps=1e-3, sentinel=None):
    """lupin_hip_transmittance_rays with LUPIN_OCCLUSION_DEVICE_POINTERS on texture memory: (status, sums as u32 words)."""
    n = len(rec)
    d_rec = DeviceArray(ctx, rec.nbytes).upload(rec)
    d_out = DeviceArray(ctx, n * 4)
    if sentinel is not None:
        d_out.upload(np.full(n, sentinel, np.uint32))
    c = _abi.OcclusionDescC(int(mode), samples, api.OCCLUSION_DEVICE_POINTERS, eps)
    rc = _abi.lib().lupin_hip_transmittance_rays(ctx.handle, scene.handle, C.byref(c), n, C.c_void_p(d_rec.ptr), C.c_void_p(d_out.ptr))
    return rc, d_out.download(np.uint32, n)


def words(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ---- the float64 judgement --------------------------------------------------------------------------------------

def judge(ctx, scene, c, eps):
    for setting in TR.TMAX_SETTINGS:
        tmax = TR.tmax_for(c.P, eps, setting)
        exp = TR.expected(c.P, c.op, eps, tmax.astype(np.float64))
        got = direct(ctx, scene, c.ori, c.dir, tmax, eps)
        assert got.dtype == np.float32 and got.shape == (len(c.ori),) and ((got >= 0) & (got <= 1)).all()
        shares, bad = TR.left_out_shares(c, exp), TR.disagreements(exp, got)
        err = np.abs(got.astype(np.float64) - exp.T)[exp.decisive & ~(exp.zero_ok & (got == 0))]
        print(c.kind, eps, setting, "left out", shares, "disagree", bad, "worst |T - ref|", float(err.max()), "partial T", int(((got > 0) & (got < 1)).sum()))
        assert max(shares.values()) <= TR.MAX_LEFT_OUT, shares
        assert bad == 0, (setting, bad)
        if setting != "half":
            assert ((got > 0) & (got < 1)).sum() > len(got) // 5 and (got == 0).sum() > len(got) // 20 and (got == 1).sum() > len(got) // 5


@pytest.mark.parametrize("eps", X.EPSILONS)
@pytest.mark.parametrize("kind", ["big", "small"])
def test_float64_judgement(gpu_ctx, kind, eps):
    scene = device_scene(gpu_ctx, kind)
    assert staged_in_lds(gpu_ctx, scene) == (kind == "small")
    judge(gpu_ctx, scene, TR.case(kind), eps)


@pytest.mark.parametrize("tlas_builder", ["cpu", "device"])
def test_moved_instances_are_judged_and_give_the_words_of_a_fresh_scene(gpu_ctx, tlas_builder):
    """After Scene.update_instances the four-wide hierarchy is stale; the query reads the binary one only."""
    c = TR.case("big", moved=True)
    moved = X.transforms(X.SEED, moved=True)
    scene = TR.build("big", gpu_ctx)[2]                                  # a scene of its own: it is changed in place
    before = direct(gpu_ctx, scene, c.ori, c.dir, np.inf)
    scene.update_instances(np.array(X.instance_records(moved)["transpose_inverse_transform"], np.float32).reshape(-1, 3, 4), tlas_builder=tlas_builder)
    judge(gpu_ctx, scene, c, 1e-3)
    fresh = TR.build("big", gpu_ctx, xf=moved)[2]
    for setting in TR.TMAX_SETTINGS:
        tmax = TR.tmax_for(c.P, 1e-3, setting)
        assert np.array_equal(words(direct(gpu_ctx, scene, c.ori, c.dir, tmax)), words(direct(gpu_ctx, fresh, c.ori, c.dir, tmax)))
    assert int((before != direct(gpu_ctx, scene, c.ori, c.dir, np.inf)).sum()) > 100     # the move is visible to these rays


# ---- the exact properties: every ray, no exclusions -------------------------------------------------------------

def ladder(ctx, scene, ori, d):
    hit, dst, _, _, _ = api.trace_rays(ctx, scene, ori, d, 1e-3)
    base = np.where(hit != 0, dst, np.float32(5.0)).astype(np.float32)
    return [np.float32(f) * base for f in (0.25, 0.5, 1.0, 2.0, 4.0, 16.0)] + [np.full(len(ori), np.inf, np.float32)]


@pytest.mark.parametrize("kind", ["big", "small"])
def test_an_opaque_scene_is_one_minus_blocked(gpu_ctx, kind):
    """Property 1: bit for bit, on a scene without an alpha-capable instance, and for the rays of the alpha scene whose
    crossings (by the reference, decisive) all lie in flag-clear instances."""
    c = TR.case(kind)
    opaque = device_scene(gpu_ctx, kind, opaque=True)
    for eps in X.EPSILONS:
        for tmax in ladder(gpu_ctx, opaque, c.ori, c.dir):
            blocked = api.occlusion_rays(gpu_ctx, opaque, api.occlusion_records(c.ori, c.dir, tmax), MODE.DIRECTION, 1, eps)
            want = np.float32(1.0) - blocked.astype(np.float32)
            assert np.array_equal(words(direct(gpu_ctx, opaque, c.ori, c.dir, tmax, eps)), words(want))
    assert 0 < blocked.sum() < len(blocked)
    scene = device_scene(gpu_ctx, kind)
    seen = 0
    for setting in ("twice", "unbounded"):
        tmax = TR.tmax_for(c.P, 1e-3, setting)
        exp = TR.expected(c.P, c.op, 1e-3, tmax.astype(np.float64))
        sel = exp.decisive & exp.only_opaque
        blocked = api.occlusion_rays(gpu_ctx, scene, api.occlusion_records(c.ori[sel], c.dir[sel], tmax[sel]))
        assert np.array_equal(words(direct(gpu_ctx, scene, c.ori[sel], c.dir[sel], tmax[sel])), words(np.float32(1.0) - blocked.astype(np.float32)))
        seen += int(blocked.sum())
    assert seen > 100                                                    # rays that the opaque instances block are among them


def test_staged_and_global_geometry_give_the_same_words(gpu_ctx, global_ctx):
    """Property 2."""
    c = TR.case("small")
    staged, unstaged = device_scene(gpu_ctx, "small"), device_scene(global_ctx, "small")
    assert staged_in_lds(gpu_ctx, staged) and not staged_in_lds(global_ctx, unstaged)
    for tmax in ladder(gpu_ctx, staged, c.ori, c.dir):
        assert np.array_equal(words(direct(gpu_ctx, staged, c.ori, c.dir, tmax)), words(direct(global_ctx, unstaged, c.ori, c.dir, tmax)))
    _, rec = hemisphere_records(gpu_ctx, "small")
    for S in (65, 1000):
        assert np.array_equal(words(api.transmittance_rays(gpu_ctx, staged, rec, MODE.COSINE_HEMISPHERE, S)),
                              words(api.transmittance_rays(global_ctx, unstaged, rec, MODE.COSINE_HEMISPHERE, S))), S


@pytest.mark.parametrize("kind", ["big", "small"])
def test_monotone_in_tmax(gpu_ctx, kind):
    """Property 3: T never grows with tmax, exactly."""
    c = TR.case(kind)
    scene = device_scene(gpu_ctx, kind)
    steps = [direct(gpu_ctx, scene, c.ori, c.dir, tmax) for tmax in ladder(gpu_ctx, scene, c.ori, c.dir)]
    for a, b in zip(steps, steps[1:]):
        assert int((a < b).sum()) == 0
    assert steps[0].sum() > steps[3].sum() >= steps[-1].sum()            # and the bound is looked at
    assert int(((steps[3] > steps[-1]) & (steps[-1] > 0)).sum()) > 0     # further surfaces keep multiplying


@pytest.mark.parametrize("kind", ["big", "small"])
def test_a_single_crossing_is_one_minus_the_probed_opacity(gpu_ctx, kind):
    """Property 4: for a ray whose segment holds exactly one crossing (by the reference), T == 1 - max(a, 0) bit for bit, or 0,
    a being the surface probe's opacity at what trace_rays reports."""
    c = TR.case(kind)
    scene = device_scene(gpu_ctx, kind)
    tmax = np.full(len(c.ori), np.inf)
    exp = TR.expected(c.P, c.op, 1e-3, tmax)
    sel = exp.decisive & (exp.n == 1)
    ori, d = c.ori[sel], c.dir[sel]
    hit, dst, uv, inst, tri = api.trace_rays(gpu_ctx, scene, ori, d, 1e-3)
    assert (hit != 0).all()
    a = api.surface_probe(gpu_ctx, scene, api.surface_records(int(api.SurfaceMode.OPACITY), inst, tri, uv))[:, 0]
    capable = TR.alpha_capable(c.sc)[inst]
    want = np.where(capable & (a < np.float32(1.0)), np.float32(1.0) - np.maximum(a, np.float32(0.0)), np.float32(0.0)).astype(np.float32)
    got = direct(gpu_ctx, scene, ori, d, np.inf)
    assert np.array_equal(words(got), words(want)), int((words(got) != words(want)).sum())
    assert capable.sum() > 200 and (~capable).sum() > 50 and len(np.unique(got)) > 100


def hemisphere_records(ctx, kind):
    """Six records on surface points of the alpha scene, normals towards the ray that found them."""
    c = TR.case(kind)
    scene = device_scene(ctx, kind)
    hit, dst, _, inst, _ = api.trace_rays(ctx, scene, c.ori, c.dir, 1e-3)
    pick = np.concatenate([np.nonzero((hit != 0) & (inst == i) & (dst > 0.5))[0][:1] for i in (3, 5, 7, 9, 1, 2)])
    assert len(pick) == 6
    p = c.ori[pick] + c.dir[pick] * (dst[pick] * np.float32(0.98))[:, None]
    return scene, api.occlusion_records(p, -c.dir[pick], np.float32([6.0, np.inf, 4.0, 6.0, 8.0, np.inf]), api.rng_seed_for(np.arange(6, dtype=np.uint32), 3))


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 129, 1000])
@pytest.mark.parametrize("kind", ["big", "small"])
def test_hemisphere_sum_is_the_restated_resolve_order_over_the_first_rays(gpu_ctx, kind, S):
    """Properties 5 and 6: bit for bit; the same words through host and device pointers."""
    scene, rec = hemisphere_records(gpu_ctx, kind)
    got = api.transmittance_rays(gpu_ctx, scene, rec, MODE.COSINE_HEMISPHERE, S)
    assert got.shape == (6,) and got.dtype == np.float32
    qrec = rec.copy()
    qrec.view(np.uint32)[:, 7] = int(api.RayMode.COSINE_HEMISPHERE)
    _, rays = api.pathtrace_rays(gpu_ctx, scene, qrec, api.RayQueryDesc(PT.Naive, 0, S), want_rays=True)
    single = direct(gpu_ctx, scene, rays[:, 0:3], rays[:, 4:7], np.repeat(rec[:, 7], S)).reshape(6, S)
    want = np.float32([TR.resolve_sum_f32(row) for row in single])
    assert np.array_equal(words(got), words(want)), (got, want)
    rc, dev = device_transmittance(gpu_ctx, scene, rec, MODE.COSINE_HEMISPHERE, S)
    assert rc == 0 and np.array_equal(dev, words(got))
    if S == 1000:
        assert ((single > 0) & (single < 1)).sum() > 100 and (single == 0).any() and (single == 1).any()
        ao = api.ambient_occlusion(gpu_ctx, scene, rec[:, 0:3], rec[:, 4:7], 4.0, samples=64, surface_offset=0.0, opacity=True)
        plain = api.ambient_occlusion(gpu_ctx, scene, rec[:, 0:3], rec[:, 4:7], 4.0, samples=64, surface_offset=0.0)
        assert ao.dtype == np.float32 and (ao >= plain).all() and (ao > plain).any()


def test_host_and_device_pointers_give_the_same_words(gpu_ctx):
    """Property 6, direction mode, batch sizes around a wave and a block."""
    c = TR.case("small")
    scene = device_scene(gpu_ctx, "small")
    tmax = TR.tmax_for(c.P, 1e-3, "twice")
    whole = direct(gpu_ctx, scene, c.ori[:257], c.dir[:257], tmax[:257])
    for n in (1, 63, 64, 65, 257):
        rec = api.occlusion_records(c.ori[257 - n:257], c.dir[257 - n:257], tmax[257 - n:257])
        assert np.array_equal(words(api.transmittance_rays(gpu_ctx, scene, rec)), words(whole[257 - n:])), n
        rc, dev = device_transmittance(gpu_ctx, scene, rec)
        assert rc == 0 and np.array_equal(dev, words(whole[257 - n:])), n
    assert api.transmittance_rays(gpu_ctx, scene, api.occlusion_records(c.ori[:0], c.dir[:0])).shape == (0,)


# ---- exact small cases ------------------------------------------------------------------------------------------

O_QUAD, D_QUAD = np.float32([[5.0, -3.5, 2.0]]), np.float32([[0.0, 0.0, 1.0]])   # meets the stack's first quad at t = 4 exactly


def through(ctx, scene, tmax=np.inf, eps=1e-3, o=O_QUAD):
    return float(direct(ctx, scene, o, D_QUAD, tmax, eps)[0])


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_stacked_quads_give_the_dyadic_product(gpu_ctx, k):
    assert through(gpu_ctx, TR.stacked_quads([0.5] * k, ctx=gpu_ctx)[2]) == 2.0 ** -k
    mixed = ([0.25, 0.75] * 3)[:k]
    assert through(gpu_ctx, TR.stacked_quads(mixed, ctx=gpu_ctx)[2]) == float(np.prod([1.0 - a for a in mixed]))


def test_texels_of_alpha_zero_and_one_and_the_segment_ends(gpu_ctx):
    px = np.zeros((2, 2, 4), np.uint8)
    px[..., :3] = 200
    px[0, :, 3] = 0                                  # the texel row v < 0.5: alpha 0; the other: alpha 1
    px[1, :, 3] = 255
    tc = np.float32([[0.25, 0.25], [0.25, 0.25], [0.25, 0.25], [0.25, 0.25]])
    clear = TR.stacked_quads([1.0, 0.5], texture=(px, tc), ctx=gpu_ctx)[2]
    assert through(gpu_ctx, clear) == 0.5            # an alpha-0 texel lets everything through: what lies behind decides
    assert through(gpu_ctx, clear, tmax=4.5) == 1.0
    solid = TR.stacked_quads([1.0, 0.5], texture=(px, tc + np.float32([0.0, 0.5])), ctx=gpu_ctx)[2]
    assert through(gpu_ctx, solid) == 0.0            # an alpha-1 texel
    behind_opaque = TR.stacked_quads([0.5, 1.0], ctx=gpu_ctx)[2]
    assert through(gpu_ctx, behind_opaque) == 0.0 and through(gpu_ctx, behind_opaque, tmax=5.0) == 0.5
    # the quad at exactly t = tmax is not counted; the quad at exactly t = eps is
    two = TR.stacked_quads([0.5, 0.5], ctx=gpu_ctx)[2]
    assert through(gpu_ctx, two, tmax=4.0) == 1.0
    assert through(gpu_ctx, two, tmax=float(np.nextafter(np.float32(4.0), np.float32(5.0)))) == 0.5
    assert through(gpu_ctx, two, tmax=5.0) == 0.5 and through(gpu_ctx, two, tmax=5.5) == 0.25
    assert through(gpu_ctx, two, eps=4.0) == 0.25
    assert through(gpu_ctx, two, eps=float(np.nextafter(np.float32(4.0), np.float32(5.0)))) == 0.5
    assert through(gpu_ctx, two, eps=0.25, o=np.float32([[5.0, -3.5, 5.75]])) == 0.25      # t = 0.25 = eps exactly
    # a vertex-alpha gradient: 1 - a(u, v), against the float64 reference
    sc, textures, grad = TR.stacked_quads([1.0], vertex_alpha=[0.0, 0.25, 0.5, 0.75], ctx=gpu_ctx)
    exp = TR.reference_T(sc, textures, grad, O_QUAD, D_QUAD, 1e-3, np.inf)
    assert exp.decisive[0] and abs(through(gpu_ctx, grad) - exp.T[0]) <= exp.tol[0] and 0.2 < exp.T[0] < 0.9
    assert api.transmittance(gpu_ctx, two, [[5.0, -3.5, 2.0], [5.0, -3.5, 2.0]], [[5.0, -3.5, 6.5], [5.0, -3.5, 9.0]]).tolist() == [0.5, 0.25]


# ---- closed form ------------------------------------------------------------------------------------------------

def test_mean_visibility_under_a_half_transparent_ceiling(gpu_ctx):
    from tests.test_gpu_occlusion import H_CEILING, quad_y
    cpu = api.SceneCPU()
    cpu.materials = np.array([api.default_material(), api.default_material()], _abi.MATERIAL_DTYPE)
    cpu.materials[1]["color"] = (0.5, 0.5, 0.5, 0.5)
    for v, idx in (quad_y(0.0, 10.0 * H_CEILING, flip=True), quad_y(H_CEILING, 10.0 * H_CEILING)):
        cpu.verts_pos_array.append(v)
        cpu.indices_array.append(idx)
    cpu.mesh_infos = np.array([api.default_mesh_info() for _ in range(2)], _abi.MESH_INFO_DTYPE)
    cpu.instances = np.array([api.default_instance() for _ in range(2)], _abi.INSTANCE_DTYPE)
    cpu.instances["mesh_idx"] = [0, 1]
    cpu.instances["mat_idx"] = [0, 1]
    api.validate_scene(cpu, 0, 0)
    scene = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], [], True)
    point, normal, radius = [[0.3, 0.0, -0.2]], [[0.0, 1.0, 0.0]], 2.0 * H_CEILING
    vis = float(api.ambient_occlusion(gpu_ctx, scene, point, normal, radius, samples=AO_SAMPLES, surface_offset=0.0, opacity=True)[0])
    want, sigma = TR.ceiling_mean_visibility(H_CEILING, radius, 0.5), TR.ceiling_sigma(H_CEILING, radius, 0.5, AO_SAMPLES)
    print(f"mean visibility {vis:.5f}, closed form {want}, sigma {sigma:.5f}")
    assert want == 0.625 and abs(vis - want) <= AO_SIGMAS * sigma
    twin = 1.0 - R.ceiling_blocked_fraction(H_CEILING, radius)          # the twin that ignores opacity expects 0.25
    assert twin == 0.25 and not abs(vis - twin) <= AO_SIGMAS * sigma
    plain = float(api.ambient_occlusion(gpu_ctx, scene, point, normal, radius, samples=AO_SAMPLES, surface_offset=0.0)[0])
    assert abs(plain - twin) <= AO_SIGMAS * R.binomial_sigma(0.75, AO_SAMPLES)       # the default path is the geometric one


# ---- refusals ---------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_the_output_untouched(gpu_ctx):
    c = TR.case("small")
    scene = device_scene(gpu_ctx, "small")
    rec = api.occlusion_records(c.ori[:64], c.dir[:64], 5.0)
    lib = _abi.lib()
    INVALID = -1

    def raw(ctx_h, scene_h, desc, n, records, out, mode=0, samples=1, flags=0, eps=1e-3):
        d = _abi.OcclusionDescC(mode, samples, flags, eps)
        return lib.lupin_hip_transmittance_rays(ctx_h, scene_h, C.byref(d) if desc else None, n, _abi.ptr(records), _abi.ptr(out))

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
    out = fresh(); cases.append(("samples above 2^20", raw(g, s, True, 64, rec, out, mode=1, samples=(1 << 20) + 1), out))
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
            rc, dout = device_transmittance(gpu_ctx, scene, r, mode, S, sentinel=SENTINEL)
            cases.append((f"{label} (device check, mode {mode})", rc, dout))
    d_rec = DeviceArray(gpu_ctx, rec.nbytes + 32).upload(np.concatenate([np.zeros(8, np.float32), rec.reshape(-1)]))
    d_out = DeviceArray(gpu_ctx, 64 * 4 + 32).upload(np.full(64 + 8, SENTINEL, np.uint32))
    cdev = _abi.OcclusionDescC(0, 1, api.OCCLUSION_DEVICE_POINTERS, 1e-3)
    for label, offs in (("records", (8, 0)), ("out_sum", (0, 2))):
        rc = lib.lupin_hip_transmittance_rays(g, s, C.byref(cdev), 64, C.c_void_p(d_rec.ptr + 32 + offs[0]), C.c_void_p(d_out.ptr + offs[1]))
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
    # accepted: n == 0 (nothing touched), samples == 2^20 on one record, tmax = +inf
    out = fresh()
    assert raw(g, s, True, 0, rec, out) == 0 and np.all(out == SENTINEL)
    out = fresh()
    assert raw(g, s, True, 1, rec, out, mode=1, samples=1 << 20) == 0 and 0.0 <= out.view(np.float32)[0] <= float(1 << 20) and np.all(out[1:] == SENTINEL)
    r = rec.copy(); r[9, 7] = np.inf
    out = fresh()
    assert raw(g, s, True, 64, r, out) == 0 and np.all(out.view(np.float32) <= 1.0)
    # what follows is unharmed
    assert np.array_equal(words(api.transmittance_rays(gpu_ctx, scene, rec)), words(direct(gpu_ctx, scene, c.ori[:64], c.dir[:64], 5.0)))


# ---- a refused call between recorded frames -----------------------------------------------------------------------

@pytest.mark.parametrize("S", [1, 65])
def test_a_refused_call_names_its_records_and_leaves_recorded_frames_intact(gpu_ctx, S):
    """Frames recorded and not yet run, then a call refused for its records: host arrays name the first bad index, device
    arrays count the bad records, the output stays untouched, and the frames are what they are without the call.  65 slots
    per record give the last lane of the resolve a partial stride; that the 65-slot sums are right is checked bit for bit
    by test_hemisphere_sum_is_the_restated_resolve_order_over_the_first_rays (S = 65 among its cases)."""
    W, H = 32, 24
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    mode = MODE.DIRECTION if S == 1 else MODE.COSINE_HEMISPHERE
    rng = np.random.default_rng(5)
    nrm = rng.normal(size=(7, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rec = api.occlusion_records(rng.uniform(-0.5, 0.5, (7, 3)) + [0.0, 1.0, 0.0], nrm, 0.7, api.rng_seed_for(np.arange(7, dtype=np.uint32), 0))
    alone = api.transmittance_rays(gpu_ctx, scene, rec, mode, S)
    bad = rec.copy(); bad[3, 1] = np.nan; bad[5, 7] = 0.0
    lib = _abi.lib()

    def host_refusal():
        out = np.full(7, SENTINEL, np.uint32)
        c = _abi.OcclusionDescC(int(mode), S, 0, 1e-3)
        assert lib.lupin_hip_transmittance_rays(gpu_ctx.handle, scene.handle, C.byref(c), 7, _abi.ptr(bad), _abi.ptr(out)) == -1
        assert lib.lupin_hip_last_error().decode().startswith("record 3: ") and np.all(out == SENTINEL)

    def device_refusal():
        rc, out = device_transmittance(gpu_ctx, scene, bad, mode, S, sentinel=SENTINEL)
        assert rc == -1 and lib.lupin_hip_last_error().decode().startswith("2 record(s): ") and np.all(out == SENTINEL)

    plain = util.gpu_accumulate(gpu_ctx, scene, cams[0], W, H, frames=4, spp=1)
    for refusal in (host_refusal, device_refusal):
        assert util.f16_words_differ(util.gpu_accumulate(gpu_ctx, scene, cams[0], W, H, frames=4, spp=1, between=refusal), plain) == 0
    assert np.array_equal(api.transmittance_rays(gpu_ctx, scene, rec, mode, S).view(np.uint32), alone.view(np.uint32))
