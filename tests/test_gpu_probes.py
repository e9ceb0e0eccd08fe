"""Light-probe baking on the device (lupin_hip_bake_probes): the coefficients against the numpy restatement
(tests/probe_ref.py) of the reduction on the bake's own first rays and one-sample queries along them, bit for bit; chunks
and device pointers; the directions' distribution; closed-form coefficients; refusals; and that frames rendered around a
bake do not notice it.  Contract: include/lupin_hip.h."""
import ctypes as C
import math

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api, loader
from tests import probe_ref, stats, util
from tests import test_gpu_ray_query as rq

PT = api.PathtraceType
words, assert_same_words = rq.words, rq.assert_same_words
INVALID = -1


def scene_box(scene):
    """The box around the scene's instances in world space (as api.scene_world_extent finds it)."""
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in scene.instances:
        box = np.asarray(scene.model_aabbs[int(inst["mesh_idx"])], np.float64)
        if not np.all(box[:3] <= box[3:]):
            continue
        m = np.asarray(inst["transpose_inverse_transform"], np.float64)
        corners = np.array([[box[0 + 3 * (k & 1)], box[1 + 3 * ((k >> 1) & 1)], box[2 + 3 * ((k >> 2) & 1)]] for k in range(8)])
        world = (corners - m[:, 3]) @ np.linalg.inv(m[:, :3]).T
        lo, hi = np.minimum(lo, world.min(axis=0)), np.maximum(hi, world.max(axis=0))
    return lo, hi


def positions_inside(scene, n, seed):
    lo, hi = scene_box(scene)
    f = np.random.default_rng(seed).uniform(0.25, 0.75, (n, 3))
    return (lo + f * (hi - lo)).astype(np.float32)


def probe_records(pos, counter=0):
    p = np.zeros((len(pos), 4), np.float32)
    p[:, :3] = pos
    p.view(np.uint32)[:, 3] = api.rng_seed_for(np.arange(len(pos), dtype=np.uint32), counter)
    return p


def restated(ctx, scene, rays, S, ptype, max_bounces=8, advanced=None):
    """The coefficients from the bake's first rays: every slot's radiance by a one-sample query along its ray (that query is
    pinned to the oracle by tests/test_gpu_ray_query.py), reduced in numpy in the kernel's order."""
    single = api.pathtrace_rays(ctx, scene, rays, api.RayQueryDesc(ptype, max_bounces, 1, 0, 0, advanced or api.AdvancedParams()))
    return probe_ref.bake(rays[:, 4:7], single[:, :3], S), single


BIT_FOR_BIT = [("cornellbox_builtin", PT.Standard), ("cornellbox_builtin", PT.MIS), ("bistro_class_small", PT.Standard),
               ("bistro_class_small", PT.MIS)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,ptype", BIT_FOR_BIT, ids=[f"{n}-{t.name}" for n, t in BIT_FOR_BIT])
def test_coefficients_equal_the_restatement_bit_for_bit(gpu_ctx, name, ptype):
    scene, _ = util.load_scene(name, gpu_ctx)
    # Cornell: geometry staged in LDS; bistro_class_small: global memory, queue sorted into shade order, path state as records
    assert rq.staged_in_lds(gpu_ctx, scene) == rq.STAGED_BY_DEFAULT[name]
    assert (len(rq.bsdf_families(scene)) >= 4) == rq.SORTED[name]
    n = 5                                      # a block of four waves and a block with one
    pos = positions_inside(scene, n, 21)
    lit = 0
    for S in (1, 2, 63, 64, 65, 129, 1000):
        got, rays = api.bake_probes(gpu_ctx, scene, pos, S, ptype, 8, want_rays=True)
        assert got.shape == (n, 9, 4) and got.dtype == np.float32 and rays.shape == (n * S, 8)
        assert_same_words(rays[:, 0:3], np.repeat(pos, S, axis=0), f"S = {S}: origins of the first rays")
        assert np.all(rays.view(np.uint32)[:, 7] == 0)
        seeds = api.ray_sample_seed(np.repeat(api.rng_seed_for(np.arange(n, dtype=np.uint32), 0), S), np.tile(np.arange(S, dtype=np.uint32), n))
        assert np.array_equal(rays.view(np.uint32)[:, 3], rq.pcg_advance(seeds, 2)), S
        want, single = restated(gpu_ctx, scene, rays, S, ptype)
        lit += int((single[:, :3] > 0).any(axis=1).sum())
        assert_same_words(got, want, f"{name} / {ptype.name} / S = {S}")
    assert lit > 100, lit                      # the probes see light: the comparison is not one of zeros


def device_bake(ctx, scene, probes, S, ptype=PT.Standard, max_slots=0, want_rays=False, sentinel=None, max_bounces=8):
    """lupin_hip_bake_probes with LUPIN_PROBES_DEVICE_POINTERS on texture memory: (status, out_sh, rays)."""
    n = len(probes)
    d_probes = rq.DeviceArray(ctx, probes.nbytes).upload(probes)
    d_out = rq.DeviceArray(ctx, n * 144)
    d_rays = rq.DeviceArray(ctx, n * S * 32) if want_rays else None
    if sentinel is not None:
        d_out.upload(np.full(n * 36, sentinel, np.float32))
        if want_rays:
            d_rays.upload(np.full(n * S * 8, sentinel, np.float32))
    c = _abi.ProbeDescC(int(ptype), max_bounces, S, api.PROBES_DEVICE_POINTERS, max_slots, _abi.AdvancedParamsC(100.0, 0, 0.001))
    rc = _abi.lib().lupin_hip_bake_probes(ctx.handle, scene.handle, C.byref(c), n, C.c_void_p(d_probes.ptr), C.c_void_p(d_out.ptr),
                                          C.c_void_p(d_rays.ptr) if want_rays else None)
    out = d_out.download(np.float32, n * 36).reshape(n, 9, 4)
    rays = d_rays.download(np.float32, n * S * 8).reshape(n * S, 8) if want_rays else None
    return rc, out, rays


@pytest.mark.gpu
def test_chunks_and_device_pointers_give_the_same_words(gpu_ctx):
    scene = rq.cornell(gpu_ctx)[0]
    n, S = 25, 100
    pos = positions_inside(scene, n, 22)
    whole, whole_rays = api.bake_probes(gpu_ctx, scene, pos, S, PT.MIS, 8, want_rays=True)
    # the comparison is not one of zeros: only a probe that fell inside the tall box (at most the five within its
    # bounding box) sees no light
    assert int((whole[:, 0, :3] > 0.0).all(axis=1).sum()) >= n - 5
    # 10 whole probes per wavefront (10, 10, 5: no multiple of 256 slots); below S: one probe each; two probes each
    for max_slots in (1003, 3, 2 * S + 1):
        got, rays = api.bake_probes(gpu_ctx, scene, pos, S, PT.MIS, 8, max_slots=max_slots, want_rays=True)
        assert_same_words(got, whole, f"max_slots = {max_slots}")
        assert_same_words(rays, whole_rays, f"first rays, max_slots = {max_slots}")
    for max_slots in (0, 1003):
        rc, got, rays = device_bake(gpu_ctx, scene, probe_records(pos), S, PT.MIS, max_slots, want_rays=True)
        assert rc == 0, _abi.lib().lupin_hip_last_error()
        assert_same_words(got, whole, f"device pointers, max_slots = {max_slots}")
        assert_same_words(rays, whole_rays, f"first rays through device pointers, max_slots = {max_slots}")
    rc, got, _ = device_bake(gpu_ctx, scene, probe_records(pos), S, PT.MIS)
    assert rc == 0
    assert_same_words(got, whole, "device pointers without out_rays")
    assert api.bake_probes(gpu_ctx, scene, pos[:0], S).shape == (0, 9, 4)       # n = 0: nothing happens


@pytest.mark.gpu
def test_directions_are_uniform_on_the_sphere(gpu_ctx):
    env = rq.empty_scene_with_environment(gpu_ctx)
    N = 100_000
    _, rays = api.bake_probes(gpu_ctx, env, [[0.5, -0.25, 2.0]], N, PT.Naive, 1, counter=7, want_rays=True)
    d = rays[:, 4:7].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(d, axis=1) - 1.0) <= 1e-6)
    qd, qbin, domega = stats.sphere_quadrature()
    nbins = 2 * stats.NC * stats.NPHI
    exp_uni = np.bincount(qbin, np.full(len(qd), domega / (4 * math.pi)), nbins) * N
    exp_cos = np.bincount(qbin, np.maximum(qd[:, 2], 0.0) / math.pi * domega, nbins) * N
    obs = np.bincount(stats.sphere_bin(d), minlength=nbins)
    stat, dof, p = stats.chi2_pooled(obs, exp_uni)
    # judged as cosine-weighted about +z: samples where that pdf is zero refute it outright, the chi-square does otherwise
    below = int(obs[exp_cos == 0.0].sum())
    p_cosine = 0.0 if below else stats.chi2_pooled(obs, exp_cos)[2]
    print(f"chi2 {stat:.1f} / {dof} dof, p = {p:.3g}; taken for cosine-weighted: {below} samples where its pdf is zero, p = {p_cosine:.3g}")
    assert p > 1e-3
    assert p_cosine < 1e-3


@pytest.mark.gpu
def test_constant_sky_gives_half_the_sample_pattern(gpu_ctx):
    env = rq.empty_scene_with_environment(gpu_ctx, 0.5)
    pos = np.float32([[0, 0, 0], [3, -2, 1], [-40, 7, 0.5]])
    for S in (1, 65, 4096):
        got = api.bake_probes(gpu_ctx, env, pos, S, PT.Standard, 8, counter=S)
        # 0.5 is a power of two: every product and every sum of the r, g, b accumulators is half that of w
        assert_same_words(got[..., :3], np.float32(0.5) * np.repeat(got[..., 3:4], 3, axis=-1), f"S = {S}")
        w = got[..., 3].astype(np.float64)
        rel = np.abs(w[:, 0] / (2.0 * math.sqrt(math.pi)) - 1.0)
        bound = (S / 64 + 8) * 2.0 ** -24        # worst-case rounding of the strided sum plus the tree
        print(f"S = {S}: |w0 / 2 sqrt(pi) - 1| = {rel.max():.3e} (bound {bound:.3e}); max |w_j| = {np.abs(w[:, 1:]).max():.4f}")
        assert np.all(rel <= bound), (S, rel, bound)
        assert np.all(np.abs(w[:, 1:]) <= 5.0 * math.sqrt(4.0 * math.pi / S)), S


def half_sky(ctx):
    """A black matte square of half-side 1e4 in the plane y = 0 (normal +y) under a constant sky of 0.5."""
    if "half_sky" not in rq._cache:
        cpu = api.SceneCPU()
        m = api.default_material()
        m["color"] = (0.0, 0.0, 0.0, 1.0)
        cpu.materials = np.array([m], _abi.MATERIAL_DTYPE)
        v = np.zeros((4, 4), np.float32)
        v[:, :3] = [(-1e4, 0, -1e4), (1e4, 0, -1e4), (1e4, 0, 1e4), (-1e4, 0, 1e4)]
        cpu.verts_pos_array.append(v)
        cpu.indices_array.append(np.array([0, 1, 2, 0, 2, 3], np.uint32))
        cpu.mesh_infos = np.array([api.default_mesh_info()], _abi.MESH_INFO_DTYPE)
        cpu.instances = np.array([api.default_instance()], _abi.INSTANCE_DTYPE)
        env = api.default_environment()
        env["emission"] = (0.5, 0.5, 0.5)
        cpu.environments = np.array([env], _abi.ENVIRONMENT_DTYPE)
        api.validate_scene(cpu, 0, 0)
        rq._cache["half_sky"] = api.build_accel_structures_and_upload(ctx, cpu, [], [api.EnvMapInfo(np.ones((1, 1, 4), np.float32), 1, 1)], True)
    return rq._cache["half_sky"]


def half_sky_misses(got, up_index, S):
    """Coefficients further than 5 sigma from the closed form of a 0.5 sky over the hemisphere about the axis whose first-band
    index is `up_index`: c0 = 0.5 sqrt(pi), c_up = 0.5 sqrt(3 pi) / 2, every other one 0 (the zonal l = 2 term about the axis
    vanishes over a hemisphere)."""
    want = np.zeros(9)
    want[0] = 0.5 * math.sqrt(math.pi)
    want[up_index] = 0.5 * math.sqrt(3.0 * math.pi) / 2.0
    tol = 5.0 * 0.5 * math.sqrt(4.0 * math.pi / S)
    err = np.abs(got.astype(np.float64) - want[:, None])
    return [(j, float(err[j].max()), tol) for j in range(9) if err[j].max() > tol]


@pytest.mark.gpu
def test_half_a_sky_puts_the_first_band_on_y(gpu_ctx):
    scene = half_sky(gpu_ctx)
    S = 65536
    got = api.bake_probes(gpu_ctx, scene, [[0.0, 1e-2, 0.0]], S, PT.Standard, 8)[0, :, :3]
    print("coefficients (r):", np.array2string(got[:, 0], precision=5))
    assert half_sky_misses(got, 1, S) == []
    # the twin that takes z for up is refuted: the basis is in world axes, index 1 is y
    assert len(half_sky_misses(got, 2, S)) >= 2


def emitter_coefficients(m=2000):
    """Float64 midpoint quadrature over the 2 x 2 emitter at height 1 seen from the origin: (c_j / L, the integral of Y_j^2 over
    its solid angle).  d(omega) = cos(theta') / r^2 dA = dA / r^3."""
    x = (np.arange(m) + 0.5) / m * 2.0 - 1.0
    xx, zz = np.meshgrid(x, x)
    r = np.sqrt(xx * xx + zz * zz + 1.0)
    d = np.stack([xx / r, 1.0 / r, zz / r], -1).reshape(-1, 3)
    domega = ((2.0 / m) ** 2 / r ** 3).reshape(-1)
    Y = api.sh_basis(d)
    return Y.T @ domega, (Y * Y).T @ domega


@pytest.mark.gpu
def test_coefficients_under_a_square_emitter(gpu_ctx):
    scene = rq.emitter_scene(gpu_ctx)
    L, S = rq.L_EMIT, 65536
    unit, squares = emitter_coefficients()
    want = L * unit
    sigma = np.sqrt(np.maximum(4.0 * math.pi * L * L * squares - want * want, 0.0) / S)
    adv = api.AdvancedParams(max_radiance=2.0 * L)
    for ptype in (PT.Naive, PT.Standard):
        got = api.bake_probes(gpu_ctx, scene, [[0.0, 0.0, 0.0]], S, ptype, 8, adv)[0]
        assert np.all(got[:, 0] == got[:, 1]) and np.all(got[:, 1] == got[:, 2])
        err = np.abs(got[:, 0].astype(np.float64) - want)
        for j in range(9):
            print(f"{ptype.name} c[{j}] = {got[j, 0]:+.5f}, quadrature {want[j]:+.5f}, sigma {sigma[j]:.5f}, off by {err[j] / sigma[j]:.2f} sigma")
        assert np.all(err <= 5.0 * sigma), (ptype, err / sigma)
        E = api.sh_irradiance(got, [0.0, 1.0, 0.0])
        print(f"{ptype.name}: sh_irradiance at +y = {E[0]:.4f}; pi L F = {math.pi * L * 0.5541:.4f} (bands above 2 are cut off: printed, not asserted)")


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    scene, cam, rec, want = rq.cornell(gpu_ctx)
    lib = _abi.lib()
    n, S = 8, 4
    probes = probe_records(positions_inside(scene, n, 23))

    def fresh():
        return np.full((n, 9, 4), -7.0, np.float32), np.full((n * S, 8), -7.0, np.float32)

    def raw(ctx_h, scene_h, desc, count, p, out, rays, **over):
        f = dict(pathtrace_type=0, max_bounces=8, samples=S, flags=0, max_slots=0)
        f.update(over)
        c = _abi.ProbeDescC(f["pathtrace_type"], f["max_bounces"], f["samples"], f["flags"], f["max_slots"], _abi.AdvancedParamsC(100.0, 0, 0.001))
        return lib.lupin_hip_bake_probes(ctx_h, scene_h, C.byref(c) if desc else None, count, _abi.ptr(p), _abi.ptr(out), _abi.ptr(rays))

    cases = []

    def case(label, ctx_h, scene_h, desc=True, count=n, p=probes, null_out=False, **over):
        out, rays = fresh()
        cases.append((label, raw(ctx_h, scene_h, desc, count, p, None if null_out else out, rays, **over), out, rays))

    ctx_h, scene_h = gpu_ctx.handle, scene.handle
    case("null context", None, scene_h)
    case("null scene", ctx_h, None)
    case("null desc", ctx_h, scene_h, desc=False)
    case("null probes", ctx_h, scene_h, p=None)
    case("null out_sh", ctx_h, scene_h, null_out=True)
    case("unknown integrator", ctx_h, scene_h, pathtrace_type=4)
    case("unknown flag", ctx_h, scene_h, flags=2)
    case("samples == 0", ctx_h, scene_h, samples=0)
    case("samples above 2^27", ctx_h, scene_h, samples=(1 << 27) + 1)
    case("max_bounces == 4095", ctx_h, scene_h, max_bounces=4095)
    case("n * samples too large", ctx_h, scene_h, count=(1 << 38) // S + 1)
    other = api.Context(0)
    foreign, _ = loader.build_scene_cornell_box(other)
    case("scene of another context", ctx_h, foreign.handle)
    other.close()
    case("scene of a destroyed context", ctx_h, foreign.handle)
    for label, row, col, value in (("NaN position", 5, 1, np.nan), ("infinite position", 0, 2, -np.inf)):
        bad = probes.copy()
        bad[row, col] = value
        case(label + " (host check)", ctx_h, scene_h, p=bad)
        rc, dout, drays = device_bake(gpu_ctx, scene, bad, S, want_rays=True, sentinel=-7.0)
        cases.append((label + " (device check)", rc, dout, drays))
    # device pointers that are not 16-byte aligned: each of the three in turn
    d_probes = rq.DeviceArray(gpu_ctx, probes.nbytes + 32).upload(np.concatenate([np.zeros(8, np.float32), probes.reshape(-1)]))
    d_out = rq.DeviceArray(gpu_ctx, n * 144 + 32).upload(np.full(n * 36 + 8, -7.0, np.float32))
    d_rays = rq.DeviceArray(gpu_ctx, n * S * 32 + 32).upload(np.full(n * S * 8 + 8, -7.0, np.float32))
    cdev = _abi.ProbeDescC(0, 8, S, api.PROBES_DEVICE_POINTERS, 0, _abi.AdvancedParamsC(100.0, 0, 0.001))
    for label, offs in (("probes", (8, 0, 0)), ("out_sh", (0, 8, 0)), ("out_rays", (0, 0, 8))):
        rc = lib.lupin_hip_bake_probes(ctx_h, scene_h, C.byref(cdev), n, C.c_void_p(d_probes.ptr + 32 + offs[0]), C.c_void_p(d_out.ptr + offs[1]),
                                       C.c_void_p(d_rays.ptr + offs[2]))
        cases.append((f"unaligned device pointer: {label}", rc, d_out.download(np.float32, n * 36 + 8), d_rays.download(np.float32, n * S * 8 + 8)))
    for label, rc, out, rays in cases:
        assert rc == INVALID, (label, rc)
        assert lib.lupin_hip_last_error()
        assert np.all(out == -7.0) and np.all(rays == -7.0), label
    # an RNG word may be any bit pattern, and the aligned pointers of the last cases are accepted
    odd = probes.copy()
    odd.view(np.uint32)[2, 3] = 0x7FC00000
    out, rays = fresh()
    assert raw(ctx_h, scene_h, True, n, odd, out, rays) == 0 and not np.any(out == -7.0) and not np.any(rays == -7.0)
    assert lib.lupin_hip_bake_probes(ctx_h, scene_h, C.byref(cdev), n, C.c_void_p(d_probes.ptr + 32), C.c_void_p(d_out.ptr), C.c_void_p(d_rays.ptr)) == 0
    assert_same_words(d_out.download(np.float32, n * 36).reshape(n, 9, 4), api.bake_probes(gpu_ctx, scene, probes[:, :3], S), "bake after the refusals")
    # what follows is unharmed: a query against the oracle's colours
    assert_same_words(api.pathtrace_rays(gpu_ctx, scene, rec)[:, :3], want, "query after the refusals")


@pytest.mark.gpu
def test_a_tree_too_deep_is_refused_as_a_render_refuses_it(gpu_ctx):
    """200 triangles in a chain of depth 200: more stack than a block's LDS holds.  The bake gives the query's (the render's)
    error and leaves its outputs alone."""
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
    scene = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], [], True, blas_builder=rq.chain_bvh)
    with pytest.raises(api.LupinError) as query:
        api.pathtrace_rays(gpu_ctx, scene, api.ray_records([[0.2, 0.2, 1.0]], [[0, 0, -1.0]]))
    with pytest.raises(api.LupinError) as bake:
        api.bake_probes(gpu_ctx, scene, [[0.2, 0.2, 1.0]], 4)
    assert bake.value.code == query.value.code == INVALID
    assert "too deep" in str(bake.value) and str(bake.value) == str(query.value)
    out, rays = np.full((1, 9, 4), -7.0, np.float32), np.full((4, 8), -7.0, np.float32)
    c = _abi.ProbeDescC(0, 8, 4, 0, 0, _abi.AdvancedParamsC(100.0, 0, 0.001))
    probes = probe_records(np.float32([[0.2, 0.2, 1.0]]))
    assert _abi.lib().lupin_hip_bake_probes(gpu_ctx.handle, scene.handle, C.byref(c), 1, _abi.ptr(probes), _abi.ptr(out), _abi.ptr(rays)) == INVALID
    assert np.all(out == -7.0) and np.all(rays == -7.0)
    rc, dout, drays = device_bake(gpu_ctx, scene, probes, 4, want_rays=True, sentinel=-7.0)
    assert rc == INVALID and np.all(dout == -7.0) and np.all(drays == -7.0)


@pytest.mark.gpu
def test_frames_around_a_bake_do_not_notice_it(gpu_ctx):
    scene, cam, _, _ = rq.cornell(gpu_ctx)
    pos = positions_inside(scene, 6, 24)

    def chain(bake_after):
        res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=8, samples_per_pixel=2))
        out = api.DoubleBufferedTexture(gpu_ctx, rq.W, rq.H)
        baked = None
        for k in range(6):
            desc = api.PathtraceDesc(accum_params=api.AccumulationParams(out.back(), k), camera_params=cam.params, camera_transform=cam.transform)
            api.pathtrace_scene(gpu_ctx, res, scene, out.front(), PT.Standard, desc)
            out.flip()
            if k + 1 == bake_after:
                baked = api.bake_probes(gpu_ctx, scene, pos, 70, PT.MIS, 8)
        out.flip()
        return out.front().download(), baked

    plain, _ = chain(None)
    with_bake, baked = chain(3)
    assert float(plain.astype(np.float32)[..., :3].max()) > 0.0
    assert util.f16_words_differ(with_bake, plain) == 0
    assert_same_words(api.bake_probes(gpu_ctx, scene, pos, 70, PT.MIS, 8), baked, "the bake between the frames against the same bake afterwards")


@pytest.mark.gpu
def test_bake_after_update_instances_equals_a_fresh_scene(gpu_ctx):
    cpu, _ = loader.cornell_box_scene_cpu()
    a = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], [], True)
    moved_cpu, _ = loader.cornell_box_scene_cpu()
    t = moved_cpu.instances["transpose_inverse_transform"].copy()
    t[5, :, 3] = (0.2, 0.0, 0.1)        # the short box: world -> local subtracts the offset
    t[6, :, 3] = (-0.1, -0.3, 0.0)      # the tall box, lifted
    moved_cpu.instances["transpose_inverse_transform"] = t
    b = api.build_accel_structures_and_upload(gpu_ctx, moved_cpu, [], [], True)
    pos = positions_inside(a, 12, 25)
    before = api.bake_probes(gpu_ctx, a, pos, 256, PT.MIS, 8)
    a.update_instances(t)
    after = api.bake_probes(gpu_ctx, a, pos, 256, PT.MIS, 8)
    fresh = api.bake_probes(gpu_ctx, b, pos, 256, PT.MIS, 8)
    assert int((words(before) != words(fresh)).sum()) > 100      # the move is visible
    assert_same_words(after, fresh, "updated scene against a freshly created moved scene")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 65])
def test_a_refused_call_names_its_records_and_leaves_recorded_frames_intact(gpu_ctx, S):
    """Frames recorded and not yet run, then a bake refused for its probes: host arrays name the first bad index, device
    arrays count the bad probes (the noun is "probe"), `out_sh` stays untouched, and the frames are what they are without
    the call.  (What 65 samples per probe sum to is checked bit for bit by the tests above: 65 leaves the last lanes of the
    resolve one sample short.)"""
    scene, cam, _, _ = rq.cornell(gpu_ctx)
    probes = probe_records(positions_inside(scene, 7, 31))
    alone = api.bake_probes(gpu_ctx, scene, probes[:, :3], S, PT.Standard, 4)
    bad = probes.copy(); bad[3, 1] = np.nan; bad[5, 2] = np.inf
    lib = _abi.lib()

    def host_refusal():
        out = np.full((7, 36), -7.0, np.float32)
        c = _abi.ProbeDescC(int(PT.Standard), 4, S, 0, 0, _abi.AdvancedParamsC(100.0, 0, 0.001))
        assert lib.lupin_hip_bake_probes(gpu_ctx.handle, scene.handle, C.byref(c), 7, _abi.ptr(bad), _abi.ptr(out), None) == INVALID
        assert lib.lupin_hip_last_error().decode().startswith("probe 3: ") and np.all(out == -7.0)

    def device_refusal():
        rc, out, _ = device_bake(gpu_ctx, scene, bad, S, max_bounces=4, sentinel=-7.0)
        assert rc == INVALID and lib.lupin_hip_last_error().decode().startswith("2 probe(s): ") and np.all(out == -7.0)

    plain = util.gpu_accumulate(gpu_ctx, scene, cam, 32, 24, frames=4, spp=1)
    for refusal in (host_refusal, device_refusal):
        assert util.f16_words_differ(util.gpu_accumulate(gpu_ctx, scene, cam, 32, 24, frames=4, spp=1, between=refusal), plain) == 0
    again = api.bake_probes(gpu_ctx, scene, probes[:, :3], S, PT.Standard, 4)
    assert np.array_equal(np.asarray(again).view(np.uint32), np.asarray(alone).view(np.uint32))
