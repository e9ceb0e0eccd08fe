"""Directional lightmap baking on the device (lupin_hip_bake_lightmap_directional): the records are the lightmap
bake's, the four planes are tests/lightmap_directional_ref.py's reduction over the radiance query's own first rays and per-slot
radiance WORD FOR WORD, chunking does not show, plane 0 is the scalar bake, the gutters are the lightmap's, moved instances,
the open-sky closed form, every refusal, recorded frames around a call, and torch tensors through the view."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import lightmap_directional_ref as D
from tests import lightmap_ref as ref
from tests import util
from tests.test_gpu_closest_hit import staged_in_lds
from tests.test_gpu_lightmap import THREE_CHARTS, assert_same_words, constant_environment, three_chart_cpu, three_chart_scene, words
from tests.test_gpu_lightmap_ao import lone_quad
from tests.test_gpu_lightmapped_view import big_cpu, setting
from tests.test_lightmap_directional_cpu import NORMAL_VARIANCE, SIGMAS, gamma

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SMOOTH = api.LIGHTMAP_SMOOTH_NORMALS
SAMPLES = (1, 2, 63, 64, 65, 129)          # a lane without a slot, one slot each, a second round for one lane, a third
ATLASES = ((8, 8), (16, 16), (33, 17))     # (width, height)


def bake_raw(ctx, scene, charts, W, H, sentinel=None, want_records=True, **over):
    """lupin_hip_bake_lightmap_directional itself: (status, planes, records or None, covered)."""
    f = dict(pathtrace_type=0, max_bounces=8, samples=1, max_slots=0, flags=0, dilate=0, counter=0, surface_offset=1e-3)
    f.update(over)
    d = _abi.LightmapDescC(W, H, int(f["pathtrace_type"]), f["max_bounces"], f["samples"], f["max_slots"], f["flags"], f["dilate"], f["counter"],
                           f["surface_offset"], _abi.AdvancedParamsC(100.0, 0, 0.001))
    cc = (_abi.LightmapChartC * max(1, len(charts)))(*[_abi.LightmapChartC(c.instance_idx, c.scale_u, c.scale_v, c.offset_u, c.offset_v) for c in charts])
    fill = 0.0 if sentinel is None else sentinel
    planes = np.full((4, H, W, 4), fill, F)
    rec = np.full((H, W, 8), fill, F) if want_records else None
    covered = C.c_uint64(12345)
    rc = _abi.lib().lupin_hip_bake_lightmap_directional(ctx.handle, scene.handle, C.byref(d), cc, len(charts), _abi.ptr(planes), _abi.ptr(rec),
                                                        C.byref(covered))
    return rc, planes, rec, int(covered.value)


def restated(ctx, scene, records, S):
    """The planes' owned texels by the restatement: the radiance query's own first rays, and each slot's radiance replayed
    as a one-sample query on that ray's RNG state (the slot's path from its first ray on)."""
    _, rays = api.pathtrace_rays(ctx, scene, records, api.RayQueryDesc(0, 8, S), want_rays=True)
    rays = np.asarray(rays, F).reshape(-1, 8)
    radiance = api.pathtrace_rays(ctx, scene, rays, api.RayQueryDesc(0, 8, 1))
    n = len(records)
    return D.resolve(rays[:, 4:7].reshape(n, S, 3), radiance[:, :3].reshape(n, S, 3))


@pytest.mark.parametrize("W,H", ATLASES)
def test_records_and_coverage_are_the_lightmap_bakes(gpu_ctx, W, H):
    cpu, scene = three_chart_scene(gpu_ctx)
    for smooth in (False, True):
        lm, lm_rec = api.bake_lightmap(gpu_ctx, scene, THREE_CHARTS, W, H, samples=1, counter=7, smooth_normals=smooth, surface_offset=1e-3, want_records=True)
        rc, planes, rec, covered = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, counter=7, flags=SMOOTH if smooth else 0, samples=3)
        assert rc == 0, _abi.lib().lupin_hip_last_error()
        assert_same_words(rec, lm_rec, f"records {W} x {H}, smooth = {smooth}")
        assert covered == api.lightmap_stats()["covered_texels"] == int((lm[..., 3] == 1.0).sum()) and 0 < covered < W * H
        for j in range(4):
            assert np.array_equal(planes[j][..., 3], lm[..., 3])


_lit = {}


def lit_setting(ctx, kind):
    """test_gpu_lightmapped_view's settings; its `big` scene has no light of its own, so here it gets a constant sky."""
    s = setting(ctx, kind)
    if kind == "three":
        return s
    if id(ctx) not in _lit:
        from types import SimpleNamespace
        cpu = big_cpu()
        envs = constant_environment(cpu, 0.5)
        api.validate_scene(cpu, 0, 0)
        scene = api.build_accel_structures_and_upload(ctx, cpu, [], envs, True)
        assert not staged_in_lds(ctx, scene)
        _lit[id(ctx)] = SimpleNamespace(cpu=cpu, scene=scene, charts=s.charts)
    return _lit[id(ctx)]


@pytest.mark.parametrize("kind", ["three", "big"])
@pytest.mark.parametrize("S", SAMPLES)
def test_the_planes_are_the_restatement_word_for_word(gpu_ctx, kind, S):
    s = lit_setting(gpu_ctx, kind)                                      # "three": geometry staged in LDS; "big": read from global memory
    for (W, H), flags in zip(ATLASES, (0, SMOOTH, 0 if kind == "big" else SMOOTH)):
        whole = None
        for max_slots in (0, S, 3 * S + 1):
            rc, planes, rec, covered = bake_raw(gpu_ctx, s.scene, s.charts, W, H, samples=S, flags=flags, max_slots=max_slots)
            assert rc == 0, _abi.lib().lupin_hip_last_error()
            mask = rec.view(np.uint32)[..., 7] == 1
            assert covered == int(mask.sum()) > 0
            if whole is None:
                whole = planes
                want = restated(gpu_ctx, s.scene, rec[mask], S)
                assert float(want[:, 0, :3].max()) > 0.0
                for j in range(4):
                    assert_same_words(planes[j][mask], want[:, j], f"plane {j}, {kind}, S = {S}, {W} x {H}, flags = {flags}")
                    assert np.all(planes[j][~mask] == 0.0)
            assert_same_words(planes, whole, f"max_slots = {max_slots} against unchunked")
    mine, mine_rec = api.bake_lightmap_directional(gpu_ctx, s.scene, s.charts, W, H, samples=S, smooth_normals=bool(flags), surface_offset=1e-3,
                                                   want_records=True)
    assert_same_words(mine, whole, "api.bake_lightmap_directional")
    assert_same_words(mine_rec, rec, "api.bake_lightmap_directional records")


@pytest.mark.parametrize("S", [5, 130])
def test_plane_0_is_the_scalar_bake_within_the_sums_bound(gpu_ctx, S):
    cpu, scene = three_chart_scene(gpu_ctx)
    W = H = 16
    rc, planes, rec, _ = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, samples=S)
    lm = api.bake_lightmap(gpu_ctx, scene, THREE_CHARTS, W, H, samples=S, surface_offset=1e-3)
    assert rc == 0
    mask = lm[..., 3] == 1.0
    got, want = planes[0][mask][:, :3].astype(np.float64) / float(D.K0), lm[mask][:, :3].astype(np.float64)
    # both sum the same non-negative terms: the planes with m = ceil(S / 64) + 8 roundings per term, the scalar bake with at most S + 1
    bound = (gamma(math.ceil(S / 64) + 8) + gamma(S + 1)) * np.maximum(got, want)
    print(S, "largest difference", np.abs(got - want).max(), "smallest bound", bound[want > 0].min())
    assert (np.abs(got - want) <= bound).all() and want.max() > 0.0


@pytest.mark.parametrize("W,H", ATLASES)
def test_dilation_equals_the_restatement_bit_for_bit(gpu_ctx, W, H):
    cpu, scene = three_chart_scene(gpu_ctx)
    rc, plain, _, covered = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, samples=4, want_records=False)
    assert rc == 0 and 0 < covered < W * H
    for passes in (1, 3):
        rc, planes, _, _ = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, samples=4, dilate=passes, want_records=False)
        assert rc == 0, _abi.lib().lupin_hip_last_error()
        for j in range(4):
            assert_same_words(planes[j], ref.dilate(plain[j], passes), f"plane {j}, dilate = {passes}")
            assert np.array_equal(planes[j][..., 3], plain[j][..., 3])                                    # gutter alpha stays 0
        assert int((planes[0][..., :3] != plain[0][..., :3]).any(axis=-1).sum()) > 0                    # the gutters took something


def test_bake_after_update_instances_equals_a_fresh_scene(gpu_ctx):
    cpu, envs = three_chart_cpu()
    a = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], envs, True)
    moved_cpu, moved_envs = three_chart_cpu(moved=True)
    b = api.build_accel_structures_and_upload(gpu_ctx, moved_cpu, [], moved_envs, True)
    kw = dict(samples=70, surface_offset=1e-3, want_records=True, dilate=1)
    before = api.bake_lightmap_directional(gpu_ctx, a, THREE_CHARTS, 32, 32, **kw)
    a.update_instances(moved_cpu.instances["transpose_inverse_transform"])
    after = api.bake_lightmap_directional(gpu_ctx, a, THREE_CHARTS, 32, 32, **kw)
    fresh = api.bake_lightmap_directional(gpu_ctx, b, THREE_CHARTS, 32, 32, **kw)
    assert int((words(before[1]) != words(fresh[1])).sum()) > 100       # the move is visible
    for got, want, what in zip(after, fresh, ("planes", "records")):
        assert_same_words(got, want, f"{what} of the updated scene against a freshly created moved scene")


def test_open_sky_closed_form(gpu_ctx):
    """A lone quad with normal +y under a white sky of radiance L = 0.5: (k0 pi L, k1 pi L 2/3, 0, 0) in the order 1, y, z, x."""
    cpu, _ = lone_quad(gpu_ctx)
    envs = constant_environment(cpu, 0.5)
    api.validate_scene(cpu, 0, 0)
    scene = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], envs, True)
    S, Lsky = 65536, 0.5
    planes = api.bake_lightmap_directional(gpu_ctx, scene, [api.LightmapChart(0)], 4, 4, samples=S)
    assert np.all(planes[..., 3] == 1.0)
    k0, k1 = float(D.K0), float(D.K1)
    want = np.array([k0 * np.pi * Lsky, k1 * np.pi * Lsky * 2.0 / 3.0, 0.0, 0.0])
    se = k1 * np.pi * Lsky * np.sqrt(np.array([0.0, NORMAL_VARIANCE, 0.25, 0.25]) / S)
    band = SIGMAS * se + gamma(math.ceil(S / 64) + 8) * k1 * np.pi * Lsky
    got = planes[..., :3].astype(np.float64)
    print("coefficients", got[:, 0, 0, 0], "want", want, "band", band)
    assert (np.abs(got - want[:, None, None, None]) <= band[:, None, None, None]).all()
    assert np.abs(got[2:]).max() > 0.0                                   # a Monte Carlo answer


def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    cpu, scene = three_chart_scene(gpu_ctx)
    lib = _abi.lib()
    W = H = 16
    one = [api.LightmapChart(0)]
    cases = []

    def case(label, charts=one, **over):
        rc, planes, rec, covered = bake_raw(gpu_ctx, scene, charts, W, H, sentinel=-7.0, **over)
        cases.append((label, rc, planes, rec, covered))

    def raw(label, ctx_h, scene_h, desc, charts, num, out, w=W, h=H):
        d = _abi.LightmapDescC(w, h, 0, 8, 4, 0, 0, 0, 0, 1e-3, _abi.AdvancedParamsC(100.0, 0, 0.001))
        cc = _abi.LightmapChartC(0, 1.0, 1.0, 0.0, 0.0)
        planes = np.full((4, H, W, 4), -7.0, F)
        rc = lib.lupin_hip_bake_lightmap_directional(ctx_h, scene_h, C.byref(d) if desc else None, C.byref(cc) if charts else None, num,
                                                     _abi.ptr(planes) if out else None, None, None)
        cases.append((label, rc, planes, None, 12345))

    g, s = gpu_ctx.handle, scene.handle
    raw("null context", None, s, True, True, 1, True)
    raw("null scene", g, None, True, True, 1, True)
    raw("null desc", g, s, False, True, 1, True)
    raw("null charts", g, s, True, False, 1, True)
    raw("null out_sh", g, s, True, True, 1, False)
    raw("num_charts == 0", g, s, True, True, 0, True)
    raw("width == 0", g, s, True, True, 1, True, w=0)
    raw("height == 0", g, s, True, True, 1, True, h=0)
    raw("width above 16384", g, s, True, True, 1, True, w=16385)
    raw("height above 16384", g, s, True, True, 1, True, h=16385)
    case("instance index out of range", [api.LightmapChart(5)])
    case("a later chart's instance out of range", [api.LightmapChart(0), api.LightmapChart(0xFFFFFFFF)])
    case("a mesh without texcoords", [api.LightmapChart(0), api.LightmapChart(4)])
    for field in ("scale_u", "scale_v", "offset_u", "offset_v"):
        for bad in (np.nan, np.inf, -np.inf):
            c = api.LightmapChart(0)
            setattr(c, field, bad)
            case(f"{field} = {bad}", [c])
    for so in (0.0, -1e-3, np.nan, np.inf):
        case(f"surface_offset = {so}", surface_offset=so)
    for flag in (2, 4, 1 << 31):
        case(f"unknown flag {flag}", flags=flag)
    case("dilate above 64", dilate=65)
    case("samples == 0", samples=0)
    case("samples above 2^27", samples=(1 << 27) + 1)
    case("unknown pathtrace_type", pathtrace_type=4)
    case("max_bounces 4095", max_bounces=4095)
    other = api.Context(0)
    ecpu, eenvs = three_chart_cpu()
    foreign = api.build_accel_structures_and_upload(other, ecpu, [], eenvs, True)
    raw("scene of another context", g, foreign.handle, True, True, 1, True)
    other.close()
    raw("scene of a destroyed context", g, foreign.handle, True, True, 1, True)
    for label, rc, planes, rec, covered in cases:
        assert rc == -1, (label, rc)
        assert lib.lupin_hip_last_error()
        assert np.all(planes == -7.0), label
        assert rec is None or np.all(rec == -7.0), label
        assert covered == 12345, label
    assert len(cases) >= 35
    # an atlas nobody covers: LUPIN_OK and zeros
    rc, planes, rec, covered = bake_raw(gpu_ctx, scene, [api.LightmapChart(0, 1.0, 1.0, 5.0, 5.0)], W, H, sentinel=-7.0, dilate=2)
    assert rc == 0 and covered == 0 and np.all(planes == 0.0) and np.all(rec == 0.0)
    # the limits themselves pass
    rc, planes, _, covered = bake_raw(gpu_ctx, scene, one, W, H, dilate=64, flags=SMOOTH, samples=2, want_records=False)
    assert rc == 0 and covered > 0


def test_frames_around_a_bake_do_not_notice_it(gpu_ctx):
    """Between recorded frames a refused call and a successful one: the frames are what they are without the calls."""
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cpu, three = three_chart_scene(gpu_ctx)
    plain = util.gpu_accumulate(gpu_ctx, scene, cams[0], 32, 32, 4, 2)
    done = {}

    def between():
        rc, planes, _, _ = bake_raw(gpu_ctx, three, [api.LightmapChart(0)], 8, 8, sentinel=-7.0, flags=8)
        assert rc == -1 and np.all(planes == -7.0)
        rc, done["planes"], _, covered = bake_raw(gpu_ctx, three, THREE_CHARTS, 8, 8, samples=3)
        assert rc == 0 and covered > 0

    with_calls = util.gpu_accumulate(gpu_ctx, scene, cams[0], 32, 32, 4, 2, between=between)
    assert util.f16_words_differ(plain, with_calls) == 0
    rc, again, _, _ = bake_raw(gpu_ctx, three, THREE_CHARTS, 8, 8, samples=3)
    assert rc == 0
    assert_same_words(done["planes"], again, "the bake between recorded frames against the bake alone")


def test_torch_tensors_give_the_same_words():
    """In a child process (torch initialises the device its own way): the planes as a device tensor through the view."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_lightmap_directional_torch_worker.py")], capture_output=True, text=True, timeout=300,
                         cwd=ROOT)
    assert out.returncode == 0 and "TORCH OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
