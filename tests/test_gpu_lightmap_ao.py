"""Ambient-occlusion and bent-normal atlases on the device (lupin_hip_bake_lightmap_ao): the records are the
lightmap bake's, the planes are the per-texel formulas over the bent-normal query on those records, the gutters are the
lightmap's, the visibility plane feeds the atlas denoiser and the lightmapped view, and every refusal."""
import ctypes as C

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import bent_normal_ref as B
from tests import film_ref
from tests import lightmap_ref as ref
from tests import lightmapped_view_ref as L
from tests.test_gpu_lightmap import (QUAD_UV, THREE_CHARTS, add_mesh, assert_same_words, floor_quad, matte, three_chart_cpu, three_chart_scene, words)
from tests.test_lightmapped_view_cpu import AMBIENT, CAMERA, FLOOR

pytestmark = pytest.mark.gpu

F = np.float32
ATLASES = ((8, 8), (33, 17), (64, 64))           # (width, height)
SMOOTH, OPACITY = api.LIGHTMAP_SMOOTH_NORMALS, api.LIGHTMAP_AO_OPACITY
S = 70                                           # more than a wave's lanes: the last lanes take one slot, the first two
MAX_DISTANCE = 1.5
EPS = 1e-3


def bake_raw(ctx, scene, charts, W, H, sentinel=None, want_bent=True, want_records=True, **over):
    """lupin_hip_bake_lightmap_ao itself: (status, ao, bent or None, records or None, covered)."""
    f = dict(samples=S, max_slots=0, flags=0, dilate=0, counter=0, surface_offset=1e-3, max_distance=MAX_DISTANCE, ray_epsilon=EPS)
    f.update(over)
    d = _abi.LightmapAoDescC(W, H, f["samples"], f["max_slots"], f["flags"], f["dilate"], f["counter"], f["surface_offset"], f["max_distance"],
                             f["ray_epsilon"])
    cc = (_abi.LightmapChartC * max(1, len(charts)))(*[_abi.LightmapChartC(c.instance_idx, c.scale_u, c.scale_v, c.offset_u, c.offset_v) for c in charts])
    fill = 0.0 if sentinel is None else sentinel
    ao = np.full((H, W, 4), fill, np.float32)
    bent = np.full((H, W, 4), fill, np.float32) if want_bent else None
    rec = np.full((H, W, 8), fill, np.float32) if want_records else None
    covered = C.c_uint64(12345)
    rc = _abi.lib().lupin_hip_bake_lightmap_ao(ctx.handle, scene.handle, C.byref(d), cc, len(charts), _abi.ptr(ao), _abi.ptr(bent), _abi.ptr(rec),
                                               C.byref(covered))
    return rc, ao, bent, rec, int(covered.value)


def formulas(sums, samples, normals):
    """The header's per-texel formulas in numpy float32: (ao texels (n, 4), bent texels (n, 4))."""
    a = np.asarray(sums, F)
    v = a[:, 3] / F(samples)
    length = np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2], dtype=F)
    zero = length == F(0.0)
    bent = np.ones((len(a), 4), F)
    bent[:, :3] = a[:, :3] / np.where(zero, F(1.0), length)[:, None]
    bent[zero, :3] = np.asarray(normals, F)[zero]
    return np.stack([v, v, v, np.ones_like(v)], axis=1), bent


@pytest.mark.parametrize("W,H", ATLASES)
def test_records_and_coverage_are_the_lightmap_bakes(gpu_ctx, W, H):
    cpu, scene = three_chart_scene(gpu_ctx)
    for smooth in (False, True):
        lm, lm_rec = api.bake_lightmap(gpu_ctx, scene, THREE_CHARTS, W, H, samples=1, counter=7, smooth_normals=smooth, surface_offset=1e-3, want_records=True)
        rc, ao, bent, rec, covered = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, counter=7, flags=SMOOTH if smooth else 0, samples=3)
        assert rc == 0, _abi.lib().lupin_hip_last_error()
        assert_same_words(rec, lm_rec, f"records {W} x {H}, smooth = {smooth}")
        assert covered == api.lightmap_stats()["covered_texels"] == int((lm[..., 3] == 1.0).sum()) and 0 < covered < W * H
        assert np.array_equal(ao[..., 3], lm[..., 3]) and np.array_equal(bent[..., 3], lm[..., 3])


@pytest.mark.parametrize("flags", [0, OPACITY, SMOOTH, SMOOTH | OPACITY])
@pytest.mark.parametrize("W,H", ATLASES)
def test_the_planes_are_the_formulas_over_the_query_on_the_records(gpu_ctx, W, H, flags):
    cpu, scene = three_chart_scene(gpu_ctx)
    whole = None
    for max_slots in (0, 5 * S + 1):
        rc, ao, bent, rec, covered = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, flags=flags, max_slots=max_slots)
        assert rc == 0, _abi.lib().lupin_hip_last_error()
        mask = rec.view(np.uint32)[..., 7] == 1
        assert covered == int(mask.sum()) > 0
        qrec = rec[mask].copy()
        qrec[:, 7] = MAX_DISTANCE
        sums = api.bent_normal_rays(gpu_ctx, scene, qrec, S, ray_epsilon=EPS, opacity=bool(flags & OPACITY))
        want_ao, want_bent = formulas(sums, S, qrec[:, 4:7])
        assert_same_words(ao[mask], want_ao, f"ao, flags = {flags}, max_slots = {max_slots}")
        assert_same_words(bent[mask], want_bent, f"bent, flags = {flags}, max_slots = {max_slots}")
        assert np.all(ao[~mask] == 0.0) and np.all(bent[~mask] == 0.0) and np.all(rec[~mask] == 0.0)
        if whole is None:
            whole = (ao, bent)
        assert_same_words(ao, whole[0], "ao, chunked against unchunked")
        assert_same_words(bent, whole[1], "bent, chunked against unchunked")
    if (W, H) == (64, 64):
        v = ao[mask][:, 0]
        assert (v < 1.0).sum() > 50 and (v == 1.0).sum() > 50                   # the floor under the spheres is occluded, their tops are not
        assert np.all(np.abs(np.linalg.norm(bent[mask][:, :3].astype(np.float64), axis=1) - 1.0) <= 1e-6)
    # the Python mirror is the same call; out_bent and out_records may be left out
    mine = api.bake_lightmap_ao(gpu_ctx, scene, THREE_CHARTS, W, H, samples=S, max_distance=MAX_DISTANCE, ray_epsilon=EPS, surface_offset=1e-3,
                                smooth_normals=bool(flags & SMOOTH), opacity=bool(flags & OPACITY), want_bent=True, want_records=True)
    for got, want, what in zip(mine, (ao, bent, rec), ("ao", "bent", "records")):
        assert_same_words(got, want, "api.bake_lightmap_ao " + what)
    alone = api.bake_lightmap_ao(gpu_ctx, scene, THREE_CHARTS, W, H, samples=S, max_distance=MAX_DISTANCE, ray_epsilon=EPS, surface_offset=1e-3,
                                 smooth_normals=bool(flags & SMOOTH), opacity=bool(flags & OPACITY))
    assert_same_words(alone, ao, "api ao alone")


@pytest.mark.parametrize("W,H", ATLASES)
def test_dilation_equals_the_restatement_bit_for_bit(gpu_ctx, W, H):
    cpu, scene = three_chart_scene(gpu_ctx)
    rc, plain_ao, plain_bent, _, covered = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, want_records=False)
    assert rc == 0 and 0 < covered < W * H
    for passes in (1, 3):
        rc, ao, bent, _, _ = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, dilate=passes, want_records=False)
        assert rc == 0, _abi.lib().lupin_hip_last_error()
        assert_same_words(ao, ref.dilate(plain_ao, passes), f"ao, dilate = {passes}")
        assert_same_words(bent, ref.dilate(plain_bent, passes), f"bent, dilate = {passes}")
        assert np.array_equal(ao[..., 3], plain_ao[..., 3]) and np.array_equal(bent[..., 3], plain_bent[..., 3])      # gutter alpha stays 0
        assert int((ao[..., :3] != plain_ao[..., :3]).any(axis=-1).sum()) > 0                                       # the gutters took something
        rc, only_ao, _, _, _ = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, dilate=passes, want_bent=False, want_records=False)
        assert rc == 0 and np.array_equal(words(only_ao), words(ao))


def lone_quad(ctx):
    cpu = api.SceneCPU()
    infos = []
    pos, tris = floor_quad(1.0)
    add_mesh(cpu, infos, pos, tris, QUAD_UV)
    cpu.mesh_infos = np.array(infos, _abi.MESH_INFO_DTYPE)
    cpu.materials = np.array([matte(1.0)], _abi.MATERIAL_DTYPE)
    cpu.instances = np.array([api.default_instance()], _abi.INSTANCE_DTYPE)
    api.validate_scene(cpu, 0, 0)
    return cpu, api.build_accel_structures_and_upload(ctx, cpu, [], [], True)


def test_a_quad_alone_sees_everything_and_bends_nowhere(gpu_ctx):
    cpu, scene = lone_quad(gpu_ctx)
    chart = api.LightmapChart(0, 0.71, 0.53, 0.113, 0.291)
    samples = 4096
    ao, bent, rec = api.bake_lightmap_ao(gpu_ctx, scene, [chart], 24, 24, samples=samples, want_bent=True, want_records=True)
    owned = ao[..., 3] == 1.0
    assert 50 < int(owned.sum()) < 24 * 24 and np.array_equal(owned, rec.view(np.uint32)[..., 7] == 1)
    assert np.all(ao[owned][:, :3] == 1.0) and np.all(ao[~owned] == 0.0) and np.all(bent[~owned] == 0.0)
    # bent = sum d / |sum d| about the normal +y.  With m = sum d / samples: E[m] = (0, 2/3, 0) and per-component standard errors
    # se = sqrt(var / samples) (tests/bent_normal_ref.py, the normal's axis being the reference's z).  To first order
    # |bent.x| <= |m.x| / m.y and |bent.z| <= |m.z| / m.y, with m.y at least 2/3 less its own band; 1 - bent.y = 1 - sqrt(1 - s) <= s for
    # s = bent.x^2 + bent.z^2 <= 2 * band^2.
    se = B.standard_errors(B.OPEN_SKY, samples)
    tangent = B.SIGMAS * se[0] / (2.0 / 3.0 - B.SIGMAS * se[2])
    b = bent[owned].astype(np.float64)
    print("largest tangent component", np.abs(b[:, [0, 2]]).max(), "band", tangent, "smallest normal component", b[:, 1].min())
    assert np.all(np.abs(b[:, [0, 2]]) <= tangent) and np.all(1.0 - b[:, 1] <= 2.0 * tangent * tangent) and np.all(bent[owned][:, 3] == 1.0)
    assert np.abs(b[:, [0, 2]]).max() > 0.0                                 # and it is a Monte Carlo answer, not the normal copied


def test_the_visibility_plane_feeds_the_atlas_denoiser(gpu_ctx):
    cpu, scene = lone_quad(gpu_ctx)
    chart = api.LightmapChart(0, 0.71, 0.53, 0.113, 0.291)
    ao, rec = api.bake_lightmap_ao(gpu_ctx, scene, [chart], 24, 24, samples=16, want_records=True)
    out = api.denoise_lightmap(gpu_ctx, ao, rec)
    assert out.shape == ao.shape and np.array_equal(out[..., 3], ao[..., 3])
    assert_same_words(out, ao, "the constant-1 atlas through the filter")
    both = api.bake_lightmap_ao(gpu_ctx, scene, [chart], 24, 24, samples=16, dilate=2, denoise=True)
    assert_same_words(both, api.denoise_lightmap(gpu_ctx, ao, rec, dilate=2), "denoise=True")
    # on an atlas that is not constant the filter runs, keeps alpha and changes texels
    _, three = three_chart_scene(gpu_ctx)
    ao, rec = api.bake_lightmap_ao(gpu_ctx, three, THREE_CHARTS, 64, 64, samples=8, max_distance=MAX_DISTANCE, surface_offset=1e-3, want_records=True)
    out = api.denoise_lightmap(gpu_ctx, ao, rec)
    assert np.array_equal(out[..., 3], ao[..., 3]) and int((out[..., 0] != ao[..., 0]).sum()) > 50 and np.all(out[ao[..., 3] == 0.0] == 0.0)


def test_the_visibility_plane_is_a_lightmap_of_the_lightmapped_view(gpu_ctx):
    """A white matte scene without emission or environment: the view draws albedo * E / pi = v / pi where the atlas is owned."""
    cpu, _ = three_chart_cpu()
    cpu.materials = np.array([matte(1.0), matte(1.0)], _abi.MATERIAL_DTYPE)
    cpu.environments = np.zeros(0, _abi.ENVIRONMENT_DTYPE)
    api.validate_scene(cpu, 0, 0)
    scene = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], [], True)
    charts = THREE_CHARTS + [FLOOR]
    W, H = 33, 17
    px = L.pieces(lambda *a: api.camera_probe(gpu_ctx, *a), lambda o, d, e: api.trace_rays(gpu_ctx, scene, o, d, e),
                  lambda r: api.surface_probe(gpu_ctx, scene, r), W, H, CAMERA[0], CAMERA[1], EPS)
    geo = L.geometry(cpu, scene)
    for AW, AH, dilate in ((64, 64, 0), (33, 17, 3)):
        atlas = api.bake_lightmap_ao(gpu_ctx, scene, charts, AW, AH, samples=32, max_distance=MAX_DISTANCE, dilate=dilate)
        tex = api.Texture(gpu_ctx, W, H)
        tex.upload(np.full((H, W, 4), -7.0, np.float16))
        g = api.render_lightmapped(gpu_ctx, scene, tex, CAMERA[0], CAMERA[1], charts, atlas, ambient=AMBIENT, ray_epsilon=EPS, want_gbuffer=True)
        got = tex.download().view(np.uint16).reshape(-1, 4)
        want_tex, want_g = L.render(px, geo, charts, atlas, None, AMBIENT, film_ref.RTZ)
        assert np.array_equal(words(g.reshape(-1, 20)), words(want_g)) and np.array_equal(got, want_tex), (AW, AH, dilate)
        # where all four taps are owned and fully visible the fetch is 1 and the pixel 1 / pi, to the store's rounding
        lm = words(g.reshape(-1, 20))[:, 19] == L.LIGHTMAP
        assert lm.sum() > 100
        rgb = got.view(np.float16).astype(np.float64)[lm][:, :3]
        assert np.all(rgb <= (1.0 / np.pi) * (1.0 + 2.0 ** -10)) and (np.abs(rgb - 1.0 / np.pi) <= 2.0 ** -11).any()


def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    cpu, scene = three_chart_scene(gpu_ctx)
    lib = _abi.lib()
    W = H = 16
    one = [api.LightmapChart(0)]
    cases = []

    def case(label, charts=one, **over):
        rc, ao, bent, rec, covered = bake_raw(gpu_ctx, scene, charts, W, H, sentinel=-7.0, **over)
        cases.append((label, rc, ao, bent, rec, covered))

    def raw(label, ctx_h, scene_h, desc, charts, num, out, w=W, h=H):
        d = _abi.LightmapAoDescC(w, h, 4, 0, 0, 0, 0, 1e-3, 1.0, 1e-3)
        cc = _abi.LightmapChartC(0, 1.0, 1.0, 0.0, 0.0)
        ao = np.full((H, W, 4), -7.0, np.float32)
        bent = np.full((H, W, 4), -7.0, np.float32)
        rc = lib.lupin_hip_bake_lightmap_ao(ctx_h, scene_h, C.byref(d) if desc else None, C.byref(cc) if charts else None, num,
                                            _abi.ptr(ao) if out else None, _abi.ptr(bent), None, None)
        cases.append((label, rc, ao, bent, None, 12345))

    g, s = gpu_ctx.handle, scene.handle
    raw("null context", None, s, True, True, 1, True)
    raw("null scene", g, None, True, True, 1, True)
    raw("null desc", g, s, False, True, 1, True)
    raw("null charts", g, s, True, False, 1, True)
    raw("null out_ao", g, s, True, True, 1, False)
    raw("num_charts == 0", g, s, True, True, 0, True)
    raw("width == 0", g, s, True, True, 1, True, w=0)                  # the size is in the descriptor alone: the arrays stay small
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
    for flag in (4, 8, 1 << 31):
        case(f"unknown flag {flag}", flags=flag)
    case("dilate above 64", dilate=65)
    case("samples == 0", samples=0)
    case("samples above 2^20", samples=(1 << 20) + 1)
    for md in (0.0, -1.0, np.nan, -np.inf):
        case(f"max_distance = {md}", max_distance=md)
    for eps in (np.nan, np.inf, -1e-3):
        case(f"ray_epsilon = {eps}", ray_epsilon=eps)
    other = api.Context(0)
    ecpu, eenvs = three_chart_cpu()
    foreign = api.build_accel_structures_and_upload(other, ecpu, [], eenvs, True)
    raw("scene of another context", g, foreign.handle, True, True, 1, True)
    other.close()
    raw("scene of a destroyed context", g, foreign.handle, True, True, 1, True)
    for label, rc, ao, bent, rec, covered in cases:
        assert rc == -1, (label, rc)
        assert lib.lupin_hip_last_error()
        assert np.all(ao == -7.0) and np.all(bent == -7.0), label
        assert rec is None or np.all(rec == -7.0), label
        assert covered == 12345, label
    assert len(cases) >= 40
    # an atlas nobody covers: LUPIN_OK and zeros
    rc, ao, bent, rec, covered = bake_raw(gpu_ctx, scene, [api.LightmapChart(0, 1.0, 1.0, 5.0, 5.0)], W, H, sentinel=-7.0, dilate=2)
    assert rc == 0 and covered == 0 and np.all(ao == 0.0) and np.all(bent == 0.0) and np.all(rec == 0.0)
    # the limits themselves pass: every flag, 64 gutter passes, an unbounded distance, a zero epsilon
    rc, ao, _, _, covered = bake_raw(gpu_ctx, scene, one, W, H, dilate=64, flags=SMOOTH | OPACITY, max_distance=np.inf, ray_epsilon=0.0, samples=2,
                                     want_bent=False, want_records=False)
    assert rc == 0 and covered > 0


def test_bake_after_update_instances_equals_a_fresh_scene(gpu_ctx):
    cpu, envs = three_chart_cpu()
    a = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], envs, True)
    moved_cpu, moved_envs = three_chart_cpu(moved=True)
    b = api.build_accel_structures_and_upload(gpu_ctx, moved_cpu, [], moved_envs, True)
    kw = dict(samples=S, max_distance=4.0, surface_offset=1e-3, want_bent=True, want_records=True, dilate=1)
    before = api.bake_lightmap_ao(gpu_ctx, a, THREE_CHARTS, 32, 32, **kw)
    a.update_instances(moved_cpu.instances["transpose_inverse_transform"])
    after = api.bake_lightmap_ao(gpu_ctx, a, THREE_CHARTS, 32, 32, **kw)
    fresh = api.bake_lightmap_ao(gpu_ctx, b, THREE_CHARTS, 32, 32, **kw)
    assert int((words(before[2]) != words(fresh[2])).sum()) > 100       # the move is visible
    for got, want, what in zip(after, fresh, ("ao", "bent", "records")):
        assert_same_words(got, want, f"{what} of the updated scene against a freshly created moved scene")
