"""Adaptive lightmap baking on the device (lupin_hip_pathtrace_rays_moments, lupin_hip_bake_lightmap_adaptive):
the moments query against tests/lightmap_adaptive_ref.py over the radiance query's own per-slot radiance WORD FOR WORD, the
bake against the restatement's round loop word for word on a fixed and on an adaptive schedule, the records, coverage and
gutters of the plain bake, a closed form, the error bars against float64, every refusal, recorded frames around a call, moved
instances, and torch tensors."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import lightmap_adaptive_ref as A
from tests import lightmap_ref as ref
from tests import util
from tests.test_gpu_lightmap import (L_EMIT, QUAD_UV, THREE_CHARTS, add_mesh, assert_same_words, constant_environment, floor_quad, matte, three_chart_cpu,
                                     three_chart_scene, words)
from tests.test_gpu_lightmap_ao import lone_quad
from tests.test_gpu_lightmap_directional import lit_setting

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
PT = api.PathtraceType
SMOOTH = api.LIGHTMAP_SMOOTH_NORMALS
SAMPLES = (1, 2, 63, 64, 65, 129)          # lanes without a slot, one slot each, a second stride for one lane, a third
RECORDS = (1, 3, 4, 5)                     # a block with idle waves, exactly full, one over
ATLASES = ((8, 8), (16, 16), (33, 17))     # (width, height)
_cache = {}


def bake_raw(ctx, scene, charts, W, H, ad=(0.05, 2, 8, 0), sentinel=None, want_stats=True, want_records=True, **over):
    """lupin_hip_bake_lightmap_adaptive itself: (status, rgba, stats or None, records or None, covered)."""
    f = dict(pathtrace_type=0, max_bounces=8, samples=1, max_slots=0, flags=0, dilate=0, counter=0, surface_offset=1e-3)
    f.update(over)
    d = _abi.LightmapDescC(W, H, int(f["pathtrace_type"]), f["max_bounces"], f["samples"], f["max_slots"], f["flags"], f["dilate"], f["counter"],
                           f["surface_offset"], _abi.AdvancedParamsC(100.0, 0, 0.001))
    a = _abi.LightmapAdaptiveDescC(*ad)
    cc = (_abi.LightmapChartC * max(1, len(charts)))(*[_abi.LightmapChartC(c.instance_idx, c.scale_u, c.scale_v, c.offset_u, c.offset_v) for c in charts])
    fill = 0.0 if sentinel is None else sentinel
    rgba = np.full((H, W, 4), fill, F)
    stats = np.full((H, W, 4), fill, F) if want_stats else None
    rec = np.full((H, W, 8), fill, F) if want_records else None
    covered = C.c_uint64(12345)
    rc = _abi.lib().lupin_hip_bake_lightmap_adaptive(ctx.handle, scene.handle, C.byref(d), C.byref(a), cc, len(charts), _abi.ptr(rgba), _abi.ptr(stats),
                                                     _abi.ptr(rec), C.byref(covered))
    return rc, rgba, stats, rec, int(covered.value)


def slot_radiance(ctx, scene, records, S, ptype=0):
    """(n, S, 4) float32: every slot's radiance, replayed as a one-sample query on the slot's first ray and RNG state."""
    _, rays = api.pathtrace_rays(ctx, scene, records, api.RayQueryDesc(ptype, 8, S), want_rays=True)
    radiance = api.pathtrace_rays(ctx, scene, np.asarray(rays, F).reshape(-1, 8), api.RayQueryDesc(ptype, 8, 1))
    return radiance.reshape(len(records), S, 4)


def owned_records(ctx, scene, charts, W, H, **kw):
    _, rec = api.bake_lightmap(ctx, scene, charts, W, H, samples=1, surface_offset=1e-3, want_records=True, **kw)
    mask = rec.view(np.uint32)[..., 7] == 1
    return rec, mask, np.flatnonzero(mask.reshape(-1))


def emitter_floor(ctx):
    """DESIGN 13's emitter (2 x 2, radiance L_EMIT, at height 1, facing down) over a black 4 x 4 floor with texcoords."""
    if "emitter" not in _cache:
        cpu = api.SceneCPU()
        infos = []
        pos, tris = floor_quad(2.0)
        add_mesh(cpu, infos, pos, tris, QUAD_UV)
        add_mesh(cpu, infos, [(-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1)], [(0, 2, 1), (2, 0, 3)])
        cpu.mesh_infos = np.array(infos, _abi.MESH_INFO_DTYPE)
        cpu.materials = np.array([matte(0.0), matte(0.0, L_EMIT)], _abi.MATERIAL_DTYPE)
        floor, light = api.default_instance(), api.default_instance()
        light["mesh_idx"], light["mat_idx"] = 1, 1
        cpu.instances = np.array([floor, light], _abi.INSTANCE_DTYPE)
        api.validate_scene(cpu, 0, 0)
        _cache["emitter"] = api.build_accel_structures_and_upload(ctx, cpu, [], [], True)
    return _cache["emitter"]


@pytest.mark.parametrize("kind", ["three", "big"])
@pytest.mark.parametrize("S", SAMPLES)
def test_the_moments_are_the_restatement_word_for_word(gpu_ctx, kind, S):
    s = lit_setting(gpu_ctx, kind)                                      # "three": geometry staged in LDS; "big": read from global memory
    rec, mask, _ = owned_records(gpu_ctx, s.scene, s.charts, 16, 16)
    pool = rec[mask][::7][:max(RECORDS)]
    assert len(pool) == max(RECORDS)
    want = A.resolve(slot_radiance(gpu_ctx, s.scene, pool, S))
    print(kind, S, "largest restated M2", float(want[:, 5].max()))
    assert float(want[:, :3].max()) > 0.0 and (float(want[:, 5].max()) > 0.0 or S < 63 or kind == "big")   # (under big's open sky most paths agree)
    plain = api.pathtrace_rays(gpu_ctx, s.scene, pool, api.RayQueryDesc(0, 8, S))
    for n in RECORDS:
        for max_slots in (0, S, 3 * S + 1):
            got = api.pathtrace_rays_moments(gpu_ctx, s.scene, pool[:n], api.RayQueryDesc(0, 8, S, 0, max_slots))
            assert got.shape == (n, 8)
            assert_same_words(got, want[:n], f"{kind}, S = {S}, n = {n}, max_slots = {max_slots}")
    assert np.all(got[:, 3] == 1.0) and np.all(got[:, 6] == F(S)) and np.all(got[:, 7] == 0.0)
    if S <= 2:
        assert_same_words(got[:, :3], plain[:, :3], "the mean against pathtrace_rays' where the two orders coincide")
    else:
        # both sum the same non-negative terms: the wave with ceil(S / 64) + 7 roundings per term, the query's own order with at most S + 1
        bound = 1.01 * 2.0 ** -24 * ((S + 63) // 64 + 7 + S + 1) * np.maximum(got[:, :3], plain[:, :3]).astype(np.float64)
        assert np.all(np.abs(got[:, :3].astype(np.float64) - plain[:, :3]) <= bound)


@pytest.mark.parametrize("W,H", ATLASES)
def test_a_fixed_schedule_is_the_restatement_word_for_word(gpu_ctx, W, H):
    cpu, scene = three_chart_scene(gpu_ctx)
    S = 3
    for smooth in (False, True):
        flags = SMOOTH if smooth else 0
        lm_rec, mask, texel_of = owned_records(gpu_ctx, scene, THREE_CHARTS, W, H, counter=7, smooth_normals=smooth)
        records = lm_rec[mask]
        for R in (1, 2, 5):
            rc, rgba, stats, rec, covered = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, ad=(0.0, R, R, 0), samples=S, counter=7, flags=flags)
            assert rc == 0, _abi.lib().lupin_hip_last_error()
            assert_same_words(rec, lm_rec, f"records {W} x {H}, smooth = {smooth}")
            assert covered == len(texel_of) and 0 < covered < W * H
            st, log = A.run(records, texel_of, W, H, S, 0.0, R, R,
                            lambda rr, r: api.pathtrace_rays_moments(gpu_ctx, scene, rr, api.RayQueryDesc(0, 8, S)))
            assert len(log) == R and np.all(st.n == R * S)
            want_rgba, want_stats = A.planes(st, texel_of, W, H, 0.0, R)
            assert np.all(stats[mask][:, 0] == F(R * S)) and np.all(stats[mask][:, 3] == 0.0) and float(want_rgba[..., :3].max()) > 0.0
            assert_same_words(rgba, want_rgba, f"out_rgba, R = {R}, {W} x {H}, smooth = {smooth}")
            assert_same_words(stats, want_stats, f"out_stats, R = {R}, {W} x {H}, smooth = {smooth}")
            t = api.lightmap_adaptive_stats()
            assert (t["covered_texels"], t["rounds"], t["paths"], t["converged_texels"], t["capped_texels"]) == (covered, R, covered * R * S, 0, covered)
            if R == 2:
                for passes in (1, 3):
                    rc, dilated, dstats, _, _ = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, ad=(0.0, R, R, 0), samples=S, counter=7, flags=flags,
                                                         dilate=passes, max_slots=5 * S + 1)
                    assert rc == 0
                    assert_same_words(dilated, ref.dilate(want_rgba, passes), f"dilate = {passes}")
                    assert_same_words(dstats, want_stats, "the statistics are not dilated")
                    assert np.array_equal(dilated[..., 3], want_rgba[..., 3]) and int((dilated[..., :3] != want_rgba[..., :3]).any(axis=-1).sum()) > 0
    mine = api.bake_lightmap_adaptive(gpu_ctx, scene, THREE_CHARTS, W, H, samples_per_round=S, threshold=0.0, min_rounds=5, max_rounds=5, counter=7,
                                      smooth_normals=True, surface_offset=1e-3, want_stats=True, want_records=True)
    for got, want, what in zip(mine, (rgba, stats, rec), ("rgba", "stats", "records")):
        assert_same_words(got, want, f"api.bake_lightmap_adaptive {what}")


def test_the_adaptive_loop_is_the_restatement_word_for_word(gpu_ctx):
    scene = emitter_floor(gpu_ctx)
    W = H = 16
    S, threshold, min_rounds, max_rounds = 8, 0.15, 2, 12
    charts = [api.LightmapChart(0)]
    lm_rec, mask, texel_of = owned_records(gpu_ctx, scene, charts, W, H)
    assert mask.all()
    traced = []

    def query(rr, r):
        traced.append(len(rr))
        return api.pathtrace_rays_moments(gpu_ctx, scene, rr, api.RayQueryDesc(PT.Naive, 8, S))

    st, log = A.run(lm_rec[mask], texel_of, W, H, S, threshold, min_rounds, max_rounds, query)
    want_rgba, want_stats = A.planes(st, texel_of, W, H, threshold, min_rounds)
    # the reference alone: the run is adaptive in every way the rule can be
    converged_early = (want_stats[..., 3].reshape(-1) == 1.0) & (st.rounds < max_rounds)
    capped = (st.rounds == max_rounds) & (want_stats[..., 3].reshape(-1) == 0.0)
    kept_alive = sum(int((active & ~wants).sum()) for _, wants, active in log)
    print("rounds", len(log), "active per round", traced, "converged early", int(converged_early.sum()), "capped", int(capped.sum()),
          "rounds kept alive by a neighbour", kept_alive)
    assert converged_early.any() and capped.any() and kept_alive > 0
    assert len(set(st.rounds.tolist())) > 2 and traced[-1] < traced[0]

    rc, rgba, stats, rec, covered = bake_raw(gpu_ctx, scene, charts, W, H, ad=(threshold, min_rounds, max_rounds, 0), samples=S, pathtrace_type=PT.Naive)
    assert rc == 0, _abi.lib().lupin_hip_last_error()
    assert_same_words(rgba, want_rgba, "out_rgba")
    assert_same_words(stats, want_stats, "out_stats")
    assert_same_words(rec, lm_rec, "out_records")
    t = api.lightmap_adaptive_stats()
    assert t["rounds"] == len(log) and t["paths"] == S * sum(traced) == int(st.n.sum()) and t["covered_texels"] == covered == W * H
    assert t["converged_texels"] == int((want_stats[..., 3] == 1.0).sum()) and t["converged_texels"] + t["capped_texels"] == covered
    for max_slots in (S, 37 * S + 3):
        rc, again, again_stats, _, _ = bake_raw(gpu_ctx, scene, charts, W, H, ad=(threshold, min_rounds, max_rounds, 0), samples=S, pathtrace_type=PT.Naive,
                                                max_slots=max_slots, want_records=False)
        assert rc == 0
        assert_same_words(again, rgba, f"max_slots = {max_slots}")
        assert_same_words(again_stats, stats, f"max_slots = {max_slots}")


def test_a_quad_under_a_constant_sky_stops_at_min_rounds(gpu_ctx):
    cpu, _ = lone_quad(gpu_ctx)
    envs = constant_environment(cpu, 0.5)
    api.validate_scene(cpu, 0, 0)
    scene = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], envs, True)
    S, min_rounds = 4, 3
    for threshold in (0.05, 1e-6):
        rgba, stats = api.bake_lightmap_adaptive(gpu_ctx, scene, [api.LightmapChart(0)], 8, 8, samples_per_round=S, threshold=threshold,
                                                 min_rounds=min_rounds, max_rounds=10, pathtrace_type=PT.Naive, want_stats=True)
        assert np.all(stats[..., 0] == F(min_rounds * S)) and np.all(stats[..., 1] == 0.0) and np.all(stats[..., 2] == 0.0)
        assert np.all(stats[..., 3] == 1.0)
        assert np.all(rgba[..., :3] == F(np.pi) * F(0.5)) and np.all(rgba[..., 3] == 1.0)
        t = api.lightmap_adaptive_stats()
        assert (t["rounds"], t["paths"], t["converged_texels"], t["capped_texels"]) == (min_rounds, 64 * min_rounds * S, 64, 0)


def test_the_error_bars_are_the_float64_standard_error(gpu_ctx):
    scene = emitter_floor(gpu_ctx)
    W = H = 16
    S, R = 64, 4
    charts = [api.LightmapChart(0)]
    lm_rec, mask, texel_of = owned_records(gpu_ctx, scene, charts, W, H)
    records = lm_rec[mask]
    rounds = [slot_radiance(gpu_ctx, scene, A.round_records(records, np.arange(len(records)), r), S) for r in range(R)]
    st = A.State(len(records))
    for radiance in rounds:
        A.merge(st, np.arange(len(records)), A.resolve(radiance), S)
    _, restated = A.planes(st, texel_of, W, H, 0.0, R)
    lum = A.luminance(np.concatenate(rounds, axis=1)[..., :3]).astype(np.float64)
    N = R * S
    se = np.pi * np.sqrt(((lum - lum.mean(axis=1, keepdims=True)) ** 2).sum(axis=1) / (N * (N - 1.0)))
    own = np.abs(restated[..., 2].reshape(-1).astype(np.float64) - se)
    assert se.max() > 0.1 and np.all(own[se == 0.0] == 0.0)
    deviation = float((own[se > 0] / se[se > 0]).max())
    rc, rgba, stats, _, _ = bake_raw(gpu_ctx, scene, charts, W, H, ad=(0.0, R, R, 0), samples=S, want_records=False)
    assert rc == 0, _abi.lib().lupin_hip_last_error()
    got = np.abs(stats[..., 2].reshape(-1).astype(np.float64) - se)
    print("restatement against float64, largest relative deviation:", deviation, "device:", float((got[se > 0] / se[se > 0]).max()))
    assert np.all(stats[..., 0] == F(N))
    assert np.all(got[se == 0.0] == 0.0) and np.all(got[se > 0] <= 4.0 * deviation * se[se > 0])
    assert_same_words(stats[..., 2], restated[..., 2], "out_stats[2] against the restatement")


def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    cpu, scene = three_chart_scene(gpu_ctx)
    lib = _abi.lib()
    W = H = 16
    one = [api.LightmapChart(0)]
    cases = []

    def case(label, charts=one, ad=(0.05, 2, 8, 0), **over):
        rc, rgba, stats, rec, covered = bake_raw(gpu_ctx, scene, charts, W, H, ad=ad, sentinel=-7.0, **over)
        cases.append((label, rc, (rgba, stats, rec), covered))

    def raw(label, ctx_h, scene_h, desc, ad, charts, num, out, w=W, h=H):
        d = _abi.LightmapDescC(w, h, 0, 8, 4, 0, 0, 0, 0, 1e-3, _abi.AdvancedParamsC(100.0, 0, 0.001))
        a = _abi.LightmapAdaptiveDescC(0.05, 2, 8, 0)
        cc = _abi.LightmapChartC(0, 1.0, 1.0, 0.0, 0.0)
        rgba, stats = np.full((H, W, 4), -7.0, F), np.full((H, W, 4), -7.0, F)
        rc = lib.lupin_hip_bake_lightmap_adaptive(ctx_h, scene_h, C.byref(d) if desc else None, C.byref(a) if ad else None, C.byref(cc) if charts else None,
                                                  num, _abi.ptr(rgba) if out else None, _abi.ptr(stats), None, None)
        cases.append((label, rc, (rgba, stats), 12345))

    g, s = gpu_ctx.handle, scene.handle
    raw("null context", None, s, True, True, True, 1, True)
    raw("null scene", g, None, True, True, True, 1, True)
    raw("null desc", g, s, False, True, True, 1, True)
    raw("null ad", g, s, True, False, True, 1, True)
    raw("null charts", g, s, True, True, False, 1, True)
    raw("null out_rgba", g, s, True, True, True, 1, False)
    raw("num_charts == 0", g, s, True, True, True, 0, True)
    raw("width == 0", g, s, True, True, True, 1, True, w=0)
    raw("height == 0", g, s, True, True, True, 1, True, h=0)
    raw("width above 16384", g, s, True, True, True, 1, True, w=16385)
    raw("height above 16384", g, s, True, True, True, 1, True, h=16385)
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
    for threshold in (-1e-6, -np.inf, np.inf, np.nan):
        case(f"threshold = {threshold}", ad=(threshold, 2, 8, 0))
    case("min_rounds == 0", ad=(0.05, 0, 8, 0))
    case("max_rounds below min_rounds", ad=(0.05, 3, 2, 0))
    case("max_rounds above the cap", ad=(0.05, 2, 4097, 0))
    case("samples * max_rounds above 2^24", ad=(0.05, 2, 4096, 0), samples=4097)
    case("samples * max_rounds above 2^24, in 64 bits only", ad=(0.05, 1, 4096, 0), samples=1 << 20)
    for flag in (1, 1 << 31):
        case(f"unknown adaptive flag {flag}", ad=(0.05, 2, 8, flag))
    other = api.Context(0)
    ecpu, eenvs = three_chart_cpu()
    foreign = api.build_accel_structures_and_upload(other, ecpu, [], eenvs, True)
    raw("scene of another context", g, foreign.handle, True, True, True, 1, True)
    other.close()
    raw("scene of a destroyed context", g, foreign.handle, True, True, True, 1, True)
    for label, rc, outs, covered in cases:
        assert rc == -1, (label, rc)
        assert lib.lupin_hip_last_error()
        for o in outs:
            assert np.all(o == -7.0), label
        assert covered == 12345, label
    assert len(cases) >= 47
    # an atlas nobody covers: LUPIN_OK and zeros
    rc, rgba, stats, rec, covered = bake_raw(gpu_ctx, scene, [api.LightmapChart(0, 1.0, 1.0, 5.0, 5.0)], W, H, sentinel=-7.0, dilate=2)
    assert rc == 0 and covered == 0 and np.all(rgba == 0.0) and np.all(stats == 0.0) and np.all(rec == 0.0)
    # the limits themselves pass
    rc, _, stats, _, covered = bake_raw(gpu_ctx, scene, one, W, H, ad=(0.0, 1, 1, 0), dilate=64, flags=SMOOTH, samples=2, want_records=False)
    assert rc == 0 and covered > 0 and float(stats[..., 0].max()) == 2.0
    rc, _, _, _, _ = bake_raw(gpu_ctx, scene, one, 4, 4, ad=(1e30, 1, 4096, 0), samples=4096, want_stats=False, want_records=False)
    assert rc == 0, _abi.lib().lupin_hip_last_error()
    # the moments query refuses what the radiance query refuses
    rec = api.ray_records(np.zeros((2, 3)), [(0, 1, 0), (0, 2, 0)])
    out = np.full((2, 8), -7.0, F)
    q = _abi.RayQueryDescC(0, 8, 4, 0, 0, _abi.AdvancedParamsC(100.0, 0, 0.001))
    assert lib.lupin_hip_pathtrace_rays_moments(g, s, C.byref(q), 2, _abi.ptr(rec), _abi.ptr(out)) == -1 and np.all(out == -7.0)
    for bad in (_abi.RayQueryDescC(4, 8, 4, 0, 0), _abi.RayQueryDescC(0, 8, 0, 0, 0), _abi.RayQueryDescC(0, 8, 4, 2, 0), _abi.RayQueryDescC(0, 4095, 4, 0, 0)):
        assert lib.lupin_hip_pathtrace_rays_moments(g, s, C.byref(bad), 1, _abi.ptr(rec), _abi.ptr(out)) == -1 and np.all(out == -7.0)
    assert lib.lupin_hip_pathtrace_rays_moments(g, s, C.byref(q), 2, None, _abi.ptr(out)) == -1
    assert lib.lupin_hip_pathtrace_rays_moments(g, s, C.byref(q), 0, _abi.ptr(rec), _abi.ptr(out)) == 0 and np.all(out == -7.0)


def test_frames_around_a_bake_do_not_notice_it(gpu_ctx):
    """Six chained recorded frames with a refused call and a successful one between them: the frames are what they are without."""
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cpu, three = three_chart_scene(gpu_ctx)
    plain = util.gpu_accumulate(gpu_ctx, scene, cams[0], 32, 32, 6, 2)
    done = {}

    def between():
        rc, rgba, stats, _, _ = bake_raw(gpu_ctx, three, [api.LightmapChart(0)], 8, 8, ad=(0.05, 0, 8, 0), sentinel=-7.0)
        assert rc == -1 and np.all(rgba == -7.0) and np.all(stats == -7.0)
        rc, done["rgba"], done["stats"], _, covered = bake_raw(gpu_ctx, three, THREE_CHARTS, 8, 8, ad=(0.1, 2, 4, 0), samples=3)
        assert rc == 0 and covered > 0

    with_calls = util.gpu_accumulate(gpu_ctx, scene, cams[0], 32, 32, 6, 2, between=between)
    assert util.f16_words_differ(plain, with_calls) == 0
    rc, again, again_stats, _, _ = bake_raw(gpu_ctx, three, THREE_CHARTS, 8, 8, ad=(0.1, 2, 4, 0), samples=3)
    assert rc == 0
    assert_same_words(done["rgba"], again, "the bake between recorded frames against the bake alone")
    assert_same_words(done["stats"], again_stats, "its statistics")


def test_bake_after_update_instances_equals_a_fresh_scene(gpu_ctx):
    cpu, envs = three_chart_cpu()
    a = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], envs, True)
    moved_cpu, moved_envs = three_chart_cpu(moved=True)
    b = api.build_accel_structures_and_upload(gpu_ctx, moved_cpu, [], moved_envs, True)
    kw = dict(samples_per_round=6, threshold=0.02, min_rounds=2, max_rounds=6, surface_offset=1e-3, want_stats=True, want_records=True, dilate=1)
    before = api.bake_lightmap_adaptive(gpu_ctx, a, THREE_CHARTS, 32, 32, **kw)
    a.update_instances(moved_cpu.instances["transpose_inverse_transform"])
    after = api.bake_lightmap_adaptive(gpu_ctx, a, THREE_CHARTS, 32, 32, **kw)
    fresh = api.bake_lightmap_adaptive(gpu_ctx, b, THREE_CHARTS, 32, 32, **kw)
    assert int((words(before[2]) != words(fresh[2])).sum()) > 100       # the move is visible
    for got, want, what in zip(after, fresh, ("rgba", "stats", "records")):
        assert_same_words(got, want, f"{what} of the updated scene against a freshly created moved scene")


def test_torch_tensors_give_the_same_words():
    """In a child process (torch initialises the device its own way): device-tensor records through pathtrace_rays_moments."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_lightmap_adaptive_torch_worker.py")], capture_output=True, text=True, timeout=300,
                         cwd=ROOT)
    assert out.returncode == 0 and "TORCH OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
