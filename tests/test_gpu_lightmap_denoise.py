"""The lightmap denoiser on the device (lupin_hip_denoise_lightmap): the output against the numpy restatement
(tests/lightmap_denoise_ref.py) bit for bit on synthetic and on baked atlases, in-place filtering, the exact cases of the CPU
file, every refusal, the Python mirrors, frames rendered around a call, torch tensors, and what the filter is for: a floor
under a square emitter against the analytic form factor.

Measured on MI355X (64 x 64 floor, Naive, 16 samples; MSE over the 4096 owned texels against pi * L * form factor):
noisy 0.7696, denoised 0.0322, ratio 0.042; mean of the denoised map 1.8280 against 1.8623 noisy (analytic 1.8723),
3 standard errors 0.0772."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import lightmap_denoise_ref as ref
from tests import test_gpu_lightmap as lm
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT = api.PathtraceType
F = np.float32
INVALID = -1
_cache = {}


def denoise_raw(ctx_handle, rgba, rec, out, W, H, passes=5, squarings=5, dilate=0, flags=0, max_stretch=4.0, desc=True):
    """lupin_hip_denoise_lightmap itself, on whatever the three arguments are (arrays, None or raw addresses)."""
    d = _abi.LightmapDenoiseDescC(W, H, passes, squarings, dilate, flags, max_stretch)
    as_ptr = lambda a: a if a is None or isinstance(a, (int, C.c_void_p)) else _abi.ptr(a)  # noqa: E731
    return _abi.lib().lupin_hip_denoise_lightmap(ctx_handle, C.byref(d) if desc else None, as_ptr(rgba), as_ptr(rec), as_ptr(out))


def three_chart_bake(ctx, smooth):
    """The three-chart sphere atlas of tests/test_gpu_lightmap.py at 64 x 64 with 5 samples: (rgba, records)."""
    key = ("bake", smooth)
    if key not in _cache:
        cpu, scene = lm.three_chart_scene(ctx)
        _cache[key] = api.bake_lightmap(ctx, scene, lm.THREE_CHARTS, 64, 64, samples=5, smooth_normals=smooth, surface_offset=1e-3, want_records=True)
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(17, 33), (64, 64)])
@pytest.mark.parametrize("passes,squarings,dilate", [(1, 0, 0), (3, 5, 3), (5, 5, 0), (5, 0, 3)])
def test_synthetic_atlases_equal_the_restatement_bit_for_bit(gpu_ctx, W, H, passes, squarings, dilate):
    rgba, rec = ref.noisy_atlas(H, W, seed=W)
    g = ref.guided(rgba, rec)
    owned = rgba[..., 3] != 0
    assert int((owned & ~g).sum()) == 2 and int((~owned).sum()) > H and np.isnan(rgba[7, 3, 1]) and g[7, 3]
    got = api.denoise_lightmap(gpu_ctx, rgba, rec, passes=passes, normal_squarings=squarings, dilate=dilate)
    want = ref.denoise(rgba, rec, passes=passes, normal_squarings=squarings, dilate=dilate)
    lm.assert_same_words(got, want, f"{W} x {H}, passes {passes}, squarings {squarings}, dilate {dilate}")
    assert not np.isnan(got[owned][:, :3]).any() and np.array_equal(got[..., 3], rgba[..., 3])
    assert int((lm.words(got[g][:, :3]) != lm.words(rgba[g][:, :3])).sum()) > g.sum()       # the filter did something
    assert np.array_equal(got[1, 1], rgba[1, 1]) and got[1, 1, 0] == 30.0                   # not guided: as it came
    half = W // 2
    if dilate:
        assert not np.any(got[..., :3] == 9.0)                                               # the leftovers of the earlier fill are gone
        assert np.all(got[: H - 2, half - 1, :3] != 0.0) and np.all(got[3:6, 2:5, :3] != 0.0)   # the gutter column and the hole are filled
    else:
        lm.assert_same_words(got[~owned], rgba[~owned], "texels nobody owns")
    stats = api.lightmap_denoise_stats()
    assert all(v > 0.0 for v in stats["pass_ms"][:passes]) and all(v == 0.0 for v in stats["pass_ms"][passes:]) and stats["call_ms"] > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("smooth", [False, True])
def test_a_baked_atlas_equals_the_restatement_bit_for_bit(gpu_ctx, smooth):
    rgba, rec = three_chart_bake(gpu_ctx, smooth)
    assert 64 * 64 // 4 < int((rgba[..., 3] == 1).sum()) < 64 * 64
    for dilate in (0, 2):
        got = api.denoise_lightmap(gpu_ctx, rgba, rec, dilate=dilate)
        lm.assert_same_words(got, ref.denoise(rgba, rec, dilate=dilate), f"three-chart atlas, smooth = {smooth}, dilate = {dilate}")
    owned = rgba[..., 3] == 1
    assert int((lm.words(got[owned][:, :3]) != lm.words(rgba[owned][:, :3])).sum()) > owned.sum()


@pytest.mark.gpu
def test_filtering_in_place_gives_the_same_words(gpu_ctx):
    rgba, rec = ref.noisy_atlas(33, 17, seed=3)
    for dilate in (0, 3):
        want = api.denoise_lightmap(gpu_ctx, rgba, rec, dilate=dilate)
        inout = rgba.copy()
        assert denoise_raw(gpu_ctx.handle, inout, rec, inout, 17, 33, dilate=dilate) == 0, _abi.lib().lupin_hip_last_error()
        lm.assert_same_words(inout, want, f"out_rgba == rgba, dilate = {dilate}")


@pytest.mark.gpu
def test_the_exact_atlases_come_back_exact(gpu_ctx):
    for name, (rgba, rec) in (("two charts", ref.two_charts()), ("a folded chart", ref.folded_chart())):
        got = api.denoise_lightmap(gpu_ctx, rgba, rec, passes=5)
        lm.assert_same_words(got, rgba, name)


@pytest.mark.gpu
def test_refusals_leave_out_rgba_untouched(gpu_ctx):
    lib = _abi.lib()
    W, H = 16, 8
    rgba, rec = ref.two_charts()
    cases = []

    def case(label, ctx_h=None, **over):
        out = np.full((H, W, 4), -7.0, F)
        args = dict(rgba=rgba, rec=rec, out=out, W=W, H=H)
        args.update(over)
        cases.append((label, denoise_raw(gpu_ctx.handle if ctx_h is None else ctx_h, **args), out))

    case("null context", ctx_h=C.c_void_p(None))
    case("null desc", desc=False)
    case("null rgba", rgba=None)
    case("null records", rec=None)
    case("width == 0", W=0)
    case("height == 0", H=0)
    case("width above 16384", W=16385)
    case("height above 16384", H=16385)
    case("passes == 0", passes=0)
    case("passes above 8", passes=9)
    case("normal_squarings above 7", squarings=8)
    case("dilate above 64", dilate=65)
    case("unknown flag", flags=2)
    case("unknown flag beside the known one", flags=3)
    for bad in (0.0, -4.0, np.nan, np.inf, -np.inf):
        case(f"max_stretch = {bad}", max_stretch=bad)
    case("a device pointer off its alignment", rgba=C.c_void_p(rgba.ctypes.data + 4), flags=1)      # refused before anything reads it
    other = api.Context(0)
    dead = C.c_void_p(other.handle.value)
    other.close()
    case("a destroyed context", ctx_h=dead)
    for label, rc, out in cases:
        assert rc == INVALID, (label, rc)
        assert lib.lupin_hip_last_error()
        assert np.all(out == -7.0), label
    assert denoise_raw(gpu_ctx.handle, rgba, rec, None, W, H) == INVALID
    # the limits themselves pass
    out = np.full((H, W, 4), -7.0, F)
    assert denoise_raw(gpu_ctx.handle, rgba, rec, out, W, H, passes=8, squarings=7, dilate=64, max_stretch=1e-30) == 0, lib.lupin_hip_last_error()
    assert np.all(out != -7.0)
    for wrong in ((rgba[..., :3], rec), (rgba, rec[..., :7]), (rgba[:4], rec)):
        with pytest.raises(ValueError):
            api.denoise_lightmap(gpu_ctx, *wrong)


@pytest.mark.gpu
def test_bake_lightmap_with_denoise_is_the_two_calls(gpu_ctx):
    cpu, scene = lm.three_chart_scene(gpu_ctx)
    kw = dict(samples=3, pathtrace_type=PT.MIS, surface_offset=1e-3, counter=4)
    before = api.bake_lightmap(gpu_ctx, scene, lm.THREE_CHARTS, 40, 24, dilate=2, **kw)
    noisy, rec = api.bake_lightmap(gpu_ctx, scene, lm.THREE_CHARTS, 40, 24, want_records=True, **kw)
    for dilate in (0, 2):
        want = api.denoise_lightmap(gpu_ctx, noisy, rec, dilate=dilate)
        got, got_rec = api.bake_lightmap(gpu_ctx, scene, lm.THREE_CHARTS, 40, 24, dilate=dilate, want_records=True, denoise=True, **kw)
        lm.assert_same_words(got, want, f"bake_lightmap(denoise=True, dilate={dilate})")
        lm.assert_same_words(got_rec, rec, "its records")
        lm.assert_same_words(api.bake_lightmap(gpu_ctx, scene, lm.THREE_CHARTS, 40, 24, dilate=dilate, denoise=True, **kw), want, "without records")
    assert int((lm.words(want) != lm.words(before)).sum()) > 100
    # the default path is what it was before any denoiser ran in this process
    lm.assert_same_words(api.bake_lightmap(gpu_ctx, scene, lm.THREE_CHARTS, 40, 24, dilate=2, **kw), before, "bake_lightmap() after a denoise")


@pytest.mark.gpu
def test_frames_around_a_denoise_do_not_notice_it(gpu_ctx):
    cpu, scene = lm.three_chart_scene(gpu_ctx)
    rgba, rec = three_chart_bake(gpu_ctx, False)
    W = H = 48

    def chain(denoise_after):
        res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=8, samples_per_pixel=2))
        out = api.DoubleBufferedTexture(gpu_ctx, W, H)
        filtered = None
        for k in range(6):
            api.pathtrace_scene(gpu_ctx, res, scene, out.front(), PT.Standard, lm.camera_desc(out, k))
            out.flip()
            if k + 1 == denoise_after:
                filtered = api.denoise_lightmap(gpu_ctx, rgba, rec, dilate=1)
        out.flip()
        return out.front().download(), filtered

    plain, _ = chain(None)
    with_denoise, filtered = chain(3)
    assert float(plain.astype(np.float32)[..., :3].max()) > 0.0
    assert util.f16_words_differ(with_denoise, plain) == 0
    lm.assert_same_words(api.denoise_lightmap(gpu_ctx, rgba, rec, dilate=1), filtered, "the denoise between the frames against the same call afterwards")


@pytest.mark.gpu
def test_torch_tensors_give_the_same_words(built):
    """Tensors on the device through api.denoise_lightmap, in a process of its own with torch imported first (see
    tests/test_gpu_ray_query.py)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_lightmap_denoise_torch_worker.py")], capture_output=True, text=True,
                         timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "LIGHTMAP DENOISE TORCH OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_a_floor_under_a_square_emitter_gets_closer_to_the_form_factor(gpu_ctx):
    if "emitter" not in lm._cache:      # the scene of tests/test_gpu_lightmap.py's form-factor test
        cpu = api.SceneCPU()
        infos = []
        pos, tris = lm.floor_quad(2.0)
        lm.add_mesh(cpu, infos, pos, tris, lm.QUAD_UV)
        lm.add_mesh(cpu, infos, [(-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1)], [(0, 2, 1), (2, 0, 3)])
        cpu.mesh_infos = np.array(infos, _abi.MESH_INFO_DTYPE)
        cpu.materials = np.array([lm.matte(0.0), lm.matte(0.0, lm.L_EMIT)], _abi.MATERIAL_DTYPE)
        floor, light = api.default_instance(), api.default_instance()
        light["mesh_idx"], light["mat_idx"] = 1, 1
        cpu.instances = np.array([floor, light], _abi.INSTANCE_DTYPE)
        lm._cache["emitter"] = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], [], True)
    scene = lm._cache["emitter"]
    W = H = 64
    noisy, rec = api.bake_lightmap(gpu_ctx, scene, [api.LightmapChart(0)], W, H, samples=16, pathtrace_type=PT.Naive, want_records=True)
    denoised = api.denoise_lightmap(gpu_ctx, noisy, rec)
    owned = noisy[..., 3] == 1
    assert owned.all() and np.array_equal(denoised[..., 3], noisy[..., 3])
    points = rec[..., 0:3].astype(np.float64)
    truth = math.pi * lm.L_EMIT * np.array([[lm.form_factor(points[y, x]) for x in range(W)] for y in range(H)])
    mse_noisy = float(((noisy[..., 0].astype(np.float64) - truth) ** 2)[owned].mean())
    mse_denoised = float(((denoised[..., 0].astype(np.float64) - truth) ** 2)[owned].mean())
    n = int(owned.sum())
    mean_noisy, mean_denoised = float(noisy[..., 0][owned].astype(np.float64).mean()), float(denoised[..., 0][owned].astype(np.float64).mean())
    standard_error = float(noisy[..., 0][owned].astype(np.float64).std(ddof=1)) / math.sqrt(n)
    print(f"MSE noisy {mse_noisy:.4f}, denoised {mse_denoised:.4f}, ratio {mse_denoised / mse_noisy:.3f}; mean noisy {mean_noisy:.4f}, "
          f"denoised {mean_denoised:.4f}, truth {float(truth.mean()):.4f}, 3 standard errors {3 * standard_error:.4f}")
    assert mse_denoised <= 0.5 * mse_noisy, (mse_denoised, mse_noisy)
    assert abs(mean_denoised - mean_noisy) <= 3.0 * standard_error, (mean_denoised, mean_noisy, standard_error)
