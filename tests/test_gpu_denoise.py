"""lp::denoise on the device (lupin_hip_denoise, csrc/lupin_denoise.hpp): parity with the numpy restatement
(tests/denoise_ref.py), determinism and the deferral contract, quality against converged renders, error behaviour."""
import ctypes as C

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import denoise_ref as R
from tests import util

pytestmark = pytest.mark.gpu

GUIDES = ["none", "albedo", "normals", "both"]


def _tex(ctx, img):
    t = api.Texture(ctx, img.shape[1], img.shape[0])
    t.upload(img)
    return t


def _random_inputs(H, W, seed):
    rng = np.random.default_rng(seed)
    col = np.empty((H, W, 4), np.float32)
    col[..., :3] = rng.exponential(0.6, (H, W, 3)) * (rng.random((H, W, 1)) < 0.97)
    col[..., 3] = rng.random((H, W))
    alb = np.zeros((H, W, 4), np.float32)
    alb[..., :3] = rng.random((H, W, 3))
    alb[..., :3] *= rng.random((H, W, 3)) > 0.1          # some channels below the demodulation floor
    nrm = np.zeros((H, W, 4), np.float32)
    nrm[..., :3] = rng.standard_normal((H, W, 3))
    nrm[..., :3] *= (rng.random((H, W, 1)) > 0.15)       # background pixels: normal 0
    return col.astype(np.float16), alb.astype(np.float16), nrm.astype(np.float16)


def _pick(guides, alb, nrm):
    return (alb if guides in ("albedo", "both") else None), (nrm if guides in ("normals", "both") else None)


def _device_denoise(ctx, col, alb, nrm, quality, res=None):
    H, W = col.shape[:2]
    res = res or api.build_denoise_resources(ctx, W, H)
    tc = _tex(ctx, col)
    ta = _tex(ctx, alb) if alb is not None else None
    tn = _tex(ctx, nrm) if nrm is not None else None
    out = api.Texture(ctx, W, H)
    api.denoise(ctx, res, api.DenoiseDesc(tc, out, albedo=ta, normals=tn, quality=api.DenoiseQuality(quality)))
    return out.download()


def _assert_parity(got, ref, what):
    g = got.view(np.uint16).astype(np.int32)
    r = ref.view(np.uint16).astype(np.int32)
    differ = int((g != r).sum())
    # f16 values of one sign are ordered like their bit patterns: one step of the word = one f16 ulp
    assert np.all(np.sign(got.astype(np.float32)) * np.sign(ref.astype(np.float32)) >= 0), what
    assert int(np.abs(g - r).max()) <= 1, f"{what}: more than 1 f16 ulp"
    assert differ <= 1e-3 * got.size, f"{what}: {differ} of {got.size} words differ"
    return differ


@pytest.mark.parametrize("quality", [0, 1, 2])
def test_parity_with_restatement_random(gpu_ctx, quality):
    H, W = 61, 97
    col, alb, nrm = _random_inputs(H, W, 100 + quality)
    res = api.build_denoise_resources(gpu_ctx, W, H)
    for guides in GUIDES:
        a, n = _pick(guides, alb, nrm)
        got = _device_denoise(gpu_ctx, col, a, n, quality, res)
        ref = R.denoise(col, a, n, quality)
        d = _assert_parity(got, ref, f"q{quality} {guides}")
        print(f"parity q{quality} {guides}: {d} differing words of {got.size}")


def _render(ctx, scene, cam, W, H, frames, spp, falsecolor=None, f32=False, bounces=8):
    res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(max_bounces=bounces, samples_per_pixel=spp))
    out = api.DoubleBufferedTexture(ctx, W, H)
    cp = api.CameraParams(**{**cam.params.__dict__, "aspect": W / H})
    if f32:
        ctx.set_accumulation_mode(1)
    try:
        for k in range(frames):
            desc = api.PathtraceDesc(accum_params=api.AccumulationParams(out.back(), k), camera_params=cp, camera_transform=cam.transform)
            if falsecolor is None:
                api.pathtrace_scene(ctx, res, scene, out.front(), api.PathtraceType.Standard, desc)
            else:
                api.pathtrace_scene_falsecolor(ctx, res, scene, out.front(), falsecolor, desc)
            out.flip()
        out.flip()
        img = out.front().download_f32() if f32 else out.front().download().astype(np.float32)
    finally:
        if f32:
            ctx.set_accumulation_mode(0)
    return img


def _frame_and_gbuffers(ctx, name, W, H=None, spp=8, cam_i=0):
    scene, cams = util.load_scene(name, ctx)
    cam = cams[cam_i]
    H = H or max(4, int(W / cam.params.aspect)) // 4 * 4
    noisy = _render(ctx, scene, cam, W, H, 1, spp)
    alb = _render(ctx, scene, cam, W, H, 16, 1, falsecolor=api.FalsecolorType.Albedo)
    nrm = _render(ctx, scene, cam, W, H, 16, 1, falsecolor=api.FalsecolorType.Normals)
    return scene, cam, H, noisy.astype(np.float16), alb.astype(np.float16), nrm.astype(np.float16)


def test_parity_with_restatement_rendered_cornell(gpu_ctx):
    _, _, H, col, alb, nrm = _frame_and_gbuffers(gpu_ctx, "cornellbox_builtin", 128, 128)
    for quality in (0, 2):
        for guides in ("none", "both"):
            a, n = _pick(guides, alb, nrm)
            got = _device_denoise(gpu_ctx, col, a, n, quality)
            _assert_parity(got, R.denoise(col, a, n, quality), f"cornell q{quality} {guides}")


def test_determinism_and_in_place(gpu_ctx):
    H, W = 61, 97
    col, alb, nrm = _random_inputs(H, W, 7)
    res = api.build_denoise_resources(gpu_ctx, W, H)
    a = _device_denoise(gpu_ctx, col, alb, nrm, 2, res)
    b = _device_denoise(gpu_ctx, col, alb, nrm, 2, res)
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    tc, ta, tn = _tex(gpu_ctx, col), _tex(gpu_ctx, alb), _tex(gpu_ctx, nrm)
    api.denoise(gpu_ctx, res, api.DenoiseDesc(tc, tc, albedo=ta, normals=tn))   # in place
    assert np.array_equal(tc.download().view(np.uint16), a.view(np.uint16))


def test_deferred_batched_calls_run_before_denoise(gpu_ctx):
    """Recorded (unsynced, batched) pathtrace calls whose targets are denoise's inputs run before the filter reads them."""
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cam = cams[0]
    W = H = 96
    res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=6, samples_per_pixel=2))
    dres = api.build_denoise_resources(gpu_ctx, W, H)

    def run(sync_first):
        out = api.DoubleBufferedTexture(gpu_ctx, W, H)
        alb, nrm = api.Texture(gpu_ctx, W, H), api.Texture(gpu_ctx, W, H)
        den = api.Texture(gpu_ctx, W, H)
        k = 0
        for _ in range(3):
            api.pathtrace_scene(gpu_ctx, res, scene, out.front(), 0, api.PathtraceDesc(
                accum_params=api.AccumulationParams(out.back(), k), camera_params=cam.params, camera_transform=cam.transform))
            out.flip()
            k += 1
        plain = api.PathtraceDesc(camera_params=cam.params, camera_transform=cam.transform)
        api.pathtrace_scene_falsecolor(gpu_ctx, res, scene, alb, api.FalsecolorType.Albedo, plain)
        api.pathtrace_scene_falsecolor(gpu_ctx, res, scene, nrm, api.FalsecolorType.Normals, plain)
        for _ in range(5):   # recorded into one wavefront, not run yet
            api.pathtrace_scene(gpu_ctx, res, scene, out.front(), 0, api.PathtraceDesc(
                accum_params=api.AccumulationParams(out.back(), k), camera_params=cam.params, camera_transform=cam.transform))
            out.flip()
            k += 1
        out.flip()
        if sync_first:
            gpu_ctx.sync()
        api.denoise(gpu_ctx, dres, api.DenoiseDesc(out.front(), den, albedo=alb, normals=nrm))
        return den.download(), out.front().download()

    gpu_ctx.set_batch_frames(8)
    try:
        a, fa = run(False)
        b, fb = run(True)
    finally:
        gpu_ctx.set_batch_frames(0)
    assert np.array_equal(fa.view(np.uint16), fb.view(np.uint16))
    assert np.array_equal(a.view(np.uint16), b.view(np.uint16))
    assert np.abs(a.astype(np.float32)[..., :3]).sum() > 0


def _relmse(x, ref):
    x, ref = x[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


def _quality_case(ctx, name, W, H, ref_spp, ref_frames, cam_i=0):
    scene, cam, H, col, alb, nrm = _frame_and_gbuffers(ctx, name, W, H, cam_i=cam_i)
    ref = _render(ctx, scene, cam, W, H, ref_frames, ref_spp, f32=True)
    res = api.build_denoise_resources(ctx, W, H)
    e_noisy = _relmse(col, ref)
    e = [_relmse(_device_denoise(ctx, col, alb, nrm, q, res), ref) for q in (0, 1, 2)]
    print(f"quality {name} {W}x{H}: relMSE noisy {e_noisy:.5f}  low {e[0]:.5f}  medium {e[1]:.5f}  high {e[2]:.5f}  "
          f"ratios {e[0] / e_noisy:.3f} {e[1] / e_noisy:.3f} {e[2] / e_noisy:.3f}")
    return e_noisy, e


def test_quality_cornell(gpu_ctx):
    # 1 frame at 8 spp with 16-frame G-buffers against 4096 spp (16 frames x 256, f32 accumulation)
    e_noisy, e = _quality_case(gpu_ctx, "cornellbox_builtin", 256, 256, 256, 16)
    assert all(x < e_noisy for x in e)
    assert e[2] <= 0.5 * e_noisy


def test_quality_textured_scene(gpu_ctx):
    e_noisy, e = _quality_case(gpu_ctx, "features1", 160, None, 128, 8, cam_i=1)
    assert e[2] < e_noisy


def test_nan_input_gives_finite_output(gpu_ctx):
    H, W = 61, 97
    col, alb, nrm = _random_inputs(H, W, 21)
    col[30, 40, 0] = np.nan
    col[3, 5, :3] = np.inf
    col[60, 96, 2] = -np.inf
    out = _device_denoise(gpu_ctx, col, alb, nrm, 2)
    assert np.all(np.isfinite(out[..., :3].astype(np.float32)))
    _assert_parity(out, R.denoise(col, alb, nrm, 2), "non-finite input")


def test_errors_leave_output_untouched(gpu_ctx):
    H, W = 32, 48
    col, alb, nrm = _random_inputs(H, W, 3)
    res = api.build_denoise_resources(gpu_ctx, W, H)
    tc, ta, tn = _tex(gpu_ctx, col), _tex(gpu_ctx, alb), _tex(gpu_ctx, nrm)
    small = api.Texture(gpu_ctx, W - 4, H)
    marker = np.full((H, W, 4), 0.125, np.float16)
    out = _tex(gpu_ctx, marker)
    lib = _abi.lib()

    def call(pt, a, n, o, q):
        c = _abi.DenoiseDescC(pt and pt.handle, a and a.handle, n and n.handle, o and o.handle, q)
        return lib.lupin_hip_denoise(gpu_ctx.handle, res.handle, C.byref(c))

    bad = [(tc, ta, tn, out, 3), (None, ta, tn, out, 2), (tc, ta, tn, None, 2), (small, None, None, out, 2),
           (tc, small, None, out, 2), (tc, None, small, out, 2), (tc, None, None, small, 0)]
    for args in bad:
        assert call(*args) == -1, args   # LUPIN_ERR_INVALID_ARGUMENT
    with pytest.raises(api.LupinError) as e:
        api.denoise(gpu_ctx, res, api.DenoiseDesc(tc, out, quality=3))
    assert e.value.code == -1
    assert np.array_equal(out.download().view(np.uint16), marker.view(np.uint16))

    # objects of another context, then of a destroyed one
    ctx2 = api.Context(0)
    res2 = api.build_denoise_resources(ctx2, W, H)
    t2 = api.Texture(ctx2, W, H)
    assert call(t2, None, None, out, 2) == -1
    c = _abi.DenoiseDescC(tc.handle, None, None, out.handle, 2)
    assert lib.lupin_hip_denoise(gpu_ctx.handle, res2.handle, C.byref(c)) == -1
    dead = ctx2.handle.value
    ctx2.close()
    c2 = _abi.DenoiseDescC(t2.handle, None, None, t2.handle, 2)
    assert lib.lupin_hip_denoise(C.c_void_p(dead), res2.handle, C.byref(c2)) == -1
    assert np.array_equal(out.download().view(np.uint16), marker.view(np.uint16))
    del res2, t2


def test_denoised_texture_has_no_f32_accumulator(gpu_ctx):
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cam = cams[0]
    W = H = 64
    res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=4, samples_per_pixel=2))
    tex = api.Texture(gpu_ctx, W, H)
    gpu_ctx.set_accumulation_mode(1)
    try:
        api.pathtrace_scene(gpu_ctx, res, scene, tex, 0, api.PathtraceDesc(camera_params=cam.params, camera_transform=cam.transform))
        tex.download_f32()   # valid before
    finally:
        gpu_ctx.set_accumulation_mode(0)
    dres = api.build_denoise_resources(gpu_ctx, W, H)
    api.denoise(gpu_ctx, dres, api.DenoiseDesc(tex, tex))
    with pytest.raises(api.LupinError):
        tex.download_f32()
    assert np.all(np.isfinite(tex.download().astype(np.float32)))


def test_full_size_4k_high(gpu_ctx):
    H, W = 2160, 3840
    rng = np.random.default_rng(4)
    col = np.ones((H, W, 4), np.float16)
    col[..., :3] = rng.exponential(0.5, (H, W, 3)).astype(np.float16)
    res = api.build_denoise_resources(gpu_ctx, W, H)
    tc = _tex(gpu_ctx, col)
    out = api.Texture(gpu_ctx, W, H)
    api.denoise(gpu_ctx, res, api.DenoiseDesc(tc, out))
    got = out.download()
    assert np.all(np.isfinite(got.astype(np.float32)))
    assert got[..., :3].astype(np.float32).var() < col[..., :3].astype(np.float32).var()
