"""The device's camera (lupin_hip_camera_probe), film (k_resolve through pathtrace_scene) and tonemapper against the float64
references of tests/camera_ref.py, film_ref.py and tonemap_ref.py.  The same records, cases and assertions
hold the oracle in tests/test_camera_film_cpu.py, where the planted defects are shown to trip them."""
import numpy as np
import pytest

from lupinpathtracer_amd import api
from tests import camera_ref as X
from tests import film_ref as F
from tests import tonemap_ref as T

pytestmark = pytest.mark.gpu

IDENTITY = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], np.float32)


def test_camera_rays_agree_with_float64(gpu_ctx):
    bad, worst_o, worst_d = [], 0.0, 0.0
    for c, ref in zip(X.cases(), X.reference()):
        got = api.camera_probe(gpu_ctx, c.width, c.height, c.cp, c.transform, c.rec)
        o, d = X.deviation(c, ref, got)
        worst_o, worst_d = max(worst_o, o), max(worst_d, d)
        bad += [f"{c.label}: {f}" for f in X.failures(c, ref, got, X.TOLERANCE)]
    print(f"worst deviation: origin {worst_o:.4g}, direction {worst_d:.4g}; tolerance {X.TOLERANCE:.4g}")
    assert bad == [], (len(bad), bad[:5])


def test_camera_probe_rejects_and_ignores(gpu_ctx):
    c = X.cases()[0]
    with pytest.raises(api.LupinError):
        api.camera_probe(gpu_ctx, 0, 4, c.cp, c.transform, c.rec[:4])
    rec = api.camera_records([1, 2], [3, 4], [7, 9], 5)                   # no such mode: zeros, state unchanged
    o, d, s = api.camera_probe(gpu_ctx, 8, 8, c.cp, c.transform, rec)
    assert not o.any() and not d.any() and list(s) == [7, 9]
    assert api.camera_probe(gpu_ctx, 8, 8, c.cp, c.transform, np.zeros((0, 4), np.uint32))[0].shape == (0, 3)


def _render(ctx, res, scene, prev_tex, out_tex, counter):
    api.pathtrace_scene(ctx, res, scene, out_tex, api.PathtraceType.Standard,
                        api.PathtraceDesc(accum_params=api.AccumulationParams(prev_tex, counter),
                                          advanced=api.AdvancedParams(max_radiance=F.MAX_RADIANCE), camera_transform=IDENTITY))
    return out_tex.download().view(np.uint16)


@pytest.mark.parametrize("emission,spp", F.EMISSIONS)
def test_film_words_are_admissible(gpu_ctx, emission, spp):
    scene = F.environment_scene(gpu_ctx, emission)
    res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=4, samples_per_pixel=spp))
    pw = F.prev_words(emission)
    prev = F.half_to_f64(pw)[..., :3]
    a, b = api.Texture(gpu_ctx, F.WIDTH, F.HEIGHT), api.Texture(gpu_ctx, F.WIDTH, F.HEIGHT)
    a.upload(pw.view(np.float16))
    bad = []
    try:
        for mode in (F.RTZ, F.RNE):
            gpu_ctx.set_f16_store_rounding(mode)
            for n in F.COUNTERS:
                film = F.frame(emission, spp, F.MAX_RADIANCE, n, prev)
                bad += F.word_failures(film, _render(gpu_ctx, res, scene, a, b, n), mode, f"counter {n} rounding {mode}")
    finally:
        gpu_ctx.set_f16_store_rounding(0)
    assert bad == [], bad


def test_film_f32_accumulation(gpu_ctx):
    """The f32 words against the reference's f32-mode result: the first frame reads the uploaded f16 prev_frame, the next ones
    the f32 accumulator of the frame before; the f16 texel is the rounded view of the f32 word."""
    emission, spp = F.EMISSIONS[2]
    scene = F.environment_scene(gpu_ctx, emission)
    res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=4, samples_per_pixel=spp))
    pw = F.prev_words(emission)
    tex = [api.Texture(gpu_ctx, F.WIDTH, F.HEIGHT), api.Texture(gpu_ctx, F.WIDTH, F.HEIGHT)]
    tex[0].upload(pw.view(np.float16))
    prev = F.half_to_f64(pw)[..., :3]
    gpu_ctx.set_accumulation_mode(1)
    try:
        for k, n in enumerate((3, 4, 5)):
            film = F.frame(emission, spp, F.MAX_RADIANCE, n, prev)
            words = _render(gpu_ctx, res, scene, tex[k % 2], tex[(k + 1) % 2], n)
            f32 = tex[(k + 1) % 2].download_f32()
            assert film.admits_f32(f32[..., :3]).all() and (f32[..., 3] == 1.0).all(), n
            assert np.array_equal(words[..., :3], F.round_to_half(f32[..., :3].astype(np.float64), F.RTZ)) and (words[..., 3] == F.ALPHA_ONE).all()
            prev = f32[..., :3].astype(np.float64)
    finally:
        gpu_ctx.set_accumulation_mode(0)


@pytest.mark.parametrize("mode", [F.RTZ, F.RNE])
def test_film_batch_of_four_equals_four_single_calls(gpu_ctx, mode):
    """A batch's frame k blends with what frame k - 1 stored, as an f16 texel: four chained calls run as one wavefront leave
    the words of four single calls, and each single call is admissible given the words the one before left."""
    emission, spp = F.EMISSIONS[2]
    scene = F.environment_scene(gpu_ctx, emission)
    res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=4, samples_per_pixel=spp))
    pw = F.prev_words(emission)
    counters = (3, 4, 5, 6)

    def run(batch):
        tex = [api.Texture(gpu_ctx, F.WIDTH, F.HEIGHT), api.Texture(gpu_ctx, F.WIDTH, F.HEIGHT)]
        tex[0].upload(pw.view(np.float16))
        gpu_ctx.set_batch_frames(batch)
        seen = []
        for k, n in enumerate(counters):
            api.pathtrace_scene(gpu_ctx, res, scene, tex[(k + 1) % 2], api.PathtraceType.Standard,
                                api.PathtraceDesc(accum_params=api.AccumulationParams(tex[k % 2], n),
                                                  advanced=api.AdvancedParams(max_radiance=F.MAX_RADIANCE), camera_transform=IDENTITY))
            if batch == 1:
                seen.append(tex[(k + 1) % 2].download().view(np.uint16))
        return seen, tex[1].download().view(np.uint16), tex[0].download().view(np.uint16)

    gpu_ctx.set_f16_store_rounding(mode)
    try:
        singles, third_1, fourth_1 = run(1)
        _, third_4, fourth_4 = run(4)
    finally:
        gpu_ctx.set_batch_frames(0)
        gpu_ctx.set_f16_store_rounding(0)
    assert np.array_equal(third_1, singles[2]) and np.array_equal(fourth_1, singles[3])
    assert np.array_equal(third_4, third_1) and np.array_equal(fourth_4, fourth_1)
    bad, before = [], pw
    for n, words in zip(counters, singles):
        film = F.frame(emission, spp, F.MAX_RADIANCE, n, F.half_to_f64(before)[..., :3])
        bad += F.word_failures(film, words, mode, f"counter {n}")
        before = words
    assert bad == [], bad


CASES = T.cases()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_tonemap_agrees_with_float64(gpu_ctx, k):
    label, src, w, h, desc, before = CASES[k]
    r = T.tonemap(src, w, h, desc, before)               # asserts the exempt share itself
    tex = api.Texture(gpu_ctx, src.shape[1], src.shape[0])
    tex.upload(src.view(np.float16))
    got = api.tonemap_and_fit_aspect(gpu_ctx, tex, w, h, desc, before)
    off = int((np.abs(got.astype(np.int64) - r.bytes) == 1).sum())
    print(label, f"exempt share {r.exempt_share:.4f}, bytes off by one {off}")
    assert T.failures(r, got) == []
