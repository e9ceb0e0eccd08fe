"""Camera, film and tonemapper against their float64 references (tests/camera_ref.py, film_ref.py, tonemap_ref.py; DESIGN.md
19), without a GPU: the oracle held to the assertions of tests/test_gpu_camera_film.py, every planted defect caught by them,
and the f32 restatement of the reprojection's camera against the same reference."""
import numpy as np
import pytest

from lupinpathtracer_amd import api
from tests import camera_ref as X
from tests import film_ref as F
from tests import tonemap_ref as T

IDENTITY = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 0]], np.float32)


# ---- camera ------------------------------------------------------------------------------------------------------

def test_rng_restatement_matches_the_stream_the_oracle_draws():
    from oracle import oracle
    for gid, counter in ((0, 0), (12345, 1), (4096 * 2160 - 1, 1000), (0xFFFFFFFF, 0xFFFFFFFF)):
        state = X.init_rng(gid, counter)
        want = oracle.rng_stream(gid, counter, 16)
        for k in range(16):
            state, v = X.random_f32(state)
            assert np.float32(v) == want[k] and float(np.float32(v)) == float(v)
    r = np.array([0, 1, (1 << 24) + 1, (1 << 24) + 3, (1 << 25) + 2, (1 << 25) + 6, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF], np.uint32)
    assert np.array_equal(X.u32_to_f32(r), r.astype(np.float32).astype(np.float64))      # ties to even, and 2^32 at the top
    assert X.random_f32(np.uint32(0))[1] < 1.0


def test_camera_tolerance_is_four_noise_floors_and_far_below_every_defect():
    floor = X.noise_floor()
    print(f"float32 noise floor {floor:.4g}, tolerance {X.TOLERANCE:.4g}")
    assert X.TOLERANCE_FACTOR * floor <= X.TOLERANCE <= 1.05 * X.TOLERANCE_FACTOR * floor
    smallest = np.inf
    for d in X.DEFECTS:
        effect = X.worst_deviation(lambda c: c.evaluate(np.float32, d))
        print(f"{d}: worst deviation {effect:.4g}")
        smallest = min(smallest, effect)
        caught = [f for c, ref in zip(X.cases(), X.reference()) for f in X.failures(c, ref, c.evaluate(np.float32, d), X.TOLERANCE)]
        assert caught, f"{d} went unnoticed"
    assert X.TOLERANCE * 100 <= smallest
    clean = [f for c, ref in zip(X.cases(), X.reference()) for f in X.failures(c, ref, c.evaluate(np.float32), X.TOLERANCE)]
    assert clean == []


def test_camera_records_cover_the_grid():
    cs = X.cases()
    assert len(cs) == 48 * 4 * 4 and {(c.width, c.height) for c in cs} == set(X.SIZES)
    n = sum(len(c.rec) for c in cs)
    assert 5e5 < n < 2e6
    big = X.pixel_records(4096, 2160)
    assert {(4095, 2159), (0, 0), (2048, 1080)} <= {(int(r[0]), int(r[1])) for r in big}
    assert {0, 0xFFFFFFFF, int(X.init_rng(0, 1000)[()])} <= {int(r[2]) for r in big if r[0] == 0 and r[1] == 0}
    t = X.transforms()
    assert not np.array_equal(t["nonaffine"][:, 3], [0, 0, 0, 1]) and np.array_equal(t["rigid"][:, 3], [0, 0, 0, 1])


def test_oracle_camera_agrees_with_float64():
    from oracle import oracle
    bad = []
    for c, ref in zip(X.cases(), X.reference()):
        got = oracle.camera_probe(c.width, c.height, c.cp, c.transform, c.rec)
        bad += [f"{c.label}: {f}" for f in X.failures(c, ref, got, X.TOLERANCE)]
    assert bad == [], bad[:5]


def test_oracle_camera_probe_is_the_camera_of_its_renders():
    """The probe's entry against oracle.camera_rays, which walks the render's own prologue."""
    from oracle import oracle
    cp = api.CameraParams(lens=0.035, film=0.03, aspect=1.6, focus=3.0, aperture=0.2)
    tr = X.transforms()["rigid"]
    scene = F.environment_scene(None, (1.0, 1.0, 1.0))
    for counter in (0, 5):
        ori, d = oracle.camera_rays(scene, 16, 10, cp, tr[:, :3], counter)
        yy, xx = np.meshgrid(np.arange(10), np.arange(16), indexing="ij")
        rec = api.camera_records(xx.reshape(-1), yy.reshape(-1), X.init_rng(yy.reshape(-1) * 16 + xx.reshape(-1), counter))
        o2, d2, _ = oracle.camera_probe(16, 10, cp, tr, rec)
        assert np.array_equal(ori.reshape(-1, 3), o2) and np.array_equal(d.reshape(-1, 3), d2)


@pytest.mark.parametrize("ortho", [False, True])
def test_reprojection_restatement_agrees_with_the_camera_reference(ortho):
    from tests import reproject_ref
    W, H = 48, 32
    cp = api.CameraParams(is_orthographic=ortho, lens=0.035, film=0.036, aspect=1.5, focus=7.0, aperture=0.25)
    tr = X.transforms()["rigid"]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    case = X.Case("centre", W, H, cp, tr, api.camera_records(xx.reshape(-1), yy.reshape(-1), 0, api.CameraMode.RAY_CENTRE))
    ref = case.evaluate(np.float64)
    o32, d32 = reproject_ref.centre_rays(W, H, cp, tr[:, :3])
    o, d = X.deviation(case, ref, (o32.reshape(-1, 3), d32.reshape(-1, 3)))
    assert o <= X.TOLERANCE and d <= X.TOLERANCE
    # project() inverts the ray: camera-space points on the reference's rays come back to their pixels.  In pixels the
    # tolerance is the direction's, times the width of the film in pixels over its angular width (resx * lens / film_x).
    m = np.eye(4)
    m[:3, :] = tr[:, :3].astype(np.float64).T
    inv = np.linalg.inv(m)
    for t in (0.5, 4.0, 90.0):
        p = ref[0] + ref[1] * t
        pc = p @ inv[:3, :3].T + inv[:3, 3]
        fx, fy = reproject_ref.project(cp, W, H, pc.astype(np.float32))
        per_pixel = X.TOLERANCE * max(W, H) * cp.lens / (cp.film / cp.aspect) * (1.0 + np.abs(pc).max())
        assert np.abs(fx - xx.reshape(-1)).max() <= max(per_pixel, 2 * W * 2.0 ** -24) * 4
        assert np.abs(fy - yy.reshape(-1)).max() <= max(per_pixel, 2 * H * 2.0 ** -24) * 4


# ---- film --------------------------------------------------------------------------------------------------------

def f32_film(emission, spp, max_radiance, counters, prev_words, mode, defect=None):
    """pathtrace_main's epilogue in numpy float32, in the shader's order, over consecutive frames each reading what the one
    before stored: the words stored by the last frame.  Stands in for a device that the planted defects can be applied to."""
    f = np.float32
    r = np.asarray(emission, np.float32)
    if not np.isfinite(r).all():
        r = np.zeros(3, np.float32)
    if (r > f(max_radiance)).any():
        r = r * (f(max_radiance) / r.max())
    prev = F.half_to_f64(prev_words)[..., :3].astype(np.float32)
    for n in counters:
        s = np.zeros(3, np.float32)
        for _ in range(spp):
            s = s + r
        c = np.maximum(s / f(spp), f(0))
        c = np.broadcast_to(c, prev.shape)
        if n != 0:
            w = f(1) / f(n + 1 if defect == "weight_n_plus_1" else n)
            c = prev * (f(1) - w) + c * w
            if defect != "no_second_max":
                c = np.maximum(c, f(0))
        words = F.round_to_half(c.astype(np.float64), F.RNE if defect == "nearest_even_store" else mode)
        prev = c if defect == "prev_unrounded" else F.half_to_f64(words).astype(np.float32)
    return words


def film_chain_failures(emission, spp, counters, pw, mode, got_final):
    """A chain of frames against the reference under its read-back rule.  The reference's own stored word carries the chain
    on; a frame whose admissible range has two words makes what follows ambiguous, so those texels are left out."""
    prev = F.half_to_f64(pw)[..., :3]
    firm = np.ones(prev.shape, bool)
    for k, n in enumerate(counters):
        film = F.frame(emission, spp, F.MAX_RADIANCE, n, prev)
        lo, hi = film.words(mode)
        if k + 1 < len(counters):
            firm &= lo == hi
            prev = F.half_to_f64(lo)
    ok = film.admits(got_final[..., :3], mode) | ~firm
    return [] if ok.all() else [f"{int((~ok).sum())} words outside the admissible set"], float(firm.mean())


def test_f16_rounding_from_the_bit_layout():
    words = np.arange(0x7C00, dtype=np.uint16)
    v = F.half_to_f64(words)
    assert np.array_equal(v, words.view(np.float16).astype(np.float64))
    for mode in (F.RTZ, F.RNE):
        assert np.array_equal(F.round_to_half(v, mode), words) and np.array_equal(F.round_to_half(-v, mode), words | 0x8000)
    mid = (v[:-1] + v[1:]) / 2
    assert np.array_equal(F.round_to_half(mid, F.RTZ), words[:-1])
    assert np.array_equal(F.round_to_half(mid, F.RNE), words[:-1] + (words[:-1] & 1))
    assert np.array_equal(F.round_to_half(np.nextafter(mid, np.inf), F.RNE), words[1:])
    assert list(F.round_to_half([65519.9, 65520.0, 1e30, np.inf], F.RNE)) == [0x7BFF, 0x7C00, 0x7C00, 0x7C00]
    assert list(F.round_to_half([65519.9, 65520.0, 1e30, np.inf], F.RTZ)) == [0x7BFF, 0x7BFF, 0x7BFF, 0x7C00]


@pytest.mark.parametrize("emission,spp", F.EMISSIONS)
def test_oracle_film_and_f32_restatement_are_admissible(emission, spp):
    from oracle import oracle
    scene = F.environment_scene(None, emission)
    pw = F.prev_words(emission)
    prev = F.half_to_f64(pw)[..., :3]
    for n in F.COUNTERS:
        for mode in (F.RTZ, F.RNE):
            film = F.frame(emission, spp, F.MAX_RADIANCE, n, prev)
            got, _, f32 = oracle.pathtrace(scene, F.WIDTH, F.HEIGHT, api.CameraParams(), IDENTITY, 4, spp, 0, accum_counter=n,
                                           prev_frame=pw.view(np.float16), advanced=api.AdvancedParams(max_radiance=F.MAX_RADIANCE),
                                           store_rounding=mode, want_f32=True)
            label = f"E {emission} spp {spp} counter {n} rounding {mode}"
            assert F.word_failures(film, got.view(np.uint16), mode, label) == []
            assert film.admits_f32(f32).all(), label
            assert F.word_failures(film, np.concatenate([f32_film(emission, spp, F.MAX_RADIANCE, [n], pw, mode), pw[..., 3:]], -1), mode, label) == []
            lo, hi = film.words(mode)
            assert (lo != hi).mean() <= (1.0 if n == 0 or n == 1 else 0.3), label    # wide only where the clamp's product sits on a boundary
            if n in (3, 7, 1000) and mode == F.RTZ and np.isfinite(emission).all():
                assert (hi[5] == pw[5, :, :3]).all() and (lo[5] == pw[5, :, :3] - 1).all()   # prev == colour: the decaying case, two words
            if n == 2 and spp in (1, 2, 4) and not (np.asarray(emission) > F.MAX_RADIANCE).any():
                assert (film.err[[0, 3, 4, 5]] == 0).all() and (lo[[0, 3, 4, 5]] == hi[[0, 3, 4, 5]]).all()   # short operands: nothing rounds


def test_oracle_f32_accumulation_chain_is_admissible():
    from oracle import oracle
    emission, spp = F.EMISSIONS[2]
    scene = F.environment_scene(None, emission)
    pw = F.prev_words(emission)
    prev = F.half_to_f64(pw)[..., :3]
    p32 = None
    for n in (3, 4, 5):
        film = F.frame(emission, spp, F.MAX_RADIANCE, n, prev)
        got, _, f32 = oracle.pathtrace(scene, F.WIDTH, F.HEIGHT, api.CameraParams(), IDENTITY, 4, spp, 0, accum_counter=n,
                                       prev_frame=pw.view(np.float16), advanced=api.AdvancedParams(max_radiance=F.MAX_RADIANCE),
                                       want_f32=True, prev_frame_f32=p32)
        assert film.admits_f32(f32).all()
        p32, prev = f32, f32.astype(np.float64)        # the next frame blends with the f32 words, not with the f16 view


@pytest.mark.parametrize("defect", ["nearest_even_store", "weight_n_plus_1", "no_second_max", "prev_unrounded"])
def test_film_detects(defect):
    emission, spp = F.EMISSIONS[2]
    pw = F.prev_words(emission)
    counters = [3, 4, 5, 6]
    clean, firm = film_chain_failures(emission, spp, counters, pw, F.RTZ, f32_film(emission, spp, F.MAX_RADIANCE, counters, pw, F.RTZ))
    assert clean == [] and firm > 0.5
    bad, _ = film_chain_failures(emission, spp, counters, pw, F.RTZ, f32_film(emission, spp, F.MAX_RADIANCE, counters, pw, F.RTZ, defect))
    print(defect, bad)
    assert bad, "the defect went unnoticed"


# ---- tonemap -----------------------------------------------------------------------------------------------------

CASES = T.cases()


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_oracle_tonemap_agrees_with_float64(k):
    from oracle import oracle
    label, src, w, h, desc, before = CASES[k]
    r = T.tonemap(src, w, h, desc, before)               # asserts the exempt share itself
    print(label, f"exempt share {r.exempt_share:.4f}")
    assert r.shaded.any()
    assert T.failures(r, oracle.tonemap(src.view(np.float16), w, h, desc, before)) == []


def test_tonemap_inputs_reach_the_edges_the_issue_names():
    g = F.half_to_f64(T.gradient_source())[..., :3]
    assert (np.isfinite(g) & (g > 0) & (g <= T.CUTOFF)).sum() >= 6 and (g > T.CUTOFF).sum() > 1000 and np.nanmax(g[np.isfinite(g)]) == 65504.0
    assert (g[7] < 0).all() and (~np.isfinite(g)).sum() == 3 and g[np.isfinite(g)].max() >= 16
    r = T.tonemap(T.gradient_source(), 96, 60, api.TonemapDesc())
    assert r.bytes[..., :3].min() == 0 and r.bytes[..., :3].max() == 255
    assert not r.bytes[np.ix_([45, 46], [75, 76])][..., 0].any()          # the +inf texel's footprint: nan -> 0


@pytest.mark.parametrize("defect", T.DEFECTS)
def test_tonemap_detects(defect):
    caught = []
    for label, src, w, h, desc, before in CASES:
        bad = T.tonemap(src, w, h, desc, before, defect=defect, check_share=False).bytes
        if T.failures(T.tonemap(src, w, h, desc, before), bad):
            caught.append(label)
    print(defect, caught)
    assert caught, "the defect went unnoticed"
