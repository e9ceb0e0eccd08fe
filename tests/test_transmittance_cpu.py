"""Transmittance queries without a GPU: the fit of K_LEAF, the cap on what the float64 judgement of
tests/transmittance_ref.py leaves out, closed forms of the reference, the planted twins it must tell apart, the numpy f32
restatement of the resolve order, the ABI, and that nothing runs without a device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import closest_hit_ref as X
from tests import transmittance_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
O_QUAD, D_QUAD = np.float32([[5.0, -3.5, 2.0]]), np.float32([[0.0, 0.0, 1.0]])   # meets a stack's first quad at t = 4 exactly


def settings(c):
    for eps in X.EPSILONS:
        for setting in TR.TMAX_SETTINGS:
            yield eps, setting, TR.tmax_for(c.P, eps, setting).astype(np.float64)


def test_k_leaf_is_four_times_the_worst_measured_leaf_error_rounded_up():
    worst = 0.0
    for kind in ("small", "big"):
        c = TR.case(kind)
        for eps, setting, tmax in settings(c):
            worst = max(worst, TR.leaf_fit(TR.leaf_alpha_lists(c.P, c.op, eps, tmax)))
    # and a synthetic set that reaches further than the scenes do: long products of opacities of every size
    rng = np.random.default_rng(3)
    worst = max(worst, TR.leaf_fit([rng.uniform(0.0, 1.0, n).astype(np.float32) ** rng.choice([0.25, 1.0, 4.0]) for n in range(1, 40) for _ in range(50)]))
    print("worst leaf error in units of 2^-24 (n + 1):", worst)
    assert 0.0 < worst and TR.K_LEAF == math.ceil(4.0 * worst)


@pytest.mark.parametrize("kind", ["small", "big"])
def test_the_judgement_leaves_out_at_most_one_percent(kind):
    c = TR.case(kind)
    print(kind, "rays", len(c.ori), "raw undecided share of the 1.25x draw", c.raw_undecided)
    assert len(c.ori) == sum(TR.target_counts(kind).values())
    for eps, setting, tmax in settings(c):
        exp = TR.expected(c.P, c.op, eps, tmax)
        shares = TR.left_out_shares(c, exp)
        print(kind, eps, setting, shares, "crossings up to", int(exp.n.max()))
        assert max(shares.values()) <= TR.MAX_LEFT_OUT, (eps, setting, shares)
        assert TR.disagreements(exp, exp.T) == 0                       # the judgement accepts its own expectation
        if setting != "half":
            dec = exp.decisive
            assert ((exp.T > 0) & (exp.T < 1) & dec).sum() > len(dec) // 5 and ((exp.T == 0) & dec).sum() > len(dec) // 20 and (exp.n[dec] > 1).sum() > len(dec) // 5
    # every source of alpha and every opaque instance is crossed by judged rays
    certain, _ = TR.classify(c.P, 1e-3, np.full(c.P.n_rays, np.inf))
    per_instance = np.bincount(c.P.inst[certain], minlength=len(X.LAYOUT))
    print(kind, "certain crossings per instance", per_instance)
    assert per_instance.min() >= 20
    assert sorted(np.nonzero(~TR.alpha_capable(c.sc))[0]) == list(TR.OPAQUE_INSTANCES)


# ---- closed forms of the reference ------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_parallel_quads_of_alpha_one_half(k):
    sc, textures, scene = TR.stacked_quads([0.5] * k)
    exp = TR.reference_T(sc, textures, scene, O_QUAD, D_QUAD, 1e-3, np.inf)
    assert exp.decisive[0] and exp.n[0] == k and abs(exp.T[0] - 2.0 ** -k) <= 1e-15
    assert float(TR.leaf_product_f32([0.5] * k)) == 2.0 ** -k


def test_vertex_alpha_gradient():
    alphas = [0.0, 0.25, 0.5, 0.75]
    sc, textures, scene = TR.stacked_quads([1.0], vertex_alpha=alphas)
    rng = np.random.default_rng(4)
    xy = rng.uniform(-0.9, 0.9, (32, 2))                                   # local quad coordinates
    o = np.concatenate([4.0 + 2.0 * xy[:, :1], -2.0 + 2.0 * xy[:, 1:], np.full((32, 1), 2.0)], 1).astype(np.float32)
    exp = TR.reference_T(sc, textures, scene, o, np.repeat(D_QUAD, 32, 0), 1e-3, np.inf)
    x, y = (o[:, 0].astype(np.float64) - 4.0) / 2.0, (o[:, 1].astype(np.float64) + 2.0) / 2.0
    # the quad's triangles (0, 1, 2) and (0, 2, 3) over vertices (-1,-1) (1,-1) (1,1) (-1,1): barycentric interpolation
    lower = x > y
    a = np.where(lower, alphas[0] + (x + 1) / 2 * (alphas[1] - alphas[0]) + (y + 1) / 2 * (alphas[2] - alphas[1]),
                 alphas[0] + (x + 1) / 2 * (alphas[2] - alphas[3]) + (y + 1) / 2 * (alphas[3] - alphas[0]))
    assert exp.decisive.sum() >= 28
    assert np.all(np.abs(exp.T - (1.0 - a))[exp.decisive] <= 1e-12)


# ---- planted twins: each must fail the judgement ----------------------------------------------------------------

def twin_disagreements(c, eps, tmax, **variant):
    exp = TR.expected(c.P, c.op, eps, tmax)
    return TR.disagreements(exp, TR.expected(c.P, c.op, eps, tmax, **variant).T)


def test_detects_a_judge_that_ignores_the_flag_clear_rule():
    c = TR.case("small")
    bad = twin_disagreements(c, 1e-3, np.full(c.P.n_rays, np.inf), ignore_flag=True)
    print(bad)
    assert bad > 100


def test_detects_a_judge_that_compares_t_less_or_equal_tmax():
    """Only a surface AT tmax tells `<` from `<=`: the exact quad at t = 4 = tmax."""
    sc, textures, scene = TR.stacked_quads([0.5, 0.5])
    P = TR.pairs(X.geometry(scene), O_QUAD, D_QUAD)
    op = TR.Opacity(sc, textures, scene)
    assert P.t.tolist() == [4.0, 5.0] or sorted(P.t.tolist()) == [4.0, 5.0]
    # in exact arithmetic (no band: the quad is exact in f32 as in f64)
    exact = lambda tmax, **kw: TR.expected(P, op, 1e-3, np.array([tmax]), **kw)
    strict = TR.classify(P, 1e-3, np.array([4.0]), s=0.0)
    assert not (strict[0] & (P.t == 4.0)).any()                       # t < tmax is false at t == tmax
    incl = TR.classify(P, 1e-3, np.array([4.0]), s=0.0, inclusive=True)
    assert (incl[0] & (P.t == 4.0)).any()                             # the twin counts it
    assert exact(4.5).T[0] == 0.5 and exact(5.5).T[0] == 0.25 and exact(3.5).T[0] == 1.0


def test_detects_a_judge_that_forgets_ray_epsilon():
    c = TR.case("small")
    tmax = TR.tmax_for(c.P, 0.25, "unbounded").astype(np.float64)
    bad = twin_disagreements(c, 0.25, tmax, ignore_eps=True)
    print(bad)
    assert bad > 0


def test_detects_a_judge_that_sums_opacities():
    c = TR.case("small")
    bad = twin_disagreements(c, 1e-3, np.full(c.P.n_rays, np.inf), summed=True)
    print(bad)
    assert bad > 100


# ---- the resolve order ------------------------------------------------------------------------------------------

def test_resolve_order_restated_in_f32():
    rng = np.random.default_rng(9)
    assert TR.resolve_sum_f32(np.float32([0.375])) == np.float32(0.375)
    assert TR.resolve_sum_f32(np.ones(1000, np.float32)) == np.float32(1000.0)
    for S in (2, 63, 64, 65, 129, 1000):
        T = (rng.uniform(0, 1, S) ** 3).astype(np.float32)
        # written out lane by lane
        p = [np.float32(0.0)] * 64
        for s in range(S):
            p[s % 64] = np.float32(p[s % 64] + T[s])
        for off in (32, 16, 8, 4, 2, 1):
            p = [np.float32(p[l] + p[l ^ off]) for l in range(64)]
        got = TR.resolve_sum_f32(T)
        assert got.dtype == np.float32 and got == p[0] and len({float(x) for x in p}) == 1
        assert abs(float(got) - float(T.astype(np.float64).sum())) <= S * 2.0 ** -24 * float(T.sum())
    # the order matters: a plain left-to-right f32 sum differs somewhere
    T = (rng.uniform(0, 1, 1000) ** 3).astype(np.float32)
    serial = np.float32(0.0)
    for x in T:
        serial = np.float32(serial + x)
    assert serial != TR.resolve_sum_f32(T)


# ---- the ABI, the mirrors and the absence of a fallback ---------------------------------------------------------

def test_abi_symbol_and_mirrors(built):
    handle = C.CDLL(_abi.LIB_PATH)
    assert hasattr(handle, "lupin_hip_transmittance_rays")
    sig = {n: (r, a) for n, r, a in _abi.SYMBOLS}
    assert sig["lupin_hip_transmittance_rays"] == sig["lupin_hip_occlusion_rays"]
    header = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    assert re.search(r"int lupin_hip_transmittance_rays\(LupinContext \*ctx, const LupinScene \*scene, const LupinOcclusionDesc \*desc,\s*"
                     r"uint64_t n, const float \*records /\* n x 8 \*/, float \*out_sum /\* n \*/\);", header)
    rust = open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    assert "pub fn lupin_hip_transmittance_rays(" in rust
    assert "pub fn transmittance_rays(" in open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "lib.rs")).read()
    cpp = open(os.path.join(ROOT, "include", "lupin.hpp")).read()
    for name in ("transmittance_rays", "transmittance"):
        assert re.search(r"inline [\w:<> ]+ %s\(" % name, cpp), name


def test_without_a_device_every_entry_refuses(built):
    if api.device_count() > 0:
        pytest.skip("a HIP device is present")
    scene = TR.case("small").scene       # built on the host: no handle
    rec = api.occlusion_records([[0, 0, 0]], [[0, 0, 1]])
    calls = [lambda: api.transmittance_rays(None, scene, rec), lambda: api.transmittance(None, scene, [[0, 0, 0]], [[0, 0, 1]]),
             lambda: api.ambient_occlusion(None, scene, [[0, 0, 0]], [[0, 0, 1]], 1.0, opacity=True)]
    for call in calls:
        with pytest.raises(api.LupinError) as e:
            call()
        assert e.value.code == -2           # LUPIN_ERR_NO_DEVICE
    out = np.full(1, 0xABCDABCD, np.uint32)
    desc = _abi.OcclusionDescC(0, 1, 0, 0.001)
    assert _abi.lib().lupin_hip_transmittance_rays(None, None, C.byref(desc), 1, _abi.ptr(rec), _abi.ptr(out)) == -2
    assert out[0] == 0xABCDABCD


def test_ambient_occlusion_default_path_makes_the_same_calls(monkeypatch):
    """opacity=False (the default) goes through occlusion_rays with the records it always built; opacity=True sends the same
    records to transmittance_rays and divides the sum."""
    calls = []

    def fake_occlusion(ctx, scene, rec, mode, samples, eps):
        calls.append(("occlusion", rec.copy(), int(mode), samples, eps))
        return np.uint32([16, 0])

    def fake_transmittance(ctx, scene, rec, mode, samples, eps):
        calls.append(("transmittance", rec.copy(), int(mode), samples, eps))
        return np.float32([48.0, 64.0])

    monkeypatch.setattr(api, "occlusion_rays", fake_occlusion)
    monkeypatch.setattr(api, "transmittance_rays", fake_transmittance)

    class FakeScene:
        handle = 1
    pts, nrm = np.float32([[0, 0, 0], [1, 2, 3]]), np.float32([[0, 1, 0], [0, 0, 1]])
    a = api.ambient_occlusion(object(), FakeScene(), pts, nrm, 2.0, surface_offset=0.5)
    b = api.ambient_occlusion(object(), FakeScene(), pts, nrm, 2.0, surface_offset=0.5, opacity=False)
    t = api.ambient_occlusion(object(), FakeScene(), pts, nrm, 2.0, surface_offset=0.5, opacity=True)
    assert [c[0] for c in calls] == ["occlusion", "occlusion", "transmittance"]
    want = api.occlusion_records(pts + nrm * np.float32(0.5), nrm, 2.0, api.rng_seed_for(np.arange(2, dtype=np.uint32), 0))
    for c in calls:
        assert np.array_equal(c[1].view(np.uint32), want.view(np.uint32)) and c[2:] == (1, 64, 0.001)
    assert a.tolist() == b.tolist() == [0.75, 1.0] and a.dtype == np.float32
    assert t.tolist() == [0.75, 1.0] and t.dtype == np.float32
