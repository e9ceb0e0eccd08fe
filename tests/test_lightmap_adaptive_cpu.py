"""Adaptive lightmap baking without a device: the numpy float32 restatement (tests/lightmap_adaptive_ref.py)
against float64 moments, the sum-of-squares twin that must not pass, the mask by hand, the compaction, the round words, the
struct layouts in the header, ctypes and the Rust shim, the exported symbols, and the refusal without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import lightmap_adaptive_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24


def m2_bound(lum):
    """What float32 can cost the restatement's M2 against float64, relative, from the inputs alone.  Every mean the restatement
    forms (a round's, a merged one) is off by at most eps = 4 u max|l|; moments about a point eps away from the mean differ by
    at most 2 eps sum|l - ml| + N eps^2 (the merge's delta^2 term is the same shift between two rounds' means).  On top of
    that the sums are of non-negative terms with under 64 roundings each: 3 per term, ceil(S / 64) + 6 in a wave, 5 per merge."""
    n = lum.shape[0]
    l64 = A.luminance(grey(lum)).astype(np.float64).reshape(n, -1)
    ml, m2 = float64_moments(lum)
    eps = 4.0 * U * np.abs(l64).max(axis=1)
    with np.errstate(all="ignore"):
        shift = np.where(m2 > 0, (2.0 * eps * np.abs(l64 - ml[:, None]).sum(axis=1) + l64.shape[1] * eps * eps) / m2, 0.0)
    return float((shift + 64.0 * U).max())


def grey(lum):
    lum = np.asarray(lum, F)
    return np.stack([lum, lum, lum], axis=-1)


def inputs():
    """name -> (n, R, S) float32 luminances: constants, exponentials, a 1-in-50 spike, a constant plus tiny noise."""
    rng = np.random.default_rng(20240611)
    n, R = 5, 6
    out = {}
    out["constants"] = np.broadcast_to(np.array([0.0, 0.5, 1.0, 3.0, 100.0], F)[:, None, None], (n, R, 16)).copy()
    for S in (16, 70, 129):
        out[f"exponentials S={S}"] = (-np.log(1.0 - rng.random((n, R, S)))).astype(F)
        out[f"spike S={S}"] = np.where(rng.integers(0, 50, (n, R, S)) == 0, 100.0, 0.1).astype(F)
        out[f"constant plus tiny noise S={S}"] = (1.0 + 1e-4 * (rng.random((n, R, S)) - 0.5)).astype(F)
    return out


def restated(lum, resolve):
    n, R, S = lum.shape
    st = A.State(n)
    for r in range(R):
        A.merge(st, np.arange(n), resolve(grey(lum[:, r])), S)
    return st


def float64_moments(lum):
    n = lum.shape[0]
    l64 = A.luminance(grey(lum)).astype(np.float64).reshape(n, -1)        # the f32 luminances the restatement sees, in float64
    ml = l64.mean(axis=1)
    return ml, ((l64 - ml[:, None]) ** 2).sum(axis=1)


def deviations(lum, resolve):
    st = restated(lum, resolve)
    ml, m2 = float64_moments(lum)
    assert np.all(st.n == lum.shape[1] * lum.shape[2]) and np.all(st.rounds == lum.shape[1])
    with np.errstate(all="ignore"):
        dev_ml = np.where(ml > 0, np.abs(st.ml.astype(np.float64) - ml) / ml, np.abs(st.ml))
        dev_m2 = np.where(m2 > 0, np.abs(st.m2.astype(np.float64) - m2) / m2, np.abs(st.m2))
    return float(dev_ml.max()), float(dev_m2.max())


def test_the_restatement_agrees_with_float64_and_the_sum_of_squares_twin_does_not():
    data = inputs()
    own = {name: deviations(lum, A.resolve) for name, lum in data.items()}
    worst = max(max(d) for d in own.values())
    tolerance = 4.0 * worst
    print("largest relative deviation of the restatement from float64:", worst, "tolerance:", tolerance)
    for name, d in own.items():
        print(f"  {name}: ml {d[0]:.3e}, M2 {d[1]:.3e}")
    assert own["constants"] == (0.0, 0.0)          # equal samples: the mean is the sample and M2 is exactly zero
    assert worst > 0.0
    for name, d in own.items():
        assert d[0] <= 8.0 * U and d[1] <= m2_bound(data[name]), (name, d, m2_bound(data[name]))
        assert max(d) <= tolerance, name
    for S in (16, 70, 129):
        name = f"constant plus tiny noise S={S}"
        twin = deviations(data[name], A.resolve_sum_of_squares)
        print(f"  twin, {name}: ml {twin[0]:.3e}, M2 {twin[1]:.3e}")
        assert twin[1] > tolerance and twin[1] > 100.0 * own[name][1], (name, twin)


def test_one_round_of_the_merge_is_the_resolve_and_the_means_merge_exactly_on_dyadic_values():
    lum = np.array([[[0.5] * 16, [1.5] * 16, [0.25] * 16]], F)                 # n = 1, R = 3: round means 0.5, 1.5, 0.25
    st = A.State(1)
    A.merge(st, [0], A.resolve(grey(lum[:, 0])), 16)
    first = A.resolve(grey(lum[:, 0]))
    assert st.ml[0] == first[0, 4] and st.m2[0] == first[0, 5] == 0.0 and np.all(st.mean[0] == first[0, :3])
    assert A.pixel_error(st.n, st.ml, st.m2)[0] == 0.0 and A.pixel_error([1], [1.0], [0.0])[0] == np.inf
    A.merge(st, [0], A.resolve(grey(lum[:, 1])), 16)
    assert st.ml[0] == F(1.0) and st.m2[0] == F(8.0)                           # 32 samples, half at 0.5 and half at 1.5
    A.merge(st, [0], A.resolve(grey(lum[:, 2])), 16)
    ml, m2 = float64_moments(lum)
    assert st.n[0] == 48 and st.rounds[0] == 3
    assert abs(float(st.ml[0]) - ml[0]) <= 2e-7 * ml[0] and abs(float(st.m2[0]) - m2[0]) <= 1e-6 * m2[0]


def test_a_five_by_five_mask_by_hand():
    W = H = 5
    owned = np.ones((H, W), bool)
    owned[2, 2] = False                                   # a hole in the chart
    owned[0, 4] = False
    texel_of = np.flatnonzero(owned.reshape(-1))
    index = {int(t): i for i, t in enumerate(texel_of)}
    max_rounds = 4
    rounds = np.full(len(texel_of), 2, np.uint32)
    want = np.zeros((H, W), bool)
    want[0, 0] = True                                     # a corner that wants samples
    want[4, 2] = True                                     # an edge texel that wants samples
    rounds[index[3 * W + 4]] = max_rounds                 # a capped texel: by the rule its want is 0
    rounds[index[4 * W + 1]] = max_rounds                 # a capped texel beside the edge texel that wants
    active = A.mask(want, texel_of, rounds, max_rounds)
    got = np.zeros((H, W), int)
    got.reshape(-1)[texel_of] = active
    by_hand = np.array([[1, 1, 0, 0, 0],
                        [1, 1, 0, 0, 0],
                        [0, 0, 0, 0, 0],                  # (2, 2) is not owned: never active, and it wants nothing
                        [0, 1, 1, 1, 0],                  # (3, 4): capped, and no neighbour of it wants anyway
                        [0, 0, 1, 1, 0]])                 # (4, 1): beside a wanting texel, but capped
    assert np.array_equal(got, by_hand)
    # a capped neighbour keeps nobody alive: with (4, 2) capped instead, its want is 0 by the rule and the row below goes quiet
    want[4, 2] = False
    rounds[index[4 * W + 2]] = max_rounds
    got.reshape(-1)[texel_of] = A.mask(want, texel_of, rounds, max_rounds)
    assert got[3:].sum() == 0 and got[:2, :2].sum() == 4


def test_compaction_is_stable():
    rng = np.random.default_rng(3)
    for n in (1, 255, 256, 257, 1000):
        for p in (0.0, 0.3, 1.0):
            active = rng.random(n) < p
            assert np.array_equal(A.compact(active), np.flatnonzero(active))


def test_round_words():
    words = np.array([0, 1, 0xFFFFFFFF, 0x9E3779B9, 0x85EBCA6B, 123456789], np.uint32)
    words = np.concatenate([words, api.rng_seed_for(np.arange(64, dtype=np.uint32), 7)])
    assert np.array_equal(A.round_word(words, 0), words)
    assert np.array_equal(api.lightmap_round_word(words, 0), words)
    assert A.ROUND_STRIDE == api.LIGHTMAP_ADAPTIVE_ROUND_STRIDE != A.SAMPLE_STRIDE
    s = np.arange(4096, dtype=np.uint32)
    for w in words:
        slots = set(api.ray_sample_seed(np.full(4096, w, np.uint32), s).tolist())
        for r in (1, 2, 3, 11, 4095):
            wr = int(A.round_word(np.array([w], np.uint32), r)[0])
            assert wr == int(api.lightmap_round_word(w, r))
            assert wr not in slots, (int(w), r)
    rec = api.ray_records(np.zeros((3, 3)), [(0, 1, 0)] * 3, words[:3], api.RayMode.COSINE_HEMISPHERE)
    rr = A.round_records(rec, [2, 0], 5)
    assert np.array_equal(rr.view(np.uint32)[:, 3], A.round_word(words[[2, 0]], 5))
    assert np.array_equal(np.delete(rr.view(np.uint32), 3, axis=1), np.delete(rec.view(np.uint32)[[2, 0]], 3, axis=1))


C_SIZES = {"float": 4, "uint32_t": 4, "uint64_t": 8}
RUST = {"float": "f32", "uint32_t": "u32", "uint64_t": "u64"}


def header_struct(name):
    text = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s+(\w+);", body)


@pytest.mark.parametrize("name,ctype,size", [("LupinLightmapAdaptiveDesc", _abi.LightmapAdaptiveDescC, 16),
                                             ("LupinLightmapAdaptiveStats", _abi.LightmapAdaptiveStatsC, 64)])
def test_struct_layouts_match_in_the_header_ctypes_and_the_rust_shim(name, ctype, size):
    fields = header_struct(name)
    offset = 0
    for (ty, field), (cname, _) in zip(fields, ctype._fields_):
        offset = (offset + C_SIZES[ty] - 1) // C_SIZES[ty] * C_SIZES[ty]
        assert field == cname and getattr(ctype, cname).offset == offset and getattr(ctype, cname).size == C_SIZES[ty], (name, field)
        offset += C_SIZES[ty]
    align = max(C_SIZES[ty] for ty, _ in fields)
    assert len(fields) == len(ctype._fields_) and C.sizeof(ctype) == size == (offset + align - 1) // align * align
    rust = open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    body = re.search(r"pub struct %s \{(.*?)\}" % name, rust, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+)", body) == [(field, RUST[ty]) for ty, field in fields]


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    for macro, value in (("LUPIN_RAY_MOMENTS_FLOATS", api.RAY_MOMENTS_FLOATS), ("LUPIN_LIGHTMAP_ADAPTIVE_MAX_ROUNDS", api.LIGHTMAP_ADAPTIVE_MAX_ROUNDS),
                         ("LUPIN_LIGHTMAP_ADAPTIVE_STATS_FLOATS", api.LIGHTMAP_ADAPTIVE_STATS_FLOATS)):
        assert int(re.search(r"#define %s (\d+)" % macro, text).group(1)) == value
    assert A.MOMENTS_FLOATS == api.RAY_MOMENTS_FLOATS
    assert "0x85EBCA6B" in text and A.ROUND_STRIDE == 0x85EBCA6B


def test_both_symbols_are_exported(built):
    handle = C.CDLL(_abi.LIB_PATH)
    bound = {n for n, _, _ in _abi.SYMBOLS}
    for symbol in ("lupin_hip_pathtrace_rays_moments", "lupin_hip_bake_lightmap_adaptive", "lupin_hip_lightmap_adaptive_stats"):
        assert hasattr(handle, symbol) and symbol in bound


def test_without_a_device_both_calls_say_so(built):
    if api.device_count() > 0:
        pytest.skip("a HIP device is present")
    lib = _abi.lib()
    q = _abi.RayQueryDescC(0, 8, 4, 0, 0, _abi.AdvancedParamsC(100.0, 0, 0.001))
    rec = api.ray_records(np.zeros((2, 3)), [(0, 1, 0)] * 2)
    out = np.full((2, 8), -7.0, F)
    assert lib.lupin_hip_pathtrace_rays_moments(None, None, C.byref(q), 2, _abi.ptr(rec), _abi.ptr(out)) == -2
    d = _abi.LightmapDescC(4, 4, 0, 8, 4, 0, 0, 0, 0, 1e-3, _abi.AdvancedParamsC(100.0, 0, 0.001))
    a = _abi.LightmapAdaptiveDescC(0.05, 2, 8, 0)
    cc = _abi.LightmapChartC(0, 1.0, 1.0, 0.0, 0.0)
    rgba, stats = np.full((4, 4, 4), -7.0, F), np.full((4, 4, 4), -7.0, F)
    assert lib.lupin_hip_bake_lightmap_adaptive(None, None, C.byref(d), C.byref(a), C.byref(cc), 1, _abi.ptr(rgba), _abi.ptr(stats), None, None) == -2
    assert np.all(out == -7.0) and np.all(rgba == -7.0) and np.all(stats == -7.0)
    scene = type("S", (), {"handle": None})()
    for call in (lambda: api.pathtrace_rays_moments(None, scene, rec), lambda: api.bake_lightmap_adaptive(None, scene, [api.LightmapChart(0)], 4, 4)):
        with pytest.raises(api.LupinError) as e:
            call()
        assert e.value.code == -2
