"""What the bent-normal query promises that needs no GPU: the pinned order of its sum, the bound against the
exact sum, the closed forms the statistical tests lean on, the resolve rule of api.bent_normals, and the descs' layouts."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import bent_normal_ref as B
from tests import transmittance_ref as TR


def words(a):
    return np.asarray(a, np.float32).view(np.uint32)


def draw(seed, S):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(S, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return rng.uniform(0.0, 1.0, S).astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 129, 1000])
def test_the_weights_alone_give_the_transmittance_resolve_word(S):
    T, d = draw(S, S)
    got = B.resolve_f32(T, d)
    assert got.dtype == np.float32 and got.shape == (4,)
    assert words(got[3]) == words(TR.resolve_sum_f32(T))
    # each direction component is summed in the same order: with T = 1 the x sum is the resolve of d.x
    ones = np.ones(S, np.float32)
    assert words(B.resolve_f32(ones, d)[0]) == words(TR.resolve_sum_f32(d[:, 0]))


def test_the_order_is_pinned_a_sequential_twin_gives_other_words():
    T, d = draw(B.ORDER_SEED, 1000)
    lanes, seq = B.resolve_f32(T, d), B.sequential_f32(T, d)
    assert (words(lanes) != words(seq)).all(), (lanes, seq)
    # up to 64 slots every lane holds one term and the twin differs only in the butterfly's order; with one slot they agree
    assert np.array_equal(words(B.resolve_f32(T[:1], d[:1])), words(B.sequential_f32(T[:1], d[:1])))


@pytest.mark.parametrize("S", [1, 65, 1000, 65536])
def test_the_restatement_stays_within_the_derived_bound_of_the_exact_sum(S):
    """sum_bound: m = ceil(S / 64) + 6 roundings per term, gamma_m * sum |term|."""
    T, d = draw(100 + S, S)
    err = np.abs(B.resolve_f32(T, d).astype(np.float64) - B.exact_f64(T, d))
    bound = B.sum_bound(T, d)
    print(S, "error", err, "bound", bound)
    assert (err <= bound).all()
    assert (bound <= (math.ceil(S / 64) + 7) * B.U * S).all()          # and the bound itself is small: the terms are at most 1


def test_closed_forms_by_float64_quadrature():
    mean, second = B.moments(lambda d: np.zeros(d.shape[:-1], bool))
    assert np.allclose(mean, B.OPEN_SKY["mean"], atol=1e-6) and np.allclose(second - mean * mean, B.OPEN_SKY["var"], atol=1e-6)
    assert np.allclose(B.OPEN_SKY["mean"], [0.0, 0.0, 2.0 / 3.0, 1.0]) and np.allclose(B.OPEN_SKY["var"], [0.25, 0.25, 1.0 / 18.0, 0.0])
    mean, second = B.moments(lambda d: d[..., 0] < 0.0)
    assert np.allclose(mean, B.WALL["mean"], atol=1e-6) and np.allclose(second - mean * mean, B.WALL["var"], atol=1e-6)
    assert np.allclose(B.WALL["mean"], [2.0 / (3.0 * math.pi), 0.0, 1.0 / 3.0, 0.5])
    assert np.allclose(B.WALL["var"], [0.125 - 4.0 / (9.0 * math.pi ** 2), 0.125, 5.0 / 36.0, 0.25])
    # the uniform-hemisphere twins, by the same quadrature
    assert np.allclose(B.moments(lambda d: np.zeros(d.shape[:-1], bool), uniform=True)[0], B.OPEN_SKY_UNIFORM, atol=1e-6)
    assert np.allclose(B.moments(lambda d: d[..., 0] < 0.0, uniform=True)[0], B.WALL_UNIFORM, atol=1e-6)
    # ... lie outside the band of the statistical test (65536 slots, 5 standard errors) in at least one component
    for closed, twin in ((B.OPEN_SKY, B.OPEN_SKY_UNIFORM), (B.WALL, B.WALL_UNIFORM)):
        assert (np.abs(twin - closed["mean"]) > B.SIGMAS * B.standard_errors(closed, 65536)).any()


def test_bent_normal_resolve_normalises_and_falls_back_to_the_normal():
    sums = np.float32([[3.0, 0.0, 4.0, 32.0], [0.0, 0.0, 0.0, 0.0], [1e-30, 0.0, 0.0, 1.0], [-0.0, 0.0, 0.0, 0.0], [1.0, 2.0, 2.0, 64.0]])
    normals = np.float32([[0, 0, 1], [0, 1, 0], [0, 0, 1], [1, 0, 0], [0, 0, 1]])
    ao, bent = api.bent_normal_resolve(sums, 64, normals)
    assert ao.dtype == np.float32 and bent.dtype == np.float32 and bent.shape == (5, 3)
    assert ao.tolist() == [0.5, 0.0, 1.0 / 64.0, 0.0, 1.0]
    assert np.array_equal(bent[0], np.float32([3.0, 0.0, 4.0]) / np.float32(5.0))
    assert bent[1].tolist() == [0.0, 1.0, 0.0] and bent[3].tolist() == [1.0, 0.0, 0.0]          # len == 0: the input normal
    # 1e-30 squares to zero in f32: len == 0, the normal again -- the rule looks at len, not at the sums
    assert bent[2].tolist() == [0.0, 0.0, 1.0]
    assert np.array_equal(words(bent[4]), words(np.float32([1.0, 2.0, 2.0]) / np.float32(3.0)))
    assert np.all(np.abs(np.linalg.norm(bent.astype(np.float64), axis=1) - 1.0) <= 1e-6)


def test_desc_layouts():
    b = _abi.BentNormalDescC
    assert C.sizeof(b) == 16
    assert [(n, getattr(b, n).offset) for n, _ in b._fields_] == [("samples", 0), ("flags", 4), ("max_slots", 8), ("ray_epsilon", 12)]
    a = _abi.LightmapAoDescC
    assert C.sizeof(a) == 40
    assert [(n, getattr(a, n).offset) for n, _ in a._fields_] == [("width", 0), ("height", 4), ("samples", 8), ("max_slots", 12), ("flags", 16),
                                                                  ("dilate", 20), ("counter", 24), ("surface_offset", 28), ("max_distance", 32),
                                                                  ("ray_epsilon", 36)]
    assert (api.BENT_NORMAL_RESULT_FLOATS, api.BENT_NORMAL_DEVICE_POINTERS, api.BENT_NORMAL_OPACITY, api.LIGHTMAP_AO_OPACITY) == (4, 1, 2, 2)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lupin_hip.h")).read()
    for text in ("#define LUPIN_BENT_NORMAL_RESULT_FLOATS 4", "LUPIN_BENT_NORMAL_DEVICE_POINTERS = 1u, LUPIN_BENT_NORMAL_OPACITY = 2u",
                 "LUPIN_LIGHTMAP_AO_OPACITY = 2u"):
        assert text in header


def test_entry_points_exist_and_refuse_without_a_device(built):
    lib = _abi.lib()
    assert hasattr(lib, "lupin_hip_bent_normal_rays") and hasattr(lib, "lupin_hip_bake_lightmap_ao")
    NO_DEVICE = -2
    rec = api.occlusion_records([[0, 0, 0]], [[0, 0, 1]], 1.0)
    for call in (lambda: api.bent_normal_rays(None, None, rec, 4),
                 lambda: api.bent_normals(None, None, [[0, 0, 0]], [[0, 0, 1]], 1.0),
                 lambda: api.bake_lightmap_ao(None, None, [(0, 1.0, 1.0, 0.0, 0.0)], 8, 8)):
        with pytest.raises(api.LupinError) as e:
            call()
        assert e.value.code == NO_DEVICE
    if api.device_count() < 1:      # the library itself says so too
        d = _abi.BentNormalDescC(4, 0, 0, 1e-3)
        out = np.zeros((1, 4), np.float32)
        assert lib.lupin_hip_bent_normal_rays(None, None, C.byref(d), 1, _abi.ptr(rec), _abi.ptr(out)) == NO_DEVICE
        a = _abi.LightmapAoDescC(8, 8, 4, 0, 0, 0, 0, 1e-3, 1.0, 1e-3)
        ch = _abi.LightmapChartC(0, 1.0, 1.0, 0.0, 0.0)
        assert lib.lupin_hip_bake_lightmap_ao(None, None, C.byref(a), C.byref(ch), 1, _abi.ptr(np.zeros((8, 8, 4), np.float32)), None, None, None) == NO_DEVICE
