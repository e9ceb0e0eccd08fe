"""Occlusion queries without a GPU: the float64 judgement of tests/occlusion_ref.py on the committed scenes,
the planted twins it must tell apart, the record builders' f32 words, the closed form of the ambient-occlusion test, the
ABI, and that nothing runs without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import closest_hit_ref as X
from tests import occlusion_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_NON_DECISIVE = 0.01        # tests/test_closest_hit_cpu.py holds the reference to the same cap on the same inputs
MIN_JUDGED_HITS = 500
MIN_HITS_PER_INSTANCE = 50     # of the judged hits, as tests/test_closest_hit_cpu.py: every instance of the layout is represented
AO_SAMPLES = 65536
AO_SIGMAS = 5.0


def check_inputs(rep, per_instance=MIN_HITS_PER_INSTANCE):
    """The conditions that keep the judgement from passing by exclusion (tests/test_gpu_occlusion.py asserts them too)."""
    assert rep["left_out_share"] <= MAX_NON_DECISIVE, rep
    assert rep["judged_hits"] >= MIN_JUDGED_HITS and rep["judged_misses"] > 0, rep
    assert len(rep["per_instance"]) == len(X.LAYOUT) and rep["per_instance"].min() >= per_instance, rep["per_instance"]


def oracle_blocked(scene, ori, dir_, eps, tmax):
    """The f32 stand-in for the device: the oracle's closest hit, blocked iff it lies below tmax."""
    from oracle import oracle
    hit, dst, _, _, _ = oracle.trace_rays(scene, ori, dir_, eps)
    return (hit != 0) & (dst < tmax)


@pytest.mark.parametrize("eps", X.EPSILONS)
@pytest.mark.parametrize("kind", ["small", "big"])
def test_judgement_leaves_out_little_and_the_oracle_passes_it(kind, eps):
    c = X.case(kind)
    keep = R.usable(c)
    assert 0.9 * len(keep) < keep.sum() < len(keep)                  # the three families that are not of unit length are gone
    ref = c.refs[eps].take(keep)
    rep = R.report(ref, lambda tmax: oracle_blocked(c.scene, c.ori[keep], c.dir[keep], eps, tmax))
    print(kind, eps, rep)
    check_inputs(rep)
    assert rep["disagree"] == 0, rep
    # the float64 evaluation of the definition agrees with its own judgement
    assert R.report(ref, lambda tmax: R.blocked_f64(c.g, c.ori[keep], c.dir[keep], eps, tmax))["disagree"] == 0


# ---- planted twins: each must trip the judgement ----------------------------------------------------------------

def test_detects_a_judge_that_ignores_ray_epsilon():
    c = X.case("small")
    keep = R.usable(c)
    ref = c.refs[0.25].take(keep)
    rep = R.report(ref, lambda tmax: R.blocked_f64(c.g, c.ori[keep], c.dir[keep], 0.0, tmax))
    print(rep)
    assert rep["disagree"] > 0
    assert rep["disagree_0.5"] > 0          # a surface nearer than ray_epsilon blocks below 0.5 t of the true first hit


def test_detects_a_judge_that_forgets_the_instance_transform():
    c = X.case("small")
    keep = R.usable(c)
    rows = np.zeros_like(c.g.rows)
    rows[:, :, :3] = np.eye(3)
    untransformed = X.Geometry(rows, c.g.mesh_idx, c.g.meshes)
    rep = R.report(c.refs[1e-3].take(keep), lambda tmax: R.blocked_f64(untransformed, c.ori[keep], c.dir[keep], 1e-3, tmax))
    print(rep)
    assert rep["disagree_2.0"] > 100        # the hits are no longer where the scene has them


def test_detects_a_judge_that_compares_t_less_or_equal_tmax():
    """Only a surface AT tmax tells `<` from `<=`: the exact quad (scale 2, integer shift, plane z = 6) from an origin at
    z = 2 straight along +z is hit at t = 4 in f32 as in f64, so tmax = 2 t' for t' = 2 sits on it exactly."""
    c = X.case("small")
    o, d = np.float32([[5.0, -3.5, 2.0]]), np.float32([[0.0, 0.0, 1.0]])   # inside one triangle of the quad, off its diagonal
    h = X.closest_hits(c.g, o, d, 1e-3)
    assert h.hit[0] and h.inst[0] == X.EXACT_QUAD and h.t[0] == 4.0
    t_half = 2.0
    assert not R.blocked_f64(c.g, o, d, 1e-3, 2 * t_half)[0]                         # t < tmax is false at t == tmax
    assert R.blocked_f64(c.g, o, d, 1e-3, 2 * t_half, inclusive=True)[0]             # the twin
    assert R.blocked_f64(c.g, o, d, 1e-3, np.nextafter(np.float32(4.0), np.float32(5.0)))[0]
    from oracle import oracle
    hit, dst, _, inst, _ = oracle.trace_rays(c.scene, o, d, 1e-3)
    assert hit[0] == 1 and inst[0] == X.EXACT_QUAD and dst[0] == np.float32(4.0)     # the f32 traversal reports 4 exactly too


# ---- the record builders ----------------------------------------------------------------------------------------

def test_occlusion_records_hold_the_stated_words():
    rec = api.occlusion_records([[1, 2, 3], [4, 5, 6]], [[0, 0, 1], [0, 1, 0]], tmax=[np.inf, 2.5], rng=[7, 0xFFFFFFFF])
    assert rec.shape == (2, api.OCCLUSION_RECORD_FLOATS) and rec.dtype == np.float32
    assert np.array_equal(rec[:, 0:3], np.float32([[1, 2, 3], [4, 5, 6]])) and np.array_equal(rec[:, 4:7], np.float32([[0, 0, 1], [0, 1, 0]]))
    assert np.array_equal(rec.view(np.uint32)[:, 3], np.uint32([7, 0xFFFFFFFF]))
    assert np.isposinf(rec[0, 7]) and rec[1, 7] == np.float32(2.5)
    assert np.isposinf(api.occlusion_records([[0, 0, 0]], [[1, 0, 0]])[0, 7]) and api.occlusion_records([[0, 0, 0]], [[1, 0, 0]]).view(np.uint32)[0, 3] == 0
    assert (int(api.OcclusionMode.DIRECTION), int(api.OcclusionMode.COSINE_HEMISPHERE)) == (0, 1)


def test_segment_records_are_the_stated_f32_arithmetic_and_short_segments_raise():
    rng = np.random.default_rng(11)
    p, q = rng.uniform(-5, 5, (200, 3)).astype(np.float32), rng.uniform(-5, 5, (200, 3)).astype(np.float32)
    eps = np.float32(1e-3)
    rec = api.segment_records(p, q, 1e-3)
    d = q - p
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert length.dtype == np.float32
    assert np.array_equal(rec[:, 0:3], p) and np.array_equal(rec[:, 4:7].view(np.uint32), (d / length[:, None]).view(np.uint32))
    assert np.array_equal(rec[:, 7].view(np.uint32), (length - eps).view(np.uint32))
    assert R.unit_directions(rec[:, 4:7]).all() and (rec[:, 7] > 0).all()
    for gap in (0.0, 1e-3, 2e-3):           # len <= 2 * ray_epsilon
        with pytest.raises(ValueError):
            api.segment_records([[0, 0, 0], [1, 1, 1]], [[5, 0, 0], [1 + gap, 1, 1]], 1e-3)
    assert len(api.segment_records([[1, 1, 1]], [[1.0021, 1, 1]], 1e-3)) == 1


def test_ao_closed_form_is_told_from_its_uniform_twin_at_the_chosen_sample_count():
    h, radius = 1.0, 2.0
    p, twin = R.ceiling_blocked_fraction(h, radius), R.ceiling_blocked_fraction_uniform_twin(h, radius)
    assert (p, twin) == (0.75, 0.5)
    # a quadrature of the cosine-weighted measure of the cap cos a > h / radius: the closed form is the integral it names
    a = (np.arange(200000) + 0.5) / 200000 * (np.pi / 2)
    w = np.cos(a) * np.sin(a) * 2.0 * (np.pi / 2) / 200000
    assert abs(w.sum() - 1.0) < 1e-9 and abs(w[np.cos(a) > h / radius].sum() - p) < 1e-5
    band = AO_SIGMAS * max(R.binomial_sigma(p, AO_SAMPLES), R.binomial_sigma(twin, AO_SAMPLES))
    assert abs(p - twin) > 10 * band          # no count can pass both
    assert R.ceiling_blocked_fraction(1.0, 0.9) == 0.0


# ---- the ABI and the absence of a fallback ----------------------------------------------------------------------

def test_abi_symbol_struct_and_constants(built):
    handle = C.CDLL(_abi.LIB_PATH)
    assert hasattr(handle, "lupin_hip_occlusion_rays")
    assert "lupin_hip_occlusion_rays" in {n for n, _, _ in _abi.SYMBOLS}
    assert C.sizeof(_abi.OcclusionDescC) == 16 and [f[0] for f in _abi.OcclusionDescC._fields_] == ["mode", "samples", "flags", "ray_epsilon"]
    header = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    assert re.search(r"#define LUPIN_OCCLUSION_RECORD_FLOATS 8\b", header) and api.OCCLUSION_RECORD_FLOATS == 8
    assert re.search(r"LUPIN_OCCLUSION_DIRECTION = 0, LUPIN_OCCLUSION_COSINE_HEMISPHERE = 1", header)
    assert re.search(r"LUPIN_OCCLUSION_DEVICE_POINTERS = 1u", header) and api.OCCLUSION_DEVICE_POINTERS == 1
    body = re.search(r"typedef struct LupinOcclusionDesc \{(.*?)\} LupinOcclusionDesc;", header, re.S).group(1)
    assert re.findall(r"(uint32_t|float)\s+(\w+);", body) == [("uint32_t", "mode"), ("uint32_t", "samples"), ("uint32_t", "flags"), ("float", "ray_epsilon")]
    rust = open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    rbody = re.search(r"pub struct LupinOcclusionDesc \{(.*?)\}", rust, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+)", rbody) == [("mode", "u32"), ("samples", "u32"), ("flags", "u32"), ("ray_epsilon", "f32")]
    assert "pub fn lupin_hip_occlusion_rays(" in rust
    cpp = open(os.path.join(ROOT, "include", "lupin.hpp")).read()
    for name in ("occlusion_rays", "visible", "ambient_occlusion"):
        assert re.search(r"inline [\w:<> ]+ %s\(" % name, cpp), name


def test_without_a_device_every_entry_refuses(built):
    if api.device_count() > 0:
        pytest.skip("a HIP device is present")
    scene = X.case("small").scene       # built on the host: no handle
    rec = api.occlusion_records([[0, 0, 0]], [[0, 0, 1]])
    calls = [lambda: api.occlusion_rays(None, scene, rec), lambda: api.occluded(None, scene, [[0, 0, 0]], [[0, 0, 1]]),
             lambda: api.visible(None, scene, [[0, 0, 0]], [[0, 0, 1]]),
             lambda: api.ambient_occlusion(None, scene, [[0, 0, 0]], [[0, 0, 1]], 1.0)]
    for call in calls:
        with pytest.raises(api.LupinError) as e:
            call()
        assert e.value.code == -2           # LUPIN_ERR_NO_DEVICE
    out = np.full(1, 0xABCDABCD, np.uint32)
    desc = _abi.OcclusionDescC(0, 1, 0, 0.001)
    assert _abi.lib().lupin_hip_occlusion_rays(None, None, C.byref(desc), 1, _abi.ptr(rec), _abi.ptr(out)) == -2
    assert out[0] == 0xABCDABCD
