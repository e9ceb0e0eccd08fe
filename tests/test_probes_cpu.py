"""Light-probe baking (lupin_hip_bake_probes), the parts that need no device: the symbol and the layouts of its
mirrors, the basis, irradiance from coefficients, and that the reduction order of tests/probe_ref.py is one a test can see."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import probe_ref, stats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbol_resolves_and_desc_sizes_agree(built):
    lib = _abi.lib()
    assert hasattr(lib, "lupin_hip_bake_probes")
    header = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    body = re.search(r"typedef struct LupinProbeDesc \{(.*?)\} LupinProbeDesc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_size = {"uint32_t": 4, "LupinAdvancedParams": C.sizeof(_abi.AdvancedParamsC)}
    c_fields = re.findall(r"(\w+)\s+(\w+);", body)
    assert [n for _, n in c_fields] == ["pathtrace_type", "max_bounces", "samples", "flags", "max_slots", "advanced"]
    assert [n for _, n in c_fields] == [n for n, _ in _abi.ProbeDescC._fields_]
    want = sum(c_size[t] for t, _ in c_fields)
    assert want == 32 and C.sizeof(_abi.ProbeDescC) == want
    offsets = [getattr(_abi.ProbeDescC, n).offset for n, _ in _abi.ProbeDescC._fields_]
    assert offsets == [0, 4, 8, 12, 16, 20]
    rust = open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    rbody = re.search(r"pub struct LupinProbeDesc \{(.*?)\}", rust, re.S).group(1)
    r_size = {"u32": 4, "LupinAdvancedParams": 12}
    r_fields = re.findall(r"pub (\w+): (\w+)", rbody)
    assert [n for n, _ in r_fields] == [n for _, n in c_fields]
    assert sum(r_size[t] for _, t in r_fields) == want
    assert "pub fn lupin_hip_bake_probes(" in rust
    for name, value in (("LUPIN_PROBE_FLOATS", api.PROBE_FLOATS), ("LUPIN_PROBE_SH_COEFFS", api.PROBE_SH_COEFFS),
                        ("LUPIN_PROBE_RESULT_FLOATS", api.PROBE_RESULT_FLOATS)):
        assert int(re.search(r"#define %s (\d+)" % name, header).group(1)) == value
        assert int(re.search(r"pub const %s: usize = (\d+);" % name, rust).group(1)) == value
    assert (api.PROBE_FLOATS, api.PROBE_SH_COEFFS, api.PROBE_RESULT_FLOATS, api.PROBES_DEVICE_POINTERS) == (4, 9, 36, 1)
    assert "LUPIN_PROBES_DEVICE_POINTERS = 1u" in header and "pub const LUPIN_PROBES_DEVICE_POINTERS: u32 = 1;" in rust
    d0 = api.ProbeDesc()
    assert (int(d0.pathtrace_type), d0.max_bounces, d0.samples, d0.flags, d0.max_slots) == (0, 8, 1024, 0, 0)
    # the header states the literals the restatement uses
    for lit in ("0.28209479f", "0.48860251f", "1.09254843f", "0.31539157f", "0.54627422f"):
        assert lit in header


def gram(SUB):
    d, _, domega = stats.sphere_quadrature(SUB)
    Y = api.sh_basis(d)
    return (Y.T @ Y) * domega


def test_basis_is_orthonormal_and_the_f32_restatement_agrees():
    """stats.sphere_quadrature is a midpoint rule, exact in phi for these trigonometric polynomials and with an error
    c h^2 + O(h^4) in cos(theta) (6e-5 at the default SUB = 6 for the square of index 6).  Two resolutions, SUB and 2 SUB,
    cancel the h^2 term (Richardson: (4 I_2 - I_1) / 3); what is left is below 1e-8, so the 1e-6 judges the basis."""
    G = (4.0 * gram(2 * stats.SUB) - gram(stats.SUB)) / 3.0
    err = np.abs(G - np.eye(9)).max()
    print(f"max |<Y_i, Y_j> - delta_ij| = {err:.3e}")
    assert err <= 1e-6
    d, _, _ = stats.sphere_quadrature()
    d32 = d.astype(np.float32)
    Y32 = probe_ref.sh_basis_f32(d32)
    assert Y32.dtype == np.float32 and Y32.shape == (len(d), 9)
    diff = np.abs(Y32.astype(np.float64) - api.sh_basis(d32.astype(np.float64))).max()
    print(f"max |f32 restatement - float64 basis| = {diff:.3e}")
    assert diff <= 1e-6
    # the order of the indices: y, z, x in band 1
    Y = api.sh_basis(np.eye(3))
    assert np.argmax(np.abs(Y[:, 1:4]), axis=1).tolist() == [2, 0, 1]


def frame_of(n):
    a = np.array([1.0, 0, 0]) if abs(n[0]) < 0.9 else np.array([0, 1.0, 0])
    x = np.cross(a, n)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(n, x), n])


def test_irradiance_from_coefficients_equals_the_cosine_integral():
    """Gauss-Legendre in cos(theta) over the hemisphere about n (the integrand is a cubic there) times a uniform rule in phi
    (a trigonometric polynomial of degree 2): exact up to rounding, so the 1e-6 judges sh_irradiance."""
    rng = np.random.default_rng(11)
    coeffs = rng.normal(size=(6, 9, 4))
    normals = rng.normal(size=(6, 3))
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    normals[0] = (0.0, 1.0, 0.0)
    t, wt = np.polynomial.legendre.leggauss(8)
    c, wc = 0.5 * (t + 1.0), 0.5 * wt                      # cos(theta) in [0, 1]
    phi = (np.arange(16) + 0.5) * (2.0 * math.pi / 16)
    cc, pp = np.meshgrid(c, phi, indexing="ij")
    ss = np.sqrt(1.0 - cc * cc)
    local = np.stack([ss * np.cos(pp), ss * np.sin(pp), cc], -1).reshape(-1, 3)
    weight = (wc[:, None] * np.full(16, 2.0 * math.pi / 16)[None, :]).reshape(-1)
    got = api.sh_irradiance(coeffs, normals)
    assert got.shape == (6, 3)
    for k in range(6):
        world = local @ frame_of(normals[k])
        L = api.sh_basis(world) @ coeffs[k, :, :3]          # (points, 3)
        want = (L * (world @ normals[k])[:, None] * weight[:, None]).sum(axis=0)
        assert np.abs(got[k] - want).max() <= 1e-6, (k, got[k], want)
    # one probe for many normals: leading dimensions broadcast; the w channel is not read
    many = api.sh_irradiance(coeffs[0], normals)
    assert many.shape == (6, 3) and np.array_equal(many[0], got[0])
    assert np.array_equal(api.sh_irradiance(coeffs[..., :3], normals), got)
    # a constant sky of radiance 1: c0 = 2 sqrt(pi), irradiance pi from every side
    sky = np.zeros((9, 3))
    sky[0] = 2.0 * math.sqrt(math.pi)
    assert np.abs(api.sh_irradiance(sky, normals) - math.pi).max() <= 1e-12


def test_the_reduction_order_is_visible():
    rng = np.random.default_rng(12)
    S = 1000
    d = rng.normal(size=(S, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    L = rng.uniform(0.0, 4.0, (S, 3)).astype(np.float32)
    strided = probe_ref.reduce(d, L)
    plain = probe_ref.reduce_ascending(d, L)
    assert strided.shape == plain.shape == (9, 4) and strided.dtype == np.float32
    differing = int((strided.view(np.uint32) != plain.view(np.uint32)).sum())
    print(f"{differing} of 36 words differ between the lane-strided tree and the ascending sum")
    assert differing >= 1
    assert np.abs(strided.astype(np.float64) - plain.astype(np.float64)).max() <= 1e-4       # the same quantity all the same
    exact = (probe_ref.terms(d, L).astype(np.float64).sum(axis=0) * (4.0 * math.pi)) / S
    assert np.abs(strided - exact).max() <= 1e-4
    # below 65 samples lane l holds sample l alone: one sample is its own sum
    one = probe_ref.reduce(d[:1], L[:1])
    t = probe_ref.terms(d[:1], L[:1])[0]
    assert np.array_equal(one.view(np.uint32), ((t * (np.float32(4.0) * np.float32(np.pi))) / np.float32(1)).view(np.uint32))
    assert probe_ref.bake(d, L, 250).shape == (4, 9, 4)
    assert np.array_equal(probe_ref.bake(d, L, 250)[1], probe_ref.reduce(d[250:500], L[250:500]))


def test_without_a_device_the_call_says_so(built):
    probes = np.zeros((1, 4), np.float32)
    out = np.full((1, 9, 4), 7.0, np.float32)
    desc = _abi.ProbeDescC(0, 8, 4, 0, 0, _abi.AdvancedParamsC(100.0, 0, 0.001))
    rc = _abi.lib().lupin_hip_bake_probes(None, None, C.byref(desc), 1, _abi.ptr(probes), _abi.ptr(out), None)
    # LUPIN_ERR_NO_DEVICE; where there is a device, a null context is an invalid argument
    assert rc == (-2 if api.device_count() < 1 else -1)
    assert np.all(out == 7.0)
    from lupinpathtracer_amd import loader
    scene, _ = loader.build_scene_cornell_box(None)
    with pytest.raises(api.LupinError) as e:
        api.bake_probes(None, scene, [[0, 0, 0]], 4)
    assert e.value.code == -2
