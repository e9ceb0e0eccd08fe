"""What directional lightmaps promise that needs no GPU: the pinned order of the resolve, its bound against the
exact sum, plane 0 against the scalar irradiance, the open-sky closed form, the ratio's range and its exact 1, the descriptor's
layout, and that without a device the entry points say so."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import lightmap_directional_ref as D

F = np.float32
U = 2.0 ** -24
ORDER_SEED = 2911
SIGMAS = 5.0
NORMAL_VARIANCE = 1.0 / 18.0      # of d . n over cosine-weighted slots: E[cos^2] - E[cos]^2 = 1/2 - 4/9


def words(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def draw(seed, n, S):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, S, 3))
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    return d.astype(F), rng.uniform(0.0, 3.0, (n, S, 3)).astype(F)


def gamma(m):
    return m * U / (1.0 - m * U)


def exact(d, L):
    """(n, 4, 3) float64: (the exact sum of the float32 factors' products) * the f32 pi / S."""
    t = np.asarray(L, np.float64)[:, :, None, :] * D.basis(d).astype(np.float64)[:, :, :, None]
    return t.sum(axis=1) * float(D.PI) / d.shape[1], np.abs(t).sum(axis=1) * float(D.PI) / d.shape[1]


def test_the_order_is_pinned_a_sequential_twin_gives_other_words():
    assert words(api.SH_K0) == words(D.K0) and words(api.SH_K1) == words(D.K1)      # the restatement's literals are the library's
    d, L = draw(ORDER_SEED, 3, 1000)
    lanes, seq = D.resolve(d, L), D.resolve_sequential(d, L)
    assert lanes.dtype == np.float32 and lanes.shape == (3, 4, 4) and np.all(lanes[..., 3] == 1.0)
    assert (words(lanes[..., :3]) != words(seq[..., :3])).mean() > 0.5, (lanes, seq)
    assert np.array_equal(words(D.resolve(d[:, :1], L[:, :1])), words(D.resolve_sequential(d[:, :1], L[:, :1])))      # one slot: one term


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 129, 1000, 65536])
def test_the_restatement_stays_within_the_derived_bound_of_the_exact_sum(S):
    """Per term: the product's rounding, ceil(S / 64) - 1 lane additions that round (the first adds to +0.0), 6 butterfly additions,
    the scale and the division: m = ceil(S / 64) + 8 roundings, so |error| <= gamma_m * sum |term|."""
    d, L = draw(100 + S, 2, S)
    want, mass = exact(d, L)
    m = math.ceil(S / 64) + 8
    err = np.abs(D.resolve(d, L)[..., :3].astype(np.float64) - want)
    print(S, "largest error", err.max(), "smallest bound", (gamma(m) * mass).min())
    assert (err <= gamma(m) * mass).all()
    # plane 0 over k0 is the scalar lightmap's irradiance pi * mean, the same terms in another order: within the same bound
    irradiance = float(D.PI) * np.asarray(L, np.float64).mean(axis=1)
    got = D.resolve(d, L)[:, 0, :3].astype(np.float64) / float(api.SH_K0)
    print(S, "plane 0 / k0 against pi * mean", np.abs(got - irradiance).max())
    assert (np.abs(got - irradiance) <= gamma(m) * mass[:, 0] / float(api.SH_K0)).all()


def cosine_slots(rng, n, S):
    """Cosine-weighted directions about +y, float64."""
    u1, u2 = rng.uniform(size=(n, S)), rng.uniform(size=(n, S))
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    return np.stack([r * np.cos(phi), np.sqrt(1.0 - u1), r * np.sin(phi)], axis=-1)


def test_the_open_sky_closed_form_by_float64_quadrature():
    """A white sky of radiance L over a lone quad with normal +y: coefficients (k0 pi L, k1 pi L 2/3, 0, 0) in the order
    1, y, z, x, and the normal component of a slot has variance 1 / 18."""
    theta = (np.arange(200000) + 0.5) * (0.5 * np.pi / 200000)
    pdf = 2.0 * np.cos(theta) * np.sin(theta) * (0.5 * np.pi / 200000)         # cosine-weighted, the azimuth integrated out
    mean, second = (np.cos(theta) * pdf).sum(), (np.cos(theta) ** 2 * pdf).sum()
    assert abs(pdf.sum() - 1.0) < 1e-9 and abs(mean - 2.0 / 3.0) < 1e-9 and abs(second - mean * mean - NORMAL_VARIANCE) < 1e-9
    S, Lsky = 65536, 0.75
    d = cosine_slots(np.random.default_rng(5), 4, S)
    coef = D.resolve(d.astype(F), np.full((4, S, 3), Lsky, F))[..., :3].astype(np.float64)
    k0, k1 = float(api.SH_K0), float(api.SH_K1)
    want = np.array([k0 * np.pi * Lsky, k1 * np.pi * Lsky * 2.0 / 3.0, 0.0, 0.0])
    # the constant term has no variance, the tangent components 1 / 4; every coefficient also carries the float32 sum's
    # rounding, at most gamma_m * sum |term| <= gamma_m * k1 pi L with m = ceil(S / 64) + 8
    se = k1 * np.pi * Lsky * np.sqrt(np.array([0.0, NORMAL_VARIANCE, 0.25, 0.25]) / S)
    band = SIGMAS * se + gamma(math.ceil(S / 64) + 8) * k1 * np.pi * Lsky
    assert (np.abs(coef - want[None, :, None]) <= band[None, :, None]).all(), coef[..., 0]
    assert np.abs(coef[:, 2:, :]).max() > 0.0


def test_the_ratio_lies_in_0_to_4_for_non_negative_radiance():
    rng = np.random.default_rng(17)
    n, K = 100000, 6
    nb = rng.normal(size=(n, 3))
    nb /= np.linalg.norm(nb, axis=1, keepdims=True)
    w = rng.normal(size=(n, K, 3))
    w /= np.linalg.norm(w, axis=2, keepdims=True)
    cos = np.einsum("nkc,nc->nk", w, nb)
    w = np.where(cos[..., None] < 0, w - 2.0 * cos[..., None] * nb[:, None, :], w)      # mirrored into n_b's hemisphere
    cos = np.abs(cos)
    L = rng.uniform(0.0, 5.0, (n, K, 3)) * (rng.uniform(size=(n, K, 1)) > 0.3)
    L[:, 0] += 1e-3                                                                   # (some light: den > 0)
    c = np.einsum("nkc,nk,nkj->njc", L, cos, D.basis(w.astype(F)).astype(np.float64)).astype(F)
    ns = rng.normal(size=(n, 3))
    ns /= np.linalg.norm(ns, axis=1, keepdims=True)
    r, bits = D.ratio(c, ns.astype(F), nb.astype(F))
    print("ratio range", r.min(), r.max())
    assert r.dtype == np.float32 and np.all(r >= 0.0) and np.all(r <= 4.0 * (1.0 + 1e-5))
    assert r.max() > 2.0 and (r == 0.0).any() and np.all(bits & D.APPLIED)
    assert np.array_equal(words(api.lightmap_directional_ratio(c, ns.astype(F), nb.astype(F))), words(r))
    # the shading normal on the bake normal: the same operations on the same numbers
    same, _ = D.ratio(c, nb.astype(F), nb.astype(F))
    assert np.all(words(same) == words(F(1.0)))
    assert np.all(words(api.lightmap_directional_ratio(c, nb.astype(F), nb.astype(F))) == words(F(1.0)))


def test_the_ratio_is_one_where_it_is_not_defined():
    c = F([[[1, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]], [[0, 0, 0], [1, 1, 1], [0, 0, 0], [0, 0, 0]], [[np.inf, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
           [[1, 1, 1], [3, 3, 3], [0, 0, 0], [0, 0, 0]]])
    up, down = F([0, 1, 0]), F([0, -1, 0])
    r, bits = D.ratio(c, np.stack([down, up, up, down]), np.stack([up, down, up, up]), back=[False, False, False, True])
    mine = api.lightmap_directional_ratio(c, np.stack([down, up, up, down]), np.stack([up, down, up, up]))
    assert np.array_equal(words(mine[:3]), words(r[:3])) and np.all(mine[3] == 0.0)      # (only the view sees a back face)
    assert np.all(r[0] == 1.0) and bits[0] == D.APPLIED                     # no directional part: n' does not matter
    assert np.all(r[1] == 1.0) and bits[1] == D.DEN_NOT_POSITIVE            # den = -k1 < 0
    assert r[2].tolist() == [1.0, 1.0, 1.0] and bits[2] == (D.NOT_FINITE | D.APPLIED)
    assert np.all(r[3] == 1.0) and bits[3] == D.BACK_FACE
    front, _ = D.ratio(c[3:], down[None], up[None])
    assert np.all(front == 0.0)                                             # num < 0: clamped


def test_desc_layout_and_constants():
    d = _abi.LightmappedDirectionalDescC
    base = C.sizeof(_abi.LightmappedViewDescC)
    assert base == 168 and C.sizeof(d) == base + 16
    assert [(n, getattr(d, n).offset) for n, _ in d._fields_] == [("base", 0), ("bake_flags", base), ("reserved", base + 4)]
    assert (api.LIGHTMAP_DIRECTIONAL_PLANES, api.LIGHTMAPPED_DIRECTIONAL_GBUFFER_FLOATS) == (4, 24)
    assert (api.LIGHTMAPPED_DIRECTIONAL_APPLIED, api.LIGHTMAPPED_DIRECTIONAL_BACK_FACE, api.LIGHTMAPPED_DIRECTIONAL_DEN_NOT_POSITIVE,
            api.LIGHTMAPPED_DIRECTIONAL_NOT_FINITE) == (D.APPLIED, D.BACK_FACE, D.DEN_NOT_POSITIVE, D.NOT_FINITE) == (1, 2, 4, 8)
    assert words(api.SH_K0) == words(D.K0) and words(api.SH_K1) == words(D.K1)
    # the literals are float32 neighbours of sh_basis' float64 constants: within one ulp (2^-25 below 0.5)
    assert abs(float(D.K0) - api.sh_basis([[0, 0, 1]])[0, 0]) <= 2.0 ** -25 and abs(float(D.K1) - api.sh_basis([[0, 0, 1]])[0, 2]) <= 2.0 ** -25
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lupin_hip.h")).read()
    for text in ("#define LUPIN_LIGHTMAP_DIRECTIONAL_PLANES 4", "#define LUPIN_LIGHTMAPPED_DIRECTIONAL_GBUFFER_FLOATS 24",
                 "LUPIN_LIGHTMAPPED_DIRECTIONAL_APPLIED = 1u, LUPIN_LIGHTMAPPED_DIRECTIONAL_BACK_FACE = 2u", "0 <= r <= 4"):
        assert text in header
    rust = open(os.path.join(root, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    assert "pub fn lupin_hip_bake_lightmap_directional(" in rust and "pub fn lupin_hip_render_lightmapped_directional(" in rust
    lib_rs = open(os.path.join(root, "integration", "rust", "lupin_hip", "src", "lib.rs")).read()
    assert "pub fn bake_lightmap_directional(" in lib_rs and "pub fn render_lightmapped_directional(" in lib_rs


def test_entry_points_exist_and_refuse_without_a_device(built):
    lib = _abi.lib()
    assert hasattr(lib, "lupin_hip_bake_lightmap_directional") and hasattr(lib, "lupin_hip_render_lightmapped_directional")
    NO_DEVICE = -2
    from lupinpathtracer_amd import loader
    scene, cams = loader.build_scene_cornell_box(None)
    target = type("T", (), {"format": lambda self: "Rgba16Float", "width": 4, "height": 4, "handle": None})()
    for call in (lambda: api.bake_lightmap_directional(None, scene, [(0, 1.0, 1.0, 0.0, 0.0)], 8, 8),
                 lambda: api.render_lightmapped(None, scene, target, cams[0].params, cams[0].transform, [], np.zeros((8, 8, 4), F),
                                                directional=np.zeros((4, 8, 8, 4), F))):
        with pytest.raises(api.LupinError) as e:
            call()
        assert e.value.code == NO_DEVICE
    if api.device_count() < 1:      # the library itself says so too
        d = _abi.LightmapDescC(8, 8, 0, 8, 4, 0, 0, 0, 0, 1e-3, _abi.AdvancedParamsC(100.0, 0, 0.001))
        ch = _abi.LightmapChartC(0, 1.0, 1.0, 0.0, 0.0)
        out = np.zeros((4, 8, 8, 4), F)
        assert lib.lupin_hip_bake_lightmap_directional(None, None, C.byref(d), C.byref(ch), 1, _abi.ptr(out), None, None) == NO_DEVICE
        dd = _abi.LightmappedDirectionalDescC()
        assert lib.lupin_hip_render_lightmapped_directional(None, None, None, C.byref(dd), None, _abi.ptr(out[0]), _abi.ptr(out), None, None, None,
                                                            None) == NO_DEVICE
