"""The baked-lighting view's contract (include/lupin_hip.h) on the CPU: tests/baked_view_ref.py composed over the
oracle's camera, closest-hit and surface restatements on the Cornell box (with a sky, so that a miss shows something), with
synthetic coefficients and the lookups of tests/probe_grid_ref.py and tests/probe_depth_ref.py.  Every check is a function
of an optional planted misreading; the contract passes them all and every plant fails at least one."""
from types import SimpleNamespace

import numpy as np
import pytest

from lupinpathtracer_amd import api, loader
from oracle import oracle
from tests import baked_view_ref as B
from tests import film_ref
from tests import probe_depth_ref as D
from tests import probe_grid_ref as G

F = np.float32
SKY = (0.3, 0.5, 0.9)
AMBIENT = F([0.11, 0.07, 0.05])
GRID = (F([-0.9, 0.1, -0.9]), F([0.6, 0.6, 0.9]), (4, 4, 3))          # probes inside the box
P = 48
EPS = 1e-3
U = 2.0 ** -24                                                         # half an ulp of float32, relative
_cache = {}


def words(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def scene():
    """The Cornell box under a sky of constant radiance, host side only."""
    if "scene" not in _cache:
        cpu, cams = loader.cornell_box_scene_cpu()
        env = api.default_environment()
        env["emission"] = F(SKY)
        cpu.environments = np.array([env], api.ENVIRONMENT_DTYPE)
        api.validate_scene(cpu, 0, 0)
        _cache["scene"] = api.build_accel_structures_and_upload(None, cpu, [], [api.EnvMapInfo(np.ones((1, 1, 4), F), 1, 1)], True), cams[0]
    return _cache["scene"]


def views():
    """(name, W, H, transform): the scene's camera, which sees the box's faces from the side their normals point away from
    (and sky in the top row); the same pulled back (the box amid sky); from the other side, turned round (the faces whose
    normals point at the camera, amid sky)."""
    cam = scene()[1]
    back = np.array(cam.transform, F).copy()
    back[3] = [0.0, 1.0, -7.0]
    behind = F([[-1, 0, 0], [0, 1, 0], [0, 0, -1], [0, 1, 7.0]])
    return (("inside", 24, 24, cam.transform), ("far", 17, 11, back), ("behind", 12, 13, behind))


def pieces(name):
    if ("px", name) not in _cache:
        sc, cam = scene()
        _, W, H, xf = next(v for v in views() if v[0] == name)
        _cache["px", name] = B.pieces(oracle.camera_probe, lambda o, d, e: oracle.trace_rays(sc, o, d, e), lambda r: oracle.surface_probe(sc, r),
                                      W, H, cam.params, xf, EPS)
    return _cache["px", name]


def coefficients(seed=5):
    return np.random.default_rng(seed).normal(size=(P, 9, 4)).astype(F)


def plain(sh, valid=None, backface=True):
    return lambda rec: G.sample(*GRID, sh, rec, valid=valid, backface=backface, blocked=None)


def dense_maps(R=6):
    rng = np.random.default_rng(9)
    maxd = api.probe_grid_depth_max_distance(GRID[1])
    maps = np.empty((P, R + 2, R + 2, 2), F)
    maps[..., 0] = rng.uniform(0.05, 0.6, maps.shape[:-1]) * maxd
    maps[..., 1] = maps[..., 0] * maps[..., 0] + rng.uniform(0.0, 0.05 * maxd * maxd, maps.shape[:-1])
    return maps, maxd


def by_maps(sh, valid=None, backface=True):
    maps, maxd = dense_maps()
    return lambda rec: D.sample(*GRID, sh, maps, rec, maxd, valid=valid, backface=backface)


# ---- the checks: each takes a planted misreading and raises where the result is not the contract's ------------------

def check_every_view_has_what_it_is_for(plant=None):
    inside, far, behind = pieces("inside"), pieces("far"), pieces("behind")
    assert inside.hit.sum() >= 550 and 10 < far.hit.sum() < far.hit.size - 10 and 10 < behind.hit.sum() < behind.hit.size - 10
    assert (inside.emission[inside.hit].max(axis=1) > 0).sum() >= 2                        # the lamp is in view
    facing = lambda px: (px.d * px.ns).sum(axis=1)[px.hit]
    assert (facing(inside) > 0).all() and (facing(behind) < 0).all()          # the normal is turned round in one, kept in the other


def check_band_zero_gives_the_closed_form(plant=None):
    """Band 0 only, the same coefficient c > 0 at every probe: every corner's irradiance is e = fl(fl(A0 * Y0) * c), and the
    pixel is emission + color * E0 / pi with E0 = pi * Y0 * c.  Bound, in units of u = 2^-24 relative (all terms are
    positive, so every rounding is relative to a partial result no larger than the final one):
      e against E0: the literals A0 and Y0 (u each), their product (u), the product with c (u)                     4 u
      the lookup: at most 8 products t * e (u each, into a sum of positives: u of the sum), 7 additions of the
        numerator (7 u), 7 of the denominator (7 u), the division (u)                                              16 u
      step 6: color * E (u), * 0.31830988f (u) whose literal is within u of 1 / pi (u), + emission (u)              4 u
    24 u to first order; the second-order terms are below 24^2 u^2 < u.  The check asks for 25 u = 1.5e-6."""
    c = F([0.8, 1.7, 0.35])
    sh = np.zeros((P, 9, 4), F)
    sh[:, 0, :3] = c
    Y0 = 0.28209479177387814
    for name in ("inside", "far", "behind"):
        px = pieces(name)
        for lookup in (plain(sh, backface=False), plain(sh), by_maps(sh)):
            rgb, g = B.compose(px, lookup, AMBIENT, plant)
            h = px.hit & (g[:, 11] > 0)
            assert h.sum() > 10
            want = px.emission[h].astype(np.float64) + px.color[h].astype(np.float64) * (Y0 * c.astype(np.float64))
            assert np.all(np.abs(rgb[h] - want) <= 25 * U * want), (name, np.abs(rgb[h] - want).max())


def check_a_miss_is_the_environment(plant=None):
    px = pieces("far")
    rgb, g = B.compose(px, plain(coefficients()), AMBIENT, plant)
    m = ~px.hit
    assert np.array_equal(words(rgb[m]), words(px.env[m])) and np.all(px.env[m] == F(SKY))
    assert np.all(words(g)[m, 3] == 0xFFFFFFFF) and np.all(g[m, 11] == 0) and np.array_equal(words(g[m, 12:15]), words(px.env[m]))
    rest = np.delete(words(g)[m], [3, 12, 13, 14], axis=1)
    assert not rest.any()                                                                  # what a miss does not define is zero
    assert np.all(words(g)[~m, 3] != 0xFFFFFFFF)


def check_an_all_invalid_grid_gives_ambient(plant=None):
    for name in ("inside", "behind"):
        px = pieces(name)
        for lookup in (plain(coefficients(), valid=np.zeros(P, np.uint8)), by_maps(coefficients(), valid=np.zeros(P, np.uint8))):
            rgb, g = B.compose(px, lookup, AMBIENT, plant)
            h = px.hit
            want = px.emission[h] + (px.color[h] * AMBIENT) * B.INV_PI
            assert np.array_equal(words(rgb[h]), words(want)) and np.all(g[:, 11] == 0)
    # ... and ambient is not what lights a pixel whose probes answer
    px = pieces("inside")
    rgb, g = B.compose(px, plain(coefficients()), AMBIENT, plant)
    lit = px.hit & (g[:, 11] > 0) & (px.color.max(axis=1) > 0)
    assert lit.sum() > 100
    want = px.emission[lit] + (px.color[lit] * AMBIENT) * B.INV_PI
    assert (words(rgb[lit]) != words(want)).any(axis=1).mean() > 0.9


def check_the_normal_faces_the_viewer(plant=None):
    """The scene's camera sees the back wall from the side its shading normal points away from: the record's normal is its
    negative, word for word, and a volume lit from the camera's side only lights the wall.  From the other side the normal
    is kept."""
    other = pieces("behind")
    g = B.compose(other, plain(coefficients()), AMBIENT, plant)[1]
    assert np.array_equal(words(g[other.hit, 4:7]), words(other.ns[other.hit]))
    px = pieces("inside")
    sh = np.zeros((P, 9, 4), F)
    sh[:, 0, :3] = 1.0
    sh[:, 2, :3] = -1.6         # band 1, the z term: light from -z, where this camera stands
    rgb, g = B.compose(px, plain(sh, backface=False), (0, 0, 0), plant)
    h = px.hit & ((px.d * px.ns).sum(axis=1) > 0) & (px.ns[:, 2] > 0.99)          # the back wall
    assert h.sum() > 10
    assert np.array_equal(words(g[h, 4:7]), words(-px.ns[h]))
    assert np.all((px.d[px.hit] * g[px.hit, 4:7]).sum(axis=1) <= 0)
    E = plain(sh, backface=False)(g[h, 0:8])
    away = G.sample(*GRID, sh, np.concatenate([g[h, 0:4], -g[h, 4:7], g[h, 7:8]], axis=1), backface=False, blocked=None)
    assert np.all(E[:, :3] > 1.5 * np.abs(away[:, :3]))
    want = px.emission[h] + (px.color[h] * E[:, :3]) * B.INV_PI
    assert np.array_equal(words(rgb[h]), words(want))


def synthetic():
    """Four hand-made hits whose shading and geometric normals lie on opposite sides of the ray, and values of d * dst + o
    that round differently in one step and in two."""
    rng = np.random.default_rng(3)
    n = 64
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F)
    o = rng.uniform(-0.5, 0.5, (n, 3)).astype(F) + F([0.0, 1.0, 0.0])
    ns = rng.normal(size=(n, 3))
    ns = (ns / np.linalg.norm(ns, axis=1, keepdims=True)).astype(F)
    ng = ns.copy()
    ng[::2] = -ng[::2]
    return SimpleNamespace(o=o, d=d, hit=np.ones(n, bool), dst=rng.uniform(0.1, 0.7, n).astype(F), inst=np.arange(n, dtype=np.uint32),
                           tri=np.arange(n, dtype=np.uint32)[::-1].copy(), ns=ns, ng=ng, color=rng.uniform(0.1, 0.9, (n, 3)).astype(F),
                           emission=np.zeros((n, 3), F), env=np.zeros((n, 3), F))


def check_p_and_n_word_for_word_on_made_up_hits(plant=None):
    px = synthetic()
    rgb, g = B.compose(px, plain(coefficients()), AMBIENT, plant)
    prod = (px.d.astype(np.float64) * px.dst[:, None].astype(np.float64)).astype(F)                      # the product, rounded
    p = (px.o.astype(np.float64) + prod.astype(np.float64)).astype(F)                                     # ... then the sum, rounded
    fused = (px.d.astype(np.float64) * px.dst[:, None].astype(np.float64) + px.o.astype(np.float64)).astype(F)
    assert (words(p) != words(fused)).any()                                                               # the two orders differ here
    assert np.array_equal(words(g[:, 0:3]), words(p))
    c = (px.d.astype(np.float64) * px.ns.astype(np.float64)).sum(axis=1)
    assert np.all(np.abs(c) > 1e-3)
    assert np.array_equal(words(g[:, 4:7]), words(np.where((c > 0)[:, None], -px.ns, px.ns)))
    assert np.array_equal(words(g)[:, 3], px.inst) and np.array_equal(words(g)[:, 7], px.tri) and np.array_equal(words(g[:, 15]), words(px.dst))
    # the first eight words are the record: re-fed they reproduce E and w
    res = plain(coefficients())(g[:, 0:8])
    assert np.array_equal(words(g[:, 11]), words(res[:, 3]))
    E = np.where((res[:, 3] != 0)[:, None], res[:, :3], AMBIENT)
    assert np.array_equal(words(rgb), words(px.emission + (px.color * E) * B.INV_PI))


def check_a_record_the_lookups_refuse_is_not_asked(plant=None):
    px = synthetic()
    px.ns[3] *= F(1.001)                                   # |n|^2 - 1 = 2e-3
    px.ns[5, 1] = np.nan
    px.o[7, 0] = np.inf
    px.ns[9] *= F(1.00004)                                 # |n|^2 - 1 = 8e-5: still a unit vector to the lookups
    asked = []

    def lookup(rec):
        asked.append(rec)
        return plain(coefficients())(rec)

    rgb, g = B.compose(px, lookup, AMBIENT, plant)
    assert len(asked) == 1 and len(asked[0]) == 61 and np.isfinite(asked[0]).all()
    bad = [3, 5, 7]
    assert np.all(g[bad, 11] == 0) and g[9, 11] > 0
    with np.errstate(all="ignore"):
        want = px.emission[bad] + (px.color[bad] * AMBIENT) * B.INV_PI
    assert np.array_equal(words(rgb[bad]), words(want))


def check_emission_is_added(plant=None):
    px = pieces("inside")
    rgb, _ = B.compose(px, plain(coefficients(), valid=np.zeros(P, np.uint8)), (0, 0, 0), plant)
    lamp = px.emission.max(axis=1) > 0
    assert lamp.sum() >= 2 and np.array_equal(words(rgb[lamp]), words(px.emission[lamp] + (px.color[lamp] * F(0)) * B.INV_PI))
    assert np.all(rgb[lamp].max(axis=1) == 17.0)


def check_the_store_on_the_bit_layout(plant=None):
    rgb = F([[0.0, 1.0, -2.0], [0.1, 65504.0, 65519.0], [65520.0, 1e-8, 5.97e-8], [1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -10],
             [0.333333, 17.0, 1e5]])
    rtz, rne = B.texels(rgb, film_ref.RTZ), B.texels(rgb, film_ref.RNE)
    assert np.all(rtz[:, 3] == 0x3C00) and np.all(rne[:, 3] == 0x3C00)
    with np.errstate(over="ignore"):
        assert np.array_equal(rne[:, :3], rgb.astype(np.float16).view(np.uint16))          # numpy's conversion rounds to nearest even
    back = film_ref.half_to_f64(rtz[:, :3])
    assert np.all(np.abs(back) <= np.abs(rgb.astype(np.float64))) and np.all(np.isfinite(back))   # toward zero: never larger, never infinite
    assert rtz[3, 0] == 0x3C00 and rne[3, 0] == 0x3C00 and rtz[3, 1] == 0x3C01 and rne[3, 1] == 0x3C02 and rtz[1, 2] == 0x7BFF and rne[2, 0] == 0x7C00
    px = pieces("far")
    for mode in (film_ref.RTZ, film_ref.RNE):
        tex, g = B.render(px, by_maps(coefficients()), AMBIENT, mode, plant)
        rgb, g2 = B.compose(px, by_maps(coefficients()), AMBIENT, plant)
        assert np.array_equal(tex, B.texels(rgb, mode)) and np.array_equal(words(g), words(g2))


CHECKS = [check_every_view_has_what_it_is_for, check_band_zero_gives_the_closed_form, check_a_miss_is_the_environment,
          check_an_all_invalid_grid_gives_ambient, check_the_normal_faces_the_viewer, check_p_and_n_word_for_word_on_made_up_hits,
          check_a_record_the_lookups_refuse_is_not_asked, check_emission_is_added, check_the_store_on_the_bit_layout]


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__)
def test_contract(built, check):
    check()


@pytest.mark.parametrize("plant", B.PLANTS)
def test_every_planted_misreading_fails_a_check(built, plant):
    failed = []
    for check in CHECKS:
        try:
            check(plant)
        except AssertionError:
            failed.append(check.__name__)
    assert failed, plant


def test_no_device_is_an_error_not_a_fallback(built):
    sc, cam = scene()
    target = type("T", (), {"format": lambda self: "Rgba16Float", "width": 4, "height": 4, "handle": None})()
    with pytest.raises(api.LupinError) as e:
        api.render_baked(None, sc, target, cam.params, cam.transform, *GRID, coefficients())
    assert e.value.code == -2 and "render_baked" in str(e.value)
    if api.device_count() == 0:
        with pytest.raises(api.LupinError) as e:
            api.Context(0)
        assert e.value.code == -2
