"""Probe depth maps without a device: tests/probe_depth_ref.py's float32 restatement of both contracts
against float64, closed forms and the words of include/lupin_hip.h, with the distances of tests/closest_hit_ref.py's float64
brute-force intersector.  The device is held to the restatement word for word in tests/test_gpu_probe_depth.py.

Every check is a function of `plant` (probe_depth_ref.PLANTS): None is the contract, and
test_every_planted_misreading_fails_a_check shows that each misreading fails at least one of them."""
import ctypes as C
import math

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import closest_hit_ref as X
from tests import probe_depth_ref as D
from tests import probe_grid_ref as G

U = D.U
F = np.float32


def unit(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


# ---- geometry for the brute-force intersector ------------------------------------------------------------------------

def geometry(meshes):
    rows = np.tile(np.eye(3, 4)[None], (len(meshes), 1, 1))
    return X.Geometry(rows, np.arange(len(meshes)), [X.Mesh(np.asarray(v, np.float64), np.asarray(t, np.int64)) for v, t in meshes])


def cube(h):
    v = np.array([[x, y, z] for x in (-h, h) for y in (-h, h) for z in (-h, h)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))])


def wall_x(half=10.0):
    """tests/test_gpu_probe_grid.py's wall: a quad in the plane x = 0."""
    v = np.array([(0.0, -half, -half), (0.0, -half, half), (0.0, half, half), (0.0, half, -half)])
    return v, np.array([(0, 1, 2), (0, 2, 3)])


_baked = {}


def traced(name, g, positions, R, K, eps=0.0):
    """(hit, dst) (n, S) of the float64 intersector for the probes' rays, dst rounded to float32."""
    key = (name, R, K)
    if key not in _baked:
        w = D.directions(R, K).astype(np.float64)
        pos = np.asarray(positions, np.float64).reshape(-1, 3)
        h = X.closest_hits(g, np.repeat(pos, len(w), axis=0), np.tile(w, (len(pos), 1)), eps)
        _baked[key] = (h.hit.reshape(len(pos), -1), np.where(h.hit, h.t, 0.0).astype(np.float32).reshape(len(pos), -1))
    return _baked[key]


# ---- encode / decode -------------------------------------------------------------------------------------------------

def check_round_trip(plant=None):
    rng = np.random.default_rng(1)
    w = np.concatenate([unit(rng, 4000), np.eye(3, dtype=F), -np.eye(3, dtype=F), F([[0.6, 0, -0.8], [0, -0.6, -0.8], [0.6, 0.8, 0]])])
    back = D.decode(D.encode(w, plant=plant), plant=plant)
    err = np.abs(back.astype(np.float64) - w)
    print("round trip: max error / bound", err.max() / D.ROUND_TRIP)
    assert err.max() <= D.ROUND_TRIP
    wide = D.decode(D.encode(w, np.float64, plant), np.float64, plant)
    assert np.abs(wide - w / np.linalg.norm(w.astype(np.float64), axis=1, keepdims=True)).max() < 1e-15


def check_texel_centres_are_unit_vectors(plant=None):
    for R, K in ((2, 1), (5, 4), (16, 4), (64, 8)):
        w = D.directions(R, K, plant=plant).astype(np.float64)
        assert np.abs(np.linalg.norm(w, axis=1) - 1.0).max() <= D.UNIT
        # ... and the sub-grid is symmetric about both axes of the square: so is the set of directions in x and in y
        assert np.abs(w[:, :2].sum(0)).max() <= len(w) * D.UNIT
        assert (w[:, 2] > 0).sum() == (w[:, 2] < 0).sum()


def check_seams_decode_to_one_direction(plant=None):
    t = np.linspace(-1, 1, 129).astype(F)
    one = np.ones_like(t)
    for s in (one, -one):
        a, b = D.decode(np.stack([s, t], -1), plant=plant), D.decode(np.stack([s, -t], -1), plant=plant)
        assert np.array_equal(a, b)          # the edge u = +-1: (u, v) and (u, -v), value for value (a zero's sign may differ)
        a, b = D.decode(np.stack([t, s], -1), plant=plant), D.decode(np.stack([-t, s], -1), plant=plant)
        assert np.array_equal(a, b)          # the edge v = +-1: (u, v) and (-u, v)
    # the fold |u| + |v| = 1 inside the square: the two branches meet there (z = 0, exact on these binary fractions)
    q = (np.arange(1, 64) / 64.0).astype(F)
    for su in (1, -1):
        for sv in (1, -1):
            uv = np.stack([su * q, sv * (F(1.0) - q)], -1)
            inner, outer = D.decode(uv * F(1 - 2.0 ** -20), np.float64, plant), D.decode(uv * F(1 + 2.0 ** -20), np.float64, plant)
            assert np.abs(inner - outer).max() < 1e-5


# ---- the border ------------------------------------------------------------------------------------------------------

def check_border_texels_equal_their_sources(plant=None):
    for R in (2, 3, 5, 16):
        inner = np.random.default_rng(R).normal(size=(2, R, R, 2)).astype(F)
        m = D.bordered(inner, plant)
        assert m.shape == (2, R + 2, R + 2, 2)
        clamp = lambda c: min(max(c, 0), R - 1)
        for by in range(-1, R + 1):
            for bx in range(-1, R + 1):
                ox, oy = bx < 0 or bx >= R, by < 0 or by >= R
                if ox and oy:
                    sx, sy = R - 1 - clamp(bx), R - 1 - clamp(by)
                elif ox:
                    sx, sy = clamp(bx), R - 1 - by
                elif oy:
                    sx, sy = R - 1 - bx, clamp(by)
                else:
                    sx, sy = bx, by
                assert np.array_equal(m[:, by + 1, bx + 1], inner[:, sy, sx]), (R, bx, by)


LIP_A = np.array([0.3, -0.5, 0.4])


def smooth(w):
    """2 + a . w: Lipschitz in w with constant |a|."""
    return 2.0 + w @ LIP_A


def check_bilinear_is_continuous_across_every_seam(plant=None):
    """A map of f at the texel centres' directions, interpolated at direction e, is a convex combination of f at four texel
    centres at most one texel (2 / R in u and in v) from e's own coordinates -- across a seam too, where the border holds the
    texel that the wrapped coordinate names.  The decode is Lipschitz from (u, v) to the sphere with constant 3 (the
    unnormalised vector moves by at most sqrt(3) |d(u, v)|: x and y by du and dv, z by |du| + |dv|; it is at least
    1 / sqrt(3) long).  So |interp(e) - f(e)| <= |a| * 3 * 2 sqrt(2) / R, float64 throughout."""
    R = 16
    f = smooth(D.directions(R, 1, np.float64)).reshape(1, R, R)
    maps = D.bordered(np.stack([f, f * f], -1).astype(F), plant)
    bound = np.linalg.norm(LIP_A) * 3.0 * 2.0 * math.sqrt(2.0) / R + 1e-6       # (+ the float32 storage of f)
    t = np.linspace(-1, 1, 201)
    edge = []
    for s in (1.0, -1.0):
        for inset in (1e-9, 0.3 / R, 0.9 / R):
            edge += [np.stack([np.full_like(t, s * (1 - inset)), t], -1), np.stack([t, np.full_like(t, s * (1 - inset))], -1)]
    corners = np.array([[su * (1 - a), sv * (1 - b)] for su in (1, -1) for sv in (1, -1) for a in (1e-9, 0.4 / R) for b in (1e-9, 0.7 / R)])
    uv = np.concatenate(edge + [corners])
    e = D.decode(uv, np.float64)
    m1, _, _ = D.fetch(maps, np.zeros(len(e), np.int64), e, R, np.float64, plant)
    err = np.abs(m1 - smooth(e))
    print("seams: max error / bound", err.max() / bound)
    assert err.max() <= bound
    # ... and the two sides of a seam agree with each other: the same direction reached from (u, v) and from (u, -v)
    side = np.stack([np.full_like(t, 1 - 1e-9), t], -1)
    a, _, _ = D.fetch(maps, np.zeros(len(t), np.int64), D.decode(side, np.float64), R, np.float64, plant)
    b, _, _ = D.fetch(maps, np.zeros(len(t), np.int64), D.decode(side * [1, -1], np.float64), R, np.float64, plant)
    assert np.abs(a - b).max() <= 1e-6


# ---- closed forms ----------------------------------------------------------------------------------------------------

def check_cube_moments(plant=None):
    h = 1.0
    for R, K in ((8, 4), (5, 2), (4, 8)):
        hit, dst = traced("cube", geometry([cube(h)]), [[0, 0, 0]], R, K)
        assert hit.all()
        maps = D.bake(hit, dst, R, K, 4.0, plant=plant).astype(np.float64)
        m1, m2 = maps[..., 0], maps[..., 1]
        s = D.moment_slack(K)
        far = h * math.sqrt(3.0)
        assert np.all(m1 >= h * (1 - s - U)) and np.all(m1 <= far * (1 + s + U))          # (+ u: dst is rounded to float32)
        assert np.all(m2 >= m1 * m1 * (1 - 3 * s))                                       # Jensen; m1^2 carries 2 s, m2 one
        assert np.all(m2 - m1 * m1 <= (far - h) ** 2 / 4 + 3 * s * far * far)            # Popoviciu
        wide = D.bake(hit, dst, R, K, 4.0, np.float64, plant)
        assert np.abs(maps - wide).max() <= s * far * far
        assert np.array_equal(maps[:, 1:-1, 1:-1], D.moments(D.capped(hit, dst, 4.0), R, K).astype(np.float64))


def check_open_scene(plant=None):
    for R, K, maxd in ((4, 1, 1.7), (6, 2, 0.3), (16, 4, 123.456)):
        S = R * R * K * K
        h = X.closest_hits(geometry([]), np.zeros((S, 3)), D.directions(R, K).astype(np.float64), 1e-3)
        assert not h.hit.any()
        maps = D.bake(h.hit[None], np.zeros((1, S), F), R, K, maxd, plant=plant)
        assert np.all(maps[..., 0] == F(maxd)) and np.all(maps[..., 1] == F(maxd) * F(maxd))


# ---- the lookup ------------------------------------------------------------------------------------------------------

ORIGIN, SPACING, DIMS = (-2.0, 1.0, 4.0), (0.5, 2.0, 1.0), (4, 3, 5)
P = int(np.prod(DIMS))


def records(rng, n, margin=0.2):
    lo, size = np.asarray(ORIGIN), np.asarray(SPACING) * (np.asarray(DIMS) - 1)
    p = lo - margin * size + rng.uniform(size=(n, 3)) * size * (1 + 2 * margin)
    return api.probe_grid_records(p.astype(F), unit(rng, n))


def check_maps_at_the_cap_reproduce_the_plain_lookup(plant=None):
    rng = np.random.default_rng(3)
    rec = records(rng, 400)
    sh = rng.normal(size=(P, 9, 4)).astype(F)
    R, maxd = 6, 0.4                                            # below the distance of most corners: r = maxd = m1, never r > m1
    maps = np.empty((P, R + 2, R + 2, 2), F)
    maps[..., 0], maps[..., 1] = maxd, rng.uniform(0, 9, maps.shape[:-1])
    valid = (rng.uniform(size=P) > 0.3).astype(np.uint8)
    for back in (False, True):
        for v in (None, valid):
            for bias in (0.0, 0.03125):
                got = D.sample(ORIGIN, SPACING, DIMS, sh, maps, rec, maxd, valid=v, backface=back, normal_bias=bias, plant=plant)
                want = G.sample(ORIGIN, SPACING, DIMS, sh, rec, valid=v, backface=back, normal_bias=bias)
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the same from a bake whose cap is below every distance
    hit, dst = traced("cube", geometry([cube(1.0)]), [[0, 0, 0]], 8, 4)
    assert np.all(D.bake(hit, dst, 8, 4, 0.5, plant=plant)[..., 0] == F(0.5))


def check_a_point_on_a_probe_returns_that_probe(plant=None):
    rng = np.random.default_rng(4)
    pos = api.probe_grid_positions(ORIGIN, SPACING, DIMS)
    nrm = unit(rng, P)
    sh = rng.normal(size=(P, 9, 4)).astype(F)
    maps = np.zeros((P, 6, 6, 2), F)                            # every probe sees a surface at distance 0: only len == 0 is visible
    got = D.sample(ORIGIN, SPACING, DIMS, sh, maps, api.probe_grid_records(pos, nrm), 3.0, plant=plant)
    want = G.sample(ORIGIN, SPACING, DIMS, sh, api.probe_grid_records(pos, nrm))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.all(got[:, 3] == 1.0)
    assert np.all(np.abs(got[:, :3] - api.sh_irradiance(sh, nrm)) <= G.irradiance_bound(sh, nrm))


def check_skipped_corners_renormalise(plant=None):
    rng = np.random.default_rng(5)
    rec = records(rng, 400, margin=0.0)
    sh = rng.normal(size=(P, 9, 4)).astype(F)
    sh[:, :, 3] = 0
    shut = rng.uniform(size=P) < 0.4
    maps = np.empty((P, 7, 7, 2), F)
    maps[..., 0], maps[..., 1] = 100.0, 10000.0                 # far: visible
    maps[shut, ..., 0], maps[shut, ..., 1] = 2.0 ** -10, 2.0 ** -20   # a surface right at the probe, no variance: vis == 0 exactly
    got = D.sample(ORIGIN, SPACING, DIMS, sh, maps, rec, 200.0, plant=plant)
    cn = G.corners(ORIGIN, SPACING, DIMS, rec)
    assert np.all(cn.len[cn.use] > 2.0 ** -9)
    want = G.sample(ORIGIN, SPACING, DIMS, sh, rec, blocked=shut[cn.index], ray_epsilon=0.0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert ((got[:, 3] > 0) & (got[:, 3] < 0.999)).sum() > 100
    # all eight skipped: four zero words
    maps[..., 0], maps[..., 1] = 2.0 ** -10, 2.0 ** -20
    assert np.all(D.sample(ORIGIN, SPACING, DIMS, sh, maps, rec, 200.0, plant=plant).view(np.uint32) == 0)


def check_a_nan_moment_of_an_invalid_probe_stays_out(plant=None):
    rng = np.random.default_rng(6)
    rec = records(rng, 300)
    sh = rng.normal(size=(P, 9, 4)).astype(F)
    valid = (rng.uniform(size=P) > 0.4).astype(np.uint8)
    maps = np.empty((P, 6, 6, 2), F)
    maps[..., 0], maps[..., 1] = 0.6, 0.5
    clean = D.sample(ORIGIN, SPACING, DIMS, sh, maps, rec, 5.0, valid=valid, backface=True, plant=plant)
    maps[valid == 0] = np.nan
    sh[valid == 0] = np.nan
    got = D.sample(ORIGIN, SPACING, DIMS, sh, maps, rec, 5.0, valid=valid, backface=True, plant=plant)
    assert np.all(np.isfinite(got)) and np.array_equal(got.view(np.uint32), clean.view(np.uint32))
    # what the header says of a NaN in a probe that IS used: a NaN m1 leaves the corner visible, a NaN m2 shuts it
    maps[...] = (0.6, 0.5)
    sh = np.nan_to_num(sh)
    maps[..., 0] = np.nan
    a = D.sample(ORIGIN, SPACING, DIMS, sh, maps, rec, 5.0, plant=plant)
    assert np.array_equal(a.view(np.uint32), G.sample(ORIGIN, SPACING, DIMS, sh, rec).view(np.uint32))
    maps[..., 0], maps[..., 1] = 2.0 ** -10, np.nan
    assert np.all(D.sample(ORIGIN, SPACING, DIMS, sh, maps, records(rng, 300, margin=0.0), 5.0, plant=plant).view(np.uint32) == 0)


def check_float32_lookup_follows_float64(plant=None):
    """Maps with real variance: the float32 restatement against its float64 form, where no corner sits at a decision."""
    rng = np.random.default_rng(7)
    rec = records(rng, 400, margin=0.0)
    sh = np.abs(rng.normal(size=(P, 9, 4))).astype(F)
    sh[:, 1:] = 0
    maps = np.empty((P, 10, 10, 2), F)
    maps[..., 0] = rng.uniform(0.2, 1.5, maps.shape[:-1])
    maps[..., 1] = maps[..., 0] ** 2 + rng.uniform(0.01, 0.3, maps.shape[:-1])
    a = D.sample(ORIGIN, SPACING, DIMS, sh, maps, rec, 1.2, backface=True, plant=plant)
    b = D.sample(ORIGIN, SPACING, DIMS, sh, maps, rec, 1.2, backface=True, dtype=np.float64, plant=plant)
    assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max()
    plain = G.sample(ORIGIN, SPACING, DIMS, sh, rec, backface=True)
    assert (np.abs(a[:, 3] - plain[:, 3]) > 1e-3).mean() > 0.5          # the maps matter


def check_the_variance_is_of_the_interpolated_moments(plant=None):
    """A checkerboard of texels without variance of their own (m2 == m1 * m1, m1 = 1 or 2): between texel centres the
    interpolated moments have the variance of the mixture, so a corner further than 2 away keeps a positive weight; the
    variance of any single texel is 0 and would shut it."""
    rng = np.random.default_rng(11)
    origin, spacing, dims = (0.0, 0.0, 0.0), (8.0, 8.0, 8.0), (2, 2, 2)
    p = rng.uniform(3.0, 5.0, (300, 3)).astype(F)                    # at least 3 sqrt(3) from every probe
    rec = api.probe_grid_records(p, unit(rng, 300))
    R = 8
    y, x = np.meshgrid(np.arange(R + 2), np.arange(R + 2), indexing="ij")
    maps = np.empty((8, R + 2, R + 2, 2), F)
    maps[..., 0] = 1.0 + ((x + y) & 1)
    maps[..., 1] = maps[..., 0] ** 2
    sh = np.ones((8, 9, 4), F)
    for T in (np.float32, np.float64):
        got = D.sample(origin, spacing, dims, sh, maps, rec, 20.0, dtype=T, plant=plant)
        assert np.all(got[:, 3] > 0) and np.all(got[:, 3] < 1e-3)    # var <= 1 / 4, (r - m1)^2 >= 9: c <= 1 / 37


# ---- no light through a wall -----------------------------------------------------------------------------------------
# The wall of DESIGN.md 23 in the plane x = 0.  Probes 0.5 from it on either side, 0.5 apart across: from a probe the wall is
# at most 35 degrees off the axis towards any point of the cell, where a 16 x 16 map's texel spans about 0.1 of distance:
# a variance below 0.005 against (r - m1)^2 >= 0.16 for a point 0.4 behind the wall.
WALL_GRID = (F([-0.5, -0.25, -0.25]), F([1.0, 0.5, 0.5]), (2, 2, 2))
WALL_L = F([1.0, 2.5, 0.25])
WALL_LEAK = 1e-3


def wall_inputs():
    pos = api.probe_grid_positions(*WALL_GRID)
    sh = np.zeros((8, 9, 4), F)
    sh[pos[:, 0] < 0, 0, :3] = WALL_L / G.K0
    rng = np.random.default_rng(8)
    n = 200
    yz = rng.uniform(-0.2, 0.2, (n, 2)).astype(F)
    dark = api.probe_grid_records(np.column_stack([np.full(n, 0.4, F), yz]), np.tile(F([1, 0, 0]), (n, 1)))
    lit = api.probe_grid_records(np.column_stack([np.full(n, -0.5, F), yz]), np.tile(F([-1, 0, 0]), (n, 1)))   # in the lit probes' plane: fx == 0
    return pos, sh, dark, lit, api.probe_grid_depth_max_distance(WALL_GRID[1])


def assert_no_light_through_the_wall(sample, maps, sh, dark, lit, maxd, exact_ref=None):
    """`sample(records, backface)` -> (n, 4): the lookup under test on `maps`."""
    for back in (False, True):
        leak = G.sample(*WALL_GRID, sh, dark, backface=back, dtype=np.float64)
        got = sample(dark, back)
        assert np.all(leak[:, :3] > 0) and np.all(got[:, 3] > 0)
        ratio = (got[:, :3] / leak[:, :3]).max()
        print("leak left:", ratio)
        assert ratio <= WALL_LEAK
        got = sample(lit, back)
        want = np.pi * WALL_L.astype(np.float64)
        bound = G.irradiance_bound(sh[0], lit[:, 4:7])
        assert np.all(np.abs(got[:, :3] - want) <= bound + np.pi * 2.0 ** -24 * WALL_L) and np.all(got[:, 3] > 0)


def check_no_light_through_a_wall(plant=None):
    pos, sh, dark, lit, maxd = wall_inputs()
    hit, dst = traced("wall", geometry([wall_x()]), pos, 16, 4, eps=1e-3)
    assert 0 < hit.sum() < hit.size
    maps = D.bake(hit, dst, 16, 4, maxd, plant=plant)
    assert_no_light_through_the_wall(lambda rec, back: D.sample(*WALL_GRID, sh, maps, rec, maxd, backface=back, dtype=np.float64, plant=plant),
                                     maps, sh, dark, lit, maxd)


CHECKS = [check_round_trip, check_texel_centres_are_unit_vectors, check_seams_decode_to_one_direction, check_border_texels_equal_their_sources,
          check_bilinear_is_continuous_across_every_seam, check_cube_moments, check_open_scene, check_maps_at_the_cap_reproduce_the_plain_lookup,
          check_a_point_on_a_probe_returns_that_probe, check_skipped_corners_renormalise, check_a_nan_moment_of_an_invalid_probe_stays_out,
          check_float32_lookup_follows_float64, check_the_variance_is_of_the_interpolated_moments, check_no_light_through_a_wall]


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__[6:])
def test_contract(check):
    check()


@pytest.mark.parametrize("plant", D.PLANTS)
def test_every_planted_misreading_fails_a_check(plant):
    failed = []
    for check in CHECKS:
        try:
            check(plant)
        except AssertionError:
            failed.append(check.__name__)
    print(plant, "fails", failed)
    assert failed, plant


def test_python_helpers():
    assert api.probe_grid_depth_max_distance((1.0, 0.5, 0.5)) == F(1.5 * math.sqrt(1.5))
    d = api.ProbeDepthDesc()
    assert (d.resolution, d.subsamples, d.flags, d.max_slots, d.ray_epsilon) == (16, 4, 0, 0, 0.001)
    assert C.sizeof(_abi.ProbeDepthDescC) == 24 and C.sizeof(_abi.ProbeGridDepthDescC) == C.sizeof(_abi.ProbeGridDescC) + 8 == 56
    assert _abi.ProbeGridDepthDescC.resolution.offset == 48 and _abi.ProbeGridDepthDescC.max_distance.offset == 52
    uv = np.array([[0.25, -0.5], [-1.0, 1.0], [0.0, 0.0], [0.75, 0.75]], F)
    assert np.array_equal(api.oct_decode(uv), D.decode(uv, plant="none"))            # api's form and the restatement's generic form
    w = unit(np.random.default_rng(9), 50)
    assert np.array_equal(api.oct_encode(w), D.encode(w, plant="none"))
    assert np.array_equal(api.oct_decode(F([[0, 0]])), F([[0, 0, 1]])) and np.array_equal(api.oct_encode(F([[0, 0, -3]])), F([[1, 1]]))


def test_no_device_is_an_error_for_both_entry_points(built):
    if api.device_count() > 0:
        pytest.skip("a HIP device is present")
    lib = _abi.lib()
    pos, out, rec = np.zeros((1, 4), F), np.zeros((1, 4, 4, 2), F), np.zeros((1, 8), F)
    rec[0, 6] = 1.0
    d = _abi.ProbeDepthDescC(2, 1, 0, 0, 1e-3, 1.0)
    fake = C.c_void_p(1)
    assert lib.lupin_hip_bake_probe_depth(fake, fake, C.byref(d), 1, _abi.ptr(pos), _abi.ptr(out), None) == -2
    grid = _abi.ProbeGridDescC((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_uint32 * 3)(1, 1, 1), 0, 0.0, 0.0)
    g = _abi.ProbeGridDepthDescC(grid, 2, 1.0)
    sh, res = np.zeros((1, 9, 4), F), np.zeros((1, 4), F)
    assert lib.lupin_hip_sample_probe_grid_depth(fake, fake, C.byref(g), _abi.ptr(sh), _abi.ptr(out), None, 1, _abi.ptr(rec), _abi.ptr(res)) == -2
    assert b"no HIP device" in lib.lupin_hip_last_error()
    scene = X.build("small", X.SEED)
    with pytest.raises(api.LupinError) as e:
        api.bake_probe_depth(None, scene, np.zeros((1, 3)), max_distance=1.0)
    assert e.value.code == -2
    with pytest.raises(api.LupinError):
        api.bake_probe_grid_depth(None, scene, (0, 0, 0), (1, 1, 1), (1, 1, 1))
    with pytest.raises(api.LupinError):
        api.sample_probe_grid_depth(None, scene, (0, 0, 0), (1, 1, 1), (1, 1, 1), sh, out, rec, max_distance=1.0)
