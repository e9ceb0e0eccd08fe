"""The irradiance volume's arithmetic without a device: tests/probe_grid_ref.py's float32 restatement of
lupin_hip_sample_probe_grid against its float64 form and against closed forms, without flags and with each of them, and
the host helpers of api.py.  The device is held to the restatement word for word in tests/test_gpu_probe_grid.py.

Tolerances.  Identical coefficients at every probe: probe_grid_ref.irradiance_bound, 40 u S, derived there from the
float32 rounding of the 9-term sum, the blend and its one division.  Where the coefficients differ between probes the
grids and points are binary fractions (integer origin, power-of-two spacing, points on multiples of 1/64, no bias), so
that the cell index, the fractions f and 1 - f are exact in float32 and what remains is: two roundings in a trilinear
weight, one in t * E, 7 additions each in acc.rgb and acc.w, one division, plus E's own 16 u -- below 32 u max|E| for
same-signed E.  With the backface factor the float32 weights themselves differ from float64 by about 12 u (a square root, a
division, a 3-term dot product, five more operations), each shifting the blend by at most that share of the spread of E
within the cell: 32 u max|E| + 8 * 16 u max|E| = 160 u max|E|."""
import numpy as np
import pytest

from lupinpathtracer_amd import api
from tests import probe_grid_ref as R

U = R.U
ORIGIN, SPACING, DIMS = (-2.0, 1.0, 4.0), (0.5, 2.0, 1.0), (4, 3, 5)
FLAGS = [dict(), dict(backface=True), dict(valid=True), dict(blocked=True)]


def unit(rng, n):
    d = rng.normal(size=(n, 3))
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def points_in(rng, n, origin=ORIGIN, spacing=SPACING, dims=DIMS, margin=0.0):
    """Points on multiples of 1/64 within the grid's box, widened by `margin` boxes on every side."""
    lo = np.asarray(origin)
    size = np.asarray(spacing) * (np.asarray(dims) - 1)
    p = lo - margin * size + rng.uniform(size=(n, 3)) * size * (1 + 2 * margin)
    return (np.round(p * 64) / 64).astype(np.float32)


def nprobes(dims=DIMS):
    return int(np.prod(dims))


def flag_inputs(rng, kw, n, dims=DIMS):
    """valid=True / blocked=True in `kw` become random arrays with about a third dropped."""
    kw = dict(kw)
    if kw.get("valid") is True:
        kw["valid"] = (rng.uniform(size=nprobes(dims)) > 0.33).astype(np.uint8)
    if kw.get("blocked") is True:
        kw["blocked"] = rng.uniform(size=(n, 8)) < 0.33
    return kw


@pytest.mark.parametrize("flags", FLAGS)
def test_identical_coefficients_give_sh_irradiance_whatever_the_weights(flags):
    rng = np.random.default_rng(1)
    n = 500
    coeffs = rng.normal(size=(9, 4)).astype(np.float32)
    sh = np.broadcast_to(coeffs, (nprobes(), 9, 4)).copy()
    nrm = unit(rng, n)
    rec = api.probe_grid_records(points_in(rng, n, margin=0.2), nrm)
    kw = flag_inputs(rng, flags, n)
    got = R.sample(ORIGIN, SPACING, DIMS, sh, rec, normal_bias=0.03125, **kw)
    want = api.sh_irradiance(coeffs, nrm)
    some = got[:, 3] > 0
    assert some.mean() > 0.9
    bound = R.irradiance_bound(coeffs, nrm)
    err = np.abs(got[:, :3].astype(np.float64) - want)
    print("max error / bound", float((err[some] / bound[some]).max()))
    assert np.all(err[some] <= bound[some])
    assert np.all(got[~some] == 0)


@pytest.mark.parametrize("flags", FLAGS)
def test_band_zero_linear_in_position_gives_the_trilinear_interpolant(flags):
    rng = np.random.default_rng(2)
    n = 500
    pos = api.probe_grid_positions(ORIGIN, SPACING, DIMS).astype(np.float64)
    a, b = 3.0, np.array([0.5, -0.25, 0.125])
    sh = np.zeros((nprobes(), 9, 4), np.float32)
    sh[:, 0, :3] = (a + pos @ b)[:, None] * [1.0, 2.0, 4.0]          # exactly representable
    assert np.all(sh[:, 0, 0] > 0)
    p, nrm = points_in(rng, n), unit(rng, n)
    rec = api.probe_grid_records(p, nrm)
    kw = flag_inputs(rng, flags, n)
    got = R.sample(ORIGIN, SPACING, DIMS, sh, rec, **kw)
    twin = R.sample(ORIGIN, SPACING, DIMS, sh, rec, dtype=np.float64, **kw)
    emax = np.pi * 0.5 * np.sqrt(1.0 / np.pi) * float(sh[:, 0, 2].max())
    tol = (160 if kw.get("backface") else 32) * U * emax
    assert np.all(np.abs(got.astype(np.float64) - twin)[:, :3] <= tol)
    assert np.all(np.abs(got[:, 3].astype(np.float64) - twin[:, 3]) <= 16 * U)
    if not flags:
        # every corner in use: the interpolant of a linear function is the function, and the weights add up to 1
        want = np.pi * 0.5 * np.sqrt(1.0 / np.pi) * (a + p.astype(np.float64) @ b)
        assert np.all(np.abs(twin[:, 0] - want) <= 1e-12 * emax) and np.all(np.abs(twin[:, 3] - 1.0) <= 1e-12)
        assert np.all(np.abs(got[:, 2].astype(np.float64) - 4.0 * want) <= tol)


@pytest.mark.parametrize("flags", FLAGS)
def test_w_is_the_sum_of_the_surviving_weights_and_dropped_corners_renormalise(flags):
    rng = np.random.default_rng(3)
    n = 400
    sh = rng.uniform(0.5, 2.0, (nprobes(), 9, 4)).astype(np.float32)
    sh[:, 1:] = 0
    rec = api.probe_grid_records(points_in(rng, n), unit(rng, n))
    kw = flag_inputs(rng, flags, n)
    cn = R.corners(ORIGIN, SPACING, DIMS, rec, valid=kw.get("valid"), backface=kw.get("backface", False))
    use = cn.use & ~kw["blocked"] if "blocked" in kw else cn.use
    got = R.sample(ORIGIN, SPACING, DIMS, sh, rec, **kw)
    w = np.zeros(n, np.float32)
    for c in range(8):                                                   # the stated order
        w = np.where(use[:, c], w + cn.t[:, c], w)
    assert np.array_equal(got[:, 3].view(np.uint32), np.where(w > 0, w, np.float32(0)).view(np.uint32))
    # renormalised: a convex combination of the surviving probes' values, none of the dropped ones'
    E = np.float64(np.pi * 0.5 * np.sqrt(1.0 / np.pi)) * sh[cn.index, 0, 0].astype(np.float64)
    lo, hi = np.where(use, E, np.inf).min(axis=1), np.where(use, E, -np.inf).max(axis=1)
    some = use.any(axis=1)
    assert np.all(got[some, 0] >= lo[some] * (1 - 40 * U)) and np.all(got[some, 0] <= hi[some] * (1 + 40 * U))
    assert np.all(got[~some] == 0)
    if flags:
        full = R.sample(ORIGIN, SPACING, DIMS, sh, rec, backface=kw.get("backface", False))
        dropped = (cn.t != 0).sum(axis=1) > use.sum(axis=1) if "backface" not in kw else np.zeros(n, bool)
        if "backface" not in kw:
            assert dropped.sum() > 50 and np.all(got[dropped & some, 3] < full[dropped & some, 3])


def test_all_eight_dropped_gives_four_zero_words():
    rng = np.random.default_rng(4)
    n = 64
    sh = rng.normal(size=(nprobes(), 9, 4)).astype(np.float32)
    rec = api.probe_grid_records(points_in(rng, n), unit(rng, n))
    for kw in (dict(valid=np.zeros(nprobes(), np.uint8)), dict(blocked=np.ones((n, 8), bool)),
               dict(valid=np.zeros(nprobes(), np.uint8), backface=True)):
        got = R.sample(ORIGIN, SPACING, DIMS, sh, rec, **kw)
        assert np.all(got.view(np.uint32) == 0)
    # a NaN coefficient of a dropped probe stays out; of a used probe it reaches the output
    sh[5] = np.nan
    valid = np.ones(nprobes(), np.uint8); valid[5] = 0
    p5 = api.probe_grid_positions(ORIGIN, SPACING, DIMS)[5] + np.float32([0.125, 0.25, 0.25])
    r5 = api.probe_grid_records(p5[None], [[0.0, 0.0, 1.0]])
    assert np.all(np.isfinite(R.sample(ORIGIN, SPACING, DIMS, sh, r5, valid=valid)))
    assert np.all(np.isnan(R.sample(ORIGIN, SPACING, DIMS, sh, r5)[:, :3]))


@pytest.mark.parametrize("flags", [dict(), dict(backface=True)])
def test_points_outside_equal_their_clamped_twins_without_a_direction_term(flags):
    """The cell and the weights of a point outside are those of the point clamped onto the grid; the backface factor looks
    at the direction from the point itself, so with it only the surviving corners agree, not the words."""
    rng = np.random.default_rng(5)
    n = 300
    sh = rng.normal(size=(nprobes(), 9, 4)).astype(np.float32)
    p = points_in(rng, n, margin=1.0)
    lo = np.float32(ORIGIN)
    hi = (np.asarray(ORIGIN) + np.asarray(SPACING) * (np.asarray(DIMS) - 1)).astype(np.float32)
    outside = np.any((p < lo) | (p > hi), axis=1)
    assert outside.sum() > 200
    nrm = unit(rng, n)
    a, b = api.probe_grid_records(p, nrm), api.probe_grid_records(np.clip(p, lo, hi), nrm)
    ca, cb = R.corners(ORIGIN, SPACING, DIMS, a), R.corners(ORIGIN, SPACING, DIMS, b)
    assert np.array_equal(ca.index, cb.index) and np.array_equal(ca.t.view(np.uint32), cb.t.view(np.uint32))
    if not flags:
        assert np.array_equal(R.sample(ORIGIN, SPACING, DIMS, sh, a).view(np.uint32), R.sample(ORIGIN, SPACING, DIMS, sh, b).view(np.uint32))
    else:
        assert np.array_equal(R.corners(ORIGIN, SPACING, DIMS, a, backface=True).use, cb.use)


def test_an_axis_with_one_probe_ignores_that_coordinate():
    rng = np.random.default_rng(6)
    n = 200
    dims = (4, 1, 3)
    sh = rng.normal(size=(nprobes(dims), 9, 4)).astype(np.float32)
    p, nrm = points_in(rng, n, dims=(4, 3, 3)), unit(rng, n)
    q = p.copy()
    q[:, 1] = rng.uniform(-100, 100, n).astype(np.float32)
    a = R.sample(ORIGIN, SPACING, dims, sh, api.probe_grid_records(p, nrm))
    b = R.sample(ORIGIN, SPACING, dims, sh, api.probe_grid_records(q, nrm))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    cn = R.corners(ORIGIN, SPACING, dims, api.probe_grid_records(q, nrm))
    assert not cn.use[:, [2, 3, 6, 7]].any() and cn.use[:, [0, 1, 4, 5]].any()      # the y + 1 corners have weight 0
    # one probe in all: its irradiance everywhere
    one = R.sample(ORIGIN, SPACING, (1, 1, 1), sh[:1], api.probe_grid_records(q, nrm))
    assert np.all(one[:, 3] == 1.0)
    assert np.all(np.abs(one[:, :3] - api.sh_irradiance(sh[0], nrm)) <= R.irradiance_bound(sh[0], nrm))


@pytest.mark.parametrize("flags", [dict(), dict(backface=True), dict(blocked=True)])
def test_a_point_on_a_probe_returns_that_probe(flags):
    """One corner has t == 1 and seven have t == 0; its segment has length 0, so it is never blocked (len <= 2 eps)."""
    rng = np.random.default_rng(7)
    pos = api.probe_grid_positions(ORIGIN, SPACING, DIMS)
    P = len(pos)
    sh = rng.normal(size=(P, 9, 4)).astype(np.float32)
    nrm = unit(rng, P)
    kw = dict(flags)
    if kw.get("blocked"):
        kw["blocked"] = np.ones((P, 8), bool)
    got = R.sample(ORIGIN, SPACING, DIMS, sh, api.probe_grid_records(pos, nrm), **kw)
    cn = R.corners(ORIGIN, SPACING, DIMS, api.probe_grid_records(pos, nrm))
    assert np.all(cn.use.sum(axis=1) == 1) and np.all(cn.index[cn.use] == np.arange(P)) and np.all(cn.len[cn.use] == 0)
    w = np.float32(1.0) * (np.float32(1.0) * np.float32(1.0) + np.float32(0.2)) if kw.get("backface") else np.float32(1.0)   # dir = nrm: b = 1
    assert np.all(np.abs(got[:, 3] - w) <= 4 * U)
    assert np.all(np.abs(got[:, :3] - api.sh_irradiance(sh, nrm)) <= R.irradiance_bound(sh, nrm))


def test_probe_grid_positions_is_the_f32_expression():
    origin, spacing, dims = np.float32([0.1, -7.3, 1e3]), np.float32([0.3, 1.7, 1e-3]), (5, 3, 4)
    pos = api.probe_grid_positions(origin, spacing, dims)
    assert pos.dtype == np.float32 and pos.shape == (60, 3)
    for iz in range(4):
        for iy in range(3):
            for ix in range(5):
                want = [origin[k] + np.float32(i) * spacing[k] for k, i in enumerate((ix, iy, iz))]
                assert np.array_equal(pos[ix + 5 * (iy + 3 * iz)], np.float32(want))
    assert np.array_equal(api.probe_grid_positions(origin, spacing, (1, 1, 1)), origin[None])
    rec = api.probe_grid_records(pos[:3], [[0, 0, 1]] * 3)
    assert rec.shape == (3, 8) and rec.dtype == np.float32 and np.array_equal(rec[:, :3], pos[:3]) and np.all(rec[:, 6] == 1) and np.all(rec[:, [3, 7]] == 0)


def test_segments_are_the_corners_in_use_longer_than_two_epsilons():
    rng = np.random.default_rng(8)
    n = 100
    p = points_in(rng, n)
    p[:10] = api.probe_grid_positions(ORIGIN, SPACING, DIMS)[:10] + np.float32([0.001, 0, 0])     # 1e-3 from a probe
    rec = api.probe_grid_records(p, unit(rng, n))
    cn = R.corners(ORIGIN, SPACING, DIMS, rec)
    for eps in (0.0, 1e-3, 0.25):
        seg, mask = R.segments(cn, eps)
        assert seg.shape == (int(mask.sum()), 8) and np.array_equal(mask, cn.use & (cn.len > np.float32(2.0) * np.float32(eps)))
        assert np.all(seg[:, 7] > 0) and np.all(np.abs((seg[:, 4:7].astype(np.float64) ** 2).sum(1) - 1) < 1e-6)
    assert R.segments(cn, 0.25)[1].sum() < R.segments(cn, 0.0)[1].sum()


def test_without_a_context_there_is_an_error_not_a_fallback(built):
    from lupinpathtracer_amd import loader
    scene, _ = loader.build_scene_cornell_box(None)
    sh = np.zeros((8, 9, 4), np.float32)
    for call in (lambda: api.sample_probe_grid(None, scene, (0, 0, 0), (1, 1, 1), (2, 2, 2), sh, [[0.5, 0.5, 0.5]], [[0, 0, 1]]),
                 lambda: api.bake_probe_grid(None, scene, (0, 0, 0), (1, 1, 1), (2, 2, 2))):
        with pytest.raises(api.LupinError) as e:
            call()
        assert e.value.code == -2   # LUPIN_ERR_NO_DEVICE
