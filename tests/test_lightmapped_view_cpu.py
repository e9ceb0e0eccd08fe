"""The lightmapped view's contract (include/lupin_hip.h) on the CPU: tests/lightmapped_view_ref.py composed over
the oracle's camera, closest-hit and surface restatements on the three-chart scene of tests/test_gpu_lightmap.py (three
spheres with charts, a floor box with texcoords, a box without), with synthetic atlases and tests/probe_grid_ref.py's lookup.
Every check is a function of an optional planted misreading; the contract passes them all and every plant fails at least one."""
from types import SimpleNamespace

import numpy as np
import pytest

from lupinpathtracer_amd import api
from oracle import oracle
from tests import baked_view_ref as B
from tests import lightmap_ref
from tests import lightmapped_view_ref as L
from tests import probe_grid_ref as G
from tests.test_gpu_lightmap import THREE_CHARTS, three_chart_cpu

F = np.float32
U = 2.0 ** -24                                                         # half an ulp of float32, relative
AMBIENT = F([0.11, 0.07, 0.05])
GRID = (F([-4.0, -1.4, -1.5]), F([2.0, 1.0, 1.5]), (5, 4, 4))          # probes around the spheres and over the floor
P = 80
EPS = 1e-3
W_IMG, H_IMG = 60, 36
AW, AH = 17, 33
FLOOR = api.LightmapChart(3, 0.9, 0.4, 0.05, 0.55)
CHARTS = THREE_CHARTS + [FLOOR]
CAMERA = (api.CameraParams(is_orthographic=False, lens=0.035, film=0.036, aspect=1.5, focus=6.5, aperture=0.0),
          F([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.0, 0.3, -6.5]]))
_cache = {}


def words(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def scene():
    if "scene" not in _cache:
        cpu, envs = three_chart_cpu()
        api.validate_scene(cpu, 0, 0)
        sc = api.build_accel_structures_and_upload(None, cpu, [], envs, True)
        _cache["scene"] = (cpu, sc, L.geometry(cpu, sc))
    return _cache["scene"]


def pieces():
    if "px" not in _cache:
        _, sc, _ = scene()
        _cache["px"] = L.pieces(oracle.camera_probe, lambda o, d, e: oracle.trace_rays(sc, o, d, e), lambda r: oracle.surface_probe(sc, r),
                                W_IMG, H_IMG, CAMERA[0], CAMERA[1], EPS)
    return _cache["px"]


def coefficients():
    sh = np.random.default_rng(5).normal(size=(P, 9, 4)).astype(F)
    sh[:, 0, :3] += F(3.0)
    return sh


def volume():
    sh = coefficients()
    return lambda rec: G.sample(*GRID, sh, rec, valid=None, backface=True, blocked=None)


def continuous(px, geo, chart, sel):
    """The atlas coordinate of the pixels `sel` under `chart` in float64 from the float32 inputs, in texels with centres at
    +0.5: what step 6 computes before its - 0.5, without any of its roundings."""
    s, t = np.zeros(len(sel)), np.zeros(len(sel))
    for j, k in enumerate(sel):
        m = geo.mesh_of[int(px.inst[k])]
        a, b, c = geo.uvs[m][geo.tris[m][int(px.tri[k])]].astype(np.float64)
        u, v = float(px.uv[k, 0]), float(px.uv[k, 1])
        tu, tv = a * (1 - u - v) + b * u + c * v
        s[j], t[j] = (tu * float(F(chart.scale_u)) + float(F(chart.offset_u))) * AW, (tv * float(F(chart.scale_v)) + float(F(chart.offset_v))) * AH
    return s, t


RAMP = (0.5, 0.125, 0.0625)


def ramp_atlas(alpha):
    """rgb = (1, 2, 3) * (a + b s + c t) at the texel centres (s, t) = (i + 0.5, j + 0.5)."""
    j, i = np.mgrid[0:AH, 0:AW]
    val = RAMP[0] + RAMP[1] * (i + 0.5) + RAMP[2] * (j + 0.5)
    atlas = np.empty((AH, AW, 4), F)
    atlas[..., 0:3] = val[..., None] * np.array([1.0, 2.0, 3.0])
    atlas[..., 3] = alpha
    return atlas


def check_the_view_has_what_it_is_for(plant=None):
    px = pieces()
    seen = {int(i): int((px.inst[px.hit] == i).sum()) for i in range(5)}
    assert all(seen[i] >= 8 for i in range(5)), seen                   # every sphere, the floor and the box without texcoords
    assert (~px.hit).sum() > 50


def check_ramp(plant, alpha):
    """A ramp a + b s + c t is reproduced by a bilinear fetch inside the outer texel centres.  With M = a + b W + c H, the
    largest value of the ramp and of any partial sum (every term is positive), in units of u = 2^-24:
      the coordinate: tu's three products and two sums (5 u), the scale, the offset, the product with W, the - 0.5 (4 u),
        each relative to at most W or H texels, times the slope: no more than 9 u M;
      the texels' own rounding to f32                                                                       1 u M
      1 - fx (u), a weight's product (u), weight * rgb (u), three additions (3 u)                            6 u M
      with owned taps also cov's three additions (3 u), its weights (2 u) and the division (u)               6 u M
    22 u M to first order; the check asks for 24 u M."""
    cpu, sc, geo = scene()
    px = pieces()
    rgb, g = L.compose(px, geo, CHARTS, ramp_atlas(alpha), None, AMBIENT, plant)
    M = RAMP[0] + RAMP[1] * AW + RAMP[2] * AH
    checked = 0
    for c, chart in enumerate(CHARTS):
        sel = np.nonzero(px.hit & (px.inst == chart.instance_idx))[0]
        s, t = continuous(px, geo, chart, sel)
        inside = (s >= 0.5) & (s <= AW - 0.5) & (t >= 0.5) & (t <= AH - 0.5)
        assert inside.sum() >= 5, (c, inside.sum())
        want = (RAMP[0] + RAMP[1] * s + RAMP[2] * t)[inside, None] * np.array([1.0, 2.0, 3.0])
        k = sel[inside]
        assert np.all(words(g)[k, 18] == c) and np.all(words(g)[k, 19] == L.LIGHTMAP)
        E = (rgb[k].astype(np.float64) - px.emission[k]) / (px.color[k].astype(np.float64) * float(B.INV_PI))
        # E is recovered through step 9's three roundings: 3 u of rgb more
        assert np.all(np.abs(E - want) <= (24 + 3) * U * 3.0 * M), (c, np.abs(E - want).max())
        assert np.all(np.abs(g[k, 16] - (s[inside] - 0.5)) <= 9 * U * AW) and np.all(np.abs(g[k, 17] - (t[inside] - 0.5)) <= 9 * U * AH)
        assert np.all(g[k, 11] == F(alpha)) or alpha == 1.0 and np.all(np.abs(g[k, 11] - 1.0) <= 5 * U)
        checked += len(k)
    assert checked > 100


def check_a_ramp_atlas_is_reproduced(plant=None):
    check_ramp(plant, 1.0)


def check_without_an_owned_tap_the_plain_sum(plant=None):
    check_ramp(plant, 0.0)


def owner_plane():
    if "owner" not in _cache:
        cpu, sc, geo = scene()
        mesh_of = [int(geo.mesh_of[c.instance_idx]) for c in CHARTS]
        _cache["owner"] = lightmap_ref.raster([geo.uvs[m] for m in mesh_of], [geo.tris[m] for m in mesh_of], CHARTS, AW, AH)[0]
    return _cache["owner"]


def check_a_constant_atlas_with_black_gutters_is_constant(plant=None):
    """Owned texels hold `value`, the others zeros with alpha 0: wherever a tap is owned E is `value` -- the products (u), three
    additions (3 u), cov's additions (3 u), the division (u): 8 u relative, the weights cancelling -- at chart borders too."""
    cpu, sc, geo = scene()
    px = pieces()
    owned = owner_plane() != lightmap_ref.NO_OWNER
    assert 0.2 < owned.mean() < 0.95
    value = F([0.8, 1.7, 0.35])
    atlas = np.zeros((AH, AW, 4), F)
    atlas[owned, 0:3], atlas[owned, 3] = value, 1.0
    rgb, g = L.compose(px, geo, CHARTS, atlas, None, AMBIENT, plant)
    lm = words(g)[:, 19] == L.LIGHTMAP
    covered = lm & (g[:, 11] > 0)
    border = covered & (g[:, 11] < 0.99)
    assert covered.sum() > 200 and border.sum() > 20 and (lm & ~covered).sum() < 0.1 * lm.sum()
    E = (rgb[covered].astype(np.float64) - px.emission[covered]) / (px.color[covered].astype(np.float64) * float(B.INV_PI))
    assert np.all(np.abs(E - value) <= (8 + 3) * U * value), np.abs(E - value).max()
    assert np.all(g[lm, 11] <= 1.0 + 5 * U)


def check_huge_coordinates_clamp(plant=None):
    """Charts that throw the sample 1e30 atlases away, and one that puts it just left of column 0: the edge texel, exactly."""
    cpu, sc, geo = scene()
    px = pieces()
    atlas = np.random.default_rng(11).uniform(0.1, 2.0, (AH, AW, 4)).astype(F)
    for chart, col, row in ((api.LightmapChart(0, 0.5, 0.5, 1e30, -1e30), AW - 1, 0), (api.LightmapChart(0, 0.5, 0.5, -1e30, 1e30), 0, AH - 1)):
        rgb, g = L.compose(px, geo, [chart], atlas, None, AMBIENT, plant)
        k = px.hit & (px.inst == 0)
        assert k.sum() >= 8 and np.all(words(g)[k, 19] == L.LIGHTMAP) and np.all(np.abs(g[k, 16]) > 1e29)
        want = px.emission[k] + (px.color[k] * atlas[row, col, 0:3]) * B.INV_PI
        assert np.array_equal(words(rgb[k]), words(want)) and np.all(g[k, 11] == 1.0)
    columns = np.broadcast_to(np.arange(1, AW + 1, dtype=F)[None, :, None], (AH, AW, 4)).copy()
    rgb, g = L.compose(px, geo, [api.LightmapChart(0, 0.05, 0.5, -0.02, 0.2)], columns, None, AMBIENT, plant)
    k = px.hit & (px.inst == 0) & (g[:, 16] < 0)
    assert k.sum() >= 8
    assert np.array_equal(words(rgb[k]), words(px.emission[k] + (px.color[k] * F(1.0)) * B.INV_PI))


def check_coordinates_that_are_not_finite_are_uncharted(plant=None):
    cpu, sc, geo = scene()
    px = pieces()
    atlas = ramp_atlas(1.0)
    nan_geo = SimpleNamespace(mesh_of=geo.mesh_of, tris=geo.tris, uvs=[None if uv is None else np.full_like(uv, np.nan) for uv in geo.uvs])
    overflow = [api.LightmapChart(c.instance_idx, 3e38, 3e38, 0.0, 0.0) for c in CHARTS]
    _, base = B.compose(px, volume(), AMBIENT)
    for geo_k, charts in ((nan_geo, CHARTS), (geo, overflow)):
        rgb, g = L.compose(px, geo_k, charts, atlas, volume(), AMBIENT, plant)
        h = px.hit
        assert np.all(words(g)[h, 18] == 0xFFFFFFFF) and not g[:, 16:18].any() and np.all(np.isin(words(g)[h, 19], (L.PROBES, L.AMBIENT)))
        assert np.array_equal(words(g[:, 0:16]), words(base))
        assert np.array_equal(words(rgb), words(B.compose(px, volume(), AMBIENT)[0]))


def check_the_first_chart_that_names_an_instance_is_its_chart(plant=None):
    cpu, sc, geo = scene()
    px = pieces()
    twice = [THREE_CHARTS[0], api.LightmapChart(0, 0.3, 0.2, 0.6, 0.7), THREE_CHARTS[1]]
    atlas = ramp_atlas(1.0)
    rgb, g = L.compose(px, geo, twice, atlas, None, AMBIENT, plant)
    k = px.hit & (px.inst == 0)
    assert k.sum() >= 8 and np.all(words(g)[k, 18] == 0)
    alone = L.compose(px, geo, [THREE_CHARTS[0]], atlas, None, AMBIENT)
    assert np.array_equal(words(g[k]), words(alone[1][k])) and np.array_equal(words(rgb[k]), words(alone[0][k]))
    assert np.all(words(g)[px.hit & (px.inst == 1), 18] == 2)


def check_an_instance_without_a_chart_takes_probes_or_ambient(plant=None):
    cpu, sc, geo = scene()
    px = pieces()
    atlas = ramp_atlas(1.0)
    box = px.hit & (px.inst == 4)                                       # the box without texcoords: no chart can name it
    rgb, g = L.compose(px, geo, CHARTS, atlas, volume(), AMBIENT, plant)
    base_rgb, base_g = B.compose(px, volume(), AMBIENT)
    answered = box & (base_g[:, 11] > 0)
    assert answered.sum() >= 8
    assert np.all(words(g)[answered, 19] == L.PROBES) and np.all(words(g)[box & ~answered, 19] == L.AMBIENT)
    assert np.array_equal(words(rgb[box]), words(base_rgb[box])) and np.array_equal(words(g[box, 0:16]), words(base_g[box]))
    assert np.all(words(g)[box, 18] == 0xFFFFFFFF) and not g[box, 16:18].any()
    # without a volume: ambient, and no lookup is asked
    rgb, g = L.compose(px, geo, CHARTS, atlas, None, AMBIENT, plant)
    assert np.all(words(g)[box, 19] == L.AMBIENT) and np.all(g[box, 11] == 0)
    assert np.array_equal(words(rgb[box]), words(px.emission[box] + (px.color[box] * AMBIENT) * B.INV_PI))
    # a miss
    m = ~px.hit
    assert np.array_equal(words(rgb[m]), words(px.env[m])) and np.all(words(g)[m, 19] == L.MISS) and np.all(words(g)[m, 18] == 0xFFFFFFFF)


def check_no_charts_and_a_volume_is_the_baked_view(plant=None):
    cpu, sc, geo = scene()
    px = pieces()
    rgb, g = L.compose(px, geo, [], ramp_atlas(1.0), volume(), AMBIENT, plant)
    base_rgb, base_g = B.compose(px, volume(), AMBIENT)
    assert np.array_equal(words(rgb), words(base_rgb)) and np.array_equal(words(g[:, 0:16]), words(base_g))
    assert (base_g[:, 11] > 0).sum() > 100
    for mode in (B.film_ref.RTZ, B.film_ref.RNE):
        assert np.array_equal(L.render(px, geo, [], ramp_atlas(1.0), volume(), AMBIENT, mode, plant)[0], B.render(px, volume(), AMBIENT, mode)[0])


def check_texcoords_word_for_word(plant=None):
    """tu = (a w + b u) + c v with every product rounded: the G-buffer's x against the same sum made of float64 products
    rounded to float32 one by one."""
    cpu, sc, geo = scene()
    px = pieces()
    chart = api.LightmapChart(2, 0.9, 0.45, 0.05, 0.53)
    _, g = L.compose(px, geo, [chart], ramp_atlas(1.0), None, AMBIENT, plant)
    sel = np.nonzero(px.hit & (px.inst == 2))[0]
    assert len(sel) >= 30
    r = lambda x: np.float64(F(x))
    want, fused = [], []
    for k in sel:
        m = geo.mesh_of[2]
        a, b, c = geo.uvs[m][geo.tris[m][int(px.tri[k])]].astype(np.float64)
        u, v = np.float64(px.uv[k, 0]), np.float64(px.uv[k, 1])
        w = r(r(1.0 - u) - v)
        tu = r(r(r(a[0] * w) + r(b[0] * u)) + r(c[0] * v))
        want.append(F(r(r(r(tu * r(chart.scale_u)) + r(chart.offset_u)) * AW) - 0.5))
        fused.append(F(r(r(r(r(a[0] * w + b[0] * u + c[0] * v) * r(chart.scale_u)) + r(chart.offset_u)) * AW) - 0.5))
    assert (words(F(want)) != words(F(fused))).any()                                # the two differ on these hits
    assert np.array_equal(words(g[sel, 16]), words(F(want)))


CHECKS = [check_the_view_has_what_it_is_for, check_a_ramp_atlas_is_reproduced, check_without_an_owned_tap_the_plain_sum,
          check_a_constant_atlas_with_black_gutters_is_constant, check_huge_coordinates_clamp, check_coordinates_that_are_not_finite_are_uncharted,
          check_the_first_chart_that_names_an_instance_is_its_chart, check_an_instance_without_a_chart_takes_probes_or_ambient,
          check_no_charts_and_a_volume_is_the_baked_view, check_texcoords_word_for_word]


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__)
def test_contract(built, check):
    check()


@pytest.mark.parametrize("plant", L.PLANTS)
def test_every_planted_misreading_fails_a_check(built, plant):
    failed = []
    for check in CHECKS:
        try:
            check(plant)
        except AssertionError:
            failed.append(check.__name__)
    assert failed, plant


def test_no_device_is_an_error_not_a_fallback(built):
    cpu, sc, geo = scene()
    target = type("T", (), {"format": lambda self: "Rgba16Float", "width": 4, "height": 4, "handle": None})()
    with pytest.raises(api.LupinError) as e:
        api.render_lightmapped(None, sc, target, CAMERA[0], CAMERA[1], CHARTS, ramp_atlas(1.0))
    assert e.value.code == -2 and "render_lightmapped" in str(e.value)
    if api.device_count() == 0:
        with pytest.raises(api.LupinError) as e:
            api.Context(0)
        assert e.value.code == -2
