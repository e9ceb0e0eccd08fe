"""The integrators' path loop against the float64 path tracer of tests/path_ref.py, on the CPU: the oracle inside
the measured bounds, the conditions on the reference alone, the prefix property, every planted twin rejected, closed forms
that do not depend on the reading of the shader, and light_ref.sample against true_density."""
import math

import numpy as np
import pytest

from lupinpathtracer_amd import api
from tests import light_ref as L
from tests import path_ref as R

PT = api.PathtraceType
VARIANTS = ("const", "textured")
_oracle = {}


def oracle_colours(c, integ, rung, max_radiance):
    """The oracle's value per record: one sample per pixel of the camera the records were taken from, f32."""
    from oracle import oracle
    key = (c.variant, int(integ), rung, max_radiance)
    if key not in _oracle:
        adv = api.AdvancedParams(max_radiance=max_radiance, ray_epsilon=R.EPS)
        _, _, rgb = oracle.pathtrace(c.scene, R.CAM_W, R.CAM_H, R.CAMERA, R.camera_transform(), rung, 1, int(integ), accum_counter=0,
                                     want_f32=True, advanced=adv)
        _oracle[key] = rgb.reshape(-1, 3).copy()
    return _oracle[key]


def worst_deviation(c, tr, rung):
    worst = 0.0
    for mr in (R.NO_CLAMP, R.CLAMP):
        clamped, _, dec = tr.at(rung, mr)
        worst = max(worst, float(R.deviation(oracle_colours(c, tr.integ, rung, mr), clamped)[dec].max()))
    return worst


@pytest.mark.parametrize("integ", R.INTEGRATORS, ids=lambda t: t.name)
@pytest.mark.parametrize("variant", VARIANTS)
def test_oracle_agrees_with_the_float64_paths(built, variant, integ):
    c = R.case(variant)
    tr = R.cached_trace(c, integ)
    for rung in R.LADDER:
        print(f"{variant} {integ.name} rung {rung}: worst deviation {worst_deviation(c, tr, rung):.3e}, bound {R.bound(integ, rung):.3e}, "
              f"excluded {1.0 - tr.vertex(rung)['decisive'].mean():.4f}")
    for mr in (R.NO_CLAMP, R.CLAMP):
        got = {rung: oracle_colours(c, integ, rung, mr) for rung in R.LADDER}
        assert R.first_failing_rung(tr, got, mr) is None, R.first_failing_rung(tr, got, mr)


def test_measured_deviation_is_the_recorded_one(built):
    """MEASURED is what this measurement gives, so BOUND is four times a measurement.  The band is a factor of two below the
    figure written down: another host compiler or libm moves the oracle's last bits, and with them the worst of a finite
    sample, without anything being wrong; above the figure the bound would no longer be four times what is measured."""
    for integ in R.INTEGRATORS:
        for rung in R.LADDER:
            worst = max(worst_deviation(R.case(v), R.cached_trace(R.case(v), integ), rung) for v in VARIANTS)
            print(f'MEASURED {integ.name} {rung}: {worst:.3e}')
            assert R.MEASURED[integ.name][rung] / 2.0 <= worst <= R.MEASURED[integ.name][rung] * 1.0005, (integ.name, rung, worst)


CAN_PRODUCE = {PT.Standard: ("miss", "surface, BSDF turn", "surface, light turn", "delta", "medium scatter"),
               PT.MIS: ("miss", "surface, BSDF turn", "delta", "medium scatter"),
               PT.Naive: ("miss", "surface, BSDF turn", "delta", "medium scatter"),
               PT.Direct: ("miss", "surface, BSDF turn", "surface, light turn", "delta", "medium scatter")}


@pytest.mark.parametrize("integ", R.INTEGRATORS, ids=lambda t: t.name)
@pytest.mark.parametrize("variant", VARIANTS)
def test_conditions_hold_on_the_reference_alone(built, variant, integ):
    cond = R.conditions(R.cached_trace(R.case(variant), integ))
    print(variant, integ.name, cond)
    for rung, share in cond["excluded"].items():
        assert share <= R.MAX_EXCLUDED, (rung, share)
    for name in CAN_PRODUCE[integ]:
        assert cond["kinds"][name] >= 200, (name, cond["kinds"][name])
    assert cond["opacity skip"] >= 200
    assert cond["ends"]["ended by roulette"] >= 200
    assert cond["ends"]["ended by a zero or non-finite weight"] >= 200
    assert cond["roulette survived"] >= 100
    assert cond["clamp scaled"] >= 100 and cond["clamp non-finite"] >= 100      # both branches of clamp_radiance


@pytest.mark.parametrize("integ", R.INTEGRATORS, ids=lambda t: t.name)
def test_prefix_property(built, integ):
    """A path with max_bounces = B is the first B + 1 vertices of the same path with a larger B: in the reference (a run to B
    equals the truncated run to 8, exactly) and in the oracle (every rung of one run to 8 agrees with the oracle's own run to
    that rung, which test_oracle_agrees asserts through `at`)."""
    c = R.case("const")
    sel = slice(0, 4096, 9)
    long = R.trace(c, integ, 8, sel=sel)
    for rung in (0, 2, 4):
        short = R.trace(c, integ, rung, sel=sel)
        a, b = short.at(rung), long.at(rung)
        assert np.array_equal(a[1], b[1], equal_nan=True) and np.array_equal(a[2], b[2])
        assert np.array_equal(short.log[-1]["rng"], long.log[rung]["rng"])


APPLIES = {"balance_heuristic": (PT.MIS,), "mis_no_pdf_divide": (PT.MIS,), "mis_keeps_next_emission": (PT.MIS,),
           "direct_keeps_next_emission": (PT.Direct,), "direct_emission_always": (PT.Direct,),
           "mixture_half_bsdf_only": (PT.Standard, PT.Direct)}


TWINS = [(d, t) for d in R.DEFECTS for t in APPLIES.get(d, R.INTEGRATORS)]


@pytest.mark.parametrize("defect,integ", TWINS, ids=[f"{d}-{t.name}" for d, t in TWINS])
def test_every_twin_is_rejected(built, defect, integ):
    """failures() on the oracle's values, with the bounds above, rejects a reference with one misreading planted, under
    every integrator the misreading applies to."""
    c = R.case("const")
    twin = R.trace(c, integ, defect=defect)
    mr = R.CLAMP if defect == "clamp_per_channel" else R.NO_CLAMP
    got = {rung: oracle_colours(c, integ, rung, mr) for rung in R.LADDER}
    found = R.first_failing_rung(twin, got, mr)
    assert found is not None, defect
    print(defect, "rejected at rung", found[0], "-", found[1][0][:200])


# ---- closed forms ---------------------------------------------------------------------------------------------------------

def test_constant_environment_seen_directly_returns_itself(built):
    c = R.case("const")
    for integ in R.INTEGRATORS:
        tr = R.cached_trace(c, integ)
        e = tr.log[0]
        seen = (e["kind"] == R.MISS) & (e["skips"] == 0)
        assert seen.sum() > 100
        assert np.allclose(e["radiance"][seen], np.asarray(c.cpu.environments[0]["emission"], np.float64)[:3], rtol=0, atol=0)


def test_integrators_agree_in_the_mean(built):
    """Unclamped radiance at max_bounces 8: Standard, Naive and Direct estimate the same integral (up to the bias of the
    truncation, which they share), so their means over the records agree within four combined standard errors.  MIS is
    compared where its environment double count (Q1) does not act: test_floor_under_a_square_emitter, a scene without an
    environment.  (Paths that collect the infinite emitter are left out of every mean: the same records, by position.)"""
    c = R.case("const")
    raws = {integ: R.cached_trace(c, integ).at(8)[1].mean(-1) for integ in (PT.Standard, PT.Naive, PT.Direct)}
    mean, se = {}, {}
    for integ, raw in raws.items():
        raw = raw[np.isfinite(raw)]
        mean[integ], se[integ] = raw.mean(), raw.std(ddof=1) / math.sqrt(len(raw))
    for a, b in ((PT.Standard, PT.Naive), (PT.Standard, PT.Direct), (PT.Naive, PT.Direct)):
        print(a.name, b.name, mean[a], mean[b], math.hypot(se[a], se[b]))
        assert abs(mean[a] - mean[b]) <= 4.0 * math.hypot(se[a], se[b]), (a.name, b.name, mean[a], mean[b])


def test_white_furnace(built):
    """The values tests/test_pins.py derives, on path_ref itself: inside a constant environment E a matte surface of albedo 1
    returns E (Naive: on every path, its weight is exactly bsdfcos / pdf = 1; Standard and Direct: in the mean), MIS returns
    2 E in the mean (Q1), and a smooth transparent sheet of colour 1 returns E on every path under all four (a delta vertex
    takes no shadow rays and keeps next_emission)."""
    c = R.case("furnace")
    E, n = R.FURNACE_E, R.FURNACE_N
    for integ in R.INTEGRATORS:
        raw = R.cached_trace(c, integ).at(8)[1]
        assert np.allclose(raw[n:], E, rtol=1e-12, atol=0), integ.name
        matte = raw[:n].mean(-1)
        want = 2.0 * E if integ == PT.MIS else E
        if integ == PT.Naive:
            assert np.allclose(raw[:n], E, rtol=1e-12, atol=0)
        se = matte.std(ddof=1) / math.sqrt(n)
        print(integ.name, matte.mean(), want, se)
        assert abs(matte.mean() - want) <= 4.0 * se + 1e-12, (integ.name, matte.mean(), want, se)
    # a twin: the environment gated by next_emission in MIS (textbook MIS) would return E, and must not pass as 2 E
    assert abs(E - 2.0 * E) > 4.0 * se


def test_floor_under_a_square_emitter(built):
    """The radiance leaving a matte floor under a square emitter is albedo x L x the float64 form factor of
    tests/test_gpu_lightmap.py, for all four integrators (no environment: MIS is comparable), within four standard errors of
    the float64 mean; and the four agree pairwise."""
    from tests.test_gpu_lightmap import form_factor
    c = R.case("emitter")
    stats = {}
    for integ in R.INTEGRATORS:
        raw = R.cached_trace(c, integ).at(8)[1].mean(-1)
        for k, p in enumerate(R.EMITTER_POINTS):
            x = raw[k * R.EMITTER_N:(k + 1) * R.EMITTER_N]
            want = R.EMITTER_ALBEDO * R.EMITTER_L * form_factor(p)
            se = x.std(ddof=1) / math.sqrt(len(x))
            print(integ.name, p, x.mean(), want, se)
            assert se > 0 and abs(x.mean() - want) <= 4.0 * se, (integ.name, p, x.mean(), want, se)
            stats[(integ, k)] = (x.mean(), se)
    for k in range(len(R.EMITTER_POINTS)):
        for a in R.INTEGRATORS:
            for b in R.INTEGRATORS:
                assert abs(stats[(a, k)][0] - stats[(b, k)][0]) <= 4.0 * math.hypot(stats[(a, k)][1], stats[(b, k)][1]), (a.name, b.name, k)


def test_light_sample_agrees_with_true_density(built):
    """Histogram of light_ref.sample's directions over the slots: a direction crosses the triangle it was aimed at, so the
    count of samples crossing slot T of a light is binomial with p = (realised alias probability of T + the uniform
    environment's share, solid angle / 4 pi) / (lights + environments) -- what true_density integrates to over T.  Within five
    standard deviations, plus the share of samples that cross two emitters at once (counted, below 2 %)."""
    c = R.case("const")
    n = 60000
    state = api.rng_seed_for(np.arange(n, dtype=np.uint32), 7)
    pos = np.tile(np.array([[0.2, 0.1, 0.4]]), (n, 1))
    d, after, margin = L.sample(c.lights, pos, state)
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-12) and (margin > 1.0).mean() > 0.999
    ntot = c.lights.n
    crossed = []
    for light in c.lights.lights:
        rows = []
        for a in range(0, n, 5000):
            s_, u_, v_ = L.crossings(pos[a:a + 5000], d[a:a + 5000], light.tris_world)
            with np.errstate(invalid="ignore"):
                rows.append(np.isfinite(s_) & (s_ > 0) & (np.minimum(u_, v_) >= -1e-9) & (u_ + v_ <= 1 + 1e-9))
        crossed.append(np.concatenate(rows))
    multi = np.concatenate(crossed, 1).sum(1) > 1
    assert multi.mean() < 0.02
    checked = 0
    for light, cr in zip(c.lights.lights, crossed):
        real = L.alias_realised(light.bins)
        for t in range(len(light.tris_world)):
            omega = L.solid_angle(pos[0], light.tris_world[t:t + 1])
            p = (real[t] + sum(1 for e in c.lights.envs if e.weights is None) * omega / (4 * math.pi)) / ntot
            k = int(cr[:, t].sum())
            sd = math.sqrt(n * p * (1 - p))
            assert abs(k - n * p) <= 5 * sd + multi.sum(), (light.instance_idx, t, k, n * p, sd)
            checked += 1
    assert checked >= 6
    # the density itself: over the samples that land on a mesh, E[1 / true_density] is the solid angle of the meshes' union
    dens = L.true_density(c.lights, pos, d)
    on = np.concatenate(crossed, 1).any(1)
    union = float(np.mean(np.where(on, 1.0 / dens, 0.0)))
    total = sum(L.solid_angle(pos[0], light.tris_world) for light in c.lights.lights)
    assert union <= total * 1.02 and union >= total * 0.9, (union, total)
