"""float64 judgement of occlusion queries, built on the brute-force intersector of tests/closest_hit_ref.py:
every triangle of every instance, no hierarchy, nothing shared with the traversal.

A segment (o, d, ray_epsilon, tmax) is blocked iff some triangle is hit at ray_epsilon <= t < tmax.  What an f32 any-hit
traversal must answer follows from a ray's reference Hits only where no f32 evaluation could plausibly differ:

  a decisive miss          0 for any tmax
  a decisive hit at t      0 for tmax = 0.5 t and 1 for tmax = 2 t.  Every possible rival of a decisive hit has t_lo beyond
                           t (1 + s) + tol_t, so nothing can report below 0.5 t; the winner reports within tol_t of t, below
                           2 t, provided tol_t < 0.25 t (asserted in judgement)
  everything else          left out (-1)

Also here: the float64 evaluation of the definition itself (blocked_f64; the planted twins of tests/test_occlusion_cpu.py are
variants of it), the choice of rays an occlusion record can carry, and the closed form of the ambient-occlusion test."""
import math

import numpy as np

from tests import closest_hit_ref as X

UNIT_TOLERANCE = 1e-4          # LP_RAY_UNIT_TOLERANCE: | |d|^2 - 1 | a record's direction may have
MISS_TMAX = 1.0e3              # the tmax a decisive miss is queried with, times the scale: any value will do
NOT_UNIT_FAMILIES = ("in_plane", "short", "long")   # closest_hit_ref's families whose directions are not of unit length


def unit_directions(dir_):
    """Which f32 directions an occlusion record accepts: the library's rule, in f32."""
    d = np.asarray(dir_, np.float32)
    off = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) - np.float32(1.0)
    return np.abs(off) <= np.float32(UNIT_TOLERANCE)


def usable(c):
    """The rays of a closest_hit_ref.Case an occlusion record can carry: all of every family but NOT_UNIT_FAMILIES."""
    keep = unit_directions(c.dir)
    fam = np.array(X.FAMILIES)[c.family]
    assert keep[~np.isin(fam, NOT_UNIT_FAMILIES)].all()
    return keep


def judgement(ref, scale):
    """(tmax (N,) float32, expected (N,) int: 0 | 1 | -1 = left out) for the rays of `ref` (Hits) at tmax = scale * t;
    scale is 0.5 or 2."""
    assert scale in (0.5, 2.0)
    hit, miss = ref.decisive & ref.hit, ref.decisive & ~ref.hit
    assert np.all(ref.tol_t[hit] < 0.25 * ref.t[hit])
    tmax = np.where(hit, scale * np.where(hit, ref.t, 0.0), scale * MISS_TMAX).astype(np.float32)
    expected = np.full(len(ref.hit), -1)
    expected[miss] = 0
    expected[hit] = 1 if scale > 1.0 else 0
    return tmax, expected


def disagreements(expected, got):
    """Judged rays whose answer is not the expected one."""
    judged = expected >= 0
    return int((judged & (np.asarray(got).astype(int) != expected)).sum())


def report(ref, query):
    """The figures the tests assert, for `query(tmax) -> blocked (N,)` over the rays of `ref` at both scales."""
    rep = dict(rays=len(ref.hit), judged_hits=int((ref.decisive & ref.hit).sum()), judged_misses=int((ref.decisive & ~ref.hit).sum()),
               left_out_share=float(1.0 - ref.decisive.mean()), disagree=0)
    for scale in (0.5, 2.0):
        tmax, expected = judgement(ref, scale)
        bad = disagreements(expected, query(tmax))
        rep[f"disagree_{scale}"] = bad
        rep["disagree"] += bad
    rep["per_instance"] = np.bincount(ref.inst[ref.decisive & ref.hit], minlength=int(ref.inst.max()) + 1)
    return rep


def blocked_f64(g, ori, dir_, ray_epsilon, tmax, inclusive=False):
    """The definition in float64: some triangle with ray_epsilon <= t < tmax (inclusive: t <= tmax, the twin).  The nearest
    accepted triangle decides: min t < tmax."""
    h = X.closest_hits(g, ori, dir_, ray_epsilon)
    tmax = np.broadcast_to(np.asarray(tmax, np.float64), h.t.shape)
    return h.hit & ((h.t <= tmax) if inclusive else (h.t < tmax))


# ---- the closed form: a point on a floor under a ceiling at height h, directions cosine-weighted about the normal ----

def ceiling_blocked_fraction(h, radius):
    """A direction at polar angle a meets the ceiling at h / cos a, within `radius` iff cos a > h / radius; the
    cosine-weighted measure of that cap is 1 - (h / radius)^2 (0 for radius <= h)."""
    return max(0.0, 1.0 - (h / radius) ** 2)


def ceiling_blocked_fraction_uniform_twin(h, radius):
    """What uniform-hemisphere weighting would give: 1 - h / radius."""
    return max(0.0, 1.0 - h / radius)


def binomial_sigma(p, samples):
    return math.sqrt(p * (1.0 - p) / samples)
