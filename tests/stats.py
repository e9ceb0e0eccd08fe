"""Statistics shared by the probe tests (test_scatter_probe.py, test_light_probe.py): a chi-square survival function
without scipy, the pooled chi-square, and an equal-area sphere grid with its quadrature."""
import math

import numpy as np

# ---- chi-square without scipy ---------------------------------------------------------------------------------------

def chi2_sf(x, k):
    """P(X > x) for X ~ chi-square with k degrees of freedom: the regularised upper incomplete gamma Q(k/2, x/2)
    (series below a + 1, Lentz continued fraction above)."""
    a, x = 0.5 * k, 0.5 * x
    if x <= 0.0:
        return 1.0
    lg = a * math.log(x) - x - math.lgamma(a)
    if x < a + 1.0:
        term = s = 1.0 / a
        ap = a
        for _ in range(10000):
            ap += 1.0
            term *= x / ap
            s += term
            if abs(term) < abs(s) * 1e-15:
                break
        return max(0.0, 1.0 - s * math.exp(lg))
    b, c, d = x + 1.0 - a, 1e300, 1.0 / (x + 1.0 - a)
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = 1e-300 if abs(d) < 1e-300 else d
        c = b + an / c
        c = 1e-300 if abs(c) < 1e-300 else c
        d = 1.0 / d
        h *= d * c
        if abs(d * c - 1.0) < 1e-15:
            break
    return math.exp(lg) * h


def chi2_pooled(obs, exp, min_expected=5.0):
    """Chi-square of observed vs expected counts with the bins expected below `min_expected` pooled into one."""
    obs, exp = np.asarray(obs, np.float64), np.asarray(exp, np.float64)
    low = exp < min_expected
    o = np.append(obs[~low], obs[low].sum())
    e = np.append(exp[~low], exp[low].sum())
    if e[-1] == 0.0:
        assert o[-1] == 0.0, "samples where the pdf integrates to zero"
        o, e = o[:-1], e[:-1]
    stat = float(np.sum((o - e) ** 2 / e))
    dof = len(o) - 1
    return stat, dof, chi2_sf(stat, dof)


# ---- equal-area sphere grid around +z -------------------------------------------------------------------------------

NC, NPHI, SUB = 24, 24, 6          # cos(theta) bands per hemisphere, phi sectors, sub-samples per bin edge


def sphere_bin(d):
    """Bin of direction d: 2 NC bands equal in cos(theta) over [-1, 1], NPHI equal sectors in phi."""
    c = np.clip(d[:, 2], -1.0, 1.0 - 1e-12)
    ci = np.clip(((c + 1.0) * NC).astype(np.int64), 0, 2 * NC - 1)
    phi = np.arctan2(d[:, 1], d[:, 0]) % (2 * math.pi)
    pi_ = np.clip((phi / (2 * math.pi) * NPHI).astype(np.int64), 0, NPHI - 1)
    return ci * NPHI + pi_


def sphere_quadrature(SUB=SUB):
    """Midpoints of SUB x SUB equal-area sub-cells of every bin, the bin of each, and the solid angle of one."""
    ci, pi_, si, sj = np.meshgrid(np.arange(2 * NC), np.arange(NPHI), np.arange(SUB), np.arange(SUB), indexing="ij")
    c = -1.0 + (ci + (si + 0.5) / SUB) / NC
    phi = (pi_ + (sj + 0.5) / SUB) * 2 * math.pi / NPHI
    s = np.sqrt(1.0 - c * c)
    d = np.stack([s * np.cos(phi), s * np.sin(phi), c], -1).reshape(-1, 3)
    return d, (ci * NPHI + pi_).reshape(-1), 4 * math.pi / (2 * NC * NPHI * SUB * SUB)
