"""numpy float32 restatement of the lightmap denoiser (lupin_hip_denoise_lightmap, include/lupin_hip.h,
lupinpathtracer_amd/csrc/lupin_lightmap_denoise.hpp).

`denoise(rgba, records, ...)` follows the kernels operation for operation: the same sums in the same order (dy outer, dx
inner), every operation one rounded f32 operation, the exponential of tests/denoise_ref.py (dn_exp_neg) and the gutter rule
of tests/lightmap_ref.py (k_lm_dilate).  `defects` plants one of three mistakes, for the tests that must notice them:
"no_footprint" (the distance test is dropped), "no_normal" (w_n = 1), "unguided_taps" (a tap need not be guided).
The second half builds the synthetic atlases the CPU and the GPU tests share.
"""
import numpy as np

from tests import lightmap_ref
from tests.denoise_ref import H_B3, _shift, exp_neg

F = np.float32
UNIT_TOLERANCE = F(1e-4)   # LP_RAY_UNIT_TOLERANCE


def lum(v):
    return (F(0.2126) * v[..., 0] + F(0.7152) * v[..., 1]) + F(0.0722) * v[..., 2]


def guided(rgba, records):
    """Owned (alpha != 0), position and normal finite, | |n|^2 - 1 | <= 1e-4."""
    x, n = records[..., 0:3], records[..., 4:7]
    with np.errstate(all="ignore"):
        off = ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]) - F(1)
    return (rgba[..., 3] != 0) & np.isfinite(x).all(axis=-1) & np.isfinite(n).all(axis=-1) & (off <= UNIT_TOLERANCE) & (off >= -UNIT_TOLERANCE)


def _dist2(xq, x):
    e = xq - x
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def prep(rgba, records):
    """(c (H, W, 3), var_0 (H, W), guided (H, W), footprint (H, W))."""
    rgba, records = np.asarray(rgba, F), np.asarray(records, F)
    H, W = rgba.shape[:2]
    c = np.where(np.isfinite(rgba[..., :3]), rgba[..., :3], F(0))
    g = guided(rgba, records)
    x = records[..., 0:3]
    l0 = lum(c)
    s1, s2, cnt = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W), F)
    foot, has = np.zeros((H, W), F), np.zeros((H, W), bool)
    with np.errstate(all="ignore"):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                lq, m = _shift(l0, dy, dx)
                gq, _ = _shift(g, dy, dx)
                m = m & gq
                s1 = np.where(m, s1 + lq, s1)
                s2 = np.where(m, s2 + lq * lq, s2)
                cnt = np.where(m, cnt + F(1), cnt)
                if (dx == 0) != (dy == 0):      # a 4-neighbour
                    xq, _ = _shift(x, dy, dx)
                    d2 = _dist2(xq, x)
                    foot = np.where(m, np.where(has, np.minimum(foot, d2), d2), foot)
                    has = has | m
        mean = s1 / cnt
        var = np.maximum(s2 / cnt - mean * mean, F(0))
    return c, np.where(g, var, F(0)).astype(F), g, np.where(g, foot, F(0)).astype(F)


def filter_pass(c, var, g, records, foot, i, normal_squarings, max_stretch, defects=()):
    """Pass i (step 2^i) over (c, var): the next (c, var)."""
    H, W = g.shape
    step = 1 << i
    x, n = records[..., 0:3], records[..., 4:7]
    stretch = (F(max_stretch) * F(max_stretch)) * F(step * step)      # K_i
    with np.errstate(all="ignore"):
        lp = lum(c)
        inv_sig = F(1) / (F(4) * np.sqrt(var) + F(1e-4))
        wsum, w2v, acc = np.zeros((H, W), F), np.zeros((H, W), F), np.zeros((H, W, 3), F)
        for ky in range(5):
            for kx in range(5):
                oy, ox = (ky - 2) * step, (kx - 2) * step
                cq, m = _shift(c, oy, ox)
                vq, _ = _shift(var, oy, ox)
                xq, _ = _shift(x, oy, ox)
                nq, _ = _shift(n, oy, ox)
                if "unguided_taps" not in defects:
                    gq, _ = _shift(g, oy, ox)
                    m = m & gq
                if (kx != 2 or ky != 2) and "no_footprint" not in defects:
                    limit = (stretch * F((kx - 2) * (kx - 2) + (ky - 2) * (ky - 2))) * foot
                    m = m & (_dist2(xq, x) <= limit)
                t = np.maximum((n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2], F(0))
                for _k in range(int(normal_squarings)):
                    t = t * t
                if "no_normal" in defects:
                    t = np.ones((H, W), F)
                dl = np.abs(lp - lum(cq))
                w = ((F(H_B3[kx]) * F(H_B3[ky])) * t) * exp_neg(-(dl * inv_sig))
                wsum = np.where(m, wsum + w, wsum)
                acc = np.where(m[..., None], acc + w[..., None] * cq, acc)
                w2v = np.where(m, w2v + (w * w) * vq, w2v)
        c2 = acc / wsum[..., None]
        v2 = w2v / (wsum * wsum)
    return np.where(g[..., None], c2, c).astype(F), np.where(g, v2, var).astype(F)


def denoise(rgba, records, passes=5, normal_squarings=5, max_stretch=4.0, dilate=0, defects=()):
    """What lupin_hip_denoise_lightmap writes to out_rgba: (H, W, 4) float32."""
    rgba, records = np.ascontiguousarray(rgba, F), np.ascontiguousarray(records, F)
    c, var, g, foot = prep(rgba, records)
    for i in range(int(passes)):
        c, var = filter_pass(c, var, g, records, foot, i, normal_squarings, max_stretch, defects)
    owned = rgba[..., 3] != 0
    out = rgba.copy()                       # texels that are not owned: the input as it is; alpha: the input's
    out[owned, :3] = c[owned]
    if dilate:
        start = np.zeros_like(rgba)
        start[owned, :3] = c[owned]
        start[owned, 3] = 1                 # the owned texels count as filled, nothing else does
        out[~owned] = lightmap_ref.dilate(start, int(dilate))[~owned]
    return out


# ---- synthetic atlases ----

def plane_records(H, W, origin=(0.0, 0.0, 0.0), du=(1.0, 0.0, 0.0), dv=(0.0, 1.0, 0.0), normal=(0.0, 0.0, 1.0)):
    """Records of a chart that maps texel (x, y) to origin + (x + 0.5) du + (y + 0.5) dv, with a constant normal."""
    ys, xs = np.mgrid[0:H, 0:W]
    rec = np.zeros((H, W, 8), F)
    rec[..., 0:3] = (np.asarray(origin, np.float64) + (xs[..., None] + 0.5) * np.asarray(du, np.float64)
                     + (ys[..., None] + 0.5) * np.asarray(dv, np.float64)).astype(F)
    rec[..., 4:7] = F(normal)
    rec.view(np.uint32)[..., 7] = 1
    return rec


def constant_atlas(H, W, value):
    a = np.empty((H, W, 4), F)
    a[..., :3] = F(value)
    a[..., 3] = 1
    return a


def two_charts():
    """16 x 8: two flat charts of constant 1.0 and 4.0, side by side in the atlas and 100 units apart in space."""
    rgba = constant_atlas(8, 16, 1.0)
    rgba[:, 8:, :3] = 4.0
    rec = plane_records(8, 16)
    rec[:, 8:, 0] += F(100)
    return rgba, rec


def folded_chart():
    """16 x 8: one chart over two planes at 90 degrees (the fold runs between columns 7 and 8), holding 1.0 and 4.0."""
    rgba = constant_atlas(8, 16, 1.0)
    rgba[:, 8:, :3] = 4.0
    rec = plane_records(8, 16)
    rec[:, 8:] = plane_records(8, 8, origin=(8.0, 0.0, 0.0), du=(0.0, 0.0, 1.0), normal=(-1.0, 0.0, 0.0))
    return rgba, rec


def chart_with_a_hole(value=2.0):
    """16 x 16 of a constant with a 3 x 3 hole: alpha 0, rgb 0 -- and records that look as good as their neighbours', which
    nobody may read."""
    rgba = constant_atlas(16, 16, value)
    rgba[6:9, 5:8] = 0
    return rgba, plane_records(16, 16)


def noisy_atlas(H, W, seed):
    """Two noisy charts side by side (the right one tilted and 50 units away), a hole, a gutter column and gutter rows of
    alpha 0 (some holding leftovers), one owned texel with a normal of length 0.9 and one with a NaN position (both not
    guided), one guided texel with a NaN colour component."""
    rng = np.random.default_rng(seed)
    half = W // 2
    rgba = np.empty((H, W, 4), F)
    rgba[..., :3] = (1.0 + 0.5 * rng.random((H, W, 3))).astype(F)
    rgba[:, half:, :3] += F(1.5)
    rgba[..., 3] = 1
    rec = plane_records(H, W, du=(0.25, 0.0, 0.0), dv=(0.0, 0.25, 0.0))
    c, s = np.cos(0.4), np.sin(0.4)
    rec[:, half:] = plane_records(H, W - half, origin=(50.0, 0.0, 0.0), du=(0.25 * c, 0.0, 0.25 * s), dv=(0.0, 0.25, 0.0), normal=(-s, 0.0, c))
    rec[..., 4:7] /= np.sqrt((rec[..., 4:7].astype(np.float64) ** 2).sum(axis=-1, keepdims=True)).astype(F)
    rgba[:, half - 1] = 0                                   # the gutter between the charts
    rgba[H - 2:, :] = 0                                     # ... and below them
    rgba[H - 1, :, :3] = 9.0                                # leftovers of an earlier gutter fill
    rgba[3:6, 2:5] = 0                                      # a hole
    rec[rgba[..., 3] == 0] = 0                              # what a bake leaves on texels nobody owns
    rec[1, 1, 4:7] *= F(0.9)
    rgba[1, 1, :3] = 30.0
    rec[2, half + 2, 0] = np.nan
    rgba[2, half + 2, :3] = 40.0
    rgba[7, 3, 1] = np.nan
    return rgba, rec
