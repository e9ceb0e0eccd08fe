"""The reference of the bent-normal query (lupin_hip_bent_normal_rays), without a GPU:

resolve_f32      the kernel's sum restated in numpy float32: 64 lanes, each adding its slots l, l + 64, ... in ascending
                 order to (+0, +0, +0, +0) as acc.xyz = acc.xyz + T * d.xyz, acc.w = acc.w + T, then the xor butterfly
sequential_f32   the twin that adds the slots one after the other: it gives other words on ORDER_SEED's input
sum_bound        how far resolve_f32 may be from the exact sum
moments          float64 quadrature of E[T d], E[T] and the second moments over the cosine-weighted (or uniform) hemisphere
                 about +z, against the closed forms OPEN_SKY and WALL below
"""
import math

import numpy as np

LANES = 64
OFFSETS = (32, 16, 8, 4, 2, 1)
U = 2.0 ** -24             # the unit roundoff of f32
ORDER_SEED = 7             # the input on which the sequential twin differs (test_bent_normal_cpu.py)
SIGMAS = 5.0               # the repository's AO_SIGMAS convention


def resolve_f32(T, dirs):
    """Four f32 words for one record's slots: T (S,), dirs (S, 3)."""
    T = np.asarray(T, np.float32).reshape(-1)
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    assert len(T) == len(d)
    terms = np.concatenate([(T[:, None] * d).astype(np.float32), T[:, None]], axis=1)     # one rounded product per component
    p = np.zeros((LANES, 4), np.float32)
    for first in range(0, len(T), LANES):
        row = terms[first:first + LANES]
        p[:len(row)] = p[:len(row)] + row
    lanes = np.arange(LANES)
    for off in OFFSETS:
        p = (p + p[lanes ^ off]).astype(np.float32)
    return p[0]


def sequential_f32(T, dirs):
    """The twin: the same terms, added in slot order by one accumulator."""
    T = np.asarray(T, np.float32).reshape(-1)
    d = np.asarray(dirs, np.float32).reshape(-1, 3)
    terms = np.concatenate([(T[:, None] * d).astype(np.float32), T[:, None]], axis=1)
    acc = np.zeros(4, np.float32)
    for row in terms:
        acc = (acc + row).astype(np.float32)
    return acc


def exact_f64(T, dirs):
    T = np.asarray(T, np.float32).astype(np.float64).reshape(-1)
    d = np.asarray(dirs, np.float32).astype(np.float64).reshape(-1, 3)
    return np.concatenate([(T[:, None] * d).sum(axis=0), [T.sum()]])


def sum_bound(T, dirs):
    """|resolve_f32 - exact| per component.  A term passes through one product (xyz; none for w), at most ceil(S / 64)
    additions in its lane (the first, to +0, is exact) and six additions in the butterfly: m = ceil(S / 64) + 6 roundings,
    each of relative size at most U, so by the standard bound the error is at most gamma_m * sum |term|,
    gamma_m = m U / (1 - m U)."""
    T = np.asarray(T, np.float32).astype(np.float64).reshape(-1)
    d = np.asarray(dirs, np.float32).astype(np.float64).reshape(-1, 3)
    m = math.ceil(len(T) / LANES) + 6
    gamma = m * U / (1.0 - m * U)
    return gamma * np.concatenate([np.abs(T[:, None] * d).sum(axis=0), [np.abs(T).sum()]])


# ---- closed forms, normal +z: (E[T d.x], E[T d.y], E[T d.z], E[T]) and the per-slot variances of the four terms ----

def _closed(mean, second):
    mean, second = np.array(mean, np.float64), np.array(second, np.float64)
    return {"mean": mean, "var": second - mean * mean}


# cosine-weighted pdf cos(theta) / pi.  Open sky: T = 1.  E[d.z] = 2/3, E[d.x^2] = E[d.y^2] = 1/4, E[d.z^2] = 1/2.
OPEN_SKY = _closed([0.0, 0.0, 2.0 / 3.0, 1.0], [0.25, 0.25, 0.5, 1.0])
# at the foot of an infinite wall that blocks every direction with d.x < 0: T = [d.x > 0].
WALL = _closed([2.0 / (3.0 * math.pi), 0.0, 1.0 / 3.0, 0.5], [0.125, 0.125, 0.25, 0.5])
# the twins that draw directions uniformly over the hemisphere (pdf 1 / (2 pi)): what a wrong sampler would give
OPEN_SKY_UNIFORM = np.array([0.0, 0.0, 0.5, 1.0])
WALL_UNIFORM = np.array([0.25, 0.0, 0.25, 0.5])


def moments(blocked, uniform=False, n_theta=2000, n_phi=2000):
    """Midpoint quadrature in float64 over theta in (0, pi/2), phi in (0, 2 pi): (mean (4,), second moment (4,)) of
    (T d.x, T d.y, T d.z, T) with T = 0 where blocked(d) and 1 elsewhere."""
    theta = (np.arange(n_theta) + 0.5) * (0.5 * math.pi / n_theta)
    phi = (np.arange(n_phi) + 0.5) * (2.0 * math.pi / n_phi)
    th, ph = np.meshgrid(theta, phi, indexing="ij")
    d = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=-1)
    pdf = np.full_like(th, 1.0 / (2.0 * math.pi)) if uniform else np.cos(th) / math.pi
    w = pdf * np.sin(th) * (0.5 * math.pi / n_theta) * (2.0 * math.pi / n_phi)
    T = np.where(blocked(d), 0.0, 1.0)
    terms = np.concatenate([T[..., None] * d, T[..., None]], axis=-1)
    return (terms * w[..., None]).sum(axis=(0, 1)), (terms * terms * w[..., None]).sum(axis=(0, 1))


def standard_errors(closed, samples):
    """Of the query's four sums divided by `samples`."""
    return np.sqrt(closed["var"] / samples)
