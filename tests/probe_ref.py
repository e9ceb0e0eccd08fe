"""Light-probe baking (lupin_hip_bake_probes) restated in numpy float32: the nine basis functions with the
header's literals and order of operations, and k_resolve_probes' reduction -- lane l of a wave of 64 sums samples l, l + 64,
... in ascending order from +0, an xor butterfly (offsets 32 .. 1) adds the lanes, then * (4 pi) / S.  Directions and
radiances are inputs: the directions come from the bake's own first rays, the radiances from one-sample queries on them."""
import numpy as np

F = np.float32
K0, K1, K2, K3, K4 = F(0.28209479), F(0.48860251), F(1.09254843), F(0.31539157), F(0.54627422)
WAVE = 64


def sh_basis_f32(dirs):
    """(S, 9) float32: Y_0 .. Y_8 of the (S, 3) float32 unit vectors, every operation one rounded f32 operation."""
    d = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    Y = np.empty((len(d), 9), F)
    Y[:, 0] = K0
    Y[:, 1] = K1 * y
    Y[:, 2] = K1 * z
    Y[:, 3] = K1 * x
    Y[:, 4] = (K2 * x) * y
    Y[:, 5] = (K2 * y) * z
    Y[:, 6] = K3 * ((F(3.0) * z) * z - F(1.0))
    Y[:, 7] = (K2 * x) * z
    Y[:, 8] = K4 * (x * x - y * y)
    return Y


def terms(dirs, radiance):
    """(S, 9, 4) float32: what sample s adds to the accumulators -- L_s[c] * Y_j for r, g, b and Y_j itself for w."""
    Y = sh_basis_f32(dirs)
    L = np.ascontiguousarray(radiance, F).reshape(-1, 3)
    assert len(L) == len(Y)
    t = np.empty((len(Y), 9, 4), F)
    t[:, :, :3] = L[:, None, :] * Y[:, :, None]
    t[:, :, 3] = Y
    return t


def reduce(dirs, radiance):
    """(9, 4) float32: one probe's coefficients from its S directions and per-path radiances, in the kernel's order."""
    t = terms(dirs, radiance)
    S = len(t)
    acc = np.zeros((WAVE, 9, 4), F)
    for first in range(0, S, WAVE):
        row = t[first:first + WAVE]
        acc[:len(row)] = acc[:len(row)] + row
    lanes = np.arange(WAVE)
    for offset in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ offset]
    assert np.array_equal(acc.view(np.uint32), np.broadcast_to(acc[0], acc.shape).view(np.uint32))   # every lane holds the sum
    return (acc[0] * (F(4.0) * F(np.pi))) / F(S)


def reduce_ascending(dirs, radiance):
    """The same quantity summed s = 0, 1, 2, ... in one accumulator: NOT what the kernel computes."""
    t = terms(dirs, radiance)
    acc = np.zeros((9, 4), F)
    for row in t:
        acc = acc + row
    return (acc * (F(4.0) * F(np.pi))) / F(len(t))


def bake(dirs, radiance, samples):
    """(n, 9, 4): reduce() per probe over the (n * samples, 3) directions and radiances, probe i owning rows i * samples ..."""
    d = np.ascontiguousarray(dirs, F).reshape(-1, samples, 3)
    L = np.ascontiguousarray(radiance, F).reshape(-1, samples, 3)
    return np.stack([reduce(d[i], L[i]) for i in range(len(d))]) if len(d) else np.zeros((0, 9, 4), F)
