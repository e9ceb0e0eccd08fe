"""Adaptive lightmap baking (lupin_hip_pathtrace_rays_moments, lupin_hip_bake_lightmap_adaptive) restated in
numpy float32, operation for operation as include/lupin_hip.h words them:

  resolve                  the wave-per-record reduction in two passes: lane partials over slots l, l + 64, ..., the xor
                           butterfly, the means; then the squared deviations of the luminance from its mean, the same way
  resolve_sum_of_squares   a twin that takes M2 as sum l^2 - S * ml^2 (NOT the contract: the CPU tests show where it cancels)
  merge, pixel_error, want, mask, compact, round_word     the steps of a round
  run                      the round loop, with the query handed in
  planes                   out_rgba (before the gutter passes) and out_stats

Every operation is one float32 operation; numpy's float32 arithmetic rounds each one."""
import numpy as np

from lupinpathtracer_amd import api

F = np.float32
PI = F(np.pi)
LANES = 64
BLOCK = 256
MEAN_FLOOR = F(1e-3)
ROUND_STRIDE = 0x85EBCA6B
SAMPLE_STRIDE = 0x9E3779B9
MOMENTS_FLOATS = 8


def luminance(c):
    c = np.asarray(c, F)
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def _wave_sum(values):
    """(n, ...) float32: the sum over axis 1 (the slots) of `values` (n, S, ...) as a wave adds it."""
    n, S = values.shape[:2]
    acc = np.zeros((n, LANES) + values.shape[2:], F)
    for first in range(0, S, LANES):                      # lane l adds slot first + l: ascending per lane
        k = min(LANES, S - first)
        acc[:, :k] = acc[:, :k] + values[:, first:first + k]
    lane = np.arange(LANES)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lane ^ off]
    return acc[:, 0]                                      # (every lane holds the same words after the butterfly)


def resolve(radiance):
    """(n, 8) float32 moments of n records from their slots' radiance (n, S, 3+)."""
    c = np.asarray(radiance, F)[:, :, :3]
    n, S = c.shape[:2]
    lum = luminance(c)
    out = np.zeros((n, MOMENTS_FLOATS), F)
    with np.errstate(all="ignore"):
        out[:, 0:3] = _wave_sum(c) / F(S)
        out[:, 3] = F(1.0)
        ml = _wave_sum(lum) / F(S)
        out[:, 4] = ml
        out[:, 5] = _wave_sum((lum - ml[:, None]) * (lum - ml[:, None]))
        out[:, 6] = F(S)
    return out


def resolve_sum_of_squares(radiance):
    out = resolve(radiance)
    lum = luminance(np.asarray(radiance, F)[:, :, :3])
    S = lum.shape[1]
    out[:, 5] = _wave_sum(lum * lum) - F(S) * (out[:, 4] * out[:, 4])
    return out


def pixel_error(n, ml, m2):
    """e_i: +inf while there is no estimate, else sqrtf(M2 / (nf * (nf - 1))) / (ml + 1e-3f)."""
    n = np.asarray(n, np.uint32)
    ml, m2 = np.asarray(ml, F), np.asarray(m2, F)
    nf = n.astype(F)
    with np.errstate(all="ignore"):
        e = np.sqrt(m2 / (nf * (nf - F(1.0)))) / (ml + MEAN_FLOOR)
    return np.where((n < 2) | ~np.isfinite(ml) | ~np.isfinite(m2), F(np.inf), e).astype(F)


class State:
    def __init__(self, n):
        self.n = np.zeros(n, np.uint32)
        self.rounds = np.zeros(n, np.uint32)
        self.mean = np.zeros((n, 3), F)
        self.ml = np.zeros(n, F)
        self.m2 = np.zeros(n, F)

    def error(self):
        return pixel_error(self.n, self.ml, self.m2)


def merge(st, index_of, moments, S):
    """The round's moments (n_active, 8) of records `index_of` into the state."""
    i = np.asarray(index_of)
    mom = np.asarray(moments, F)
    first = st.n[i] == 0
    with np.errstate(all="ignore"):
        nA, nB = st.n[i].astype(F), F(S)
        w = nB / (nA + nB)
        delta = mom[:, 4] - st.ml[i]
        mean = st.mean[i] + (mom[:, 0:3] - st.mean[i]) * w[:, None]
        ml = st.ml[i] + delta * w
        m2 = (st.m2[i] + mom[:, 5]) + ((delta * delta) * nA) * w
    st.mean[i] = np.where(first[:, None], mom[:, 0:3], mean)
    st.ml[i] = np.where(first, mom[:, 4], ml)
    st.m2[i] = np.where(first, mom[:, 5], m2)
    st.n[i] += np.uint32(S)
    st.rounds[i] += np.uint32(1)


def want(st, threshold, min_rounds, max_rounds):
    e = st.error()
    return (st.rounds < max_rounds) & ((st.rounds < min_rounds) | ~(e < F(threshold)))


def mask(want_plane, texel_of, rounds, max_rounds):
    """active per record: not at the cap, and the texel or one of its eight neighbours inside the atlas wants samples."""
    H, W = want_plane.shape
    padded = np.zeros((H + 2, W + 2), bool)
    padded[1:-1, 1:-1] = want_plane
    near = np.zeros((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            near |= padded[dy:dy + H, dx:dx + W]
    return (np.asarray(rounds) < max_rounds) & near.reshape(-1)[np.asarray(texel_of)]


def compact(active):
    """index_of: the active records' indices by the device's steps -- counts per block of 256, their exclusive scan, every
    active record at its block's offset plus its rank in the block."""
    active = np.asarray(active, bool)
    n = len(active)
    blocks = (n + BLOCK - 1) // BLOCK
    totals = np.array([int(active[b * BLOCK:(b + 1) * BLOCK].sum()) for b in range(blocks)], np.uint32)
    offsets = np.concatenate([[0], np.cumsum(totals)]).astype(np.uint32)
    index_of = np.zeros(int(offsets[-1]), np.uint32)
    for b in range(blocks):
        inside = active[b * BLOCK:(b + 1) * BLOCK]
        rank = np.cumsum(inside) - inside
        for t in np.nonzero(inside)[0]:
            index_of[int(offsets[b]) + int(rank[t])] = b * BLOCK + t
    return index_of


def round_word(word, r):
    word = np.asarray(word, np.uint32)
    with np.errstate(over="ignore"):
        return word.copy() if r == 0 else api._hash_u32(word + np.uint32(r) * np.uint32(ROUND_STRIDE))


def round_records(records, index_of, r):
    rec = np.array(np.asarray(records, F).reshape(-1, 8)[np.asarray(index_of, np.int64)], F, copy=True)
    rec.view(np.uint32)[:, 3] = round_word(rec.view(np.uint32)[:, 3], r)
    return rec


def run(records, texel_of, W, H, S, threshold, min_rounds, max_rounds, query):
    """The round loop over the owned texels' `records` (n, 8) at `texel_of` (n,): query(round records, r) -> (n_active, 8)
    moments.  Returns (state, log), log[r] = (index_of, want after the round (n,), active after the round (n,))."""
    n = len(records)
    st = State(n)
    active = np.ones(n, bool)
    want_plane = np.zeros(W * H, bool)
    log = []
    for r in range(len(records) * max_rounds + 1):        # (every round that traces adds to some record's rounds: it ends before that)
        index_of = compact(active)
        if len(index_of) == 0:
            break
        merge(st, index_of, query(round_records(records, index_of, r), r), S)
        wants = want(st, threshold, min_rounds, max_rounds)
        want_plane[np.asarray(texel_of)[index_of]] = wants[index_of]       # only the round's records write their byte
        active = mask(want_plane.reshape(H, W), texel_of, st.rounds, max_rounds)
        log.append((index_of, want_plane[np.asarray(texel_of)].copy(), active.copy()))
    return st, log


def planes(st, texel_of, W, H, threshold, min_rounds):
    """(out_rgba before the gutter passes, out_stats): (H, W, 4) float32 each."""
    rgba, stats = np.zeros((W * H, 4), F), np.zeros((W * H, 4), F)
    t = np.asarray(texel_of)
    e = st.error()
    nf = st.n.astype(F)
    with np.errstate(all="ignore"):
        se = np.where(st.n < 2, F(0.0), PI * np.sqrt(st.m2 / (nf * (nf - F(1.0))))).astype(F)
    rgba[t, 0:3] = PI * st.mean
    rgba[t, 3] = F(1.0)
    stats[t, 0], stats[t, 1], stats[t, 2] = nf, e, se
    stats[t, 3] = ((st.rounds >= min_rounds) & (e < F(threshold))).astype(F)
    return rgba.reshape(H, W, 4), stats.reshape(H, W, 4)
