"""The film in float64, from the shader's text: clamp_radiance (pathtracer.wgsl:1774-1783 with
vec3f_is_finite, :2769-2772) and pathtrace_main's epilogue (:228-289) -- the sum over the samples, `/ SAMPLES_PER_PIXEL`,
max(., 0), the `accum_counter != 0` blend with prev_frame and its second max(., 0), and the Rgba16Float store.  The next
frame reads the stored texel back as prev_frame: what it blends with is the f16 value, not the f32 one it came from.

f16 is handled from its bit layout (1 sign, 5 exponent, 10 fraction bits, bias 15): decoding is exact in float64, and
rounding a real number to f16 is done toward zero or to nearest even on the scaled integer.

The shader computes in f32 and the order of its roundings is not part of the contract, so the reference answers with the set
of admissible f16 words per channel: every real within `e` of the exact value, rounded in the selected mode.  As f16 words
of non-negative values are ordered like the values, the set is the range [lo, hi] of words.  `e` is counted along the
expression tree.  Every operation adds half an f32 ulp of its own result, unless its operands are exact so far and the
exact result is an f32 number (then the f32 operation is exact too), and passes its operands' errors on:

    per sample   t = max_radiance / max(r): rnd;  c = r * t: r e(t) + rnd          (only when a component exceeds max_radiance)
    new colour   S_k = S_(k-1) + c, k = 2 .. spp: e(S_(k-1)) + e(c) + rnd;  colour = S / spp: e(S) / spp + rnd
    blend        w = 1 / n: rnd;  a = 1 - w: e(w) + rnd;  p = prev * a: |prev| e(a) + rnd;  q = colour * w:
                 colour e(w) + w e(colour) + rnd;  p + q: e(p) + e(q) + rnd

This is the count "one rounding each for 1 / n, 1 - w, the two products and the sum" with each rounding at its own
magnitude, never more than an ulp of the largest operand.  One f16 ulp is 2^13 f32 ulps: the set has one word unless the
exact value lies within e of a rounding boundary.  With n = 0, 1 or 2 and a power-of-two spp nothing rounds: e = 0.  When
prev equals the new colour and n is not a power of two, the exact blend is that f16 value itself, a boundary of the
rounding toward zero, and e > 0: the words of the value and of its predecessor are both admissible, which is the decay of a
converged image under the reference's store.
"""
import numpy as np

RTZ, RNE = 0, 1
F16_MAX = 65504.0
ALPHA_ONE = 0x3C00


def half_to_f64(bits):
    """Value of f16 words, exactly; inf and nan as such."""
    b = np.asarray(bits, np.uint16).astype(np.int64)
    sign = np.where(b & 0x8000, -1.0, 1.0)
    e, f = (b >> 10) & 0x1F, (b & 0x3FF).astype(np.float64)
    with np.errstate(all="ignore"):
        v = np.where(e == 0, f * 2.0 ** -24, (1024.0 + f) * 2.0 ** (e.astype(np.float64) - 25.0))
        v = np.where(e == 31, np.where(f == 0, np.inf, np.nan), v)
    return sign * v


def round_to_half(x, mode):
    """f16 words of reals x (float64, no nan) rounded toward zero (RTZ) or to nearest even (RNE).  RTZ never produces an
    infinity from a finite number; RNE does from 65520 up."""
    x = np.asarray(x, np.float64)
    sign = np.where(np.signbit(x), 0x8000, 0).astype(np.int64)
    a = np.abs(x)
    finite = np.isfinite(a)
    a_f = np.where(finite, a, 0.0)
    _, ex = np.frexp(a_f)                                # a = m 2^ex, m in [0.5, 1)
    qexp = np.maximum(ex - 1, -14) - 10                  # exponent of the quantum: 2^-24 below 2^-14
    q = np.ldexp(a_f, -qexp)                             # exact: a power-of-two scaling
    n = np.floor(q)
    if mode == RNE:
        frac = q - n
        n = n + ((frac > 0.5) | ((frac == 0.5) & (np.mod(n, 2.0) == 1.0)))
    # n in [0, 2048]; 2048 means the next binade
    up = n >= 2048.0
    n = np.where(up, 1024.0, n)
    ex = np.where(a_f == 0.0, -100, ex)                  # zero: frexp's exponent 0 means nothing
    e_field = np.where(ex - 1 < -14, np.where(n >= 1024.0, 1, 0), (ex - 1 + 15) + up)
    frac_field = np.where(n >= 1024.0, n - 1024.0, n)
    word = (e_field.astype(np.int64) << 10) | frac_field.astype(np.int64)
    overflow = word >= 0x7C00
    word = np.where(overflow, 0x7BFF if mode == RTZ else 0x7C00, word)
    word = np.where(finite, word, 0x7C00)
    return (sign | word).astype(np.uint16)


def ulp32(x):
    """One f32 ulp at |x| (of the smallest normal below it)."""
    _, ex = np.frexp(np.maximum(np.abs(np.asarray(x, np.float64)), 2.0 ** -126))
    return np.ldexp(1.0, ex - 1 - 23)


def clamp_radiance(r, max_radiance):
    """(clamped (..., 3), scaled (...) bool).  `r` holds f32 values; non-finite in any component -> zero."""
    r = np.asarray(r, np.float64)
    ok = np.isfinite(r).all(-1, keepdims=True)
    r = np.where(ok, r, 0.0)
    big = (r > max_radiance).any(-1, keepdims=True)
    with np.errstate(all="ignore"):
        r = np.where(big, r * (max_radiance / r.max(-1, keepdims=True)), r)
    return r, big[..., 0]


class Film:
    """Exact value (before the last max(., 0)) and error bound of one frame's texels."""

    def __init__(self, raw, err):
        self.raw, self.err = raw, err                    # (..., 3) float64 each
        self.value = np.maximum(raw, 0.0)

    def words(self, mode):
        """(lo, hi) f16 words per channel: the admissible range."""
        lo = round_to_half(np.maximum(self.raw - self.err, 0.0), mode)
        hi = round_to_half(np.maximum(self.raw + self.err, 0.0), mode)
        return lo, hi

    def admits(self, got_words, mode):
        lo, hi = self.words(mode)
        g = np.asarray(got_words, np.uint16)
        return (g >= lo) & (g <= hi)

    def admits_f32(self, got):
        """f32 accumulation: the f32 word itself, within the bound."""
        g = np.asarray(got, np.float64)
        return (g >= np.maximum(self.raw - self.err, 0.0)) & (g <= np.maximum(self.raw + self.err, 0.0))


def _rnd(value, err_in):
    """Half an f32 ulp of `value`, or 0 where the operands were exact (err_in == 0) and value is an f32 number."""
    value = np.asarray(value, np.float64)
    with np.errstate(all="ignore"):
        exact = (err_in == 0) & (value.astype(np.float32).astype(np.float64) == value)
    return np.where(exact, 0.0, 0.5 * ulp32(np.abs(value) + err_in) * (1.0 + 2.0 ** -20))


def sample_colour(sample_radiance, spp, max_radiance):
    """(colour (3,), error (3,)): clamp_radiance of equal samples, summed, divided by spp, max(., 0)."""
    r = np.asarray(sample_radiance, np.float32).astype(np.float64)
    mr = float(np.float32(max_radiance))
    c, scaled = clamp_radiance(r, mr)
    ec = np.zeros(3)
    if scaled:
        t = mr / r.max()
        et = _rnd(t, 0.0)
        ec = r * et + _rnd(c, et)
    s, es = c, ec
    for _ in range(2, spp + 1):
        s, es = s + c, es + ec + _rnd(s + c, es + ec)
    colour = s / spp
    return np.maximum(colour, 0.0), es / spp + _rnd(colour, es)


def frame(sample_radiance, spp, max_radiance, accum_counter, prev=None):
    """One pathtrace_main call whose every sample returns `sample_radiance` (3,): the Film of texels whose previous frame
    holds `prev` (..., 3) float64 (values as read back: f16 words decoded, or the f32 accumulator).  accum_counter 0: no
    blend, prev only gives the shape."""
    colour, ec = sample_colour(sample_radiance, spp, max_radiance)
    if accum_counter == 0:
        shape = () if prev is None else np.shape(prev)[:-1]
        return Film(np.broadcast_to(colour, shape + (3,)).copy(), np.broadcast_to(ec, shape + (3,)).copy())
    prev = np.asarray(prev, np.float64)
    w = 1.0 / accum_counter
    ew = _rnd(w, 0.0)
    a = 1.0 - w
    ea = ew + _rnd(a, ew)
    p = prev * a
    ep = np.abs(prev) * ea + _rnd(p, ea + 0.0 * p)
    q = colour * w
    eq = colour * ew + w * ec + _rnd(q, ew + ec)
    return Film(p + q, ep + eq + _rnd(p + q, ep + eq))


# ---- the cases of DESIGN.md 19: an environment of emission E and no geometry, so every sample's radiance is E -------------

WIDTH, HEIGHT = 32, 16
MAX_RADIANCE = 100.0
# (emission, samples per pixel)
EMISSIONS = [((0.5, 0.25, 1.0), 1), ((0.5, 0.25, 1.0), 2), ((0.5, 0.25, 1.0), 3), ((0.5, 0.25, 1.0), 4),
             ((300.0, 30.0, 3.0), 2),              # above max_radiance: scaled to (100, 10, 1)
             ((np.inf, 1.0, 1.0), 2)]              # not finite: the sample counts as zero
COUNTERS = (0, 1, 2, 3, 7, 1000)


def prev_words(emission):
    """(HEIGHT, WIDTH, 4) uint16 prev_frame for an emission: rows of zeros, f16 subnormals, 65504, the clamped colour's
    predecessor, successor and the colour itself, then random finite words of either sign."""
    colour = round_to_half(clamp_radiance(np.asarray(emission, np.float32), MAX_RADIANCE)[0], RNE).astype(np.int64)
    rng = np.random.default_rng(16)
    w = rng.integers(0, 0x10000, (HEIGHT, WIDTH, 4)).astype(np.int64)
    w = np.where((w & 0x7C00) == 0x7C00, w & 0x83FF, w)          # finite
    w[0] = 0
    w[1] = rng.integers(1, 0x400, (WIDTH, 4))
    w[2] = 0x7BFF
    w[3, :, :3], w[4, :, :3], w[5, :, :3] = np.maximum(colour - 1, 0), colour + 1, colour
    w[6, :, :3] = colour
    w[6, ::2, :3] = np.maximum(colour - 1, 0)
    w[..., 3] = ALPHA_ONE
    return w.astype(np.uint16)


def environment_scene(ctx, emission):
    """One untextured environment of that emission, no geometry (ctx None: host side only, for the oracle)."""
    from lupinpathtracer_amd import api
    sc = api.SceneCPU()
    env = api.default_environment()
    env["emission"] = np.asarray(emission, np.float32)
    sc.environments = np.array([env], api.ENVIRONMENT_DTYPE)
    api.validate_scene(sc, 0, 0)
    return api.build_accel_structures_and_upload(ctx, sc, [], [api.EnvMapInfo(np.ones((1, 1, 4), np.float32), 1, 1)], True)


def word_failures(film, got_words, mode, label):
    """`got_words` (H, W, 4) uint16 against a Film, as a list of strings."""
    got = np.asarray(got_words).view(np.uint16).reshape(np.shape(got_words))
    out = []
    ok = film.admits(got[..., :3], mode)
    if not ok.all():
        y, x, c = np.argwhere(~ok)[0]
        lo, hi = film.words(mode)
        out.append(f"{label}: {int((~ok).sum())} words outside the admissible set, first at ({x}, {y}, {c}): "
                   f"{got[y, x, c]:#06x} not in [{lo[y, x, c]:#06x}, {hi[y, x, c]:#06x}]")
    if not (got[..., 3] == ALPHA_ONE).all():
        out.append(f"{label}: alpha is not 1.0")
    return out
