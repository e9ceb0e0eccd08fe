"""tonemap_and_fit_aspect in float64, from the reference's text: the host half (tonemapping.rs:155-224: the
default viewport, the aspect fit, `set_scissor_rect(x as u32, ...)`, LoadOp::Clear(0, 0, 0, 1) or Load) and the shader
(tonemapping.wgsl: the quad of vert_main scaled by `scale`, textureSample through a linear, clamp-to-edge sampler, max(., 0),
exp2(exposure), tonemap_filmic, linear_to_srgb), then the Rgba8Unorm store.

A pixel of the scissor rectangle is shaded when its centre lies in the quad; the rasteriser interpolates tex_coords from
(0, 0) at NDC (-scale.x, scale.y) to (1, 1) at (scale.x, -scale.y).  The sampler is restated as the usual bilinear formula on
texel centres (texel i covers [i, i + 1), so the sample position is uv * size - 0.5) with indices clamped to the edge.
Shader literals (`0.6f`, `1.0f / 2.4f`, ...) are the f32 values.  Non-finite values follow IEEE arithmetic through the
formula (inf * 0 = nan); the store writes 0 for nan, 255 for +inf.

The device computes in f32, so next to each byte the reference returns how far 255 v lies from the nearest rounding boundary
(`slack`) and a bound on the f32 chain's error in the same unit (`bound`).  The bound is

    coordinates  f = (x + 0.5 - vp.x) / vp.w: 2 roundings of a value below 1, 2^-24; ndc = 2 f - 1: twice that and one more,
                 2.5 * 2^-24 (NDC_ERR rounds this and scale's own two roundings up to 5 * 2^-24 for the test against the
                 quad's edge); ndc / scale <= 1: the same divided by scale, plus scale's two roundings and the quotient's,
                 3 * 2^-24; + 1 (one rounding of a value below 2, 2^-24) and * 0.5: uv is off by at most
                 (1.25 / scale + 2) * 2^-24.  Times the source size, plus an ulp of the size for `* size - 0.5`: the sample
                 position's error.  Its effect on the colour is measured, not estimated: the whole chain is evaluated at the
                 four shifted positions, and twice the worst change counts (the filter is piecewise bilinear, the chain
                 monotonic);
    filter       9 roundings and the weights 1 - t: 6 ulp32 of the largest texel of the footprint, pushed through the chain
                 the same way;
    chain        exp2 by lpm_powf (<= 1 ulp: tests/test_detmath.py) and its product, through filmic's elasticity of at most
                 2: 3 ulp; filmic: 9; lpm_powf, the product and the subtraction of linear_to_srgb: 3; `* 255`: 1.  16 ulp32
                 relative to v + 0.055 (the subtraction's operand).

A device byte may differ from the reference's by one only where slack < bound (`exempt`); a pixel centre closer to the
quad's edge than the coordinates' error may be shaded or not.  Both exemptions together may cover at most MAX_EXEMPT_SHARE
of an input's scissor pixels: tonemap() asserts it, so an input that leans on the exemption is rejected, not tolerated.
"""
import numpy as np

from tests import film_ref

MAX_EXEMPT_SHARE = 0.01
U32 = 2.0 ** -23
NDC_ERR = 5 * 2.0 ** -24


def uv_err(scale):
    return (1.25 / scale + 2.0) * 2.0 ** -24

F = lambda x: float(np.float32(x))
K_HDR, K_A, K_B, K_C, K_D, K_E = F(0.6), F(2.51), F(0.03), F(2.43), F(0.59), F(0.14)
CUTOFF, S_MUL, S_ADD, S_LOW = F(0.0031308), F(1.055), F(0.055), F(12.92)
S_POW = float(np.float32(1.0) / np.float32(2.4))

DEFECTS = ("cutoff_wrong_side", "exposure_after_filmic", "no_half_texel", "wrap", "scissor_rounded")


def filmic(c):
    hdr = c * K_HDR
    return np.maximum((hdr * hdr * K_A + hdr * K_B) / (hdr * hdr * K_C + hdr * K_D + K_E), 0.0)


def linear_to_srgb(c, defect=None):
    cutoff = (c >= CUTOFF) if defect == "cutoff_wrong_side" else (c <= CUTOFF)
    cutoff = cutoff.astype(np.float64)
    higher = S_MUL * np.power(c, S_POW) - S_ADD
    return higher * (1.0 - cutoff) + c * S_LOW * cutoff          # mix(higher, lower, cutoff)


def chain(c, desc, defect=None):
    """The fragment shader after the sample: (..., 3) linear colour -> the value stored."""
    with np.errstate(all="ignore"):
        c = np.maximum(c, 0.0)                                    # max(nan, 0) = 0 in WGSL and in fmaxf
        c = np.where(np.isnan(c), 0.0, c)
        gain = 2.0 ** F(desc.exposure)
        if desc.exposure != 0.0 and defect != "exposure_after_filmic":
            c = c * gain
        if desc.filmic:
            c = filmic(c)
        if desc.exposure != 0.0 and defect == "exposure_after_filmic":
            c = c * gain
        if desc.srgb:
            c = linear_to_srgb(c, defect)
    return c


def unorm8(v):
    """(byte, 255 v clamped): Rgba8Unorm's conversion, nan -> 0."""
    with np.errstate(all="ignore"):
        s = np.where(np.isnan(v), 0.0, np.clip(v, 0.0, 1.0)) * 255.0
    return np.rint(s).astype(np.uint8), s


def sample(tex, sx, sy, defect=None):
    """Bilinear, clamp to edge: tex (H, W, 3) float64 at sample positions in texel units (texel centres at integers)."""
    h, w = tex.shape[:2]
    x0, y0 = np.floor(sx), np.floor(sy)
    tx, ty = (sx - x0)[..., None], (sy - y0)[..., None]
    if defect == "wrap":
        idx = lambda i, n: np.mod(i, n).astype(np.int64)
    else:
        idx = lambda i, n: np.clip(i, 0, n - 1).astype(np.int64)
    xa, xb, ya, yb = idx(x0, w), idx(x0 + 1, w), idx(y0, h), idx(y0 + 1, h)
    with np.errstate(all="ignore"):
        top = tex[ya, xa] * (1.0 - tx) + tex[ya, xb] * tx
        bot = tex[yb, xa] * (1.0 - tx) + tex[yb, xb] * tx
        out = top * (1.0 - ty) + bot * ty
    foot = np.stack([tex[ya, xa], tex[ya, xb], tex[yb, xa], tex[yb, xb]], 0)
    return out, foot


class Result:
    pass


def tonemap(src_words, dst_width, dst_height, desc, dst=None, defect=None, check_share=True):
    """src_words (H, W, 4) uint16: the Rgba16Float source's words.  Returns a Result: bytes (dst_height, dst_width, 4) uint8,
    shaded (h, w) bool, exempt (h, w, 3) bool (the byte may be off by one), edge (h, w) bool (the pixel may be shaded or
    not), before (the target's contents under the draw), scissor (x0, y0, x1, y1), exempt_share."""
    src = film_ref.half_to_f64(np.asarray(src_words).view(np.uint16).reshape(np.shape(src_words)))[..., :3]
    sh, sw = src.shape[:2]
    vp = desc.viewport
    vx, vy, vw, vh = (0.0, 0.0, float(dst_width), float(dst_height)) if vp is None else (F(vp.x), F(vp.y), F(vp.w), F(vp.h))
    src_aspect, dst_aspect = sw / sh, vw / vh
    scx, scy = (1.0, dst_aspect / src_aspect) if src_aspect > dst_aspect else (src_aspect / dst_aspect, 1.0)
    as_u32 = (lambda v: int(np.rint(v))) if defect == "scissor_rounded" else (lambda v: int(min(max(v, 0.0), 4294967295.0)))
    x0, y0 = min(as_u32(vx), dst_width), min(as_u32(vy), dst_height)
    x1, y1 = min(x0 + as_u32(vw), dst_width), min(y0 + as_u32(vh), dst_height)

    r = Result()
    if desc.clear:
        before = np.zeros((dst_height, dst_width, 4), np.uint8)
        before[..., 3] = 255
    else:
        before = np.ascontiguousarray(dst, np.uint8).reshape(dst_height, dst_width, 4).copy()
    r.before, r.bytes, r.scissor = before, before.copy(), (x0, y0, x1, y1)
    r.shaded = np.zeros((dst_height, dst_width), bool)
    r.edge = np.zeros((dst_height, dst_width), bool)
    r.exempt = np.zeros((dst_height, dst_width, 3), bool)
    r.exempt_share = 0.0
    if x1 <= x0 or y1 <= y0:
        return r
    yy, xx = np.meshgrid(np.arange(y0, y1, dtype=np.float64), np.arange(x0, x1, dtype=np.float64), indexing="ij")
    nx, ny = 2.0 * ((xx + 0.5 - vx) / vw) - 1.0, 1.0 - 2.0 * ((yy + 0.5 - vy) / vh)
    inside = (np.abs(nx) <= scx) & (np.abs(ny) <= scy)
    edge = (np.abs(np.abs(nx) - scx) <= NDC_ERR) & (np.abs(ny) <= scy + NDC_ERR) | \
           (np.abs(np.abs(ny) - scy) <= NDC_ERR) & (np.abs(nx) <= scx + NDC_ERR)
    u, v = (nx / scx + 1.0) * 0.5, (1.0 - ny / scy) * 0.5
    off = 0.0 if defect == "no_half_texel" else 0.5
    sx, sy = u * sw - off, v * sh - off
    colour, foot = sample(src, sx, sy, defect)
    stored = chain(colour, desc, defect)
    byte, s255 = unorm8(stored)

    # the f32 chain's error, in units of the byte
    dsx, dsy = sw * uv_err(scx) + float(film_ref.ulp32(sw)), sh * uv_err(scy) + float(film_ref.ulp32(sh))
    with np.errstate(all="ignore"):
        pmax = np.where(np.isfinite(foot), np.abs(foot), 0.0).max(0)
        filt = 6.0 * film_ref.ulp32(pmax)
        dev = np.zeros_like(s255)
        for ex, ey in ((-dsx, -dsy), (-dsx, dsy), (dsx, -dsy), (dsx, dsy)):
            moved, _ = sample(src, sx + ex, sy + ey, defect)
            for shifted in (moved - filt, moved + filt):
                dev = np.fmax(dev, np.abs(unorm8(chain(shifted, desc, defect))[1] - s255))
        for shifted in (colour - filt, colour + filt):
            dev = np.fmax(dev, np.abs(unorm8(chain(shifted, desc, defect))[1] - s255))
    bound = 2.0 * dev + 16.0 * U32 * (s255 + 255.0 * S_ADD)
    slack = np.abs((s255 - np.floor(s255)) - 0.5)
    # a footprint with a non-finite texel and a weight that may be zero in one precision only: anything goes
    nonfinite = ~np.isfinite(foot).all((0, -1))
    frac = lambda t, d: (np.abs(t - np.rint(t)) <= d)
    fragile = nonfinite & (frac(sx, dsx) | frac(sy, dsy))
    exempt = (slack < bound) | fragile[..., None]

    sel = (slice(y0, y1), slice(x0, x1))
    r.shaded[sel] = inside
    r.edge[sel] = edge
    r.exempt[sel] = exempt & inside[..., None]
    rgba = np.concatenate([byte, np.full(byte.shape[:2] + (1,), 255, np.uint8)], -1)
    r.bytes[sel] = np.where(inside[..., None], rgba, before[sel])
    r.fragile = np.zeros((dst_height, dst_width), bool)
    r.fragile[sel] = fragile & inside
    r.exempt_share = float((r.exempt.any(-1) | r.edge)[sel].mean())
    if check_share:
        assert r.exempt_share <= MAX_EXEMPT_SHARE, f"{r.exempt_share:.4f} of the pixels are exempt: choose another input"
    return r


# ---- the inputs of DESIGN.md 19 ----------------------------------------------------------------------------------

def _words(rgb):
    a = np.zeros(rgb.shape[:2] + (4,), np.float16)
    with np.errstate(all="ignore"):
        a[..., :3] = rgb.astype(np.float16)
    a[..., 3] = 1.0
    return a.view(np.uint16)


def gradient_source():
    """64 x 40: 0 to 16 along x on a quartic (several texels on either side of the sRGB cutoff 0.0031308), the rows scaled
    apart; a row of negatives, a row of 65504 between two rows of 64 (every desc used saturates them: the f32 error of a
    weight next to 65504 would otherwise decide the neighbours' bytes), and three non-finite texels."""
    x = np.linspace(0.0, 1.0, 64)[None, :, None]
    y = np.linspace(1.0, 0.35, 40)[:, None, None]
    rgb = 16.0 * x ** 4 * y * np.array([1.0, 0.7, 0.45]) + np.array([0.0, 0.0011, 0.0027]) * (1.0 - x)
    rgb[7] = -rgb[7] - 0.25
    rgb[21] = 65504.0
    rgb[20] = rgb[22] = 64.0
    w = _words(rgb)
    w[30, 50, 0], w[12, 9, 1], w[35, 20, 2] = 0x7C00, 0xFC00, 0x7E00     # +inf, -inf, nan
    return w


def small_source(width, height):
    rng = np.random.default_rng(width * 16 + height)
    return _words(rng.uniform(0.0, 1.5, (height, width, 3)) ** 3)


def minified_source():
    rng = np.random.default_rng(4)
    yy, xx = np.meshgrid(np.linspace(0, 1, 120), np.linspace(0, 1, 200), indexing="ij")
    base = np.stack([xx * yy, 0.5 * xx + 0.01, 2.0 * (1.0 - yy) ** 2], -1)
    return _words(base * rng.uniform(0.8, 1.2, base.shape))


def cases():
    """(label, source words, dst width, dst height, TonemapDesc, previous target contents or None).  No case maps texels to
    pixels one to one: every sample would sit within the coordinates' error of a texel centre, where f32 decides which
    neighbour gets a weight of 1e-7, and next to the 65504 row that weight is worth whole bytes."""
    from lupinpathtracer_amd import api
    D, V = api.TonemapDesc, api.Viewport
    g = gradient_source()
    before = np.random.default_rng(8).integers(0, 256, (80, 96, 4)).astype(np.uint8)
    out = [("default", g, 96, 60, D(), None),
           ("srgb off", g, 96, 60, D(srgb=False), None),
           ("filmic", g, 96, 60, D(filmic=True), None),
           ("filmic, linear", g, 96, 60, D(filmic=True, srgb=False), None),
           ("exposure +1.5", g, 80, 50, D(exposure=1.5), None),
           ("exposure -1.5, filmic", g, 80, 50, D(exposure=-1.5, filmic=True), None),
           ("letterbox", g, 96, 80, D(), None),
           ("pillarbox", g, 160, 50, D(), None),
           ("fractional viewport", g, 100, 50, D(viewport=V(7.5, 11.25, 80.75, 33.5)), None),
           ("viewport past the target", g, 100, 50, D(viewport=V(60.25, 30.25, 80.0, 50.0), filmic=True), None),
           ("load, letterbox", g, 96, 80, D(clear=False, exposure=1.5), before),
           ("1x1", small_source(1, 1), 9, 7, D(), None),
           ("1x9", small_source(1, 9), 12, 36, D(filmic=True), None),
           ("9x1", small_source(9, 1), 36, 12, D(exposure=-1.5), None),
           ("minified 200x120 -> 50x30", minified_source(), 50, 30, D(), None)]
    return out


def failures(r, got):
    """What is wrong with the (h, w, 4) uint8 image `got` against a Result, as a list of strings."""
    got = np.asarray(got, np.uint8)
    out = []
    diff = np.abs(got.astype(np.int64) - r.bytes.astype(np.int64))
    unshaded_ok = (got == r.before).all(-1)                       # an edge pixel may have been left alone
    x0, y0, x1, y1 = r.scissor
    outside = np.ones(r.shaded.shape, bool)
    outside[y0:y1, x0:x1] = False
    if not unshaded_ok[outside].all():
        out.append(f"scissor: {int((~unshaded_ok[outside]).sum())} pixels outside it changed")
    firm = ~r.edge
    wrong_cover = firm & ~r.shaded & ~unshaded_ok & ~outside
    if wrong_cover.any():
        out.append(f"quad: {int(wrong_cover.sum())} pixels outside the quad were written")
    sh = r.shaded & (firm | ~unshaded_ok)
    rgb = diff[..., :3]
    strict = sh[..., None] & ~r.exempt & ~r.fragile[..., None]
    if (rgb[strict] != 0).any():
        out.append(f"bytes: {int((rgb[strict] != 0).sum())} differ outside the exempt band (worst {int(rgb[strict].max())})")
    loose = sh[..., None] & r.exempt & ~r.fragile[..., None]
    if (rgb[loose] > 1).any():
        out.append(f"bytes: {int((rgb[loose] > 1).sum())} differ by more than one")
    if (got[..., 3][sh] != 255).any():
        out.append("alpha: not 255 on shaded pixels")
    return out
