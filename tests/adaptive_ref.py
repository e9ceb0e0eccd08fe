"""numpy restatement of adaptive sampling's update rule (csrc/lupin_adaptive.hpp) in float32 with the kernels'
order of operations, so that the device's block errors and masks can be checked exactly."""
import numpy as np

B = 8                      # block edge (one block = one wave64)
MEAN_FLOOR = np.float32(1e-3)


def f(x):
    return np.float32(x)


def luminance(rgb):
    rgb = np.asarray(rgb, np.float32)
    return (f(0.2126) * rgb[..., 0] + f(0.7152) * rgb[..., 1]) + f(0.0722) * rgb[..., 2]


def welford(values):
    """(n, mean, M2) after folding `values` (frames first axis) in order, as k_resolve_adaptive does."""
    values = np.asarray(values, np.float32)
    mean = np.zeros(values.shape[1:], np.float32)
    m2 = np.zeros(values.shape[1:], np.float32)
    for k, l in enumerate(values):
        n = f(k + 1)
        d = l - mean
        mean = mean + d / n
        m2 = m2 + d * (l - mean)
    return len(values), mean, m2


def pixel_error(frames, mean, m2):
    """e_p: sqrt(M2 / (n (n - 1))) / (mean + 1e-3); +inf for n < 2 or non-finite moments."""
    frames = np.asarray(frames)
    mean = np.asarray(mean, np.float32)
    m2 = np.asarray(m2, np.float32)
    nf = frames.astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e = np.sqrt(m2 / (nf * (nf - f(1.0)))) / (mean + MEAN_FLOOR)
    bad = (frames < 2) | ~np.isfinite(mean) | ~np.isfinite(m2)
    return np.where(bad, np.float32(np.inf), e).astype(np.float32)


def _pad_blocks(a, fill):
    h, w = a.shape
    by, bx = -(-h // B), -(-w // B)
    out = np.full((by * B, bx * B), fill, a.dtype)
    out[:h, :w] = a
    return out.reshape(by, B, bx, B).transpose(0, 2, 1, 3).reshape(by, bx, B * B)


def block_error(frames, mean, m2):
    """E_b: max of e_p over the block's in-image pixels, (ceil(H/8), ceil(W/8))."""
    return _pad_blocks(pixel_error(frames, mean, m2), np.float32(-np.inf)).max(-1)


def block_min_frames(frames):
    return _pad_blocks(np.asarray(frames, np.uint32), np.uint32(0xFFFFFFFF)).min(-1)


def block_mask(block_err, block_min_n, threshold, min_frames, max_frames=0):
    """Active blocks for the next call: the block or one of its 8 neighbours not converged, and not capped."""
    converged = (block_err < f(threshold)) & (block_min_n >= min_frames)
    open_ = ~converged
    by, bx = open_.shape
    pad = np.zeros((by + 2, bx + 2), bool)
    pad[1:-1, 1:-1] = open_
    near = np.zeros_like(open_)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            near |= pad[dy:dy + by, dx:dx + bx]
    capped = (block_min_n >= max_frames) if max_frames else np.zeros_like(open_)
    return near & ~capped


def update(frames, mean, m2, threshold, min_frames, max_frames=0):
    """(block_error, block_active) after a frame: the two device passes."""
    e = block_error(frames, mean, m2)
    return e, block_mask(e, block_min_frames(frames), threshold, min_frames, max_frames)


def block_pixels(width, height):
    """In-image pixels of every block, (ceil(H/8), ceil(W/8))."""
    return _pad_blocks(np.ones((height, width), np.uint32), np.uint32(0)).sum(-1)


def expand(block_values, width, height):
    """Per-block values -> per-pixel (H, W)."""
    return np.repeat(np.repeat(block_values, B, 0), B, 1)[:height, :width]
