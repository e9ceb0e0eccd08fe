"""numpy restatement of the reference's camera, written from the shader's text and from nothing else:
pathtrace_main's per-sample prologue (pathtracer.wgsl:226, :236-237), compute_camera_ray (:505-542), init_rng / hash_u32 /
random_f32 / random_vec2f / random_in_disk (:1563-1629) and transform_point / transform_dir / transform_ray (:2648-2669).

The random number generator is restated exactly, in integers: the four numbers a sample's first ray consumes are the f32
values the shader draws, and the state afterwards compares bit for bit.  Everything else is evaluated in `dtype`: float64
is the reference the device and the oracle are held to, float32 (numpy's own operation order) gives the rounding noise of
the formula itself and evaluates the planted defects.

Conventions: a camera transform is a (4, 4) array [column][row], the shader's mat4x4f (api.camera_transform_mat4 makes one
from the renderer's 4 x 3); camera parameters and matrix entries are rounded to f32 first, as the push constants hold them.
"""
import functools
import itertools

import numpy as np

from lupinpathtracer_amd import api

M32 = np.uint64(0xFFFFFFFF)
PI_F32 = float(np.float32(3.14159265358979323846264338327950288))   # `const PI: f32` (:2646)

# planted defects (tests/test_camera_film_cpu.py): one-line misreadings of the text above
DEFECTS = ("no_row_offset", "no_half_pixel", "film_branches_swapped", "lens_drawn_before_jitter", "lens_radius_halved",
           "ortho_ignores_focus", "w_divide", "no_final_normalise")


# ---- RNG, in integers ------------------------------------------------------------------------------------------

def _u64(x):
    return np.asarray(x, np.uint64) & M32


def hash_u32(seed):                                   # :1569-1580
    x = _u64(seed)
    x = x ^ (x >> np.uint64(17))
    x = (x * np.uint64(0xED5AD4BB)) & M32
    x = x ^ (x >> np.uint64(11))
    x = (x * np.uint64(0xAC4C1B51)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x31848BAB)) & M32
    x = x ^ (x >> np.uint64(14))
    return x


def init_rng(global_id, accum_counter):               # :1563-1567; global_id = y * width + x (:226), `seed` is the literal 0
    a = (_u64(global_id) * np.uint64(19349663)) & M32
    b = (_u64(accum_counter) * np.uint64(83492791)) & M32
    return hash_u32(a ^ b).astype(np.uint32)


def random_u32(state):                                # :1584-1591 -> (state afterwards, result), uint64 holding u32 values
    s = (_u64(state) * np.uint64(747796405) + np.uint64(2891336453)) & M32
    r = (((s >> ((s >> np.uint64(28)) + np.uint64(4))) ^ s) * np.uint64(277803737)) & M32
    r = (r >> np.uint64(22)) ^ r
    return s, r


def u32_to_f32(r):
    """f32(r) for a u32, round to nearest even, from the integer: 24 significant bits are kept."""
    r = _u64(r)
    out = r.astype(np.float64)
    for e in range(1, 9):                              # r in [2^(23+e), 2^(24+e)): the quantum is 2^e
        sel = (r >> np.uint64(23 + e)) == np.uint64(1)
        q, rem = r >> np.uint64(e), r & np.uint64((1 << e) - 1)
        half = np.uint64(1 << (e - 1))
        up = (rem > half) | ((rem == half) & ((q & np.uint64(1)) == np.uint64(1)))
        out = np.where(sel, ((q + up.astype(np.uint64)) << np.uint64(e)).astype(np.float64), out)
    return out                                         # float64 holding an f32 value exactly


def random_f32(state):                                # :1594-1600 -> (state afterwards, the f32 drawn, as float64)
    s, r = random_u32(state)
    return s, u32_to_f32(r) / 4294967296.0             # `4294967295.0f` is 2^32 in f32; the division is exact


# ---- the camera --------------------------------------------------------------------------------------------------

def _normalize(v):
    return v / np.sqrt((v * v).sum(-1, dtype=v.dtype))[..., None]


def _mat_xyz(m, v, w):
    """(m * vec4(v, w)).xyz and the w row, for m [column][row]."""
    out = [m[0][r] * v[..., 0] + m[1][r] * v[..., 1] + m[2][r] * v[..., 2] + m[3][r] * w for r in range(4)]
    return np.stack(out[:3], -1), out[3]


def rays(width, height, camera_params, transform, gx, gy, rng_state, dtype=np.float64, pinhole=False, defect=None):
    """The first ray of a sample of pixels (gx, gy) in a width x height image, drawn from `rng_state` (u32 per record):
    (ori (n, 3), dir (n, 3), rng_state_after (n,) uint32).  pinhole: the ray through the pixel centre with a zero
    aperture; nothing is drawn.  `defect`: one of DEFECTS."""
    assert defect is None or defect in DEFECTS
    T = dtype
    gx, gy = np.asarray(gx, np.uint32).reshape(-1), np.asarray(gy, np.uint32).reshape(-1)
    state = _u64(np.asarray(rng_state, np.uint32).reshape(-1))
    cp = camera_params
    lens, film, aspect, focus, aperture = (T(np.float32(v)) for v in (cp.lens, cp.film, cp.aspect, cp.focus, cp.aperture))
    m = np.asarray(transform, np.float32).reshape(4, 4).astype(T)
    half, one, two = T(0.5), T(1.0), T(2.0)

    if pinhole:
        offx = offy = np.zeros(len(gx), T)
        lens_uv = np.zeros((len(gx), 2), T)
        aperture = T(0.0)
    else:
        draws = []
        for _ in range(4):                             # random_vec2f for the pixel offset (:236), then random_in_disk (:518)
            state, v = random_f32(state)
            draws.append(v.astype(T))
        if defect == "lens_drawn_before_jitter":
            draws = draws[2:] + draws[:2]
        offx, offy = draws[0] - half, draws[1] - half
        r, phi = np.sqrt(draws[3]), two * T(PI_F32) * draws[2]          # :1623-1629: r from rnd.y, phi from rnd.x
        lens_uv = np.stack([np.cos(phi) * r, np.sin(phi) * r], -1)

    resx, resy = T(width), T(height)
    add = T(0.0) if defect == "no_half_pixel" else half
    row = (resy - one - gy.astype(T)) if defect == "no_row_offset" else (resy - gy.astype(T))   # :508
    pcx, pcy = gx.astype(T) + add, row + add
    uvx, uvy = (pcx + offx) / resx, (pcy + offy) / resy
    wide = aspect >= one
    if defect == "film_branches_swapped":
        wide = not wide
    fsx, fsy = (film, film / aspect) if wide else (film * aspect, film)  # :517
    lens_radius = aperture / (T(4.0) if defect == "lens_radius_halved" else two)
    zero = np.zeros(len(gx), T)
    flip = np.array([1.0, 1.0, -1.0], T)
    with np.errstate(all="ignore"):
        if cp.is_orthographic:                         # :520-530
            scale = one / lens
            qx, qy = fsx * (half - uvx) * scale, fsy * (half - uvy) * scale
            e = np.stack([-qx + lens_uv[:, 0] * lens_radius, -qy + lens_uv[:, 1] * lens_radius, zero], -1)
            p = np.stack([-qx, -qy, zero - focus], -1)
            d = _normalize(np.stack([zero, zero, zero - one], -1) if defect == "ortho_ignores_focus" else p - e) * flip
        else:                                          # :531-541
            q = np.stack([fsx * (half - uvx), fsy * (half - uvy), zero + lens], -1)
            look_at = -_normalize(q)
            e = np.stack([lens_uv[:, 0] * lens_radius, lens_uv[:, 1] * lens_radius, zero], -1)
            focus_point = look_at * focus / np.abs(look_at[:, 2:3])
            d = _normalize(focus_point - e) * flip
        ori, w = _mat_xyz(m, e, one)                    # transform_point: no division by w (:2648-2654)
        if defect == "w_divide":
            ori = ori / w[..., None]
        dirv, _ = _mat_xyz(m, d, T(0.0))               # transform_dir (:2656-2660)
        if defect != "no_final_normalise":
            dirv = _normalize(dirv)
    return ori.astype(T), dirv.astype(T), state.astype(np.uint32)


def origin_scale(camera_params, transform):
    """Magnitude of the operands the origin's three sums add up, per component: |M| applied to the extent of the lens /
    film points, plus the translation.  Deviations of an origin are measured in units of it (0: the component is exact)."""
    cp = camera_params
    m = np.abs(np.asarray(transform, np.float32).reshape(4, 4).astype(np.float64))
    fsx, fsy = (cp.film, cp.film / cp.aspect) if np.float32(cp.aspect) >= 1 else (cp.film * cp.aspect, cp.film)
    ex = ey = cp.aperture / 2.0
    if cp.is_orthographic:
        ex, ey = ex + 0.5 * fsx / cp.lens, ey + 0.5 * fsy / cp.lens
    return np.array([m[0][r] * ex + m[1][r] * ey + m[3][r] for r in range(3)])


# ---- the records of DESIGN.md 19 -------------------------------------------------------------------------------------

def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def transforms():
    rng = np.random.default_rng(19)
    rot = np.eye(4)
    rot[:3, :3], rot[:3, 3] = _rotation(rng), [1.5, -2.0, 7.0]
    scale = np.eye(4)
    scale[:3, :3], scale[:3, 3] = _rotation(rng) @ np.diag([2.0, 0.5, 3.0]), [-0.25, 0.5, 1.0]
    nonaffine = rot.copy()
    nonaffine[3] = [0.25, -0.5, 0.125, 1.5]           # a last row no render has: nothing may read it
    # [column][row] = the transpose of the usual row-major matrix
    return {k: np.ascontiguousarray(v.T, np.float32) for k, v in
            (("identity", np.eye(4)), ("rigid", rot), ("scaled", scale), ("nonaffine", nonaffine))}


def cameras():
    out = []
    for ortho, aperture, aspect, (lens, film), focus in itertools.product(
            (False, True), (0.0, 0.3), (16.0 / 9.0, 1.0, 9.0 / 16.0), ((0.05, 0.036), (0.024, 0.07)), (0.5, 50.0)):
        out.append(api.CameraParams(is_orthographic=ortho, lens=lens, film=film, aspect=aspect, focus=focus, aperture=aperture))
    return out


SIZES = ((1, 1), (7, 5), (64, 40), (4096, 2160))
ACCUM_COUNTERS = (0, 1, 1000)


def pixel_records(width, height):
    """(n, 4) uint32 records of one image size: every pixel (4096 x 2160: the corners and the centre) with the state init_rng
    gives it at accum_counter 0, 1 and 1000 and the states 0 and 0xFFFFFFFF (64 x 40: one of the five per pixel, in turn),
    then every pixel once more in RAY_CENTRE mode."""
    if (width, height) == (4096, 2160):
        px = np.array([(0, 0), (width - 1, 0), (0, height - 1), (width - 1, height - 1), (width // 2, height // 2)], np.uint32)
    else:
        yy, xx = np.meshgrid(np.arange(height, dtype=np.uint32), np.arange(width, dtype=np.uint32), indexing="ij")
        px = np.stack([xx.reshape(-1), yy.reshape(-1)], -1)
    gid = px[:, 1].astype(np.uint64) * np.uint64(width) + px[:, 0]
    states = np.stack([init_rng(gid, c) for c in ACCUM_COUNTERS] +
                      [np.zeros(len(px), np.uint32), np.full(len(px), 0xFFFFFFFF, np.uint32)], 0)      # (5, n)
    if (width, height) == (64, 40):
        which = np.arange(len(px)) % 5
        ray = api.camera_records(px[:, 0], px[:, 1], states[which, np.arange(len(px))], api.CameraMode.RAY)
    else:
        ray = np.concatenate([api.camera_records(px[:, 0], px[:, 1], s, api.CameraMode.RAY) for s in states])
    return np.concatenate([ray, api.camera_records(px[:, 0], px[:, 1], 0, api.CameraMode.RAY_CENTRE)])


class Case:
    def __init__(self, label, width, height, cp, transform, rec):
        self.label, self.width, self.height, self.cp, self.transform, self.rec = label, width, height, cp, transform, rec

    def evaluate(self, dtype=np.float64, defect=None):
        """rays() over the records of both modes: (ori, dir, state afterwards)."""
        centre = self.rec[:, 3] == api.CameraMode.RAY_CENTRE
        ori, d, st = rays(self.width, self.height, self.cp, self.transform, self.rec[:, 0], self.rec[:, 1], self.rec[:, 2], dtype,
                          False, defect)
        o1, d1, _ = rays(self.width, self.height, self.cp, self.transform, self.rec[:, 0], self.rec[:, 1], self.rec[:, 2], dtype,
                         True, defect)
        ori[centre], d[centre], st[centre] = o1[centre], d1[centre], self.rec[centre, 2]
        return ori, d, st


@functools.lru_cache(maxsize=None)
def cases():
    """Every camera x transform x image size of DESIGN.md 19, one Case (= one probe call) each."""
    recs = {s: pixel_records(*s) for s in SIZES}
    out = []
    for ci, cp in enumerate(cameras()):
        for tname, t in transforms().items():
            for (w, h) in SIZES:
                out.append(Case(f"camera {ci} ({'ortho' if cp.is_orthographic else 'persp'} ap {cp.aperture} aspect {cp.aspect:.3f} "
                                f"lens {cp.lens} focus {cp.focus}) / {tname} / {w}x{h}", w, h, cp, t, recs[(w, h)]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def reference():
    """The float64 rays of cases(), computed once: a tuple of (ori, dir, state afterwards)."""
    return tuple(c.evaluate(np.float64) for c in cases())


def deviation(case, ref, got):
    """Worst deviation of `got` from `ref` (each (ori, dir, ...)) over a case's records: (origin, in units of
    origin_scale; direction, absolute: its operands have magnitude 1)."""
    scale = origin_scale(case.cp, case.transform)
    diff = np.abs(np.asarray(got[0], np.float64) - ref[0]).max(0)
    with np.errstate(all="ignore"):
        o = np.where(diff == 0, 0.0, diff / scale)     # a component without operands (scale 0) must be exact: inf otherwise
    d = np.abs(np.asarray(got[1], np.float64) - ref[1])
    return float(np.nanmax(o)) if np.isfinite(o).all() else np.inf, float(d.max()) if np.isfinite(d).all() else np.inf


def worst_deviation(evaluate):
    """max of deviation() over all cases of `evaluate(case) -> (ori, dir, ...)` against reference()."""
    worst = 0.0
    for c, ref in zip(cases(), reference()):
        worst = max(worst, *deviation(c, ref, evaluate(c)))
    return worst


@functools.lru_cache(maxsize=None)
def noise_floor():
    """Worst deviation of the formula evaluated in float32 from float64, over all records."""
    return worst_deviation(lambda c: c.evaluate(np.float32))


TOLERANCE_FACTOR = 4.0          # the kernel's operation order and lpm_sincosf differ from numpy's: a few ulps more, not 10x
UNIT_LENGTH_BOUND = 5.0 * 2.0 ** -24   # | |dir| - 1 |: three squares and two adds (3 u), sqrt (halves it, + u), 1 / . (u), the product (u)


# Measured on the CPU: noise_floor() is 2.88e-7 over the records of cases(); tests/test_camera_film_cpu.py asserts that this
# constant is TOLERANCE_FACTOR floors (to 5 %), so the GPU test need not measure it again.
TOLERANCE = 1.16e-6


def failures(case, ref, got, tol):
    """What is wrong with `got` = (ori, dir, state afterwards) float32 / uint32 for a case, as a list of strings."""
    out = []
    if not np.array_equal(np.asarray(got[2], np.uint32), ref[2]):
        out.append(f"rng_state: {int((np.asarray(got[2], np.uint32) != ref[2]).sum())} records differ")
    o, d = deviation(case, ref, got)
    if not o <= tol:
        out.append(f"origin={o:.3g} > {tol:.3g}")
    if not d <= tol:
        out.append(f"direction={d:.3g} > {tol:.3g}")
    n = np.abs(np.sqrt((np.asarray(got[1], np.float64) ** 2).sum(-1)) - 1.0).max()
    if not n <= UNIT_LENGTH_BOUND:
        out.append(f"unit_length={n:.3g} > {UNIT_LENGTH_BOUND:.3g}")
    return out
