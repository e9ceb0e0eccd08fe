"""Float64 restatement of the reference's light sampling and its pdf, written from the reference's text
(pathtracer.wgsl:2468-2549 sample_lights / sample_lights_pdf, :2551-2638 environment maps and alias picks,
bvh_custom.wgsl:112-152 compute_instance_lights_pdf, data_structures.rs:20-113 build_lights) -- not from the oracle or the
device code.  Plain numpy: no BVH, every triangle of every emissive instance is tested against every query.

Two densities live here, and where they differ is the list of reference properties ("Light sampling on its own"):

  pdf()           what the reference *returns*: the march with its restart at light_pos + incoming and its cap of 100
                  crossings, the model-space area, |n . incoming| with the world-space geometric normal
  true_density()  what the reference's sampler *does*: light 1 / (nl + ne), triangle slot by its alias probability, uniform
                  on that slot's world-space triangle, dist^2 / |cos| summed over every crossing of the ray

Conventions: an instance carries the rows of world -> local (3 x 4); an environment's transform is stored column-major
as (4, 4) [column][row]; directions handed to true_density() are unit vectors."""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

MAX_CROSSINGS = 100


@dataclass
class RefLight:
    instance_idx: int
    area: float                 # model-space area, summed over the triangles (build_lights)
    prob: np.ndarray            # (T,) alias-table probability per slot: model-space area / total, original triangle order
    tris_world: np.ndarray      # (T, 3, 3) world-space corners of the triangle the *sampler* reads at slot t
    normals_world: np.ndarray   # (T, 3) geometric normal as compute_tri_geom_normal builds it
    area_world: np.ndarray      # (T,)


@dataclass
class RefEnv:
    transform: np.ndarray                 # (3, 3) M with world = M local  (columns = env.transform[0..2].xyz)
    weights: Optional[np.ndarray] = None  # (H, W) alias weights of a textured environment, None = uniform sphere
    prob: Optional[np.ndarray] = None     # weights / sum


@dataclass
class RefScene:
    lights: List[RefLight] = field(default_factory=list)
    envs: List[RefEnv] = field(default_factory=list)

    @property
    def n(self):
        return len(self.lights) + len(self.envs)


def local_to_world(rows):
    """Inverse of the affine whose rows (3 x 4) map world to local."""
    rows = np.asarray(rows, np.float64).reshape(3, 4)
    a = np.linalg.inv(rows[:, :3])
    return a, -a @ rows[:, 3]


def tri_areas(v):
    return 0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=-1)


def build(scene_cpu, envs_info, sampled_indices=None):
    """RefScene of an api.SceneCPU.  sampled_indices[mesh] = the index buffer the sampler reads (the BVH builder's
    reordered clone); None = the original order.  The alias weights always come from the original order."""
    out = RefScene()
    for i, inst in enumerate(scene_cpu.instances):
        mat = scene_cpu.materials[int(inst["mat_idx"])]
        mesh = int(inst["mesh_idx"])
        idx = np.asarray(scene_cpu.indices_array[mesh], np.int64).reshape(-1, 3)
        if not np.any(np.asarray(mat["emission"]) != 0.0) or len(idx) == 0:
            continue
        verts = np.asarray(scene_cpu.verts_pos_array[mesh], np.float64)[:, :3]
        w = tri_areas(verts[idx])
        if w.sum() <= 0.0:
            continue
        sidx = idx if sampled_indices is None or sampled_indices[mesh] is None else np.asarray(sampled_indices[mesh], np.int64).reshape(-1, 3)
        rows = np.asarray(inst["transpose_inverse_transform"], np.float64).reshape(3, 4)
        a, t = local_to_world(rows)
        local = verts[sidx]
        world = local @ a.T + t
        ln = np.cross(local[:, 2] - local[:, 0], local[:, 1] - local[:, 0])
        ln /= np.linalg.norm(ln, axis=-1, keepdims=True)
        wn = ln @ rows[:, :3]               # transpose(world -> local) applied to the local normal
        wn /= np.linalg.norm(wn, axis=-1, keepdims=True)
        out.lights.append(RefLight(i, float(w.sum()), w / w.sum(), world, wn, tri_areas(world)))
    for env, info in zip(scene_cpu.environments, envs_info):
        m = np.asarray(env["transform"], np.float64).reshape(4, 4)[:3, :3].T
        if int(env["emission_tex_idx"]) == 0xFFFFFFFF:
            out.envs.append(RefEnv(m))
            continue
        tex = np.asarray(info.data, np.float64).reshape(info.height, info.width, 4)
        scale = np.asarray(env["emission"], np.float64)[:3]
        y = np.arange(info.height)[:, None]
        wts = np.max(tex[..., :3] * scale, axis=-1) * np.sin((y + 0.5) * math.pi / info.height)
        if np.all(scale <= 0.0):
            wts = np.ones_like(wts)
        out.envs.append(RefEnv(m, wts, wts / wts.sum()))
    return out


# ---- ray against every triangle ---------------------------------------------------------------------------------------

def crossings(o, d, tris):
    """Ray o + s d against triangles (T, 3, 3) for queries (Q, 3): s, u, v as (Q, T) arrays (Cramer's rule, float64)."""
    v0 = tris[None, :, 0]
    e1, e2 = tris[None, :, 1] - v0, tris[None, :, 2] - v0
    n = np.cross(e1, e2)
    ro = o[:, None, :] - v0
    dd = d[:, None, :]
    q = np.cross(ro, dd)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.sum(dd * n, -1)
        u = -inv * np.sum(q * e2, -1)
        v = inv * np.sum(q * e1, -1)
        s = -inv * np.sum(n * ro, -1)
    return s, u, v


@dataclass
class PdfResult:
    pdf: np.ndarray          # (Q,)
    edge_margin: np.ndarray  # (Q,) smallest barycentric distance to a triangle edge over crossings ahead of the origin
    eps_margin: np.ndarray   # (Q,) smallest |t - eps| / max(|t|, eps, 1e-30) over the march's accept / reject decisions
    min_cos: np.ndarray      # (Q,) smallest |cos| between a counted crossing's normal and the direction
    texel_margin: np.ndarray  # (Q,) smallest distance, in texels, of the direction to a texel border of a textured environment


def _hits_per_query(o, d, light, chunk):
    """For each query: sorted (s, triangle) of the crossings inside a triangle, and the smallest edge distance met."""
    Q = len(o)
    per = [[] for _ in range(Q)]
    margin = np.full(Q, np.inf)
    T = len(light.tris_world)
    step = max(1, chunk // max(T, 1))
    for a in range(0, Q, step):
        s, u, v = crossings(o[a:a + step], d[a:a + step], light.tris_world)
        m = np.minimum(np.minimum(u, v), 1.0 - u - v)          # > 0 inside, distance to the nearest edge in barycentrics
        ahead = np.isfinite(s) & (s > -1e-3)
        am = np.where(ahead & np.isfinite(m), np.abs(m), np.inf)
        margin[a:a + step] = am.min(axis=1) if T else np.inf
        qi, ti = np.nonzero(ahead & (np.minimum(u, v) >= 0.0) & (u + v <= 1.0))
        for q, t in zip(qi, ti):
            per[a + q].append((s[q, t], t))
    for p in per:
        p.sort()
    return per, margin


def pdf(scene: RefScene, pos, incoming, eps, chunk=4_000_000):
    """sample_lights_pdf at `incoming` (any length), with what decides how well-conditioned each query is."""
    o = np.asarray(pos, np.float64).reshape(-1, 3)
    d = np.asarray(incoming, np.float64).reshape(-1, 3)
    eps = np.broadcast_to(np.asarray(eps, np.float64), (len(o),))
    Q = len(o)
    total = np.zeros(Q)
    edge = np.full(Q, np.inf)
    epsm = np.full(Q, np.inf)
    mcos = np.full(Q, np.inf)
    texm = np.full(Q, np.inf)
    dn = np.linalg.norm(d, axis=-1)
    for light in scene.lights:
        per, margin = _hits_per_query(o, d, light, chunk)
        edge = np.minimum(edge, margin)
        for q in range(Q):
            cur, acc, count = 0.0, 0.0, 0
            for s, t in per[q]:
                if count >= MAX_CROSSINGS:
                    break
                tt = s - cur                                   # distance along the restarted ray
                epsm[q] = min(epsm[q], abs(tt - eps[q]) / max(abs(s), abs(cur), eps[q], 1e-30))
                if tt < eps[q]:
                    continue
                c = abs(float(light.normals_world[t] @ d[q]))
                mcos[q] = min(mcos[q], c / dn[q])
                acc += (s * dn[q]) ** 2 / (c * light.area)
                cur = s + 1.0                                  # next_pos = light_pos + incoming
                count += 1
            total[q] += acc
    for k, env in enumerate(scene.envs):
        if env.weights is None:
            total += 1.0 / (4.0 * math.pi)
            continue
        cx, cy, m = env_dir_to_texel(env, d)
        H, W = env.weights.shape
        solid = (2.0 * math.pi / W) * (math.pi / H) * np.sin(math.pi * (cy + 0.5) / H)
        total += env.prob[cy, cx] / solid
        texm = np.minimum(texm, m)
    return PdfResult(total / max(scene.n, 1), edge, epsm, mcos, texm)


def true_density(scene: RefScene, pos, dirs, slot_prob=None, chunk=4_000_000):
    """Solid-angle density of sample_lights' mesh and uniform-environment samples at unit directions `dirs`.
    slot_prob[light] overrides the per-slot pick probability (default: the alias weights).  Textured environments are
    point masses and are not part of a density: their share is missing from the integral of this function."""
    o = np.asarray(pos, np.float64).reshape(-1, 3)
    d = np.asarray(dirs, np.float64).reshape(-1, 3)
    out = np.zeros(len(o))
    for li, light in enumerate(scene.lights):
        p = light.prob if slot_prob is None else slot_prob[li]
        T = len(light.tris_world)
        step = max(1, chunk // T)
        for a in range(0, len(o), step):
            s, u, v = crossings(o[a:a + step], d[a:a + step], light.tris_world)
            inside = np.isfinite(s) & (s > 0.0) & (np.minimum(u, v) >= 0.0) & (u + v <= 1.0)
            c = np.abs(d[a:a + step] @ light.normals_world.T)
            with np.errstate(divide="ignore", invalid="ignore"):
                term = np.where(inside, s * s / c * (p / light.area_world)[None, :], 0.0)
            out[a:a + step] += term.sum(axis=1)
    out += sum(1 for e in scene.envs if e.weights is None) / (4.0 * math.pi)
    return out / max(scene.n, 1)


# ---- the sampler for given draws ------------------------------------------------------------------------------------------

PICK_ULPS = 8.0 * 2.0 ** -24     # rnd * n is one f32 product of exact numbers: a relative rounding of 2^-24, taken eight times


def attach_tables(scene: RefScene, alias_tables, env_alias_tables):
    """Hand the sampler the alias bins the scene was uploaded with (api.build_lights' tables: data, in light / environment
    order).  The thresholds and the draws are f32 numbers, so `rnd >= threshold` is an exact comparison."""
    for light, t in zip(scene.lights, alias_tables):
        light.bins = t
    for env, t in zip(scene.envs, env_alias_tables):
        env.bins = t


def _pick(r, n):
    """random_u32_range_unsafe for a drawn r: min(u32(r * n), n - 1), and its margin (> 1: no f32 rounding changes it)."""
    x = r * float(n)
    k = np.minimum(np.floor(x).astype(np.int64), n - 1)
    near = np.abs(x - np.round(x))
    with np.errstate(divide="ignore"):
        margin = np.where((np.round(x) >= 1) & (np.round(x) <= n - 1), near / (PICK_ULPS * np.maximum(x, 1.0)), np.inf)
    return k, margin


def _alias(bins, state, random_f32):
    n = len(bins)
    state, r = random_f32(state)
    k, margin = _pick(r, n)
    state, r2 = random_f32(state)
    thr = np.asarray(bins["alias_threshold"], np.float64)[k]
    return np.where(r2 >= thr, np.asarray(bins["alias"], np.int64)[k], k), state, margin


def sample(scene: RefScene, pos, rng_state):
    """sample_lights (pathtracer.wgsl:2468-2514, :2610-2638, :1675-1679) for the draws that follow rng_state, per query: the
    pick among mesh lights and environments, the alias pick of a slot, the point on the slot's triangle (the triangle the
    sampler reads: tris_world), the uniform sphere (not turned by the environment's transform) or the alias pick of a texel
    and its centre.  Returns (direction (Q, 3), RNG state afterwards (Q,) uint64, margin (Q,)): the margin is the smallest
    distance of a rnd * n to an integer in units of its f32 rounding; above 1 every pick is certain.  Needs attach_tables."""
    from tests.camera_ref import random_f32
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    state = np.asarray(rng_state, np.uint64).copy()
    Q = len(pos)
    out, margin = np.zeros((Q, 3)), np.full(Q, np.inf)
    nl, n = len(scene.lights), scene.n
    if n == 0:
        return out, state, margin
    state, r = random_f32(state)
    which, margin = _pick(r, n)
    for li in range(n):
        sel = np.nonzero(which == li)[0]
        if not len(sel):
            continue
        if li < nl:
            light = scene.lights[li]
            slot, st, m = _alias(light.bins, state[sel], random_f32)
            st, r0 = random_f32(st)
            st, r1 = random_f32(st)
            u, v = 1.0 - np.sqrt(r0), r1 * np.sqrt(r0)
            t = light.tris_world[slot]
            p = t[:, 0] * (1.0 - u - v)[:, None] + t[:, 1] * u[:, None] + t[:, 2] * v[:, None]
            d = p - pos[sel]
            out[sel] = d / np.linalg.norm(d, axis=-1, keepdims=True)
        else:
            env = scene.envs[li - nl]
            if env.weights is None:
                st, r0 = random_f32(state[sel])
                st, r1 = random_f32(st)
                z = 2.0 * r1 - 1.0
                rr = np.sqrt(np.clip(1.0 - z * z, 0.0, 1.0))
                out[sel] = np.stack([rr * np.cos(2.0 * math.pi * r0), rr * np.sin(2.0 * math.pi * r0), z], -1)
                m = np.full(len(sel), np.inf)
            else:
                texel, st, m = _alias(env.bins, state[sel], random_f32)
                out[sel] = env_texel_to_dir(env, texel)
        state[sel] = st
        margin[sel] = np.minimum(margin[sel], m)
    return out, state, margin


# ---- solid angles -------------------------------------------------------------------------------------------------------

def solid_angle(pos, tris):
    """Sum of the unsigned solid angles of triangles (T, 3, 3) seen from pos (Van Oosterom and Strackee, 1983)."""
    r = np.asarray(tris, np.float64) - np.asarray(pos, np.float64)
    a, b, c = r[:, 0], r[:, 1], r[:, 2]
    la, lb, lc = (np.linalg.norm(x, axis=-1) for x in (a, b, c))
    num = np.sum(a * np.cross(b, c), -1)
    den = la * lb * lc + np.sum(a * b, -1) * lc + np.sum(a * c, -1) * lb + np.sum(b * c, -1) * la
    return float(np.sum(np.abs(2.0 * np.arctan2(num, den))))


# ---- environment maps -----------------------------------------------------------------------------------------------------

def env_texel_to_dir(env: RefEnv, idx):
    """env_idx_to_dir: the centre of texel idx (row-major) as a world direction."""
    H, W = env.weights.shape
    idx = np.asarray(idx, np.int64)
    u = (idx % W + 0.5) / W
    v = (idx // W + 0.5) / H
    local = np.stack([np.cos(2 * math.pi * u) * np.sin(math.pi * v), np.cos(math.pi * v), np.sin(2 * math.pi * u) * np.sin(math.pi * v)], -1)
    w = local @ env.transform.T
    return w / np.linalg.norm(w, axis=-1, keepdims=True)


def env_dir_to_uv(env: RefEnv, d):
    """dir_to_env_uv: the columns of the transform dotted with the direction, normalised; u from atan2(z, x), v from acos(y)."""
    t = np.asarray(d, np.float64) @ env.transform
    t = t / np.linalg.norm(t, axis=-1, keepdims=True)
    u = np.arctan2(t[:, 2], t[:, 0]) / (2 * math.pi)
    u = np.where(u < 0.0, u + 1.0, u)
    return u, np.arccos(np.clip(t[:, 1], -1.0, 1.0)) / math.pi


def env_dir_to_texel(env: RefEnv, d):
    """dir_to_env_coords, and the direction's distance to the nearest texel border in texels."""
    H, W = env.weights.shape
    u, v = env_dir_to_uv(env, d)
    x, y = u * W, v * H
    cx = np.clip(np.floor(x).astype(np.int64), 0, W - 1)
    cy = np.clip(np.floor(y).astype(np.int64), 0, H - 1)
    # borders: every integer in x (the seam included) unless the row is one texel; the interior integers in y (no pole)
    mx = np.abs(x - np.round(x)) if W > 1 else np.full(len(x), np.inf)
    ry = np.round(y)
    my = np.where((ry >= 1) & (ry <= H - 1), np.abs(y - ry), np.inf)
    m = np.minimum(mx, my)
    return cx, cy, m


def env_pdf_integral(env: RefEnv):
    """Integral over the sphere of prob / solid_angle: each texel's exact solid angle times its constant density."""
    H, W = env.weights.shape
    y = np.arange(H)
    exact = (2.0 * math.pi / W) * (np.cos(math.pi * y / H) - np.cos(math.pi * (y + 1) / H))
    stated = (2.0 * math.pi / W) * (math.pi / H) * np.sin(math.pi * (y + 0.5) / H)
    return float(np.sum(env.prob * (exact / stated)[:, None]))


# ---- alias tables ---------------------------------------------------------------------------------------------------------

def alias_realised(bins):
    """Probability each slot is returned by the pick `slot = uniform bin; r >= threshold -> alias` (thresholds in [0, 1])."""
    n = len(bins)
    thr = np.clip(np.asarray(bins["alias_threshold"], np.float64), 0.0, 1.0)
    out = thr / n
    np.add.at(out, np.asarray(bins["alias"], np.int64), (1.0 - thr) / n)
    return out
