"""float64 judgement of transmittance queries: numpy only, nothing shared with the traversal.  Built from two
references the project already trusts:

  crossings   Moller-Trumbore of every ray against every triangle of every instance on closest_hit_ref.geometry(scene), with
              closest_hit_ref's error bands (K_BOUND, S_DECISIVE).  Each (ray, triangle) pair is a CERTAIN crossing of
              [eps, tmax), CERTAINLY NOT one, or UNCERTAIN: inside the band of an edge, of eps or of tmax, or with a
              determinant within its own f32 error of zero.  (A determinant that is zero by structure -- every product has a
              factor that is exactly 0 -- is 0 in f32 as well: tri_dst then computes infinities or NaN and rejects, so such
              a pair is certainly not a crossing, exactly as closest_hit_ref treats it.)
  opacity     surface_ref.SurfaceRef.material_point at each certain crossing of an alpha-capable instance, with its
              forward-error bound (conditioning x C_OPACITY x 2^-24), plus what the f32 (u, v) of the triangle test can move
              it: the vertex alphas' and the texture's Lipschitz constants times tol_uv.

Expected T = product of 1 - clip(a, 0, 1) over the certain crossings, 0 if any a >= 1 or any crossing lies in an instance
that cannot have an opacity other than 1.  A ray is DECISIVE iff it has no uncertain pair; the others are left out.

  tol_T = sum_k tol_a,k prod_{j != k} (1 - a_j)  +  K_LEAF 2^-24 (n + 1)

K_LEAF is fitted, not guessed (leaf_fit below; tests/test_transmittance_cpu.py asserts the rounding).  Where a crossing's
reference opacity is within tol_a of 1, f32 may or may not see a < 1: both 0 and the product within tol_T are accepted.

Also here: the alpha scenes, the ray sets (drawn 1.25 times over and chosen on the CPU by the reference alone, as DESIGN.md
20 does), the numpy f32 restatement of the resolve order, and the closed forms."""
import math
from dataclasses import dataclass

import numpy as np

from lupinpathtracer_amd import api
from tests import closest_hit_ref as X
from tests import occlusion_ref as R
from tests import reproject_ref
from tests import surface_ref

U32 = X.U32
C_OPACITY = 5.0            # tests/test_surface_probe.py C_MODE["MATERIAL"]: the measured constant of surface_ref's conditioning
K_LEAF = 2.0               # fitted: four times the worst measured error of leaf_product_f32, rounded up
OVERDRAW = 1.25
MAX_LEFT_OUT = 0.01
TMAX_SETTINGS = ("half", "twice", "unbounded")
GROUPS = {"main": ("aimed", "uniform", "inside"), "special": ("axis", "zero_component", "surface_away", "surface_into", "far")}
SENTINEL = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------------
# The alpha scenes: closest_hit_ref's big / small with alpha from each of the three sources and their combinations
# ------------------------------------------------------------------------------------------------

MAT_ALPHA = (1.0, 0.25, 0.5, float(1.0 - 2.0 ** -24), 0.0)         # materials 0 .. 4: colour alpha alone
MAT_TEX, MAT_TEX_HALF = 5, 6                                        # the 8 x 8 texture; the texture and colour alpha 0.5
GRID_UV, BLOB_COL, QUAD_UV_COL = 5, 6, 7                            # meshes appended after closest_hit_ref's five
# instance -> (mesh override or None, material): 1, 4, 6, 11 stay opaque
ASSIGN = {0: (None, 2), 1: (None, 0), 2: (None, 1), 3: (GRID_UV, MAT_TEX), 4: (None, 0), 5: (BLOB_COL, 0), 6: (None, 0), 7: (BLOB_COL, 2),
          8: (None, 3), 9: (QUAD_UV_COL, MAT_TEX_HALF), 10: (None, 4), 11: (None, 0), 12: (None, 1)}
OPAQUE_INSTANCES = (1, 4, 6, 11)


def alpha_texture():
    """8 x 8 RGBA8: alpha 0, 255 and intermediate texels."""
    rng = np.random.default_rng(5)
    t = rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)
    a = rng.integers(1, 255, (8, 8), dtype=np.uint8)
    a[rng.random((8, 8)) < 0.3] = 0
    a[rng.random((8, 8)) < 0.25] = 255
    a[0, 0], a[3, 4], a[5, 5] = 0, 255, 128
    t[..., 3] = a
    return np.ascontiguousarray(t)


def alpha_scene_cpu(kind, seed=X.SEED, xf=None, opaque=False):
    """(SceneCPU, textures).  opaque: the same geometry and attributes with every source of alpha removed (material alpha 1,
    no texture reference, no vertex colours): no instance is alpha-capable."""
    sc = X.scene_cpu(kind, seed, xf)
    rng = np.random.default_rng(seed + 77)
    mats = np.array([api.default_material() for _ in range(7)], api.MATERIAL_DTYPE)
    for i in range(7):
        mats[i]["color"] = (0.5, 0.5, 0.5, MAT_ALPHA[i] if i < 5 else (1.0 if i == MAT_TEX else 0.5))
    mats[MAT_TEX]["color_tex_idx"] = mats[MAT_TEX_HALF]["color_tex_idx"] = 0
    sc.materials = mats
    infos = []
    for src, uv, col in ((X.GRID, True, False), (X.BLOB, False, True), (X.QUAD_MESH, True, True)):
        v = sc.verts_pos_array[src].copy()
        sc.verts_pos_array.append(v)
        sc.indices_array.append(sc.indices_array[src].copy())
        info = api.default_mesh_info()
        if uv:
            info["texcoords_buf_idx"] = len(sc.verts_texcoord_array)
            tc = np.stack([v[:, 0] * 0.7 + 0.1, (v[:, 2] if src == X.GRID else v[:, 1]) * 0.9 - 0.2], -1) + rng.uniform(-0.05, 0.05, (len(v), 2))
            sc.verts_texcoord_array.append(tc.astype(np.float32))
        if col:
            info["colors_buf_idx"] = len(sc.verts_color_array)
            c = rng.uniform(0.2, 1.0, (len(v), 4)).astype(np.float32)
            c[::5, 3] = 1.0
            c[1::7, 3] = 0.0
            sc.verts_color_array.append(c)
        infos.append(info)
    sc.mesh_infos = np.concatenate([sc.mesh_infos, np.array(infos, api.MESH_INFO_DTYPE)])
    for i, (mesh, mat) in ASSIGN.items():
        if mesh is not None:
            sc.instances[i]["mesh_idx"] = mesh
        sc.instances[i]["mat_idx"] = mat
    textures = [api.TextureCPU(alpha_texture())]
    if opaque:
        sc.materials["color"][:, 3] = 1.0
        sc.materials["color_tex_idx"] = SENTINEL
        for info in sc.mesh_infos:
            info["colors_buf_idx"] = SENTINEL
        sc.verts_color_array = []
    api.validate_scene(sc, len(textures), len(textures))
    return sc, textures


def build(kind, ctx=None, xf=None, opaque=False, **kw):
    sc, textures = alpha_scene_cpu(kind, X.SEED, xf, opaque)
    return sc, textures, api.build_accel_structures_and_upload(ctx, sc, textures, [], True, **kw)


def alpha_capable(sc):
    """Instance flag bit 0 as the upload sets it: material colour alpha != 1, a colour texture on a mesh with texcoords, or
    vertex colours."""
    out = np.zeros(len(sc.instances), bool)
    for i, ins in enumerate(sc.instances):
        mat, info = sc.materials[int(ins["mat_idx"])], sc.mesh_infos[int(ins["mesh_idx"])]
        out[i] = (np.float32(mat["color"][3]) != np.float32(1.0)) or \
                 (int(mat["color_tex_idx"]) != SENTINEL and int(info["texcoords_buf_idx"]) != SENTINEL) or int(info["colors_buf_idx"]) != SENTINEL
    return out


# ------------------------------------------------------------------------------------------------
# Crossings: every (ray, triangle) pair that could be one, with closest_hit_ref's bands
# ------------------------------------------------------------------------------------------------

@dataclass
class Pairs:
    """The pairs that are possibly inside their triangle and possibly at t >= 0, sparse; everything else is certainly not a
    crossing for any eps >= 0."""
    n_rays: int
    ray: np.ndarray
    inst: np.ndarray
    tri: np.ndarray        # mesh-local triangle index, in the scene's (BLAS leaf) order
    t: np.ndarray
    u: np.ndarray
    v: np.ndarray
    tol_uv: np.ndarray
    tn: np.ndarray         # t D
    D: np.ndarray
    E_t: np.ndarray
    E_D: np.ndarray
    inside: np.ndarray     # certainly inside the triangle, determinant clear of zero


def pairs(g, ori, dir_, s=X.S_DECISIVE, k=X.K_BOUND):
    o_all, d_all = np.asarray(ori, np.float64).reshape(-1, 3), np.asarray(dir_, np.float64).reshape(-1, 3)
    cols = {key: [] for key in ("ray", "inst", "tri", "t", "u", "v", "tol_uv", "tn", "D", "E_t", "E_D", "inside")}
    for a in range(0, len(o_all), X.CHUNK):
        o, d = o_all[a:a + X.CHUNK], d_all[a:a + X.CHUNK]
        for i in range(len(g.rows)):
            m = g.meshes[g.mesh_idx[i]]
            if not len(m.tris):
                continue
            p = X._pre(m)
            Rm, tr = g.rows[i, :, :3], g.rows[i, :, 3]
            co, cd = o @ Rm.T + tr, d @ Rm.T
            A = np.cross(co, cd)
            det = cd @ p["nn"].T
            sgn = np.where(det < 0, -1.0, 1.0)
            D = np.abs(det)
            nu = (cd @ p["c2"].T - A @ p["e2"].T) * sgn
            nv = (A @ p["e1"].T - cd @ p["c1"].T) * sgn
            tn = (p["nv0"][None] - co @ p["nn"].T) * sgn
            nw = D - nu - nv
            L = np.linalg.norm(np.abs(o) @ np.abs(Rm).T + np.abs(tr), axis=1)[:, None] + p["v0n"][None]
            dn = np.linalg.norm(np.abs(d) @ np.abs(Rm).T, axis=1)[:, None]
            E_uv = k * U32 * L * dn * p["emax"][None]
            E_D = k * U32 * dn * p["ee"][None]
            E_t = k * U32 * L * p["ee"][None]
            zc = ((Rm[None] == 0) | (d[:, None, :] == 0)).all(-1)
            sz = (zc[:, None, :] | p["zn"][None]).all(-1)
            band = np.maximum(E_uv + E_D, s * D)
            in_poss = (nu >= -band) & (nv >= -band) & (nw >= -2 * band) & ~sz
            in_cert = (nu >= band) & (nv >= band) & (nw >= 2 * band) & (D > 2 * E_D)
            r, j = np.nonzero(in_poss & (tn >= -E_t))
            with np.errstate(all="ignore"):
                Dp = D[r, j]
                cols["t"].append(tn[r, j] / Dp); cols["u"].append(nu[r, j] / Dp); cols["v"].append(nv[r, j] / Dp)
                cols["tol_uv"].append((E_uv[r, j] + E_D[r, j]) / Dp)
            cols["ray"].append(r + a); cols["inst"].append(np.full(len(r), i)); cols["tri"].append(j)
            cols["tn"].append(tn[r, j]); cols["D"].append(Dp); cols["E_t"].append(E_t[r, j]); cols["E_D"].append(E_D[r, j])
            cols["inside"].append(in_cert[r, j])
    return Pairs(len(o_all), *[np.concatenate(cols[key]) for key in ("ray", "inst", "tri", "t", "u", "v", "tol_uv", "tn", "D", "E_t", "E_D", "inside")])


def classify(P, eps, tmax, s=X.S_DECISIVE, inclusive=False, ignore_eps=False):
    """(certain, uncertain) per pair for the segment [eps, tmax[ray]); tmax (N,) float64, inf = unbounded.
    inclusive / ignore_eps: the planted twins' readings (t <= tmax; no lower bound)."""
    tm = np.asarray(tmax, np.float64)[P.ray]
    e = 0.0 if ignore_eps else float(eps)
    band_lo = P.E_t + e * P.E_D + s * e * P.D
    cert_lo, poss_lo = P.tn >= e * P.D + band_lo, P.tn >= e * P.D - band_lo
    if ignore_eps:
        cert_lo, poss_lo = P.tn > band_lo, P.tn >= -band_lo
    fin = np.isfinite(tm)
    tmf = np.where(fin, tm, 0.0)
    band_hi = P.E_t + tmf * P.E_D + s * tmf * P.D
    if inclusive:
        cert_hi, poss_hi = ~fin | (P.tn <= tmf * P.D), ~fin | (P.tn <= tmf * P.D + band_hi)
    else:
        cert_hi, poss_hi = ~fin | (P.tn <= tmf * P.D - band_hi), ~fin | (P.tn < tmf * P.D + band_hi)
    certain = P.inside & cert_lo & cert_hi
    return certain, poss_lo & poss_hi & ~certain


def first_crossing(P, eps):
    """Per ray, the smallest t of a pair that is possibly a crossing of [eps, inf); inf where there is none."""
    certain, uncertain = classify(P, eps, np.full(P.n_rays, np.inf))
    t1 = np.full(P.n_rays, np.inf)
    sel = certain | uncertain
    np.minimum.at(t1, P.ray[sel], np.where(np.isfinite(P.t[sel]), P.t[sel], np.inf))
    return t1


def tmax_for(P, eps, setting):
    """float32 tmax per ray: half / twice the first crossing (R.MISS_TMAX times the factor where there is none or where it
    is not clearly positive), or +inf."""
    if setting == "unbounded":
        return np.full(P.n_rays, np.inf, np.float32)
    f = 0.5 if setting == "half" else 2.0
    t1 = first_crossing(P, eps)
    usable = np.isfinite(t1) & (t1 > 1e-6)          # (a record's tmax must be positive: an origin on a surface has t1 about 0)
    return np.where(usable, f * np.where(usable, t1, 0.0), f * R.MISS_TMAX).astype(np.float32)


# ------------------------------------------------------------------------------------------------
# Opacity at a crossing
# ------------------------------------------------------------------------------------------------

class Opacity:
    """Reference opacity and its tolerance per (instance, triangle, u, v), cached by pair index."""

    def __init__(self, sc, textures, scene):
        idx = [reproject_ref.mesh_arrays(scene, i)[1] for i in range(scene.desc.num_meshes)]
        self.ref = surface_ref.SurfaceRef(sc, textures, idx)
        self.sc = sc
        self.capable = alpha_capable(sc)
        self.cache = {}
        self.lip = []
        for t in self.ref.tex:
            a = t.t[..., 3]
            self.lip.append((float(np.abs(a - np.roll(a, 1, 1)).max()) * t.w, float(np.abs(a - np.roll(a, 1, 0)).max()) * t.h))

    def at(self, inst, tri, u, v, tol_uv, variant=None):
        """(a, tol_a).  The forward error of the f32 evaluation at exact (u, v), plus the change over |du|, |dv| <= tol_uv:
        vertex alpha moves by (|a1 - a0| + |a2 - a0|) tol_uv, the texture's alpha by its Lipschitz constants times the
        texcoords' movement; the product rule joins them."""
        key = (inst, tri, u, v, variant)
        if key not in self.cache:
            val, cond, _ = self.ref.material_point(inst, tri, u, v, variant)
            a, tol = val["opacity"], C_OPACITY * U32 * cond["opacity"]
            ins, mesh, info, mat, ids = self.ref._tri(inst, tri)
            ma = abs(float(mat["color"][3]))
            vc, d_vc = 1.0, 0.0
            if int(info["colors_buf_idx"]) != SENTINEL:
                al = [float(self.sc.verts_color_array[int(info["colors_buf_idx"])][k][3]) for k in ids]
                vc = abs(al[0] * (1 - u - v) + al[1] * u + al[2] * v)
                d_vc = (abs(al[1] - al[0]) + abs(al[2] - al[0])) * tol_uv
            ta, d_ta = 1.0, 0.0
            if int(info["texcoords_buf_idx"]) != SENTINEL and int(mat["color_tex_idx"]) != SENTINEL:
                (tc, _), uv = self.ref.texcoords(inst, tri, u, v)
                lu, lv = self.lip[int(mat["color_tex_idx"])]
                d_ta = (lu * (abs(uv[1][0] - uv[0][0]) + abs(uv[2][0] - uv[0][0])) + lv * (abs(uv[1][1] - uv[0][1]) + abs(uv[2][1] - uv[0][1]))) * tol_uv
                ta = abs(self.ref.tex[int(mat["color_tex_idx"])].sample(tc[0], tc[1])[0][3])
            tol += ma * (vc * d_ta + ta * d_vc + d_ta * d_vc)
            self.cache[key] = (a, tol)
        return self.cache[key]


# ------------------------------------------------------------------------------------------------
# Expected transmittance
# ------------------------------------------------------------------------------------------------

@dataclass
class Expect:
    T: np.ndarray          # (N,) float64
    tol: np.ndarray        # (N,)
    zero_ok: np.ndarray    # (N,) bool: 0 is accepted beside T within tol (an opacity within its tolerance of 1)
    decisive: np.ndarray   # (N,) bool
    n: np.ndarray          # (N,) certain crossings
    only_opaque: np.ndarray  # (N,) bool: every certain crossing lies in an instance that is not alpha-capable


def expected(P, op, eps, tmax, k_leaf=K_LEAF, **variant):
    """variant: inclusive / ignore_eps (classify), ignore_flag (a crossing in a flag-clear instance is not counted), summed
    (T = 1 - sum of opacities): the planted twins."""
    ignore_flag, summed = variant.pop("ignore_flag", False), variant.pop("summed", False)
    certain, uncertain = classify(P, eps, tmax, **variant)
    N = P.n_rays
    decisive = np.ones(N, bool)
    decisive[P.ray[uncertain]] = False
    T, tol, zero_ok, n = np.ones(N), np.zeros(N), np.zeros(N, bool), np.zeros(N, int)
    only_opaque = np.ones(N, bool)
    by_ray = {}
    for q in np.nonzero(certain)[0]:
        by_ray.setdefault(int(P.ray[q]), []).append(q)
    for r, qs in by_ray.items():
        n[r] = len(qs)
        if not decisive[r]:
            continue
        fac, tols, dead = [], [], False
        for q in qs:
            i = int(P.inst[q])
            if op.capable[i]:
                only_opaque[r] = False
            else:
                dead = dead or not ignore_flag      # the twin lets a flag-clear instance through untouched
                continue
            a, ta = op.at(i, int(P.tri[q]), float(P.u[q]), float(P.v[q]), float(P.tol_uv[q]))
            if a - ta >= 1.0:
                dead = True
            elif a + ta >= 1.0:
                zero_ok[r] = True
            fac.append(1.0 - min(max(a, 0.0), 1.0)); tols.append(ta)
        if dead:
            T[r], tol[r], zero_ok[r] = 0.0, 0.0, False
            continue
        if summed:
            T[r] = 1.0 - sum(1.0 - f for f in fac)
        else:
            T[r] = float(np.prod(fac))
        tol[r] = sum(tols[k] * float(np.prod(fac[:k] + fac[k + 1:])) for k in range(len(fac))) + k_leaf * U32 * (len(fac) + 1)
    return Expect(T, tol, zero_ok, decisive, n, only_opaque)


def disagreements(exp, got):
    """Decisive rays whose T is neither within tol of the expected value nor an accepted 0."""
    got = np.asarray(got, np.float64)
    ok = (np.abs(got - exp.T) <= exp.tol) | (exp.zero_ok & (got == 0.0))
    return int((exp.decisive & ~ok).sum())


# ------------------------------------------------------------------------------------------------
# The leaf arithmetic, restated in f32, and the fit of K_LEAF
# ------------------------------------------------------------------------------------------------

def leaf_product_f32(alphas):
    """T = T * (1.0f - fmaxf(a, 0.0f)) over f32 opacities below 1, in order."""
    T = np.float32(1.0)
    for a in alphas:
        T = np.float32(T * np.float32(np.float32(1.0) - np.maximum(np.float32(a), np.float32(0.0))))
    return T


def leaf_fit(alpha_lists):
    """The worst error of leaf_product_f32 against the float64 product of the same f32 opacities, in units of 2^-24 (n + 1)."""
    worst = 0.0
    for al in alpha_lists:
        al = [np.float32(a) for a in al]
        exact = float(np.prod([1.0 - max(float(a), 0.0) for a in al])) if al else 1.0
        worst = max(worst, abs(float(leaf_product_f32(al)) - exact) / (U32 * (len(al) + 1)))
    return worst


def leaf_alpha_lists(P, op, eps, tmax):
    """Per decisive ray with crossings, the f32-rounded reference opacities of its alpha-capable crossings that are below 1."""
    certain, uncertain = classify(P, eps, tmax)
    bad = np.zeros(P.n_rays, bool)
    bad[P.ray[uncertain]] = True
    lists = {}
    for q in np.nonzero(certain)[0]:
        r, i = int(P.ray[q]), int(P.inst[q])
        if bad[r] or not op.capable[i]:
            continue
        a = np.float32(op.at(i, int(P.tri[q]), float(P.u[q]), float(P.v[q]), float(P.tol_uv[q]))[0])
        if a < np.float32(1.0):
            lists.setdefault(r, []).append(a)
    return list(lists.values())


# ------------------------------------------------------------------------------------------------
# The resolve order, restated
# ------------------------------------------------------------------------------------------------

def resolve_sum_f32(T):
    """k_transmittance_resolve on one record's slots T (S,) f32: 64 partial sums p[l] = ((0 + T[l]) + T[l + 64]) + ..., then
    for off = 32, 16, 8, 4, 2, 1: p[l] = p[l] + p[l ^ off]; the result is p[0]."""
    T = np.asarray(T, np.float32)
    p = np.zeros(64, np.float32)
    for first in range(0, len(T), 64):
        row = T[first:first + 64]
        p[:len(row)] = p[:len(row)] + row
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        p = (p + p[lanes ^ off]).astype(np.float32)
    return p[0]


# ------------------------------------------------------------------------------------------------
# Rays: closest_hit_ref's families less the three that are not of unit length, drawn OVERDRAW times over, chosen by the
# reference alone
# ------------------------------------------------------------------------------------------------

def target_counts(kind):
    return {name: (0 if name in R.NOT_UNIT_FAMILIES else c) for name, c in X.MAIN_COUNTS[kind].items()}


def undecided_anywhere(P):
    """Per ray: undecided at some ray_epsilon of closest_hit_ref.EPSILONS and some tmax setting."""
    und = np.zeros(P.n_rays, bool)
    for eps in X.EPSILONS:
        for setting in TMAX_SETTINGS:
            _, uncertain = classify(P, eps, tmax_for(P, eps, setting).astype(np.float64))
            und[P.ray[uncertain]] = True
    return und


def choose(family, undecided, counts):
    """Indices of the chosen candidates.  Per family group, in candidate order: floor(1 %) of the group's target that the
    reference cannot decide STAY (if there are that many), the rest are decided ones."""
    names = np.array(X.FAMILIES)[family]
    keep, raw = [], {}
    for group, fams in GROUPS.items():
        cand = np.nonzero(np.isin(names, fams))[0]
        n = sum(counts[f] for f in fams)
        raw[group] = float(undecided[cand].mean())
        und = cand[undecided[cand]][:n // 100]
        dec = cand[~undecided[cand]][:n - len(und)]
        assert len(und) + len(dec) == n, f"{group}: too few decided candidates; raise OVERDRAW"
        keep.append(np.concatenate([und, dec]))
    return np.sort(np.concatenate(keep)), raw


_cases = {}


@dataclass
class Case:
    kind: str
    sc: object
    textures: list
    scene: object          # host build (ctx = None)
    g: X.Geometry
    ori: np.ndarray
    dir: np.ndarray
    family: np.ndarray
    P: Pairs
    op: Opacity
    raw_undecided: dict    # group -> share of the raw draw the reference cannot decide


def case(kind, moved=False):
    """`big` / `small` at closest_hit_ref.SEED; moved: under closest_hit_ref's second set of transforms, a third of the rays."""
    key = (kind, moved)
    if key not in _cases:
        sc, textures, scene = build(kind, xf=X.transforms(X.SEED, moved))
        g = X.geometry(scene)
        counts = target_counts(kind)
        if moved:
            counts = {name: c // 3 for name, c in counts.items()}
        draw = {name: int(math.ceil(c * OVERDRAW)) for name, c in counts.items()}
        ori, d, fam = X.make_rays(g, X.SEED + (22 if moved else 21), draw)
        P0 = pairs(g, ori, d)
        pick, raw = choose(fam, undecided_anywhere(P0), counts)
        ori, d, fam = ori[pick], d[pick], fam[pick]
        _cases[key] = Case(kind, sc, textures, scene, g, ori, d, fam, pairs(g, ori, d), Opacity(sc, textures, scene), raw)
    return _cases[key]


def left_out_shares(c, exp):
    """group -> share of its rays that `exp` leaves out."""
    names = np.array(X.FAMILIES)[c.family]
    return {group: float(1.0 - exp.decisive[np.isin(names, fams)].mean()) for group, fams in GROUPS.items()}


# ------------------------------------------------------------------------------------------------
# Small exact scenes and closed forms
# ------------------------------------------------------------------------------------------------

def stacked_quads(alphas, z0=6.0, dz=1.0, vertex_alpha=None, texture=None, textured=(0,), ctx=None):
    """(sc, textures, scene): copies of closest_hit_ref's quad under the exact quad's transform style (scale 2, integer shifts)
    at z = z0, z0 + dz, ..., copy k with material colour alpha alphas[k].  vertex_alpha: four alphas on the quad's vertices (one
    shared mesh).  texture: (pixels, texcoords (4, 2)), referenced by the materials of the copies in `textured`."""
    sc = api.SceneCPU()
    mats = np.array([api.default_material() for _ in alphas], api.MATERIAL_DTYPE)
    for i, a in enumerate(alphas):
        mats[i]["color"] = (0.5, 0.5, 0.5, a)
        if texture is not None and i in textured:
            mats[i]["color_tex_idx"] = 0
    sc.materials = mats
    sc.verts_pos_array.append(X.QUAD[0].copy())
    sc.indices_array.append(X.QUAD[1].copy())
    info = api.default_mesh_info()
    if vertex_alpha is not None:
        info["colors_buf_idx"] = 0
        col = np.ones((4, 4), np.float32)
        col[:, 3] = vertex_alpha
        sc.verts_color_array.append(col)
    if texture is not None:
        info["texcoords_buf_idx"] = 0
        sc.verts_texcoord_array.append(np.asarray(texture[1], np.float32))
    sc.mesh_infos = np.array([info], api.MESH_INFO_DTYPE)
    sc.instances = np.array([api.instance_from_transform(X.mat3x4(np.diag([2.0, 2.0, 2.0]), (4.0, -2.0, z0 + dz * k)), 0, k) for k in range(len(alphas))],
                            api.INSTANCE_DTYPE)
    textures = [api.TextureCPU(np.ascontiguousarray(texture[0]))] if texture is not None else []
    api.validate_scene(sc, len(textures), len(textures))
    return sc, textures, api.build_accel_structures_and_upload(ctx, sc, textures, [], True)


def reference_T(sc, textures, scene, ori, dir_, eps, tmax, **variant):
    """Expect for a small scene, straight from the definition."""
    g = X.geometry(scene)
    P = pairs(g, ori, dir_)
    tm = np.broadcast_to(np.asarray(tmax, np.float64), (P.n_rays,))
    return expected(P, Opacity(sc, textures, scene), eps, tm, **variant)


def ceiling_mean_visibility(h, radius, alpha):
    """A floor under a ceiling of opacity alpha at height h: the cosine-weighted measure of the directions that meet it within
    `radius` is 1 - (h / radius)^2 (occlusion_ref.ceiling_blocked_fraction); each of them lets 1 - alpha through."""
    return 1.0 - alpha * R.ceiling_blocked_fraction(h, radius)


def ceiling_sigma(h, radius, alpha, samples):
    """T is 1 - alpha with probability p and 1 otherwise: sigma of the mean = alpha sqrt(p (1 - p) / samples)."""
    p = R.ceiling_blocked_fraction(h, radius)
    return alpha * math.sqrt(p * (1.0 - p) / samples)
