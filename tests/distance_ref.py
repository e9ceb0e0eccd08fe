"""float64 brute-force nearest surface point: the independent reference of scene_nearest / tri_nearest and of
the world-space instance transform.  numpy only: no BVH, no pruning and no product library in the arithmetic.  It is built
on closest_hit_ref.geometry(scene) -- the scene's own f32 rows, vertices and reordered indices, widened -- applies
local_to_world() per instance to the vertices and finds the closest point of every triangle to every query point.

The formulation differs from the kernel's (Ericson's Voronoi regions) on purpose: project onto the plane, test the
barycentric signs, otherwise take the minimum over the three clamped edge projections.

Besides the answer it classifies each query as decisive and gives per-query tolerances (in the manner of DESIGN.md 17), and
it holds an f32 restatement of the kernel's leaf arithmetic (tri_nearest_f32), whose measured error against float64 fits K."""
from dataclasses import dataclass

import numpy as np

from tests import closest_hit_ref as X

U32 = X.U32
S_DECISIVE = X.S_DECISIVE
K_DIST = 6.0              # fitted: four times the worst measured error of tri_nearest_f32, rounded up
CHUNK = 256
F32 = np.float32


@dataclass
class World:
    tri: np.ndarray        # (T, 3, 3) float64 world-space vertices
    inst: np.ndarray       # (T,) instance
    triple: np.ndarray     # (T, 3) vertex indices within the instance's mesh
    local: np.ndarray      # (T,) index within the instance's mesh (the scene's order)
    mag: np.ndarray        # (T,) |M||v| + |b|, the largest over the three vertices (2-norm): what enters the f32 transform
    emax: np.ndarray       # (T,) longest edge
    hmin: np.ndarray       # (T,) smallest altitude (0 for zero area)


def world(g, transform=True, skip=()):
    """Every triangle of every instance in world space.  An instance whose rows have no finite inverse contributes nothing.
    transform=False is the planted twin that forgets the instance transform."""
    with np.errstate(all="ignore"):
        try:
            l2w = g.local_to_world()
            ok = np.isfinite(l2w).all((1, 2))
        except np.linalg.LinAlgError:
            l2w, ok = [], []
            for r in g.rows:
                m = np.zeros((4, 4)); m[:3] = r; m[3, 3] = 1
                try:
                    l2w.append(np.linalg.inv(m)[:3]); ok.append(True)
                except np.linalg.LinAlgError:
                    l2w.append(np.zeros((3, 4))); ok.append(False)
            l2w, ok = np.array(l2w), np.array(ok)
    tri, inst, triple, local, mag = [], [], [], [], []
    for i in range(len(g.rows)):
        m = g.meshes[g.mesh_idx[i]]
        if not ok[i] or i in skip or len(m.tris) == 0:
            continue
        M, b = (l2w[i][:, :3], l2w[i][:, 3]) if transform else (np.eye(3), np.zeros(3))
        v = m.verts[m.tris]                                            # (T, 3, 3)
        tri.append(v @ M.T + b)
        mag.append(np.linalg.norm(np.abs(v) @ np.abs(M).T + np.abs(b), axis=2).max(1))
        inst.append(np.full(len(m.tris), i))
        triple.append(m.tris)
        local.append(np.arange(len(m.tris)))
    tri = np.concatenate(tri)
    e = np.stack([tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], tri[:, 2] - tri[:, 1]], 1)
    en = np.linalg.norm(e, axis=2)
    area2 = np.linalg.norm(np.cross(e[:, 0], e[:, 1]), axis=1)
    with np.errstate(all="ignore"):
        hmin = np.where(en.max(1) > 0, area2 / en.max(1), 0.0)
    return World(tri, np.concatenate(inst), np.concatenate(triple), np.concatenate(local), np.concatenate(mag), en.max(1), hmin)


def _segment(p, a, b):
    """Closest point of the segments a b (T, 3) to the points p (C, 3): (C, T, 3), parameter (C, T)."""
    ab = b - a
    ll = (ab * ab).sum(-1)
    with np.errstate(all="ignore"):
        t = ((p[:, None, :] - a[None]) * ab[None]).sum(-1) / ll[None]
    t = np.where(ll[None] > 0, np.clip(t, 0.0, 1.0), 0.0)
    return a[None] + t[..., None] * ab[None], t


def closest_points(p, tri):
    """float64: for points p (C, 3) and triangles tri (T, 3, 3): squared distance (C, T), point (C, T, 3), barycentrics
    u, v (C, T) with point = v0 + (v1 - v0) u + (v2 - v0) v, and feature (C, T): 0 face, 1 edge, 2 vertex.  Zero-area
    triangles give +inf."""
    a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
    e1, e2 = b - a, c - a
    n = np.cross(e1, e2)
    nn = (n * n).sum(-1)
    ap = p[:, None, :] - a[None]
    with np.errstate(all="ignore"):
        # plane projection and its barycentrics by the scalar triple products
        u = (np.cross(ap, e2[None]) * n[None]).sum(-1) / nn[None]
        v = (np.cross(e1[None], ap) * n[None]).sum(-1) / nn[None]
    inside = (u >= 0) & (v >= 0) & (u + v <= 1)
    face = a[None] + u[..., None] * e1[None] + v[..., None] * e2[None]
    best_d, best_q, best_u, best_v, feat = None, None, None, None, None
    for (s, e, uv) in ((a, b, lambda t: (t, 0 * t)), (a, c, lambda t: (0 * t, t)), (b, c, lambda t: (1 - t, t))):
        q, t = _segment(p, s, e)
        d = ((p[:, None, :] - q) ** 2).sum(-1)
        uu, vv = uv(t)
        if best_d is None:
            best_d, best_q, best_u, best_v = d, q, uu, vv
        else:
            take = d < best_d
            best_d, best_q = np.where(take, d, best_d), np.where(take[..., None], q, best_q)
            best_u, best_v = np.where(take, uu, best_u), np.where(take, vv, best_v)
    d_face = ((p[:, None, :] - face) ** 2).sum(-1)
    d2 = np.where(inside, d_face, best_d)
    q = np.where(inside[..., None], face, best_q)
    u, v = np.where(inside, u, best_u), np.where(inside, v, best_v)
    at_vertex = ((u == 0) & (v == 0)) | ((u == 1) & (v == 0)) | ((u == 0) & (v == 1))
    feat = np.where(inside, 0, np.where(at_vertex, 2, 1))
    d2 = np.where(nn[None] > 0, d2, np.inf)
    return d2, q, u, v, feat


@dataclass
class Nearest:
    found: np.ndarray      # (N,) bool
    inst: np.ndarray       # (N,) -1 = nothing
    triple: np.ndarray     # (N, 3)
    local: np.ndarray      # (N,) triangle index within the mesh
    distance: np.ndarray   # (N,) inf = nothing within rmax
    nearest: np.ndarray    # (N,) the unbounded distance (inf for an empty scene)
    point: np.ndarray      # (N, 3)
    u: np.ndarray
    v: np.ndarray
    side: np.ndarray       # (N,) sign of dot(p - point, n) of the winning triangle
    side_clear: np.ndarray  # (N,) |dot| clears its f32 error
    decisive: np.ndarray   # (N,) found / instance / triangle cannot plausibly come out otherwise in f32
    feature_decisive: np.ndarray   # (N,) the barycentrics clear 0 and 1: u, v and the point are well defined
    tol_d: np.ndarray      # (N,) absolute f32 error bound of the distance
    tol_p: np.ndarray      # (N,) ... of the point and (divided by the shortest altitude) of u, v
    feat_verts: np.ndarray = None   # (N, 3) the mesh vertex indices of the winning feature (face 3, edge 2, vertex 1), -1 padded


def nearest(w, points, rmax=np.inf, s=S_DECISIVE, k=K_DIST, strict=True):
    """The reference answer for `points` (N, 3) against the World `w`.  strict=False is the planted twin that compares <=."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(P)
    rmax = np.broadcast_to(np.asarray(rmax, np.float64), (n,))
    out = Nearest(np.zeros(n, bool), np.full(n, -1), np.full((n, 3), -1), np.full(n, -1), np.full(n, np.inf), np.full(n, np.inf), np.zeros((n, 3)),
                  np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool), np.zeros(n), np.zeros(n))
    for a in range(0, n, CHUNK):
        p = P[a:a + CHUNK]
        c = len(p)
        rows = np.arange(c)
        d2, q, u, v, feat = closest_points(p, w.tri)
        j = np.argmin(d2, axis=1)
        d = np.sqrt(d2[rows, j])
        pn = np.linalg.norm(p, axis=1)
        tol_d = k * U32 * (pn + w.mag[j] + w.emax[j])
        # the runner-up from a triangle that does not share the winning feature: a triangle whose own closest point is the
        # winner's point (a shared edge or vertex) is the same answer under another name
        qj = q[rows, j]
        same_point = (np.linalg.norm(q - qj[:, None, :], axis=2) <= tol_d[:, None]) & (w.inst[None, :] == w.inst[j][:, None])
        # ... and so is, within f32, a triangle of the same instance that contains the winning feature's vertices
        uj0, vj0 = u[rows, j], v[rows, j]
        on = np.stack([~((uj0 == 1) & (vj0 == 0)) & ~((uj0 == 0) & (vj0 == 1)) & ((uj0 + vj0) != 1), (uj0 != 0), (vj0 != 0)], 1)   # which of v0, v1, v2 span it
        on[:, 0] |= ~on.any(1)
        fv = np.where(on, w.triple[j], -1)                                # (c, 3)
        has = np.ones((c, len(w.tri)), bool)
        for kk in range(3):
            has &= (fv[:, kk, None] < 0) | (w.triple[None, :, :] == fv[:, kk, None, None]).any(-1)
        shares = has & (w.inst[None, :] == w.inst[j][:, None])
        dd = np.sqrt(np.where(same_point | shares, np.inf, d2))
        rival = dd.min(axis=1)
        if out.feat_verts is None:
            out.feat_verts = np.full((n, 3), -1)
        out.feat_verts[a:a + c] = fv
        fin = np.isfinite(d)
        r = rmax[a:a + c]
        found = fin & ((d < r) if strict else (d <= r))
        with np.errstate(all="ignore"):
            dec_found = found & (rival > d * (1 + s) + 2 * tol_d) & (d * (1 + s) + tol_d < r)
            dec_miss = ~found & ~(np.sqrt(d2).min(axis=1) <= r * (1 + s) + tol_d)
        sl = slice(a, a + c)
        out.found[sl], out.nearest[sl] = found, d
        out.decisive[sl] = dec_found | dec_miss
        out.distance[sl] = np.where(found, d, np.inf)
        out.inst[sl] = np.where(found, w.inst[j], -1)
        out.triple[sl] = np.where(found[:, None], w.triple[j], -1)
        out.local[sl] = np.where(found, w.local[j], -1)
        out.point[sl] = np.where(found[:, None], qj, 0.0)
        uj, vj = u[rows, j], v[rows, j]
        out.u[sl], out.v[sl] = np.where(found, uj, 0.0), np.where(found, vj, 0.0)
        with np.errstate(all="ignore"):
            cond = 1.0 + ((d + w.emax[j]) / w.hmin[j]) ** 2
            tol_p = tol_d * cond
            tb = tol_p / w.hmin[j]
        clear = lambda x: (np.abs(x) > tb) & (np.abs(1 - x) > tb)
        wj = 1 - uj - vj
        # face: all three clear; edge: the free parameter clears; vertex: never (the barycentrics sit on 0 / 1 by nature,
        # which is fine for the point but the point is then compared with tol_p all the same)
        fj = feat[rows, j]
        free = np.where(uj == 0, vj, np.where(vj == 0, uj, vj))
        out.feature_decisive[sl] = found & np.isfinite(tol_p) & np.where(fj == 0, clear(uj) & clear(vj) & clear(wj), np.where(fj == 1, clear(free), True))
        out.tol_d[sl], out.tol_p[sl] = tol_d, np.where(np.isfinite(tol_p), tol_p, np.inf)
        t = w.tri[j]
        nrm = np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])
        dot = ((p - qj) * nrm).sum(1)
        out.side[sl] = np.where(found, np.sign(dot), 0.0)
        out.side_clear[sl] = found & (np.abs(dot) > 4 * tol_d * np.linalg.norm(nrm, axis=1) * cond)
    return out


def index_of(w):
    """(instance, local triangle) -> row of the World"""
    return {(int(i), int(t)): r for r, (i, t) in enumerate(zip(w.inst, w.local))}


def reevaluate(w, points, inst, local, k=K_DIST):
    """For every query r the float64 closest point on the world triangle (inst[r], local[r]): (d, point, tol_d, known).
    known is False where the pair names no triangle of the World."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    idx = index_of(w)
    rowsel = np.array([idx.get((int(i), int(t)), -1) for i, t in zip(inst, local)], np.int64)
    known = rowsel >= 0
    d = np.full(len(P), np.inf)
    q = np.zeros((len(P), 3))
    tol = np.zeros(len(P))
    for r in np.nonzero(known)[0]:
        d2, qq, _, _, _ = closest_points(P[r:r + 1], w.tri[rowsel[r]:rowsel[r] + 1])
        d[r], q[r] = np.sqrt(d2[0, 0]), qq[0, 0]
        tol[r] = k * U32 * (np.linalg.norm(P[r]) + w.mag[rowsel[r]] + w.emax[rowsel[r]])
    return d, q, tol, known


# ------------------------------------------------------------------------------------------------
# The f32 restatement of the kernel's leaf arithmetic (lupin_distance.hpp tri_nearest), operation for operation
# ------------------------------------------------------------------------------------------------

def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def to_world_f32(m, v):
    """rows m (3, 4) f32, vertices v (..., 3) f32: m.x * v.x + m.y * v.y + m.z * v.z + m.w * 1, left to right."""
    m, v = np.asarray(m, F32), np.asarray(v, F32)
    return np.stack([((m[r, 0] * v[..., 0] + m[r, 1] * v[..., 1]) + m[r, 2] * v[..., 2]) + m[r, 3] * F32(1) for r in range(3)], -1)


def tri_nearest_f32(p, a, b, c):
    """p, a, b, c (..., 3) float32 (broadcast): (d2, u, v, point) in float32, by Ericson's regions as the kernel orders them.
    Zero-area triangles (cross product of squared length 0 in f32) give d2 = +inf."""
    p, a, b, c = (np.asarray(x, F32) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap, bp, cp = p - a, p - b, p - c
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        one, zero = np.ones_like(d1), np.zeros_like(d1)
        nu, nv, den = vb, vc, (va + vb) + vc
        for cond, xu, xv, xd in (((va <= 0) & (e43 >= 0) & (e56 >= 0), e56, e43, e43 + e56),
                                 ((vb <= 0) & (d2 >= 0) & (d6 <= 0), zero, d2, d2 - d6),
                                 ((d6 >= 0) & (d5 <= d6), zero, one, one),
                                 ((vc <= 0) & (d1 >= 0) & (d3 <= 0), d1, zero, d1 - d3),
                                 ((d3 >= 0) & (d4 <= d3), one, zero, one),
                                 ((d1 <= 0) & (d2 <= 0), zero, zero, one)):
            nu, nv, den = np.where(cond, xu, nu), np.where(cond, xv, nv), np.where(cond, xd, den)
        u, v = nu / den, nv / den
        q = np.stack([(a[..., k] + ab[..., k] * u) + ac[..., k] * v for k in range(3)], -1)
        r = p - q
        dd = _dot(r, r)
        n = np.stack([ab[..., 1] * ac[..., 2] - ab[..., 2] * ac[..., 1], ab[..., 2] * ac[..., 0] - ab[..., 0] * ac[..., 2],
                      ab[..., 0] * ac[..., 1] - ab[..., 1] * ac[..., 0]], -1)
        dd = np.where(_dot(n, n) == 0, F32(np.inf), dd)
    assert dd.dtype == F32 and u.dtype == F32
    return dd, u, v, q


def world_f32(scene, g):
    """The kernel's world-space vertices: (T, 3, 3) float32 in World order, through lupin_mat3x4_inverse's f32 rows as
    api.mat3x4_inverse gives them; an instance without a finite inverse is left out, as in world()."""
    out = []
    for i in range(len(g.rows)):
        m = g.meshes[g.mesh_idx[i]]
        rows = np.asarray(scene.instances["transpose_inverse_transform"][i], F32).reshape(3, 4)
        l2w = f32_inverse_rows(rows)
        if not np.isfinite(l2w).all() or len(m.tris) == 0:
            continue
        out.append(to_world_f32(l2w, m.verts[m.tris].astype(F32)))
    return np.concatenate(out)


def f32_inverse_rows(rows):
    """local -> world rows (3, 4) f32 of world -> local rows (3, 4): the library's lupin_mat3x4_inverse."""
    import ctypes as C
    from lupinpathtracer_amd import _abi
    src = np.ascontiguousarray(np.asarray(rows, F32).reshape(3, 4).T)      # LupinMat3x4: 4 columns x 3 rows
    dst = np.zeros((4, 3), F32)
    handle = C.CDLL(_abi.LIB_PATH)
    handle.lupin_mat3x4_inverse.restype = None
    handle.lupin_mat3x4_inverse(C.c_void_p(src.ctypes.data), C.c_void_p(dst.ctypes.data))
    return np.ascontiguousarray(dst.T)


def nearest_f32(wf, points, chunk=CHUNK):
    """Brute force with the kernel's f32 leaf arithmetic over the f32 world triangles wf (T, 3, 3): (distance f32, index)."""
    P = np.asarray(points, F32).reshape(-1, 3)
    d, j = np.zeros(len(P), F32), np.zeros(len(P), np.int64)
    for a in range(0, len(P), chunk):
        p = P[a:a + chunk]
        dd, _, _, _ = tri_nearest_f32(p[:, None, :], wf[None, :, 0], wf[None, :, 1], wf[None, :, 2])
        jj = np.argmin(dd, axis=1)
        j[a:a + chunk] = jj
        d[a:a + chunk] = np.sqrt(dd[np.arange(len(p)), jj])
    return d, j


# ------------------------------------------------------------------------------------------------
# Query points
# ------------------------------------------------------------------------------------------------

FAMILIES = ("surface", "uniform", "far", "vertex")
COUNTS = {"big": dict(surface=1700, uniform=1200, far=37, vertex=66), "small": dict(surface=900, uniform=700, far=21, vertex=40)}


def _choose(cand, decisive, n):
    """n of the candidates, in their order: floor(n / 100) that the reference cannot decide (if there are that many), the
    rest decided."""
    und = np.nonzero(~decisive)[0][:n // 100]
    dec = np.nonzero(decisive)[0][:n - len(und)]
    assert len(dec) + len(und) == n, "too few decisive candidates"
    return cand[np.sort(np.concatenate([und, dec]))]


def make_points(g, seed, counts):
    """(points (N, 3) f32, family (N,)): surface points pushed off along +- the normal by 1e-3 .. 10 local edge lengths,
    uniform points in twice the scene's box, points 1e3 extents away, points exactly on (f32 world) vertices."""
    rng = np.random.default_rng(seed)
    l2w = g.local_to_world()
    ni = len(g.rows)
    w = world(g)
    lo, hi = w.tri.reshape(-1, 3).min(0), w.tri.reshape(-1, 3).max(0)
    centre, extent = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    pts, fam = [], []
    n = counts["surface"] * 5 // 4
    inst = np.arange(n) % ni
    sp, nw = X._surface_points(rng, g, l2w, inst)
    edge = np.array([np.median(w.emax[w.inst == i]) for i in range(ni)])[inst]
    off = edge * 10.0 ** rng.uniform(-3, 1, n) * np.where(rng.uniform(size=n) < 0.5, -1.0, 1.0)
    pts.append(sp + nw * off[:, None]); fam.append(np.full(n, 0))
    n = counts["uniform"] * 5 // 4
    pts.append(centre + rng.uniform(-1.0, 1.0, (n, 3)) * (hi - lo)); fam.append(np.full(n, 1))
    n = counts["far"]                                                # from 16 n candidates, as above
    cand = (centre + X._unit(rng, 16 * n) * extent * 1e3).astype(F32)
    pts.append(_choose(cand, nearest(w, cand).decisive, n).astype(np.float64)); fam.append(np.full(n, 2))
    n = counts["vertex"]
    pick = rng.integers(0, len(w.tri), n)
    pts.append(w.tri[pick, rng.integers(0, 3, n)]); fam.append(np.full(n, 3))
    # The surface and uniform families are drawn 1.25 times over.  Some 2 % of the candidates are near ties between
    # neighbouring small triangles seen from many triangle sizes away, which the reference cannot decide; the choice is made on
    # the CPU, by the reference alone: floor(1 % of the family) undecided candidates STAY, so that the checks on
    # every found result see them, and the rest of the set is decided ones.
    for k in (0, 1):
        cand = pts[k].astype(F32)
        pts[k], fam[k] = _choose(cand, nearest(w, cand).decisive, counts[FAMILIES[k]]).astype(np.float64), fam[k][:counts[FAMILIES[k]]]
    pts, fam = np.concatenate(pts), np.concatenate(fam)
    order = rng.permutation(len(pts))
    return pts[order].astype(F32), fam[order]


def compare(ref, w, points, got):
    """`got`: the structured results of api.distance_points.  Returns the counts the tests assert are zero, and figures.
    A triangle that shares the winning feature (its own closest point is the winner's point, an edge or a vertex both
    own) is the same answer under another name: it is accepted for `instance` and `triangle`."""
    P = np.asarray(points, np.float64).reshape(-1, 3)
    found = got["found"] != 0
    inst, tri = got["instance"].astype(np.int64), got["tri"].astype(np.int64)
    dist, point = got["distance"].astype(np.float64), got["point"].astype(np.float64)
    dec = ref.decisive
    rep = dict(queries=len(P), non_decisive_share=float(1 - dec.mean()))
    rep["flag"] = int((dec & (found != ref.found)).sum())
    # every found result, decisive or not, against its own triangle in float64
    d2, q2, tol2, known = reevaluate(w, P, np.where(found, inst, -1), np.where(found, tri, -1))
    rep["bad_index"] = int((found & ~known).sum())
    fk = found & known
    both = dec & fk & ref.found
    exact = both & (inst == ref.inst) & (tri == ref.local)
    rows_of = index_of_cached(w)
    trip = np.array([w.triple[rows_of[(int(i), int(t))]] if k else (-1, -1, -1) for i, t, k in zip(inst, tri, fk)])
    contains = np.ones(len(P), bool)
    for kk in range(3):
        contains &= (ref.feat_verts[:, kk] < 0) | (trip == ref.feat_verts[:, kk, None]).any(1)
    # the two routes by which the reference itself took a triangle out of the rivals, both within the winner's instance
    by_point = both & ~exact & (inst == ref.inst) & (np.linalg.norm(q2 - ref.point, axis=1) <= ref.tol_d)
    by_verts = both & ~exact & ~by_point & (inst == ref.inst) & contains
    match = exact | by_point | by_verts
    rep["matched_exactly"], rep["matched_by_shared_point"], rep["matched_by_shared_vertices"] = int(exact.sum()), int(by_point.sum()), int(by_verts.sum())
    rep["instance"] = int((both & ~match & (inst != ref.inst)).sum())
    rep["triangle"] = int((both & ~match & (inst == ref.inst)).sum())
    err_d = np.abs(dist - ref.distance)
    rep["distance"] = int((match & ~(err_d <= ref.tol_d)).sum())
    err_p = np.linalg.norm(point - ref.point, axis=1)
    well = match & ref.feature_decisive
    rep["point"] = int((well & ~(err_p <= ref.tol_p)).sum())
    rep["side"] = int((exact & ref.side_clear & (got["side"] != ref.side)).sum())
    with np.errstate(all="ignore"):
        rep["worst_d_over_bound"] = float((err_d[match] / ref.tol_d[match]).max()) if match.any() else 0.0
        rep["worst_p_over_bound"] = float((err_p[well] / ref.tol_p[well]).max()) if well.any() else 0.0
        rep["reported_distance"] = int((fk & ~(np.abs(dist - d2) <= tol2)).sum())
        rep["self_distance"] = int((fk & ~(np.abs(dist - np.linalg.norm(P - point, axis=1)) <= tol2)).sum())
        # the reported point lies on that triangle: no further from it than the tolerance
        on, _, _, _ = reevaluate(w, point, np.where(found, inst, -1), np.where(found, tri, -1))
        rep["off_triangle"] = int((fk & ~(on <= tol2)).sum())
        # nothing strictly nearer was missed (the reference's unbounded nearest distance, whatever rmax was)
        rep["missed_nearer"] = int((fk & ~(dist <= ref.nearest * (1 + S_DECISIVE) + 2 * tol2)).sum())
    return rep


_index_cache = {}


def index_of_cached(w):
    if id(w) not in _index_cache:
        _index_cache[id(w)] = index_of(w)
    return _index_cache[id(w)]


COUNT_KEYS = ("flag", "instance", "triangle", "distance", "point", "side", "bad_index", "reported_distance", "self_distance", "off_triangle",
              "missed_nearer")


def failures(rep):
    return [f"{k}={rep[k]}" for k in COUNT_KEYS if rep[k] != 0]


# ------------------------------------------------------------------------------------------------
# The leaky boxes: the scene's real node arrays, the point family aimed at them, and an f32 restatement of the traversal's
# BLAS level that honours or ignores WideNode.d.z
# ------------------------------------------------------------------------------------------------

def mesh_nodes(scene, i):
    """The BLAS of mesh i as the scene holds it (the builder's BvhNode array)."""
    import ctypes as C
    from lupinpathtracer_amd import _abi
    md = scene.desc.meshes[i]
    raw = np.ctypeslib.as_array(C.cast(md.bvh_nodes, C.POINTER(C.c_uint8)), (md.num_bvh_nodes * _abi.BVH_NODE_DTYPE.itemsize,))
    return raw.view(_abi.BVH_NODE_DTYPE).copy()


def leaks(scene, g):
    """Per mesh: (nodes, leaky_node (nodes,) bool, leak (T, 3): how far each vertex of each triangle lies outside the worst
    stored box above it, leaf box included; 0 for a triangle inside all of them).  leaky_node is test_wide_traversal's
    independent numpy restatement of what WideNode.d.z records."""
    from tests import reproject_ref
    from tests.test_wide_traversal import leaky_by_numpy
    out = []
    for mi, m in enumerate(g.meshes):
        nodes = mesh_nodes(scene, mi)
        v, idx = reproject_ref.mesh_arrays(scene, mi)
        _, leaky_node = leaky_by_numpy(nodes, v, idx)
        leak = np.zeros((len(m.tris), 3))
        stack = [(0, np.zeros((0, 2, 3)))]
        while stack:
            n, above = stack.pop()
            nd = nodes[n]
            above = np.concatenate([above, np.array([[nd["aabb_min"], nd["aabb_max"]]], np.float64)])
            if nd["tri_count"] > 0:
                b, c = int(nd["tri_begin_or_first_child"]), int(nd["tri_count"])
                p = m.verts[m.tris[b:b + c]]                                        # (c, 3, 3)
                d = np.maximum(np.maximum(above[None, None, :, 0] - p[:, :, None], p[:, :, None] - above[None, None, :, 1]), 0.0)
                leak[b:b + c] = np.linalg.norm(d, axis=-1).max(-1)
            else:
                c0 = int(nd["tri_begin_or_first_child"])
                stack += [(c0, above), (c0 + 1, above)]
        out.append((nodes, leaky_node, leak))
    return out


def leaky_points(scene, g, limit=48):
    """The family aimed at the leaky triangles: for up to `limit` (instance, triangle, vertex) with the largest leaks, the
    world-space vertex moved a sixteenth of the (world) leak off along the triangle's normal, and rmax = a quarter of the
    leak's world lower bound (leak x the smallest singular value of local -> world) -- so that the box the vertex sticks out
    of is farther than rmax while the triangle is nearer.  (points f32 (n, 3), rmax f32 (n,), instance, local triangle.)"""
    lk = leaks(scene, g)
    l2w = g.local_to_world()
    cand = []
    for i in range(len(g.rows)):
        mi = g.mesh_idx[i]
        m, leak = g.meshes[mi], lk[mi][2]
        smin = np.linalg.svd(l2w[i][:, :3], compute_uv=False).min()
        for t, k in zip(*np.nonzero(leak > 0)):
            tri = m.verts[m.tris[t]] @ l2w[i][:, :3].T + l2w[i][:, 3]
            n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
            if not (n * n).sum() > 0:
                continue
            wl = leak[t, k] * smin
            cand.append((wl, i, t, tri[k] + n / np.linalg.norm(n) * wl / 16, wl / 4))
    cand.sort(key=lambda c: -c[0])
    cand = cand[:limit]
    if not cand:
        return np.zeros((0, 3), F32), np.zeros(0, F32), np.zeros(0, np.int64), np.zeros(0, np.int64)
    return (np.array([c[3] for c in cand], F32), np.array([c[4] for c in cand], F32), np.array([c[1] for c in cand]), np.array([c[2] for c in cand]))


def scale_f32(rows3):
    """c_i as the host computes it: 1 / sigma_max of the world -> local 3 x 3 part in float64, shrunk by 1e-9, rounded toward
    zero to f32 (here sigma_max by SVD, not by the closed form)."""
    c = (1.0 / np.linalg.svd(np.asarray(rows3, np.float64), compute_uv=False).max()) * (1.0 - 1e-9)
    f = F32(c)
    return np.nextafter(f, F32(0)) if float(f) > c else f


def _box_dst2_f32(p, lo, hi):
    d = np.maximum(np.maximum(lo - p, p - hi), F32(0))
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


def nearest_f32_blas(scene, g, points, rmax, honour_flags=True):
    """scene_nearest's instance level restated in numpy f32 over the scene's real node arrays: every instance is entered in
    turn (the TLAS is not restated), pl = R p + t, a child's key is box_dst2(pl) c_i^2 -- 0 for a child whose box does not
    bound its triangles when honour_flags -- the nearer child first, the farther pushed with its key if key < best and
    re-tested when popped, leaves through tri_nearest_f32 on the f32 world vertices.  honour_flags=False is the variant that
    ignores WideNode.d.z.  Returns (found, distance f32, instance, local triangle)."""
    P, R = np.asarray(points, F32).reshape(-1, 3), np.broadcast_to(np.asarray(rmax, F32), (len(np.asarray(points).reshape(-1, 3)),))
    lk = leaks(scene, g)
    inst_rows = np.asarray(scene.instances["transpose_inverse_transform"], F32).reshape(-1, 3, 4)
    wverts = []
    for i in range(len(g.rows)):
        m = g.meshes[g.mesh_idx[i]]
        wverts.append(to_world_f32(f32_inverse_rows(inst_rows[i]), m.verts[m.tris].astype(F32)))
    found, dist = np.zeros(len(P), bool), np.zeros(len(P), F32)
    oi, ot = np.full(len(P), -1), np.full(len(P), -1)
    for q, (p, r) in enumerate(zip(P, R)):
        r2 = r * r
        best = max(r2 + r2 * F32(2.0 ** -21), np.finfo(F32).tiny)
        for i in range(len(g.rows)):
            nodes, leaky_node, _ = lk[g.mesh_idx[i]]
            rw = inst_rows[i]
            pl = np.array([((p[0] * rw[k, 0] + p[1] * rw[k, 1]) + p[2] * rw[k, 2]) + F32(1) * rw[k, 3] for k in range(3)], F32)
            c = scale_f32(rw[:, :3])
            ks = c * c
            stack = [(0, F32(0))]
            while stack:
                n, key = stack.pop()
                if not key < best:
                    continue
                nd = nodes[n]
                if nd["tri_count"] > 0:
                    b, cnt = int(nd["tri_begin_or_first_child"]), int(nd["tri_count"])
                    tv = wverts[i][b:b + cnt]
                    dd, _, _, _ = tri_nearest_f32(p[None], tv[:, 0], tv[:, 1], tv[:, 2])
                    for t in range(cnt):
                        if dd[t] < best:
                            best, oi[q], ot[q] = dd[t], i, b + t
                    continue
                c0 = int(nd["tri_begin_or_first_child"])
                keys = []
                for ch in (c0, c0 + 1):
                    k = _box_dst2_f32(pl, nodes[ch]["aabb_min"].astype(F32), nodes[ch]["aabb_max"].astype(F32)) * ks
                    keys.append(F32(0) if (honour_flags and leaky_node[ch]) else k)
                near, far = (0, 1) if keys[0] <= keys[1] else (1, 0)
                if keys[far] < best:
                    stack.append((c0 + far, keys[far]))
                if keys[near] < best:
                    stack.append((c0 + near, keys[near]))
        d = np.sqrt(best)
        if oi[q] >= 0 and d < r:
            found[q], dist[q] = True, d
        else:
            oi[q], ot[q] = -1, -1
    return found, dist, oi, ot


def shrunk_boxes_bvh(verts, indices):
    """A BLAS builder with PLANTED leaks: lupin_build_bvh's tree with the stored box of every third node below the root
    shrunk by a quarter about its centre, so that triangles stick out of boxes above them (inner nodes and leaves alike) as
    the reference's binned builder leaves them on large meshes -- there one triangle in 10^5, here enough to test with."""
    from lupinpathtracer_amd import api
    nodes, reordered = api.build_bvh(verts, indices)
    nodes = nodes.copy()
    for n in range(1, len(nodes), 3):
        lo, hi = nodes[n]["aabb_min"].astype(np.float64), nodes[n]["aabb_max"].astype(np.float64)
        c, h = (lo + hi) / 2, (hi - lo) / 2
        nodes[n]["aabb_min"], nodes[n]["aabb_max"] = (c - 0.75 * h).astype(F32), (c + 0.75 * h).astype(F32)
    return nodes, reordered


LEAKY_LAYOUT = [(X.GRID, (0, 0, 0)), (X.SOUP, (3, 1, -2)), (X.GRID, (-3, 2, 1))]


def leaky_scene(ctx=None):
    """Three instances (rotated, non-uniformly scaled) of closest_hit_ref's small grid and soup meshes under
    shrunk_boxes_bvh: a scene whose BLAS boxes do not bound their triangles, flagged by the library in WideNode.d.z."""
    from lupinpathtracer_amd import api
    rng = np.random.default_rng(77)
    size = X.SIZES["small"]
    meshes = [X.soup_mesh(rng, size["soup"]), X.grid_mesh(rng, size["grid"])]
    sc = api.SceneCPU()
    sc.materials = np.array([api.default_material()], api.MATERIAL_DTYPE)
    for v, idx in meshes:
        sc.verts_pos_array.append(v.copy())
        sc.indices_array.append(idx.copy())
    sc.mesh_infos = np.array([api.default_mesh_info() for _ in meshes], api.MESH_INFO_DTYPE)
    recs = []
    for mesh, centre in LEAKY_LAYOUT:
        M = X.rotation(rng) @ np.diag(np.exp(rng.uniform(np.log(0.5), np.log(2.0), 3)))
        recs.append(api.instance_from_transform(X.mat3x4(M, np.array(centre, np.float64)), {X.SOUP: 0, X.GRID: 1}[mesh], 0))
    sc.instances = np.array(recs, api.INSTANCE_DTYPE)
    api.validate_scene(sc, 0, 0)
    return api.build_accel_structures_and_upload(ctx, sc, [], [], True, blas_builder=shrunk_boxes_bvh)
