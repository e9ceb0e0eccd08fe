"""numpy float32 restatement of lupin_hip_stitch_lightmap (include/lupin_hip.h), operation for operation: seam
edges, sample pairs, footprints, the incidence order, the conjugate gradients and the order of their sums; and beside it a
float64 reference on the same rows: the dense optimum and a float64 CG with its objective per step.

A chart is given as (tris, uvs, chart): the (T, 3) vertex indices of its instance's mesh in the scene's own triangle order,
the (T, 3, 2) lightmap UVs per corner, and a LightmapChart-like item (scale_u, scale_v, offset_u, offset_v)."""
import numpy as np

from tests import lightmapped_view_ref as L

F = np.float32
MAX_EDGE_SAMPLES = 65536
PLANTS = ("b_sign", "reversed_incidence")


def corner_uvs(tris, texcoords):
    """The per-corner UVs of a mesh that has texcoords and no lightmap UV set."""
    return np.asarray(texcoords, F)[np.asarray(tris, np.int64)]


def atlas_xy(uvs, chart, W, H):
    """lm_triangle's texel-space corners: (u * scale_u + offset_u) * W, (v * scale_v + offset_v) * H."""
    uvs = np.asarray(uvs, F)
    x = (uvs[..., 0] * F(chart.scale_u) + F(chart.offset_u)) * F(W)
    y = (uvs[..., 1] * F(chart.scale_v) + F(chart.offset_v)) * F(H)
    return np.stack([x, y], axis=-1).astype(F)


def chart_seams(tris, xy):
    """The seam edges of one chart in ascending hA: ((E, 8) float32 rows a0, a1, b0, b1; hA (E,); non-manifold edge count)."""
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    h = np.arange(3 * len(tris))
    t, k = h // 3, h % 3
    va, vb = tris[t, k], tris[t, (k + 1) % 3]
    key = (np.minimum(va, vb).astype(np.uint64) << np.uint64(32)) | np.maximum(va, vb).astype(np.uint64)
    ok = va != vb                                            # a half-edge with equal indices is skipped
    hs, ks = h[ok], key[ok]
    order = np.argsort(ks, kind="stable")
    hs, ks = hs[order], ks[order]
    _, start, counts = np.unique(ks, return_index=True, return_counts=True)
    non_manifold = int((counts >= 3).sum())
    two = start[counts == 2]
    hA, hB = hs[two], hs[two + 1]                            # hA < hB: the sort is stable
    tA, kA, tB, kB = hA // 3, hA % 3, hB // 3, hB % 3
    a0, a1 = xy[tA, kA], xy[tA, (kA + 1) % 3]
    same = tris[tB, kB] == tris[tA, kA]
    first, last = np.where(same, kB, (kB + 1) % 3), np.where(same, (kB + 1) % 3, kB)
    b0, b1 = xy[tB, first], xy[tB, last]
    rows = np.concatenate([a0, a1, b0, b1], axis=1).astype(F).reshape(-1, 8)
    bits = rows.view(np.uint32)
    seam = np.any(bits[:, 0:4] != bits[:, 4:8], axis=1)
    keep = np.argsort(hA[seam], kind="stable")
    return rows[seam][keep], hA[seam][keep], non_manifold


def seam_edges(charts, W, H):
    """All charts: ((E, 8) edges in ascending (chart, hA), non-manifold count)."""
    edges, non_manifold = [np.zeros((0, 8), F)], 0
    for tris, uvs, chart in charts:
        rows, _, nm = chart_seams(tris, atlas_xy(uvs, chart, W, H))
        edges.append(rows)
        non_manifold += nm
    return np.concatenate(edges), non_manifold


def sample_points(edges, samples_per_texel):
    """(A (P, 2), B (P, 2), edge of pair (P,)) float32, edge by edge, j ascending."""
    e = np.asarray(edges, F)
    with np.errstate(all="ignore"):
        def length(p, q):
            dx, dy = q[:, 0] - p[:, 0], q[:, 1] - p[:, 1]
            return np.sqrt(dx * dx + dy * dy)
        m = np.ceil(np.fmax(length(e[:, 0:2], e[:, 2:4]), length(e[:, 4:6], e[:, 6:8])) * F(samples_per_texel))
        ne = np.where(m >= F(MAX_EDGE_SAMPLES), MAX_EDGE_SAMPLES, np.where(m >= F(1.0), np.nan_to_num(m, nan=1.0, posinf=1.0).astype(np.int64), 1))
        offsets = np.concatenate([[0], np.cumsum(ne)])
        of = np.repeat(np.arange(len(e)), ne)
        j = np.arange(int(offsets[-1])) - offsets[of]
        t = (j.astype(F) + F(0.5)) / ne[of].astype(F)
        a = np.stack([e[of, 0] + (e[of, 2] - e[of, 0]) * t, e[of, 1] + (e[of, 3] - e[of, 1]) * t], axis=1).astype(F)
        b = np.stack([e[of, 4] + (e[of, 6] - e[of, 4]) * t, e[of, 5] + (e[of, 7] - e[of, 5]) * t], axis=1).astype(F)
    return a, b, of


def footprint(alpha, pts):
    """The four taps of the view's fetch at pts - 0.5: (texel (P, 4), weight (P, 4) float32, kept (P,))."""
    H, W = alpha.shape
    with np.errstate(all="ignore"):
        cx, cy = pts[:, 0] - F(0.5), pts[:, 1] - F(0.5)
        finite = np.isfinite(cx) & np.isfinite(cy)
        x0, x1, fx = L._axis(np.where(finite, cx, F(0.0)).astype(F), W, None)
        y0, y1, fy = L._axis(np.where(finite, cy, F(0.0)).astype(F), H, None)
        one = F(1.0)
        gx, gy = one - fx, one - fy
        wt = np.stack([gx * gy, fx * gy, gx * fy, fx * fy], axis=1).astype(F)             # taps 00, 10, 01, 11
        tex = np.stack([y0 * W + x0, y0 * W + x1, y1 * W + x0, y1 * W + x1], axis=1)
        owned = alpha.reshape(-1)[tex] != 0
        cov = np.zeros(len(pts), F)
        for k in range(4):
            cov = np.where(owned[:, k], cov + wt[:, k], cov)
        kept = finite & (cov > 0)
        w = np.where(owned & kept[:, None], wt / np.where(kept, cov, one)[:, None], F(0.0)).astype(F)
    return tex, w, kept


def rows_of(rgba, charts, samples_per_texel, plant=None):
    """The problem's rows: dict of tex (P, 8), w (P, 8) float32, and the counts."""
    rgba = np.asarray(rgba, F)
    H, W = rgba.shape[:2]
    edges, non_manifold = seam_edges(charts, W, H)
    a, b, _ = sample_points(edges, samples_per_texel)
    ta, wa, ka = footprint(rgba[..., 3], a)
    tb, wb, kb = footprint(rgba[..., 3], b)
    kept = ka & kb
    tex = np.where(kept[:, None], np.concatenate([ta, tb], axis=1), 0)
    w = np.where(kept[:, None], np.concatenate([wa, wb if plant == "b_sign" else -wb], axis=1), F(0.0)).astype(F)
    return dict(tex=tex, w=w, a=a, b=b, kept=kept, seam_edges=len(edges), non_manifold_edges=non_manifold, sample_pairs=len(a),
                dropped_pairs=int((~kept).sum()))


def incidence(rows, plant=None):
    """The active texels (ascending), col (P, 8) (0 where the weight is 0), and the incidence list: entries (8 p + e) sorted
    by texel, ascending within a texel, with the start of every texel's run (A + 1,)."""
    tex, w = rows["tex"].reshape(-1), rows["w"].reshape(-1)
    live = np.nonzero(w != 0)[0]
    order = live[np.argsort(tex[live], kind="stable")]
    active, start = np.unique(tex[order], return_index=True)
    start = np.concatenate([start, [len(order)]]).astype(np.int64)
    col = np.zeros(len(tex), np.int64)
    col[order] = np.repeat(np.arange(len(active)), np.diff(start))
    if plant == "reversed_incidence":
        order = np.concatenate([order[start[i]:start[i + 1]][::-1] for i in range(len(active))]) if len(active) else order
    return active, col.reshape(-1, 8), order, start


def fixed_sum(v):
    """The header's sum of the rows of v (n, 3) float32."""
    v = np.asarray(v, F)
    n = len(v)
    blocks = (n + 255) // 256
    x = np.zeros((blocks * 256, 3), F)
    x[:n] = v
    x = x.reshape(blocks, 4, 64, 3)
    lane = np.arange(64)
    for m in (32, 16, 8, 4, 2, 1):
        x = x + x[:, :, lane ^ m]
    s = x[:, 0, 0]
    for wave in (1, 2, 3):
        s = s + x[:, wave, 0]
    acc = np.zeros((64, 3), F)
    for first in range(0, blocks, 64):
        part = s[first:first + 64]
        acc[:len(part)] = acc[:len(part)] + part
    for m in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lane ^ m]
    return acc[0].astype(F)


def apply(rows, col, v):
    """s = A v: the eight entries in entry order from zero, an entry without weight adding 0."""
    w = rows["w"]
    s = np.zeros((len(w), 3), F)
    with np.errstate(all="ignore"):
        for k in range(8):
            term = np.where((w[:, k] != 0)[:, None], w[:, k, None] * v[col[:, k]], F(0.0)).astype(F)
            s = s + term
    return s


def adjoint(rows, order, start, s):
    """t = A^T s: every texel's incidence list in list order, from zero."""
    w = rows["w"].reshape(-1)
    n = len(start) - 1
    t = np.zeros((n, 3), F)
    length = np.diff(start)
    with np.errstate(all="ignore"):
        for rank in range(int(length.max()) if n else 0):
            has = np.nonzero(length > rank)[0]
            at = order[start[has] + rank]
            t[has] = t[has] + w[at, None] * s[at >> 3]
    return t


def stitch(rgba, charts, iterations, samples_per_texel=2.0, lam=0.1, plant=None, rows=None):
    """What lupin_hip_stitch_lightmap writes: (out (H, W, 4) float32, info dict as api.stitch_lightmap's)."""
    rgba = np.asarray(rgba, F)
    rows = rows_of(rgba, charts, samples_per_texel, plant) if rows is None else rows
    info = {k: rows[k] for k in ("seam_edges", "non_manifold_edges", "sample_pairs", "dropped_pairs")}
    info.update(active_texels=0, iterations=0, energy_before=np.zeros(3, F), energy_after=np.zeros(3, F))
    out = rgba.copy()
    active, col, order, start = incidence(rows, plant)
    if len(active) == 0:
        return out, info
    lam = F(lam)
    flat = out.reshape(-1, 4)
    x0 = flat[active, 0:3].copy()
    with np.errstate(all="ignore"):
        s = apply(rows, col, x0)
        before = fixed_sum(s * s)
        r = -adjoint(rows, order, start, s)
        p, d = r.copy(), np.zeros_like(r)
        rr = fixed_sum(r * r)
        stopped = np.zeros(3, bool)
        for _ in range(iterations):
            s = apply(rows, col, p)
            q = adjoint(rows, order, start, s) + lam * p
            pq = fixed_sum(p * q)
            stopped |= ~((pq != 0) & np.isfinite(pq))
            alpha = np.where(stopped, F(0.0), rr / np.where(stopped, F(1.0), pq)).astype(F)
            d = d + alpha * p
            r = r - alpha * q
            rr_new = fixed_sum(r * r)
            beta = np.where(stopped, F(0.0), rr_new / rr).astype(F)
            rr = rr_new
            p = r + beta * p
        x = x0 + d
        s = apply(rows, col, x)
        after = fixed_sum(s * s)
    if iterations:
        flat[active, 0:3] = x
    info.update(active_texels=len(active), iterations=iterations, energy_before=before, energy_after=after)
    return out, info


# ---- the float64 reference ---------------------------------------------------------------------------------------------

def dense_system(rows):
    """(A (P, n) float64 over the active texels, active texels) of the rows as they stand."""
    active, col, _, _ = incidence(rows)
    A = np.zeros((len(rows["w"]), len(active)))
    for k in range(8):
        np.add.at(A, (np.arange(len(A)), col[:, k]), rows["w"][:, k].astype(np.float64))
    return A, active


def objective(A, x, x0, lam):
    """|A x|^2 + lam |x - x0|^2 per channel, float64."""
    s = A @ x
    return (s * s).sum(axis=0) + lam * ((x - x0) ** 2).sum(axis=0)


def dense_optimum(A, x0, lam):
    """x = x0 + d with (A^T A + lam I) d = -A^T (A x0), solved densely."""
    return x0 + np.linalg.solve(A.T @ A + lam * np.eye(A.shape[1]), -(A.T @ (A @ x0)))


def cg64(A, x0, lam, iterations):
    """Plain conjugate gradients in float64 from d = 0: the iterates x_0 .. x_iterations."""
    d = np.zeros_like(x0)
    r = -(A.T @ (A @ x0))
    p = r.copy()
    rr = (r * r).sum(axis=0)
    xs = [x0.copy()]
    for _ in range(iterations):
        q = A.T @ (A @ p) + lam * p
        pq = (p * q).sum(axis=0)
        go = (pq != 0) & np.isfinite(pq)
        alpha = np.where(go, rr / np.where(go, pq, 1.0), 0.0)
        d = d + alpha * p
        r = r - alpha * q
        rr_new = (r * r).sum(axis=0)
        beta = np.where(go & (rr != 0), rr_new / np.where(rr != 0, rr, 1.0), 0.0)
        rr = rr_new
        p = r + beta * p
        xs.append(x0 + d)
    return xs


def seam_energy_by_fetch(atlas, rows):
    """The seam energy of an atlas per channel in float64, from the view's own fetch (lightmapped_view_ref.fetch) at the kept
    sample pairs: sum |E(A) - E(B)|^2.  It reads the sample points only, not the rows' weights."""
    k = rows["kept"]
    ea, _ = L.fetch(atlas, rows["a"][k, 0] - F(0.5), rows["a"][k, 1] - F(0.5))
    eb, _ = L.fetch(atlas, rows["b"][k, 0] - F(0.5), rows["b"][k, 1] - F(0.5))
    diff = ea.astype(np.float64) - eb.astype(np.float64)
    return (diff * diff).sum(axis=0)


# ---- the inputs the tests share ------------------------------------------------------------------------------------------

def fin():
    """Three triangles that share the edge (0, 1): one non-manifold edge, no interior edge."""
    v = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0.5], [-0.6, 0.8, 0.5], [-0.6, -0.8, 0.5]], F)
    return v, np.array([(0, 1, 2), (0, 1, 3), (0, 1, 4)], np.uint32)


def patch():
    """One planar quad: one chart, one interior edge, no seam."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], F)
    return v, np.array([(0, 1, 2), (0, 2, 3)], np.uint32)


def random_atlas(owner_mask, seed):
    """rgb from a seeded generator on the owned texels, zeros and alpha 0 elsewhere."""
    rng = np.random.default_rng(seed)
    rgba = np.zeros(owner_mask.shape + (4,), F)
    rgba[..., 0:3] = rng.random(owner_mask.shape + (3,), dtype=F)
    rgba[..., 3] = 1.0
    rgba[~owner_mask] = 0.0
    return rgba
