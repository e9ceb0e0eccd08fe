"""numpy restatement of the adaptive history's reprojection (csrc/lupin_reproject.hpp) in float32 with the
kernels' order of operations: the pixel-centre ray (camera_ray_centre), its inverse (rp_project) and the gather.  The gather
takes visibility buffers as input, the device's or the ones visibility_from_oracle makes from the oracle's closest-hit
query, so it runs without a GPU."""
import ctypes as C

import numpy as np

from lupinpathtracer_amd import api

MISS = np.uint32(0xFFFFFFFF)
SNAP = np.float32(64.0)


def f(x):
    return np.float32(x)


def _normalize(x, y, z):
    """lpm_normalize3f: v * (1 / |v|)."""
    inv = f(1.0) / np.sqrt(x * x + y * y + z * z)
    return x * inv, y * inv, z * inv


def film_size(cp):
    film, aspect = f(cp.film), f(cp.aspect)
    return (film, film / aspect) if aspect >= f(1.0) else (film * aspect, film)


def centre_rays(width, height, cp, transform):
    """camera_ray_centre for every pixel: (ori (H, W, 3), dir (H, W, 3)), float32."""
    m = np.asarray(transform, np.float32).reshape(4, 3)
    gy, gx = np.meshgrid(np.arange(height, dtype=np.float32), np.arange(width, dtype=np.float32), indexing="ij")
    resx, resy = f(width), f(height)
    pcx, pcy = gx + f(0.5), (resy - gy) + f(0.5)
    uvx, uvy = (pcx + f(0.0)) / resx, (pcy + f(0.0)) / resy
    lens, focus = f(cp.lens), f(cp.focus)
    fsx, fsy = film_size(cp)
    zero = np.zeros_like(uvx)
    with np.errstate(all="ignore"):
        if cp.is_orthographic:
            sc = f(1.0) / lens
            qx, qy = fsx * (f(0.5) - uvx) * sc, fsy * (f(0.5) - uvy) * sc
            ex, ey, ez = -qx + f(0.0), -qy + f(0.0), zero
            dx, dy, dz = _normalize(-qx - ex, -qy - ey, (-focus) - ez)
        else:
            qx, qy, qz = fsx * (f(0.5) - uvx), fsy * (f(0.5) - uvy), zero + lens
            lx, ly, lz = _normalize(qx, qy, qz)
            lx, ly, lz = -lx, -ly, -lz
            ex, ey, ez = zero, zero, zero
            az = np.abs(lz)
            dx, dy, dz = _normalize((lx * focus) / az - ex, (ly * focus) / az - ey, (lz * focus) / az - ez)
        dz = dz * f(-1.0)
        dx, dy = dx * f(1.0), dy * f(1.0)
        ori = np.stack([m[0][k] * ex + m[1][k] * ey + m[2][k] * ez + m[3][k] * f(1.0) for k in range(3)], -1)
        d = _normalize(*[m[0][k] * dx + m[1][k] * dy + m[2][k] * dz + m[3][k] * f(0.0) for k in range(3)])
    return ori.astype(np.float32), np.stack(d, -1).astype(np.float32)


def mat_point(m, p):
    """rp_mat_point: affine LupinMat3x4 (4 columns x 3 rows) applied to points (..., 3)."""
    m = np.asarray(m, np.float32).reshape(4, 3)
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    return np.stack([m[0][k] * x + m[1][k] * y + m[2][k] * z + m[3][k] for k in range(3)], -1)


def rows_point(rows, p):
    """rp_rows_point: per-point affine rows (N, 3, 4) applied to points (N, 3)."""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([x * rows[:, k, 0] + y * rows[:, k, 1] + z * rows[:, k, 2] + rows[:, k, 3] for k in range(3)], -1)


def camera_inverse(transform):
    return api.mat3x4_inverse(np.asarray(transform, np.float32).reshape(4, 3))


def depth_of(transform, ori, dir_, t):
    """Camera-space z of ori + dir * t, as k_reproject_trace computes it."""
    p = ori + dir_ * np.asarray(t, np.float32)[..., None]
    return mat_point(camera_inverse(transform), p)[..., 2]


def project(cp, width, height, pc):
    """rp_project: continuous pixel coordinates (integers = pixel centres) of camera-space points (..., 3), before the snap."""
    fsx, fsy = film_size(cp)
    lens = f(cp.lens)
    x, y, z = pc[..., 0], pc[..., 1], pc[..., 2]
    with np.errstate(all="ignore"):
        if cp.is_orthographic:
            uvx, uvy = f(0.5) + (x * lens) / fsx, f(0.5) + (y * lens) / fsy
        else:
            uvx, uvy = f(0.5) + (x * lens) / (z * fsx), f(0.5) + (y * lens) / (z * fsy)
        resx, resy = f(width), f(height)
        return uvx * resx - f(0.5), (resy + f(0.5)) - uvy * resy


def local_to_world_rows(transpose_inverse_transforms):
    """(n, 3, 4) world -> local rows -> (n, 3, 4) local -> world rows through Mat3x4::inverse, as the host does."""
    t = np.asarray(transpose_inverse_transforms, np.float32).reshape(-1, 3, 4)
    return np.stack([api.mat3x4_inverse(np.ascontiguousarray(r.T)).T for r in t]).astype(np.float32) if len(t) else np.zeros((0, 3, 4), np.float32)


def mesh_arrays(scene, i):
    """Views of mesh i as the scene holds it: (vertex positions (V, 4) float32, the builder's reordered indices (3 T,) uint32)."""
    md = scene.desc.meshes[i]
    v = np.ctypeslib.as_array(C.cast(md.verts_pos, C.POINTER(C.c_float)), (md.num_verts, 4)) if md.num_verts else np.zeros((0, 4), np.float32)
    idx = np.ctypeslib.as_array(C.cast(md.indices, C.POINTER(C.c_uint32)), (md.num_indices,)) if md.num_indices else np.zeros(0, np.uint32)
    return v, idx


def scene_triangles(scene):
    """(vertices (T, 3, 3) of every global triangle: the meshes' triangles in order, as uploaded; first global triangle per mesh)."""
    tris, offsets, total = [], [], 0
    for i in range(scene.desc.num_meshes):
        v, idx = mesh_arrays(scene, i)
        offsets.append(total)
        tris.append(v[idx.reshape(-1, 3)][:, :, :3].astype(np.float32))
        total += len(idx) // 3
    return (np.concatenate(tris) if tris else np.zeros((0, 3, 3), np.float32)), np.array(offsets, np.uint32)


def global_triangle(scene, inst, tri_local):
    """Mesh-local triangle numbers (trace_rays') -> global ones (the visibility record's)."""
    _, offsets = scene_triangles(scene)
    mesh = scene.instances["mesh_idx"][np.minimum(inst, len(scene.instances) - 1)]
    return (offsets[mesh] + tri_local).astype(np.uint32)


def visibility_from_oracle(scene, width, height, cp, transform, ray_epsilon=0.001):
    """(inst, tri, uv, depth) of a view through the oracle's closest-hit query on the restated centre rays."""
    from oracle import oracle
    ori, d = centre_rays(width, height, cp, transform)
    hit, dst, uv, inst, tri = oracle.trace_rays(scene, ori.reshape(-1, 3), d.reshape(-1, 3), ray_epsilon)
    hit = hit.astype(bool)
    inst = np.where(hit, inst, MISS).astype(np.uint32)
    tri = np.where(hit, global_triangle(scene, np.where(hit, inst, 0), tri), 0).astype(np.uint32)
    depth = np.where(hit, depth_of(transform, ori.reshape(-1, 3), d.reshape(-1, 3), dst), f(0.0)).astype(np.float32)
    uv = np.where(hit[:, None], uv, f(0.0)).astype(np.float32)
    return inst.reshape(height, width), tri.reshape(height, width), uv.reshape(height, width, 2), depth.reshape(height, width)


def gather(cur, prev, prev_cp, prev_transform, tris, prev_rows, frames_in, moments_in, colour_in, depth_tolerance, max_history=0,
           prev_valid=True):
    """k_reproject_gather.  cur / prev: (inst, tri, uv, depth) of the new / the previous view; prev_cp, prev_transform: the
    previous camera; tris: scene_triangles' vertices; prev_rows: local_to_world_rows of the previous transforms;
    colour_in: (H, W, 3) float32, what the kernel reads (the f32 accumulator, or the f16 texel widened).
    Returns (colour (H, W, 3) float32, texel (H, W, 4) float16, n (H, W) uint32, moments (H, W, 2) float32)."""
    inst, tri, uv, _ = cur
    H, W = inst.shape
    n = np.zeros(H * W, np.uint32)
    mom = np.zeros((H * W, 2), np.float32)
    col = np.zeros((H * W, 3), np.float32)
    idx = np.nonzero(inst.reshape(-1) != MISS)[0]
    if prev_valid and len(idx):
        p_inst, p_depth = prev[0].reshape(-1), prev[3].reshape(-1)
        fin = np.asarray(frames_in, np.uint32).reshape(-1)
        min_ = np.asarray(moments_in, np.float32).reshape(-1, 2)
        cin = np.asarray(colour_in, np.float32).reshape(-1, 3)
        tol = f(depth_tolerance)
        ii = inst.reshape(-1)[idx]
        u, v = uv.reshape(-1, 2)[idx, 0], uv.reshape(-1, 2)[idx, 1]
        tv = tris[tri.reshape(-1)[idx]]
        w0 = (f(1.0) - u) - v
        pl = tv[:, 0] * w0[:, None] + tv[:, 1] * u[:, None] + tv[:, 2] * v[:, None]
        with np.errstate(all="ignore"):
            pc = mat_point(camera_inverse(prev_transform), rows_point(prev_rows[ii], pl))
            z = pc[:, 2]
            fx, fy = project(prev_cp, W, H, pc)
            sx, sy = np.rint(fx * SNAP) / SNAP, np.rint(fy * SNAP) / SNAP
            ok = (z > f(0.0)) & (sx > f(-1.0)) & (sx < f(W)) & (sy > f(-1.0)) & (sy < f(H))
            sx, sy = np.where(ok, sx, f(0.0)), np.where(ok, sy, f(0.0))
            x0f, y0f = np.floor(sx), np.floor(sy)
            tx, ty = sx - x0f, sy - y0f
            x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
            bw = [(f(1.0) - tx) * (f(1.0) - ty), tx * (f(1.0) - ty), (f(1.0) - tx) * ty, tx * ty]
            w, nq, q = [], [], []
            nmin = np.full(len(idx), 0xFFFFFFFF, np.uint32)
            for k in range(4):
                qx, qy = x0 + (k & 1), y0 + (k >> 1)
                valid = ok & (bw[k] > f(0.0)) & (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
                qi = np.where(valid, qy * W + qx, 0)
                nn = fin[qi]
                valid &= (nn >= 1) & (p_inst[qi] == ii)
                valid &= np.abs(p_depth[qi] - z) <= tol * z
                w.append(np.where(valid, bw[k], f(0.0)).astype(np.float32))
                nq.append(np.where(valid, nn, 0).astype(np.uint32))
                q.append(qi)
                nmin = np.where(valid, np.minimum(nmin, nn), nmin)
            wsum = ((w[0] + w[1]) + w[2]) + w[3]
            have = wsum > f(0.0)
            nn_out = np.minimum(nmin, np.uint32(max_history)) if max_history else nmin
            nf = nn_out.astype(np.float32)
            s = np.zeros((len(idx), 5), np.float32)
            for k in range(4):
                use = w[k] > f(0.0)
                m2 = np.where(nq[k] == nn_out, min_[q[k], 1], (min_[q[k], 1] / nq[k].astype(np.float32)) * nf)
                terms = np.stack([cin[q[k], 0], cin[q[k], 1], cin[q[k], 2], min_[q[k], 0], m2], -1)
                s = np.where(use[:, None], s + w[k][:, None] * terms, s)
            out = s / wsum[:, None]
        n[idx] = np.where(have, nn_out, 0)
        col[idx] = np.where(have[:, None], out[:, :3], f(0.0))
        mom[idx] = np.where(have[:, None], out[:, 3:], f(0.0))
    texel = np.ones((H * W, 4), np.float16)
    with np.errstate(over="ignore"):
        texel[:, :3] = col.astype(np.float16)   # round to nearest even
    return col.reshape(H, W, 3), texel.reshape(H, W, 4), n.reshape(H, W), mom.reshape(H, W, 2)
