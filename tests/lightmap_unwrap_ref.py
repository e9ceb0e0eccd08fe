"""numpy float32 restatement of lupin_hip_unwrap_lightmap_uvs (include/lupin_hip.h): classify, charts,
rectangles, packer and UVs, every float operation one rounded f32 operation in the order the header states, so that the
device's words can be compared one for one.  Also the small meshes the unwrap's tests share, and a scene builder.

The packer here (shelf_pack) is written out from the header's text, not imported from the Python host: the host's own
api.shelf_pack is held to it in tests/test_lightmap_unwrap_cpu.py."""
import math

import numpy as np

from lupinpathtracer_amd import api

F = np.float32
NO_CHART = 0xFFFFFFFF
MAX_SIZE = 16384


def classify(pos, tris):
    """Per triangle the bucket 2 * axis + (1 if negative), or -1 for a degenerate triangle."""
    p = np.asarray(pos, F).reshape(-1, 4)[:, :3] if np.asarray(pos).shape[-1] == 4 else np.asarray(pos, F).reshape(-1, 3)
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        a, b = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=-1)
    degenerate = ~np.isfinite(n).all(axis=1) | (n == 0).all(axis=1)
    mag = np.abs(n)
    k = np.zeros(len(t), np.int64)
    best = mag[:, 0].copy()
    with np.errstate(invalid="ignore"):
        y = mag[:, 1] > best
        k[y], best[y] = 1, mag[y, 1]
        z = mag[:, 2] > best
        k[z] = 2
    nk = n[np.arange(len(t)), k]
    with np.errstate(invalid="ignore"):
        bucket = 2 * k + np.where(nk >= 0, 0, 1)
    bucket[degenerate] = -1
    return p, t, bucket


def components(t, bucket):
    """Per triangle the label of its chart: the smallest triangle index of its connected component over (same bucket, shared
    vertex index), NO_CHART for a degenerate triangle.  A plain union-find in triangle order."""
    T = len(t)
    parent = list(range(T))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    first = {}
    for i in range(T):
        b = int(bucket[i])
        if b < 0:
            continue
        for v in t[i]:
            o = first.setdefault((b, int(v)), i)
            ra, rb = find(i), find(o)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) if bucket[i] >= 0 else NO_CHART for i in range(T)], np.int64).reshape(T)


def project(p, bucket):
    """(s, t) of points p (n, 3) in buckets `bucket` (n,): (p[(k+1)%3] + 0, p[(k+2)%3] + 0), swapped for a negative bucket."""
    k = bucket >> 1
    rows = np.arange(len(p))
    a = p[rows, (k + 1) % 3] + F(0)
    b = p[rows, (k + 2) % 3] + F(0)
    neg = (bucket & 1) == 1
    return np.where(neg, b, a).astype(F), np.where(neg, a, b).astype(F)


def isqrt_ceil(n):
    r = math.isqrt(n)
    return r if r * r == n else r + 1


def shelf_pack(rects):
    """rects: (w, h, label).  Returns (width, height, {label: (x, y)})."""
    order = sorted(rects, key=lambda r: (-r[1], -r[0], r[2]))
    width = max([r[0] for r in rects] + [isqrt_ceil(sum(r[0] * r[1] for r in rects))]) if rects else 0
    x = y = shelf = 0
    place = {}
    for w, h, label in order:
        if x + w > width:
            y += shelf
            x = shelf = 0
        place[label] = (x, y)
        x += w
        shelf = max(shelf, h)
    return width, y + shelf, place


def unwrap(pos, tris, texel_size, padding):
    """What lupin_hip_unwrap_lightmap_uvs writes for a mesh whose triangles, in the scene's own order, are `tris`: a dict of
    uvs (T, 3, 2) f32, chart_of_tri (T,) u32, num_charts, width, height, degenerate_tris, and for the tests labels (T,),
    bucket (T,) and the charts' rectangles {dense: (x, y, w, h)}.  None when the atlas is above MAX_SIZE (the call is refused)."""
    p, t, bucket = classify(pos, tris)
    T = len(t)
    label = components(t, bucket)
    good = bucket >= 0
    labels = np.unique(label[good])
    dense_of = {int(l): c for c, l in enumerate(labels)}
    texel = F(texel_size)
    uvs = np.zeros((T, 3, 2), F)
    chart = np.full(T, NO_CHART, np.uint32)
    s = np.zeros((T, 3), F)
    q = np.zeros((T, 3), F)
    for k in range(3):
        sk, qk = project(p[t[good, k]], bucket[good])
        s[good, k], q[good, k] = sk, qk
    rects, boxes = [], {}
    for l in labels:
        sel = label == l
        lo_s, hi_s, lo_t, hi_t = s[sel].min(), s[sel].max(), q[sel].min(), q[sel].max()
        with np.errstate(all="ignore"):
            ew, eh = np.ceil((hi_s - lo_s) / texel), np.ceil((hi_t - lo_t) / texel)
        if not (ew <= MAX_SIZE and eh <= MAX_SIZE):
            return None
        c = dense_of[int(l)]
        rects.append((max(int(ew), 1) + 2 * padding, max(int(eh), 1) + 2 * padding, c))
        boxes[c] = (lo_s, lo_t)
    width, height, place = shelf_pack(rects)
    if width > MAX_SIZE or height > MAX_SIZE:
        return None
    for l in labels:
        sel = label == l
        c = dense_of[int(l)]
        x, y = place[c]
        uvs[sel, :, 0] = F(x + padding) + (s[sel] - boxes[c][0]) / texel
        uvs[sel, :, 1] = F(y + padding) + (q[sel] - boxes[c][1]) / texel
        chart[sel] = c
    return dict(uvs=uvs, chart_of_tri=chart, num_charts=len(labels), width=width, height=height, degenerate_tris=int((~good).sum()),
                labels=label, bucket=bucket, rects={c: (*place[c], w, h) for w, h, c in rects})


# ---- the meshes the tests share: (positions (n, 3) f32, triangles (T, 3)) -------------------------------------------

def cube(size=1.0):
    """8 shared vertices, 12 triangles, outward winding: 6 charts of 2 triangles."""
    v = np.array([[x, y, z] for z in (0, 1) for y in (0, 1) for x in (0, 1)], F) * F(size)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]      # -z +z -y +y -x +x
    t = [tri for a, b, c, d in quads for tri in ((a, b, c), (a, c, d))]
    return v, np.array(t, np.uint32)


def octahedron():
    """Six vertices on the axes: every normal is (+-1, +-1, +-1), every tie goes to x: 2 charts of 4 triangles."""
    v = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
    t = []
    for sx, ix in ((1, 0), (-1, 1)):
        for sy, iy in ((1, 2), (-1, 3)):
            for sz, iz in ((1, 4), (-1, 5)):
                t.append((ix, iy, iz) if sx * sy * sz > 0 else (ix, iz, iy))
    return v, np.array(t, np.uint32)


def bowtie():
    """Two fans in the plane z = 0 (bucket +z) that meet in vertex 0 alone: one chart."""
    v = np.array([[0, 0, 0], [1, -0.5, 0], [1.5, 0, 0], [1, 0.5, 0], [-1, 0.5, 0], [-1.5, 0.25, 0], [-1, -0.5, 0]], F)
    t = [(0, 1, 2), (0, 2, 3), (0, 4, 5), (0, 5, 6)]
    return v, np.array(t, np.uint32)


def two_patches():
    """Two quads in the plane z = 0 without a common vertex: two charts in one bucket."""
    v = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [3, 0, 0], [4.5, 0, 0], [4.5, 0.75, 0], [3, 0.75, 0]], F)
    t = [(0, 1, 2), (0, 2, 3), (4, 5, 6), (4, 6, 7)]
    return v, np.array(t, np.uint32)


def chain(n=4099, reverse=False):
    """A strip of n triangles in the plane y = 0 whose triangle k shares vertices with k - 1 and k + 1 only through the strip:
    one chart, whose union needs every link.  4 099 is the smallest count that spans more than one 4 096-triangle stretch.
    `reverse`: the same strip with its triangle order reversed, so that the smallest label sits at the far end."""
    k = np.arange(n + 2)
    v = np.stack([(k // 2).astype(F) * F(0.25), np.zeros(n + 2, F), (k % 2).astype(F) * F(0.5)], axis=-1)
    t = np.array([(i, i + 2, i + 1) if i % 2 == 0 else (i, i + 1, i + 2) for i in range(n)], np.uint32)       # all normals +y
    return v, (t[::-1].copy() if reverse else t)


def with_bad_triangles():
    """two_patches plus a zero-area triangle and a triangle with a NaN vertex among the good ones."""
    v, t = two_patches()
    v = np.concatenate([v, np.array([[2, 2, 0], [2, 2, 0], [np.nan, 0, 0]], F)])
    t = np.concatenate([t[:2], np.array([[8, 9, 0], [0, 1, 10]], np.uint32), t[2:]])
    return v, t


def scene_cpu_of(meshes, instances=None, sky=None):
    """(SceneCPU, environment infos) of `meshes` ((positions, triangles) each) WITHOUT texcoords, one matte material, and
    `instances` ((mesh index, translation) each; default: every mesh once, in place); sky: a constant environment's emission."""
    from lupinpathtracer_amd._abi import INSTANCE_DTYPE, MATERIAL_DTYPE, MESH_INFO_DTYPE, ENVIRONMENT_DTYPE
    cpu = api.SceneCPU()
    m = api.default_material()
    m["color"] = (0.8, 0.8, 0.8, 1.0)
    cpu.materials = np.array([m], MATERIAL_DTYPE)
    for pos, tris in meshes:
        v = np.zeros((len(pos), 4), F)
        v[:, :3] = np.asarray(pos, F).reshape(-1, 3)
        cpu.verts_pos_array.append(v)
        cpu.indices_array.append(np.asarray(tris, np.uint32).reshape(-1))
    cpu.mesh_infos = np.array([api.default_mesh_info() for _ in meshes], MESH_INFO_DTYPE)
    insts = []
    for mesh_idx, move in (instances if instances is not None else [(i, (0, 0, 0)) for i in range(len(meshes))]):
        inst = api.default_instance()
        inst["mesh_idx"] = mesh_idx
        inst["transpose_inverse_transform"][:, 3] = -np.asarray(move, F)      # world -> local of a translation
        insts.append(inst)
    cpu.instances = np.array(insts, INSTANCE_DTYPE)
    envs = []
    if sky is not None:
        e = api.default_environment()
        e["emission"] = (sky, sky, sky)
        cpu.environments = np.array([e], ENVIRONMENT_DTYPE)
        envs = [api.EnvMapInfo(np.ones((1, 1, 4), F), 1, 1)]
    api.validate_scene(cpu, 0, 0)
    return cpu, envs


def upload(ctx, cpu, envs=(), textures=()):
    """The scene of a SceneCPU (ctx None: its descriptor alone, with the triangles in the scene's own order)."""
    return api.build_accel_structures_and_upload(ctx, cpu, list(textures), list(envs), True)


def scene_mesh(scene, cpu, mesh_idx):
    """(positions, triangles in the scene's own order) of a mesh: what the device unwraps."""
    from tests import lightmap_ref
    return np.asarray(cpu.verts_pos_array[mesh_idx], F).reshape(-1, 4)[:, :3], lightmap_ref.mesh_triangles(scene)[mesh_idx]


def corner_set(uvs):
    """A per-corner set as lightmap_ref.raster takes a chart: ((3T, 2) uvs, (T, 3) corner indices)."""
    uvs = np.asarray(uvs, F).reshape(-1, 2)
    return uvs, np.arange(len(uvs)).reshape(-1, 3)
