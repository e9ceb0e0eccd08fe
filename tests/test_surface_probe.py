"""What runs between a hit and the scattering functions -- texture lookup, material point, opacity, shading and geometric
normal, environment radiance -- through lupin_hip_surface_probe / oracle_surface_probe (record layout: include/lupin_hip.h).

CPU tests: the oracle against tests/surface_ref.py, an independent float64 restatement, point by point within a forward
error model the reference evaluates (its conditioning terms * 2^-24 * one constant per mode), at texture seams, and with each
reference property pinned by a twin that reads the text differently and must fail.
GPU tests (-m gpu): the device equals the oracle bit for bit on every query set, staged in LDS and from global memory.

The constants: measured on the query sets below as the largest ratio of |oracle - reference| to
conditioning * 2^-24, then set to at most 4 times that ratio, the margin for a later legal reordering of roundings."""
import hashlib
import os
import subprocess
import tempfile

import numpy as np
import pytest

from lupinpathtracer_amd import api
from lupinpathtracer_amd._abi import ENVIRONMENT_DTYPE, INSTANCE_DTYPE, MATERIAL_DTYPE, MESH_INFO_DTYPE
from tests import surface_ref as sr
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = api.SurfaceMode
EPS = 2.0 ** -24
TINY = 2.0 ** -140          # absolute floor: results in the float32 subnormal range round to multiples of 2^-149
# largest |oracle - reference| / (conditioning * 2^-24) measured over the CPU query sets of this file -> constant (<= 4 x)
#   TEXTURE      2.45 -> 9.0
#   MATERIAL     1.37 -> 5.0   (OPACITY, the same field computed on its own: 0.74)
#   NORMAL       0.152 -> 0.6
#   ENVIRONMENT  0.367 -> 1.4
C_MODE = {"TEXTURE": 9.0, "MATERIAL": 5.0, "NORMAL": 0.6, "ENVIRONMENT": 1.4}
MAX_EXCLUDED = 0.01         # of any one (scene, mode) set, as in test_light_probe.py

FIXTURES = ["features1", "materials1", "materials2", "materials3", "materials4", "materials5", "environments1", "environments2"]
SIZES = [(1, 1), (1, 7), (7, 1), (3, 5), (6, 10), (64, 64), (256, 128)]   # (width, height)


# ---- inputs ------------------------------------------------------------------------------------------------------------

def make_textures(seed=7):
    """Per size one RGBA8 texture (sRGB values on both sides of 0.04045 = 10.3 / 255; alpha unlike rgb) and one RGBA16F
    (subnormals, values above 1, values near 65504); then a 4 x 4 RGBA16F sky.  Index = 2 * size index + format."""
    rng = np.random.default_rng(seed)
    out = []
    for w, h in SIZES:
        t8 = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        low = rng.random((h, w, 3)) < 0.3
        t8[..., :3] = np.where(low, rng.integers(0, 21, (h, w, 3)), t8[..., :3])
        t8[..., 3] = 255 - t8[..., 0] // 2
        t16 = rng.uniform(0.0, 2.0, (h, w, 4)).astype(np.float16)
        kind = rng.integers(0, 8, (h, w, 4))
        t16 = np.where(kind == 0, np.float16(6e-8) * rng.integers(1, 900, (h, w, 4)).astype(np.float16), t16)   # subnormal halves
        t16 = np.where(kind == 1, rng.uniform(60000.0, 65504.0, (h, w, 4)).astype(np.float16), t16)
        out += [api.TextureCPU(np.ascontiguousarray(t8)), api.TextureCPU(np.ascontiguousarray(t16.astype(np.float16)))]
    sky = rng.uniform(0.05, 3.0, (4, 4, 4)).astype(np.float16)
    out.append(api.TextureCPU(sky))
    return out


def pad4(a, w=0.0):
    out = np.full((len(a), 4), w, np.float32)
    out[:, :a.shape[1]] = a
    return out


def soup_mesh(rng):
    """Six separate triangles: uv regular / mirrored (negative div) / all equal (div == 0) / outside [0, 1] with negative
    values / in the thousands / collinear (div == 0).  Returns positions, indices, uvs, normals, colours."""
    pos, uv = [], []
    uvs = [[(0.1, 0.2), (0.9, 0.3), (0.4, 0.8)],
           [(0.1, 0.2), (0.4, 0.8), (0.9, 0.3)],
           [(0.25, 0.75), (0.25, 0.75), (0.25, 0.75)],
           [(-2.3, 3.7), (1.6, -0.4), (-0.7, -5.1)],
           [(1000.25, -2000.5), (1003.5, -1999.25), (1001.0, -1996.75)],
           [(0.0, 0.0), (1.0, 2.0), (2.0, 4.0)]]
    for t in range(6):
        c = np.array([t % 3 - 1.0, t // 3 - 0.5, 0.0]) * 1.5
        p = c + rng.uniform(-0.6, 0.6, (3, 3))
        pos += list(p)
        uv += uvs[t]
    pos = np.array(pos, np.float32)
    idx = np.arange(18, dtype=np.uint32)
    nrm = np.zeros((18, 3))
    for t in range(6):
        p = pos[t * 3:t * 3 + 3].astype(np.float64)
        g = np.cross(p[2] - p[0], p[1] - p[0]); g /= np.linalg.norm(g)
        for k in range(3):
            v = g + rng.uniform(-0.4, 0.4, 3)
            nrm[t * 3 + k] = v / np.linalg.norm(v)
    col = rng.uniform(0.2, 1.0, (18, 4)).astype(np.float32)
    return pos, idx, np.array(uv, np.float32), nrm.astype(np.float32), col


def transform(kind, rng):
    """(4, 3) local -> world: 0 non-uniform scale, 1 shear, 2 reflection (negative determinant), 3 all with a rotation"""
    a = np.eye(3)
    if kind in (0, 3):
        a = a @ np.diag(rng.uniform(0.3, 3.0, 3))
    if kind in (1, 3):
        sh = np.eye(3); sh[0, 1] = rng.uniform(0.4, 0.9); sh[2, 0] = rng.uniform(-0.7, -0.3)
        a = sh @ a
    if kind in (2, 3):
        a = a @ np.diag([1.0, -1.0, 1.0])
    if kind == 3:
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        a = q @ a
    f = np.zeros((4, 3), np.float32)
    f[:3] = a.T          # rows of f = columns of the matrix
    f[3] = rng.uniform(-2, 2, 3)
    return f


class Probe:
    """A scene, its oracle-side build and the float64 reference over the same inputs."""

    def __init__(self, scene_cpu, textures, envs_info, ctx=None):
        self.cpu, self.textures, self.envs_info = scene_cpu, textures, envs_info
        order = []

        def builder(v, i):
            nodes, reordered = api.build_bvh(v, i)
            order.append(reordered)
            return nodes, reordered
        self.scene = api.build_accel_structures_and_upload(ctx, scene_cpu, textures, envs_info, True, blas_builder=builder)
        self.ref = sr.SurfaceRef(scene_cpu, textures, order)
        self.tris = [len(o) // 3 for o in order]


def synthetic_cpu(seed=3, big=False, simple=None):
    """Eight meshes = every combination of normals / texcoords / colours over the triangle soup; 16 materials = every
    LupinMatType without and with textures; 24 instances over the four transform kinds; two environments.
    big: one more instance of a 3200-triangle grid, so that the scene is traversed from global memory.
    simple: "plain" | "partial_alpha" | "vertex_colors" | "one_texture" | "one_env" -- matte-only scenes for the simple_matte
    predicate."""
    rng = np.random.default_rng(seed)
    s = api.SceneCPU()
    textures = make_textures()
    pos, idx, uv, nrm, col = soup_mesh(rng)
    infos = []
    for combo in range(8):
        if simple and combo not in (0, 1, 2, 3):
            continue
        if simple and simple != "vertex_colors" and combo & 4:
            continue
        info = api.default_mesh_info()
        s.verts_pos_array.append(pad4(pos)); s.indices_array.append(idx.copy())
        if combo & 1:
            info["normals_buf_idx"] = len(s.verts_normal_array); s.verts_normal_array.append(pad4(nrm))
        if combo & 2:
            info["texcoords_buf_idx"] = len(s.verts_texcoord_array); s.verts_texcoord_array.append(uv.copy())
        if combo & 4 or (simple == "vertex_colors" and combo == 3):
            info["colors_buf_idx"] = len(s.verts_color_array); s.verts_color_array.append(col.copy())
        infos.append(info)
    nmesh = len(infos)
    if big:
        n = 40
        gu, gw = np.meshgrid(np.linspace(0, 1, n + 1), np.linspace(0, 1, n + 1), indexing="ij")
        gv = np.stack([gu * 8 - 4, 0.3 * np.sin(9 * gu) * np.cos(7 * gw) - 3.0, gw * 8 - 4], -1).reshape(-1, 3).astype(np.float32)
        gi = []
        for i in range(n):
            for j in range(n):
                a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
                gi += [a, c, b, a, d, c]
        info = api.default_mesh_info()
        info["texcoords_buf_idx"] = len(s.verts_texcoord_array)
        s.verts_texcoord_array.append(np.stack([gu * 5 - 1, gw * 3], -1).reshape(-1, 2).astype(np.float32))
        s.verts_pos_array.append(pad4(gv)); s.indices_array.append(np.array(gi, np.uint32)); infos.append(info)
    s.mesh_infos = np.array(infos, MESH_INFO_DTYPE)

    ntex = 2 * len(SIZES)
    mats = []
    for t in range(8):
        for variant in range(2):
            m = api.default_material()
            m["mat_type"] = 0 if simple else t
            m["color"] = (*rng.uniform(0.2, 0.95, 3), 1.0 if variant == 0 and simple != "partial_alpha" else rng.uniform(0.3, 0.9))
            m["emission"][:3] = rng.uniform(0.0, 4.0, 3)
            m["roughness"] = rng.uniform(0.0, 0.9) if (t + variant) % 3 else rng.uniform(0.0, 0.05)
            m["metallic"] = rng.uniform(0, 1)
            m["ior"] = rng.uniform(1.1, 2.0)
            m["scattering"][:3] = rng.uniform(0.05, 0.9, 3)
            m["sc_anisotropy"] = rng.uniform(-0.6, 0.6)
            m["tr_depth"] = rng.uniform(0.02, 0.5)
            if variant == 1 and not simple:
                k = t * 5
                m["color_tex_idx"] = (k + 0) % ntex
                m["emission_tex_idx"] = (k + 3) % ntex
                m["roughness_tex_idx"] = (k + 6) % 10      # sizes up to 6 x 10: at texcoords in the thousands a wider texture's
                                                           # filter loses all precision, and rule E1 would exclude those queries
                m["scattering_tex_idx"] = (k + 9) % ntex
                m["normal_tex_idx"] = (k + 12) % ntex
            mats.append(m)
    if simple == "one_texture":
        mats[5]["color_tex_idx"] = 6
    s.materials = np.array(mats, MATERIAL_DTYPE)

    insts = []
    for i in range(24):
        insts.append(api.instance_from_transform(transform(i % 4, rng), i % nmesh, (i * 7 + i // 8) % 16))
    # every mesh with texcoords also under a textured material of a clamped and of a snapping type, under shear and reflection
    for j, mesh in enumerate(k for k in range(nmesh) if int(infos[k]["texcoords_buf_idx"]) != api.SENTINEL_IDX):
        for mat in (1, 3, 7, 9, 11, 13, 15, 5):
            insts.append(api.instance_from_transform(transform((j + mat) % 4, rng), mesh, mat))
    if big:
        insts.append(api.instance_from_transform(transform(1, rng), nmesh, 15))
    s.instances = np.array(insts, INSTANCE_DTYPE)

    envs, envs_info = [], []
    if not simple or simple == "one_env":
        e0 = api.default_environment(); e0["emission"] = (0.5, 0.55, 0.7); e0["emission_tex_idx"] = ntex
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        e0["transform"][:3, :3] = q.astype(np.float32)
        envs.append(e0)
        envs_info.append(api.EnvMapInfo(textures[ntex].pixels.astype(np.float32), 4, 4))
        if not simple:
            e1 = api.default_environment(); e1["emission"] = (0.05, 0.04, 0.03); envs.append(e1)
            envs_info.append(api.EnvMapInfo(np.ones((1, 1, 4), np.float32), 1, 1))
    s.environments = np.array(envs, ENVIRONMENT_DTYPE)
    api.validate_scene(s, len(textures), len(textures))
    return s, textures, envs_info


_cache = {}


def synthetic(ctx=None, **kw):
    key = (id(ctx) if ctx is not None else None, tuple(sorted(kw.items())))
    if key not in _cache:
        _cache[key] = Probe(*synthetic_cpu(**kw), ctx=ctx)
    return _cache[key]


def fixture_probe(name, ctx=None):
    from lupinpathtracer_amd import loader
    key = ("fixture", name, id(ctx) if ctx is not None else None)
    if key not in _cache:
        path = os.path.join(util.SCENES, name, name + ".json")
        scene_cpu, textures, envs_info, cams = loader.load_scene_cpu_yoctogl_v24(path, [util.SHARED])
        _cache[key] = Probe(scene_cpu, textures, envs_info, ctx=ctx)
    return _cache[key]


def barycentrics(rng, k):
    fixed = [(0, 0), (1, 0), (0, 1), (0.5, 0), (0, 0.5), (0.5, 0.5)]
    r0, r1 = rng.random(k), rng.random(k)
    rnd = np.stack([1 - np.sqrt(r0), r1 * np.sqrt(r0)], -1)
    return np.concatenate([np.array(fixed), rnd]).astype(np.float32)


def surface_queries(p, seed, per_tri=6, max_tris=40):
    """(instance, triangle, u, v) over every instance: the three vertices, the three edge midpoints and random points"""
    rng = np.random.default_rng(seed)
    rows = []
    for inst, rec in enumerate(p.cpu.instances):
        ntri = p.tris[int(rec["mesh_idx"])]
        tris = range(ntri) if ntri <= max_tris else rng.choice(ntri, max_tris, replace=False)
        for tri in tris:
            for bu, bv in barycentrics(rng, per_tri):
                rows.append((inst, int(tri), bu, bv))
    a = np.array(rows, np.float64)
    return a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32), a[:, 2:4].astype(np.float32)


def surface_record_set(p, mode, seed, **kw):
    inst, tri, uv = surface_queries(p, seed, **kw)
    return api.surface_records(mode, inst, tri, uv)


def direction_records(seed, n):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-2, 2, (n, 1))
    d[:6] = np.concatenate([np.eye(3), -np.eye(3)])      # axes: the poles of an untransformed environment and its u seam
    return api.surface_records(M.ENVIRONMENT, direction=d.astype(np.float32))


def texture_records(textures, seed, n_random=300):
    """Random coordinates in [-3, 4]^2 plus the seam set on every texture: u (and v) exactly 0, 1, -1, k / n, (k + 0.5) / n for
    every k, and one float either side of each; the other coordinate at a texel centre and at a random place."""
    rng = np.random.default_rng(seed)
    recs = []
    for ti, t in enumerate(textures):
        h, w = t.pixels.shape[:2]
        uv = [rng.uniform(-3, 4, (n_random, 2))]
        for axis, n in ((0, w), (1, h)):
            base = np.concatenate([[0.0, 1.0, -1.0], np.arange(n + 1) / n, (np.arange(n) + 0.5) / n, -(np.arange(n) + 0.5) / n]).astype(np.float32)
            c = np.concatenate([base, np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf))])
            for other in (np.float32(0.5 / (h if axis == 0 else w)), np.float32(rng.random())):
                q = np.zeros((len(c), 2)); q[:, axis] = c; q[:, 1 - axis] = other
                uv.append(q)
        uv = np.concatenate(uv).astype(np.float32)
        recs.append(api.surface_records(M.TEXTURE, ti, 0, uv))
    return np.concatenate(recs)


def periodic_records(textures):
    """u0 = k / 8 and u0 + m (exact in float32) for integer m up to 2^20 in magnitude, on both axes"""
    rows = []
    for ti in range(len(textures)):
        for m in (0, 1, -1, 2, 1000, -1000, 2 ** 16, -2 ** 16, 2 ** 20, -2 ** 20):
            for k in range(8):
                rows.append((ti, k / 8 + m, 0.3125))
                rows.append((ti, 0.6875, k / 8 + m))
    a = np.array(rows)
    return api.surface_records(M.TEXTURE, a[:, 0].astype(np.uint32), 0, a[:, 1:3].astype(np.float32))


EXTREME = [1e9, -1e9, 3e38, -3e38, np.inf, -np.inf, np.nan, 2147483648.0, -2147483648.0, 2147483520.0, -2147483904.0]


def extreme_records(textures):
    rows = []
    for ti in range(len(textures)):
        for a in EXTREME:
            for b in (0.3, a):
                rows += [(ti, a, b), (ti, b, a)]
    arr = np.array(rows, np.float64)
    return api.surface_records(M.TEXTURE, arr[:, 0].astype(np.uint32), 0, arr[:, 1:3].astype(np.float32))


# ---- comparison with the reference -------------------------------------------------------------------------------------

MAT_FIELDS = [("emission", 1, 3), ("color", 4, 3), ("opacity", 7, 1), ("roughness", 8, 1), ("metallic", 9, 1), ("ior", 10, 1),
              ("density", 11, 3), ("scattering", 14, 3), ("anisotropy", 17, 1)]


class ModelExceeded(AssertionError):
    """a compared value is outside the error model (or differs where the model allows no error)"""


class Tally:
    """largest error / (conditioning * 2^-24) per mode, and exclusions per set"""

    def __init__(self):
        self.ratio, self.worst, self.n, self.excluded = 0.0, None, 0, 0

    def check(self, got, want, cond, what):
        got, want, cond = np.atleast_1d(got).astype(np.float64), np.atleast_1d(want), np.atleast_1d(cond)
        for g, w, c in zip(got, want, np.broadcast_to(cond, got.shape)):
            assert np.isfinite(w) and np.isfinite(c), (what, w, c)
            err = abs(g - float(np.float32(w))) if c == 0.0 else abs(g - w)
            if c == 0.0:
                if err != 0.0:
                    raise ModelExceeded((what, g, w, "must be equal"))
                continue
            r = err / (c * EPS + TINY)
            if r > self.ratio:
                self.ratio, self.worst = r, (what, g, w, c)

    def done(self, what, constant):
        print(f"{what}: {self.n} queries, {self.excluded} excluded, largest error / model = {self.ratio:.3f} (constant {constant}) at {self.worst}")
        assert self.excluded <= MAX_EXCLUDED * self.n, (what, self.excluded, self.n)
        if self.ratio > constant:
            raise ModelExceeded((what, self.ratio, self.worst))


def check_material(p, rec, out, mode="MATERIAL", variant=None, tally=None):
    t = tally or Tally()
    for r, o in zip(rec, out):
        inst, tri = int(r.view(np.uint32)[1]), int(r.view(np.uint32)[2])
        val, cond, excl = p.ref.material_point(inst, tri, float(r[3]), float(r[4]), variant=variant)
        t.n += 1
        if mode == "OPACITY":
            t.check(o[0], val["opacity"], cond["opacity"], (inst, tri, "opacity"))
            continue
        assert int(o.view(np.uint32)[0]) == val["type"]
        if excl:
            t.excluded += 1
        for name, at, n in MAT_FIELDS:
            if name not in excl:
                t.check(o[at:at + n], val[name], cond[name], (inst, tri, float(r[3]), float(r[4]), name))
    return t


def check_normal(p, rec, out, variant=None, tally=None):
    t = tally or Tally()
    for r, o in zip(rec, out):
        inst, tri = int(r.view(np.uint32)[1]), int(r.view(np.uint32)[2])
        t.n += 1
        gv, gc, gex = p.ref.geometric_normal(inst, tri, variant=variant)
        sv, sc, sex = p.ref.shading_normal(inst, tri, float(r[3]), float(r[4]), variant=variant)
        if gex or sex:
            t.excluded += 1
        if not gex:
            t.check(o[3:6], gv, gc, (inst, tri, "geometric"))
        if not sex:
            t.check(o[0:3], sv, sc, (inst, tri, float(r[3]), float(r[4]), "shading"))
    return t


def check_texture(p, rec, out, tally=None):
    t = tally or Tally()
    for r, o in zip(rec, out):
        ti = int(r.view(np.uint32)[1])
        val, cond = p.ref.tex[ti].sample(float(r[3]), float(r[4]))
        t.n += 1
        t.check(o[0:4], val, cond, (ti, float(r[3]), float(r[4])))
    return t


def check_environment(p, rec, out, tally=None):
    t = tally or Tally()
    for r, o in zip(rec, out):
        d = [float(x) for x in r[5:8]]
        val, cond, uv, uvc, excl = p.ref.environment_radiance(d)
        t.n += 1
        if excl:
            t.excluded += 1
        if not (excl - {"E5"}):
            t.check(o[0:3], val, cond, (d, "radiance"))
            if not excl:
                t.check(o[3:5], uv, uvc, (d, "uv"))
    return t


# ---- CPU: oracle against reference -------------------------------------------------------------------------------------

def oracle_probe(p, rec):
    from oracle import oracle
    return oracle.surface_probe(p.scene, rec)


def test_record_layout_matches_the_header(built):
    text = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    assert f"#define LUPIN_SURFACE_IN_FLOATS {api.SURFACE_IN_FLOATS}\n" in text
    assert f"#define LUPIN_SURFACE_OUT_FLOATS {api.SURFACE_OUT_FLOATS}\n" in text
    for m in M:
        assert f"LUPIN_SURFACE_{m.name} = {int(m)}" in text


def test_texture_point_by_point_seams_and_periodicity(built):
    p = synthetic()
    rec = texture_records(p.textures, 21)
    check_texture(p, rec, oracle_probe(p, rec)).done("TEXTURE random + seams", C_MODE["TEXTURE"])
    rec = periodic_records(p.textures)
    out = oracle_probe(p, rec)
    check_texture(p, rec, out).done("TEXTURE periodic", C_MODE["TEXTURE"])
    # sample(u + m) against sample(u): within the sum of the two models
    t = Tally()
    big_exact = False
    per = 10 * 16
    for ti in range(len(p.textures)):
        blk_r, blk_o = rec[ti * per:(ti + 1) * per], out[ti * per:(ti + 1) * per]
        for j in range(16, per):
            base = j % 16
            _, c0 = p.ref.tex[ti].sample(float(blk_r[base][3]), float(blk_r[base][4]))
            v1, c1 = p.ref.tex[ti].sample(float(blk_r[j][3]), float(blk_r[j][4]))
            t.n += 1
            t.check(blk_o[j][:4], blk_o[base][:4].astype(np.float64), np.array(c0) + np.array(c1), (ti, j))
    t.done("TEXTURE sample(u + m) vs sample(u)", C_MODE["TEXTURE"])
    # the model is vacuous once the rounding of u * w - 0.5 reaches half a texel (it allows the texture's whole range), so:
    # where float32 evaluates u * w - 0.5 exactly on both axes, for u and for u + m, the two samples are the same bits
    exact_pairs = 0
    for ti, tx in enumerate(p.textures):
        h, w = tx.pixels.shape[:2]
        blk_r, blk_o = rec[ti * per:(ti + 1) * per], out[ti * per:(ti + 1) * per]
        x32 = (blk_r[:, 3] * np.float32(w)).astype(np.float32) - np.float32(0.5)
        y32 = (blk_r[:, 4] * np.float32(h)).astype(np.float32) - np.float32(0.5)
        ok = (x32.astype(np.float64) == blk_r[:, 3].astype(np.float64) * w - 0.5) & (y32.astype(np.float64) == blk_r[:, 4].astype(np.float64) * h - 0.5)
        for j in range(16, per):
            if ok[j] and ok[j % 16]:
                assert np.array_equal(blk_o[j, :4].view(np.uint32), blk_o[j % 16, :4].view(np.uint32)), (ti, blk_r[j])
                exact_pairs += 1
                if abs(blk_r[j, 3]) >= 2 ** 20 or abs(blk_r[j, 4]) >= 2 ** 20:
                    big_exact = True
    print(f"TEXTURE sample(u + m) == sample(u) bit for bit on {exact_pairs} pairs")
    assert exact_pairs > 600 and big_exact


def test_texture_equals_the_texel_at_centres(built):
    """Where float32 evaluates u * w - 0.5 to an integer exactly (every centre of a power-of-two size, most of the others),
    the weights are 1 and 0 and the sample is the texel itself."""
    p = synthetic()
    exact_total = 0
    for ti, t in enumerate(p.textures):
        h, w = t.pixels.shape[:2]
        ky, kx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        for off in (0, 3, -2):
            u = ((kx + np.float32(0.5)) / np.float32(w)).astype(np.float32) + np.float32(off)
            v = ((ky + np.float32(0.5)) / np.float32(h)).astype(np.float32) + np.float32(-off)
            x = (u * np.float32(w)).astype(np.float32) - np.float32(0.5)
            y = (v * np.float32(h)).astype(np.float32) - np.float32(0.5)
            exact = ((x == np.floor(x)) & (y == np.floor(y))).reshape(-1)
            if (w & (w - 1)) == 0 and (h & (h - 1)) == 0:
                assert exact.all()
            out = oracle_probe(p, api.surface_records(M.TEXTURE, ti, 0, np.stack([u.reshape(-1), v.reshape(-1)], -1)))
            want = t.pixels.reshape(-1, 4).astype(np.float32)
            if t.pixels.dtype == np.uint8:
                want = want / np.float32(255.0)
            assert np.array_equal(out[exact, :4], want[exact]), ti
            exact_total += int(exact.sum())
    assert exact_total > 50000


def test_material_opacity_and_normal_point_by_point(built):
    p = synthetic()
    rec = surface_record_set(p, M.MATERIAL, 5)
    check_material(p, rec, oracle_probe(p, rec)).done("MATERIAL synthetic", C_MODE["MATERIAL"])
    rec[:, 0] = float(M.OPACITY)
    check_material(p, rec, oracle_probe(p, rec), mode="OPACITY").done("OPACITY synthetic", C_MODE["MATERIAL"])
    rec[:, 0] = float(M.NORMAL)
    check_normal(p, rec, oracle_probe(p, rec)).done("NORMAL synthetic", C_MODE["NORMAL"])


def test_environment_point_by_point(built):
    p = synthetic()
    rec = direction_records(8, 3000)
    check_environment(p, rec, oracle_probe(p, rec)).done("ENVIRONMENT synthetic", C_MODE["ENVIRONMENT"])


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_scenes_point_by_point(built, name):
    p = fixture_probe(name)
    rec = surface_record_set(p, M.MATERIAL, 9, per_tri=1, max_tris=6)
    check_material(p, rec, oracle_probe(p, rec)).done(f"MATERIAL {name}", C_MODE["MATERIAL"])
    rec[:, 0] = float(M.NORMAL)
    check_normal(p, rec, oracle_probe(p, rec)).done(f"NORMAL {name}", C_MODE["NORMAL"])
    if len(p.cpu.environments):
        rec = direction_records(10, 400)
        check_environment(p, rec, oracle_probe(p, rec)).done(f"ENVIRONMENT {name}", C_MODE["ENVIRONMENT"])


# ---- reference properties, each with the twin that must fail ------------------------------------------------------------

def must_fail(fn):
    """the twin must fail in a numeric comparison (not at the exclusion cap, not at a NaN)"""
    with pytest.raises(ModelExceeded):
        fn()


MATERIAL_TWINS = ["no_srgb_decode", "alpha_decoded", "emission_decoded", "roughness_from_r", "roughness_not_squared",
                  "clamp_every_type", "density_every_type", "density_before_vertex_color", "texture_without_texcoords", "vertex_color_default_zero"]


@pytest.mark.parametrize("variant", MATERIAL_TWINS)
def test_material_properties_are_pinned(built, variant):
    """Properties 1, 2 and 7: the oracle agrees with the reference as written (test above) and not with the reading `variant`."""
    p = synthetic()
    rec = surface_record_set(p, M.MATERIAL, 5, per_tri=0)
    out = oracle_probe(p, rec)
    check_material(p, rec, out).done("as written", C_MODE["MATERIAL"])
    must_fail(lambda: check_material(p, rec, out, variant=variant).done(variant, C_MODE["MATERIAL"]))


@pytest.mark.parametrize("variant", ["forward_transform", "flip_xy_only", "fallback_frame_swapped", "cross_v1_v2"])
def test_normal_properties_are_pinned(built, variant):
    """Properties 3 (on the sheared instances), 4, 5 and 6."""
    p = synthetic()
    inst, tri, uv = surface_queries(p, 5, per_tri=2)
    if variant == "forward_transform":
        keep = np.array([k % 4 == 1 for k in range(24)] + [True] * (len(p.cpu.instances) - 24))[inst]   # kind 1 = shear
        inst, tri, uv = inst[keep], tri[keep], uv[keep]
    rec = api.surface_records(M.NORMAL, inst, tri, uv)
    out = oracle_probe(p, rec)
    check_normal(p, rec, out).done("as written", C_MODE["NORMAL"])
    must_fail(lambda: check_normal(p, rec, out, variant=variant).done(variant, C_MODE["NORMAL"]))


# ---- simple_matte ------------------------------------------------------------------------------------------------------

SIMPLE_KINDS = {"plain": True, "partial_alpha": True, "vertex_colors": False, "one_texture": False, "one_env": False}


@pytest.mark.parametrize("kind", sorted(SIMPLE_KINDS))
def test_simple_matte_in_the_oracle(built, kind):
    from oracle import oracle
    p = synthetic(simple=kind)
    rec = surface_record_set(p, M.MATERIAL, 12, per_tri=2)
    general = oracle_probe(p, rec)
    rec[:, 0] = float(M.MATERIAL_SIMPLE)
    if SIMPLE_KINDS[kind]:
        assert np.array_equal(oracle_probe(p, rec).view(np.uint32), general.view(np.uint32))
    else:
        with pytest.raises(oracle.SurfaceProbeError) as e:
            oracle_probe(p, rec)
        assert e.value.code == -3


def test_oracle_rejects_indices_outside_the_scene(built):
    from oracle import oracle
    p = synthetic()
    ninst, ntex = len(p.cpu.instances), len(p.textures)
    bad = [api.surface_records(M.TEXTURE, ntex, 0, [[0.5, 0.5]]), api.surface_records(M.TEXTURE, 0xFFFFFFFF, 0, [[0.5, 0.5]])]
    for mode in (M.MATERIAL, M.OPACITY, M.NORMAL):
        bad += [api.surface_records(mode, ninst, 0, [[0.2, 0.2]]), api.surface_records(mode, 0, p.tris[0], [[0.2, 0.2]]),
                api.surface_records(mode, 0, 0xFFFFFFFF, [[0.2, 0.2]])]
    for rec in bad:
        with pytest.raises(oracle.SurfaceProbeError) as e:
            oracle_probe(p, rec)
        assert e.value.code == -2
    out = oracle_probe(p, np.array([[7.0, 0, 0, 0, 0, 0, 0, 0], [np.nan, 0, 0, 0, 0, 0, 0, 0], [-1.0, 0, 0, 0, 0, 0, 0, 0]], np.float32))
    assert not out.any()      # no such mode: zeros


# ---- extreme coordinates: a sanitised host run first ------------------------------------------------------------------

SANITIZE_FLAGS = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
# sha256 over the texels of make_textures() and the records of extreme_records(make_textures()): the set the sanitised host run
# below passes.  The CPU test asserts it next to the sanitised result, the GPU test before it sends anything.
EXTREME_DIGEST = "1e7230f0ba2cea42a7bba13901bf0e30f150fa2b24c3774e5cc3c3cdd778e7ee"


def extreme_digest(textures, rec):
    h = hashlib.sha256()
    for t in textures:
        h.update(np.array([t.pixels.shape[1], t.pixels.shape[0], t.format], np.uint32).tobytes())
        h.update(np.ascontiguousarray(t.pixels).tobytes())
    h.update(np.ascontiguousarray(rec, np.float32).tobytes())
    return h.hexdigest()


def sanitizer_runtime_flags(tmp):
    """The flags that link a sanitizer runtime the host compiler has (static, else shared), found with an empty program that
    must build and start; skips when neither does.  Only this empty program can turn a failure into a skip."""
    src, exe = os.path.join(tmp, "empty.cpp"), os.path.join(tmp, "empty")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    errors = []
    for runtimes in (["-static-libasan", "-static-libubsan"], []):
        try:
            build = subprocess.run(["g++"] + SANITIZE_FLAGS + runtimes + [src, "-o", exe], capture_output=True, text=True, timeout=120)
            if build.returncode == 0:
                start = subprocess.run([exe], capture_output=True, text=True, timeout=60)
                if start.returncode == 0:
                    return runtimes
                errors.append(start.stderr[-300:])
            else:
                errors.append(build.stderr[-300:])
        except (OSError, subprocess.SubprocessError) as e:
            errors.append(str(e))
    pytest.skip("the host compiler's sanitizer runtimes are not usable: an empty program with -fsanitize=address,undefined fails: " + " | ".join(errors))


def sanitised_texture_run(textures, rec):
    """oracle_surface_probe's TEXTURE mode over `rec` in a host build with -fsanitize=address,undefined
    (tests/surface_sanitize_main.cpp), a stand-alone program: returns its outputs; fails on any sanitizer report and when the
    driver does not build.  Skips only when the host compiler has no usable sanitizer runtimes."""
    with tempfile.TemporaryDirectory() as tmp:
        runtimes = sanitizer_runtime_flags(tmp)
        exe, fin, fout = (os.path.join(tmp, n) for n in ("probe", "in.bin", "out.bin"))
        build = subprocess.run(["g++"] + SANITIZE_FLAGS + runtimes + ["-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-mfma", "-fopenmp",
                                "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "surface_sanitize_main.cpp"), "-o", exe],
                               capture_output=True, text=True, timeout=600)
        assert build.returncode == 0, build.stderr[-4000:]
        with open(fin, "wb") as f:
            f.write(np.array([len(textures), len(rec)], np.uint32).tobytes())
            for t in textures:
                f.write(np.array([t.pixels.shape[1], t.pixels.shape[0], t.format], np.uint32).tobytes())
                f.write(np.ascontiguousarray(t.pixels).tobytes())
            f.write(np.ascontiguousarray(rec, np.float32).tobytes())
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", OMP_NUM_THREADS="4")
        run = subprocess.run([exe, fin, fout], capture_output=True, text=True, env=env, timeout=600)
        assert run.returncode == 0 and "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr[-4000:]
        return np.fromfile(fout, np.float32).reshape(-1, api.SURFACE_OUT_FLOATS)


def test_extreme_coordinates_are_clean_under_the_sanitizers(built):
    """The sanitised host run of exactly the records test_device_equals_oracle_at_extreme_coordinates sends (pinned by
    EXTREME_DIGEST), and of the periodic set: it reports nothing and gives the oracle's bits."""
    p = synthetic()
    ext = extreme_records(p.textures)
    assert extreme_digest(p.textures, ext) == EXTREME_DIGEST
    rec = np.concatenate([ext, periodic_records(p.textures)])
    out = sanitised_texture_run(p.textures, rec)
    assert np.array_equal(out.view(np.uint32), oracle_probe(p, rec).view(np.uint32))


# ---- GPU: the device equals the oracle ---------------------------------------------------------------------------------

def assert_bits_equal(got, want, what):
    diff = got.view(np.uint32) != want.view(np.uint32)
    diff &= ~(np.isnan(got) & np.isnan(want))      # a NaN on both sides is equal whatever its sign and payload
    n = int(diff.sum())
    print(f"{what}: {n} differing words of {diff.size}")
    if n:
        i = int(np.argmax(diff.any(axis=1)))
        raise AssertionError(f"{what}: {n} differing words of {diff.size}; first at record {i}: device {got[i]} oracle {want[i]}")


@pytest.fixture(scope="module")
def global_ctx(built):
    old = os.environ.get("LUPIN_LDS_GEOMETRY")
    os.environ["LUPIN_LDS_GEOMETRY"] = "0"     # read at context creation: small scenes stay in global memory
    try:
        ctx = api.Context(0)
    finally:
        if old is None:
            os.environ.pop("LUPIN_LDS_GEOMETRY", None)
        else:
            os.environ["LUPIN_LDS_GEOMETRY"] = old
    yield ctx
    for k in [k for k, v in _cache.items() if v.scene.ctx is ctx]:
        del _cache[k]
    ctx.close()


def staged_in_lds(ctx, scene):
    try:
        api.trace_rays_wide(ctx, scene, [[0.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    except api.LupinError as e:
        assert "staged in LDS" in str(e), str(e)
        return True
    return False


def all_records(p):
    sets = [surface_record_set(p, mode, 5) for mode in (M.MATERIAL, M.OPACITY, M.NORMAL)]
    sets += [direction_records(8, 3000), texture_records(p.textures, 21), periodic_records(p.textures)]
    return np.concatenate(sets)


@pytest.mark.gpu
def test_device_equals_oracle_on_the_cpu_query_sets(gpu_ctx, global_ctx):
    host = synthetic()
    rec = all_records(host)
    want = oracle_probe(host, rec)
    for label, ctx in (("lds", gpu_ctx), ("global", global_ctx)):
        dev = synthetic(ctx)
        assert staged_in_lds(ctx, dev.scene) == (label == "lds")
        assert_bits_equal(api.surface_probe(ctx, dev.scene, rec), want, f"synthetic / {label}")
    big_host, big = synthetic(big=True), synthetic(gpu_ctx, big=True)
    assert not staged_in_lds(gpu_ctx, big.scene)
    rec = all_records(big_host)
    assert_bits_equal(api.surface_probe(gpu_ctx, big.scene, rec), oracle_probe(big_host, rec), "synthetic with the large mesh")


@pytest.mark.gpu
def test_device_equals_oracle_at_extreme_coordinates(gpu_ctx, global_ctx):
    """u, v of +-1e9, +-3e38, +-inf, NaN, +-2^31 and its neighbours on every texture: f2i_sat and both addressing paths.  The
    records are exactly the set that test_extreme_coordinates_are_clean_under_the_sanitizers passes through the sanitised host
    run: EXTREME_DIGEST pins it, and nothing is sent if the set has changed.  Nothing sanitised is built or run here."""
    host = synthetic()
    ext = extreme_records(host.textures)
    assert extreme_digest(host.textures, ext) == EXTREME_DIGEST
    want = oracle_probe(host, ext)
    for label, ctx in (("lds", gpu_ctx), ("global", global_ctx)):
        assert_bits_equal(api.surface_probe(ctx, synthetic(ctx).scene, ext), want, f"extreme coordinates / {label}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_device_equals_oracle_on_the_fixture_scenes(gpu_ctx, name):
    host, dev = fixture_probe(name), fixture_probe(name, gpu_ctx)
    sets = [surface_record_set(host, mode, 9, per_tri=1, max_tris=200) for mode in (M.MATERIAL, M.OPACITY, M.NORMAL)]
    sets.append(direction_records(10, 4000))
    rec = np.concatenate(sets)
    assert_bits_equal(api.surface_probe(gpu_ctx, dev.scene, rec), oracle_probe(host, rec), name)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", sorted(SIMPLE_KINDS))
def test_simple_matte_on_the_device(gpu_ctx, kind):
    host, dev = synthetic(simple=kind), synthetic(gpu_ctx, simple=kind)
    rec = surface_record_set(host, M.MATERIAL, 12, per_tri=2)
    general = api.surface_probe(gpu_ctx, dev.scene, rec)
    assert_bits_equal(general, oracle_probe(host, rec), f"{kind} / MATERIAL")
    rec[:, 0] = float(M.MATERIAL_SIMPLE)
    if SIMPLE_KINDS[kind]:
        assert np.array_equal(api.surface_probe(gpu_ctx, dev.scene, rec).view(np.uint32), general.view(np.uint32))
    else:
        with pytest.raises(api.LupinError) as e:
            api.surface_probe(gpu_ctx, dev.scene, rec)
        assert e.value.code == -1      # LUPIN_ERR_INVALID_ARGUMENT


@pytest.mark.gpu
def test_device_rejects_indices_outside_the_scene(gpu_ctx):
    """Checked on the host before any launch: the probe is no way to read out of bounds."""
    p = synthetic(gpu_ctx)
    ninst, ntex = len(p.cpu.instances), len(p.textures)
    bad = [api.surface_records(M.TEXTURE, ntex, 0, [[0.5, 0.5]]), api.surface_records(M.TEXTURE, 0xFFFFFFFF, 0, [[0.5, 0.5]])]
    for mode in (M.MATERIAL, M.MATERIAL_SIMPLE, M.OPACITY, M.NORMAL):
        bad += [api.surface_records(mode, ninst, 0, [[0.2, 0.2]]), api.surface_records(mode, 0, p.tris[0], [[0.2, 0.2]]),
                api.surface_records(mode, 0xFFFFFFFF, 0, [[0.2, 0.2]]), api.surface_records(mode, 0, 0xFFFFFFFF, [[0.2, 0.2]])]
    good = surface_record_set(p, M.NORMAL, 5, per_tri=0)[:64]
    for rec in bad:
        with pytest.raises(api.LupinError) as e:
            api.surface_probe(gpu_ctx, p.scene, np.concatenate([good, rec]))      # one bad record fails the whole call
        assert e.value.code == -1
    out = api.surface_probe(gpu_ctx, p.scene, np.array([[7.0, 0, 0, 0, 0, 0, 0, 0], [np.nan, 0, 0, 0, 0, 0, 0, 0], [-1.0, 0, 0, 0, 0, 0, 0, 0]], np.float32))
    assert not out.any()


@pytest.mark.gpu
def test_normals_follow_update_instances(gpu_ctx, global_ctx):
    """The sheared and the mirrored instances get new transforms in place: NORMAL (and the rest) equals the oracle on the updated
    scene and a scene created from the new transforms."""
    for label, ctx in (("lds", gpu_ctx), ("global", global_ctx)):
        cpu, textures, infos = synthetic_cpu()
        p = Probe(cpu, textures, infos, ctx=ctx)
        rng = np.random.default_rng(31)
        moved = cpu.instances.copy()
        for i in range(len(moved)):
            if i % 4 in (1, 2):
                moved[i] = api.instance_from_transform(transform(i % 4, rng), int(moved[i]["mesh_idx"]), int(moved[i]["mat_idx"]))
        p.scene.update_instances(moved)
        cpu2, _, _ = synthetic_cpu()
        cpu2.instances = moved
        fresh = Probe(cpu2, textures, infos, ctx=ctx)
        rec = np.concatenate([surface_record_set(fresh, mode, 5) for mode in (M.NORMAL, M.MATERIAL)])
        got = api.surface_probe(ctx, p.scene, rec)
        assert_bits_equal(got, oracle_probe(fresh, rec), f"updated scene / {label}")
        assert_bits_equal(got, api.surface_probe(ctx, fresh.scene, rec), f"updated against a fresh scene / {label}")
        old = oracle_probe(synthetic(), rec[:len(rec) // 2])
        assert (got[:len(rec) // 2, :3] != old[:, :3]).any()      # the normals did move


@pytest.mark.gpu
def test_device_equals_oracle_on_a_million_mixed_records(gpu_ctx):
    host, dev = synthetic(big=True), synthetic(gpu_ctx, big=True)
    base = all_records(host)
    rng = np.random.default_rng(44)
    n = 1 << 20
    rec = base[rng.integers(0, len(base), n)]
    surf = (rec[:, 0] >= 1) & (rec[:, 0] <= 4)
    rec[surf, 3:5] = barycentrics(rng, n)[6:][:int(surf.sum())]
    assert_bits_equal(api.surface_probe(gpu_ctx, dev.scene, rec), oracle_probe(host, rec), "2^20 mixed records")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["materials1", "instances1"])
def test_hits_of_the_tracer_feed_the_probe(gpu_ctx, name):
    """The 200 000 rays of test_gpu_parity.test_closest_hit_kernel_exact: their hits, as trace_rays returns them, go straight
    into MATERIAL and NORMAL."""
    from oracle import oracle
    scene, cams = util.load_scene(name, gpu_ctx)
    rng = np.random.default_rng(5)
    n = 200000
    ori = (rng.random((n, 3), dtype=np.float32) * 2 - 1) * np.float32(3.0) + np.array([0, 1, 0], np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(np.float32)
    d[:100] = np.array([0, -1, 0], np.float32)
    d[100:200] = np.array([1, 0, 0], np.float32)
    hit, dst, uv, inst, tri = api.trace_rays(gpu_ctx, scene, ori, d)
    h = hit == 1
    assert h.sum() > n // 10
    for mode in (M.MATERIAL, M.NORMAL):
        rec = api.surface_records(mode, inst[h], tri[h], uv[h])
        assert_bits_equal(api.surface_probe(gpu_ctx, scene, rec), oracle.surface_probe(scene, rec), f"{name} hits / {mode.name}")


def half_toward_zero(x):
    """float32 -> float16 rounded toward zero (the render target's store), for x >= 0"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    over = h.astype(np.float32) > x
    return np.where(over, np.nextafter(h, np.float16(0)), h)


@pytest.mark.gpu
def test_falsecolor_images_show_the_probe_values(gpu_ctx):
    """The tie to a shipped kernel.  One sample per pixel on the fuzz scene: the falsecolor kernel's Opacity image is the probe's
    opacity at the primary hit of every pixel, and its Albedo, Normals and Emission images are the probe's color, shading
    normal and emission there wherever that opacity is 1 (the alpha-skipping query then stops at the primary hit without
    drawing a random number) -- each max(., 0) and rounded to half toward zero as the kernel stores it; 0 where the ray
    misses.  The primary hits come from the camera rays (oracle.camera_rays, the rays the parity tests tie to the kernel's)
    through trace_rays."""
    from oracle import oracle
    from tests.test_gpu_fuzz import random_scene
    scene_cpu, textures, envs_info, cams = random_scene(2)
    scene = api.build_accel_structures_and_upload(gpu_ctx, scene_cpu, textures, envs_info)
    cam = cams[0]
    W, H = 120, 80
    res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=4, samples_per_pixel=1))
    desc = api.PathtraceDesc(camera_params=cam.params, camera_transform=cam.transform)
    tex = api.Texture(gpu_ctx, W, H)
    images = {}
    for ft in (api.FalsecolorType.Albedo, api.FalsecolorType.Normals, api.FalsecolorType.Emission, api.FalsecolorType.Opacity):
        api.pathtrace_scene_falsecolor(gpu_ctx, res, scene, tex, ft, desc)
        images[ft] = tex.download().reshape(-1, 4)[:, :3].copy()
    ori, d = oracle.camera_rays(scene, W, H, cam.params, cam.transform)
    hit, dst, uv, inst, tri = api.trace_rays(gpu_ctx, scene, ori.reshape(-1, 3), d.reshape(-1, 3), api.AdvancedParams().ray_epsilon)
    h = hit == 1
    assert h.sum() > W * H // 4 and (~h).sum() > 0
    mat = api.surface_probe(gpu_ctx, scene, api.surface_records(M.MATERIAL, inst[h], tri[h], uv[h]))
    nrm = api.surface_probe(gpu_ctx, scene, api.surface_records(M.NORMAL, inst[h], tri[h], uv[h]))
    opa = api.surface_probe(gpu_ctx, scene, api.surface_records(M.OPACITY, inst[h], tri[h], uv[h]))
    assert np.array_equal(opa[:, 0].view(np.uint32), mat[:, 7].view(np.uint32))
    opaque = mat[:, 7] >= 1.0
    assert opaque.sum() > W * H // 8 and (~opaque).sum() > 50      # the scene has alpha holes and partial opacity
    for ft, values, where in ((api.FalsecolorType.Opacity, np.repeat(mat[:, 7:8], 3, axis=1), np.ones(len(mat), bool)),
                              (api.FalsecolorType.Albedo, mat[:, 4:7], opaque), (api.FalsecolorType.Emission, mat[:, 1:4], opaque),
                              (api.FalsecolorType.Normals, nrm[:, 0:3], opaque)):
        want = half_toward_zero(np.maximum(values, np.float32(0.0)))
        got = images[ft][h]
        bad = int((got[where].view(np.uint16) != want[where].view(np.uint16)).sum())
        print(f"{ft.name}: {bad} differing f16 words of {want[where].size} at {int(where.sum())} primary hits")
        assert bad == 0, ft
        assert not images[ft][~h].any(), ft      # a miss shows 0
    assert images[api.FalsecolorType.Albedo][h][opaque].any() and images[api.FalsecolorType.Emission][h][opaque].any()
