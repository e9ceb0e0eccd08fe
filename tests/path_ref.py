"""float64 restatement of the four integrator loops: pathtrace_standard, pathtrace_mis, pathtrace_naive and
pathtrace_direct, written from the reference's shader (pathtracer.wgsl:588-1245 the loops, :1774-1783 clamp_radiance,
bvh_custom.wgsl:154-180 the opacity pass-through) and composed from the float64 references of the pieces: closest_hit_ref
(closest hit, shadow rays), surface_ref (material point, opacity, shading normal, emission, environments), scatter_ref (BSDF,
delta, phase, medium), light_ref (sample, pdf) and camera_ref (the u32 RNG, reproduced exactly).  Nothing here is taken from
integrate_vertex or from the oracle.

Vectorised over paths.  One run at the largest max_bounces serves every smaller one: a path with max_bounces = B draws the
same numbers as the same path with a larger B, so its radiance is the radiance after vertex B of the longer run (`at`).  MIS
and Direct add their shadow terms inside the vertex, so they are part of that prefix.

Reference quirks, restated as they are:
  Q1  MIS: a BSDF-sampled ray that leaves the scene adds the environment with its MIS weight, and the next iteration, whose
      hit is that stored miss, adds it again with the full weight (tests/test_pins.py).
  Q2  MIS: next_intersection is only written when the BSDF sample passes the gate (all(bsdfcos != 0) and mis_weight != 0);
      otherwise the next iteration reads the hit stored by an earlier vertex (or the initial miss).
  Q3  MIS: a zero BSDF sample leaves the inner loop only; incoming stays zero and the weight becomes non-finite.
  Q4  the volume stack holds one entry: entering a second body pops the first.
  Q5  inside a medium the scatter branch draws three numbers and uses two.
  Q6  Direct: the environment of a miss is added only after a delta vertex (or at the first vertex).

Decisions (each with a margin; a path is decisive when every decision up to the vertex asked for is clear): the closest hit
(closest_hit_ref's own rule at the relative floor S_PATH), the opacity coin, the light / slot / texel picks, the lobe pick,
total internal reflection, the sign tests of the normal against both directions (evaluation side, volume stack), volume_dst
against hit_dst, the channel pick, the light pdf's crossings (light_ref.pdf's margins), roulette, and the weight / pdf gates.
The mixture coin rnd < 0.5 and the alias thresholds compare exact f32 numbers and need no margin."""
import math
from dataclasses import dataclass, field

import numpy as np

from lupinpathtracer_amd import api
from lupinpathtracer_amd._abi import ENVIRONMENT_DTYPE, INSTANCE_DTYPE, MATERIAL_DTYPE, MESH_INFO_DTYPE
from tests import camera_ref
from tests import closest_hit_ref as X
from tests import light_ref as L
from tests import reproject_ref
from tests import scatter_ref as S
from tests import surface_ref

PT = api.PathtraceType
INTEGRATORS = (PT.Standard, PT.MIS, PT.Naive, PT.Direct)
LADDER = (0, 1, 2, 4, 8)
EPS = 1e-3                   # ray_epsilon of every query here
NO_CLAMP, CLAMP = 1e30, 2.0  # max_radiance: one that scales no path here (a non-finite radiance is zeroed under any), one that scales hundreds
F32_MAX = float(np.finfo(np.float32).max)

# event kinds of a vertex, and how a path ended at it
NOT_REACHED, MISS, SURF_BSDF, SURF_LIGHT, DELTA, MEDIUM = range(6)
KIND_NAMES = ("not reached", "miss", "surface, BSDF turn", "surface, light turn", "delta", "medium scatter")
RUNS, END_ROULETTE, END_WEIGHT, END_ZERO_INCOMING = range(4)
END_NAMES = ("continues", "ended by roulette", "ended by a zero or non-finite weight", "ended by a zero direction")

# Margins.  The f32 path reaches a vertex with a position and a direction that differ from the float64 ones by the roundings
# of the vertices before it; over the ladder here the oracle's radiance stays within 1e-4 of the float64 one (MEASURED below),
# and a quantity compared with a random number is no worse conditioned than the weight.  REL is ten times that.
REL = 1e-3                   # |rnd - threshold| of a computed threshold (opacity, Fresnel, survive), |k| of the TIR test
SIGN = 1e-3                  # |n . w| of a sign test on unit vectors
S_PATH = 1e-3                # closest_hit_ref's relative floor for rays whose origin carries the path's error
PICK = 8.0 * 2.0 ** -24      # relative rounding of rnd * n against an integer (exact inputs, one product)
EDGE, EPS_REL, MIN_COS, TEXEL = 2e-4, 2e-4, 1e-2, 2e-3   # light_ref.pdf's margins: twice those of tests/test_light_probe.py, whose queries are exact

DEFECTS = ("roulette_from_2", "roulette_from_4", "survive_cap_1", "no_survive_divide", "balance_heuristic", "mis_no_pdf_divide",
           "direct_keeps_next_emission", "mis_keeps_next_emission", "direct_emission_always", "medium_draw_kept", "no_tr_over_tp",
           "medium_pushed_not_popped", "clamp_per_channel", "mixture_half_bsdf_only", "loop_ends_before_max",
           "opacity_coin_always")


# ------------------------------------------------------------------------------------------------ the scene
(M_ROOM, M_GLOSSY, M_REFL_R, M_REFL_D, M_TRANSP_R, M_TRANSP_D, M_REFR_R, M_REFR_D, M_PBR, M_SUBSURF, M_VOLUME, M_LIGHT_A,
 M_LIGHT_TEX, M_LIGHT_INST, M_OPACITY, M_NORMAL_MAP, M_LIGHT_INF) = range(17)


def _materials(matte_only):
    m = np.array([api.default_material() for _ in range(17)], MATERIAL_DTYPE)

    def put(i, type_, color, rough=0.0, **kw):
        m[i]["mat_type"], m[i]["color"], m[i]["roughness"] = int(type_), tuple(color) + ((1.0,) if len(color) == 3 else ()), rough
        for k, v in kw.items():
            m[i][k] = v
    T = api.MaterialType
    put(M_ROOM, T.Matte, (0.7, 0.6, 0.5), 1.0)
    put(M_GLOSSY, T.Glossy, (0.3, 0.6, 0.4), 0.5)
    put(M_REFL_R, T.Reflective, (0.9, 0.7, 0.4), 0.5)
    put(M_REFL_D, T.Reflective, (0.8, 0.8, 0.9), 0.0)
    put(M_TRANSP_R, T.Transparent, (0.8, 0.9, 0.7), 0.4)
    put(M_TRANSP_D, T.Transparent, (0.9, 0.8, 0.8), 0.0)
    put(M_REFR_R, T.Refractive, (0.7, 0.8, 0.9), 0.4, tr_depth=0.1)
    put(M_REFR_D, T.Refractive, (0.9, 0.7, 0.7), 0.0, tr_depth=0.1)
    put(M_PBR, T.GltfPbr, (0.6, 0.4, 0.7), 0.6, metallic=0.5)
    put(M_SUBSURF, T.Subsurface, (0.8, 0.6, 0.5), 0.5, tr_depth=0.07, sc_anisotropy=-0.3)   # no scattering colour: a scatter inside zeroes the weight
    put(M_VOLUME, T.Volumetric, (0.5, 0.7, 0.9), 0.0, tr_depth=0.4, scattering=(0.9, 0.8, 0.7, 0.0), sc_anisotropy=0.4)
    put(M_LIGHT_A, T.Matte, (0.5, 0.5, 0.5), 1.0, emission=(9.0, 8.0, 7.0, 0.0))
    put(M_LIGHT_TEX, T.Matte, (0.5, 0.5, 0.5), 1.0, emission=(8.0, 8.0, 8.0, 0.0), emission_tex_idx=0)
    put(M_LIGHT_INST, T.Matte, (0.2, 0.2, 0.2), 1.0, emission=(3.0, 5.0, 7.0, 0.0))
    put(M_OPACITY, T.Matte, (0.4, 0.5, 0.8, 0.5), 1.0)
    put(M_NORMAL_MAP, T.Matte, (0.8, 0.8, 0.8), 1.0, normal_tex_idx=1)
    # an emitter of infinite radiance: every path that collects it has a non-finite radiance in f32 and in float64 alike, away
    # from every gate, so clamp_radiance's first branch is reached by decisive paths
    put(M_LIGHT_INF, T.Matte, (0.5, 0.5, 0.5), 1.0, emission=(np.inf, np.inf, np.inf, 0.0))
    if matte_only:
        for i in range(17):
            if i not in (M_LIGHT_A, M_LIGHT_INST):
                put(i, T.Matte, tuple(float(x) for x in m[i]["color"][:3]), 1.0)
                m[i]["emission"], m[i]["emission_tex_idx"], m[i]["normal_tex_idx"] = 0.0, api.SENTINEL_IDX, api.SENTINEL_IDX
    return m


def _textures(rng):
    """0: the emission texture (f16, 4 x 4), 1: the normal map (u8, 8 x 8, normals within 35 degrees of +z)."""
    em = np.ones((4, 4, 4), np.float32)
    em[..., :3] = rng.uniform(0.2, 1.0, (4, 4, 3))
    a, r = rng.uniform(0, 2 * math.pi, (8, 8)), rng.uniform(0.0, 0.55, (8, 8))
    n = np.stack([r * np.cos(a), r * np.sin(a), np.sqrt(1 - r * r)], -1)
    nm = np.full((8, 8, 4), 255, np.uint8)
    nm[..., :3] = np.round((n * 0.5 + 0.5) * 255)
    return [api.TextureCPU(em.astype(np.float16)), api.TextureCPU(nm)]


def _rot(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = math.radians(deg)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * k + (1 - math.cos(a)) * (k @ k)


ROOM, BLOB, QUAD_UV, TRI = range(4)


def layout(moved=False):
    """(mesh, material, local -> world 3 x 3, translation) per instance.  moved: the second set of transforms, for
    update_instances (every body shifted and turned; the room stays)."""
    out = [(ROOM, M_ROOM, np.eye(3), (0.0, 0.0, 0.0))]
    bodies = [M_GLOSSY, M_REFL_R, M_REFL_D, M_TRANSP_R, M_TRANSP_D, M_PBR, M_REFR_D, M_VOLUME, M_REFR_R, M_SUBSURF]
    rng = np.random.default_rng(11 if moved else 10)
    for k, mat in enumerate(bodies):
        x, z = -3.0 + 1.5 * (k % 5), -1.5 + 2.2 * (k // 5)
        sc = 0.7 if mat != M_VOLUME else 1.3
        out.append((BLOB, mat, X.rotation(rng) * sc, (x + (0.2 if moved else 0.0), -1.2 + 0.35 * (k % 3), z)))
    out.append((QUAD_UV, M_LIGHT_A, _rot((1, 0, 0), 90) * 0.8, (-1.5, 2.4, -0.5)))            # facing down
    out.append((QUAD_UV, M_LIGHT_TEX, _rot((1, 0, 0), 70) @ np.diag([0.9, 0.6, 1.0]), (2.0, 2.2, 0.5)))
    out.append((TRI, M_LIGHT_INST, _rot((0, 1, 0), 30) * 0.9, (-3.5, 0.8, -3.2)))
    out.append((TRI, M_LIGHT_INST, _rot((1, 1, 0), 50) @ np.diag([1.6, 0.5, 1.0]), (3.3, 0.5, -3.0)))   # non-uniform
    out.append((TRI, M_LIGHT_INF, _rot((0, 0, 1), 20) * 1.7, (1.0, 1.2, -4.2)))
    out.append((QUAD_UV, M_OPACITY, _rot((0, 1, 0), 15) * 1.2, (0.0, -0.3, 2.0)))
    out.append((QUAD_UV, M_NORMAL_MAP, _rot((1, 0, 0), -60) @ np.diag([1.5, 1.0, 1.0]), (0.5, -1.4, -3.0)))
    return out


def instance_records(moved=False):
    return np.array([api.instance_from_transform(X.mat3x4(M, b), mesh, mat) for mesh, mat, M, b in layout(moved)], INSTANCE_DTYPE)


def scene_cpu(variant):
    """variant: "const" (a constant environment), "textured" (a 6 x 3 textured one), "matte" (every body matte, the two plain
    emitters, the constant environment: the SIMPLE instantiation of the shade kernel).  About 400 triangles."""
    rng = np.random.default_rng(5)
    room_v = np.array([(x, y, z) for x in (-4.5, 4.5) for y in (-2.0, 3.0) for z in (-4.5, 4.5)], np.float64)
    faces = [(0, 1, 5, 4), (0, 2, 3, 1), (4, 5, 7, 6), (0, 4, 6, 2), (1, 3, 7, 5)]          # floor, four walls; open top
    room_i = np.array([(a, b, c, a, c, d) for a, b, c, d in faces], np.uint32).reshape(-1)
    blob_v, blob_i = X.blob_mesh(rng, 6, 4)
    sc = api.SceneCPU()
    for v, i in ((room_v, room_i), (blob_v[:, :3], blob_i), (X.QUAD[0][:, :3], X.QUAD[1]), (X.TRIANGLE[0][:, :3], X.TRIANGLE[1])):
        v4 = np.zeros((len(v), 4), np.float32)
        v4[:, :3] = v
        sc.verts_pos_array.append(v4)
        sc.indices_array.append(np.asarray(i, np.uint32).copy())
    sc.mesh_infos = np.array([api.default_mesh_info() for _ in range(4)], MESH_INFO_DTYPE)
    sc.mesh_infos[QUAD_UV]["texcoords_buf_idx"] = 0
    sc.verts_texcoord_array.append(np.array([(0.1, 0.1), (1.9, 0.2), (1.8, 1.7), (0.0, 1.6)], np.float32))   # wraps (Repeat)
    sc.materials = _materials(variant == "matte")
    sc.instances = instance_records()
    textures = _textures(rng)
    env = api.default_environment()
    env["emission"] = (0.6, 0.7, 0.9)
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = _rot((1, 2, 0.5), 40).T
    env["transform"] = m
    if variant == "textured":
        t4 = np.ones((3, 6, 4), np.float32)
        t4[..., :3] = rng.uniform(0.1, 1.0, (3, 6, 3)) * np.array([1.0, 3.0, 0.5])[:, None, None]
        env["emission_tex_idx"] = len(textures)
        textures.append(api.TextureCPU(t4.astype(np.float16)))
        infos = [api.EnvMapInfo(t4, 6, 3)]
    else:
        infos = [api.EnvMapInfo(np.ones((1, 1, 4), np.float32), 1, 1)]
    sc.environments = np.array([env], ENVIRONMENT_DTYPE)
    api.validate_scene(sc, len(textures), len(textures))
    return sc, textures, infos


CAMERA = api.CameraParams(lens=0.02, film=0.036, aspect=1.0)
CAM_W = CAM_H = 64


def camera_transform():
    """4 columns x 3 rows; the view direction is the camera's +z."""
    pos = np.array([0.3, 0.6, 4.0])
    z = np.array([-0.05, -0.25, -1.0])
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z, pos]).astype(np.float32)


def pcg_advance(state, draws):
    s = np.asarray(state, np.uint64)
    for _ in range(draws):
        s = (s * np.uint64(747796405) + np.uint64(2891336453)) & np.uint64(0xFFFFFFFF)
    return s.astype(np.uint32)


# ------------------------------------------------------------------------------------------------ surfaces, batched
class Surfaces:
    """surface_ref's scalar material point and shading normal over arrays of hits, cached where they cannot depend on the
    barycentrics (a mesh without texture coordinates, colours and normals)."""

    def __init__(self, cpu, textures, scene, g):
        idx = [reproject_ref.mesh_arrays(scene, i)[1] for i in range(scene.desc.num_meshes)]
        self.ref = surface_ref.SurfaceRef(cpu, textures, idx)
        self.cpu, self.g = cpu, g
        self.lookup = [{tuple(t): j for j, t in enumerate(m.tris.tolist())} for m in g.meshes]
        self.flat = [all(int(info[k]) == api.SENTINEL_IDX for k in ("normals_buf_idx", "texcoords_buf_idx", "colors_buf_idx"))
                     for info in cpu.mesh_infos]
        self.cache = {}
        self.env_textured = any(int(e["emission_tex_idx"]) != api.SENTINEL_IDX for e in cpu.environments)

    def tri_index(self, inst, triple):
        return np.array([self.lookup[self.g.mesh_idx[i]][tuple(t)] for i, t in zip(inst.tolist(), triple.tolist())], np.int64).reshape(-1)

    def _one(self, inst, tri, u, v):
        flat = self.flat[int(self.cpu.instances[inst]["mesh_idx"])]
        key = (inst, tri) if flat else (inst, tri, u, v)
        if key not in self.cache:
            val, _, ex1 = self.ref.material_point(inst, tri, u, v)
            n, _, ex2 = self.ref.shading_normal(inst, tri, u, v)
            self.cache[key] = (val["type"], val["color"], val["opacity"], val["emission"], val["roughness"], val["metallic"], val["ior"],
                               val["density"], val["scattering"], val["anisotropy"], n, bool(ex1 or ex2))
            if not flat and len(self.cache) > 400000:
                self.cache.clear()
        return self.cache[key]

    def points(self, inst, tri, u, v):
        rows = [self._one(int(i), int(t), float(a), float(b)) for i, t, a, b in zip(inst, tri, u, v)]
        n = len(rows)
        col = lambda k, shape: np.array([r[k] for r in rows], np.float64).reshape((n,) + shape)
        return dict(type=np.array([r[0] for r in rows], np.int64), color=col(1, (3,)), opacity=col(2, ()), emission=col(3, (3,)),
                    rough=col(4, ()), metal=col(5, ()), ior=col(6, ()), density=col(7, (3,)), scattering=col(8, (3,)), g=col(9, ()),
                    normal=col(10, (3,)), excluded=np.array([r[11] for r in rows], bool))

    def environment(self, d):
        """sample_environments per direction, and whether the lookup is well conditioned."""
        d = np.asarray(d, np.float64).reshape(-1, 3)
        if not self.env_textured:
            e = np.sum([np.asarray(env["emission"], np.float64)[:3] for env in self.cpu.environments], axis=0) if len(self.cpu.environments) else np.zeros(3)
            return np.broadcast_to(e, d.shape).copy(), np.ones(len(d), bool)
        out, ok = np.zeros_like(d), np.ones(len(d), bool)
        for k in range(len(d)):
            val, _, _, _, ex = self.ref.environment_radiance(d[k].tolist())
            out[k], ok[k] = val, not ex
        return out, ok


def _mat(P, sel=None):
    t = (lambda a: a) if sel is None else (lambda a: a[sel])
    return S.Mat(t(P["type"]), t(P["color"]), t(P["rough"]), t(P["metal"]), t(P["ior"]), t(P["density"]), t(P["scattering"]), t(P["g"]))


# ------------------------------------------------------------------------------------------------ a case
@dataclass
class Case:
    variant: str
    cpu: object
    textures: list
    infos: list
    scene: object          # built on the host: what the oracle traces
    g: object
    surf: Surfaces
    lights: object
    ori: np.ndarray        # (4096, 3) f32: the camera's rays
    dir: np.ndarray
    word: np.ndarray       # (4096,) u32
    moved: bool = False
    traces: dict = field(default_factory=dict)


_cases = {}


def make_case(variant, scene=None, moved=False):
    """The Case of a scene variant.  scene: an api.Scene to read instead of building one on the host (after
    update_instances); moved: the second set of transforms."""
    from oracle import oracle
    cpu, textures, infos = scene_cpu(variant)
    if moved:
        cpu.instances = instance_records(True)
    host = scene if scene is not None else api.build_accel_structures_and_upload(None, cpu, textures, infos, True)
    g = X.geometry(host)
    order = [reproject_ref.mesh_arrays(host, i)[1] for i in range(host.desc.num_meshes)]
    lights = L.build(cpu, infos, order)
    L.attach_tables(lights, host.alias_tables, host.env_alias_tables)
    ori, d = oracle.camera_rays(host, CAM_W, CAM_H, CAMERA, camera_transform(), 0)
    word = pcg_advance(api.rng_seed_for(np.arange(CAM_W * CAM_H, dtype=np.uint32), 0), 4)
    return Case(variant, cpu, textures, infos, host, g, Surfaces(cpu, textures, host, g), lights, ori.reshape(-1, 3), d.reshape(-1, 3), word, moved)


def case(variant):
    if variant not in _cases:
        _cases[variant] = {"furnace": furnace_case, "emitter": emitter_case}.get(variant, lambda: make_case(variant))()
    return _cases[variant]


def custom_case(name, cpu, textures, infos, ori, dir_, word):
    """A Case of any scene with records of the caller's own."""
    host = api.build_accel_structures_and_upload(None, cpu, textures, infos, True)
    g = X.geometry(host)
    order = [reproject_ref.mesh_arrays(host, i)[1] for i in range(host.desc.num_meshes)]
    lights = L.build(cpu, infos, order)
    L.attach_tables(lights, host.alias_tables, host.env_alias_tables)
    return Case(name, cpu, textures, infos, host, g, Surfaces(cpu, textures, host, g), lights, np.asarray(ori, np.float32),
                np.asarray(dir_, np.float32), np.asarray(word, np.uint32))


def _plain_scene(meshes, materials, instances, env_emission=None):
    sc = api.SceneCPU()
    for v, i in meshes:
        v4 = np.zeros((len(v), 4), np.float32)
        v4[:, :3] = v
        sc.verts_pos_array.append(v4)
        sc.indices_array.append(np.asarray(i, np.uint32).reshape(-1).copy())
    sc.mesh_infos = np.array([api.default_mesh_info() for _ in meshes], MESH_INFO_DTYPE)
    sc.materials = materials
    sc.instances = np.array([api.instance_from_transform(X.mat3x4(M, b), mesh, mat) for mesh, mat, M, b in instances], INSTANCE_DTYPE)
    infos = []
    if env_emission is not None:
        env = api.default_environment()
        env["emission"] = env_emission
        sc.environments = np.array([env], ENVIRONMENT_DTYPE)
        infos = [api.EnvMapInfo(np.ones((1, 1, 4), np.float32), 1, 1)]
    api.validate_scene(sc, 0, 0)
    return sc, [], infos


FURNACE_E = 0.5
FURNACE_N = 2048


def furnace_case():
    """A white furnace: a matte quad of albedo 1 and a smooth thin transparent quad of colour 1, side by side in the plane
    z = 0, inside a constant environment of radiance FURNACE_E.  Records 0 .. FURNACE_N - 1 are aimed at the matte quad from
    z > 0, the rest at the transparent one.  No cosine sample of a plane meets the scene again, so the closed forms hold per
    path or in the mean without a truncation bias."""
    m = np.array([api.default_material(), api.default_material()], MATERIAL_DTYPE)
    m[0]["mat_type"], m[0]["color"], m[0]["roughness"] = int(api.MaterialType.Matte), (1.0, 1.0, 1.0, 1.0), 1.0
    m[1]["mat_type"], m[1]["color"], m[1]["roughness"] = int(api.MaterialType.Transparent), (1.0, 1.0, 1.0, 1.0), 0.0
    cpu, tex, infos = _plain_scene([(X.QUAD[0][:, :3], X.QUAD[1])], m, [(0, 0, np.eye(3), (-1.5, 0.0, 0.0)), (0, 1, np.eye(3), (1.5, 0.0, 0.0))],
                                   (FURNACE_E,) * 3)
    rng = np.random.default_rng(21)
    n = 2 * FURNACE_N
    target = np.concatenate([rng.uniform(-0.9, 0.9, (n, 2)), np.zeros((n, 1))], 1)
    target[:, 0] += np.where(np.arange(n) < FURNACE_N, -1.5, 1.5)
    ori = target + X._unit(rng, n) * np.array([1.0, 1.0, 0.0]) + np.array([0.0, 0.0, 1.0]) * rng.uniform(0.5, 2.0, (n, 1))
    d = target - ori
    return custom_case("furnace", cpu, tex, infos, ori, d / np.linalg.norm(d, axis=1, keepdims=True), camera_ref.hash_u32(np.arange(n) + 77))


EMITTER_L, EMITTER_ALBEDO = 3.0, 0.8
EMITTER_POINTS = ((0.3, 0.0, -0.2), (1.4, 0.0, 1.1))
EMITTER_N = 3000


def emitter_case():
    """A matte floor of albedo EMITTER_ALBEDO (y = 0, [-2, 2]^2) under a square emitter of radiance EMITTER_L ([-1, 1]^2 in
    the plane y = 1, albedo 0), no environment: the radiance leaving the floor at p is albedo x L x form_factor(p), for every
    integrator (without an environment the MIS double count does not act).  EMITTER_N records per point of EMITTER_POINTS,
    from below the emitter straight at p."""
    m = np.array([api.default_material(), api.default_material()], MATERIAL_DTYPE)
    m[0]["mat_type"], m[0]["color"], m[0]["roughness"] = int(api.MaterialType.Matte), (EMITTER_ALBEDO,) * 3 + (1.0,), 1.0
    m[1]["mat_type"], m[1]["color"], m[1]["roughness"] = int(api.MaterialType.Matte), (0.0, 0.0, 0.0, 1.0), 1.0
    m[1]["emission"] = (EMITTER_L, EMITTER_L, EMITTER_L, 0.0)
    floor = (np.array([(-2, 0, -2), (-2, 0, 2), (2, 0, 2), (2, 0, -2)], np.float64), [(0, 1, 2), (0, 2, 3)])
    light = (np.array([(-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1)], np.float64), [(0, 2, 1), (2, 0, 3)])
    cpu, tex, infos = _plain_scene([floor, light], m, [(0, 0, np.eye(3), (0.0, 0.0, 0.0)), (1, 1, np.eye(3), (0.0, 0.0, 0.0))])
    n = EMITTER_N * len(EMITTER_POINTS)
    p = np.repeat(np.array(EMITTER_POINTS), EMITTER_N, 0)
    ori = p + np.array([0.05, 0.5, -0.03])
    d = p - ori
    return custom_case("emitter", cpu, tex, infos, ori, d / np.linalg.norm(d, axis=1, keepdims=True), camera_ref.hash_u32(np.arange(n) + 991))


def records(c, sel=slice(None)):
    return api.ray_records(c.ori[sel], c.dir[sel], c.word[sel], api.RayMode.DIRECTION)


# ------------------------------------------------------------------------------------------------ the loops
@dataclass
class Trace:
    integ: int
    defect: object
    log: list              # per vertex b: dict of (N, ...) arrays: kind, end, weight, radiance, rng, in_medium, shadow, skips,
    #                        decisive (cumulative), roulette_survived (cumulative)
    reason: np.ndarray     # (N,) object: the first decision that was not clear, "" if none

    def vertex(self, max_bounces):
        b = max_bounces - 1 if self.defect == "loop_ends_before_max" else max_bounces
        return self.log[min(b, len(self.log) - 1)] if b >= 0 else None

    def at(self, max_bounces, max_radiance=NO_CLAMP):
        """(clamped radiance, unclamped radiance, decisive) of the query with this max_bounces: the prefix property."""
        e = self.vertex(max_bounces)
        if e is None:
            z = np.zeros_like(self.log[0]["radiance"])
            return z, z, np.ones(len(z), bool)
        raw = e["radiance"]
        return clamp_radiance(raw, max_radiance, self.defect == "clamp_per_channel"), raw, e["decisive"]


def clamp_radiance(rad, max_radiance, per_channel=False):
    res = np.where(np.isfinite(rad).all(-1, keepdims=True), rad, 0.0)
    if per_channel:
        return np.minimum(res, max_radiance)
    big = res.max(-1, keepdims=True)
    with np.errstate(all="ignore"):
        return np.where(big > max_radiance, res * (max_radiance / big), res)


def clamp_branch(rad, max_radiance):
    """0 = untouched, 1 = non-finite set to zero, 2 = scaled by the largest channel."""
    nf = ~np.isfinite(rad).all(-1)
    return np.where(nf, 1, np.where(np.where(nf[:, None], 0.0, rad).max(-1) > max_radiance, 2, 0))


def trace(c, integ, max_bounces=LADDER[-1], sel=slice(None), word=None, defect=None, eps=EPS):
    """Every path of the records `sel` of Case c, to max_bounces, in float64.  word: other RNG words for the same rays."""
    assert defect is None or defect in DEFECTS
    integ = int(integ)
    o = np.array(c.ori[sel], np.float64)
    d = np.array(c.dir[sel], np.float64)
    N = len(o)
    rng = np.asarray(c.word[sel] if word is None else word, np.uint64).copy()
    w, rad = np.ones((N, 3)), np.zeros((N, 3))
    alive = np.ones(N, bool)
    dec = np.ones(N, bool)
    reason = np.full(N, "", object)
    vol_len = np.zeros(N, np.int64)
    vol_d, vol_s, vol_g = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros(N)
    next_em = np.ones(N, bool)
    nh = dict(hit=np.zeros(N, bool), inst=np.zeros(N, np.int64), tri=np.zeros(N, np.int64), t=np.zeros(N), u=np.zeros(N), v=np.zeros(N))
    cur = {k: a.copy() for k, a in nh.items()}
    survived = np.zeros(N, bool)
    surf, g, lights = c.surf, c.g, c.lights
    roulette_from = {"roulette_from_2": 2, "roulette_from_4": 4}.get(defect, 3)
    log = []

    def unclear(idx, bad, why):
        hit = idx[bad]
        first = hit[dec[hit]]
        reason[first] = why
        dec[hit] = False

    def draw(idx):
        s, r = camera_ref.random_f32(rng[idx])
        rng[idx] = s
        return r

    def closest(idx, org, dr, why):
        H = X.closest_hits(g, org, dr, eps, s=S_PATH)
        unclear(idx, ~H.decisive, why)
        tri = np.zeros(len(idx), np.int64)
        if H.hit.any():
            tri[H.hit] = surf.tri_index(H.inst[H.hit], H.tri[H.hit])
        return H, tri

    def continuation(idx):
        """ray_skip_alpha_stochastically: the hit of cur[...] for the paths idx, and the skips taken."""
        org, dr = o[idx].copy(), d[idx]
        dst, skips = np.zeros(len(idx)), np.zeros(len(idx), np.int64)
        pend = np.arange(len(idx))
        cur["hit"][idx] = False
        for _ in range(128):
            if not len(pend):
                break
            H, tri = closest(idx[pend], org[pend], dr[pend], "closest hit")
            hp = pend[H.hit]
            if not len(hp):
                break
            Hh, trih = H.take(H.hit), tri[H.hit]
            P = surf.points(Hh.inst, trih, Hh.u, Hh.v)
            unclear(idx[hp], P["excluded"], "material point")
            dst[hp] += Hh.t
            op = P["opacity"]
            coin = (op < 1.0) | (defect == "opacity_coin_always")
            r = np.zeros(len(hp))
            r[coin] = draw(idx[hp[coin]])
            skip = (op < 1.0) & coin & (r >= op)
            unclear(idx[hp], (op < 1.0) & (np.abs(r - op) < REL), "opacity coin")
            fin = hp[~skip]
            gi = idx[fin]
            cur["hit"][gi], cur["inst"][gi], cur["tri"][gi] = True, Hh.inst[~skip], trih[~skip]
            cur["t"][gi], cur["u"][gi], cur["v"][gi] = dst[fin], Hh.u[~skip], Hh.v[~skip]
            org[hp[skip]] += dr[hp[skip]] * Hh.t[skip][:, None]
            skips[hp[skip]] += 1
            pend = hp[skip]
        return skips

    def light_sample(idx, pos):
        dr, s, margin = L.sample(lights, pos, rng[idx])
        rng[idx] = s
        unclear(idx, margin <= 1.0, "light pick")
        return dr

    def light_pdf(idx, pos, inc):
        out = np.zeros(len(idx))
        nz = np.any(inc != 0.0, -1)
        if nz.any():
            r = L.pdf(lights, pos[nz], inc[nz], eps)
            out[nz] = r.pdf
            unclear(idx[nz], ~((r.edge_margin >= EDGE) & (r.eps_margin >= EPS_REL) & (r.min_cos >= MIN_COS) & (r.texel_margin >= TEXEL)),
                    "light pdf crossing")
        return out

    def side_clear(idx, n, a, b, why):
        unclear(idx, (np.abs(S.dot(n, a)) < SIGN) | (np.any(b != 0, -1) & (np.abs(S.dot(n, b)) < SIGN)), why)

    def bsdf_sample(idx, m, n, out):
        rnl, r0, r1 = draw(idx), draw(idx), draw(idx)
        inc, info = S.bsdf_sample(m, n, out, rnl, r0, r1)
        with np.errstate(invalid="ignore"):
            unclear(idx, np.isfinite(info["fresnel"]) & (np.abs(rnl - info["fresnel"]) < REL), "lobe pick")
            unclear(idx, np.isfinite(info["k"]) & (np.abs(info["k"]) < REL), "total internal reflection")
        return inc

    def emission_along(idx, pos, inc):
        """The emission a shadow ray meets (no opacity pass-through), and the hit itself."""
        H, tri = closest(idx, pos, inc, "shadow ray")
        em = np.zeros((len(idx), 3))
        if H.hit.any():
            P = surf.points(H.inst[H.hit], tri[H.hit], H.u[H.hit], H.v[H.hit])
            unclear(idx[H.hit], P["excluded"], "material point")
            em[H.hit] = P["emission"]
        if (~H.hit).any():
            e, ok = surf.environment(inc[~H.hit])
            em[~H.hit] = e
            unclear(idx[~H.hit], ~ok, "environment lookup")
        return em, H, tri

    for b in range(max_bounces + 1):
        kind, end = np.zeros(N, np.int8), np.zeros(N, np.int8)
        shadow, skips = np.zeros((N, 3)), np.zeros(N, np.int64)
        a = np.nonzero(alive)[0]
        # ---- the hit
        fresh = next_em[a] if integ == PT.MIS else np.ones(len(a), bool)
        if fresh.any():
            skips[a[fresh]] = continuation(a[fresh])
        st = a[~fresh]
        for k in cur:
            cur[k][st] = nh[k][st]                                                  # Q2: whatever was stored last
        miss = ~cur["hit"][a]
        m = a[miss]
        if len(m):
            e, ok = surf.environment(d[m])
            unclear(m, ~ok, "environment lookup")
            if integ == PT.Direct:
                e = np.where(next_em[m][:, None], e, 0.0)                                         # Q6
            rad[m] += w[m] * e
            kind[m], alive[m] = MISS, False
        a = a[~miss]
        # ---- transmission inside a volume
        hd = cur["t"][a]
        vd = hd.copy()
        inmed = vol_len[a] > 0
        am = a[inmed]
        if len(am):
            rl, rd = draw(am), draw(am)
            dens = vol_d[am]
            unclear(am, np.abs(rl * 3.0 - np.round(rl * 3.0)) < 3.0 * PICK, "channel pick")
            ch = np.clip(np.trunc(rl * 3.0).astype(np.int64), 0, 2)
            dc = dens[np.arange(len(am)), ch]
            with np.errstate(divide="ignore"):
                free = np.where(dc == 0.0, F32_MAX, -np.log1p(-rd) / dc)
            unclear(am, np.abs(free - hd[inmed]) < REL * hd[inmed], "volume_dst against hit_dst")
            dist = np.minimum(free, hd[inmed])
            if defect != "no_tr_over_tp":
                w[am] *= S.medium_transmittance(dens, dist) / S.medium_distance_pdf(dens, dist, hd[inmed])[:, None]
            vd[inmed] = dist
        in_volume = vd < hd
        # ---- a surface
        s = a[~in_volume]
        if len(s):
            pos, out = o[s] + d[s] * cur["t"][s][:, None], -d[s]
            P = surf.points(cur["inst"][s], cur["tri"][s], cur["u"][s], cur["v"][s])
            unclear(s, P["excluded"], "material point")
            n = P["normal"]
            mat = _mat(P)
            gate = np.ones(len(s), bool)
            if integ in (PT.MIS, PT.Direct) and not (integ == PT.Direct and defect == "direct_emission_always"):
                gate = next_em[s]
            rad[s] += np.where(gate[:, None], w[s] * P["emission"], 0.0)              # (an infinite emission behind a closed gate adds nothing)
            delta = S.is_delta(mat)
            inc = np.zeros((len(s), 3))
            stop = np.zeros(len(s), bool)
            nd = np.nonzero(~delta)[0]
            if len(nd):
                sn, mn, nn, on, pn = s[nd], _mat(P, nd), n[nd], out[nd], pos[nd]
                if integ == PT.Direct:
                    li = light_sample(sn, pn)
                    lp = light_pdf(sn, pn, li)
                    side_clear(sn, nn, on, li, "side of the normal")
                    bc = S.bsdf_eval(mn, nn, on, li)
                    ok = np.all(bc != 0.0, -1) & (lp > 0.0)
                    if ok.any():
                        em, _, _ = emission_along(sn[ok], pn[ok], li[ok])
                        term = w[sn[ok]] * bc[ok] * em / lp[ok][:, None]
                        rad[sn[ok]] += term
                        shadow[sn[ok]] += term
                if integ == PT.MIS:
                    bi = bsdf_sample(sn, mn, nn, on)
                    zero = np.all(bi == 0.0, -1)                                    # Q3
                    for turn in (0, 1):
                        go = np.nonzero(~zero)[0]
                        if not len(go):
                            break
                        gi = sn[go]
                        mi = bi[go] if turn == 0 else light_sample(gi, pn[go])
                        z2 = np.all(mi == 0.0, -1)
                        go, gi, mi = go[~z2], gi[~z2], mi[~z2]
                        mg = _mat(P, nd[go])
                        side_clear(gi, nn[go], on[go], mi, "side of the normal")
                        bc = S.bsdf_eval(mg, nn[go], on[go], mi)
                        lp = light_pdf(gi, pn[go], mi)
                        bp = S.bsdf_pdf(mg, nn[go], on[go], mi)
                        this, other = (bp, lp) if turn == 0 else (lp, bp)
                        with np.errstate(all="ignore"):
                            if defect == "balance_heuristic":
                                mw = this / (this + other)
                            else:
                                mw = this * this / (this * this + other * other)
                            if defect != "mis_no_pdf_divide":
                                mw = mw / this
                        unclear(gi, ~np.isfinite(mw), "mis weight")
                        ok = np.all(bc != 0.0, -1) & (mw != 0.0)
                        if ok.any():
                            em, H, tri = emission_along(gi[ok], pn[go][ok], mi[ok])
                            if turn == 0:
                                q = gi[ok]
                                nh["hit"][q], nh["inst"][q], nh["tri"][q] = H.hit, H.inst, tri
                                nh["t"][q], nh["u"][q], nh["v"][q] = H.t, H.u, H.v
                            term = w[gi[ok]] * bc[ok] * em * mw[ok][:, None]
                            rad[gi[ok]] += term
                            shadow[gi[ok]] += term
                    inc[nd] = bi
                    with np.errstate(all="ignore"):
                        w[sn] *= S.bsdf_eval(mn, nn, on, bi) / S.bsdf_pdf(mn, nn, on, bi)[:, None]
                    next_em[sn] = defect == "mis_keeps_next_emission"
                    kind[sn] = SURF_BSDF
                elif integ == PT.Naive:
                    bi = bsdf_sample(sn, mn, nn, on)
                    inc[nd] = bi
                    z = np.all(bi == 0.0, -1)
                    stop[nd[z]] = True
                    with np.errstate(all="ignore"):
                        w[sn[~z]] *= (S.bsdf_eval(mn, nn, on, bi) / S.bsdf_pdf(mn, nn, on, bi)[:, None])[~z]
                    kind[sn] = SURF_BSDF
                else:
                    turn_b = draw(sn) < 0.5
                    bi = np.zeros((len(sn), 3))
                    if turn_b.any():
                        bi[turn_b] = bsdf_sample(sn[turn_b], _mat(P, nd[turn_b]), nn[turn_b], on[turn_b])
                    if (~turn_b).any():
                        bi[~turn_b] = light_sample(sn[~turn_b], pn[~turn_b])
                    inc[nd] = bi
                    z = np.all(bi == 0.0, -1)
                    stop[nd[z]] = True
                    k2 = ~z
                    bp, lp = S.bsdf_pdf(mn, nn, on, bi), light_pdf(sn, pn, np.where(k2[:, None], bi, 0.0))
                    prob = (0.5 * bp + lp) if defect == "mixture_half_bsdf_only" else (0.5 * bp + 0.5 * lp)
                    with np.errstate(all="ignore"):
                        w[sn[k2]] *= (S.bsdf_eval(mn, nn, on, bi) / prob[:, None])[k2]
                    kind[sn] = np.where(turn_b, SURF_BSDF, SURF_LIGHT)
                    if integ == PT.Direct:
                        next_em[sn] = defect == "direct_keeps_next_emission"
            dl = np.nonzero(delta)[0]
            if len(dl):
                sd, md = s[dl], _mat(P, dl)
                rn = draw(sd)
                di, info = S.delta_sample(md, n[dl], out[dl], rn)
                with np.errstate(invalid="ignore"):
                    unclear(sd, np.isfinite(info["fresnel"]) & (np.abs(rn - info["fresnel"]) < REL), "lobe pick")
                inc[dl] = di
                z = np.all(di == 0.0, -1)
                stop[dl[z]] = True
                with np.errstate(all="ignore"):
                    w[sd[~z]] *= (S.delta_eval(md, n[dl], out[dl], di) / S.delta_pdf(md, n[dl], out[dl], di)[:, None])[~z]
                next_em[sd] = True
                kind[sd] = DELTA
            side_clear(s, n, out, inc, "side of the normal")
            end[s[stop]], alive[s[stop]] = END_ZERO_INCOMING, False
            # update_volume_stack
            cross = np.isin(P["type"], [S.REFRACTIVE, S.VOLUMETRIC, S.SUBSURFACE]) & (S.dot(n, out) * S.dot(n, inc) < 0.0) & ~stop
            push = cross & ((vol_len[s] == 0) | (defect == "medium_pushed_not_popped"))
            pop = cross & ~push
            vol_d[s[push]], vol_s[s[push]], vol_g[s[push]] = P["density"][push], P["scattering"][push], P["g"][push]
            vol_len[s[push]] = 1                                                    # Q4
            vol_len[s[pop]] -= 1
            o[s], d[s] = pos, inc
        # ---- inside the medium
        v = a[in_volume]
        if len(v):
            pos, out = o[v] + d[v] * vd[in_volume][:, None], -d[v]
            vm = S.Mat(np.full(len(v), S.VOLUMETRIC), np.zeros((len(v), 3)), np.zeros(len(v)), np.zeros(len(v)), np.ones(len(v)),
                       vol_d[v], vol_s[v], vol_g[v])
            sc = np.ones(len(v), bool) if integ == PT.Naive else draw(v) < 0.5
            inc = np.zeros((len(v), 3))
            if sc.any():
                q = v[sc]
                if defect != "medium_draw_kept":
                    draw(q)                                                         # Q5
                r0, r1 = draw(q), draw(q)
                inc[sc] = S.phase_sample(S.Mat(vm.type[sc], vm.color[sc], vm.rough[sc], vm.metal[sc], vm.ior[sc], vm.density[sc],
                                               vm.scattering[sc], vm.g[sc]), out[sc], r0, r1)
            if (~sc).any():
                inc[~sc] = light_sample(v[~sc], pos[~sc])
            if integ == PT.MIS:
                next_em[v] = True
            z = np.all(inc == 0.0, -1)
            pp = S.phase_pdf(vm, out, inc)
            prob = pp if integ == PT.Naive else 0.5 * pp + 0.5 * light_pdf(v, pos, np.where(z[:, None], 0.0, inc))
            with np.errstate(all="ignore"):
                w[v[~z]] *= (S.phase_eval(vm, out, inc) / prob[:, None])[~z]
            kind[v] = MEDIUM
            end[v[z]], alive[v[z]] = END_ZERO_INCOMING, False
            o[v], d[v] = pos, inc
        # ---- the weight, roulette
        a = a[alive[a]]
        dead = np.all(w[a] == 0.0, -1) | ~np.isfinite(w[a]).all(-1)
        end[a[dead]], alive[a[dead]] = END_WEIGHT, False
        a = a[~dead]
        if b > roulette_from and len(a):
            surv = np.minimum(1.0 if defect == "survive_cap_1" else float(np.float32(0.99)), w[a].max(-1))
            r = draw(a)
            unclear(a, np.abs(r - surv) < REL, "roulette")
            out_ = r >= surv
            end[a[out_]], alive[a[out_]] = END_ROULETTE, False
            k = a[~out_]
            if defect != "no_survive_divide":
                w[k] *= (1.0 / surv[~out_])[:, None]
            survived[k] = True
        log.append(dict(kind=kind, end=end, weight=w.copy(), radiance=rad.copy(), rng=rng.astype(np.uint32), in_medium=vol_len > 0,
                        shadow=shadow, skips=skips, decisive=dec.copy(), roulette_survived=survived.copy(), reason=reason.copy()))
    return Trace(integ, defect, log, reason)


def cached_trace(c, integ):
    if int(integ) not in c.traces:
        c.traces[int(integ)] = trace(c, integ)
    return c.traces[int(integ)]


# ------------------------------------------------------------------------------------------------ the comparison
FLOOR = 1e-2                 # radiance floor of the relative metric: the environments here emit 0.1 .. 3, the meshes 3 .. 9
MAX_EXCLUDED = 0.25


def deviation(got, ref):
    """|got - ref|_inf / (|ref|_inf + FLOOR) per path; a non-finite `got` counts as infinite."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(all="ignore"):
        e = np.abs(got - ref).max(-1) / (np.abs(ref).max(-1) + FLOOR)
    return np.where(np.isfinite(got).all(-1), e, np.inf)


# MEASURED: the oracle (f32, the device's arithmetic by DESIGN.md 3) against trace(), on the 4096 camera records of the
# "const" and "textured" scenes, over the decisive paths, worst of unclamped and clamped radiance and of the two scenes, per
# integrator and rung.  Measured on a CPU with tests/test_path_cpu.py::test_measured_deviation_is_the_recorded_one; not
# measured on an MI355X: the device is tied to the oracle word for word elsewhere (tests/test_gpu_ray_query.py).
# BOUND is 4 x MEASURED (DESIGN.md 17's factor for K_BOUND, for the same reason).
MEASURED = {
    "Standard": {0: 2.679e-06, 1: 1.296e-05, 2: 2.022e-05, 4: 2.310e-05, 8: 3.203e-05},
    "MIS": {0: 3.033e-05, 1: 1.971e-05, 2: 1.971e-05, 4: 1.533e-05, 8: 4.722e-05},
    "Naive": {0: 2.679e-06, 1: 4.683e-06, 2: 2.425e-05, 4: 1.495e-04, 8: 1.495e-04},
    "Direct": {0: 2.805e-05, 1: 2.805e-05, 2: 2.805e-05, 4: 2.805e-05, 8: 2.805e-05},
}
BOUND_FACTOR = 4.0


def bound(integ, rung):
    return BOUND_FACTOR * MEASURED[PT(int(integ)).name][rung]


def failures(tr, got, rung, max_radiance=NO_CLAMP, tol=None, names=None):
    """The records whose decisive reference answer `got` (n, 3) misses by more than the bound, as messages."""
    clamped, raw, dec = tr.at(rung, max_radiance)
    tol = bound(tr.integ, rung) if tol is None else tol
    dev = deviation(np.asarray(got)[:, :3], clamped)
    bad = np.nonzero(dec & ~(dev <= tol))[0]
    out = []
    for r in bad[:8]:
        e = tr.vertex(rung) or tr.log[0]
        out.append(f"record {names[r] if names is not None else r}, {PT(tr.integ).name}, max_bounces {rung}: got {np.asarray(got)[r, :3]}, float64 "
                   f"{clamped[r]} (deviation {dev[r]:.3e} > {tol:.3e}); vertex {min(rung, len(tr.log) - 1)}: {KIND_NAMES[e['kind'][r]]}, "
                   f"{END_NAMES[e['end'][r]]}, weight {e['weight'][r]}, radiance {e['radiance'][r]}, shadow {e['shadow'][r]}, "
                   f"in medium {bool(e['in_medium'][r])}, rng {int(e['rng'][r]):#010x}")
    if len(bad) > 8:
        out.append(f"... and {len(bad) - 8} more")
    return out


def first_failing_rung(tr, got_by_rung, max_radiance=NO_CLAMP):
    """failures() of the first rung of LADDER that has any: (rung, messages) or None."""
    for rung in LADDER:
        if rung in got_by_rung:
            f = failures(tr, got_by_rung[rung], rung, max_radiance)
            if f:
                return rung, f
    return None


def conditions(tr, max_radiance_clamp=CLAMP):
    """The counts section 2 asks for, from the reference alone."""
    out = dict(excluded={}, kinds={}, ends={})
    for rung in LADDER:
        out["excluded"][rung] = float(1.0 - tr.vertex(rung)["decisive"].mean())
    last = tr.log[-1]["decisive"]
    kinds = np.stack([e["kind"] for e in tr.log], 1)
    ends = np.stack([e["end"] for e in tr.log], 1)
    for k in range(1, 6):
        out["kinds"][KIND_NAMES[k]] = int(((kinds == k).any(1) & last).sum())
    for k in range(1, 3):
        out["ends"][END_NAMES[k]] = int(((ends == k).any(1) & last).sum())
    out["opacity skip"] = int(((np.stack([e["skips"] for e in tr.log], 1) > 0).any(1) & last).sum())
    out["roulette survived"] = int((tr.log[-1]["roulette_survived"] & last).sum())
    _, raw, dec = tr.at(LADDER[-1])
    br = clamp_branch(raw, max_radiance_clamp)
    out["clamped"] = int(((br != 0) & dec).sum())
    out["clamp non-finite"] = int(((br == 1) & dec).sum())
    out["clamp scaled"] = int(((br == 2) & dec).sum())
    return out
