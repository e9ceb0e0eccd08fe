"""Light sampling on its own: sample_lights and sample_lights_pdf through lupin_hip_light_probe / oracle_light_probe.

CPU: the oracle against the float64 restatement in light_ref.py -- the pdf point by point, the samples against the float64
*true* density by chi-square, E[1 / pdf] against the solid angle of the support, the environment maps as maps and as
distributions, and the reference properties pinned ("Light sampling on its own").
GPU: the device bit-identical to the oracle on every output word, the RNG state included: the CPU query sets through both
geometry accessors, the cull set (1 .. 257 lights, rays aimed at the bounding spheres), the same after update_instances.

Record layout: lupin_hip_light_probe in include/lupin_hip.h."""
import math
import os

import numpy as np
import pytest

from lupinpathtracer_amd import api, loader
from lupinpathtracer_amd._abi import ENVIRONMENT_DTYPE, INSTANCE_DTYPE, MATERIAL_DTYPE, MESH_INFO_DTYPE
from tests import light_ref as L
from tests import util
from tests.stats import NC, NPHI, chi2_pooled, sphere_bin, sphere_quadrature

EPS = 1e-3
# A query is ill-conditioned, by the float64 reference alone, when a crossing lies within EDGE (barycentric) of a triangle
# edge, an accept / reject decision of the march within EPS_REL (relative) of the ray epsilon, a counted crossing has
# |cos| below MIN_COS, or the direction lies within TEXEL (texels) of a texel border of a textured environment.
EDGE, EPS_REL, MIN_COS, TEXEL = 1e-4, 1e-4, 1e-2, 1e-3
MAX_EXCLUDED = 0.02
# Largest oracle-to-float64 relative error measured over the kept queries of the scenes below: 3.9e-5 ("instances": the
# sheared and scaled emitters; quads 4e-6, box 7e-6, bunny 1.6e-5, environments 5e-7).  The bound is that times the margin of
# 4: a maximum over a finite sample of float32 roundings.  The device must equal the oracle exactly, so it inherits the bound.
PDF_RTOL = 1.6e-4


# ---- scenes -----------------------------------------------------------------------------------------------------------

def quad(w=1.0, h=1.0):
    return np.array([(-w, 0, -h), (w, 0, -h), (w, 0, h), (-w, 0, h)], np.float64), np.array([0, 1, 2, 2, 3, 0], np.uint32)


def disc(n=24, r=1.0):
    a = np.arange(n) * 2 * math.pi / n
    v = np.vstack([[0, 0, 0], np.stack([r * np.cos(a), 0 * a, r * np.sin(a)], -1)])
    idx = np.array([(0, 1 + k, 1 + (k + 1) % n) for k in range(n)], np.uint32).reshape(-1)
    return v, idx


def box(sx, sy, sz):
    v = np.array([(x, y, z) for x in (-sx, sx) for y in (-sy, sy) for z in (-sz, sz)], np.float64)
    f = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = np.array([(a, b, c, a, c, d) for a, b, c, d in f], np.uint32).reshape(-1)
    return v, idx


def rot(axis, deg):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    a = math.radians(deg)
    k = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(a) * k + (1 - math.cos(a)) * (k @ k)


SHEAR = np.array([[1.0, 0.6, 0.0], [0.0, 1.0, 0.0], [0.3, 0.0, 1.2]])
MIRROR = np.diag([-1.0, 1.0, 1.0])


class Spec:
    """Meshes, instances (mesh, 3x3 linear part, translation, emissive) and environments of a test scene."""

    def __init__(self):
        self.meshes, self.instances, self.envs = [], [], []

    def mesh(self, verts, idx):
        self.meshes.append((np.asarray(verts, np.float64), np.asarray(idx, np.uint32)))
        return len(self.meshes) - 1

    def inst(self, mesh, a=np.eye(3), t=(0, 0, 0), emissive=True):
        self.instances.append((mesh, np.asarray(a, np.float64), np.asarray(t, np.float64), emissive))
        return self

    def env(self, a=np.eye(3), emission=(1, 1, 1), tex=None):
        self.envs.append((np.asarray(a, np.float64), emission, tex))
        return self

    def scene_cpu(self):
        s = api.SceneCPU()
        dark, lit = api.default_material(), api.default_material()
        dark["color"] = (0.5, 0.5, 0.5, 1.0)
        lit["emission"] = (5.0, 4.0, 3.0, 0.0)
        s.materials = np.array([dark, lit], MATERIAL_DTYPE)
        for v, idx in self.meshes:
            v4 = np.zeros((len(v), 4), np.float32)
            v4[:, :3] = v
            s.verts_pos_array.append(v4)
            s.indices_array.append(idx.copy())
        s.mesh_infos = np.array([api.default_mesh_info() for _ in self.meshes], MESH_INFO_DTYPE)
        insts = []
        for mesh, a, t, emissive in self.instances:
            l2w = np.vstack([a.T, t[None]]).astype(np.float32)      # (4 columns, 3 rows)
            insts.append(api.instance_from_transform(l2w, mesh, 1 if emissive else 0))
        s.instances = np.array(insts, INSTANCE_DTYPE) if insts else np.zeros(0, INSTANCE_DTYPE)
        textures, infos, envs = [], [], []
        for a, emission, tex in self.envs:
            e = api.default_environment()
            e["emission"] = emission
            m = np.eye(4, dtype=np.float32)
            m[:3, :3] = a.T                                            # [column][row]
            e["transform"] = m
            if tex is None:
                infos.append(api.EnvMapInfo(np.ones((1, 1, 4), np.float32), 1, 1))
            else:
                t4 = np.ones(tex.shape[:2] + (4,), np.float32)
                t4[..., :3] = tex
                e["emission_tex_idx"] = len(textures)
                textures.append(api.TextureCPU(t4.astype(np.float16)))
                infos.append(api.EnvMapInfo(t4, tex.shape[1], tex.shape[0]))
            envs.append(e)
        s.environments = np.array(envs, ENVIRONMENT_DTYPE) if envs else np.zeros(0, ENVIRONMENT_DTYPE)
        api.validate_scene(s, len(textures), len(textures))
        return s, textures, infos


class Built:
    """A Spec as the three parties see it: the uploaded / host Scene, and the float64 RefScene."""

    def __init__(self, spec, ctx=None):
        self.spec = spec
        self.cpu, self.textures, self.infos = spec.scene_cpu()
        self.scene = api.build_accel_structures_and_upload(ctx, self.cpu, self.textures, self.infos, True)
        order = [api.build_bvh(v, i)[1] for v, i in zip(self.cpu.verts_pos_array, self.cpu.indices_array)]
        self.ref = L.build(self.cpu, self.infos, order)


def env_texture(h, w, seed):
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.05, 1.0, (h, w, 3)) ** 3
    t[rng.integers(h), rng.integers(w)] = (40.0, 30.0, 20.0)             # a sun
    return t.astype(np.float16).astype(np.float64)                       # what both the weights and the shader see


def spec_quads():
    s = Spec()
    q, d = s.mesh(*quad()), s.mesh(*disc())
    s.inst(q, rot((1, 0, 0), 180), (0, 2, 0)).inst(q, rot((0, 0, 1), 90), (-2, 0.5, 0.3)).inst(d, rot((1, 0, 1), 70), (1.5, 0.8, -1))
    s.inst(q, np.eye(3) * 3, (0, -1, 0), emissive=False)
    return s


def spec_instances():
    s = Spec()
    q, d = s.mesh(*quad()), s.mesh(*disc())
    s.inst(q, rot((1, 0, 0), 180) * 2.5, (0, 2, 0)).inst(q, SHEAR @ rot((0, 0, 1), 80), (-2, 0.5, 0))
    s.inst(d, MIRROR @ rot((1, 1, 0), 60) * 0.5, (1.5, 0.5, -1)).inst(d, np.diag([2.0, 1.0, 0.4]) @ rot((0, 1, 1), 30), (0.5, 1.0, 2.0))
    return s


def spec_box():
    s = Spec()
    b = s.mesh(*box(0.5, 0.4, 0.3))
    s.inst(b, rot((1, 2, 3), 40), (0, 1, 0)).env()
    return s


def spec_env_only():
    return Spec().env()


def spec_envs():
    s = Spec()
    q = s.mesh(*quad())
    s.inst(q, rot((1, 0, 0), 180), (0, 2, 0))
    s.env().env(rot((1, 2, 0.5), 50), (1.0, 0.8, 0.6), env_texture(8, 16, 1)).env(rot((0, 1, 0), 120), (2, 2, 2), env_texture(1, 1, 2))
    s.env(rot((3, 1, 2), 200), (0.5, 1.0, 1.0), env_texture(5, 7, 3))
    return s


_bunny = []


def spec_bunny():
    if not _bunny:
        tmp = api.SceneCPU()
        loader.load_mesh_ply(os.path.join(util.SHARED, "shapes", "bunny.ply"), tmp)
        _bunny.append((tmp.verts_pos_array[0][:, :3].astype(np.float64), tmp.indices_array[0]))
    s = Spec()
    b = s.mesh(*_bunny[0])
    v = _bunny[0][0]
    c, r = 0.5 * (v.min(0) + v.max(0)), 0.5 * np.linalg.norm(v.max(0) - v.min(0))
    s.inst(b, rot((0, 1, 0), 30) / r, -(rot((0, 1, 0), 30) / r) @ c + (0, 1, 0))       # unit size, centred at (0, 1, 0)
    return s


SPECS = {"quads": spec_quads, "instances": spec_instances, "box": spec_box, "env_only": spec_env_only, "envs": spec_envs,
         "bunny": spec_bunny}
N_POINT = {"bunny": 160}
_built = {}


def built_scene(name, ctx=None):
    """Scenes are built once per (name, context).  The key holds the context itself, and the fixtures below drop a
    context's scenes before it closes and the rest when the module is done."""
    key = (name, ctx)
    if key not in _built:
        _built[key] = Built(SPECS[name](), ctx)
    return _built[key]


def drop_scenes(ctx):
    for key in [k for k in _built if k[1] is ctx]:
        del _built[key]


@pytest.fixture(scope="module", autouse=True)
def scene_cache():
    yield
    _built.clear()


def pdf_queries(b, n, seed):
    """Random shading points around the scene; half the directions aimed at random points of random emitters (scaled to a
    random length 1e-2 .. 1e2: `incoming` need not be a unit vector), half uniform on the sphere."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-2.5, 2.5, (n, 3)) + (0, 0.8, 0)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    if b.ref.lights:
        for q in range(0, n, 2):
            light = b.ref.lights[rng.integers(len(b.ref.lights))]
            tri = light.tris_world[rng.integers(len(light.tris_world))]
            w = rng.dirichlet((1, 1, 1))
            d[q] = (w @ tri - pos[q]) / np.linalg.norm(w @ tri - pos[q])
    d *= 10.0 ** rng.uniform(-2, 2, (n, 1))
    return api.light_records(api.LightMode.PDF, pos, d, EPS, 0)


def sample_records(pos, n, seed):
    rng = np.random.default_rng(seed)
    return api.light_records(api.LightMode.SAMPLE, np.broadcast_to(np.asarray(pos, np.float32), (n, 3)), None, EPS,
                             rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))


def oracle_probe(b):
    from oracle import oracle
    return lambda rec: oracle.light_probe(b.scene, rec)


# ---- CPU: point by point --------------------------------------------------------------------------------------------------

def kept_queries(b, rec):
    r = L.pdf(b.ref, rec[:, 1:4].astype(np.float64), rec[:, 4:7].astype(np.float64), rec[:, 7].astype(np.float64))
    keep = (r.edge_margin >= EDGE) & (r.eps_margin >= EPS_REL) & (r.min_cos >= MIN_COS) & (r.texel_margin >= TEXEL)
    return r, keep


@pytest.mark.parametrize("name", list(SPECS))
def test_oracle_pdf_matches_float64(built, name):
    b = built_scene(name)
    rec = pdf_queries(b, N_POINT.get(name, 3000), 11)
    r, keep = kept_queries(b, rec)
    excluded = 1.0 - keep.mean()
    out = oracle_probe(b)(rec)
    got = out[:, 3].astype(np.float64)
    err = np.abs(got - r.pdf) / np.maximum(r.pdf, 1e-30)
    err = np.where((r.pdf == 0.0) & (got == 0.0), 0.0, err)
    nz = float((r.pdf[keep] > 0).mean())
    print(f"{name}: excluded {excluded:.4f}, nonzero {nz:.3f}, max rel err kept {err[keep].max():.3e}, max pdf {r.pdf[keep].max():.3e}")
    assert excluded <= MAX_EXCLUDED
    if b.ref.lights:
        assert nz > 0.3                      # the aimed half reaches its emitter
    assert np.array_equal(out[:, 0:3], rec[:, 4:7]) and np.array_equal(out[:, 4].view(np.uint32), rec[:, 8].view(np.uint32))
    assert err[keep].max() <= PDF_RTOL


# ---- CPU: the samples follow the true density -------------------------------------------------------------------------------

SUB_FINE = 24
_quad_cache = []


def fine_quadrature():
    if not _quad_cache:
        _quad_cache.append(sphere_quadrature(SUB_FINE))
    return _quad_cache[0]


def sphere_chi2(b, pos, probe, n, seed, slot_prob=None, density_scale=None, ref=None, density=None):
    """Chi-square of n sampled directions at `pos` on the sphere grid, expected from the float64 true density of `ref`
    (default: the scene's own RefScene) or from `density(positions, directions)`."""
    out = probe(sample_records(pos, n, seed))
    d = out[:, 0:3].astype(np.float64)
    q, qbin, dw = fine_quadrature()
    qpos = np.broadcast_to(np.asarray(pos, np.float64), q.shape)
    dens = density(qpos, q) if density is not None else L.true_density(ref or b.ref, qpos, q, slot_prob)
    if density_scale is not None:
        dens = density_scale(dens, q)
    p = np.bincount(qbin, dens * dw, minlength=2 * NC * NPHI)
    obs = np.bincount(sphere_bin(d), minlength=2 * NC * NPHI)
    exp = p * n
    pooled = float(exp[exp < 5.0].sum() / n)
    stat, dof, pv = chi2_pooled(obs, exp)
    return dict(total=float(p.sum()), pooled=pooled, stat=stat, dof=dof, p=pv, out=out)


# (shading points chosen so that the grid quadrature passes assert_grid_adequate: silhouettes converge slowly)
SPHERE_CONFIGS = [("quads", (0.0, 0.2, 0.0)), ("box", (0.2, 0.2, 0.1)), ("overlap", (0.0, 0.0, 0.0))]
N_SPHERE = 60_000


def spec_overlap():
    """Three rigid planar emitters stacked in direction above the point (their pdf terms add), and a uniform environment."""
    s = Spec()
    q = s.mesh(*quad())
    s.inst(q, rot((1, 0, 0), 180), (0, 1.0, 0)).inst(q, rot((1, 0, 0), 170), (0.3, 1.6, 0)).inst(q, rot((0, 0, 1), 100), (-1.2, 0.3, 0.2))
    return s.env()


SPECS["overlap"] = spec_overlap


def assert_grid_adequate(r, want_total=1.0):
    assert abs(r["total"] - want_total) < 3e-3, r["total"]
    assert r["pooled"] <= 0.05, r["pooled"]


@pytest.mark.parametrize("name,pos", SPHERE_CONFIGS, ids=[c[0] for c in SPHERE_CONFIGS])
def test_sampling_follows_true_density(built, name, pos):
    b = built_scene(name)
    r = sphere_chi2(b, pos, oracle_probe(b), N_SPHERE, 21)
    print(f"{name}: integral {r['total']:.5f}, pooled mass {r['pooled']:.4f}, chi2 {r['stat']:.1f} / {r['dof']} dof, p = {r['p']:.3g}")
    assert_grid_adequate(r)
    assert r["p"] > 1e-3 / (len(SPHERE_CONFIGS) + 1)
    # rigid, planar, one crossing per emitter: the returned pdf is the true density at the samples
    d = r["out"][:, 0:3].astype(np.float64)
    td = L.true_density(b.ref, np.broadcast_to(np.asarray(pos, np.float64), d.shape), d)
    if name != "box":
        ok = td > 0
        assert np.allclose(r["out"][ok, 3], td[ok], rtol=1e-3)


def test_alias_slots_index_the_reordered_triangles(built):
    """Reference property (d): the alias table is built from the original triangle order, the sampler reads the BVH
    builder's reordered triangles at the drawn slot.  On the box (faces of three sizes, reordered by the builder) the
    chi-square above passes with that modelled and fails when the slots are taken to index the original order."""
    b = built_scene("box")
    original = L.build(b.cpu, b.infos, None)
    moved = np.abs(original.lights[0].area_world - b.ref.lights[0].area_world) > 1e-9
    assert moved.any()
    r = sphere_chi2(b, SPHERE_CONFIGS[1][1], oracle_probe(b), N_SPHERE, 21, ref=original)
    print(f"box, slots in the original order: {int(moved.sum())} of 12 slots differ in area; chi2 {r['stat']:.1f} / {r['dof']} dof, p = {r['p']:.3g}")
    assert r["p"] < 1e-6


def texel_chi2(b, env_index, probe, n, seed):
    """A textured environment's samples are its texel centres: count them by texel against the alias probabilities."""
    out = probe(sample_records((0.3, 0.2, 0.1), n, seed))
    d = out[:, 0:3].astype(np.float64)
    env = b.ref.envs[env_index]
    H, W = env.weights.shape
    centres = L.env_texel_to_dir(env, np.arange(H * W))
    # a sample belongs to this environment when it is one of its texel centres (float32 accuracy)
    cx, cy, _ = L.env_dir_to_texel(env, d)
    idx = cy * W + cx
    mine = np.linalg.norm(centres[idx] - d, axis=-1) < 1e-5
    share = 1.0 / b.ref.n
    obs = np.append(np.bincount(idx[mine], minlength=H * W), n - mine.sum())
    exp = np.append(env.prob.reshape(-1) * share, 1.0 - share) * n
    return chi2_pooled(obs, exp), float(mine.mean())


def test_textured_environment_samples_are_texel_centres(built):
    """Reference property: the pdf of a textured environment is piecewise constant, its sampler a set of point masses."""
    b = built_scene("envs")
    for k in (1, 3):
        (stat, dof, p), share = texel_chi2(b, k, oracle_probe(b), 200_000, 31 + k)
        print(f"env {k}: share {share:.4f}, chi2 {stat:.1f} / {dof} dof, p = {p:.3g}")
        assert abs(share - 1.0 / b.ref.n) < 5 * math.sqrt(0.2 * 0.8 / 200_000)
        assert p > 1e-3 / 2


# ---- CPU: E[1 / pdf] = solid angle of the support ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,pos", [("quads", (0.0, 0.9, 0.0)), ("overlap", (0.0, 0.0, 0.0))])
def test_mean_inverse_pdf_is_the_support(built, name, pos):
    """E over the sampler of 1 / (returned pdf) is the measure of the support where the pdf is the density of the samples
    (rigid, planar emitters): the emitters' solid angle by Van Oosterom and Strackee (in "quads" no two emitters overlap in
    direction from this point), 4 pi with a uniform environment.  The same with the float64 true density beside it."""
    b = built_scene(name)
    n = 100_000
    out = oracle_probe(b)(sample_records(pos, n, 41))
    d = out[:, 0:3].astype(np.float64)
    want = 4 * math.pi if b.ref.envs else sum(L.solid_angle(pos, lt.tris_world) for lt in b.ref.lights)
    td = L.true_density(b.ref, np.broadcast_to(np.asarray(pos, np.float64), d.shape), d)
    for label, dens in (("returned pdf", out[:, 3].astype(np.float64)), ("true density", td)):
        assert (dens > 0).all()
        inv = 1.0 / dens
        est, sigma = inv.mean(), inv.std(ddof=1) / math.sqrt(n)
        print(f"{name}: E[1 / {label}] = {est:.5f} +- {sigma:.5f}, support = {want:.5f}")
        assert abs(est - want) <= 5 * sigma


# ---- CPU: the samples are uniform on the emitters' surface -------------------------------------------------------------------

SURFACE_CONFIGS = [("quads", (0.0, 0.9, 0.0)), ("instances", (0.0, 1.0, 0.5))]   # points from which no two emitters overlap


def surface_chi2(b, pos, probe, n, seed, chunk=2_000_000):
    """Where a silhouette makes the sphere grid too coarse: bin each sample by the cell of the emitter it lands on -- light,
    triangle slot, one of the slot's four congruent sub-triangles -- where the expected count is exact:
    n / lights * slot probability / 4.  Needs every sampled direction to cross exactly one emitter triangle ahead of the
    point, which the float64 reference checks (the share that does not is returned: a float32 direction may miss a border by
    a rounding).  A closed emitter such as the bunny cannot be judged this way: a direction does not say which face was drawn."""
    out = probe(sample_records(pos, n, seed))
    d = out[:, 0:3].astype(np.float64)
    o = np.broadcast_to(np.asarray(pos, np.float64), d.shape)
    cell = np.full(n, -1, np.int64)
    count = np.zeros(n, np.int64)
    base, exp = 0, []
    for light in b.ref.lights:
        T = len(light.tris_world)
        step = max(1, chunk // T)
        for a in range(0, n, step):
            s_, u, v = L.crossings(o[a:a + step], d[a:a + step], light.tris_world)
            hit = np.isfinite(s_) & (s_ > 0) & (np.minimum(u, v) >= 0) & (u + v <= 1)
            qi, ti = np.nonzero(hit)
            uu, vv = u[qi, ti], v[qi, ti]
            sub = np.where(uu > 0.5, 1, np.where(vv > 0.5, 2, np.where(uu + vv < 0.5, 0, 3)))
            np.add.at(count, a + qi, 1)
            cell[a + qi] = base + 4 * ti + sub
        exp.append(np.repeat(light.prob / 4.0, 4) / b.ref.n)
        base += 4 * T
    exp = np.concatenate(exp) * n
    single = count == 1
    obs = np.bincount(cell[single], minlength=base)
    return chi2_pooled(obs, exp * single.mean()), 1.0 - float(single.mean())


@pytest.mark.parametrize("name,pos", SURFACE_CONFIGS, ids=[c[0] for c in SURFACE_CONFIGS])
def test_samples_are_uniform_on_the_emitters(built, name, pos):
    b = built_scene(name)
    (stat, dof, p), ambiguous = surface_chi2(b, pos, oracle_probe(b), 200_000, 71)
    print(f"{name}: {ambiguous:.4f} of the samples cross no or several triangles; chi2 {stat:.1f} / {dof} dof, p = {p:.3g}")
    assert ambiguous <= 1e-4
    assert p > 1e-3 / len(SURFACE_CONFIGS)


# ---- CPU: environment maps ---------------------------------------------------------------------------------------------------

def test_environment_maps_invert_and_integrate(built):
    b = built_scene("envs")
    for k, bins in zip((1, 2, 3), [b.scene.env_alias_tables[i] for i in (1, 2, 3)]):
        env = b.ref.envs[k]
        H, W = env.weights.shape
        cx, cy, m = L.env_dir_to_texel(env, L.env_texel_to_dir(env, np.arange(H * W)))
        assert np.array_equal(cy * W + cx, np.arange(H * W))
        assert (m > 0.49).all() or W == 1
        # Reference property: the stated texel solid angle takes sin at the row's middle, the exact band is narrower by
        # sin(x) / x with x = pi / (2 H) in every row, so the pdf integrates to that instead of one (2 / pi for one row)
        x = math.pi / (2 * H)
        assert L.env_pdf_integral(env) == pytest.approx(math.sin(x) / x, rel=1e-12)
        # the committed tables: prob is the weight share, and the threshold / alias pairs realise it
        assert np.allclose(bins["prob"], env.prob.reshape(-1), rtol=2e-6, atol=1e-12)
        assert np.allclose(L.alias_realised(bins), env.prob.reshape(-1), rtol=0, atol=2e-6)
    for light, bins in zip(b.ref.lights, b.scene.alias_tables):
        assert np.allclose(bins["prob"], light.prob, rtol=2e-6)
        assert np.allclose(L.alias_realised(bins), light.prob, atol=2e-6)


# ---- CPU: reference properties, pinned ----------------------------------------------------------------------------------------

def spec_scaled(s_=2.5):
    s = Spec()
    q = s.mesh(*quad())
    return s.inst(q, rot((1, 0, 0), 180) * s_, (0, 1.5, 0))


def spec_sheared():
    s = Spec()
    q = s.mesh(*quad())
    return s.inst(q, SHEAR @ rot((1, 0, 0), 180), (0, 1.5, 0))


def spec_thin_box():
    s = Spec()
    b = s.mesh(*box(0.8, 0.05, 0.8))
    return s.inst(b, np.eye(3), (0, 1.2, 0))


PROPERTY_POS = {"scaled": (0.0, 0.8, 0.1), "sheared": (0.0, 0.5, 0.0)}     # where the grid quadrature is adequate
SPECS.update(scaled=spec_scaled, sheared=spec_sheared, thin_box=spec_thin_box)


@pytest.mark.parametrize("name", ["scaled", "sheared"])
def test_pdf_uses_the_model_space_area(built, name):
    """Reference property (a): Light.area is the model-space area, the samples land on the world-space surface: the true
    density is (model area / world area) times the returned pdf -- 1 / s^2 under uniform scale s."""
    b = built_scene(name)
    light = b.ref.lights[0]
    factor = light.area / light.area_world.sum()
    if name == "scaled":
        assert factor == pytest.approx(1 / 2.5 ** 2, rel=1e-6)      # the transform is stored in float32
    pos = PROPERTY_POS[name]
    r = sphere_chi2(b, pos, oracle_probe(b), N_SPHERE, 51)
    d = r["out"][:, 0:3].astype(np.float64)
    td = L.true_density(b.ref, np.broadcast_to(np.asarray(pos, np.float64), d.shape), d)
    measured = td / r["out"][:, 3]
    print(f"{name}: true density / returned pdf = {measured.mean():.6f} (model / world area = {factor:.6f}); chi2 p = {r['p']:.3g}")
    assert np.allclose(measured, factor, rtol=1e-4)
    assert_grid_adequate(r)
    assert r["p"] > 1e-3 / 4


@pytest.mark.parametrize("name", ["scaled", "sheared"])
def test_area_check_fails_when_the_returned_pdf_is_taken_for_the_density(built, name):
    b = built_scene(name)
    light = b.ref.lights[0]
    factor = light.area / light.area_world.sum()
    r = sphere_chi2(b, PROPERTY_POS[name], oracle_probe(b), N_SPHERE, 51, density_scale=lambda dens, q: dens / factor)
    assert abs(r["total"] - 1.0) > 3e-3 and r["p"] < 1e-6


THIN_POS = (0.0, 0.0, 0.0)
THIN_GRID_POS = (0.15, 0.4, -0.1)      # where the sphere grid's quadrature is adequate for the slab (assert_grid_adequate)


def thin_box_counts(b, probe, n=20_000, seed=61):
    out = probe(sample_records(THIN_POS, n, seed))
    d = out[:, 0:3].astype(np.float64)
    o = np.broadcast_to(np.asarray(THIN_POS, np.float64), d.shape)
    td = L.true_density(b.ref, o, d)
    ref = L.pdf(b.ref, o, d, EPS)
    keep = (ref.edge_margin >= EDGE) & (ref.eps_margin >= EPS_REL) & (ref.min_cos >= MIN_COS)
    return out, td, ref, keep


def test_pdf_skips_a_face_behind_a_thin_emitter(built):
    """Reference property (b): the march restarts at light_pos + incoming, one unit further: the far face of a closed
    emitter thinner than |incoming| is never counted, the sampler picks it by area all the same."""
    b = built_scene("thin_box")
    out, td, ref, keep = thin_box_counts(b, oracle_probe(b))
    assert keep.mean() > 0.95
    assert np.allclose(out[keep, 3], ref.pdf[keep], rtol=PDF_RTOL)
    # through both large faces the float64 march counts the near one only; the true density counts both
    ratio = td[keep] / ref.pdf[keep]
    both = ratio > 1.5
    print(f"thin box: {both.mean():.3f} of the samples cross two faces; true / returned there = {np.median(ratio[both]):.4f}")
    assert both.mean() > 0.8
    # the faces y = 1.15 and y = 1.25 seen from the origin: through both, true / returned = 1 + (far / near)^2
    d = out[keep, 0:3].astype(np.float64)
    top = 1.25 / d[:, 1]
    through = (d[:, 1] > 0) & (np.abs(top * d[:, 0]) < 0.8) & (np.abs(top * d[:, 2]) < 0.8)
    assert through.mean() > 0.8
    assert np.allclose(ratio[through], 1.0 + (1.25 / 1.15) ** 2, rtol=1e-5)
    # and the samples follow the true density, both faces counted
    r = sphere_chi2(b, THIN_GRID_POS, oracle_probe(b), N_SPHERE, 63)
    print(f"thin box: integral {r['total']:.5f}, pooled mass {r['pooled']:.4f}, chi2 {r['stat']:.1f} / {r['dof']} dof, p = {r['p']:.3g}")
    assert_grid_adequate(r)
    assert r["p"] > 1e-3 / 4


def test_thin_emitter_check_fails_when_the_returned_pdf_is_taken_for_the_density(built):
    """The same chi-square with the expected counts from the float64 restatement of the *returned* pdf (one face): it
    integrates to well under one and the chi-square fails."""
    b = built_scene("thin_box")
    r = sphere_chi2(b, THIN_GRID_POS, oracle_probe(b), N_SPHERE, 63, density=lambda o, d: L.pdf(b.ref, o, d, EPS).pdf)
    print(f"thin box, returned pdf as the density: integral {r['total']:.5f}, chi2 {r['stat']:.1f} / {r['dof']} dof, p = {r['p']:.3g}")
    assert r["total"] < 0.7 and r["p"] < 1e-6


# ---- the cull scenes ------------------------------------------------------------------------------------------------------------

CULL_DISTANCES = (1e3, 1e4, 1e5)
CULL_COUNTS = [1, 2, 3, 4, 5, 31, 32, 33, 96, 97, 127, 128, 129, 160, 257]


def spec_cull(n, seed=7, moved=False):
    """n small quads, rigid / scaled / sheared / mirrored in turn, on three jittered grids 1e3, 1e4 and 1e5 units from the
    origin: light k belongs to grid (k + n) % 3, so every count of two or more spans two distances, three or more all three,
    and each kind of transform meets each distance.  At 1e5 a float32 ulp of a position is 0.008, against a 1 x 0.6 quad."""
    rng = np.random.default_rng(seed + (1000 if moved else 0))
    s = Spec()
    q = s.mesh(*quad(0.5, 0.3))
    axis = np.array([1.0, 0.3, -0.2]) / np.linalg.norm([1.0, 0.3, -0.2])
    for k in range(n):
        base = CULL_DISTANCES[(k + n) % 3] * axis
        a = rot(rng.normal(size=3), rng.uniform(0, 360))
        kind = k % 4
        if kind == 1:
            a = a * rng.uniform(0.3, 3.0)
        elif kind == 2:
            a = SHEAR @ a
        elif kind == 3:
            a = MIRROR @ a
        s.inst(q, a, base + (4.0 * (k % 17), 4.0 * (k // 17), 0) + rng.uniform(-1, 1, 3))
    return s


def bounding_sphere(light):
    """Centre and radius of the (unpadded) sphere the cull must never shrink: box centre, farthest vertex."""
    v = light.tris_world.reshape(-1, 3)
    c = 0.5 * (v.min(0) + v.max(0))
    return c, float(np.linalg.norm(v - c, axis=-1).max())


def cull_queries(ref, seed=5):
    """Per light: through the farthest vertex region (just inside the emitter's corner), tangent to the sphere just inside and
    just outside, from inside the sphere, from just past the emitter looking back and away; lengths 1e-3 .. 1e3; eps 0 and 1e-3."""
    rng = np.random.default_rng(seed)
    pos, d, eps = [], [], []

    def f32(x):          # origins are float32 in the records: aim from where the ray will really start
        return np.asarray(x, np.float32).astype(np.float64)

    for light in ref.lights:
        c, r = bounding_sphere(light)
        v = light.tris_world.reshape(-1, 3)
        far_v = v[np.argmax(np.linalg.norm(v - c, axis=-1))]
        ctr = light.tris_world.reshape(-1, 3).mean(0)
        n = light.normals_world[0]

        def ray(origin, target, length, e):
            origin = f32(origin)
            dd = target - origin
            pos.append(origin); d.append(dd / np.linalg.norm(dd) * length); eps.append(e)

        o = f32(c + 6.0 * r * (n + 0.3 * rng.normal(size=3)))
        ray(o, ctr + 0.97 * (far_v - ctr), 10.0 ** rng.uniform(-3, 3), EPS)         # hits beyond 0.95 r of the centre
        ray(o, ctr + 0.999 * (far_v - ctr), 1.0, 0.0)
        t = np.cross(o - c, rng.normal(size=3))
        t /= np.linalg.norm(t)
        dist = np.linalg.norm(c - o)
        for f in (0.97, 0.98, 0.99, 1.01, 1.02, 1.03, 1.04):                         # the ray's line passes the centre at f r:
            a = math.asin(f * r / dist)                                               # just inside the rim, and just missing it
            ray(o, o + dist * (math.cos(a) * (c - o) / dist + math.sin(a) * t), 10.0 ** rng.uniform(-3, 3), EPS)
        inside = c + 0.4 * r * n + 0.2 * r * rng.normal(size=3) / 3
        ray(inside, ctr + 0.5 * (far_v - ctr), 10.0 ** rng.uniform(-3, 3), EPS)     # origin inside the sphere
        ray(inside, inside + n, 1.0, 0.0)
        past = ctr - 1.5 * r * n
        ray(past, past - n + 0.1 * rng.normal(size=3), 1.0, EPS)                     # outside, the emitter behind
        ray(ctr - 1e-2 * r * n, ctr + 0.3 * (far_v - ctr) + r * n, 10.0 ** rng.uniform(-3, 3), EPS)   # just past, looking back
    return api.light_records(api.LightMode.PDF, np.array(pos), np.array(d), np.array(eps), 0)


def test_cull_queries_are_sharp(built):
    """In float64, no device: per light of the cull scene, a hit farther than 0.95 r from the sphere's centre, an origin
    inside the sphere, an origin outside with the emitter behind, and a miss of the sphere by less than 0.05 r.  A cull that
    shrank the radius by 5 % could then not pass the GPU test."""
    for spec in (spec_cull(33), spec_cull(257), spec_cull(33, moved=True)):
        b = Built(spec)
        dist = np.array([np.linalg.norm(lt.tris_world.reshape(-1, 3).mean(0)) for lt in b.ref.lights])
        for want in CULL_DISTANCES:                      # the emitters do lie 1e3, 1e4 and 1e5 units out
            assert (np.abs(dist / want - 1.0) < 0.1).sum() >= len(dist) // 3
        rec = cull_queries(b.ref)
        o, d = rec[:, 1:4].astype(np.float64), rec[:, 4:7].astype(np.float64)
        per = len(rec) // len(b.ref.lights)
        for k, light in enumerate(b.ref.lights):
            c, r = bounding_sphere(light)
            oo, dd = o[k * per:(k + 1) * per], d[k * per:(k + 1) * per]
            s, u, v = L.crossings(oo, dd, light.tris_world)
            hit = np.isfinite(s) & (s > 0) & (np.minimum(u, v) >= 0) & (u + v <= 1)
            p = oo[:, None] + s[..., None] * dd[:, None]
            rim_hit = (hit & (np.linalg.norm(np.nan_to_num(p) - c, axis=-1) > 0.95 * r)).any()
            inside = np.linalg.norm(oo - c, axis=-1) < r
            du = dd / np.linalg.norm(dd, axis=-1, keepdims=True)
            along = np.sum((c - oo) * du, -1)
            line = np.sqrt(np.maximum(np.sum((c - oo) ** 2, -1) - along ** 2, 0))
            behind = (~inside) & (along < 0)
            near_miss = (~inside) & (along > 0) & (line > r) & (line < 1.05 * r)
            assert rim_hit and inside.any() and behind.any() and near_miss.any(), (k, rim_hit, inside.any(), behind.any(), near_miss.any())


# ---- GPU: the device equals the oracle ------------------------------------------------------------------------------------------

def assert_bits_equal(got, want, what):
    diff = got.view(np.uint32) != want.view(np.uint32)
    # a NaN on both sides is equal whatever its sign and payload, as in the scatter probe's test; the RNG word is bits
    both_nan = np.isnan(got) & np.isnan(want)
    both_nan[:, 4] = False
    diff &= ~both_nan
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
    drop_scenes(ctx)
    ctx.close()


def staged_in_lds(ctx, scene):
    """Whether this context's kernels read the scene's geometry from LDS (GeoLds): such a scene has no four-wide hierarchy,
    and the wide probe says so."""
    try:
        api.trace_rays_wide(ctx, scene, [[0.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    except api.LupinError as e:
        assert "staged in LDS" in str(e), str(e)
        return True
    return False


def both_modes(b, n, seed):
    pdfs = pdf_queries(b, n, seed)
    rng = np.random.default_rng(seed + 1)
    smp = api.light_records(api.LightMode.SAMPLE, pdfs[:, 1:4], None, EPS, rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))
    return np.concatenate([pdfs, smp])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["quads", "instances", "box", "env_only", "envs", "overlap", "scaled", "sheared", "thin_box", "bunny"])
def test_device_equals_oracle_on_the_cpu_query_sets(gpu_ctx, global_ctx, name):
    from oracle import oracle
    assert os.environ.get("LUPIN_LIGHT_STAGE") is None
    host = built_scene(name)
    rec = both_modes(host, 20_000 if name != "bunny" else 4_000, 11)
    want = oracle.light_probe(host.scene, rec)
    for label, ctx in (("lds", gpu_ctx), ("global", global_ctx)):
        dev = built_scene(name, ctx)
        if host.ref.lights:          # (a scene without instances has no geometry to stage)
            # the bunny (144 046 triangles) is too large to stage: both legs then go through GeoGlobal
            assert staged_in_lds(ctx, dev.scene) == (label == "lds" and name != "bunny"), (name, label)
        assert_bits_equal(api.light_probe(ctx, dev.scene, rec), want, f"{name} / {label}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", CULL_COUNTS)
def test_device_equals_oracle_on_the_cull_set(gpu_ctx, n):
    from oracle import oracle
    b = Built(spec_cull(n), gpu_ctx)
    assert len(b.ref.lights) == n
    rec = np.concatenate([cull_queries(b.ref), both_modes_far(b, 4096, n)])
    assert_bits_equal(api.light_probe(gpu_ctx, b.scene, rec), oracle.light_probe(b.scene, rec), f"cull set, {n} lights")


def both_modes_far(b, n, seed):
    """Random records around a cull scene: origins within a few radii of random emitters, aimed at emitters or anywhere."""
    rng = np.random.default_rng(seed)
    centres = np.array([lt.tris_world.reshape(-1, 3).mean(0) for lt in b.ref.lights])
    oi = rng.integers(len(centres), size=n)
    ti = (oi + 3 * rng.integers(-3, 4, size=n)) % len(centres)        # mostly an emitter of the same grid
    pos = centres[oi] + rng.normal(size=(n, 3)) * 3.0
    tgt = centres[ti] + rng.uniform(-0.5, 0.5, (n, 3))
    d = tgt - pos
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    d *= 10.0 ** rng.uniform(-3, 3, (n, 1))
    pdfs = api.light_records(api.LightMode.PDF, pos, d, np.where(rng.random(n) < 0.2, 0.0, EPS), 0)
    smp = api.light_records(api.LightMode.SAMPLE, pos, None, EPS, rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32))
    return np.concatenate([pdfs, smp])


@pytest.mark.gpu
def test_device_cull_keeps_a_singular_light(gpu_ctx):
    """An emitter whose world -> local rows are singular has no finite bounding sphere: its bound must mean 'never culled'.
    (update_instances refuses such a transform, so the scene is created with it.)"""
    from oracle import oracle
    host = Built(spec_cull(5))
    cpu, textures, infos = spec_cull(5).scene_cpu()
    t = cpu.instances["transpose_inverse_transform"].copy()
    t[2, 2] = t[2, 1]                                   # instance 2: two equal rows
    cpu.instances["transpose_inverse_transform"] = t
    scene = api.build_accel_structures_and_upload(gpu_ctx, cpu, textures, infos, True)
    rec = np.concatenate([cull_queries(host.ref), both_modes_far(host, 4096, 3)])
    assert_bits_equal(api.light_probe(gpu_ctx, scene, rec), oracle.light_probe(scene, rec), "singular light")


@pytest.mark.gpu
@pytest.mark.parametrize("n", CULL_COUNTS)
def test_device_equals_oracle_after_update_instances(gpu_ctx, n):
    """The eight-corner bounds of scene_update_instances: moved, scaled and sheared emitters against the oracle on the
    updated scene and against a scene created from the new transforms."""
    from oracle import oracle
    b = Built(spec_cull(n), gpu_ctx)
    moved = Built(spec_cull(n, moved=True), gpu_ctx)
    b.scene.update_instances(moved.scene.instances["transpose_inverse_transform"])
    rec = np.concatenate([cull_queries(moved.ref), both_modes_far(moved, 4096, n + 1)])
    got = api.light_probe(gpu_ctx, b.scene, rec)
    assert_bits_equal(got, oracle.light_probe(b.scene, rec), f"updated scene, {n} lights")
    assert_bits_equal(got, api.light_probe(gpu_ctx, moved.scene, rec), f"updated against fresh scene, {n} lights")


@pytest.mark.gpu
def test_device_sampling_follows_true_density(gpu_ctx):
    for name, pos in (SPHERE_CONFIGS[0], SPHERE_CONFIGS[2]):
        b = built_scene(name, gpu_ctx)
        r = sphere_chi2(b, pos, lambda rec: api.light_probe(gpu_ctx, b.scene, rec), N_SPHERE, 77)
        print(f"device {name}: chi2 {r['stat']:.1f} / {r['dof']} dof, p = {r['p']:.3g}")
        assert_grid_adequate(r)
        assert r["p"] > 1e-3 / 2


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["bistro_class_small", "cull257"])
def test_device_equals_oracle_on_a_million_records(gpu_ctx, which):
    from oracle import oracle
    n = 1 << 20
    rng = np.random.default_rng(99)
    if which == "cull257":
        b = Built(spec_cull(257), gpu_ctx)
        scene = b.scene
        rec = both_modes_far(b, n // 2, 99)
    else:
        scene, _ = util.load_scene(which, gpu_ctx)
        pos = rng.uniform(-12, 12, (n, 3)) * (1, 0.3, 1) + (0, 2, 0)
        d = rng.normal(size=(n, 3))
        rec = api.light_records(api.LightMode.PDF, pos, d, EPS, 0)
        rec[n // 2:, 0] = float(api.LightMode.SAMPLE)
        rec.view(np.uint32)[n // 2:, 8] = rng.integers(0, 2 ** 32, n - n // 2, dtype=np.uint64).astype(np.uint32)
    assert_bits_equal(api.light_probe(gpu_ctx, scene, rec), oracle.light_probe(scene, rec), which)
