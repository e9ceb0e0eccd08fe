"""Irradiance volume lookups on the device (lupin_hip_sample_probe_grid): the fused kernel against
tests/probe_grid_ref.py WORD FOR WORD -- every flag combination, grid shape, record count around a group, a wave and a
block, with the visibility of every corner taken from api.occlusion_rays on the restatement's own segment records -- then
the properties the feature exists for (no light through a wall, invalid probes never used, the backface weight, a baked
grid end to end), the same words from staged and global geometry and after instances moved, every refusal, frames around
a call, and device memory in place."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import closest_hit_ref as X
from tests import probe_grid_ref as R
from tests import util
from tests.test_gpu_closest_hit import device_scene, staged_in_lds
from tests.test_gpu_ray_query import DeviceArray, chain_bvh

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT = api.PathtraceType
SENTINEL = np.float32(-7.0)
COUNTS = (1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 1000)
GRIDS = ((2, 2, 2), (1, 1, 1), (4, 1, 3), (3, 4, 2))
_cache = {}


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scene_box(c):
    """The box around the instances of a closest_hit_ref case, float32."""
    l2w = c.g.local_to_world()
    pts = np.concatenate([c.g.meshes[c.g.mesh_idx[i]].verts @ l2w[i][:, :3].T + l2w[i][:, 3] for i in range(len(c.g.rows))])
    return pts.min(0).astype(np.float32), pts.max(0).astype(np.float32)


def grid_over(lo, hi, dims):
    """(origin, spacing, dims): the first and last probe on the box's faces; an axis with one probe gets the box's side."""
    dims = tuple(int(d) for d in dims)
    spacing = np.float32([(hi[k] - lo[k]) / max(1, dims[k] - 1) for k in range(3)])
    return np.float32(lo), spacing, dims


def surface_points(c, moved=False):
    """Hit points of the case's rays with their geometric normals (float64 reference hits, rounded to float32)."""
    ref = c.refs[1e-3]
    sel = np.nonzero(ref.hit)[0]
    p = c.ori[sel].astype(np.float64) + c.dir[sel].astype(np.float64) * ref.t[sel, None]
    nrm = np.zeros((len(sel), 3))
    for r, k in enumerate(sel):
        i = ref.inst[k]
        v = c.g.meshes[c.g.mesh_idx[i]].verts[ref.tri[k]]
        nw = c.g.rows[i][:, :3].T @ np.cross(v[1] - v[0], v[2] - v[0])
        nrm[r] = nw / np.linalg.norm(nw)
    ok = np.all(np.isfinite(nrm), axis=1) & np.all(np.abs(p) < 1e3, axis=1)
    return p[ok].astype(np.float32), nrm[ok].astype(np.float32)


def batch(kind, grid, moved=False):
    """1000 records: surface points with their normals, 30 points outside the box and 30 exactly on probes mixed in, so
    that every prefix of COUNTS holds some of each."""
    key = (kind, grid[2], moved)
    if key not in _cache:
        c = X.case(kind, moved)
        rng = np.random.default_rng(23)
        p, nrm = surface_points(c)
        assert len(p) >= 940
        pick = rng.permutation(len(p))[:940]
        lo, hi = scene_box(c)
        outside = (lo + (rng.uniform(-0.5, 1.5, (30, 3)) * (hi - lo))).astype(np.float32)
        outside[:, 0] = np.where(np.arange(30) % 2, lo[0] - 1.0, hi[0] + 2.5)
        pos = api.probe_grid_positions(*grid)
        on = pos[rng.integers(0, len(pos), 30)]
        d = rng.normal(size=(60, 3))
        extra_n = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
        pts, nrms = np.concatenate([p[pick], outside, on]), np.concatenate([nrm[pick], extra_n])
        order = np.concatenate([[940, 970, 0, 941, 971, 1, 2], rng.permutation(np.setdiff1d(np.arange(1000), [940, 970, 0, 941, 971, 1, 2]))])
        _cache[key] = api.probe_grid_records(pts[order], nrms[order])
    return _cache[key]


def expected(ctx, scene, grid, sh, rec, valid, vis, back, eps, bias):
    """The restatement, its `blocked` flags from api.occlusion_rays on its own segments."""
    blocked = None
    if vis:
        cn = R.corners(*grid, rec, bias, valid)
        seg, mask = R.segments(cn, eps)
        blocked = np.zeros(mask.shape, bool)
        if len(seg):
            blocked[mask] = api.occlusion_rays(ctx, scene, seg, ray_epsilon=eps) != 0
    return R.sample(*grid, sh, rec, valid=valid, backface=back, blocked=blocked, ray_epsilon=eps, normal_bias=bias), blocked


def lookup(ctx, scene, grid, sh, rec, valid, vis, back, eps, bias):
    return api.sample_probe_grid(ctx, scene, *grid, sh, rec, valid=valid, visibility=vis, backface=back, ray_epsilon=eps, normal_bias=bias)


@pytest.fixture(scope="module")
def global_ctx(built):
    """A context whose kernels read every scene from global memory, as tests/test_gpu_occlusion.py makes one."""
    old = os.environ.get("LUPIN_LDS_GEOMETRY")
    os.environ["LUPIN_LDS_GEOMETRY"] = "0"     # read at context creation
    try:
        ctx = api.Context(0)
    finally:
        if old is None:
            os.environ.pop("LUPIN_LDS_GEOMETRY", None)
        else:
            os.environ["LUPIN_LDS_GEOMETRY"] = old
    yield ctx
    ctx.close()


# ---- 1. word for word ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dims", GRIDS)
@pytest.mark.parametrize("kind", ["small", "big"])
def test_word_for_word_against_the_restatement(gpu_ctx, kind, dims):
    c = X.case(kind)
    scene = device_scene(gpu_ctx, kind)
    assert staged_in_lds(gpu_ctx, scene) == (kind == "small")
    grid = grid_over(*scene_box(c), dims)
    rec = batch(kind, grid)
    P = int(np.prod(dims))
    rng = np.random.default_rng(1000 + 10 * GRIDS.index(dims) + (kind == "big"))
    sh = rng.normal(size=(P, 9, 4)).astype(np.float32)
    some_valid = (rng.uniform(size=P) > 0.33).astype(np.uint8)
    default_bias = api.LIGHTMAP_OFFSET_FRACTION * api.scene_world_extent(scene)
    assert default_bias > 0
    seen_blocked = seen_short = calls = 0
    for valid in (None, some_valid):
        for eps in (0.0, 1e-3):
            for bias in (0.0, default_bias):
                for vis in (False, True):
                    for back in (False, True):
                        want, blocked = expected(gpu_ctx, scene, grid, sh, rec, valid, vis, back, eps, bias)
                        if vis:
                            seen_blocked += int(blocked.sum())
                            cn = R.corners(*grid, rec, bias, valid)
                            seen_short += int((cn.use & ~(cn.len > np.float32(2.0) * np.float32(eps))).sum())
                        for n in COUNTS:
                            got = lookup(gpu_ctx, scene, grid, sh, rec[:n], valid, vis, back, eps, bias)
                            assert got.shape == (n, 4) and got.dtype == np.float32
                            diff = np.nonzero((words(got) != words(want[:n])).any(axis=1))[0]
                            assert len(diff) == 0, (kind, dims, valid is not None, eps, bias, vis, back, n, diff[:5], got[diff[:5]], want[diff[:5]])
                            calls += 1
    assert calls == 2 * 2 * 2 * 4 * len(COUNTS)
    assert seen_short > 0                                   # points on probes: the len <= 2 eps branch was taken
    if P > 1:
        assert seen_blocked > 100                           # and walls were in the way


# ---- 2. no light through a wall -----------------------------------------------------------------------------------

def quad_x(x, half):
    v = np.zeros((4, 4), np.float32)
    v[:, :3] = [(x, -half, -half), (x, -half, half), (x, half, half), (x, half, -half)]
    return v, np.array([0, 1, 2, 0, 2, 3], np.uint32)


def quad_y(y, half, flip=False):
    v = np.zeros((4, 4), np.float32)
    v[:, :3] = [(-half, y, -half), (-half, y, half), (half, y, half), (half, y, -half)]
    return v, np.array([0, 1, 2, 0, 2, 3] if flip else [0, 2, 1, 2, 0, 3], np.uint32)


def upload(ctx, meshes):
    cpu = api.SceneCPU()
    cpu.materials = np.array([api.default_material()], _abi.MATERIAL_DTYPE)
    for v, idx in meshes:
        cpu.verts_pos_array.append(v)
        cpu.indices_array.append(idx)
    cpu.mesh_infos = np.array([api.default_mesh_info() for _ in meshes], _abi.MESH_INFO_DTYPE)
    cpu.instances = np.array([api.default_instance() for _ in meshes], _abi.INSTANCE_DTYPE)
    cpu.instances["mesh_idx"] = np.arange(len(meshes))
    api.validate_scene(cpu, 0, 0)
    return api.build_accel_structures_and_upload(ctx, cpu, [], [], True)


def wall(ctx):
    if "wall" not in _cache:
        _cache["wall"] = upload(ctx, [quad_x(0.0, 10.0)])
    return _cache["wall"]


def room(ctx):
    """tests/test_gpu_occlusion.py's room: a floor at y = 0 under a ceiling at y = 1, both 20 wide."""
    if "room" not in _cache:
        _cache["room"] = upload(ctx, [quad_y(0.0, 10.0, flip=True), quad_y(1.0, 10.0)])
    return _cache["room"]


WALL_GRID = (np.float32([-1, -1, -1]), np.float32([2, 2, 2]), (2, 2, 2))


def test_no_light_through_a_wall(gpu_ctx):
    scene = wall(gpu_ctx)
    L = np.float32([1.0, 2.5, 0.25])
    pos = api.probe_grid_positions(*WALL_GRID)
    sh = np.zeros((8, 9, 4), np.float32)
    sh[pos[:, 0] < 0, 0, :3] = L / R.K0                     # band-0 radiance L on the lit side, darkness on the other
    rng = np.random.default_rng(3)
    n = 200
    yz = rng.uniform(-0.9, 0.9, (n, 2)).astype(np.float32)
    dark = api.probe_grid_records(np.column_stack([np.full(n, 0.25, np.float32), yz]), np.tile(np.float32([1, 0, 0]), (n, 1)))
    lit = api.probe_grid_records(np.column_stack([np.full(n, -0.25, np.float32), yz]), np.tile(np.float32([-1, 0, 0]), (n, 1)))
    for back in (False, True):
        leak = lookup(gpu_ctx, scene, WALL_GRID, sh, dark, None, False, back, 1e-3, 0.0)
        assert np.all(leak[:, :3] > 0) and np.all(leak[:, 3] > 0)                    # the leak this feature exists to stop
        got = lookup(gpu_ctx, scene, WALL_GRID, sh, dark, None, True, back, 1e-3, 0.0)
        assert np.all(words(got[:, :3]) == 0) and np.all(got[:, 3] > 0)             # exactly +0.0f
        got = lookup(gpu_ctx, scene, WALL_GRID, sh, lit, None, True, back, 1e-3, 0.0)
        want = np.pi * L.astype(np.float64)
        bound = R.irradiance_bound(sh[0], lit[:, 4:7])
        assert np.all(np.abs(got[:, :3] - want) <= bound + np.pi * 2.0 ** -24 * L) and np.all(got[:, 3] > 0)   # (L / k0 is rounded once more)


# ---- 3. validity ---------------------------------------------------------------------------------------------------

def test_invalid_probes_never_contribute(gpu_ctx):
    c = X.case("small")
    scene = device_scene(gpu_ctx, "small")
    grid = grid_over(*scene_box(c), (3, 4, 2))
    rec = batch("small", grid)
    rng = np.random.default_rng(4)
    valid = (rng.uniform(size=24) > 0.4).astype(np.uint8)
    sh = rng.normal(size=(24, 9, 4)).astype(np.float32)
    sh[valid == 0] = np.nan                                  # an invalid probe's coefficients must not even be multiplied by 0
    for vis in (False, True):
        got = lookup(gpu_ctx, scene, grid, sh, rec, valid, vis, True, 1e-3, 0.0)
        assert np.all(np.isfinite(got))
        want, _ = expected(gpu_ctx, scene, grid, sh, rec, valid, vis, True, 1e-3, 0.0)
        assert np.array_equal(words(got), words(want))
        assert (got[:, 3] == 0).sum() > 0 and (got[:, 3] > 0).sum() > 100
    # a cell with all eight invalid: four zero words
    got = lookup(gpu_ctx, scene, grid, sh, rec, np.zeros(24, np.uint8), True, True, 1e-3, 0.0)
    assert np.all(words(got) == 0)
    # NaN coefficients of a probe in use reach the output
    got = lookup(gpu_ctx, scene, grid, sh, rec, None, False, False, 1e-3, 0.0)
    assert np.isnan(got[:, :3]).any()


# ---- 4. the backface weight ---------------------------------------------------------------------------------------

def test_the_backface_weight_moves_the_result_toward_the_probe_the_normal_faces(gpu_ctx):
    scene = room(gpu_ctx)
    grid = (np.float32([0, 0.5, 0]), np.float32([1, 1, 1]), (2, 1, 1))
    sh = np.zeros((2, 9, 4), np.float32)
    sh[0, 0, :3], sh[1, 0, :3] = 1.0, 3.0
    p = np.float32([[0.5, 0.5, 0.0]] * 3)
    nrm = np.float32([[1, 0, 0], [-1, 0, 0], [0, 0, 1]])
    rec = api.probe_grid_records(p, nrm)
    plain = lookup(gpu_ctx, scene, grid, sh, rec, None, False, False, 1e-3, 0.0)
    got = lookup(gpu_ctx, scene, grid, sh, rec, None, False, True, 1e-3, 0.0)
    k = np.pi * 0.5 * np.sqrt(1.0 / np.pi)
    assert np.allclose(plain[:, 0], 2.0 * k, rtol=1e-6) and np.all(plain[:, 3] == 1.0)
    assert got[0, 0] > plain[0, 0] > got[1, 0]               # toward probe 1 (value 3) | toward probe 0 (value 1)
    assert np.isclose(got[0, 0], k * (0.1 * 1 + 0.6 * 3) / 0.7, rtol=1e-6) and np.isclose(got[1, 0], k * (0.6 * 1 + 0.1 * 3) / 0.7, rtol=1e-6)
    assert np.isclose(got[2, 0], 2.0 * k, rtol=1e-6)         # a normal across the axis favours neither
    for back in (False, True):
        assert np.array_equal(words(lookup(gpu_ctx, scene, grid, sh, rec, None, False, back, 1e-3, 0.0)), words(R.sample(*grid, sh, rec, backface=back)))


# ---- 5. a baked grid end to end -----------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["room", "cornell"])
def test_a_baked_grid_sampled_at_its_probes_returns_their_irradiance(gpu_ctx, which):
    if which == "room":
        scene, grid = room(gpu_ctx), (np.float32([-1, 0.25, -1]), np.float32([1, 0.5, 2]), (3, 2, 2))
    else:
        scene, grid = util.load_scene("cornellbox_builtin", gpu_ctx)[0], (np.float32([-0.6, 0.4, -0.6]), np.float32([0.6, 0.6, 1.2]), (3, 3, 2))
    pos, sh = api.bake_probe_grid(gpu_ctx, scene, *grid, samples=16, max_bounces=2)
    P = int(np.prod(grid[2]))
    assert pos.shape == (P, 3) and sh.shape == (P, 9, 4) and np.array_equal(pos, api.probe_grid_positions(*grid))
    assert np.array_equal(words(sh), words(api.bake_probes(gpu_ctx, scene, pos, samples=16, max_bounces=2)))   # one bake_probes call, nothing else
    assert np.all(sh[:, 0, 3] > 0)
    if which == "cornell":
        assert float(sh[:, 0, :3].max()) > 0
    rng = np.random.default_rng(5)
    d = rng.normal(size=(P, 3))
    nrm = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rec = api.probe_grid_records(pos, nrm)
    got = lookup(gpu_ctx, scene, grid, sh, rec, None, False, False, 1e-3, 0.0)
    assert np.array_equal(words(got), words(R.sample(*grid, sh, rec)))
    assert np.all(got[:, 3] == 1.0)
    assert np.all(np.abs(got[:, :3] - api.sh_irradiance(sh, nrm)) <= R.irradiance_bound(sh, nrm))
    # the defaults (visibility, backface, the scene's bias) run and weigh the same probe alone
    full = api.sample_probe_grid(gpu_ctx, scene, *grid, sh, pos, nrm)
    assert full.shape == (P, 4) and np.all(np.isfinite(full))


# ---- 6. staged and global geometry --------------------------------------------------------------------------------

def test_staged_and_global_geometry_give_the_same_words(gpu_ctx, global_ctx):
    c = X.case("small")
    staged, unstaged = device_scene(gpu_ctx, "small"), X.build("small", X.SEED, global_ctx)
    assert staged_in_lds(gpu_ctx, staged) and not staged_in_lds(global_ctx, unstaged)
    grid = grid_over(*scene_box(c), (3, 4, 2))
    rec = batch("small", grid)
    sh = np.random.default_rng(6).normal(size=(24, 9, 4)).astype(np.float32)
    for vis in (True, False):
        for n in (9, 65, 1000):
            a = lookup(gpu_ctx, staged, grid, sh, rec[:n], None, vis, True, 1e-3, 0.0)
            b = lookup(global_ctx, unstaged, grid, sh, rec[:n], None, vis, True, 1e-3, 0.0)
            assert np.array_equal(words(a), words(b)), (vis, n)


# ---- 7. after Scene.update_instances ------------------------------------------------------------------------------

@pytest.mark.parametrize("tlas_builder", ["cpu", "device"])
def test_moved_instances_give_the_answers_of_a_fresh_scene(gpu_ctx, tlas_builder):
    c = X.case("big", moved=True)
    moved = X.transforms(X.SEED, moved=True)
    scene = X.build("big", X.SEED, gpu_ctx)                              # a scene of its own: it is changed in place
    grid = grid_over(*scene_box(c), (3, 4, 2))
    rec = batch("big", grid, moved=True)
    sh = np.random.default_rng(7).normal(size=(24, 9, 4)).astype(np.float32)
    before = lookup(gpu_ctx, scene, grid, sh, rec, None, True, True, 1e-3, 0.0)
    scene.update_instances(X.instance_records(moved), tlas_builder=tlas_builder)
    fresh = X.build("big", X.SEED, gpu_ctx, xf=moved)
    after = lookup(gpu_ctx, scene, grid, sh, rec, None, True, True, 1e-3, 0.0)
    assert np.array_equal(words(after), words(lookup(gpu_ctx, fresh, grid, sh, rec, None, True, True, 1e-3, 0.0)))
    want, _ = expected(gpu_ctx, fresh, grid, sh, rec, None, True, True, 1e-3, 0.0)
    assert np.array_equal(words(after), words(want))
    assert int((words(before) != words(after)).any(axis=1).sum()) > 20  # the move is visible to these points


# ---- 8. refusals ---------------------------------------------------------------------------------------------------

def device_lookup(ctx, scene, desc_fields, sh, valid, rec, sentinel=None, offsets=(0, 0, 0, 0)):
    """lupin_hip_sample_probe_grid with LUPIN_PROBE_GRID_DEVICE_POINTERS on texture memory: (status, out).  offsets: bytes
    added to the sh, valid, records and out pointers (the arrays are placed that far into their allocations)."""
    n = len(rec)

    def place(a, off):
        raw = np.concatenate([np.zeros(off, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1)])
        return DeviceArray(ctx, len(raw)).upload(raw)

    d_sh, d_rec = place(sh, offsets[0]), place(rec, offsets[2])
    d_valid = place(valid, offsets[1]) if valid is not None else None
    d_out = place(np.full(n * 4, SENTINEL if sentinel is None else sentinel, np.float32), offsets[3])
    f = dict(desc_fields)
    f["flags"] = f["flags"] | api.PROBE_GRID_DEVICE_POINTERS
    rc = _abi.lib().lupin_hip_sample_probe_grid(ctx.handle, scene.handle, C.byref(make_desc(**f)), C.c_void_p(d_sh.ptr + offsets[0]),
                                                C.c_void_p(d_valid.ptr + offsets[1]) if d_valid else None, n, C.c_void_p(d_rec.ptr + offsets[2]),
                                                C.c_void_p(d_out.ptr + offsets[3]))
    return rc, d_out.download(np.uint8, offsets[3] + n * 16)[offsets[3]:].view(np.float32).reshape(n, 4)


def make_desc(origin=(0, 0, 0), spacing=(1, 1, 1), dims=(2, 2, 2), flags=api.PROBE_GRID_VISIBILITY | api.PROBE_GRID_BACKFACE, eps=1e-3, bias=0.0):
    return _abi.ProbeGridDescC((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_uint32 * 3)(*dims), flags, eps, bias)


def test_every_refusal_leaves_the_output_untouched(gpu_ctx):
    c = X.case("small")
    scene = device_scene(gpu_ctx, "small")
    lo, hi = scene_box(c)
    origin, spacing, dims = grid_over(lo, hi, (2, 2, 2))
    base = dict(origin=tuple(origin), spacing=tuple(spacing), dims=dims)
    rec = batch("small", (origin, spacing, dims))[:64].copy()
    sh = np.random.default_rng(8).normal(size=(8, 9, 4)).astype(np.float32)
    lib = _abi.lib()
    INVALID = -1
    g, s = gpu_ctx.handle, scene.handle

    def raw(ctx_h, scene_h, desc, sh_, n, records, out, **over):
        f = dict(base); f.update(over)
        return lib.lupin_hip_sample_probe_grid(ctx_h, scene_h, C.byref(make_desc(**f)) if desc else None, _abi.ptr(sh_), None, n, _abi.ptr(records), _abi.ptr(out))

    def fresh():
        return np.full((64, 4), SENTINEL, np.float32)

    cases = []
    out = fresh(); cases.append(("null context", raw(None, s, True, sh, 64, rec, out), out))
    out = fresh(); cases.append(("null scene", raw(g, None, True, sh, 64, rec, out), out))
    out = fresh(); cases.append(("null desc", raw(g, s, False, sh, 64, rec, out), out))
    out = fresh(); cases.append(("null sh", raw(g, s, True, None, 64, rec, out), out))
    out = fresh(); cases.append(("null records", raw(g, s, True, sh, 64, None, out), out))
    out = fresh(); cases.append(("null out", raw(g, s, True, sh, 64, rec, None), out))
    out = fresh(); cases.append(("unknown flag", raw(g, s, True, sh, 64, rec, out, flags=8), out))
    for k in range(3):
        for label, value in (("NaN", np.nan), ("infinite", np.inf)):
            o = list(base["origin"]); o[k] = value
            out = fresh(); cases.append((f"{label} origin {k}", raw(g, s, True, sh, 64, rec, out, origin=o), out))
        for label, value in (("NaN", np.nan), ("infinite", np.inf), ("zero", 0.0), ("negative", -1.0)):
            sp = list(base["spacing"]); sp[k] = value
            out = fresh(); cases.append((f"{label} spacing {k}", raw(g, s, True, sh, 64, rec, out, spacing=sp), out))
            d1 = [2, 2, 2]; d1[k] = 1                        # also on an axis with one probe
            out = fresh(); cases.append((f"{label} spacing {k}, one probe", raw(g, s, True, sh, 64, rec, out, spacing=sp, dims=d1), out))
        d0 = [2, 2, 2]; d0[k] = 0
        out = fresh(); cases.append((f"zero dim {k}", raw(g, s, True, sh, 64, rec, out, dims=d0), out))
    out = fresh(); cases.append(("more than 2^31 probes", raw(g, s, True, sh, 64, rec, out, dims=(1 << 16, 1 << 15, 2), spacing=(1e-3, 1e-3, 1e-3)), out))
    out = fresh(); cases.append(("more than 2^31 probes on one axis", raw(g, s, True, sh, 64, rec, out, dims=((1 << 31) + 1, 1, 1)), out))
    out = fresh(); cases.append(("last probe not finite", raw(g, s, True, sh, 64, rec, out, dims=(2, 1000, 2), spacing=(1.0, 3e38, 1.0)), out))
    for name in ("eps", "bias"):
        for label, value in (("NaN", np.nan), ("infinite", np.inf), ("negative", -1e-3)):
            out = fresh(); cases.append((f"{label} {name}", raw(g, s, True, sh, 64, rec, out, **{name: value}), out))
    out = fresh(); cases.append(("n above 2^38", raw(g, s, True, sh, (1 << 38) + 1, rec, out), out))
    other = api.Context(0)
    foreign = X.build("small", X.SEED, other)
    out = fresh(); cases.append(("scene of another context", raw(g, foreign.handle, True, sh, 64, rec, out), out))
    other.close()
    out = fresh(); cases.append(("scene of a destroyed context", raw(g, foreign.handle, True, sh, 64, rec, out), out))
    bad_records = {}
    for label, row, col, value in (("NaN point", 17, 1, np.nan), ("infinite point", 0, 0, np.inf), ("infinite normal", 17, 5, np.inf), ("NaN normal", 63, 6, np.nan)):
        r = rec.copy(); r[row, col] = value
        bad_records[label] = r
    r = rec.copy(); r[40, 4:7] *= np.float32(1.001)
    bad_records["normal too long"] = r
    r = rec.copy(); r[3, 4:7] = 0.0
    bad_records["zero normal"] = r
    flags = api.PROBE_GRID_VISIBILITY | api.PROBE_GRID_BACKFACE
    for label, r in bad_records.items():
        for fl in (flags, 0):
            out = fresh(); cases.append((f"{label} (host check, flags {fl})", raw(g, s, True, sh, 64, r, out, flags=fl), out))
            rc, dout = device_lookup(gpu_ctx, scene, dict(base, flags=fl), sh, None, r)
            cases.append((f"{label} (device check, flags {fl})", rc, dout))
    assert lib.lupin_hip_last_error().decode().startswith("1 record(s): ")
    for label, offs in (("sh", (8, 0, 0, 0)), ("records", (0, 0, 8, 0)), ("out", (0, 0, 0, 4))):
        rc, dout = device_lookup(gpu_ctx, scene, dict(base, flags=flags), sh, None, rec, offsets=offs)
        cases.append((f"misaligned device pointer: {label}", rc, dout))
    # a hierarchy too deep for the stack: 200 triangles in a chain (tests/test_gpu_ray_query.py)
    cpu = api.SceneCPU()
    cpu.materials = np.array([api.default_material()], _abi.MATERIAL_DTYPE)
    T = 200
    v = np.zeros((3 * T, 4), np.float32)
    for t in range(T):
        v[3 * t:3 * t + 3, :3] = [(t, 0, 0), (t + 0.9, 0, 0), (t, 0.9, 0)]
    cpu.verts_pos_array.append(v)
    cpu.indices_array.append(np.arange(3 * T, dtype=np.uint32))
    cpu.mesh_infos = np.array([api.default_mesh_info()], _abi.MESH_INFO_DTYPE)
    cpu.instances = np.array([api.default_instance()], _abi.INSTANCE_DTYPE)
    deep = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], [], True, blas_builder=chain_bvh)
    out = fresh(); cases.append(("hierarchy too deep, with visibility", raw(g, deep.handle, True, sh, 64, rec, out), out))
    assert "too deep" in lib.lupin_hip_last_error().decode()
    for label, rc, out in cases:
        assert rc == INVALID, (label, rc)
        assert np.all(out == SENTINEL), label
    assert len(cases) >= 80
    # accepted: without visibility the deep scene is not traversed at all
    out = fresh()
    assert raw(g, deep.handle, True, sh, 64, rec, out, flags=api.PROBE_GRID_BACKFACE) == 0
    assert np.array_equal(words(out), words(R.sample(origin, spacing, dims, sh, rec, backface=True)))
    # n == 0 touches nothing
    out = fresh()
    assert raw(g, s, True, sh, 0, rec, out) == 0 and np.all(out == SENTINEL)
    # the limits themselves: a normal within the tolerance, anything in floats 3 and 7, zero epsilon and bias
    r = rec.copy(); r[40, 4:7] *= np.float32(1.00004); r[5, 3] = np.nan; r[6, 7] = np.inf
    out = fresh()
    assert raw(g, s, True, sh, 64, r, out, eps=0.0, bias=0.0) == 0 and np.all(np.isfinite(out))
    # ... and 2^31 probes: a device grid of which only the first two are ever in reach of these points
    near = api.probe_grid_records(np.float32([[0.25, 5.0, -3.0], [-4.0, 0.0, 0.0], [0.75, 0.0, 0.0]]), np.float32([[0, 1, 0]] * 3))
    big = dict(origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), dims=(1 << 31, 1, 1), flags=0)
    rc, dout = device_lookup(gpu_ctx, scene, big, sh[:2], np.ones(2, np.uint8), near, offsets=(0, 1, 0, 0))      # valid: any alignment
    assert rc == 0 and np.array_equal(words(dout), words(R.sample((0, 0, 0), (1, 1, 1), (1 << 31, 1, 1), sh[:2], near)))
    # what follows is unharmed
    want, _ = expected(gpu_ctx, scene, (origin, spacing, dims), sh, rec, None, True, True, 1e-3, 0.0)
    assert np.array_equal(words(lookup(gpu_ctx, scene, (origin, spacing, dims), sh, rec, None, True, True, 1e-3, 0.0)), words(want))


# ---- 9. frames around a call --------------------------------------------------------------------------------------

def test_frames_around_a_lookup_do_not_notice_it(gpu_ctx):
    W, H = 64, 48
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cam = cams[0]
    rng = np.random.default_rng(9)
    nrm = rng.normal(size=(300, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rec = api.probe_grid_records(rng.uniform(-0.8, 0.8, (300, 3)) + [0.0, 1.0, 0.0], nrm)
    grid = (np.float32([-0.9, 0.1, -0.9]), np.float32([0.6, 0.6, 0.9]), (4, 4, 3))
    sh = rng.normal(size=(48, 9, 4)).astype(np.float32)
    alone = lookup(gpu_ctx, scene, grid, sh, rec, None, True, True, 1e-3, 0.0)

    def chain(call_after):
        res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=8, samples_per_pixel=2))
        out = api.DoubleBufferedTexture(gpu_ctx, W, H)
        for k in range(6):
            desc = api.PathtraceDesc(accum_params=api.AccumulationParams(out.back(), k), camera_params=cam.params, camera_transform=cam.transform)
            api.pathtrace_scene(gpu_ctx, res, scene, out.front(), PT.Standard, desc)
            out.flip()
            if k + 1 == call_after:
                assert np.array_equal(words(lookup(gpu_ctx, scene, grid, sh, rec, None, True, True, 1e-3, 0.0)), words(alone))
        out.flip()
        return out.front().download()

    plain = chain(None)
    assert util.f16_words_differ(chain(3), plain) == 0
    assert util.f16_words_differ(plain, util.oracle_accumulate(scene, cam, W, H, frames=6, spp=2)) == 0
    want, blocked = expected(gpu_ctx, scene, grid, sh, rec, None, True, True, 1e-3, 0.0)
    assert np.array_equal(words(alone), words(want)) and 0 < int(blocked.sum()) < blocked.size


# ---- 10. device memory in place -----------------------------------------------------------------------------------

def test_device_pointers_give_the_host_arrays_words(gpu_ctx):
    c = X.case("big")
    scene = device_scene(gpu_ctx, "big")
    grid = grid_over(*scene_box(c), (3, 4, 2))
    rec = batch("big", grid)
    rng = np.random.default_rng(10)
    sh = rng.normal(size=(24, 9, 4)).astype(np.float32)
    valid = (rng.uniform(size=24) > 0.33).astype(np.uint8)
    for v, voff in ((None, 0), (valid, 0), (valid, 3)):
        for fl in (0, api.PROBE_GRID_VISIBILITY | api.PROBE_GRID_BACKFACE):
            for n in (9, 1000):
                f = dict(origin=tuple(grid[0]), spacing=tuple(grid[1]), dims=grid[2], flags=fl, eps=1e-3, bias=0.0)
                rc, got = device_lookup(gpu_ctx, scene, f, sh, v, rec[:n], offsets=(0, voff, 0, 0))
                assert rc == 0
                assert np.array_equal(words(got), words(lookup(gpu_ctx, scene, grid, sh, rec[:n], v, fl != 0, fl != 0, 1e-3, 0.0))), (voff, fl, n)


def test_torch_tensors_give_the_same_words():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_probe_grid_torch_worker.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "PROBE GRID TORCH OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
