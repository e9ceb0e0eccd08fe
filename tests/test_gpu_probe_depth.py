"""Probe depth maps on the device (lupin_hip_bake_probe_depth, lupin_hip_sample_probe_grid_depth) against
tests/probe_depth_ref.py WORD FOR WORD: the bake fed with api.trace_rays' distances for the same directions, every texel
and the border, over staged and global geometry, resolutions that make probes straddle waves and blocks, every sub-sample
count, caps that bind and caps that do not, and launches of 64 rays; the stats against counts formed from api.trace_rays and
api.surface_probe; the lookup against the restatement on the device-baked maps.  Then the properties: no light through a
wall, a scene without a software BVH, moved instances, device memory in place, torch tensors, every refusal, frames around
the calls."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import closest_hit_ref as X
from tests import probe_depth_ref as D
from tests import probe_grid_ref as G
from tests import util
from tests.test_gpu_closest_hit import device_scene, staged_in_lds
from tests import test_gpu_probe_grid as PG
from tests.test_gpu_probe_grid import grid_over, scene_box, wall, words
from tests.test_gpu_ray_query import DeviceArray, chain_bvh
from tests.test_probe_depth_cpu import assert_no_light_through_the_wall, cube, wall_inputs, WALL_GRID

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SENTINEL = np.float32(-7.0)
SHAPES = ((2, 1), (4, 1), (4, 8), (6, 2), (5, 4), (16, 4))       # (R, K); R = 6 and R = 5 make probes straddle waves and blocks
PROBES = (1, 2, 3, 5, 17)
COUNTS = (1, 7, 8, 9, 63, 64, 65, 1000)
GRIDS = ((2, 2, 2), (1, 1, 1), (4, 1, 3))
_cache = {}


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


def batch(kind, grid, moved=False):
    """tests/test_gpu_probe_grid.py's 1000 records (surface points, points outside the box, points exactly on probes) for THIS
    grid: that module keeps its batches by dims alone, so its entry is put back as it was."""
    key = ("batch", kind, moved, grid[2], np.asarray(grid[0], F).tobytes(), np.asarray(grid[1], F).tobytes())
    if key not in _cache:
        theirs = (kind, grid[2], moved)
        saved = PG._cache.pop(theirs, None)
        try:
            _cache[key] = PG.batch(kind, grid, moved)
        finally:
            PG._cache.pop(theirs, None)
            if saved is not None:
                PG._cache[theirs] = saved
    return _cache[key]


def probe_positions(kind, moved=False):
    """17 probes: the box's centre, a point outside the box, a vertex of the scene, then points in and around the box."""
    key = ("positions", kind, moved)
    if key not in _cache:
        c = X.case(kind, moved)
        lo, hi = scene_box(c)
        rng = np.random.default_rng(31)
        l2w = c.g.local_to_world()
        vertex = c.g.meshes[c.g.mesh_idx[1]].verts[0] @ l2w[1][:, :3].T + l2w[1][:, 3]
        rest = lo + rng.uniform(-0.3, 1.3, (14, 3)) * (hi - lo)
        _cache[key] = np.concatenate([[(lo + hi) / 2], [lo - 1.0], [vertex], rest]).astype(F)
    return _cache[key]


def traced(ctx, scene, pos, R, K, eps):
    """api.trace_rays for every slot of the probes: (hit, dst, inst, tri, uv) shaped (n, S, ...), and the directions."""
    w = D.directions(R, K)
    hit, dst, uv, inst, tri = api.trace_rays(ctx, scene, np.repeat(pos, len(w), axis=0), np.tile(w, (len(pos), 1)), eps)
    n = len(pos)
    return hit.reshape(n, -1), dst.reshape(n, -1), inst.reshape(n, -1), tri.reshape(n, -1), uv.reshape(n, -1, 2), w


def expected_stats(ctx, scene, pos, R, K, eps, maxd):
    hit, dst, inst, tri, uv, w = traced(ctx, scene, pos, R, K, eps)
    rec = api.surface_records(api.SurfaceMode.NORMAL, inst.reshape(-1), tri.reshape(-1), uv.reshape(-1, 2))
    g = api.surface_probe(ctx, scene, rec)[:, 3:6].reshape(len(pos), -1, 3)
    return D.stats(hit, dst, w, g, maxd), hit, dst


# ---- 1. the bake, word for word -----------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "R%dK%d" % s)
@pytest.mark.parametrize("kind", ["small", "big"])
def test_bake_word_for_word_against_the_restatement(gpu_ctx, kind, shape):
    R, K = shape
    scene = device_scene(gpu_ctx, kind)
    assert staged_in_lds(gpu_ctx, scene) == (kind == "small")
    pos = probe_positions(kind)
    extent = float(np.ptp(np.stack(scene_box(X.case(kind))), axis=0).max())
    capped_some = capped_none = calls = 0
    for eps in (0.0, 1e-3):
        hit, dst = traced(gpu_ctx, scene, pos, R, K, eps)[:2]
        assert 0 < hit.sum() < hit.size
        for maxd in (0.2 * extent, 100.0 * extent):
            want = D.bake(hit, dst, R, K, maxd)
            over = int((hit != 0).sum() - ((hit != 0) & (dst <= F(maxd))).sum())
            capped_some += over if maxd < extent else 0
            capped_none += over if maxd > extent else 0
            for n in PROBES:
                for max_slots in (64, 0):
                    got = api.bake_probe_depth(gpu_ctx, scene, pos[:n], R, K, max_distance=maxd, ray_epsilon=eps, max_slots=max_slots)
                    assert got.shape == (n, R + 2, R + 2, 2) and got.dtype == np.float32
                    diff = np.argwhere(words(got) != words(want[:n]))
                    assert len(diff) == 0, (kind, shape, eps, maxd, n, max_slots, diff[:5])
                    calls += 1
    assert calls == 2 * 2 * len(PROBES) * 2 and capped_some > 0 and capped_none == 0


# ---- 2. the stats, word for word ------------------------------------------------------------------------------------

def two_cubes(ctx):
    """A closed cube at the origin and its mirror image (x -> -x) at x = 5: the mirrored instance's normals turn round."""
    if "cubes" not in _cache:
        v, t = cube(1.0)
        verts = np.zeros((8, 4), F)
        verts[:, :3] = v
        cpu = api.SceneCPU()
        cpu.materials = np.array([api.default_material()], _abi.MATERIAL_DTYPE)
        cpu.verts_pos_array.append(verts)
        cpu.indices_array.append(t.reshape(-1).astype(np.uint32))
        cpu.mesh_infos = np.array([api.default_mesh_info()], _abi.MESH_INFO_DTYPE)
        xf = [(np.eye(3), np.zeros(3)), (np.diag([-1.0, 1.0, 1.0]), np.array([5.0, 0.0, 0.0]))]
        cpu.instances = np.array([api.instance_from_transform(X.mat3x4(M, b), 0, 0) for M, b in xf], api.INSTANCE_DTYPE)
        api.validate_scene(cpu, 0, 0)
        _cache["cubes"] = api.build_accel_structures_and_upload(ctx, cpu, [], [], True)
    return _cache["cubes"]


def test_stats_word_for_word(gpu_ctx):
    scene = two_cubes(gpu_ctx)
    pos = F([[0.1, 0.2, -0.1], [2.5, 0.3, 0.2], [5.1, 0.0, 0.1], [2.5, 7.0, 0.0]])     # inside | between | inside the mirror image | above both
    for R, K in ((5, 4), (6, 2), (4, 1), (16, 4)):
        for maxd in (0.95, 50.0):
            want, hit, dst = expected_stats(gpu_ctx, scene, pos, R, K, 1e-3, maxd)
            for max_slots in (64, 0):
                maps, got = api.bake_probe_depth(gpu_ctx, scene, pos, R, K, max_distance=maxd, ray_epsilon=1e-3, want_stats=True, max_slots=max_slots)
                assert got.dtype == np.uint32 and np.array_equal(got, want), (R, K, maxd, max_slots, got, want)
                assert np.array_equal(words(maps), words(D.bake(hit, dst, R, K, maxd)))                 # the maps do not notice the stats
            S = R * R * K * K
            assert np.all(want[:, 0] == S) and want[0, 1] == S and want[2, 1] == S and 0 < want[1, 1] < S
            # inside a closed mesh every hit is on one side -- for the mirror image too -- and from outside on the other (but for
            # the odd ray that slips in along an edge)
            assert want[0, 2] in (0, S) and want[2, 2] == want[0, 2]
            assert abs(int(want[1, 2]) - (int(want[1, 1]) if want[0, 2] == 0 else 0)) <= 0.01 * want[1, 1]
            assert want[3, 3] == (F(maxd).view(np.uint32) if maxd < 1 else want[3, 3]) and np.all(want[:, 3] <= F(maxd).view(np.uint32))


# ---- 3. the lookup, word for word -----------------------------------------------------------------------------------

def lookup(ctx, scene, grid, sh, maps, rec, maxd, valid, back, bias):
    return api.sample_probe_grid_depth(ctx, scene, *grid, sh, maps, rec, max_distance=maxd, valid=valid, backface=back, normal_bias=bias)


@pytest.mark.parametrize("dims", GRIDS)
@pytest.mark.parametrize("kind", ["small", "big"])
def test_lookup_word_for_word_against_the_restatement(gpu_ctx, kind, dims):
    c = X.case(kind)
    scene = device_scene(gpu_ctx, kind)
    lo, hi = scene_box(c)
    grid = grid_over(lo + F(0.3) * (hi - lo), hi - F(0.3) * (hi - lo), dims)          # probes among the instances, points also outside the grid
    rec = batch(kind, grid)
    P = int(np.prod(dims))
    R, K = 6, 2
    pos, baked, maxd = api.bake_probe_grid_depth(gpu_ctx, scene, *grid, R, K)
    assert maxd == api.probe_grid_depth_max_distance(grid[1]) and baked.shape == (P, R + 2, R + 2, 2)
    assert np.array_equal(words(baked), words(api.bake_probe_depth(gpu_ctx, scene, pos, R, K, max_distance=maxd)))
    rng = np.random.default_rng(2000 + 10 * GRIDS.index(dims) + (kind == "big"))
    sh = rng.normal(size=(P, 9, 4)).astype(F)
    some_valid = (rng.uniform(size=P) > 0.33).astype(np.uint8)
    default_bias = api.LIGHTMAP_OFFSET_FRACTION * api.scene_world_extent(scene)
    # the scene is sparse and few corners lie behind what their probe sees: maps of the same shape with surfaces close to
    # every probe put every branch of the test to work; every third probe sees one distance in all directions, without
    # variance (its interpolated moments are that texel's, m2 - m1 * m1 is exactly 0 and vis with it)
    dense = np.empty_like(baked)
    dense[..., 0] = rng.uniform(0.05, 0.6, baked.shape[:-1]) * maxd
    dense[..., 1] = dense[..., 0] * dense[..., 0] + rng.uniform(0.0, 0.05 * maxd * maxd, baked.shape[:-1])
    dense[::3, ..., 0] = F(0.03125) * maxd
    dense[::3, ..., 1] = dense[::3, ..., 0] * dense[::3, ..., 0]
    for maps, name in ((baked, "baked"), (dense, "dense")):
        tested = shut = 0
        for valid in (None, some_valid):
            for bias in (0.0, default_bias):
                for back in (False, True):
                    want = D.sample(*grid, sh, maps, rec, maxd, valid=valid, backface=back, normal_bias=bias)
                    vis, was = D.visibility(G.corners(*grid, rec, bias, valid, back), maps, R, maxd)
                    tested, shut = tested + int(was.sum()), shut + int((was & (vis == 0)).sum())
                    for n in COUNTS:
                        got = lookup(gpu_ctx, scene, grid, sh, maps, rec[:n], maxd, valid, back, bias)
                        assert got.shape == (n, 4) and got.dtype == np.float32
                        diff = np.nonzero((words(got) != words(want[:n])).any(axis=1))[0]
                        assert len(diff) == 0, (kind, dims, name, valid is not None, bias, back, n, diff[:5], got[diff[:5]], want[diff[:5]])
        assert tested > (50 if name == "baked" else 2000), (name, tested)       # r > m1 was taken
        assert name == "baked" or shut > 100, (name, shut)                       # ... and corners were shut by vis == 0


@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 1, 1), (3, 2, 2)])
def test_maps_that_say_nothing_give_the_untraced_lookups_words(gpu_ctx, dims):
    """Every texel (max_distance, max_distance^2): the bilinear mean is max_distance exactly (m + g * (m - m)), r =
    min(len, max_distance) > m1 never holds and no corner is weighed -- what is left is what the two lookups share, so
    sample_probe_grid_depth equals sample_probe_grid(visibility=False) in every word.  (1, 1, 1): all fractions 0, seven
    corners skipped; (2, 1, 1): two degenerate axes; (3, 2, 2): a cell index that is not 0."""
    c = X.case("small")
    scene = device_scene(gpu_ctx, "small")
    lo, hi = scene_box(c)
    grid = grid_over(lo + F(0.3) * (hi - lo), hi - F(0.3) * (hi - lo), dims)
    P, R = int(np.prod(dims)), 2
    pos = api.probe_grid_positions(*grid)
    rec = batch("small", grid)[:65].copy()          # surface points inside and outside the grid, and
    rec[1, :3], rec[5, :3], rec[64, :3] = pos[0], pos[-1], pos[P // 2]          # ... points on probes (len == 0 with no bias),
    rec[2, :3], rec[7, :3] = lo - F(1.0), hi + F(2.5)                           # ... and outside the scene's box
    maxd = api.probe_grid_depth_max_distance(grid[1])
    maps = np.empty((P, R + 2, R + 2, 2), F)
    maps[..., 0], maps[..., 1] = maxd, maxd * maxd
    rng = np.random.default_rng(3000 + P)
    sh = rng.normal(size=(P, 9, 4)).astype(F)
    some_valid = np.ones(P, np.uint8)
    some_valid[::2] = 0
    for valid in (None, some_valid):
        for back in (False, True):
            cn = G.corners(*grid, rec, 0.0, valid, back)
            vis, was = D.visibility(cn, maps, R, maxd)
            assert not was.any() and np.all(vis == 1)
            want = G.sample(*grid, sh, rec, valid=valid, backface=back, blocked=None)
            from_maps = D.sample(*grid, sh, maps, rec, maxd, valid=valid, backface=back)
            assert np.array_equal(words(from_maps), words(want)), (dims, valid is not None, back)          # the restatements agree
            for n in (1, 9, 65):
                by_maps = lookup(gpu_ctx, scene, grid, sh, maps, rec[:n], maxd, valid, back, 0.0)
                untraced = api.sample_probe_grid(gpu_ctx, scene, *grid, sh, rec[:n], valid=valid, visibility=False, backface=back, normal_bias=0.0)
                for got, name in ((untraced, "sample_probe_grid"), (by_maps, "sample_probe_grid_depth")):
                    assert got.shape == (n, 4) and np.array_equal(words(got), words(want[:n])), (name, dims, valid is not None, back, n)


# ---- 4. properties --------------------------------------------------------------------------------------------------

def test_no_light_through_a_wall_on_the_device(gpu_ctx):
    scene = wall(gpu_ctx)
    pos, sh, dark, lit, maxd = wall_inputs()
    got_pos, maps, got_maxd = api.bake_probe_grid_depth(gpu_ctx, scene, *WALL_GRID, 16, 4)
    assert np.array_equal(got_pos, pos) and got_maxd == maxd
    assert_no_light_through_the_wall(lambda rec, back: lookup(gpu_ctx, scene, WALL_GRID, sh, maps, rec, maxd, None, back, 0.0), maps, sh, dark, lit, maxd)


def test_the_lookup_needs_no_software_bvh_and_no_shallow_hierarchy(gpu_ctx):
    c = X.case("small")
    scene = device_scene(gpu_ctx, "small")
    grid = grid_over(*scene_box(c), (2, 2, 2))
    rec = batch("small", grid)[:200]
    pos, maps, maxd = api.bake_probe_grid_depth(gpu_ctx, scene, *grid, 4, 2)
    sh = np.random.default_rng(41).normal(size=(8, 9, 4)).astype(F)
    want = D.sample(*grid, sh, maps, rec, maxd, backface=True)
    # lupin_hip_scene_create makes no scene without a TLAS (tests/test_gpu_reproject.py), so the scene whose hierarchy cannot
    # be traversed is the one too deep for the stack: the bake refuses it, the lookup never reads it
    with pytest.raises(api.LupinError) as e:
        api.bake_probe_depth(gpu_ctx, deep_scene(gpu_ctx), pos, 4, 2, max_distance=maxd)
    assert e.value.code == -1 and "too deep" in str(e.value)
    assert np.array_equal(words(lookup(gpu_ctx, deep_scene(gpu_ctx), grid, sh, maps, rec, maxd, None, True, 0.0)), words(want))


def deep_scene(ctx):
    """200 triangles in a chain (tests/test_gpu_ray_query.py): a hierarchy too deep for the traversal stack."""
    if "deep" not in _cache:
        cpu = api.SceneCPU()
        cpu.materials = np.array([api.default_material()], _abi.MATERIAL_DTYPE)
        T = 200
        v = np.zeros((3 * T, 4), F)
        for t in range(T):
            v[3 * t:3 * t + 3, :3] = [(t, 0, 0), (t + 0.9, 0, 0), (t, 0.9, 0)]
        cpu.verts_pos_array.append(v)
        cpu.indices_array.append(np.arange(3 * T, dtype=np.uint32))
        cpu.mesh_infos = np.array([api.default_mesh_info()], _abi.MESH_INFO_DTYPE)
        cpu.instances = np.array([api.default_instance()], _abi.INSTANCE_DTYPE)
        _cache["deep"] = api.build_accel_structures_and_upload(ctx, cpu, [], [], True, blas_builder=chain_bvh)
    return _cache["deep"]


def test_staged_and_global_geometry_bake_the_same_words(gpu_ctx, global_ctx):
    staged, unstaged = device_scene(gpu_ctx, "small"), X.build("small", X.SEED, global_ctx)
    assert staged_in_lds(gpu_ctx, staged) and not staged_in_lds(global_ctx, unstaged)
    pos = probe_positions("small")
    for R, K in ((5, 4), (6, 2)):
        a = api.bake_probe_depth(gpu_ctx, staged, pos, R, K, max_distance=3.0, want_stats=True)
        b = api.bake_probe_depth(global_ctx, unstaged, pos, R, K, max_distance=3.0, want_stats=True)
        assert np.array_equal(words(a[0]), words(b[0])) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("tlas_builder", ["cpu", "device"])
def test_after_update_instances_the_bake_equals_a_fresh_scenes(gpu_ctx, tlas_builder):
    moved = X.transforms(X.SEED, moved=True)
    scene = X.build("big", X.SEED, gpu_ctx)                              # a scene of its own: it is changed in place
    pos = probe_positions("big", moved=True)
    before = api.bake_probe_depth(gpu_ctx, scene, pos, 6, 2, max_distance=4.0)
    scene.update_instances(X.instance_records(moved), tlas_builder=tlas_builder)          # (the four-wide hierarchy is stale from here on)
    fresh = X.build("big", X.SEED, gpu_ctx, xf=moved)
    after = api.bake_probe_depth(gpu_ctx, scene, pos, 6, 2, max_distance=4.0, want_stats=True)
    want = api.bake_probe_depth(gpu_ctx, fresh, pos, 6, 2, max_distance=4.0, want_stats=True)
    assert np.array_equal(words(after[0]), words(want[0])) and np.array_equal(after[1], want[1])
    hit, dst = traced(gpu_ctx, fresh, pos, 6, 2, 1e-3)[:2]
    assert np.array_equal(words(after[0]), words(D.bake(hit, dst, 6, 2, 4.0)))
    assert int((words(before) != words(after[0])).sum()) > 100           # the move is visible to these probes


# ---- 5. device memory in place ------------------------------------------------------------------------------------

def place(ctx, a, off=0):
    raw = np.concatenate([np.zeros(off, np.uint8), np.ascontiguousarray(a).view(np.uint8).reshape(-1)])
    return DeviceArray(ctx, len(raw)).upload(raw)


def device_bake(ctx, scene, pos, R, K, eps, maxd, stats=True, max_slots=0, offsets=(0, 0, 0), flags=api.PROBE_DEPTH_DEVICE_POINTERS):
    """lupin_hip_bake_probe_depth on texture memory: (status, maps, stats); offsets: bytes added to the three pointers."""
    n = len(pos)
    p4 = np.zeros((n, 4), F)
    p4[:, :3] = pos
    side = R + 2
    d_pos = place(ctx, p4, offsets[0])
    d_out = place(ctx, np.full(n * side * side * 2, SENTINEL, F), offsets[1])
    d_stats = place(ctx, np.full(n * 4, 0xDEADBEEF, np.uint32), offsets[2])
    desc = _abi.ProbeDepthDescC(R, K, flags, max_slots, eps, maxd)
    rc = _abi.lib().lupin_hip_bake_probe_depth(ctx.handle, scene.handle, C.byref(desc), n, C.c_void_p(d_pos.ptr + offsets[0]),
                                               C.c_void_p(d_out.ptr + offsets[1]), C.c_void_p(d_stats.ptr + offsets[2]) if stats else None)
    maps = d_out.download(np.uint8, offsets[1] + n * side * side * 8)[offsets[1]:].view(F).reshape(n, side, side, 2)
    return rc, maps, d_stats.download(np.uint8, offsets[2] + n * 16)[offsets[2]:].view(np.uint32).reshape(n, 4)


def device_lookup(ctx, scene, grid, R, maxd, sh, maps, rec, flags=0, offsets=(0, 0, 0, 0)):
    n = len(rec)
    d_sh, d_maps, d_rec = place(ctx, sh, offsets[0]), place(ctx, maps, offsets[1]), place(ctx, rec, offsets[2])
    d_out = place(ctx, np.full(n * 4, SENTINEL, F), offsets[3])
    gd = _abi.ProbeGridDescC((C.c_float * 3)(*grid[0]), (C.c_float * 3)(*grid[1]), (C.c_uint32 * 3)(*grid[2]), flags | api.PROBE_GRID_DEVICE_POINTERS, 0.0, 0.0)
    rc = _abi.lib().lupin_hip_sample_probe_grid_depth(ctx.handle, scene.handle, C.byref(_abi.ProbeGridDepthDescC(gd, R, maxd)),
                                                      C.c_void_p(d_sh.ptr + offsets[0]), C.c_void_p(d_maps.ptr + offsets[1]), None, n,
                                                      C.c_void_p(d_rec.ptr + offsets[2]), C.c_void_p(d_out.ptr + offsets[3]))
    return rc, d_out.download(np.uint8, offsets[3] + n * 16)[offsets[3]:].view(F).reshape(n, 4)


def test_device_pointers_give_the_host_arrays_words(gpu_ctx):
    c = X.case("big")
    scene = device_scene(gpu_ctx, "big")
    pos = probe_positions("big")
    for R, K in ((5, 4), (6, 2)):
        want = api.bake_probe_depth(gpu_ctx, scene, pos, R, K, max_distance=3.0, want_stats=True)
        for max_slots in (64, 0):
            rc, maps, stats = device_bake(gpu_ctx, scene, pos, R, K, 1e-3, 3.0, max_slots=max_slots)
            assert rc == 0 and np.array_equal(words(maps), words(want[0])) and np.array_equal(stats, want[1])
        rc, maps, stats = device_bake(gpu_ctx, scene, pos, R, K, 1e-3, 3.0, stats=False, offsets=(0, 8, 0))          # maps: 8-byte aligned
        assert rc == 0 and np.array_equal(words(maps), words(want[0])) and np.all(stats == 0xDEADBEEF)
    grid = grid_over(*scene_box(c), (2, 2, 2))
    rec = batch("big", grid)
    _, gmaps, maxd = api.bake_probe_grid_depth(gpu_ctx, scene, *grid, 6, 2)
    sh = np.random.default_rng(51).normal(size=(8, 9, 4)).astype(F)
    for back in (0, api.PROBE_GRID_BACKFACE):
        for n in (9, 1000):
            rc, got = device_lookup(gpu_ctx, scene, grid, 6, maxd, sh, gmaps, rec[:n], flags=back, offsets=(0, 8, 0, 0))
            assert rc == 0 and np.array_equal(words(got), words(lookup(gpu_ctx, scene, grid, sh, gmaps, rec[:n], maxd, None, back != 0, 0.0)))


def test_torch_tensors_give_the_same_words():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_probe_depth_torch_worker.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "PROBE DEPTH TORCH OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- 6. refusals ----------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_sentinels_in_all_outputs(gpu_ctx):
    scene = device_scene(gpu_ctx, "small")
    lib = _abi.lib()
    g, s = gpu_ctx.handle, scene.handle
    pos = np.zeros((5, 4), F)
    pos[:, :3] = probe_positions("small")[:5]
    R, K = 4, 2
    INVALID = -1

    def bake(ctx_h, scene_h, desc, p, out, stats, n=5, **over):
        f = dict(resolution=R, subsamples=K, flags=0, max_slots=0, ray_epsilon=1e-3, max_distance=2.0)
        f.update(over)
        d = _abi.ProbeDepthDescC(f["resolution"], f["subsamples"], f["flags"], f["max_slots"], f["ray_epsilon"], f["max_distance"])
        return lib.lupin_hip_bake_probe_depth(ctx_h, scene_h, C.byref(d) if desc else None, n, _abi.ptr(p), _abi.ptr(out), _abi.ptr(stats))

    cases = []

    def refuse(label, *args, **over):
        side = over.get("side", 66)
        over.pop("side", None)
        out, stats = np.full((5, side, side, 2), SENTINEL, F), np.full((5, 4), 0xDEADBEEF, np.uint32)
        a = [out if isinstance(x, str) and x == "out" else stats if isinstance(x, str) and x == "stats" else x for x in args]
        cases.append((label, bake(*a, **over), out, stats))

    refuse("null context", None, s, True, pos, "out", "stats")
    refuse("null scene", g, None, True, pos, "out", "stats")
    refuse("null desc", g, s, False, pos, "out", "stats")
    refuse("null positions", g, s, True, None, "out", "stats")
    refuse("null out", g, s, True, pos, None, "stats")
    refuse("unknown flag", g, s, True, pos, "out", "stats", flags=2)
    for r in (0, 1, 65, 1 << 31):
        refuse(f"resolution {r}", g, s, True, pos, "out", "stats", resolution=r)
    for k in (0, 3, 5, 6, 7, 16):
        refuse(f"subsamples {k}", g, s, True, pos, "out", "stats", subsamples=k)
    for label, v in (("NaN", np.nan), ("infinite", np.inf), ("negative", -1e-3)):
        refuse(f"{label} ray_epsilon", g, s, True, pos, "out", "stats", ray_epsilon=v)
    for label, v in (("NaN", np.nan), ("infinite", np.inf), ("zero", 0.0), ("negative", -1.0)):
        refuse(f"{label} max_distance", g, s, True, pos, "out", "stats", max_distance=v)
    refuse("n * rays above 2^38", g, s, True, pos, "out", "stats", n=(1 << 38) // (R * R * K * K) + 1)
    for label, row, col, v in (("NaN position", 3, 1, np.nan), ("infinite position", 0, 0, np.inf), ("-infinite position", 4, 2, -np.inf)):
        p = pos.copy(); p[row, col] = v
        refuse(f"{label} (host check)", g, s, True, p, "out", "stats")
        rc, maps, stats = device_bake(gpu_ctx, scene, p[:, :3], R, K, 1e-3, 2.0)
        cases.append((f"{label} (device check)", rc, maps, stats))
    assert lib.lupin_hip_last_error().decode().startswith("1 position(s): ")
    for label, offs in (("positions", (8, 0, 0)), ("maps", (0, 4, 0)), ("stats", (0, 0, 8))):
        rc, maps, stats = device_bake(gpu_ctx, scene, pos[:, :3], R, K, 1e-3, 2.0, offsets=offs)
        cases.append((f"misaligned device pointer: {label}", rc, maps, stats))
    other = api.Context(0)
    foreign = X.build("small", X.SEED, other)
    refuse("scene of another context", g, foreign.handle, True, pos, "out", "stats")
    other.close()
    refuse("scene of a destroyed context", g, foreign.handle, True, pos, "out", "stats")
    refuse("hierarchy too deep", g, deep_scene(gpu_ctx).handle, True, pos, "out", "stats")
    assert "too deep" in lib.lupin_hip_last_error().decode()
    for label, rc, out, stats in cases:
        assert rc == INVALID, (label, rc)
        assert np.all(out == SENTINEL) and np.all(stats == 0xDEADBEEF), label
    assert len(cases) >= 35
    # accepted: n == 0 touches nothing; float 3 of a position is not looked at; the smallest and the largest of everything
    out, stats = np.full((5, 6, 6, 2), SENTINEL, F), np.full((5, 4), 0xDEADBEEF, np.uint32)
    assert bake(g, s, True, pos, out, stats, n=0) == 0 and np.all(out == SENTINEL) and np.all(stats == 0xDEADBEEF)
    p = pos.copy(); p[:, 3] = np.nan
    assert bake(g, s, True, p, out, None, ray_epsilon=0.0) == 0 and np.all(np.isfinite(out)) and np.all(stats == 0xDEADBEEF)
    assert np.array_equal(words(out), words(api.bake_probe_depth(gpu_ctx, scene, pos[:, :3], R, K, max_distance=2.0, ray_epsilon=0.0)))
    big = np.full((1, 66, 66, 2), SENTINEL, F)
    assert bake(g, s, True, pos, big, None, n=1, resolution=64, subsamples=8, max_slots=1) == 0 and np.all(big > 0)      # max_slots 1: launches of 64

    # ---- the lookup's
    grid = grid_over(*scene_box(X.case("small")), (2, 2, 2))
    rec = batch("small", grid)[:64].copy()
    sh = np.random.default_rng(61).normal(size=(8, 9, 4)).astype(F)
    maps = api.bake_probe_depth(gpu_ctx, scene, api.probe_grid_positions(*grid), R, K, max_distance=2.0)

    def look(ctx_h, scene_h, desc, sh_, maps_, records, out, n=64, **over):
        f = dict(origin=tuple(grid[0]), spacing=tuple(grid[1]), dims=grid[2], flags=api.PROBE_GRID_BACKFACE, eps=0.0, bias=0.0, resolution=R, max_distance=2.0)
        f.update(over)
        gd = _abi.ProbeGridDescC((C.c_float * 3)(*f["origin"]), (C.c_float * 3)(*f["spacing"]), (C.c_uint32 * 3)(*f["dims"]), f["flags"], f["eps"], f["bias"])
        d = _abi.ProbeGridDepthDescC(gd, f["resolution"], f["max_distance"])
        return lib.lupin_hip_sample_probe_grid_depth(ctx_h, scene_h, C.byref(d) if desc else None, _abi.ptr(sh_), _abi.ptr(maps_), None, n, _abi.ptr(records),
                                                     _abi.ptr(out))

    cases = []

    def refuse_lookup(label, *args, **over):
        out = np.full((64, 4), SENTINEL, F)
        cases.append((label, look(*[out if isinstance(x, str) else x for x in args], **over), out))

    refuse_lookup("null context", None, s, True, sh, maps, rec, "out")
    refuse_lookup("null scene", g, None, True, sh, maps, rec, "out")
    refuse_lookup("null desc", g, s, False, sh, maps, rec, "out")
    refuse_lookup("null sh", g, s, True, None, maps, rec, "out")
    refuse_lookup("null depth", g, s, True, sh, None, rec, "out")
    refuse_lookup("null records", g, s, True, sh, maps, None, "out")
    refuse_lookup("null out", g, s, True, sh, maps, rec, None)
    refuse_lookup("VISIBILITY", g, s, True, sh, maps, rec, "out", flags=api.PROBE_GRID_VISIBILITY)
    refuse_lookup("unknown flag", g, s, True, sh, maps, rec, "out", flags=8)
    for r in (0, 1, 65):
        refuse_lookup(f"resolution {r}", g, s, True, sh, maps, rec, "out", resolution=r)
    for label, v in (("NaN", np.nan), ("infinite", np.inf), ("zero", 0.0), ("negative", -1.0)):
        refuse_lookup(f"{label} max_distance", g, s, True, sh, maps, rec, "out", max_distance=v)
    refuse_lookup("NaN origin", g, s, True, sh, maps, rec, "out", origin=(np.nan, 0, 0))
    refuse_lookup("zero spacing", g, s, True, sh, maps, rec, "out", spacing=(1, 0, 1))
    refuse_lookup("zero dim", g, s, True, sh, maps, rec, "out", dims=(2, 0, 2))
    refuse_lookup("more than 2^31 probes", g, s, True, sh, maps, rec, "out", dims=(1 << 16, 1 << 15, 2))
    refuse_lookup("negative bias", g, s, True, sh, maps, rec, "out", bias=-1.0)
    refuse_lookup("NaN epsilon", g, s, True, sh, maps, rec, "out", eps=np.nan)
    refuse_lookup("n above 2^38", g, s, True, sh, maps, rec, "out", n=(1 << 38) + 1)
    refuse_lookup("scene of a destroyed context", g, foreign.handle, True, sh, maps, rec, "out")
    r = rec.copy(); r[17, 1] = np.nan
    refuse_lookup("NaN point (host check)", g, s, True, sh, maps, r, "out")
    rc, dout = device_lookup(gpu_ctx, scene, grid, R, 2.0, sh, maps, r)
    cases.append(("NaN point (device check)", rc, dout))
    r = rec.copy(); r[40, 4:7] *= F(1.001)
    refuse_lookup("normal too long", g, s, True, sh, maps, r, "out")
    for label, offs in (("sh", (8, 0, 0, 0)), ("depth", (0, 4, 0, 0)), ("records", (0, 0, 8, 0)), ("out", (0, 0, 0, 4))):
        rc, dout = device_lookup(gpu_ctx, scene, grid, R, 2.0, sh, maps, rec, offsets=offs)
        cases.append((f"misaligned device pointer: {label}", rc, dout))
    for label, rc, out in cases:
        assert rc == INVALID, (label, rc)
        assert np.all(out == SENTINEL), label
    assert len(cases) >= 30
    out = np.full((64, 4), SENTINEL, F)
    assert look(g, s, True, sh, maps, rec, out, n=0) == 0 and np.all(out == SENTINEL)
    # what follows is unharmed
    assert look(g, s, True, sh, maps, rec, out) == 0
    assert np.array_equal(words(out), words(D.sample(*grid, sh, maps, rec, 2.0, backface=True)))


UNKNOWN_FLAG = ("unknown flag", "unknown flag (LUPIN_PROBE_GRID_VISIBILITY belongs to lupin_hip_sample_probe_grid)")
BAD_GRIDS = {          # what both lookups refuse in a grid descriptor: the fields that differ from a good one, and the message
    "unknown flag bit": (dict(flags=8), UNKNOWN_FLAG),
    "NaN origin": (dict(origin=(0.0, np.nan, 0.0)), "origin must be finite"),
    "infinite origin": (dict(origin=(0.0, 0.0, -np.inf)), "origin must be finite"),
    "zero spacing": (dict(spacing=(1.0, 0.0, 1.0)), "spacing must be finite and positive"),
    "negative spacing": (dict(spacing=(-1.0, 1.0, 1.0)), "spacing must be finite and positive"),
    "NaN spacing": (dict(spacing=(1.0, 1.0, np.nan)), "spacing must be finite and positive"),
    "zero dim": (dict(dims=(2, 0, 2)), "a dimension is zero"),
    "more than 2^31 probes": (dict(dims=(1 << 16, 1 << 15, 2)), "the grid must not exceed 2^31 probes"),
    "non-finite last probe": (dict(spacing=(3e38, 1.0, 1.0), dims=(3, 1, 1)), "the grid's last probe position is not finite"),
    "NaN ray_epsilon": (dict(eps=np.nan), "ray_epsilon must be finite and not negative"),
    "negative normal_bias": (dict(bias=-1.0), "normal_bias must be finite and not negative"),
}


@pytest.mark.parametrize("label", BAD_GRIDS)
def test_one_bad_grid_descriptor_one_answer_from_both_lookups(gpu_ctx, label):
    over, message = BAD_GRIDS[label]
    scene = device_scene(gpu_ctx, "small")
    lib = _abi.lib()
    f = dict(origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), dims=(2, 2, 2), flags=api.PROBE_GRID_BACKFACE, eps=0.0, bias=0.0)
    rec = api.probe_grid_records([[0.5, 0.5, 0.5]], [[0.0, 0.0, 1.0]])
    sh, maps = np.ones((8, 9, 4), F), np.ones((8, 4, 4, 2), F)

    def both(**f):
        gd = _abi.ProbeGridDescC((C.c_float * 3)(*f["origin"]), (C.c_float * 3)(*f["spacing"]), (C.c_uint32 * 3)(*f["dims"]), f["flags"], f["eps"], f["bias"])
        outs = np.full((2, 1, 4), SENTINEL, F)
        rc = [lib.lupin_hip_sample_probe_grid(gpu_ctx.handle, scene.handle, C.byref(gd), _abi.ptr(sh), None, 1, _abi.ptr(rec), _abi.ptr(outs[0]))]
        said = [lib.lupin_hip_last_error().decode()]
        rc.append(lib.lupin_hip_sample_probe_grid_depth(gpu_ctx.handle, scene.handle, C.byref(_abi.ProbeGridDepthDescC(gd, 2, 2.0)), _abi.ptr(sh),
                                                        _abi.ptr(maps), None, 1, _abi.ptr(rec), _abi.ptr(outs[1])))
        said.append(lib.lupin_hip_last_error().decode())
        return rc, said, outs

    rc, said, outs = both(**f)
    assert rc == [0, 0] and not np.any(outs == SENTINEL)          # the good descriptor is accepted by both
    rc, said, outs = both(**dict(f, **over))
    assert rc == [-1, -1], (label, rc)
    assert tuple(said) == (message if isinstance(message, tuple) else (message, message)), (label, said)
    assert np.all(outs == SENTINEL), label


# ---- 7. frames around the calls -------------------------------------------------------------------------------------

def test_frames_around_a_bake_and_a_lookup_do_not_notice_them(gpu_ctx):
    W, H = 64, 48
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cam = cams[0]
    rng = np.random.default_rng(71)
    nrm = rng.normal(size=(300, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rec = api.probe_grid_records(rng.uniform(-0.8, 0.8, (300, 3)) + [0.0, 1.0, 0.0], nrm)
    grid = (F([-0.9, 0.1, -0.9]), F([0.6, 0.6, 0.9]), (4, 4, 3))
    sh = rng.normal(size=(48, 9, 4)).astype(F)
    _, maps, maxd = api.bake_probe_grid_depth(gpu_ctx, scene, *grid, 8, 2)
    alone = lookup(gpu_ctx, scene, grid, sh, maps, rec, maxd, None, True, 0.0)

    def chain(call_after):
        res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=8, samples_per_pixel=2))
        out = api.DoubleBufferedTexture(gpu_ctx, W, H)
        for k in range(6):
            desc = api.PathtraceDesc(accum_params=api.AccumulationParams(out.back(), k), camera_params=cam.params, camera_transform=cam.transform)
            api.pathtrace_scene(gpu_ctx, res, scene, out.front(), api.PathtraceType.Standard, desc)
            out.flip()
            if k + 1 == call_after:
                assert np.array_equal(words(api.bake_probe_grid_depth(gpu_ctx, scene, *grid, 8, 2)[1]), words(maps))
                assert np.array_equal(words(lookup(gpu_ctx, scene, grid, sh, maps, rec, maxd, None, True, 0.0)), words(alone))
        out.flip()
        return out.front().download()

    plain = chain(None)
    assert util.f16_words_differ(chain(3), plain) == 0
    assert util.f16_words_differ(plain, util.oracle_accumulate(scene, cam, W, H, frames=6, spp=2)) == 0
    want = D.sample(*grid, sh, maps, rec, maxd, backface=True)
    assert np.array_equal(words(alone), words(want))
    assert int((words(want) != words(G.sample(*grid, sh, rec, backface=True))).any(axis=1).sum()) > 0      # the maps matter to some
