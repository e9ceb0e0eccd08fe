"""Distance queries on the device (lupin_hip_distance_points, lupin_hip_bake_distance_grid): the float64
judgement of tests/distance_ref.py on closest_hit_ref's scenes (LDS-staged and global, and after instances moved), the
exact properties (the same words from LDS and global geometry, monotone in rmax, grid = points, signed = unsigned x side,
host = device pointers, moved = created anew), a closed form, and every refusal."""
import ctypes as C

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import closest_hit_ref as X
from tests import distance_ref as D
from tests.test_distance_cpu import case, leaky_case
from tests.test_gpu_closest_hit import device_scene, staged_in_lds
from tests.test_gpu_occlusion import global_ctx  # noqa: F401  (a context that reads every scene from global memory)
from tests.test_gpu_ray_query import DeviceArray

pytestmark = pytest.mark.gpu
CANARY = 0xABCDABCD
INV = -1                   # LUPIN_ERR_INVALID_ARGUMENT


def words(res):
    return np.ascontiguousarray(res).view(np.uint32).reshape(len(res), -1)


def judge(ctx, scene, kind, moved=False, rmax=np.inf):
    _, g, w, pts, fam, ref = case(kind, moved)
    if np.isfinite(np.asarray(rmax)).any():
        ref = D.nearest(w, pts, rmax)
    got = api.distance_points(ctx, scene, api.distance_records(pts, rmax))
    rep = D.compare(ref, w, pts, got)
    print(kind, moved, rep)
    for f, name in enumerate(D.FAMILIES):
        left, n = int((~ref.decisive[fam == f]).sum()), int((fam == f).sum())
        print(" family", name, n, "left out:", left, "=", left / n)
        assert 100 * left <= n                             # at most 1 %, counted in integers
    assert D.failures(rep) == [], rep
    assert (got["pad"] == 0).all()
    return got


@pytest.mark.parametrize("kind", ["big", "small"])
def test_float64_judgement(gpu_ctx, kind):
    scene = device_scene(gpu_ctx, kind)
    assert staged_in_lds(gpu_ctx, scene) == (kind == "small")
    got = judge(gpu_ctx, scene, kind)
    assert (got["found"] == 1).all()


def test_float64_judgement_with_a_radius(gpu_ctx):
    """rmax = 1.5 or 0.5 times the reference's distance: found and not found, each decisively.  (A point on a vertex has
    no distance to scale: its radius is 1.)"""
    _, _, _, pts, _, ref = case("big")
    rmax = np.where(ref.distance > 1e-3, ref.distance * np.where(np.arange(len(pts)) % 2, 1.5, 0.5), 1.0).astype(np.float32)
    got = judge(gpu_ctx, device_scene(gpu_ctx, "big"), "big", rmax=rmax)
    assert 0.4 < (got["found"] != 0).mean() < 0.6
    miss = got["found"] == 0
    assert (words(got)[miss] == 0).all()


def test_leaky_boxes_are_entered(gpu_ctx, global_ctx):  # noqa: F811
    """The family aimed at the triangles that stick out of a stored box above them, with rmax a quarter of the leak: a
    traversal that ignored WideNode.d.z would prune the box and report nothing (tests/test_distance_cpu.py shows it on the
    same node arrays).  From LDS-staged geometry and from global memory: node_flags has one reader for each."""
    _, g, w, pts, rmax, ref = leaky_case()
    res = []
    for ctx, lds in ((gpu_ctx, True), (global_ctx, False)):
        scene = D.leaky_scene(ctx)
        assert staged_in_lds(ctx, scene) == lds
        got = api.distance_points(ctx, scene, api.distance_records(pts, rmax))
        rep = D.compare(ref, w, pts, got)
        print("leaky", "lds" if lds else "global", rep)
        assert (got["found"] == 1).all() and D.failures(rep) == [], rep
        # ... and the scene's other queries are judged like any scene's
        more, _ = D.make_points(g, 5, dict(surface=300, uniform=200, far=0, vertex=20))
        ref2 = D.nearest(w, more)
        rep2 = D.compare(ref2, w, more, api.distance_points(ctx, scene, api.distance_records(more)))
        print(rep2)
        assert D.failures(rep2) == [], rep2
        res.append(words(got))
    assert np.array_equal(res[0], res[1])


@pytest.mark.parametrize("tlas_builder", ["cpu", "device"])
def test_after_update_instances_equals_a_scene_created_anew(gpu_ctx, tlas_builder):
    """Property (f), and the judgement on the moved scene."""
    _, _, _, pts, _, _ = case("big", True)
    scene = X.build("big", X.SEED, gpu_ctx, tlas_builder=tlas_builder)
    xf = X.transforms(X.SEED, True)
    scene.update_instances(X.instance_records(xf), tlas_builder=tlas_builder)
    got = judge(gpu_ctx, scene, "big", True)
    anew = api.distance_points(gpu_ctx, X.build("big", X.SEED, gpu_ctx, xf=xf, tlas_builder=tlas_builder), api.distance_records(pts))
    assert np.array_equal(words(got), words(anew))


def test_lds_and_global_geometry_give_the_same_words(gpu_ctx, global_ctx):  # noqa: F811
    """Property (a)."""
    _, _, _, pts, _, _ = case("small")
    rec = api.distance_records(pts)
    a = api.distance_points(gpu_ctx, device_scene(gpu_ctx, "small"), rec)
    scene_g = device_scene(global_ctx, "small")
    assert not staged_in_lds(global_ctx, scene_g)
    b = api.distance_points(global_ctx, scene_g, rec)
    assert np.array_equal(words(a), words(b))
    o, s, dims = [-7.0, -7.0, -7.0], [0.9, 1.1, 1.3], (17, 5, 3)
    assert np.array_equal(api.bake_distance_grid(gpu_ctx, device_scene(gpu_ctx, "small"), o, s, dims).view(np.uint32),
                          api.bake_distance_grid(global_ctx, scene_g, o, s, dims).view(np.uint32))


@pytest.mark.parametrize("kind", ["big", "small"])
def test_monotone_in_rmax(gpu_ctx, kind):
    """Property (b): found at r1 => found at r2 > r1 with the same words."""
    _, _, _, pts, _, _ = case(kind)
    scene = device_scene(gpu_ctx, kind)
    full = api.distance_points(gpu_ctx, scene, api.distance_records(pts))
    base = np.maximum(full["distance"], np.float32(1e-3))          # a point on a vertex has distance 0, and rmax must be > 0
    prev = None
    for f in (0.5, 1.5, 4.0, np.inf):
        got = api.distance_points(gpu_ctx, scene, api.distance_records(pts, base * np.float32(f) if np.isfinite(f) else np.inf))
        if prev is not None:
            was = prev["found"] != 0
            assert (got["found"][was] != 0).all() and np.array_equal(words(got)[was], words(prev)[was])
        prev = got
    assert np.array_equal(words(prev), words(full))
    assert (api.distance_points(gpu_ctx, scene, api.distance_records(pts, base * np.float32(0.5)))["found"] == 0).mean() > 0.9
    # any rmax >= FLT_MAX is unbounded
    assert np.array_equal(words(api.distance_points(gpu_ctx, scene, api.distance_records(pts, np.finfo(np.float32).max))), words(full))


@pytest.mark.parametrize("dims", [(5, 4, 3), (65, 3, 2)])
@pytest.mark.parametrize("kind", ["big", "small"])
def test_grid_equals_points_and_signed_equals_unsigned_times_side(gpu_ctx, kind, dims):
    """Properties (c) and (d), bit for bit; the 65-voxel rows cross a wave boundary."""
    scene = device_scene(gpu_ctx, kind)
    o, s = np.array([-8.0, -7.5, -8.25], np.float32), np.array([16.0 / dims[0], 3.7, 5.1], np.float32)
    for rmax in (np.inf, 3.0):
        vol = api.bake_distance_grid(gpu_ctx, scene, o, s, dims, rmax)
        assert vol.shape == (dims[2], dims[1], dims[0]) and vol.dtype == np.float32
        res = api.distance_points(gpu_ctx, scene, api.distance_records(api.grid_centres(o, s, dims).reshape(-1, 3), rmax))
        found = res["found"] != 0
        fill = np.float32(min(rmax, np.finfo(np.float32).max))
        assert np.array_equal(vol.reshape(-1).view(np.uint32), np.where(found, res["distance"], fill).astype(np.float32).view(np.uint32))
        signed = api.bake_distance_grid(gpu_ctx, scene, o, s, dims, rmax, signed=True)
        expect = np.where(found, np.where(res["side"] == 0, np.float32(0), res["distance"] * res["side"]), fill).astype(np.float32)
        assert np.array_equal(signed.reshape(-1).view(np.uint32), expect.view(np.uint32))
        if np.isfinite(rmax):
            assert 0 < found.sum() < found.size
    assert (res["side"] < 0).any() and (res["side"] > 0).any()


def device_points(ctx, scene, rec, flags=api.DISTANCE_DEVICE_POINTERS, canary=False, misalign=0):
    n = len(rec)
    d_rec = DeviceArray(ctx, rec.nbytes + 16).upload(rec)
    d_out = DeviceArray(ctx, n * 48 + 16)
    if canary:
        d_out.upload(np.full(n * 12 + 4, CANARY, np.uint32))
    rc = _abi.lib().lupin_hip_distance_points(ctx.handle, scene.handle, flags, n, C.c_void_p(d_rec.ptr + misalign), C.c_void_p(d_out.ptr))
    return rc, d_out.download(np.uint32, n * 12).reshape(n, 12)


def test_host_arrays_and_device_pointers_give_the_same_words(gpu_ctx):
    """Property (e), for the points and for the grid."""
    _, _, _, pts, _, _ = case("small")
    scene = device_scene(gpu_ctx, "small")
    rec = api.distance_records(pts, 2.5)
    rc, dev = device_points(gpu_ctx, scene, rec)
    assert rc == 0 and np.array_equal(dev, words(api.distance_points(gpu_ctx, scene, rec)))
    dims = (65, 3, 2)
    o, s, d = (C.c_float * 3)(-8, -7, -8), (C.c_float * 3)(0.25, 4, 5), (C.c_uint32 * 3)(*dims)
    d_vol = DeviceArray(gpu_ctx, 65 * 3 * 2 * 4)
    rc = _abi.lib().lupin_hip_bake_distance_grid(gpu_ctx.handle, scene.handle, api.DISTANCE_DEVICE_POINTERS | api.DISTANCE_GRID_SIGNED, o, s, d, 2.5, C.c_void_p(d_vol.ptr))
    assert rc == 0
    host = api.bake_distance_grid(gpu_ctx, scene, [-8, -7, -8], [0.25, 4, 5], dims, 2.5, signed=True)
    assert np.array_equal(d_vol.download(np.uint32, host.size), host.reshape(-1).view(np.uint32))


def quad_scene(ctx, half=64.0):
    sc = api.SceneCPU()
    sc.materials = np.array([api.default_material()], api.MATERIAL_DTYPE)
    v = np.array([[-half, -half, 0, 0], [half, -half, 0, 0], [half, half, 0, 0], [-half, half, 0, 0]], np.float32)
    sc.verts_pos_array.append(v)
    sc.indices_array.append(np.array([0, 1, 2, 0, 2, 3], np.uint32))
    sc.mesh_infos = np.array([api.default_mesh_info()], api.MESH_INFO_DTYPE)
    sc.instances = np.array([api.instance_from_transform(X.mat3x4(np.eye(3), np.zeros(3)), 0, 0)], api.INSTANCE_DTYPE)
    api.validate_scene(sc, 0, 0)
    return api.build_accel_structures_and_upload(ctx, sc, [], [], True)


def test_height_over_a_large_quad_is_exact(gpu_ctx):
    scene = quad_scene(gpu_ctx)
    for h in (0.125, 3.0, 40.0):
        for sign in (1.0, -1.0):
            p = [[1.0, 2.0, sign * h]]
            res = api.distance_points(gpu_ctx, scene, api.distance_records(p))[0]
            assert res["found"] == 1 and res["distance"] == np.float32(h) and res["point"].tolist() == [1.0, 2.0, 0.0] and res["side"] == sign
            assert api.distance_points(gpu_ctx, scene, api.distance_records(p, h * 0.5))[0]["found"] == 0
            assert api.distance_points(gpu_ctx, scene, api.distance_records(p, h))[0]["found"] == 0      # found is strict: |p - c| < rmax
            assert api.nearest_distance(gpu_ctx, scene, p, h * 2)[0] == np.float32(h)
    assert np.isinf(api.nearest_distance(gpu_ctx, scene, [[0, 0, 5]], 1.0)[0])
    # an rmax whose square is 0 in f32: a point ON the surface is at distance 0 < rmax and is found; one off it is not
    tiny = api.distance_points(gpu_ctx, scene, api.distance_records([[1, 2, 0], [1, 2, 0.125]], 1e-30))
    assert tiny["found"].tolist() == [1, 0] and tiny["distance"][0] == 0
    assert api.surface_clearance(gpu_ctx, scene, [[3, 3, 0]], [[0, 0, 1]], 0.25)[0] == np.float32(0.25)


def test_a_zero_area_triangle_and_an_empty_radius_report_nothing(gpu_ctx):
    """The soup's triangles with two equal vertices are skipped: a point on such a triangle's doubled vertex still finds the
    nearest REAL surface, at a positive distance or on another triangle, and never a NaN."""
    _, g, w, _, _, _ = case("small")
    scene = device_scene(gpu_ctx, "small")
    m = g.meshes[X.SOUP]
    dup = np.nonzero((m.verts[m.tris[:, 1]] == m.verts[m.tris[:, 2]]).all(1))[0]
    assert len(dup) == 4
    l2w = g.local_to_world()[1]
    p = (m.verts[m.tris[dup, 1]] @ l2w[:, :3].T + l2w[:, 3]).astype(np.float32)
    res = api.distance_points(gpu_ctx, scene, api.distance_records(p))
    assert (res["found"] == 1).all() and np.isfinite(res["distance"]).all() and np.isfinite(res["point"]).all()
    assert not ((res["instance"] == 1) & np.isin(res["tri"], dup)).any()
    ref = D.nearest(w, p)
    assert np.abs(res["distance"] - ref.distance).max() <= ref.tol_d.max()


def test_refusals_leave_the_output_untouched(gpu_ctx):
    scene = device_scene(gpu_ctx, "small")
    lib = _abi.lib()
    good = api.distance_records([[0, 0, 0], [1, 1, 1]], 2.0)

    def host_call(rec, flags=0, ctx=gpu_ctx, sc=scene, n=None):
        out = np.full((len(rec), 12), CANARY, np.uint32)
        rc = lib.lupin_hip_distance_points(ctx.handle if ctx else None, sc.handle if sc else None, flags, len(rec) if n is None else n, _abi.ptr(rec), _abi.ptr(out))
        assert (out == CANARY).all()
        return rc

    out = np.full((2, 12), CANARY, np.uint32)
    assert lib.lupin_hip_distance_points(gpu_ctx.handle, scene.handle, 0, 2, _abi.ptr(good), _abi.ptr(out)) == 0 and (out[:, 10:] == 0).all()
    assert lib.lupin_hip_distance_points(gpu_ctx.handle, scene.handle, 0, 0, _abi.ptr(good), _abi.ptr(np.full((2, 12), CANARY, np.uint32))) == 0
    for bad in ([np.nan, 0, 0, 1], [0, np.inf, 0, 1], [0, 0, -np.inf, 1], [0, 0, 0, np.nan], [0, 0, 0, 0.0], [0, 0, 0, -1.0], [0, 0, 0, -np.inf]):
        rec = good.copy()
        rec[1] = bad
        assert host_call(rec) == INV, bad
        rc, words_ = device_points(gpu_ctx, scene, rec, canary=True)
        assert rc == INV and (words_ == CANARY).all(), bad
    assert host_call(good, flags=4) == INV and host_call(good, flags=api.DISTANCE_GRID_SIGNED) == INV
    assert host_call(good, sc=None) == INV and host_call(good, ctx=None) == INV
    assert lib.lupin_hip_distance_points(gpu_ctx.handle, scene.handle, 0, 2, None, _abi.ptr(out)) == INV
    assert lib.lupin_hip_distance_points(gpu_ctx.handle, scene.handle, 0, 2, _abi.ptr(good), None) == INV
    rc, words_ = device_points(gpu_ctx, scene, good, canary=True, misalign=4)
    assert rc == INV and (words_ == CANARY).all()
    d_rec, d_out = DeviceArray(gpu_ctx, good.nbytes).upload(good), DeviceArray(gpu_ctx, 2 * 48 + 16).upload(np.full(2 * 12 + 4, CANARY, np.uint32))
    for off in (4, 8):                                     # a misaligned device out_results
        assert lib.lupin_hip_distance_points(gpu_ctx.handle, scene.handle, api.DISTANCE_DEVICE_POINTERS, 2, C.c_void_p(d_rec.ptr), C.c_void_p(d_out.ptr + off)) == INV
    assert (d_out.download(np.uint32, 28) == CANARY).all()
    other = api.Context(0)
    try:
        assert host_call(good, ctx=other) == INV          # a scene of another context
        dead_scene = X.build("small", X.SEED, other)
    finally:
        other.close()
    out = np.full((2, 12), CANARY, np.uint32)
    assert lib.lupin_hip_distance_points(gpu_ctx.handle, dead_scene.handle, 0, 2, _abi.ptr(good), _abi.ptr(out)) == INV and (out == CANARY).all()

    def grid(origin=(0, 0, 0), spacing=(1, 1, 1), dims=(2, 2, 2), rmax=1.0, flags=0, null=None):
        vol = np.full(8, CANARY, np.uint32)
        o, s, d = (C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_uint32 * 3)(*dims)
        args = dict(o=o, s=s, d=d, v=_abi.ptr(vol))
        if null:
            args[null] = None
        rc = lib.lupin_hip_bake_distance_grid(gpu_ctx.handle, scene.handle, flags, args["o"], args["s"], args["d"], rmax, args["v"])
        if rc != 0:
            assert (vol == CANARY).all()
        return rc

    assert grid() == 0
    for kw in (dict(origin=(np.nan, 0, 0)), dict(origin=(0, np.inf, 0)), dict(spacing=(0, 1, 1)), dict(spacing=(1, -1, 1)), dict(spacing=(1, 1, np.inf)),
               dict(spacing=(1, np.nan, 1)), dict(dims=(0, 2, 2)), dict(dims=(2, 2, 0)), dict(dims=(1 << 20, 1 << 20, 2)), dict(rmax=0.0), dict(rmax=-1.0),
               dict(rmax=float("nan")), dict(flags=8), dict(null="o"), dict(null="s"), dict(null="d"), dict(null="v"),
               dict(origin=(3e38, 0, 0), spacing=(3e38, 1, 1))):
        assert grid(**kw) == INV, kw
    d_vol = DeviceArray(gpu_ctx, 64)
    o, s, d = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_uint32 * 3)(2, 2, 1)
    assert lib.lupin_hip_bake_distance_grid(gpu_ctx.handle, scene.handle, api.DISTANCE_DEVICE_POINTERS, o, s, d, 1.0, C.c_void_p(d_vol.ptr + 2)) == INV


def chain_scene(ctx, T):
    from tests.test_gpu_ray_query import chain_bvh
    cpu = api.SceneCPU()
    cpu.materials = np.array([api.default_material()], api.MATERIAL_DTYPE)
    v = np.zeros((3 * T, 4), np.float32)
    for t in range(T):
        v[3 * t:3 * t + 3, :3] = [(t, 0, 0), (t + 0.9, 0, 0), (t, 0.9, 0)]
    cpu.verts_pos_array.append(v)
    cpu.indices_array.append(np.arange(3 * T, dtype=np.uint32))
    cpu.mesh_infos = np.array([api.default_mesh_info()], api.MESH_INFO_DTYPE)
    cpu.instances = np.array([api.default_instance()], api.INSTANCE_DTYPE)
    return api.build_accel_structures_and_upload(ctx, cpu, [], [], True, blas_builder=chain_bvh)


def test_a_hierarchy_too_deep_for_the_pair_stack_is_refused(gpu_ctx):
    """The stack holds two words per entry.  A chain of 100 triangles, whose 100 single words per lane a ray query accepts,
    is refused (2 x 100 KB exceed the LDS of a CU); a chain of 60 is answered, its far end included."""
    rec = api.distance_records([[99.2, 0.2, 1.0], [0.2, 0.2, 0.5]])
    deep = chain_scene(gpu_ctx, 100)
    assert api.occluded(gpu_ctx, deep, [[0.2, 0.2, 1.0]], [[0, 0, -1.0]])[0]
    with pytest.raises(api.LupinError) as e:
        api.distance_points(gpu_ctx, deep, rec)
    assert e.value.code == INV and "too deep" in str(e.value)
    res = api.distance_points(gpu_ctx, chain_scene(gpu_ctx, 60), api.distance_records([[59.2, 0.2, 1.0], [0.2, 0.2, 0.5]]))
    assert res["tri"].tolist() == [59, 0] and res["distance"].tolist() == [1.0, 0.5]


def test_a_refused_call_names_its_records_and_leaves_recorded_frames_intact(gpu_ctx):
    """Frames recorded and not yet run, then a call refused for its records: host arrays name the first bad index, device
    arrays count the bad records, the results stay untouched, and the frames are what they are without the call."""
    from tests import util
    W, H = 32, 24
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    rec = api.distance_records([[0, 1, 0], [0.2, 0.5, 0.1], [0.1, 1.5, -0.2], [-0.3, 0.7, 0.2], [0, 0.2, 0]], 2.0)
    alone = words(api.distance_points(gpu_ctx, scene, rec))
    bad = rec.copy(); bad[1, 2] = np.inf; bad[4, 3] = -1.0
    lib = _abi.lib()

    def host_refusal():
        out = np.full((5, 12), CANARY, np.uint32)
        assert lib.lupin_hip_distance_points(gpu_ctx.handle, scene.handle, 0, 5, _abi.ptr(bad), _abi.ptr(out)) == INV
        assert lib.lupin_hip_last_error().decode().startswith("record 1: ") and (out == CANARY).all()

    def device_refusal():
        rc, out = device_points(gpu_ctx, scene, bad, canary=True)
        assert rc == INV and lib.lupin_hip_last_error().decode().startswith("2 record(s): ") and (out == CANARY).all()

    plain = util.gpu_accumulate(gpu_ctx, scene, cams[0], W, H, frames=4, spp=1)
    for refusal in (host_refusal, device_refusal):
        assert util.f16_words_differ(util.gpu_accumulate(gpu_ctx, scene, cams[0], W, H, frames=4, spp=1, between=refusal), plain) == 0
    assert np.array_equal(words(api.distance_points(gpu_ctx, scene, rec)), alone)
