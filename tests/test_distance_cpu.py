"""The float64 reference of the distance queries (tests/distance_ref.py) pinned without a GPU: closed forms,
invariance under a rigid motion, the fit of K on the committed point sets, planted twins that the judgement must catch,
and the ABI of the two entry points against the built library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import closest_hit_ref as X
from tests import distance_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = np.array([[[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]])
_cache = {}


def case(kind, moved=False):
    """(scene built on the host, Geometry, World, points f32, family, reference) of closest_hit_ref's scenes."""
    key = (kind, moved)
    if key not in _cache:
        scene = X.build(kind, X.SEED, xf=X.transforms(X.SEED, moved))
        g = X.geometry(scene)
        w = D.world(g)
        counts = D.COUNTS[kind]
        if moved:
            counts = {k: max(8, c // 3) for k, c in counts.items()}
        pts, fam = D.make_points(g, X.SEED + (21 if moved else 20), counts)
        _cache[key] = (scene, g, w, pts, fam, D.nearest(w, pts))
    return _cache[key]


def as_results(ref):
    """A reference answer in the layout of api.distance_points, so that compare() can judge a twin."""
    got = np.zeros(len(ref.found), api.DISTANCE_RESULT_DTYPE)
    got["found"] = ref.found
    got["distance"] = np.where(ref.found, ref.distance, 0.0)
    got["point"], got["u"], got["v"] = ref.point, ref.u, ref.v
    got["instance"], got["tri"] = np.maximum(ref.inst, 0), np.maximum(ref.local, 0)
    got["side"] = ref.side
    return got


def one(p, tri=UNIT):
    d2, q, u, v, feat = D.closest_points(np.array([p], np.float64), np.asarray(tri, np.float64))
    return np.sqrt(d2[0, 0]), q[0, 0], u[0, 0], v[0, 0], feat[0, 0]


# ---- closed forms, to 1e-12 -----------------------------------------------------------------------------------------

def test_point_above_the_interior():
    d, q, u, v, feat = one([0.25, 0.25, 2.0])
    assert abs(d - 2.0) < 1e-12 and np.abs(q - [0.25, 0.25, 0]).max() < 1e-12 and abs(u - 0.25) < 1e-12 and abs(v - 0.25) < 1e-12 and feat == 0


def test_point_beyond_an_edge():
    d, q, u, v, feat = one([0.5, -3.0, 4.0])              # beyond v0 v1
    assert abs(d - 5.0) < 1e-12 and np.abs(q - [0.5, 0, 0]).max() < 1e-12 and abs(u - 0.5) < 1e-12 and v == 0 and feat == 1
    d, q, u, v, feat = one([1.0, 1.0, 0.0])               # beyond the hypotenuse
    assert abs(d - np.sqrt(0.5)) < 1e-12 and np.abs(q - [0.5, 0.5, 0]).max() < 1e-12 and abs(u + v - 1) < 1e-12 and feat == 1


def test_point_beyond_a_vertex():
    d, q, u, v, feat = one([-3.0, -4.0, 12.0])
    assert abs(d - 13.0) < 1e-12 and np.abs(q).max() < 1e-12 and u == 0 and v == 0 and feat == 2
    d, q, u, v, feat = one([3.0, -1.0, 0.0])
    assert abs(d - np.sqrt(5.0)) < 1e-12 and np.abs(q - [1, 0, 0]).max() < 1e-12 and u == 1 and v == 0 and feat == 2


def test_zero_area_triangles_are_skipped():
    d2 = D.closest_points(np.array([[0.0, 0, 1]]), np.array([[[0.0, 0, 0], [1, 0, 0], [2, 0, 0]], [[0.0, 0, 0], [1, 1, 1], [1, 1, 1]]]))[0]
    assert np.isinf(d2).all()
    dd = D.tri_nearest_f32(np.array([0, 0, 1], np.float32), *np.array([[0.0, 0, 0], [1, 1, 1], [1, 1, 1]], np.float32))[0]
    assert np.isinf(dd)


def scaled_geometry():
    """One triangle under local -> world diag(1, 4, 0.25) (a dyadic inverse): world triangle (0,0,0) (1,0,0) (0,4,0)."""
    M = np.diag([1.0, 4.0, 0.25])
    rows = np.zeros((1, 3, 4))
    rows[0, :, :3] = np.linalg.inv(M)
    mesh = X.Mesh(np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), np.array([[0, 1, 2]]))
    return X.Geometry(rows, np.array([0]), [mesh])


def test_non_uniform_scale_is_measured_in_world_space():
    g = scaled_geometry()
    w = D.world(g)
    assert np.array_equal(w.tri[0], [[0, 0, 0], [1, 0, 0], [0, 4, 0]])
    p = np.array([[2.0, 2.0, 0.0]])                       # beyond the hypotenuse x + y / 4 = 1 of the world triangle
    ref = D.nearest(w, p)
    # world: foot on the line from (1, 0) to (0, 4): t = ((p - a) . e) / (e . e), e = (-1, 4)
    t = (np.array([1.0, 2.0]) @ np.array([-1.0, 4.0])) / 17.0
    foot = np.array([1 - t, 4 * t, 0.0])
    assert np.abs(ref.point[0] - foot).max() < 1e-12 and abs(ref.distance[0] - np.linalg.norm(p[0] - foot)) < 1e-12
    # local: p is (2, 0.5, 0), the unit triangle's foot is (1.25, -0.25) clamped ... mapped back it is another point
    pl = p @ g.rows[0, :, :3].T
    loc = D.nearest(D.world(g, transform=False), pl)
    back = loc.point[0] @ np.diag([1.0, 4.0, 0.25])
    assert np.linalg.norm(back - foot) > 0.1              # the local-space nearest point is provably not the world-space one
    assert np.linalg.norm(p[0] - back) > ref.distance[0] + 0.01


# ---- properties -----------------------------------------------------------------------------------------------------

def test_invariant_under_a_rigid_motion():
    _, g, w, pts, _, ref = case("small")
    rng = np.random.default_rng(5)
    Q, b = X.rotation(rng), rng.uniform(-3, 3, 3)
    w2 = D.World(w.tri @ Q.T + b, w.inst, w.triple, w.local, w.mag, w.emax, w.hmin)
    moved = D.nearest(w2, pts.astype(np.float64) @ Q.T + b)
    face = (ref.feat_verts >= 0).all(1)                   # on a shared edge or vertex the tie may resolve either way
    assert face.sum() > len(pts) // 4
    assert np.array_equal(moved.inst, ref.inst) and np.array_equal(moved.local[face], ref.local[face])
    assert np.abs(moved.distance - ref.distance).max() < 1e-10
    assert np.abs(moved.point - (ref.point @ Q.T + b)).max() < 1e-10


@pytest.mark.parametrize("kind", ["small", "big"])
def test_the_reference_decides_all_but_one_percent_per_family(kind):
    for moved in (False, True) if kind == "big" else (False,):
        _, _, _, _, fam, ref = case(kind, moved)
        for f, name in enumerate(D.FAMILIES):
            left, n = int((~ref.decisive[fam == f]).sum()), int((fam == f).sum())
            print(kind, moved, name, n, "left out:", left, "=", left / n)
            assert 100 * left <= n                         # at most 1 %, counted in integers


def test_f32_restatement_against_float64_fits_k(built):
    """K_DIST is four times the worst error of the kernel's leaf arithmetic restated in f32, in units of
    2^-24 (|p| + |M||v| + |b| + longest edge), rounded up, over the committed scenes and points."""
    worst = 0.0
    for kind in ("small", "big"):
        scene, g, w, pts, fam, ref = case(kind)
        wf = D.world_f32(scene, g)
        assert wf.shape == w.tri.shape
        rows = D.index_of_cached(w)
        j = np.array([rows[(int(i), int(t))] for i, t in zip(ref.inst, ref.local)])
        dd, u, v, q = D.tri_nearest_f32(pts, wf[j, 0], wf[j, 1], wf[j, 2])
        unit = D.U32 * (np.linalg.norm(pts.astype(np.float64), axis=1) + w.mag[j] + w.emax[j])
        err = np.abs(np.sqrt(dd.astype(np.float64)) - ref.distance) / unit
        print(kind, "worst f32 distance error in units:", err.max(), "per family:", [float(err[fam == f].max()) for f in range(4)])
        worst = max(worst, float(err.max()))
        # and the f32 brute force agrees with the reference under the judgement itself
        d32, j32 = D.nearest_f32(wf, pts)
        got = as_results(ref)
        got["distance"], got["instance"], got["tri"] = d32, w.inst[j32], w.local[j32]
        dd2, u2, v2, q2 = D.tri_nearest_f32(pts, wf[j32, 0], wf[j32, 1], wf[j32, 2])
        got["point"], got["u"], got["v"] = q2, u2, v2
        nrm = np.cross(wf[j32, 1] - wf[j32, 0], wf[j32, 2] - wf[j32, 0])
        got["side"] = np.sign(((pts - q2) * nrm).sum(1))
        rep = D.compare(ref, w, pts, got)
        print(rep)
        assert D.failures(rep) == []
    assert np.ceil(4 * worst) == D.K_DIST, worst


# ---- planted twins that the judgement must catch --------------------------------------------------------------------

def test_detects_a_reference_that_measures_in_local_space():
    _, g, w, pts, _, _ = case("small")
    i = 1                                                  # the soup under scale (3, 1, 0.25)
    only = D.world(g, skip=[k for k in range(len(g.rows)) if k != i])
    ref = D.nearest(only, pts)
    pl = pts.astype(np.float64) @ g.rows[i, :, :3].T + g.rows[i, :, 3]
    loc = D.nearest(D.world(X.Geometry(g.rows[i:i + 1], g.mesh_idx[i:i + 1], g.meshes), transform=False), pl)
    twin = as_results(loc)
    twin["instance"] = i
    l2w = g.local_to_world()[i]
    twin["point"] = loc.point @ l2w[:, :3].T + l2w[:, 3]
    rep = D.compare(ref, only, pts, twin)
    assert rep["distance"] > len(pts) // 10 and rep["reported_distance"] > len(pts) // 10, rep


def test_detects_a_reference_that_forgets_the_instance_transform():
    _, g, w, pts, _, ref = case("small")
    twin = as_results(D.nearest(D.world(g, transform=False), pts))
    rep = D.compare(ref, w, pts, twin)
    assert rep["instance"] + rep["triangle"] > len(pts) // 10 and rep["distance"] + rep["reported_distance"] > 0, rep


def test_detects_a_reference_that_compares_less_or_equal_at_rmax():
    g = scaled_geometry()
    w = D.world(g)
    p = np.array([[0.25, 0.5, 0.375]], np.float32)        # exactly 0.375 above the face, in f32 as in f64
    ref = D.nearest(w, p, rmax=0.375)
    assert not ref.found[0] and ref.nearest[0] == 0.375
    assert D.nearest(w, p, rmax=np.nextafter(np.float32(0.375), np.float32(1))).found[0]
    twin = D.nearest(w, p, rmax=0.375, strict=False)
    assert twin.found[0]
    # at exactly rmax nothing is decisive by tolerance, so the twin is told from the reference by the flag alone
    assert twin.found[0] != ref.found[0]


# ---- the leaky boxes ------------------------------------------------------------------------------------------------

def leaky_case():
    if "leaky" not in _cache:
        scene = D.leaky_scene()
        g = X.geometry(scene)
        w = D.world(g)
        pts, rmax, inst, tri = D.leaky_points(scene, g)
        _cache["leaky"] = (scene, g, w, pts, rmax, D.nearest(w, pts, rmax))
    return _cache["leaky"]


def test_the_library_flags_the_planted_leaks(built):
    """WideNode.d.z comes from blas_child_pairs; lupin_hip_collapse_bvh4 runs the same function on the same node arrays and
    returns its triangle marks, which must be the triangles that stick out of a box above them."""
    from tests import reproject_ref
    from tests.test_wide_traversal import collapse
    scene, g, _, _, _, _ = leaky_case()
    total = 0
    for mi, (nodes, leaky_node, leak) in enumerate(D.leaks(scene, g)):
        v, idx = reproject_ref.mesh_arrays(scene, mi)
        _, _, flags = collapse(nodes, v, idx)
        assert np.array_equal((flags & 2) != 0, (leak > 0).any(1))
        assert leaky_node.sum() > 0
        total += int((leak > 0).any(1).sum())
    assert total > 20


def test_leaky_family_needs_the_flags():
    """The point family aimed at the leaky triangles (a vertex that sticks out of a stored box, rmax a quarter of the leak)
    on the scene's real node arrays, through the f32 restatement of the traversal: honouring WideNode.d.z every query is
    found, on the reference's terms; the variant that ignores the flags prunes the box and misses most of them."""
    scene, g, w, pts, rmax, ref = leaky_case()
    assert len(pts) == 48 and ref.found.all() and ref.decisive.all()
    found, dist, inst, tri = D.nearest_f32_blas(scene, g, pts, rmax, honour_flags=True)
    assert found.all()
    got = as_results(ref)
    got["distance"], got["instance"], got["tri"] = dist, inst, tri
    rows = D.index_of_cached(w)
    wf = D.world_f32(scene, g)
    j = np.array([rows[(int(i), int(t))] for i, t in zip(inst, tri)])
    _, u, v, q = D.tri_nearest_f32(pts, wf[j, 0], wf[j, 1], wf[j, 2])
    got["point"], got["u"], got["v"] = q, u, v
    got["side"] = np.sign(((pts - q) * np.cross(wf[j, 1] - wf[j, 0], wf[j, 2] - wf[j, 0])).sum(1))
    rep = D.compare(ref, w, pts, got)
    print(rep)
    assert D.failures(rep) == []
    blind, _, _, _ = D.nearest_f32_blas(scene, g, pts, rmax, honour_flags=False)
    print("found without the flags:", int(blind.sum()), "of", len(pts))
    assert blind.sum() < len(pts) // 2
    twin = as_results(ref)
    twin["found"] = blind
    assert D.compare(ref, w, pts, twin)["flag"] == int((~blind).sum()) > 0


# ---- records, ABI, and the absence of a fallback --------------------------------------------------------------------

def test_records_and_grid_centres_hold_the_stated_words():
    rec = api.distance_records([[1, 2, 3], [4, 5, 6]], [0.5, np.inf])
    assert rec.dtype == np.float32 and rec.shape == (2, 4) and rec[0].tolist() == [1, 2, 3, 0.5] and np.isinf(rec[1, 3])
    c = api.grid_centres([0.1, 0.2, 0.3], [0.7, 0.5, 0.25], (5, 4, 3))
    assert c.shape == (3, 4, 5, 3) and c.dtype == np.float32
    f = np.float32
    assert c[2, 3, 4].tolist() == [f(0.1) + (f(4) + f(0.5)) * f(0.7), f(0.2) + (f(3) + f(0.5)) * f(0.5), f(0.3) + (f(2) + f(0.5)) * f(0.25)]


def test_abi_symbols_constants_and_mirrors(built):
    handle = C.CDLL(_abi.LIB_PATH)
    names = {n for n, _, _ in _abi.SYMBOLS}
    for sym in ("lupin_hip_distance_points", "lupin_hip_bake_distance_grid"):
        assert hasattr(handle, sym) and sym in names
    assert api.DISTANCE_RESULT_DTYPE.itemsize == 48 and api.DISTANCE_RESULT_DTYPE.names[:3] == ("found", "distance", "point")
    assert [api.DISTANCE_RESULT_DTYPE.fields[k][1] // 4 for k in ("found", "distance", "point", "u", "v", "instance", "tri", "side")] == [0, 1, 2, 5, 6, 7, 8, 9]
    header = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    assert re.search(r"#define LUPIN_DISTANCE_RECORD_FLOATS 4\b", header) and api.DISTANCE_RECORD_FLOATS == 4
    assert re.search(r"#define LUPIN_DISTANCE_RESULT_FLOATS 12\b", header) and api.DISTANCE_RESULT_FLOATS == 12
    assert re.search(r"LUPIN_DISTANCE_DEVICE_POINTERS = 1u, LUPIN_DISTANCE_GRID_SIGNED = 2u", header)
    assert (api.DISTANCE_DEVICE_POINTERS, api.DISTANCE_GRID_SIGNED) == (1, 2)
    assert "NOT an inside / outside classification" in header
    rust = open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    assert "pub fn lupin_hip_distance_points(" in rust and "pub fn lupin_hip_bake_distance_grid(" in rust
    cpp = open(os.path.join(ROOT, "include", "lupin.hpp")).read()
    for name in ("distance_points", "bake_distance_grid"):
        assert re.search(r"inline [\w:<> ]+ %s\(" % name, cpp), name


def test_without_a_device_every_entry_refuses(built):
    if api.device_count() > 0:
        pytest.skip("a HIP device is present")
    scene = case("small")[0]                               # built on the host: no handle
    calls = [lambda: api.distance_points(None, scene, api.distance_records([[0, 0, 0]])), lambda: api.nearest_distance(None, scene, [[0, 0, 0]]),
             lambda: api.bake_distance_grid(None, scene, [0, 0, 0], [1, 1, 1], (2, 2, 2)),
             lambda: api.surface_clearance(None, scene, [[0, 0, 0]], [[0, 0, 1]], 0.1)]
    for call in calls:
        with pytest.raises(api.LupinError) as e:
            call()
        assert e.value.code == -2                          # LUPIN_ERR_NO_DEVICE
    rec = api.distance_records([[0, 0, 0]])
    out = np.full(12, 0xABCDABCD, np.uint32)
    assert _abi.lib().lupin_hip_distance_points(None, None, 0, 1, _abi.ptr(rec), _abi.ptr(out)) == -2
    vol = np.full(8, 0xABCDABCD, np.uint32)
    o, s, d = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_uint32 * 3)(2, 2, 2)
    assert _abi.lib().lupin_hip_bake_distance_grid(None, None, 0, o, s, d, 1.0, _abi.ptr(vol)) == -2
    assert (out == 0xABCDABCD).all() and (vol == 0xABCDABCD).all()
