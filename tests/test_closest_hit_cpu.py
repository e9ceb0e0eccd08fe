"""Closest-hit traversal against the float64 brute-force intersector (tests/closest_hit_ref.py), without a GPU:
the oracle against the reference on the committed scenes, the comparison failing on each planted defect, and the reference
itself against closed forms."""
import numpy as np
import pytest

from lupinpathtracer_amd import api
from tests import closest_hit_ref as X
from tests import lbvh_ref

# DESIGN.md 17.  Measured for the oracle on the committed scenes and rays (SEED 1, three ray_epsilon each): the worst error
# of t is 1.67 U32 x conditioning, that of u, v 1.16; K_BOUND is four times the larger, rounded up.  In absolute terms the
# worst relative error of t is 4.7e-4 and the worst error of u, v 2.4e-3 (both on rays from 1e3 scene extents away); the
# median bound of u, v is 7e-5 on `big` and 5e-5 on `small`.
S_DECISIVE = X.S_DECISIVE          # 1e-4: floor of every decisive margin
K_BOUND = X.K_BOUND                # 7.0
MEASURED_WORST_OVER_BOUND = 0.26   # worst error / bound the oracle shows; 1 / 4 by the choice of K_BOUND
MAX_NON_DECISIVE = 0.01
MIN_DECISIVE_HITS = 0.25
MIN_HITS_PER_INSTANCE = 50
MIN_DECISIVE_PER_FAMILY = 3
SURFACE = (X.FAMILIES.index("surface_away"), X.FAMILIES.index("surface_into"))


def check_inputs(c, eps, rep):
    """The conditions that keep the comparison from passing by exclusion."""
    ref = c.refs[eps]
    assert rep["non_decisive_share"] <= MAX_NON_DECISIVE, rep
    assert rep["decisive_hits"] >= MIN_DECISIVE_HITS * rep["rays"], rep
    per_instance = np.bincount(ref.inst[ref.decisive & ref.hit], minlength=len(c.g.rows))
    assert per_instance.min() >= MIN_HITS_PER_INSTANCE, per_instance
    for f, name in enumerate(X.FAMILIES):
        if eps == 0.0 and f in SURFACE:
            continue            # an origin on a surface is at t = 0 = ray_epsilon: fragile by construction
        n = int((ref.decisive & (c.family == f)).sum())
        assert n >= MIN_DECISIVE_PER_FAMILY, (name, n)


def agree(c, eps, got, g=None, exclude=None):
    rep = X.compare(c.refs[eps], got, g or c.g, c.ori, c.dir, exclude)
    print(c.kind, eps, {k: (float(f"{v:.3g}") if isinstance(v, float) else v) for k, v in rep.items()})
    return rep


@pytest.mark.parametrize("eps", X.EPSILONS)
@pytest.mark.parametrize("kind", ["big", "small"])
def test_oracle_agrees_with_float64_brute_force(kind, eps):
    from oracle import oracle
    c = X.case(kind)
    assert len(c.ori) % 64 and len(c.ori) % 256
    rep = agree(c, eps, oracle.trace_rays(c.scene, c.ori, c.dir, eps))
    check_inputs(c, eps, rep)
    assert X.failures(rep) == []
    assert max(rep["worst_t_over_bound"], rep["worst_uv_over_bound"]) <= 1.1 * MEASURED_WORST_OVER_BOUND   # the factor 4 is there


def test_scene_sizes_are_on_both_sides_of_the_lds_limit():
    """lupin_hip_scene_create stages a scene in LDS when 80 B per node pair and instance and 48 B per triangle fit 24 KB; a
    binary tree has at most one pair per triangle."""
    tris = {k: sum(len(m.tris) for m in X.case(k).g.meshes) for k in ("big", "small")}
    assert tris["big"] * 48 > 24 * 1024
    assert tris["small"] * (48 + 80) + 2 * 13 * 80 < 24 * 1024


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_oracle_over_a_bounding_tree_agrees_on_any_seed(seed):
    """lbvh_ref.build's boxes contain their triangles, so no seed may show a missed hit."""
    from oracle import oracle
    builder = lambda v, i: lbvh_ref.build(v, i) if len(i) >= 3 * 64 else api.build_bvh(v, i)
    scene = X.build("big", seed, blas_builder=builder)
    g = X.geometry(scene)
    ori, d, _ = X.make_rays(g, seed + 7, {k: v // 4 for k, v in X.MAIN_COUNTS["big"].items()})
    ref = X.closest_hits(g, ori, d, 1e-3)
    rep = X.compare(ref, oracle.trace_rays(scene, ori, d, 1e-3), g, ori, d)
    assert rep["decisive_hits"] > 500 and X.failures(rep) == [], rep


# ---- planted defects: each must trip the comparison -------------------------------------------------------------

def _doctored(rep, *expected):
    fails = X.failures(rep)
    print(fails)
    assert fails, "the defect went unnoticed"
    assert any(f.split("=")[0] in expected for f in fails), fails


def test_detects_a_child_box_shrunk_by_two_percent():
    from oracle import oracle
    c = X.case("big")

    def builder(v, i):
        nodes, idx = api.build_bvh(v, i)
        if len(i) // 3 == len(c.g.meshes[X.GRID].tris):              # the height field, two instances
            nodes = nodes.copy()
            k = int(nodes[0]["tri_begin_or_first_child"])
            nodes[k]["aabb_max"] -= np.float32(0.02) * (nodes[k]["aabb_max"] - nodes[k]["aabb_min"])
        return nodes, idx
    scene = X.build("big", X.SEED, blas_builder=builder)
    _doctored(agree(c, 1e-3, oracle.trace_rays(scene, c.ori, c.dir, 1e-3), X.geometry(scene)), "flag", "triangle", "instance", "behind")


def _with_instance(c, i, change):
    xf = X.transforms(X.SEED)
    xf[i] = change(*xf[i])
    return X.build(c.kind, X.SEED, xf=xf)


def test_detects_a_transposed_instance_matrix():
    from oracle import oracle
    c = X.case("big")
    scene = _with_instance(c, 1, lambda M, b: (M.T, b))
    _doctored(agree(c, 1e-3, oracle.trace_rays(scene, c.ori, c.dir, 1e-3), X.geometry(scene)), "flag", "instance", "triangle")


def test_detects_a_mirrored_instance_flipped_back():
    from oracle import oracle
    c = X.case("big")
    assert X.LAYOUT[4][2] and np.linalg.det(c.g.rows[4, :, :3]) < 0
    assert sum(np.linalg.det(r[:, :3]) < 0 for r in c.g.rows) >= 3
    scene = _with_instance(c, 4, lambda M, b: (M @ np.diag([1.0, -1.0, 1.0]), b))
    _doctored(agree(c, 1e-3, oracle.trace_rays(scene, c.ori, c.dir, 1e-3), X.geometry(scene)), "flag", "instance", "triangle")


def test_detects_a_vertex_moved_after_the_tree_was_built():
    from oracle import oracle
    from tests import reproject_ref
    c = X.case("big")
    ref = c.refs[1e-3]
    on = ref.decisive & ref.hit & (c.g.mesh_idx[np.maximum(ref.inst, 0)] == X.GRID)
    verts, counts = np.unique(ref.tri[on][:, 0], return_counts=True)
    scene = X.build("big", X.SEED)
    v, _ = reproject_ref.mesh_arrays(scene, X.GRID)
    extent = float(np.linalg.norm(v[:, :3].max(0) - v[:, :3].min(0)))
    v[int(verts[np.argmax(counts)]), 1] += np.float32(1e-3 * extent)   # the scene's own buffer: the tree stays as built
    rep = agree(c, 1e-3, oracle.trace_rays(scene, c.ori, c.dir, 1e-3))
    _doctored(rep, "t", "uv")


def test_detects_the_wrong_ray_epsilon():
    from oracle import oracle
    c = X.case("big")
    _doctored(agree(c, 1e-3, oracle.trace_rays(c.scene, c.ori, c.dir, 0.0)), "flag", "instance", "triangle", "behind")


def test_detects_a_flipped_comparison_in_the_triangle_test():
    """A hit table in which u + v > 1 is accepted (the twin edit of tri_dst and the oracle a reviewer would try), imitated on
    the returned table: the nearest hit of the triangle's mirror image across its v1-v2 edge."""
    from oracle import oracle
    c = X.case("small")
    hit, dst, uv, inst, tri = [a.copy() for a in oracle.trace_rays(c.scene, c.ori, c.dir, 1e-3)]
    k = np.nonzero(hit == 1)[0][:20]
    uv[k] = 1.0 - uv[k][:, ::-1]
    _doctored(agree(c, 1e-3, (hit, dst, uv, inst, tri)), "uv", "reported_uv", "outside")


# ---- the reference against closed forms -------------------------------------------------------------------------

M_AFFINE = np.array([[2.0, 1.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 0.5]])     # its inverse is dyadic: exact in f32
B_AFFINE = np.array([3.0, -2.0, 5.0])


def _single_triangle(M, b):
    sc = api.SceneCPU()
    sc.materials = np.array([api.default_material()], api.MATERIAL_DTYPE)
    sc.verts_pos_array.append(np.array([[0, 0, 0, 0], [1, 0, 0, 0], [0, 1, 0, 0]], np.float32))
    sc.indices_array.append(np.array([0, 1, 2], np.uint32))
    sc.mesh_infos = np.array([api.default_mesh_info()], api.MESH_INFO_DTYPE)
    sc.instances = np.array([api.instance_from_transform(X.mat3x4(M, b), 0, 0)], api.INSTANCE_DTYPE)
    return api.build_accel_structures_and_upload(None, sc, [], [], True)


def _known_rays():
    """Local rays from (x, y, h) along (a, b, -c): they meet z = 0 at t = h / c in (u, v) = (x + a t, y + b t)."""
    local_o = np.array([[0.25, 0.25, 2.0], [0.125, 0.125, 1.0], [0.5, 0.25, 4.0], [0.75, 0.5, 1.0], [0.25, 0.25, -1.0],
                        [0.25, 0.25, 0.0005], [-0.5, 0.25, 1.0], [0.25, 0.25, 0.0], [0.125, 0.125, 1.0]])
    local_d = np.array([[0.0, 0.0, -1.0], [0.125, 0.0625, -0.5], [-0.0625, 0.0625, -2.0], [0.0, 0.0, -1.0], [0.0, 0.0, -1.0],
                        [0.0, 0.0, -1.0], [0.0, 0.0, -1.0], [1.0, 0.5, 0.0], [0.25, 0.125, -0.5]])
    # misses: u + v > 1, behind, t < eps, u < 0, in the plane; the last ray meets the edge u + v = 1 exactly
    t = np.array([2.0, 2.0, 2.0, np.inf, np.inf, np.inf, np.inf, np.inf, 2.0])
    u = local_o[:, 0] + local_d[:, 0] * np.where(np.isfinite(t), t, 0)
    v = local_o[:, 1] + local_d[:, 1] * np.where(np.isfinite(t), t, 0)
    return local_o, local_d, t, u, v


def test_reference_gives_the_closed_form_under_a_known_affine_transform():
    scene = _single_triangle(M_AFFINE, B_AFFINE)
    lo, ld, t, u, v = _known_rays()
    ori, d = lo @ M_AFFINE.T + B_AFFINE, ld @ M_AFFINE.T
    h = X.closest_hits(scene, ori, d, 1e-3)
    assert np.array_equal(h.hit, np.isfinite(t))
    assert np.allclose(h.t[h.hit], t[h.hit], rtol=1e-14) and np.allclose(h.u[h.hit], u[h.hit], atol=1e-14)
    assert np.allclose(h.v[h.hit], v[h.hit], atol=1e-14)
    assert (h.inst[h.hit] == 0).all() and (h.tri[h.hit] == [0, 1, 2]).all() and (h.inst[~h.hit] == -1).all()
    assert h.decisive[:8].all() and not h.decisive[8]   # det is 0 by structure for the ray in the plane; the edge is fragile
    assert X.closest_hits(scene, ori[5:6], d[5:6], 0.0).hit[0]          # t = 0.0005 counts once ray_epsilon allows it
    t2, u2, v2, _, _ = X.evaluate(X.geometry(scene), ori[:3], d[:3], [0, 0, 0], [[0, 1, 2]] * 3)
    assert np.allclose(t2, t[:3], rtol=1e-14) and np.allclose(u2, u[:3], atol=1e-14) and np.allclose(v2, v[:3], atol=1e-14)
    # a non-symmetric matrix told apart from its transpose
    wrong = X.closest_hits(_single_triangle(M_AFFINE.T, B_AFFINE), ori, d, 1e-3)
    assert not np.allclose(np.where(wrong.hit, wrong.u, -1)[:3], u[:3])


def test_reference_is_invariant_under_a_rigid_motion_of_instance_and_rays():
    rng = np.random.default_rng(5)
    g = X.geometry(_single_triangle(M_AFFINE, B_AFFINE))
    o = B_AFFINE + rng.uniform(-6, 6, (400, 3))
    d = (M_AFFINE @ np.array([0.3, 0.3, 0.0]) + B_AFFINE) + rng.uniform(-2, 2, (400, 3)) - o
    a = X.closest_hits(g, o, d, 1e-3)
    Q, shift = X.rotation(rng), np.array([10.0, -20.0, 5.0])
    l2w = np.eye(4)
    l2w[:3, :3], l2w[:3, 3] = Q @ M_AFFINE, Q @ B_AFFINE + shift
    moved = X.Geometry(np.linalg.inv(l2w)[None, :3], g.mesh_idx, g.meshes)
    b = X.closest_hits(moved, o @ Q.T + shift, d @ Q.T, 1e-3)
    both = a.decisive & b.decisive
    assert both.mean() > 0.95 and 50 < (a.hit & both).sum() < 350
    assert np.array_equal(a.hit[both], b.hit[both])
    hit = a.hit & both
    assert np.allclose(a.t[hit], b.t[hit], rtol=1e-12) and np.allclose(a.u[hit], b.u[hit], atol=1e-12) and np.allclose(a.v[hit], b.v[hit], atol=1e-12)


def test_float64_pinhole_matches_the_f32_restatement_of_the_kernel():
    """The float64 camera of the reprojection test is written from the header and DESIGN.md 16; the f32 restatement follows
    the kernel's operations.  They must describe the same rays."""
    from tests import reproject_ref
    cp = api.CameraParams(lens=0.035, film=0.036, aspect=1.5, focus=7.0)
    tr = X.mat3x4(X.rotation(np.random.default_rng(3)), [1.0, -2.0, 3.0])
    o64, d64 = X.pinhole_rays(48, 32, cp, tr)
    o32, d32 = reproject_ref.centre_rays(48, 32, cp, tr)
    assert np.abs(o64 - o32.reshape(-1, 3)).max() == 0 and np.abs(d64 - d32.reshape(-1, 3)).max() < 4e-7
    p = o64 + d64 * 5.0
    assert np.allclose(X.camera_depth(tr, p), reproject_ref.depth_of(tr, o32.reshape(-1, 3), d32.reshape(-1, 3), np.full(len(p), 5.0)), atol=1e-5)
