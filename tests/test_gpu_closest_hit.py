"""The device's closest-hit query against the float64 brute-force intersector (tests/closest_hit_ref.py):
lupin_hip_trace_rays from global memory and from LDS, the four-wide probe, every BLAS and TLAS builder, instances moved in
place, the primary visibility of the reprojection and the small batch sizes.  The float64 answer depends on geometry and
rays only and is computed once per scene and ray set; the assertions are those of tests/test_closest_hit_cpu.py."""
import numpy as np
import pytest

from lupinpathtracer_amd import api
from tests import closest_hit_ref as X
from tests import reproject_ref
from tests.test_closest_hit_cpu import agree, check_inputs

pytestmark = pytest.mark.gpu

# the device is bit-equal to the oracle (tests/test_gpu_parity.py), so the bounds are the oracle's
S_DECISIVE = X.S_DECISIVE          # 1e-4
K_BOUND = X.K_BOUND                # 7.0: four times the oracle's worst error in units of U32 x conditioning
MAX_NON_DECISIVE = 0.01
MAX_RETRACE = 0.03                 # tests/test_wide_traversal.py
_scenes = {}


def device_scene(ctx, kind, **kw):
    key = (id(ctx), kind, tuple(sorted(kw.items())))
    if key not in _scenes:
        _scenes[key] = X.build(kind, X.SEED, ctx, **kw)
    return _scenes[key]


def staged_in_lds(ctx, scene):
    try:
        api.trace_rays_wide(ctx, scene, [[0.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    except api.LupinError as e:
        assert "staged in LDS" in str(e), str(e)
        return True
    return False


@pytest.mark.parametrize("eps", X.EPSILONS)
@pytest.mark.parametrize("kind", ["big", "small"])
def test_trace_rays_agrees_with_float64_brute_force(gpu_ctx, kind, eps):
    c = X.case(kind)
    scene = device_scene(gpu_ctx, kind)
    assert staged_in_lds(gpu_ctx, scene) == (kind == "small")
    rep = agree(c, eps, api.trace_rays(gpu_ctx, scene, c.ori, c.dir, eps), X.geometry(scene))
    check_inputs(c, eps, rep)
    assert X.failures(rep) == []


def test_wide_probe_agrees_unless_flagged(gpu_ctx):
    c = X.case("big")
    scene = device_scene(gpu_ctx, "big")
    *got, flag = api.trace_rays_wide(gpu_ctx, scene, c.ori, c.dir, 1e-3)
    assert flag.mean() < MAX_RETRACE
    rep = agree(c, 1e-3, got, X.geometry(scene), exclude=flag != 0)
    assert rep["non_decisive_share"] <= MAX_NON_DECISIVE and rep["decisive_hits"] >= 0.25 * rep["rays"]
    assert X.failures(rep) == []


@pytest.mark.parametrize("tlas_builder", ["cpu", "device"])
@pytest.mark.parametrize("blas_builder", ["sah", "sah_device", "lbvh"])
def test_every_builder_gives_the_float64_answer(gpu_ctx, blas_builder, tlas_builder):
    c = X.case("big")                                                   # the same object for all six
    scene = device_scene(gpu_ctx, "big", blas_builder=blas_builder, tlas_builder=tlas_builder)
    g = X.geometry(scene)
    assert sum(len(m.tris) >= 64 for m in g.meshes) == 3                # meshes the device builders take
    rep = agree(c, 1e-3, api.trace_rays(gpu_ctx, scene, c.ori, c.dir, 1e-3), g)
    assert X.failures(rep) == []


@pytest.mark.parametrize("tlas_builder", ["cpu", "device"])
def test_moved_instances_give_the_float64_answer_of_the_new_transforms(gpu_ctx, tlas_builder):
    """No old row and no old TLAS box may survive Scene.update_instances."""
    c = X.case("big", moved=True)
    scene = X.build("big", X.SEED, gpu_ctx)                             # a scene of its own: it is changed in place
    scene.update_instances(X.instance_records(X.transforms(X.SEED, moved=True)), tlas_builder=tlas_builder)
    g = X.geometry(scene)
    assert np.array_equal(g.rows, c.g.rows)
    rep = agree(c, 1e-3, api.trace_rays(gpu_ctx, scene, c.ori, c.dir, 1e-3), g)
    assert rep["non_decisive_share"] <= MAX_NON_DECISIVE and rep["decisive_hits"] >= 0.25 * rep["rays"]
    per_instance = np.bincount(c.refs[1e-3].inst[c.refs[1e-3].decisive & c.refs[1e-3].hit], minlength=len(g.rows))
    assert per_instance.min() >= 15, per_instance                       # a third of the main batch's rays
    assert X.failures(rep) == []
    old = X.compare(X.closest_hits(X.case("big").g, c.ori, c.dir, 1e-3), api.trace_rays(gpu_ctx, scene, c.ori, c.dir, 1e-3), g, c.ori, c.dir)
    assert X.failures(old), "the move must be visible to these rays"


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("kind", ["big", "small"])
def test_small_batches(gpu_ctx, kind, n):
    c = X.case(kind)
    ref = c.refs[1e-3]
    first = np.nonzero(ref.decisive & ref.hit)[0][0]                    # the single ray is a decisive hit
    sel = np.arange(first, first + n)
    got = api.trace_rays(gpu_ctx, device_scene(gpu_ctx, kind), c.ori[sel], c.dir[sel], 1e-3)
    rep = X.compare(ref.take(sel), got, c.g, c.ori[sel], c.dir[sel])
    assert rep["decisive_hits"] >= 1 and X.failures(rep) == [], rep


def test_reprojection_primary_visibility_against_a_float64_pinhole(gpu_ctx):
    """k_reproject_trace: camera_ray_of<PINHOLE>, scene_closest and the depth the reprojection gate depends on, against float64
    rays through the pixel centres (closest_hit_ref.pinhole_rays, from the header and DESIGN.md 16) and their brute-force hits."""
    W, H = 48, 32
    c = X.case("big")
    scene = device_scene(gpu_ctx, "big")
    cp = api.CameraParams(lens=0.060, film=0.036, aspect=W / H, focus=20.0, aperture=0.0)
    rot = X.rotation(np.random.default_rng(12))
    pos = np.array([3.0, 2.0, -1.0]) - rot[:, 2] * 20.0                 # looks along its +z at the middle of the scene
    tr = X.mat3x4(rot, pos)
    ares, rp = api.build_adaptive_resources(gpu_ctx, W, H), api.build_reproject_resources(gpu_ctx, W, H)
    out = api.DoubleBufferedTexture(gpu_ctx, W, H)
    api.adaptive_reproject(gpu_ctx, ares, rp, scene, api.ReprojectDesc(camera_params=cp, camera_transform=tr, ray_epsilon=1e-3),
                           out.back(), out.front())
    inst, tri, uv, depth = rp.download(0)
    ori, d = X.pinhole_rays(W, H, cp, tr)
    hit = (inst != reproject_ref.MISS).reshape(-1)
    # global triangle -> (mesh-local triangle of the hit instance): the inverse of reproject_ref.global_triangle
    _, offsets = reproject_ref.scene_triangles(scene)
    g = X.geometry(scene)
    safe = np.where(hit, inst.reshape(-1), 0).astype(np.int64)
    local = np.where(hit, tri.reshape(-1).astype(np.int64) - offsets[g.mesh_idx[safe]].astype(np.int64), 0)
    assert (local >= 0).all()
    # depth = camera-space z of o + d t = t (d . z axis) under a rigid camera: the reported t follows from the reported depth.
    # The camera's own f32 work is charged separately: four more roundings on the ray (pixel -> direction, two normalisations,
    # the 3 x 3 product) enter like the roundings of cd, and the depth's evaluation (p = o + d t, the rounded inverse rows,
    # three products and sums) costs 8 roundings at |pos| + |p|.
    k = K_BOUND + 4.0
    ref = X.closest_hits(c.g, ori, d, 1e-3, k=k)
    cos = d @ rot[:, 2]
    assert cos.min() > 0.5
    extra_t = 8 * X.U32 * (np.abs(pos).sum() + np.abs(ori + d * np.where(ref.hit, ref.t, 0.0)[:, None]).sum(1)) / cos
    got = (hit.astype(np.uint32), np.where(hit, depth.reshape(-1) / cos, 0.0), uv.reshape(-1, 2), safe, local)
    rep = X.compare(ref, got, g, ori, d, k=k, extra_t=extra_t)
    print(rep)
    assert rep["non_decisive_share"] <= MAX_NON_DECISIVE and rep["decisive_hits"] >= 0.25 * rep["rays"], rep
    assert len(np.unique(ref.inst[ref.decisive & ref.hit])) >= 6
    assert X.failures(rep) == []
    both = ref.decisive & ref.hit & hit
    z = X.camera_depth(tr, ori + d * np.where(ref.hit, ref.t, 0.0)[:, None])
    assert np.all(np.abs(depth.reshape(-1)[both] - z[both]) <= ((ref.tol_t + extra_t) * cos)[both])
    assert (depth.reshape(-1)[~hit] == 0).all()
