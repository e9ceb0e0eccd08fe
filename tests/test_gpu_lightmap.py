"""Lightmap baking on the device (lupin_hip_bake_lightmap): the records against the numpy restatement
(tests/lightmap_ref.py) bit for bit, the atlas against the radiance query on those records bit for bit, closed forms, the
dilation, every refusal, and that frames rendered around a bake do not notice it."""
import ctypes as C
import math

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import lightmap_ref as ref
from tests import stats, util

PT = api.PathtraceType
PI32 = np.float32(np.pi)
_cache = {}


def words(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same_words(got, want, what):
    bad = int((words(got) != words(want)).sum())
    assert bad == 0, f"{what}: {bad} of {words(want).size} f32 words differ"


def add_mesh(cpu, infos, pos, tris, uv=None, normals=None):
    info = api.default_mesh_info()
    v = np.zeros((len(pos), 4), np.float32)
    v[:, :3] = pos
    cpu.verts_pos_array.append(v)
    cpu.indices_array.append(np.asarray(tris, np.uint32).reshape(-1))
    if uv is not None:
        info["texcoords_buf_idx"] = len(cpu.verts_texcoord_array)
        cpu.verts_texcoord_array.append(np.asarray(uv, np.float32).reshape(-1, 2))
    if normals is not None:
        info["normals_buf_idx"] = len(cpu.verts_normal_array)
        n4 = np.zeros((len(pos), 4), np.float32)
        n4[:, :3] = normals
        cpu.verts_normal_array.append(n4)
    infos.append(info)


def matte(color=0.7, emission=0.0):
    m = api.default_material()
    m["color"] = (color, color, color, 1.0)
    m["emission"] = (emission, emission, emission, 0.0)
    return m


def constant_environment(cpu, emission):
    env = api.default_environment()
    env["emission"] = (emission, emission, emission)
    cpu.environments = np.array([env], _abi.ENVIRONMENT_DTYPE)
    return [api.EnvMapInfo(np.ones((1, 1, 4), np.float32), 1, 1)]


def sphere_mesh(nlat=8, nlon=12):
    """A latitude-longitude sphere with its own vertex per (ring, slice) corner, u = slice / nlon, v = ring / nlat, outward
    vertex normals, and no triangle without area at the poles: 2 * nlon * (nlat - 1) = 168 triangles, geometric normals outward."""
    pos, uv = [], []
    for i in range(nlat + 1):
        for j in range(nlon + 1):
            th, ph = math.pi * i / nlat, 2 * math.pi * j / nlon
            pos.append((math.sin(th) * math.cos(ph), math.cos(th), math.sin(th) * math.sin(ph)))
            uv.append((j / nlon, i / nlat))
    pos = np.array(pos, np.float32)
    tris = []
    at = lambda i, j: i * (nlon + 1) + j
    for i in range(nlat):
        for j in range(nlon):
            if i > 0:
                tris.append((at(i, j), at(i, j + 1), at(i + 1, j + 1)))
            if i < nlat - 1:
                tris.append((at(i, j), at(i + 1, j + 1), at(i + 1, j)))
    tris = np.array(tris, np.uint32)
    p = pos[tris].astype(np.float64)
    outward = np.einsum("ij,ij->i", np.cross(p[:, 2] - p[:, 0], p[:, 1] - p[:, 0]), p.mean(axis=1)) > 0
    tris[~outward] = tris[~outward][:, ::-1]
    assert len(tris) == 168
    return pos, tris, np.array(uv, np.float32), pos.copy()


def box_mesh():
    """12 triangles, four vertices of their own per face; face f takes the f-th sixth of u."""
    pos, tris, uv = [], [], []
    for f, (axis, sign) in enumerate([(0, 1), (0, -1), (1, 1), (1, -1), (2, 1), (2, -1)]):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        base = len(pos)
        for ca, cb in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
            p = [0.0, 0.0, 0.0]
            p[axis], p[a], p[b] = sign, ca, cb
            pos.append(p)
            uv.append(((f + (ca + 1) / 2) / 6, (cb + 1) / 2))
        tris += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
    return np.array(pos, np.float32), np.array(tris, np.uint32), np.array(uv, np.float32)


def transform(cols, translation):
    """(4, 3) column-major local -> world: three basis columns and the translation."""
    return np.array(list(cols) + [translation], np.float32)


def rotation(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K


def three_chart_cpu(moved=False):
    """Three instances of the sphere (two translated and uniformly scaled, one rotated and scaled 1.5 x 0.6 x 1.1), a box
    with texcoords and a box without, under a constant environment."""
    cpu = api.SceneCPU()
    infos = []
    pos, tris, uv, nrm = sphere_mesh()
    add_mesh(cpu, infos, pos, tris, uv, nrm)
    bpos, btris, buv = box_mesh()
    add_mesh(cpu, infos, bpos, btris, buv)
    add_mesh(cpu, infos, bpos, btris)
    cpu.mesh_infos = np.array(infos, _abi.MESH_INFO_DTYPE)
    cpu.materials = np.array([matte(0.7), matte(0.4)], _abi.MATERIAL_DTYPE)
    R = rotation((1, 2, 0.5), 0.7) @ np.diag([1.5, 0.6, 1.1])
    shift = (0.3, 0.1, -0.2) if moved else (0.0, 0.0, 0.0)
    cpu.instances = np.array([
        api.instance_from_transform(transform(np.eye(3), (-2.5 + shift[0], shift[1], shift[2])), 0, 0),
        api.instance_from_transform(transform(0.5 * np.eye(3), (0.0, 1.0, 0.5)), 0, 1),
        api.instance_from_transform(transform(R.T, (2.5, 0.2, 0.0)), 0, 0),
        api.instance_from_transform(transform(np.diag([6.0, 0.1, 6.0]), (0.0, -1.6, 0.0)), 1, 1),
        api.instance_from_transform(transform(0.3 * np.eye(3), (0.0, -0.5, 2.0)), 2, 0)], _abi.INSTANCE_DTYPE)
    return cpu, constant_environment(cpu, 0.5)


THREE_CHARTS = [api.LightmapChart(0, 0.5, 0.5, 0.0, 0.0), api.LightmapChart(1, 0.45, 0.4, 0.52, 0.03),
                api.LightmapChart(2, 0.9, 0.45, 0.05, 0.53)]


def three_chart_scene(ctx):
    if "three" not in _cache:
        cpu, envs = three_chart_cpu()
        api.validate_scene(cpu, 0, 0)
        _cache["three"] = (cpu, api.build_accel_structures_and_upload(ctx, cpu, [], envs, True))
    return _cache["three"]


def bake_raw(ctx, scene, charts, W, H, sentinel=None, want_records=True, **over):
    """lupin_hip_bake_lightmap itself: (status, rgba, records or None, covered)."""
    f = dict(pathtrace_type=0, max_bounces=8, samples=1, max_slots=0, flags=0, dilate=0, counter=0, surface_offset=1e-3)
    f.update(over)
    d = _abi.LightmapDescC(W, H, int(f["pathtrace_type"]), f["max_bounces"], f["samples"], f["max_slots"], f["flags"], f["dilate"], f["counter"],
                           f["surface_offset"], _abi.AdvancedParamsC(100.0, 0, 0.001))
    cc = (_abi.LightmapChartC * max(1, len(charts)))(*[_abi.LightmapChartC(c.instance_idx, c.scale_u, c.scale_v, c.offset_u, c.offset_v) for c in charts])
    fill = 0.0 if sentinel is None else sentinel
    rgba = np.full((H, W, 4), fill, np.float32)
    rec = np.full((H, W, 8), fill, np.float32) if want_records else None
    covered = C.c_uint64(12345)
    rc = _abi.lib().lupin_hip_bake_lightmap(ctx.handle, scene.handle, C.byref(d), cc, len(charts), _abi.ptr(rgba), _abi.ptr(rec), C.byref(covered))
    return rc, rgba, rec, int(covered.value)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(17, 33), (64, 64)])
@pytest.mark.parametrize("smooth", [False, True])
def test_records_equal_the_restatement_bit_for_bit(gpu_ctx, W, H, smooth):
    cpu, scene = three_chart_scene(gpu_ctx)
    want, owner = ref.records(cpu, scene, THREE_CHARTS, W, H, np.float32(1e-3), counter=7, smooth_normals=smooth)
    rc, rgba, got, covered = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, counter=7, flags=1 if smooth else 0, surface_offset=1e-3)
    assert rc == 0, _abi.lib().lupin_hip_last_error()
    n = int((owner != ref.NO_OWNER).sum())
    assert n > W * H // 4 and covered == n == api.lightmap_stats()["covered_texels"]
    assert len({int(k) // 168 for k in np.unique(owner) if k != ref.NO_OWNER}) == 3          # all three charts own texels
    assert np.array_equal(got.view(np.uint32)[..., 7] == 1, owner != ref.NO_OWNER)
    assert_same_words(got, want, f"records {W} x {H}, smooth = {smooth}")
    assert np.array_equal(rgba[..., 3] == 1.0, owner != ref.NO_OWNER) and np.all(rgba[owner == ref.NO_OWNER] == 0.0)
    if smooth:       # the smooth normals are not the geometric ones, and agree with them in sign
        flat, _ = ref.records(cpu, scene, THREE_CHARTS, W, H, np.float32(1e-3), counter=7, smooth_normals=False)
        assert int((words(flat[..., 4:7]) != words(want[..., 4:7])).sum()) > n
        assert np.all(np.einsum("...i,...i", flat[..., 4:7], want[..., 4:7])[owner != ref.NO_OWNER] > 0)


@pytest.mark.gpu
@pytest.mark.parametrize("ptype", [PT.Standard, PT.MIS])
def test_the_atlas_is_pi_times_the_query_on_its_records(gpu_ctx, ptype):
    cpu, scene = three_chart_scene(gpu_ctx)
    W = H = 32
    S = 5
    whole = None
    for max_slots in (0, 1000):       # unchunked; 200 records per wavefront
        rc, rgba, rec, covered = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, samples=S, pathtrace_type=ptype, max_slots=max_slots)
        assert rc == 0, _abi.lib().lupin_hip_last_error()
        mask = rec.view(np.uint32)[..., 7] == 1
        assert covered == int(mask.sum()) and (max_slots == 0 or covered * S >= 3 * max_slots)      # at least three chunks
        mean = api.pathtrace_rays(gpu_ctx, scene, rec[mask], api.RayQueryDesc(ptype, 8, S))
        assert float(mean[:, :3].max()) > 0.0
        assert_same_words(rgba[mask][:, :3], PI32 * mean[:, :3], f"{ptype.name}, max_slots = {max_slots}")
        assert np.all(rgba[mask][:, 3] == 1.0) and np.all(rgba[~mask] == 0.0)
        if whole is None:
            whole = rgba
        assert_same_words(rgba, whole, "chunked against unchunked")
    # the Python mirror is the same call
    mine, mine_rec = api.bake_lightmap(gpu_ctx, scene, THREE_CHARTS, W, H, samples=S, pathtrace_type=ptype, surface_offset=1e-3, want_records=True)
    assert mine.shape == (H, W, 4) and mine_rec.shape == (H, W, 8)
    assert_same_words(mine, whole, "api.bake_lightmap")
    assert_same_words(mine_rec, rec, "api.bake_lightmap records")


QUAD_UV = [(0, 0), (1, 0), (1, 1), (0, 1)]


def floor_quad(half):
    """A square of side 2 * half in the plane y = 0 whose geometric normal (reference winding) is +y; u along x, v along z."""
    pos = np.float32([(-half, 0, -half), (half, 0, -half), (half, 0, half), (-half, 0, half)])
    tris = np.uint32([(0, 1, 2), (0, 2, 3)])
    p = pos.astype(np.float64)
    assert np.cross(p[2] - p[0], p[1] - p[0])[1] > 0
    return pos, tris


@pytest.mark.gpu
def test_a_quad_under_a_constant_sky_is_exactly_pi_times_it(gpu_ctx):
    cpu = api.SceneCPU()
    infos = []
    pos, tris = floor_quad(1.0)
    add_mesh(cpu, infos, pos, tris, QUAD_UV)
    cpu.mesh_infos = np.array(infos, _abi.MESH_INFO_DTYPE)
    cpu.materials = np.array([matte(0.5)], _abi.MATERIAL_DTYPE)
    cpu.instances = np.array([api.default_instance()], _abi.INSTANCE_DTYPE)
    scene = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], constant_environment(cpu, 0.5), True)
    chart = api.LightmapChart(0, 0.71, 0.53, 0.113, 0.291)
    got = api.bake_lightmap(gpu_ctx, scene, [chart], 24, 24, samples=64, pathtrace_type=PT.Naive)
    owner, _, _ = ref.raster([QUAD_UV], [ref.mesh_triangles(scene)[0]], [chart], 24, 24)
    covered = owner != ref.NO_OWNER
    assert 50 < int(covered.sum()) < 24 * 24
    assert np.all(got[covered][:, :3] == PI32 * np.float32(0.5)) and np.all(got[covered][:, 3] == 1.0)
    assert np.all(got[~covered] == 0.0)
    # the default offset: 1e-4 of the largest world extent (the quad's side, 2)
    _, rec = api.bake_lightmap(gpu_ctx, scene, [chart], 24, 24, samples=1, want_records=True)
    assert api.scene_world_extent(scene) == pytest.approx(2.0)
    assert np.all(rec[covered][:, 1] == np.float32(2e-4))


L_EMIT = 3.0


def form_factor(p, lo=-1.0, hi=1.0, height=1.0):
    """Point-to-parallel-rectangle form factor, float64: the fraction of the cosine-weighted hemisphere about +y at p that
    the rectangle [lo, hi]^2 in the plane y = height fills.  The corner formula, signed over the four corners."""
    c = height - p[1]

    def corner(a, b):
        ra, rb = math.sqrt(a * a + c * c), math.sqrt(b * b + c * c)
        return (a / ra * math.atan(b / ra) + b / rb * math.atan(a / rb)) / (2.0 * math.pi)
    x1, x2, z1, z2 = lo - p[0], hi - p[0], lo - p[2], hi - p[2]
    return corner(x2, z2) - corner(x1, z2) - corner(x2, z1) + corner(x1, z1)


def form_factor_quadrature(p, m=1500):
    x = (np.arange(m) + 0.5) / m * 2.0 - 1.0
    xx, zz = np.meshgrid(x - p[0], x - p[2])
    c = 1.0 - p[1]
    return float(np.sum(c * c / (math.pi * (xx * xx + zz * zz + c * c) ** 2)) * (2.0 / m) ** 2)


def test_form_factor_agrees_with_quadrature_and_the_known_centre():
    assert abs(form_factor((0.0, 0.0, 0.0)) - 0.5541) < 1e-4
    for p in ((0.125, 0.0004, -0.125), (1.875, 0.0004, 1.875), (-0.875, 0.0004, 1.375)):       # three texel centres of the 16 x 16 atlas
        assert abs(form_factor(p) - form_factor_quadrature(p)) < 1e-6, p


@pytest.mark.gpu
@pytest.mark.parametrize("ptype", [PT.Naive, PT.Standard])
def test_a_floor_under_a_square_emitter_follows_the_form_factor(gpu_ctx, ptype):
    if "emitter" not in _cache:
        cpu = api.SceneCPU()
        infos = []
        pos, tris = floor_quad(2.0)
        add_mesh(cpu, infos, pos, tris, QUAD_UV)
        add_mesh(cpu, infos, [(-1, 1, -1), (-1, 1, 1), (1, 1, 1), (1, 1, -1)], [(0, 2, 1), (2, 0, 3)])     # facing down, as DESIGN 13's
        cpu.mesh_infos = np.array(infos, _abi.MESH_INFO_DTYPE)
        cpu.materials = np.array([matte(0.0), matte(0.0, L_EMIT)], _abi.MATERIAL_DTYPE)
        floor, light = api.default_instance(), api.default_instance()
        light["mesh_idx"], light["mat_idx"] = 1, 1
        cpu.instances = np.array([floor, light], _abi.INSTANCE_DTYPE)
        _cache["emitter"] = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], [], True)
    scene = _cache["emitter"]
    W = H = 16
    S = 4096
    got, rec = api.bake_lightmap(gpu_ctx, scene, [api.LightmapChart(0)], W, H, samples=S, pathtrace_type=ptype, want_records=True)
    assert np.all(got[..., 3] == 1.0) and np.all(got[..., 0] == got[..., 1]) and np.all(got[..., 1] == got[..., 2])
    ys, xs = np.mgrid[0:H, 0:W]
    centre = np.stack([(xs + 0.5) / W * 4 - 2, np.zeros((H, W)), (ys + 0.5) / H * 4 - 2], axis=-1)
    assert np.abs(rec[..., 0:3].astype(np.float64) - centre).max() < 1e-3        # texel (x, y) lies where its centre maps to
    hits = got[..., 0].astype(np.float64) / (math.pi * L_EMIT)                   # the fraction of the texel's paths that reached the emitter

    def judge(points):
        F = np.array([[form_factor(points[y, x]) for x in range(W)] for y in range(H)])
        z = (hits - F) / np.sqrt(F * (1.0 - F) / S)
        chi2 = float((z * z).sum())
        return float(np.abs(z).max()), chi2, stats.chi2_sf(chi2, W * H)
    worst, chi2, p = judge(rec[..., 0:3].astype(np.float64))
    print(f"{ptype.name}: worst |z| = {worst:.2f}, chi2 = {chi2:.1f} / {W * H} dof, p = {p:.4f}")
    assert worst <= 5.0 and p > 0.001, (worst, chi2, p)
    # the twin: the form factor at the texel's corner instead of its centre must NOT pass, or a half-texel shift would go unseen
    corner = rec[..., 0:3].astype(np.float64) - np.array([2.0 / W, 0.0, 2.0 / H])
    worst_c, chi2_c, p_c = judge(corner)
    print(f"corner twin: worst |z| = {worst_c:.2f}, chi2 = {chi2_c:.1f}, p = {p_c:.3g}")
    assert worst_c > 5.0 or p_c < 0.001


@pytest.mark.gpu
def test_dilation_equals_the_restatement_bit_for_bit(gpu_ctx):
    cpu, scene = three_chart_scene(gpu_ctx)
    W, H = 40, 24
    rc, plain, _, covered = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, samples=3, want_records=False)
    assert rc == 0 and 0 < covered < W * H
    for passes in (0, 1, 3):
        rc, got, _, _ = bake_raw(gpu_ctx, scene, THREE_CHARTS, W, H, samples=3, dilate=passes, want_records=False)
        assert rc == 0, _abi.lib().lupin_hip_last_error()
        want = ref.dilate(plain, passes)
        assert_same_words(got, want, f"dilate = {passes}")
        assert np.array_equal(got[..., 3] == 1.0, plain[..., 3] == 1.0) and np.all((got[..., 3] == 0.0) | (got[..., 3] == 1.0))
        if passes:
            assert int((got[..., :3] != plain[..., :3]).any(axis=-1).sum()) > 20        # the gutters took something


@pytest.mark.gpu
def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    cpu, scene = three_chart_scene(gpu_ctx)
    lib = _abi.lib()
    W = H = 16
    one = [api.LightmapChart(0)]
    cases = []

    def case(label, charts=one, **over):
        rc, rgba, rec, covered = bake_raw(gpu_ctx, scene, charts, W, H, sentinel=-7.0, **over)
        cases.append((label, rc, rgba, rec, covered))

    def raw(label, ctx_h, scene_h, desc, charts, num, out):
        d = _abi.LightmapDescC(W, H, 0, 8, 1, 0, 0, 0, 0, 1e-3, _abi.AdvancedParamsC(100.0, 0, 0.001))
        cc = _abi.LightmapChartC(0, 1.0, 1.0, 0.0, 0.0)
        rgba = np.full((H, W, 4), -7.0, np.float32)
        rc = lib.lupin_hip_bake_lightmap(ctx_h, scene_h, C.byref(d) if desc else None, C.byref(cc) if charts else None, num,
                                         _abi.ptr(rgba) if out else None, None, None)
        cases.append((label, rc, rgba, None, 12345))

    raw("null context", None, scene.handle, True, True, 1, True)
    raw("null scene", gpu_ctx.handle, None, True, True, 1, True)
    raw("null desc", gpu_ctx.handle, scene.handle, False, True, 1, True)
    raw("null charts", gpu_ctx.handle, scene.handle, True, False, 1, True)
    raw("null out_rgba", gpu_ctx.handle, scene.handle, True, True, 1, False)
    raw("num_charts == 0", gpu_ctx.handle, scene.handle, True, True, 0, True)

    def sized(label, w, h):       # the size is in the descriptor alone: the arrays stay small
        d = _abi.LightmapDescC(w, h, 0, 8, 1, 0, 0, 0, 0, 1e-3, _abi.AdvancedParamsC(100.0, 0, 0.001))
        cc = _abi.LightmapChartC(0, 1.0, 1.0, 0.0, 0.0)
        rgba = np.full((H, W, 4), -7.0, np.float32)
        cases.append((label, lib.lupin_hip_bake_lightmap(gpu_ctx.handle, scene.handle, C.byref(d), C.byref(cc), 1, _abi.ptr(rgba), None, None),
                      rgba, None, 12345))
    sized("width == 0", 0, 16)
    sized("height == 0", 16, 0)
    sized("width above 16384", 16385, 16)
    sized("height above 16384", 16, 16385)
    case("instance index out of range", [api.LightmapChart(5)])
    case("a later chart's instance out of range", [api.LightmapChart(0), api.LightmapChart(0xFFFFFFFF)])
    case("a mesh without texcoords", [api.LightmapChart(0), api.LightmapChart(4)])
    for k, field in enumerate(("scale_u", "scale_v", "offset_u", "offset_v")):
        for bad in (np.nan, np.inf, -np.inf):
            c = api.LightmapChart(0)
            setattr(c, field, bad)
            case(f"{field} = {bad}", [c])
    for so in (0.0, -1e-3, np.nan, np.inf):
        case(f"surface_offset = {so}", surface_offset=so)
    case("unknown flag", flags=2)
    case("dilate above 64", dilate=65)
    case("unknown integrator", pathtrace_type=4)
    case("samples == 0", samples=0)
    case("samples above 2^27", samples=(1 << 27) + 1)
    case("max_bounces == 4095", max_bounces=4095)
    other = api.Context(0)
    ecpu, eenvs = three_chart_cpu()
    foreign = api.build_accel_structures_and_upload(other, ecpu, [], eenvs, True)
    raw("scene of another context", gpu_ctx.handle, foreign.handle, True, True, 1, True)
    other.close()
    raw("scene of a destroyed context", gpu_ctx.handle, foreign.handle, True, True, 1, True)
    for label, rc, rgba, rec, covered in cases:
        assert rc == -1, (label, rc)
        assert lib.lupin_hip_last_error()
        assert np.all(rgba == -7.0), label
        assert rec is None or np.all(rec == -7.0), label
        assert covered == 12345, label
    # an atlas nobody covers: LUPIN_OK and zeros
    rc, rgba, rec, covered = bake_raw(gpu_ctx, scene, [api.LightmapChart(0, 1.0, 1.0, 5.0, 5.0)], W, H, sentinel=-7.0, dilate=2)
    assert rc == 0 and covered == 0 and np.all(rgba == 0.0) and np.all(rec == 0.0)
    # the limits themselves pass
    rc, rgba, _, covered = bake_raw(gpu_ctx, scene, one, W, H, dilate=64, flags=1, want_records=False)
    assert rc == 0 and covered > 0


def camera_desc(out, k):
    return api.PathtraceDesc(accum_params=api.AccumulationParams(out.back(), k), camera_params=api.CameraParams(aspect=1.0))


@pytest.mark.gpu
def test_frames_around_a_bake_do_not_notice_it(gpu_ctx):
    cpu, scene = three_chart_scene(gpu_ctx)
    W = H = 48

    def chain(bake_after):
        res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=8, samples_per_pixel=2))
        out = api.DoubleBufferedTexture(gpu_ctx, W, H)
        baked = None
        for k in range(6):
            api.pathtrace_scene(gpu_ctx, res, scene, out.front(), PT.Standard, camera_desc(out, k))
            out.flip()
            if k + 1 == bake_after:
                baked = api.bake_lightmap(gpu_ctx, scene, THREE_CHARTS, 32, 32, samples=2, pathtrace_type=PT.MIS, dilate=1, surface_offset=1e-3)
        out.flip()
        return out.front().download(), baked

    plain, _ = chain(None)
    with_bake, baked = chain(3)
    assert float(plain.astype(np.float32)[..., :3].max()) > 0.0
    assert util.f16_words_differ(with_bake, plain) == 0
    again = api.bake_lightmap(gpu_ctx, scene, THREE_CHARTS, 32, 32, samples=2, pathtrace_type=PT.MIS, dilate=1, surface_offset=1e-3)
    assert_same_words(again, baked, "the bake between the frames against the same bake afterwards")


@pytest.mark.gpu
def test_bake_after_update_instances_equals_a_fresh_scene(gpu_ctx):
    cpu, envs = three_chart_cpu()
    a = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], envs, True)
    moved_cpu, moved_envs = three_chart_cpu(moved=True)
    b = api.build_accel_structures_and_upload(gpu_ctx, moved_cpu, [], moved_envs, True)
    kw = dict(samples=2, pathtrace_type=PT.MIS, surface_offset=1e-3, want_records=True)
    before, before_rec = api.bake_lightmap(gpu_ctx, a, THREE_CHARTS, 32, 32, **kw)
    a.update_instances(moved_cpu.instances["transpose_inverse_transform"])
    after, after_rec = api.bake_lightmap(gpu_ctx, a, THREE_CHARTS, 32, 32, **kw)
    fresh, fresh_rec = api.bake_lightmap(gpu_ctx, b, THREE_CHARTS, 32, 32, **kw)
    assert int((words(before_rec) != words(fresh_rec)).sum()) > 100       # the move is visible
    assert_same_words(after_rec, fresh_rec, "records of the updated scene against a freshly created moved scene")
    assert_same_words(after, fresh, "atlas of the updated scene against a freshly created moved scene")
    want, _ = ref.records(moved_cpu, a, THREE_CHARTS, 32, 32, np.float32(1e-3))
    assert_same_words(after_rec, want, "records of the updated scene against the restatement")


@pytest.mark.gpu
def test_uvs_the_rule_skips_or_clamps_harm_nothing(gpu_ctx):
    """One chart whose mesh carries a NaN UV, UVs of 1e30, UVs below zero and a triangle without UV area among good ones:
    inputs the contract defines.  (Were this ever to fault: the cause is in lm_span's clamp, to be found by reading it.)"""
    cpu = api.SceneCPU()
    infos = []
    pos, tris = floor_quad(1.0)
    extra = np.float32([(3, 0, 0), (4, 0, 0), (3, 0, 1)])                       # a triangle with area in space, reused below
    pos = np.concatenate([pos] + [extra + np.float32([0, 0, 2 * k]) for k in range(5)])
    uv = np.float32(QUAD_UV + [(np.nan, 0.3), (0.8, 0.1), (0.9, 0.9),
                               (1e30, 1e30), (2e30, 1e30), (1e30, 2e30),
                               (0.5, 0.5), (0.5, 0.5), (0.7, 0.7),
                               (-5, -5), (-4, -5), (-5, -4),
                               (0.1, 0.2), (1e30, 0.3), (0.2, 0.9)])             # one vertex far away: a finite area2, a clamped box
    tris = np.concatenate([np.uint32([(4 + 3 * k, 5 + 3 * k, 6 + 3 * k) for k in range(5)]), tris])
    add_mesh(cpu, infos, pos, tris, uv)
    cpu.mesh_infos = np.array(infos, _abi.MESH_INFO_DTYPE)
    cpu.materials = np.array([matte(0.5)], _abi.MATERIAL_DTYPE)
    cpu.instances = np.array([api.default_instance()], _abi.INSTANCE_DTYPE)
    scene = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], constant_environment(cpu, 0.5), True)
    chart = [api.LightmapChart(0, 0.75, 0.75, 0.125, 0.125)]
    want, owner = ref.records(cpu, scene, chart, 16, 16, np.float32(1e-3))
    rc, rgba, got, covered = bake_raw(gpu_ctx, scene, chart, 16, 16, samples=2)
    assert rc == 0, _abi.lib().lupin_hip_last_error()
    assert covered == int((owner != ref.NO_OWNER).sum()) >= 144
    assert np.array_equal(got.view(np.uint32)[..., 7] == 1, owner != ref.NO_OWNER)
    assert_same_words(got, want, "records beside the skipped triangles")
    assert np.array_equal(rgba[..., 3] == 1.0, owner != ref.NO_OWNER)
