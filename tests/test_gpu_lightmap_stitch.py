"""Lightmap seam stitching on the device (lupin_hip_stitch_lightmap): the output and every word of the info
against the numpy float32 restatement (tests/lightmap_stitch_ref.py), the float64 reference's conditions, what must stay
untouched, the chain bake -> denoise -> stitch -> view, and every refusal."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api, loader
from tests import lightmap_stitch_ref as S
from tests import lightmap_unwrap_ref as U
from tests import lightmapped_view_ref as L
from tests import util
from tests.test_gpu_ray_query import DeviceArray
from tests.test_lightmap_stitch_cpu import FACE_COLOURS

F = np.float32
PT = api.PathtraceType
INVALID = -1
_cache = {}


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def differing(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((words(got) != words(want)).sum())


def ply(name):
    cpu = api.SceneCPU()
    loader.load_mesh_ply(os.path.join(util.SHARED, "shapes", name + ".ply"), cpu)
    return np.asarray(cpu.verts_pos_array[0], F)[:, :3], cpu.indices_array[0].reshape(-1, 3)


def cube_mesh():
    pos, tris = U.cube()
    return pos, tris[:, ::-1].copy()      # wound so that the renderer's geometric normal points outward


# name: (mesh, texel size, padding).  The cube's faces are 8 x 8 texels; the cylinder fixture is 0.15 across and its wall is cut along curved seams
# (sphere.ply is six patches with vertices of their own: no edge is shared by index, so it has no seam to stitch).
INPUTS = {"cube": (cube_mesh, 0.125, 2), "octahedron": (U.octahedron, 0.11, 1), "fin": (S.fin, 0.1, 1), "uvcylinder": (lambda: ply("uvcylinder"), 0.005, 1),
          "bowtie": (U.bowtie, 0.09, 1)}


def fixture(ctx, name):
    """One mesh under a white sky, unwrapped on the device and attached, as one chart over its own atlas; its ownership from
    a one-sample bake; and the same as the restatement takes it."""
    if (name, id(ctx)) not in _cache:
        make, texel, pad = INPUTS[name]
        cpu, envs = U.scene_cpu_of([make()], sky=1.0)
        scene = U.upload(ctx, cpu, envs)
        uvs, info = scene.unwrap_lightmap_uvs(0, texel, pad)
        W, H, charts = api.pack_lightmap_instances([(info["width"], info["height"])], [1.0], 0)
        assert W <= 128 and H <= 128, (name, W, H)
        tris = U.scene_mesh(scene, cpu, 0)[1]
        alpha = api.bake_lightmap(ctx, scene, charts, W, H, samples=1, max_bounces=1, surface_offset=1e-3)[..., 3]
        _cache[name, id(ctx)] = SimpleNamespace(cpu=cpu, scene=scene, charts=charts, W=W, H=H, owned=alpha != 0, ref=[(tris, uvs, charts[0])], rows={})
    return _cache[name, id(ctx)]


def raw_stitch(ctx_h, scene_h, charts, rgba, out, iterations=4, spt=2.0, lam=0.1, flags=0, reserved=0, W=None, H=None, desc=True, info=True,
               num_charts=None):
    """lupin_hip_stitch_lightmap itself on whatever the arguments are (arrays, None or raw addresses): (status, info)."""
    def as_ptr(a):
        return a if (a is None or isinstance(a, C.c_void_p)) else _abi.ptr(a)
    h, w = (rgba.shape[:2] if hasattr(rgba, "shape") else (0, 0))
    d = _abi.LightmapStitchDescC(w if W is None else W, h if H is None else H, iterations, spt, lam, flags, reserved)
    c = None if charts is None else (_abi.LightmapChartC * max(1, len(charts)))(*[_abi.LightmapChartC(int(k.instance_idx), k.scale_u, k.scale_v, k.offset_u, k.offset_v)
                                                                                   for k in charts])
    i = _abi.LightmapStitchInfoC(77, 77, 77, 77, 77, 77, (C.c_float * 3)(-7, -7, -7), (C.c_float * 3)(-7, -7, -7))
    n = (0 if charts is None else len(charts)) if num_charts is None else num_charts
    rc = _abi.lib().lupin_hip_stitch_lightmap(ctx_h, scene_h, C.byref(d) if desc else None, c, n, as_ptr(rgba), as_ptr(out), C.byref(i) if info else None)
    return rc, i


def info_words(i):
    """Every integer and float of a LupinLightmapStitchInfo (ctypes) or of the restatement's dict, as 12 words."""
    if isinstance(i, dict):
        ints = [i[k] for k in ("seam_edges", "non_manifold_edges", "sample_pairs", "dropped_pairs", "active_texels", "iterations")]
        return np.concatenate([np.uint32(ints), words(F(i["energy_before"])), words(F(i["energy_after"]))])
    return np.frombuffer(bytes(i), np.uint32).copy()


def input_atlas(ctx, f, kind):
    if kind == "random":
        return S.random_atlas(f.owned, 11)
    return api.bake_lightmap(ctx, f.scene, f.charts, f.W, f.H, samples=4, max_bounces=2, surface_offset=1e-3, dilate=1)      # "baked"


CASES = [(name, "random", it) for name in ("cube", "octahedron", "fin", "uvcylinder") for it in (0, 1, 2, 16)] + [("cube", "baked", 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kind,iterations", CASES)
def test_the_device_equals_the_restatement_word_for_word(gpu_ctx, name, kind, iterations):
    f = fixture(gpu_ctx, name)
    rgba = input_atlas(gpu_ctx, f, kind)
    if kind not in f.rows:
        f.rows[kind] = S.rows_of(rgba, f.ref, 2.0)
    want, want_info = S.stitch(rgba, f.ref, iterations, rows=f.rows[kind])
    print(name, kind, iterations, {k: v for k, v in want_info.items()}, "atlas", f.W, f.H)
    if name == "cube":
        assert (want_info["seam_edges"], want_info["non_manifold_edges"]) == (12, 0)
    if name == "fin":
        assert want_info["non_manifold_edges"] == 1
    if name != "fin":
        assert want_info["sample_pairs"] > 0 and want_info["active_texels"] > 0
    if name == "uvcylinder":
        assert want_info["seam_edges"] > 200
    # host pointers, twice
    for attempt in range(2):
        out = np.full_like(rgba, -7.0)
        rc, info = raw_stitch(gpu_ctx.handle, f.scene.handle, f.charts, rgba, out, iterations)
        assert rc == 0, _abi.lib().lupin_hip_last_error()
        assert differing(out, want) == 0, (name, attempt)
        assert np.array_equal(info_words(info), info_words(want_info)), (name, attempt, info_words(info), info_words(want_info))
    # device pointers, twice, then in place
    d_in = DeviceArray(gpu_ctx, rgba.nbytes).upload(rgba)
    for attempt in range(2):
        d_out = DeviceArray(gpu_ctx, rgba.nbytes).upload(np.full_like(rgba, -7.0))
        rc, info = raw_stitch(gpu_ctx.handle, f.scene.handle, f.charts, C.c_void_p(d_in.ptr), C.c_void_p(d_out.ptr), iterations, flags=1, W=f.W, H=f.H)
        assert rc == 0, _abi.lib().lupin_hip_last_error()
        assert differing(d_out.download(F, rgba.size).reshape(rgba.shape), want) == 0, (name, attempt)
        assert np.array_equal(info_words(info), info_words(want_info))
    rc, _ = raw_stitch(gpu_ctx.handle, f.scene.handle, f.charts, C.c_void_p(d_in.ptr), C.c_void_p(d_in.ptr), iterations, flags=1, W=f.W, H=f.H)
    assert rc == 0 and differing(d_in.download(F, rgba.size).reshape(rgba.shape), want) == 0
    # the Python mirror is the same call
    mine, mine_info = api.stitch_lightmap(gpu_ctx, f.scene, f.charts, rgba, iterations=iterations, want_info=True)
    assert differing(mine, want) == 0 and np.array_equal(info_words(mine_info), info_words(want_info))
    stats = api.lightmap_stitch_stats()
    assert stats["call_ms"] > 0.0 and stats["edges_ms"] > 0.0


def six_colours(f):
    """The cube's atlas with one colour per face: the face of a texel from the chart of its owning triangle's corner UVs."""
    tris, uvs, chart = f.ref[0]
    from tests import lightmap_ref as R
    owner, _, _ = R.raster([uvs.reshape(-1, 2)], [np.arange(3 * len(tris)).reshape(-1, 3)], [chart], f.W, f.H)
    assert np.array_equal(owner != R.NO_OWNER, f.owned)
    pos = np.asarray(f.cpu.verts_pos_array[0], F)[:, :3][tris.astype(np.int64)]                     # (T, 3, 3)
    n = np.cross(pos[:, 1] - pos[:, 0], pos[:, 2] - pos[:, 0])
    face = 2 * np.abs(n).argmax(axis=1) + (n[np.arange(len(n)), np.abs(n).argmax(axis=1)] < 0)
    rgba = np.zeros((f.H, f.W, 4), F)
    rgba[f.owned, 0:3] = FACE_COLOURS[face[owner[f.owned]]]
    rgba[f.owned, 3] = 1.0
    return rgba


# The device runs the float32 restatement word for word, so its distance from the float64 CG is the restatement's, which is
# measured without a device: on this input the seam energy of the float32 result after 16 steps is within
# 7.2e-7 relative of the float64 CG's, both evaluated by the view's own float32 fetch, and the solver's float32 report is within
# 2.5e-7 of that evaluation.  Both figures are a few float32 roundings (6e-8 each) of sums of 192 squared differences.  The
# assertions stand at 1e-4, about a hundred times the measured figures: a different but equally valid order of the same
# float32 operations passes, and the bound stays seven orders below the factor of 1900 by which 16 steps lower the energy.
ENERGY_MARGIN = 1e-4


@pytest.mark.gpu
def test_sixteen_steps_reach_the_float64_references_energy(gpu_ctx):
    f = fixture(gpu_ctx, "cube")
    rgba = six_colours(f)
    rows = S.rows_of(rgba, f.ref, 2.0)
    out, info = api.stitch_lightmap(gpu_ctx, f.scene, f.charts, rgba, iterations=16, want_info=True)
    before, after = S.seam_energy_by_fetch(rgba, rows), S.seam_energy_by_fetch(out, rows)
    A, active = S.dense_system(rows)
    x0 = rgba.reshape(-1, 4)[active, 0:3].astype(np.float64)
    x16 = S.cg64(A, x0, 0.1, 16)[-1]
    ref_atlas = rgba.copy()
    ref_atlas.reshape(-1, 4)[active, 0:3] = x16.astype(F)
    ref_after = S.seam_energy_by_fetch(ref_atlas, rows)
    print("seam energy before", before, "device after 16", after, "float64 CG after 16", ref_after, "ratio", after / ref_after,
          "reported", info["energy_before"], info["energy_after"])
    assert np.all(after < before)
    assert np.all(np.abs(after / ref_after - 1.0) <= ENERGY_MARGIN)
    # the solver's own report, summed in float32 in its fixed order, against the float64 evaluation: the same margin
    assert np.all(np.abs(info["energy_before"] / before - 1.0) <= ENERGY_MARGIN)
    assert np.all(np.abs(info["energy_after"] / after - 1.0) <= ENERGY_MARGIN)


@pytest.mark.gpu
def test_untouched_texels_a_constant_atlas_and_an_atlas_without_a_seam(gpu_ctx):
    f = fixture(gpu_ctx, "cube")
    rgba = S.random_atlas(f.owned, 5)
    rgba[~f.owned, 0:3] = 9.0                                 # what a gutter pass may have left: not re-dilated, not touched
    rows = S.rows_of(rgba, f.ref, 2.0)
    active = np.zeros(f.W * f.H, bool)
    active[S.incidence(rows)[0]] = True
    out = api.stitch_lightmap(gpu_ctx, f.scene, f.charts, rgba, iterations=16)
    assert differing(out.reshape(-1, 4)[~active], rgba.reshape(-1, 4)[~active]) == 0 and 0 < active.sum() < f.owned.sum()
    assert differing(out[..., 3], rgba[..., 3]) == 0
    assert int((words(out.reshape(-1, 4)[active][:, :3]) != words(rgba.reshape(-1, 4)[active][:, :3])).sum()) > active.sum()
    # one constant colour: both sides of every seam already agree up to the rounding of the weights.  The bound is the float32
    # restatement's own deviation on this input, computed here.
    const = np.zeros_like(rgba)
    const[f.owned] = (0.7, 0.4, 0.2, 1.0)
    bound = float(np.abs(S.stitch(const, f.ref, 16)[0] - const).max())
    got = api.stitch_lightmap(gpu_ctx, f.scene, f.charts, const, iterations=16)
    print("constant atlas: the restatement's deviation", bound, "the device's", float(np.abs(got - const).max()))
    assert bound < 1e-5 and float(np.abs(got - const).max()) <= bound
    # a bow-tie has no seam: the input comes back bit for bit, with zero pairs
    b = fixture(gpu_ctx, "bowtie")
    atlas = S.random_atlas(b.owned, 9)
    out, info = api.stitch_lightmap(gpu_ctx, b.scene, b.charts, atlas, iterations=8, want_info=True)
    assert differing(out, atlas) == 0
    assert (info["seam_edges"], info["sample_pairs"], info["active_texels"], info["iterations"]) == (0, 0, 0, 0)


CAMERA = (api.CameraParams(is_orthographic=False, lens=0.035, film=0.036, aspect=1.0, focus=2.0, aperture=0.0), F([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, -2.0]]))


@pytest.mark.gpu
def test_bake_denoise_stitch_view_and_frames_that_do_not_notice(gpu_ctx):
    f = fixture(gpu_ctx, "cube")
    baked, rec = api.bake_lightmap(gpu_ctx, f.scene, f.charts, f.W, f.H, samples=4, max_bounces=2, surface_offset=1e-3, want_records=True)
    smooth = api.denoise_lightmap(gpu_ctx, baked, rec, dilate=1)
    stitched, info = api.stitch_lightmap(gpu_ctx, f.scene, f.charts, smooth, want_info=True)
    assert info["seam_edges"] == 12 and info["iterations"] == 32
    tex = api.Texture(gpu_ctx, 32, 32)
    g = api.render_lightmapped(gpu_ctx, f.scene, tex, CAMERA[0], CAMERA[1], f.charts, stitched, ambient=F([0.1, 0.1, 0.1]), ray_epsilon=1e-3,
                               want_gbuffer=True).reshape(-1, 20)
    source = words(g)[:, 19]
    lit = source == L.LIGHTMAP
    assert lit.sum() > 100 and np.all(source[~lit] == 0)      # every pixel that hits the cube reads the lightmap; the others miss
    assert np.all(np.isfinite(tex.download().astype(F)))

    def chain(stitch_after):
        res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=4, samples_per_pixel=2))
        out = api.DoubleBufferedTexture(gpu_ctx, 32, 32)
        between = None
        for k in range(6):
            desc = api.PathtraceDesc(accum_params=api.AccumulationParams(out.back(), k), camera_params=CAMERA[0], camera_transform=CAMERA[1])
            api.pathtrace_scene(gpu_ctx, res, f.scene, out.front(), PT.Standard, desc)
            out.flip()
            if k + 1 == stitch_after:
                between = api.stitch_lightmap(gpu_ctx, f.scene, f.charts, smooth)
        out.flip()
        return out.front().download(), between

    plain, _ = chain(None)
    with_stitch, between = chain(3)
    assert float(plain.astype(F)[..., :3].max()) > 0.0
    assert util.f16_words_differ(with_stitch, plain) == 0
    assert differing(between, stitched) == 0
    # stitching is in UV space: the moved scene stitches to the same words
    moved = np.array(f.cpu.instances, copy=True)
    moved["transpose_inverse_transform"][:, :, 3] = F([-0.25, 0.5, 0.125])
    f.scene.update_instances(moved)
    try:
        assert differing(api.stitch_lightmap(gpu_ctx, f.scene, f.charts, smooth), stitched) == 0
    finally:
        f.scene.update_instances(np.array(f.cpu.instances, copy=True))


@pytest.mark.gpu
def test_every_refusal_leaves_sentinels(gpu_ctx):
    f = fixture(gpu_ctx, "cube")
    lib = _abi.lib()
    rgba = S.random_atlas(f.owned, 2)
    ch = f.charts[0]
    inf, nan = float("inf"), float("nan")
    bare_cpu, _ = U.scene_cpu_of([cube_mesh()])
    bare = U.upload(gpu_ctx, bare_cpu)                        # a mesh with neither a lightmap UV set nor texcoords
    cases = []

    def case(label, ctx_h=None, scene_h=None, charts=f.charts, rgba_=rgba, no_out=False, **kw):
        out = np.full_like(rgba, -7.0)
        rc, info = raw_stitch(gpu_ctx.handle if ctx_h is None else ctx_h, f.scene.handle if scene_h is None else scene_h, charts, rgba_,
                              None if no_out else out, **kw)
        cases.append((label, rc, out, info))

    case("null context", ctx_h=C.c_void_p(None))
    case("null scene", scene_h=C.c_void_p(None))
    case("null desc", desc=False)
    case("null charts", charts=None, num_charts=1)
    case("null rgba", rgba_=None, W=f.W, H=f.H)
    case("null out_rgba", no_out=True)
    case("no charts", num_charts=0)
    case("width == 0", W=0)
    case("height == 0", H=0)
    case("width above 16384", W=16385)
    case("height above 16384", H=16385)
    case("iterations above the maximum", iterations=1025)
    for bad in (0.0, -2.0, nan, inf, -inf):
        case(f"samples_per_texel = {bad}", spt=bad)
        case(f"lambda = {bad}", lam=bad)
    case("unknown flag", flags=2)
    case("unknown flag beside the known one", flags=3)
    case("reserved != 0", reserved=1)
    case("a device pointer off its alignment", rgba_=C.c_void_p(rgba.ctypes.data + 4), flags=1, W=f.W, H=f.H)      # refused before anything reads it
    case("an instance out of range", charts=[api.LightmapChart(1, ch.scale_u, ch.scale_v, 0.0, 0.0)])
    case("a mesh with neither a set nor texcoords", scene_h=bare.handle)
    for k, field in enumerate(("scale_u", "scale_v", "offset_u", "offset_v")):
        vals = [ch.scale_u, ch.scale_v, ch.offset_u, ch.offset_v]
        vals[k] = (nan, inf, -inf, nan)[k]
        case(f"{field} not finite", charts=[api.LightmapChart(0, *vals)])
    other = api.Context(0)
    dead = C.c_void_p(other.handle.value)
    other.close()
    case("a destroyed context", ctx_h=dead)
    for label, rc, out, info in cases:
        assert rc == INVALID, (label, rc)
        assert lib.lupin_hip_last_error(), label
        assert np.all(out == -7.0), label
        assert (info.seam_edges, info.active_texels, info.iterations) == (77, 77, 77) and info.energy_before[0] == -7.0 and info.energy_after[2] == -7.0, label
    # out_info may be NULL, and the limits themselves pass
    out = np.full_like(rgba, -7.0)
    rc, _ = raw_stitch(gpu_ctx.handle, f.scene.handle, f.charts, rgba, out, iterations=1, info=False)
    assert rc == 0 and np.all(out != -7.0)
    rc, info = raw_stitch(gpu_ctx.handle, f.scene.handle, f.charts, rgba, out, iterations=1024, spt=1e-30, lam=1e30)
    assert rc == 0 and info.iterations == 1024 and info.sample_pairs == info.seam_edges == 12      # one sample an edge at the least
    for wrong in (rgba[..., :3], rgba[0]):
        with pytest.raises(ValueError):
            api.stitch_lightmap(gpu_ctx, f.scene, f.charts, wrong)
