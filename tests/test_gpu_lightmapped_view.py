"""The lightmapped view on the device (lupin_hip_render_lightmapped) against tests/lightmapped_view_ref.py WORD
FOR WORD -- texels and all 20 G-buffer words -- the pieces taken from the device's own api.camera_probe, api.trace_rays,
api.surface_probe and lookups: staged and global geometry, images whose rows straddle a wave and a block, atlases from
1 x 1 up, random atlases with ownership holes and real bakes, a duplicated instance, no volume and all three lookups, both f16
roundings, small launches, moved instances, device memory in place, torch tensors, every refusal, frames around the call,
and one closed form end to end."""
import ctypes as C
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import baked_view_ref as B
from tests import closest_hit_ref as X
from tests import film_ref
from tests import lightmapped_view_ref as L
from tests import util
from tests.test_gpu_baked_view import camera as case_camera
from tests.test_gpu_closest_hit import staged_in_lds
from tests.test_gpu_lightmap import THREE_CHARTS, add_mesh, constant_environment, matte, sphere_mesh, three_chart_cpu
from tests.test_gpu_probe_depth import deep_scene, place
from tests.test_gpu_probe_grid import grid_over, scene_box, words
from tests.test_lightmapped_view_cpu import AMBIENT, CAMERA, FLOOR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SENTINEL = np.float32(-7.0)
IMAGES = ((1, 1), (7, 5), (64, 1), (65, 3), (33, 17))          # rows that end inside a wave, on its end, one past it; more than one block
ATLASES = ((1, 1), (2, 2), (17, 33), (64, 64))                 # (width, height)
VOLUMES = ("none", "plain", "traced", "maps")
DIMS = (2, 2, 2)
R_MAPS, K_MAPS = 6, 2
EPS = 1e-3
_cache = {}


def test_the_entry_point_and_its_python_mirror_exist(built):
    assert hasattr(C.CDLL(_abi.LIB_PATH), "lupin_hip_render_lightmapped")
    assert callable(api.render_lightmapped) and C.sizeof(_abi.LightmappedViewDescC) == 152 + 16
    assert (api.LIGHTMAPPED_VIEW_GBUFFER_FLOATS, api.LIGHTMAPPED_SOURCE_MISS, api.LIGHTMAPPED_SOURCE_LIGHTMAP, api.LIGHTMAPPED_SOURCE_PROBES,
            api.LIGHTMAPPED_SOURCE_AMBIENT) == (20, 0, 1, 2, 3)


# ---- scenes: (cpu, scene, geometry, camera, box, charts) ------------------------------------------------------------------

def big_cpu(moved=False):
    """closest_hit_ref's `big` with texcoords on the grid and the blob meshes (meshes 1 and 2; the others have none)."""
    cpu = X.scene_cpu("big", X.SEED, X.transforms(X.SEED, moved=True) if moved else None)
    rng = np.random.default_rng(77)
    for m in (1, 2):
        cpu.mesh_infos[m]["texcoords_buf_idx"] = len(cpu.verts_texcoord_array)
        cpu.verts_texcoord_array.append(rng.uniform(0.0, 1.0, (len(cpu.verts_pos_array[m]), 2)).astype(F))
    api.validate_scene(cpu, 0, 0)
    return cpu


def setting(ctx, kind, moved=False):
    k = ("setting", id(ctx), kind, moved)
    if k not in _cache:
        if kind == "three":
            cpu, envs = three_chart_cpu(moved)
            api.validate_scene(cpu, 0, 0)
            scene = api.build_accel_structures_and_upload(ctx, cpu, [], envs, True)
            cam, box = CAMERA, (F([-4.0, -1.45, -1.5]), F([4.0, 1.6, 3.0]))
            charts = THREE_CHARTS + [FLOOR]
        else:
            cpu = big_cpu(moved)
            scene = api.build_accel_structures_and_upload(ctx, cpu, [], [], True)
            cam = case_camera("big", moved)
            lo, hi = scene_box(X.case("big", moved))
            box = (lo + F(0.2) * (hi - lo), hi - F(0.2) * (hi - lo))
            rng = np.random.default_rng(78)
            charted = [i for i in range(len(cpu.instances)) if int(cpu.instances[i]["mesh_idx"]) in (1, 2)]
            charts = [api.LightmapChart(i, *rng.uniform(0.2, 0.5, 2), *rng.uniform(0.0, 0.5, 2)) for i in charted]
            assert len(charts) >= 2
        assert staged_in_lds(ctx, scene) == (kind == "three")
        _cache[k] = SimpleNamespace(cpu=cpu, scene=scene, geo=L.geometry(cpu, scene), cam=cam, box=box, charts=charts)
    return _cache[k]



def probes(ctx, scene):
    return (lambda *a: api.camera_probe(ctx, *a), lambda o, d, e: api.trace_rays(ctx, scene, o, d, e), lambda r: api.surface_probe(ctx, scene, r))


def pieces(ctx, s, W, H):
    k = ("px", id(ctx), id(s), W, H)
    if k not in _cache:
        _cache[k] = L.pieces(*probes(ctx, s.scene), W, H, s.cam[0], s.cam[1], EPS)
    return _cache[k]


def volume(ctx, s, which):
    """(the device's own lookup as a function of records or None, render_lightmapped's keyword arguments for it)"""
    if which == "none":
        return None, {}
    k = ("volume", id(ctx), id(s))
    if k not in _cache:
        grid = grid_over(*s.box, DIMS)
        rng = np.random.default_rng(4100)
        sh = rng.normal(size=(8, 9, 4)).astype(F)
        sh[:, 0, :3] += F(2.0)
        holes = np.array([1, 1, 0, 1, 1, 1, 0, 1], np.uint8)
        _, maps, maxd = api.bake_probe_grid_depth(ctx, s.scene, *grid, R_MAPS, K_MAPS)
        _cache[k] = (grid, sh, holes, maps, maxd)
    grid, sh, holes, maps, maxd = _cache[k]
    where = dict(origin=grid[0], spacing=grid[1], dims=grid[2], sh=sh, valid=holes, normal_bias=0.0)
    if which == "maps":
        return (lambda rec: api.sample_probe_grid_depth(ctx, s.scene, *grid, sh, maps, rec, max_distance=maxd, valid=holes, normal_bias=0.0),
                dict(where, depth=maps, max_distance=maxd))
    vis = which == "traced"
    return (lambda rec: api.sample_probe_grid(ctx, s.scene, *grid, sh, rec, valid=holes, visibility=vis, ray_epsilon=EPS, normal_bias=0.0),
            dict(where, visibility=vis))


def random_atlas(AW, AH, seed=0):
    rng = np.random.default_rng(900 + 7 * AW + AH + seed)
    atlas = rng.uniform(0.05, 3.0, (AH, AW, 4)).astype(F)
    atlas[..., 3] = rng.uniform(size=(AH, AW)) > 0.35                     # ownership holes
    return atlas


def render(ctx, s, W, H, charts, atlas, kw, max_slots=0, scene=None):
    """(texels (W * H, 4) uint16, gbuffer (W * H, 20) float32) of api.render_lightmapped into a fresh texture."""
    tex = api.Texture(ctx, W, H)
    tex.upload(np.full((H, W, 4), SENTINEL, np.float16))
    g = api.render_lightmapped(ctx, scene or s.scene, tex, s.cam[0], s.cam[1], charts, atlas, ambient=AMBIENT, ray_epsilon=EPS, want_gbuffer=True,
                               max_slots=max_slots, **kw)
    assert g.shape == (H, W, 20) and g.dtype == np.float32
    return tex.download().view(np.uint16).reshape(-1, 4), g.reshape(-1, 20)


def assert_same(got, want, label):
    tex, g = got
    wt, wg = want
    bad = np.nonzero((words(g) != words(wg)).any(axis=1))[0]
    assert len(bad) == 0, (label, "gbuffer", bad[:5], g[bad[:3]], wg[bad[:3]])
    bad = np.nonzero((tex != wt).any(axis=1))[0]
    assert len(bad) == 0, (label, "texels", bad[:5], tex[bad[:3]], wt[bad[:3]])


# ---- 1. word for word -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", VOLUMES)
@pytest.mark.parametrize("kind", ["three", "big"])
def test_word_for_word_against_the_restatement(gpu_ctx, kind, which):
    s = setting(gpu_ctx, kind)
    lookup, kw = volume(gpu_ctx, s, which)
    twice = [s.charts[0], api.LightmapChart(s.charts[0].instance_idx, 0.3, 0.2, 0.6, 0.7)] + s.charts[1:]          # a duplicated instance
    sources = np.zeros(4, np.int64)
    for W, H in IMAGES:
        px = pieces(gpu_ctx, s, W, H)
        for AW, AH in ATLASES:
            for charts in ((s.charts, twice, s.charts[:-1]) if (AW, AH) == (17, 33) else (s.charts,)):          # the last: the floor uncharted
                atlas = random_atlas(AW, AH)
                want = L.render(px, s.geo, charts, atlas, lookup, AMBIENT, film_ref.RTZ)
                got = render(gpu_ctx, s, W, H, charts, atlas, kw)
                assert_same(got, want, (kind, which, W, H, AW, AH, len(charts)))
                if (W, H) == (33, 17):
                    sources += np.bincount(words(want[1])[:, 19], minlength=4)
    print(kind, which, "pixels by source (miss, lightmap, probes, ambient):", sources.tolist())
    assert sources[L.MISS] > 100 and sources[L.LIGHTMAP] > 100 and (sources[L.AMBIENT] > 0 or which != "none"), sources
    assert (sources[L.PROBES] > 20) == (which != "none"), sources


@pytest.mark.parametrize("dilate", [0, 2])
def test_a_real_bake_word_for_word(gpu_ctx, dilate):
    s = setting(gpu_ctx, "three")
    px = pieces(gpu_ctx, s, 33, 17)
    lookup, kw = volume(gpu_ctx, s, "maps")
    for AW, AH in ((17, 33), (64, 64)):
        atlas = api.bake_lightmap(gpu_ctx, s.scene, s.charts, AW, AH, samples=1, dilate=dilate)
        assert 0.1 < (atlas[..., 3] != 0).mean() < 1.0
        got = render(gpu_ctx, s, 33, 17, s.charts, atlas, kw)
        assert_same(got, L.render(px, s.geo, s.charts, atlas, lookup, AMBIENT, film_ref.RTZ), (dilate, AW, AH))
        lm = words(got[1])[:, 19] == L.LIGHTMAP
        assert lm.sum() > 100 and (got[1][lm, 11] > 0).mean() > 0.8          # most lightmapped pixels find an owned tap


def test_no_charts_and_a_volume_is_render_baked_bit_for_bit(gpu_ctx):
    for kind in ("three", "big"):
        s = setting(gpu_ctx, kind)
        for which in ("plain", "traced", "maps"):
            _, kw = volume(gpu_ctx, s, which)
            tex, g = render(gpu_ctx, s, 33, 17, [], random_atlas(2, 2), kw)
            base = api.Texture(gpu_ctx, 33, 17)
            bkw = {k: v for k, v in kw.items() if k not in ("origin", "spacing", "dims", "sh")}
            bg = api.render_baked(gpu_ctx, s.scene, base, s.cam[0], s.cam[1], kw["origin"], kw["spacing"], kw["dims"], kw["sh"], ambient=AMBIENT,
                                  ray_epsilon=EPS, want_gbuffer=True, **bkw)
            assert np.array_equal(tex, base.download().view(np.uint16).reshape(-1, 4))
            assert np.array_equal(words(g[:, 0:16]), words(bg.reshape(-1, 16))) and (g[:, 11] > 0).sum() > 50
            assert not g[:, 16:18].any() and np.all(words(g)[:, 18] == api.BAKED_VIEW_MISS)


# ---- 2. the store's rounding, the launch size, moved instances -----------------------------------------------------------

def test_both_store_roundings(built):
    """The switch is the context's: a context of this test's own, so that no other test sees it."""
    ctx = api.Context(0)
    try:
        s = setting(ctx, "three")
        px = pieces(ctx, s, 33, 17)
        lookup, kw = volume(ctx, s, "plain")
        atlas = random_atlas(17, 33)
        seen = {}
        for mode in (film_ref.RNE, film_ref.RTZ):
            ctx.set_f16_store_rounding(mode)
            got = render(ctx, s, 33, 17, s.charts, atlas, kw)
            assert_same(got, L.render(px, s.geo, s.charts, atlas, lookup, AMBIENT, mode), mode)
            seen[mode] = got[0]
        assert int((seen[film_ref.RNE] != seen[film_ref.RTZ]).sum()) > 100
    finally:
        for k in [k for k in _cache if k[1] == id(ctx)]:
            del _cache[k]
        ctx.close()


@pytest.mark.parametrize("which", ["none", "traced"])
def test_the_picture_does_not_depend_on_max_slots(gpu_ctx, which):
    for kind in ("three", "big"):
        s = setting(gpu_ctx, kind)
        _, kw = volume(gpu_ctx, s, which)
        atlas = random_atlas(17, 33)
        for W, H in ((65, 3), (33, 17)):
            whole = render(gpu_ctx, s, W, H, s.charts, atlas, kw)
            for max_slots in (64, 100):          # 100 rounds to 64
                assert_same(render(gpu_ctx, s, W, H, s.charts, atlas, kw, max_slots=max_slots), whole, (kind, which, W, H, max_slots))


@pytest.mark.parametrize("tlas_builder", ["cpu", "device"])
def test_after_update_instances_the_view_equals_a_fresh_scenes(gpu_ctx, tlas_builder):
    s, fresh = setting(gpu_ctx, "big"), setting(gpu_ctx, "big", moved=True)
    scene = api.build_accel_structures_and_upload(gpu_ctx, big_cpu(), [], [], True)          # a scene of its own: it is changed in place
    _, kw = volume(gpu_ctx, s, "traced")
    atlas = random_atlas(17, 33)
    before = render(gpu_ctx, s, 33, 17, s.charts, atlas, kw, scene=scene)
    scene.update_instances(X.instance_records(X.transforms(X.SEED, moved=True)), tlas_builder=tlas_builder)
    after = render(gpu_ctx, s, 33, 17, s.charts, atlas, kw, scene=scene)
    assert_same(after, render(gpu_ctx, s, 33, 17, s.charts, atlas, kw, scene=fresh.scene), tlas_builder)
    px = L.pieces(*probes(gpu_ctx, fresh.scene), 33, 17, s.cam[0], s.cam[1], EPS)
    grid, sh, holes = kw["origin"], kw["sh"], kw["valid"]
    lookup = lambda rec: api.sample_probe_grid(gpu_ctx, fresh.scene, kw["origin"], kw["spacing"], kw["dims"], sh, rec, valid=holes, visibility=True,
                                               ray_epsilon=EPS, normal_bias=0.0)
    assert_same(after, L.render(px, fresh.geo, s.charts, atlas, lookup, AMBIENT, film_ref.RTZ), "restatement")
    assert int((before[0] != after[0]).any(axis=1).sum()) > 20           # the move is visible


# ---- 3. device memory in place, torch ------------------------------------------------------------------------------------

def raw_call(ctx, s, W, H, charts, atlas, tex, g=None, sh=None, depth=None, valid=None, device=False, offset=0, **over):
    """lupin_hip_render_lightmapped itself: (status, gbuffer (H, W, 20)).  device: the atlas and the G-buffer in device memory,
    the atlas `offset` bytes into its allocation."""
    f = dict(ctx_h=ctx.handle, scene_h=s.scene.handle, tex_h=tex.handle, desc=True, null_atlas=False, null_charts=False, flags=0, eps=EPS,
             ambient=tuple(AMBIENT), width=atlas.shape[1], height=atlas.shape[0], num_charts=len(charts), reserved=0, max_slots=0, grid=None,
             resolution=R_MAPS, max_distance=1.0)
    f.update(over)
    d = _abi.LightmappedViewDescC()
    cp = s.cam[0]
    d.view.camera_params = _abi.CameraParamsC(1 if cp.is_orthographic else 0, cp.lens, cp.film, cp.aspect, cp.focus, cp.aperture)
    for col in range(4):
        for row in range(3):
            d.view.camera_transform.m[col][row] = float(s.cam[1][col][row])
    if f["grid"] is not None:
        d.view.grid = f["grid"]
    d.view.resolution, d.view.max_distance, d.view.ray_epsilon, d.view.max_slots = f["resolution"], f["max_distance"], f["eps"], f["max_slots"]
    d.view.flags = f["flags"] | (api.BAKED_VIEW_DEVICE_POINTERS if device else 0)
    d.view.ambient = (C.c_float * 3)(*f["ambient"])
    d.lightmap_width, d.lightmap_height, d.num_charts, d.reserved = f["width"], f["height"], f["num_charts"], f["reserved"]
    cc = (_abi.LightmapChartC * max(1, len(charts)))(*[_abi.LightmapChartC(int(c.instance_idx), c.scale_u, c.scale_v, c.offset_u, c.offset_v) for c in charts])
    g = np.full((H, W, 20), SENTINEL, F) if g is None else g
    if device:
        d_atlas, d_g = place(ctx, atlas, offset), place(ctx, g)
        p_atlas, p_g = C.c_void_p(d_atlas.ptr + offset), C.c_void_p(d_g.ptr)
    else:
        p_atlas, p_g = _abi.ptr(np.ascontiguousarray(atlas, F)), _abi.ptr(g)
    rc = _abi.lib().lupin_hip_render_lightmapped(f["ctx_h"], f["scene_h"], f["tex_h"], C.byref(d) if f["desc"] else None, None if f["null_charts"] else cc,
                                                 None if f["null_atlas"] else p_atlas, _abi.ptr(sh), _abi.ptr(depth), _abi.ptr(valid), p_g)
    if device:
        g = d_g.download(np.uint8, W * H * 80).view(F).reshape(H, W, 20)
    return rc, g


def test_device_pointers_give_the_host_arrays_words(gpu_ctx):
    s = setting(gpu_ctx, "big")
    atlas = random_atlas(17, 33)
    want = render(gpu_ctx, s, 65, 3, s.charts, atlas, {})
    for max_slots in (0, 64):
        tex = api.Texture(gpu_ctx, 65, 3)
        rc, g = raw_call(gpu_ctx, s, 65, 3, s.charts, atlas, tex, device=True, max_slots=max_slots)
        assert rc == 0, _abi.lib().lupin_hip_last_error()
        assert_same((tex.download().view(np.uint16).reshape(-1, 4), g.reshape(-1, 20)), want, max_slots)


def test_torch_tensors_give_the_same_words():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_lightmapped_view_torch_worker.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "LIGHTMAPPED VIEW TORCH OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- 4. refusals ----------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_sentinels_in_the_target_and_the_gbuffer(gpu_ctx):
    s = setting(gpu_ctx, "three")
    W, H = 7, 5
    atlas = random_atlas(17, 33)
    tex = api.Texture(gpu_ctx, W, H)
    tex.upload(np.full((H, W, 4), SENTINEL, np.float16))
    _, kw = volume(gpu_ctx, s, "maps")
    sh, maps, holes = kw["sh"], kw["depth"], kw["valid"]

    def grid(origin=None, spacing=None, dims=None, flags=api.PROBE_GRID_BACKFACE, eps=EPS, bias=0.0):
        return _abi.ProbeGridDescC((C.c_float * 3)(*(origin or kw["origin"])), (C.c_float * 3)(*(spacing or kw["spacing"])),
                                   (C.c_uint32 * 3)(*(dims or kw["dims"])), flags, eps, bias)

    cases = []

    def call(label, charts=s.charts, atlas_=atlas, **over):
        rc, g = raw_call(gpu_ctx, s, W, H, charts, atlas_, tex, **over)
        cases.append((label, rc, g, _abi.lib().lupin_hip_last_error().decode()))
        return rc

    call("null context", ctx_h=None)
    call("null scene", scene_h=None)
    call("null target", tex_h=None)
    call("null desc", desc=False)
    call("null lightmap", null_atlas=True)
    call("null charts with num_charts > 0", null_charts=True)
    call("unknown flag", flags=2)
    for label, v in (("NaN", np.nan), ("infinite", np.inf)):
        call(f"{label} ambient", ambient=(0.1, v, 0.1))
    for label, v in (("NaN", np.nan), ("infinite", np.inf), ("negative", -1e-3)):
        call(f"{label} ray_epsilon", eps=v)
    for label, wh in (("zero width", (0, 33)), ("zero height", (17, 0)), ("width above the maximum", (16385, 33)), ("height above the maximum", (17, 16385))):
        call(label, width=wh[0], height=wh[1])
    call("reserved", reserved=1)
    call("chart instance out of range", charts=s.charts + [api.LightmapChart(5, 1, 1, 0, 0)])
    call("chart on a mesh without texcoords", charts=s.charts + [api.LightmapChart(4, 1, 1, 0, 0)])
    assert "no texcoords" in cases[-1][3]
    for k, v in enumerate((np.nan, np.inf, -np.inf, np.nan)):
        c = [1.0, 1.0, 0.0, 0.0]
        c[k] = v
        call(f"chart with a non-finite field {k}", charts=[api.LightmapChart(0, *c)])
    call("depth without sh", depth=maps)
    call("valid without sh", valid=holes)
    # what render_baked refuses in the grid, with sh only
    call("unknown grid flag", sh=sh, grid=grid(flags=8))
    call("DEVICE_POINTERS in the grid's flags", sh=sh, grid=grid(flags=api.PROBE_GRID_DEVICE_POINTERS))
    call("VISIBILITY with depth maps", sh=sh, depth=maps, grid=grid(flags=api.PROBE_GRID_VISIBILITY))
    call("NaN origin", sh=sh, grid=grid(origin=(np.nan, 0, 0)))
    call("zero spacing", sh=sh, grid=grid(spacing=(1, 0, 1)))
    call("zero dim", sh=sh, grid=grid(dims=(2, 0, 2)))
    call("negative normal_bias", sh=sh, grid=grid(bias=-1.0))
    for r in (0, 1, 65):
        call(f"resolution {r}", sh=sh, depth=maps, grid=grid(), resolution=r)
    for label, v in (("NaN", np.nan), ("zero", 0.0)):
        call(f"{label} max_distance", sh=sh, depth=maps, grid=grid(), max_distance=v)
    other = api.Context(0)
    foreign = setting(other, "three")
    foreign_tex = api.Texture(other, W, H)
    call("scene of another context", scene_h=foreign.scene.handle)
    call("target of another context", tex_h=foreign_tex.handle)
    for k in [k for k in _cache if k[1] == id(other)]:
        del _cache[k]
    other.close()
    call("scene of a destroyed context", scene_h=foreign.scene.handle)
    call("target of a destroyed context", tex_h=foreign_tex.handle)
    call("hierarchy too deep", scene_h=deep_scene(gpu_ctx).handle, charts=[])
    assert "too deep" in cases[-1][3]
    call("misaligned device lightmap", device=True, offset=8)
    for label, rc, g, said in cases:
        assert rc == -1, (label, rc, said)
        assert np.all(g == SENTINEL), label
    assert len(cases) >= 40
    assert np.all(tex.download() == np.float16(SENTINEL))                              # the target was never touched
    # accepted: without sh the grid, resolution and max_distance may hold anything; what follows a refusal is unharmed
    assert call("accepted", grid=grid(spacing=(0, 0, 0), dims=(0, 0, 0), flags=99), resolution=0, max_distance=np.nan, max_slots=1) == 0
    px = pieces(gpu_ctx, s, W, H)
    assert_same((tex.download().view(np.uint16).reshape(-1, 4), cases[-1][2].reshape(-1, 20)), L.render(px, s.geo, s.charts, atlas, None, AMBIENT), "after the refusals")


# ---- 5. frames around the call; the closed form -------------------------------------------------------------------------

def test_frames_around_a_view_do_not_notice_it(gpu_ctx):
    W, H = 64, 48
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cam = cams[0]
    s = setting(gpu_ctx, "three")
    atlas = random_atlas(17, 33)
    alone = render(gpu_ctx, s, 40, 30, s.charts, atlas, {})

    def chain(call_after):
        res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=8, samples_per_pixel=2))
        out = api.DoubleBufferedTexture(gpu_ctx, W, H)
        for k in range(6):
            desc = api.PathtraceDesc(accum_params=api.AccumulationParams(out.back(), k), camera_params=cam.params, camera_transform=cam.transform)
            api.pathtrace_scene(gpu_ctx, res, scene, out.front(), api.PathtraceType.Standard, desc)
            out.flip()
            if k + 1 == call_after:
                assert_same(render(gpu_ctx, s, 40, 30, s.charts, atlas, {}), alone, "between frames")
        out.flip()
        return out.front().download()

    plain = chain(None)
    assert util.f16_words_differ(chain(3), plain) == 0
    assert util.f16_words_differ(plain, util.oracle_accumulate(scene, cam, W, H, frames=6, spp=2)) == 0


def test_a_sphere_under_a_constant_sky_end_to_end(gpu_ctx):
    """One unit sphere alone under a constant environment of 0.5, baked into one 32 x 32 chart with 4 samples and two gutter
    passes: the sphere is convex, so every path meets the sky and every owned texel is exactly pi * 0.5f; a gutter texel is a
    mean of such texels.  A hit pixel is then emission (0) + (0.7f * E) * 0.31830988f with E = pi * 0.5f up to step 7's
    roundings.  In units of u = 2^-24 relative: the gutter's mean (a sum of up to 8 equal terms and a division: 9 u, as loose
    as it can be), step 7's products (u), three additions (3 u), cov's three additions (3 u) and the division (u), step 9's
    two products (2 u), the literals pi (f32: u) and 0.31830988f (u): 21 u, and one f16 step of the store (2^-10, toward
    zero) on top."""
    cpu = api.SceneCPU()
    infos = []
    pos, tris, uv, nrm = sphere_mesh()
    add_mesh(cpu, infos, pos, tris, uv, nrm)
    cpu.mesh_infos = np.array(infos, _abi.MESH_INFO_DTYPE)
    cpu.materials = np.array([matte(0.7)], _abi.MATERIAL_DTYPE)
    cpu.instances = np.array([api.default_instance()], _abi.INSTANCE_DTYPE)
    envs = constant_environment(cpu, 0.5)
    api.validate_scene(cpu, 0, 0)
    scene = api.build_accel_structures_and_upload(gpu_ctx, cpu, [], envs, True)
    chart = [api.LightmapChart(0, 1.0, 1.0, 0.0, 0.0)]
    atlas = api.bake_lightmap(gpu_ctx, scene, chart, 32, 32, samples=4, dilate=2)
    owned = atlas[..., 3] != 0
    assert owned.sum() > 500 and np.all(atlas[owned][:, 0:3] == F(np.pi) * F(0.5))
    tex = api.Texture(gpu_ctx, 33, 17)
    cam = (api.CameraParams(is_orthographic=False, lens=0.035, film=0.036, aspect=1.5, focus=3.0, aperture=0.0), F([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -3.0]]))
    g = api.render_lightmapped(gpu_ctx, scene, tex, cam[0], cam[1], chart, atlas, want_gbuffer=True).reshape(-1, 20)
    rgb = tex.download().astype(np.float64).reshape(-1, 4)[:, 0:3]
    hit = words(g)[:, 3] != api.BAKED_VIEW_MISS
    assert 50 < hit.sum() < len(g) - 50 and np.all(words(g)[hit, 19] == L.LIGHTMAP) and np.all(g[hit, 11] > 0)
    want = 0.7 * 0.5
    bound = want * (21 * 2.0 ** -24 + 2.0 ** -10)
    print("largest |pixel - 0.35| =", np.abs(rgb[hit] - want).max(), "bound", bound)
    assert np.all(np.abs(rgb[hit] - want) <= bound), np.abs(rgb[hit] - want).max()
    assert np.all(rgb[~hit] == 0.5)
