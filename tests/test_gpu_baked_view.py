"""The baked-lighting view on the device (lupin_hip_render_baked) against tests/baked_view_ref.py WORD FOR WORD,
the pieces taken from the device's own api.camera_probe, api.trace_rays, api.surface_probe and api.sample_probe_grid /
api.sample_probe_grid_depth: staged and global geometry, images whose rows straddle a wave and a block, three grids, all
three lookups on baked and on dense synthetic maps, validity holes, the backface weight, two biases, both f16 roundings,
launches of 64 pixels, the G-buffer re-fed to the lookups, a sky and a lamp, moved instances, an aperture, device memory in
place, torch tensors, every refusal, frames around the call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import baked_view_ref as B
from tests import closest_hit_ref as X
from tests import film_ref
from tests import util
from tests.test_baked_view_cpu import AMBIENT, SKY
from tests.test_gpu_closest_hit import device_scene, staged_in_lds
from tests.test_gpu_probe_depth import deep_scene, place
from tests.test_gpu_probe_grid import grid_over, scene_box, words

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SENTINEL = np.float32(-7.0)
IMAGES = ((1, 1), (7, 5), (64, 1), (65, 3), (33, 17))          # rows that end inside a wave, on its end, one past it; more than one block
GRIDS = ((2, 2, 2), (3, 2, 4), (4, 1, 3))
LOOKUPS = ("plain", "traced", "baked", "dense")
R_MAPS, K_MAPS = 6, 2
EPS = 1e-3
_cache = {}


def test_the_entry_point_and_its_python_mirror_exist(built):
    assert hasattr(C.CDLL(_abi.LIB_PATH), "lupin_hip_render_baked")
    assert callable(api.render_baked) and C.sizeof(_abi.BakedViewDescC) == 152
    assert (api.BAKED_VIEW_GBUFFER_FLOATS, api.BAKED_VIEW_MISS, api.BAKED_VIEW_DEVICE_POINTERS) == (16, 0xFFFFFFFF, 1)


def camera(kind, moved=False, aperture=0.0):
    """A perspective camera in front of the case's box, looking along +z at its centre: hits amid misses."""
    lo, hi = scene_box(X.case(kind, moved))
    centre, extent = (lo + hi) / 2, float((hi - lo).max())
    xf = F([[1, 0, 0], [0, 1, 0], [0, 0, 1], [centre[0], centre[1], lo[2] - 0.9 * extent]])
    return api.CameraParams(is_orthographic=False, lens=0.035, film=0.036, aspect=1.5, focus=0.9 * extent, aperture=aperture), xf


def probes(ctx, scene):
    return (lambda *a: api.camera_probe(ctx, *a), lambda o, d, e: api.trace_rays(ctx, scene, o, d, e), lambda r: api.surface_probe(ctx, scene, r))


def pieces(ctx, scene, key, W, H, cam, eps=EPS):
    k = ("px", id(ctx), key, W, H, eps)
    if k not in _cache:
        _cache[k] = B.pieces(*probes(ctx, scene), W, H, cam[0], cam[1], eps)
    return _cache[k]


def volume(ctx, scene, kind, dims):
    """(grid, sh, valid with holes, baked maps, dense synthetic maps, max_distance) of a grid among the case's instances."""
    k = ("volume", id(ctx), kind, dims)
    if k not in _cache:
        lo, hi = scene_box(X.case(kind))
        grid = grid_over(lo + F(0.2) * (hi - lo), hi - F(0.2) * (hi - lo), dims)
        P = int(np.prod(dims))
        rng = np.random.default_rng(4000 + 10 * GRIDS.index(dims) + (kind == "big"))
        sh = rng.normal(size=(P, 9, 4)).astype(F)
        sh[:, 0, :3] += F(2.0)
        holes = (rng.uniform(size=P) > 0.33).astype(np.uint8)
        _, baked, maxd = api.bake_probe_grid_depth(ctx, scene, *grid, R_MAPS, K_MAPS)
        dense = np.empty_like(baked)                       # surfaces close to every probe: every branch of the depth test at work
        dense[..., 0] = rng.uniform(0.05, 0.6, baked.shape[:-1]) * maxd
        dense[..., 1] = dense[..., 0] * dense[..., 0] + rng.uniform(0.0, 0.05 * maxd * maxd, baked.shape[:-1])
        _cache[k] = (grid, sh, holes, baked, dense, maxd)
    return _cache[k]


def lookup_of(ctx, scene, vol, which, valid, back, bias, eps=EPS):
    """(the device's own lookup as a function of records, render_baked's keyword arguments for the same lookup)"""
    grid, sh, _, baked, dense, maxd = vol
    if which in ("baked", "dense"):
        maps = baked if which == "baked" else dense
        return (lambda rec: api.sample_probe_grid_depth(ctx, scene, *grid, sh, maps, rec, max_distance=maxd, valid=valid, backface=back, normal_bias=bias),
                dict(depth=maps, max_distance=maxd, valid=valid, backface=back, normal_bias=bias))
    vis = which == "traced"
    return (lambda rec: api.sample_probe_grid(ctx, scene, *grid, sh, rec, valid=valid, visibility=vis, backface=back, ray_epsilon=eps, normal_bias=bias),
            dict(valid=valid, visibility=vis, backface=back, normal_bias=bias))


def render(ctx, scene, W, H, cam, vol, kw, ambient=AMBIENT, eps=EPS, max_slots=0):
    """(texels (W * H, 4) uint16, gbuffer (W * H, 16) float32) of api.render_baked into a fresh texture."""
    tex = api.Texture(ctx, W, H)
    tex.upload(np.full((H, W, 4), SENTINEL, np.float16))
    g = api.render_baked(ctx, scene, tex, cam[0], cam[1], *vol[0], vol[1], ambient=ambient, ray_epsilon=eps, want_gbuffer=True, max_slots=max_slots, **kw)
    assert g.shape == (H, W, 16) and g.dtype == np.float32
    return tex.download().view(np.uint16).reshape(-1, 4), g.reshape(-1, 16)


def assert_same(got, want, label):
    tex, g = got
    wt, wg = want
    bad = np.nonzero((words(g) != words(wg)).any(axis=1))[0]
    assert len(bad) == 0, (label, "gbuffer", bad[:5], g[bad[:3]], wg[bad[:3]])
    bad = np.nonzero((tex != wt).any(axis=1))[0]
    assert len(bad) == 0, (label, "texels", bad[:5], tex[bad[:3]], wt[bad[:3]])


# ---- 1. word for word -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", LOOKUPS)
@pytest.mark.parametrize("kind", ["small", "big"])
def test_word_for_word_against_the_restatement(gpu_ctx, kind, which):
    scene = device_scene(gpu_ctx, kind)
    assert staged_in_lds(gpu_ctx, scene) == (kind == "small")
    cam = camera(kind)
    default_bias = api.LIGHTMAP_OFFSET_FRACTION * api.scene_world_extent(scene)
    hits = misses = answered = unanswered = calls = 0
    for W, H in IMAGES:
        px = pieces(gpu_ctx, scene, kind, W, H, cam)
        for dims in GRIDS:
            vol = volume(gpu_ctx, scene, kind, dims)
            for valid in (None, vol[2]):
                for back in (False, True):
                    for bias in (0.0, default_bias):
                        lookup, kw = lookup_of(gpu_ctx, scene, vol, which, valid, back, bias)
                        want = B.render(px, lookup, AMBIENT, film_ref.RTZ)
                        got = render(gpu_ctx, scene, W, H, cam, vol, kw)
                        assert_same(got, want, (kind, which, W, H, dims, valid is not None, back, bias))
                        assert np.all(got[0][:, 3] == film_ref.ALPHA_ONE)
                        calls += 1
                        if (W, H) == (33, 17):
                            h = px.hit
                            hits, misses = hits + int(h.sum()), misses + int((~h).sum())
                            answered, unanswered = answered + int((want[1][h, 11] > 0).sum()), unanswered + int((want[1][h, 11] == 0).sum())
    assert calls == len(IMAGES) * len(GRIDS) * 8
    assert hits > 500 and misses > 500 and answered > 500, (hits, misses, answered, unanswered)


def test_pixels_no_probe_answers_show_ambient(gpu_ctx):
    scene = device_scene(gpu_ctx, "small")
    cam = camera("small")
    vol = volume(gpu_ctx, scene, "small", (2, 2, 2))
    px = pieces(gpu_ctx, scene, "small", 33, 17, cam)
    for which in ("plain", "dense"):
        lookup, kw = lookup_of(gpu_ctx, scene, vol, which, np.zeros(8, np.uint8), True, 0.0)
        tex, g = render(gpu_ctx, scene, 33, 17, cam, vol, kw)
        assert_same((tex, g), B.render(px, lookup, AMBIENT, film_ref.RTZ), which)
        h = px.hit
        assert h.sum() > 50 and np.all(g[:, 11] == 0)
        assert np.array_equal(tex[h], B.texels(px.emission[h] + (px.color[h] * AMBIENT) * B.INV_PI, film_ref.RTZ))


# ---- 2. the store's rounding, the launch size ------------------------------------------------------------------------

def test_both_store_roundings(built):
    """The switch is the context's: a context of this test's own, so that no other test sees it."""
    ctx = api.Context(0)
    try:
        scene = X.build("small", X.SEED, ctx)
        cam = camera("small")
        vol = volume(ctx, scene, "small", (3, 2, 4))
        px = pieces(ctx, scene, "small", 33, 17, cam)
        lookup, kw = lookup_of(ctx, scene, vol, "dense", vol[2], True, 0.0)
        seen = {}
        for mode in (film_ref.RNE, film_ref.RTZ):
            ctx.set_f16_store_rounding(mode)
            got = render(ctx, scene, 33, 17, cam, vol, kw)
            assert_same(got, B.render(px, lookup, AMBIENT, mode), mode)
            seen[mode] = got[0]
        assert int((seen[film_ref.RNE] != seen[film_ref.RTZ]).sum()) > 100          # about half of the words of the lit pixels
    finally:
        ctx.close()


@pytest.mark.parametrize("which", ["traced", "baked"])
def test_the_picture_does_not_depend_on_max_slots(gpu_ctx, which):
    for kind in ("small", "big"):
        scene = device_scene(gpu_ctx, kind)
        cam = camera(kind)
        vol = volume(gpu_ctx, scene, kind, (3, 2, 4))
        _, kw = lookup_of(gpu_ctx, scene, vol, which, vol[2], True, 0.0)
        for W, H in ((65, 3), (33, 17)):
            whole = render(gpu_ctx, scene, W, H, cam, vol, kw)
            for max_slots in (64, 1, 100, 200):          # 1 and 100 round to 64, 200 to 192
                assert_same(render(gpu_ctx, scene, W, H, cam, vol, kw, max_slots=max_slots), whole, (kind, which, W, H, max_slots))


# ---- 3. the G-buffer ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", LOOKUPS)
def test_the_gbuffers_records_refed_to_the_lookup_reproduce_it(gpu_ctx, which):
    scene = device_scene(gpu_ctx, "big")
    cam = camera("big")
    vol = volume(gpu_ctx, scene, "big", (3, 2, 4))
    lookup, kw = lookup_of(gpu_ctx, scene, vol, which, vol[2], True, 0.0)
    tex, g = render(gpu_ctx, scene, 33, 17, cam, vol, kw)
    hit = words(g)[:, 3] != api.BAKED_VIEW_MISS
    assert 50 < hit.sum() < len(g) - 50
    res = lookup(g[hit, 0:8])
    assert np.array_equal(words(res[:, 3]), words(g[hit, 11]))
    E = np.where((res[:, 3] != 0)[:, None], res[:, 0:3], AMBIENT)
    assert np.array_equal(tex[hit], B.texels(g[hit, 12:15] + (g[hit, 8:11] * E) * B.INV_PI, film_ref.RTZ))
    assert np.array_equal(tex[~hit], B.texels(g[~hit, 12:15], film_ref.RTZ)) and not np.delete(words(g)[~hit], [3, 12, 13, 14], axis=1).any()
    # without a G-buffer the picture is the same
    plain = api.Texture(gpu_ctx, 33, 17)
    assert api.render_baked(gpu_ctx, scene, plain, cam[0], cam[1], *vol[0], vol[1], ambient=AMBIENT, ray_epsilon=EPS, **kw) is None
    assert np.array_equal(plain.download().view(np.uint16).reshape(-1, 4), tex)


# ---- 4. a sky and a lamp; moved instances; an aperture ------------------------------------------------------------------

def sky_cornell(ctx):
    from lupinpathtracer_amd import loader
    if ("sky", id(ctx)) not in _cache:
        cpu, cams = loader.cornell_box_scene_cpu()
        env = api.default_environment()
        env["emission"] = F(SKY)
        cpu.environments = np.array([env], api.ENVIRONMENT_DTYPE)
        api.validate_scene(cpu, 0, 0)
        _cache["sky", id(ctx)] = api.build_accel_structures_and_upload(ctx, cpu, [], [api.EnvMapInfo(np.ones((1, 1, 4), F), 1, 1)], True), cams[0]
    return _cache["sky", id(ctx)]


def test_a_sky_a_lamp_and_normals_that_face_away(gpu_ctx):
    scene, c = sky_cornell(gpu_ctx)
    grid = (F([-0.9, 0.1, -0.9]), F([0.6, 0.6, 0.9]), (4, 4, 3))
    sh = np.random.default_rng(5).normal(size=(48, 9, 4)).astype(F)
    _, maps, maxd = api.bake_probe_grid_depth(gpu_ctx, scene, *grid, 8, 2)
    vol = (grid, sh, None, maps, maps, maxd)
    back = np.array(c.transform, F).copy()
    back[3] = [0.0, 1.0, -7.0]
    behind = F([[-1, 0, 0], [0, 1, 0], [0, 0, -1], [0, 1, 7.0]])
    flipped = kept = lamp = sky = 0
    for name, W, H, xf in (("inside", 24, 24, c.transform), ("far", 17, 11, back), ("behind", 12, 13, behind)):
        cam = (c.params, xf)
        px = pieces(gpu_ctx, scene, "sky " + name, W, H, cam)
        for which in ("traced", "baked"):
            lookup, kw = lookup_of(gpu_ctx, scene, vol, which, None, True, None)
            got = render(gpu_ctx, scene, W, H, cam, vol, kw)
            assert_same(got, B.render(px, lookup, AMBIENT, film_ref.RTZ), (name, which))
        facing = (px.d * px.ns).sum(axis=1)
        flipped, kept = flipped + int((px.hit & (facing > 0)).sum()), kept + int((px.hit & (facing < 0)).sum())
        lamp, sky = lamp + int((px.emission.max(axis=1) > 0).sum()), sky + int((~px.hit).sum())
        assert np.all(px.env[~px.hit] == F(SKY)) and np.all(got[0][~px.hit, 0:3] == B.texels(F([SKY]), film_ref.RTZ)[0, 0:3])
    assert flipped > 100 and kept > 20 and lamp >= 2 and sky > 100


@pytest.mark.parametrize("tlas_builder", ["cpu", "device"])
def test_after_update_instances_the_view_equals_a_fresh_scenes(gpu_ctx, tlas_builder):
    moved = X.transforms(X.SEED, moved=True)
    scene = X.build("big", X.SEED, gpu_ctx)                              # a scene of its own: it is changed in place
    cam = camera("big", aperture=0.2)                                    # RAY_CENTRE ignores the aperture
    vol = volume(gpu_ctx, device_scene(gpu_ctx, "big"), "big", (3, 2, 4))
    _, kw = lookup_of(gpu_ctx, scene, vol, "traced", None, True, 0.0)
    before = render(gpu_ctx, scene, 33, 17, cam, vol, kw)
    scene.update_instances(X.instance_records(moved), tlas_builder=tlas_builder)          # (the four-wide hierarchy is stale from here on)
    fresh = X.build("big", X.SEED, gpu_ctx, xf=moved)
    after = render(gpu_ctx, scene, 33, 17, cam, vol, kw)
    assert_same(after, render(gpu_ctx, fresh, 33, 17, cam, vol, kw), tlas_builder)
    px = B.pieces(*probes(gpu_ctx, fresh), 33, 17, cam[0], cam[1], EPS)
    assert_same(after, B.render(px, lookup_of(gpu_ctx, fresh, vol, "traced", None, True, 0.0)[0], AMBIENT, film_ref.RTZ), "restatement")
    assert int((before[0] != after[0]).any(axis=1).sum()) > 20           # the move is visible
    pinhole = (api.CameraParams(is_orthographic=False, lens=0.035, film=0.036, aspect=1.5, focus=cam[0].focus, aperture=0.0), cam[1])
    assert_same(render(gpu_ctx, fresh, 33, 17, pinhole, vol, kw), after, "aperture")


def test_an_orthographic_camera(gpu_ctx):
    scene = device_scene(gpu_ctx, "small")
    lo, hi = scene_box(X.case("small"))
    extent = float((hi - lo).max())
    cam = (api.CameraParams(is_orthographic=True, lens=0.036 / (1.2 * extent), film=0.036, aspect=1.5, focus=extent, aperture=0.0), camera("small")[1])
    vol = volume(gpu_ctx, scene, "small", (2, 2, 2))
    lookup, kw = lookup_of(gpu_ctx, scene, vol, "plain", None, False, 0.0)
    px = B.pieces(*probes(gpu_ctx, scene), 33, 17, cam[0], cam[1], EPS)
    assert 20 < px.hit.sum() < px.hit.size
    assert_same(render(gpu_ctx, scene, 33, 17, cam, vol, kw), B.render(px, lookup, AMBIENT, film_ref.RTZ), "ortho")


# ---- 5. device memory in place --------------------------------------------------------------------------------------

def device_render(ctx, scene, W, H, cam, vol, which, valid=None, flags=api.BAKED_VIEW_DEVICE_POINTERS, grid_flags=api.PROBE_GRID_BACKFACE, offsets=(0, 0, 0),
                  gbuffer=True, max_slots=0):
    """lupin_hip_render_baked on texture memory: (status, texels, gbuffer); offsets: bytes added to sh, depth, out_gbuffer."""
    grid, sh, _, baked, dense, maxd = vol
    maps = None if which in ("plain", "traced") else baked if which == "baked" else dense
    d_sh = place(ctx, sh, offsets[0])
    d_maps = place(ctx, maps, offsets[1]) if maps is not None else None
    d_valid = place(ctx, valid) if valid is not None else None
    d_g = place(ctx, np.full(W * H * 16, SENTINEL, F), offsets[2])
    tex = api.Texture(ctx, W, H)
    tex.upload(np.full((H, W, 4), SENTINEL, np.float16))
    desc = _abi.BakedViewDescC()
    cp = cam[0]
    desc.camera_params = _abi.CameraParamsC(1 if cp.is_orthographic else 0, cp.lens, cp.film, cp.aspect, cp.focus, cp.aperture)
    for col in range(4):
        for row in range(3):
            desc.camera_transform.m[col][row] = float(cam[1][col][row])
    desc.grid = _abi.ProbeGridDescC((C.c_float * 3)(*grid[0]), (C.c_float * 3)(*grid[1]), (C.c_uint32 * 3)(*grid[2]),
                                    grid_flags | (api.PROBE_GRID_VISIBILITY if which == "traced" else 0), EPS, 0.0)
    desc.resolution, desc.max_distance, desc.ray_epsilon, desc.flags, desc.max_slots = R_MAPS, float(maxd), EPS, flags, max_slots
    desc.ambient = (C.c_float * 3)(*AMBIENT)
    rc = _abi.lib().lupin_hip_render_baked(ctx.handle, scene.handle, tex.handle, C.byref(desc), C.c_void_p(d_sh.ptr + offsets[0]),
                                           C.c_void_p(d_maps.ptr + offsets[1]) if d_maps else None, C.c_void_p(d_valid.ptr) if d_valid else None,
                                           C.c_void_p(d_g.ptr + offsets[2]) if gbuffer else None)
    g = d_g.download(np.uint8, offsets[2] + W * H * 64)[offsets[2]:].view(F).reshape(-1, 16)
    return rc, tex.download().view(np.uint16).reshape(-1, 4), g


def test_device_pointers_give_the_host_arrays_words(gpu_ctx):
    scene = device_scene(gpu_ctx, "big")
    cam = camera("big")
    vol = volume(gpu_ctx, scene, "big", (3, 2, 4))
    for which in LOOKUPS:
        for valid in (None, vol[2]):
            _, kw = lookup_of(gpu_ctx, scene, vol, which, valid, True, 0.0)
            want = render(gpu_ctx, scene, 65, 3, cam, vol, kw)
            for max_slots in (0, 64):
                rc, tex, g = device_render(gpu_ctx, scene, 65, 3, cam, vol, which, valid, max_slots=max_slots)
                assert rc == 0
                assert_same((tex, g), want, (which, valid is not None, max_slots))
    rc, tex, g = device_render(gpu_ctx, scene, 65, 3, cam, vol, "dense", offsets=(0, 8, 0), gbuffer=False)          # maps: 8-byte aligned
    assert rc == 0 and np.all(g == SENTINEL)
    assert np.array_equal(tex, render(gpu_ctx, scene, 65, 3, cam, vol, lookup_of(gpu_ctx, scene, vol, "dense", None, True, 0.0)[1])[0])


def test_torch_tensors_give_the_same_words():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_baked_view_torch_worker.py")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0 and "BAKED VIEW TORCH OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- 6. refusals ----------------------------------------------------------------------------------------------------

def test_every_refusal_leaves_sentinels_in_the_target_and_the_gbuffer(gpu_ctx):
    scene = device_scene(gpu_ctx, "small")
    lib = _abi.lib()
    cam = camera("small")
    vol = volume(gpu_ctx, scene, "small", (2, 2, 2))
    grid, sh, _, baked, dense, maxd = vol
    W, H = 7, 5
    tex = api.Texture(gpu_ctx, W, H)
    tex.upload(np.full((H, W, 4), SENTINEL, np.float16))
    INVALID = -1
    cases = []

    def call(label, ctx_h=gpu_ctx.handle, scene_h=scene.handle, tex_h=tex.handle, desc=True, sh_=sh, depth=None, **over):
        f = dict(origin=tuple(grid[0]), spacing=tuple(grid[1]), dims=grid[2], grid_flags=api.PROBE_GRID_BACKFACE, grid_eps=EPS, bias=0.0, resolution=R_MAPS,
                 max_distance=float(maxd), eps=EPS, ambient=tuple(AMBIENT), flags=0, max_slots=0)
        f.update(over)
        d = _abi.BakedViewDescC()
        cp = cam[0]
        d.camera_params = _abi.CameraParamsC(0, cp.lens, cp.film, cp.aspect, cp.focus, cp.aperture)
        for col in range(4):
            for row in range(3):
                d.camera_transform.m[col][row] = float(cam[1][col][row])
        d.grid = _abi.ProbeGridDescC((C.c_float * 3)(*f["origin"]), (C.c_float * 3)(*f["spacing"]), (C.c_uint32 * 3)(*f["dims"]), f["grid_flags"], f["grid_eps"],
                                     f["bias"])
        d.resolution, d.max_distance, d.ray_epsilon, d.flags, d.max_slots = f["resolution"], f["max_distance"], f["eps"], f["flags"], f["max_slots"]
        d.ambient = (C.c_float * 3)(*f["ambient"])
        g = np.full((H, W, 16), SENTINEL, F)
        rc = lib.lupin_hip_render_baked(ctx_h, scene_h, tex_h, C.byref(d) if desc else None, _abi.ptr(sh_), _abi.ptr(depth), None, _abi.ptr(g))
        cases.append((label, rc, g, lib.lupin_hip_last_error().decode()))
        return rc

    call("null context", ctx_h=None)
    call("null scene", scene_h=None)
    call("null target", tex_h=None)
    call("null desc", desc=False)
    call("null sh", sh_=None)
    call("unknown flag", flags=2)
    for label, v in (("NaN", np.nan), ("infinite", np.inf), ("-infinite", -np.inf)):
        call(f"{label} ambient", ambient=(0.1, v, 0.1))
    for label, v in (("NaN", np.nan), ("infinite", np.inf), ("negative", -1e-3)):
        call(f"{label} ray_epsilon", eps=v)
    # what the chosen lookup refuses
    call("unknown grid flag", grid_flags=8)
    call("DEVICE_POINTERS in the grid's flags", grid_flags=api.PROBE_GRID_DEVICE_POINTERS)
    call("VISIBILITY with depth maps", depth=baked, grid_flags=api.PROBE_GRID_VISIBILITY)
    assert "belongs to lupin_hip_sample_probe_grid" in cases[-1][3]
    call("NaN origin", origin=(np.nan, 0, 0))
    call("zero spacing", spacing=(1, 0, 1))
    call("negative spacing", depth=baked, spacing=(1, 1, -1))
    call("zero dim", dims=(2, 0, 2))
    call("more than 2^31 probes", dims=(1 << 16, 1 << 15, 2))
    call("non-finite last probe", spacing=(3e38, 1.0, 1.0), dims=(3, 1, 1))
    call("NaN grid ray_epsilon", grid_eps=np.nan)
    call("negative normal_bias", bias=-1.0)
    for r in (0, 1, 65):
        call(f"resolution {r}", depth=baked, resolution=r)
    for label, v in (("NaN", np.nan), ("infinite", np.inf), ("zero", 0.0), ("negative", -1.0)):
        call(f"{label} max_distance", depth=baked, max_distance=v)
    other = api.Context(0)
    foreign = X.build("small", X.SEED, other)
    foreign_tex = api.Texture(other, W, H)
    call("scene of another context", scene_h=foreign.handle)
    call("target of another context", tex_h=foreign_tex.handle)
    other.close()
    call("scene of a destroyed context", scene_h=foreign.handle)
    call("target of a destroyed context", tex_h=foreign_tex.handle)
    call("hierarchy too deep", scene_h=deep_scene(gpu_ctx).handle)
    assert "too deep" in cases[-1][3]
    for which, offs in (("plain", (8, 0, 0)), ("dense", (0, 4, 0)), ("plain", (0, 0, 8))):
        rc, t, g = device_render(gpu_ctx, scene, W, H, cam, vol, which, offsets=offs)
        cases.append((f"misaligned device pointer {offs}", rc, g, ""))
        assert np.all(t.view(np.float16) == np.float16(SENTINEL))
    for label, rc, g, said in cases:
        assert rc == INVALID, (label, rc, said)
        assert np.all(g == SENTINEL), label
    assert len(cases) >= 38
    assert np.all(tex.download() == np.float16(SENTINEL))                              # the target was never touched
    # the Python mirror refuses a target of another format before the library is asked
    fake = type("T", (), {"format": lambda self: "Rgba8Unorm", "width": W, "height": H, "handle": tex.handle})()
    with pytest.raises(api.LupinError) as e:
        api.render_baked(gpu_ctx, scene, fake, cam[0], cam[1], *grid, sh)
    assert e.value.code == INVALID and np.all(tex.download() == np.float16(SENTINEL))
    # accepted: the unused fields of a call without maps may hold anything; what follows a refusal is unharmed
    assert call("accepted", resolution=0, max_distance=np.nan, max_slots=1) == 0
    px = pieces(gpu_ctx, scene, "small", W, H, cam)
    lookup, _ = lookup_of(gpu_ctx, scene, vol, "plain", None, True, 0.0)
    assert_same((tex.download().view(np.uint16).reshape(-1, 4), cases[-1][2].reshape(-1, 16)), B.render(px, lookup, AMBIENT, film_ref.RTZ), "after the refusals")


# ---- 7. frames around the call --------------------------------------------------------------------------------------

def test_frames_around_a_view_do_not_notice_it(gpu_ctx):
    W, H = 64, 48
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cam = cams[0]
    grid = (F([-0.9, 0.1, -0.9]), F([0.6, 0.6, 0.9]), (4, 4, 3))
    sh = np.random.default_rng(71).normal(size=(48, 9, 4)).astype(F)
    _, maps, maxd = api.bake_probe_grid_depth(gpu_ctx, scene, *grid, 8, 2)
    view = api.Texture(gpu_ctx, 40, 30)

    def baked_view():
        g = api.render_baked(gpu_ctx, scene, view, cam.params, cam.transform, *grid, sh, depth=maps, max_distance=maxd, ambient=AMBIENT, want_gbuffer=True)
        return view.download().view(np.uint16).copy(), g

    alone = baked_view()

    def chain(call_after):
        res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=8, samples_per_pixel=2))
        out = api.DoubleBufferedTexture(gpu_ctx, W, H)
        for k in range(6):
            desc = api.PathtraceDesc(accum_params=api.AccumulationParams(out.back(), k), camera_params=cam.params, camera_transform=cam.transform)
            api.pathtrace_scene(gpu_ctx, res, scene, out.front(), api.PathtraceType.Standard, desc)
            out.flip()
            if k + 1 == call_after:
                got = baked_view()
                assert np.array_equal(got[0], alone[0]) and np.array_equal(words(got[1]), words(alone[1]))
        out.flip()
        return out.front().download()

    plain = chain(None)
    assert util.f16_words_differ(chain(3), plain) == 0
    assert util.f16_words_differ(plain, util.oracle_accumulate(scene, cam, W, H, frames=6, spp=2)) == 0
    px = B.pieces(*probes(gpu_ctx, scene), 40, 30, cam.params, cam.transform, EPS)
    lookup = lambda rec: api.sample_probe_grid_depth(gpu_ctx, scene, *grid, sh, maps, rec, max_distance=maxd, backface=True)
    assert_same((alone[0].reshape(-1, 4), alone[1].reshape(-1, 16)), B.render(px, lookup, AMBIENT, film_ref.RTZ), "alone")
