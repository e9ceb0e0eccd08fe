"""Reprojection of the adaptive history on the device (lupin_hip_adaptive_reproject, csrc/lupin_reproject.hpp):
the primary trace against lupin_hip_trace_rays on the restated centre rays, the identity, parity of the gather with
tests/reproject_ref.py on the device's own visibility buffers, continuation by the next adaptive call, quality against
resetting, and errors / ordering / determinism."""
import os

import numpy as np
import pytest

from lupinpathtracer_amd import api
from tests import reproject_ref as R
from tests import util

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_SAME_TARGET = -1, -6
NOTHING = api.AdaptiveParams(threshold=0.0, min_frames=0)   # no block ever converges: every call renders every pixel
BLACK = np.array([0, 0, 0, 1], np.float16)


@pytest.fixture(scope="module")
def global_ctx(built):
    """A context whose kernels read every scene from global memory (GeoGlobal), as tests/test_gpu_ray_query.py makes one."""
    old = os.environ.get("LUPIN_LDS_GEOMETRY")
    os.environ["LUPIN_LDS_GEOMETRY"] = "0"     # read at context creation: small scenes stay in global memory
    try:
        ctx = api.Context(0)
    finally:
        if old is None:
            os.environ.pop("LUPIN_LDS_GEOMETRY", None)
        else:
            os.environ["LUPIN_LDS_GEOMETRY"] = old
    yield ctx
    for key in [k for k in util._scene_cache if k[1] == id(ctx)]:
        del util._scene_cache[key]
    ctx.close()


def _params(cam, W, H, ortho=False):
    d = dict(cam.params.__dict__)
    d.update(aspect=W / H, aperture=0.0)
    if ortho:
        d.update(is_orthographic=True, lens=d["film"] / 2.6)   # the film spans 2.6 world units: the Cornell box
    return api.CameraParams(**d)


def _moved(transform, dx, dy, dz, yaw=0.0):
    """The camera transform translated along its own axes and turned about its y axis."""
    m = np.asarray(transform, np.float64).reshape(4, 3)
    rot, pos = m[:3].T, m[3]
    c, s = np.cos(yaw), np.sin(yaw)
    rot2 = rot @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.concatenate([rot2.T, (pos + rot @ np.array([dx, dy, dz]))[None]], 0).astype(np.float32)


class Session:
    """Resources of one W x H sequence: out.back() holds the history, out.front() is written next."""

    def __init__(self, ctx, scene, W, H, spp=2):
        self.ctx, self.scene, self.W, self.H = ctx, scene, W, H
        self.res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(max_bounces=8, samples_per_pixel=spp))
        self.out = api.DoubleBufferedTexture(ctx, W, H)
        self.ares = api.build_adaptive_resources(ctx, W, H)
        self.rp = api.build_reproject_resources(ctx, W, H)

    def reproject(self, cp, tr, **kw):
        api.adaptive_reproject(self.ctx, self.ares, self.rp, self.scene, api.ReprojectDesc(camera_params=cp, camera_transform=tr, **kw),
                               self.out.back(), self.out.front())
        self.out.flip()

    def frames(self, cp, tr, count, base=0):
        for _ in range(count):
            api.pathtrace_scene_adaptive(self.ctx, self.res, self.scene, self.out.front(), 0,
                                         api.PathtraceDesc(accum_params=api.AccumulationParams(self.out.back(), base), camera_params=cp,
                                                           camera_transform=tr), self.ares, NOTHING)
            self.out.flip()

    def history(self):
        return self.out.back().download()


@pytest.mark.parametrize("geometry", ["lds", "global"])
@pytest.mark.parametrize("W,H", [(64, 48), (97, 61)])
@pytest.mark.parametrize("name", ["cornellbox_builtin", "instances1"])
def test_primary_trace_is_trace_rays_on_the_centre_rays(gpu_ctx, global_ctx, name, W, H, geometry):
    ctx = gpu_ctx if geometry == "lds" else global_ctx
    scene, cams = util.load_scene(name, ctx)
    cp, tr = _params(cams[0], W, H), cams[0].transform
    s = Session(ctx, scene, W, H)
    s.reproject(cp, tr)
    inst, tri, uv, depth = s.rp.download(0)
    ori, d = R.centre_rays(W, H, cp, tr)
    hit, dst, uv_t, inst_t, tri_t = api.trace_rays(ctx, scene, ori.reshape(-1, 3), d.reshape(-1, 3), 0.001)
    hit = hit.astype(bool).reshape(H, W)
    assert hit.any()
    assert np.array_equal(inst != R.MISS, hit)
    assert np.array_equal(inst[hit], inst_t.reshape(H, W)[hit])
    assert np.array_equal(tri[hit], R.global_triangle(scene, inst_t, tri_t).reshape(H, W)[hit])
    assert np.array_equal(uv.view(np.uint32)[hit], uv_t.reshape(H, W, 2).view(np.uint32)[hit])
    want = R.depth_of(tr, ori.reshape(-1, 3), d.reshape(-1, 3), dst).reshape(H, W)
    assert np.array_equal(depth.view(np.uint32)[hit], want.view(np.uint32)[hit])
    assert (tri[~hit] == 0).all() and (uv[~hit] == 0).all() and (depth[~hit] == 0).all()
    # a first call has no previous view: nothing survives
    f, m, _, act = s.ares.download()
    assert (f == 0).all() and (m == 0).all() and act.all() and (s.history() == BLACK).all()


@pytest.mark.parametrize("mode", ["f16", "f32"])
@pytest.mark.parametrize("W,H", [(64, 48), (97, 61)])
def test_unmoved_view_is_an_exact_copy(gpu_ctx, W, H, mode):
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cp, tr = _params(cams[0], W, H), cams[0].transform
    f32 = mode == "f32"
    if f32:
        gpu_ctx.set_accumulation_mode(1)
    try:
        s = Session(gpu_ctx, scene, W, H)
        s.reproject(cp, tr)
        s.frames(cp, tr, 4)
        before16, before32 = s.history(), (s.out.back().download_f32() if f32 else None)
        f0, m0, _, _ = s.ares.download()
        s.reproject(cp, tr, depth_tolerance=0.02)
        hit = s.rp.download(0)[0] != R.MISS
        after16, after32 = s.history(), (s.out.back().download_f32() if f32 else None)
        f1, m1, err, act = s.ares.download()
        assert hit.mean() > 0.9 and (f0 == 4).all()
        if f32:
            assert np.array_equal(after32.view(np.uint32)[hit], before32.view(np.uint32)[hit])
            assert np.array_equal(after16[..., :3], after32[..., :3].astype(np.float16))   # nearest even, whatever the store mode
        else:
            assert np.array_equal(after16.view(np.uint16)[hit], before16.view(np.uint16)[hit])
        assert np.array_equal(f1[hit], f0[hit]) and np.array_equal(m1.view(np.uint32)[hit], m0.view(np.uint32)[hit])
        assert (f1[~hit] == 0).all() and (m1[~hit] == 0).all() and (after16[~hit] == BLACK).all()
        assert act.all() and np.isinf(err).all()
        st = s.ares.stats()
        assert (st.active_pixels, st.pixel_frames, st.max_frames_taken) == (W * H, int(f1.sum()), int(f1.max()))
        # a cap of 2
        s.reproject(cp, tr, depth_tolerance=0.02, max_history=2)
        f2, m2, _, _ = s.ares.download()
        assert (f2[hit] == 2).all() and np.array_equal(m2[..., 0], m1[..., 0])
        assert np.array_equal(m2[..., 1][hit], ((m1[..., 1] / np.float32(4.0)) * np.float32(2.0))[hit])
        assert np.array_equal(s.history().view(np.uint16), after16.view(np.uint16))
        assert s.ares.stats().pixel_frames == int(f2.sum())
    finally:
        gpu_ctx.set_accumulation_mode(0)


def _moved_setup(ctx, W, H, ortho, spp=2):
    """Four frames of view A, then the camera moves and turns by a few pixels and the short box moves: everything the
    restatement needs, before the reprojection to view B."""
    scene, cams = util.load_scene("cornellbox_builtin", ctx)
    cp, tr = _params(cams[0], W, H, ortho), cams[0].transform
    s = Session(ctx, scene, W, H, spp)
    s.reproject(cp, tr)
    s.frames(cp, tr, 4)
    old = scene.instances["transpose_inverse_transform"].copy()
    new = old.copy()
    new[5] = api.instance_from_transform(np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [-0.12, 0.0, 0.05]], np.float32), 5, 0)["transpose_inverse_transform"]
    tr2 = _moved(tr, 0.07, -0.03, 0.05, yaw=0.012)
    return scene, s, cp, tr, tr2, old, new


@pytest.mark.parametrize("mode", ["f16", "f32"])
@pytest.mark.parametrize("ortho", [False, True], ids=["perspective", "orthographic"])
def test_gather_matches_the_restatement(gpu_ctx, ortho, mode):
    """frames equal everywhere; colour within 1 f16 ulp and moments within 1 f32 ulp on at most 0.1 % of the pixels (the aim,
    and the measurement recorded in DESIGN.md 16: zero differing words).  In f32 accumulation mode the colour is gathered
    from history_in's accumulator, and history_out's accumulator is held to the restatement's f32 colour in the same way."""
    W, H = 97, 61
    f32 = mode == "f32"
    if f32:
        gpu_ctx.set_accumulation_mode(1)
    scene = None
    try:
        scene, s, cp, tr, tr2, old, new = _moved_setup(gpu_ctx, W, H, ortho)
        hist_in = s.out.back().download_f32()[..., :3] if f32 else s.history()[..., :3].astype(np.float32)
        f0, m0, _, _ = s.ares.download()
        scene.update_instances(new)
        s.reproject(cp, tr2, depth_tolerance=0.02, prev_instance_transforms=old)
        cur, prev = s.rp.download(0), s.rp.download(1)
        got16 = s.history()
        got32 = s.out.back().download_f32() if f32 else None
        f1, m1, _, _ = s.ares.download()
        tris, _ = R.scene_triangles(scene)
        want32, want16, wn, wm = R.gather(cur, prev, cp, tr, tris, R.local_to_world_rows(old), f0, m0, hist_in, 0.02)
    finally:
        gpu_ctx.set_accumulation_mode(0)
        if scene is not None:
            scene.update_instances(old)
    hit = cur[0] != R.MISS
    kept = f1 > 0
    print(f"ortho={ortho}: {int(kept.sum())} of {int(hit.sum())} hit pixels keep history; n histogram {np.bincount(f1.reshape(-1)).tolist()}")
    assert kept.mean() > 0.5 and (hit & ~kept).sum() > 20, "the move must keep most pixels and disocclude some"
    assert np.array_equal(f1, wn)
    dc = np.abs(got16.view(np.int16).astype(np.int32) - want16.view(np.int16).astype(np.int32)).max(-1)
    dm = np.abs(m1.view(np.int32).astype(np.int64) - wm.view(np.int32).astype(np.int64)).max(-1)
    print(f"ortho={ortho}: pixels with differing colour words {int((dc > 0).sum())}, moment words {int((dm > 0).sum())} of {W * H}")
    assert dc.max() <= 1 and dm.max() <= 1
    assert (dc > 0).sum() <= W * H // 1000 and (dm > 0).sum() <= W * H // 1000
    if f32:
        assert (got32[..., 3] == 1.0).all()
        d32 = np.abs(got32[..., :3].view(np.int32).astype(np.int64) - want32.view(np.int32).astype(np.int64)).max(-1)
        print(f"ortho={ortho}: pixels with differing f32 accumulator words {int((d32 > 0).sum())} of {W * H}")
        assert d32.max() <= 1 and (d32 > 0).sum() <= W * H // 1000


@pytest.mark.parametrize("base", [0, 5])
def test_the_next_adaptive_call_continues_every_pixel(gpu_ctx, base):
    """After a reprojection one adaptive call equals, at pixel p, lupin_hip_pathtrace_scene with accum_counter base + n_p blending
    into history_out (k_resolve's blend); pixels with n_p = 0 are a plain frame at counter base, checked against the oracle."""
    from oracle import oracle
    W, H = 64, 48
    scene, s, cp, tr, tr2, old, new = _moved_setup(gpu_ctx, W, H, False)
    try:
        scene.update_instances(new)
        s.reproject(cp, tr2, depth_tolerance=0.02, prev_instance_transforms=old)
        n = s.ares.download()[0]
        hist = s.out.back()
        plain = api.DoubleBufferedTexture(gpu_ctx, W, H)
        want = np.zeros((H, W, 4), np.uint16)
        for c in np.unique(n):
            api.pathtrace_scene(gpu_ctx, s.res, scene, plain.front(), 0,
                                api.PathtraceDesc(accum_params=api.AccumulationParams(hist, base + int(c)), camera_params=cp, camera_transform=tr2))
            want[n == c] = plain.front().download().view(np.uint16)[n == c]
        hist16 = hist.download()
        s.frames(cp, tr2, 1, base=base)
        got = s.history().view(np.uint16)
        n1 = s.ares.download()[0]
        ref, _ = oracle.pathtrace(scene, W, H, cp, tr2, 8, 2, 0, accum_counter=base, prev_frame=hist16)
    finally:
        scene.update_instances(old)
    assert len(np.unique(n)) >= 2 and (n == 0).sum() > 20
    assert np.array_equal(got, want)
    assert np.array_equal(n1, n + 1)
    fresh = n == 0
    g, r = got.view(np.float16)[fresh], ref[fresh]
    diff = np.abs(g.astype(np.float32) - r.astype(np.float32))
    nbad = util.f16_words_differ(g, r)
    print(f"fresh pixels vs oracle: max |diff| {diff.max():.3e}, differing words {nbad} / {g.size}")
    assert diff.max() <= 1e-2 and nbad <= max(1, g.size // 1000)   # the smoke test's bound for device vs oracle


def _relmse(x, ref):
    x, ref = x[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 1e-2)))


def test_reprojection_beats_resetting_on_a_dolly(gpu_ctx):
    """Eight dolly steps of a few pixels, one adaptive frame per step: with the history reprojected at every step the last
    image is closer (relMSE of DESIGN.md 9) to a converged render of the last view than with a reset at every step."""
    W = H = 128
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cp, tr = _params(cams[0], W, H), cams[0].transform
    views = [_moved(tr, 0.03 * k, 0.01 * k, 0.04 * k) for k in range(9)]
    a = Session(gpu_ctx, scene, W, H)
    a.reproject(cp, views[0])
    a.frames(cp, views[0], 1)
    for v in views[1:]:
        a.reproject(cp, v, depth_tolerance=0.02)
        a.frames(cp, v, 1)
    b = Session(gpu_ctx, scene, W, H)
    for v in views:
        b.ares.reset()
        b.frames(cp, v, 1)
    ref = util.gpu_accumulate(gpu_ctx, scene, type(cams[0])(transform=views[-1], params=cp), W, H, 96, 8).astype(np.float32)
    e_rp, e_reset = _relmse(a.history().astype(np.float32), ref), _relmse(b.history().astype(np.float32), ref)
    print(f"dolly relMSE: reprojected {e_rp:.4e}  reset {e_reset:.4e}  ratio {e_rp / e_reset:.3f}; mean n_p {a.ares.download()[0].mean():.2f}")
    assert e_rp < e_reset


def test_errors_leave_everything_untouched(gpu_ctx):
    """Every refusal of lupin_hip.h but LUPIN_ERR_NO_SW_BVH: lupin_hip_scene_create makes no scene without a TLAS, so that
    branch cannot be reached from here."""
    W, H = 64, 48
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cp, tr = _params(cams[0], W, H), cams[0].transform
    s = Session(gpu_ctx, scene, W, H)
    s.reproject(cp, tr)
    s.frames(cp, tr, 2)
    before = (s.out.back().download(), s.out.front().download(), *s.ares.download())
    other, small = api.Context(0), api.Texture(gpu_ctx, 32, 32)
    try:
        desc = api.ReprojectDesc(camera_params=cp, camera_transform=tr)
        xforms = scene.instances["transpose_inverse_transform"]
        singular = xforms.copy()
        singular[2] = 0.0
        cases = [
            (ERR_SAME_TARGET, dict(history_out=s.out.back())),
            (ERR_INVALID, dict(history_out=small)),
            (ERR_INVALID, dict(history_in=small)),
            (ERR_INVALID, dict(adaptive_resources=api.build_adaptive_resources(gpu_ctx, 32, 32))),
            (ERR_INVALID, dict(resources=api.build_reproject_resources(gpu_ctx, 32, 32))),
            (ERR_INVALID, dict(history_out=api.Texture(other, W, H))),
            (ERR_INVALID, dict(desc=api.ReprojectDesc(camera_params=cp, camera_transform=tr, depth_tolerance=-0.5))),
            (ERR_INVALID, dict(desc=api.ReprojectDesc(camera_params=cp, camera_transform=tr, depth_tolerance=float("nan")))),
            (ERR_INVALID, dict(desc=api.ReprojectDesc(camera_params=cp, camera_transform=tr, depth_tolerance=float("inf")))),
            (ERR_INVALID, dict(desc=api.ReprojectDesc(camera_params=cp, camera_transform=tr, prev_instance_transforms=xforms[:-1]))),
            (ERR_INVALID, dict(desc=api.ReprojectDesc(camera_params=cp, camera_transform=tr, prev_instance_transforms=singular))),
        ]
        for code, change in cases:
            kw = dict(adaptive_resources=s.ares, resources=s.rp, scene=scene, desc=desc, history_in=s.out.back(), history_out=s.out.front())
            kw.update(change)
            with pytest.raises(api.LupinError) as e:
                api.adaptive_reproject(gpu_ctx, **kw)
            assert e.value.code == code, (change, e.value)
        lib, h = api.lib(), lambda o: o.handle
        import ctypes as C
        from lupinpathtracer_amd import _abi
        c = _abi.ReprojectDescC()
        args = [gpu_ctx.handle, h(s.ares), h(s.rp), h(scene), C.byref(c), h(s.out.back()), h(s.out.front())]
        for k in range(len(args)):
            assert lib.lupin_hip_adaptive_reproject(*[None if j == k else v for j, v in enumerate(args)]) == ERR_INVALID
        after = (s.out.back().download(), s.out.front().download(), *s.ares.download())
        for x, y in zip(before, after):
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        # the previous view survived the refused calls: an unmoved view still keeps its history
        s.reproject(cp, tr)
        assert (s.ares.download()[0][s.rp.download(0)[0] != R.MISS] == 2).all()
    finally:
        other.close()


def test_ordering_determinism_and_invalidate(gpu_ctx):
    W, H = 97, 61
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    cp, tr = _params(cams[0], W, H), cams[0].transform
    tr2 = _moved(tr, 0.05, 0.02, 0.0, yaw=0.01)

    def run(plain_frames):
        """View A's history comes from ordinary pathtrace calls that may still be recorded when the reprojection is called."""
        s = Session(gpu_ctx, scene, W, H)
        s.reproject(cp, tr)
        s.frames(cp, tr, 1)
        for k in range(plain_frames):   # recorded (batched) calls whose last target is history_in
            api.pathtrace_scene(gpu_ctx, s.res, scene, s.out.front(), 0,
                                api.PathtraceDesc(accum_params=api.AccumulationParams(s.out.back(), 1 + k), camera_params=cp, camera_transform=tr))
            s.out.flip()
        s.reproject(cp, tr2, depth_tolerance=0.02)
        return s, s.history().view(np.uint16), s.ares.download()

    s1, img1, st1 = run(3)
    s2, img2, st2 = run(3)
    assert np.array_equal(img1, img2) and all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(st1, st2))
    # the recorded frames were seen: the result differs from reprojecting the history before them, and equals the restatement
    _, img0, _ = run(0)
    assert not np.array_equal(img1, img0)
    hist = util.gpu_accumulate(gpu_ctx, scene, type(cams[0])(transform=tr, params=cp), W, H, 4, 2)
    tris, _ = R.scene_triangles(scene)
    rows = R.local_to_world_rows(scene.instances["transpose_inverse_transform"])
    ones = np.ones((H, W), np.uint32)
    _, want, _, _ = R.gather(s1.rp.download(0), s1.rp.download(1), cp, tr, tris, rows, ones, np.zeros((H, W, 2), np.float32),
                             hist[..., :3].astype(np.float32), 0.02)
    assert np.array_equal(img1, want.view(np.uint16))
    # invalidate: the next call keeps nothing
    s1.rp.invalidate()
    s1.reproject(cp, tr2)
    f, m, _, act = s1.ares.download()
    assert (f == 0).all() and (m == 0).all() and act.all() and (s1.history() == BLACK).all()
