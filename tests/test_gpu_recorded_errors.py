"""The error of a recorded pathtrace_scene call is reported by the call that runs the batch (include/lupin_hip.h, "Frames per
wavefront"; DESIGN.md 5, "Recorded frames run first").

Under default batching a render of a scene whose hierarchy is too deep for the LDS stack is only recorded and returns OK; the
refusal (traversal_lds, before any launch) belongs to whichever call needs the batch next.  For each such observing call:
it raises the render's own error, it leaves the arrays its caller supplied untouched, the same call repeated at once
succeeds (the batch was dropped with its error), and the context renders afterwards what a context that never saw the deep
scene renders.  No case launches a kernel on the failing path."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api, loader
from tests import util
from tests.lightmap_denoise_ref import plane_records
from tests.test_gpu_ray_query import deep_chain_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT = api.PathtraceType
W = H = 8
PARAMS = dict(max_bounces=2, samples_per_pixel=1)
SENTINEL = 0xA5          # every byte of a caller-supplied output before the observing call
INVALID_ARGUMENT = -1    # LUPIN_ERR_INVALID_ARGUMENT: what the render of the deep scene gives under set_batch_frames(1)


def render_healthy(ctx, scene, cam):
    """8 x 8 of the Cornell box: the f16 texels."""
    res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(**PARAMS))
    target = api.Texture(ctx, W, H)
    api.pathtrace_scene(ctx, res, scene, target, PT.Standard, api.PathtraceDesc(camera_params=cam.params, camera_transform=cam.transform))
    return target.download()


@pytest.fixture(scope="module")
def untouched(built):
    """The healthy render on a context that never saw the deep scene: computed once, shared, left unchanged."""
    ctx = api.Context(0)
    try:
        scene, cams = loader.build_scene_cornell_box(ctx)
        image = render_healthy(ctx, scene, cams[0])
        del scene
    finally:
        ctx.close()
    image.setflags(write=False)
    return image


def record_deep_render(ctx, deep):
    """A render of the deep scene under default batching: recorded, so it returns OK.  The caller keeps what is returned
    alive until the batch has run (destroying the target would run, and drop, the batch)."""
    res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(**PARAMS))
    target = api.Texture(ctx, W, H)
    api.pathtrace_scene(ctx, res, deep, target, PT.Standard, api.PathtraceDesc())
    return res, target


# ---- the observing calls ----------------------------------------------------------------------------------------------------
# Each takes the case's objects (made before the render is recorded) and returns (call, outputs): `call()` makes the observing
# call and raises LupinError as the api does; `outputs` tell, one callable per array the caller supplied, whether the array
# still holds the SENTINEL bytes it was filled with.

def still_sentinel(a):
    return lambda: bool(np.all(a.view(np.uint8) == SENTINEL))


def observe_sync(e):
    return e.ctx.sync, []


def observe_stats(e):
    return e.ctx.stats, []


def observe_download(e):
    # lupin_hip_texture_download_rgba16f as Texture.download calls it, into an array of the test's own
    out = np.full((H, W, 4), SENTINEL * 0x0101, np.uint16)
    return (lambda: _abi.check(_abi.lib().lupin_hip_texture_download_rgba16f(e.target.handle, _abi.ptr(out)))), [still_sentinel(out)]


def observe_upload(e):
    texels = np.full((H, W, 4), 0.25, np.float16)
    return (lambda: e.target.upload(texels)), []


def observe_copy_front_to_back(e):
    return e.dbuf.copy_front_to_back, []


def observe_tonemap(e):
    # lupin_hip_tonemap_and_fit_aspect as api.tonemap_and_fit_aspect calls it with the default descriptor, into a dst of the test's own
    dst = np.full((H, W, 4), SENTINEL, np.uint8)
    d = api.TonemapDesc()
    c = _abi.TonemapDescC(0, 0.0, 0.0, 0.0, 0.0, float(d.exposure), 1 if d.filmic else 0, 1 if d.srgb else 0, 1 if d.clear else 0)
    return (lambda: _abi.check(_abi.lib().lupin_hip_tonemap_and_fit_aspect(e.ctx.handle, e.target.handle, _abi.ptr(dst), W, H, C.byref(c)))), [still_sentinel(dst)]


def observe_falsecolor(e):
    # on the healthy scene: the error can only be the recorded one
    desc = api.PathtraceDesc(camera_params=e.cam.params, camera_transform=e.cam.transform)
    return (lambda: api.pathtrace_scene_falsecolor(e.ctx, e.res, e.healthy, e.other, api.FalsecolorType(0), desc)), []


def observe_camera_probe(e):
    rec = api.camera_records([0, 3, 7], [0, 4, 7], [1, 2, 3])
    return (lambda: api.camera_probe(e.ctx, W, H, e.cam.params, e.cam.transform, rec)), []


def observe_light_probe(e):
    rec = api.light_records(api.LightMode.SAMPLE, [[0.0, 1.0, 0.0], [0.3, 0.5, 0.2]], rng=[7, 8])
    return (lambda: api.light_probe(e.ctx, e.healthy, rec)), []


def observe_adaptive_stats(e):
    return e.adaptive.stats, []


def observe_denoise_lightmap(e):
    rgba = np.full((4, 4, 4), 0.5, np.float32)                # a flat 4 x 4 chart, every texel owned
    records = plane_records(4, 4, du=(0.25, 0.0, 0.0), dv=(0.0, 0.25, 0.0))
    return (lambda: api.denoise_lightmap(e.ctx, rgba, records, passes=1)), []


OBSERVERS = [observe_sync, observe_stats, observe_download, observe_upload, observe_copy_front_to_back, observe_tonemap, observe_falsecolor,
             observe_camera_probe, observe_light_probe, observe_adaptive_stats, observe_denoise_lightmap]


def check_observer(ctx, deep, healthy, cam, untouched, observer, **extra):
    """The three properties of one observing call (the module's docstring)."""
    e = types.SimpleNamespace(ctx=ctx, healthy=healthy, cam=cam, **extra)
    e.res, e.target = record_deep_render(ctx, deep)
    call, outputs = observer(e)
    with pytest.raises(api.LupinError) as err:
        call()
    assert err.value.code == INVALID_ARGUMENT and "too deep" in str(err.value), str(err.value)
    assert all(untouched_output() for untouched_output in outputs), "a refused observing call wrote to its caller's array"
    call()              # the batch was dropped with its error: the same call succeeds
    ctx.sync()
    assert util.f16_words_differ(render_healthy(ctx, healthy, cam), untouched) == 0


@pytest.mark.parametrize("observer", OBSERVERS, ids=lambda f: f.__name__[len("observe_"):])
def test_the_observing_call_reports_the_recorded_error(gpu_ctx, untouched, observer):
    healthy, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    # everything the observers use exists before the render is recorded
    extra = dict(other=api.Texture(gpu_ctx, W, H), dbuf=api.DoubleBufferedTexture(gpu_ctx, W, H), adaptive=api.build_adaptive_resources(gpu_ctx, W, H))
    check_observer(gpu_ctx, deep_chain_scene(gpu_ctx), healthy, cams[0], untouched, observer, **extra)


def test_pack_tiles_into_a_torch_buffer_reports_the_recorded_error(built):
    """The same for pack_tiles into a torch buffer, in a process of its own: torch brings its own HIP runtime, and a process
    with two of them cannot create further contexts."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_recorded_errors_torch_worker.py")], capture_output=True, text=True, timeout=600,
                         cwd=ROOT)
    assert out.returncode == 0 and "RECORDED ERRORS TORCH OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


def test_teardown_drops_a_failing_batch_silently(built):
    """Nothing observes the recorded render: the target, the scene and the context are destroyed, and nobody is told."""
    ctx = api.Context(0)
    deep = deep_chain_scene(ctx)
    res, target = record_deep_render(ctx, deep)
    lib = _abi.lib()
    lib.lupin_hip_texture_destroy(target.handle)
    target.handle = None
    lib.lupin_hip_scene_destroy(deep.handle)
    deep.handle = None
    del res
    ctx.close()
    # the process goes on: another context renders
    ctx = api.Context(0)
    try:
        scene, cams = loader.build_scene_cornell_box(ctx)
        assert render_healthy(ctx, scene, cams[0]).shape == (H, W, 4)
        del scene
    finally:
        ctx.close()
