"""Every device allocation has an owner (csrc/lupin_owned.hpp, DESIGN.md "Who owns device memory"): the holders that free,
regrow, swap or outlive something give, bit for bit, what freshly made objects give in the same process.  No test provokes an
allocation failure on the device: tests/test_owned_cpu.py covers those paths on the host."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api, loader
from tests import lbvh_ref, tlas_ref, util
from tests.test_lbvh import random_mesh
from tests.test_sah_device import assert_same_tree

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NOTHING = api.AdaptiveParams(threshold=0.0, min_frames=0)   # no block ever converges: every call renders every pixel

# (width, height, max_bounces).  The first three are the sequence this test was specified with: the counter block grows at the
# second and is kept at the third.  The slot buffers hold whole rounds of 65 536 slots (LP_SHARDS x LP_BLOCK), which those
# sizes never leave even at sixteen frames per wavefront, so 264 x 250 = 66 000 pixels follows to make the nine slot buffers
# themselves be freed and allocated again, and 16 x 16 once more runs in the larger buffers.
PATH_STATE_STEPS = [(16, 16, 2), (48, 32, 5), (16, 16, 2), (264, 250, 2), (16, 16, 2)]


@pytest.mark.parametrize("switch", [{"LUPIN_PATH_RECORDS": "0"}, {"LUPIN_PATH_RECORDS": "1"}, {"LUPIN_BATCH": "1"}],
                         ids=lambda s: ",".join(f"{k[6:]}={v}" for k, v in s.items()))
def test_path_state_regrows_and_shrinks(built, switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LUPIN_") or k in ("LUPIN_HIP_LIB",)}
    env.update(switch)
    p = subprocess.run([sys.executable, os.path.join(HERE, "_owner_worker.py"), json.dumps(PATH_STATE_STEPS)], env=env, capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert res["differing_words"] == [0] * len(PATH_STATE_STEPS)


def _f32_pair(ctx, scene, cam, resize):
    """A double-buffered texture, made at 16 x 16 and resized or made at 24 x 8, after one f32-accumulated frame and two
    copy_front_to_back: (front, back, back after the second copy) as f32 arrays."""
    out = api.DoubleBufferedTexture(ctx, 16, 16) if resize else api.DoubleBufferedTexture(ctx, 24, 8)
    if resize:
        out.resize(24, 8)
    res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(max_bounces=4, samples_per_pixel=2))
    api.pathtrace_scene(ctx, res, scene, out.front(), 0,
                        api.PathtraceDesc(accum_params=api.AccumulationParams(out.back(), 0), camera_params=cam.params, camera_transform=cam.transform))
    out.copy_front_to_back()          # makes the back texture's accumulator
    front, back = out.front().download_f32(), out.back().download_f32()
    out.copy_front_to_back()          # reuses it
    return front, back, out.back().download_f32()


def test_resized_double_buffer_carries_its_f32_accumulator(gpu_ctx):
    scene, cams = util.load_scene("cornellbox_builtin", gpu_ctx)
    gpu_ctx.set_accumulation_mode(1)
    try:
        front, back, again = _f32_pair(gpu_ctx, scene, cams[0], resize=True)
        fresh = _f32_pair(gpu_ctx, scene, cams[0], resize=False)
    finally:
        gpu_ctx.set_accumulation_mode(0)
    assert front.shape == (8, 24, 4) and front[..., :3].any()
    assert np.array_equal(front.view(np.uint32), back.view(np.uint32)) and np.array_equal(back.view(np.uint32), again.view(np.uint32))
    assert np.array_equal(front.view(np.uint32), fresh[0].view(np.uint32)) and np.array_equal(back.view(np.uint32), fresh[1].view(np.uint32))


def _cornell_prefix(ctx, count):
    """The first `count` instances of the Cornell box as a scene of their own."""
    scene_cpu, cams = loader.cornell_box_scene_cpu()
    scene_cpu.instances = scene_cpu.instances[:count].copy()
    api.validate_scene(scene_cpu, 0, 0)
    return api.build_accel_structures_and_upload(ctx, scene_cpu, [], [], True), cams[0]


class _History:
    """One adaptive + reproject resource pair at 16 x 16 and the texture pair their history lives in."""
    W = H = 16

    def __init__(self, ctx):
        self.ctx = ctx
        self.res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(max_bounces=2, samples_per_pixel=1))
        self.out = api.DoubleBufferedTexture(ctx, self.W, self.H)
        self.ares = api.build_adaptive_resources(ctx, self.W, self.H)
        self.rp = api.build_reproject_resources(ctx, self.W, self.H)

    def step(self, scene, cam):
        """reproject into the scene's view, two adaptive frames, reproject again from the same view: the state before and
        after the second call and the hit mask of the view."""
        d = dict(cam.params.__dict__)
        d.update(aspect=1.0, aperture=0.0)
        cp = api.CameraParams(**d)
        for k in range(2):
            if k == 1:
                for _ in range(2):
                    api.pathtrace_scene_adaptive(self.ctx, self.res, scene, self.out.front(), 0,
                                                 api.PathtraceDesc(accum_params=api.AccumulationParams(self.out.back(), 0), camera_params=cp,
                                                                   camera_transform=cam.transform), self.ares, NOTHING)
                    self.out.flip()
                before = self.ares.download()
            api.adaptive_reproject(self.ctx, self.ares, self.rp, scene, api.ReprojectDesc(camera_params=cp, camera_transform=cam.transform),
                                   self.out.back(), self.out.front())
            self.out.flip()
        return before, self.everything()

    def everything(self):
        return list(self.ares.download()) + list(self.rp.download(0)) + list(self.rp.download(1)) + [self.out.back().download()]


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_reproject_rows_regrow_with_the_instance_count(gpu_ctx):
    scenes = {n: _cornell_prefix(gpu_ctx, n) for n in (1, 3)}
    order = [1, 3, 1]                      # the per-instance rows are allocated, grown (freed first), then kept
    kept = _History(gpu_ctx)
    for done in range(1, len(order) + 1):
        before, got = kept.step(*scenes[order[done - 1]])
        # the gathered counts and moments are what the adaptive resources now hold: the unmoved view keeps every hit pixel's two frames
        hit = got[4] != 0xFFFFFFFF
        assert hit.any() and (before[0] >= 2).all()
        assert np.array_equal(got[0][hit], before[0][hit]) and np.array_equal(got[1][hit].view(np.uint32), before[1][hit].view(np.uint32))
        assert (got[0][~hit] == 0).all()
        fresh = _History(gpu_ctx)
        for n in order[:done]:
            _, want = fresh.step(*scenes[n])
        assert _same(got, want), f"step {done}: kept resources differ from fresh ones"


def _destroy(obj, name):
    getattr(_abi.lib(), name)(obj.handle)
    obj.handle = None          # the Python wrapper has nothing left to release


@pytest.mark.parametrize("context_first", [True, False], ids=["context_closed_first", "context_closed_last"])
def test_objects_outlive_their_context(built, context_first):
    """Textures, scenes and resources free their memory whether or not their context still exists; a context made afterwards renders
    the oracle's image."""
    ctx = api.Context(0)
    scene, cams = loader.build_scene_cornell_box(ctx)
    cam = cams[0]
    tex, dbuf = api.Texture(ctx, 16, 16), api.DoubleBufferedTexture(ctx, 16, 16)
    dn, ad, rp = api.build_denoise_resources(ctx, 16, 16), api.build_adaptive_resources(ctx, 16, 16), api.build_reproject_resources(ctx, 16, 16)
    res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(max_bounces=2, samples_per_pixel=1))
    api.pathtrace_scene(ctx, res, scene, dbuf.front(), 0,
                        api.PathtraceDesc(accum_params=api.AccumulationParams(dbuf.back(), 0), camera_params=cam.params, camera_transform=cam.transform))
    api.pathtrace_scene(ctx, res, scene, tex, 0, api.PathtraceDesc(camera_params=cam.params, camera_transform=cam.transform))
    if context_first:
        ctx.close()
    for obj, name in ((tex, "lupin_hip_texture_destroy"), (dbuf, "lupin_hip_dbuf_destroy"), (scene, "lupin_hip_scene_destroy"),
                      (dn, "lupin_hip_destroy_denoise_resources"), (ad, "lupin_hip_destroy_adaptive_resources"),
                      (rp, "lupin_hip_destroy_reproject_resources")):
        _destroy(obj, name)
    if not context_first:
        del res
        ctx.close()
    after = api.Context(0)
    try:
        scene2, cams2 = loader.build_scene_cornell_box(after)
        got = util.gpu_accumulate(after, scene2, cams2[0], 32, 32, frames=2, spp=2, max_bounces=4)
        want = util.oracle_accumulate(scene2, cams2[0], 32, 32, frames=2, spp=2, max_bounces=4)
        assert util.f16_words_differ(got, want) == 0
        del scene2
    finally:
        after.close()


def test_builders_thrice(gpu_ctx):
    """The three device builders free their scratch on return: three builds in a row of the smallest inputs give the same
    nodes every time, and the trees the suite compares them with elsewhere."""
    for n in (1, 2):
        verts, idx = random_mesh(n, 900 + n)
        lbvh = [api.build_bvh_device(gpu_ctx, verts, idx) for _ in range(3)]
        sah = [api.build_bvh_sah_device(gpu_ctx, verts, idx) for _ in range(3)]
        for runs in (lbvh, sah):
            assert all(r[0].tobytes() == runs[0][0].tobytes() and np.array_equal(r[1], runs[0][1]) for r in runs[1:])
        assert_same_tree(api.build_bvh(verts, idx), sah[0], verts)
        want_nodes, want_idx = lbvh_ref.build(verts, idx)
        assert lbvh[0][0].tobytes() == want_nodes.tobytes() and np.array_equal(lbvh[0][1], want_idx)
    inst, aabbs = tlas_ref.random_set(3, 23)
    want = api.build_tlas(inst, aabbs)
    for _ in range(3):
        got = api.build_tlas_device(gpu_ctx, inst, aabbs)
        assert len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in ("left", "right", "instance_idx", "aabb_min", "aabb_max"))
