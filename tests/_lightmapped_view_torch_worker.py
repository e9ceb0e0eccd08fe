"""Worker of tests/test_gpu_lightmapped_view.py::test_torch_tensors_give_the_same_words: api.render_lightmapped over torch
tensors on the device against the numpy path.  torch is imported first, as a torch host would do it: the process then has
one HIP runtime (torch's), and the library runs on it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lupinpathtracer_amd import api   # noqa: E402
from tests.test_gpu_lightmap import THREE_CHARTS, three_chart_cpu   # noqa: E402


def main():
    assert torch.cuda.is_available()
    ctx = api.Context(0)
    cpu, envs = three_chart_cpu()
    api.validate_scene(cpu, 0, 0)
    scene = api.build_accel_structures_and_upload(ctx, cpu, [], envs, True)
    cam = (api.CameraParams(is_orthographic=False, lens=0.035, film=0.036, aspect=1.5, focus=6.5, aperture=0.0),
           np.float32([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.0, 0.3, -6.5]]))
    rng = np.random.default_rng(13)
    grid = (np.float32([-4.0, -1.4, -1.5]), np.float32([2.0, 1.0, 1.5]), (5, 4, 4))
    sh = rng.normal(size=(80, 9, 4)).astype(np.float32)
    atlas = rng.uniform(0.1, 2.0, (33, 17, 4)).astype(np.float32)
    atlas[..., 3] = rng.uniform(size=(33, 17)) > 0.3
    _, maps, maxd = api.bake_probe_grid_depth(ctx, scene, *grid, 8, 2)
    tsh, tmaps, tatlas = (torch.from_numpy(x).to("cuda:0") for x in (sh, maps, atlas))
    W, H = 33, 17
    a, b = api.Texture(ctx, W, H), api.Texture(ctx, W, H)
    for kw, tkw in ((dict(), dict()), (dict(sh=sh, visibility=True), dict(sh=tsh, visibility=True)),
                    (dict(sh=sh, depth=maps, max_distance=maxd), dict(sh=tsh, depth=tmaps, max_distance=maxd))):
        vol = dict(origin=grid[0], spacing=grid[1], dims=grid[2]) if kw else {}
        for want_g in (True, False):
            want = api.render_lightmapped(ctx, scene, a, cam[0], cam[1], THREE_CHARTS, atlas, ambient=(0.1, 0.2, 0.3), want_gbuffer=want_g, **vol, **kw)
            got = api.render_lightmapped(ctx, scene, b, cam[0], cam[1], THREE_CHARTS, tatlas, ambient=(0.1, 0.2, 0.3), want_gbuffer=want_g, **vol, **tkw)
            assert np.array_equal(a.download().view(np.uint16), b.download().view(np.uint16))
            if want_g:
                assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (H, W, 20)
                assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
                seen = set(np.unique(want.view(np.uint32)[..., 19]).tolist())          # a miss, a lightmapped hit, and the uncharted boxes
                assert seen >= ({0, 1, 2} if kw else {0, 1, 3}), seen
            else:
                assert got is None and want is None
    vol = dict(origin=grid[0], spacing=grid[1], dims=grid[2])
    for lm, s in ((tatlas, sh), (atlas, tsh), (tatlas.double(), None), (tatlas[..., :3], None), (tatlas.cpu(), None)):
        try:
            api.render_lightmapped(ctx, scene, b, cam[0], cam[1], THREE_CHARTS, lm, sh=s, **(vol if s is not None else {}))
        except ValueError:
            pass
        else:
            raise AssertionError("a tensor of the wrong kind was accepted")
    ctx.close()
    print("LIGHTMAPPED VIEW TORCH OK")


if __name__ == "__main__":
    main()
