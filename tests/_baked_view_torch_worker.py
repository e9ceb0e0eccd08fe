"""Worker of tests/test_gpu_baked_view.py::test_torch_tensors_give_the_same_words: api.render_baked over torch tensors on the
device against the numpy path.  torch is imported first, as a torch host would do it: the process then has one HIP runtime
(torch's), and the library runs on it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lupinpathtracer_amd import api, loader   # noqa: E402


def main():
    assert torch.cuda.is_available()
    ctx = api.Context(0)
    scene, cams = loader.build_scene_cornell_box(ctx)
    cam = cams[0]
    rng = np.random.default_rng(13)
    grid = (np.float32([-0.9, 0.1, -0.9]), np.float32([0.6, 0.6, 0.9]), (4, 4, 3))
    sh = rng.normal(size=(48, 9, 4)).astype(np.float32)
    valid = (rng.uniform(size=48) > 0.33).astype(np.uint8)
    pos, maps, maxd = api.bake_probe_grid_depth(ctx, scene, *grid, 8, 2)
    tsh, tmaps = torch.from_numpy(sh).to("cuda:0"), torch.from_numpy(maps).to("cuda:0")
    W, H = 33, 17
    a, b = api.Texture(ctx, W, H), api.Texture(ctx, W, H)
    for v in (None, valid):
        tv = None if v is None else torch.from_numpy(v).to("cuda:0")
        for kw, tkw in ((dict(visibility=True), dict(visibility=True)), (dict(depth=maps, max_distance=maxd), dict(depth=tmaps, max_distance=maxd))):
            for want_g in (True, False):
                want = api.render_baked(ctx, scene, a, cam.params, cam.transform, *grid, sh, valid=v, ambient=(0.1, 0.2, 0.3), want_gbuffer=want_g, **kw)
                got = api.render_baked(ctx, scene, b, cam.params, cam.transform, *grid, tsh, valid=tv, ambient=(0.1, 0.2, 0.3), want_gbuffer=want_g, **tkw)
                assert np.array_equal(a.download().view(np.uint16), b.download().view(np.uint16))
                if want_g:
                    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (H, W, 16)
                    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32)) and float(want[..., 11].max()) > 0.0
                else:
                    assert got is None and want is None
    for s, d in ((tsh, maps), (sh, tmaps), (tsh.double(), tmaps), (tsh, tmaps[:40]), (tsh.cpu(), tmaps)):
        try:
            api.render_baked(ctx, scene, b, cam.params, cam.transform, *grid, s, depth=d, max_distance=maxd)
        except ValueError:
            pass
        else:
            raise AssertionError("a tensor of the wrong kind was accepted")
    ctx.close()
    print("BAKED VIEW TORCH OK")


if __name__ == "__main__":
    main()
