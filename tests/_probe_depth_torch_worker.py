"""Worker of tests/test_gpu_probe_depth.py::test_torch_tensors_give_the_same_words: api.sample_probe_grid_depth over torch
tensors on the device against the numpy path.  torch is imported first, as a torch host would do it: the process then has
one HIP runtime (torch's), and the library runs on it."""
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
    rng = np.random.default_rng(13)
    n = 777
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rec = api.probe_grid_records(rng.uniform(-0.9, 0.9, (n, 3)) * (1, 0.9, 1) + (0, 1, 0), d)
    grid = (np.float32([-0.9, 0.1, -0.9]), np.float32([0.6, 0.6, 0.9]), (4, 4, 3))
    sh = rng.normal(size=(48, 9, 4)).astype(np.float32)
    valid = (rng.uniform(size=48) > 0.33).astype(np.uint8)
    pos, maps, maxd = api.bake_probe_grid_depth(ctx, scene, *grid, 8, 2)
    t, tsh, tmaps = torch.from_numpy(rec).to("cuda:0"), torch.from_numpy(sh).to("cuda:0"), torch.from_numpy(maps).to("cuda:0")
    for v in (None, valid):
        for back in (True, False):
            want = api.sample_probe_grid_depth(ctx, scene, *grid, sh, maps, rec, max_distance=maxd, valid=v, backface=back, normal_bias=0.0)
            tv = None if v is None else torch.from_numpy(v).to("cuda:0")
            got = api.sample_probe_grid_depth(ctx, scene, *grid, tsh, tmaps, t, max_distance=maxd, valid=tv, backface=back, normal_bias=0.0)
            assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (n, 4)
            assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert float(want[:, 3].max()) > 0.0
    plain = api.sample_probe_grid(ctx, scene, *grid, sh, rec, valid=valid, visibility=False, backface=False, normal_bias=0.0)
    assert (plain.view(np.uint32) != want.view(np.uint32)).any()            # the maps matter
    bad = t.clone()
    bad[5, 0] = float("nan")
    try:
        api.sample_probe_grid_depth(ctx, scene, *grid, tsh, tmaps, bad, max_distance=maxd)
    except api.LupinError as e:
        assert e.code == -1
    else:
        raise AssertionError("a NaN record was accepted")
    for a, b, c in ((tsh, tmaps, t.double()), (tsh, tmaps.double(), t), (tsh, tmaps[:40], t), (tsh, maps, t), (sh, tmaps, t), (tsh, tmaps, rec), (tsh, tmaps.cpu(), t)):
        try:
            api.sample_probe_grid_depth(ctx, scene, *grid, a, b, c, max_distance=maxd)
        except ValueError:
            pass
        else:
            raise AssertionError("a tensor of the wrong kind was accepted")
    ctx.close()
    print("PROBE DEPTH TORCH OK")


if __name__ == "__main__":
    main()
