"""Worker of tests/test_gpu_ray_query.py::test_torch_tensors_give_the_same_words: api.pathtrace_rays over torch tensors on
the device against the numpy path.  torch is imported first, as a torch host would do it: the process then has one HIP
runtime (torch's), and the library runs on it."""
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
    rng = np.random.default_rng(12)
    n = 777
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rec = api.ray_records(rng.uniform(-0.9, 0.9, (n, 3)) * (1, 0.9, 1) + (0, 1, 0), d, rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32),
                          (np.arange(n) % 2).astype(np.uint32))
    desc = api.RayQueryDesc(api.PathtraceType.MIS, 8, 3, 0, 1000)
    want, want_rays = api.pathtrace_rays(ctx, scene, rec, desc, want_rays=True)
    t = torch.from_numpy(rec).to("cuda:0")
    got, rays = api.pathtrace_rays(ctx, scene, t, desc, want_rays=True)
    assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (n, 4)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(rays.cpu().numpy().view(np.uint32), want_rays.view(np.uint32))
    got = api.pathtrace_rays(ctx, scene, t, desc)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    bad = t.clone()
    bad[5, 0] = float("nan")
    try:
        api.pathtrace_rays(ctx, scene, bad, desc)
    except api.LupinError as e:
        assert e.code == -1
    else:
        raise AssertionError("a NaN record was accepted")
    for wrong in (t.double(), t[:, :7], t.cpu()):
        try:
            api.pathtrace_rays(ctx, scene, wrong, desc)
        except ValueError:
            pass
        else:
            raise AssertionError("a tensor of the wrong kind was accepted")
    assert float(want[:, :3].max()) > 0.0
    ctx.close()
    print("RAY QUERY TORCH OK")


if __name__ == "__main__":
    main()
