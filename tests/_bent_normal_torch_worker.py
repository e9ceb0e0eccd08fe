"""Worker of tests/test_gpu_bent_normal.py::test_torch_tensors_give_the_same_words: api.bent_normal_rays over a torch tensor
on the device against the numpy path.  torch is imported first, as a torch host would do it: the process then has one HIP
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
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rec = api.occlusion_records(rng.uniform(-0.9, 0.9, (n, 3)) * (1, 0.9, 1) + (0, 1, 0), nrm, rng.uniform(0.2, 2.0, n),
                                api.rng_seed_for(np.arange(n, dtype=np.uint32), 2))
    t = torch.from_numpy(rec).to("cuda:0")
    for S in (1, 65):
        for opacity in (False, True):
            for max_slots in (0, 100 * S + 1):
                want = api.bent_normal_rays(ctx, scene, rec, S, opacity=opacity)
                got = api.bent_normal_rays(ctx, scene, t, S, opacity=opacity, max_slots=max_slots)
                assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (n, 4)
                assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert 0.0 < float(want[:, 3].sum()) < n * 65
    bad = t.clone()
    bad[5, 0] = float("nan")
    try:
        api.bent_normal_rays(ctx, scene, bad, 4)
    except api.LupinError as e:
        assert e.code == -1
    else:
        raise AssertionError("a NaN record was accepted")
    for wrong in (t.double(), t[:, :7], t.cpu(), t.t()):
        try:
            api.bent_normal_rays(ctx, scene, wrong, 4)
        except ValueError:
            pass
        else:
            raise AssertionError("a tensor of the wrong kind was accepted")
    ctx.close()
    print("BENT NORMAL TORCH OK")


if __name__ == "__main__":
    main()
