"""Worker of tests/test_gpu_lightmap_adaptive.py::test_torch_tensors_give_the_same_words: lightmap records as a torch tensor on
the device through api.pathtrace_rays_moments against the numpy path, chunked and not.  torch is imported first, as a torch
host would do it: the process then has one HIP runtime (torch's), and the library runs on it."""
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
    _, plane = api.bake_lightmap(ctx, scene, THREE_CHARTS, 16, 16, samples=1, surface_offset=1e-3, want_records=True)
    rec = np.ascontiguousarray(plane[plane.view(np.uint32)[..., 7] == 1])
    assert len(rec) > 50
    S = 70
    want = api.pathtrace_rays_moments(ctx, scene, rec, api.RayQueryDesc(0, 8, S))
    assert want.shape == (len(rec), 8) and float(want[:, 5].max()) > 0.0
    t = torch.from_numpy(rec).to("cuda:0")
    for max_slots in (0, 3 * S + 1):
        got = api.pathtrace_rays_moments(ctx, scene, t, api.RayQueryDesc(0, 8, S, 0, max_slots))
        assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (len(rec), 8)
        assert np.array_equal(got.cpu().numpy().view(np.uint32), want.view(np.uint32))
    for wrong in (t.double(), t[:, :7], t.cpu(), t.t()):
        try:
            api.pathtrace_rays_moments(ctx, scene, wrong, api.RayQueryDesc(0, 8, S))
        except ValueError:
            pass
        else:
            raise AssertionError("records of the wrong kind were accepted")
    ctx.close()
    print("LIGHTMAP ADAPTIVE TORCH OK")


if __name__ == "__main__":
    main()
