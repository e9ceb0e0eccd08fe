"""Worker of tests/test_gpu_lightmap_directional.py::test_torch_tensors_give_the_same_words: a directional lightmap baked
through numpy, then api.render_lightmapped(..., directional=...) with the atlas and the planes as torch tensors on the device
against the numpy path.  torch is imported first, as a torch host would do it: the process then has one HIP runtime (torch's),
and the library runs on it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lupinpathtracer_amd import api   # noqa: E402
from tests.test_gpu_lightmap import THREE_CHARTS, three_chart_cpu   # noqa: E402
from tests.test_lightmapped_view_cpu import AMBIENT, CAMERA, FLOOR   # noqa: E402


def main():
    assert torch.cuda.is_available()
    ctx = api.Context(0)
    cpu, envs = three_chart_cpu()
    api.validate_scene(cpu, 0, 0)
    scene = api.build_accel_structures_and_upload(ctx, cpu, [], envs, True)
    charts = THREE_CHARTS + [FLOOR]
    AW, AH, W, H = 33, 17, 40, 24
    atlas = api.bake_lightmap(ctx, scene, charts, AW, AH, samples=8, dilate=2, surface_offset=1e-3)
    planes = api.bake_lightmap_directional(ctx, scene, charts, AW, AH, samples=8, dilate=2, surface_offset=1e-3)
    assert planes.shape == (4, AH, AW, 4) and np.array_equal(planes[0][..., 3], atlas[..., 3])

    def view(lightmap, directional, **kw):
        tex = api.Texture(ctx, W, H)
        tex.upload(np.full((H, W, 4), -7.0, np.float16))
        g = api.render_lightmapped(ctx, scene, tex, CAMERA[0], CAMERA[1], charts, lightmap, ambient=AMBIENT, want_gbuffer=True, directional=directional, **kw)
        return tex.download().view(np.uint16), g

    want_tex, want_g = view(atlas, planes)
    assert want_g.shape == (H, W, 24) and int((want_g.view(np.uint32)[..., 23] & 1).sum()) > 50
    t_atlas, t_planes = torch.from_numpy(atlas).to("cuda:0"), torch.from_numpy(planes).to("cuda:0")
    for max_slots in (0, 64):
        got_tex, got_g = view(t_atlas, t_planes, max_slots=max_slots)
        assert isinstance(got_g, torch.Tensor) and got_g.is_cuda and tuple(got_g.shape) == (H, W, 24)
        assert np.array_equal(got_g.cpu().numpy().view(np.uint32), want_g.view(np.uint32)) and np.array_equal(got_tex, want_tex)
    for wrong in (planes, t_planes.double(), t_planes[:3], t_planes.cpu(), t_planes.permute(0, 2, 1, 3)):
        try:
            view(t_atlas, wrong)
        except ValueError:
            pass
        else:
            raise AssertionError("planes of the wrong kind were accepted beside a tensor atlas")
    ctx.close()
    print("LIGHTMAP DIRECTIONAL TORCH OK")


if __name__ == "__main__":
    main()
