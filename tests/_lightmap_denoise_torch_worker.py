"""Worker of tests/test_gpu_lightmap_denoise.py::test_torch_tensors_give_the_same_words: api.denoise_lightmap over torch
tensors on the device against the numpy path.  torch is imported first, as a torch host would do it: the process then has
one HIP runtime (torch's), and the library runs on it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lupinpathtracer_amd import api   # noqa: E402
from tests import lightmap_denoise_ref as ref   # noqa: E402


def same_words(t, a):
    return np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))


def main():
    assert torch.cuda.is_available()
    ctx = api.Context(0)
    rgba, rec = ref.noisy_atlas(33, 17, seed=9)
    t_rgba, t_rec = torch.from_numpy(rgba).to("cuda:0"), torch.from_numpy(rec).to("cuda:0")
    for dilate in (0, 3):
        want = api.denoise_lightmap(ctx, rgba, rec, dilate=dilate)
        assert np.array_equal(want.view(np.uint32), ref.denoise(rgba, rec, dilate=dilate).view(np.uint32))
        got = api.denoise_lightmap(ctx, t_rgba, t_rec, dilate=dilate)
        assert isinstance(got, torch.Tensor) and got.is_cuda and tuple(got.shape) == (33, 17, 4)
        assert same_words(got, want)
        assert same_words(t_rgba, rgba) and same_words(t_rec, rec)          # the inputs are read only
    for wrong in ((t_rgba.double(), t_rec), (t_rgba[..., :3], t_rec), (t_rgba, t_rec[..., :7]), (t_rgba.cpu(), t_rec), (t_rgba, rec),
                  (t_rgba[:5], t_rec), (t_rgba.reshape(-1, 4), t_rec)):
        try:
            api.denoise_lightmap(ctx, *wrong)
        except ValueError:
            pass
        else:
            raise AssertionError("a tensor of the wrong kind was accepted")
    ctx.close()
    print("LIGHTMAP DENOISE TORCH OK")


if __name__ == "__main__":
    main()
