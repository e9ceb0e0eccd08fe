"""Worker of tests/test_gpu_recorded_errors.py::test_pack_tiles_into_a_torch_buffer_reports_the_recorded_error: the observing
call is pack_tiles into a torch buffer.  torch is imported first, as a torch host would do it: the process then has one HIP
runtime (torch's), and the library runs on it."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lupinpathtracer_amd import api, loader   # noqa: E402
from tests import test_gpu_recorded_errors as T   # noqa: E402
from tests.test_gpu_ray_query import deep_chain_scene   # noqa: E402


def main():
    assert torch.cuda.is_available()
    # the healthy render on a context that never sees the deep scene
    ctx = api.Context(0)
    scene, cams = loader.build_scene_cornell_box(ctx)
    untouched = T.render_healthy(ctx, scene, cams[0])
    del scene
    ctx.close()

    ctx = api.Context(0)
    healthy, cams = loader.build_scene_cornell_box(ctx)
    tile_size, rank, world = 1, 0, 1          # every 4 x 4 tile of the 8 x 8 target: 64 texels of 8 bytes
    buf = torch.full((T.W * T.H * 8,), T.SENTINEL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    def observe_pack_tiles(e):
        return (lambda: api.pack_tiles(e.ctx, e.target, tile_size, rank, world, buf.data_ptr())), [lambda: bool((buf == T.SENTINEL).all())]

    T.check_observer(ctx, deep_chain_scene(ctx), healthy, cams[0], untouched, observe_pack_tiles)
    assert api.packed_tile_pixels(T.W, T.H, tile_size, rank, world) == T.W * T.H
    assert not bool((buf == T.SENTINEL).all())      # the repeated call packed the (cleared) target: zeros
    del healthy
    ctx.close()
    print("RECORDED ERRORS TORCH OK")


if __name__ == "__main__":
    main()
