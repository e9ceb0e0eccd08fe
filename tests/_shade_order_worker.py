"""Worker of tests/test_gpu_shade_order.py: renders the cases given as JSON under THIS process's LUPIN_* environment and saves
every image (f16, as Texture.download returns it) with the run's statistics to an .npz.  Prints one line, "OK <path>"."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lupinpathtracer_amd import api   # noqa: E402
from tests import util   # noqa: E402


def main():
    out_path, cases = sys.argv[1], json.loads(sys.argv[2])
    ctx = api.Context(0)
    arrays = {}
    for c in cases:
        scene, cams = util.load_scene(c["scene"], ctx)
        ctx.stats_reset(0)
        img = util.gpu_accumulate(ctx, scene, cams[c.get("cam", 0)], c["w"], c["h"], c["frames"], c["spp"], max_bounces=c["bounces"], ptype=c["type"])
        st = ctx.stats()
        arrays[c["key"]] = img
        arrays[c["key"] + ":frames_per_wavefront"] = np.array(st["frames_per_wavefront"])
    np.savez(out_path, **arrays)
    print("OK " + out_path)


if __name__ == "__main__":
    main()
