"""Worker of tests/test_gpu_owners.py: under THIS process's LUPIN_* environment, one context renders a sequence of sizes and
bounce counts that makes its lanes' path state grow, stay and grow again (ensure_path_buffers frees before it allocates);
every image is compared with that of a fresh context.  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lupinpathtracer_amd import api   # noqa: E402
from tests import util   # noqa: E402

FRAMES = 5   # more than the four lanes an LDS-resident scene uses: with LUPIN_BATCH=1 a lane is reused within a step


def render(ctx, w, h, bounces):
    scene, cams = util.load_scene("cornellbox_builtin", ctx)
    return util.gpu_accumulate(ctx, scene, cams[0], w, h, frames=FRAMES, spp=1, max_bounces=bounces)


def main():
    steps = json.loads(sys.argv[1])
    kept = api.Context(0)
    differing = []
    for w, h, bounces in steps:
        got = render(kept, w, h, bounces)
        fresh = api.Context(0)
        want = render(fresh, w, h, bounces)
        for key in [k for k in util._scene_cache if k[1] == id(fresh)]:
            del util._scene_cache[key]   # the scene goes before its context
        fresh.close()
        assert got.any()
        differing.append(util.f16_words_differ(got, want))
    print("RESULT " + json.dumps({"differing_words": differing}))


if __name__ == "__main__":
    main()
