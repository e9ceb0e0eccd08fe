"""Worker of tests/test_gpu_path.py's switch legs: runs one-sample radiance queries on the records of tests/path_ref.py under
THIS process's LUPIN_* environment and writes what the device returned; the parent judges it against the float64 paths."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lupinpathtracer_amd import api   # noqa: E402
from tests import path_ref as R   # noqa: E402


def main():
    job = np.load(sys.argv[1])
    queries = json.loads(str(job["queries"]))
    ctx = api.Context(0)
    scenes, out = {}, {}
    for variant, integ, rung, max_radiance in queries:
        if variant not in scenes:
            cpu, textures, infos = R.scene_cpu(variant)
            scenes[variant] = api.build_accel_structures_and_upload(ctx, cpu, textures, infos, True)
        adv = api.AdvancedParams(max_radiance=max_radiance, ray_epsilon=R.EPS)
        got = api.pathtrace_rays(ctx, scenes[variant], job[f"records:{variant}"], api.RayQueryDesc(integ, rung, 1, 0, 0, adv))
        out[f"{variant}:{integ}:{rung}:{max_radiance}"] = got
    np.savez(sys.argv[2], **out)
    print("RESULT " + json.dumps({"queries": len(queries)}))


if __name__ == "__main__":
    main()
