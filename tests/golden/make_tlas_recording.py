"""Records lupin_build_tlas' output for the instance sets of tests/tlas_ref.py:recorded_sets into tlas_parent_recording.npz.
Made once with the build that preceded the leaf-loop refactor; tests/test_tlas_device_cpu.py compares every
later build with it byte for byte.  Run from the repository root: python tests/golden/make_tlas_recording.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from lupinpathtracer_amd import api   # noqa: E402
from tests import tlas_ref            # noqa: E402

out = {}
for name, (inst, aabbs) in tlas_ref.recorded_sets().items():
    out[name] = api.build_tlas(inst, aabbs).view(np.uint8)
    print(name, len(inst), "instances,", out[name].nbytes, "bytes")
np.savez_compressed(tlas_ref.RECORDING, **out)
