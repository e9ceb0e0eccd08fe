"""The host's dispatch from run-time choices to kernel variants (DESIGN.md 5 "Where a launch is planned"), where the switch matrix
of test_gpu_switches.py does not reach: the Naive integrator through the tracer's variants, and the work-counting
instantiations of all four integrators under the binary and the four-wide traversal.  Always against the oracle, word for word."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from lupinpathtracer_amd import api
from tests import util

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

NAIVE = 2
# the first scene is traversed from global memory and has a four-wide hierarchy, the second is staged in LDS
NAIVE_CASES = [dict(scene="bistro_class_small", type=NAIVE, w=48, h=32, frames=2, spp=1, bounces=4),
               dict(scene="cornellbox_builtin", type=NAIVE, w=32, h=32, frames=2, spp=1, bounces=4)]
NAIVE_SWITCHES = [{}, {"LUPIN_EXTEND": "simple"}, {"LUPIN_TRAVERSAL": "wide"}, {"LUPIN_SHORT_STACK": "5"}, {"LUPIN_LDS_GEOMETRY": "0"}]

COUNT_CASE = dict(scene="bistro_class_small", w=48, h=32, spp=1, bounces=4)


@pytest.fixture(scope="module")
def naive_reference(tmp_path_factory, built):
    """The oracle's image of every Naive case, once per session, in the file format of tests/_switch_worker.py."""
    path = str(tmp_path_factory.mktemp("launch_dispatch") / "reference.npz")
    arrays = {"cases": json.dumps(NAIVE_CASES)}
    for c in NAIVE_CASES:
        scene, cams = util.load_scene(c["scene"], None)
        arrays[f"{c['scene']}:{c['type']}"] = util.oracle_accumulate(scene, cams[0], c["w"], c["h"], c["frames"], c["spp"], max_bounces=c["bounces"], ptype=c["type"])
    np.savez(path, **arrays)
    return path


@pytest.fixture(scope="module")
def count_reference(built):
    """The oracle's one-frame image of the counting case under each of the four integrators."""
    c = COUNT_CASE
    scene, cams = util.load_scene(c["scene"], None)
    return [util.oracle_accumulate(scene, cams[0], c["w"], c["h"], 1, c["spp"], max_bounces=c["bounces"], ptype=t) for t in range(4)]


@pytest.mark.gpu
@pytest.mark.parametrize("switch", NAIVE_SWITCHES, ids=lambda s: ",".join(f"{k[6:]}={v}" for k, v in s.items()) or "default")
def test_naive_integrator_through_the_tracers_variants(naive_reference, switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LUPIN_") or k in ("LUPIN_HIP_LIB",)}
    env.update(switch)
    p = subprocess.run([sys.executable, os.path.join(HERE, "_switch_worker.py"), naive_reference], env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    print(switch, res)
    assert all(v == 0 for v in res["differing_words"].values()), res["differing_words"]
    big = res["stats"][f"bistro_class_small:{NAIVE}"]
    if switch.get("LUPIN_TRAVERSAL") == "wide":
        assert big["wide_traversal"] == 1, big
    if "LUPIN_SHORT_STACK" in switch:
        assert big["short_stack_entries"] == 5, big


@pytest.mark.gpu
@pytest.mark.parametrize("ptype", range(4), ids=["standard", "mis", "naive", "direct"])
def test_work_counting_of_every_integrator_binary_and_wide(gpu_ctx, count_reference, ptype):
    c = COUNT_CASE
    scene, cams = util.load_scene(c["scene"], gpu_ctx)
    res = api.build_pathtrace_resources(gpu_ctx, api.BakedPathtraceParams(max_bounces=c["bounces"], samples_per_pixel=c["spp"]))
    desc = api.PathtraceDesc(camera_params=cams[0].params, camera_transform=cams[0].transform)
    a, b = api.Texture(gpu_ctx, c["w"], c["h"]), api.Texture(gpu_ctx, c["w"], c["h"])
    try:
        for traversal, counter in (("binary", "node_visits"), ("wide", "wide_node_visits")):
            gpu_ctx.set_traversal(traversal)
            gpu_ctx.stats_reset(0)
            api.pathtrace_scene(gpu_ctx, res, scene, a, ptype, desc)
            plain = gpu_ctx.stats()
            gpu_ctx.stats_reset(2)
            api.pathtrace_scene(gpu_ctx, res, scene, b, ptype, desc)
            counted = gpu_ctx.stats()
            print(ptype, traversal, "counted", counted["node_visits"], counted["wide_node_visits"], "plain", plain["node_visits"], plain["wide_node_visits"])
            assert plain["wide_traversal"] == counted["wide_traversal"] == (1 if traversal == "wide" else 0)
            assert util.f16_words_differ(a.download(), b.download()) == 0
            assert util.f16_words_differ(a.download(), count_reference[ptype]) == 0
            assert counted[counter][0] > 0, counted
            assert plain["node_visits"] == [0, 0, 0] and plain["wide_node_visits"] == [0, 0, 0], plain
    finally:
        gpu_ctx.set_traversal("binary")
        gpu_ctx.stats_reset(0)
