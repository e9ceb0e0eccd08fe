"""The device's path loop against the float64 path tracer of tests/path_ref.py: lupin_hip_pathtrace_rays with one
sample runs one production path per record; path_ref.failures judges it inside the bounds measured on the CPU.  The float64
answers are computed once per scene and integrator and shared (path_ref.cached_trace)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from lupinpathtracer_amd import api
from tests import path_ref as R

PT = api.PathtraceType
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def global_ctx(built):
    """A context whose kernels read every scene from global memory (as tests/test_gpu_ray_query.py makes one)."""
    old = os.environ.get("LUPIN_LDS_GEOMETRY")
    os.environ["LUPIN_LDS_GEOMETRY"] = "0"     # read at context creation
    try:
        ctx = api.Context(0)
    finally:
        if old is None:
            os.environ.pop("LUPIN_LDS_GEOMETRY", None)
        else:
            os.environ["LUPIN_LDS_GEOMETRY"] = old
    yield ctx
    _scenes.clear()
    ctx.close()


_scenes = {}


def device_scene(ctx, variant):
    key = (id(ctx), variant)
    if key not in _scenes:
        c = R.case(variant)
        _scenes[key] = api.build_accel_structures_and_upload(ctx, c.cpu, c.textures, c.infos, True)
    return _scenes[key]


def query(ctx, scene, rec, integ, rung, max_radiance=R.NO_CLAMP, samples=1, max_slots=0):
    adv = api.AdvancedParams(max_radiance=max_radiance, ray_epsilon=R.EPS)
    got = api.pathtrace_rays(ctx, scene, rec, api.RayQueryDesc(integ, rung, samples, 0, max_slots, adv))
    assert got.shape == (len(rec), 4) and np.all(got[:, 3] == 1.0)
    return got


def judge(tr, got_by_rung, max_radiance=R.NO_CLAMP):
    for rung in got_by_rung:                                   # the conditions, again: on the cells this test compares
        assert 1.0 - tr.vertex(rung)["decisive"].mean() <= R.MAX_EXCLUDED
    found = R.first_failing_rung(tr, got_by_rung, max_radiance)
    assert found is None, f"first failing rung {found[0]}:\n" + "\n".join(found[1])


@pytest.mark.gpu
@pytest.mark.parametrize("integ", R.INTEGRATORS, ids=lambda t: t.name)
@pytest.mark.parametrize("variant", ("const", "textured"))
@pytest.mark.parametrize("leg", ("default", "global"))
def test_device_paths_agree_with_the_float64_paths(gpu_ctx, global_ctx, leg, variant, integ):
    ctx = gpu_ctx if leg == "default" else global_ctx
    c = R.case(variant)
    scene, rec = device_scene(ctx, variant), R.records(c)
    tr = R.cached_trace(c, integ)
    judge(tr, {rung: query(ctx, scene, rec, integ, rung) for rung in R.LADDER})
    judge(tr, {rung: query(ctx, scene, rec, integ, rung, R.CLAMP) for rung in (2, 8)}, R.CLAMP)
    cond = R.conditions(tr)
    assert cond["roulette survived"] >= 100 and cond["clamp scaled"] >= 100 and cond["clamp non-finite"] >= 100


@pytest.mark.gpu
@pytest.mark.parametrize("integ", R.INTEGRATORS, ids=lambda t: t.name)
def test_matte_only_scene(gpu_ctx, integ):
    """Every body matte: the SIMPLE instantiation of the shade kernel."""
    c = R.case("matte")
    scene = device_scene(gpu_ctx, "matte")
    judge(R.cached_trace(c, integ), {rung: query(gpu_ctx, scene, R.records(c), integ, rung) for rung in (1, 8)})


class _Sub:
    """A Trace restricted to some records."""

    def __init__(self, tr, sel):
        self.tr, self.sel, self.integ, self.log = tr, sel, tr.integ, tr.log

    def vertex(self, rung):
        return {k: v[self.sel] for k, v in self.tr.vertex(rung).items()}

    def at(self, rung, max_radiance=R.NO_CLAMP):
        return tuple(x[self.sel] for x in self.tr.at(rung, max_radiance))


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 63, 65))
def test_tails(gpu_ctx, n):
    c = R.case("const")
    scene = device_scene(gpu_ctx, "const")
    sel = np.random.default_rng(n).permutation(4096)[:n]
    for integ in (PT.Standard, PT.MIS):
        tr = _Sub(R.cached_trace(c, integ), sel)
        got = query(gpu_ctx, scene, R.records(c, sel), integ, 8)
        f = R.failures(tr, got, 8, names=sel)
        assert not f, "\n".join(f)


@pytest.mark.gpu
def test_three_wavefronts(gpu_ctx):
    """max_slots small enough that the 4096 records take three wavefronts."""
    c = R.case("const")
    scene = device_scene(gpu_ctx, "const")
    for integ in (PT.MIS, PT.Direct):
        judge(R.cached_trace(c, integ), {8: query(gpu_ctx, scene, R.records(c), integ, 8, max_slots=1400)})


@pytest.mark.gpu
def test_four_samples_are_the_ordered_mean_of_four_reference_paths(gpu_ctx):
    c = R.case("const")
    scene = device_scene(gpu_ctx, "const")
    sel = slice(0, 4096, 8)
    rung, integ = 4, PT.Standard
    total = np.zeros((512, 3), np.float32)
    dec = np.ones(512, bool)
    for s in range(4):
        tr = R.trace(c, integ, rung, sel=sel, word=api.ray_sample_seed(c.word[sel], s))
        clamped, _, d = tr.at(rung, R.NO_CLAMP)
        total = total + clamped.astype(np.float32)
        dec &= d
    want = total / np.float32(4)
    got = query(gpu_ctx, scene, R.records(c, sel), integ, rung, samples=4)
    dev = R.deviation(got[:, :3], want)
    assert dec.mean() >= 0.5
    bad = np.nonzero(dec & ~(dev <= R.bound(integ, rung)))[0]
    assert len(bad) == 0, [(int(r), got[r, :3], want[r], float(dev[r])) for r in bad[:5]]


@pytest.mark.gpu
def test_after_update_instances(gpu_ctx):
    """The bodies moved in place; the reference rebuilt on the new transforms."""
    c0 = R.case("const")
    scene = api.build_accel_structures_and_upload(gpu_ctx, c0.cpu, c0.textures, c0.infos, True)
    scene.update_instances(R.instance_records(True))
    c = R.make_case("const", scene=scene, moved=True)
    sel = slice(0, 4096, 4)
    for integ in (PT.Standard, PT.MIS):
        tr = R.trace(c, integ, 8, sel=sel)
        assert 1.0 - tr.vertex(8)["decisive"].mean() <= R.MAX_EXCLUDED
        got = query(gpu_ctx, scene, R.records(c, sel), integ, 8)
        f = R.failures(tr, got, 8)
        assert not f, "\n".join(f)


# The switches that select other instantiations of the loop (the list and the way to set them: tests/test_gpu_switches.py and
# tests/test_gpu_launch_dispatch.py; read at context creation, so each value runs in a fresh process): the light-pdf stage on
# and off (k_light_pdf / k_light_pdf_mis with its power-heuristic weights against the fused march), the shade-order sort and
# the path state kept as records, the simple tracer and shadow kernels against the persistent tracer with its pretraced shadow
# rays, both with the geometry in global memory, where the persistent tracer runs.
SWITCHES = [{"LUPIN_LIGHT_STAGE": "0"}, {"LUPIN_LIGHT_STAGE": "1"}, {"LUPIN_SORT_SHADE": "0"}, {"LUPIN_SORT_SHADE": "1"},
            {"LUPIN_PATH_RECORDS": "0"}, {"LUPIN_PATH_RECORDS": "1"}, {"LUPIN_SIMPLE_SHADE": "0"},
            {"LUPIN_LDS_GEOMETRY": "0", "LUPIN_SHADOW": "simple"}, {"LUPIN_LDS_GEOMETRY": "0", "LUPIN_EXTEND": "simple"},
            {"LUPIN_LDS_GEOMETRY": "0", "LUPIN_LIGHT_STAGE": "1", "LUPIN_SORT_SHADE": "1"},
            {"LUPIN_LDS_GEOMETRY": "0", "LUPIN_LIGHT_STAGE": "0", "LUPIN_SORT_SHADE": "0"}]
SWITCH_QUERIES = [("const", int(t), rung, mr) for t in R.INTEGRATORS for rung, mr in ((2, R.NO_CLAMP), (8, R.NO_CLAMP), (8, R.CLAMP))]


@pytest.fixture(scope="module")
def switch_job(tmp_path_factory, built):
    path = str(tmp_path_factory.mktemp("path_switches") / "job.npz")
    np.savez(path, queries=json.dumps(SWITCH_QUERIES), **{"records:const": R.records(R.case("const"))})
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: ",".join(f"{k[6:]}={v}" for k, v in s.items()))
def test_switch_value_follows_the_float64_paths(switch_job, tmp_path, switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith("LUPIN_") or k in ("LUPIN_HIP_LIB",)}
    env.update(switch)
    out = str(tmp_path / "got.npz")
    p = subprocess.run([sys.executable, os.path.join(HERE, "_path_switch_worker.py"), switch_job, out], env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    got = np.load(out)
    c = R.case("const")
    for integ in R.INTEGRATORS:
        tr = R.cached_trace(c, integ)
        judge(tr, {rung: got[f"const:{int(integ)}:{rung}:{R.NO_CLAMP}"] for rung in (2, 8)})
        judge(tr, {8: got[f"const:{int(integ)}:8:{R.CLAMP}"]}, R.CLAMP)
