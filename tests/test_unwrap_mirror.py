"""The C++ host mirror of the lightmap UV sets (include/lupin_unwrap.hpp, lp::Scene::set_lightmap_uvs), run by
tests/unwrap_mirror_probe.cpp and compared with the Python host on the same inputs through the same library: the words are
equal.  In the manner of tests/test_cpp_mirror.py, whose blob format and input rule these reuse.  Without a device: the
program compiles under -Wall -Wextra -Werror -ffp-contract=off, the packer's section, and a guard that every wrapper of the
header has a section."""
import os
import re
import subprocess

import numpy as np
import pytest

from lupinpathtracer_amd import api, loader
from tests import cpp_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lupin_unwrap.hpp")
SOURCE = os.path.join(ROOT, "tests", "unwrap_mirror_probe.cpp")
EXE = os.path.join(ROOT, "tests", "unwrap_mirror_probe")
FLAGS = ["-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
F = np.float32

# no multiplier is a power of two: m / W and (x + gutter) / W round
PACK = dict(sizes=np.array([[30, 36], [18, 22], [18, 22], [7, 50], [30, 36]], np.uint32), multipliers=np.array([1.0, 2.3, 0.7, 1.1, 1.0], F), gutter=3)
UNWRAP = M.distinct("unwrap_lightmap_uvs", mesh_idx=5, num_tris=12, padding=2, instance_idx=5, gutter=1, samples=4, max_bounces=3, counter=7,
                    same=("instance_idx",), texel_size=0.031, multiplier=1.7, surface_offset=0.003)


def inputs():
    return dict(M.flat("pack_lightmap_instances", PACK), **M.flat("unwrap_lightmap_uvs", UNWRAP))


@pytest.fixture(scope="module")
def probe(built):
    lib_dir = os.path.join(ROOT, "lupinpathtracer_amd")
    subprocess.check_call(["g++", *FLAGS, "-I" + os.path.join(ROOT, "include"), SOURCE, "-L" + lib_dir, "-llupin_hip", "-L/opt/rocm/lib", "-lz",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", EXE])
    return EXE


def run_probe(exe, tmp, sections=()):
    src, dst = os.path.join(tmp, "inputs.bin"), os.path.join(tmp, "outputs.bin")
    M.write_blob(src, inputs())
    p = subprocess.run([exe, src, dst, *sections], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    return M.read_blob(dst)


def words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_same_words(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = int((words(got) != words(want)).sum())
    assert bad == 0, f"{what}: {bad} of {want.size} words differ between the C++ host and the Python host"


def charts_arrays(charts):
    return (np.array([c.instance_idx for c in charts], np.uint32),
            np.array([[c.scale_u, c.scale_v, c.offset_u, c.offset_v] for c in charts], F))


def test_pack_lightmap_instances_equals_the_python_hosts(probe, tmp_path):
    got = run_probe(probe, str(tmp_path), ["pack_lightmap_instances"])
    assert got["done.pack_lightmap_instances"] == 1
    width, height, charts = api.pack_lightmap_instances([tuple(s) for s in PACK["sizes"].tolist()], PACK["multipliers"], PACK["gutter"])
    assert (int(got["pack_lightmap_instances.width"][0]), int(got["pack_lightmap_instances.height"][0])) == (width, height)
    inst, so = charts_arrays(charts)
    assert_same_words(got["pack_lightmap_instances.charts.instance_idx"], inst, "instance_idx")
    assert_same_words(got["pack_lightmap_instances.charts.scale_offset"], so, "scale and offset")
    assert len(np.unique(so.view(np.uint32))) > 12          # the divisions round: a host that divides otherwise shows
    assert got["pack_lightmap_instances.refused"].tolist() == [1, 1, 1]


def test_every_wrapper_of_the_header_has_a_section(probe):
    text = open(HEADER).read()
    names = set(re.findall(r"^inline [^\n(]*?(\w+)\(", text, re.M))
    assert names == {"unwrap_lightmap_uvs", "pack_lightmap_instances"}
    lines = subprocess.run([probe, "--list"], capture_output=True, text=True, check=True).stdout.splitlines()
    covered = set().union(*[set(line.split(":")[1].split()) for line in lines])
    assert names <= covered and "set_lightmap_uvs" in covered
    source = open(SOURCE).read()
    for name in covered:
        assert re.search(r"\.set_lightmap_uvs\(" if name == "set_lightmap_uvs" else r"\blp::" + name + r"\(", source), name
    assert '#include "lupin.hpp"' in text


@pytest.mark.gpu
def test_the_device_section_equals_the_python_host_word_for_word(gpu_ctx, probe, tmp_path):
    got = run_probe(probe, str(tmp_path), ["unwrap_lightmap_uvs"])
    assert got["done.unwrap_lightmap_uvs"] == 1
    p = UNWRAP
    scene = loader.build_scene_cornell_box(gpu_ctx)[0]
    uvs, chart, info = scene.unwrap_lightmap_uvs(p["mesh_idx"], p["texel_size"], p["padding"], want_charts=True)      # attached
    assert_same_words(got["unwrap_lightmap_uvs.uvs"], uvs, "uvs")
    assert_same_words(got["unwrap_lightmap_uvs.chart_of_tri"], chart, "chart_of_tri")
    assert got["unwrap_lightmap_uvs.info"].tolist() == [info["num_charts"], info["width"], info["height"], info["degenerate_tris"]]
    assert info["num_charts"] == 6          # the short box has its own vertices per face
    width, height, charts = api.pack_lightmap_instances([(info["width"], info["height"])], [p["multiplier"]], p["gutter"])
    charts[0].instance_idx = p["instance_idx"]
    rgba, records = api.bake_lightmap(gpu_ctx, scene, charts, width, height, samples=p["samples"], max_bounces=p["max_bounces"], counter=p["counter"],
                                      surface_offset=p["surface_offset"], want_records=True)
    assert_same_words(got["unwrap_lightmap_uvs.rgba"], rgba, "rgba")
    assert_same_words(got["unwrap_lightmap_uvs.records"], records, "records")
    covered = int((rgba[..., 3] == 1.0).sum())
    assert int(got["unwrap_lightmap_uvs.covered"][0]) == covered and covered > 100
    assert int(got["unwrap_lightmap_uvs.refused_without_a_set"][0]) == 1
