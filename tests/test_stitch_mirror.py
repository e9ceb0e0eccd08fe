"""The C++ host mirror of lightmap seam stitching (include/lupin_stitch.hpp), run by tests/stitch_mirror_probe.cpp and compared
with the Python host on the same inputs through the same library: the words are equal.  In the manner of
tests/test_cpp_mirror.py, whose blob format and input rule these reuse.  Without a device: the program compiles under
-Wall -Wextra -Werror -ffp-contract=off, and a guard that every wrapper of the header has a section."""
import os
import re
import subprocess

import numpy as np
import pytest

from lupinpathtracer_amd import api, loader
from tests import cpp_mirror as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lupin_stitch.hpp")
SOURCE = os.path.join(ROOT, "tests", "stitch_mirror_probe.cpp")
EXE = os.path.join(ROOT, "tests", "stitch_mirror_probe")
FLAGS = ["-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
F = np.float32

# Mesh 0 of the Cornell box is two triangles that share one edge by index; the set places them apart, so that edge is a seam,
# 12 or 12 * sqrt(2) texels long by whichever corners the scene's indices share.  No two fields carry the same value.
STITCH = M.distinct("stitch_lightmap", mesh_idx=0, instance_idx=0, width=32, height=16, iterations=5, same=("mesh_idx", "instance_idx"),
                    samples_per_texel=1.7, lam=0.23, scale_u=1.0 / 32, scale_v=1.0 / 16, offset_u=1.0 / 64, offset_v=1.0 / 128)
UVS = F([[(1, 1), (13, 1), (1, 13)], [(16, 2), (28, 2), (16, 14)]])


def atlas():
    rgba = np.random.default_rng(17).random((STITCH["height"], STITCH["width"], 4), dtype=F)
    rgba[..., 3] = 1.0
    rgba[:, 14:16, 3] = 0.0          # a gutter between the two triangles
    return rgba


def inputs():
    return dict(M.flat("stitch_lightmap", STITCH), **{"stitch_lightmap.uvs": UVS, "stitch_lightmap.rgba": atlas()})


@pytest.fixture(scope="module")
def probe(built):
    lib_dir = os.path.join(ROOT, "lupinpathtracer_amd")
    subprocess.check_call(["g++", *FLAGS, "-I" + os.path.join(ROOT, "include"), SOURCE, "-L" + lib_dir, "-llupin_hip", "-L/opt/rocm/lib", "-lz",
                           "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib", "-o", EXE])
    return EXE


def test_every_wrapper_of_the_header_has_a_section(probe):
    text = open(HEADER).read()
    names = set(re.findall(r"^inline [^\n(]*?(\w+)\(", text, re.M))
    assert names == {"stitch_lightmap", "lightmap_stitch_stats"}
    lines = subprocess.run([probe, "--list"], capture_output=True, text=True, check=True).stdout.splitlines()
    covered = set().union(*[set(line.split(":")[1].split()) for line in lines])
    assert names <= covered
    source = open(SOURCE).read()
    for name in names:
        assert re.search(r"\blp::" + name + r"\(", source), name
    assert '#include "lupin.hpp"' in text


@pytest.mark.gpu
def test_the_device_section_equals_the_python_host_word_for_word(gpu_ctx, probe, tmp_path):
    src, dst = os.path.join(str(tmp_path), "inputs.bin"), os.path.join(str(tmp_path), "outputs.bin")
    M.write_blob(src, inputs())
    p = subprocess.run([probe, src, dst, "stitch_lightmap"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    got = M.read_blob(dst)
    assert got["done.stitch_lightmap"] == 1
    s = STITCH
    scene = loader.build_scene_cornell_box(gpu_ctx)[0]
    assert scene.mesh_triangle_count(s["mesh_idx"]) == 2
    scene.set_lightmap_uvs(s["mesh_idx"], UVS)
    chart = api.LightmapChart(s["instance_idx"], float(F(s["scale_u"])), float(F(s["scale_v"])), float(F(s["offset_u"])), float(F(s["offset_v"])))
    out, info = api.stitch_lightmap(gpu_ctx, scene, [chart], atlas(), iterations=s["iterations"], samples_per_texel=s["samples_per_texel"], lam=s["lam"],
                                    want_info=True)
    assert info["seam_edges"] == 1 and info["sample_pairs"] in (21, 29) and info["active_texels"] > 20 and info["iterations"] == s["iterations"]
    assert int((out.view(np.uint32) != atlas().view(np.uint32)).sum()) > 60
    want_info = np.concatenate([np.uint32([info[k] for k in ("seam_edges", "non_manifold_edges", "sample_pairs", "dropped_pairs", "active_texels", "iterations")]),
                                info["energy_before"].view(np.uint32), info["energy_after"].view(np.uint32)])
    assert got["stitch_lightmap.out"].dtype == F and np.array_equal(got["stitch_lightmap.out"].view(np.uint32), out.view(np.uint32))
    assert np.array_equal(got["stitch_lightmap.info"], want_info)
    assert got["stitch_lightmap.timed"][0] == 1 and got["stitch_lightmap.refused"].tolist() == [1, 1, 1]
    assert got["stitch_lightmap.defaults"].tolist() == [32.0, 2.0, float(F(0.1))]
