"""The lightmap unwrap without a device: properties of the numpy restatement (tests/lightmap_unwrap_ref.py) on
inputs chosen so that they hold, the shelf packer, the ABI's structs in the header, ctypes and the Rust shim, the refusals that
need no device, and include/lupin_pack.hpp under the sanitizers in a stand-alone program (tests/unwrap_pack_main.cpp)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api, loader
from tests import lightmap_ref as R
from tests import lightmap_unwrap_ref as U
from tests import util
from tests.test_owned_cpu import SANITIZE_FLAGS, sanitizer_runtime_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def sizes(r):
    c = r["chart_of_tri"]
    return np.bincount(c[c != U.NO_CHART]).tolist()


def test_a_cube_with_shared_vertices_is_six_charts_of_two_triangles():
    r = U.unwrap(*U.cube(), 0.1, 1)
    assert r["num_charts"] == 6 and sizes(r) == [2] * 6 and r["degenerate_tris"] == 0
    assert sorted(set(r["bucket"].tolist())) == [0, 1, 2, 3, 4, 5]
    assert np.array_equal(np.unique(r["labels"]), [0, 2, 4, 6, 8, 10])      # a label is the smallest triangle of its chart


def test_an_octahedron_is_two_charts_because_every_tie_goes_to_x():
    r = U.unwrap(*U.octahedron(), 0.1, 1)
    assert r["num_charts"] == 2 and sizes(r) == [4, 4] and set(r["bucket"].tolist()) == {0, 1}


def test_a_bow_tie_is_one_chart_and_two_patches_are_two():
    assert U.unwrap(*U.bowtie(), 0.1, 1)["num_charts"] == 1
    r = U.unwrap(*U.two_patches(), 0.1, 1)
    assert r["num_charts"] == 2 and set(r["bucket"].tolist()) == {4}


def test_a_chain_is_one_chart_in_either_order():
    for reverse in (False, True):
        r = U.unwrap(*U.chain(reverse=reverse), 0.13, 1)
        assert r["num_charts"] == 1 and sizes(r) == [4099] and np.all(r["labels"] == 0)


def test_degenerate_and_nan_triangles_are_counted_and_zeroed():
    pos, tris = U.with_bad_triangles()
    r = U.unwrap(pos, tris, 0.1, 1)
    assert r["degenerate_tris"] == 2 and r["num_charts"] == 2
    bad = r["chart_of_tri"] == U.NO_CHART
    assert bad.tolist() == [False, False, True, True, False, False] and np.all(r["uvs"][bad] == 0) and np.all(np.isfinite(r["uvs"]))
    assert r["chart_of_tri"][~bad].tolist() == [0, 0, 1, 1]


def test_no_chart_is_mirrored_and_the_unit_is_the_texel():
    pos, tris = U.cube(0.6)
    r = U.unwrap(pos, tris, 0.05, 2)
    uv = r["uvs"].astype(np.float64)
    area2 = (uv[:, 1, 0] - uv[:, 0, 0]) * (uv[:, 2, 1] - uv[:, 0, 1]) - (uv[:, 1, 1] - uv[:, 0, 1]) * (uv[:, 2, 0] - uv[:, 0, 0])
    assert np.all(area2 > 0)
    assert np.allclose(area2, 12.0 * 12.0, rtol=1e-5)          # a face of side 0.6 at 0.05 a texel: two triangles of half 12 x 12 texels
    for x, y, w, h in r["rects"].values():
        assert (w, h) == (12 + 4, 12 + 4)
    assert uv.min() >= 2.0 and uv[..., 0].max() <= r["width"] - 2.0 and uv[..., 1].max() <= r["height"] - 2.0


def ply(name):
    cpu = api.SceneCPU()
    loader.load_mesh_ply(os.path.join(util.SHARED, "shapes", name + ".ply"), cpu)
    return np.asarray(cpu.verts_pos_array[0], F)[:, :3], cpu.indices_array[0].reshape(-1, 3)


# mesh: (positions and triangles, texel size).  The fixtures are 0.15 across; the texel sizes make a typical triangle several
# texels wide (the sphere's and the cylinder's are about 0.004 long, the bunny's about 0.0007).
MESHES = {"cube": lambda: U.cube(0.6), "sphere": lambda: ply("sphere"), "uvcylinder": lambda: ply("uvcylinder"), "bunny": lambda: ply("bunny")}
RASTER_INPUTS = {"cube": 0.05, "sphere": 0.001, "uvcylinder": 0.001, "bunny": 0.0005}
# The third property is a condition on the input: a thin diagonal triangle's bounding box can span two texels both ways and
# still miss every centre, and the bunny has such slivers at 0.0005 (22 of its 29 590 spanning triangles) and at 0.00025 (7 of
# 141 609).  At a texel of the bunny's own triangle size, 0.0007, the spanning triangles are its few large ones and each owns
# a texel: that is the input the property is asserted on.  The other meshes keep the texel size of the first two properties.
SPAN_INPUTS = dict(RASTER_INPUTS, bunny=0.0007)
_whole = {}


def whole_raster(name, texel):
    """(the unwrap of a mesh with padding 1, its owner plane through tests/lightmap_ref.py's rasteriser in the mesh's own
    atlas: scale 1 / size, offset 0), computed once per (mesh, texel size)."""
    if (name, texel) not in _whole:
        pos, tris = MESHES[name]()
        r = U.unwrap(pos, tris, texel, 1)
        chart = api.LightmapChart(0, 1.0 / r["width"], 1.0 / r["height"], 0.0, 0.0)
        uvs, corners = U.corner_set(r["uvs"])
        _whole[name, texel] = (r, R.raster([uvs], [corners], [chart], r["width"], r["height"])[0])
    return _whole[name, texel]


@pytest.fixture(scope="module", params=list(RASTER_INPUTS))
def rastered(request):
    """whole_raster, and every chart rasterised on its own: per texel the number of charts that cover its centre."""
    name, texel = request.param, RASTER_INPUTS[request.param]
    r, owner = whole_raster(name, texel)
    W, H = r["width"], r["height"]
    chart = api.LightmapChart(0, 1.0 / W, 1.0 / H, 0.0, 0.0)
    uvs, corners = U.corner_set(r["uvs"])
    covered_by = np.zeros((H, W), np.int64)
    for c in range(r["num_charts"]):
        sel = r["chart_of_tri"] == c
        covered_by += R.raster([uvs], [corners[sel]], [chart], W, H)[0] != R.NO_OWNER
    return name, r, owner, covered_by, texel


def test_no_texel_centre_is_covered_by_two_charts(rastered):
    name, r, owner, covered_by, _ = rastered
    assert covered_by.max() == 1, name
    assert np.array_equal(covered_by == 1, owner != R.NO_OWNER)
    assert (owner != R.NO_OWNER).mean() > 0.2, name


def test_with_padding_texels_of_different_charts_are_never_neighbours(rastered):
    name, r, owner, _, _ = rastered
    chart = np.where(owner != R.NO_OWNER, r["chart_of_tri"][np.minimum(owner, len(r["chart_of_tri"]) - 1)].astype(np.int64), -1)
    H, W = chart.shape
    padded = np.full((H + 2, W + 2), -1, np.int64)
    padded[1:-1, 1:-1] = chart
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            other = padded[dy:dy + H, dx:dx + W]
            assert not ((chart >= 0) & (other >= 0) & (other != chart)).any(), (name, dy, dx)


@pytest.mark.parametrize("name", list(SPAN_INPUTS))
def test_every_triangle_that_spans_two_texels_both_ways_owns_a_texel(name):
    r, owner = whole_raster(name, SPAN_INPUTS[name])
    uv = r["uvs"]
    good = r["chart_of_tri"] != U.NO_CHART
    span = (uv.max(axis=1) - uv.min(axis=1) >= 2).all(axis=1) & good
    owners = np.zeros(len(uv), bool)
    owners[owner[owner != R.NO_OWNER]] = True
    print(name, "triangles:", len(uv), "spanning two texels both ways:", int(span.sum()), "of them without a texel:", int((span & ~owners).sum()))
    assert span.sum() > 0 and not (span & ~owners).any(), name
    # and what holds at any texel size: a triangle whose inscribed circle has a radius of sqrt(2) / 2 texels contains a centre
    p = uv.astype(np.float64)
    a, b, c = (np.linalg.norm(p[:, i] - p[:, j], axis=1) for i, j in ((0, 1), (1, 2), (2, 0)))
    area = 0.5 * np.abs((p[:, 1, 0] - p[:, 0, 0]) * (p[:, 2, 1] - p[:, 0, 1]) - (p[:, 1, 1] - p[:, 0, 1]) * (p[:, 2, 0] - p[:, 0, 0]))
    fat = good & (area / np.maximum(0.5 * (a + b + c), 1e-30) >= np.sqrt(0.5) + 1e-6)
    assert not (fat & ~owners).any(), name


# ---- the packer -----------------------------------------------------------------------------------------------------

def check_packing(rects):
    width, height, place = api.shelf_pack(rects)
    w2, h2, place2 = U.shelf_pack([(w, h, i) for i, (w, h) in enumerate(rects)])
    assert (width, height) == (w2, h2) and place == [place2[i] for i in range(len(rects))]      # the host's packer is the restatement's
    boxes = [(x, y, x + w, y + h) for (x, y), (w, h) in zip(place, rects)]
    for i, a in enumerate(boxes):
        assert 0 <= a[0] and 0 <= a[1] and a[2] <= width and a[3] <= height
        for b in boxes[:i]:
            assert a[2] <= b[0] or b[2] <= a[0] or a[3] <= b[1] or b[3] <= a[1], (a, b)
    return width, height, place


def test_the_packer_keeps_rectangles_apart_and_inside():
    assert check_packing([(7, 3)]) == (7, 3, [(0, 0)])                                    # one rectangle
    assert check_packing([(4, 4)] * 4)[:2] == (8, 8)                                      # equal rectangles
    assert check_packing([(40, 2), (3, 5), (3, 3)])[0] == 40                              # one as wide as the atlas
    rng = np.random.default_rng(5)
    for n in (2, 3, 17, 300):
        check_packing([(int(w), int(h)) for w, h in rng.integers(1, 40, (n, 2))])
    assert api.shelf_pack([]) == (0, 0, [])
    assert [api.isqrt_ceil(n) for n in (0, 1, 2, 4, 5, 16384 ** 2, 16384 ** 2 + 1)] == [0, 1, 2, 2, 3, 16384, 16385]


def test_instances_are_placed_by_the_same_packer():
    width, height, charts = api.pack_lightmap_instances([(30, 36), (18, 22), (18, 22)], [1.0, 2.0, 0.5], 2)
    rects = [(34, 40), (40, 48), (13, 15)]
    assert (width, height) == api.shelf_pack(rects)[:2]
    for i, (c, (x, y), m) in enumerate(zip(charts, api.shelf_pack(rects)[2], (1.0, 2.0, 0.5))):
        assert c.instance_idx == i
        assert (F(c.scale_u), F(c.scale_v)) == (F(m) / F(width), F(m) / F(height))
        assert (F(c.offset_u), F(c.offset_v)) == (F(x + 2) / F(width), F(y + 2) / F(height))
    for bad in (dict(sizes=[(8, 8)], multipliers=[0.0]), dict(sizes=[(0, 8)], multipliers=[1.0]), dict(sizes=[(16000, 8)], multipliers=[2.0]),
                dict(sizes=[(8, 8)], multipliers=[float("nan")]), dict(sizes=[(8, 8)], multipliers=[1.0, 2.0])):
        with pytest.raises(ValueError):
            api.pack_lightmap_instances(gutter=1, **bad)


# ---- the ABI ----------------------------------------------------------------------------------------------------------

def test_struct_sizes_and_offsets_match_the_header_ctypes_and_rust(built):
    header = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    rust = open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    for name, cls in (("LupinUnwrapDesc", _abi.UnwrapDescC), ("LupinUnwrapInfo", _abi.UnwrapInfoC)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"(float|uint32_t)\s+(\w+)\s*;", body)
        assert [f for _, f in fields] == [f for f, _ in cls._fields_]
        assert [C.c_float if t == "float" else C.c_uint32 for t, _ in fields] == [t for _, t in cls._fields_]
        assert C.sizeof(cls) == 4 * len(fields) and [getattr(cls, f).offset for f, _ in cls._fields_] == [4 * i for i in range(len(fields))]
        rs = re.search(r"pub struct %s \{(.*?)\}" % name, rust, re.S).group(1)
        rs_fields = re.findall(r"pub (\w+): (\w+)", rs)
        assert [(f, {"float": "f32", "uint32_t": "u32"}[t]) for t, f in fields] == rs_fields
    assert (C.sizeof(_abi.UnwrapDescC), C.sizeof(_abi.UnwrapInfoC)) == (12, 32)
    assert (api.UNWRAP_MAX_PADDING, api.UNWRAP_NO_CHART) == (16, 0xFFFFFFFF)
    assert "#define LUPIN_UNWRAP_MAX_PADDING 16u" in header and "#define LUPIN_UNWRAP_NO_CHART 0xFFFFFFFFu" in header
    for fn in ("lupin_hip_scene_set_lightmap_uvs", "lupin_hip_unwrap_lightmap_uvs"):
        assert re.search(r"pub fn %s\(" % fn, rust)


def test_the_symbols_exist_and_refuse_without_a_device(built):
    handle = C.CDLL(_abi.LIB_PATH)
    assert hasattr(handle, "lupin_hip_scene_set_lightmap_uvs") and hasattr(handle, "lupin_hip_unwrap_lightmap_uvs")
    assert callable(api.Scene.set_lightmap_uvs) and callable(api.Scene.unwrap_lightmap_uvs) and callable(api.pack_lightmap_instances)
    lib = _abi.lib()
    uvs = np.full((2, 3, 2), -7.0, F)
    assert lib.lupin_hip_scene_set_lightmap_uvs(None, 0, _abi.ptr(uvs), 6) == -1          # a NULL scene
    assert lib.lupin_hip_scene_mesh_triangle_count(None, 0) == -1
    d = _abi.UnwrapDescC(0.1, 1, 0)
    info = _abi.UnwrapInfoC(77, 77, 77, 77, 0, 0, 0, 0)
    rc = lib.lupin_hip_unwrap_lightmap_uvs(None, None, 0, C.byref(d), _abi.ptr(uvs), None, C.byref(info))
    assert rc == (-1 if api.device_count() > 0 else -2)
    assert np.all(uvs == -7.0) and info.num_charts == 77
    scene = loader.build_scene_cornell_box(None)[0]          # a scene without a device
    assert scene.mesh_triangle_count(5) == 12
    for call in (lambda: scene.set_lightmap_uvs(5, np.zeros((12, 3, 2), F)), lambda: scene.unwrap_lightmap_uvs(5, 0.05)):
        with pytest.raises(api.LupinError) as e:
            call()
        assert e.value.code == -2


# ---- the host code under the sanitizers ---------------------------------------------------------------------------------

def test_the_packer_and_the_descriptor_checks_under_the_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        runtimes = sanitizer_runtime_flags(tmp)
        exe = os.path.join(tmp, "unwrap_pack")
        build = subprocess.run(["g++"] + SANITIZE_FLAGS + runtimes + ["-O1", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                                os.path.join(ROOT, "tests", "unwrap_pack_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
        assert build.returncode == 0, build.stderr[-4000:]
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
        print(run.stdout, run.stderr)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
