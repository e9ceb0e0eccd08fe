"""Lightmap baking (lupin_hip_bake_lightmap), the parts that need no device: the rasterisation rule and the
dilation of the numpy restatement (tests/lightmap_ref.py) on cases worked out by hand, the layouts of the mirrors, the symbol."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import lightmap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUAD_UV = np.float32([[0, 0], [1, 0], [1, 1], [0, 1]])
QUAD_TRIS = np.uint32([[0, 1, 2], [0, 2, 3]])
# the unit square onto texels [2, 14)^2 of a 16 x 16 atlas: every product and sum below is exact in f32
INSET = api.LightmapChart(0, 0.75, 0.75, 0.125, 0.125)


def test_a_chart_on_whole_texels_owns_exactly_those():
    owner, u, v = ref.raster([QUAD_UV], [QUAD_TRIS], [INSET], 16, 16)
    inside = np.zeros((16, 16), bool)
    inside[2:14, 2:14] = True
    assert int((owner != ref.NO_OWNER).sum()) == 144
    assert np.array_equal(owner != ref.NO_OWNER, inside)
    # the shared edge runs through the centres (k + 0.5, k + 0.5): the lower key owns them; below it (x > y) triangle 0
    ys, xs = np.nonzero(inside)
    assert np.all(owner[ys, xs] == np.where(xs >= ys, 0, 1))
    assert all(owner[k, k] == 0 for k in range(2, 14))


def test_barycentrics_reconstruct_the_centre():
    chart = api.LightmapChart(0, 0.71, 0.53, 0.113, 0.291)         # nothing on whole texels
    W, H = 17, 33
    owner, u, v = ref.raster([QUAD_UV], [QUAD_TRIS], [chart], W, H)
    t, _, _ = ref.texel_triangles(QUAD_UV, QUAD_TRIS, chart, W, H)
    ys, xs = np.nonzero(owner != ref.NO_OWNER)
    assert len(ys) > 100
    tri = t[owner[ys, xs]].astype(np.float64)                       # (n, 3, 2)
    uu, vv = u[ys, xs].astype(np.float64), v[ys, xs].astype(np.float64)
    p = tri[:, 0] * (1 - uu - vv)[:, None] + tri[:, 1] * uu[:, None] + tri[:, 2] * vv[:, None]
    err = np.abs(p - np.stack([xs + 0.5, ys + 0.5], axis=1)).max()
    assert err <= 1e-5, err
    assert np.all(uu >= 0) and np.all(vv >= 0) and np.all(uu + vv <= 1 + 1e-6)


def test_triangles_the_rule_skips_own_nothing_and_cast_nothing_invalid():
    uv = np.float32([[0, 0], [1, 0], [1, 1], [0, 1],
                     [0.5, 0.5], [0.5, 0.5], [0.7, 0.7],            # 4..6: two vertices coincide
                     [0.2, 0.2], [0.4, 0.4], [0.6, 0.6],            # 7..9: collinear
                     [np.nan, 0.3], [0.8, 0.1], [0.9, 0.9],         # 10..12: a NaN
                     [1e30, 1e30], [2e30, 1e30], [1e30, 2e30],      # 13..15: far outside, area2 overflows
                     [-5, -5], [-4, -5], [-5, -4],                  # 16..18: below zero, a finite area
                     [np.inf, 0.1], [0.2, 0.2], [0.3, 0.9]])        # 19..21: an infinity
    tris = np.uint32([[4, 5, 6], [7, 8, 9], [10, 11, 12], [13, 14, 15], [16, 17, 18], [19, 20, 21], [0, 1, 2], [0, 2, 3]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        owner, _, _ = ref.raster([uv], [tris], [INSET], 16, 16)
    assert set(np.unique(owner).tolist()) == {6, 7, ref.NO_OWNER}
    assert int((owner != ref.NO_OWNER).sum()) == 144
    _, area2, ok = ref.texel_triangles(uv, tris, INSET, 16, 16)
    assert ok.tolist() == [False, False, False, False, True, False, True, True]
    assert np.isinf(area2[3]) or np.isnan(area2[3])


def test_a_mirrored_chart_owns_what_its_mirror_owns():
    plain, u0, v0 = ref.raster([QUAD_UV], [QUAD_TRIS], [INSET], 16, 16)
    mirrored_chart = api.LightmapChart(0, -0.75, 0.75, 0.875, 0.125)        # u -> 1 - u inside the same texels: area2 < 0
    _, area2, ok = ref.texel_triangles(QUAD_UV, QUAD_TRIS, mirrored_chart, 16, 16)
    assert np.all(area2 < 0) and ok.all()
    mirrored, u1, v1 = ref.raster([QUAD_UV], [QUAD_TRIS], [mirrored_chart], 16, 16)
    assert np.array_equal(mirrored, plain[:, ::-1])
    assert np.array_equal(u1, u0[:, ::-1]) and np.array_equal(v1, v0[:, ::-1])
    # an earlier chart keeps what a later one also covers
    both, _, _ = ref.raster([QUAD_UV, QUAD_UV], [QUAD_TRIS, QUAD_TRIS], [INSET, api.LightmapChart(0, 1.0, 1.0, 0.0, 0.0)], 16, 16)
    assert np.array_equal(both[2:14, 2:14], plain[2:14, 2:14]) and int((both >= 2).sum()) == 256 - 144 and both.max() <= 3


def test_dilation_of_a_pattern_worked_out_by_hand():
    a = np.zeros((5, 5, 4), np.float32)
    a[0, 0] = (1, 10, 100, 1)
    a[0, 2] = (3, 30, 300, 1)
    a[2, 2] = (8, 80, 800, 1)
    one = ref.dilate(a, 1)
    assert np.array_equal(ref.dilate(a, 0), a)
    want = np.zeros((5, 5, 4), np.float32)
    want[0, 0], want[0, 2], want[2, 2] = a[0, 0], a[0, 2], a[2, 2]
    want[0, 1, :3] = np.float32([4, 40, 400]) / np.float32(2)                    # (0,0) + (0,2)
    want[1, 0, :3] = (1, 10, 100)
    want[1, 1, :3] = (np.float32([1, 10, 100]) + np.float32([3, 30, 300]) + np.float32([8, 80, 800])) / np.float32(3)
    want[1, 2, :3] = np.float32([11, 110, 1100]) / np.float32(2)                 # (0,2) + (2,2)
    want[1, 3, :3] = np.float32([11, 110, 1100]) / np.float32(2)
    want[0, 3, :3] = (3, 30, 300)
    for y, x in ((2, 1), (2, 3), (3, 1), (3, 2), (3, 3)):
        want[y, x, :3] = (8, 80, 800)
    assert np.array_equal(one, want)
    assert np.all(one[..., 3] == a[..., 3])                                      # alpha: rasterised texels only
    two = ref.dilate(a, 2)
    # pass 2 fills from pass 1's texels as well: (4, 0) has the one filled neighbour (3, 1); (0, 4) has (0, 3) and (1, 3)
    assert np.array_equal(two[4, 0, :3], one[3, 1, :3])
    assert np.array_equal(two[0, 4, :3], (one[0, 3, :3] + one[1, 3, :3]) / np.float32(2))
    assert np.array_equal(two[1, 1], one[1, 1]) and np.all(two[..., 3] == a[..., 3])
    assert np.all((ref.dilate(a, 3)[..., :3] != 0).any(axis=-1))                 # three passes reach every texel


def c_struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s+(\w+);", body)


def test_symbol_resolves_and_struct_layouts_agree(built):
    lib = _abi.lib()
    assert hasattr(lib, "lupin_hip_bake_lightmap") and hasattr(lib, "lupin_hip_lightmap_stats")
    header = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    rust = open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    c_size = {"uint32_t": 4, "float": 4, "uint64_t": 8, "LupinAdvancedParams": C.sizeof(_abi.AdvancedParamsC)}
    r_size = {"u32": 4, "f32": 4, "u64": 8, "LupinAdvancedParams": 12}
    for name, mirror, size in (("LupinLightmapChart", _abi.LightmapChartC, 20), ("LupinLightmapDesc", _abi.LightmapDescC, 52),
                               ("LupinLightmapStats", _abi.LightmapStatsC, 32)):
        fields = c_struct_fields(header, name)
        assert [n for _, n in fields] == [n for n, _ in mirror._fields_], name
        # no padding anywhere: the packed sum of the members is the size, and every offset is the sum before it
        assert sum(c_size[t] for t, _ in fields) == size == C.sizeof(mirror), name
        at = 0
        for t, n in fields:
            assert getattr(mirror, n).offset == at, (name, n)
            at += c_size[t]
        rbody = re.search(r"pub struct %s \{(.*?)\}" % name, rust, re.S).group(1)
        r_fields = re.findall(r"pub (\w+): (\w+)", rbody)
        assert [n for n, _ in r_fields] == [n for _, n in fields], name
        assert sum(r_size[t] for _, t in r_fields) == size, name
    assert _abi.LightmapDescC.surface_offset.offset == 36 and _abi.LightmapDescC.advanced.offset == 40
    assert "pub fn lupin_hip_bake_lightmap(" in rust
    for must in ("LUPIN_LIGHTMAP_SMOOTH_NORMALS = 1u", "#define LUPIN_LIGHTMAP_MAX_SIZE 16384u", "#define LUPIN_LIGHTMAP_MAX_DILATE 64u"):
        assert must in header
    assert (api.LIGHTMAP_SMOOTH_NORMALS, api.LIGHTMAP_MAX_SIZE, api.LIGHTMAP_MAX_DILATE) == (1, 16384, 64)
    cpp = open(os.path.join(ROOT, "include", "lupin.hpp")).read()
    assert "inline uint64_t bake_lightmap(" in cpp


def test_without_a_device_the_call_says_so(built):
    out = np.full((4, 4, 4), 7.0, np.float32)
    desc = _abi.LightmapDescC(4, 4, 0, 8, 1, 0, 0, 0, 0, 1e-3, _abi.AdvancedParamsC(100.0, 0, 0.001))
    chart = _abi.LightmapChartC(0, 1.0, 1.0, 0.0, 0.0)
    rc = _abi.lib().lupin_hip_bake_lightmap(None, None, C.byref(desc), C.byref(chart), 1, _abi.ptr(out), None, None)
    # LUPIN_ERR_NO_DEVICE; where there is a device, a null context is an invalid argument
    assert rc == (-2 if api.device_count() < 1 else -1)
    assert np.all(out == 7.0)
    from lupinpathtracer_amd import loader
    scene, _ = loader.build_scene_cornell_box(None)
    with pytest.raises(api.LupinError) as e:
        api.bake_lightmap(None, scene, [api.LightmapChart(0)], 16, 16)
    assert e.value.code == -2


def test_default_surface_offset_comes_from_the_model_boxes(built):
    from lupinpathtracer_amd import loader
    scene, _ = loader.build_scene_cornell_box(None)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    cpu, _ = loader.cornell_box_scene_cpu()
    for inst in cpu.instances:
        m = np.asarray(inst["transpose_inverse_transform"], np.float64)
        v = np.asarray(cpu.verts_pos_array[int(inst["mesh_idx"])], np.float64)[:, :3]
        world = (v - m[:, 3]) @ np.linalg.inv(m[:, :3]).T
        lo, hi = np.minimum(lo, world.min(axis=0)), np.maximum(hi, world.max(axis=0))
    # the box of the boxes bounds the box of the vertices, and equals it under the Cornell box's axis-aligned transforms
    assert api.scene_world_extent(scene) == pytest.approx(float((hi - lo).max()), rel=1e-6)
    assert api.LIGHTMAP_OFFSET_FRACTION == 1e-4
