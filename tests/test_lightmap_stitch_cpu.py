"""Lightmap seam stitching without a device: properties of the numpy restatement and of the float64 reference
(tests/lightmap_stitch_ref.py), plants that show the checks have teeth, the ABI's structs in the header, ctypes and the Rust
shim, the refusals that need no device, and include/lupin_stitch_rules.hpp under the sanitizers in a stand-alone program
(tests/stitch_rules_main.cpp)."""
import ctypes as C
import os
import re
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api, loader
from tests import lightmap_ref as R
from tests import lightmap_stitch_ref as S
from tests import lightmap_unwrap_ref as U
from tests.test_owned_cpu import SANITIZE_FLAGS, sanitizer_runtime_flags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
FACE_COLOURS = F([(0.9, 0.1, 0.1), (0.1, 0.8, 0.2), (0.2, 0.2, 0.9), (0.9, 0.8, 0.1), (0.1, 0.7, 0.8), (0.7, 0.2, 0.8)])


def unwrapped(mesh, texel, padding):
    """A mesh unwrapped by the restatement, as one chart over its own atlas: (charts as the restatement takes them, W, H,
    owner plane)."""
    pos, tris = mesh
    r = U.unwrap(pos, tris, texel, padding)
    W, H = r["width"], r["height"]
    chart = SimpleNamespace(instance_idx=0, scale_u=float(F(1.0) / F(W)), scale_v=float(F(1.0) / F(H)), offset_u=0.0, offset_v=0.0)
    owner, _, _ = R.raster([r["uvs"].reshape(-1, 2)], [np.arange(3 * len(tris)).reshape(-1, 3)], [chart], W, H)
    return [(tris, r["uvs"], chart)], W, H, owner


def cube_with_six_colours():
    charts, W, H, owner = unwrapped(U.cube(), 0.125, 2)           # faces of 8 x 8 texels
    rgba = np.zeros((H, W, 4), F)
    owned = owner != R.NO_OWNER
    rgba[owned, 0:3] = FACE_COLOURS[owner[owned] // 2]
    rgba[owned, 3] = 1.0
    return charts, rgba


def test_the_unwrapped_cube_has_twelve_seams():
    charts, rgba = cube_with_six_colours()
    rows = S.rows_of(rgba, charts, 2.0)
    assert (rows["seam_edges"], rows["non_manifold_edges"]) == (12, 0)
    assert rows["sample_pairs"] == 12 * 16 and rows["dropped_pairs"] == 0      # edges of 8 texels at 2 samples a texel
    w = rows["w"]
    assert np.allclose(w[:, :4].sum(axis=1), 1.0, atol=1e-6) and np.allclose(w[:, 4:].sum(axis=1), -1.0, atol=1e-6)
    assert np.all(w[:, :4] >= 0) and np.all(w[:, 4:] <= 0)


def test_a_bow_tie_and_a_planar_patch_have_no_seam():
    for mesh in (U.bowtie(), S.patch()):
        charts, W, H, owner = unwrapped(mesh, 0.09, 1)
        rgba = S.random_atlas(owner != R.NO_OWNER, 1)
        rows = S.rows_of(rgba, charts, 2.0)
        assert (rows["seam_edges"], rows["non_manifold_edges"], rows["sample_pairs"]) == (0, 0, 0)
        out, info = S.stitch(rgba, charts, 8)
        assert np.array_equal(out.view(np.uint32), rgba.view(np.uint32)) and info["active_texels"] == 0


def test_a_fin_has_one_non_manifold_edge_that_gives_no_pair():
    pos, tris = S.fin()
    uvs = F([[(1, 1), (1, 9), (9, 5)], [(11, 1), (11, 9), (19, 5)], [(21, 1), (21, 9), (29, 5)]])       # three sides of the shared edge
    chart = SimpleNamespace(instance_idx=0, scale_u=1.0 / 32, scale_v=1.0 / 16, offset_u=0.0, offset_v=0.0)
    rgba = np.ones((16, 32, 4), F)
    rows = S.rows_of(rgba, [(tris, uvs, chart)], 2.0)
    assert (rows["seam_edges"], rows["non_manifold_edges"], rows["sample_pairs"]) == (0, 1, 0)


def test_a_half_edge_with_equal_indices_is_skipped():
    tris = np.uint32([(0, 1, 2), (2, 1, 3), (4, 4, 1)])
    uvs = F([[(1, 1), (5, 1), (1, 5)], [(9, 5), (9, 1), (13, 5)], [(0, 0), (0, 0), (0, 0)]])
    chart = SimpleNamespace(instance_idx=0, scale_u=1.0 / 16, scale_v=1.0 / 8, offset_u=0.0, offset_v=0.0)
    edges, non_manifold = S.seam_edges([(tris, uvs, chart)], 16, 8)
    assert len(edges) == 1 and non_manifold == 0
    assert edges[0].tolist() == [5, 1, 1, 5, 9, 1, 9, 5]          # the vertex hA starts at comes first on both sides


def test_the_rows_are_the_views_fetch_on_both_sides():
    charts, rgba = cube_with_six_colours()
    rgba = S.random_atlas(rgba[..., 3] != 0, 7)
    rows = S.rows_of(rgba, charts, 2.0)
    A, active = S.dense_system(rows)
    x = rgba.reshape(-1, 4)[active, 0:3].astype(np.float64)
    by_rows = ((A @ x) ** 2).sum(axis=0)
    by_fetch = S.seam_energy_by_fetch(rgba, rows)
    assert np.allclose(by_rows, by_fetch, rtol=1e-5), (by_rows, by_fetch)


def cg_check(plant):
    """Whether float64 CG on the rows (as planted) never raises the true objective and reaches the true dense optimum within
    1e-9 relative by n_active steps."""
    charts, rgba = cube_with_six_colours()
    true_rows = S.rows_of(rgba, charts, 2.0)
    A, active = S.dense_system(true_rows)
    x0 = rgba.reshape(-1, 4)[active, 0:3].astype(np.float64)
    best = S.objective(A, S.dense_optimum(A, x0, 0.1), x0, 0.1)
    Ap, active_p = S.dense_system(S.rows_of(rgba, charts, 2.0, plant=plant))
    assert np.array_equal(active, active_p)
    xs = S.cg64(Ap, x0, 0.1, len(active))
    f = np.array([S.objective(A, x, x0, 0.1) for x in xs])
    assert np.all(best > 0) and np.all(best < f[0])
    monotone = bool(np.all(f[1:] <= f[:-1] * (1 + 1e-12)))
    reached = bool(np.all(np.abs(f[-1] - best) <= 1e-9 * best))
    return monotone, reached, f, best


def test_float64_cg_descends_to_the_dense_optimum():
    monotone, reached, f, best = cg_check(None)
    print("objective before", f[0], "after 16 steps", f[16], "optimum", best)
    assert monotone and reached


def test_a_wrong_sign_on_side_b_fails_that_check():
    monotone, reached, _, _ = cg_check("b_sign")
    assert not reached and not monotone


def test_a_reversed_incidence_order_changes_words():
    charts, rgba = cube_with_six_colours()
    rgba = S.random_atlas(rgba[..., 3] != 0, 3)
    rows = S.rows_of(rgba, charts, 2.0)
    want, _ = S.stitch(rgba, charts, 4, rows=rows)
    planted, _ = S.stitch(rgba, charts, 4, rows=rows, plant="reversed_incidence")
    assert int((want.view(np.uint32) != planted.view(np.uint32)).sum()) > 0
    assert np.allclose(want, planted, atol=1e-5)


def test_the_restatement_leaves_inactive_texels_and_lowers_the_energy():
    charts, rgba = cube_with_six_colours()
    out, info = S.stitch(rgba, charts, 16)
    rows = S.rows_of(rgba, charts, 2.0)
    active = S.incidence(rows)[0]
    mask = np.zeros(rgba.shape[0] * rgba.shape[1], bool)
    mask[active] = True
    assert np.array_equal(out.reshape(-1, 4)[~mask].view(np.uint32), rgba.reshape(-1, 4)[~mask].view(np.uint32))
    assert np.array_equal(out[..., 3].view(np.uint32), rgba[..., 3].view(np.uint32))
    assert info["active_texels"] == len(active) and np.all(info["energy_after"] < 0.5 * info["energy_before"])
    zero, info0 = S.stitch(rgba, charts, 0)
    assert np.array_equal(zero.view(np.uint32), rgba.view(np.uint32))
    assert np.array_equal(info0["energy_before"].view(np.uint32), info["energy_before"].view(np.uint32))


def test_the_sum_is_the_same_for_any_split_of_the_work():
    rng = np.random.default_rng(2)
    for n in (1, 63, 64, 65, 255, 256, 257, 256 * 64 + 3):
        v = rng.standard_normal((n, 3)).astype(F)
        got = S.fixed_sum(v)
        assert np.allclose(got, v.astype(np.float64).sum(axis=0), atol=1e-3 * np.sqrt(n))
        assert got.dtype == F


# ---- the ABI ----------------------------------------------------------------------------------------------------------

STRUCTS = (("LupinLightmapStitchDesc", _abi.LightmapStitchDescC, 28), ("LupinLightmapStitchInfo", _abi.LightmapStitchInfoC, 48),
           ("LupinLightmapStitchStats", _abi.LightmapStitchStatsC, 20))


def test_struct_sizes_and_offsets_match_the_header_ctypes_and_rust(built):
    header = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    rust = open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    for name, cls, size in STRUCTS:
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = re.findall(r"(float|uint32_t)\s+(\w+)(?:\[(\d+)\])?\s*;", body)
        assert [f for _, f, _ in fields] == [f for f, _ in cls._fields_]
        offset = 0
        for (t, f, n), (_, ct) in zip(fields, cls._fields_):
            base = C.c_float if t == "float" else C.c_uint32
            assert ct == (base * int(n) if n else base) or (n and ct._type_ == base and ct._length_ == int(n)), f
            assert getattr(cls, f).offset == offset, f
            offset += 4 * (int(n) if n else 1)
        assert C.sizeof(cls) == offset == size
        rs = re.search(r"pub struct %s \{(.*?)\}" % name, rust, re.S).group(1)
        rs_fields = re.findall(r"pub (\w+): ([\w\[\]; ]+),", rs)
        want = [(f, ("[%s; %s]" % (r, n)) if n else r) for t, f, n in fields for r in [{"float": "f32", "uint32_t": "u32"}[t]]]
        assert rs_fields == want
    assert (api.LIGHTMAP_STITCH_DEVICE_POINTERS, api.LIGHTMAP_STITCH_MAX_ITERATIONS, api.LIGHTMAP_STITCH_MAX_EDGE_SAMPLES) == (1, 1024, 65536)
    assert "#define LUPIN_LIGHTMAP_STITCH_MAX_ITERATIONS 1024u" in header and "#define LUPIN_LIGHTMAP_STITCH_MAX_EDGE_SAMPLES 65536u" in header
    assert S.MAX_EDGE_SAMPLES == api.LIGHTMAP_STITCH_MAX_EDGE_SAMPLES
    for fn in ("lupin_hip_stitch_lightmap", "lupin_hip_lightmap_stitch_stats"):
        assert re.search(r"pub fn %s\(" % fn, rust)
    cpp = open(os.path.join(ROOT, "include", "lupin_stitch.hpp")).read()
    assert "inline StitchResult stitch_lightmap(" in cpp


def test_the_symbols_exist_and_refuse_without_a_device(built):
    handle = C.CDLL(_abi.LIB_PATH)
    assert hasattr(handle, "lupin_hip_stitch_lightmap") and hasattr(handle, "lupin_hip_lightmap_stitch_stats")
    lib = _abi.lib()
    rgba, out = np.ones((4, 4, 4), F), np.full((4, 4, 4), -7.0, F)
    d = _abi.LightmapStitchDescC(4, 4, 1, 2.0, 0.1, 0, 0)
    chart = _abi.LightmapChartC(0, 1.0, 1.0, 0.0, 0.0)
    info = _abi.LightmapStitchInfoC(77, 77, 77, 77, 77, 77)
    rc = lib.lupin_hip_stitch_lightmap(None, None, C.byref(d), C.byref(chart), 1, _abi.ptr(rgba), _abi.ptr(out), C.byref(info))
    assert rc == (-1 if api.device_count() > 0 else -2)
    assert np.all(out == -7.0) and info.seam_edges == 77
    assert lib.lupin_hip_lightmap_stitch_stats(None) == -1
    stats = api.lightmap_stitch_stats()
    assert set(stats) == {"edges_ms", "samples_ms", "incidence_ms", "solve_ms", "call_ms"}
    scene = loader.build_scene_cornell_box(None)[0]          # a scene without a device
    with pytest.raises(api.LupinError) as e:
        api.stitch_lightmap(None, scene, [api.LightmapChart(0)], rgba)
    assert e.value.code == -2
    import inspect
    sig = inspect.signature(api.stitch_lightmap)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[4:]] == [("iterations", 32), ("samples_per_texel", 2.0), ("lam", 0.1),
                                                                                ("want_info", False)]


# ---- the host code under the sanitizers ---------------------------------------------------------------------------------

def test_the_descriptor_checks_under_the_sanitizers():
    with tempfile.TemporaryDirectory() as tmp:
        runtimes = sanitizer_runtime_flags(tmp)
        exe = os.path.join(tmp, "stitch_rules")
        build = subprocess.run(["g++"] + SANITIZE_FLAGS + runtimes + ["-O1", "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
                                os.path.join(ROOT, "tests", "stitch_rules_main.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
        assert build.returncode == 0, build.stderr[-4000:]
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
        run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
        print(run.stdout, run.stderr)
        assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
        assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
