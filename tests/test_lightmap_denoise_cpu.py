"""The lightmap denoiser (lupin_hip_denoise_lightmap), the parts that need no device: the layouts of the
mirrors and the symbol, and the properties of the numpy restatement (tests/lightmap_denoise_ref.py) on atlases small enough
to reason about by hand -- each with a planted defect that the property must notice."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import lightmap_denoise_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
SMALL = F(2.0 ** -20)


def c_struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return re.findall(r"(\w+)\s+(\w+)(?:\[(\d+)\])?;", body)


def test_symbol_resolves_and_struct_layouts_agree(built):
    lib = _abi.lib()
    assert hasattr(lib, "lupin_hip_denoise_lightmap") and hasattr(lib, "lupin_hip_lightmap_denoise_stats")
    header = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    rust = open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    c_size = {"uint32_t": 4, "float": 4}
    r_size = {"u32": 4, "f32": 4, "[f32; 8]": 32}
    for name, mirror, size in (("LupinLightmapDenoiseDesc", _abi.LightmapDenoiseDescC, 28), ("LupinLightmapDenoiseStats", _abi.LightmapDenoiseStatsC, 44)):
        fields = c_struct_fields(header, name)
        assert [n for _, n, _ in fields] == [n for n, _ in mirror._fields_], name
        # no padding anywhere: the packed sum of the members is the size, and every offset is the sum before it
        at = 0
        for t, n, count in fields:
            assert getattr(mirror, n).offset == at, (name, n)
            at += c_size[t] * int(count or 1)
        assert at == size == C.sizeof(mirror), name
        rbody = re.search(r"pub struct %s \{(.*?)\}" % name, rust, re.S).group(1)
        r_fields = re.findall(r"pub (\w+): (\[f32; 8\]|\w+)", rbody)
        assert [n for n, _ in r_fields] == [n for _, n, _ in fields], name
        assert sum(r_size[t] for _, t in r_fields) == size, name
    assert _abi.LightmapDenoiseDescC.max_stretch.offset == 24
    assert "pub fn lupin_hip_denoise_lightmap(" in rust and "pub fn lupin_hip_lightmap_denoise_stats(" in rust
    for must in ("LUPIN_LIGHTMAP_DENOISE_DEVICE_POINTERS = 1u", "#define LUPIN_LIGHTMAP_DENOISE_MAX_PASSES 8u", "#define LUPIN_LIGHTMAP_DENOISE_MAX_SQUARINGS 7u"):
        assert must in header
    assert (api.LIGHTMAP_DENOISE_DEVICE_POINTERS, api.LIGHTMAP_DENOISE_MAX_PASSES, api.LIGHTMAP_DENOISE_MAX_SQUARINGS) == (1, 8, 7)
    cpp = open(os.path.join(ROOT, "include", "lupin.hpp")).read()
    assert "inline void denoise_lightmap(" in cpp
    import inspect
    sig = inspect.signature(api.denoise_lightmap)
    assert [(k, p.default) for k, p in sig.parameters.items()][3:] == [("passes", 5), ("normal_squarings", 5), ("max_stretch", 4.0), ("dilate", 0)]
    bake = inspect.signature(api.bake_lightmap)
    assert list(bake.parameters)[-1] == "denoise" and bake.parameters["denoise"].default is False


def test_without_a_device_the_call_says_so(built):
    rgba, rec = ref.two_charts()
    out = np.full((8, 16, 4), 7.0, F)
    desc = _abi.LightmapDenoiseDescC(16, 8, 5, 5, 0, 0, 4.0)
    rc = _abi.lib().lupin_hip_denoise_lightmap(None, C.byref(desc), _abi.ptr(rgba), _abi.ptr(rec), _abi.ptr(out))
    # LUPIN_ERR_NO_DEVICE; where there is a device, a null context is an invalid argument
    assert rc == (-2 if api.device_count() < 1 else -1)
    assert np.all(out == 7.0)
    with pytest.raises(api.LupinError) as e:
        api.denoise_lightmap(None, rgba, rec)
    assert e.value.code == -2


def test_two_charts_side_by_side_do_not_mix():
    rgba, rec = ref.two_charts()
    got = ref.denoise(rgba, rec, passes=5)
    assert np.array_equal(got, rgba)                       # exactly: sum w c / sum w of a power of two is exact
    leaky = ref.denoise(rgba, rec, passes=5, defects=("no_footprint",))
    assert not np.array_equal(leaky, rgba)
    assert leaky[:, :8, 0].max() > 1.0 and leaky[:, 8:, 0].min() < 4.0


def test_a_folded_chart_does_not_mix_across_the_fold():
    rgba, rec = ref.folded_chart()
    # across the fold the texels ARE neighbours in space: the footprint lets them through, the normals do not
    _, _, g, foot = ref.prep(rgba, rec)
    assert g.all() and np.all(foot[:, 7] == F(0.5)) and np.all(foot[:, :7] == 1.0)
    got = ref.denoise(rgba, rec, passes=5)
    assert np.array_equal(got, rgba)
    leaky = ref.denoise(rgba, rec, passes=5, defects=("no_normal",))
    assert leaky[:, :8, 0].max() > 1.0 and leaky[:, 8:, 0].min() < 4.0


def test_a_hole_is_never_a_tap():
    # a chart of 2^-20: next to the 1e-4 of s_p a step to zero is no edge, so only the tap rule keeps the hole's zeros out
    rgba, rec = ref.chart_with_a_hole(SMALL)
    got = ref.denoise(rgba, rec, passes=5)
    assert np.array_equal(got, rgba)                       # the chart stays 2^-20 exactly, the hole as it came
    bled = ref.denoise(rgba, rec, passes=5, defects=("unguided_taps",))
    owned = rgba[..., 3] != 0
    assert bled[owned][:, 0].min() < 0.9 * SMALL           # the hole's zeros came in
    assert np.array_equal(bled[~owned], rgba[~owned])


def test_an_isolated_texel_passes_through():
    rgba = np.zeros((7, 7, 4), F)
    rec = np.zeros((7, 7, 8), F)
    rgba[3, 3] = (2.5, 0.75, 6.0, 1.0)
    rec[3, 3] = ref.plane_records(7, 7)[3, 3]
    c, var, g, foot = ref.prep(rgba, rec)
    assert int(g.sum()) == 1 and foot[3, 3] == 0.0 and var[3, 3] == 0.0
    assert np.array_equal(ref.denoise(rgba, rec, passes=5), rgba)
    # two texels that touch only at a corner have no 4-neighbour either
    rgba[4, 4] = (1.5, 1.5, 1.5, 1.0)
    rec[4, 4] = ref.plane_records(7, 7)[4, 4]
    assert np.all(ref.prep(rgba, rec)[3] == 0.0)
    assert np.array_equal(ref.denoise(rgba, rec, passes=5), rgba)


def test_texels_that_are_not_guided_are_no_taps_and_keep_their_value():
    rgba, rec = ref.chart_with_a_hole(SMALL)               # (small values: see the hole)
    rgba[6:9, 5:8] = (SMALL, SMALL, SMALL, 1.0)            # no hole this time
    rec[2, 3, 1] = np.nan                                  # a NaN position
    rgba[2, 3, :3] = 4 * SMALL
    rec[10, 12, 4:7] = (0.0, 0.0, 0.9)                     # a normal of length 0.9
    rgba[10, 12, :3] = 4 * SMALL
    rec[12, 4, 6] = np.inf                                 # an infinite normal, and a NaN colour
    rgba[12, 4, :3] = (np.nan, 3.0, np.inf)
    g = ref.guided(rgba, rec)
    assert int((~g).sum()) == 3 and not g[2, 3] and not g[10, 12] and not g[12, 4]
    got = ref.denoise(rgba, rec, passes=5)
    want = rgba.copy()
    want[12, 4, :3] = (0.0, 3.0, 0.0)
    assert np.array_equal(got, want)                       # 2^-18 reached nobody, and stayed
    # the twin: were they taps, their neighbours would have moved
    assert not np.array_equal(ref.denoise(rgba, rec, passes=5, defects=("unguided_taps",)), want)


def test_gutters_are_refilled_from_the_filtered_texels_by_the_bakes_rule():
    a = np.zeros((5, 5, 4), F)
    a[..., :3] = 77.0                                      # what an earlier gutter fill left behind
    a[0, 0] = (1, 10, 100, 1)
    a[0, 2] = (3, 30, 300, 1)
    a[2, 2] = (8, 80, 800, 1)
    rec = np.zeros((5, 5, 8), F)
    for k, (y, x) in enumerate(((0, 0), (0, 2), (2, 2))):  # three texels far from one another in space: the filter leaves them
        rec[y, x] = ref.plane_records(1, 1, origin=(100.0 * k, 0.0, 0.0))[0, 0]
    assert np.array_equal(ref.denoise(a, rec, dilate=0), a)
    one = ref.denoise(a, rec, dilate=1)
    want = np.zeros((5, 5, 4), F)
    want[0, 0], want[0, 2], want[2, 2] = a[0, 0], a[0, 2], a[2, 2]
    want[0, 1, :3] = F([4, 40, 400]) / F(2)                                      # (0,0) + (0,2)
    want[1, 0, :3] = (1, 10, 100)
    want[1, 1, :3] = (F([1, 10, 100]) + F([3, 30, 300]) + F([8, 80, 800])) / F(3)
    want[1, 2, :3] = F([11, 110, 1100]) / F(2)                                   # (0,2) + (2,2)
    want[1, 3, :3] = F([11, 110, 1100]) / F(2)
    want[0, 3, :3] = (3, 30, 300)
    for y, x in ((2, 1), (2, 3), (3, 1), (3, 2), (3, 3)):
        want[y, x, :3] = (8, 80, 800)
    assert np.array_equal(one, want)                                             # among it: zeros where one pass does not reach
    three = ref.denoise(a, rec, dilate=3)
    assert np.all((three[..., :3] != 0).any(axis=-1)) and not np.any(three == 77.0)
    assert np.array_equal(three[..., 3], a[..., 3])
    assert np.array_equal(three[4, 0, :3], one[3, 1, :3])                        # pass 2 filled (4, 0) from (3, 1); pass 3 keeps it
    assert np.array_equal(three[0, 4, :3], (one[0, 3, :3] + one[1, 3, :3]) / F(2))


def test_one_pass_reduces_the_variance_of_flat_noise_as_the_kernel_predicts():
    # sigma far below the 1e-4 of s_p = 1 / (4 sigma + 1e-4): |l_p - l_q| s_p ~ 1e-2 and the edge-stopping term is ~ 0.99, so a
    # pass is the plain B3 kernel, and a sum of independent values weighted by h_x h_y has (sum h^2)^2 of their variance
    sigma = 1e-6
    noise = np.random.default_rng(5).normal(0.0, sigma, (32, 32)).astype(F)
    rgba = ref.constant_atlas(32, 32, 0.0)
    rgba[..., :3] = noise[..., None]
    rec = ref.plane_records(32, 32)
    got = ref.denoise(rgba, rec, passes=1)
    ratio = float(got[2:-2, 2:-2, 0].astype(np.float64).var() / noise[2:-2, 2:-2].astype(np.float64).var())
    predicted = (70.0 / 256.0) ** 2
    print(f"variance ratio {ratio:.5f}, predicted {predicted:.5f}")
    assert abs(ratio / predicted - 1.0) <= 0.2, (ratio, predicted)
