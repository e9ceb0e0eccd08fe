"""lp::denoise without a device: the C ABI, the Python surface and the numpy restatement of the filter (tests/denoise_ref.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import denoise_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("lupin_hip_build_denoise_resources", "lupin_hip_destroy_denoise_resources", "lupin_hip_denoise")


def test_denoise_symbols_exported(built):
    handle = C.CDLL(_abi.LIB_PATH)
    bound = {n for n, _, _ in _abi.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    for n in SYMS:
        assert hasattr(handle, n), n
        assert n in bound, n
        assert n + "(" in header, n


def test_denoise_quality_default_is_high():
    # denoising.rs:208-218: #[default] High
    assert api.DenoiseQuality.default() == api.DenoiseQuality.High
    assert [int(q) for q in api.DenoiseQuality] == [0, 1, 2]
    assert api.DenoiseDesc(pathtrace_output=None, denoise_output=None).quality == api.DenoiseQuality.High
    d = api.DenoiseDesc(None, None)
    assert d.albedo is None and d.normals is None


def test_denoise_desc_layout_matches_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lupin_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(LupinDenoiseDesc),'
                   ' offsetof(LupinDenoiseDesc, pathtrace_output), offsetof(LupinDenoiseDesc, albedo), offsetof(LupinDenoiseDesc, normals),'
                   ' offsetof(LupinDenoiseDesc, denoise_output), offsetof(LupinDenoiseDesc, quality),'
                   ' LUPIN_DENOISE_LOW, LUPIN_DENOISE_MEDIUM, LUPIN_DENOISE_HIGH); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    D = _abi.DenoiseDescC
    assert got[:6] == [C.sizeof(D), D.pathtrace_output.offset, D.albedo.offset, D.normals.offset, D.denoise_output.offset, D.quality.offset]
    assert got[6:] == [int(api.DenoiseQuality.Low), int(api.DenoiseQuality.Medium), int(api.DenoiseQuality.High)]


def _rgba(rgb, alpha=1.0):
    h, w = rgb.shape[:2]
    return np.concatenate([rgb, np.full((h, w, 1), alpha, np.float32)], -1).astype(np.float16)


@pytest.mark.parametrize("guides", ["none", "albedo", "normals", "both"])
def test_restatement_keeps_constant_image(guides):
    H, W = 13, 21
    col = _rgba(np.broadcast_to(np.float32([0.75, 0.5, 0.25]), (H, W, 3)).copy(), 0.5)
    alb = _rgba(np.broadcast_to(np.float32([0.5, 0.25, 0.8]), (H, W, 3)).copy()) if guides in ("albedo", "both") else None
    nrm = _rgba(np.broadcast_to(np.float32([0.0, 0.6, 0.8]), (H, W, 3)).copy(), 0.0) if guides in ("normals", "both") else None
    for q in (0, 1, 2):
        rgb = R.denoise(col, alb, nrm, q, raw=True)
        ref = col[..., :3].astype(np.float32)
        assert np.all(np.abs(rgb - ref) <= np.spacing(ref)), (guides, q, np.abs(rgb - ref).max())
        out = R.denoise(col, alb, nrm, q)
        assert np.array_equal(out.view(np.uint16), col.view(np.uint16))


def _two_planes(H=32, W=64, noise=0.3, seed=3):
    rng = np.random.default_rng(seed)
    base = np.where(np.arange(W) < W // 2, 0.2, 2.0).astype(np.float32)[None, :, None]
    rgb = np.maximum(base * (1 + noise * rng.standard_normal((H, W, 1)).astype(np.float32)), 0).astype(np.float32)
    nrm = np.zeros((H, W, 3), np.float32)
    nrm[:, :W // 2, 2] = 1.0
    nrm[:, W // 2:, 0] = 1.0
    return _rgba(np.repeat(rgb, 3, -1)), _rgba(nrm, 0.0)


def test_restatement_stops_at_normal_edges():
    col, nrm = _two_planes()
    W = col.shape[1]
    x = W // 2 - 1   # the dark plane's column next to the edge
    with_n = R.denoise(col, None, nrm, 2).astype(np.float32)[:, x, :3].mean()
    without = R.denoise(col, None, None, 2).astype(np.float32)[:, x, :3].mean()
    assert abs(with_n / 0.2 - 1) <= 0.05, with_n
    # without the normals the bright plane leaks into the column: the test sees the edge
    assert abs(without / 0.2 - 1) > 4 * abs(with_n / 0.2 - 1) + 0.1, (with_n, without)


def test_restatement_cuts_noise_on_flat_patch():
    rng = np.random.default_rng(11)
    H, W = 48, 48
    lum = np.maximum(0.5 * (1 + 0.5 * rng.standard_normal((H, W, 1))), 0).astype(np.float32)
    col = _rgba(np.repeat(lum, 3, -1))
    before = col[..., :3].astype(np.float32).var()
    ratios = [before / R.denoise(col, None, None, q).astype(np.float32)[..., :3].var() for q in (0, 1, 2)]
    assert ratios[0] > 10 and ratios[2] > ratios[0], ratios
    assert abs(R.denoise(col, None, None, 2).astype(np.float32)[..., :3].mean() / col[..., :3].astype(np.float32).mean() - 1) < 0.02


def test_restatement_maps_non_finite_to_zero_and_copies_alpha():
    rng = np.random.default_rng(5)
    col = _rgba(rng.random((9, 11, 3), dtype=np.float32), 0.25)
    col[4, 5, 0] = np.nan
    col[2, 3, 1] = np.inf
    out = R.denoise(col, None, None, 2)
    assert np.all(np.isfinite(out.astype(np.float32)))
    assert np.array_equal(out[..., 3].view(np.uint16), col[..., 3].view(np.uint16))


def test_exp_of_the_filter_is_accurate():
    x = np.concatenate([-np.linspace(0, 79.999, 400001, dtype=np.float32), np.float32([-0.0, -1e-30, -79.99])])
    got = R.exp_neg(x).astype(np.float64)
    ref = np.exp(x.astype(np.float64))
    assert np.all(np.abs(got - ref) <= 4 * np.spacing(ref.astype(np.float32)).astype(np.float64))
    assert R.exp_neg(np.float32([-80.0, -1e30, -np.inf])).tolist() == [0.0, 0.0, 0.0]


def test_float32_restatement_agrees_with_float64():
    rng = np.random.default_rng(9)
    H, W = 17, 23
    col = _rgba(rng.random((H, W, 3), dtype=np.float32) * 3)
    alb = _rgba(rng.random((H, W, 3), dtype=np.float32))
    nrm = _rgba(rng.standard_normal((H, W, 3)).astype(np.float32), 0.0)
    for q in (0, 2):
        a = R.denoise(col, alb, nrm, q).astype(np.float32)
        b = R.denoise64(col, alb, nrm, q).astype(np.float32)
        assert np.all(np.abs(a - b) <= 2 * np.spacing(np.abs(b).astype(np.float16)).astype(np.float32) + 1e-6)


def test_denoise_without_device_raises_not_falls_back(built):
    """The Python surface never filters on the CPU: without a device context it raises."""
    with pytest.raises(api.LupinError) as e:
        api.build_denoise_resources(None, 8, 8)
    assert e.value.code == -2   # LUPIN_ERR_NO_DEVICE
    with pytest.raises(api.LupinError):
        api.denoise(None, None, api.DenoiseDesc(None, None))
    if api.device_count() < 1:
        with pytest.raises(api.LupinError):
            api.Context(0)
