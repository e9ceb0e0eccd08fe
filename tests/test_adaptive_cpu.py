"""Adaptive sampling without a device: the C ABI surface, the Python / Rust declarations and the properties of the numpy
restatement of the update rule (tests/adaptive_ref.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api
from tests import adaptive_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMS = ("lupin_hip_build_adaptive_resources", "lupin_hip_destroy_adaptive_resources", "lupin_hip_adaptive_reset",
        "lupin_hip_pathtrace_scene_adaptive", "lupin_hip_adaptive_stats", "lupin_hip_adaptive_download")


def test_adaptive_symbols_exported(built):
    handle = C.CDLL(_abi.LIB_PATH)
    bound = {n for n, _, _ in _abi.SYMBOLS}
    header = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    for n in SYMS:
        assert hasattr(handle, n), n
        assert n in bound, n
        assert n + "(" in header, n


def test_adaptive_structs_match_header(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "lupin_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n",'
                   ' sizeof(LupinAdaptiveParams), offsetof(LupinAdaptiveParams, threshold), offsetof(LupinAdaptiveParams, min_frames),'
                   ' offsetof(LupinAdaptiveParams, max_frames), sizeof(LupinAdaptiveStats), offsetof(LupinAdaptiveStats, active_pixels),'
                   ' offsetof(LupinAdaptiveStats, pixel_frames), offsetof(LupinAdaptiveStats, calls),'
                   ' offsetof(LupinAdaptiveStats, max_frames_taken)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    P, S = _abi.AdaptiveParamsC, _abi.AdaptiveStatsC
    assert got == [C.sizeof(P), P.threshold.offset, P.min_frames.offset, P.max_frames.offset,
                   C.sizeof(S), S.active_pixels.offset, S.pixel_frames.offset, S.calls.offset, S.max_frames_taken.offset]
    assert got[0] == 12 and got[4] == 24


def test_rust_shim_adaptive_structs():
    src = open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    fns = set(re.findall(r"pub fn (lupin_\w+)\(", src))
    assert set(SYMS) <= fns
    size = {"u32": 4, "f32": 4, "u64": 8}
    for name, ctype in (("LupinAdaptiveParams", _abi.AdaptiveParamsC), ("LupinAdaptiveStats", _abi.AdaptiveStatsC)):
        body = re.search(r"pub struct %s \{(.*?)\}" % name, src, re.S).group(1)
        fields = re.findall(r"pub (\w+): (\w+)", body)
        assert [n for n, _ in fields] == [n for n, _ in ctype._fields_], name
        assert sum(size[t] for _, t in fields) == C.sizeof(ctype), name


def test_adaptive_params_defaults():
    p = api.AdaptiveParams()
    assert (p.threshold, p.min_frames, p.max_frames) == (0.01, 8, 0)


def test_welford_matches_two_pass_variance():
    rng = np.random.default_rng(1)
    vals = rng.gamma(0.7, 2.0, size=(40, 7, 9)).astype(np.float32)
    for n in (1, 2, 5, 40):
        cnt, mean, m2 = R.welford(vals[:n])
        v64 = vals[:n].astype(np.float64)
        assert cnt == n
        np.testing.assert_allclose(mean, v64.mean(0), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(m2, ((v64 - v64.mean(0)) ** 2).sum(0), rtol=2e-5, atol=1e-5)
        assert (m2 >= 0).all()


def _state(h, w, n, value=0.5, noise=0.0, seed=0):
    rng = np.random.default_rng(seed)
    vals = np.float32(value) + np.float32(noise) * rng.standard_normal((n, h, w)).astype(np.float32)
    cnt, mean, m2 = R.welford(np.maximum(vals, 0))
    return np.full((h, w), cnt, np.uint32), mean, m2


def test_error_is_infinite_without_two_frames_or_with_bad_moments():
    e = R.pixel_error(np.array([0, 1, 2, 2, 2]), np.float32([0, 0.5, 0.5, np.nan, 0.5]), np.float32([0, 0, 0.02, 0, np.inf]))
    assert np.isinf(e[:2]).all() and np.isfinite(e[2]) and np.isinf(e[3:]).all()
    # relative standard error of the mean: sqrt(0.02 / 2) / (0.5 + 1e-3)
    assert e[2] == np.float32(np.sqrt(np.float32(0.02) / np.float32(2.0)) / (np.float32(0.5) + np.float32(1e-3)))


def test_threshold_zero_keeps_every_block_active():
    frames, mean, m2 = _state(40, 48, 12)   # zero variance: e_p = 0 everywhere
    e, act = R.update(frames, mean, m2, threshold=0.0, min_frames=0)
    assert (e == 0).all() and act.all()


def test_zero_variance_block_stops_unless_a_neighbour_is_open():
    H, W = 48, 64   # 6 x 8 blocks
    frames, mean, m2 = _state(H, W, 8)
    e, act = R.update(frames, mean, m2, threshold=0.01, min_frames=8)
    assert not act.any()
    # fewer frames than min_frames: nothing stops
    _, act = R.update(frames, mean, m2, threshold=0.01, min_frames=9)
    assert act.all()
    # one noisy pixel in block (2, 3): that block and its 8 neighbours stay active, nothing else
    _, nmean, nm2 = _state(H, W, 8, noise=0.3, seed=3)
    mean2, m22 = mean.copy(), m2.copy()
    mean2[2 * 8 + 5, 3 * 8 + 1], m22[2 * 8 + 5, 3 * 8 + 1] = nmean[0, 0], nm2[0, 0]
    e, act = R.update(frames, mean2, m22, threshold=0.01, min_frames=8)
    want = np.zeros((6, 8), bool)
    want[1:4, 2:5] = True
    assert e[2, 3] > 0.01 and (np.delete(e.ravel(), 2 * 8 + 3) == 0).all()
    assert (act == want).all()


def test_edge_blocks_use_only_in_image_pixels():
    H, W = 61, 97   # 8 x 13 blocks; the last row / column of blocks is partial (5 rows, 1 column)
    frames, mean, m2 = _state(H, W, 10, noise=0.2, seed=5)
    e = R.block_error(frames, mean, m2)
    assert e.shape == (8, 13)
    pe = R.pixel_error(frames, mean, m2)
    for by in range(8):
        for bx in range(13):
            assert e[by, bx] == pe[by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].max()
    assert (R.block_pixels(W, H)[-1, :-1] == 40).all() and R.block_pixels(W, H)[-1, -1] == 5 and R.block_pixels(W, H)[0, -1] == 8
    # pixels outside the image must not matter: garbage beyond the edge changes nothing
    big = _state(64, 104, 10, noise=0.2, seed=5)
    bf, bm, bm2 = (a.copy() for a in big)
    bf[:H, :W], bm[:H, :W], bm2[:H, :W] = frames, mean, m2
    assert (R.block_error(bf[:H, :W], bm[:H, :W], bm2[:H, :W]) == e).all()
    # a converged interior with an unconverged partial edge column: the edge column and its neighbours stay open
    f2, mm, mm2 = _state(H, W, 10)
    mm2[:, 96] = np.float32(5.0)
    _, act = R.update(f2, mm, mm2, threshold=0.01, min_frames=4)
    assert act[:, 11:].all() and not act[:, :11].any()
    assert R.block_min_frames(np.where(np.arange(W)[None, :] < 96, 10, 3).astype(np.uint32) + np.zeros((H, 1), np.uint32))[0, -1] == 3


def test_max_frames_cap():
    frames, mean, m2 = _state(32, 32, 6, noise=0.4, seed=7)   # noisy: nothing converges
    _, act = R.update(frames, mean, m2, threshold=0.01, min_frames=2, max_frames=0)
    assert act.all()
    _, act = R.update(frames, mean, m2, threshold=0.01, min_frames=2, max_frames=7)
    assert act.all()
    _, act = R.update(frames, mean, m2, threshold=0.01, min_frames=2, max_frames=6)
    assert not act.any()
    # capped wins over an open neighbour; uncapped blocks next to capped ones are unaffected
    f2 = frames.copy()
    f2[:, :16] = 5
    _, act = R.update(f2, mean, m2, threshold=0.01, min_frames=2, max_frames=6)
    assert act[:, :2].all() and not act[:, 2:].any()
