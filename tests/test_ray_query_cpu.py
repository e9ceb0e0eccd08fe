"""Radiance queries (lupin_hip_pathtrace_rays), the parts that need no device: the symbol and the layouts of
its mirrors, the numpy restatement of the device's seeding, the record packer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from lupinpathtracer_amd import _abi, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pcg_step(state):
    """rnd() of the device (lupin_device.hpp) on uint32 arrays: (next state, the f32 in [0, 1])."""
    with np.errstate(over="ignore"):
        s = state.astype(np.uint32) * np.uint32(747796405) + np.uint32(2891336453)
        r = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)
        r = (r >> np.uint32(22)) ^ r
    return s, r.astype(np.float32) / np.float32(4294967295.0)


def test_symbol_resolves_and_desc_sizes_agree(built):
    lib = _abi.lib()
    assert hasattr(lib, "lupin_hip_pathtrace_rays")
    header = open(os.path.join(ROOT, "include", "lupin_hip.h")).read()
    body = re.search(r"typedef struct LupinRayQueryDesc \{(.*?)\} LupinRayQueryDesc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_size = {"uint32_t": 4, "LupinAdvancedParams": C.sizeof(_abi.AdvancedParamsC)}
    c_fields = re.findall(r"(\w+)\s+(\w+);", body)
    assert [n for _, n in c_fields] == [n for n, _ in _abi.RayQueryDescC._fields_]
    want = sum(c_size[t] for t, _ in c_fields)
    assert want == 32 and C.sizeof(_abi.RayQueryDescC) == want
    assert _abi.RayQueryDescC.advanced.offset == 20
    rust = open(os.path.join(ROOT, "integration", "rust", "lupin_hip", "src", "ffi.rs")).read()
    rbody = re.search(r"pub struct LupinRayQueryDesc \{(.*?)\}", rust, re.S).group(1)
    r_size = {"u32": 4, "LupinAdvancedParams": 12}
    r_fields = re.findall(r"pub (\w+): (\w+)", rbody)
    assert [n for n, _ in r_fields] == [n for _, n in c_fields]
    assert sum(r_size[t] for _, t in r_fields) == want
    assert "pub fn lupin_hip_pathtrace_rays(" in rust
    assert (api.RAY_RECORD_FLOATS, api.RAY_RESULT_FLOATS, api.RAYS_DEVICE_POINTERS) == (8, 4, 1)
    assert (int(api.RayMode.DIRECTION), int(api.RayMode.COSINE_HEMISPHERE)) == (0, 1)
    # one default chunk size: the header's macro, which the library and the Python mirror use
    assert int(re.search(r"#define LUPIN_RAYS_DEFAULT_MAX_SLOTS (\d+)u", header).group(1)) == api.RAYS_DEFAULT_MAX_SLOTS
    host = open(os.path.join(ROOT, "lupinpathtracer_amd", "csrc", "lupin_hip.hip")).read()
    assert "LP_RAYS_DEFAULT_SLOTS = LUPIN_RAYS_DEFAULT_MAX_SLOTS;" in host
    for must in ("LUPIN_RAY_DIRECTION = 0", "LUPIN_RAY_COSINE_HEMISPHERE = 1", "LUPIN_RAYS_DEVICE_POINTERS = 1u"):
        assert must in header


def test_without_a_device_the_call_says_so(built):
    rec = api.ray_records([[0, 0, 0]], [[0, 0, 1]])
    out = np.full((1, 4), 7.0, np.float32)
    desc = _abi.RayQueryDescC(0, 8, 1, 0, 0, _abi.AdvancedParamsC(100.0, 0, 0.001))
    rc = _abi.lib().lupin_hip_pathtrace_rays(None, None, C.byref(desc), 1, _abi.ptr(rec), _abi.ptr(out), None)
    # LUPIN_ERR_NO_DEVICE; where there is a device, a null context is an invalid argument
    assert rc == (-2 if api.device_count() < 1 else -1)
    assert np.all(out == 7.0)
    from lupinpathtracer_amd import loader
    scene, _ = loader.build_scene_cornell_box(None)
    for call in (lambda: api.pathtrace_rays(None, scene, rec), lambda: api.bake_irradiance(None, scene, [[0, 0, 0]], [[0, 0, 1]], 4)):
        with pytest.raises(api.LupinError) as e:
            call()
        assert e.value.code == -2


def test_rng_seed_for_and_the_pcg_step_reproduce_the_oracle_stream(built):
    from oracle import oracle
    rng = np.random.default_rng(5)
    index = np.concatenate([[0, 1, 2, 64 * 48 - 1, 0xFFFFFFFF], rng.integers(0, 2 ** 32, 295, dtype=np.uint64)]).astype(np.uint32)
    counter = np.concatenate([[0, 0, 1, 7, 0xFFFFFFFF], rng.integers(0, 2 ** 32, 295, dtype=np.uint64)]).astype(np.uint32)
    state = api.rng_seed_for(index, counter)
    assert state.dtype == np.uint32 and state.shape == (300,)
    assert int(api.rng_seed_for(5, 3)) == int(api.rng_seed_for(np.uint32([5]), np.uint32([3]))[0])
    draws = []
    for _ in range(6):
        state, u = pcg_step(state)
        draws.append(u)
    mine = np.stack(draws, axis=1)
    for k in range(len(index)):
        want = oracle.rng_stream(int(index[k]), int(counter[k]), 6)
        assert np.array_equal(mine[k].view(np.uint32), want.view(np.uint32)), (k, index[k], counter[k])


def test_sample_seeds_follow_the_stated_recurrence():
    word = np.uint32([0, 1, 0xDEADBEEF, 0xFFFFFFFF])
    assert np.array_equal(api.ray_sample_seed(word, 0), word)

    def hash_u32(x):
        x &= 0xFFFFFFFF
        x ^= x >> 17; x = (x * 0xed5ad4bb) & 0xFFFFFFFF
        x ^= x >> 11; x = (x * 0xac4c1b51) & 0xFFFFFFFF
        x ^= x >> 15; x = (x * 0x31848bab) & 0xFFFFFFFF
        x ^= x >> 14
        return x
    for s in (1, 2, 5, 4095):
        want = [hash_u32((int(w) + s * 0x9E3779B9) & 0xFFFFFFFF) for w in word]
        assert api.ray_sample_seed(word, s).tolist() == want


def test_ray_records_pack_what_the_header_says():
    ori = np.float32([[1, 2, 3], [4, 5, 6]])
    d = np.float32([[0, 0, 1], [0, 1, 0]])
    rec = api.ray_records(ori, d, np.uint32([0x3F800000, 0xFFFFFFFF]), api.RayMode.COSINE_HEMISPHERE)
    assert rec.dtype == np.float32 and rec.shape == (2, 8) and rec.flags["C_CONTIGUOUS"] and rec.nbytes == 64
    assert np.array_equal(rec[:, 0:3], ori) and np.array_equal(rec[:, 4:7], d)
    bits = rec.view(np.uint32)
    assert bits[:, 3].tolist() == [0x3F800000, 0xFFFFFFFF]       # the RNG word's bits survive, also those of a NaN pattern
    assert bits[:, 7].tolist() == [1, 1]
    rec = api.ray_records(ori, d)                                  # defaults: RNG word 0, mode DIRECTION
    assert rec.view(np.uint32)[:, 3].tolist() == [0, 0] and rec.view(np.uint32)[:, 7].tolist() == [0, 0]
    rec = api.ray_records(ori, d, 9, np.uint32([0, 1]))            # per-record modes
    assert rec.view(np.uint32)[:, 7].tolist() == [0, 1] and rec.view(np.uint32)[:, 3].tolist() == [9, 9]
    d0 = api.RayQueryDesc()
    assert (int(d0.pathtrace_type), d0.max_bounces, d0.samples, d0.flags, d0.max_slots) == (0, 8, 1, 0, 0)
    assert (d0.advanced.max_radiance, d0.advanced.ray_epsilon) == (100.0, 0.001)
