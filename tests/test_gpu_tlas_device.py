"""The device TLAS builder (csrc/tlas.hip) against lupin_build_tlas: the same tree node for node.
Every case launches the builder once."""
import os

import numpy as np
import pytest

from lupinpathtracer_amd import api, loader
from tests import tlas_ref, util

pytestmark = pytest.mark.gpu

LDS_SLOTS = 5800   # kLdsSlots of csrc/tlas.hip: above it the builder's state lives in global memory


def bistro_set(n_instances):
    kw = dict(n_meshes=3, n_instances=n_instances, n_lights=min(12, n_instances), n_materials=24)
    scene_cpu, textures, envs, _ = loader.build_scene_bistro_class_cpu(util.SHARED, **kw)
    scene = api.build_accel_structures_and_upload(None, scene_cpu, textures, envs)
    return scene.instances, scene.model_aabbs


CASES = {
    "bistro_40": lambda: bistro_set(40),
    "bistro_400": lambda: bistro_set(400),
    "bistro_2000": lambda: bistro_set(2000),
    "tie_grid": lambda: tlas_ref.grid_set(6),
    "n1": lambda: tlas_ref.random_set(1, 21),
    "n2": lambda: tlas_ref.random_set(2, 22),
    "n3": lambda: tlas_ref.random_set(3, 23),
    "n1025": lambda: tlas_ref.random_set(1025, 24),
    "line_300": lambda: tlas_ref.line_set(300),
    "above_lds_6000": lambda: tlas_ref.random_set(6000, 25),
}


@pytest.mark.parametrize("case", list(CASES))
def test_device_builder_equals_cpu_builder(gpu_ctx, case):
    inst, aabbs = CASES[case]()
    n = len(inst)
    want = api.build_tlas(inst, aabbs)
    got = api.build_tlas_device(gpu_ctx, inst, aabbs)
    st = api.tlas_build_stats()
    print(f"{case}: {n} instances, {st}")
    assert len(got) == len(want) == 2 * n
    assert np.array_equal(got["left"], want["left"]) and np.array_equal(got["right"], want["right"])
    assert np.array_equal(got["instance_idx"], want["instance_idx"])
    assert np.array_equal(got["aabb_min"], want["aabb_min"]) and np.array_equal(got["aabb_max"], want["aabb_max"])   # as float values
    assert st["num_instances"] == n and st["state_in_lds"] == (n <= LDS_SLOTS)
    assert st["scans"] < n * n + 4 * n
    if n <= 2000:
        # the restatement makes the same scans plus the CPU code's last one, which has no candidate left
        _, scans = tlas_ref.cluster(*tlas_ref.leaves_of(want, n))
        assert st["scans"] == scans - 1


def test_scene_built_with_the_device_tlas_is_the_same_scene(gpu_ctx):
    scene_cpu, textures, envs, cams = loader.build_scene_bistro_class_cpu(util.SHARED, n_meshes=3, n_instances=40, n_lights=12, n_materials=24)
    a = api.build_accel_structures_and_upload(gpu_ctx, scene_cpu, textures, envs, tlas_builder="cpu")
    b = api.build_accel_structures_and_upload(gpu_ctx, scene_cpu, textures, envs, tlas_builder="device")
    assert tlas_ref.same_tree(a.tlas, b.tlas)
    W, H = 96, 56
    assert util.f16_words_differ(util.gpu_accumulate(gpu_ctx, a, cams[0], W, H, frames=1, spp=2),
                                 util.gpu_accumulate(gpu_ctx, b, cams[0], W, H, frames=1, spp=2)) == 0


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_non_finite_transform_is_rejected_before_the_launch(gpu_ctx, bad):
    inst, aabbs = tlas_ref.random_set(16, 30)
    api.build_tlas_device(gpu_ctx, inst, aabbs)
    before = api.tlas_build_stats()
    inst["transpose_inverse_transform"][5, 1, 2] = bad
    with pytest.raises(api.LupinError) as e:
        api.build_tlas_device(gpu_ctx, inst, aabbs)
    assert e.value.code == -1 and "non-finite" in str(e.value)
    assert api.tlas_build_stats() == before   # nothing ran


def test_bad_mesh_index_is_rejected(gpu_ctx):
    inst, aabbs = tlas_ref.random_set(16, 31)
    inst["mesh_idx"][3] = 99
    with pytest.raises(api.LupinError) as e:
        api.build_tlas_device(gpu_ctx, inst, aabbs)
    assert e.value.code == -1
