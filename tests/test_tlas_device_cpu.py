"""TLAS building without a device: lupin_build_tlas after its leaf loop and tail were factored out equals the
recording made before, byte for byte; the numpy restatement of the clustering (tests/tlas_ref.py) equals lupin_build_tlas,
also where most comparisons tie; and the device entry points refuse to run without a device."""
import numpy as np
import pytest

from lupinpathtracer_amd import api
from tests import tlas_ref, util

def all_sets():
    sets = dict(tlas_ref.recorded_sets())
    sets["grid_6x6x6"] = tlas_ref.grid_set(6)
    sets["line_64"] = tlas_ref.line_set(64)
    for n in (1, 2, 3):
        sets[f"random_{n}"] = tlas_ref.random_set(n, 10 + n)
    return sets


def test_refactored_builder_equals_the_parent_recording(built):
    rec = np.load(tlas_ref.RECORDING)
    sets = tlas_ref.recorded_sets()
    assert sorted(rec.files) == sorted(sets)
    for name, (inst, aabbs) in sets.items():
        got = api.build_tlas(inst, aabbs)
        assert got.tobytes() == rec[name].tobytes(), name


def test_fixture_scenes_still_carry_the_recorded_tlas(built):
    rec = np.load(tlas_ref.RECORDING)
    for name in ("bistro_class_small", "instances1"):
        scene, _ = util.load_scene(name, None)
        assert scene.tlas.tobytes() == rec[name].tobytes(), name


def test_restatement_equals_the_cpu_builder_and_counts_scans(built):
    worst = 0.0
    for name, (inst, aabbs) in all_sets().items():
        want = api.build_tlas(inst, aabbs)
        n = len(inst)
        assert len(want) == 2 * n
        lo, hi = tlas_ref.leaves_of(want, n)
        got, scans = tlas_ref.cluster(lo, hi)
        assert tlas_ref.same_tree(got, want), name
        print(f"{name}: {n} instances, {scans} scans, {scans / n:.2f} per instance (cap {n + 4})")
        assert scans < n * n + 4 * n   # the device builder's cap: at most n + 1 scans per merge
        if n >= 8:
            worst = max(worst, scans / n)
    print(f"largest scans per instance: {worst:.2f}")   # recorded in DESIGN.md 11; the proven cap is n + 4 per instance


def test_tie_grid_really_ties(built):
    """The 6 x 6 x 6 grid is in the set because its first scan sees many equal areas: the lowest index must win."""
    inst, aabbs = tlas_ref.grid_set(6)
    lo, hi = tlas_ref.leaves_of(api.build_tlas(inst, aabbs), len(inst))
    e = np.maximum(hi[0], hi[1:]) - np.minimum(lo[0], lo[1:])
    area = e[:, 0] * e[:, 1] + e[:, 1] * e[:, 2] + e[:, 2] * e[:, 0]
    assert (area == area.min()).sum() >= 3


def test_device_entry_points_need_a_device(built):
    inst, aabbs = tlas_ref.random_set(8, 3)
    with pytest.raises(api.LupinError) as e:
        api.build_tlas_device(None, inst, aabbs)
    assert e.value.code == -2   # LUPIN_ERR_NO_DEVICE
    scene, _ = util.load_scene("instances1", None)
    with pytest.raises(api.LupinError) as e:
        scene.update_instances(scene.instances["transpose_inverse_transform"].copy())
    assert e.value.code == -2
    scene_cpu, textures, envs, _ = _instances1_cpu()
    with pytest.raises(api.LupinError) as e:
        api.build_accel_structures_and_upload(None, scene_cpu, textures, envs, tlas_builder="device")
    assert e.value.code == -2
    with pytest.raises(ValueError):
        api.build_accel_structures_and_upload(None, scene_cpu, textures, envs, tlas_builder="gpu")


def _instances1_cpu():
    import os
    from lupinpathtracer_amd import loader
    return loader.load_scene_cpu_yoctogl_v24(os.path.join(util.SCENES, "instances1", "instances1.json"), [util.SHARED])
