#!/usr/bin/env python3
"""What moving the instances of a bistro_class scene costs: one JSON line per instance count with
  cpu_build_ms            lupin_build_tlas on the host
  device_kernel_ms        the clustering kernel of lupin_hip_build_tlas_device, between two events
  device_kernel_global_ms the same kernel with its state in global memory instead of LDS (LUPIN_TLAS_LDS_SLOTS=0)
  device_call_ms          the whole call: leaf boxes, upload, kernel, download, reversal
  update_cpu_ms / update_device_ms   Scene.update_instances wall time per builder
  recreate_ms             scene_destroy + lupin_build_tlas + lupin_hip_scene_create of the same change (BLASes reused)
each as [min, median, max] over --repeats runs in this process.  Run it several times for fresh-process spread.

    python tools/scene_update_bench.py --sizes 400 2000 8000 --repeats 3
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(xs):
    return [round(min(xs), 4), round(statistics.median(xs), 4), round(max(xs), 4)]


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[400, 2000, 8000])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cpu-repeats-above", type=int, default=4000, help="instance count from which the CPU builder legs run once")
    args = ap.parse_args()
    import numpy as np
    from lupinpathtracer_amd import api, loader
    from lupinpathtracer_amd._abi import check, lib, ptr
    from tests import util
    if api.device_count() < 1:
        raise SystemExit("scene_update_bench needs a HIP device")
    ctx = api.Context(0)
    for n in args.sizes:
        scene_cpu, textures, envs, cams = loader.build_scene_bistro_class_cpu(util.SHARED, n_instances=n)
        t = time.perf_counter()
        scene = api.build_accel_structures_and_upload(ctx, scene_cpu, textures, envs, True)
        first_create_s = time.perf_counter() - t
        n_inst = len(scene.instances)
        rng = np.random.default_rng(n)
        base = scene.instances["transpose_inverse_transform"].copy()

        def moved(k):
            rows = base.copy()
            rows[:, :, 3] += rng.uniform(-0.05, 0.05, size=(n_inst, 3)).astype(np.float32) * (k + 1)   # world -> local offsets
            return rows
        inst = scene.instances.copy()
        inst["transpose_inverse_transform"] = moved(0)
        cpu_reps = 1 if n_inst >= args.cpu_repeats_above else args.repeats
        api.build_tlas_device(ctx, inst, scene.model_aabbs)            # warm-up: code object load
        rec = {"scene": "bistro_class", "instances": n_inst, "first_create_s": round(first_create_s, 2), "repeats": args.repeats, "cpu_repeats": cpu_reps}
        rec["cpu_build_ms"] = spread(timed(lambda: api.build_tlas(inst, scene.model_aabbs), cpu_reps))
        kernel, call = [], []
        for _ in range(args.repeats):
            call += timed(lambda: api.build_tlas_device(ctx, inst, scene.model_aabbs), 1)
            st = api.tlas_build_stats()
            kernel.append(st["kernel_ms"])
        rec["device_kernel_ms"], rec["device_call_ms"] = spread(kernel), spread(call)
        rec["scans"], rec["state_in_lds"] = st["scans"], st["state_in_lds"]
        os.environ["LUPIN_TLAS_LDS_SLOTS"] = "0"
        kernel = []
        for _ in range(args.repeats):
            api.build_tlas_device(ctx, inst, scene.model_aabbs)
            kernel.append(api.tlas_build_stats()["kernel_ms"])
        del os.environ["LUPIN_TLAS_LDS_SLOTS"]
        rec["device_kernel_global_ms"] = spread(kernel)
        k = [0]

        def update(builder):
            k[0] += 1
            scene.update_instances(moved(k[0]), tlas_builder=builder)
        update("device")
        rec["update_device_ms"] = spread(timed(lambda: update("device"), args.repeats))
        rec["update_cpu_ms"] = spread(timed(lambda: update("cpu"), cpu_reps))

        def recreate():
            k[0] += 1
            new = scene.instances.copy()
            new["transpose_inverse_transform"] = moved(k[0])
            lib().lupin_hip_scene_destroy(scene.handle)
            tlas = api.build_tlas(new, scene.model_aabbs)
            scene._keep += [new, tlas]
            scene.desc.instances, scene.desc.tlas_nodes, scene.desc.num_tlas_nodes = ptr(new), ptr(tlas), len(tlas)
            h = C.c_void_p()
            check(lib().lupin_hip_scene_create(ctx.handle, C.byref(scene.desc), C.byref(h)))
            scene.handle, scene.instances, scene.tlas = h, new, tlas
        rec["recreate_ms"] = spread(timed(recreate, cpu_reps))
        print(json.dumps(rec), flush=True)
        del scene


if __name__ == "__main__":
    main()
