"""Time the baked-lighting view (lupin_hip_render_baked) against the two calls it is composed of.

usage: python tools/baked_view_bench.py [--scene bistro_class] [--sizes 3840x2160,1920x1080] [--dims 16x16x4] [--resolution 16]
                                        [--subsamples 4] [--runs 5] [--warmup 2] [--out profiles/baked_view_bench.jsonl]
The grid is tools/probe_depth_bench.py's: `dims` probes over the box of 2^20 surface points seen from the scene's camera, with
baked depth maps and random coefficients; coefficients, maps and every result are in device memory.  Per image size, the view
with the untraced lookup, with depth maps and with traced visibility.  Every figure is the median (min - max) of `runs`
host-clock times of one call that ends synchronised, after `warmup` calls.  The yardsticks, in the same process:
lupin_hip_pathtrace_scene_falsecolor (albedo, 1 sample a pixel) for the primary hit, and lupin_hip_sample_probe_grid_depth
over W * H device records (the view's own G-buffer records; a miss is a record at the origin) for the lookup.  The view's
time is reported as a ratio to their sum, and the bytes of scratch memory the three-kernel staging writes and reads again.
Prints one JSON line per size and appends it to --out.  Needs a HIP device; there is no CPU fallback.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCRATCH_BYTES_PER_PIXEL = 2 * (32 + 32 + 16)   # record, compose record and lookup result: each written once and read once


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bistro_class")
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--dims", default="16x16x4")
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--subsamples", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "baked_view_bench.jsonl"))
    args = ap.parse_args()

    from lupinpathtracer_amd import _abi, api
    from oracle import oracle
    from tests import reproject_ref, util
    from tools.occlusion_bench import surface_points
    from tools.probe_grid_bench import device_array

    if api.device_count() < 1:
        raise SystemExit("baked_view_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    scene, cams = util.load_scene(args.scene, ctx)
    cam = cams[0]
    eps, R, K = 0.001, args.resolution, args.subsamples
    dims = tuple(int(x) for x in args.dims.split("x"))
    extent = float(api.scene_world_extent(scene))
    bias = np.float32(api.LIGHTMAP_OFFSET_FRACTION * extent)
    points, _ = surface_points(api, oracle, reproject_ref, ctx, scene, cam, 1 << 20)
    lo, hi = points.min(0), points.max(0)
    origin = lo.astype(np.float32)
    spacing = np.float32([max((hi[k] - lo[k]) / max(1, dims[k] - 1), 1e-3 * extent) for k in range(3)])
    P = int(np.prod(dims))
    sh = np.random.default_rng(0).normal(size=(P, 9, 4)).astype(np.float32)
    _, maps, maxd = api.bake_probe_grid_depth(ctx, scene, origin, spacing, dims, R, K)
    d_sh, d_maps = device_array(api, ctx, sh), device_array(api, ctx, maps)
    lib = _abi.lib()
    res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(max_bounces=1, samples_per_pixel=1))

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        ms = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    def report(ms, items):
        med = statistics.median(ms)
        return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "mitems_per_s": round(items / med / 1e3, 2)}

    def grid_desc(flags):
        return _abi.ProbeGridDescC((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_uint32 * 3)(*dims), flags, eps, float(bias))

    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        n = W * H
        target = api.Texture(ctx, W, H)
        row = {"tool": "baked_view_bench", "scene": args.scene, "width": W, "height": H, "dims": list(dims), "resolution": R, "subsamples": K,
               "max_distance": float(maxd), "normal_bias": float(bias), "ray_epsilon": eps, "runs": args.runs, "warmup": args.warmup,
               "max_slots": api.BAKED_VIEW_DEFAULT_MAX_SLOTS, "scratch_bytes_per_pixel": SCRATCH_BYTES_PER_PIXEL, "scratch_mb": round(n * SCRATCH_BYTES_PER_PIXEL / 1e6, 1)}

        def view(grid_flags, depth, gbuffer=None):
            d = _abi.BakedViewDescC()
            cp = cam.params
            d.camera_params = _abi.CameraParamsC(1 if cp.is_orthographic else 0, cp.lens, cp.film, cp.aspect, cp.focus, cp.aperture)
            m = np.asarray(cam.transform, np.float32).reshape(4, 3)
            for col in range(4):
                for r in range(3):
                    d.camera_transform.m[col][r] = float(m[col][r])
            d.grid = grid_desc(grid_flags)
            d.resolution, d.max_distance, d.ray_epsilon, d.flags, d.max_slots = R, float(maxd), eps, api.BAKED_VIEW_DEVICE_POINTERS, 0
            d.ambient = (C.c_float * 3)(0.05, 0.05, 0.05)
            return lambda: _abi.check(lib.lupin_hip_render_baked(ctx.handle, scene.handle, target.handle, C.byref(d), C.c_void_p(d_sh.device_ptr()),
                                                                 C.c_void_p(d_maps.device_ptr()) if depth else None, None,
                                                                 C.c_void_p(gbuffer.device_ptr()) if gbuffer is not None else None))

        bf = api.PROBE_GRID_BACKFACE
        row["view_plain"] = report(timed(view(bf, False)), n)
        row["view_depth"] = report(timed(view(bf, True)), n)
        row["view_visibility"] = report(timed(view(bf | api.PROBE_GRID_VISIBILITY, False)), n)

        # the yardsticks: the primary hit ...
        desc = api.PathtraceDesc(camera_params=cam.params, camera_transform=cam.transform)
        row["falsecolor_albedo_1spp"] = report(timed(lambda: api.pathtrace_scene_falsecolor(ctx, res, scene, target, 0, desc)), n)
        # ... and the lookup over the view's own records
        d_g = api.Texture(ctx, 4, (n * 64 + 31) // 32)
        view(bf, True, d_g)()
        g = d_g.download().view(np.uint8).reshape(-1)[:n * 64].view(np.float32).reshape(n, 16)
        hit = g[:, 3].view(np.uint32) != api.BAKED_VIEW_MISS
        rec = np.zeros((n, 8), np.float32)
        rec[:, 6] = 1.0
        rec[hit] = g[hit, 0:8]
        row.update(hit_pixels=int(hit.sum()), unanswered_pixels=int((hit & (g[:, 11] == 0)).sum()))
        del d_g, g
        d_rec = device_array(api, ctx, rec)
        d_out = api.Texture(ctx, 4, (n * 16 + 31) // 32)
        dd = _abi.ProbeGridDepthDescC(grid_desc(bf | api.PROBE_GRID_DEVICE_POINTERS), R, float(maxd))
        row["lookup_depth_records"] = report(timed(lambda: _abi.check(lib.lupin_hip_sample_probe_grid_depth(
            ctx.handle, scene.handle, C.byref(dd), C.c_void_p(d_sh.device_ptr()), C.c_void_p(d_maps.device_ptr()), None, n, C.c_void_p(d_rec.device_ptr()),
            C.c_void_p(d_out.device_ptr())))), n)
        parts = row["falsecolor_albedo_1spp"]["median_ms"] + row["lookup_depth_records"]["median_ms"]
        row["yardstick_sum_ms"] = round(parts, 3)
        row["view_depth_over_yardsticks"] = round(row["view_depth"]["median_ms"] / parts, 4)
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del d_rec, d_out, target
    ctx.close()


if __name__ == "__main__":
    main()
