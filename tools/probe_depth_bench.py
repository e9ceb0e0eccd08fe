"""Time the probe depth bake (lupin_hip_bake_probe_depth) and the lookup that reads it (lupin_hip_sample_probe_grid_depth).

usage: python tools/probe_depth_bench.py [--scene bistro_class] [--points 1048576] [--dims 16x16x4] [--resolution 16]
                                         [--subsamples 4] [--runs 5] [--warmup 2] [--out profiles/probe_depth_bench.jsonl]
A `dims` grid over the box of `points` surface points (the first hits of a square frame's camera rays with their geometric
normals turned toward the camera: tools/occlusion_bench.py's); positions, maps, coefficients, records and results in device
memory.  Every figure is the median (min - max) of `runs` host-clock times of one call that ends synchronised, after `warmup`
calls.  The yardstick for the lookup, in the same process on the same records: lupin_hip_sample_probe_grid with and without
LUPIN_PROBE_GRID_VISIBILITY (the traversal the maps replace, and the lookup with no visibility at all).
Prints one JSON line and appends it to --out.  Needs a HIP device; there is no CPU fallback.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bistro_class")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--dims", default="16x16x4")
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--subsamples", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_depth_bench.jsonl"))
    args = ap.parse_args()

    from lupinpathtracer_amd import _abi, api
    from oracle import oracle
    from tests import reproject_ref, util
    from tools.occlusion_bench import surface_points
    from tools.probe_grid_bench import device_array

    if api.device_count() < 1:
        raise SystemExit("probe_depth_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    scene, cams = util.load_scene(args.scene, ctx)
    n, eps, R, K = args.points, 0.001, args.resolution, args.subsamples
    dims = tuple(int(x) for x in args.dims.split("x"))
    extent = float(api.scene_world_extent(scene))
    bias = np.float32(api.LIGHTMAP_OFFSET_FRACTION * extent)
    points, normals = surface_points(api, oracle, reproject_ref, ctx, scene, cams[0], n)
    lo, hi = points.min(0), points.max(0)
    origin = lo.astype(np.float32)
    spacing = np.float32([max((hi[k] - lo[k]) / max(1, dims[k] - 1), 1e-3 * extent) for k in range(3)])
    P = int(np.prod(dims))
    maxd = float(api.probe_grid_depth_max_distance(spacing))
    pos4 = np.zeros((P, 4), np.float32)
    pos4[:, :3] = api.probe_grid_positions(origin, spacing, dims)
    sh = np.random.default_rng(0).normal(size=(P, 9, 4)).astype(np.float32)
    rec = api.probe_grid_records(points, normals)
    d_pos, d_sh, d_rec = device_array(api, ctx, pos4), device_array(api, ctx, sh), device_array(api, ctx, rec)
    side = R + 2
    d_maps = api.Texture(ctx, 4, (P * side * side * 8 + 31) // 32)
    d_stats = api.Texture(ctx, 4, (P * 16 + 31) // 32)
    d_out = api.Texture(ctx, 4, (n * 16 + 31) // 32)

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

    row = {"tool": "probe_depth_bench", "scene": args.scene, "points": n, "dims": list(dims), "resolution": R, "subsamples": K,
           "max_distance": maxd, "scene_world_extent": extent, "normal_bias": float(bias), "ray_epsilon": eps, "runs": args.runs, "warmup": args.warmup}
    lib = _abi.lib()
    rays = P * R * R * K * K
    for stats in (False, True):
        bd = _abi.ProbeDepthDescC(R, K, api.PROBE_DEPTH_DEVICE_POINTERS, 0, eps, maxd)

        def bake():
            _abi.check(lib.lupin_hip_bake_probe_depth(ctx.handle, scene.handle, C.byref(bd), P, C.c_void_p(d_pos.device_ptr()), C.c_void_p(d_maps.device_ptr()),
                                                      C.c_void_p(d_stats.device_ptr()) if stats else None))
        row["bake_with_stats" if stats else "bake"] = dict(report(timed(bake), rays), rays=rays)
    st = d_stats.download().view(np.uint8).reshape(-1)[:P * 16].view(np.uint32).reshape(P, 4).astype(np.int64)
    row["bake_with_stats"].update(hits=int(st[:, 1].sum()), back_face_hits=int(st[:, 2].sum()))

    def grid_desc(flags):
        return _abi.ProbeGridDescC((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_uint32 * 3)(*dims), flags | api.PROBE_GRID_DEVICE_POINTERS, eps,
                                   float(bias))

    def unusable():
        res = d_out.download().view(np.uint8).reshape(-1)[:n * 16].view(np.float32).reshape(n, 4)
        return int((res[:, 3] == 0).sum())

    for back in (False, True):
        tag = "_backface" if back else ""
        bf = api.PROBE_GRID_BACKFACE if back else 0
        dd = _abi.ProbeGridDepthDescC(grid_desc(bf), R, maxd)

        def depth_lookup():
            _abi.check(lib.lupin_hip_sample_probe_grid_depth(ctx.handle, scene.handle, C.byref(dd), C.c_void_p(d_sh.device_ptr()), C.c_void_p(d_maps.device_ptr()),
                                                             None, n, C.c_void_p(d_rec.device_ptr()), C.c_void_p(d_out.device_ptr())))
        row["lookup_depth" + tag] = dict(report(timed(depth_lookup), n), unusable=(depth_lookup(), unusable())[1])
        for vis in (False, True):
            gd = grid_desc(bf | (api.PROBE_GRID_VISIBILITY if vis else 0))

            def plain_lookup():
                _abi.check(lib.lupin_hip_sample_probe_grid(ctx.handle, scene.handle, C.byref(gd), C.c_void_p(d_sh.device_ptr()), None, n,
                                                           C.c_void_p(d_rec.device_ptr()), C.c_void_p(d_out.device_ptr())))
            key = "lookup_" + ("visibility" if vis else "plain") + tag
            row[key] = dict(report(timed(plain_lookup), n), unusable=(plain_lookup(), unusable())[1])
        row["depth_over_visibility" + tag] = round(row["lookup_depth" + tag]["median_ms"] / row["lookup_visibility" + tag]["median_ms"], 4)
        row["depth_over_plain" + tag] = round(row["lookup_depth" + tag]["median_ms"] / row["lookup_plain" + tag]["median_ms"], 4)
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
