"""Time distance queries (lupin_hip_distance_points, lupin_hip_bake_distance_grid).

usage: python tools/distance_bench.py [--scene bistro_class] [--points 1048576] [--grid 256] [--radius-fraction 0.05]
                                      [--runs 5] [--warmup 2] [--only device|host|grid|grid_unbounded] [--out profiles/distance_bench.jsonl]
Query points: the first hits of a square frame's camera rays, moved off the surface along their geometric normals by 1e-3 of
the scene's extent (tools/occlusion_bench.py's surface points).  Every figure is the median of `runs` host-clock times of one
call that ends synchronised, after `warmup` calls, with the spread (min, max) beside it:
  device          distance_points, unbounded, records and results in device memory
  host            the same from host arrays (16 B per record up, 48 B per result down)
  grid            a grid^3 volume over the scene's box, rmax = `radius-fraction` of scene_world_extent, into device memory
  grid_unbounded  the same grid with rmax = inf
Prints one JSON line and appends it to --out.  --only runs one leg alone (for a kernel trace of that leg).  Needs a HIP
device; there is no CPU fallback.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(call, runs, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t) * 1e3)
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bistro_class")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--radius-fraction", type=float, default=0.05)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_bench.jsonl"))
    a = ap.parse_args()
    from lupinpathtracer_amd import _abi, api
    from oracle import oracle
    from tests import reproject_ref, util
    import occlusion_bench
    if api.device_count() < 1:
        raise SystemExit("distance_bench needs a HIP device; there is no CPU fallback")
    ctx = api.Context(0)
    scene, cams = util.load_scene(a.scene, ctx)
    extent = float(api.scene_world_extent(scene))
    pts, nrm = occlusion_bench.surface_points(api, oracle, reproject_ref, ctx, scene, cams[0], a.points)
    pts, nrm = np.asarray(pts, np.float32), np.asarray(nrm, np.float32)
    rec = api.distance_records(pts + nrm * np.float32(1e-3 * extent))
    lib = _abi.lib()
    res = dict(tool="distance_bench", scene=a.scene, points=a.points, grid_size=a.grid, runs=a.runs, warmup=a.warmup, extent=extent)
    legs = [a.only] if a.only else ["device", "host", "grid", "grid_unbounded"]
    n = len(rec)
    if "device" in legs:
        d_rec, d_out = api.Texture(ctx, 4, (rec.nbytes + 31) // 32), api.Texture(ctx, 4, (n * 48 + 31) // 32)
        raw = np.zeros(d_rec.height * 32, np.uint8)
        raw[:rec.nbytes] = rec.view(np.uint8).reshape(-1)
        d_rec.upload(raw.view(np.float16).reshape(d_rec.height, 4, 4))

        def dev():
            api.check(lib.lupin_hip_distance_points(ctx.handle, scene.handle, api.DISTANCE_DEVICE_POINTERS, n, C.c_void_p(d_rec.device_ptr()), C.c_void_p(d_out.device_ptr())))
        res["device"] = timed(dev, a.runs, a.warmup)
    if "host" in legs:
        res["host"] = timed(lambda: api.distance_points(ctx, scene, rec), a.runs, a.warmup)
        found = api.distance_points(ctx, scene, rec)
        res["found_share"], res["median_distance"] = float((found["found"] != 0).mean()), float(np.median(found["distance"]))
    lo, hi = pts.min(0), pts.max(0)
    G = a.grid
    for leg, rmax in (("grid", a.radius_fraction * extent), ("grid_unbounded", float("inf"))):
        if leg not in legs:
            continue
        d_vol = api.Texture(ctx, 4, (G * G * G * 4 + 31) // 32)
        o, s, d = (C.c_float * 3)(*lo), (C.c_float * 3)(*((hi - lo) / G)), (C.c_uint32 * 3)(G, G, G)

        def grid():
            api.check(lib.lupin_hip_bake_distance_grid(ctx.handle, scene.handle, api.DISTANCE_DEVICE_POINTERS, o, s, d, rmax, C.c_void_p(d_vol.device_ptr())))
        res[leg] = timed(grid, a.runs, a.warmup)
    line = json.dumps(res)
    print(line)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
