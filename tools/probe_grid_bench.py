"""Time irradiance volume lookups (lupin_hip_sample_probe_grid) against the occlusion query they fuse.

usage: python tools/probe_grid_bench.py [--scene bistro_class] [--points 1048576] [--dims 16x16x4] [--runs 5] [--warmup 2]
                                        [--out profiles/probe_grid_bench.jsonl]
A `dims` grid of random coefficients over the scene's box, `points` surface points (the first hits of a square frame's camera
rays with their geometric normals turned toward the camera: tools/occlusion_bench.py's), records and results in device
memory.  Every figure is the median (min - max) of `runs` host-clock times of one call that ends synchronised, after `warmup`
calls, for each combination of the VISIBILITY and BACKFACE flags.  The yardstick, in the same process: api.occlusion_rays'
entry point on the same 8 x points segments as direction-mode records in device memory -- what the fused kernel replaces,
less the building of those records (here done once by tests/probe_grid_ref.py, outside the timing) and the blend.
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


def device_array(api, ctx, a):
    """Device memory without another runtime in the process: the texels of a texture (8 bytes each, 32 a row)."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    rows = max(1, (len(raw) + 31) // 32)
    buf = np.zeros(rows * 32, np.uint8)
    buf[:len(raw)] = raw
    tex = api.Texture(ctx, 4, rows)
    tex.upload(buf.view(np.float16).reshape(rows, 4, 4))
    return tex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bistro_class")
    ap.add_argument("--points", type=int, default=1 << 20)
    ap.add_argument("--dims", default="16x16x4")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_grid_bench.jsonl"))
    args = ap.parse_args()

    from lupinpathtracer_amd import _abi, api
    from oracle import oracle
    from tests import probe_grid_ref, reproject_ref, util
    from tools.occlusion_bench import surface_points

    if api.device_count() < 1:
        raise SystemExit("probe_grid_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    scene, cams = util.load_scene(args.scene, ctx)
    n, eps = args.points, 0.001
    dims = tuple(int(x) for x in args.dims.split("x"))
    extent = float(api.scene_world_extent(scene))
    bias = np.float32(api.LIGHTMAP_OFFSET_FRACTION * extent)
    points, normals = surface_points(api, oracle, reproject_ref, ctx, scene, cams[0], n)
    lo, hi = points.min(0), points.max(0)
    origin = lo.astype(np.float32)
    spacing = np.float32([max((hi[k] - lo[k]) / max(1, dims[k] - 1), 1e-3 * extent) for k in range(3)])
    P = int(np.prod(dims))
    sh = np.random.default_rng(0).normal(size=(P, 9, 4)).astype(np.float32)
    rec = api.probe_grid_records(points, normals)
    d_sh, d_rec = device_array(api, ctx, sh), device_array(api, ctx, rec)
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

    row = {"tool": "probe_grid_bench", "scene": args.scene, "points": n, "dims": list(dims), "scene_world_extent": extent,
           "normal_bias": float(bias), "ray_epsilon": eps, "runs": args.runs, "warmup": args.warmup}
    lib = _abi.lib()
    for vis in (False, True):
        for back in (False, True):
            flags = api.PROBE_GRID_DEVICE_POINTERS | (api.PROBE_GRID_VISIBILITY if vis else 0) | (api.PROBE_GRID_BACKFACE if back else 0)
            c = _abi.ProbeGridDescC((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_uint32 * 3)(*dims), flags, eps, float(bias))

            def fused():
                _abi.check(lib.lupin_hip_sample_probe_grid(ctx.handle, scene.handle, C.byref(c), C.c_void_p(d_sh.device_ptr()), None, n,
                                                           C.c_void_p(d_rec.device_ptr()), C.c_void_p(d_out.device_ptr())))
            key = "fused" + ("_visibility" if vis else "") + ("_backface" if back else "")
            row[key] = report(timed(fused), n)
            res = d_out.download().view(np.uint8).reshape(-1)[:n * 16].view(np.float32).reshape(n, 4)
            row[key]["unusable"] = int((res[:, 3] == 0).sum())

    # the yardstick: the same segments through lupin_hip_occlusion_rays, records already in device memory
    cn = probe_grid_ref.corners(origin, spacing, dims, rec, bias)
    seg, mask = probe_grid_ref.segments(cn, eps)
    m = len(seg)
    d_seg = device_array(api, ctx, seg)
    d_cnt = api.Texture(ctx, 4, (m * 4 + 31) // 32)
    oc = _abi.OcclusionDescC(int(api.OcclusionMode.DIRECTION), 1, api.OCCLUSION_DEVICE_POINTERS, eps)

    def unfused():
        _abi.check(lib.lupin_hip_occlusion_rays(ctx.handle, scene.handle, C.byref(oc), m, C.c_void_p(d_seg.device_ptr()), C.c_void_p(d_cnt.device_ptr())))
    row["occlusion_rays_same_segments"] = report(timed(unfused), m)
    row["occlusion_rays_same_segments"]["segments"] = m
    row["occlusion_rays_same_segments"]["blocked"] = int(d_cnt.download().view(np.uint32).reshape(-1)[:m].astype(np.int64).sum())
    row["fused_visibility_over_occlusion_rays"] = round(row["fused_visibility"]["median_ms"] / row["occlusion_rays_same_segments"]["median_ms"], 4)
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
