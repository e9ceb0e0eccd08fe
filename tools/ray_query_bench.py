"""Time radiance queries (lupin_hip_pathtrace_rays) against pathtrace_scene on the same first rays.

usage: python tools/ray_query_bench.py [--scene bistro_class] [--size 1920x1080] [--bounces 16] [--runs 5] [--warmup 2]
                                       [--chunk-samples 4] [--only render|query]
Prints one JSON line.  The records are the frame's camera rays (the oracle's, seeded as the pixels are), queried through
device pointers with one sample per record.  Every figure is Mpaths/s from the median of `runs` host-clock times of one
call that ends synchronised, after `warmup` calls:
  render          pathtrace_scene of the frame, samples_per_pixel 1, one frame per wavefront (set_batch_frames(1))
  query           the query with the default max_slots
  query_half / query_double       the same query at half and at double the default max_slots.  A set that fits half the
                  default (1080p does) is one wavefront at all three: these two rows then repeat `query` and show its
                  run-to-run spread, nothing about the default
  chunks          the query with `chunk-samples` samples per record at half, the default and double max_slots: these rows
                  differ in the number of wavefronts and are the ones that bear on the default
--only runs one leg alone (for a kernel trace of that leg).  Needs a HIP device; there is no CPU fallback.
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
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--bounces", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--chunk-samples", type=int, default=4)
    ap.add_argument("--only", choices=("render", "query"), default=None)
    args = ap.parse_args()

    from lupinpathtracer_amd import _abi, api
    from oracle import oracle
    from tests import util

    if api.device_count() < 1:
        raise SystemExit("ray_query_bench needs a HIP device; the product has no CPU fallback")
    DEFAULT_MAX_SLOTS = api.RAYS_DEFAULT_MAX_SLOTS
    W, H = (int(v) for v in args.size.split("x"))
    ctx = api.Context(0)
    scene, cams = util.load_scene(args.scene, ctx)
    cam = cams[0]
    cp = api.CameraParams(**{**cam.params.__dict__, "aspect": W / H})
    n = W * H

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

    def report(paths, ms):
        med = statistics.median(ms)
        return {"mpaths_per_s": round(paths / med / 1e3, 2), "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    row = {"tool": "ray_query_bench", "scene": args.scene, "size": args.size, "paths": n, "bounces": args.bounces, "runs": args.runs,
           "warmup": args.warmup, "default_max_slots": DEFAULT_MAX_SLOTS}

    if args.only != "query":
        res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(max_bounces=args.bounces, samples_per_pixel=1))
        target = api.Texture(ctx, W, H)
        ctx.set_batch_frames(1)
        desc = api.PathtraceDesc(camera_params=cp, camera_transform=cam.transform)
        row["render"] = report(n, timed(lambda: api.pathtrace_scene(ctx, res, scene, target, api.PathtraceType.Standard, desc)))
        ctx.set_batch_frames(0)

    if args.only != "render":
        ori, dir_ = oracle.camera_rays(scene, W, H, cp, cam.transform, 0)
        seed = api.rng_seed_for(np.arange(n, dtype=np.uint32), 0)
        with np.errstate(over="ignore"):
            for _ in range(4):   # the camera's four draws
                seed = seed * np.uint32(747796405) + np.uint32(2891336453)
        rec = api.ray_records(ori.reshape(-1, 3), dir_.reshape(-1, 3), seed)
        # device memory without another runtime in the process: the texels of textures (8 bytes each)
        d_rec = api.Texture(ctx, 4, n)
        d_rec.upload(rec.view(np.float16).reshape(n, 4, 4))
        d_out = api.Texture(ctx, 2, n)

        def query(samples, max_slots):
            c = _abi.RayQueryDescC(0, args.bounces, samples, api.RAYS_DEVICE_POINTERS, max_slots, _abi.AdvancedParamsC(100.0, 0, 0.001))
            _abi.check(_abi.lib().lupin_hip_pathtrace_rays(ctx.handle, scene.handle, C.byref(c), n, C.c_void_p(d_rec.device_ptr()),
                                                           C.c_void_p(d_out.device_ptr()), None))

        row["query"] = report(n, timed(lambda: query(1, 0)))
        if args.only is None:
            row["query_half"] = report(n, timed(lambda: query(1, DEFAULT_MAX_SLOTS // 2)))
            row["query_double"] = report(n, timed(lambda: query(1, DEFAULT_MAX_SLOTS * 2)))
            S = args.chunk_samples
            row["chunks"] = {"samples": S, "paths": n * S}
            for label, slots in (("half", DEFAULT_MAX_SLOTS // 2), ("default", DEFAULT_MAX_SLOTS), ("double", DEFAULT_MAX_SLOTS * 2)):
                row["chunks"][label] = {"max_slots": slots, "wavefronts": -(-n // max(1, slots // S)), **report(n * S, timed(lambda: query(S, slots)))}
            mean = d_out.download().view(np.float32).reshape(n, 4)[:, :3].astype(np.float64).mean()
            row["mean_radiance"] = round(float(mean), 5)
    if "render" in row and "query" in row:
        row["query_over_render"] = round(row["query"]["mpaths_per_s"] / row["render"]["mpaths_per_s"], 4)
    print(json.dumps(row), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
