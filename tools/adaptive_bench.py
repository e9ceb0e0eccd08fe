"""Time adaptive sampling (lupin_hip_pathtrace_scene_adaptive) against plain pathtrace_scene calls on the same frame.

usage: python tools/adaptive_bench.py [--cases bistro_class:3840x2160,materials1:1920x1080] [--reps 10] [--warmup 3]
                                      [--spp 1] [--bounces 8] [--thresholds 1,0.5,0.3,0.2,0.1] [--settle 8]
Prints one JSON line per case.  Every time is the mean milliseconds per call of a host clock around `reps` chained calls
that end in a context sync, after `warmup` calls:
  plain_batched   pathtrace_scene with the default frames per wavefront
  plain_k1        pathtrace_scene, one frame per wavefront (set_batch_frames(1)): the fair comparison
  adaptive_full   adaptive calls with threshold 0 (every block active)
  sweep           per threshold: reset, `settle` calls (min_frames 4), then the timed calls; `active` is the mean
                  fraction of pixels the timed calls rendered (pixel-frames they added / (reps * W * H))
Needs a HIP device; there is no CPU fallback.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="bistro_class:3840x2160,materials1:1920x1080")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--thresholds", default="1,0.5,0.3,0.2,0.1")
    ap.add_argument("--settle", type=int, default=8)
    args = ap.parse_args()

    from lupinpathtracer_amd import api
    from tests import util

    if api.device_count() < 1:
        raise SystemExit("adaptive_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(max_bounces=args.bounces, samples_per_pixel=args.spp))
    for case in args.cases.split(","):
        name, size = case.split(":")
        W, H = (int(v) for v in size.split("x"))
        scene, cams = util.load_scene(name, ctx)
        cam = cams[0]
        cp = api.CameraParams(**{**cam.params.__dict__, "aspect": W / H})
        out = api.DoubleBufferedTexture(ctx, W, H)
        ares = api.build_adaptive_resources(ctx, W, H)
        state = {"k": 0}

        def plain():
            api.pathtrace_scene(ctx, res, scene, out.front(), api.PathtraceType.Standard, api.PathtraceDesc(
                accum_params=api.AccumulationParams(out.back(), state["k"]), camera_params=cp, camera_transform=cam.transform))
            state["k"] += 1
            out.flip()

        def adaptive(params):
            api.pathtrace_scene_adaptive(ctx, res, scene, out.front(), api.PathtraceType.Standard, api.PathtraceDesc(
                accum_params=api.AccumulationParams(out.back(), 0), camera_params=cp, camera_transform=cam.transform), ares, params)
            out.flip()

        def timed(fn, reps):
            for _ in range(args.warmup):
                fn()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            ctx.sync()
            return round((time.perf_counter() - t0) * 1e3 / reps, 3)

        row = {"tool": "adaptive_bench", "scene": name, "size": size, "pixels": W * H, "spp": args.spp, "bounces": args.bounces,
               "reps": args.reps, "warmup": args.warmup}
        row["plain_batched"] = timed(plain, args.reps)
        ctx.set_batch_frames(1)
        row["plain_k1"] = timed(plain, args.reps)
        ctx.set_batch_frames(0)
        full = api.AdaptiveParams(threshold=0.0, min_frames=0)
        ares.reset()
        row["adaptive_full"] = timed(lambda: adaptive(full), args.reps)
        sweep = []
        for t in (float(v) for v in args.thresholds.split(",")):
            p = api.AdaptiveParams(threshold=t, min_frames=4)
            ares.reset()
            for _ in range(args.settle):
                adaptive(p)
            before = ares.stats()
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                adaptive(p)
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3 / args.reps
            after = ares.stats()
            sweep.append({"threshold": t, "active": round((after.pixel_frames - before.pixel_frames) / (args.reps * W * H), 4),
                          "ms": round(ms, 3)})
        row["sweep"] = sweep
        print(json.dumps(row), flush=True)
        del out, ares
    ctx.close()


if __name__ == "__main__":
    main()
