"""Time lupin_hip_adaptive_reproject and its two kernels against one adaptive frame of the same scene, size and spp.

usage: python tools/reproject_bench.py --case cornellbox_builtin:1920x1080 --step trace [--reps 10] [--warmup 3] [--spp 1]
                                       [--bounces 8] [--out profiles/reproject_bench.jsonl]
One case and ONE timed step per process (run each under its own time limit); prints one JSON line and appends it to --out:
  adaptive_frame   lupin_hip_pathtrace_scene_adaptive at threshold 0 (every block active): the yardstick.  Mean milliseconds
                   per call of a host clock around `reps` chained calls that end in a context sync
  reproject        the whole call, same clock, on a camera that moves by a few pixels every call
  trace, gather    device time of k_reproject_trace / k_reproject_gather: hipEvents around the launch
                   (lupin_hip_reproject_timings in the kernel-timing stats mode), mean over `reps` calls of the same sequence
Every step runs after `warmup` calls of its own kind, on a history of four adaptive frames.  The reprojecting steps also
report kept_fraction, the share of pixels that kept history in the last timed call.  Needs a HIP device; there is no CPU
fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = ("adaptive_frame", "reproject", "trace", "gather")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="cornellbox_builtin:1920x1080")
    ap.add_argument("--step", choices=STEPS, required=True)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spp", type=int, default=1)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    from lupinpathtracer_amd import api
    from tests import util

    if api.device_count() < 1:
        raise SystemExit("reproject_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(max_bounces=args.bounces, samples_per_pixel=args.spp))
    name, size = args.case.split(":")
    W, H = (int(v) for v in size.split("x"))
    scene, cams = util.load_scene(name, ctx)
    cam = cams[0]
    cp = api.CameraParams(**{**cam.params.__dict__, "aspect": W / H, "aperture": 0.0})
    out = api.DoubleBufferedTexture(ctx, W, H)
    ares = api.build_adaptive_resources(ctx, W, H)
    rp = api.build_reproject_resources(ctx, W, H)
    base = np.asarray(cam.transform, np.float32).reshape(4, 3)
    state = {"k": 0}

    def view():
        state["k"] += 1
        t = base.copy()
        t[3] += base[0] * np.float32(1e-3 * (state["k"] % 7))   # a few pixels along the camera's x axis
        return t

    def frame():
        api.pathtrace_scene_adaptive(ctx, res, scene, out.front(), api.PathtraceType.Standard, api.PathtraceDesc(
            accum_params=api.AccumulationParams(out.back(), 0), camera_params=cp, camera_transform=base), ares,
            api.AdaptiveParams(threshold=0.0, min_frames=0))
        out.flip()

    def reproject():
        api.adaptive_reproject(ctx, ares, rp, scene, api.ReprojectDesc(camera_params=cp, camera_transform=view()), out.back(), out.front())
        out.flip()

    row = {"tool": "reproject_bench", "scene": name, "size": size, "pixels": W * H, "spp": args.spp, "bounces": args.bounces,
           "reps": args.reps, "warmup": args.warmup, "step": args.step}
    reproject()   # the first view: no history yet
    for _ in range(4):
        frame()
    if args.step in ("adaptive_frame", "reproject"):
        fn = frame if args.step == "adaptive_frame" else reproject
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        ctx.sync()
        row["ms"] = round((time.perf_counter() - t0) * 1e3 / args.reps, 4)
    else:
        ctx.stats_reset(1)
        total = 0.0
        for k in range(args.warmup + args.reps):
            reproject()
            t = rp.timings()[0 if args.step == "trace" else 1]
            if k >= args.warmup:
                total += t
        row["ms"] = round(total / args.reps, 4)
    if args.step != "adaptive_frame":
        row["kept_fraction"] = round(float((ares.download()[0] > 0).mean()), 4)
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
