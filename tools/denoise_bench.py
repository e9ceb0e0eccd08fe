"""Time lp::denoise (lupin_hip_denoise) at Low / Medium / High on a rendered frame with its G-buffers.

usage: python tools/denoise_bench.py [--sizes 1920x1080,3840x2160] [--reps 20] [--warmup 3] [--scene cornellbox_builtin]
Prints one JSON line: per size and quality the mean milliseconds per call (host clock around `reps` enqueued calls that
end in a context sync, after `warmup` calls), plus the pixel count.  Needs a HIP device; there is no CPU fallback.
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
    ap.add_argument("--sizes", default="1920x1080,3840x2160")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scene", default="cornellbox_builtin")
    args = ap.parse_args()

    import numpy as np
    from lupinpathtracer_amd import api
    from tests import util

    if api.device_count() < 1:
        raise SystemExit("denoise_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    scene, cams = util.load_scene(args.scene, ctx)
    cam = cams[0]
    res = api.build_pathtrace_resources(ctx, api.BakedPathtraceParams(max_bounces=8, samples_per_pixel=4))
    result = {"tool": "denoise_bench", "scene": args.scene, "reps": args.reps, "warmup": args.warmup, "ms": {}}
    for size in args.sizes.split(","):
        W, H = (int(v) for v in size.split("x"))
        desc = api.PathtraceDesc(camera_params=api.CameraParams(**{**cam.params.__dict__, "aspect": W / H}), camera_transform=cam.transform)
        color, alb, nrm, out = (api.Texture(ctx, W, H) for _ in range(4))
        api.pathtrace_scene(ctx, res, scene, color, api.PathtraceType.Standard, desc)
        api.pathtrace_scene_falsecolor(ctx, res, scene, alb, api.FalsecolorType.Albedo, desc)
        api.pathtrace_scene_falsecolor(ctx, res, scene, nrm, api.FalsecolorType.Normals, desc)
        dres = api.build_denoise_resources(ctx, W, H)
        ctx.sync()
        row = {"pixels": W * H}
        for q in api.DenoiseQuality:
            d = api.DenoiseDesc(color, out, albedo=alb, normals=nrm, quality=q)
            for _ in range(args.warmup):
                api.denoise(ctx, dres, d)
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                api.denoise(ctx, dres, d)
            ctx.sync()
            row[q.name] = round((time.perf_counter() - t0) * 1e3 / args.reps, 4)
        img = out.download().astype(np.float32)
        row["finite"] = bool(np.all(np.isfinite(img)))
        result["ms"][size] = row
        del dres, color, alb, nrm, out
    print(json.dumps(result))
    ctx.close()


if __name__ == "__main__":
    main()
