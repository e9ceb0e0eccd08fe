"""Time occlusion queries (lupin_hip_occlusion_rays) against the closest-hit probe on the same rays.

usage: python tools/occlusion_bench.py [--scene bistro_class] [--points 65536] [--samples 64] [--radius-fraction 0.05]
                                       [--runs 5] [--warmup 2] [--only device|host|closest] [--out profiles/occlusion_bench.jsonl]
Ambient occlusion at `points` surface points (the first hits of a square frame's camera rays, with their geometric normals
turned toward the camera, moved off the surface by 1e-4 of the scene's extent), `samples` cosine-weighted directions each,
radius = `radius-fraction` of scene_world_extent.  Every figure is the median of `runs` host-clock times of one call that ends
synchronised, after `warmup` calls:
  device    occlusion_rays in hemisphere mode, records and counts in device memory
  host      the same from host arrays (32 B per record up, 4 B per record down)
  closest   what the library offered before: api.trace_rays (closest hit, host arrays) on the same points * samples first
            rays, taken once from pathtrace_rays(..., want_rays=True) at max_bounces = 0, then hit & (dst < tmax) in numpy
Prints one JSON line and appends it to --out.  --only runs one leg alone (for a kernel trace of that leg: k_occlusion against
k_trace).  Needs a HIP device; there is no CPU fallback.
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


def surface_points(api, oracle, reproject_ref, ctx, scene, cam, count):
    """`count` surface points seen by the camera: (points, unit normals facing the camera), float32."""
    side = 64
    while True:
        cp = api.CameraParams(**{**cam.params.__dict__, "aspect": 1.0})
        ori, dir_ = oracle.camera_rays(scene, side, side, cp, cam.transform, 0)
        ori, dir_ = ori.reshape(-1, 3), dir_.reshape(-1, 3)
        hit, dst, _, inst, tri = api.trace_rays(ctx, scene, ori, dir_, 0.001)
        if int((hit != 0).sum()) >= count or side >= 2048:
            break
        side *= 2
    sel = np.nonzero(hit != 0)[0]
    sel = np.resize(sel, count) if len(sel) < count else sel[np.linspace(0, len(sel) - 1, count).astype(np.int64)]
    o, d, t, inst, tri = ori[sel].astype(np.float64), dir_[sel].astype(np.float64), dst[sel].astype(np.float64), inst[sel], tri[sel]
    rows = np.array(scene.instances["transpose_inverse_transform"], np.float64).reshape(-1, 3, 4)
    mesh_idx = np.array(scene.instances["mesh_idx"], np.int64)
    normals = np.zeros((count, 3))
    for m in np.unique(mesh_idx[inst]):
        v, idx = reproject_ref.mesh_arrays(scene, int(m))
        v, idx = np.array(v[:, :3], np.float64), np.array(idx, np.int64).reshape(-1, 3)
        on = mesh_idx[inst] == m
        a = idx[tri[on]]
        nl = np.cross(v[a[:, 1]] - v[a[:, 0]], v[a[:, 2]] - v[a[:, 0]])
        normals[on] = np.einsum("nji,nj->ni", rows[inst[on]][:, :, :3], nl)      # normals go through the inverse transpose
    length = np.linalg.norm(normals, axis=1, keepdims=True)
    normals = np.where(length > 0, normals / np.where(length > 0, length, 1.0), -d)
    normals *= np.where((normals * d).sum(1, keepdims=True) > 0, -1.0, 1.0)
    return (o + d * t[:, None]).astype(np.float32), normals.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bistro_class")
    ap.add_argument("--points", type=int, default=1 << 16)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--radius-fraction", type=float, default=0.05)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("device", "host", "closest"), default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion_bench.jsonl"))
    args = ap.parse_args()

    from lupinpathtracer_amd import _abi, api
    from oracle import oracle
    from tests import reproject_ref, util

    if api.device_count() < 1:
        raise SystemExit("occlusion_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    scene, cams = util.load_scene(args.scene, ctx)
    n, S, eps = args.points, args.samples, 0.001
    extent = float(api.scene_world_extent(scene))
    radius = np.float32(args.radius_fraction * extent)
    points, normals = surface_points(api, oracle, reproject_ref, ctx, scene, cams[0], n)
    rec = api.occlusion_records(points + normals * np.float32(api.LIGHTMAP_OFFSET_FRACTION * extent), normals, radius,
                                api.rng_seed_for(np.arange(n, dtype=np.uint32), 0))

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

    def report(ms):
        med = statistics.median(ms)
        return {"mslots_per_s": round(n * S / med / 1e3, 2), "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    row = {"tool": "occlusion_bench", "scene": args.scene, "points": n, "samples": S, "slots": n * S, "radius": float(radius),
           "scene_world_extent": extent, "runs": args.runs, "warmup": args.warmup}

    if args.only in (None, "device"):
        # device memory without another runtime in the process: the texels of textures (8 bytes each)
        d_rec = api.Texture(ctx, 4, n)
        d_rec.upload(rec.view(np.float16).reshape(n, 4, 4))
        d_out = api.Texture(ctx, 4, (n * 4 + 31) // 32)
        c = _abi.OcclusionDescC(int(api.OcclusionMode.COSINE_HEMISPHERE), S, api.OCCLUSION_DEVICE_POINTERS, eps)

        def device():
            _abi.check(_abi.lib().lupin_hip_occlusion_rays(ctx.handle, scene.handle, C.byref(c), n, C.c_void_p(d_rec.device_ptr()),
                                                           C.c_void_p(d_out.device_ptr())))
        row["device"] = report(timed(device))
        row["device"]["blocked"] = int(d_out.download().view(np.uint32).reshape(-1)[:n].astype(np.int64).sum())

    if args.only in (None, "host"):
        out = {}
        row["host"] = report(timed(lambda: out.__setitem__("c", api.occlusion_rays(ctx, scene, rec, api.OcclusionMode.COSINE_HEMISPHERE, S, eps))))
        row["host"]["blocked"] = int(out["c"].astype(np.int64).sum())

    if args.only in (None, "closest"):
        qrec = rec.copy()
        qrec.view(np.uint32)[:, 7] = int(api.RayMode.COSINE_HEMISPHERE)
        _, rays = api.pathtrace_rays(ctx, scene, qrec, api.RayQueryDesc(api.PathtraceType.Naive, 0, S), want_rays=True)
        ori, dir_ = np.ascontiguousarray(rays[:, 0:3]), np.ascontiguousarray(rays[:, 4:7])
        del rays
        out = {}

        def closest():
            hit, dst, _, _, _ = api.trace_rays(ctx, scene, ori, dir_, eps)
            out["b"] = (hit != 0) & (dst < radius)
        row["closest"] = report(timed(closest))
        row["closest"]["blocked"] = int(out["b"].sum())

    if "device" in row and "closest" in row:
        row["device_over_closest"] = round(row["device"]["median_ms"] / row["closest"]["median_ms"], 4)
    if "host" in row and "closest" in row:
        row["host_over_closest"] = round(row["host"]["median_ms"] / row["closest"]["median_ms"], 4)
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
