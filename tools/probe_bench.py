"""Time light-probe baking (lupin_hip_bake_probes) against its emulation on the host and against the trace alone.

usage: python tools/probe_bench.py [--scene bistro_class] [--grid 16x16x4] [--samples 1024] [--bounces 16] [--runs 5] [--warmup 2]
                                   [--out profiles/probe_bench.jsonl]
Prints one JSON line and appends it to --out.  A grid of probes over the middle of the scene's box (margins of 10 %),
Standard integrator.  Every figure comes from the median of `runs` host-clock times of one call that ends synchronised,
after `warmup` calls:
  bake        api.bake_probes from host positions: 16 B per probe up, 144 B per probe down
  emulation   what a caller did before: n * samples mode-0 records built in numpy (seeds, two PCG draws, the sphere
              sampler), api.pathtrace_rays from host arrays with samples = 1 (32 B per path up, 16 B per path down), the
              projection in numpy; `records_ms`, `query_ms` and `project_ms` are its three parts
  trace       lupin_hip_pathtrace_rays with samples = 1 on the bake's own first rays, records and results in device
              memory: the same paths without k_begin_probes' sampling and k_resolve_probes' reduction
Needs a HIP device; there is no CPU fallback.
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


def pcg_draw(state):
    """rnd() of the device on uint32 arrays: (next state, the f32 in [0, 1])."""
    with np.errstate(over="ignore"):
        s = state * np.uint32(747796405) + np.uint32(2891336453)
        r = ((s >> ((s >> np.uint32(28)) + np.uint32(4))) ^ s) * np.uint32(277803737)
        r = (r >> np.uint32(22)) ^ r
    return s, r.astype(np.float32) / np.float32(4294967295.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bistro_class")
    ap.add_argument("--grid", default="16x16x4")
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--bounces", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_bench.jsonl"))
    args = ap.parse_args()

    from lupinpathtracer_amd import _abi, api
    from tests import util

    if api.device_count() < 1:
        raise SystemExit("probe_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    scene, _ = util.load_scene(args.scene, ctx)
    gx, gy, gz = (int(v) for v in args.grid.split("x"))
    S, n = args.samples, gx * gy * gz
    paths = n * S

    # the scene's box from the instances' model boxes (as api.scene_world_extent walks them)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    for inst in scene.instances:
        box = np.asarray(scene.model_aabbs[int(inst["mesh_idx"])], np.float64)
        if not np.all(box[:3] <= box[3:]):
            continue
        m = np.asarray(inst["transpose_inverse_transform"], np.float64)
        corners = np.array([[box[0 + 3 * (k & 1)], box[1 + 3 * ((k >> 1) & 1)], box[2 + 3 * ((k >> 2) & 1)]] for k in range(8)])
        world = (corners - m[:, 3]) @ np.linalg.inv(m[:, :3]).T
        lo, hi = np.minimum(lo, world.min(axis=0)), np.maximum(hi, world.max(axis=0))
    fx, fy, fz = np.meshgrid((np.arange(gx) + 0.5) / gx, (np.arange(gy) + 0.5) / gy, (np.arange(gz) + 0.5) / gz, indexing="ij")
    frac = 0.1 + 0.8 * np.stack([fx, fy, fz], -1).reshape(-1, 3)
    pos = (lo + frac * (hi - lo)).astype(np.float32)

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
        return {"mpaths_per_s": round(paths / med / 1e3, 2), "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    row = {"tool": "probe_bench", "scene": args.scene, "grid": args.grid, "probes": n, "samples": S, "paths": paths, "bounces": args.bounces,
           "runs": args.runs, "warmup": args.warmup, "integrator": "Standard"}

    ptype = api.PathtraceType.Standard
    row["bake"] = report(timed(lambda: api.bake_probes(ctx, scene, pos, S, ptype, args.bounces)))

    parts = {"records_ms": [], "query_ms": [], "project_ms": []}
    desc1 = api.RayQueryDesc(ptype, args.bounces, 1)
    result = {}

    def emulate():
        t0 = time.perf_counter()
        word = np.repeat(api.rng_seed_for(np.arange(n, dtype=np.uint32), 0), S)
        state = api.ray_sample_seed(word, np.tile(np.arange(S, dtype=np.uint32), n))
        state, r0 = pcg_draw(state)
        state, r1 = pcg_draw(state)
        z = np.float32(1.0) - np.float32(2.0) * r1
        rad = np.sqrt(np.maximum(np.float32(0.0), np.float32(1.0) - z * z))
        phi = np.float32(2.0 * np.pi) * r0
        d = np.stack([rad * np.cos(phi), rad * np.sin(phi), z], -1)
        rec = api.ray_records(np.repeat(pos, S, axis=0), d, state)
        t1 = time.perf_counter()
        L = api.pathtrace_rays(ctx, scene, rec, desc1)[:, :3]
        t2 = time.perf_counter()
        Y = api.sh_basis(d).astype(np.float32)
        sh = np.einsum("psj,psc->pjc", Y.reshape(n, S, 9), L.reshape(n, S, 3)) * np.float32(4.0 * np.pi / S)
        t3 = time.perf_counter()
        parts["records_ms"].append((t1 - t0) * 1e3)
        parts["query_ms"].append((t2 - t1) * 1e3)
        parts["project_ms"].append((t3 - t2) * 1e3)
        result["sh"] = sh

    row["emulation"] = report(timed(emulate))
    for k, v in parts.items():
        row["emulation"][k] = round(statistics.median(v[args.warmup:]), 3)

    sh, rays = api.bake_probes(ctx, scene, pos, S, ptype, args.bounces, want_rays=True)
    # device memory without another runtime in the process: the texels of textures (8 bytes each)
    d_rec = api.Texture(ctx, 4, paths)
    d_rec.upload(rays.view(np.float16).reshape(paths, 4, 4))
    d_out = api.Texture(ctx, 2, paths)

    def trace():
        c = _abi.RayQueryDescC(int(ptype), args.bounces, 1, api.RAYS_DEVICE_POINTERS, 0, _abi.AdvancedParamsC(100.0, 0, 0.001))
        _abi.check(_abi.lib().lupin_hip_pathtrace_rays(ctx.handle, scene.handle, C.byref(c), paths, C.c_void_p(d_rec.device_ptr()),
                                                       C.c_void_p(d_out.device_ptr()), None))

    row["trace"] = report(timed(trace))
    row["emulation_over_bake"] = round(row["emulation"]["median_ms"] / row["bake"]["median_ms"], 3)
    row["bake_over_trace"] = round(row["bake"]["median_ms"] / row["trace"]["median_ms"], 4)
    row["mean_c0"] = [round(float(v), 5) for v in sh[:, 0, :3].astype(np.float64).mean(axis=0)]
    row["emulated_mean_c0"] = [round(float(v), 5) for v in result["sh"][:, 0, :].astype(np.float64).mean(axis=0)]
    row["mean_w0"] = round(float(sh[:, 0, 3].astype(np.float64).mean()), 6)
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
