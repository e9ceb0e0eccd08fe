"""Time adaptive lightmap baking (lupin_hip_bake_lightmap_adaptive) on bistro_class' ground, against the plain bake
(lupin_hip_bake_lightmap) at the sample count the adaptive bake's busiest texel took.

usage: python tools/lightmap_adaptive_bench.py [--sizes 1024] [--samples-per-round 16] [--threshold 0.05] [--min-rounds 2]
                                               [--max-rounds 16] [--bounces 8] [--dilate 2] [--runs 3] [--warmup 1]
                                               [--out profiles/lightmap_adaptive_bench.jsonl]
Needs a HIP device (there is no CPU fallback): without one it stops at once and says so.
The atlas is tools/lightmap_bench.py's: the ground quad, its UVs scaled by 1 / 40, its two triangles turned over.  One JSON
line per atlas size, medians of `runs` calls after `warmup`, appended to --out:
  adaptive   call_ms (host clock around the Python call), the phases of lupin_hip_lightmap_adaptive_stats summed over the
             rounds, rounds, paths, converged_texels, capped_texels, max_samples (the busiest texel's), and sample_histogram:
             {paths per texel: texels}
  plain      api.bake_lightmap with samples = max_samples: what every texel costs when all of them get what the worst one
             needs.  call_ms, trace_ms, paths
  paths_saved = 1 - adaptive paths / plain paths;  speedup = plain call_ms / adaptive call_ms
  mean_irradiance of both, and the largest and mean relative difference of the texels' luminance between the two
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    from lupinpathtracer_amd import api
    if api.device_count() < 1:
        raise SystemExit("lightmap_adaptive_bench needs a HIP device; the product has no CPU fallback")
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024")
    ap.add_argument("--samples-per-round", type=int, default=16)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--min-rounds", type=int, default=2)
    ap.add_argument("--max-rounds", type=int, default=16)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap_adaptive_bench.jsonl"))
    args = ap.parse_args()

    from lupinpathtracer_amd import loader
    from tests import util

    ctx = api.Context(0)
    cpu, textures, envs_info, _ = loader.build_scene_bistro_class_cpu(util.SHARED)
    with_uv = [i for i, inst in enumerate(cpu.instances) if int(cpu.mesh_infos[int(inst["mesh_idx"])]["texcoords_buf_idx"]) != 0xFFFFFFFF]
    ground = with_uv[0]
    gmesh = int(cpu.instances[ground]["mesh_idx"])
    cpu.indices_array[gmesh] = np.ascontiguousarray(cpu.indices_array[gmesh].reshape(-1, 3)[:, ::-1]).reshape(-1)   # as tools/lightmap_bench.py
    scene = api.build_accel_structures_and_upload(ctx, cpu, textures, envs_info, True)
    chart = api.LightmapChart(ground, 1.0 / 40.0, 1.0 / 40.0, 0.0, 0.0)
    offset = api.LIGHTMAP_OFFSET_FRACTION * api.scene_world_extent(scene)
    phase_keys = ("raster_ms", "compact_ms", "trace_ms", "merge_mask_ms", "scatter_dilate_ms", "download_ms")

    def luminance(rgba):
        return 0.2126 * rgba[..., 0].astype(np.float64) + 0.7152 * rgba[..., 1] + 0.0722 * rgba[..., 2]

    for size in (int(s) for s in args.sizes.split(",")):
        whole, phases = [], []
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            rgba, stats = api.bake_lightmap_adaptive(ctx, scene, [chart], size, size, samples_per_round=args.samples_per_round, threshold=args.threshold,
                                                     min_rounds=args.min_rounds, max_rounds=args.max_rounds, max_bounces=args.bounces, dilate=args.dilate,
                                                     surface_offset=offset, want_stats=True)
            ms = (time.perf_counter() - t0) * 1e3
            if r >= args.warmup:
                whole.append(ms)
                phases.append(api.lightmap_adaptive_stats())
        owned = rgba[..., 3] == 1
        counts, texels = np.unique(stats[..., 0][owned].astype(np.int64), return_counts=True)
        max_samples = int(counts.max())
        adaptive = {"call_ms": round(statistics.median(whole), 3), **{k: round(statistics.median(p[k] for p in phases), 3) for k in phase_keys},
                    "rounds": phases[0]["rounds"], "paths": phases[0]["paths"], "converged_texels": phases[0]["converged_texels"],
                    "capped_texels": phases[0]["capped_texels"], "max_samples": max_samples,
                    "sample_histogram": {str(int(c)): int(t) for c, t in zip(counts, texels)},
                    "mean_irradiance": round(float(rgba[..., :3][owned].astype(np.float64).mean()), 5)}
        # the comparison: the plain bake, every texel at the busiest texel's count
        pwhole, pphases = [], []
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            plain = api.bake_lightmap(ctx, scene, [chart], size, size, samples=max_samples, max_bounces=args.bounces, dilate=args.dilate,
                                      surface_offset=offset)
            ms = (time.perf_counter() - t0) * 1e3
            if r >= args.warmup:
                pwhole.append(ms)
                pphases.append(api.lightmap_stats())
        covered = pphases[0]["covered_texels"]
        plain_row = {"samples": max_samples, "call_ms": round(statistics.median(pwhole), 3),
                     "trace_ms": round(statistics.median(p["trace_ms"] for p in pphases), 3), "paths": covered * max_samples,
                     "mean_irradiance": round(float(plain[..., :3][owned].astype(np.float64).mean()), 5)}
        la, lp = luminance(rgba)[owned], luminance(plain)[owned]
        rel = np.abs(la - lp) / np.maximum(lp, 1e-3)
        row = {"tool": "lightmap_adaptive_bench", "scene": "bistro_class", "atlas": size, "samples_per_round": args.samples_per_round,
               "threshold": args.threshold, "min_rounds": args.min_rounds, "max_rounds": args.max_rounds, "bounces": args.bounces,
               "dilate": args.dilate, "runs": args.runs, "covered_texels": covered, "adaptive": adaptive, "plain": plain_row,
               "paths_saved": round(1.0 - adaptive["paths"] / plain_row["paths"], 4),
               "speedup": round(plain_row["call_ms"] / adaptive["call_ms"], 3),
               "luminance_rel_diff_max": round(float(rel.max()), 4), "luminance_rel_diff_mean": round(float(rel.mean()), 5)}
        print(json.dumps(row), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
