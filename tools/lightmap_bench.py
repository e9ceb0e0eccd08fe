"""Time lightmap baking (lupin_hip_bake_lightmap) on bistro_class: where the call's time goes, and what the same paths
cost through the radiance query alone.

usage: python tools/lightmap_bench.py [--sizes 1024,2048] [--samples 64] [--bounces 8] [--dilate 2] [--runs 3] [--warmup 1]
                                      [--out profiles/lightmap_bench.jsonl]
Needs a HIP device (there is no CPU fallback): without one it stops at once and says so.
The atlas is the one large instance of the scene that has texcoords, the ground quad (its UVs run to 40: the chart scales
them by 1 / 40, so that two triangles cover every texel -- the case one wave per triangle is there for); its two
triangles are turned over first, because the stand-in winds them facing down and a bake is of the front side.  One JSON line per
atlas size, medians of `runs` calls after `warmup`:
  raster_ms, compact_ms, scatter_dilate_ms, download_ms, trace_ms   the call's phases (lupin_hip_lightmap_stats, host clock,
                                each phase ends synchronised); other_share = everything but the trace / the whole call
  bake_mpaths_per_s             covered texels * samples / the whole call;  trace_mpaths_per_s: / the trace alone
  query_mpaths_per_s            api.pathtrace_rays on the same records from host arrays, the same number of paths
  denoise                       lupin_hip_denoise_lightmap (defaults, `dilate` gutter passes) on that atlas baked without gutter
                                passes: prep_ms, pass_ms per pass, dilate_ms (device events; lupin_hip_lightmap_denoise_stats),
                                their sum kernels_ms and its share of trace_ms, the call from host arrays (host clock)
  baseline (first size only, once)  the nearest equivalent without this entry point: the records built on the host by
                                tests/lightmap_ref.py (host_records_ms), then api.bake_irradiance-style tracing of them (query)
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
        raise SystemExit("lightmap_bench needs a HIP device; the product has no CPU fallback")
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1024,2048")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--dilate", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from lupinpathtracer_amd import loader
    from tests import lightmap_ref, util

    ctx = api.Context(0)
    cpu, textures, envs_info, _ = loader.build_scene_bistro_class_cpu(util.SHARED)
    with_uv = [i for i, inst in enumerate(cpu.instances) if int(cpu.mesh_infos[int(inst["mesh_idx"])]["texcoords_buf_idx"]) != 0xFFFFFFFF]
    ground = with_uv[0]
    # the stand-in's ground is wound so that its geometric normal (reference winding) points DOWN; a bake is of the front
    # side, so the tool turns the two triangles over: the hemispheres then look up into the scene, as a lightmap's would
    gmesh = int(cpu.instances[ground]["mesh_idx"])
    cpu.indices_array[gmesh] = np.ascontiguousarray(cpu.indices_array[gmesh].reshape(-1, 3)[:, ::-1]).reshape(-1)
    scene = api.build_accel_structures_and_upload(ctx, cpu, textures, envs_info, True)
    chart = api.LightmapChart(ground, 1.0 / 40.0, 1.0 / 40.0, 0.0, 0.0)
    offset = api.LIGHTMAP_OFFSET_FRACTION * api.scene_world_extent(scene)
    rows = []
    for k, size in enumerate(int(s) for s in args.sizes.split(",")):
        kw = dict(samples=args.samples, max_bounces=args.bounces, dilate=args.dilate, surface_offset=offset)
        phases, whole = [], []
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            out = api.bake_lightmap(ctx, scene, [chart], size, size, **kw)
            ms = (time.perf_counter() - t0) * 1e3
            if r >= args.warmup:
                whole.append(ms)
                phases.append(api.lightmap_stats())
        med = {key: statistics.median(p[key] for p in phases) for key in ("raster_ms", "compact_ms", "trace_ms", "scatter_dilate_ms", "download_ms")}
        covered = phases[0]["covered_texels"]
        paths = covered * args.samples
        call_ms = statistics.median(whole)
        other = med["raster_ms"] + med["compact_ms"] + med["scatter_dilate_ms"] + med["download_ms"]
        row = {"tool": "lightmap_bench", "scene": "bistro_class", "atlas": size, "samples": args.samples, "bounces": args.bounces,
               "dilate": args.dilate, "runs": args.runs, "covered_texels": covered, "paths": paths, "call_ms": round(call_ms, 3),
               **{key: round(v, 3) for key, v in med.items()}, "other_ms": round(other, 3),
               "other_share": round(other / (other + med["trace_ms"]), 4),
               "bake_mpaths_per_s": round(paths / call_ms / 1e3, 2), "trace_mpaths_per_s": round(paths / med["trace_ms"] / 1e3, 2),
               "mean_irradiance": round(float(out[..., :3][out[..., 3] == 1].astype(np.float64).mean()), 5)}
        # the denoise leg: the same bake without gutter passes and with its records, then lupin_hip_denoise_lightmap on them
        noisy, rec = api.bake_lightmap(ctx, scene, [chart], size, size, samples=args.samples, max_bounces=args.bounces, surface_offset=offset,
                                       want_records=True)
        dn_whole, dn = [], []
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            filtered = api.denoise_lightmap(ctx, noisy, rec, dilate=args.dilate)
            ms = (time.perf_counter() - t0) * 1e3
            if r >= args.warmup:
                dn_whole.append(ms)
                dn.append(api.lightmap_denoise_stats())
        passes = 5
        pass_ms = [statistics.median(d["pass_ms"][i] for d in dn) for i in range(passes)]
        prep_ms, dilate_ms = statistics.median(d["prep_ms"] for d in dn), statistics.median(d["dilate_ms"] for d in dn)
        kernels_ms = prep_ms + sum(pass_ms) + dilate_ms
        row["denoise"] = {"passes": passes, "normal_squarings": 5, "max_stretch": 4.0, "dilate": args.dilate,
                          "call_ms_host_arrays": round(statistics.median(dn_whole), 3),       # with 48 bytes per texel up and 16 down
                          "library_call_ms": round(statistics.median(d["call_ms"] for d in dn), 3),
                          "prep_ms": round(prep_ms, 4), "pass_ms": [round(v, 4) for v in pass_ms], "dilate_ms": round(dilate_ms, 4),
                          "kernels_ms": round(kernels_ms, 4), "kernels_over_trace": round(kernels_ms / med["trace_ms"], 6),
                          "pass_ns_per_texel": [round(v * 1e6 / (size * size), 4) for v in pass_ms],
                          "mean_irradiance_filtered": round(float(filtered[..., :3][filtered[..., 3] == 1].astype(np.float64).mean()), 5),
                          "mean_irradiance_noisy": round(float(noisy[..., :3][noisy[..., 3] == 1].astype(np.float64).mean()), 5)}
        rec = rec[rec.view(np.uint32)[..., 7] == 1]
        desc = api.RayQueryDesc(api.PathtraceType.Standard, args.bounces, args.samples)
        q = []
        for r in range(args.warmup + args.runs):
            t0 = time.perf_counter()
            api.pathtrace_rays(ctx, scene, rec, desc)
            q.append((time.perf_counter() - t0) * 1e3)
        row["query_ms"] = round(statistics.median(q[args.warmup:]), 3)
        row["query_mpaths_per_s"] = round(paths / row["query_ms"] / 1e3, 2)
        if k == 0:
            t0 = time.perf_counter()
            host_rec, owner = lightmap_ref.records(cpu, scene, [chart], size, size, np.float32(offset))
            host_rec = host_rec[owner != lightmap_ref.NO_OWNER]
            host_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            mean = api.pathtrace_rays(ctx, scene, host_rec, desc)
            trace_ms = (time.perf_counter() - t0) * 1e3
            same = bool(np.array_equal(np.float32(np.pi) * mean[:, :3], api.bake_lightmap(ctx, scene, [chart], size, size, samples=args.samples,
                                                                                         max_bounces=args.bounces, surface_offset=offset)[..., :3][owner != lightmap_ref.NO_OWNER]))
            row["baseline"] = {"host_records_ms": round(host_ms, 1), "query_ms": round(trace_ms, 3), "total_ms": round(host_ms + trace_ms, 1),
                               "same_words_as_the_bake": same}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
