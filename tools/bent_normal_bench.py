"""Time bent-normal queries (lupin_hip_bent_normal_rays) against the occlusion and transmittance queries on the same slots.

usage: python tools/bent_normal_bench.py [--points 65536] [--samples 16,64,256] [--radius-fraction 0.05] [--runs 5] [--warmup 2]
                                         [--atlas 1024] [--out profiles/bent_normal_bench.jsonl]
Ambient occlusion at `points` surface points of bistro_class (tools/occlusion_bench.py's points, tools/transmittance_bench.py's
records), S cosine-weighted directions each for every S of --samples, up to radius = fraction x scene_world_extent, records
and results in device memory.  Four legs per S, each the median of `runs` host-clock times of one synchronised call after
`warmup` calls, with min and max:
  occlusion            lupin_hip_occlusion_rays        (one kernel, integer atomics)
  transmittance        lupin_hip_transmittance_rays    (two kernels and a plane of one float per slot)
  bent_normal          lupin_hip_bent_normal_rays      (one kernel, one wave per record)
  bent_normal_opacity  the same with LUPIN_BENT_NORMAL_OPACITY
One JSON line per S, and with --atlas N one more for lupin_hip_bake_lightmap_ao of an N x N atlas over the instances that have
texcoords (64 slots per texel, both planes).  Lines are printed and appended to --out.  Needs a HIP device; no CPU fallback.
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
SHARED = os.path.join(ROOT, "tests", "golden", "scenes", "_shared")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 16)
    ap.add_argument("--samples", default="16,64,256")
    ap.add_argument("--radius-fraction", type=float, default=0.05)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--atlas", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bent_normal_bench.jsonl"))
    args = ap.parse_args()

    from lupinpathtracer_amd import _abi, api, loader
    from oracle import oracle
    from tests import reproject_ref
    import occlusion_bench

    if api.device_count() < 1:
        raise SystemExit("bent_normal_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    scene_cpu, textures, envs_info, cams = loader.build_scene_bistro_class_cpu(SHARED)
    scene = api.build_accel_structures_and_upload(ctx, scene_cpu, textures, envs_info, True)
    n, eps = args.points, 0.001
    extent = float(api.scene_world_extent(scene))
    radius = np.float32(args.radius_fraction * extent)
    points, normals = occlusion_bench.surface_points(api, oracle, reproject_ref, ctx, scene, cams[0], n)
    rec = api.occlusion_records(points + normals * np.float32(api.LIGHTMAP_OFFSET_FRACTION * extent), normals, radius,
                                api.rng_seed_for(np.arange(n, dtype=np.uint32), 0))

    d_rec = api.Texture(ctx, 4, n)      # device memory without another runtime in the process: the texels of textures
    d_rec.upload(rec.view(np.float16).reshape(n, 4, 4))
    d_out = api.Texture(ctx, 4, (n * 16 + 31) // 32)
    lib = _abi.lib()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def timed(fn, work):
        for _ in range(args.warmup):
            fn()
        ctx.sync()
        ms = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ms.append((time.perf_counter() - t0) * 1e3)
        med = statistics.median(ms)
        return {"mslots_per_s": round(work / med / 1e3, 2), "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    def out_floats(count):
        return d_out.download().view(np.float32).reshape(-1)[:count].astype(np.float64)

    for S in [int(s) for s in args.samples.split(",") if s]:
        seg = _abi.OcclusionDescC(int(api.OcclusionMode.COSINE_HEMISPHERE), S, api.OCCLUSION_DEVICE_POINTERS, eps)
        row = {"tool": "bent_normal_bench", "scene": "bistro_class", "points": n, "samples": S, "slots": n * S, "radius": float(radius),
               "scene_world_extent": extent, "runs": args.runs, "warmup": args.warmup}

        def segment(entry):
            return lambda: _abi.check(entry(ctx.handle, scene.handle, C.byref(seg), n, C.c_void_p(d_rec.device_ptr()), C.c_void_p(d_out.device_ptr())))

        def bent(flags):
            d = _abi.BentNormalDescC(S, flags | api.BENT_NORMAL_DEVICE_POINTERS, 0, eps)
            return lambda: _abi.check(lib.lupin_hip_bent_normal_rays(ctx.handle, scene.handle, C.byref(d), n, C.c_void_p(d_rec.device_ptr()),
                                                                     C.c_void_p(d_out.device_ptr())))

        row["occlusion"] = timed(segment(lib.lupin_hip_occlusion_rays), n * S)
        blocked = d_out.download().view(np.uint32).reshape(-1)[:n].astype(np.int64)
        row["occlusion"]["mean_visibility"] = float(1.0 - blocked.sum() / (n * S))
        row["transmittance"] = timed(segment(lib.lupin_hip_transmittance_rays), n * S)
        row["transmittance"]["mean_visibility"] = float(out_floats(n).sum() / (n * S))
        for leg, flags in (("bent_normal", 0), ("bent_normal_opacity", api.BENT_NORMAL_OPACITY)):
            row[leg] = timed(bent(flags), n * S)
            sums = out_floats(4 * n).reshape(n, 4)
            row[leg]["mean_visibility"] = float(sums[:, 3].sum() / (n * S))
            length = np.linalg.norm(sums[:, :3], axis=1)
            cos = np.einsum("ij,ij->i", sums[:, :3], normals.astype(np.float64))[length > 0] / length[length > 0]
            row[leg]["mean_cos_bent_to_normal"] = float(cos.mean())
        row["bent_normal_over_occlusion"] = round(row["bent_normal"]["median_ms"] / row["occlusion"]["median_ms"], 3)
        row["bent_normal_opacity_over_transmittance"] = round(row["bent_normal_opacity"]["median_ms"] / row["transmittance"]["median_ms"], 3)
        emit(row)

    if args.atlas:
        sentinel = 0xFFFFFFFF
        charted = [i for i, inst in enumerate(scene_cpu.instances) if int(scene_cpu.mesh_infos[int(inst["mesh_idx"])]["texcoords_buf_idx"]) != sentinel]
        charts = [api.LightmapChart(i) for i in charted[:64]]
        A, S = args.atlas, 64
        row = {"tool": "bent_normal_bench", "leg": "bake_lightmap_ao", "scene": "bistro_class", "atlas": [A, A], "samples": S, "charts": len(charts),
               "max_distance": float(radius), "runs": args.runs, "warmup": args.warmup}
        if charts:
            got = {}

            def bake():
                got["ao"], got["bent"] = api.bake_lightmap_ao(ctx, scene, charts, A, A, samples=S, max_distance=float(radius), dilate=2, want_bent=True)
            bake()
            covered = int((got["ao"][..., 3] == 1.0).sum())
            row.update(timed(bake, covered * S))
            row["covered_texels"] = covered
            row["mean_visibility"] = float(got["ao"][..., 0][got["ao"][..., 3] == 1.0].astype(np.float64).mean()) if covered else None
        emit(row)
    ctx.close()


if __name__ == "__main__":
    main()
