"""Time lightmap seam stitching (lupin_hip_stitch_lightmap).

usage: python tools/lightmap_stitch_bench.py [--runs 3] [--texels 128] [--padding 2] [--atlas 2048] [--iterations 32] [--out profiles/lightmap_stitch_bench.jsonl]
Needs a HIP device (there is no CPU fallback): without one it stops at once and says so.
Two inputs, one JSON line each: the largest mesh of bistro_class as one chart over its own atlas, and every instance of
bistro_class in one atlas (placed as tools/lightmap_unwrap_bench.py places them).  The atlas is a one-sample bake.  Per line:
the counts of the call, the medians over `runs` calls (after one that is not counted) of its host-clock phases (edges_ms,
samples_ms, incidence_ms, solve_ms), solve_ms_per_iteration, call_ms, and restatement_ms, the numpy restatement
(tests/lightmap_stitch_ref.py) on the same input once: the only baseline."""
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
        raise SystemExit("lightmap_stitch_bench needs a HIP device; the product has no CPU fallback")
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--texels", type=int, default=128)
    ap.add_argument("--padding", type=int, default=2)
    ap.add_argument("--atlas", type=int, default=2048)
    ap.add_argument("--iterations", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from lupinpathtracer_amd import loader
    from tests import lightmap_ref, lightmap_stitch_ref, util

    ctx = api.Context(0)
    lines = []

    def extent(pos):
        p = np.asarray(pos, np.float32).reshape(-1, 4)[:, :3]
        return float((p.max(axis=0) - p.min(axis=0)).max())

    def measure(name, scene, cpu, charts, width, height, sets):
        rgba = api.bake_lightmap(ctx, scene, charts, width, height, samples=1, max_bounces=2, dilate=1)
        calls, phases = [], []
        for _ in range(args.runs + 1):
            t = time.perf_counter()
            out, info = api.stitch_lightmap(ctx, scene, charts, rgba, iterations=args.iterations, want_info=True)
            calls.append((time.perf_counter() - t) * 1e3)
            phases.append(api.lightmap_stitch_stats())
        calls, phases = calls[1:], phases[1:]
        tris = lightmap_ref.mesh_triangles(scene)
        ref_charts = [(tris[int(cpu.instances[c.instance_idx]["mesh_idx"])], sets[int(cpu.instances[c.instance_idx]["mesh_idx"])], c) for c in charts]
        t = time.perf_counter()
        ref, ref_info = lightmap_stitch_ref.stitch(rgba, ref_charts, args.iterations)
        ref_ms = (time.perf_counter() - t) * 1e3
        line = dict(input=name, charts=len(charts), width=width, height=height, iterations=args.iterations,
                    half_edges=int(sum(3 * len(c[0]) for c in ref_charts)), call_ms=statistics.median(calls), restatement_ms=ref_ms,
                    words_differing_from_restatement=int((ref.view(np.uint32) != out.view(np.uint32)).sum()))
        for k in ("seam_edges", "non_manifold_edges", "sample_pairs", "dropped_pairs", "active_texels"):
            line[k] = info[k]
        line["energy_before"] = [float(v) for v in info["energy_before"]]
        line["energy_after"] = [float(v) for v in info["energy_after"]]
        for k in ("edges_ms", "samples_ms", "incidence_ms", "solve_ms"):
            line[k] = statistics.median(p[k] for p in phases)
        line["solve_ms_per_iteration"] = line["solve_ms"] / max(1, args.iterations)
        lines.append(line)
        print(json.dumps(line), flush=True)

    cpu, textures, envs_info, _ = loader.build_scene_bistro_class_cpu(util.SHARED)
    scene = api.build_accel_structures_and_upload(ctx, cpu, textures, envs_info, True)
    sizes, sets = {}, {}
    for m in range(len(cpu.indices_array)):
        if len(cpu.indices_array[m]) == 0:
            continue
        uvs, info = scene.unwrap_lightmap_uvs(m, extent(cpu.verts_pos_array[m]) / args.texels, args.padding)
        if info["num_charts"]:
            sizes[m], sets[m] = (info["width"], info["height"]), uvs
        else:
            scene.set_lightmap_uvs(m, None)

    largest = int(np.argmax([len(i) for i in cpu.indices_array]))
    first = next(i for i, inst in enumerate(cpu.instances) if int(inst["mesh_idx"]) == largest)
    width, height, charts = api.pack_lightmap_instances([sizes[largest]], [1.0], 0)
    charts[0].instance_idx = first
    measure(f"bistro_class mesh {largest}", scene, cpu, charts, width, height, sets)

    placed = [i for i, inst in enumerate(cpu.instances) if int(inst["mesh_idx"]) in sizes]
    entry_sizes = [sizes[int(cpu.instances[i]["mesh_idx"])] for i in placed]
    m = 1.0
    for _ in range(8):          # scale all instances alike until the atlas is about --atlas wide
        width, height, charts = api.pack_lightmap_instances(entry_sizes, [m] * len(placed), 1)
        if max(width, height) <= args.atlas:
            break
        m *= 0.9 * args.atlas / max(width, height)
    for c, i in zip(charts, placed):
        c.instance_idx = i
    measure(f"bistro_class, {len(placed)} instances", scene, cpu, charts, width, height, sets)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
