"""Time lightmap UV generation (lupin_hip_unwrap_lightmap_uvs) and count what it opens to the lightmap bake.

usage: python tools/lightmap_unwrap_bench.py [--runs 3] [--texels 128] [--padding 2] [--atlas 2048] [--out profiles/lightmap_unwrap_bench.jsonl]
Needs a HIP device (there is no CPU fallback): without one it stops at once and says so.
One JSON line per mesh -- the largest mesh of bistro_class and bunny.ply -- with texel_size = the mesh's largest extent /
`texels`: triangles, vertices, charts, the mesh's atlas, degenerate triangles, the medians over `runs` calls of the call's
host-clock phases (charts_ms, rects_ms, pack_ms, uvs_ms) and of the whole call, and restatement_ms, the numpy restatement
(tests/lightmap_unwrap_ref.py) on the same mesh once: the host baseline.
Then one line "bistro_class_charted": every mesh of bistro_class unwrapped and attached, every instance placed in one atlas
(api.pack_lightmap_instances, multipliers scaled so that the atlas is about `atlas` texels wide), and a one-sample bake:
how many of the scene's instances the bake can chart now, against the one with material texcoords before, and at what
covered-texel count."""
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
        raise SystemExit("lightmap_unwrap_bench needs a HIP device; the product has no CPU fallback")
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--texels", type=int, default=128)
    ap.add_argument("--padding", type=int, default=2)
    ap.add_argument("--atlas", type=int, default=2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from lupinpathtracer_amd import loader
    from tests import lightmap_ref, lightmap_unwrap_ref, util

    ctx = api.Context(0)
    lines = []

    def extent(pos):
        p = np.asarray(pos, np.float32).reshape(-1, 4)[:, :3]
        return float((p.max(axis=0) - p.min(axis=0)).max())

    def measure(name, scene, cpu, mesh):
        texel = extent(cpu.verts_pos_array[mesh]) / args.texels
        calls, phases = [], []
        for _ in range(args.runs + 1):
            t = time.perf_counter()
            _, info = scene.unwrap_lightmap_uvs(mesh, texel, args.padding, attach=False)
            calls.append((time.perf_counter() - t) * 1e3)
            phases.append(info)
        calls, phases = calls[1:], phases[1:]
        pos = np.asarray(cpu.verts_pos_array[mesh], np.float32).reshape(-1, 4)[:, :3]
        tris = lightmap_ref.mesh_triangles(scene)[mesh]
        t = time.perf_counter()
        ref = lightmap_unwrap_ref.unwrap(pos, tris, texel, args.padding)
        ref_ms = (time.perf_counter() - t) * 1e3
        info = phases[0]
        assert ref is not None and (ref["num_charts"], ref["width"], ref["height"]) == (info["num_charts"], info["width"], info["height"])
        line = dict(mesh=name, triangles=len(tris), vertices=len(pos), texel_size=texel, padding=args.padding, charts=info["num_charts"], width=info["width"],
                    height=info["height"], degenerate_tris=info["degenerate_tris"], call_ms=statistics.median(calls), restatement_ms=ref_ms)
        for k in ("charts_ms", "rects_ms", "pack_ms", "uvs_ms"):
            line[k] = statistics.median(p[k] for p in phases)
        lines.append(line)
        print(json.dumps(line), flush=True)

    cpu, textures, envs_info, _ = loader.build_scene_bistro_class_cpu(util.SHARED)
    scene = api.build_accel_structures_and_upload(ctx, cpu, textures, envs_info, True)
    largest = int(np.argmax([len(i) for i in cpu.indices_array]))
    measure(f"bistro_class mesh {largest}", scene, cpu, largest)

    bunny = api.SceneCPU()
    loader.load_mesh_ply(os.path.join(util.SHARED, "shapes", "bunny.ply"), bunny)
    bunny.materials = np.array([api.default_material()], api.MATERIAL_DTYPE)
    inst = api.default_instance()
    bunny.instances = np.array([inst], api.INSTANCE_DTYPE)
    measure("bunny.ply", api.build_accel_structures_and_upload(ctx, bunny, [], [], True), bunny, 0)

    # every instance of bistro_class in one atlas
    with_uv = sum(int(cpu.mesh_infos[int(i["mesh_idx"])]["texcoords_buf_idx"]) != 0xFFFFFFFF for i in cpu.instances)
    t = time.perf_counter()
    sizes = {}
    for m in range(len(cpu.indices_array)):
        if len(cpu.indices_array[m]) == 0:
            continue
        _, info = scene.unwrap_lightmap_uvs(m, extent(cpu.verts_pos_array[m]) / args.texels, args.padding)
        if info["num_charts"]:
            sizes[m] = (info["width"], info["height"])
        else:
            scene.set_lightmap_uvs(m, None)
    unwrap_all_ms = (time.perf_counter() - t) * 1e3
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
    t = time.perf_counter()
    rgba = api.bake_lightmap(ctx, scene, charts, width, height, samples=1, max_bounces=2)
    bake_ms = (time.perf_counter() - t) * 1e3
    stats = api.lightmap_stats()
    line = dict(mesh="bistro_class_charted", instances=len(cpu.instances), chartable_with_texcoords=int(with_uv), chartable_with_sets=len(placed),
                meshes_unwrapped=len(sizes), unwrap_all_ms=unwrap_all_ms, multiplier=m, atlas_width=width, atlas_height=height,
                covered_texels=int((rgba[..., 3] == 1.0).sum()), keys=stats["keys"], raster_ms=stats["raster_ms"], compact_ms=stats["compact_ms"],
                one_sample_bake_ms=bake_ms)
    lines.append(line)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
