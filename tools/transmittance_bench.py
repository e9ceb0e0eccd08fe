"""Time transmittance queries (lupin_hip_transmittance_rays) against occlusion queries on the same slots.

usage: python tools/transmittance_bench.py [--points 65536] [--samples 64] [--radius-fraction 0.05] [--runs 5] [--warmup 2]
                                           [--out profiles/transmittance_bench.jsonl]
Ambient occlusion at `points` surface points of bistro_class (tools/occlusion_bench.py's points), `samples` cosine-weighted
directions each, up to radius = fraction x scene_world_extent, records and results in device memory.  Three legs, each the
median of `runs` host-clock times of one synchronised call after `warmup` calls:
  occlusion        lupin_hip_occlusion_rays on the scene as it is (the yardstick: k_occlusion on the same slots)
  transmittance    lupin_hip_transmittance_rays on the scene as it is: only the textured ground is alpha-capable, so every
                   other accepted triangle ends its slot as any-hit does
  alpha            lupin_hip_transmittance_rays on a copy whose foliage-like instances (those of every third mesh) carry
                   planar texcoords and whose materials reference a 64 x 64 cut-out alpha texture; the same records
Prints one JSON line and appends it to --out.  Needs a HIP device; there is no CPU fallback.
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


def cutout_texture(size=64, seed=11):
    """RGBA8: round holes (alpha 0) in a solid sheet (alpha 255) with a two-texel soft rim."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:size, 0:size]
    alpha = np.ones((size, size))
    for _ in range(24):
        cx, cy, r = rng.uniform(0, size, 2).tolist() + [rng.uniform(2.0, 7.0)]
        dx, dy = np.minimum(np.abs(x - cx), size - np.abs(x - cx)), np.minimum(np.abs(y - cy), size - np.abs(y - cy))
        alpha = np.minimum(alpha, np.clip((np.sqrt(dx * dx + dy * dy) - r) / 2.0, 0.0, 1.0))
    px = np.full((size, size, 4), 160, np.uint8)
    px[..., 3] = np.round(alpha * 255).astype(np.uint8)
    return np.ascontiguousarray(px)


def with_foliage_alpha(api, scene_cpu, textures, n_meshes=20):
    """The copy: meshes 0, 3, 6, ... of the first `n_meshes` get planar texcoords, every material that had no colour texture
    references the cut-out.  Returns the number of alpha-capable instances."""
    textures = list(textures) + [api.TextureCPU(cutout_texture())]
    tex = len(textures) - 1
    foliage = set(range(0, n_meshes, 3))
    for m in foliage:
        v = scene_cpu.verts_pos_array[m]
        span = float((v[:, :3].max(0) - v[:, :3].min(0)).max())
        scene_cpu.verts_texcoord_array.append(np.ascontiguousarray(v[:, :2] * np.float32(6.0 / span), np.float32))
        scene_cpu.mesh_infos[m]["texcoords_buf_idx"] = len(scene_cpu.verts_texcoord_array) - 1
    for mat in scene_cpu.materials:
        if int(mat["color_tex_idx"]) == 0xFFFFFFFF:
            mat["color_tex_idx"] = tex
    api.validate_scene(scene_cpu, len(textures), len(textures))
    return textures, int(np.isin(scene_cpu.instances["mesh_idx"], list(foliage)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1 << 16)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--radius-fraction", type=float, default=0.05)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "transmittance_bench.jsonl"))
    args = ap.parse_args()

    from lupinpathtracer_amd import _abi, api, loader
    from oracle import oracle
    from tests import reproject_ref
    import occlusion_bench

    if api.device_count() < 1:
        raise SystemExit("transmittance_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    scene_cpu, textures, envs_info, cams = loader.build_scene_bistro_class_cpu(SHARED)
    scene = api.build_accel_structures_and_upload(ctx, scene_cpu, textures, envs_info, True)
    n, S, eps = args.points, args.samples, 0.001
    extent = float(api.scene_world_extent(scene))
    radius = np.float32(args.radius_fraction * extent)
    points, normals = occlusion_bench.surface_points(api, oracle, reproject_ref, ctx, scene, cams[0], n)
    rec = api.occlusion_records(points + normals * np.float32(api.LIGHTMAP_OFFSET_FRACTION * extent), normals, radius,
                                api.rng_seed_for(np.arange(n, dtype=np.uint32), 0))
    alpha_cpu, alpha_textures, alpha_envs, _ = loader.build_scene_bistro_class_cpu(SHARED)
    alpha_textures, capable = with_foliage_alpha(api, alpha_cpu, alpha_textures)
    alpha_scene = api.build_accel_structures_and_upload(ctx, alpha_cpu, alpha_textures, alpha_envs, True)

    d_rec = api.Texture(ctx, 4, n)      # device memory without another runtime in the process: the texels of textures
    d_rec.upload(rec.view(np.float16).reshape(n, 4, 4))
    d_out = api.Texture(ctx, 4, (n * 4 + 31) // 32)
    c = _abi.OcclusionDescC(int(api.OcclusionMode.COSINE_HEMISPHERE), S, api.OCCLUSION_DEVICE_POINTERS, eps)

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
        med = statistics.median(ms)
        return {"mslots_per_s": round(n * S / med / 1e3, 2), "median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    def call(entry, sc):
        return lambda: _abi.check(entry(ctx.handle, sc.handle, C.byref(c), n, C.c_void_p(d_rec.device_ptr()), C.c_void_p(d_out.device_ptr())))

    lib = _abi.lib()
    row = {"tool": "transmittance_bench", "scene": "bistro_class", "points": n, "samples": S, "slots": n * S, "radius": float(radius),
           "scene_world_extent": extent, "runs": args.runs, "warmup": args.warmup, "alpha_capable_instances_of_the_copy": capable}
    row["occlusion"] = timed(call(lib.lupin_hip_occlusion_rays, scene))
    blocked = d_out.download().view(np.uint32).reshape(-1)[:n].astype(np.int64)
    row["occlusion"]["mean_visibility"] = float(1.0 - blocked.sum() / (n * S))
    row["transmittance"] = timed(call(lib.lupin_hip_transmittance_rays, scene))
    row["transmittance"]["mean_visibility"] = float(d_out.download().view(np.float32).reshape(-1)[:n].astype(np.float64).sum() / (n * S))
    row["alpha"] = timed(call(lib.lupin_hip_transmittance_rays, alpha_scene))
    row["alpha"]["mean_visibility"] = float(d_out.download().view(np.float32).reshape(-1)[:n].astype(np.float64).sum() / (n * S))
    row["alpha_occlusion"] = timed(call(lib.lupin_hip_occlusion_rays, alpha_scene))
    row["transmittance_over_occlusion"] = round(row["transmittance"]["median_ms"] / row["occlusion"]["median_ms"], 3)
    row["alpha_over_occlusion"] = round(row["alpha"]["median_ms"] / row["occlusion"]["median_ms"], 3)
    line = json.dumps(row)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
