"""Time directional lightmaps (lupin_hip_bake_lightmap_directional, lupin_hip_render_lightmapped_directional) against the
scalar bake and the scalar view on the same tree.

usage: python tools/lightmap_directional_bench.py [--atlas 1024] [--samples 16,64,256] [--view 1920x1080] [--runs 5] [--warmup 2]
                                                  [--max-bounces 2] [--out profiles/lightmap_directional_bench.jsonl]
bistro_class, an N x N atlas over the first 64 instances that have texcoords.  Per S of --samples two legs, each the median of
`runs` host-clock times of one synchronised call after `warmup` calls, with min and max:
  bake_lightmap               lupin_hip_bake_lightmap               (k_resolve_rays, one plane)   -- unchanged code: the yardstick
  bake_lightmap_directional   lupin_hip_bake_lightmap_directional   (k_resolve_lightmap_sh, four planes)
and one line for the view of the S = 64 bakes: lupin_hip_render_lightmapped against the same call with `directional`, from a
camera aimed at the charted instance (of six directions the one that shows most of it); the tool fails if no pixel took a ratio.
The bake lines also time the entry point itself writing into one host array that has been written before (the Python wrapper
hands it a fresh, untouched np.zeros array each call), so that the library's share of a difference can be told from the host
pages' first touch.
Lines are printed and appended to --out.  Needs a HIP device; no CPU fallback.
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
SHARED = os.path.join(ROOT, "tests", "golden", "scenes", "_shared")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atlas", type=int, default=1024)
    ap.add_argument("--samples", default="16,64,256")
    ap.add_argument("--view", default="1920x1080")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--max-bounces", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmap_directional_bench.jsonl"))
    args = ap.parse_args()

    import ctypes as C
    from lupinpathtracer_amd import _abi, api, loader

    if api.device_count() < 1:
        raise SystemExit("lightmap_directional_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    scene_cpu, textures, envs_info, cams = loader.build_scene_bistro_class_cpu(SHARED)
    scene = api.build_accel_structures_and_upload(ctx, scene_cpu, textures, envs_info, True)
    sentinel = 0xFFFFFFFF
    charted = [i for i, inst in enumerate(scene_cpu.instances) if int(scene_cpu.mesh_infos[int(inst["mesh_idx"])]["texcoords_buf_idx"]) != sentinel]
    charts = [api.LightmapChart(i) for i in charted[:64]]
    if not charts:
        raise SystemExit("no instance of the scene has texcoords")
    A = args.atlas
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

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
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}

    def emit(row):
        line = json.dumps(row)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    kept = {}
    for S in [int(s) for s in args.samples.split(",") if s]:
        kw = dict(samples=S, max_bounces=args.max_bounces, dilate=2)
        got = {}

        def scalar():
            got["atlas"] = api.bake_lightmap(ctx, scene, charts, A, A, **kw)

        def directional():
            got["planes"] = api.bake_lightmap_directional(ctx, scene, charts, A, A, **kw)

        row = {"tool": "lightmap_directional_bench", "leg": "bake", "scene": "bistro_class", "atlas": [A, A], "samples": S, "charts": len(charts),
               "max_bounces": args.max_bounces, "runs": args.runs, "warmup": args.warmup}
        row["bake_lightmap"] = timed(scalar)
        row["bake_lightmap_directional"] = timed(directional)
        # the library alone, writing into one array that has been written before: api.bake_lightmap_directional hands it a fresh
        # np.zeros array every call, whose 64 MB of untouched pages the copy from the device has to fault in
        d = _abi.LightmapDescC(A, A, 0, args.max_bounces, S, 0, 0, 2, 0, float(api.LIGHTMAP_OFFSET_FRACTION * (api.scene_world_extent(scene) or 1.0)),
                               _abi.AdvancedParamsC(100.0, 0, 0.001))
        cc = (_abi.LightmapChartC * len(charts))(*[_abi.LightmapChartC(int(c.instance_idx), c.scale_u, c.scale_v, c.offset_u, c.offset_v) for c in charts])
        touched = np.ones((4, A, A, 4), np.float32)
        row["bake_lightmap_directional_into_a_touched_array"] = timed(lambda: _abi.check(_abi.lib().lupin_hip_bake_lightmap_directional(
            ctx.handle, scene.handle, C.byref(d), cc, len(charts), _abi.ptr(touched), None, None)))
        assert np.array_equal(touched.view(np.uint32), got["planes"].view(np.uint32))
        s = api.lightmap_stats()
        row["scalar_phases_ms"] = {k: round(s[k], 3) for k in ("raster_ms", "compact_ms", "trace_ms", "scatter_dilate_ms", "download_ms")}
        owned = got["atlas"][..., 3] == 1.0
        row["covered_texels"] = int(owned.sum())
        row["directional_over_scalar"] = round(row["bake_lightmap_directional"]["median_ms"] / row["bake_lightmap"]["median_ms"], 3)
        k0 = float(api.SH_K0)
        scalar_mean = float(got["atlas"][owned][:, :3].astype(np.float64).mean())
        row["mean_irradiance"] = scalar_mean
        row["mean_plane0_over_k0"] = float(got["planes"][0][owned][:, :3].astype(np.float64).mean() / k0)
        emit(row)
        if S == 64 or "atlas" not in kept:
            kept = dict(got)

    W, H = (int(v) for v in args.view.split("x"))
    tex = api.Texture(ctx, W, H)
    cam = cams[0]
    # a camera that sees the charted instance: its world box from the model box and the instance's world -> local affine
    inst = scene.instances[charts[0].instance_idx]
    box = np.asarray(scene.model_aabbs[int(inst["mesh_idx"])], np.float64)
    m = np.asarray(inst["transpose_inverse_transform"], np.float64)
    corners = np.array([[box[0 + 3 * (k & 1)], box[1 + 3 * ((k >> 1) & 1)], box[2 + 3 * ((k >> 2) & 1)]] for k in range(8)])
    world = (corners - m[:, 3]) @ np.linalg.inv(m[:, :3]).T
    centre, radius = world.mean(axis=0), 0.5 * np.linalg.norm(world.max(axis=0) - world.min(axis=0))

    def aimed(direction):
        z = -np.asarray(direction, np.float64) / np.linalg.norm(direction)          # the camera looks along its +z
        up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
        x = np.cross(up, z)
        x /= np.linalg.norm(x)
        return np.array([x, np.cross(z, x), z, centre - z * 1.2 * radius], np.float32)

    def ratio_pixels(transform, w, h):
        small = api.Texture(ctx, w, h)
        gb = api.render_lightmapped(ctx, scene, small, cam.params, transform, charts, kept["atlas"], directional=kept["planes"], want_gbuffer=True)
        return int((gb.view(np.uint32)[..., 23] & api.LIGHTMAPPED_DIRECTIONAL_APPLIED != 0).sum())

    views = [aimed(d) for d in ((0.3, 0.6, -1.0), (0.3, 0.6, 1.0), (1.0, 0.6, 0.3), (-1.0, 0.6, 0.3), (0.2, 1.0, 0.1), (0.2, -1.0, 0.1))]
    transform = max(views, key=lambda t: ratio_pixels(t, 160, 90))
    row = {"tool": "lightmap_directional_bench", "leg": "view", "scene": "bistro_class", "image": [W, H], "atlas": [A, A], "charts": len(charts),
           "runs": args.runs, "warmup": args.warmup}
    row["render_lightmapped"] = timed(lambda: api.render_lightmapped(ctx, scene, tex, cam.params, transform, charts, kept["atlas"]))
    row["render_lightmapped_directional"] = timed(lambda: api.render_lightmapped(ctx, scene, tex, cam.params, transform, charts, kept["atlas"],
                                                                                 directional=kept["planes"]))
    g = api.render_lightmapped(ctx, scene, tex, cam.params, transform, charts, kept["atlas"], directional=kept["planes"], want_gbuffer=True)
    bits = g.view(np.uint32)[..., 23]
    row["pixels_with_a_ratio"] = int((bits & api.LIGHTMAPPED_DIRECTIONAL_APPLIED != 0).sum())
    row["mean_ratio"] = float(g[..., 20:23][bits & api.LIGHTMAPPED_DIRECTIONAL_APPLIED != 0].astype(np.float64).mean()) if row["pixels_with_a_ratio"] else None
    row["directional_over_scalar"] = round(row["render_lightmapped_directional"]["median_ms"] / row["render_lightmapped"]["median_ms"], 3)
    emit(row)
    if not row["pixels_with_a_ratio"]:
        raise SystemExit("the view applied no ratio: no charted pixel is visible from any of the cameras tried")
    ctx.close()


if __name__ == "__main__":
    main()
