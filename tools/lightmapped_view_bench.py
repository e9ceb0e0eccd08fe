"""Time the lightmapped view (lupin_hip_render_lightmapped) against the baked-lighting view it extends.

usage: python tools/lightmapped_view_bench.py [--scene bistro_class] [--sizes 3840x2160,1920x1080] [--atlas 2048] [--dims 16x16x4]
                                              [--resolution 16] [--subsamples 4] [--runs 5] [--warmup 2]
                                              [--out profiles/lightmapped_view_bench.jsonl]
The scene from its camera, one chart per instance whose mesh has texcoords (the charts tile the atlas in a square grid), an
atlas of random radiance with random ownership holes in device memory, no G-buffer.  The grid is tools/baked_view_bench.py's:
`dims` probes over the box of 2^20 surface points seen from the camera, baked depth maps, random coefficients, all in
device memory.  Per image size four cases: the view with no volume, the view with a depth-map volume, and the yardsticks
in the same process, lupin_hip_render_baked untraced and with depth maps.  Every figure is the median (min - max) of `runs`
host-clock times of one call that ends synchronised, after `warmup` calls.
Prints one JSON line per size and appends it to --out.  Needs a HIP device; there is no CPU fallback.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="bistro_class")
    ap.add_argument("--sizes", default="3840x2160,1920x1080")
    ap.add_argument("--atlas", type=int, default=2048)
    ap.add_argument("--dims", default="16x16x4")
    ap.add_argument("--resolution", type=int, default=16)
    ap.add_argument("--subsamples", type=int, default=4)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lightmapped_view_bench.jsonl"))
    args = ap.parse_args()

    from lupinpathtracer_amd import _abi, api
    from oracle import oracle
    from tests import reproject_ref, util
    from tools.occlusion_bench import surface_points
    from tools.probe_grid_bench import device_array

    if api.device_count() < 1:
        raise SystemExit("lightmapped_view_bench needs a HIP device; the product has no CPU fallback")
    ctx = api.Context(0)
    scene, cams = util.load_scene(args.scene, ctx)
    cam = cams[0]
    eps, R, K, A = 0.001, args.resolution, args.subsamples, args.atlas
    dims = tuple(int(x) for x in args.dims.split("x"))
    extent = float(api.scene_world_extent(scene))
    bias = np.float32(api.LIGHTMAP_OFFSET_FRACTION * extent)
    points, _ = surface_points(api, oracle, reproject_ref, ctx, scene, cam, 1 << 20)
    lo, hi = points.min(0), points.max(0)
    origin = lo.astype(np.float32)
    spacing = np.float32([max((hi[k] - lo[k]) / max(1, dims[k] - 1), 1e-3 * extent) for k in range(3)])
    rng = np.random.default_rng(0)
    sh = rng.normal(size=(int(np.prod(dims)), 9, 4)).astype(np.float32)
    _, maps, maxd = api.bake_probe_grid_depth(ctx, scene, origin, spacing, dims, R, K)
    d_sh, d_maps = device_array(api, ctx, sh), device_array(api, ctx, maps)

    # a chart per instance whose mesh has texcoords, the charts in a square grid over the atlas
    n_meshes = int(scene.desc.num_meshes)
    infos = np.frombuffer((C.c_uint8 * (n_meshes * _abi.MESH_INFO_DTYPE.itemsize)).from_address(scene.desc.mesh_infos), _abi.MESH_INFO_DTYPE)
    charted = [i for i, inst in enumerate(scene.instances) if int(infos[int(inst["mesh_idx"])]["texcoords_buf_idx"]) != 0xFFFFFFFF]
    side = max(1, math.ceil(math.sqrt(max(1, len(charted)))))
    charts = (_abi.LightmapChartC * max(1, len(charted)))(*[_abi.LightmapChartC(i, 0.9 / side, 0.9 / side, (k % side) / side, (k // side) / side)
                                                            for k, i in enumerate(charted)])
    atlas = rng.uniform(0.0, 2.0, (A, A, 4)).astype(np.float32)
    atlas[..., 3] = rng.uniform(size=(A, A)) > 0.25
    d_atlas = device_array(api, ctx, atlas)
    lib = _abi.lib()

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

    def report(ms, items):
        med = statistics.median(ms)
        return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "mitems_per_s": round(items / med / 1e3, 2)}

    for size in args.sizes.split(","):
        W, H = (int(x) for x in size.split("x"))
        n = W * H
        target = api.Texture(ctx, W, H)
        row = {"tool": "lightmapped_view_bench", "scene": args.scene, "width": W, "height": H, "atlas": A, "charts": len(charted),
               "instances": len(scene.instances), "dims": list(dims), "resolution": R, "subsamples": K, "max_distance": float(maxd),
               "normal_bias": float(bias), "ray_epsilon": eps, "runs": args.runs, "warmup": args.warmup, "max_slots": api.BAKED_VIEW_DEFAULT_MAX_SLOTS}

        def view_desc():
            d = _abi.BakedViewDescC()
            cp = cam.params
            d.camera_params = _abi.CameraParamsC(1 if cp.is_orthographic else 0, cp.lens, cp.film, cp.aspect, cp.focus, cp.aperture)
            m = np.asarray(cam.transform, np.float32).reshape(4, 3)
            for col in range(4):
                for r in range(3):
                    d.camera_transform.m[col][r] = float(m[col][r])
            d.grid = _abi.ProbeGridDescC((C.c_float * 3)(*origin), (C.c_float * 3)(*spacing), (C.c_uint32 * 3)(*dims), api.PROBE_GRID_BACKFACE, eps, float(bias))
            d.resolution, d.max_distance, d.ray_epsilon, d.flags, d.max_slots = R, float(maxd), eps, api.BAKED_VIEW_DEVICE_POINTERS, 0
            d.ambient = (C.c_float * 3)(0.05, 0.05, 0.05)
            return d

        def lightmapped(volume):
            d = _abi.LightmappedViewDescC(view_desc(), A, A, len(charted), 0)
            return lambda: _abi.check(lib.lupin_hip_render_lightmapped(ctx.handle, scene.handle, target.handle, C.byref(d), charts, C.c_void_p(d_atlas.device_ptr()),
                                                                       C.c_void_p(d_sh.device_ptr()) if volume else None,
                                                                       C.c_void_p(d_maps.device_ptr()) if volume else None, None, None))

        def baked(depth):
            d = view_desc()
            return lambda: _abi.check(lib.lupin_hip_render_baked(ctx.handle, scene.handle, target.handle, C.byref(d), C.c_void_p(d_sh.device_ptr()),
                                                                 C.c_void_p(d_maps.device_ptr()) if depth else None, None, None))

        row["lightmapped_no_volume"] = report(timed(lightmapped(False)), n)
        row["lightmapped_depth"] = report(timed(lightmapped(True)), n)
        row["baked_plain"] = report(timed(baked(False)), n)
        row["baked_depth"] = report(timed(baked(True)), n)
        row["no_volume_over_baked_plain"] = round(row["lightmapped_no_volume"]["median_ms"] / row["baked_plain"]["median_ms"], 4)
        row["depth_over_baked_depth"] = round(row["lightmapped_depth"]["median_ms"] / row["baked_depth"]["median_ms"], 4)
        line = json.dumps(row)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
        del target
    ctx.close()


if __name__ == "__main__":
    main()
