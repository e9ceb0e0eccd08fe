"""The baked-lighting view (lupin_hip_render_baked) restated in numpy float32: steps 3 to 7 of the contract in
include/lupin_hip.h as a PURE FUNCTION of a pixel's ray, hit, normals, material, environment radiance and the lookup's
answer.  Steps 1 and 2 and the surface are not restated here: `pieces` collects them from whoever computes them -- the
oracle's camera, closest-hit and surface restatements on the CPU, the device's own probes on the GPU -- and the lookup is
tests/probe_grid_ref.py's or tests/probe_depth_ref.py's sample (CPU) or the device's own entry points (GPU), handed in as a
function of records.

Every operation is one float32 operation in the order written in the header; numpy's float32 arithmetic rounds each one.
The f16 store is done on the bit layout, by tests/film_ref.py's round_to_half on the float32 value widened exactly.

`plant` names a deliberate misreading of the contract (PLANTS); tests/test_baked_view_cpu.py shows each of them failing."""
from types import SimpleNamespace

import numpy as np

from lupinpathtracer_amd import api
from tests import film_ref

F = np.float32
INV_PI = F(0.31830988)
UNIT_TOLERANCE = F(1e-4)
MISS = np.uint32(0xFFFFFFFF)
GBUFFER_FLOATS = 16
PLANTS = ("no_flip", "no_inv_pi", "ambient_when_answered", "ambient_on_miss", "no_emission", "contracted_p", "flip_by_geometric_normal")


def pixels(W, H):
    """(gx, gy) of every pixel in the G-buffer's order: row-major, row 0 first."""
    gy, gx = np.divmod(np.arange(W * H, dtype=np.uint32), np.uint32(W))
    return gx, gy


def pieces(camera_probe, trace_rays, surface_probe, W, H, camera_params, camera_transform, ray_epsilon):
    """Steps 1 and 2 and the surface of every pixel, from three functions with the signatures of api.camera_probe (without
    the context), api.trace_rays and api.surface_probe (without context and scene).  Returns a namespace of arrays in pixel
    order: o, d, hit (bool), dst, inst, tri, ns, ng, color, emission, env."""
    gx, gy = pixels(W, H)
    o, d, _ = camera_probe(W, H, camera_params, camera_transform, api.camera_records(gx, gy, 0, api.CameraMode.RAY_CENTRE))
    hit, dst, uv, inst, tri = trace_rays(o, d, ray_epsilon)
    hit = hit != 0
    n = W * H
    ns, ng, color, emission = (np.zeros((n, 3), F) for _ in range(4))
    if hit.any():
        nrm = surface_probe(api.surface_records(api.SurfaceMode.NORMAL, inst[hit], tri[hit], uv[hit]))
        mat = surface_probe(api.surface_records(api.SurfaceMode.MATERIAL, inst[hit], tri[hit], uv[hit]))
        ns[hit], ng[hit], color[hit], emission[hit] = nrm[:, 0:3], nrm[:, 3:6], mat[:, 4:7], mat[:, 1:4]
    env = surface_probe(api.surface_records(api.SurfaceMode.ENVIRONMENT, direction=d))[:, 0:3]
    return SimpleNamespace(o=o, d=d, hit=hit, dst=dst, inst=inst, tri=tri, ns=ns, ng=ng, color=color, emission=emission, env=env)


def record_ok(p, n):
    """The lookups' own look at a record (ray_record_ok): finite p and n, and | |n|^2 - 1 | <= 1e-4 in float32."""
    with np.errstate(all="ignore"):
        off = ((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]) - F(1.0)
        return np.isfinite(p).all(axis=1) & np.isfinite(n).all(axis=1) & (off <= UNIT_TOLERANCE) & (off >= -UNIT_TOLERANCE)


def compose(px, lookup, ambient, plant=None):
    """Steps 3 to 6: (rgb (n, 3) float32, gbuffer (n, 16) float32).  `px` as `pieces` returns it; lookup(records (m, 8)) ->
    (m, 4), the chosen lookup over the records of the pixels that ask it; `ambient` three numbers."""
    assert plant is None or plant in PLANTS
    o, d, hit = px.o.astype(F), px.d.astype(F), px.hit
    dst = np.where(hit, px.dst, F(0.0)).astype(F)
    amb = np.asarray(ambient, F).reshape(3)
    n_px = len(o)
    with np.errstate(all="ignore"):
        if plant == "contracted_p":
            p = (d.astype(np.float64) * dst[:, None].astype(np.float64) + o.astype(np.float64)).astype(F)   # one rounding: an fma
        else:
            p = o + d * dst[:, None]
        toward = px.ng if plant == "flip_by_geometric_normal" else px.ns
        c = (d[:, 0] * toward[:, 0] + d[:, 1] * toward[:, 1]) + d[:, 2] * toward[:, 2]
        flip = np.zeros(n_px, bool) if plant == "no_flip" else c > 0
        n = np.where(flip[:, None], -px.ns, px.ns).astype(F)
        ask = hit & record_ok(p, n)
        rec = np.zeros((int(ask.sum()), api.PROBE_GRID_RECORD_FLOATS), F)
        rec[:, 0:3], rec[:, 4:7] = p[ask], n[ask]
        E = np.broadcast_to(amb, (n_px, 3)).copy()
        w = np.zeros(n_px, F)
        if len(rec):
            res = np.asarray(lookup(rec), F)
            answered = res[:, 3] != 0
            w[ask] = np.where(answered, res[:, 3], F(0.0))
            if plant != "ambient_when_answered":
                idx = np.nonzero(ask)[0][answered]
                E[idx] = res[answered, 0:3]
        scale = F(1.0) if plant == "no_inv_pi" else INV_PI
        emission = np.zeros_like(px.emission) if plant == "no_emission" else px.emission
        lit = emission + (px.color * E) * scale
        missed = np.broadcast_to(amb, (n_px, 3)) if plant == "ambient_on_miss" else px.env
        rgb = np.where(hit[:, None], lit, missed).astype(F)
    g = np.zeros((n_px, GBUFFER_FLOATS), F)
    gw = g.view(np.uint32)
    g[hit, 0:3], g[hit, 4:7], g[hit, 8:11], g[hit, 12:15], g[hit, 15] = p[hit], n[hit], px.color[hit], px.emission[hit], dst[hit]
    gw[:, 3] = np.where(hit, px.inst, MISS)
    gw[hit, 7] = px.tri[hit]
    g[:, 11] = w
    g[~hit, 12:15] = px.env[~hit]
    return rgb, g


def texels(rgb, mode):
    """Step 7: (n, 4) uint16 words of `rgb` (n, 3) float32 stored as Rgba16Float under film_ref.RTZ or film_ref.RNE, alpha 1.0."""
    out = np.empty((len(rgb), 4), np.uint16)
    out[:, 0:3] = film_ref.round_to_half(np.asarray(rgb, F).astype(np.float64), mode)
    out[:, 3] = film_ref.ALPHA_ONE
    return out


def render(px, lookup, ambient, mode=film_ref.RTZ, plant=None):
    """(texels (n, 4) uint16, gbuffer (n, 16) float32) of the whole contract from the pieces."""
    rgb, g = compose(px, lookup, ambient, plant)
    return texels(rgb, mode), g
