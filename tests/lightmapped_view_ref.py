"""The lightmapped view (lupin_hip_render_lightmapped) restated in numpy float32: steps 5 to 9 of the contract
in include/lupin_hip.h as a PURE FUNCTION of the pieces tests/baked_view_ref.py gathers for steps 1 to 4 (plus the hit's
barycentrics, which `pieces` here keeps), the scene's texcoord and index arrays (`geometry`), the charts, the atlas and a
lookup function.  Steps 1 to 4 and the f16 store are tests/baked_view_ref.py's.

Every operation is one float32 operation in the order written in the header; numpy's float32 arithmetic rounds each one.

`plant` names a deliberate misreading of the contract (PLANTS); tests/test_lightmapped_view_cpu.py shows each of them failing."""
from types import SimpleNamespace

import numpy as np

from lupinpathtracer_amd import api
from tests import baked_view_ref as B
from tests import lightmap_ref

F = np.float32
GBUFFER_FLOATS = 20
MISS, LIGHTMAP, PROBES, AMBIENT = 0, 1, 2, 3
NO_CHART = np.uint32(0xFFFFFFFF)
PLANTS = ("no_half_texel", "v_flipped", "unowned_counted", "no_renormalisation", "nearest_when_uncovered", "wrap", "last_chart", "fused_texcoords",
          "ambient_despite_probes", "offset_then_scale")


def pieces(camera_probe, trace_rays, surface_probe, W, H, camera_params, camera_transform, ray_epsilon):
    """baked_view_ref.pieces, and the hits' barycentrics as `uv` (n, 2)."""
    kept = {}

    def tracing(o, d, eps):
        got = trace_rays(o, d, eps)
        kept["uv"] = np.asarray(got[2], F).reshape(-1, 2)
        return got

    px = B.pieces(camera_probe, tracing, surface_probe, W, H, camera_params, camera_transform, ray_epsilon)
    px.uv = kept["uv"]
    return px


def geometry(cpu, scene):
    """What step 6 reads of the SceneCPU `cpu` uploaded as `scene`: per instance its mesh, per mesh its (T, 3) vertex ids in
    the scene's own triangle order and its (n, 2) texcoords (None where the mesh has none)."""
    tris = lightmap_ref.mesh_triangles(scene)
    uvs = []
    for info in cpu.mesh_infos:
        k = int(info["texcoords_buf_idx"])
        uvs.append(np.asarray(cpu.verts_texcoord_array[k], F).reshape(-1, 2) if k < len(cpu.verts_texcoord_array) else None)
    return SimpleNamespace(mesh_of=np.array([int(i["mesh_idx"]) for i in scene.instances], np.int64), tris=tris, uvs=uvs)


def chart_of_instance(charts, n_instances, plant=None):
    """Step 5: per instance the chart of lowest index that names it, or NO_CHART."""
    out = np.full(n_instances, NO_CHART, np.uint32)
    for c, ch in enumerate(charts):
        if plant == "last_chart" or out[ch.instance_idx] == NO_CHART:
            out[ch.instance_idx] = c
    return out


def atlas_coordinates(px, geo, charts, W, H, plant=None):
    """Steps 5 and 6: (chart (n,) uint32 with NO_CHART where uncharted, x (n,), y (n,)) float32; x = y = 0 where uncharted."""
    n = len(px.hit)
    chart = np.full(n, NO_CHART, np.uint32)
    x, y = np.zeros(n, F), np.zeros(n, F)
    table = chart_of_instance(charts, len(geo.mesh_of), plant)
    one, half = F(1.0), F(0.5)
    for k in np.nonzero(px.hit)[0]:
        c = table[int(px.inst[k])]
        if c == NO_CHART:
            continue
        m = geo.mesh_of[int(px.inst[k])]
        a, b, cc = geo.uvs[m][geo.tris[m][int(px.tri[k])]]
        u, v = F(px.uv[k, 0]), F(px.uv[k, 1])
        ch = charts[int(c)]
        with np.errstate(all="ignore"):
            w = one - u - v
            if plant == "fused_texcoords":       # the products unrounded: one rounding for the whole sum
                t = (a.astype(np.float64) * np.float64(w) + b.astype(np.float64) * np.float64(u) + cc.astype(np.float64) * np.float64(v)).astype(F)
            else:
                t = a * w + b * u + cc * v
            if plant == "offset_then_scale":
                au, av = (t[0] + F(ch.offset_u)) * F(ch.scale_u), (t[1] + F(ch.offset_v)) * F(ch.scale_v)
            else:
                au, av = t[0] * F(ch.scale_u) + F(ch.offset_u), t[1] * F(ch.scale_v) + F(ch.offset_v)
            if plant == "v_flipped":
                av = one - av
            shift = F(0.0) if plant == "no_half_texel" else half
            cx, cy = au * F(W) - shift, av * F(H) - shift
        if np.isfinite(cx) and np.isfinite(cy):
            chart[k], x[k], y[k] = c, cx, cy
    return chart, x, y


def _axis(x, size, plant):
    if plant == "wrap":
        fl = np.floor(x)
        i0 = np.mod(fl, F(size)).astype(np.int64)
        return i0, np.mod(i0 + 1, size), (x - fl).astype(F)
    xf = np.minimum(np.maximum(x, F(0.0)), F(size - 1))          # clamped in float before any conversion to integer
    fl = np.floor(xf)
    i0 = fl.astype(np.int64)
    return i0, np.minimum(i0 + 1, size - 1), (xf - fl).astype(F)


def fetch(atlas, x, y, plant=None):
    """Step 7 at finite coordinates x, y (m,): (E (m, 3), cov (m,)) float32 from the (H, W, 4) atlas."""
    atlas = np.asarray(atlas, F)
    H, W = atlas.shape[:2]
    x0, x1, fx = _axis(np.asarray(x, F), W, plant)
    y0, y1, fy = _axis(np.asarray(y, F), H, plant)
    one = F(1.0)
    with np.errstate(all="ignore"):
        gx, gy = one - fx, one - fy
        weights = (gx * gy, fx * gy, gx * fy, fx * fy)                          # taps 00, 10, 01, 11
        taps = (atlas[y0, x0], atlas[y0, x1], atlas[y1, x0], atlas[y1, x1])
        cov = np.zeros(len(x0), F)
        owned_sum, plain_sum = np.zeros((len(x0), 3), F), np.zeros((len(x0), 3), F)
        for wt, t in zip(weights, taps):
            term = wt[:, None] * t[:, 0:3]
            plain_sum = plain_sum + term
            owned = np.ones(len(x0), bool) if plant == "unowned_counted" else t[:, 3] != 0
            cov = np.where(owned, cov + wt, cov)
            owned_sum = np.where(owned[:, None], owned_sum + term, owned_sum)      # a tap that is not owned enters neither sum
        covered = cov > 0
        E = owned_sum if plant == "no_renormalisation" else owned_sum / np.where(covered, cov, one)[:, None]
        uncovered = plain_sum
        if plant == "nearest_when_uncovered":
            uncovered = atlas[np.where(fy < F(0.5), y0, y1), np.where(fx < F(0.5), x0, x1), 0:3]
        E = np.where(covered[:, None], E, uncovered).astype(F)
    return E, cov


def compose(px, geo, charts, atlas, lookup, ambient, plant=None):
    """Steps 5 to 9: (rgb (n, 3) float32, gbuffer (n, 20) float32).  `px` as `pieces` returns it; `geo` as `geometry`;
    `charts` LightmapChart items; `atlas` (H, W, 4); lookup(records (m, 8)) -> (m, 4) or None for no volume; `ambient` three
    numbers."""
    assert plant is None or plant in PLANTS
    atlas = np.asarray(atlas, F)
    amb = np.asarray(ambient, F).reshape(3)
    n_px = len(px.hit)
    hit = px.hit
    chart, x, y = atlas_coordinates(px, geo, charts, atlas.shape[1], atlas.shape[0], plant)
    charted = hit & (chart != NO_CHART)
    # the uncharted hits (and the G-buffer's first 16 words of every pixel) are the baked-lighting view's
    asks = lookup is not None and plant != "ambient_despite_probes"
    uncharted = SimpleNamespace(**vars(px))
    uncharted.hit = hit & ~charted
    asked = []

    def counted(rec):
        asked.append(len(rec))
        return lookup(rec)

    rgb_u, g_u = B.compose(uncharted, counted if asks else (lambda rec: np.zeros((len(rec), 4), F)), amb)
    _, g16 = B.compose(px, lambda rec: np.zeros((len(rec), 4), F), amb)
    E = np.broadcast_to(amb, (n_px, 3)).copy()
    source = np.where(hit, AMBIENT, MISS).astype(np.uint32)
    w = g_u[:, 11].copy()
    source[uncharted.hit & (w != 0)] = PROBES
    if charted.any():
        E[charted], w[charted] = fetch(atlas, x[charted], y[charted], plant)
        source[charted] = LIGHTMAP
    with np.errstate(all="ignore"):
        lit = px.emission + (px.color * E) * B.INV_PI
    rgb = np.where(charted[:, None], lit, rgb_u).astype(F)
    rgb[~hit] = px.env[~hit]
    g = np.zeros((n_px, GBUFFER_FLOATS), F)
    gw = g.view(np.uint32)
    g[:, 0:16] = g16
    g[:, 11], g[:, 16], g[:, 17] = w, x, y
    gw[:, 18], gw[:, 19] = chart, source
    return rgb, g


def render(px, geo, charts, atlas, lookup, ambient, mode=B.film_ref.RTZ, plant=None):
    """(texels (n, 4) uint16, gbuffer (n, 20) float32) of the whole contract from the pieces."""
    rgb, g = compose(px, geo, charts, atlas, lookup, ambient, plant)
    return B.texels(rgb, mode), g
