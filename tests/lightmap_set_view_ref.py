"""The lightmapped view with lightmap UV sets, restated on top of tests/lightmapped_view_ref.py.

Step 6 of the view reads, for a hit on triangle t of a mesh with a set, the three corners lm_uvs[3 t + k] in place of
texcoords[index_k], and interpolates them with the same weights in the same order.  A per-corner set is therefore a texcoord
array of 3 T entries read through the indices (3 t, 3 t + 1, 3 t + 2): `geometry` hands lightmapped_view_ref exactly that,
and everything else -- the chart, the fetch, the shading, the albedo the surface probe took from the MATERIAL texcoords --
is lightmapped_view_ref's, unchanged."""
import numpy as np

from tests import lightmapped_view_ref as L

F = np.float32


def geometry(cpu, scene, sets):
    """lightmapped_view_ref.geometry with the meshes of `sets` ({mesh index: (T, 3, 2) or (3 T, 2) lightmap UVs}) reading
    their set per corner; a mesh that is not in `sets` reads its texcoords as before."""
    geo = L.geometry(cpu, scene)
    for m, uvs in sets.items():
        uvs = np.asarray(uvs, F).reshape(-1, 2)
        assert len(uvs) == 3 * len(geo.tris[m]), "one UV per triangle corner"
        geo.uvs[m] = uvs
        geo.tris[m] = np.arange(len(uvs), dtype=np.int64).reshape(-1, 3)
    return geo


def corner_interpolation(px, geo, sets):
    """Per pixel the per-corner interpolation a * w + b * u + c * v of the hit mesh's set (NaN where the pixel misses or its
    mesh has no set): what G-buffer words 16..17 hold before the chart's scale and offset and the atlas' size."""
    out = np.full((len(px.hit), 2), np.nan, F)
    for k in np.nonzero(px.hit)[0]:
        m = int(geo.mesh_of[int(px.inst[k])])
        if m not in sets:
            continue
        a, b, c = np.asarray(sets[m], F).reshape(-1, 3, 2)[int(px.tri[k])]
        u, v = F(px.uv[k, 0]), F(px.uv[k, 1])
        w = F(1.0) - u - v
        out[k] = a * w + b * u + c * v
    return out
