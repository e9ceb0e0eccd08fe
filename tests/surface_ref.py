"""float64 restatement of what runs between a hit and the scattering functions: texture lookup (the ideal bilinear filter with
Repeat addressing of a linear / Repeat sampler: texel centres at (i + 0.5) / n, exact weights), the sRGB decode with a true
pow, get_material_point, get_vert_color, get_vert_normal, compute_tri_geom_normal, compute_tangents_from_uv,
compute_shading_normal, dir_to_env_uv and sample_environments.  Written from pathtracer.wgsl (:1265-1416, :1699-1770,
:2561-2587, :2729-2736) and the sampler description; nothing here is shared with the device code or the oracle.

Inputs are the loader's SceneCPU, the textures, the index buffers in the order the BLAS build left them (the triangle numbering
of a hit) and the float32 fields of a record taken as exact numbers.  Plain Python floats are IEEE doubles.

Beside each value stands its CONDITIONING: a number c such that an evaluation in float32 that rounds every operation once
is within about c * 2^-24 of the exact value (first order; the tests multiply by one measured constant per mode).  The
terms are the ones a forward error analysis gives:
  texture       the variation of the filtered texture over the rounding of u * w - 0.5 (grows with |u|; the whole range of the
                texture once that rounding reaches half a texel), plus the weighted sum of |texel| for the lerps
  sRGB          the decode's derivative times the sample's term; the jump of the two branches when the sample is within its
                own error of 0.04045
  products      first-order propagation
  density       the colour's term / (c * tr_depth): this is 1 / (c |log c|) relative to the density, large near c = 1
  normals       sum of |terms| / length of the interpolated normal; 1 / sin of the triangle's corner for the cross product;
                |N| |v| / |N v| for the normal matrix
  normal map    (|sx ty| + |sy tx|) / |div| and the tangent numerators' cancellation; 1 / sin(tangent, normal) for the
                orthonormalisation
  environment   1 / distance from the poles for u and v
and the EXCLUSION rules (a query to which one applies is reported in `excluded` and not compared; nothing else may be):
  E1  roughness of a type that snaps to zero below MIN_ROUGHNESS, within its own error of MIN_ROUGHNESS (a discontinuity)
  E2  a nonzero div below the rounding of its two products (float32 may compute exactly 0 and take the fallback)
  E3  |dot(frame[1], bitangent)| < FLIP_MIN: the bitangent flip is a discontinuity
  E4  environment direction within POLE_MIN (sine of the polar angle) of a pole
  E5  environment direction within its own error of the u seam: u jumps between 0 and 1 (the uv outputs only)
  E6  a zero-length interpolated normal, triangle normal or tangent (the result is NaN by definition)
  E7  sin(tangent, normal) < FLIP_MIN: the orthonormalised tangent is 0 / 0"""
import math

import numpy as np

EPS = 2.0 ** -24
SENTINEL = 0xFFFFFFFF
MIN_ROUGHNESS = float(np.float32(0.03) * np.float32(0.03))   # the f32 constant of pathtracer.wgsl:1262
FLIP_MIN = 1e-3
POLE_MIN = 1e-3
MATTE, GLOSSY, REFLECTIVE, TRANSPARENT, REFRACTIVE, SUBSURFACE, VOLUMETRIC, GLTFPBR = range(8)   # renderer.rs:126-139
CUT = float(np.float32(0.04045))


def _f(x):
    return float(x)


# ------------------------------------------------------------------------------------------------ textures
class Tex:
    def __init__(self, pixels):
        px = np.asarray(pixels)
        self.h, self.w = px.shape[0], px.shape[1]
        t = px.astype(np.float64)
        if px.dtype == np.uint8:
            t = t / 255.0
        self.t = t                # float64 [h][w][4]; bilinear takes its four taps out as Python floats
        fin = np.where(np.isfinite(t), t, 0.0)
        self.range = (fin.reshape(-1, 4).max(0) - fin.reshape(-1, 4).min(0)).tolist()

    def bilinear(self, x, y):
        """ideal filter at continuous texel coordinates (x = u * w - 0.5): value[4], sum of weight * |texel| [4]"""
        x0, y0 = math.floor(x), math.floor(y)
        fx, fy = x - x0, y - y0
        xa, ya = x0 % self.w, y0 % self.h
        xb, yb = (xa + 1) % self.w, (ya + 1) % self.h
        t = self.t
        taps = ((t[ya, xa].tolist(), (1 - fx) * (1 - fy)), (t[ya, xb].tolist(), fx * (1 - fy)), (t[yb, xa].tolist(), (1 - fx) * fy), (t[yb, xb].tolist(), fx * fy))
        val = [sum(p[c] * wgt for p, wgt in taps) for c in range(4)]
        mag = [sum(abs(p[c]) * wgt for p, wgt in taps) for c in range(4)]
        return val, mag

    def sample(self, u, v, du=0.0, dv=0.0):
        """sample_texture at (u, v); du, dv: conditioning of the coordinates themselves (error <= du * 2^-24).
        Returns value[4], conditioning[4]."""
        x, y = u * self.w - 0.5, v * self.h - 0.5
        val, mag = self.bilinear(x, y)
        cond = list(mag)
        for axis in (0, 1):
            n = self.w if axis == 0 else self.h
            c, dc = (x, du) if axis == 0 else (y, dv)
            e = abs(c + 0.5) + abs(c) + 1.0 + dc * n     # u * w, the subtraction, the coordinate's own error in texels
            step = 4.0 * EPS * e
            if step < 0.5:
                hi = self.bilinear(x + step, y)[0] if axis == 0 else self.bilinear(x, y + step)[0]
                lo = self.bilinear(x - step, y)[0] if axis == 0 else self.bilinear(x, y - step)[0]
                for ch in range(4):
                    cond[ch] += max(abs(hi[ch] - val[ch]), abs(lo[ch] - val[ch])) / (4.0 * EPS)
            else:
                for ch in range(4):
                    cond[ch] += self.range[ch] / EPS
        return val, cond


def srgb_to_linear(s, cs, true_pow=True):
    """vec3f_srgb_to_linear on one channel: value, conditioning (cs: the sample's)."""
    lower = s / 12.92
    base = (s + 0.055) / 1.055
    higher = math.pow(base, 2.4) if base > 0 else 0.0
    if s < CUT:
        val, der = lower, 1.0 / 12.92
    else:
        val, der = higher, 2.4 / 1.055 * math.pow(base, 1.4)
    cond = der * cs + 8.0 * abs(val)
    if abs(s - CUT) <= 4.0 * EPS * cs:
        cond += abs(higher - lower) / EPS
    return val, cond


# ------------------------------------------------------------------------------------------------ scene access
class SurfaceRef:
    def __init__(self, scene_cpu, textures, indices):
        """indices: per mesh, the index buffer in BLAS leaf order (what a hit's triangle index counts in)."""
        self.s = scene_cpu
        self.tex = [Tex(t.pixels if hasattr(t, "pixels") else t) for t in textures]
        self.idx = [np.asarray(i, np.int64) for i in indices]

    def _tri(self, inst, tri):
        ins = self.s.instances[inst]
        mesh = int(ins["mesh_idx"])
        i = self.idx[mesh][tri * 3:tri * 3 + 3]
        return ins, mesh, self.s.mesh_infos[mesh], self.s.materials[int(ins["mat_idx"])], [int(k) for k in i]

    def _attr(self, arr, buf, ids, n):
        return [[_f(arr[buf][k][c]) for c in range(n)] for k in ids]

    @staticmethod
    def _interp(vals, bu, bv):
        """a * w + b * u + c * v: value per component, conditioning per component"""
        w = 1.0 - bu - bv
        ws = (w, bu, bv)
        wmag = (1.0 + abs(bu) + abs(bv), abs(bu), abs(bv))
        n = len(vals[0])
        val = [sum(vals[k][c] * ws[k] for k in range(3)) for c in range(n)]
        cond = [4.0 * sum(abs(vals[k][c]) * wmag[k] for k in range(3)) for c in range(n)]
        return val, cond

    def texcoords(self, inst, tri, bu, bv):
        ins, mesh, info, mat, ids = self._tri(inst, tri)
        uv = self._attr(self.s.verts_texcoord_array, int(info["texcoords_buf_idx"]), ids, 2)
        return self._interp(uv, bu, bv), uv

    def vertex_color(self, inst, tri, bu, bv):
        ins, mesh, info, mat, ids = self._tri(inst, tri)
        if int(info["colors_buf_idx"]) == SENTINEL:
            return [1.0] * 4, [0.0] * 4
        return self._interp(self._attr(self.s.verts_color_array, int(info["colors_buf_idx"]), ids, 4), bu, bv)

    # -------------------------------------------------------------------------------------------- material point
    def material_point(self, inst, tri, bu, bv, variant=None):
        """get_material_point.  Returns (values, conditioning, excluded): dicts keyed like the probe's fields; `excluded` a
        set of field names under rule E1.  `variant` names a deliberately wrong reading (the tests' twins)."""
        ins, mesh, info, mat, ids = self._tri(inst, tri)
        mtype = int(mat["mat_type"])
        color_s, color_c = [1.0] * 4, [0.0] * 4
        emis_s, emis_c = [1.0] * 3, [0.0] * 3
        rough_s, rough_c, metal_s, metal_c = 1.0, 0.0, 1.0, 0.0
        scat_s, scat_c = [1.0] * 3, [0.0] * 3
        has_uv = int(info["texcoords_buf_idx"]) != SENTINEL
        if variant == "texture_without_texcoords":
            has_uv = True
        if has_uv:
            if int(info["texcoords_buf_idx"]) != SENTINEL:
                (tc, tcc), _ = self.texcoords(inst, tri, bu, bv)
            else:
                tc, tcc = [0.0, 0.0], [0.0, 0.0]

            def look(key):
                return self.tex[int(mat[key])].sample(tc[0], tc[1], tcc[0], tcc[1])
            if int(mat["color_tex_idx"]) != SENTINEL:
                t, c = look("color_tex_idx")
                for ch in range(3):
                    color_s[ch], color_c[ch] = (t[ch], c[ch]) if variant == "no_srgb_decode" else srgb_to_linear(t[ch], c[ch])
                color_s[3], color_c[3] = srgb_to_linear(t[3], c[3]) if variant == "alpha_decoded" else (t[3], c[3])
            if int(mat["emission_tex_idx"]) != SENTINEL:
                t, c = look("emission_tex_idx")
                for ch in range(3):
                    emis_s[ch], emis_c[ch] = srgb_to_linear(t[ch], c[ch]) if variant == "emission_decoded" else (t[ch], c[ch])
            if int(mat["roughness_tex_idx"]) != SENTINEL:
                t, c = look("roughness_tex_idx")
                gi, bi = (0, 1) if variant == "roughness_from_r" else (1, 2)
                rough_s, rough_c, metal_s, metal_c = t[gi], c[gi], t[bi], c[bi]
            if int(mat["scattering_tex_idx"]) != SENTINEL:
                t, c = look("scattering_tex_idx")
                scat_s, scat_c = t[:3], c[:3]
        vc, vcc = self.vertex_color(inst, tri, bu, bv)
        if variant == "vertex_color_default_zero" and int(info["colors_buf_idx"]) == SENTINEL:
            vc = [0.0] * 4
        mc = [_f(x) for x in mat["color"]]
        val, cond, excl = {}, {}, set()
        val["type"] = mtype
        col = [color_s[c] * mc[c] * vc[c] for c in range(4)]
        colc = [color_c[c] * abs(mc[c] * vc[c]) + abs(color_s[c] * mc[c]) * vcc[c] + 2.0 * abs(col[c]) for c in range(4)]
        val["color"], cond["color"] = col[:3], colc[:3]
        val["opacity"], cond["opacity"] = col[3], colc[3]
        me = [_f(x) for x in mat["emission"]][:3]
        val["emission"] = [emis_s[c] * me[c] for c in range(3)]
        cond["emission"] = [emis_c[c] * abs(me[c]) + abs(val["emission"][c]) for c in range(3)]
        mr = _f(mat["roughness"])
        rg = rough_s * mr
        rgc = rough_c * abs(mr) + abs(rg)
        r = rg if variant == "roughness_not_squared" else rg * rg
        rc = 2.0 * abs(rg) * rgc + abs(r)
        clamp_types = (MATTE, GLTFPBR, GLOSSY)
        if variant == "clamp_every_type":
            clamp_types = tuple(range(8))
        if mtype in clamp_types:
            r = min(max(r, MIN_ROUGHNESS), 1.0)
        elif mtype == VOLUMETRIC:
            r, rc = 0.0, 0.0
        else:
            if abs(r - MIN_ROUGHNESS) <= 4.0 * EPS * rc:
                excl.add("roughness")   # E1
            if r < MIN_ROUGHNESS:
                r = 0.0
        val["roughness"], cond["roughness"] = r, rc
        val["metallic"] = metal_s * _f(mat["metallic"])
        cond["metallic"] = metal_c * abs(_f(mat["metallic"])) + abs(val["metallic"])
        val["ior"], cond["ior"] = _f(mat["ior"]), 0.0
        dens, densc = [0.0] * 3, [0.0] * 3
        dens_types = (REFRACTIVE, VOLUMETRIC, SUBSURFACE)
        if variant == "density_every_type":
            dens_types = tuple(range(8))
        if mtype in dens_types:
            trd = _f(mat["tr_depth"])
            src = [color_s[c] * mc[c] for c in range(3)] if variant == "density_before_vertex_color" else col
            for c in range(3):
                cc = min(max(src[c], float(np.float32(0.0001))), 1.0)
                dens[c] = -math.log(cc) / trd
                densc[c] = (colc[c] / cc + 4.0 * abs(math.log(cc)) + 2.0) / abs(trd) + 2.0 * abs(dens[c])
        val["density"], cond["density"] = dens, densc
        ms = [_f(x) for x in mat["scattering"]][:3]
        val["scattering"] = [scat_s[c] * ms[c] for c in range(3)]
        cond["scattering"] = [scat_c[c] * abs(ms[c]) + abs(val["scattering"][c]) for c in range(3)]
        val["anisotropy"], cond["anisotropy"] = _f(mat["sc_anisotropy"]), 0.0
        return val, cond, excl

    # -------------------------------------------------------------------------------------------- normals
    def normal_matrix(self, inst, forward=False):
        """columns transform[0].xyz, transform[1].xyz, transform[2].xyz of transpose_inverse_transform (:1748-1750);
        forward=True: the local -> world matrix instead (a wrong reading, for the twin of property 3)"""
        t = np.asarray(self.s.instances[inst]["transpose_inverse_transform"], np.float64).reshape(3, 4)
        n = t[:, :3].T   # matrix whose columns are the rows t[i, :3]
        if forward:
            n = np.linalg.inv(t[:, :3])   # rows of t = world -> local; its inverse carries local -> world
        return n

    @staticmethod
    def _apply(nm, v, vc):
        """normalize(N v): value, conditioning (vector norm), ok"""
        r = nm @ np.asarray(v)
        length = float(np.linalg.norm(r))
        if length == 0.0 or not math.isfinite(length):
            return [math.nan] * 3, math.inf, False
        kappa = float(np.linalg.norm(np.abs(nm) @ np.abs(np.asarray(v)))) / length
        return (r / length).tolist(), kappa * (vc + 4.0) + 4.0, True

    def _positions(self, inst, tri):
        ins, mesh, info, mat, ids = self._tri(inst, tri)
        return [[_f(self.s.verts_pos_array[mesh][k][c]) for c in range(3)] for k in ids]

    def geometric_normal(self, inst, tri, variant=None):
        p = np.asarray(self._positions(inst, tri))
        a, b = p[2] - p[0], p[1] - p[0]
        if variant == "cross_v1_v2":
            a, b = b, a
        cr = np.cross(a, b)
        length = float(np.linalg.norm(cr))
        if length == 0.0:
            return [math.nan] * 3, math.inf, {"E6"}
        cc = 4.0 * float(np.linalg.norm(a)) * float(np.linalg.norm(b)) / length + 4.0
        val, cond, ok = self._apply(self.normal_matrix(inst), cr / length, cc)
        return val, cond, set() if ok else {"E6"}

    def vertex_normal(self, inst, tri, bu, bv):
        ins, mesh, info, mat, ids = self._tri(inst, tri)
        if int(info["normals_buf_idx"]) == SENTINEL:
            return self.geometric_normal(inst, tri)
        nv, nc = self._interp(self._attr(self.s.verts_normal_array, int(info["normals_buf_idx"]), ids, 3), bu, bv)
        length = math.sqrt(sum(x * x for x in nv))
        if length == 0.0:
            return [math.nan] * 3, math.inf, {"E6"}
        cc = math.sqrt(sum(x * x for x in nc)) / length + 4.0
        val, cond, ok = self._apply(self.normal_matrix(inst), [x / length for x in nv], cc)
        return val, cond, set() if ok else {"E6"}

    def shading_normal(self, inst, tri, bu, bv, variant=None):
        """compute_shading_normal: value[3], conditioning (one number for the vector), set of exclusion rules that apply"""
        ins, mesh, info, mat, ids = self._tri(inst, tri)
        res, resc, excl = self.vertex_normal(inst, tri, bu, bv)
        if excl or int(info["texcoords_buf_idx"]) == SENTINEL or int(mat["normal_tex_idx"]) == SENTINEL:
            return res, resc, excl
        (tc, tcc), uv = self.texcoords(inst, tri, bu, bv)
        pos = np.asarray(self._positions(inst, tri))
        p, q = pos[1] - pos[0], pos[2] - pos[0]
        sx, sy = uv[1][0] - uv[0][0], uv[2][0] - uv[0][0]
        tx, ty = uv[1][1] - uv[0][1], uv[2][1] - uv[0][1]
        div = sx * ty - sy * tx
        dmag = abs(sx * ty) + abs(sy * tx)
        tl, bl, tlc, blc = np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), 0.0, 0.0
        if variant == "fallback_frame_swapped":
            tl, bl = bl, tl      # (has an effect only where the fallback is taken)
        if div != 0.0:
            if abs(div) <= 8.0 * EPS * dmag:
                excl.add("E2")
            tl, bl = (ty * p - tx * q) / div, (sx * q - sy * p) / div
            for vec, m1, m2 in ((tl, abs(ty) * np.linalg.norm(p) + abs(tx) * np.linalg.norm(q), 0), (bl, abs(sx) * np.linalg.norm(q) + abs(sy) * np.linalg.norm(p), 1)):
                ln = float(np.linalg.norm(vec)) * abs(div)
                if ln == 0.0:
                    return [math.nan] * 3, math.inf, excl | {"E6"}
                c = 6.0 * float(m1) / ln + 4.0 * dmag / abs(div) + 4.0
                if m2 == 0:
                    tlc = c
                else:
                    blc = c
        nm = self.normal_matrix(inst, forward=(variant == "forward_transform"))
        tg, tgc, ok1 = self._apply(nm, tl, tlc)
        bt, btc, ok2 = self._apply(nm, bl, blc)
        if not (ok1 and ok2):
            return [math.nan] * 3, math.inf, excl | {"E6"}
        ns, nsc = self.tex[int(mat["normal_tex_idx"])].sample(tc[0], tc[1], tcc[0], tcc[1])
        nl = np.array([-1.0 + 2.0 * ns[c] for c in range(3)])
        nlc = math.sqrt(sum((2.0 * nsc[c] + abs(nl[c]) + 1.0) ** 2 for c in range(3)))
        fz, tg, bt = np.asarray(res), np.asarray(tg), np.asarray(bt)
        d = float(tg @ fz)
        fx = tg - fz * d
        sin_tn = float(np.linalg.norm(fx))
        if sin_tn < FLIP_MIN:
            return [math.nan] * 3, math.inf, excl | {"E7"}
        fxc = (2.0 * tgc + 2.0 * resc + 8.0) / sin_tn
        fx = fx / sin_tn
        fy = np.cross(fz, fx)
        fyc = 2.0 * (fxc + resc) + 6.0
        fy = fy / np.linalg.norm(fy)
        flip = float(fy @ bt)
        if abs(flip) < FLIP_MIN:
            excl.add("E3")
        if flip < 0.0:
            nl = -nl if variant != "flip_xy_only" else np.array([-nl[0], -nl[1], nl[2]])
        out = fx * nl[0] + fy * nl[1] + fz * nl[2]
        length = float(np.linalg.norm(out))
        if length == 0.0:
            return [math.nan] * 3, math.inf, excl | {"E6"}
        nlen = float(np.linalg.norm(nl))
        cond = (nlen * (fxc + fyc + resc) + nlc + 6.0 * nlen) / length + 4.0
        return (out / length).tolist(), cond, excl

    # -------------------------------------------------------------------------------------------- environments
    def env_uv(self, env_idx, direction):
        """dir_to_env_uv: (u, v), (cond u, cond v), exclusion rules"""
        m = np.asarray(self.s.environments[env_idx]["transform"], np.float64).reshape(4, 4)
        d = np.asarray([_f(x) for x in direction])
        t = np.array([m[0, :3] @ d, m[1, :3] @ d, m[2, :3] @ d])
        tmag = np.array([np.abs(m[k, :3]) @ np.abs(d) for k in range(3)])
        length = float(np.linalg.norm(t))
        if length == 0.0 or not math.isfinite(length):
            return (math.nan, math.nan), (math.inf, math.inf), {"E6"}
        tc = 4.0 * float(np.linalg.norm(tmag)) / length + 4.0
        t = t / length
        excl = set()
        rho = math.hypot(t[0], t[2])
        if rho < POLE_MIN:
            return (math.nan, math.nan), (math.inf, math.inf), {"E4"}
        ang = math.atan2(t[2], t[0])
        u = ang / (2.0 * math.pi)
        uc = (tc / rho + 4.0) / (2.0 * math.pi) + 2.0
        if abs(ang) * 0.5 / math.pi <= 4.0 * EPS * uc and t[0] > 0:
            excl.add("E5")
        if u < 0.0:
            u += 1.0
        if u > 1.0:
            u -= 1.0
        y = min(max(t[1], -1.0), 1.0)
        v = math.acos(y) / math.pi
        vc = (tc / rho + 4.0) / math.pi + 2.0
        return (u, v), (uc, vc), excl

    def environment_radiance(self, direction):
        """sample_environments: value[3], conditioning[3], uv of environment 0 and its conditioning, exclusion rules"""
        total, totc, excl = [0.0] * 3, [0.0] * 3, set()
        uv0, uvc0 = (0.0, 0.0), (0.0, 0.0)
        for i, env in enumerate(self.s.environments):
            uv, uvc, ex = self.env_uv(i, direction)
            if i == 0:
                uv0, uvc0 = uv, uvc
            excl |= ex
            if ex - {"E5"}:
                return [math.nan] * 3, [math.inf] * 3, uv0, uvc0, excl
            e = [_f(x) for x in env["emission"]][:3]
            ec = [0.0] * 3
            if int(env["emission_tex_idx"]) != SENTINEL:
                t, c = self.tex[int(env["emission_tex_idx"])].sample(uv[0], uv[1], uvc[0], uvc[1])
                ec = [abs(e[k]) * c[k] + abs(e[k] * t[k]) for k in range(3)]
                e = [e[k] * t[k] for k in range(3)]
            for k in range(3):
                total[k] += e[k]
                totc[k] += ec[k] + abs(total[k])
        return total, totc, uv0, uvc0, excl
