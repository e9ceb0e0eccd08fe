"""float64 numpy restatement of the reference's scattering functions: BSDF sample / eval / pdf, the delta lobes, the
Henyey-Greenstein phase function and the homogeneous-medium distance sampler (pathtracer.wgsl:1433-1560 Fresnel and
GGX, :1789-1949 sampling, :1951-2095 evaluation, :2097-2229 pdfs, :2231-2422 delta lobes and media, :2424-2463 frames).

It is written from the formulas those lines implement, not from oracle/ or the HIP code, so that a mistake shared by
those two shows up here.  Where the algebra allows, it takes a different route to the same value (the conductor
Fresnel term with zero extinction is evaluated as the dielectric one, the microfacet Jacobians are written out from
Walter et al. 2007).  Every function is vectorised over a leading axis: vectors are (n, 3), scalars (n,).

`refraction_jacobian` selects the transmission Jacobian of the rough refractive pdf:
  "reference"  |h.i| / (eta_rel (h.i) + (h.o))^2          what :2167-2192 computes
  "walter"     eta_rel^2 |h.i| / (eta_rel (h.i) + (h.o))^2  Walter et al. 2007, eq. 17, with eta_i / eta_o = eta_rel
The tests pin the reference's form and show that the textbook one would fail the same test."""
import numpy as np

PI = np.pi
MATTE, GLOSSY, REFLECTIVE, TRANSPARENT, REFRACTIVE, SUBSURFACE, VOLUMETRIC, GLTFPBR = range(8)
F32_MAX = float(np.finfo(np.float32).max)


def dot(a, b):
    return np.sum(a * b, axis=-1)


def normalize(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def col(s):
    return np.asarray(s, np.float64)[..., None]


def reflect(w, n):
    """Mirror w about n (both pointing away from the surface), :2439-2442."""
    return -w + 2.0 * col(dot(n, w)) * n


def refract(w, n, inv_eta):
    """Snell refraction of w (pointing away) through the plane with normal n, eta_o / eta_i = inv_eta; zero on total
    internal reflection (:2444-2450).  Also returns k = cos^2 of the transmitted angle (negative: TIR)."""
    c = dot(n, w)
    k = 1.0 + inv_eta * inv_eta * (c * c - 1.0)
    t = -w * col(inv_eta) + col(inv_eta * c - np.sqrt(np.maximum(k, 0.0))) * n
    return np.where(col(k < 0.0), 0.0, t), k


def frame_from_z(v):
    """Orthonormal basis (x, y, z) with z = v/|v|, Duff et al. 2017 (Pixar), the sign taken as -1 only for z.z < 0
    (:2424-2437)."""
    z = normalize(v)
    s = np.where(z[:, 2] < 0.0, -1.0, 1.0)
    a = -1.0 / (s + z[:, 2])
    b = z[:, 0] * z[:, 1] * a
    x = np.stack([1.0 + s * z[:, 0] ** 2 * a, s * b, -s * z[:, 0]], -1)
    y = np.stack([b, s + z[:, 1] ** 2 * a, -z[:, 1]], -1)
    return x, y, z


def to_world(v, local):
    x, y, z = frame_from_z(v)
    return col(local[:, 0]) * x + col(local[:, 1]) * y + col(local[:, 2]) * z


# ---- Fresnel (:1433-1504) -------------------------------------------------------------------------------------------

def fresnel_dielectric(eta, n, w):
    """Unpolarised Fresnel reflectance of a dielectric interface of relative index eta at cos = |n.w|; 1 under TIR."""
    c = np.abs(dot(n, w))
    cos2t = 1.0 - (1.0 - c * c) / (eta * eta)
    ct = np.sqrt(np.maximum(cos2t, 0.0))
    rs = (c - eta * ct) / (c + eta * ct)
    rp = (ct - eta * c) / (ct + eta * c)
    return np.where(cos2t < 0.0, 1.0, 0.5 * (rs * rs + rp * rp))


def conductor_zero_k(color, n, w):
    """The conductor Fresnel term with extinction 0 and eta = (1 + sqrt(R)) / (1 - sqrt(R)), R = clamp(color, 0, 0.99),
    per channel; 0 when n.w <= 0.  With k = 0 it is the dielectric reflectance (eta >= 1: no TIR)."""
    r = np.clip(color, 0.0, 0.99)
    eta = (1.0 + np.sqrt(r)) / (1.0 - np.sqrt(r))
    c = np.clip(dot(n, w), -1.0, 1.0)
    f = np.stack([fresnel_dielectric(eta[:, k], n, w) for k in range(3)], -1)
    return np.where(col(dot(n, w) <= 0.0), 0.0, np.where(col(c) > 0.0, f, 0.0))


def schlick(r0, n, w):
    """Schlick's approximation, per channel; zero for a zero reflectivity (:1445-1451)."""
    p = np.clip(1.0 - np.abs(dot(n, w)), 0.0, 1.0) ** 5
    f = r0 + (1.0 - r0) * col(p)
    return np.where(col(np.all(r0 == 0.0, -1)), 0.0, f)


def gltf_reflectivity(ior, color, metallic):
    f0 = ((ior - 1.0) / (ior + 1.0)) ** 2
    return col(f0 * (1.0 - metallic)) + color * col(metallic)


# ---- GGX (:1506-1555, :1902-1918, :2209-2214) -----------------------------------------------------------------------

def ggx_d(alpha, n, h):
    """Trowbridge-Reitz normal distribution D(h), alpha = the material roughness; 0 for n.h <= 0."""
    c = dot(n, h)
    a2 = alpha * alpha
    t = 1.0 + (a2 - 1.0) * c * c
    return np.where(c <= 0.0, 0.0, a2 / (PI * t * t))


def ggx_g1(alpha, n, h, w):
    """Smith masking of the GGX distribution; 0 when w is on the other side of n than of h."""
    c = dot(n, w)
    ok = c * dot(h, w) > 0.0
    a2 = alpha * alpha
    g = 2.0 * np.abs(c) / (np.abs(c) + np.sqrt(a2 + (1.0 - a2) * c * c))
    return np.where(ok, g, 0.0)


def ggx_g(alpha, n, h, o, i):
    return ggx_g1(alpha, n, h, o) * ggx_g1(alpha, n, h, i)


def ggx_h_pdf(alpha, n, h):
    """Density of the sampled half vector, D(h) |n.h|, over solid angle; 0 below the surface."""
    c = dot(n, h)
    return np.where(c < 0.0, 0.0, ggx_d(alpha, n, h) * c)


def ggx_sample_h(alpha, n, r0, r1):
    """Half vector with density D(h) (n.h): tan(theta) = alpha sqrt(u / (1 - u)), phi = 2 pi u0."""
    theta = np.arctan(alpha * np.sqrt(r1 / (1.0 - r1)))
    phi = 2.0 * PI * r0
    local = np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], -1)
    return normalize(to_world(n, local))


def cos_sample(n, r0, r1):
    """Cosine-weighted hemisphere around n (:2216-2223)."""
    z = np.sqrt(r1)
    r = np.sqrt(1.0 - z * z)
    phi = 2.0 * PI * r0
    return normalize(to_world(n, np.stack([r * np.cos(phi), r * np.sin(phi), z], -1)))


def cos_pdf(n, w):
    c = dot(n, w)
    return np.where(c <= 0.0, 0.0, c / PI)


# ---- materials ------------------------------------------------------------------------------------------------------

class Mat:
    """Material arrays, one entry per record (types as ints; roughness as the material point stores it)."""

    def __init__(self, type_, color, roughness, metallic, ior, density=None, scattering=None, anisotropy=None):
        n = len(type_)
        self.type = np.asarray(type_, np.int64)
        self.color = np.asarray(color, np.float64).reshape(n, 3)
        self.rough = np.asarray(roughness, np.float64)
        self.metal = np.asarray(metallic, np.float64)
        self.ior = np.asarray(ior, np.float64)
        z3 = np.zeros((n, 3))
        self.density = z3 if density is None else np.asarray(density, np.float64).reshape(n, 3)
        self.scattering = z3 if scattering is None else np.asarray(scattering, np.float64).reshape(n, 3)
        self.g = np.zeros(n) if anisotropy is None else np.asarray(anisotropy, np.float64)


def is_delta(m):
    lobe = np.isin(m.type, [REFLECTIVE, TRANSPARENT, REFRACTIVE]) & (m.rough == 0.0)
    return lobe | (m.type == VOLUMETRIC)


def up_of(n, o):
    """The normal turned to o's side; n.o == 0 counts as below (:1810 and its twins)."""
    return np.where(col(dot(n, o) <= 0.0), -n, n)


def _refr_frame(m, n, o):
    entering = dot(n, o) >= 0.0
    up = np.where(col(entering), n, -n)
    eta = np.where(entering, m.ior, 1.0 / m.ior)    # eta_i / eta_t seen from o's side
    return entering, up, eta


def bsdf_sample(m, n, o, rnl, r0, r1):
    """sample_bsdfcos (:1789-1900).  Returns (direction, info): info holds, per record, the Fresnel value rnl was
    compared with (nan when none) and the refraction k (nan when none), for the ill-conditioned bands of the tests."""
    N = len(m.type)
    out = np.zeros((N, 3))
    f_thr = np.full(N, np.nan)
    k_tir = np.full(N, np.nan)
    up = up_of(n, o)
    h_up = ggx_sample_h(m.rough, up, r0, r1)
    cs = cos_sample(up, r0, r1)
    refl_h = reflect(o, h_up)
    keep_refl = dot(up, o) * dot(up, refl_h) >= 0.0

    t = m.type == MATTE
    out[t] = cs[t]

    t = m.type == REFLECTIVE
    out[t] = np.where(col(keep_refl), refl_h, 0.0)[t]

    t = m.type == GLOSSY
    F = fresnel_dielectric(m.ior, up, o)
    spec = rnl < F
    out[t] = np.where(col(spec), np.where(col(keep_refl), refl_h, 0.0), cs)[t]
    f_thr[t] = F[t]

    t = m.type == GLTFPBR
    F = np.mean(schlick(gltf_reflectivity(m.ior, m.color, m.metal), up, o), -1)
    spec = rnl < F
    out[t] = np.where(col(spec), np.where(col(keep_refl), refl_h, 0.0), cs)[t]
    f_thr[t] = F[t]

    t = m.type == TRANSPARENT
    F = fresnel_dielectric(m.ior, h_up, o)
    spec = rnl < F
    # thin sheet: the reflected direction mirrored back through the macro surface
    thru = -reflect(refl_h, up)
    keep_thru = dot(up, o) * dot(up, thru) < 0.0
    out[t] = np.where(col(spec), np.where(col(keep_refl), refl_h, 0.0), np.where(col(keep_thru), thru, 0.0))[t]
    f_thr[t] = F[t]

    t = (m.type == REFRACTIVE) | (m.type == SUBSURFACE)
    entering, upr, eta = _refr_frame(m, n, o)
    h = ggx_sample_h(m.rough, upr, r0, r1)
    F = fresnel_dielectric(eta, h, o)
    spec = rnl < F
    rr = reflect(o, h)
    keep_r = dot(upr, o) * dot(upr, rr) >= 0.0
    tt, k = refract(o, h, 1.0 / eta)
    keep_t = dot(upr, o) * dot(upr, tt) < 0.0
    out[t] = np.where(col(spec), np.where(col(keep_r), rr, 0.0), np.where(col(keep_t), tt, 0.0))[t]
    f_thr[t] = F[t]
    k_tir[t & ~spec] = k[t & ~spec]

    out[m.rough == 0.0] = 0.0
    return out, dict(fresnel=f_thr, k=k_tir)


def bsdf_eval(m, n, o, i):
    """eval_bsdfcos (:1951-2090): BSDF times |cos| of the incoming direction."""
    N = len(m.type)
    out = np.zeros((N, 3))
    ndi, ndo = dot(n, i), dot(n, o)
    same = ndi * ndo > 0.0
    up = up_of(n, o)
    ai = np.abs(dot(up, i))
    with np.errstate(all="ignore"):
        h = normalize(i + o)
        D = ggx_d(m.rough, up, h)
        G = ggx_g(m.rough, up, h, o, i)
        spec = D * G / (4.0 * dot(up, o) * dot(up, i)) * ai

        t = m.type == MATTE
        out[t] = (m.color * col(ai / PI))[t]

        t = m.type == GLOSSY
        F1 = fresnel_dielectric(m.ior, up, o)
        F = fresnel_dielectric(m.ior, h, i)
        out[t] = (m.color * col((1.0 - F1) / PI * ai) + col(F * spec))[t]

        t = m.type == REFLECTIVE
        out[t] = (conductor_zero_k(m.color, h, i) * col(spec))[t]

        t = m.type == GLTFPBR
        r0 = gltf_reflectivity(m.ior, m.color, m.metal)
        out[t] = (m.color * col(1.0 - m.metal) * (1.0 - schlick(r0, up, o)) / PI * col(ai) + schlick(r0, h, i) * col(spec))[t]
        out[np.isin(m.type, [MATTE, GLOSSY, REFLECTIVE, GLTFPBR]) & ~same] = 0.0

        t = m.type == TRANSPARENT
        refl_side = ndi * ndo >= 0.0
        Fr = fresnel_dielectric(m.ior, h, o)
        # transmission: the sheet's through direction is the mirror image of a reflection about the macro normal
        ir = reflect(-i, up)
        hr = normalize(ir + o)
        Ft = fresnel_dielectric(m.ior, hr, o)
        tr = ggx_d(m.rough, up, hr) * ggx_g(m.rough, up, hr, o, ir) / (4.0 * dot(up, o) * dot(up, ir)) * np.abs(dot(up, ir))
        val = np.where(col(refl_side), col(Fr * spec), m.color * col((1.0 - Ft) * tr))
        out[t] = val[t]

        t = (m.type == REFRACTIVE) | (m.type == SUBSURFACE)
        entering, upr, eta = _refr_frame(m, n, o)
        refl_side = ndi * ndo >= 0.0
        Fr = fresnel_dielectric(eta, h, o)
        Dr = ggx_d(m.rough, upr, h)
        Gr = ggx_g(m.rough, upr, h, o, i)
        vr = Fr * Dr * Gr / np.abs(4.0 * ndo * ndi) * np.abs(ndi)
        ht = generalized_half(eta, i, o, entering)
        Ft = fresnel_dielectric(eta, ht, o)
        Dt = ggx_d(m.rough, upr, ht)
        Gt = ggx_g(m.rough, upr, ht, o, i)
        den = eta * dot(ht, i) + dot(ht, o)
        # Walter et al. 2007 eq. 21 without the eta_o^2 radiance factor, times |n.i|
        vt = np.abs(dot(o, ht) * dot(i, ht) / (ndo * ndi)) * (1.0 - Ft) * Dt * Gt / (den * den) * np.abs(ndi)
        out[t] = col(np.where(refl_side, vr, vt))[t]

    out[m.rough == 0.0] = 0.0
    return out


def generalized_half(eta, i, o, entering):
    """Half vector of a refraction, -(eta i + o) normalised, turned to the side the macro normal faces from o."""
    return -normalize(col(eta) * i + o) * col(np.where(entering, 1.0, -1.0))


def bsdf_pdf(m, n, o, i, refraction_jacobian="reference"):
    """sample_bsdfcos_pdf (:2097-2207) over solid angle."""
    N = len(m.type)
    out = np.zeros(N)
    ndi, ndo = dot(n, i), dot(n, o)
    same = ndi * ndo > 0.0
    up = up_of(n, o)
    with np.errstate(all="ignore"):
        h = normalize(i + o)
        # reflection about h: d(omega_h) / d(omega_i) = 1 / (4 |o.h|)
        refl = ggx_h_pdf(m.rough, up, h) / (4.0 * np.abs(dot(o, h)))

        t = m.type == MATTE
        out[t] = cos_pdf(up, i)[t]
        t = m.type == GLOSSY
        F = fresnel_dielectric(m.ior, up, o)
        out[t] = (F * refl + (1.0 - F) * cos_pdf(up, i))[t]
        t = m.type == REFLECTIVE
        out[t] = refl[t]
        t = m.type == GLTFPBR
        F = np.mean(schlick(gltf_reflectivity(m.ior, m.color, m.metal), up, o), -1)
        out[t] = (F * refl + (1.0 - F) * cos_pdf(up, i))[t]
        out[np.isin(m.type, [MATTE, GLOSSY, REFLECTIVE, GLTFPBR]) & ~same] = 0.0

        t = m.type == TRANSPARENT
        refl_side = ndi * ndo >= 0.0
        ir = reflect(-i, up)
        hr = normalize(ir + o)
        v = np.where(refl_side, fresnel_dielectric(m.ior, h, o) * refl,
                     (1.0 - fresnel_dielectric(m.ior, hr, o)) * ggx_h_pdf(m.rough, up, hr) / (4.0 * np.abs(dot(o, hr))))
        out[t] = v[t]

        t = (m.type == REFRACTIVE) | (m.type == SUBSURFACE)
        entering, upr, eta = _refr_frame(m, n, o)
        refl_side = ndi * ndo >= 0.0
        vr = fresnel_dielectric(eta, h, o) * ggx_h_pdf(m.rough, upr, h) / (4.0 * np.abs(dot(o, h)))
        ht = generalized_half(eta, i, o, entering)
        den = eta * dot(ht, i) + dot(ht, o)
        jac = np.abs(dot(ht, i)) / (den * den)
        if refraction_jacobian == "walter":
            jac = jac * eta * eta
        vt = (1.0 - fresnel_dielectric(eta, ht, o)) * ggx_h_pdf(m.rough, upr, ht) * jac
        out[t] = np.where(refl_side, vr, vt)[t]

    out[m.rough == 0.0] = 0.0
    return out


# ---- delta lobes (:2231-2404) ---------------------------------------------------------------------------------------

def _refr_passthrough(m):
    return np.abs(m.ior - 1.0) < 1e-3


def delta_sample(m, n, o, rnl):
    N = len(m.type)
    out = np.zeros((N, 3))
    f_thr = np.full(N, np.nan)
    up = up_of(n, o)
    t = m.type == REFLECTIVE
    out[t] = reflect(o, up)[t]
    t = m.type == TRANSPARENT
    F = fresnel_dielectric(m.ior, up, o)
    out[t] = np.where(col(rnl < F), reflect(o, up), -o)[t]
    f_thr[t] = F[t]
    t = m.type == REFRACTIVE
    entering, upr, eta = _refr_frame(m, n, o)
    F = fresnel_dielectric(eta, upr, o)
    tt, _ = refract(o, upr, 1.0 / eta)
    v = np.where(col(rnl < F), reflect(o, upr), tt)
    v = np.where(col(_refr_passthrough(m)), -o, v)
    out[t] = v[t]
    f_thr[t & ~_refr_passthrough(m)] = F[t & ~_refr_passthrough(m)]
    t = m.type == VOLUMETRIC
    out[t] = -o[t]
    out[(m.rough != 0.0)] = 0.0
    return out, dict(fresnel=f_thr)


def delta_eval(m, n, o, i):
    N = len(m.type)
    out = np.zeros((N, 3))
    side = dot(n, i) * dot(n, o)
    up = up_of(n, o)
    t = m.type == REFLECTIVE
    out[t] = np.where(col(side <= 0.0), 0.0, conductor_zero_k(m.color, up, o))[t]
    t = m.type == TRANSPARENT
    F = fresnel_dielectric(m.ior, up, o)
    out[t] = np.where(col(side >= 0.0), col(F), m.color * col(1.0 - F))[t]
    t = m.type == REFRACTIVE
    entering, upr, eta = _refr_frame(m, n, o)
    F = fresnel_dielectric(eta, upr, o)
    v = np.where(side >= 0.0, F, (1.0 - F) / (eta * eta))
    v = np.where(_refr_passthrough(m), np.where(side <= 0.0, 1.0, 0.0), v)
    out[t] = col(v)[t]
    t = m.type == VOLUMETRIC
    out[t] = col(np.where(side >= 0.0, 0.0, 1.0))[t]
    out[(m.rough != 0.0)] = 0.0
    return out


def delta_pdf(m, n, o, i):
    N = len(m.type)
    out = np.zeros(N)
    side = dot(n, i) * dot(n, o)
    up = up_of(n, o)
    t = m.type == REFLECTIVE
    out[t] = np.where(side <= 0.0, 0.0, 1.0)[t]
    t = m.type == TRANSPARENT
    F = fresnel_dielectric(m.ior, up, o)
    out[t] = np.where(side >= 0.0, F, 1.0 - F)[t]
    t = m.type == REFRACTIVE
    entering, upr, eta = _refr_frame(m, n, o)
    F = fresnel_dielectric(eta, upr, o)
    v = np.where(side >= 0.0, F, 1.0 - F)
    v = np.where(_refr_passthrough(m), np.where(side < 0.0, 1.0, 0.0), v)
    out[t] = v[t]
    t = m.type == VOLUMETRIC
    out[t] = np.where(side >= 0.0, 0.0, 1.0)[t]
    out[(m.rough != 0.0)] = 0.0
    return out


# ---- phase function and distance sampling (:1920-1949, :2092-2095, :2339-2347, :2406-2422) ------------------------

def hg_pdf(g, cos_theta):
    """Henyey-Greenstein density over solid angle, cos_theta = -o.i (the angle from the forward direction -o)."""
    d = 1.0 + g * g - 2.0 * g * cos_theta
    return (1.0 - g * g) / (4.0 * PI * d * np.sqrt(d))


def hg_sample_cos(g, r1):
    """Inverse of the HG cumulative distribution in cos_theta; uniform for |g| < 1e-3."""
    with np.errstate(all="ignore"):
        s = (1.0 - g * g) / (1.0 + g - 2.0 * g * r1)
        c = (1.0 + g * g - s * s) / (2.0 * g)
    return np.where(np.abs(g) < 1e-3, 1.0 - 2.0 * r1, c)


def phase_sample(m, o, r0, r1):
    c = hg_sample_cos(m.g, r1)
    s = np.sqrt(np.maximum(0.0, 1.0 - c * c))
    phi = 2.0 * PI * r0
    d = to_world(-o, np.stack([s * np.cos(phi), s * np.sin(phi), c], -1))
    return np.where(col(np.all(m.density == 0.0, -1)), 0.0, d)


def phase_pdf(m, o, i):
    return np.where(np.all(m.density == 0.0, -1), 0.0, hg_pdf(m.g, -dot(o, i)))


def phase_eval(m, o, i):
    return m.scattering * m.density * col(phase_pdf(m, o, i))


def medium_sample_distance(density, max_distance, rl, rd):
    """Pick a channel with rl, then an exponential free path in it; capped at max_distance (a zero density never
    scatters: F32_MAX before the cap)."""
    ch = np.clip(np.trunc(rl * 3.0).astype(np.int64), 0, 2)
    dc = density[np.arange(len(ch)), ch]
    with np.errstate(divide="ignore"):
        d = np.where(dc == 0.0, F32_MAX, -np.log1p(-rd) / dc)
    return np.minimum(d, max_distance)


def medium_transmittance(density, d):
    return np.exp(-density * col(d))


def medium_distance_pdf(density, d, max_distance):
    """Mixture density of the three channels' exponentials below max_distance; the probability of reaching
    max_distance (a point mass) at it."""
    return np.where(d < max_distance, np.mean(density * np.exp(-density * col(d)), -1),
                    np.mean(np.exp(-density * col(max_distance)), -1))
