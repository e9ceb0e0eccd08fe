// lupin_reproject.hpp -- temporal reprojection of the adaptive history, included once by lupin_hip.hip
// after lupin_adaptive.hpp.
//
// When the camera or an instance moves, lupin_hip_adaptive_reproject carries the accumulated image and the adaptive
// state (n_p and the luminance moments) over to the new view instead of starting every pixel from zero samples:
//
//   k_reproject_trace    one thread per pixel: the pinhole ray through the pixel centre (camera_ray_centre: zero jitter and
//                        zero aperture), scene_closest -> the current visibility record (instance, triangle, u, v, depth)
//   k_reproject_gather   one thread per pixel, 16 x 16 blocks: hit point -> where it was in the previous view -> bilinear
//                        2 x 2 gather of the previous image, n_p and moments from the taps that show the same surface
//   k_reproject_refresh  one wave64 per 8x8 block: (sum, max) of the new n_p, no error estimate, flags cleared;
//                        k_adaptive_mask (unchanged) then makes every block active and recomputes the statistics
//
// Every operation is one rounded f32 operation (the Makefile builds with -ffp-contract=off and IEEE division), every sum
// in a fixed order, so tests/reproject_ref.py restates the gather exactly.
#pragma once

#include "lupin_adaptive.hpp"
#include "lupin_denoise.hpp"

// one view's visibility buffer, W*H entries each
struct ReprojectVis
{
    uint32_t *inst;   // instance, or HIT_MISS
    uint32_t *tri;    // global triangle (index into SceneDev::tris)
    float2 *uv;       // barycentric u, v of the hit
    float *depth;     // z of the hit point in the view's camera space (the camera looks along +z there)
};

constexpr float LP_RP_SNAP = 64.0f;   // reprojected positions are snapped to 1/64 pixel

// affine map given as three rows (x y z | translation): the form InstanceDev keeps world -> local in
LP_DEV f3 rp_rows_point(float4 r0, float4 r1, float4 r2, f3 p)
{
    return mk3(p.x * r0.x + p.y * r0.y + p.z * r0.z + r0.w, p.x * r1.x + p.y * r1.y + p.z * r1.z + r1.w,
               p.x * r2.x + p.y * r2.y + p.z * r2.z + r2.w);
}
// affine map given as a LupinMat3x4 (four columns of three rows)
LP_DEV f3 rp_mat_point(const LupinMat3x4 &m, f3 p)
{
    return mk3(m.m[0][0] * p.x + m.m[1][0] * p.y + m.m[2][0] * p.z + m.m[3][0], m.m[0][1] * p.x + m.m[1][1] * p.y + m.m[2][1] * p.z + m.m[3][1],
               m.m[0][2] * p.x + m.m[1][2] * p.y + m.m[2][2] * p.z + m.m[3][2]);
}

template <bool LDSGEO>
__global__ void __launch_bounds__(LP_BLOCK) k_reproject_trace(SceneDev sc, FrameParams fp, uint32_t n, LupinMat3x4 cam_inv, ReprojectVis vis,
                                                              uint32_t stack_words)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_stack[];
    const auto geo = make_geo<LDSGEO>(sc, lds_stack, stack_words);
    const uint32_t slot = blockIdx.x * LP_BLOCK + threadIdx.x;
    if (slot >= n) return;
    const uint32_t gx = slot % fp.width, gy = slot / fp.width;
    f3 o, d;
    camera_ray_centre(fp, gx, gy, o, d);
    const Closest c = scene_closest(geo, sc, lds_stack, o, d, fp.pc.ray_epsilon);   // opacity is not consulted: cut-outs count as opaque
    const bool hit = c.t != LP_F32_MAX;
    const f3 p = add(o, scale(d, c.t));
    vis.inst[slot] = hit ? c.inst : HIT_MISS;
    vis.tri[slot] = hit ? c.tri : 0u;
    vis.uv[slot] = hit ? make_float2(c.u, c.v) : make_float2(0.0f, 0.0f);
    vis.depth[slot] = hit ? rp_mat_point(cam_inv, p).z : 0.0f;
}

struct ReprojectArgs
{
    uint32_t width, height;
    LupinPushConstants prev_pc;       // the previous call's camera: lens, film, aspect and kind are read
    LupinMat3x4 prev_cam_inv;         // world -> the previous camera's space
    const float4 *prev_local_to_world;   // per instance three rows: local -> world as it was when history_in was rendered
    const TriVerts *tris;
    float depth_tolerance;
    uint32_t max_history;             // 0 = no cap
    uint32_t prev_valid;              // 0: there is no previous view (first call, or after an invalidate)
    ReprojectVis cur, prev;
    const uint32_t *frames_in;        // the adaptive state that goes with history_in
    const float2 *moments_in;
    uint32_t *frames_out;             // ... and with history_out
    float2 *moments_out;
    const uint2 *hist_in;             // Rgba16Float texels
    const float4 *hist_in32;          // history_in's f32 accumulator when it is valid, else NULL
    uint2 *hist_out;
    float4 *hist_out32;               // history_out's f32 accumulator in f32 accumulation mode, else NULL
};

// Continuous pixel coordinates (integers = pixel centres) of a point of camera space: the inverse of camera_ray_centre.
// Perspective x / z = fsx (uvx - 0.5) / lens; orthographic x = fsx (uvx - 0.5) / lens; then uvx = (gx + 0.5) / resx and
// uvy = ((resy - gy) + 0.5) / resy.  The caller has checked z > 0.
LP_DEV void rp_project(const LupinPushConstants &pc, float resx, float resy, f3 c, float &fx, float &fy)
{
    float fsx, fsy;
    camera_film_size(pc.camera_film, pc.camera_aspect, fsx, fsy);
    const float lens = pc.camera_lens;
    float uvx, uvy;
    if (pc.flags & LUPIN_FLAG_CAMERA_ORTHO)
    {
        uvx = 0.5f + (c.x * lens) / fsx;
        uvy = 0.5f + (c.y * lens) / fsy;
    }
    else
    {
        uvx = 0.5f + (c.x * lens) / (c.z * fsx);
        uvy = 0.5f + (c.y * lens) / (c.z * fsy);
    }
    fx = uvx * resx - 0.5f;
    fy = (resy + 0.5f) - uvy * resy;
}

__global__ void __launch_bounds__(LP_DN_BX * LP_DN_BY) k_reproject_gather(ReprojectArgs a)
{
    const uint32_t x = blockIdx.x * LP_DN_BX + threadIdx.x, y = blockIdx.y * LP_DN_BY + threadIdx.y;
    if (x >= a.width || y >= a.height) return;
    const uint32_t p = y * a.width + x;
    // what a pixel without usable history takes
    uint32_t n = 0u;
    float2 mom = make_float2(0.0f, 0.0f);
    f3 col = mk3(0.0f, 0.0f, 0.0f);
    const uint32_t inst = a.cur.inst[p];
    if (inst != HIT_MISS && a.prev_valid)
    {
        const float2 uv = a.cur.uv[p];
        const TriVerts tv = a.tris[a.cur.tri[p]];
        const float w0 = (1.0f - uv.x) - uv.y;
        const f3 pl = mk3(tv.v0.x * w0 + tv.v1.x * uv.x + tv.v2.x * uv.y, tv.v0.y * w0 + tv.v1.y * uv.x + tv.v2.y * uv.y,
                          tv.v0.z * w0 + tv.v1.z * uv.x + tv.v2.z * uv.y);
        const float4 *rows = a.prev_local_to_world + (size_t)inst * 3u;
        const f3 pw = rp_rows_point(rows[0], rows[1], rows[2], pl);
        const f3 pc = rp_mat_point(a.prev_cam_inv, pw);
        if (pc.z > 0.0f)   // else behind the previous camera (NaN included)
        {
            float fx, fy;
            rp_project(a.prev_pc, (float)a.width, (float)a.height, pc, fx, fy);
            const float sx = rintf(fx * LP_RP_SNAP) / LP_RP_SNAP, sy = rintf(fy * LP_RP_SNAP) / LP_RP_SNAP;
            if (sx > -1.0f && sx < (float)a.width && sy > -1.0f && sy < (float)a.height)   // some tap inside (NaN: none)
            {
                const float x0f = floorf(sx), y0f = floorf(sy);
                const float tx = sx - x0f, ty = sy - y0f;
                const int x0 = (int)x0f, y0 = (int)y0f;
                const float bw[4] = {(1.0f - tx) * (1.0f - ty), tx * (1.0f - ty), (1.0f - tx) * ty, tx * ty};
                float w[4];
                uint32_t nq[4], q[4];
                uint32_t nmin = 0xFFFFFFFFu;
                for (int k = 0; k < 4; k++)
                {
                    const int qx = x0 + (k & 1), qy = y0 + (k >> 1);
                    w[k] = 0.0f; nq[k] = 0u; q[k] = 0u;
                    // a tap of bilinear weight 0 is not read: it could only lower n (an unmoved view stays an exact copy)
                    if (!(bw[k] > 0.0f) || qx < 0 || qy < 0 || qx >= (int)a.width || qy >= (int)a.height) continue;
                    const uint32_t qi = (uint32_t)qy * a.width + (uint32_t)qx;
                    const uint32_t nn = a.frames_in[qi];
                    if (nn < 1u || a.prev.inst[qi] != inst) continue;
                    if (!(fabsf(a.prev.depth[qi] - pc.z) <= a.depth_tolerance * pc.z)) continue;
                    w[k] = bw[k]; nq[k] = nn; q[k] = qi;
                    nmin = min(nmin, nn);
                }
                const float wsum = ((w[0] + w[1]) + w[2]) + w[3];
                if (wsum > 0.0f)
                {
                    n = (a.max_history != 0u) ? min(nmin, a.max_history) : nmin;
                    const float nf = (float)n;
                    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sm = 0.0f, s2 = 0.0f;
                    for (int k = 0; k < 4; k++)
                    {
                        if (!(w[k] > 0.0f)) continue;
                        f3 c;
                        if (a.hist_in32) { const float4 v = a.hist_in32[q[k]]; c = mk3(v.x, v.y, v.z); }
                        else { const float4 v = dn_load_h4(a.hist_in, q[k]); c = mk3(v.x, v.y, v.z); }
                        const float2 m = a.moments_in[q[k]];
                        // M2 scales with the sample count: a tap's M2 / n_q * n (its own M2 where n_q == n, exactly)
                        const float m2 = (nq[k] == n) ? m.y : (m.y / (float)nq[k]) * nf;
                        sr = sr + w[k] * c.x; sg = sg + w[k] * c.y; sb = sb + w[k] * c.z;
                        sm = sm + w[k] * m.x; s2 = s2 + w[k] * m2;
                    }
                    col = mk3(sr / wsum, sg / wsum, sb / wsum);
                    mom = make_float2(sm / wsum, s2 / wsum);
                }
            }
        }
    }
    a.frames_out[p] = n;
    a.moments_out[p] = mom;
    // always nearest even: toward zero would darken the image by up to 2^-11 with every reprojection
    a.hist_out[p] = make_uint2(dn_pack2(col.x, col.y), dn_pack2(col.z, 1.0f));
    if (a.hist_out32) a.hist_out32[p] = make_float4(col.x, col.y, col.z, 1.0f);
}

// After the gather: one wave64 per 8x8 block (four blocks per workgroup, as k_adaptive_update), lane = pixel.  The block
// keeps (sum, max) of its new n_p for the statistics, has no error estimate and no flags; k_adaptive_mask, run next, then
// finds every block open and uncapped, makes it active and adds up the statistics.
__global__ void __launch_bounds__(LP_BLOCK) k_reproject_refresh(AdaptiveDev ad)
{
    const uint32_t b = blockIdx.x * (LP_BLOCK / 64u) + (threadIdx.x >> 6);
    if (b >= ad.blocks_x * ad.blocks_y) return;   // whole waves leave together
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gx = (b % ad.blocks_x) * LP_AD_BLOCK + (lane & 7u), gy = (b / ad.blocks_x) * LP_AD_BLOCK + (lane >> 3);
    uint32_t nmax = 0u, nsum = 0u;
    if (gx < ad.width && gy < ad.height) nmax = nsum = ad.frames[(size_t)gy * ad.width + gx];
    for (int off = 32; off > 0; off >>= 1)
    {
        nmax = max(nmax, (uint32_t)__shfl_xor((int)nmax, off));
        nsum += (uint32_t)__shfl_xor((int)nsum, off);   // 64 counts below 2^26 each: no overflow
    }
    if (lane == 0)
    {
        ad.block_error[b] = __builtin_inff();
        ad.block_flags[b] = 0u;
        ad.block_active[b] = 1u;
        ad.block_count[b] = make_uint2(nsum, nmax);
    }
}
