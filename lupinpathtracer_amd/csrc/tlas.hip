// Device TLAS builder: lp::build_tlas' agglomerative clustering (data_structures.rs:545-641, restated in builders.cpp
// lupin_build_tlas) run by ONE workgroup, emitting the same tree node for node.
//
// The CPU builder is a serial chain of tlas_find_best_match scans, each a linear arg-min over the live nodes in which the
// lowest index wins ties.  Here a scan is a block-wide reduction of (area, index) pairs ordered by area, then index, which
// selects exactly the first minimal index of the ascending scan; everything else (the walk a -> b -> c, the merge, the
// swap-with-last removal) is the CPU code's control flow, executed uniformly by every thread.
#include "lupin_internal.hpp"
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

namespace {

constexpr uint32_t kMaxBlock = 1024;
constexpr uint32_t kFields = 7;                    // per live slot: min xyz, max xyz, node index
constexpr uint32_t kRedWords = 2 * 2 * 16;         // two alternating sets of 16 per-wave (area, index) pairs
// Live slots the LDS-resident state holds: 7 x 4 bytes per slot + the reduction words in the 160 KiB a single workgroup
// may declare on gfx950.  Larger inputs keep the state in global memory (same kernel, other address space).
constexpr uint32_t kLdsSlots = 5800;
constexpr uint32_t kNone = 0xFFFFFFFFu;

enum : uint32_t { TLAS_OK = 0, TLAS_SCAN_CAP = 1, TLAS_NO_CANDIDATE = 2 };

thread_local LupinTlasBuildStats g_stats = {0, 0, 0, 0.0f};

// status: [0] error word, [1] scans low, [2] scans high
template <bool IN_LDS>
__global__ __launch_bounds__(kMaxBlock) void k_tlas_cluster(LupinTlasNode *nodes, uint32_t n, float *gstate, uint32_t *status)
{
    extern __shared__ float smem[];
    // red[set][wave] pairs first, then (IN_LDS) the seven state arrays of n slots each
    float *red_area = smem;
    uint32_t *red_idx = reinterpret_cast<uint32_t *>(smem) + 2 * 16;
    float *lstate = smem + kRedWords;
    const uint32_t tid = threadIdx.x, nthreads = blockDim.x;
    const uint32_t lane = tid & 63u, wave = tid >> 6, nwaves = (nthreads + 63u) >> 6;

#define ST(f, i) (IN_LDS ? lstate[(f) * n + (i)] : gstate[(size_t)(f) * n + (i)])
#define ST_SET(f, i, v) do { if (IN_LDS) lstate[(f) * n + (i)] = (v); else gstate[(size_t)(f) * n + (i)] = (v); } while (0)

    for (uint32_t i = tid; i < n; i += nthreads)
    {
        const LupinTlasNode nd = nodes[i];
        ST_SET(0, i, nd.aabb_min[0]); ST_SET(1, i, nd.aabb_min[1]); ST_SET(2, i, nd.aabb_min[2]);
        ST_SET(3, i, nd.aabb_max[0]); ST_SET(4, i, nd.aabb_max[1]); ST_SET(5, i, nd.aabb_max[2]);
        ST_SET(6, i, __uint_as_float(i));
    }
    __syncthreads();

    uint32_t live = n;
    uint32_t next = n;                                           // index the next merged node gets
    unsigned long long scans = 0;
    const unsigned long long cap = (unsigned long long)n * n + 4ull * n;   // more scans than any input needs
    uint32_t err = TLAS_OK;

    // tlas_find_best_match (data_structures.rs:670-692): uniform result in every thread.  One barrier per scan: the
    // per-wave partial results alternate between two sets, so a set is rewritten only after the barrier of the scan between.
    auto best_match = [&](uint32_t node_a) -> uint32_t {
        const float alx = ST(0, node_a), aly = ST(1, node_a), alz = ST(2, node_a);
        const float ahx = ST(3, node_a), ahy = ST(4, node_a), ahz = ST(5, node_a);
        float smallest = FLT_MAX;
        uint32_t best_b = kNone;
        for (uint32_t i = tid; i < live; i += nthreads)
        {
            if (i == node_a) continue;
            const float ex = fmaxf(ahx, ST(3, i)) - fminf(alx, ST(0, i));
            const float ey = fmaxf(ahy, ST(4, i)) - fminf(aly, ST(1, i));
            const float ez = fmaxf(ahz, ST(5, i)) - fminf(alz, ST(2, i));
            const float area = ex * ey + ey * ez + ez * ex;
            if (area < smallest) { smallest = area; best_b = i; }
        }
        for (int off = 32; off > 0; off >>= 1)
        {
            const float oa = __shfl_down(smallest, off, 64);
            const uint32_t oi = (uint32_t)__shfl_down((int)best_b, off, 64);
            if (oa < smallest || (oa == smallest && oi < best_b)) { smallest = oa; best_b = oi; }
        }
        const uint32_t set = (uint32_t)(scans & 1ull) * 16u;
        if (lane == 0) { red_area[set + wave] = smallest; red_idx[set + wave] = best_b; }
        __syncthreads();
        smallest = red_area[set];
        best_b = red_idx[set];
        for (uint32_t w = 1; w < nwaves; w++)
        {
            const float oa = red_area[set + w];
            const uint32_t oi = red_idx[set + w];
            if (oa < smallest || (oa == smallest && oi < best_b)) { smallest = oa; best_b = oi; }
        }
        scans++;
        return best_b;
    };

    // agglomerative clustering (data_structures.rs:572-610 as builders.cpp restates it)
    uint32_t a = 0;
    uint32_t b = live > 1 ? best_match(a) : kNone;
    if (live > 1 && b == kNone) err = TLAS_NO_CANDIDATE;
    while (live > 1 && err == TLAS_OK)
    {
        if (scans >= cap) { err = TLAS_SCAN_CAP; break; }
        const uint32_t c = best_match(b);
        if (c == kNone) { err = TLAS_NO_CANDIDATE; break; }
        if (a == c)
        {
            if (tid == 0)
            {
                const uint32_t ia = __float_as_uint(ST(6, a)), ib = __float_as_uint(ST(6, b));
                LupinTlasNode nn;
                nn.left = ia; nn.right = ib;
                if (nn.left == 0) { nn.left = ib; nn.right = ia; }   // leaf 0 cannot be a left child (builders.cpp)
                for (int k = 0; k < 3; k++)
                {
                    nn.aabb_min[k] = fminf(ST(k, a), ST(k, b));
                    nn.aabb_max[k] = fmaxf(ST(3 + k, a), ST(3 + k, b));
                    nn._padding0[k] = 0.0f;
                }
                nn.instance_idx = 0;
                nodes[next] = nn;
                // node_indices[a] = new node; node_indices[b] = node_indices.back(); pop_back()  -- in this order
                for (int k = 0; k < 3; k++) { ST_SET(k, a, nn.aabb_min[k]); ST_SET(3 + k, a, nn.aabb_max[k]); }
                ST_SET(6, a, __uint_as_float(next));
                const uint32_t last = live - 1;
                for (uint32_t f = 0; f < kFields; f++) { const float v = ST(f, last); ST_SET(f, b, v); }
            }
            next++;
            live--;
            if (a >= live) a = live - 1;
            __syncthreads();
            if (live > 1)
            {
                b = best_match(a);
                if (b == kNone) err = TLAS_NO_CANDIDATE;
            }
        }
        else
        {
            a = b;
            b = c;
        }
    }
    if (tid == 0)
    {
        status[0] = err;
        status[1] = (uint32_t)scans;
        status[2] = (uint32_t)(scans >> 32);
        status[3] = __float_as_uint(ST(6, a));                   // the root: node_indices[a]
    }
#undef ST
#undef ST_SET
}

}  // namespace

extern "C" {

int64_t lupin_hip_build_tlas_device(LupinContext *ctx, const LupinInstance *instances, uint32_t num_instances,
                                    const float *model_aabbs, uint32_t num_meshes, LupinTlasNode *out_nodes)
{
    if (!ctx) return lupin_internal_fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (!lupin_internal_ctx_alive(ctx)) return lupin_internal_fail(LUPIN_ERR_INVALID_ARGUMENT, "the context has been destroyed");
    if (num_instances == 0 || num_meshes == 0) return 0;   // data_structures.rs:547
    if (!instances || !model_aabbs || !out_nodes) return lupin_internal_fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (num_instances > (1u << 26)) return lupin_internal_fail(LUPIN_ERR_INVALID_ARGUMENT, "more than 2^26 instances");
    const uint32_t n = num_instances;

    // leaves: the host helper lupin_build_tlas uses, so the boxes are the same floats by construction
    std::vector<LupinTlasNode> tlas((size_t)n * 2);
    if (lupin_internal_tlas_leaves(instances, n, model_aabbs, num_meshes, tlas.data()) != LUPIN_OK)
        return lupin_internal_fail(LUPIN_ERR_INVALID_ARGUMENT, "instance mesh_idx out of range");
    if (!lupin_internal_tlas_leaves_finite(instances, tlas.data(), n))
        return lupin_internal_fail(LUPIN_ERR_INVALID_ARGUMENT, "instance with a non-finite transform or world-space box (NaN / infinite / singular transform)");

    if (hipSetDevice(lupin_internal_ctx_device(ctx)) != hipSuccess) return lupin_internal_fail(LUPIN_ERR_HIP, "hipSetDevice");
    hipStream_t st = lupin_internal_ctx_stream(ctx);

    // LUPIN_TLAS_LDS_SLOTS=k: keep the state in LDS up to k live slots (A/B runs of the two residences; at most kLdsSlots)
    uint32_t lds_slots = kLdsSlots;
    if (const char *e = getenv("LUPIN_TLAS_LDS_SLOTS")) lds_slots = std::min<uint32_t>(kLdsSlots, (uint32_t)strtoul(e, nullptr, 10));
    const bool in_lds = n <= lds_slots;
    const uint32_t block = std::min(kMaxBlock, std::max(64u, (n + 63u) / 64u * 64u));

    // scratch of this build, freed when the function returns, by whichever path
    DeviceArray<LupinTlasNode> d_nodes;
    DeviceArray<float> d_state;
    DeviceArray<uint32_t> d_status;
    Event ev0, ev1;
    const size_t node_bytes = (size_t)n * 2 * sizeof(LupinTlasNode);
    HIP_TRY(d_nodes.alloc((size_t)n * 2));
    if (!in_lds) HIP_TRY(d_state.alloc((size_t)n * kFields));
    HIP_TRY(d_status.alloc(4));
    HIP_TRY(ev0.create());
    HIP_TRY(ev1.create());
    HIP_TRY(hipMemcpyAsync(d_nodes, tlas.data(), (size_t)n * sizeof(LupinTlasNode), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_status, 0xFF, 4 * sizeof(uint32_t), st));   // a kernel that never ran reads as an error
    HIP_TRY(hipEventRecord(ev0, st));
    const size_t lds = (kRedWords + (in_lds ? (size_t)n * kFields : 0)) * sizeof(float);
    if (in_lds) hipLaunchKernelGGL(k_tlas_cluster<true>, dim3(1), dim3(block), lds, st, d_nodes, n, d_state, d_status);
    else hipLaunchKernelGGL(k_tlas_cluster<false>, dim3(1), dim3(block), lds, st, d_nodes, n, d_state, d_status);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1, st));
    uint32_t status[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(status, d_status, sizeof(status), hipMemcpyDeviceToHost, st));
    if (n > 1) HIP_TRY(hipMemcpyAsync(tlas.data() + n, d_nodes + n, (size_t)(n - 1) * sizeof(LupinTlasNode), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, ev0, ev1));
    g_stats.num_instances = n;
    g_stats.scans = (uint64_t)status[1] | ((uint64_t)status[2] << 32);
    g_stats.state_in_lds = in_lds ? 1u : 0u;
    g_stats.kernel_ms = ms;
    if (status[0] == TLAS_SCAN_CAP) return lupin_internal_fail(LUPIN_ERR_INVALID_ARGUMENT, "device TLAS build stopped at its scan cap (n^2 + 4n best-match scans): no tree was produced");
    if (status[0] == TLAS_NO_CANDIDATE) return lupin_internal_fail(LUPIN_ERR_INVALID_ARGUMENT, "device TLAS build found no merge candidate (every union area is NaN or >= FLT_MAX): no tree was produced");
    if (status[0] != TLAS_OK || status[3] != 2 * n - 2) return lupin_internal_fail(LUPIN_ERR_HIP, "device TLAS build did not complete");

    // push a copy of the root, reverse, remap the children: the tail of lupin_build_tlas (data_structures.rs:612-635)
    tlas[(size_t)2 * n - 1] = tlas[status[3]];
    lupin_internal_tlas_finish(tlas.data(), 2 * n);
    memcpy(out_nodes, tlas.data(), node_bytes);
    return (int64_t)2 * n;
}

void lupin_hip_tlas_build_stats(LupinTlasBuildStats *out)
{
    if (out) *out = g_stats;
}

}  // extern "C"
