// lupin_hip.hip -- host side of liblupin_hip.so: the C ABI of include/lupin_hip.h (contexts and their lanes, scene upload,
// textures, the pathtrace_scene family, measurement hooks, probes).  The stage kernels live in lupin_stages.hpp, the
// traversal / material / light device functions in lupin_device.hpp, the CPU builders in builders.cpp, the device BLAS
// builder in lbvh.hip, the denoiser's kernels in lupin_denoise.hpp, adaptive sampling's in lupin_adaptive.hpp, its
// reprojection's in lupin_reproject.hpp, the radiance queries' in lupin_rays.hpp, light-probe baking's in lupin_probes.hpp,
// lightmap baking's in lupin_lightmap.hpp and lupin_lightmap_adaptive.hpp, the occlusion queries' in lupin_occlusion.hpp, the distance queries' in
// lupin_distance.hpp.
//
// THERE IS NO CPU FALLBACK: without a HIP device every entry point that needs one fails with LUPIN_ERR_NO_DEVICE.

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <cfloat>
#include <string>
#include <type_traits>
#include <vector>
#include <set>
#include <mutex>
#include <algorithm>
#include <atomic>
#include <chrono>

#include "lupin_stages.hpp"
#include "lupin_denoise.hpp"
#include "lupin_adaptive.hpp"
#include "lupin_reproject.hpp"
#include "lupin_rays.hpp"
#include "lupin_probes.hpp"
#include "lupin_lightmap.hpp"
#include "lupin_lightmap_directional.hpp"
#include "lupin_lightmap_adaptive.hpp"
#include "lupin_lightmap_denoise.hpp"
#include "lupin_unwrap.hpp"
#include "lupin_occlusion.hpp"
#include "lupin_transmittance.hpp"
#include "lupin_bent_normal.hpp"
#include "lupin_distance.hpp"
#include "lupin_probe_grid.hpp"
#include "lupin_probe_depth.hpp"
#include "lupin_baked_view.hpp"
#include "lupin_lightmapped_view.hpp"
#include "lupin_lightmap_stitch.hpp"
#include "lupin_internal.hpp"
#include "../../include/lupin_pack.hpp"
#include "../../include/lupin_stitch_rules.hpp"

// ------------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------------

static inline float host_u2f(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static thread_local std::string g_last_error;
static int fail(int code, const std::string &msg) { g_last_error = msg; return code; }

#define LP_MAX_LANES 8
#define LP_WIDE_WORDS 10   // [0] wide queries, [1] re-traced, [2..9] LUPIN_VERIFY_WIDE: checked, flagged, mismatches among unflagged, raw mismatches, 4 reasons
#define LP_COUNTER_ROWS 7   // per iteration and shard: 1 queue counter + 2 hand-out cursors + 2 re-trace counters + 2 re-trace cursors
#define LP_WORK_WORDS 28   // 3 tracing modes (closest hit | shadow rays | light-pdf marching) x {nodes, triangles, instances, four-wide nodes}, then 10 round statistics
// "Lanes" (stream + path buffers + counters) let consecutive pathtrace_scene calls overlap: the wavefront of
// frame k+1 starts while the thin tail of frame k is still draining.  Frames only meet at k_resolve (frame k+1 blends
// with frame k's output), which waits on the previous call's completion event.
struct Lane
{
    hipStream_t stream = nullptr;
    PathBuffers pb{};               // the plain view of the owners below that the kernels get by value
    // The nine per-slot buffers (bytes per slot: kPathSlotBytes).  HOT: the eight per-bounce fields, capacity x 128 bytes, planes or
    // records (set_path_layout); SHADOW: the eight MIS / Direct fields, likewise; SKEY: k_sort_queue's keys; the rest: pb's members.
    enum { HOT, SHADOW, SKEY, VOL0, VOL1, QUEUE0, QUEUE1, RETRACE, SHADE_ORDER, NUM_PATH_BUFFERS };
    DeviceBuffer path[NUM_PATH_BUFFERS];
    DeviceArray<uint32_t> counts;   // pb.counts, and pb.cursors / retrace_counts / retrace_cursors carved from it
    uint64_t capacity = 0;          // slots the path buffers hold
    uint32_t counts_capacity = 0;
    DeviceArray<unsigned long long> stat_counters;   // per shard: [2s] path bounces, [2s+1] paths
    DeviceArray<unsigned long long> work_counters;   // [4 * mode + {nodes, triangles, instances, wide nodes}] of the COUNT kernels (stats mode 2)
    DeviceArray<unsigned long long> wide_counters;   // [0] queries the wide tracer took, [1] queries re-traced by the binary tracer
    hipEvent_t done = nullptr;      // recorded after the last kernel of the lane's latest call
    bool used = false;
    DeviceArray<FrameParams> d_fp;  // this lane's per-call parameters (k_set_params writes, the stage kernels read)
    uint64_t pb_generation = 0;     // bumped when the path buffers are reallocated
    // the lane's wavefront (memset + k_begin + all iterations) as a replayable graph
    struct GraphKey
    {
        uint64_t scene_id = 0, pb_generation = 0;
        uint32_t n = 0, blocks = 0, type = 0, iterations = 0, stack_words = 0, lds = 0, pblocks = 0;
        uint32_t wide_blocks = 0, wide_stack_words = 0;
        int persistent = 0, persistent_shadow = 0, lds_geometry = 0;
        bool operator==(const GraphKey &o) const { return memcmp(this, &o, sizeof(GraphKey)) == 0; }
    } graph_key, seen_key;           // key of graph_exec | key of the lane's previous call
    hipGraph_t graph = nullptr;
    hipGraphExec_t graph_exec = nullptr;
};

struct LupinContext
{
    int device = 0;
    hipStream_t stream = nullptr;   // primary stream (= lanes[0].stream): every non-pathtrace operation runs here
    Lane lanes[LP_MAX_LANES];
    int num_lanes = LP_MAX_LANES;   // LUPIN_LANES=1..8; see the lane choice in flush_pending
    bool lanes_from_env = false;
    uint64_t call_index = 0;
    int last_lane = -1;
    hipEvent_t marker = nullptr;
    bool timing = false;
    int path_records = -1;          // LUPIN_PATH_RECORDS=0/1: path state as planes / 128-byte records (default: records where the queues are sorted)
    uint32_t short_stack = 26;      // LUPIN_SHORT_STACK=n: first pass of the binary tracer on n stack entries per lane when the scene's depth bound
                                    // asks for more (26 KB per block: six blocks per CU instead of four); 0 = always the full stack, one pass
    int light_stage = -1;           // LUPIN_LIGHT_STAGE=0/1: sample_lights_pdf inline in k_shade / in its own stage (k_light_pdf, k_light_pdf_mis); default: stage for MIS only
    bool debug_sync = false;        // LUPIN_DEBUG_SYNC=1: synchronise and report after every stage launch (fault localisation)
    bool counting = false;          // lupin_hip_stats_reset(ctx, 2): the tracing kernels run their work-counting instantiation
    int accum_mode = 0;             // LUPIN_ACCUM_F16_RUNNING_AVERAGE | LUPIN_ACCUM_F32
    int runtime_version = 0;        // hipRuntimeGetVersion of the libamdhip64 this process bound
    int store_rounding = 0;        // LUPIN_STORE_ROUND_TOWARD_ZERO
    bool lds_geometry = true;       // LUPIN_LDS_GEOMETRY=0 keeps small scenes in global memory (A/B runs)
    int persistent_extend = 2;      // LUPIN_EXTEND: "simple" 0 | "persistent" 1 (always) | default 2: persistent for scenes traversed from global memory
    uint32_t num_cus = 256;
    bool specialize_simple = true;          // LUPIN_SIMPLE_SHADE=0: always the general k_shade
    bool use_graph = false;                 // LUPIN_GRAPH=1: replay the lane-private wavefront as a HIP graph (opt-in)
    bool persistent_shadow = true;          // LUPIN_SHADOW=simple: MIS / Direct shadow rays stay in k_shadow even on large scenes
    bool wide_traversal = false;           // LUPIN_TRAVERSAL=wide / lupin_hip_set_traversal: four-wide hierarchy + certificate + re-trace (same images, not faster: DESIGN 5)
    static constexpr uint32_t wide_stack_pairs = 20;   // (reference, distance) stack entries per lane of the wide tracer: 40 KB per block, four blocks per CU
    bool verify_wide = false;              // LUPIN_VERIFY_WIDE=1: every closest-hit query is also checked wide-vs-binary on the device (stats)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_extend, ev_shade, ev_total;
    std::vector<hipEvent_t> ev_pool;
    uint64_t extend_launches = 0;
    // Frames per wavefront: pathtrace_scene calls that differ only in camera / accum_counter and chain their textures
    // (each call's prev_frame is the previous call's render_target) are recorded here and run as ONE wavefront when the batch is
    // full or anything needs their result (flush_pending: sync, texture reads and writes, another kind of call, teardown).
    // An adaptive call (lupin_hip_pathtrace_scene_adaptive) is a record with `adaptive` set; it is never batched (K == 1).
    struct PendingFrame { FrameParams fp; LupinTexture *target; const LupinTexture *prev; LupinAdaptiveResources *adaptive = nullptr; };
    std::vector<PendingFrame> pending;
    const LupinScene *pending_scene = nullptr;
    uint32_t pending_type = 0;
    uint32_t batch_frames = 0;             // LUPIN_BATCH=1..16: calls per wavefront (1 = every call is its own wavefront); 0 = by dispatch size,
                                           // see frames_per_wavefront()
    int last_lanes = 0;                    // frames in flight the latest pathtrace call could use (reported by lupin_hip_stats_get)
    bool last_wide = false;                // ... and whether it ran the four-wide tracer
    uint32_t last_batch = 0, last_short = 0;   // frames the latest wavefront carried; its first-pass stack entries (0 = one pass)
    // the scene queries' device check of records: its counter of refused records (count_bad_records), made by the first check
    DeviceBuffer bad_records;
    // lupin_hip_occlusion_rays: the staging of host arrays (one chunk's records and counts), kept from call to call and grown
    // when a call needs more (grow_buffer); freed with the context
    DeviceBuffer occ_records, occ_counts;
    size_t occ_records_bytes = 0, occ_counts_bytes = 0;
    // lupin_hip_transmittance_rays: it shares the two buffers above (a result is four bytes, as a count is) and adds the
    // per-slot plane of hemisphere mode (one float per slot of a chunk), kept and grown the same way
    DeviceBuffer trans_plane;
    size_t trans_plane_bytes = 0;
    // lupin_hip_bent_normal_rays: it shares occ_records and adds the staging of one chunk's results (four floats per record)
    DeviceBuffer bent_results;
    size_t bent_results_bytes = 0;
    // lupin_hip_distance_points / lupin_hip_bake_distance_grid: the same for the distance queries, and the per-instance
    // auxiliary array (local -> world rows and c_i) that every call rebuilds from the scene's current rows
    DeviceBuffer dist_records, dist_results, dist_aux;
    size_t dist_records_bytes = 0, dist_results_bytes = 0, dist_aux_bytes = 0;
    // lupin_hip_sample_probe_grid: the staging of host arrays (the grid's coefficients and validity bytes, one chunk's
    // records and results), kept and grown the same way
    DeviceBuffer grid_sh, grid_valid, grid_records, grid_results;
    size_t grid_sh_bytes = 0, grid_valid_bytes = 0, grid_records_bytes = 0, grid_results_bytes = 0;
    // lupin_hip_denoise_lightmap: the staging of host arrays (rgba, which is also where the result lands, and records) and the
    // filter's scratch (two (irradiance, variance) planes, the two guide planes, the footprint, two `filled` planes for
    // the gutter passes), kept and grown the same way
    enum { LMD_RGBA, LMD_RECORDS, LMD_IV0, LMD_IV1, LMD_G0, LMD_G1, LMD_FOOT, LMD_FILLED0, LMD_FILLED1, LMD_BUFFERS };
    DeviceBuffer lmd[LMD_BUFFERS];
    size_t lmd_bytes[LMD_BUFFERS] = {};
};

struct LupinPathtraceResources
{
    LupinContext *ctx;
    LupinBakedPathtraceParams params;
};

// adaptive sampling's per-pixel and per-block state (lupin_adaptive.hpp)
struct LupinAdaptiveResources
{
    LupinContext *ctx = nullptr;
    int device = 0;
    AdaptiveDev dev{};   // device pointers, size and the latest call's parameters: the plain view the kernels get by value
    DeviceBuffer frames, moments, block_error, block_flags, block_active, block_count, stats;   // own what dev's pointers of the same names point to
    uint32_t calls = 0;  // adaptive calls since the latest reset
};

struct LupinDoubleBufferedTexture
{
    LupinContext *ctx;
    LupinTexture *tex[2];
    int front_idx, back_idx;
};

struct LupinScene
{
    LupinContext *ctx;
    int device = 0;                                 // the context's device ordinal (the scene may outlive the context)
    SceneDev dev{};
    std::vector<DeviceBuffer> allocations;          // everything `dev` points to
    uint32_t stack_entries = 1;
    // grids of k_extend_persistent per integrator, filled on first use by resident_grid (so `mutable`: a render takes the scene const)
    mutable uint32_t persistent_blocks[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};   // binary; [1]: sharing the chip with other lanes' stages
    mutable uint32_t wide_blocks[4] = {0, 0, 0, 0};         // its four-wide instantiation
    mutable uint32_t short_blocks[4] = {0, 0, 0, 0};        // its short-stack instantiation
    bool has_wide = false;                          // the four-wide hierarchies were built (scenes traversed from global memory)
    uint64_t leaky_triangles = 0;                   // triangles outside some box above them (reference builder: bins vs partition)
    uint64_t id = 0;                                // unique per created scene (graph cache key)
    bool all_opaque = false;                        // no instance can have opacity != 1: k_extend<.., OPAQUE> drops the alpha test
    bool simple_matte = false;                      // only untextured matte materials, no vertex colours, no environments: k_shade<.., SIMPLE>
    bool has_sw_bvh = false;
    bool envs_empty = true, lights_empty = true, instances_empty = true;
    // host-side copies lupin_hip_scene_update_instances works from
    std::vector<float> model_aabbs;                 // per mesh: f32 min xyz, max xyz of verts_pos (Aabb::neutral() for an empty mesh)
    std::vector<InstanceDev> host_instances;        // as uploaded (mesh_idx, mat_idx, blas_root and flags never change)
    std::vector<uint32_t> light_instance;           // light -> instance
    std::vector<uint32_t> mesh_tri_count;           // per mesh; with num_textures what lupin_hip_surface_probe checks a record's indices against
    std::vector<uint8_t> mesh_has_texcoords;        // per mesh; lupin_hip_bake_lightmap refuses a chart on a mesh without them and without a lightmap set
    std::vector<uint32_t> mesh_vert_count;          // per mesh; lupin_hip_unwrap_lightmap_uvs sizes its (bucket, vertex) table by it
    std::vector<uint32_t> mesh_tri_offset;          // per mesh: MeshDev::tri_offset, its first global triangle
    std::vector<DeviceBuffer> lightmap_uvs;         // per mesh: the lightmap UV set (one float2 per triangle corner), empty without one
    const float2 *lightmap_set(uint32_t mesh) const { return lightmap_uvs[mesh].as<float2>(); }
    uint32_t num_textures = 0;
    std::vector<LupinTlasNode> tlas_nodes;          // the TLAS in lupin_build_tlas' format (lupin_hip_scene_get_tlas)
    uint32_t nblas = 0, ntlas = 0;                  // the one node array is [nblas BLAS nodes | ntlas TLAS nodes]
    uint32_t max_blas_depth = 0;
    bool wide_stale = false;                        // an update moved the instances: the four-wide TLAS describes the old ones
};

template <typename T>
static int upload(LupinScene *sc, const std::vector<T> &host, const T **out)
{
    *out = nullptr;
    size_t bytes = std::max<size_t>(host.size() * sizeof(T), sizeof(T) > 16 ? sizeof(T) : 16);
    sc->allocations.emplace_back();
    HIP_TRY(DeviceBuffer::make(bytes, &sc->allocations.back()));
    void *d = sc->allocations.back().get();
    HIP_TRY(hipMemsetAsync(d, 0, bytes, sc->ctx->stream));
    if (!host.empty()) HIP_TRY(hipMemcpyAsync(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, sc->ctx->stream));
    *out = reinterpret_cast<const T *>(d);
    return LUPIN_OK;
}

static hipEvent_t get_event(LupinContext *ctx)
{
    if (!ctx->ev_pool.empty()) { hipEvent_t e = ctx->ev_pool.back(); ctx->ev_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    hipEventCreate(&e);
    return e;
}

// Points the lane's per-bounce fields into its HOT allocation: planes (neighbouring slots coalesce) or 128-byte records
// (scattered slots cost two sectors per path, not one per field).  See PathField.
static void set_path_layout(Lane *ln, bool records)
{
    PathBuffers &pb = ln->pb;
    char *b = ln->path[Lane::HOT].as<char>();
    const size_t cap = (size_t)ln->capacity;
    pb.skey = {ln->path[Lane::SKEY].as<char>(), 4};   // always a plane: k_sort_queue reads nothing else of a path
    if (records)
    {
        const uint32_t st = LP_PATH_RECORD_BYTES;
        pb.ori_rng = {b + 0, st}; pb.dir_meta = {b + 16, st}; pb.hit = {b + 32, st}; pb.hit_tri = {b + 48, st};
        pb.weight = {b + 64, st}; pb.radiance = {b + 80, st}; pb.color = {b + 96, st};
        char *m = ln->path[Lane::SHADOW].as<char>();
        pb.sh_org = {m + 0, st}; pb.sh_d0 = {m + 16, st}; pb.sh_d1 = {m + 32, st}; pb.next_tri = {m + 48, st};
        pb.sh_f0 = {m + 64, st}; pb.sh_f1 = {m + 80, st}; pb.next_hit = {m + 96, st}; pb.sh_hit1 = {m + 112, st};
    }
    else
    {
        pb.ori_rng = {b, 16}; pb.dir_meta = {b + 16 * cap, 16}; pb.hit = {b + 32 * cap, 16}; pb.weight = {b + 48 * cap, 16};
        pb.radiance = {b + 64 * cap, 16}; pb.color = {b + 80 * cap, 16}; pb.hit_tri = {b + 96 * cap, 4};
        char *m = ln->path[Lane::SHADOW].as<char>();
        pb.sh_org = {m, 16}; pb.sh_d0 = {m + 16 * cap, 16}; pb.sh_d1 = {m + 32 * cap, 16}; pb.sh_f0 = {m + 48 * cap, 16};
        pb.sh_f1 = {m + 64 * cap, 16}; pb.next_hit = {m + 80 * cap, 16}; pb.sh_hit1 = {m + 96 * cap, 16}; pb.next_tri = {m + 112 * cap, 4};
    }
}

// bytes per slot of Lane::path[k]; re-trace tokens: up to two jobs per slot (shadow rays)
static constexpr size_t kPathSlotBytes[Lane::NUM_PATH_BUFFERS] = {LP_PATH_RECORD_BYTES, LP_PATH_RECORD_BYTES, 4, 16, 16, 4, 4, 8, 4};

// pb's plain pointers follow their owners (null for an empty owner); the PathFields are set_path_layout's
static void set_path_views(Lane *ln)
{
    PathBuffers &pb = ln->pb;
    pb.vol0 = ln->path[Lane::VOL0].as<float4>(); pb.vol1 = ln->path[Lane::VOL1].as<float4>();
    pb.queue[0] = ln->path[Lane::QUEUE0].as<uint32_t>(); pb.queue[1] = ln->path[Lane::QUEUE1].as<uint32_t>();
    pb.retrace = ln->path[Lane::RETRACE].as<uint32_t>(); pb.shade_order = ln->path[Lane::SHADE_ORDER].as<uint32_t>();
    // queue counters, then the persistent tracer's hand-out cursors, the re-trace counters and the re-trace cursors (two
    // per iteration each): one allocation, one clear per call (an empty owner has counts_capacity 0: all four are null)
    const size_t row = (size_t)ln->counts_capacity * LP_SHARDS;
    pb.counts = ln->counts; pb.cursors = pb.counts + row; pb.retrace_counts = pb.cursors + 2 * row; pb.retrace_cursors = pb.retrace_counts + 2 * row;
}

static int ensure_path_buffers(LupinContext *ctx0, Lane *ctx, uint64_t slots, uint32_t iterations)
{
    (void)ctx0;
    // shard segments are whole blocks: round the queue length up to LP_SHARDS * LP_BLOCK
    const uint64_t per_round = (uint64_t)LP_SHARDS * LP_BLOCK;
    slots = (slots + per_round - 1) / per_round * per_round;
    if (slots > ctx->capacity)
    {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        // the lane holds nothing until every allocation has succeeded: a failure part-way (make returns through
        // HIP_TRY) must not leave a capacity behind that a later, smaller dispatch would trust.  All nine are freed before any
        // is allocated: the peak is the new size, not the old one plus the new
        ctx->capacity = 0;
        ctx->pb_generation++;
        for (DeviceBuffer &b : ctx->path) b.reset();
        set_path_views(ctx);
        for (int k = 0; k < Lane::NUM_PATH_BUFFERS; k++)
            HIP_TRY(DeviceBuffer::make((size_t)slots * kPathSlotBytes[k], &ctx->path[k]));
        // touch every page now (a fill runs at several TB/s): otherwise the first wavefront that reaches a slot pays the
        // mapping of its pages inside its kernels -- 1 % of the first full wavefront of eight 4K frames
        for (int k = 0; k < Lane::NUM_PATH_BUFFERS; k++)
            HIP_TRY(hipMemsetAsync(ctx->path[k].get(), 0, (size_t)slots * kPathSlotBytes[k], ctx->stream));
        ctx->capacity = slots;
        set_path_views(ctx);
    }
    if (iterations + 2 > ctx->counts_capacity)
    {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->counts_capacity = 0;
        ctx->counts.reset();
        set_path_views(ctx);
        HIP_TRY(ctx->counts.alloc(LP_COUNTER_ROWS * (size_t)(iterations + 2) * LP_SHARDS));
        ctx->counts_capacity = iterations + 2;
        set_path_views(ctx);
        ctx->pb_generation++;
    }
    return LUPIN_OK;
}

// Four-wide collapse of a binary hierarchy given as child-pair nodes (`bin`, references as in WideNode.d): starting from
// a node's two children, the internal child with the largest box surface is replaced by its own two children until the
// node has four children or only leaves.  Every child box is a box of the reference's tree, every leaf keeps its
// reference, so the set of triangles under a reference is unchanged.
// A child is opened only if BOTH its children's boxes lie inside its own box (exact comparison): then passing a
// grandchild's slab test implies passing the dropped child's (the slab test is monotone under box inclusion: same
// roundings of monotone operations), so the wide traversal skips nothing the reference's would not skip.  The
// reference's builder does produce boxes that are not nested (its child boxes come from centroid BINS, its partition from
// a comparison with the split plane; a triangle on the wrong side of that rounding is outside its node's stored box --
// first seen as the one ray in 8 x 10^5 whose closest hit the binary order misses): such a child stays a child.
// WideNode.d.z carries, per child of a pair (bit 0 left, bit 1 right), "some triangle below is not inside this child's
// box" (blas_child_pairs); it becomes REF_LEAKY in the wide node's child reference: those children are never pruned by distance.  Nodes are appended to `out` in depth-first order
// (a 128-byte node is a cache line of its own: order among nodes does not matter to the caches).  Returns the root
// reference (a leaf root passes through).
static uint32_t collapse_to_wide4(const std::vector<WideNode> &bin, uint32_t root_ref, std::vector<Wide4> &out, uint32_t *out_depth = nullptr)
{
    if (out_depth) *out_depth = 0;
    if (root_ref & REF_LEAF) return root_ref;
    struct Child { float lo[3], hi[3]; uint32_t ref; bool leaky, closed; };
    auto children_of = [&](uint32_t b, Child &l, Child &r) {
        const WideNode &w = bin[b];
        l.lo[0] = w.a.x; l.lo[1] = w.a.z; l.lo[2] = w.b.x; l.hi[0] = w.b.z; l.hi[1] = w.c.x; l.hi[2] = w.c.z; l.ref = w.d.x;
        r.lo[0] = w.a.y; r.lo[1] = w.a.w; r.lo[2] = w.b.y; r.hi[0] = w.b.w; r.hi[1] = w.c.y; r.hi[2] = w.c.w; r.ref = w.d.y;
        l.leaky = (w.d.z & 1u) != 0; r.leaky = (w.d.z & 2u) != 0;
        l.closed = r.closed = false;
    };
    auto inside = [](const Child &in, const Child &out) {   // exact; a NaN bound is "not inside"
        for (int ax = 0; ax < 3; ax++)
            if (!(in.lo[ax] >= out.lo[ax] && in.hi[ax] <= out.hi[ax])) return false;
        return true;
    };
    auto area = [](const Child &c) {
        const double ex = (double)c.hi[0] - c.lo[0], ey = (double)c.hi[1] - c.lo[1], ez = (double)c.hi[2] - c.lo[2];
        const double a = ex * ey + ey * ez + ez * ex;
        return a == a ? a : 0.0;
    };
    struct Item { uint32_t bin_node, wide_node, depth; };
    std::vector<Item> todo;
    const uint32_t root = (uint32_t)out.size();
    out.emplace_back();
    todo.push_back({root_ref, root, 1u});
    const float nanf_ = std::nanf("");
    while (!todo.empty())
    {
        const Item it = todo.back();
        todo.pop_back();
        if (out_depth) *out_depth = std::max(*out_depth, it.depth);
        Child c[4];
        int n = 2;
        children_of(it.bin_node, c[0], c[1]);
        while (n < 4)
        {
            int pick = -1;
            double best = -1.0;
            for (int k = 0; k < n; k++)
                if (!(c[k].ref & REF_LEAF) && !c[k].closed) { const double a = area(c[k]); if (a > best) { best = a; pick = k; } }
            if (pick < 0) break;
            Child l, r;
            children_of(c[pick].ref, l, r);
            if (!inside(l, c[pick]) || !inside(r, c[pick])) { c[pick].closed = true; continue; }   // not nested: this box must be tested
            c[pick] = l;
            c[n++] = r;
        }
        Wide4 w;
        float *lo[3] = {&w.lox.x, &w.loy.x, &w.loz.x}, *hi[3] = {&w.hix.x, &w.hiy.x, &w.hiz.x};
        uint32_t refs[4];
        for (int k = 0; k < 4; k++)
        {
            for (int ax = 0; ax < 3; ax++) { lo[ax][k] = k < n ? c[k].lo[ax] : nanf_; hi[ax][k] = k < n ? c[k].hi[ax] : nanf_; }
            refs[k] = REF_NONE;
            if (k < n)
            {
                if (c[k].ref & REF_LEAF) refs[k] = c[k].ref;
                else
                {
                    refs[k] = (uint32_t)out.size();
                    out.emplace_back();
                    todo.push_back({c[k].ref, refs[k], it.depth + 1});
                }
            }
        }
        for (int k = 0; k < n; k++) if (c[k].leaky) refs[k] |= REF_LEAKY;
        w.ref = make_uint4(refs[0], refs[1], refs[2], refs[3]);
        w.pad = make_uint4(0u, 0u, 0u, 0u);
        out[it.wide_node] = w;
    }
    return root;
}

// One mesh's BLAS (the reference's BvhNode array, data_structures.rs:196-325) as child-pair nodes appended to `blas`:
// node index -> child reference (leaf: REF_LEAF | global index of its first triangle; internal: index into `blas`).
// `leaf_ends` receives the global index of every leaf's last triangle.  Returns the root reference; *why != nullptr on a
// malformed array (the caller has checked that the array is a tree).
// With vertex data (verts_pos4 / indices, mesh-local) the boxes are also checked against what they should bound -- the wide
// tracer's certificate needs to know where the reference's boxes do not:
//   WideNode.d.z bit 0 / 1  the left / right child's stored box does not contain every triangle below it
//   leaky_tris              (global indices) triangles that are not inside every box above them, leaf box included
static uint32_t blas_child_pairs(const LupinBvhNode *nodes, uint32_t num_nodes, uint32_t ntris, uint32_t tri_offset, std::vector<WideNode> &blas,
                                 std::vector<uint32_t> &leaf_ends, const char **why,
                                 const float *verts_pos4 = nullptr, const uint32_t *indices = nullptr, std::vector<uint32_t> *leaky_tris = nullptr)
{
    *why = nullptr;
    std::vector<uint32_t> ref(num_nodes);
    uint32_t wide_base = (uint32_t)blas.size(), wide_count = 0;
    for (uint32_t n = 0; n < num_nodes; n++)
    {
        const LupinBvhNode &nd = nodes[n];
        if (nd.tri_count > 0)
        {
            if ((uint64_t)nd.tri_begin_or_first_child + nd.tri_count > ntris) { *why = "BLAS leaf range out of bounds"; return 0; }
            ref[n] = REF_LEAF | (tri_offset + nd.tri_begin_or_first_child);
            leaf_ends.push_back(tri_offset + nd.tri_begin_or_first_child + nd.tri_count - 1);
        }
        else
        {
            if ((uint64_t)nd.tri_begin_or_first_child + 1 >= num_nodes) { *why = "BLAS child index out of bounds"; return 0; }
            ref[n] = wide_base + wide_count++;
        }
    }
    // what the boxes should bound: true bounds per node (bottom-up) and, top-down, the intersection of the boxes above a leaf
    std::vector<uint8_t> leaky_node(num_nodes, 0);
    if (verts_pos4 && indices)
    {
        struct B { float lo[3], hi[3]; };
        auto tri_bounds = [&](uint32_t t) {
            B b;
            for (int ax = 0; ax < 3; ax++) { b.lo[ax] = INFINITY; b.hi[ax] = -INFINITY; }
            for (int k = 0; k < 3; k++)
                for (int ax = 0; ax < 3; ax++)
                {
                    const float x = verts_pos4[(size_t)indices[(size_t)t * 3 + k] * 4 + ax];
                    b.lo[ax] = std::min(b.lo[ax], x); b.hi[ax] = std::max(b.hi[ax], x);
                }
            return b;
        };
        std::vector<B> truth(num_nodes);
        // iterative post-order over the tree rooted at node 0 (children may have any index)
        std::vector<std::pair<uint32_t, int>> st;
        st.push_back({0u, 0});
        while (!st.empty())
        {
            auto [n, phase] = st.back();
            const LupinBvhNode &nd = nodes[n];
            if (nd.tri_count > 0)
            {
                B b;
                for (int ax = 0; ax < 3; ax++) { b.lo[ax] = INFINITY; b.hi[ax] = -INFINITY; }
                for (uint32_t t = nd.tri_begin_or_first_child; t < nd.tri_begin_or_first_child + nd.tri_count; t++)
                {
                    const B tb = tri_bounds(t);
                    for (int ax = 0; ax < 3; ax++) { b.lo[ax] = std::min(b.lo[ax], tb.lo[ax]); b.hi[ax] = std::max(b.hi[ax], tb.hi[ax]); }
                }
                truth[n] = b;
                st.pop_back();
            }
            else if (phase == 0)
            {
                st.back().second = 1;
                st.push_back({nd.tri_begin_or_first_child, 0});
                st.push_back({nd.tri_begin_or_first_child + 1, 0});
                continue;
            }
            else
            {
                const B &l = truth[nd.tri_begin_or_first_child], &r = truth[nd.tri_begin_or_first_child + 1];
                for (int ax = 0; ax < 3; ax++) { truth[n].lo[ax] = std::min(l.lo[ax], r.lo[ax]); truth[n].hi[ax] = std::max(l.hi[ax], r.hi[ax]); }
                st.pop_back();
            }
            bool in = true;
            for (int ax = 0; ax < 3; ax++) in = in && truth[n].lo[ax] >= nd.aabb_min[ax] && truth[n].hi[ax] <= nd.aabb_max[ax];
            leaky_node[n] = in ? 0 : 1;
        }
        if (leaky_tris)
        {
            // top-down: clip = intersection of the stored boxes from the root down to the node
            std::vector<std::pair<uint32_t, B>> down;
            B all;
            for (int ax = 0; ax < 3; ax++) { all.lo[ax] = -INFINITY; all.hi[ax] = INFINITY; }
            down.push_back({0u, all});
            while (!down.empty())
            {
                auto [n, clip] = down.back();
                down.pop_back();
                const LupinBvhNode &nd = nodes[n];
                for (int ax = 0; ax < 3; ax++) { clip.lo[ax] = std::max(clip.lo[ax], nd.aabb_min[ax]); clip.hi[ax] = std::min(clip.hi[ax], nd.aabb_max[ax]); }
                if (nd.tri_count > 0)
                {
                    for (uint32_t t = nd.tri_begin_or_first_child; t < nd.tri_begin_or_first_child + nd.tri_count; t++)
                    {
                        const B tb = tri_bounds(t);
                        bool in = true;
                        for (int ax = 0; ax < 3; ax++) in = in && tb.lo[ax] >= clip.lo[ax] && tb.hi[ax] <= clip.hi[ax];
                        if (!in) leaky_tris->push_back(tri_offset + t);
                    }
                }
                else
                {
                    down.push_back({nd.tri_begin_or_first_child, clip});
                    down.push_back({nd.tri_begin_or_first_child + 1, clip});
                }
            }
        }
    }
    blas.resize(wide_base + wide_count);
    for (uint32_t n = 0; n < num_nodes; n++)
    {
        const LupinBvhNode &nd = nodes[n];
        if (nd.tri_count > 0) continue;
        const uint32_t lc = nd.tri_begin_or_first_child, rc = lc + 1;
        const LupinBvhNode &l = nodes[lc];
        const LupinBvhNode &r = nodes[rc];
        WideNode w;
        w.a = make_float4(l.aabb_min[0], r.aabb_min[0], l.aabb_min[1], r.aabb_min[1]);
        w.b = make_float4(l.aabb_min[2], r.aabb_min[2], l.aabb_max[0], r.aabb_max[0]);
        w.c = make_float4(l.aabb_max[1], r.aabb_max[1], l.aabb_max[2], r.aabb_max[2]);
        w.d = make_uint4(ref[lc], ref[rc], (leaky_node[lc] ? 1u : 0u) | (leaky_node[rc] ? 2u : 0u), 0u);
        blas[ref[n]] = w;
    }
    return ref[0];
}

// depth of a hierarchy in internal levels = worst-case number of parked far children
// depth of a BLAS in internal levels; UINT32_MAX for a node array that is not a tree (bounded walk, like the TLAS check)
static uint32_t blas_depth(const LupinBvhNode *nodes, uint32_t count)
{
    if (count == 0) return 0;
    uint32_t best = 0;
    uint64_t visited = 0;
    std::vector<std::pair<uint32_t, uint32_t>> st;
    st.push_back({0u, 0u});
    while (!st.empty())
    {
        auto [n, d] = st.back();
        st.pop_back();
        if (++visited > (uint64_t)count + 1) return 0xFFFFFFFFu;
        if (nodes[n].tri_count == 0)
        {
            best = std::max(best, d + 1);
            st.push_back({nodes[n].tri_begin_or_first_child, d + 1});
            st.push_back({nodes[n].tri_begin_or_first_child + 1, d + 1});
        }
    }
    return best;
}

// ------------------------------------------------------------------------------------------------
// Launch plan.  A run-time choice becomes a kernel variant through with_type / with_bool at the launch that needs it (an
// `if constexpr` keeps out the combinations that are never launched); whatever a kernel asks of LDS is added in traversal_lds.
// ------------------------------------------------------------------------------------------------

// f(std::integral_constant<int, TYPE>) for the integrator `type` (pathtrace_impl has checked its range)
template <typename F>
static auto with_type(uint32_t type, F &&f)
{
    switch (type)
    {
    case LUPIN_PATHTRACE_STANDARD: return f(std::integral_constant<int, LUPIN_PATHTRACE_STANDARD>{});
    case LUPIN_PATHTRACE_MIS: return f(std::integral_constant<int, LUPIN_PATHTRACE_MIS>{});
    case LUPIN_PATHTRACE_NAIVE: return f(std::integral_constant<int, LUPIN_PATHTRACE_NAIVE>{});
    default: return f(std::integral_constant<int, LUPIN_PATHTRACE_DIRECT>{});
    }
}
// f(std::true_type) or f(std::false_type)
template <typename F>
static auto with_bool(bool b, F &&f)
{
    if (b) return f(std::true_type{});
    return f(std::false_type{});
}

// What the traversal of one launch takes of LDS: `stack_words` of per-lane stacks in front of the scene's staged geometry.
struct TraversalLds
{
    bool geo = false;            // the kernel reads the scene from LDS (its LDSGEO instantiation)
    uint32_t stack_words = 0;
    size_t lds = 0;              // bytes
};
static constexpr size_t LP_LDS_LIMIT = 160 * 1024;   // the LDS of a CU, which one block may have to itself

// small scenes are staged in LDS by the one-ray-per-lane kernels (LUPIN_LDS_GEOMETRY=0: never)
static bool stages_geometry(const LupinContext *ctx, const LupinScene *scene) { return scene->dev.geo_blob_words && ctx->lds_geometry; }

// `stack_entries` per lane: the scene's depth bound, a tracer's own bound, or 0 for a kernel that never traverses.
// `stage` is false for the kernels that read the geometry from global memory whatever the scene (the persistent tracers, k_trace).
static int traversal_lds(const LupinContext *ctx, const LupinScene *scene, uint32_t stack_entries, bool stage, TraversalLds *out)
{
    out->geo = stage && stages_geometry(ctx, scene);
    out->stack_words = stack_entries * LP_BLOCK;
    out->lds = (size_t)out->stack_words * sizeof(uint32_t) + (out->geo ? (size_t)scene->dev.geo_blob_words * 16 : 0);
    if (out->lds > LP_LDS_LIMIT) return fail(LUPIN_ERR_INVALID_ARGUMENT, "BVH too deep for the LDS traversal stack");
    return LUPIN_OK;
}

// Grid of a persistent tracer: as many blocks of `kernel` as the device keeps resident with `lds` bytes each (whole waves
// per shard), after `per_cu_rule` has had its say.  Queried once per scene, integrator and instantiation, outside any
// stream capture, and kept in `cached`.
template <typename Kernel, typename Rule = int (*)(int)>
static uint32_t resident_grid(const LupinContext *ctx, Kernel kernel, size_t lds, uint32_t &cached, Rule per_cu_rule = [](int per_cu) { return per_cu; })
{
    if (cached == 0)
    {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, LP_BLOCK, lds) != hipSuccess || per_cu < 1) per_cu = 1;
        cached = std::max(64u, ctx->num_cus * (uint32_t)per_cu_rule(per_cu) / 64u * 64u);
    }
    return cached;
}

// The phase-scheduled persistent tracer serves scenes traversed from global memory; scenes staged in LDS (a few dozen node
// visits per ray) are faster with one ray per lane (k_extend; Cornell box 6.4 vs 5.4 Gsamples/s in round 1).
// LUPIN_EXTEND=simple forces k_extend everywhere.
static bool use_persistent(const LupinContext *ctx, bool lds_geo) { return ctx->persistent_extend != 0 && !lds_geo; }

// LUPIN_LIGHT_STAGE=1: sample_lights_pdf of the Standard / MIS integrators runs in its own stage (k_light_pdf / k_light_pdf_mis) instead of inline
// in k_shade.  Same results; off by default (faster kernel for kernel, slower with frames in flight).
static bool use_light_stage(const LupinContext *ctx, const LupinScene *scene, uint32_t type)
{
    if (scene->simple_matte && ctx->specialize_simple) return false;
    if (ctx->light_stage >= 0) return ctx->light_stage > 0;
    // default: MIS runs its two sample_lights_pdf evaluations per vertex in k_light_pdf_mis (k_shade<MIS, DEFER> is then
    // straight-line BSDF code at 138 VGPRs instead of 256 + scratch with the marches inline); the Standard integrator keeps
    // its single evaluation inline (faster with frames in flight)
    return type == LUPIN_PATHTRACE_MIS;
}

// launch shape of one call's stage kernels
struct TracerGrid
{
    uint32_t blocks = 0;         // 0 = off
    size_t lds = 0;
    uint32_t stack_words = 0;
};
struct Shape
{
    uint32_t blocks = 0;         // one thread per slot, LP_SHARDS-aligned
    bool lds_geo = false;        // the stage kernels read the scene from LDS
    TracerGrid binary;           // persistent tracer (binary hierarchy); blocks == 0 = the one-ray-per-lane k_extend.  Its lds and
                                 // stack_words, traversal stacks (+ staged geometry), serve every one-thread-per-slot stage as well
    TracerGrid wide;             // four-wide tracer
    TracerGrid shrt;             // short-stack first pass of the binary tracer
    size_t verify_lds = 0;       // k_verify_wide walks both hierarchies: the larger of the binary and the four-wide stacks
};

// The persistent tracers of one call: which run, their LDS and their grids.  `t` is the call's traversal_lds.
static void plan_tracers(LupinContext *ctx, const LupinScene *scene, uint32_t type, bool chip_to_itself, const TraversalLds &t, Shape *sh)
{
    // a tracer's own stack bound, never staged geometry; both are below limits checked before (40 KB; less than t.lds)
    auto stacks = [&](uint32_t entries) { TraversalLds x; traversal_lds(ctx, scene, entries, false, &x); return TracerGrid{0u, x.lds, x.stack_words}; };
    // the wide tracer keeps (reference, distance) pairs on a bounded stack; a query that would overflow it is re-traced
    const TracerGrid wide_stacks = stacks(2u * ctx->wide_stack_pairs);
    sh->lds_geo = t.geo;
    sh->binary = TracerGrid{0u, t.lds, t.stack_words};
    sh->verify_lds = std::max(t.lds, wide_stacks.lds);
    if (!use_persistent(ctx, t.geo)) return;
    const bool wide = scene->has_wide && ctx->wide_traversal;
    // A fifth block per CU for scenes whose depth bound asks for more than 32 KB of stack per block (bistro-class: 40):
    // the tracer is bound by latency x waves (four blocks instead of three: -18 %, five instead of four: -10 %), and the
    // stack a query actually uses is far below the bound (bistro-class 4K: 33 of 3.5 G queries need more than 20 entries).
    // Only with the chip to itself: sharing it, the larger tracer loses more to the other lanes' stages than it gains.
    const bool shrt = !wide && chip_to_itself && ctx->short_stack && scene->stack_entries > ctx->short_stack;
    if (wide) sh->wide = wide_stacks;
    if (shrt) sh->shrt = stacks(ctx->short_stack);
    with_type(type, [&](auto T) {
        constexpr int TYPE = decltype(T)::value;
        // With frames in flight the persistent tracer of one frame shares the chip with the shading of another: when five
        // or more of its blocks fit per CU, three leave that room and the pair finishes sooner (materials1 / environments1
        // +5 %); deeper scenes fit four at most and are latency-bound, they keep them all (bistro-class -9 % with two).
        const bool shares_chip = !chip_to_itself;
        sh->binary.blocks = resident_grid(ctx, k_extend_persistent<TYPE, false, 0, false>, sh->binary.lds, scene->persistent_blocks[shares_chip ? 1 : 0][TYPE],
                                          [=](int per_cu) { return shares_chip && per_cu > 4 ? 3 : per_cu; });
        // the other instantiations have their own LDS footprint and register count
        if (wide) sh->wide.blocks = resident_grid(ctx, k_extend_persistent<TYPE, false, 0, false, true, false>, sh->wide.lds, scene->wide_blocks[TYPE]);
        if (shrt) sh->shrt.blocks = resident_grid(ctx, k_extend_persistent<TYPE, false, 0, false, false, false, true>, sh->shrt.lds, scene->short_blocks[TYPE]);
    });
}

// The launch shape of a wavefront of `n` slots on lane `ln`: every shard gets the same number of blocks, block b serves shard
// b % LP_SHARDS (the lane's shard capacity follows from it), then the tracers.
static Shape plan_wavefront(LupinContext *ctx, Lane *ln, const LupinScene *scene, uint32_t type, bool chip_to_itself, const TraversalLds &t, uint32_t n)
{
    const uint32_t blocks_needed = (n + LP_BLOCK - 1) / LP_BLOCK;
    const uint32_t blocks_per_shard = (blocks_needed + LP_SHARDS - 1) / LP_SHARDS;
    ln->pb.shard_cap = blocks_per_shard * LP_BLOCK;
    Shape sh;
    sh.blocks = blocks_per_shard * LP_SHARDS;
    plan_tracers(ctx, scene, type, chip_to_itself, t, &sh);
    return sh;
}

// the tracing stage of MODE 0 (closest hits of the integrator loop) or 1 (recorded shadow rays) on the persistent tracer
template <int TYPE, int MODE>
static void launch_persistent_tracer(LupinContext *ctx, Lane *ln, const LupinScene *scene, const Shape &sh, uint32_t iter)
{
    auto launch = [&](auto kernel, const TracerGrid &g) {
        hipLaunchKernelGGL(kernel, dim3(g.blocks), dim3(LP_BLOCK), g.lds, ln->stream, scene->dev, (const FrameParams *)ln->d_fp, ln->pb, iter, ln->stat_counters,
                           LP_REFILL_MIN, g.stack_words, LP_NODE_STEPS, ln->work_counters, ln->wide_counters);
    };
    with_bool(ctx->counting, [&](auto C) {
        constexpr bool COUNT = decltype(C)::value;
        if (sh.wide.blocks)
        {
            // four-wide traversal with the exactness certificate, then the queries it did not certify in the reference's order
            launch(k_extend_persistent<TYPE, false, MODE, COUNT, true, false>, sh.wide);
            launch(k_extend_persistent<TYPE, false, MODE, COUNT, false, true>, sh.binary);
            return;
        }
        if constexpr (!COUNT)   // the short-stack pass does not count work
        {
            if (sh.shrt.blocks)
            {
                // the binary traversal on a short stack (one more block per CU), then the few queries that needed the full one
                launch(k_extend_persistent<TYPE, false, MODE, false, false, false, true>, sh.shrt);
                launch(k_extend_persistent<TYPE, false, MODE, false, false, true>, sh.binary);
                return;
            }
        }
        launch(k_extend_persistent<TYPE, false, MODE, COUNT>, sh.binary);
    });
}

template <int TYPE, bool LDSGEO>
static void launch_iteration(LupinContext *ctx, Lane *ln, const LupinScene *scene, const Shape &sh, uint32_t iter)
{
    const uint32_t blocks = sh.blocks, stack_words = sh.binary.stack_words;
    const size_t lds = sh.binary.lds;
    hipStream_t st = ln->stream;
    const FrameParams *fp = ln->d_fp;
    hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
    if (ctx->timing) { e0 = get_event(ctx); e1 = get_event(ctx); e2 = get_event(ctx); hipEventRecord(e0, st); }
    const bool persistent = sh.binary.blocks != 0;
    unsigned long long *work = ln->work_counters;
    if constexpr (!LDSGEO)
    {
        if (ctx->verify_wide && scene->has_wide)   // checker only: every query of this iteration, binary vs wide, one ray per lane
            hipLaunchKernelGGL(k_verify_wide<0>, dim3(blocks), dim3(LP_BLOCK), sh.verify_lds, st,
                               scene->dev, fp, ln->pb, iter, ctx->wide_stack_pairs, ln->wide_counters + 2);
    }
    bool traced = false;
    if constexpr (!LDSGEO) { if (persistent) { launch_persistent_tracer<TYPE, 0>(ctx, ln, scene, sh, iter); traced = true; } }
    if (!traced)
    {
        with_bool(scene->all_opaque && ctx->specialize_simple, [&](auto O) {
            with_bool(ctx->counting, [&](auto C) {
                hipLaunchKernelGGL((k_extend<TYPE, LDSGEO, decltype(O)::value, decltype(C)::value>), dim3(blocks), dim3(LP_BLOCK), lds, st, scene->dev, fp, ln->pb, iter,
                                   ln->stat_counters, stack_words, work);
            });
        });
    }
    if (ctx->timing) hipEventRecord(e1, st);
    if (ctx->debug_sync)
    {
        hipError_t de = hipStreamSynchronize(st);
        fprintf(stderr, "[lupin] iteration %u type %d: extend done: %s\n", iter, TYPE, hipGetErrorString(de)); fflush(stderr);
    }
    bool light_stage = false;
    if constexpr (TYPE == LUPIN_PATHTRACE_STANDARD || TYPE == LUPIN_PATHTRACE_MIS) light_stage = use_light_stage(ctx, scene, TYPE);
    // several material families: sort the queue in windows first, k_shade then finds its 256 paths (nearly) uniform.  The sort
    // leaves the queue as it is and hands k_shade a permutation (pb.shade_order); shade_dev.sort_shade tells k_shade it ran.
    // MIS / Direct sort in place: their k_shade keeps its registers, and k_shadow appends in the sorted order as before.
    SceneDev shade_dev = scene->dev;
    shade_dev.sort_shade = 0;
    const uint32_t windows = ((blocks / LP_SHARDS) * LP_BLOCK + LP_SORT_WINDOW - 1) / LP_SORT_WINDOW;
    const uint32_t sort_in_place = TYPE == LUPIN_PATHTRACE_MIS || TYPE == LUPIN_PATHTRACE_DIRECT;
    if (scene->dev.sort_shade && scene->dev.num_instances)
    {
        // the Standard integrator's persistent tracer leaves the key with the hit; otherwise the pass derives it
        if (TYPE == LUPIN_PATHTRACE_STANDARD && persistent)
            hipLaunchKernelGGL((k_sort_queue<true, true>), dim3(windows * LP_SHARDS), dim3(LP_BLOCK), 0, st, scene->dev, ln->pb, iter, sort_in_place);
        else
            hipLaunchKernelGGL((k_sort_queue<TYPE == LUPIN_PATHTRACE_STANDARD, false>), dim3(windows * LP_SHARDS), dim3(LP_BLOCK), 0, st, scene->dev, ln->pb, iter, sort_in_place);
        shade_dev.sort_shade = 1;
    }
    if (scene->simple_matte && ctx->specialize_simple)
        hipLaunchKernelGGL((k_shade<TYPE, LDSGEO, true>), dim3(blocks), dim3(LP_BLOCK), lds, st, shade_dev, fp, ln->pb, iter, ln->stat_counters, stack_words);
    else if (!light_stage)
        hipLaunchKernelGGL((k_shade<TYPE, LDSGEO, false>), dim3(blocks), dim3(LP_BLOCK), lds, st, shade_dev, fp, ln->pb, iter, ln->stat_counters, stack_words);
    // k_shade read through the permutation and left each verdict at its entry: the survivors go to the next queue in the
    // queue's order (light stage: k_light_pdf appends, walking the queue in its order; MIS / Direct: k_shadow appends)
    if (TYPE != LUPIN_PATHTRACE_MIS && TYPE != LUPIN_PATHTRACE_DIRECT && shade_dev.sort_shade && !light_stage)
        hipLaunchKernelGGL(k_compact_queue, dim3(windows * LP_SHARDS), dim3(LP_BLOCK), 0, st, ln->pb, iter);
    if constexpr (TYPE == LUPIN_PATHTRACE_STANDARD)
    {
        if (light_stage)
        {
            // sample_lights_pdf has its own stage: k_shade tags the vertices that need it, k_light_pdf finishes them and appends
            // (this k_shade never traverses: without LDS-staged geometry it needs the block sort's 256 words only)
            const size_t shade_lds = LDSGEO ? lds : std::min(lds, (size_t)LP_BLOCK * sizeof(uint32_t));
            hipLaunchKernelGGL((k_shade<TYPE, LDSGEO, false, true>), dim3(blocks), dim3(LP_BLOCK), shade_lds, st, shade_dev, fp, ln->pb, iter, ln->stat_counters, stack_words);
            hipLaunchKernelGGL((k_light_pdf<TYPE, LDSGEO>), dim3(blocks), dim3(LP_BLOCK), lds, st, scene->dev, fp, ln->pb, iter, stack_words);
        }
    }
    if constexpr (TYPE == LUPIN_PATHTRACE_MIS)
    {
        if (light_stage)
        {
            // the two MIS weights per vertex need sample_lights_pdf: k_shade parks the candidates, this pass weighs them
            hipLaunchKernelGGL((k_shade<TYPE, LDSGEO, false, true>), dim3(blocks), dim3(LP_BLOCK), lds, st, shade_dev, fp, ln->pb, iter, ln->stat_counters, stack_words);
            hipLaunchKernelGGL((k_light_pdf_mis<LDSGEO>), dim3(blocks), dim3(LP_BLOCK), lds, st, scene->dev, fp, ln->pb, iter, stack_words);
        }
    }
    if constexpr (TYPE == LUPIN_PATHTRACE_MIS || TYPE == LUPIN_PATHTRACE_DIRECT)   // shadow rays + path finish (booked with "shade" in the timing)
    {
        bool pretraced = false;
        if constexpr (!LDSGEO)
        {
            if (persistent && ctx->persistent_shadow)
            {
                // large scenes: the shadow rays go through the phase-scheduled persistent tracer as well, then a light finish pass
                if (ctx->verify_wide && scene->has_wide)
                    hipLaunchKernelGGL(k_verify_wide<1>, dim3(blocks), dim3(LP_BLOCK), sh.verify_lds, st,
                                       scene->dev, fp, ln->pb, iter, ctx->wide_stack_pairs, ln->wide_counters + 2);
                launch_persistent_tracer<TYPE, 1>(ctx, ln, scene, sh, iter);
                hipLaunchKernelGGL((k_shadow<TYPE, false, true>), dim3(blocks), dim3(LP_BLOCK), lds, st, scene->dev, fp, ln->pb, iter, stack_words);
                pretraced = true;
            }
        }
        if (!pretraced)
            hipLaunchKernelGGL((k_shadow<TYPE, LDSGEO, false>), dim3(blocks), dim3(LP_BLOCK), lds, st, scene->dev, fp, ln->pb, iter, stack_words);
    }
    if (ctx->debug_sync)
    {
        fprintf(stderr, "[lupin] iteration %u type %d: stages launched, syncing\n", iter, TYPE); fflush(stderr);
        hipError_t de = hipStreamSynchronize(st);
        fprintf(stderr, "[lupin] iteration %u: %s\n", iter, hipGetErrorString(de)); fflush(stderr);
    }
    if (ctx->timing)
    {
        hipEventRecord(e2, st);
        ctx->ev_extend.push_back({e0, e1});
        ctx->ev_shade.push_back({e1, e2});
    }
    ctx->extend_launches++;
}

// first rays of a radiance query's chunk (lupin_hip_pathtrace_rays): k_begin_rays instead of k_begin
struct RayBegin
{
    const float4 *records;   // the chunk's first record
    uint32_t samples;
    float4 *out_rays;        // the chunk's first slot, or nullptr
};

// first rays of a probe bake's chunk (lupin_hip_bake_probes): k_begin_probes
struct ProbeBegin
{
    const float4 *probes;    // the chunk's first probe
    uint32_t samples;
    float4 *out_rays;        // the chunk's first slot, or nullptr
};

// the lane-private part of one call: clear the queue counters, first rays, every iteration of the wavefront
static hipError_t enqueue_wavefront(LupinContext *ctx, Lane *ln, const LupinScene *scene, uint32_t pathtrace_type, uint32_t n,
                                    const Shape &sh, uint32_t iterations, const AdaptiveDev *ad = nullptr, const RayBegin *rays = nullptr,
                                    const ProbeBegin *probes = nullptr)
{
    const uint32_t blocks = sh.blocks;
    hipStream_t st = ln->stream;
    hipError_t e = hipMemsetAsync(ln->pb.counts, 0, LP_COUNTER_ROWS * (size_t)ln->counts_capacity * LP_SHARDS * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    if (ad)
        hipLaunchKernelGGL(k_begin_adaptive, dim3(blocks), dim3(LP_BLOCK), 0, st, (const FrameParams *)ln->d_fp, ln->pb, n,
                           (const uint8_t *)ad->block_active, (const uint32_t *)ad->frames, ad->blocks_x);
    else if (rays)
        hipLaunchKernelGGL(k_begin_rays, dim3(blocks), dim3(LP_BLOCK), 0, st, ln->pb, n, rays->records, rays->samples, rays->out_rays);
    else if (probes)
        hipLaunchKernelGGL(k_begin_probes, dim3(blocks), dim3(LP_BLOCK), 0, st, ln->pb, n, probes->probes, probes->samples, probes->out_rays);
    else
        hipLaunchKernelGGL(k_begin, dim3(blocks), dim3(LP_BLOCK), 0, st, (const FrameParams *)ln->d_fp, ln->pb, n);
    with_type(pathtrace_type, [&](auto T) {
        with_bool(sh.lds_geo, [&](auto G) {
            for (uint32_t it = 0; it < iterations; it++) launch_iteration<decltype(T)::value, decltype(G)::value>(ctx, ln, scene, sh, it);
        });
    });
    return hipSuccess;
}

// The wavefront as a replayed graph (LUPIN_GRAPH=1).  Everything between k_set_params and the resolve depends on the call only through
// *d_fp, so it is captured once per (scene, dispatch size, integrator, buffers) and replayed: one graph launch instead of 2-4 per iteration.
static int replay_wavefront(LupinContext *ctx, Lane *ln, const LupinScene *scene, uint32_t pathtrace_type, uint32_t n, const Shape &sh, uint32_t iterations)
{
    hipStream_t st = ln->stream;
    Lane::GraphKey key;
    key.scene_id = scene->id; key.pb_generation = ln->pb_generation; key.n = n; key.blocks = sh.blocks; key.type = pathtrace_type;
    key.iterations = iterations; key.stack_words = sh.binary.stack_words; key.lds = (uint32_t)sh.binary.lds; key.pblocks = sh.binary.blocks;
    key.persistent = ctx->persistent_extend;
    key.persistent_shadow = ctx->persistent_shadow ? 1 : 0; key.lds_geometry = sh.lds_geo ? 1 : 0;
    const TracerGrid &first_pass = sh.wide.blocks ? sh.wide : sh.shrt;   // at most one of the two runs
    key.wide_blocks = first_pass.blocks; key.wide_stack_words = first_pass.stack_words;
    const bool have = ln->graph_exec && key == ln->graph_key;
    if (!have && ln->graph_exec && !(key == ln->seen_key))
    {
        // the lane holds a graph of another shape and this one is new (shapes alternate, e.g. edge tiles): capturing
        // costs about a millisecond, so launch directly and re-capture only if the shape repeats
        ln->seen_key = key;
        HIP_TRY(enqueue_wavefront(ctx, ln, scene, pathtrace_type, n, sh, iterations));
        return LUPIN_OK;
    }
    if (!have)
    {
        if (ln->graph_exec) { hipGraphExecDestroy(ln->graph_exec); ln->graph_exec = nullptr; }
        if (ln->graph) { hipGraphDestroy(ln->graph); ln->graph = nullptr; }
        HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
        hipError_t ce = enqueue_wavefront(ctx, ln, scene, pathtrace_type, n, sh, iterations);
        hipError_t ee = hipStreamEndCapture(st, &ln->graph);
        if (ce != hipSuccess || ee != hipSuccess) return fail(LUPIN_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(ce != hipSuccess ? ce : ee));
        HIP_TRY(hipGraphInstantiate(&ln->graph_exec, ln->graph, nullptr, nullptr, 0));
        ln->graph_key = key;
    }
    else ctx->extend_launches += iterations;
    ln->seen_key = key;
    HIP_TRY(hipGraphLaunch(ln->graph_exec, st));
    return LUPIN_OK;
}

// Lane `ln` waits for everything enqueued so far on the primary stream (texture uploads and copies, an adaptive reset;
// lane 0 is that stream) and on the lane of the wavefront before (its resolve, an adaptive call's update).
static int order_lane(LupinContext *ctx, Lane *ln)
{
    const int w = (int)(ln - ctx->lanes);
    if (w != 0)
    {
        HIP_TRY(hipEventRecord(ctx->marker, ctx->stream));
        HIP_TRY(hipStreamWaitEvent(ln->stream, ctx->marker, 0));
    }
    if (ctx->last_lane >= 0 && ctx->last_lane != w)
        HIP_TRY(hipStreamWaitEvent(ln->stream, ctx->lanes[ctx->last_lane].done, 0));
    return LUPIN_OK;
}

static int flush_pending(LupinContext *ctx);

// The gate (DESIGN 5 "Recorded frames run first"): every reader / writer of a texture on the primary stream comes through here, or
// through sync_all, before any work of its own.  The recorded calls run; if they fail, their code is the caller's and their message stays.
// The resolves form a chain (each waits for the previous call's), so the latest call's event covers all lanes' texture writes.
static int join_primary(LupinContext *ctx)
{
    if (int rc = flush_pending(ctx)) return rc;
    if (ctx->last_lane > 0) hipStreamWaitEvent(ctx->stream, ctx->lanes[ctx->last_lane].done, 0);
    return LUPIN_OK;
}
// ... and the host waits for every lane.  The lanes are drained even when the batch failed: teardown frees what they may use.
static int sync_all(LupinContext *ctx)
{
    int rc = flush_pending(ctx);
    for (int k = 0; k < LP_MAX_LANES; k++)
    {
        hipError_t e = ctx->lanes[k].stream ? hipStreamSynchronize(ctx->lanes[k].stream) : hipSuccess;
        if (e != hipSuccess && rc == LUPIN_OK) rc = fail(LUPIN_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    }
    return rc;
}

// "Records in, launch, records out" on the primary stream, in scratch buffers that live for the call.  `launch` gets the
// device copies of `in` (in order) and the output buffer and enqueues the kernel; errors are reported under `who`.
struct ProbeInput { const void *host; size_t bytes; };
template <size_t N, typename Launch>
static int run_probe(LupinContext *ctx, const char *who, const ProbeInput (&in)[N], void *out, size_t out_bytes, Launch launch)
{
    DeviceBuffer din[N], dout;
    hipError_t e = hipSuccess;
    for (size_t k = 0; k < N && e == hipSuccess; k++) e = DeviceBuffer::make(in[k].bytes, &din[k]);
    if (e == hipSuccess) e = DeviceBuffer::make(out_bytes, &dout);
    for (size_t k = 0; k < N && e == hipSuccess; k++) e = hipMemcpyAsync(din[k].get(), in[k].host, in[k].bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess)
    {
        launch(din, dout.as<float>());
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout.get(), out_bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(LUPIN_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return LUPIN_OK;
}

// Handles outlive their context in host code that tears down in the wrong order (garbage-collected hosts do): every entry
// point that reaches a context through a texture / scene / communicator checks this registry instead of dereferencing a
// freed pointer.  (An address reused by a later context counts as alive again; its objects are then merely foreign.)
static std::mutex g_live_mu;
static std::set<const LupinContext *> g_live_contexts;
static bool ctx_alive(const LupinContext *ctx)
{
    std::lock_guard<std::mutex> lock(g_live_mu);
    return ctx && g_live_contexts.count(ctx) != 0;
}
#define CTX_ALIVE_TRY(c) do { if (!ctx_alive(c)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "the context of this object has been destroyed"); } while (0)

bool lupin_internal_ctx_alive(const LupinContext *ctx) { return ctx_alive(ctx); }
int lupin_internal_fail(int code, const char *msg) { return fail(code, msg); }
int lupin_internal_sync_all(LupinContext *ctx) { HIP_TRY(hipSetDevice(ctx->device)); return sync_all(ctx); }
// pack / unpack launches on the primary stream, ordered after every frame enqueued so far (see k_tiles_copy for `mode`)
int lupin_internal_tiles_copy(LupinContext *ctx, const LupinTexture *tex, void *packed, uint32_t tile_size, uint32_t rank, uint32_t world,
                              uint64_t capacity_px, int mode)
{
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t tpx = tile_size * LUPIN_WORKGROUP_SIZE;
    const uint32_t ntx = (tex->width - 1) / tpx + 1, nty = (tex->height - 1) / tpx + 1;
    const uint32_t blocks = mode == 2 ? ntx * nty : lupin_owned_tile_count(ntx * nty, rank, world);
    if (int rc = join_primary(ctx)) return rc;
    // unpacked texels also refresh a valid f32 accumulator (widened: another rank's tile arrives as f16), so that
    // lupin_hip_texture_download_rgba32f and the next frame's blend see the gathered frame, not stale or zero words
    float4 *shadow = (mode != 0 && tex->accum32 && tex->accum32_valid) ? tex->accum32 : nullptr;
    if (blocks)
        hipLaunchKernelGGL(k_tiles_copy, dim3(blocks), dim3(LP_BLOCK), 0, ctx->stream, (uint2 *)tex->data, (uint2 *)packed, shadow, tex->width, tex->height,
                           tpx, rank, world, (unsigned long long)capacity_px, mode);
    HIP_TRY(hipGetLastError());
    return LUPIN_OK;
}
int lupin_internal_ctx_device(const LupinContext *ctx) { return ctx->device; }
hipStream_t lupin_internal_ctx_stream(const LupinContext *ctx) { return ctx->stream; }

// Frames in flight run on one stream each; the HIP runtime multiplexes streams onto GPU_MAX_HW_QUEUES hardware queues
// (default 4).  Ask for 8 unless the host already chose -- effective when this library loads before the process's first
// HIP call; otherwise the lanes beyond the queue count share queues (correct, less overlap).
__attribute__((constructor)) static void lupin_hw_queues_default() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }

extern "C" {

const char *lupin_hip_last_error(void) { return g_last_error.c_str(); }

int lupin_hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lupin_hip_create_context(int device_ordinal, LupinContext **out_ctx)
{
    if (!out_ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "out_ctx is null");
    int n = lupin_hip_device_count();
    if (n <= 0) return fail(LUPIN_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    if (device_ordinal < 0 || device_ordinal >= n) return fail(LUPIN_ERR_INVALID_ARGUMENT, "device ordinal out of range");
    HIP_TRY(hipSetDevice(device_ordinal));
    LupinRuntimeInfo ri;
    lupin_hip_runtime_info(&ri);
    if (ri.num_hip_runtimes_mapped > 1)
        return fail(LUPIN_ERR_HIP, std::string("two HIP runtimes are mapped into this process (") + ri.hip_runtime_paths +
                                   "): load liblupin_hip.so in a process that has not imported another copy (e.g. a PyTorch wheel's)");
    LupinContext *ctx = new LupinContext();
    { std::lock_guard<std::mutex> lock(g_live_mu); g_live_contexts.insert(ctx); }
    ctx->device = device_ordinal;
    ctx->runtime_version = ri.runtime_hip_version;
    hipError_t e = hipSuccess;
    const char *nl = getenv("LUPIN_LANES");
    if (nl) { ctx->num_lanes = std::min(LP_MAX_LANES, std::max(1, atoi(nl))); ctx->lanes_from_env = true; }
    for (int k = 0; k < ctx->num_lanes && e == hipSuccess; k++)
    {
        Lane &ln = ctx->lanes[k];
        e = hipStreamCreateWithFlags(&ln.stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ln.done, hipEventDisableTiming);
        if (e == hipSuccess) e = ln.d_fp.alloc(LP_MAX_BATCH);
        const std::pair<DeviceArray<unsigned long long> *, size_t> counters[] = {{&ln.stat_counters, 2 * LP_SHARDS}, {&ln.work_counters, LP_WORK_WORDS}, {&ln.wide_counters, LP_WIDE_WORDS}};
        for (const auto &c : counters)
        {
            if (e == hipSuccess) e = c.first->alloc(c.second);
            if (e == hipSuccess) e = hipMemsetAsync(c.first->get(), 0, c.second * sizeof(unsigned long long), ln.stream);
        }
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ctx->marker, hipEventDisableTiming);
    if (e != hipSuccess)
    {
        lupin_hip_destroy_context(ctx);   // one cleanup path: registry entry, streams, events and buffers of the lanes made so far
        return fail(LUPIN_ERR_HIP, std::string("context setup: ") + hipGetErrorString(e));
    }
    ctx->stream = ctx->lanes[0].stream;
    const char *ext = getenv("LUPIN_EXTEND");
    if (ext && strcmp(ext, "persistent") == 0) ctx->persistent_extend = 1;
    else if (ext && strcmp(ext, "simple") == 0) ctx->persistent_extend = 0;
    const char *lg = getenv("LUPIN_LDS_GEOMETRY");
    ctx->lds_geometry = !(lg && strcmp(lg, "0") == 0);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess && prop.multiProcessorCount > 0)
    {
        ctx->num_cus = (uint32_t)prop.multiProcessorCount;
    }
    const char *dbs = getenv("LUPIN_DEBUG_SYNC");
    ctx->debug_sync = dbs && strcmp(dbs, "0") != 0;
    if (const char *lsg = getenv("LUPIN_LIGHT_STAGE")) ctx->light_stage = atoi(lsg) != 0 ? 1 : 0;
    if (const char *pr = getenv("LUPIN_PATH_RECORDS")) ctx->path_records = atoi(pr) != 0 ? 1 : 0;
    const char *ssh = getenv("LUPIN_SIMPLE_SHADE");
    if (ssh && strcmp(ssh, "0") == 0) ctx->specialize_simple = false;
    const char *gr = getenv("LUPIN_GRAPH");
    if (gr) ctx->use_graph = strcmp(gr, "0") != 0;
    if (ctx->use_graph && ctx->runtime_version / 100000 != HIP_VERSION / 100000)
    {
        // Graph replay is validated on the runtime this library was built against (HIP_VERSION major.minor).  Round 1 saw a
        // memory fault on replay when a PyTorch wheel's older libamdhip64 served the process: refuse rather than risk it.
        lupin_hip_destroy_context(ctx);
        return fail(LUPIN_ERR_HIP, "LUPIN_GRAPH=1 needs the HIP runtime this library was built against (built " + std::to_string(HIP_VERSION) +
                                   ", running on " + std::to_string(ri.runtime_hip_version) + ")");
    }
    const char *shd = getenv("LUPIN_SHADOW");
    if (shd && strcmp(shd, "simple") == 0) ctx->persistent_shadow = false;
    if (const char *bf = getenv("LUPIN_BATCH")) ctx->batch_frames = (uint32_t)std::min((int)LP_MAX_BATCH, std::max(0, atoi(bf)));
    if (const char *tv = getenv("LUPIN_TRAVERSAL")) ctx->wide_traversal = strcmp(tv, "wide") == 0;
    if (const char *vw = getenv("LUPIN_VERIFY_WIDE")) ctx->verify_wide = atoi(vw) != 0;
    if (const char *ss = getenv("LUPIN_SHORT_STACK")) ctx->short_stack = (uint32_t)std::max(0, atoi(ss));
    *out_ctx = ctx;
    return LUPIN_OK;
}

void lupin_hip_destroy_context(LupinContext *ctx)
{
    if (!ctx) return;
    {
        std::lock_guard<std::mutex> lock(g_live_mu);
        if (!g_live_contexts.erase(ctx)) return;   // not ours, or destroyed already
    }
    hipSetDevice(ctx->device);
    (void)sync_all(ctx);   // nobody to tell: a batch that fails at teardown is dropped (DESIGN 5 "Teardown order"); the lanes are drained all the same
    for (int k = 0; k < LP_MAX_LANES; k++)
    {
        if (ctx->lanes[k].done) hipEventDestroy(ctx->lanes[k].done);
        if (ctx->lanes[k].graph_exec) hipGraphExecDestroy(ctx->lanes[k].graph_exec);
        if (ctx->lanes[k].graph) hipGraphDestroy(ctx->lanes[k].graph);
    }
    if (ctx->marker) hipEventDestroy(ctx->marker);
    for (auto &pr : ctx->ev_extend) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (auto &pr : ctx->ev_shade) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (auto &pr : ctx->ev_total) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    for (auto e : ctx->ev_pool) hipEventDestroy(e);
    for (int k = 0; k < LP_MAX_LANES; k++) if (ctx->lanes[k].stream) hipStreamDestroy(ctx->lanes[k].stream);
    delete ctx;   // frees every device buffer of the context and its lanes, after the streams are gone: safe only because sync_all above drained them
}

int lupin_hip_sync(LupinContext *ctx)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "ctx is null");
    HIP_TRY(hipSetDevice(ctx->device));
    return sync_all(ctx);
}

int lupin_hip_set_f16_store_rounding(LupinContext *ctx, int mode)
{
    CTX_ALIVE_TRY(ctx);
    if (int rc = flush_pending(ctx)) return rc;   // calls recorded so far ran under the old setting
    if (!ctx || (mode != 0 && mode != 1)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "mode must be 0 (toward zero) or 1 (nearest even)");
    ctx->store_rounding = mode;
    return LUPIN_OK;
}

// How many recorded calls one wavefront of `pixels`-pixel dispatches may carry.  Left to the library (batch_frames == 0): sixteen up
// to 4 M pixels -- 1080p launches are the small ones: materials1 / environments1 + 5 % / + 7 % over eight -- and eight above
// (3840 x 2160: + 0.9 % for twice the path state).  Always within the queue entries' slot bits.
static uint32_t frames_per_wavefront(const LupinContext *ctx, uint64_t pixels)
{
    uint64_t k = ctx->batch_frames ? ctx->batch_frames : (pixels <= (4ull << 20) ? 16u : 8u);
    if (pixels) k = std::min<uint64_t>(k, (uint64_t)QUEUE_SLOT_MASK / pixels);
    return (uint32_t)std::max<uint64_t>(k, 1);
}

int lupin_hip_set_batch_frames(LupinContext *ctx, uint32_t frames)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || frames > LP_MAX_BATCH) return fail(LUPIN_ERR_INVALID_ARGUMENT, "frames per wavefront must be in [1, 16] (0: chosen by dispatch size)");
    if (int rc = flush_pending(ctx)) return rc;   // calls recorded so far ran under the old setting
    ctx->batch_frames = frames;
    return LUPIN_OK;
}

int lupin_hip_set_traversal(LupinContext *ctx, int mode)
{
    CTX_ALIVE_TRY(ctx);
    if (int rc = flush_pending(ctx)) return rc;   // calls recorded so far ran under the old setting
    if (!ctx || (mode != LUPIN_TRAVERSAL_WIDE && mode != LUPIN_TRAVERSAL_BINARY)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown traversal mode");
    ctx->wide_traversal = mode == LUPIN_TRAVERSAL_WIDE;
    return LUPIN_OK;
}

int lupin_hip_set_accumulation_mode(LupinContext *ctx, int mode)
{
    CTX_ALIVE_TRY(ctx);
    if (int rc = flush_pending(ctx)) return rc;   // calls recorded so far ran under the old setting
    if (!ctx || (mode != LUPIN_ACCUM_F16_RUNNING_AVERAGE && mode != LUPIN_ACCUM_F32)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown accumulation mode");
    ctx->accum_mode = mode;
    return LUPIN_OK;
}

// Allocates, for every frame in flight, the path state of dispatches up to `pixels` pixels with the given baked parameters --
// what the first `num_lanes` pathtrace calls would otherwise do one after the other inside the caller's frame loop.
int lupin_hip_reserve_path_state(LupinContext *ctx, uint64_t pixels, uint32_t max_bounces, uint32_t samples_per_pixel)
{
    CTX_ALIVE_TRY(ctx);
    if (pixels == 0 || pixels > (uint64_t)QUEUE_SLOT_MASK || samples_per_pixel == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad path-state reservation");
    const uint32_t batch = frames_per_wavefront(ctx, pixels);
    HIP_TRY(hipSetDevice(ctx->device));
    const uint32_t iterations = samples_per_pixel * (max_bounces + 1);
    // the lanes the dispatches will rotate over (flush_pending's choice for a scene traced from global memory)
    const int lanes = ctx->lanes_from_env ? ctx->num_lanes : std::min(batch > 1 ? 1 : LP_MAX_LANES, ctx->num_lanes);
    for (int k = 0; k < lanes; k++)
    {
        int rc = ensure_path_buffers(ctx, &ctx->lanes[k], pixels * batch, iterations);
        if (rc != LUPIN_OK) return rc;
    }
    return LUPIN_OK;
}

int lupin_hip_build_pathtrace_resources(LupinContext *ctx, const LupinBakedPathtraceParams *params, LupinPathtraceResources **out_res)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !params || !out_res) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (params->samples_per_pixel == 0 || params->samples_per_pixel > 0xFFFFu) return fail(LUPIN_ERR_INVALID_ARGUMENT, "samples_per_pixel must be in [1, 65535]");
    if (params->max_bounces >= META_BOUNCE_MASK) return fail(LUPIN_ERR_INVALID_ARGUMENT, "max_bounces must be < 4095");
    LupinPathtraceResources *r = new LupinPathtraceResources();
    r->ctx = ctx;
    r->params = *params;
    *out_res = r;
    return LUPIN_OK;
}
void lupin_hip_destroy_pathtrace_resources(LupinPathtraceResources *res) { delete res; }

// ---- scene upload ----

// The TLAS as child-pair nodes behind `nblas` BLAS nodes of the one node array (global references), its root reference and
// its depth.  Returns nullptr or why the nodes are not a tree over `num_instances` instances.
static const char *tlas_child_pairs(const LupinTlasNode *nodes, uint32_t num_nodes, uint32_t num_instances, uint32_t nblas,
                                    std::vector<WideNode> &tlas, uint32_t *tlas_root, uint32_t *tlas_depth)
{
    std::vector<uint32_t> ref(num_nodes);
    uint32_t wide_count = 0;
    for (uint32_t n = 0; n < num_nodes; n++)
    {
        const LupinTlasNode &nd = nodes[n];
        if (nd.left == 0)
        {
            if (nd.instance_idx >= num_instances) return "TLAS leaf instance out of range";
            ref[n] = REF_LEAF | nd.instance_idx;
        }
        else
        {
            if (nd.left >= num_nodes || nd.right >= num_nodes) return "TLAS child out of range";
            ref[n] = nblas + wide_count++;
        }
    }
    tlas.resize(wide_count);
    for (uint32_t n = 0; n < num_nodes; n++)
    {
        const LupinTlasNode &nd = nodes[n];
        if (nd.left == 0) continue;
        const LupinTlasNode &l = nodes[nd.left];
        const LupinTlasNode &r = nodes[nd.right];
        WideNode w;
        w.a = make_float4(l.aabb_min[0], r.aabb_min[0], l.aabb_min[1], r.aabb_min[1]);
        w.b = make_float4(l.aabb_min[2], r.aabb_min[2], l.aabb_max[0], r.aabb_max[0]);
        w.c = make_float4(l.aabb_max[1], r.aabb_max[1], l.aabb_max[2], r.aabb_max[2]);
        w.d = make_uint4(ref[nd.left], ref[nd.right], 0u, 0u);
        tlas[ref[n] - nblas] = w;
    }
    *tlas_root = ref[0];
    // depth from the root (bounded walk: a malformed cyclic TLAS is rejected)
    *tlas_depth = 0;
    std::vector<std::pair<uint32_t, uint32_t>> st;
    st.push_back({0u, 0u});
    uint64_t visited = 0;
    while (!st.empty())
    {
        auto [n, d] = st.back();
        st.pop_back();
        if (++visited > (uint64_t)num_nodes * 2 + 2) return "TLAS is not a tree";
        if (nodes[n].left != 0)
        {
            *tlas_depth = std::max(*tlas_depth, d + 1);
            st.push_back({nodes[n].left, d + 1});
            st.push_back({nodes[n].right, d + 1});
        }
    }
    return nullptr;
}

// Conservative world-space bounding sphere of a light instance: `npts` local-space points (`stride` floats apart) that
// enclose the mesh -- all its vertices at creation, the corners of its model box in an update -- through the inverse of
// the stored world->local rows, in double, radius padded.  lights_pdf skips lights whose sphere the ray cannot reach; a
// skipped light contributes exactly +0.0f in the reference's sum, so results do not change.  .w = padded radius squared.
static float4 light_bound(const LupinMat4x3 &rows, const float *pts, size_t npts, size_t stride)
{
    const float (*r)[4] = rows.m;   // 3 rows x 4: world -> local
    const double a = r[0][0], b = r[0][1], c = r[0][2], d = r[1][0], e = r[1][1], f = r[1][2], g = r[2][0], h = r[2][1], k = r[2][2];
    const double det = a * (e * k - f * h) - b * (d * k - f * g) + c * (d * h - e * g);
    float4 bound = make_float4(0.0f, 0.0f, 0.0f, INFINITY);   // singular / non-finite transform: never culled
    if (std::isfinite(det) && det != 0.0 && npts > 0)
    {
        const double inv[3][3] = {{(e * k - f * h) / det, (c * h - b * k) / det, (b * f - c * e) / det},
                                  {(f * g - d * k) / det, (a * k - c * g) / det, (c * d - a * f) / det},
                                  {(d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det}};
        double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
        bool finite = true;
        for (size_t v = 0; v < npts; v++)
        {
            const double q[3] = {pts[stride * v + 0] - (double)r[0][3], pts[stride * v + 1] - (double)r[1][3], pts[stride * v + 2] - (double)r[2][3]};
            for (int ax = 0; ax < 3; ax++)
            {
                const double w = inv[ax][0] * q[0] + inv[ax][1] * q[1] + inv[ax][2] * q[2];
                finite = finite && std::isfinite(w);
                lo[ax] = std::min(lo[ax], w); hi[ax] = std::max(hi[ax], w);
            }
        }
        if (finite)
        {
            const double cx = 0.5 * (lo[0] + hi[0]), cy = 0.5 * (lo[1] + hi[1]), cz = 0.5 * (lo[2] + hi[2]);
            const double rad = 0.5 * std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2]));
            const double cmag = std::fabs(cx) + std::fabs(cy) + std::fabs(cz);
            const double padded = rad * 1.02 + 1e-4 * (cmag + rad) + 1e-6;
            bound = make_float4((float)cx, (float)cy, (float)cz, (float)(padded * padded * (1.0 + 1e-6)));
        }
    }
    return bound;
}

int lupin_hip_scene_create(LupinContext *ctx, const LupinSceneDesc *desc, LupinScene **out_scene)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !desc || !out_scene) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    const LupinSceneDesc &s = *desc;

    // ---- validation (validate_scene, data_structures.rs:876-928, plus what the kernels index) ----
    if (s.num_instances > (1u << 26)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "more than 2^26 instances (the tracer keeps an instance's flags above its 26-bit index)");
    for (uint32_t i = 0; i < s.num_instances; i++)
    {
        if (s.instances[i].mesh_idx >= s.num_meshes) return fail(LUPIN_ERR_INVALID_ARGUMENT, "instance mesh_idx out of range");
        if (s.instances[i].mat_idx >= s.num_materials) return fail(LUPIN_ERR_INVALID_ARGUMENT, "instance mat_idx out of range");
    }
    auto tex_ok = [&](uint32_t t) { return t == LUPIN_SENTINEL_IDX || t < s.num_textures; };
    for (uint32_t i = 0; i < s.num_materials; i++)
    {
        const LupinMaterial &m = s.materials[i];
        if (!tex_ok(m.color_tex_idx) || !tex_ok(m.emission_tex_idx) || !tex_ok(m.roughness_tex_idx) || !tex_ok(m.scattering_tex_idx) || !tex_ok(m.normal_tex_idx))
            return fail(LUPIN_ERR_INVALID_ARGUMENT, "material texture index out of range");
    }
    if (s.num_environments > LUPIN_MAX_ENVS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "too many environments");
    for (uint32_t i = 0; i < s.num_environments; i++)
    {
        const LupinEnvironment &e = s.environments[i];
        if (!tex_ok(e.emission_tex_idx)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "environment texture index out of range");
        if (e.emission_tex_idx != LUPIN_SENTINEL_IDX)
        {
            const LupinTextureDesc &t = s.textures[e.emission_tex_idx];
            if (!s.env_alias_tables || s.env_alias_tables[i].num_bins != t.width * t.height)
                return fail(LUPIN_ERR_INVALID_ARGUMENT, "environment alias table must have one bin per texel");
        }
    }
    for (uint32_t i = 0; i < s.num_lights; i++)
    {
        if (s.lights[i].instance_idx >= s.num_instances) return fail(LUPIN_ERR_INVALID_ARGUMENT, "light instance_idx out of range");
        if (!s.alias_tables || s.alias_tables[i].num_bins == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "light without alias table");
        uint32_t mesh = s.instances[s.lights[i].instance_idx].mesh_idx;
        if (s.alias_tables[i].num_bins != s.meshes[mesh].num_indices / 3) return fail(LUPIN_ERR_INVALID_ARGUMENT, "light alias table size != triangle count");
    }
    for (uint32_t i = 0; i < s.num_textures; i++)
        if (s.textures[i].width == 0 || s.textures[i].height == 0 || !s.textures[i].pixels || s.textures[i].format > LUPIN_TEX_RGBA16_FLOAT)
            return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad texture descriptor");

    LupinScene *sc = new LupinScene();
    sc->ctx = ctx;
    sc->device = ctx->device;
    sc->instances_empty = s.num_instances == 0;
    sc->lights_empty = s.num_lights == 0;
    sc->envs_empty = s.num_environments == 0;
    sc->has_sw_bvh = s.num_tlas_nodes > 0 || s.num_instances == 0;
    if (s.num_instances > 0 && s.num_tlas_nodes == 0) { delete sc; return fail(LUPIN_ERR_NO_SW_BVH, "scene has instances but no TLAS (software BVH required)"); }

    // ---- vertex attribute pools ----
    std::vector<uint32_t> normal_base(s.num_normal_buffers), uv_base(s.num_texcoord_buffers), color_base(s.num_color_buffers);
    std::vector<float4> normals;
    std::vector<float2> texcoords;
    std::vector<float4> colors;
    for (uint32_t b = 0; b < s.num_normal_buffers; b++)
    {
        normal_base[b] = (uint32_t)normals.size();
        for (uint32_t v = 0; v < s.verts_normal_array[b].num_verts; v++) { const float *p = s.verts_normal_array[b].data + (size_t)v * 4; normals.push_back(make_float4(p[0], p[1], p[2], 0.0f)); }
    }
    for (uint32_t b = 0; b < s.num_texcoord_buffers; b++)
    {
        uv_base[b] = (uint32_t)texcoords.size();
        for (uint32_t v = 0; v < s.verts_texcoord_array[b].num_verts; v++) { const float *p = s.verts_texcoord_array[b].data + (size_t)v * 2; texcoords.push_back(make_float2(p[0], p[1])); }
    }
    for (uint32_t b = 0; b < s.num_color_buffers; b++)
    {
        color_base[b] = (uint32_t)colors.size();
        for (uint32_t v = 0; v < s.verts_color_array[b].num_verts; v++) { const float *p = s.verts_color_array[b].data + (size_t)v * 4; colors.push_back(make_float4(p[0], p[1], p[2], p[3])); }
    }

    // ---- meshes: triangles in leaf order, BLAS as 64-byte child-pair nodes ----
    std::vector<TriVerts> tris;
    std::vector<uint32_t> tri_indices;
    std::vector<WideNode> blas;
    std::vector<MeshDev> meshes(s.num_meshes);
    std::vector<uint32_t> mesh_root(s.num_meshes);
    uint32_t max_blas_depth = 0;
    for (uint32_t mi = 0; mi < s.num_meshes; mi++)
    {
        const LupinMeshDesc &m = s.meshes[mi];
        const LupinMeshInfo &info = s.mesh_infos[mi];
        MeshDev md;
        md.tri_offset = (uint32_t)tris.size();
        auto attr_base = [&](uint32_t idx, const std::vector<uint32_t> &bases, uint32_t nbuf, const LupinVertexBufferDesc *bufs, bool &ok) -> uint32_t {
            if (idx == LUPIN_SENTINEL_IDX) return LUPIN_SENTINEL_IDX;
            if (idx >= nbuf || bufs[idx].num_verts != m.num_verts) { ok = false; return LUPIN_SENTINEL_IDX; }
            return bases[idx];
        };
        bool ok = true;
        md.normals_base = attr_base(info.normals_buf_idx, normal_base, s.num_normal_buffers, s.verts_normal_array, ok);
        md.texcoords_base = attr_base(info.texcoords_buf_idx, uv_base, s.num_texcoord_buffers, s.verts_texcoord_array, ok);
        md.colors_base = attr_base(info.colors_buf_idx, color_base, s.num_color_buffers, s.verts_color_array, ok);
        if (!ok) { lupin_hip_scene_destroy(sc); return fail(LUPIN_ERR_INVALID_ARGUMENT, "mesh attribute buffer index / size mismatch"); }
        meshes[mi] = md;

        {
            float box[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};   // Aabb::neutral()
            for (uint32_t v = 0; v < m.num_verts; v++)
                for (int ax = 0; ax < 3; ax++)
                {
                    const float x = m.verts_pos[(size_t)v * 4 + ax];
                    box[ax] = x < box[ax] ? x : box[ax];
                    box[3 + ax] = x > box[3 + ax] ? x : box[3 + ax];
                }
            sc->model_aabbs.insert(sc->model_aabbs.end(), box, box + 6);
        }

        uint32_t ntris = m.num_indices / 3;
        sc->mesh_tri_count.push_back(ntris);
        sc->mesh_has_texcoords.push_back(md.texcoords_base != LUPIN_SENTINEL_IDX);
        sc->mesh_vert_count.push_back(m.num_verts);
        sc->mesh_tri_offset.push_back(md.tri_offset);
        sc->lightmap_uvs.emplace_back();
        for (uint32_t i = 0; i < ntris * 3; i++)
            if (m.indices[i] >= m.num_verts) { lupin_hip_scene_destroy(sc); return fail(LUPIN_ERR_INVALID_ARGUMENT, "vertex index out of range"); }
        for (uint32_t t = 0; t < ntris; t++)
        {
            TriVerts tv;
            const float *p0 = m.verts_pos + (size_t)m.indices[t * 3 + 0] * 4;
            const float *p1 = m.verts_pos + (size_t)m.indices[t * 3 + 1] * 4;
            const float *p2 = m.verts_pos + (size_t)m.indices[t * 3 + 2] * 4;
            tv.v0 = make_float4(p0[0], p0[1], p0[2], 0.0f);
            tv.v1 = make_float4(p1[0], p1[1], p1[2], 0.0f);
            tv.v2 = make_float4(p2[0], p2[1], p2[2], 0.0f);
            tris.push_back(tv);
            tri_indices.push_back(m.indices[t * 3 + 0]);
            tri_indices.push_back(m.indices[t * 3 + 1]);
            tri_indices.push_back(m.indices[t * 3 + 2]);
        }
        if (ntris == 0 || m.num_bvh_nodes == 0)
        {
            // degenerate mesh: one never-hit triangle so that traversal has a well-formed leaf
            TriVerts tv;
            tv.v0 = make_float4(0, 0, 0, host_u2f(LEAF_END_BITS));
            tv.v1 = tv.v2 = make_float4(0, 0, 0, 0);
            mesh_root[mi] = REF_LEAF | (uint32_t)tris.size();
            tris.push_back(tv);
            tri_indices.push_back(0); tri_indices.push_back(0); tri_indices.push_back(0);
            continue;
        }
        for (uint32_t n = 0; n < m.num_bvh_nodes; n++)
            if (m.bvh_nodes[n].tri_count == 0 && (uint64_t)m.bvh_nodes[n].tri_begin_or_first_child + 1 >= m.num_bvh_nodes)
            { lupin_hip_scene_destroy(sc); return fail(LUPIN_ERR_INVALID_ARGUMENT, "BLAS child index out of bounds"); }
        const uint32_t bd = blas_depth(m.bvh_nodes, m.num_bvh_nodes);
        if (bd == 0xFFFFFFFFu) { lupin_hip_scene_destroy(sc); return fail(LUPIN_ERR_INVALID_ARGUMENT, "BLAS is not a tree"); }
        max_blas_depth = std::max(max_blas_depth, bd);
        std::vector<uint32_t> leaf_ends, leaky_tris;
        const char *why = nullptr;
        const uint32_t root_ref = blas_child_pairs(m.bvh_nodes, m.num_bvh_nodes, ntris, md.tri_offset, blas, leaf_ends, &why, m.verts_pos, m.indices, &leaky_tris);
        if (why) { lupin_hip_scene_destroy(sc); return fail(LUPIN_ERR_INVALID_ARGUMENT, why); }
        // v0.w of a triangle: bit 0 = last of its leaf, bit 1 = not inside every box above it (the wide tracer re-traces hits on it)
        for (uint32_t t : leaky_tris) tris[t].v0.w = host_u2f(TRI_LEAKY_BITS);
        for (uint32_t last : leaf_ends) tris[last].v0.w = host_u2f(__builtin_bit_cast(uint32_t, tris[last].v0.w) | LEAF_END_BITS);
        sc->leaky_triangles += leaky_tris.size();
        mesh_root[mi] = root_ref;
    }

    // ---- TLAS ----
    std::vector<WideNode> tlas;
    uint32_t tlas_root = REF_LEAF;
    uint32_t tlas_depth = 0;
    if (s.num_tlas_nodes > 0)
    {
        // TLAS nodes go behind the BLAS nodes in ONE array (no per-lane base select in the traversal step): global references
        const char *why = tlas_child_pairs(s.tlas_nodes, s.num_tlas_nodes, s.num_instances, (uint32_t)blas.size(), tlas, &tlas_root, &tlas_depth);
        if (why) { lupin_hip_scene_destroy(sc); return fail(LUPIN_ERR_INVALID_ARGUMENT, why); }
    }
    sc->nblas = (uint32_t)blas.size();
    sc->ntlas = (uint32_t)tlas.size();
    sc->max_blas_depth = max_blas_depth;
    sc->tlas_nodes.assign(s.tlas_nodes, s.tlas_nodes + s.num_tlas_nodes);
    sc->stack_entries = tlas_depth + max_blas_depth + 1;
    blas.insert(blas.end(), tlas.begin(), tlas.end());   // the one node array: [BLAS | TLAS]

    // ---- the same hierarchies four-wide (wide tracer; scenes small enough for LDS staging are traced by k_extend) ----
    std::vector<Wide4> wide4;   // TLAS nodes first, then every mesh's BLAS nodes: one array, global indices
    std::vector<uint32_t> mesh_root4(s.num_meshes, REF_LEAF);
    uint32_t tlas4_root = tlas_root;
    const size_t lds_bytes_if_staged = blas.size() * 80 + tris.size() * 48 + (size_t)s.num_instances * 80;
    const bool build_wide = s.num_instances > 0 && !(lds_bytes_if_staged <= LP_GEO_LDS_LIMIT && ctx->lds_geometry);
    if (build_wide)
    {
        tlas4_root = collapse_to_wide4(blas, tlas_root, wide4);
        for (uint32_t mi = 0; mi < s.num_meshes; mi++) mesh_root4[mi] = collapse_to_wide4(blas, mesh_root[mi], wide4);
        if (wide4.size() >= (size_t)REF_INDEX_MASK || tris.size() >= (size_t)REF_INDEX_MASK) { lupin_hip_scene_destroy(sc); return fail(LUPIN_ERR_INVALID_ARGUMENT, "scene too large for 30-bit references"); }
        sc->has_wide = true;
    }

    // ---- instances ----
    std::vector<InstanceDev> instances(s.num_instances);
    uint32_t mat_types_seen = 0;
    bool any_alpha = false;
    for (uint32_t i = 0; i < s.num_instances; i++)
    {
        const LupinInstance &in = s.instances[i];
        const float (*m)[4] = in.transpose_inverse_transform.m;
        InstanceDev d;
        d.r0 = make_float4(m[0][0], m[0][1], m[0][2], m[0][3]);
        d.r1 = make_float4(m[1][0], m[1][1], m[1][2], m[1][3]);
        d.r2 = make_float4(m[2][0], m[2][1], m[2][2], m[2][3]);
        d.blas_root = mesh_root[in.mesh_idx];
        d.mat_idx = in.mat_idx;
        d.mesh_idx = in.mesh_idx;
        const LupinMaterial &mat = s.materials[in.mat_idx];
        bool maybe_alpha = !(mat.color[3] == 1.0f) ||
                           (mat.color_tex_idx != LUPIN_SENTINEL_IDX && meshes[in.mesh_idx].texcoords_base != LUPIN_SENTINEL_IDX) ||
                           meshes[in.mesh_idx].colors_base != LUPIN_SENTINEL_IDX;
        any_alpha = any_alpha || maybe_alpha;
        // bits 8..11: material type, bit 12: the material's own roughness is zero (a hint: smooth reflective / refractive /
        // transparent surfaces take the delta branch unless a roughness texture says otherwise) = k_sort_queue's key
        const bool smooth = mat.roughness == 0.0f && (mat.mat_type == LUPIN_MAT_REFLECTIVE || mat.mat_type == LUPIN_MAT_REFRACTIVE || mat.mat_type == LUPIN_MAT_TRANSPARENT);
        d.flags = (maybe_alpha ? 1u : 0u) | ((mat.mat_type & 0xFu) << 8) | (smooth ? 1u << 12 : 0u);
        mat_types_seen |= 1u << (mat.mat_type & 0xFu);
        instances[i] = d;
    }

    // per-instance copies of the mesh record and the material (shading fetches them beside the instance record)
    std::vector<MeshDev> inst_meshes(s.num_instances);
    std::vector<LupinMaterial> inst_materials(s.num_instances);
    for (uint32_t i = 0; i < s.num_instances; i++)
    {
        inst_meshes[i] = meshes[s.instances[i].mesh_idx];
        inst_materials[i] = s.materials[s.instances[i].mat_idx];
    }
    std::vector<uint32_t> inst_root4(s.num_instances);
    for (uint32_t i = 0; i < s.num_instances; i++) inst_root4[i] = mesh_root4[s.instances[i].mesh_idx];

    // ---- textures ----
    std::vector<TextureDev> textures(s.num_textures);
    std::vector<uint8_t> texels;
    sc->num_textures = s.num_textures;
    for (uint32_t i = 0; i < s.num_textures; i++)
    {
        const LupinTextureDesc &t = s.textures[i];
        size_t bpp = (t.format == LUPIN_TEX_RGBA8_UNORM) ? 4 : 8;
        size_t bytes = (size_t)t.width * t.height * bpp;
        size_t off = (texels.size() + 15) & ~(size_t)15;
        texels.resize(off + bytes);
        memcpy(texels.data() + off, t.pixels, bytes);
        textures[i].offset = off;
        textures[i].width = t.width;
        textures[i].height = t.height;
        textures[i].format = t.format;
        textures[i].pad = 0;
    }

    // ---- lights ----
    std::vector<AliasRange> alias_ranges(s.num_lights), env_alias_ranges(s.num_environments);
    std::vector<LupinAliasBin> alias_bins;
    for (uint32_t i = 0; i < s.num_lights; i++)
    {
        alias_ranges[i] = {(uint32_t)alias_bins.size(), s.alias_tables[i].num_bins};
        alias_bins.insert(alias_bins.end(), s.alias_tables[i].bins, s.alias_tables[i].bins + s.alias_tables[i].num_bins);
    }
    for (uint32_t i = 0; i < s.num_environments; i++)
    {
        uint32_t nb = s.env_alias_tables ? s.env_alias_tables[i].num_bins : 0;
        env_alias_ranges[i] = {(uint32_t)alias_bins.size(), nb};
        if (nb) alias_bins.insert(alias_bins.end(), s.env_alias_tables[i].bins, s.env_alias_tables[i].bins + nb);
    }

    // light_bound() of every light instance over all its mesh's vertices
    // (padded to whole groups of four: lights_pdf fetches the bounds four at a time, 64 aligned bytes per scalar load)
    std::vector<float4> light_bounds(((size_t)s.num_lights + 3) / 4 * 4, make_float4(0.0f, 0.0f, 0.0f, -1.0f));
    for (uint32_t i = 0; i < s.num_lights; i++)
    {
        const LupinInstance &in = s.instances[s.lights[i].instance_idx];
        const LupinMeshDesc &m = s.meshes[in.mesh_idx];
        light_bounds[i] = light_bound(in.transpose_inverse_transform, m.verts_pos, m.num_verts, 4);
        sc->light_instance.push_back(s.lights[i].instance_idx);
    }

    // small scenes: one blob [tlas | blas | tris | instances] in 16-byte words for LDS staging.  Nodes and instances are
    // laid out at a stride of FIVE words (80 bytes) instead of four: a wave's lanes read records at divergent indices with
    // ds_read_b128, and at a 64-byte stride records i and i + 4 start in the same LDS bank (round 1's PMC: 62 M
    // SQ_LDS_BANK_CONFLICT cycles against 184 M SQ_ACTIVE_INST_LDS on the Cornell box); at 80 bytes only i and i + 16
    // collide.  Triangles keep 48 bytes (3 words: i and i + 16 collide as well).
    std::vector<float4> geo_blob;
    uint32_t off_blas = 0, off_tris = 0, off_inst = 0;
    {
        const size_t bytes = blas.size() * 80 + tris.size() * 48 + instances.size() * 80;
        if (bytes > 0 && bytes <= LP_GEO_LDS_LIMIT)
        {
            auto append = [&](const void *p, size_t count, size_t words) {   // records of `words` 16-byte words, padded to LP_GEO_LDS_STRIDE
                const float4 *f = reinterpret_cast<const float4 *>(p);
                for (size_t r = 0; r < count; r++)
                {
                    geo_blob.insert(geo_blob.end(), f + r * words, f + (r + 1) * words);
                    if (words == 4) geo_blob.push_back(make_float4(0.0f, 0.0f, 0.0f, 0.0f));
                }
            };
            append(blas.data(), blas.size(), 4);   // [BLAS | TLAS] nodes, indexed by the global references
            off_blas = 0;
            off_tris = (uint32_t)geo_blob.size();
            append(tris.data(), tris.size(), 3);
            off_inst = (uint32_t)geo_blob.size();
            append(instances.data(), instances.size(), 4);
        }
    }

    SceneDev &dv = sc->dev;
    int rc = LUPIN_OK;
    std::vector<LupinMaterial> materials(s.materials, s.materials + s.num_materials);
    std::vector<LupinEnvironment> envs(s.environments, s.environments + s.num_environments);
    std::vector<LupinLight> lights(s.lights, s.lights + s.num_lights);
    if ((rc = upload(sc, blas, &dv.blas)) || (rc = upload(sc, tris, &dv.tris)) ||
        (rc = upload(sc, tri_indices, &dv.tri_indices)) || (rc = upload(sc, instances, &dv.instances)) ||
        (rc = upload(sc, meshes, &dv.meshes)) || (rc = upload(sc, materials, &dv.materials)) ||
        (rc = upload(sc, inst_meshes, &dv.inst_meshes)) || (rc = upload(sc, inst_materials, &dv.inst_materials)) ||
        (rc = upload(sc, normals, &dv.normals)) || (rc = upload(sc, texcoords, &dv.texcoords)) || (rc = upload(sc, colors, &dv.colors)) ||
        (rc = upload(sc, textures, &dv.textures)) || (rc = upload(sc, texels, &dv.texels)) ||
        (rc = upload(sc, envs, &dv.environments)) || (rc = upload(sc, lights, &dv.lights)) ||
        (rc = upload(sc, alias_ranges, &dv.alias_ranges)) || (rc = upload(sc, env_alias_ranges, &dv.env_alias_ranges)) ||
        (rc = upload(sc, alias_bins, &dv.alias_bins)) || (rc = upload(sc, geo_blob, &dv.geo_blob)) ||
        (rc = upload(sc, light_bounds, &dv.light_bounds)) ||
        (rc = upload(sc, wide4, &dv.wide4)) || (rc = upload(sc, inst_root4, &dv.inst_root4)))
    {
        lupin_hip_scene_destroy(sc);
        return rc;
    }
    sc->host_instances = instances;
    dv.tlas = dv.blas;
    dv.tlas_root = tlas_root;
    dv.tlas4_root = tlas4_root;
    dv.num_lights = s.num_lights;
    dv.num_envs = s.num_environments;
    dv.num_instances = s.num_instances;
    {
        // simple_matte: every instance's material is matte with no texture reference, no mesh carries vertex colours, and
        // there is no environment -- then material type, texture use and environment terms are constants of the scene
        bool simple = s.num_instances > 0 && s.num_environments == 0 && s.num_color_buffers == 0;
        for (uint32_t i = 0; i < s.num_instances && simple; i++)
        {
            const LupinMaterial &mat = s.materials[s.instances[i].mat_idx];
            simple = mat.mat_type == LUPIN_MAT_MATTE && mat.color_tex_idx == LUPIN_SENTINEL_IDX && mat.emission_tex_idx == LUPIN_SENTINEL_IDX &&
                     mat.roughness_tex_idx == LUPIN_SENTINEL_IDX && mat.scattering_tex_idx == LUPIN_SENTINEL_IDX && mat.normal_tex_idx == LUPIN_SENTINEL_IDX;
        }
        sc->simple_matte = simple;
        sc->all_opaque = !any_alpha;
    }
    dv.sort_shade = __builtin_popcount(mat_types_seen) >= 4;   // pays off from about four BSDF families (measured: 3 lose 10 %, 8 win 17 % of k_shade)
    { const char *ss = getenv("LUPIN_SORT_SHADE"); if (ss) dv.sort_shade = strcmp(ss, "0") != 0; }
    dv.geo_blob_words = (uint32_t)geo_blob.size();
    dv.geo_off_blas = off_blas; dv.geo_off_tris = off_tris; dv.geo_off_inst = off_inst;
    static std::atomic<uint64_t> next_scene_id{1};   // contexts may live on different host threads
    sc->id = next_scene_id.fetch_add(1);
    hipError_t e = hipStreamSynchronize(ctx->stream);   // host vectors go out of scope
    if (e != hipSuccess) { lupin_hip_scene_destroy(sc); return fail(LUPIN_ERR_HIP, hipGetErrorString(e)); }
    *out_scene = sc;
    return LUPIN_OK;
}

void lupin_hip_scene_destroy(LupinScene *scene)
{
    if (!scene) return;
    hipSetDevice(scene->device);
    if (ctx_alive(scene->ctx)) (void)sync_all(scene->ctx);   // a destroyed context has drained its streams already; a batch that fails here is dropped
    delete scene;   // frees its allocations: after the synchronisation above
}

// Moves the instances in place.  Everything is validated and built in host staging first; device memory is
// written only once the new tree exists and every lane that may read the scene has drained, so an error leaves the scene
// rendering exactly as before.
int lupin_hip_scene_update_instances(LupinScene *scene, const LupinMat4x3 *transpose_inverse_transforms, uint32_t num_instances, int tlas_builder)
{
    if (!scene || !transpose_inverse_transforms) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    LupinContext *ctx = scene->ctx;
    CTX_ALIVE_TRY(ctx);
    if (tlas_builder != 0 && tlas_builder != 1) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown tlas_builder (0 = CPU, 1 = device)");
    if (!scene->has_sw_bvh) return fail(LUPIN_ERR_NO_SW_BVH, "no software BVH was built for this scene");
    const uint32_t n = scene->dev.num_instances;
    if (num_instances != n) return fail(LUPIN_ERR_INVALID_ARGUMENT, "update_instances: the instance count cannot change (" + std::to_string(num_instances) + " transforms for " + std::to_string(n) + " instances)");
    if (n == 0) return LUPIN_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = flush_pending(ctx)) return rc;   // calls recorded so far render the old transforms

    // ---- staging: instance records, TLAS, child pairs, light bounds ----
    std::vector<LupinInstance> inst(n);
    std::vector<InstanceDev> instances = scene->host_instances;
    for (uint32_t i = 0; i < n; i++)
    {
        memset(&inst[i], 0, sizeof(LupinInstance));
        inst[i].transpose_inverse_transform = transpose_inverse_transforms[i];
        inst[i].mesh_idx = instances[i].mesh_idx;
        inst[i].mat_idx = instances[i].mat_idx;
        const float (*m)[4] = transpose_inverse_transforms[i].m;
        instances[i].r0 = make_float4(m[0][0], m[0][1], m[0][2], m[0][3]);
        instances[i].r1 = make_float4(m[1][0], m[1][1], m[1][2], m[1][3]);
        instances[i].r2 = make_float4(m[2][0], m[2][1], m[2][2], m[2][3]);
    }
    const uint32_t num_meshes = (uint32_t)(scene->model_aabbs.size() / 6);
    std::vector<LupinTlasNode> nodes((size_t)n * 2);
    if (tlas_builder == 0)
    {
        // the device builder rejects non-finite world boxes itself; the CPU builder would cluster them
        if (lupin_internal_tlas_leaves(inst.data(), n, scene->model_aabbs.data(), num_meshes, nodes.data()) != LUPIN_OK)
            return fail(LUPIN_ERR_INVALID_ARGUMENT, "instance mesh_idx out of range");
        if (!lupin_internal_tlas_leaves_finite(inst.data(), nodes.data(), n))
            return fail(LUPIN_ERR_INVALID_ARGUMENT, "instance with a non-finite transform or world-space box (NaN / infinite / singular transform)");
    }
    const int64_t built = tlas_builder == 0 ? lupin_build_tlas(inst.data(), n, scene->model_aabbs.data(), num_meshes, nodes.data())
                                            : lupin_hip_build_tlas_device(ctx, inst.data(), n, scene->model_aabbs.data(), num_meshes, nodes.data());
    if (built < 0) return tlas_builder == 0 ? fail((int)built, "lupin_build_tlas failed") : (int)built;   // the device builder left its message
    if (built != (int64_t)n * 2) return fail(LUPIN_ERR_INVALID_ARGUMENT, "TLAS builder returned an unexpected node count");
    std::vector<WideNode> tlas;
    uint32_t tlas_root = REF_LEAF, tlas_depth = 0;
    if (const char *why = tlas_child_pairs(nodes.data(), (uint32_t)built, n, scene->nblas, tlas, &tlas_root, &tlas_depth)) return fail(LUPIN_ERR_INVALID_ARGUMENT, why);
    // a binary tree over n leaves has n - 1 inner nodes: the TLAS segment of the node array keeps its size
    if (tlas.size() != scene->ntlas) return fail(LUPIN_ERR_INVALID_ARGUMENT, "rebuilt TLAS does not fit the scene's TLAS segment");
    const uint32_t stack_entries = tlas_depth + scene->max_blas_depth + 1;
    SceneDev &dv = scene->dev;
    {
        // the limit every render applies (pathtrace_impl / flush_pending), here before anything is written
        TraversalLds t;
        if (int rc = traversal_lds(ctx, scene, stack_entries, true, &t)) return rc;
    }
    const size_t nlights = scene->light_instance.size();
    std::vector<float4> light_bounds((nlights + 3) / 4 * 4, make_float4(0.0f, 0.0f, 0.0f, -1.0f));
    for (size_t i = 0; i < nlights; i++)
    {
        // the eight corners of the mesh's model box instead of all its vertices: a sphere that contains them contains the mesh
        const uint32_t ii = scene->light_instance[i];
        const float *ab = scene->model_aabbs.data() + (size_t)instances[ii].mesh_idx * 6;
        float corners[8][3];
        for (int k = 0; k < 8; k++) { corners[k][0] = (k & 4) ? ab[3] : ab[0]; corners[k][1] = (k & 2) ? ab[4] : ab[1]; corners[k][2] = (k & 1) ? ab[5] : ab[2]; }
        const bool empty_mesh = ab[0] > ab[3];   // Aabb::neutral(): creation never culls such a light either
        light_bounds[i] = light_bound(inst[ii].transpose_inverse_transform, &corners[0][0], empty_mesh ? 0 : 8, 3);
    }
    // the LDS-staged copy of small scenes: records of LP_GEO_LDS_STRIDE words, nodes by global index, then instances
    std::vector<float4> blob_tlas, blob_inst;
    if (dv.geo_blob_words)
    {
        auto append = [](std::vector<float4> &dst, const void *p, size_t count) {
            const float4 *f = reinterpret_cast<const float4 *>(p);
            for (size_t r = 0; r < count; r++)
            {
                dst.insert(dst.end(), f + r * 4, f + (r + 1) * 4);
                dst.push_back(make_float4(0.0f, 0.0f, 0.0f, 0.0f));
            }
        };
        append(blob_tlas, tlas.data(), tlas.size());
        append(blob_inst, instances.data(), instances.size());
        const size_t tlas_word = (size_t)dv.geo_off_blas + (size_t)scene->nblas * LP_GEO_LDS_STRIDE;
        if (tlas_word + blob_tlas.size() > dv.geo_off_tris || (size_t)dv.geo_off_inst + blob_inst.size() > dv.geo_blob_words)
            return fail(LUPIN_ERR_INVALID_ARGUMENT, "staged geometry layout mismatch");
    }

    // ---- every lane that may still read the scene drains, then the writes ----
    for (int k = 0; k < LP_MAX_LANES; k++)
        if (ctx->lanes[k].stream) HIP_TRY(hipStreamSynchronize(ctx->lanes[k].stream));
    hipStream_t st = ctx->stream;
    HIP_TRY(hipMemcpyAsync(const_cast<InstanceDev *>(dv.instances), instances.data(), instances.size() * sizeof(InstanceDev), hipMemcpyHostToDevice, st));
    if (!tlas.empty()) HIP_TRY(hipMemcpyAsync(const_cast<WideNode *>(dv.blas) + scene->nblas, tlas.data(), tlas.size() * sizeof(WideNode), hipMemcpyHostToDevice, st));
    if (nlights) HIP_TRY(hipMemcpyAsync(const_cast<float4 *>(dv.light_bounds), light_bounds.data(), light_bounds.size() * sizeof(float4), hipMemcpyHostToDevice, st));
    if (dv.geo_blob_words)
    {
        float4 *blob = const_cast<float4 *>(dv.geo_blob);
        if (!blob_tlas.empty()) HIP_TRY(hipMemcpyAsync(blob + dv.geo_off_blas + (size_t)scene->nblas * LP_GEO_LDS_STRIDE, blob_tlas.data(), blob_tlas.size() * sizeof(float4), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(blob + dv.geo_off_inst, blob_inst.data(), blob_inst.size() * sizeof(float4), hipMemcpyHostToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));   // the staging vectors go out of scope; later calls on any lane see the new scene
    dv.tlas_root = tlas_root;
    scene->stack_entries = stack_entries;
    scene->host_instances.swap(instances);
    scene->tlas_nodes.swap(nodes);
    // launch shapes cached per scene depend on the stack size; a captured wavefront holds the old root
    memset(scene->persistent_blocks, 0, sizeof(scene->persistent_blocks));
    memset(scene->wide_blocks, 0, sizeof(scene->wide_blocks));
    memset(scene->short_blocks, 0, sizeof(scene->short_blocks));
    static std::atomic<uint64_t> next_update_id{1ull << 40};   // disjoint from the ids scene_create hands out
    scene->id = next_update_id.fetch_add(1);
    // The four-wide TLAS has no fixed size and is not re-collapsed: refuse the wide tracer for this scene from now on.
    if (scene->has_wide) { scene->has_wide = false; scene->wide_stale = true; }
    return LUPIN_OK;
}

int64_t lupin_hip_scene_get_tlas(const LupinScene *scene, LupinTlasNode *out_nodes, uint64_t capacity)
{
    if (!scene) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    const uint64_t count = scene->tlas_nodes.size();
    if (!out_nodes) return (int64_t)count;
    if (capacity < count) return fail(LUPIN_ERR_INVALID_ARGUMENT, "node buffer too small");
    if (count) memcpy(out_nodes, scene->tlas_nodes.data(), count * sizeof(LupinTlasNode));
    return (int64_t)count;
}

// ---- textures / double buffering ----

// The texture has its f32 shadow: made and cleared on `st` by the first call that needs it, kept afterwards.
static int ensure_accum32(LupinTexture *tex, hipStream_t st)
{
    if (tex->accum32) return LUPIN_OK;
    HIP_TRY(device_view(&tex->accum32_mem, (size_t)tex->width * tex->height, &tex->accum32));
    HIP_TRY(hipMemsetAsync(tex->accum32, 0, (size_t)tex->width * tex->height * sizeof(float4), st));
    return LUPIN_OK;
}

int lupin_hip_texture_create(LupinContext *ctx, uint32_t width, uint32_t height, LupinTexture **out_tex)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !out_tex || width == 0 || height == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad texture size");
    HIP_TRY(hipSetDevice(ctx->device));
    LupinTexture *t = new LupinTexture();
    t->ctx = ctx; t->device = ctx->device; t->width = width; t->height = height; t->data = nullptr; t->accum32 = nullptr; t->accum32_valid = false;
    size_t bytes = (size_t)width * height * 4 * sizeof(__half);
    hipError_t e = device_view(&t->data_mem, (size_t)width * height * 4, &t->data);
    if (e != hipSuccess) { delete t; return fail(LUPIN_ERR_OUT_OF_MEMORY, hipGetErrorString(e)); }
    hipMemsetAsync(t->data, 0, bytes, ctx->stream);
    *out_tex = t;
    return LUPIN_OK;
}
void lupin_hip_texture_destroy(LupinTexture *tex)
{
    if (!tex) return;
    hipSetDevice(tex->device);
    if (ctx_alive(tex->ctx)) (void)sync_all(tex->ctx);   // a destroyed context has drained its streams already; a batch that fails here is dropped
    delete tex;   // frees the texels and the f32 shadow: after the synchronisation above
}
uint32_t lupin_hip_texture_width(const LupinTexture *tex) { return tex ? tex->width : 0; }
uint32_t lupin_hip_texture_height(const LupinTexture *tex) { return tex ? tex->height : 0; }
void *lupin_hip_texture_device_ptr(const LupinTexture *tex) { return tex ? (void *)tex->data : nullptr; }

int lupin_hip_texture_upload_rgba16f(LupinTexture *tex, const uint16_t *pixels)
{
    if (!tex || !pixels) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    CTX_ALIVE_TRY(tex->ctx);
    HIP_TRY(hipSetDevice(tex->ctx->device));
    if (int rc = join_primary(tex->ctx)) return rc;
    HIP_TRY(hipMemcpyAsync(tex->data, pixels, (size_t)tex->width * tex->height * 8, hipMemcpyHostToDevice, tex->ctx->stream));
    HIP_TRY(hipStreamSynchronize(tex->ctx->stream));
    tex->accum32_valid = false;   // the f16 texels are now the only truth
    return LUPIN_OK;
}
int lupin_hip_texture_download_rgba32f(const LupinTexture *tex, float *out_pixels)
{
    if (!tex || !out_pixels) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (!tex->accum32 || !tex->accum32_valid) return fail(LUPIN_ERR_INVALID_ARGUMENT, "texture has no f32 accumulator (render into it with LUPIN_ACCUM_F32 first)");
    CTX_ALIVE_TRY(tex->ctx);
    HIP_TRY(hipSetDevice(tex->ctx->device));
    if (int rc = join_primary(tex->ctx)) return rc;
    HIP_TRY(hipMemcpyAsync(out_pixels, tex->accum32, (size_t)tex->width * tex->height * 16, hipMemcpyDeviceToHost, tex->ctx->stream));
    HIP_TRY(hipStreamSynchronize(tex->ctx->stream));
    return LUPIN_OK;
}
int lupin_hip_texture_download_rgba16f(const LupinTexture *tex, uint16_t *out_pixels)
{
    if (!tex || !out_pixels) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    CTX_ALIVE_TRY(tex->ctx);
    HIP_TRY(hipSetDevice(tex->ctx->device));
    if (int rc = join_primary(tex->ctx)) return rc;
    HIP_TRY(hipMemcpyAsync(out_pixels, tex->data, (size_t)tex->width * tex->height * 8, hipMemcpyDeviceToHost, tex->ctx->stream));
    HIP_TRY(hipStreamSynchronize(tex->ctx->stream));
    return LUPIN_OK;
}

int lupin_hip_dbuf_create(LupinContext *ctx, uint32_t width, uint32_t height, LupinDoubleBufferedTexture **out)
{
    CTX_ALIVE_TRY(ctx);
    if (!out) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    LupinDoubleBufferedTexture *d = new LupinDoubleBufferedTexture();
    d->ctx = ctx; d->tex[0] = d->tex[1] = nullptr; d->front_idx = 1; d->back_idx = 0;   // wgpu_utils.rs:293-298
    int rc = lupin_hip_texture_create(ctx, width, height, &d->tex[0]);
    if (rc == LUPIN_OK) rc = lupin_hip_texture_create(ctx, width, height, &d->tex[1]);
    if (rc != LUPIN_OK) { lupin_hip_texture_destroy(d->tex[0]); delete d; return rc; }
    *out = d;
    return LUPIN_OK;
}
void lupin_hip_dbuf_destroy(LupinDoubleBufferedTexture *t)
{
    if (!t) return;
    lupin_hip_texture_destroy(t->tex[0]);
    lupin_hip_texture_destroy(t->tex[1]);
    delete t;
}
LupinTexture *lupin_hip_dbuf_front(LupinDoubleBufferedTexture *t) { return t ? t->tex[t->front_idx] : nullptr; }
LupinTexture *lupin_hip_dbuf_back(LupinDoubleBufferedTexture *t) { return t ? t->tex[t->back_idx] : nullptr; }
int lupin_hip_dbuf_copy_front_to_back(LupinDoubleBufferedTexture *t)
{
    if (!t) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    LupinTexture *f = t->tex[t->front_idx], *b = t->tex[t->back_idx];
    CTX_ALIVE_TRY(t->ctx);
    HIP_TRY(hipSetDevice(t->ctx->device));
    if (int rc = join_primary(t->ctx)) return rc;
    HIP_TRY(hipMemcpyAsync(b->data, f->data, (size_t)f->width * f->height * 8, hipMemcpyDeviceToDevice, t->ctx->stream));
    b->accum32_valid = false;
    if (f->accum32 && f->accum32_valid)
    {
        if (int rc = ensure_accum32(b, t->ctx->stream)) return rc;
        HIP_TRY(hipMemcpyAsync(b->accum32, f->accum32, (size_t)f->width * f->height * 16, hipMemcpyDeviceToDevice, t->ctx->stream));
        b->accum32_valid = true;
    }
    return LUPIN_OK;
}
void lupin_hip_dbuf_flip(LupinDoubleBufferedTexture *t) { if (t) std::swap(t->front_idx, t->back_idx); }
int lupin_hip_dbuf_resize(LupinDoubleBufferedTexture *t, uint32_t width, uint32_t height)
{
    if (!t) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (t->tex[0]->width == width && t->tex[0]->height == height) return LUPIN_OK;   // wgpu_utils.rs:343
    LupinTexture *a = nullptr, *b = nullptr;
    CTX_ALIVE_TRY(t->ctx);
    int rc = lupin_hip_texture_create(t->ctx, width, height, &a);
    if (rc == LUPIN_OK) rc = lupin_hip_texture_create(t->ctx, width, height, &b);
    if (rc != LUPIN_OK) { lupin_hip_texture_destroy(a); return rc; }
    lupin_hip_texture_destroy(t->tex[0]);
    lupin_hip_texture_destroy(t->tex[1]);
    t->tex[0] = a; t->tex[1] = b;
    return LUPIN_OK;
}

// ---- the hot path ----

static const char *const kWideStale = "lupin_hip_scene_update_instances moved this scene's instances and its four-wide hierarchy was not rebuilt: "
                                      "use the binary traversal or create the scene anew";

// The camera's share of get_push_constants (renderer.rs:1426-1493): what camera_ray_of reads.  Every entry point that
// generates camera rays (pathtrace_impl, the reprojection's primary trace, lupin_hip_camera_probe) fills it here.
static void set_camera_constants(LupinPushConstants &pc, const LupinCameraParams &cp, const LupinMat3x4 &ct)
{
    if (cp.is_orthographic) pc.flags |= LUPIN_FLAG_CAMERA_ORTHO;
    // Mat3x4::to_mat4 (base.rs:695-705)
    for (int c = 0; c < 4; c++) { pc.camera_transform.m[c][0] = ct.m[c][0]; pc.camera_transform.m[c][1] = ct.m[c][1]; pc.camera_transform.m[c][2] = ct.m[c][2]; pc.camera_transform.m[c][3] = (c == 3) ? 1.0f : 0.0f; }
    pc.camera_lens = cp.lens;
    pc.camera_film = cp.film;
    pc.camera_aspect = cp.aspect;
    pc.camera_focus = cp.focus;
    pc.camera_aperture = cp.aperture;
}
// ... and the scene's share: what an integrator may skip.  (The reprojection's primary trace shades nothing and sets none.)
static void set_scene_constants(LupinPushConstants &pc, const LupinScene *scene)
{
    if (scene->envs_empty) pc.flags |= LUPIN_FLAG_ENVS_EMPTY;
    if (scene->lights_empty) pc.flags |= LUPIN_FLAG_LIGHTS_EMPTY;
    if (scene->instances_empty) pc.flags |= LUPIN_FLAG_INSTANCES_EMPTY;
}

static int pathtrace_impl(LupinContext *ctx, const LupinPathtraceResources *res, const LupinScene *scene,
                          LupinTexture *render_target, uint32_t pathtrace_type, const LupinPathtraceDesc *desc,
                          bool tile_set, uint32_t set_tile_size, uint32_t rank, uint32_t world, int falsecolor_type = -1,
                          const LupinDebugVizDesc *debug = nullptr, LupinAdaptiveResources *adaptive = nullptr)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !res || !scene || !render_target || !desc) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (falsecolor_type < 0 && pathtrace_type > LUPIN_PATHTRACE_DIRECT) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown pathtrace_type");
    if (falsecolor_type > 11) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown falsecolor_type");
    if (debug && debug->viz_type > LUPIN_DEBUG_VIZ_NUM_BOUNCES) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown viz_type");
    if (!scene->has_sw_bvh) return fail(LUPIN_ERR_NO_SW_BVH, "no software BVH was built for this scene");   // renderer.rs:774-777
    if (scene->wide_stale && ctx->wide_traversal) return fail(LUPIN_ERR_INVALID_ARGUMENT, kWideStale);
    const uint32_t W = render_target->width, H = render_target->height;
    const LupinTexture *prev = desc->accum_params ? desc->accum_params->prev_frame : nullptr;
    if (prev && prev == render_target) return fail(LUPIN_ERR_SAME_TARGET, "render_target must differ from accum_params.prev_frame");
    if (prev && (prev->width != W || prev->height != H)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "prev_frame size differs from render_target");
    HIP_TRY(hipSetDevice(ctx->device));

    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    // get_push_constants (renderer.rs:1426-1493)
    LupinPushConstants &pc = fp.pc;
    set_camera_constants(pc, desc->camera_params, desc->camera_transform);
    set_scene_constants(pc, scene);
    if (debug)  // get_push_constants (renderer.rs:1430-1454)
    {
        pc.flags |= debug->viz_type == LUPIN_DEBUG_VIZ_BVH_AABB_CHECKS ? LUPIN_FLAG_DEBUG_AABB_CHECKS
                  : debug->viz_type == LUPIN_DEBUG_VIZ_BVH_TRI_CHECKS ? LUPIN_FLAG_DEBUG_TRI_CHECKS : LUPIN_FLAG_DEBUG_NUM_BOUNCES;
        if (debug->first_hit_only) pc.flags |= LUPIN_FLAG_DEBUG_FIRST_HIT_ONLY;
        pc.heatmap_min = debug->heatmap_min;
        pc.heatmap_max = debug->heatmap_max;
    }
    pc.pathtrace_type = (falsecolor_type < 0 && !debug) ? pathtrace_type : 0u;   // get_push_constants leaves the other selector at 0
    pc.falsecolor_type = falsecolor_type < 0 ? 0u : (uint32_t)falsecolor_type;
    pc.accum_counter = desc->accum_params ? desc->accum_params->accum_counter : 0u;
    pc.max_radiance = desc->advanced.max_radiance;
    pc.rng_seed = desc->advanced.rng_seed;
    pc.ray_epsilon = desc->advanced.ray_epsilon;

    fp.width = W; fp.height = H;
    fp.store_rne = (ctx->store_rounding == 1) ? 1u : 0u;
    fp.max_bounces = res->params.max_bounces;
    fp.spp = res->params.samples_per_pixel;
    uint64_t n64;
    if (tile_set)
    {
        if (set_tile_size == 0 || world == 0 || rank >= world) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad tile-set arguments");
        const uint32_t tpx = set_tile_size * LUPIN_WORKGROUP_SIZE;
        const uint32_t ntx = (std::max(1u, W) - 1) / tpx + 1, nty = (std::max(1u, H) - 1) / tpx + 1;
        const uint32_t total = ntx * nty;
        const uint32_t owned = lupin_owned_tile_count(total, rank, world);
        fp.tile_px = tpx; fp.tiles_x = ntx; fp.rank = rank; fp.world = world;
        n64 = (uint64_t)owned * tpx * tpx;
    }
    else
    {
        // dispatch extent (renderer.rs:807-838)
        uint32_t groups_x, groups_y;
        if (desc->tile_params)
        {
            uint32_t tile_size = desc->tile_params->tile_size, tile_idx = desc->tile_params->tile_idx;
            if (tile_size == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "tile_size must be > 0");
            uint32_t ntx = (std::max(1u, W) - 1) / (tile_size * LUPIN_WORKGROUP_SIZE) + 1;
            uint32_t nty = (std::max(1u, H) - 1) / (tile_size * LUPIN_WORKGROUP_SIZE) + 1;
            if (tile_idx >= ntx * nty) return fail(LUPIN_ERR_TILE_OUT_OF_RANGE, "tile_idx out of range!");
            pc.id_offset[0] = (tile_idx % ntx) * tile_size * LUPIN_WORKGROUP_SIZE;
            pc.id_offset[1] = (tile_idx / ntx) * tile_size * LUPIN_WORKGROUP_SIZE;
            groups_x = std::min(tile_size, (W - pc.id_offset[0]) / LUPIN_WORKGROUP_SIZE);   // floor: edge remainders are skipped
            groups_y = std::min(tile_size, (H - pc.id_offset[1]) / LUPIN_WORKGROUP_SIZE);
        }
        else
        {
            groups_x = (W + LUPIN_WORKGROUP_SIZE - 1) / LUPIN_WORKGROUP_SIZE;
            groups_y = (H + LUPIN_WORKGROUP_SIZE - 1) / LUPIN_WORKGROUP_SIZE;
        }
        fp.off_x = pc.id_offset[0]; fp.off_y = pc.id_offset[1];
        fp.reg_w = std::min(groups_x * LUPIN_WORKGROUP_SIZE, W - fp.off_x);   // texels outside the image are never stored (:287)
        fp.reg_h = std::min(groups_y * LUPIN_WORKGROUP_SIZE, H - fp.off_y);
        n64 = (uint64_t)fp.reg_w * fp.reg_h;
    }
    if (n64 == 0) return LUPIN_OK;
    if (n64 * 8u > (uint64_t)QUEUE_SLOT_MASK) return fail(LUPIN_ERR_INVALID_ARGUMENT, "dispatch too large");   // queue entries keep two bits for the light-pdf stage; a wavefront of dispatches this size holds up to eight frames (frames_per_wavefront)
    const uint32_t n = (uint32_t)n64;

    if (falsecolor_type >= 0 || debug)
    {
        const uint32_t fblocks = (n + LP_BLOCK - 1) / LP_BLOCK;
        TraversalLds t;
        if (int rc = traversal_lds(ctx, scene, scene->stack_entries, true, &t)) return rc;
        const __half *pv = prev ? prev->data : (const __half *)nullptr;
        if (int rc = join_primary(ctx)) return rc;
        render_target->accum32_valid = false;
        with_bool(t.geo, [&](auto G) {
            constexpr bool LDSGEO = decltype(G)::value;
            if (debug) hipLaunchKernelGGL(k_debug<LDSGEO>, dim3(fblocks), dim3(LP_BLOCK), t.lds, ctx->stream, scene->dev, fp, n, pv, render_target->data, t.stack_words);
            else hipLaunchKernelGGL(k_falsecolor<LDSGEO>, dim3(fblocks), dim3(LP_BLOCK), t.lds, ctx->stream, scene->dev, fp, n, pv, render_target->data, t.stack_words);
        });
        HIP_TRY(hipGetLastError());
        return LUPIN_OK;
    }

    // ---- record the call; run the batch when it is full or cannot grow (DESIGN 5 "Frames per wavefront") ----
    fp.frame_slots = n;
    fp.num_frames = 1;
    if (adaptive)
    {
        // one frame per wavefront: the next call's first rays read the mask this call's update writes
        if (int rc = flush_pending(ctx)) return rc;
        ctx->pending.push_back({fp, render_target, prev, adaptive});
        ctx->pending_scene = scene;
        ctx->pending_type = pathtrace_type;
        return flush_pending(ctx);
    }
    const uint32_t max_frames = frames_per_wavefront(ctx, n64);
    const bool batchable = max_frames > 1 && !ctx->counting && !ctx->verify_wide && !ctx->debug_sync && ctx->accum_mode != LUPIN_ACCUM_F32;
    if (!ctx->pending.empty())
    {
        // a call joins the batch if it differs from the batch's first call only in camera and accum_counter, and blends with
        // what the previous call of the batch stores (or with nothing: accum_counter 0)
        FrameParams a = ctx->pending.front().fp, b = fp;
        for (FrameParams *q : {&a, &b})
        {
            memset(&q->pc.camera_transform, 0, sizeof(q->pc.camera_transform));
            q->pc.camera_lens = q->pc.camera_film = q->pc.camera_aspect = q->pc.camera_focus = q->pc.camera_aperture = 0.0f;
            q->pc.accum_counter = 0;
            q->pc.flags &= ~(uint32_t)LUPIN_FLAG_CAMERA_ORTHO;
            q->num_frames = 1;
        }
        const bool joins = batchable && ctx->pending_scene == scene && ctx->pending_type == pathtrace_type && memcmp(&a, &b, sizeof(a)) == 0 &&
                           (fp.pc.accum_counter == 0 || prev == ctx->pending.back().target) && ctx->pending.size() < max_frames;
        if (!joins)
            if (int rc = flush_pending(ctx)) return rc;
    }
    ctx->pending.push_back({fp, render_target, prev});
    ctx->pending_scene = scene;
    ctx->pending_type = pathtrace_type;
    if (!batchable || ctx->pending.size() >= max_frames) return flush_pending(ctx);
    return LUPIN_OK;
}

// Runs the recorded calls as one wavefront: slot = frame * frame_slots + pixel slot, one resolve that applies the frames'
// blends per pixel in call order.  Errors of a deferred call surface here, i.e. at the call that needed its result.
static int flush_pending(LupinContext *ctx)
{
    if (ctx->pending.empty()) return LUPIN_OK;
    // run or refused, the batch is gone when this returns (nothing called from here comes back into it)
    struct Done { LupinContext *c; ~Done() { c->pending.clear(); c->pending_scene = nullptr; } } done{ctx};
    HIP_TRY(hipSetDevice(ctx->device));
    const LupinScene *scene = ctx->pending_scene;
    const uint32_t pathtrace_type = ctx->pending_type;
    const uint32_t K = (uint32_t)ctx->pending.size();
    FrameParams fp = ctx->pending.front().fp;
    fp.num_frames = K;
    const uint32_t frame_slots = fp.frame_slots;
    const uint32_t n = K * frame_slots;                         // slots of the wavefront
    LupinTexture *render_target = ctx->pending.back().target;    // (f32 accumulation is never batched: K == 1 there)
    const LupinTexture *prev = ctx->pending.front().prev;
    LupinAdaptiveResources *adaptive = ctx->pending.front().adaptive;   // (adaptive calls are never batched: K == 1 there)

    // Lane choice: consecutive wavefronts alternate over `lanes` streams so that they overlap; per-kernel timing needs them serial.
    // * A wavefront of ONE frame of a scene traced by the persistent kernel does not fill the chip in its middle iterations
    //   (bounded by the latency of one traversal): every lane is used (an eighth of the 4K frame: 34.1 -> 30.1 ms with 8 lanes).
    // * A wavefront of SEVERAL frames (the default: up to eight calls) fills it on its own, and then stages of different
    //   wavefronts only take LDS, registers and cache from each other: one lane, every stage with the chip to itself
    //   (bistro-class 4K, eight frames: 159 ms per step on one lane, 175 - 183 on two, 177 on three; profiles/r03_batch_matrix_short.txt).
    // * Launch-bound LDS-resident scenes are best with four lanes (Cornell box 8.0 against 7.2 Gsamples/s on one).
    const bool lds_scene = stages_geometry(ctx, scene);
    const int lanes = ctx->lanes_from_env ? ctx->num_lanes : std::min(lds_scene ? 4 : (K > 1 ? 1 : LP_MAX_LANES), ctx->num_lanes);
    const bool chip_to_itself = lanes == 1 || ctx->timing;
    const int w = ctx->timing ? 0 : (int)(ctx->call_index % (uint64_t)lanes);
    ctx->call_index++;
    Lane *ln = &ctx->lanes[w];
    hipStream_t st = ln->stream;

    const uint32_t iterations = fp.spp * (fp.max_bounces + 1);
    if (int rc = ensure_path_buffers(ctx, ln, n, iterations)) return rc;
    // scenes whose queues get sorted by material read the path state at scattered slots: records; otherwise planes
    set_path_layout(ln, ctx->path_records < 0 ? (scene->dev.sort_shade != 0) : ctx->path_records != 0);
    TraversalLds t;
    if (int rc = traversal_lds(ctx, scene, scene->stack_entries, true, &t)) return rc;

    hipEvent_t t0 = nullptr, t1 = nullptr;
    if (ctx->timing) { t0 = get_event(ctx); t1 = get_event(ctx); hipEventRecord(t0, st); }

    const Shape sh = plan_wavefront(ctx, ln, scene, pathtrace_type, chip_to_itself, t, n);
    ctx->last_lanes = lanes;
    ctx->last_wide = sh.wide.blocks != 0;
    ctx->last_batch = K;
    ctx->last_short = sh.shrt.blocks ? ctx->short_stack : 0u;
    for (uint32_t k = 0; k < K; k++)
    {
        FrameParams fk = ctx->pending[k].fp;
        fk.num_frames = K;
        hipLaunchKernelGGL(k_set_params, dim3(1), dim3(1), 0, st, fk, ln->d_fp + k);
    }
    if (adaptive)
    {
        // k_begin_adaptive reads the counts and the mask that the previous adaptive call's update wrote (on its lane, before
        // its `done`; the resolves chain every call after the one before) and that a reset wrote on the primary stream.
        // Consecutive one-frame wavefronts change lanes, so wait for both before the first rays.  No graph: launched directly.
        if (int rc = order_lane(ctx, ln)) return rc;
        HIP_TRY(enqueue_wavefront(ctx, ln, scene, pathtrace_type, n, sh, iterations, &adaptive->dev));
    }
    else if (ctx->use_graph && !ctx->timing && !ctx->counting && !ctx->verify_wide)
    {
        if (int rc = replay_wavefront(ctx, ln, scene, pathtrace_type, n, sh, iterations)) return rc;
    }
    else
        HIP_TRY(enqueue_wavefront(ctx, ln, scene, pathtrace_type, n, sh, iterations));
    // The frames meet here: the resolve reads prev_frame and overwrites render_target, so it is ordered after everything
    // enqueued so far on the other lane (the previous call's resolve) and, for lane 1, on the primary stream (texture
    // uploads / copies).  The path state itself is private to the lane.
    if (int rc = order_lane(ctx, ln)) return rc;
    const float4 *prev32 = nullptr;
    float4 *out32 = nullptr;
    if (ctx->accum_mode == LUPIN_ACCUM_F32)
    {
        if (int rc = ensure_accum32(render_target, st)) return rc;
        out32 = render_target->accum32;
        if (prev && prev->accum32 && prev->accum32_valid) prev32 = prev->accum32;
    }
    render_target->accum32_valid = out32 != nullptr;
    ResolveBatch rb;
    memset(&rb, 0, sizeof(rb));
    rb.count = K;
    for (uint32_t k = 0; k < K; k++)
    {
        rb.target[k] = ctx->pending[k].target->data;
        rb.accum_counter[k] = ctx->pending[k].fp.pc.accum_counter;
        bool last_write = true;
        for (uint32_t q = k + 1; q < K; q++) last_write = last_write && ctx->pending[q].target != ctx->pending[k].target;
        if (last_write) rb.store_mask |= 1u << k;
        if (k + 1 < K) ctx->pending[k].target->accum32_valid = false;
    }
    if (adaptive)
    {
        const AdaptiveDev &ad = adaptive->dev;
        const uint32_t nblocks = ad.blocks_x * ad.blocks_y;
        hipLaunchKernelGGL(k_resolve_adaptive, dim3((frame_slots + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, fp, ln->pb, frame_slots, ad,
                           render_target->data, prev->data, prev32, out32);
        HIP_TRY(hipMemsetAsync(ad.stats, 0, 3 * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(k_adaptive_update, dim3((nblocks + LP_BLOCK / 64 - 1) / (LP_BLOCK / 64)), dim3(LP_BLOCK), 0, st, ad);
        hipLaunchKernelGGL(k_adaptive_mask, dim3((nblocks + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, ad);
        adaptive->calls++;
    }
    else
        hipLaunchKernelGGL(k_resolve, dim3((frame_slots + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, fp, ln->pb, frame_slots, rb,
                           prev ? prev->data : (const __half *)nullptr, prev32, out32);
    HIP_TRY(hipEventRecord(ln->done, st));
    ln->used = true;
    ctx->last_lane = w;
    if (ctx->timing) { hipEventRecord(t1, st); ctx->ev_total.push_back({t0, t1}); }
    HIP_TRY(hipGetLastError());
    return LUPIN_OK;
}

int lupin_hip_pathtrace_scene(LupinContext *ctx, const LupinPathtraceResources *res, const LupinScene *scene,
                              LupinTexture *render_target, uint32_t pathtrace_type, const LupinPathtraceDesc *desc)
{
    return pathtrace_impl(ctx, res, scene, render_target, pathtrace_type, desc, false, 0, 0, 1);
}

int lupin_hip_pathtrace_scene_falsecolor(LupinContext *ctx, const LupinPathtraceResources *res, const LupinScene *scene,
                                         LupinTexture *render_target, uint32_t falsecolor_type, const LupinPathtraceDesc *desc)
{
    if (falsecolor_type > 11) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown falsecolor_type");
    return pathtrace_impl(ctx, res, scene, render_target, 0, desc, false, 0, 0, 1, (int)falsecolor_type);
}

int lupin_hip_pathtrace_scene_debug(LupinContext *ctx, const LupinPathtraceResources *res, const LupinScene *scene,
                                    LupinTexture *render_target, const LupinDebugVizDesc *debug_desc, const LupinPathtraceDesc *desc)
{
    if (!debug_desc) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    return pathtrace_impl(ctx, res, scene, render_target, 0, desc, false, 0, 0, 1, -1, debug_desc);
}

int lupin_hip_pathtrace_scene_tiles(LupinContext *ctx, const LupinPathtraceResources *res, const LupinScene *scene,
                                    LupinTexture *render_target, uint32_t pathtrace_type, const LupinPathtraceDesc *desc,
                                    uint32_t tile_size, uint32_t rank, uint32_t world)
{
    return pathtrace_impl(ctx, res, scene, render_target, pathtrace_type, desc, true, tile_size, rank, world);
}

// ---- measurement hooks ----

int lupin_hip_stats_reset(LupinContext *ctx, int enable_kernel_timing)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "ctx is null");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = sync_all(ctx)) return rc;
    for (int k = 0; k < ctx->num_lanes; k++)
        HIP_TRY(hipMemsetAsync(ctx->lanes[k].stat_counters, 0, 2 * LP_SHARDS * sizeof(unsigned long long), ctx->lanes[k].stream));
    // extend/shade pairs share their middle event: recycle each event once
    for (auto &p : ctx->ev_extend) { ctx->ev_pool.push_back(p.first); ctx->ev_pool.push_back(p.second); }
    for (auto &p : ctx->ev_shade) { ctx->ev_pool.push_back(p.second); }
    ctx->ev_extend.clear();
    ctx->ev_shade.clear();
    for (auto &p : ctx->ev_total) { ctx->ev_pool.push_back(p.first); ctx->ev_pool.push_back(p.second); }
    ctx->ev_total.clear();
    for (int k = 0; k < ctx->num_lanes; k++)
    {
        HIP_TRY(hipMemsetAsync(ctx->lanes[k].work_counters, 0, LP_WORK_WORDS * sizeof(unsigned long long), ctx->lanes[k].stream));
        HIP_TRY(hipMemsetAsync(ctx->lanes[k].wide_counters, 0, LP_WIDE_WORDS * sizeof(unsigned long long), ctx->lanes[k].stream));
    }
    ctx->timing = enable_kernel_timing == LUPIN_STATS_KERNEL_TIMING;
    ctx->counting = enable_kernel_timing == LUPIN_STATS_WORK_COUNTERS;
    ctx->extend_launches = 0;
    return LUPIN_OK;
}

int lupin_hip_stats_get(LupinContext *ctx, LupinStats *out)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !out) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = sync_all(ctx)) return rc;
    std::vector<unsigned long long> c(2 * LP_SHARDS, 0ull);
    memset(out, 0, sizeof(*out));
    for (int l = 0; l < ctx->num_lanes; l++)
    {
        HIP_TRY(hipMemcpy(c.data(), ctx->lanes[l].stat_counters, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < LP_SHARDS; k++) { out->path_bounces += c[2 * k]; out->paths += c[2 * k + 1]; }
    }
    for (int l = 0; l < ctx->num_lanes; l++)
    {
        unsigned long long w[LP_WORK_WORDS];
        HIP_TRY(hipMemcpy(w, ctx->lanes[l].work_counters, sizeof(w), hipMemcpyDeviceToHost));
        for (int m = 0; m < 3; m++)
        {
            out->node_visits[m] += w[4 * m + 0]; out->tri_tests[m] += w[4 * m + 1]; out->instance_entries[m] += w[4 * m + 2];
            out->wide_node_visits[m] += w[4 * m + 3];
        }
        for (int k = 0; k < 10; k++) out->tracer_rounds[k] += w[12 + k];
        for (int k = 0; k < 6; k++) out->tracer_cycles[k] += w[22 + k];
        unsigned long long wd[LP_WIDE_WORDS];
        HIP_TRY(hipMemcpy(wd, ctx->lanes[l].wide_counters, sizeof(wd), hipMemcpyDeviceToHost));
        out->wide_queries += wd[0]; out->wide_retraced += wd[1];
        out->verify_checked += wd[2]; out->verify_flagged += wd[3]; out->verify_mismatches += wd[4]; out->verify_raw_mismatches += wd[5];
        for (int k = 0; k < 4; k++) out->verify_reasons[k] += wd[6 + k];
    }
    out->frames_in_flight = (uint32_t)std::max(0, ctx->last_lanes);
    out->wide_traversal = ctx->last_wide ? 1u : 0u;
    out->frames_per_wavefront = ctx->last_batch;
    out->short_stack_entries = ctx->last_short;
    out->extend_launches = ctx->extend_launches;
    auto sum = [](const std::vector<std::pair<hipEvent_t, hipEvent_t>> &v) {
        double ms = 0.0;
        for (auto &p : v) { float f = 0.0f; if (hipEventElapsedTime(&f, p.first, p.second) == hipSuccess) ms += f; }
        return ms;
    };
    out->extend_ms = sum(ctx->ev_extend);
    out->shade_ms = sum(ctx->ev_shade);
    out->total_ms = sum(ctx->ev_total);
    return LUPIN_OK;
}

int lupin_hip_measure_copy_bandwidth(LupinContext *ctx, uint64_t bytes, uint32_t reps, double *out_gb_per_s)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !out_gb_per_s || bytes < 16 || reps == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad copy-bandwidth arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = sync_all(ctx)) return rc;
    const size_t n = bytes / 16;
    DeviceBuffer da, db;
    hipError_t e = DeviceBuffer::make(n * 16, &da);
    if (e == hipSuccess) e = DeviceBuffer::make(n * 16, &db);
    if (e != hipSuccess) return fail(LUPIN_ERR_OUT_OF_MEMORY, hipGetErrorString(e));
    float4 *a = da.as<float4>(), *b = db.as<float4>();
    hipEvent_t e0 = get_event(ctx), e1 = get_event(ctx);
    HIP_TRY(hipMemsetAsync(a, 0x3C, n * 16, ctx->stream));
    const uint32_t blocks = (uint32_t)((n + LP_BLOCK - 1) / LP_BLOCK);   // one 16-byte element per thread: the shape that reaches the guide's 6.29 TB/s (tools/calib/copy_probe.hip)
    hipLaunchKernelGGL(k_copy_bw, dim3(blocks), dim3(LP_BLOCK), 0, ctx->stream, (const float4 *)a, b, n);   // warm-up: pages touched
    HIP_TRY(hipEventRecord(e0, ctx->stream));
    for (uint32_t r = 0; r < reps; r++)
        hipLaunchKernelGGL(k_copy_bw, dim3(blocks), dim3(LP_BLOCK), 0, ctx->stream, (const float4 *)((r & 1) ? b : a), (r & 1) ? a : b, n);
    HIP_TRY(hipEventRecord(e1, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    ctx->ev_pool.push_back(e0); ctx->ev_pool.push_back(e1);
    *out_gb_per_s = ms > 0.0f ? 2.0 * (double)(n * 16) * reps / (ms * 1e-3) / 1e9 : 0.0;   // bytes read + bytes written
    return LUPIN_OK;
}

int lupin_hip_runtime_info(LupinRuntimeInfo *out)
{
    if (!out) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    memset(out, 0, sizeof(*out));
    out->build_hip_version = HIP_VERSION;
    int v = 0;
    if (hipRuntimeGetVersion(&v) == hipSuccess) out->runtime_hip_version = v;
    // every distinct libamdhip64 mapped into this process (a PyTorch wheel bundles its own copy)
    std::vector<std::string> libs;
    if (FILE *f = fopen("/proc/self/maps", "r"))
    {
        char line[4096];
        while (fgets(line, sizeof(line), f))
        {
            const char *p = strstr(line, "libamdhip64");
            if (!p) continue;
            const char *path = strchr(line, '/');
            if (!path) continue;
            std::string sp(path);
            while (!sp.empty() && (sp.back() == '\n' || sp.back() == ' ')) sp.pop_back();
            if (std::find(libs.begin(), libs.end(), sp) == libs.end()) libs.push_back(sp);
        }
        fclose(f);
    }
    out->num_hip_runtimes_mapped = (uint32_t)libs.size();
    std::string joined;
    for (auto &l : libs) { if (!joined.empty()) joined += ";"; joined += l; }
    strncpy(out->hip_runtime_paths, joined.c_str(), sizeof(out->hip_runtime_paths) - 1);
    return LUPIN_OK;
}

int64_t lupin_hip_collapse_bvh4(const LupinBvhNode *nodes, uint32_t num_nodes, const float *verts_pos4, uint32_t num_verts, const uint32_t *indices,
                                uint32_t num_indices, void *out_nodes, uint64_t capacity, uint32_t *out_root, uint8_t *out_tri_flags)
{
    if (!nodes || num_nodes == 0 || !out_root) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    const uint32_t num_tris = num_indices / 3;
    for (uint32_t n = 0; n < num_nodes; n++)
        if (nodes[n].tri_count == 0 && (uint64_t)nodes[n].tri_begin_or_first_child + 1 >= num_nodes) return fail(LUPIN_ERR_INVALID_ARGUMENT, "BLAS child index out of bounds");
    if (blas_depth(nodes, num_nodes) == 0xFFFFFFFFu) return fail(LUPIN_ERR_INVALID_ARGUMENT, "BLAS is not a tree");
    if (verts_pos4 && indices)
        for (uint32_t i = 0; i < num_tris * 3; i++) if (indices[i] >= num_verts) return fail(LUPIN_ERR_INVALID_ARGUMENT, "vertex index out of range");
    std::vector<WideNode> pairs;
    std::vector<uint32_t> leaf_ends, leaky;
    const char *why = nullptr;
    const uint32_t root = blas_child_pairs(nodes, num_nodes, num_tris, 0u, pairs, leaf_ends, &why, verts_pos4, indices, &leaky);
    if (why) return fail(LUPIN_ERR_INVALID_ARGUMENT, why);
    std::vector<Wide4> wide;
    *out_root = collapse_to_wide4(pairs, root, wide);
    if (out_tri_flags)
    {
        memset(out_tri_flags, 0, num_tris);
        for (uint32_t t : leaky) out_tri_flags[t] |= 2u;
        for (uint32_t t : leaf_ends) out_tri_flags[t] |= 1u;
    }
    if (out_nodes)
    {
        if (wide.size() > capacity) return fail(LUPIN_ERR_INVALID_ARGUMENT, "out_nodes too small");
        if (!wide.empty()) memcpy(out_nodes, wide.data(), wide.size() * sizeof(Wide4));
    }
    return (int64_t)wide.size();
}

static int trace_rays_impl(LupinContext *ctx, const LupinScene *scene, uint32_t n, const float *ori_xyz, const float *dir_xyz,
                           float ray_epsilon, uint32_t *out_hit, float *out_dst, float *out_uv, uint32_t *out_instance, uint32_t *out_tri, uint32_t *out_flag)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !scene || !ori_xyz || !dir_xyz || !out_hit || !out_dst || !out_uv || !out_instance || !out_tri) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (out_flag && scene->wide_stale) return fail(LUPIN_ERR_INVALID_ARGUMENT, kWideStale);
    if (out_flag && !scene->has_wide) return fail(LUPIN_ERR_INVALID_ARGUMENT, "this scene has no four-wide hierarchy (it is small enough to be staged in LDS)");
    if (n == 0) return LUPIN_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    // stacks only: both kernels read the geometry from global memory
    TraversalLds t;
    if (int rc = traversal_lds(ctx, scene, out_flag ? 2u * ctx->wide_stack_pairs : scene->stack_entries, false, &t)) return rc;
    DeviceBuffer b_ori, b_dir, b_dst, b_uv, b_hit, b_inst, b_tri, b_flag;   // freed on every path out of here
    HIP_TRY(DeviceBuffer::make((size_t)n * 12, &b_ori));
    HIP_TRY(DeviceBuffer::make((size_t)n * 12, &b_dir));
    HIP_TRY(DeviceBuffer::make((size_t)n * 4, &b_dst));
    HIP_TRY(DeviceBuffer::make((size_t)n * 8, &b_uv));
    HIP_TRY(DeviceBuffer::make((size_t)n * 4, &b_hit));
    HIP_TRY(DeviceBuffer::make((size_t)n * 4, &b_inst));
    HIP_TRY(DeviceBuffer::make((size_t)n * 4, &b_tri));
    if (out_flag) HIP_TRY(DeviceBuffer::make((size_t)n * 4, &b_flag));
    float *d_ori = b_ori.as<float>(), *d_dir = b_dir.as<float>(), *d_dst = b_dst.as<float>(), *d_uv = b_uv.as<float>();
    uint32_t *d_hit = b_hit.as<uint32_t>(), *d_inst = b_inst.as<uint32_t>(), *d_tri = b_tri.as<uint32_t>(), *d_flag = b_flag.as<uint32_t>();
    HIP_TRY(hipMemcpyAsync(d_ori, ori_xyz, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_dir, dir_xyz, (size_t)n * 12, hipMemcpyHostToDevice, ctx->stream));
    if (out_flag)
    {
        hipLaunchKernelGGL(k_trace_wide, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), t.lds, ctx->stream, scene->dev, n, d_ori, d_dir, ray_epsilon,
                           ctx->wide_stack_pairs, d_hit, d_dst, d_uv, d_inst, d_tri, d_flag);
        HIP_TRY(hipMemcpyAsync(out_flag, d_flag, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    else
        hipLaunchKernelGGL(k_trace, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), t.lds, ctx->stream, scene->dev, n, d_ori, d_dir, ray_epsilon,
                           d_hit, d_dst, d_uv, d_inst, d_tri);
    HIP_TRY(hipMemcpyAsync(out_hit, d_hit, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out_dst, d_dst, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out_uv, d_uv, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out_instance, d_inst, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out_tri, d_tri, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return LUPIN_OK;
}

int lupin_hip_trace_rays(LupinContext *ctx, const LupinScene *scene, uint32_t n, const float *ori_xyz, const float *dir_xyz,
                         float ray_epsilon, uint32_t *out_hit, float *out_dst, float *out_uv, uint32_t *out_instance, uint32_t *out_tri)
{
    return trace_rays_impl(ctx, scene, n, ori_xyz, dir_xyz, ray_epsilon, out_hit, out_dst, out_uv, out_instance, out_tri, nullptr);
}

int lupin_hip_trace_rays_wide(LupinContext *ctx, const LupinScene *scene, uint32_t n, const float *ori_xyz, const float *dir_xyz,
                              float ray_epsilon, uint32_t *out_hit, float *out_dst, float *out_uv, uint32_t *out_instance, uint32_t *out_tri,
                              uint32_t *out_needs_retrace)
{
    if (!out_needs_retrace) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    return trace_rays_impl(ctx, scene, n, ori_xyz, dir_xyz, ray_epsilon, out_hit, out_dst, out_uv, out_instance, out_tri, out_needs_retrace);
}

int lupin_hip_detmath_probe(LupinContext *ctx, int fn, uint32_t n, const float *x, const float *y, float *out)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !x || !y || !out) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return LUPIN_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    return run_probe(ctx, "lupin_hip_detmath_probe", {{x, (size_t)n * 4}, {y, (size_t)n * 4}}, out, (size_t)n * 4, [&](const DeviceBuffer *in, float *dout) {
        hipLaunchKernelGGL(k_detmath, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, ctx->stream, fn, n, in[0].as<float>(), in[1].as<float>(), dout);
    });
}

int lupin_hip_scatter_probe(LupinContext *ctx, uint32_t n, const float *records, float *out)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !records || !out) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (n == 0) return LUPIN_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    const size_t in_bytes = (size_t)n * LUPIN_SCATTER_IN_FLOATS * 4, out_bytes = (size_t)n * LUPIN_SCATTER_OUT_FLOATS * 4;
    return run_probe(ctx, "lupin_hip_scatter_probe", {{records, in_bytes}}, out, out_bytes, [&](const DeviceBuffer *in, float *dout) {
        hipLaunchKernelGGL(k_scatter_probe, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, ctx->stream, n, in[0].as<float>(), dout);
    });
}

int lupin_hip_light_probe(LupinContext *ctx, const LupinScene *scene, uint32_t n, const float *records, float *out)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !scene || !records || !out) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (scene->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "the scene belongs to another context");
    if (n == 0) return LUPIN_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    TraversalLds t;
    if (int rc = traversal_lds(ctx, scene, scene->stack_entries, true, &t)) return rc;
    if (int rc = join_primary(ctx)) return rc;   // recorded calls run first
    const size_t in_bytes = (size_t)n * LUPIN_LIGHT_IN_FLOATS * 4, out_bytes = (size_t)n * LUPIN_LIGHT_OUT_FLOATS * 4;
    return run_probe(ctx, "lupin_hip_light_probe", {{records, in_bytes}}, out, out_bytes, [&](const DeviceBuffer *in, float *dout) {
        with_bool(t.geo, [&](auto G) {
            hipLaunchKernelGGL(k_light_probe<decltype(G)::value>, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), t.lds, ctx->stream, scene->dev, n,
                               in[0].as<float>(), dout, t.stack_words);
        });
    });
}

int lupin_hip_surface_probe(LupinContext *ctx, const LupinScene *scene, uint32_t n, const float *records, float *out)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !scene || !records || !out) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (scene->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "the scene belongs to another context");
    if (n == 0) return LUPIN_OK;
    // every index a record names is checked here: the kernel dereferences them as they are
    for (uint32_t i = 0; i < n; i++)
    {
        const float *r = records + (size_t)i * LUPIN_SURFACE_IN_FLOATS;
        const uint32_t mode = surface_probe_mode(r[0]);
        uint32_t a, tri;
        memcpy(&a, &r[1], 4); memcpy(&tri, &r[2], 4);
        if (mode == LUPIN_SURFACE_TEXTURE)
        {
            if (a >= scene->num_textures) return fail(LUPIN_ERR_INVALID_ARGUMENT, "lupin_hip_surface_probe: texture index out of range");
        }
        else if (mode >= LUPIN_SURFACE_MATERIAL && mode <= LUPIN_SURFACE_NORMAL)
        {
            if (a >= scene->host_instances.size()) return fail(LUPIN_ERR_INVALID_ARGUMENT, "lupin_hip_surface_probe: instance index out of range");
            if (tri >= scene->mesh_tri_count[scene->host_instances[a].mesh_idx]) return fail(LUPIN_ERR_INVALID_ARGUMENT, "lupin_hip_surface_probe: triangle index out of range");
            if (mode == LUPIN_SURFACE_MATERIAL_SIMPLE && !scene->simple_matte)
                return fail(LUPIN_ERR_INVALID_ARGUMENT, "lupin_hip_surface_probe: MATERIAL_SIMPLE on a scene that is not one of untextured matte materials");
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    TraversalLds t;   // the staged geometry, if any: this kernel never traverses
    if (int rc = traversal_lds(ctx, scene, 0, true, &t)) return rc;
    if (int rc = join_primary(ctx)) return rc;   // recorded calls run first
    const size_t in_bytes = (size_t)n * LUPIN_SURFACE_IN_FLOATS * 4, out_bytes = (size_t)n * LUPIN_SURFACE_OUT_FLOATS * 4;
    return run_probe(ctx, "lupin_hip_surface_probe", {{records, in_bytes}}, out, out_bytes, [&](const DeviceBuffer *in, float *dout) {
        with_bool(t.geo, [&](auto G) {
            hipLaunchKernelGGL(k_surface_probe<decltype(G)::value>, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), t.lds, ctx->stream, scene->dev, n,
                               in[0].as<float>(), dout);
        });
    });
}

int lupin_hip_camera_probe(LupinContext *ctx, uint32_t width, uint32_t height, const LupinCameraParams *camera_params,
                           const LupinMat4 *camera_transform, uint32_t n, const uint32_t *records, float *out)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !camera_params || !camera_transform || !records || !out) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (width == 0 || height == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "lupin_hip_camera_probe: empty image");
    if (n == 0) return LUPIN_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    LupinMat3x4 ct;
    for (int c = 0; c < 4; c++) for (int r = 0; r < 3; r++) ct.m[c][r] = camera_transform->m[c][r];
    set_camera_constants(fp.pc, *camera_params, ct);
    // the renderer's last row is (0, 0, 0, 1); the probe passes the caller's on, and the ray must not depend on it
    for (int c = 0; c < 4; c++) fp.pc.camera_transform.m[c][3] = camera_transform->m[c][3];
    fp.width = width; fp.height = height; fp.reg_w = width; fp.reg_h = height;
    if (int rc = join_primary(ctx)) return rc;   // recorded calls run first
    const size_t in_bytes = (size_t)n * LUPIN_CAMERA_IN_WORDS * 4, out_bytes = (size_t)n * LUPIN_CAMERA_OUT_FLOATS * 4;
    return run_probe(ctx, "lupin_hip_camera_probe", {{records, in_bytes}}, out, out_bytes, [&](const DeviceBuffer *in, float *dout) {
        hipLaunchKernelGGL(k_camera_probe, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, ctx->stream, fp, n, in[0].as<uint32_t>(), dout);
    });
}

// ---- what the scene queries share (DESIGN.md 5 "The scene queries' host scaffold") ----
// An entry point reads: query_refuse, the checks of its own arguments, query_refuse_hierarchy, n == 0, query_start, its
// chunks, query_end.  The order is the contract: the first check that fails decides the error.
extern "C++" {   // (there are templates among them, and the entry points around them are extern "C")

// the refusals every scene query opens with; `args`: the entry point's own pointers are all there
static int query_refuse_context(const LupinContext *ctx, bool args)   // (the part that needs no scene: lupin_hip_denoise_lightmap has none)
{
    if (!ctx_alive(ctx) && lupin_hip_device_count() <= 0) return fail(LUPIN_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !args) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    return LUPIN_OK;
}
static int query_refuse(const LupinContext *ctx, const LupinScene *scene, bool args)
{
    if (int rc = query_refuse_context(ctx, scene && args)) return rc;
    if (scene->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "the scene belongs to another context, or to one that has been destroyed");
    return LUPIN_OK;
}
// ... and the ones about the scene's hierarchies (a stale four-wide hierarchy is no obstacle to a query that reads only the binary one)
static int query_refuse_hierarchy(const LupinContext *ctx, const LupinScene *scene, bool reads_wide)
{
    if (!scene->has_sw_bvh) return fail(LUPIN_ERR_NO_SW_BVH, "no software BVH was built for this scene");
    if (reads_wide && scene->wide_stale && ctx->wide_traversal) return fail(LUPIN_ERR_INVALID_ARGUMENT, kWideStale);
    return LUPIN_OK;
}
// the calls recorded so far run first, whatever becomes of this one from here on
static int query_flush(LupinContext *ctx)
{
    HIP_TRY(hipSetDevice(ctx->device));
    return flush_pending(ctx);
}
// the LDS plan for a per-lane stack of `stack_entries` entries; then the gate: the primary stream, the query's own, waits for the latest of the recorded calls
static int query_plan(LupinContext *ctx, const LupinScene *scene, uint32_t stack_entries, TraversalLds *t)
{
    if (int rc = traversal_lds(ctx, scene, stack_entries, true, t)) return rc;
    return join_primary(ctx);
}
// every call ends synchronised
static int query_end(LupinContext *ctx, const char *who)
{
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(LUPIN_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    return LUPIN_OK;
}

// host records: the first one the format's Rule (lupin_rays.hpp) refuses is named
template <typename Rule>
static int refuse_bad_host_records(uint64_t n, const float *records)
{
    for (uint64_t i = 0; i < n; i++)
        if (!Rule::host_ok(records + i * Rule::FLOATS))
            return fail(LUPIN_ERR_INVALID_ARGUMENT, std::string(Rule::NOUN) + " " + std::to_string(i) + ": " + Rule::WHY);
    return LUPIN_OK;
}
// device records: `validate` (a k_validate_records<Rule>) counts them into the context's counter; the host waits for the count
static int count_bad_records(LupinContext *ctx, void (*validate)(const float4 *, unsigned long long, unsigned long long *), const float *records, uint64_t n,
                             unsigned long long *count)
{
    hipStream_t st = ctx->stream;
    if (!ctx->bad_records.get()) HIP_TRY(DeviceBuffer::make(sizeof(unsigned long long), &ctx->bad_records));
    HIP_TRY(hipMemsetAsync(ctx->bad_records.get(), 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(validate, dim3((uint32_t)((n + LP_BLOCK - 1) / LP_BLOCK)), dim3(LP_BLOCK), 0, st, reinterpret_cast<const float4 *>(records),
                       (unsigned long long)n, ctx->bad_records.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(count, ctx->bad_records.get(), sizeof(*count), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LUPIN_OK;
}
template <typename Rule>
static int refuse_bad_device_records(LupinContext *ctx, uint64_t n, const float *records)
{
    unsigned long long count = 0;
    if (int rc = count_bad_records(ctx, k_validate_records<Rule>, records, n, &count)) return rc;
    if (count) return fail(LUPIN_ERR_INVALID_ARGUMENT, std::to_string(count) + " " + Rule::NOUN + "(s): " + Rule::WHY);
    return LUPIN_OK;
}

// The start of a query over `n` records of format Rule, once the entry point's own arguments are accepted: host records
// are looked at after the recorded calls have run and before anything is planned, device records once the stream is the
// query's.  The plan is for a stack of `stack_entries` (`stage`: traversal_lds'); t == nullptr: a query that does not read
// the scene plans nothing.  (The distance queries put the same pieces in their own order.)
template <typename Rule>
static int query_start(LupinContext *ctx, const LupinScene *scene, bool on_device, uint64_t n, const float *records, uint32_t stack_entries, bool stage,
                       TraversalLds *t)
{
    if (int rc = query_flush(ctx)) return rc;
    if (!on_device)
        if (int rc = refuse_bad_host_records<Rule>(n, records)) return rc;
    if (t)
        if (int rc = traversal_lds(ctx, scene, stack_entries, stage, t)) return rc;
    if (int rc = join_primary(ctx)) return rc;
    return on_device ? refuse_bad_device_records<Rule>(ctx, n, records) : LUPIN_OK;
}
// ... with a stack of the scene's depth: every query but the irradiance volume's two
template <typename Rule>
static int query_start(LupinContext *ctx, const LupinScene *scene, bool on_device, uint64_t n, const float *records, TraversalLds *t)
{
    return query_start<Rule>(ctx, scene, on_device, n, records, scene->stack_entries, true, t);
}

// The path queries (radiance queries, probe bakes: DESIGN.md 13, 15).
// Path state is 312 bytes per slot (ensure_path_buffers: two 128-byte records, 16 + 16 of medium, 4 + 4 of queues, 8 of
// re-trace tokens, 4 + 4 of sort key and shade order): the default chunk of 4 Mi paths holds 1.3 GB of it.
static constexpr uint64_t LP_RAYS_DEFAULT_SLOTS = LUPIN_RAYS_DEFAULT_MAX_SLOTS;
static constexpr uint64_t LP_RAYS_MAX_CHUNK_SLOTS = 1ull << 27;   // the largest dispatch a render accepts (QUEUE_SLOT_MASK / 8)
static constexpr uint64_t LP_RAYS_MAX_PATHS = 1ull << 38;         // n * samples: record and slot indices, byte offsets and grids stay far from their types' ends

// What the wavefronts of a radiance query and of a probe bake share.  The frame parameters of paths that are slots, not pixels:
static FrameParams query_frame_params(const LupinScene *scene, uint32_t pathtrace_type, uint32_t max_bounces, const LupinAdvancedParams &advanced)
{
    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    LupinPushConstants &pc = fp.pc;
    set_scene_constants(pc, scene);
    pc.pathtrace_type = pathtrace_type;
    pc.max_radiance = advanced.max_radiance;
    pc.rng_seed = advanced.rng_seed;
    pc.ray_epsilon = advanced.ray_epsilon;
    fp.height = fp.reg_h = 1;
    fp.max_bounces = max_bounces;
    fp.spp = 1;            // a path that ends is never followed by a camera sample (path_epilogue)
    fp.num_frames = 1;
    return fp;
}
// ... and the launch shape of one chunk of `slots` paths (the lane's shard capacity and fp's width with it)
static Shape query_chunk_shape(LupinContext *ctx, const LupinScene *scene, uint32_t pathtrace_type, const TraversalLds &t, uint32_t slots, Lane *ln,
                               FrameParams *fp)
{
    fp->width = fp->reg_w = fp->frame_slots = slots;
    return plan_wavefront(ctx, ln, scene, pathtrace_type, true, t, slots);
}

// lupin_hip_pathtrace_rays and lupin_hip_bake_probes are twins: records (rays | probes) of format Rule expand into `samples`
// paths each, chunks of them run the wavefront, a resolve kernel folds a record's paths into `result_floats` floats.  What
// differs is the descriptor's type, here flattened, and the two launches of a chunk, handed in.
struct PathQuery
{
    const char *who;
    uint32_t pathtrace_type, flags, samples, max_bounces, max_slots;   // flags: bit 0 = device pointers, for both
    const LupinAdvancedParams *advanced;
    uint32_t result_floats;
};
struct PathChunk   // all that `launch` sees of the query and of one chunk: device pointers whichever side the caller's arrays are on
{
    Lane *ln;
    Shape sh;
    uint32_t pathtrace_type, samples, slots, records, iterations;
    const float4 *d_records;
    float4 *d_rays, *d_out;   // d_rays: the chunk's first slot, or nullptr
};
template <typename Rule, typename Launch>
static int path_query(LupinContext *ctx, const LupinScene *scene, const PathQuery &q, uint64_t n, const float *records, float *out, float *out_rays,
                      Launch launch)
{
    if (q.pathtrace_type > LUPIN_PATHTRACE_DIRECT) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown pathtrace_type");
    static_assert(LUPIN_RAYS_DEVICE_POINTERS == LUPIN_PROBES_DEVICE_POINTERS, "one flag word for both twins");
    if (q.flags & ~(uint32_t)LUPIN_RAYS_DEVICE_POINTERS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown flag");
    if (q.samples == 0 || q.samples > LP_RAYS_MAX_CHUNK_SLOTS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "samples must be in [1, 2^27]");
    if (q.max_bounces >= META_BOUNCE_MASK) return fail(LUPIN_ERR_INVALID_ARGUMENT, "max_bounces must be < 4095");
    const uint64_t S = q.samples;
    if (n > LP_RAYS_MAX_PATHS / S) return fail(LUPIN_ERR_INVALID_ARGUMENT, "n * samples must not exceed 2^38");
    if (int rc = query_refuse_hierarchy(ctx, scene, true)) return rc;
    const bool on_device = (q.flags & LUPIN_RAYS_DEVICE_POINTERS) != 0;
    if (on_device && (((uintptr_t)records | (uintptr_t)out | (uintptr_t)out_rays) & 15u))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "device pointers must be 16-byte aligned");
    if (n == 0) return LUPIN_OK;
    TraversalLds t;
    if (int rc = query_start<Rule>(ctx, scene, on_device, n, records, &t)) return rc;
    Lane *ln = &ctx->lanes[0];   // one lane for every chunk: its stream is the primary stream
    hipStream_t st = ln->stream;

    const uint64_t max_slots = std::min(q.max_slots ? (uint64_t)q.max_slots : LP_RAYS_DEFAULT_SLOTS, LP_RAYS_MAX_CHUNK_SLOTS);
    const uint64_t chunk_records = std::min(n, std::max<uint64_t>(1, max_slots / S));
    const uint32_t iterations = q.max_bounces + 1;
    int rc = ensure_path_buffers(ctx, ln, chunk_records * S, iterations);
    if (rc != LUPIN_OK) return rc;
    set_path_layout(ln, ctx->path_records < 0 ? (scene->dev.sort_shade != 0) : ctx->path_records != 0);

    // host arrays: one chunk's records, results and first rays at a time through device buffers that live for the call
    // (the path state beside them is the large allocation, and these are released with the call as they always were)
    DeviceBuffer d_rec, d_out, d_rays;
    if (!on_device)
    {
        HIP_TRY(DeviceBuffer::make((size_t)chunk_records * Rule::FLOATS * 4, &d_rec));
        HIP_TRY(DeviceBuffer::make((size_t)chunk_records * q.result_floats * 4, &d_out));
        if (out_rays) HIP_TRY(DeviceBuffer::make((size_t)(chunk_records * S) * LUPIN_RAY_RECORD_FLOATS * 4, &d_rays));
    }

    FrameParams fp = query_frame_params(scene, q.pathtrace_type, q.max_bounces, *q.advanced);

    for (uint64_t first = 0; first < n; first += chunk_records)
    {
        const uint64_t recs = std::min(chunk_records, n - first);
        const uint32_t slots = (uint32_t)(recs * S);
        const float *src = records + first * Rule::FLOATS;
        float *dst = out + first * q.result_floats;
        float *dst_rays = out_rays ? out_rays + first * S * LUPIN_RAY_RECORD_FLOATS : nullptr;
        PathChunk c{ln, query_chunk_shape(ctx, scene, q.pathtrace_type, t, slots, ln, &fp), q.pathtrace_type, q.samples, slots, (uint32_t)recs, iterations,
                    reinterpret_cast<const float4 *>(src), reinterpret_cast<float4 *>(dst_rays), reinterpret_cast<float4 *>(dst)};
        if (!on_device)
        {
            HIP_TRY(hipMemcpyAsync(d_rec.get(), src, (size_t)recs * Rule::FLOATS * 4, hipMemcpyHostToDevice, st));
            c.d_records = d_rec.as<float4>();
            c.d_rays = out_rays ? d_rays.as<float4>() : nullptr;
            c.d_out = d_out.as<float4>();
        }
        hipLaunchKernelGGL(k_set_params, dim3(1), dim3(1), 0, st, fp, ln->d_fp);
        if (int rc = launch(c)) return rc;   // enqueue_wavefront from the chunk's first rays, then the resolve kernel
        if (!on_device)
        {
            HIP_TRY(hipMemcpyAsync(dst, d_out.get(), (size_t)recs * q.result_floats * 4, hipMemcpyDeviceToHost, st));
            if (out_rays) HIP_TRY(hipMemcpyAsync(dst_rays, d_rays.get(), (size_t)slots * LUPIN_RAY_RECORD_FLOATS * 4, hipMemcpyDeviceToHost, st));
        }
    }
    return query_end(ctx, q.who);
}

// The segment queries (occlusion, transmittance: DESIGN.md 18, 21).
static constexpr uint64_t LP_OCCLUSION_MAX_LAUNCH_SLOTS = 1ull << 30;    // slots of one launch: slot indices and the grid's threads fit 32 bits
static constexpr uint64_t LP_OCCLUSION_MAX_STAGED_RECORDS = 1ull << 22;  // host arrays: records of one launch (128 MB of staging)
static constexpr uint32_t LP_TRANSMITTANCE_MAX_SAMPLES = 1u << 20;
static constexpr uint64_t LP_TRANSMITTANCE_MAX_PLANE_SLOTS = 1ull << 24;   // slots of one hemisphere launch: the plane stays within 64 MB

// The chunk loop of the two segment queries: whole records per launch, at most `chunk_records` of them, and four bytes of
// result per record; host arrays go through the context's staging.  launch(records, slots, d_records, d_out) enqueues one
// chunk's kernels on the primary stream.
template <typename Launch>
static int segment_chunks(LupinContext *ctx, const char *who, bool on_device, uint64_t n, uint64_t S, uint64_t chunk_records, const float *records,
                          void *out, Launch launch)
{
    hipStream_t st = ctx->stream;
    for (uint64_t first = 0; first < n; first += chunk_records)
    {
        const uint64_t recs = std::min(chunk_records, n - first);
        const float *src = records + first * LUPIN_OCCLUSION_RECORD_FLOATS;
        void *dst = static_cast<uint32_t *>(out) + first;
        const float4 *d_rec = reinterpret_cast<const float4 *>(src);
        void *d_out = dst;
        if (!on_device)
        {
            HIP_TRY(hipMemcpyAsync(ctx->occ_records.get(), src, (size_t)recs * LUPIN_OCCLUSION_RECORD_FLOATS * 4, hipMemcpyHostToDevice, st));
            d_rec = ctx->occ_records.as<float4>();
            d_out = ctx->occ_counts.get();
        }
        if (int rc = launch((uint32_t)recs, (uint32_t)(recs * S), d_rec, d_out)) return rc;
        if (!on_device) HIP_TRY(hipMemcpyAsync(dst, d_out, (size_t)recs * 4, hipMemcpyDeviceToHost, st));
    }
    return query_end(ctx, who);
}
// ... and its chunk size: `max_slots` slots per launch, and host arrays within the staging, which this grows
static int segment_chunk_records(LupinContext *ctx, bool on_device, uint64_t n, uint64_t S, uint64_t max_slots, uint64_t *chunk_records)
{
    *chunk_records = std::min(n, std::max<uint64_t>(1, max_slots / S));
    if (on_device) return LUPIN_OK;
    *chunk_records = std::min(*chunk_records, LP_OCCLUSION_MAX_STAGED_RECORDS);
    HIP_TRY(grow_buffer(&ctx->occ_records, &ctx->occ_records_bytes, (size_t)*chunk_records * LUPIN_OCCLUSION_RECORD_FLOATS * 4));
    HIP_TRY(grow_buffer(&ctx->occ_counts, &ctx->occ_counts_bytes, (size_t)*chunk_records * 4));
    return LUPIN_OK;
}

// The bent-normal query: lupin_hip_bent_normal_rays and the query inside lupin_hip_bake_lightmap_ao.
static constexpr uint32_t LP_BENT_NORMAL_MAX_SAMPLES = 1u << 20;
static constexpr uint64_t LP_BENT_NORMAL_DEFAULT_SLOTS = 1ull << 30;
static constexpr uint64_t LP_BENT_NORMAL_MAX_LAUNCH_RECORDS = 1ull << 25;   // one wave per record: the grid's threads fit 32 bits
static constexpr uint64_t LP_BENT_NORMAL_MAX_STAGED_RECORDS = 1ull << 22;   // host arrays: records of one launch (128 + 64 MB of staging)
struct BentNormalQuery
{
    const char *who;
    uint32_t samples, max_slots;
    bool opacity, on_device;
    float ray_epsilon;
    bool fixed_tmax;    // every slot's tmax is `tmax`; the records' word [7] is the Rule's
    float tmax;
};
// what both entry points refuse in these fields
static int bent_normal_refuse(uint32_t samples, float ray_epsilon)
{
    if (samples == 0 || samples > LP_BENT_NORMAL_MAX_SAMPLES) return fail(LUPIN_ERR_INVALID_ARGUMENT, "samples must be in [1, 2^20]");
    if (!(std::isfinite(ray_epsilon) && ray_epsilon >= 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "ray_epsilon must be finite and not negative");
    return LUPIN_OK;
}
// From query_start to query_end, once the arguments are accepted and n != 0: whole records per launch, at most
// max_slots / samples of them (at least one), host arrays through the context's staging, four floats of result per record.
template <typename Rule>
static int bent_normal_query(LupinContext *ctx, const LupinScene *scene, const BentNormalQuery &q, uint64_t n, const float *records, float *out)
{
    TraversalLds t;
    if (int rc = query_start<Rule>(ctx, scene, q.on_device, n, records, &t)) return rc;
    const uint64_t S = q.samples, max_slots = q.max_slots ? q.max_slots : LP_BENT_NORMAL_DEFAULT_SLOTS;
    uint64_t chunk = std::min({n, std::max<uint64_t>(1, max_slots / S), LP_BENT_NORMAL_MAX_LAUNCH_RECORDS});
    if (!q.on_device)
    {
        chunk = std::min(chunk, LP_BENT_NORMAL_MAX_STAGED_RECORDS);
        HIP_TRY(grow_buffer(&ctx->occ_records, &ctx->occ_records_bytes, (size_t)chunk * Rule::FLOATS * 4));
        HIP_TRY(grow_buffer(&ctx->bent_results, &ctx->bent_results_bytes, (size_t)chunk * LUPIN_BENT_NORMAL_RESULT_FLOATS * 4));
    }
    hipStream_t st = ctx->stream;
    for (uint64_t first = 0; first < n; first += chunk)
    {
        const uint32_t recs = (uint32_t)std::min(chunk, n - first);
        const float *src = records + first * Rule::FLOATS;
        float *dst = out + first * LUPIN_BENT_NORMAL_RESULT_FLOATS;
        if (!q.on_device) HIP_TRY(hipMemcpyAsync(ctx->occ_records.get(), src, (size_t)recs * Rule::FLOATS * 4, hipMemcpyHostToDevice, st));
        const float4 *d_rec = q.on_device ? reinterpret_cast<const float4 *>(src) : ctx->occ_records.as<float4>();
        float4 *d_out = q.on_device ? reinterpret_cast<float4 *>(dst) : ctx->bent_results.as<float4>();
        const dim3 blocks((recs + LP_BENT_NORMAL_RECORDS_PER_BLOCK - 1) / LP_BENT_NORMAL_RECORDS_PER_BLOCK);
        with_bool(t.geo, [&](auto G) {
            with_bool(q.opacity, [&](auto O) {
                hipLaunchKernelGGL((k_bent_normal<decltype(G)::value, decltype(O)::value>), blocks, dim3(LP_BLOCK), t.lds, st, scene->dev, recs, d_rec,
                                   q.samples, q.ray_epsilon, q.fixed_tmax ? 1u : 0u, q.tmax, d_out, t.stack_words);
            });
        });
        HIP_TRY(hipGetLastError());
        if (!q.on_device) HIP_TRY(hipMemcpyAsync(dst, d_out, (size_t)recs * LUPIN_BENT_NORMAL_RESULT_FLOATS * 4, hipMemcpyDeviceToHost, st));
    }
    return query_end(ctx, q.who);
}

// The irradiance volume's two lookups (by segments, by depth maps: DESIGN.md 23, 25).
static constexpr uint64_t LP_PROBE_GRID_MAX_LAUNCH = 1ull << 27;          // records of one launch: eight lanes each, and the lane index fits 32 bits
static constexpr uint64_t LP_PROBE_GRID_MAX_STAGED_RECORDS = 1ull << 20;  // host arrays: records of one launch (32 + 16 MB of staging)
static constexpr uint64_t LP_PROBE_GRID_MAX_PROBES = 1ull << 31;

// What both refuse in a grid, in this order (both look at ray_epsilon, whether they trace or not); *probes: the grid's.
static int probe_grid_refuse(const LupinProbeGridDesc &d, uint32_t known_flags, const char *unknown_flag_msg, uint64_t *probes)
{
    if (d.flags & ~known_flags) return fail(LUPIN_ERR_INVALID_ARGUMENT, unknown_flag_msg);
    for (int k = 0; k < 3; k++)
    {
        if (!std::isfinite(d.origin[k])) return fail(LUPIN_ERR_INVALID_ARGUMENT, "origin must be finite");
        if (!(std::isfinite(d.spacing[k]) && d.spacing[k] > 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "spacing must be finite and positive");
        if (d.dims[k] == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "a dimension is zero");
    }
    const uint64_t slice = (uint64_t)d.dims[0] * d.dims[1];   // below 2^64: both factors are below 2^32
    if (slice > LP_PROBE_GRID_MAX_PROBES || d.dims[2] > LP_PROBE_GRID_MAX_PROBES / slice)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "the grid must not exceed 2^31 probes");
    for (int k = 0; k < 3; k++)   // the last probe, by the kernel's own expression: every probe of the axis lies between the first and this one
        if (!std::isfinite(d.origin[k] + (float)(d.dims[k] - 1u) * d.spacing[k]))
            return fail(LUPIN_ERR_INVALID_ARGUMENT, "the grid's last probe position is not finite");
    if (!(std::isfinite(d.ray_epsilon) && d.ray_epsilon >= 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "ray_epsilon must be finite and not negative");
    if (!(std::isfinite(d.normal_bias) && d.normal_bias >= 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "normal_bias must be finite and not negative");
    *probes = slice * d.dims[2];
    return LUPIN_OK;
}
static ProbeGridDev probe_grid_dev(const LupinProbeGridDesc &d)
{
    return ProbeGridDev{d.origin[0], d.origin[1], d.origin[2], d.spacing[0], d.spacing[1], d.spacing[2],
                        d.dims[0],   d.dims[1],   d.dims[2],   d.flags,      d.ray_epsilon, d.normal_bias};
}
// records of one launch (host arrays: of one staging), and the launch's blocks
static uint64_t probe_grid_chunk_records(bool on_device, uint64_t n) { return std::min(n, on_device ? LP_PROBE_GRID_MAX_LAUNCH : LP_PROBE_GRID_MAX_STAGED_RECORDS); }
static dim3 probe_grid_blocks(uint32_t records) { return dim3((records + LP_PROBE_GRID_RECORDS_PER_BLOCK - 1) / LP_PROBE_GRID_RECORDS_PER_BLOCK); }
// The chunk loop of the two: at most `chunk` records per launch, host arrays through `stage_records` / `stage_results`
// (the entry point's, for `chunk` records: nothing is allocated here).  launch(records, d_records, d_results) enqueues one
// chunk's kernel on the primary stream; its launch error is looked at here.
template <typename Launch>
static int probe_grid_chunks(LupinContext *ctx, const char *who, bool on_device, uint64_t n, uint64_t chunk, const float *records, float *out,
                             void *stage_records, void *stage_results, Launch launch)
{
    hipStream_t st = ctx->stream;
    for (uint64_t first = 0; first < n; first += chunk)
    {
        const uint32_t recs = (uint32_t)std::min(chunk, n - first);
        const float *src = records + first * LUPIN_PROBE_GRID_RECORD_FLOATS;
        float *dst = out + first * LUPIN_PROBE_GRID_RESULT_FLOATS;
        if (!on_device) HIP_TRY(hipMemcpyAsync(stage_records, src, (size_t)recs * LUPIN_PROBE_GRID_RECORD_FLOATS * 4, hipMemcpyHostToDevice, st));
        float4 *d_res = static_cast<float4 *>(on_device ? (void *)dst : stage_results);
        launch(recs, static_cast<const float4 *>(on_device ? (const void *)src : stage_records), d_res);
        HIP_TRY(hipGetLastError());
        if (!on_device) HIP_TRY(hipMemcpyAsync(dst, d_res, (size_t)recs * LUPIN_PROBE_GRID_RESULT_FLOATS * 4, hipMemcpyDeviceToHost, st));
    }
    return query_end(ctx, who);
}

}   // extern "C++"

// ---- radiance queries and light-probe baking (no reference counterpart; kernels: lupin_rays.hpp, lupin_probes.hpp) ----

int lupin_hip_pathtrace_rays(LupinContext *ctx, const LupinScene *scene, const LupinRayQueryDesc *desc, uint64_t n, const float *records,
                             float *out, float *out_rays)
{
    if (int rc = query_refuse(ctx, scene, desc && records && out)) return rc;
    const PathQuery q = {"lupin_hip_pathtrace_rays", desc->pathtrace_type, desc->flags, desc->samples, desc->max_bounces, desc->max_slots, &desc->advanced,
                         LUPIN_RAY_RESULT_FLOATS};
    return path_query<RayRecordRule>(ctx, scene, q, n, records, out, out_rays, [ctx, scene](const PathChunk &c) -> int {
        const RayBegin rb{c.d_records, c.samples, c.d_rays};
        HIP_TRY(enqueue_wavefront(ctx, c.ln, scene, c.pathtrace_type, c.slots, c.sh, c.iterations, nullptr, &rb));
        hipLaunchKernelGGL(k_resolve_rays, dim3((c.records + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, c.ln->stream, c.ln->pb, c.records, c.samples, c.d_out);
        HIP_TRY(hipGetLastError());
        return LUPIN_OK;
    });
}

// lupin_hip_pathtrace_rays with k_resolve_moments (lupin_lightmap_adaptive.hpp) as its resolve: the launch of a
// chunk, shared with the rounds of lupin_hip_bake_lightmap_adaptive
static int launch_moments_chunk(LupinContext *ctx, const LupinScene *scene, const PathChunk &c)
{
    const RayBegin rb{c.d_records, c.samples, c.d_rays};
    HIP_TRY(enqueue_wavefront(ctx, c.ln, scene, c.pathtrace_type, c.slots, c.sh, c.iterations, nullptr, &rb));
    hipLaunchKernelGGL(k_resolve_moments, dim3((c.records + LP_LM_AD_RECORDS_PER_BLOCK - 1) / LP_LM_AD_RECORDS_PER_BLOCK), dim3(LP_BLOCK), 0, c.ln->stream,
                       c.ln->pb, c.records, c.samples, c.d_out);
    HIP_TRY(hipGetLastError());
    return LUPIN_OK;
}

int lupin_hip_pathtrace_rays_moments(LupinContext *ctx, const LupinScene *scene, const LupinRayQueryDesc *desc, uint64_t n, const float *records,
                                     float *out)
{
    if (int rc = query_refuse(ctx, scene, desc && records && out)) return rc;
    const PathQuery q = {"lupin_hip_pathtrace_rays_moments", desc->pathtrace_type, desc->flags, desc->samples, desc->max_bounces, desc->max_slots,
                         &desc->advanced, LUPIN_RAY_MOMENTS_FLOATS};
    return path_query<RayRecordRule>(ctx, scene, q, n, records, out, nullptr,
                                     [ctx, scene](const PathChunk &c) -> int { return launch_moments_chunk(ctx, scene, c); });
}

int lupin_hip_bake_probes(LupinContext *ctx, const LupinScene *scene, const LupinProbeDesc *desc, uint64_t n, const float *probes, float *out_sh,
                          float *out_rays)
{
    if (int rc = query_refuse(ctx, scene, desc && probes && out_sh)) return rc;
    const PathQuery q = {"lupin_hip_bake_probes", desc->pathtrace_type, desc->flags, desc->samples, desc->max_bounces, desc->max_slots, &desc->advanced,
                         LUPIN_PROBE_RESULT_FLOATS};
    return path_query<ProbeRule>(ctx, scene, q, n, probes, out_sh, out_rays, [ctx, scene](const PathChunk &c) -> int {
        const ProbeBegin pbg{c.d_records, c.samples, c.d_rays};
        HIP_TRY(enqueue_wavefront(ctx, c.ln, scene, c.pathtrace_type, c.slots, c.sh, c.iterations, nullptr, nullptr, &pbg));
        hipLaunchKernelGGL(k_resolve_probes, dim3((c.records + LP_PROBES_PER_BLOCK - 1) / LP_PROBES_PER_BLOCK), dim3(LP_BLOCK), 0, c.ln->stream, c.ln->pb,
                           c.records, c.d_records, c.samples, c.d_out);
        HIP_TRY(hipGetLastError());
        return LUPIN_OK;
    });
}

// ---- occlusion and transmittance queries (no reference counterpart; kernels: lupin_occlusion.hpp, lupin_transmittance.hpp) ----

int lupin_hip_occlusion_rays(LupinContext *ctx, const LupinScene *scene, const LupinOcclusionDesc *desc, uint64_t n, const float *records,
                             uint32_t *out_blocked)
{
    if (int rc = query_refuse(ctx, scene, desc && records && out_blocked)) return rc;
    if (desc->mode > LUPIN_OCCLUSION_COSINE_HEMISPHERE) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown mode");
    if (desc->flags & ~(uint32_t)LUPIN_OCCLUSION_DEVICE_POINTERS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown flag");
    if (desc->samples == 0 || desc->samples > LP_RAYS_MAX_CHUNK_SLOTS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "samples must be in [1, 2^27]");
    if (desc->mode == LUPIN_OCCLUSION_DIRECTION && desc->samples != 1) return fail(LUPIN_ERR_INVALID_ARGUMENT, "direction mode takes samples == 1");
    const uint64_t S = desc->samples;
    if (n > LP_RAYS_MAX_PATHS / S) return fail(LUPIN_ERR_INVALID_ARGUMENT, "n * samples must not exceed 2^38");
    if (!(std::isfinite(desc->ray_epsilon) && desc->ray_epsilon >= 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "ray_epsilon must be finite and not negative");
    if (int rc = query_refuse_hierarchy(ctx, scene, false)) return rc;
    const bool on_device = (desc->flags & LUPIN_OCCLUSION_DEVICE_POINTERS) != 0;
    if (on_device && (((uintptr_t)records & 15u) || ((uintptr_t)out_blocked & 3u)))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "device records must be 16-byte aligned, device counts 4-byte aligned");
    if (n == 0) return LUPIN_OK;
    TraversalLds t;
    if (int rc = query_start<OcclusionRecordRule>(ctx, scene, on_device, n, records, &t)) return rc;

    uint64_t chunk_records;
    if (int rc = segment_chunk_records(ctx, on_device, n, S, LP_OCCLUSION_MAX_LAUNCH_SLOTS, &chunk_records)) return rc;
    return segment_chunks(ctx, "lupin_hip_occlusion_rays", on_device, n, S, chunk_records, records, out_blocked,
                          [&](uint32_t recs, uint32_t slots, const float4 *d_rec, void *d_out) -> int {
        HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)recs * 4, ctx->stream));
        with_bool(t.geo, [&](auto G) {
            hipLaunchKernelGGL(k_occlusion<decltype(G)::value>, dim3((slots + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), t.lds, ctx->stream, scene->dev, slots,
                               d_rec, desc->samples, desc->mode, desc->ray_epsilon, static_cast<uint32_t *>(d_out), t.stack_words);
        });
        HIP_TRY(hipGetLastError());
        return LUPIN_OK;
    });
}

int lupin_hip_transmittance_rays(LupinContext *ctx, const LupinScene *scene, const LupinOcclusionDesc *desc, uint64_t n, const float *records,
                                 float *out_sum)
{
    if (int rc = query_refuse(ctx, scene, desc && records && out_sum)) return rc;
    if (desc->mode > LUPIN_OCCLUSION_COSINE_HEMISPHERE) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown mode");
    if (desc->flags & ~(uint32_t)LUPIN_OCCLUSION_DEVICE_POINTERS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown flag");
    if (desc->samples == 0 || desc->samples > LP_TRANSMITTANCE_MAX_SAMPLES) return fail(LUPIN_ERR_INVALID_ARGUMENT, "samples must be in [1, 2^20]");
    if (desc->mode == LUPIN_OCCLUSION_DIRECTION && desc->samples != 1) return fail(LUPIN_ERR_INVALID_ARGUMENT, "direction mode takes samples == 1");
    const uint64_t S = desc->samples;
    if (n > LP_RAYS_MAX_PATHS / S) return fail(LUPIN_ERR_INVALID_ARGUMENT, "n * samples must not exceed 2^38");
    if (!(std::isfinite(desc->ray_epsilon) && desc->ray_epsilon >= 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "ray_epsilon must be finite and not negative");
    if (int rc = query_refuse_hierarchy(ctx, scene, false)) return rc;
    const bool on_device = (desc->flags & LUPIN_OCCLUSION_DEVICE_POINTERS) != 0;
    if (on_device && (((uintptr_t)records & 15u) || ((uintptr_t)out_sum & 3u)))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "device records must be 16-byte aligned, device results 4-byte aligned");
    if (n == 0) return LUPIN_OK;
    TraversalLds t;
    if (int rc = query_start<OcclusionRecordRule>(ctx, scene, on_device, n, records, &t)) return rc;

    // with more than one slot per record the slots go through the plane, which bounds the chunk
    const bool planed = S > 1;
    uint64_t chunk_records;
    if (int rc = segment_chunk_records(ctx, on_device, n, S, planed ? LP_TRANSMITTANCE_MAX_PLANE_SLOTS : LP_OCCLUSION_MAX_LAUNCH_SLOTS, &chunk_records)) return rc;
    if (planed) HIP_TRY(grow_buffer(&ctx->trans_plane, &ctx->trans_plane_bytes, (size_t)(chunk_records * S) * 4));
    return segment_chunks(ctx, "lupin_hip_transmittance_rays", on_device, n, S, chunk_records, records, out_sum,
                          [&](uint32_t recs, uint32_t slots, const float4 *d_rec, void *d_out) -> int {
        float *d_sum = static_cast<float *>(d_out), *d_slots = planed ? ctx->trans_plane.as<float>() : d_sum;
        with_bool(t.geo, [&](auto G) {
            hipLaunchKernelGGL(k_transmittance<decltype(G)::value>, dim3((slots + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), t.lds, ctx->stream, scene->dev,
                               slots, d_rec, desc->samples, desc->mode, desc->ray_epsilon, d_slots, t.stack_words);
        });
        HIP_TRY(hipGetLastError());
        if (planed)
        {
            hipLaunchKernelGGL(k_transmittance_resolve, dim3((recs + LP_TRANSMITTANCE_RECORDS_PER_BLOCK - 1) / LP_TRANSMITTANCE_RECORDS_PER_BLOCK), dim3(LP_BLOCK), 0,
                               ctx->stream, d_slots, recs, desc->samples, d_sum);
            HIP_TRY(hipGetLastError());
        }
        return LUPIN_OK;
    });
}

// ---- bent-normal queries (no reference counterpart; kernels: lupin_bent_normal.hpp) ----

int lupin_hip_bent_normal_rays(LupinContext *ctx, const LupinScene *scene, const LupinBentNormalDesc *desc, uint64_t n, const float *records, float *out)
{
    if (int rc = query_refuse(ctx, scene, desc && records && out)) return rc;
    if (desc->flags & ~(uint32_t)(LUPIN_BENT_NORMAL_DEVICE_POINTERS | LUPIN_BENT_NORMAL_OPACITY)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown flag");
    if (int rc = bent_normal_refuse(desc->samples, desc->ray_epsilon)) return rc;
    if (n > LP_RAYS_MAX_PATHS / desc->samples) return fail(LUPIN_ERR_INVALID_ARGUMENT, "n * samples must not exceed 2^38");
    if (int rc = query_refuse_hierarchy(ctx, scene, false)) return rc;
    const bool on_device = (desc->flags & LUPIN_BENT_NORMAL_DEVICE_POINTERS) != 0;
    if (on_device && (((uintptr_t)records & 15u) || ((uintptr_t)out & 15u)))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "device records and device results must be 16-byte aligned");
    if (n == 0) return LUPIN_OK;
    const BentNormalQuery q = {"lupin_hip_bent_normal_rays", desc->samples, desc->max_slots, (desc->flags & LUPIN_BENT_NORMAL_OPACITY) != 0, on_device,
                               desc->ray_epsilon, false, 0.0f};
    return bent_normal_query<OcclusionRecordRule>(ctx, scene, q, n, records, out);
}

// ---- distance queries (no reference counterpart; kernels: lupin_distance.hpp) ----

static constexpr uint64_t LP_DISTANCE_MAX_LAUNCH = 1ull << 30;          // records / voxels of one launch: indices fit 32 bits
static constexpr uint64_t LP_DISTANCE_MAX_STAGED_RECORDS = 1ull << 20;  // host arrays: records of one launch (16 + 48 MB of staging)
static constexpr uint64_t LP_DISTANCE_MAX_STAGED_VOXELS = 1ull << 24;   // host volume: voxels of one launch (64 MB of staging)
static constexpr uint64_t LP_DISTANCE_MAX_VOXELS = 1ull << 36;

// c_i of DESIGN.md 20: a float not above 1 / sigma_max of the world -> local rows' 3x3 part, so that c_i * (a distance in the
// instance's local space) is a lower bound of the world distance.  sigma_max^2 is the largest eigenvalue of R^T R, by the
// closed form for a symmetric 3x3 matrix in float64; the quotient is shrunk by 1e-9 (far above the closed form's error) and
// rounded toward zero.  0 for a zero or non-finite sigma: nothing of that instance is pruned by distance.
static float distance_scale(const InstanceDev &in)
{
    const double r[3][3] = {{in.r0.x, in.r0.y, in.r0.z}, {in.r1.x, in.r1.y, in.r1.z}, {in.r2.x, in.r2.y, in.r2.z}};
    double a[3][3];
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) a[i][j] = r[0][i] * r[0][j] + r[1][i] * r[1][j] + r[2][i] * r[2][j];
    const double p1 = a[0][1] * a[0][1] + a[0][2] * a[0][2] + a[1][2] * a[1][2];
    const double q = (a[0][0] + a[1][1] + a[2][2]) / 3.0;
    const double p2 = (a[0][0] - q) * (a[0][0] - q) + (a[1][1] - q) * (a[1][1] - q) + (a[2][2] - q) * (a[2][2] - q) + 2.0 * p1;
    const double p = std::sqrt(p2 / 6.0);
    double lam = q;
    if (p > 0.0)
    {
        double b[3][3];
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) b[i][j] = (a[i][j] - (i == j ? q : 0.0)) / p;
        const double det = b[0][0] * (b[1][1] * b[2][2] - b[1][2] * b[2][1]) - b[0][1] * (b[1][0] * b[2][2] - b[1][2] * b[2][0]) +
                           b[0][2] * (b[1][0] * b[2][1] - b[1][1] * b[2][0]);
        const double h = std::min(1.0, std::max(-1.0, det / 2.0));
        lam = q + 2.0 * p * std::cos(std::acos(h) / 3.0);
    }
    const double sigma = std::sqrt(lam);
    if (!(std::isfinite(sigma) && sigma > 0.0)) return 0.0f;
    const double c = (1.0 / sigma) * (1.0 - 1e-9);
    float f = (float)c;
    if ((double)f > c) f = std::nextafterf(f, 0.0f);
    return std::isfinite(f) ? f : 0.0f;
}

// What both entry points share once their own arguments are accepted: the query's start with a stack sized for (reference,
// key) pairs, then the auxiliary array is built from the scene's current rows and copied.
static int distance_begin(LupinContext *ctx, const LupinScene *scene, TraversalLds *t)
{
    if (int rc = query_flush(ctx)) return rc;
    if (int rc = query_plan(ctx, scene, 2u * scene->stack_entries, t)) return rc;
    const uint32_t ninst = scene->dev.num_instances;
    std::vector<float4> aux((size_t)std::max(1u, ninst) * LP_DISTANCE_AUX_WORDS, make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    for (uint32_t i = 0; i < ninst; i++)
    {
        const InstanceDev &in = scene->host_instances[i];
        const float4 rr[3] = {in.r0, in.r1, in.r2};
        LupinMat3x4 w2l, l2w;
        for (int r = 0; r < 3; r++) { w2l.m[0][r] = rr[r].x; w2l.m[1][r] = rr[r].y; w2l.m[2][r] = rr[r].z; w2l.m[3][r] = rr[r].w; }
        lupin_mat3x4_inverse(&w2l, &l2w);   // the TLAS builder's own local -> world: the same floats
        bool finite = true;
        for (int r = 0; r < 3; r++)
        {
            aux[(size_t)i * LP_DISTANCE_AUX_WORDS + r] = make_float4(l2w.m[0][r], l2w.m[1][r], l2w.m[2][r], l2w.m[3][r]);
            for (int c = 0; c < 4; c++) finite = finite && std::isfinite(l2w.m[c][r]);
        }
        aux[(size_t)i * LP_DISTANCE_AUX_WORDS + 3] = make_float4(finite ? distance_scale(in) : -1.0f, 0.0f, 0.0f, 0.0f);
    }
    // every call ends synchronised, so the buffer of the call before is free; the copy is from pageable memory and has left
    // the vector when hipMemcpyAsync returns
    HIP_TRY(grow_buffer(&ctx->dist_aux, &ctx->dist_aux_bytes, aux.size() * sizeof(float4)));
    HIP_TRY(hipMemcpyAsync(ctx->dist_aux.get(), aux.data(), aux.size() * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    return LUPIN_OK;
}

int lupin_hip_distance_points(LupinContext *ctx, const LupinScene *scene, uint32_t flags, uint64_t n, const float *records, float *out_results)
{
    if (int rc = query_refuse(ctx, scene, records && out_results)) return rc;
    if (flags & ~(uint32_t)LUPIN_DISTANCE_DEVICE_POINTERS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown flag");
    if (n > LP_RAYS_MAX_PATHS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "n must not exceed 2^38");
    if (int rc = query_refuse_hierarchy(ctx, scene, false)) return rc;
    const bool on_device = (flags & LUPIN_DISTANCE_DEVICE_POINTERS) != 0;
    if (on_device && (((uintptr_t)records & 15u) || ((uintptr_t)out_results & 15u)))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "device records and results must be 16-byte aligned");
    if (n == 0) return LUPIN_OK;
    // (host records are looked at before the recorded calls run: query_start's pieces, in this entry point's own order)
    if (!on_device)
        if (int rc = refuse_bad_host_records<DistanceRecordRule>(n, records)) return rc;
    TraversalLds t;
    if (int rc = distance_begin(ctx, scene, &t)) return rc;
    if (on_device)
        if (int rc = refuse_bad_device_records<DistanceRecordRule>(ctx, n, records)) return rc;
    hipStream_t st = ctx->stream;

    uint64_t chunk = std::min(n, LP_DISTANCE_MAX_LAUNCH);
    if (!on_device)
    {
        chunk = std::min(chunk, LP_DISTANCE_MAX_STAGED_RECORDS);
        HIP_TRY(grow_buffer(&ctx->dist_records, &ctx->dist_records_bytes, (size_t)chunk * LUPIN_DISTANCE_RECORD_FLOATS * 4));
        HIP_TRY(grow_buffer(&ctx->dist_results, &ctx->dist_results_bytes, (size_t)chunk * LUPIN_DISTANCE_RESULT_FLOATS * 4));
    }
    for (uint64_t first = 0; first < n; first += chunk)
    {
        const uint32_t recs = (uint32_t)std::min(chunk, n - first);
        const float *src = records + first * LUPIN_DISTANCE_RECORD_FLOATS;
        float *dst = out_results + first * LUPIN_DISTANCE_RESULT_FLOATS;
        const float4 *d_rec = reinterpret_cast<const float4 *>(src);
        float4 *d_res = reinterpret_cast<float4 *>(dst);
        if (!on_device)
        {
            HIP_TRY(hipMemcpyAsync(ctx->dist_records.get(), src, (size_t)recs * LUPIN_DISTANCE_RECORD_FLOATS * 4, hipMemcpyHostToDevice, st));
            d_rec = ctx->dist_records.as<float4>();
            d_res = ctx->dist_results.as<float4>();
        }
        with_bool(t.geo, [&](auto G) {
            hipLaunchKernelGGL(k_distance<decltype(G)::value>, dim3((recs + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), t.lds, st, scene->dev, recs, d_rec,
                               ctx->dist_aux.as<float4>(), d_res, t.stack_words);
        });
        HIP_TRY(hipGetLastError());
        if (!on_device) HIP_TRY(hipMemcpyAsync(dst, d_res, (size_t)recs * LUPIN_DISTANCE_RESULT_FLOATS * 4, hipMemcpyDeviceToHost, st));
    }
    return query_end(ctx, "lupin_hip_distance_points");
}

int lupin_hip_bake_distance_grid(LupinContext *ctx, const LupinScene *scene, uint32_t flags, const float *origin, const float *spacing,
                                 const uint32_t *dims, float rmax, float *out_volume)
{
    if (int rc = query_refuse(ctx, scene, origin && spacing && dims && out_volume)) return rc;
    if (flags & ~(uint32_t)(LUPIN_DISTANCE_DEVICE_POINTERS | LUPIN_DISTANCE_GRID_SIGNED)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown flag");
    for (int k = 0; k < 3; k++)
    {
        if (!std::isfinite(origin[k])) return fail(LUPIN_ERR_INVALID_ARGUMENT, "origin must be finite");
        if (!(std::isfinite(spacing[k]) && spacing[k] > 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "spacing must be finite and positive");
        if (dims[k] == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "a dimension is zero");
        // the last centre, by the kernel's own expression: every centre of the axis lies between the first and this one
        if (!std::isfinite(origin[k] + ((float)(dims[k] - 1u) + 0.5f) * spacing[k])) return fail(LUPIN_ERR_INVALID_ARGUMENT, "the grid's far corner is not finite");
    }
    if (!(rmax > 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "rmax must be positive (+inf: unbounded)");
    const uint64_t slice = (uint64_t)dims[0] * dims[1];   // below 2^64: both factors are below 2^32
    if (slice > LP_DISTANCE_MAX_VOXELS || dims[2] > LP_DISTANCE_MAX_VOXELS / slice)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "the grid must not exceed 2^36 voxels");
    if (int rc = query_refuse_hierarchy(ctx, scene, false)) return rc;
    const bool on_device = (flags & LUPIN_DISTANCE_DEVICE_POINTERS) != 0;
    if (on_device && ((uintptr_t)out_volume & 3u)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "a device volume must be 4-byte aligned");
    const uint64_t n = (uint64_t)dims[0] * dims[1] * dims[2];
    TraversalLds t;
    if (int rc = distance_begin(ctx, scene, &t)) return rc;
    hipStream_t st = ctx->stream;
    DistanceGrid g;
    g.ox = origin[0]; g.oy = origin[1]; g.oz = origin[2];
    g.sx = spacing[0]; g.sy = spacing[1]; g.sz = spacing[2];
    g.nx = dims[0]; g.ny = dims[1];
    g.rmax = std::min(rmax, LP_F32_MAX);
    g.flags = flags;
    uint64_t chunk = std::min(n, LP_DISTANCE_MAX_LAUNCH);
    if (!on_device)
    {
        chunk = std::min(chunk, LP_DISTANCE_MAX_STAGED_VOXELS);
        HIP_TRY(grow_buffer(&ctx->dist_results, &ctx->dist_results_bytes, (size_t)chunk * 4));
    }
    for (uint64_t first = 0; first < n; first += chunk)
    {
        const uint32_t voxels = (uint32_t)std::min(chunk, n - first);
        float *dst = out_volume + first;
        float *d_out = on_device ? dst : ctx->dist_results.as<float>();
        with_bool(t.geo, [&](auto G) {
            hipLaunchKernelGGL(k_distance_grid<decltype(G)::value>, dim3((voxels + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), t.lds, st, scene->dev,
                               (unsigned long long)first, voxels, g, ctx->dist_aux.as<float4>(), d_out, t.stack_words);
        });
        HIP_TRY(hipGetLastError());
        if (!on_device) HIP_TRY(hipMemcpyAsync(dst, d_out, (size_t)voxels * 4, hipMemcpyDeviceToHost, st));
    }
    return query_end(ctx, "lupin_hip_bake_distance_grid");
}

// ---- irradiance volume lookup (no reference counterpart; kernel: lupin_probe_grid.hpp) ----

int lupin_hip_sample_probe_grid(LupinContext *ctx, const LupinScene *scene, const LupinProbeGridDesc *desc, const float *sh, const uint8_t *valid,
                                uint64_t n, const float *records, float *out)
{
    if (int rc = query_refuse(ctx, scene, desc && sh && records && out)) return rc;
    uint64_t probes;
    if (int rc = probe_grid_refuse(*desc, LUPIN_PROBE_GRID_DEVICE_POINTERS | LUPIN_PROBE_GRID_VISIBILITY | LUPIN_PROBE_GRID_BACKFACE, "unknown flag", &probes))
        return rc;
    if (n > LP_RAYS_MAX_PATHS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "n must not exceed 2^38");
    const bool vis = (desc->flags & LUPIN_PROBE_GRID_VISIBILITY) != 0;
    if (vis)
        if (int rc = query_refuse_hierarchy(ctx, scene, false)) return rc;
    const bool on_device = (desc->flags & LUPIN_PROBE_GRID_DEVICE_POINTERS) != 0;
    if (on_device && (((uintptr_t)sh | (uintptr_t)records | (uintptr_t)out) & 15u))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "device coefficients, records and results must be 16-byte aligned");
    if (n == 0) return LUPIN_OK;
    TraversalLds t;   // this query's own stack: none at all without visibility, where the scene is not read
    if (int rc = query_start<ProbeGridRecordRule>(ctx, scene, on_device, n, records, vis ? scene->stack_entries : 0u, vis, &t)) return rc;
    hipStream_t st = ctx->stream;

    const ProbeGridDev g = probe_grid_dev(*desc);
    const uint64_t chunk = probe_grid_chunk_records(on_device, n);
    const float4 *d_sh = reinterpret_cast<const float4 *>(sh);
    const uint8_t *d_valid = valid;
    if (!on_device)   // host arrays: the grid whole, one chunk's records and results, in the context's staging
    {
        const size_t sh_bytes = (size_t)probes * LUPIN_PROBE_RESULT_FLOATS * 4;
        HIP_TRY(grow_buffer(&ctx->grid_sh, &ctx->grid_sh_bytes, sh_bytes));
        HIP_TRY(grow_buffer(&ctx->grid_records, &ctx->grid_records_bytes, (size_t)chunk * LUPIN_PROBE_GRID_RECORD_FLOATS * 4));
        HIP_TRY(grow_buffer(&ctx->grid_results, &ctx->grid_results_bytes, (size_t)chunk * LUPIN_PROBE_GRID_RESULT_FLOATS * 4));
        HIP_TRY(hipMemcpyAsync(ctx->grid_sh.get(), sh, sh_bytes, hipMemcpyHostToDevice, st));
        d_sh = ctx->grid_sh.as<float4>();
        if (valid)
        {
            HIP_TRY(grow_buffer(&ctx->grid_valid, &ctx->grid_valid_bytes, (size_t)probes));
            HIP_TRY(hipMemcpyAsync(ctx->grid_valid.get(), valid, (size_t)probes, hipMemcpyHostToDevice, st));
            d_valid = ctx->grid_valid.as<uint8_t>();
        }
    }
    auto launch = [&](uint32_t recs, const float4 *d_rec, float4 *d_res) {
        with_bool(t.geo, [&](auto G) {
            with_bool(vis, [&](auto V) {
                hipLaunchKernelGGL((k_probe_grid<decltype(G)::value, decltype(V)::value>), probe_grid_blocks(recs), dim3(LP_BLOCK), t.lds, st, scene->dev,
                                   recs, g, d_sh, d_valid, d_rec, d_res, t.stack_words);
            });
        });
    };
    return probe_grid_chunks(ctx, "lupin_hip_sample_probe_grid", on_device, n, chunk, records, out, ctx->grid_records.get(), ctx->grid_results.get(), launch);
}

// ---- probe depth maps (no reference counterpart; kernels: lupin_probe_depth.hpp) ----

static constexpr uint64_t LP_PROBE_DEPTH_DEFAULT_SLOTS = LUPIN_PROBE_DEPTH_DEFAULT_MAX_SLOTS;
static constexpr uint64_t LP_PROBE_DEPTH_MAX_LAUNCH_SLOTS = 1ull << 30;    // slots of one launch: the lane index and the grid's threads fit 32 bits
static constexpr uint64_t LP_PROBE_DEPTH_MAX_STAGED_PROBES = 1ull << 10;   // host arrays: probes of one batch (at most 34 MB of maps)

static bool probe_depth_resolution_ok(uint32_t R) { return R >= LUPIN_PROBE_DEPTH_MIN_RESOLUTION && R <= LUPIN_PROBE_DEPTH_MAX_RESOLUTION; }

int lupin_hip_bake_probe_depth(LupinContext *ctx, const LupinScene *scene, const LupinProbeDepthDesc *desc, uint64_t n, const float *positions,
                               float *out_depth, uint32_t *out_stats)
{
    if (int rc = query_refuse(ctx, scene, desc && positions && out_depth)) return rc;
    if (desc->flags & ~(uint32_t)LUPIN_PROBE_DEPTH_DEVICE_POINTERS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown flag");
    const uint32_t R = desc->resolution, K = desc->subsamples;
    if (!probe_depth_resolution_ok(R)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "resolution must be in [2, 64]");
    if (K != 1 && K != 2 && K != 4 && K != 8) return fail(LUPIN_ERR_INVALID_ARGUMENT, "subsamples must be 1, 2, 4 or 8");
    if (!(std::isfinite(desc->ray_epsilon) && desc->ray_epsilon >= 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "ray_epsilon must be finite and not negative");
    if (!(std::isfinite(desc->max_distance) && desc->max_distance > 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "max_distance must be finite and positive");
    const uint64_t rays = (uint64_t)R * R * K * K;   // per probe: at most 2^18
    if (n > LP_RAYS_MAX_PATHS / rays) return fail(LUPIN_ERR_INVALID_ARGUMENT, "n * resolution^2 * subsamples^2 must not exceed 2^38");
    if (int rc = query_refuse_hierarchy(ctx, scene, false)) return rc;
    const bool on_device = (desc->flags & LUPIN_PROBE_DEPTH_DEVICE_POINTERS) != 0;
    if (on_device && (((uintptr_t)positions & 15u) || ((uintptr_t)out_depth & 7u) || ((uintptr_t)out_stats & 15u)))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "device positions and stats must be 16-byte aligned, device maps 8-byte aligned");
    if (n == 0) return LUPIN_OK;
    TraversalLds t;
    if (int rc = query_start<ProbeDepthPositionRule>(ctx, scene, on_device, n, positions, &t)) return rc;
    hipStream_t st = ctx->stream;

    const uint64_t asked = desc->max_slots ? (uint64_t)desc->max_slots : LP_PROBE_DEPTH_DEFAULT_SLOTS;
    const uint64_t max_slots = std::min(std::max<uint64_t>(asked / 64u * 64u, 64u), LP_PROBE_DEPTH_MAX_LAUNCH_SLOTS);
    const size_t map_floats = (size_t)(R + 2u) * (R + 2u) * 2u;
    // host arrays: a batch of probes at a time through device buffers that live for the call; device arrays: one batch
    const uint64_t batch = on_device ? n : std::min(n, LP_PROBE_DEPTH_MAX_STAGED_PROBES);
    DeviceBuffer b_pos, b_depth, b_stats;
    if (!on_device)
    {
        HIP_TRY(DeviceBuffer::make((size_t)batch * 16, &b_pos));
        HIP_TRY(DeviceBuffer::make((size_t)batch * map_floats * 4, &b_depth));
        if (out_stats) HIP_TRY(DeviceBuffer::make((size_t)batch * LUPIN_PROBE_DEPTH_STATS_WORDS * 4, &b_stats));
    }
    for (uint64_t p0 = 0; p0 < n; p0 += batch)
    {
        const uint64_t probes = std::min(batch, n - p0);
        const float *src = positions + p0 * 4;
        float *dst = out_depth + p0 * map_floats;
        uint32_t *dst_stats = out_stats ? out_stats + p0 * LUPIN_PROBE_DEPTH_STATS_WORDS : nullptr;
        const float4 *d_pos = reinterpret_cast<const float4 *>(src);
        float2 *d_depth = reinterpret_cast<float2 *>(dst);
        uint32_t *d_stats = dst_stats;
        if (!on_device)
        {
            HIP_TRY(hipMemcpyAsync(b_pos.get(), src, (size_t)probes * 16, hipMemcpyHostToDevice, st));
            d_pos = b_pos.as<float4>();
            d_depth = b_depth.as<float2>();
            d_stats = out_stats ? b_stats.as<uint32_t>() : nullptr;
        }
        if (d_stats)
            hipLaunchKernelGGL(k_probe_depth_stats_init, dim3((uint32_t)((probes + LP_BLOCK - 1) / LP_BLOCK)), dim3(LP_BLOCK), 0, st, (uint32_t)probes,
                               (uint32_t)rays, reinterpret_cast<uint4 *>(d_stats));
        const uint64_t total = probes * rays;
        for (uint64_t first = 0; first < total; first += max_slots)
        {
            const uint32_t slots = (uint32_t)std::min(max_slots, total - first);
            with_bool(t.geo, [&](auto G) {
                with_bool(d_stats != nullptr, [&](auto S) {
                    hipLaunchKernelGGL((k_probe_depth<decltype(G)::value, decltype(S)::value>), dim3((slots + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), t.lds,
                                       st, scene->dev, (unsigned long long)first, slots, R, K, desc->ray_epsilon, desc->max_distance, d_pos, d_depth, d_stats,
                                       t.stack_words);
                });
            });
            HIP_TRY(hipGetLastError());
        }
        if (!on_device)
        {
            HIP_TRY(hipMemcpyAsync(dst, d_depth, (size_t)probes * map_floats * 4, hipMemcpyDeviceToHost, st));
            if (out_stats) HIP_TRY(hipMemcpyAsync(dst_stats, d_stats, (size_t)probes * LUPIN_PROBE_DEPTH_STATS_WORDS * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));   // (the next batch writes the same buffers; the copies are to pageable memory)
        }
    }
    return query_end(ctx, "lupin_hip_bake_probe_depth");
}

int lupin_hip_sample_probe_grid_depth(LupinContext *ctx, const LupinScene *scene, const LupinProbeGridDepthDesc *desc, const float *sh, const float *depth,
                                      const uint8_t *valid, uint64_t n, const float *records, float *out)
{
    if (int rc = query_refuse(ctx, scene, desc && sh && depth && records && out)) return rc;
    const LupinProbeGridDesc &gd = desc->grid;
    uint64_t probes;   // (the visibility is the maps': VISIBILITY is the other entry point's)
    if (int rc = probe_grid_refuse(gd, LUPIN_PROBE_GRID_DEVICE_POINTERS | LUPIN_PROBE_GRID_BACKFACE,
                                   "unknown flag (LUPIN_PROBE_GRID_VISIBILITY belongs to lupin_hip_sample_probe_grid)", &probes))
        return rc;
    if (!probe_depth_resolution_ok(desc->resolution)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "resolution must be in [2, 64]");
    if (!(std::isfinite(desc->max_distance) && desc->max_distance > 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "max_distance must be finite and positive");
    if (n > LP_RAYS_MAX_PATHS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "n must not exceed 2^38");
    const bool on_device = (gd.flags & LUPIN_PROBE_GRID_DEVICE_POINTERS) != 0;
    if (on_device && ((((uintptr_t)sh | (uintptr_t)records | (uintptr_t)out) & 15u) || ((uintptr_t)depth & 7u)))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "device coefficients, records and results must be 16-byte aligned, device maps 8-byte aligned");
    if (n == 0) return LUPIN_OK;
    // the scene is not read: no hierarchy is asked for and nothing is planned
    if (int rc = query_start<ProbeGridRecordRule>(ctx, scene, on_device, n, records, 0u, false, nullptr)) return rc;
    hipStream_t st = ctx->stream;

    const ProbeGridDev g = probe_grid_dev(gd);
    const uint32_t R = desc->resolution;
    const uint64_t chunk = probe_grid_chunk_records(on_device, n);
    const float4 *d_sh = reinterpret_cast<const float4 *>(sh);
    const float2 *d_depth = reinterpret_cast<const float2 *>(depth);
    const uint8_t *d_valid = valid;
    DeviceBuffer b_sh, b_depth, b_valid, b_rec, b_res;   // host arrays: the grid whole, one chunk's records and results; they live for the call
    if (!on_device)
    {
        const size_t sh_bytes = (size_t)probes * LUPIN_PROBE_RESULT_FLOATS * 4, depth_bytes = (size_t)probes * (R + 2u) * (R + 2u) * 8u;
        HIP_TRY(DeviceBuffer::make(sh_bytes, &b_sh));
        HIP_TRY(DeviceBuffer::make(depth_bytes, &b_depth));
        HIP_TRY(DeviceBuffer::make((size_t)chunk * LUPIN_PROBE_GRID_RECORD_FLOATS * 4, &b_rec));
        HIP_TRY(DeviceBuffer::make((size_t)chunk * LUPIN_PROBE_GRID_RESULT_FLOATS * 4, &b_res));
        HIP_TRY(hipMemcpyAsync(b_sh.get(), sh, sh_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(b_depth.get(), depth, depth_bytes, hipMemcpyHostToDevice, st));
        d_sh = b_sh.as<float4>();
        d_depth = b_depth.as<float2>();
        if (valid)
        {
            HIP_TRY(DeviceBuffer::make((size_t)probes, &b_valid));
            HIP_TRY(hipMemcpyAsync(b_valid.get(), valid, (size_t)probes, hipMemcpyHostToDevice, st));
            d_valid = b_valid.as<uint8_t>();
        }
    }
    auto launch = [&](uint32_t recs, const float4 *d_rec, float4 *d_res) {
        hipLaunchKernelGGL(k_probe_grid_depth, probe_grid_blocks(recs), dim3(LP_BLOCK), 0, st, recs, g, R, desc->max_distance, d_sh, d_depth, d_valid, d_rec,
                           d_res);
    };
    return probe_grid_chunks(ctx, "lupin_hip_sample_probe_grid_depth", on_device, n, chunk, records, out, b_rec.get(), b_res.get(), launch);
}

// ---- baked-lighting view (no reference counterpart; kernels: lupin_baked_view.hpp) ----

static constexpr uint64_t LP_BAKED_VIEW_DEFAULT_SLOTS = LUPIN_BAKED_VIEW_DEFAULT_MAX_SLOTS;
static constexpr uint64_t LP_BAKED_VIEW_MAX_LAUNCH_SLOTS = LP_PROBE_GRID_MAX_LAUNCH;   // the lookup's kernel runs over a launch's slots

// What the two views (this one and the lightmapped view) refuse alike in a target and a view descriptor, neither of them NULL.
// `volume`: an irradiance volume was given (sh != NULL); the grid, and with depth maps their resolution and max_distance,
// are looked at only then, and *probes is the grid's probe count (0 without a volume).
static int baked_view_refuse(const LupinContext *ctx, const LupinTexture *render_target, const LupinBakedViewDesc *desc, bool volume, const float *depth,
                             uint64_t *probes)
{
    *probes = 0;
    if (render_target->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "the render target belongs to another context, or to one that has been destroyed");
    if (desc->flags & ~(uint32_t)LUPIN_BAKED_VIEW_DEVICE_POINTERS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown flag");
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(desc->ambient[k])) return fail(LUPIN_ERR_INVALID_ARGUMENT, "ambient must be finite");
    if (!(std::isfinite(desc->ray_epsilon) && desc->ray_epsilon >= 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "ray_epsilon must be finite and not negative");
    if (!volume) return LUPIN_OK;
    // the chosen lookup's refusals, by its own function and with its own message; where the arrays live is this descriptor's to say
    if (int rc = depth ? probe_grid_refuse(desc->grid, LUPIN_PROBE_GRID_BACKFACE,
                                           "unknown flag (LUPIN_PROBE_GRID_VISIBILITY belongs to lupin_hip_sample_probe_grid)", probes)
                       : probe_grid_refuse(desc->grid, LUPIN_PROBE_GRID_VISIBILITY | LUPIN_PROBE_GRID_BACKFACE, "unknown flag", probes))
        return rc;
    if (depth)
    {
        if (!probe_depth_resolution_ok(desc->resolution)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "resolution must be in [2, 64]");
        if (!(std::isfinite(desc->max_distance) && desc->max_distance > 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "max_distance must be finite and positive");
    }
    return LUPIN_OK;
}

// An irradiance volume as the lookup kernels take it.  Host arrays go whole into buffers that live as long as this does.
struct BakedVolume
{
    DeviceBuffer b_sh, b_depth, b_valid;
    const float4 *sh = nullptr;
    const float2 *depth = nullptr;
    const uint8_t *valid = nullptr;
};

static int baked_volume_stage(hipStream_t st, bool on_device, uint64_t probes, uint32_t R, const float *sh, const float *depth, const uint8_t *valid,
                              BakedVolume *v)
{
    v->sh = reinterpret_cast<const float4 *>(sh);
    v->depth = reinterpret_cast<const float2 *>(depth);
    v->valid = valid;
    if (on_device) return LUPIN_OK;
    const size_t sh_bytes = (size_t)probes * LUPIN_PROBE_RESULT_FLOATS * 4;
    HIP_TRY(DeviceBuffer::make(sh_bytes, &v->b_sh));
    HIP_TRY(hipMemcpyAsync(v->b_sh.get(), sh, sh_bytes, hipMemcpyHostToDevice, st));
    v->sh = v->b_sh.as<float4>();
    if (depth)
    {
        const size_t depth_bytes = (size_t)probes * (R + 2u) * (R + 2u) * 8u;
        HIP_TRY(DeviceBuffer::make(depth_bytes, &v->b_depth));
        HIP_TRY(hipMemcpyAsync(v->b_depth.get(), depth, depth_bytes, hipMemcpyHostToDevice, st));
        v->depth = v->b_depth.as<float2>();
    }
    if (valid)
    {
        HIP_TRY(DeviceBuffer::make((size_t)probes, &v->b_valid));
        HIP_TRY(hipMemcpyAsync(v->b_valid.get(), valid, (size_t)probes, hipMemcpyHostToDevice, st));
        v->valid = v->b_valid.as<uint8_t>();
    }
    return LUPIN_OK;
}

// The chosen lookup's own kernel over a launch's records: with depth maps k_probe_grid_depth, otherwise k_probe_grid by the
// lookup's plan `tl`.
static void baked_view_lookup(const LupinScene *scene, hipStream_t st, const LupinBakedViewDesc *desc, const BakedVolume &vol, bool vis, const TraversalLds &tl,
                              uint32_t slots, const float4 *rec, float4 *res)
{
    const ProbeGridDev g = probe_grid_dev(desc->grid);
    if (vol.depth)
        hipLaunchKernelGGL(k_probe_grid_depth, probe_grid_blocks(slots), dim3(LP_BLOCK), 0, st, slots, g, desc->resolution, desc->max_distance, vol.sh, vol.depth,
                           vol.valid, rec, res);
    else
        with_bool(tl.geo, [&](auto G) {
            with_bool(vis, [&](auto V) {
                hipLaunchKernelGGL((k_probe_grid<decltype(G)::value, decltype(V)::value>), probe_grid_blocks(slots), dim3(LP_BLOCK), tl.lds, st, scene->dev, slots,
                                   g, vol.sh, vol.valid, rec, res, tl.stack_words);
            });
        });
}

// The pixels of one launch: max_slots as asked (0: the default), a multiple of 64, at least 64, no more than the image needs.
static uint64_t baked_view_launch_slots(uint32_t asked_slots, uint64_t pixels)
{
    const uint64_t asked = asked_slots ? (uint64_t)asked_slots : LP_BAKED_VIEW_DEFAULT_SLOTS;
    return std::min(std::min(std::max<uint64_t>(asked / 64u * 64u, 64u), LP_BAKED_VIEW_MAX_LAUNCH_SLOTS), (pixels + 63u) / 64u * 64u);
}

static FrameParams baked_view_frame(const LupinBakedViewDesc *desc, uint32_t W, uint32_t H)
{
    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    set_camera_constants(fp.pc, desc->camera_params, desc->camera_transform);
    fp.width = W; fp.height = H; fp.reg_w = W; fp.reg_h = H;
    return fp;
}

int lupin_hip_render_baked(LupinContext *ctx, const LupinScene *scene, LupinTexture *render_target, const LupinBakedViewDesc *desc, const float *sh,
                           const float *depth, const uint8_t *valid, float *out_gbuffer)
{
    if (int rc = query_refuse(ctx, scene, render_target && desc && sh)) return rc;
    uint64_t probes;
    if (int rc = baked_view_refuse(ctx, render_target, desc, true, depth, &probes)) return rc;
    const LupinProbeGridDesc &gd = desc->grid;
    const uint32_t R = desc->resolution;
    if (int rc = query_refuse_hierarchy(ctx, scene, false)) return rc;
    const bool on_device = (desc->flags & LUPIN_BAKED_VIEW_DEVICE_POINTERS) != 0;
    if (on_device && ((((uintptr_t)sh | (uintptr_t)out_gbuffer) & 15u) || ((uintptr_t)depth & 7u)))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "device coefficients and G-buffer must be 16-byte aligned, device maps 8-byte aligned");
    const uint32_t W = render_target->width, H = render_target->height;
    const uint64_t pixels = (uint64_t)W * H;   // (not 0: lupin_hip_texture_create makes no empty texture)
    if (int rc = query_flush(ctx)) return rc;
    // two plans: the primary hit's (a stack of the scene's depth, staged geometry) and the lookup's own (lupin_hip_sample_probe_grid's)
    const bool vis = !depth && (gd.flags & LUPIN_PROBE_GRID_VISIBILITY) != 0;
    TraversalLds t, tl;
    if (int rc = traversal_lds(ctx, scene, scene->stack_entries, true, &t)) return rc;
    if (int rc = traversal_lds(ctx, scene, vis ? scene->stack_entries : 0u, vis, &tl)) return rc;
    if (int rc = join_primary(ctx)) return rc;
    hipStream_t st = ctx->stream;

    const FrameParams fp = baked_view_frame(desc, W, H);
    const BakedViewDev v{desc->ambient[0], desc->ambient[1], desc->ambient[2], (ctx->store_rounding == 1) ? 1u : 0u};

    const uint64_t max_slots = baked_view_launch_slots(desc->max_slots, pixels);
    // scratch for one launch; host arrays: the grid whole and one launch's G-buffer.  All of it lives for the call.
    DeviceBuffer b_rec, b_aux, b_res, b_gbuf;
    BakedVolume vol;
    HIP_TRY(DeviceBuffer::make((size_t)max_slots * LUPIN_PROBE_GRID_RECORD_FLOATS * 4, &b_rec));
    HIP_TRY(DeviceBuffer::make((size_t)max_slots * 32, &b_aux));
    HIP_TRY(DeviceBuffer::make((size_t)max_slots * LUPIN_PROBE_GRID_RESULT_FLOATS * 4, &b_res));
    if (int rc = baked_volume_stage(st, on_device, probes, R, sh, depth, valid, &vol)) return rc;
    if (!on_device && out_gbuffer) HIP_TRY(DeviceBuffer::make((size_t)max_slots * LUPIN_BAKED_VIEW_GBUFFER_FLOATS * 4, &b_gbuf));
    render_target->accum32_valid = false;   // the f16 texels are the only truth of this picture
    for (uint64_t first = 0; first < pixels; first += max_slots)
    {
        const uint32_t slots = (uint32_t)std::min(max_slots, pixels - first);
        float *dst = out_gbuffer ? out_gbuffer + first * LUPIN_BAKED_VIEW_GBUFFER_FLOATS : nullptr;
        float4 *d_gbuf = reinterpret_cast<float4 *>(out_gbuffer && !on_device ? b_gbuf.as<float>() : dst);
        const dim3 blocks((slots + LP_BLOCK - 1) / LP_BLOCK);
        with_bool(t.geo, [&](auto G) {
            hipLaunchKernelGGL(k_baked_gbuffer<decltype(G)::value>, blocks, dim3(LP_BLOCK), t.lds, st, scene->dev, fp, (unsigned long long)first, slots,
                               desc->ray_epsilon, b_rec.as<float4>(), b_aux.as<float4>(), d_gbuf, t.stack_words);
        });
        HIP_TRY(hipGetLastError());
        baked_view_lookup(scene, st, desc, vol, vis, tl, slots, b_rec.as<float4>(), b_res.as<float4>());
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_baked_compose, blocks, dim3(LP_BLOCK), 0, st, v, (unsigned long long)first, slots, b_aux.as<float4>(), b_res.as<float4>(),
                           render_target->data, d_gbuf);
        HIP_TRY(hipGetLastError());
        if (out_gbuffer && !on_device)
        {
            HIP_TRY(hipMemcpyAsync(dst, d_gbuf, (size_t)slots * LUPIN_BAKED_VIEW_GBUFFER_FLOATS * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));   // (the next launch writes the same buffer; the copy is to pageable memory)
        }
    }
    return query_end(ctx, "lupin_hip_render_baked");
}

// ---- lightmapped view (no reference counterpart; kernels: lupin_lightmapped_view.hpp) ----

// Both entry points of the view.  dd == NULL: lupin_hip_render_lightmapped (`directional` is not looked at); otherwise the
// directional variant, whose desc (dd->base) `desc` is.
static int render_lightmapped(const char *who, LupinContext *ctx, const LupinScene *scene, LupinTexture *render_target, const LupinLightmappedViewDesc *desc,
                              const LupinLightmappedDirectionalDesc *dd, const LupinLightmapChart *charts, const float *lightmap, const float *directional,
                              const float *sh, const float *depth, const uint8_t *valid, float *out_gbuffer)
{
    if (int rc = query_refuse(ctx, scene, render_target && desc && lightmap && (!dd || directional))) return rc;
    const LupinBakedViewDesc *view = &desc->view;
    const uint32_t gbuffer_floats = dd ? LUPIN_LIGHTMAPPED_DIRECTIONAL_GBUFFER_FLOATS : LUPIN_LIGHTMAPPED_VIEW_GBUFFER_FLOATS;
    uint64_t probes;
    if (int rc = baked_view_refuse(ctx, render_target, view, sh != nullptr, depth, &probes)) return rc;
    if (!sh && (depth || valid)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "depth and valid belong to a volume: sh is NULL");
    const uint32_t AW = desc->lightmap_width, AH = desc->lightmap_height, num_charts = desc->num_charts;
    if (AW == 0 || AH == 0 || AW > LUPIN_LIGHTMAP_MAX_SIZE || AH > LUPIN_LIGHTMAP_MAX_SIZE)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "lightmap_width and lightmap_height must be in [1, 16384]");
    if (desc->reserved != 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "reserved must be 0");
    if (dd)
    {
        if (dd->bake_flags & ~(uint32_t)LUPIN_LIGHTMAP_SMOOTH_NORMALS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown bake_flags bit");
        if (dd->reserved[0] | dd->reserved[1] | dd->reserved[2]) return fail(LUPIN_ERR_INVALID_ARGUMENT, "reserved must be 0");
    }
    if (num_charts > 0 && !charts) return fail(LUPIN_ERR_INVALID_ARGUMENT, "charts is NULL with num_charts > 0");
    // the chart of an instance is the first that names it; a chart is refused as lupin_hip_bake_lightmap refuses it
    const uint32_t num_instances = (uint32_t)scene->host_instances.size();
    std::vector<uint32_t> h_chart_of(std::max<uint32_t>(num_instances, 1u), LP_LMV_NO_CHART);
    std::vector<float4> h_charts(std::max<uint32_t>(num_charts, 1u), make_float4(0.0f, 0.0f, 0.0f, 0.0f));
    std::vector<const float2 *> h_chart_uvs(std::max<uint32_t>(num_charts, 1u), nullptr);   // per chart: its mesh's lightmap UV set, or null (the texcoords)
    for (uint32_t c = 0; c < num_charts; c++)
    {
        const LupinLightmapChart &ch = charts[c];
        if (ch.instance_idx >= num_instances) return fail(LUPIN_ERR_INVALID_ARGUMENT, "chart " + std::to_string(c) + ": instance index out of range");
        const uint32_t mesh = scene->host_instances[ch.instance_idx].mesh_idx;
        if (!scene->mesh_has_texcoords[mesh] && !scene->lightmap_set(mesh))
            return fail(LUPIN_ERR_INVALID_ARGUMENT, "chart " + std::to_string(c) + ": the instance's mesh has no texcoords and no lightmap UV set");
        if (!(std::isfinite(ch.scale_u) && std::isfinite(ch.scale_v) && std::isfinite(ch.offset_u) && std::isfinite(ch.offset_v)))
            return fail(LUPIN_ERR_INVALID_ARGUMENT, "chart " + std::to_string(c) + ": non-finite scale or offset");
        h_charts[c] = make_float4(ch.scale_u, ch.scale_v, ch.offset_u, ch.offset_v);
        h_chart_uvs[c] = scene->lightmap_set(mesh);
        if (h_chart_of[ch.instance_idx] == LP_LMV_NO_CHART) h_chart_of[ch.instance_idx] = c;
    }
    if (int rc = query_refuse_hierarchy(ctx, scene, false)) return rc;
    const bool on_device = (view->flags & LUPIN_BAKED_VIEW_DEVICE_POINTERS) != 0;
    if (on_device && ((((uintptr_t)lightmap | (uintptr_t)sh | (uintptr_t)out_gbuffer | (dd ? (uintptr_t)directional : 0u)) & 15u) || ((uintptr_t)depth & 7u)))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "device lightmap, coefficients and G-buffer must be 16-byte aligned, device maps 8-byte aligned");
    const uint32_t W = render_target->width, H = render_target->height;
    const uint64_t pixels = (uint64_t)W * H;
    if (int rc = query_flush(ctx)) return rc;
    // two plans, as lupin_hip_render_baked: the primary hit's and, with a volume, the lookup's own
    const bool vis = sh && !depth && (view->grid.flags & LUPIN_PROBE_GRID_VISIBILITY) != 0;
    TraversalLds t, tl;
    if (int rc = traversal_lds(ctx, scene, scene->stack_entries, true, &t)) return rc;
    if (int rc = traversal_lds(ctx, scene, vis ? scene->stack_entries : 0u, vis, &tl)) return rc;
    if (int rc = join_primary(ctx)) return rc;
    hipStream_t st = ctx->stream;

    const FrameParams fp = baked_view_frame(view, W, H);
    const LightmappedViewDev v{{view->ambient[0], view->ambient[1], view->ambient[2], (ctx->store_rounding == 1) ? 1u : 0u}, AW, AH, sh ? 1u : 0u};

    const uint64_t max_slots = baked_view_launch_slots(view->max_slots, pixels);
    // scratch for one launch (the lookup's results only with a volume); the chart tables; host arrays: the atlas and the grid
    // whole, one launch's G-buffer.  All of it lives for the call.
    DeviceBuffer b_rec, b_aux, b_lm, b_res, b_chart_of, b_charts, b_chart_uvs, b_atlas, b_gbuf, b_dir, b_planes;
    BakedVolume vol;
    HIP_TRY(DeviceBuffer::make((size_t)max_slots * LUPIN_PROBE_GRID_RECORD_FLOATS * 4, &b_rec));
    HIP_TRY(DeviceBuffer::make((size_t)max_slots * 32, &b_aux));
    HIP_TRY(DeviceBuffer::make((size_t)max_slots * 16, &b_lm));
    if (dd) HIP_TRY(DeviceBuffer::make((size_t)max_slots * 32, &b_dir));
    if (sh) HIP_TRY(DeviceBuffer::make((size_t)max_slots * LUPIN_PROBE_GRID_RESULT_FLOATS * 4, &b_res));
    HIP_TRY(DeviceBuffer::make(h_chart_of.size() * 4, &b_chart_of));
    HIP_TRY(DeviceBuffer::make(h_charts.size() * 16, &b_charts));
    HIP_TRY(hipMemcpyAsync(b_chart_of.get(), h_chart_of.data(), h_chart_of.size() * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(b_charts.get(), h_charts.data(), h_charts.size() * 16, hipMemcpyHostToDevice, st));
    HIP_TRY(DeviceBuffer::make(h_chart_uvs.size() * sizeof(const float2 *), &b_chart_uvs));
    HIP_TRY(hipMemcpyAsync(b_chart_uvs.get(), h_chart_uvs.data(), h_chart_uvs.size() * sizeof(const float2 *), hipMemcpyHostToDevice, st));
    const float4 *d_atlas = reinterpret_cast<const float4 *>(lightmap), *d_planes = reinterpret_cast<const float4 *>(directional);
    if (!on_device)
    {
        const size_t atlas_bytes = (size_t)AW * AH * 16;
        HIP_TRY(DeviceBuffer::make(atlas_bytes, &b_atlas));
        HIP_TRY(hipMemcpyAsync(b_atlas.get(), lightmap, atlas_bytes, hipMemcpyHostToDevice, st));
        d_atlas = b_atlas.as<float4>();
        if (dd)
        {
            HIP_TRY(DeviceBuffer::make(atlas_bytes * LUPIN_LIGHTMAP_DIRECTIONAL_PLANES, &b_planes));
            HIP_TRY(hipMemcpyAsync(b_planes.get(), directional, atlas_bytes * LUPIN_LIGHTMAP_DIRECTIONAL_PLANES, hipMemcpyHostToDevice, st));
            d_planes = b_planes.as<float4>();
        }
        if (out_gbuffer) HIP_TRY(DeviceBuffer::make((size_t)max_slots * gbuffer_floats * 4, &b_gbuf));
    }
    if (sh)
        if (int rc = baked_volume_stage(st, on_device, probes, view->resolution, sh, depth, valid, &vol)) return rc;
    render_target->accum32_valid = false;   // the f16 texels are the only truth of this picture
    for (uint64_t first = 0; first < pixels; first += max_slots)
    {
        const uint32_t slots = (uint32_t)std::min(max_slots, pixels - first);
        float *dst = out_gbuffer ? out_gbuffer + first * gbuffer_floats : nullptr;
        float4 *d_gbuf = reinterpret_cast<float4 *>(out_gbuffer && !on_device ? b_gbuf.as<float>() : dst);
        const dim3 blocks((slots + LP_BLOCK - 1) / LP_BLOCK);
        with_bool(t.geo, [&](auto G) {
            if (dd)
                hipLaunchKernelGGL(k_lightmapped_gbuffer_directional<decltype(G)::value>, blocks, dim3(LP_BLOCK), t.lds, st, scene->dev, fp, v,
                                   (unsigned long long)first, slots, view->ray_epsilon, b_chart_of.as<uint32_t>(), b_charts.as<float4>(), b_rec.as<float4>(),
                                   b_aux.as<float4>(), b_lm.as<float4>(), d_gbuf, t.stack_words, dd->bake_flags, b_dir.as<float4>(),
                                   b_chart_uvs.as<const float2 *>());
            else
                hipLaunchKernelGGL(k_lightmapped_gbuffer<decltype(G)::value>, blocks, dim3(LP_BLOCK), t.lds, st, scene->dev, fp, v, (unsigned long long)first,
                                   slots, view->ray_epsilon, b_chart_of.as<uint32_t>(), b_charts.as<float4>(), b_rec.as<float4>(), b_aux.as<float4>(),
                                   b_lm.as<float4>(), d_gbuf, t.stack_words, b_chart_uvs.as<const float2 *>());
        });
        HIP_TRY(hipGetLastError());
        if (sh)
        {
            baked_view_lookup(scene, st, view, vol, vis, tl, slots, b_rec.as<float4>(), b_res.as<float4>());
            HIP_TRY(hipGetLastError());
        }
        if (dd)
            hipLaunchKernelGGL(k_lightmapped_compose_directional, blocks, dim3(LP_BLOCK), 0, st, v, (unsigned long long)first, slots, b_aux.as<float4>(),
                               b_lm.as<float4>(), b_res.as<float4>(), d_atlas, render_target->data, d_gbuf, d_planes, b_dir.as<float4>());
        else
            hipLaunchKernelGGL(k_lightmapped_compose, blocks, dim3(LP_BLOCK), 0, st, v, (unsigned long long)first, slots, b_aux.as<float4>(),
                               b_lm.as<float4>(), b_res.as<float4>(), d_atlas, render_target->data, d_gbuf);
        HIP_TRY(hipGetLastError());
        if (out_gbuffer && !on_device)
        {
            HIP_TRY(hipMemcpyAsync(dst, d_gbuf, (size_t)slots * gbuffer_floats * 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));   // (the next launch writes the same buffer; the copy is to pageable memory)
        }
    }
    return query_end(ctx, who);
}

int lupin_hip_render_lightmapped(LupinContext *ctx, const LupinScene *scene, LupinTexture *render_target, const LupinLightmappedViewDesc *desc,
                                 const LupinLightmapChart *charts, const float *lightmap, const float *sh, const float *depth, const uint8_t *valid,
                                 float *out_gbuffer)
{
    return render_lightmapped("lupin_hip_render_lightmapped", ctx, scene, render_target, desc, nullptr, charts, lightmap, nullptr, sh, depth, valid,
                              out_gbuffer);
}

// (kernels: the _directional variants of lupin_lightmapped_view.hpp)
int lupin_hip_render_lightmapped_directional(LupinContext *ctx, const LupinScene *scene, LupinTexture *render_target,
                                             const LupinLightmappedDirectionalDesc *desc, const LupinLightmapChart *charts, const float *lightmap,
                                             const float *directional, const float *sh, const float *depth, const uint8_t *valid, float *out_gbuffer)
{
    return render_lightmapped("lupin_hip_render_lightmapped_directional", ctx, scene, render_target, desc ? &desc->base : nullptr, desc, charts, lightmap,
                              directional, sh, depth, valid, out_gbuffer);
}

// ---- lightmap baking (no reference counterpart; kernels: lupin_lightmap.hpp) ----

static thread_local LupinLightmapStats g_lightmap_stats = {0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
void lupin_hip_lightmap_stats(LupinLightmapStats *out) { if (out) *out = g_lightmap_stats; }

// What the two atlas bakes (lupin_hip_bake_lightmap, lupin_hip_bake_lightmap_ao) share: the refusals about the atlas ...
static int lightmap_refuse_atlas(uint32_t W, uint32_t H, uint32_t num_charts, uint32_t unknown_flags, uint32_t dilate, float surface_offset)
{
    if (W == 0 || H == 0 || W > LUPIN_LIGHTMAP_MAX_SIZE || H > LUPIN_LIGHTMAP_MAX_SIZE)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "width and height must be in [1, 16384]");
    if (num_charts == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "no charts");
    if (unknown_flags) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown flag");
    if (dilate > LUPIN_LIGHTMAP_MAX_DILATE) return fail(LUPIN_ERR_INVALID_ARGUMENT, "dilate must be <= 64");
    if (!(std::isfinite(surface_offset) && surface_offset > 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "surface_offset must be finite and positive");
    return LUPIN_OK;
}
// ... the refusals about the charts, and the charts as the kernels read them
static int lightmap_host_charts(const LupinScene *scene, const LupinLightmapChart *charts, uint32_t num_charts, std::vector<LmChartDev> *h_charts,
                                uint64_t *keys)
{
    h_charts->resize(num_charts);
    uint64_t total_keys = 0;
    for (uint32_t c = 0; c < num_charts; c++)
    {
        const LupinLightmapChart &ch = charts[c];
        if (ch.instance_idx >= scene->host_instances.size()) return fail(LUPIN_ERR_INVALID_ARGUMENT, "chart " + std::to_string(c) + ": instance index out of range");
        const uint32_t mesh = scene->host_instances[ch.instance_idx].mesh_idx;
        if (!scene->mesh_has_texcoords[mesh] && !scene->lightmap_set(mesh))
            return fail(LUPIN_ERR_INVALID_ARGUMENT, "chart " + std::to_string(c) + ": the instance's mesh has no texcoords and no lightmap UV set");
        if (!(std::isfinite(ch.scale_u) && std::isfinite(ch.scale_v) && std::isfinite(ch.offset_u) && std::isfinite(ch.offset_v)))
            return fail(LUPIN_ERR_INVALID_ARGUMENT, "chart " + std::to_string(c) + ": non-finite scale or offset");
        (*h_charts)[c] = LmChartDev{ch.instance_idx, (uint32_t)total_keys, scene->mesh_tri_count[mesh], 0u, ch.scale_u, ch.scale_v, ch.offset_u, ch.offset_v,
                                    scene->lightmap_set(mesh)};
        total_keys += scene->mesh_tri_count[mesh];
        if (total_keys >= 0xFFFFFFFFull) return fail(LUPIN_ERR_INVALID_ARGUMENT, "the charts hold 2^32 - 1 or more triangles");
    }
    *keys = total_keys;
    return LUPIN_OK;
}
using LmClock = std::chrono::steady_clock;
static float lm_ms_since(LmClock::time_point t0) { return std::chrono::duration<float, std::milli>(LmClock::now() - t0).count(); }
// ... and the records: raster, count, scan, emit on the primary stream `st`, each phase ending synchronised.  *n: the owned
// texels; with *n != 0, d_rec holds their records in ascending texel order and d_texel their texel indices.
static int lightmap_emit_records(const LupinScene *scene, hipStream_t st, const char *who, uint32_t W, uint32_t H, const std::vector<LmChartDev> &h_charts,
                                 uint64_t total_keys, uint32_t flags, uint32_t counter, float surface_offset, uint32_t *n_out, DeviceBuffer *d_rec,
                                 DeviceBuffer *d_texel, float *raster_ms, float *compact_ms)
{
    const uint32_t num_charts = (uint32_t)h_charts.size();
    const uint32_t texels = W * H;
    const uint32_t texel_blocks = (texels + LP_BLOCK - 1) / LP_BLOCK;
    DeviceBuffer d_charts, d_owner, d_totals;
    HIP_TRY(DeviceBuffer::make(h_charts.size() * sizeof(LmChartDev), &d_charts));
    HIP_TRY(DeviceBuffer::make((size_t)texels * 4, &d_owner));
    HIP_TRY(DeviceBuffer::make(((size_t)texel_blocks + 1) * 4, &d_totals));
    auto t0 = LmClock::now();
    HIP_TRY(hipMemcpyAsync(d_charts.get(), h_charts.data(), h_charts.size() * sizeof(LmChartDev), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_owner.get(), 0xFF, (size_t)texels * 4, st));
    if (total_keys)
        hipLaunchKernelGGL(k_lm_raster, dim3((uint32_t)((total_keys + LP_BLOCK / 64 - 1) / (LP_BLOCK / 64))), dim3(LP_BLOCK), 0, st, scene->dev,
                           d_charts.as<LmChartDev>(), num_charts, (uint32_t)total_keys, W, H, d_owner.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    *raster_ms = lm_ms_since(t0);

    t0 = LmClock::now();
    hipLaunchKernelGGL(k_lm_count, dim3(texel_blocks), dim3(LP_BLOCK), 0, st, d_owner.as<uint32_t>(), texels, d_totals.as<uint32_t>());
    hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(LP_LM_SCAN_THREADS), 0, st, d_totals.as<uint32_t>(), texel_blocks);
    HIP_TRY(hipGetLastError());
    uint32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, d_totals.as<uint32_t>() + texel_blocks, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n > texels) return fail(LUPIN_ERR_HIP, std::string(who) + ": the compaction counted more texels than the atlas has");
    *n_out = n;
    if (n != 0)
    {
        HIP_TRY(DeviceBuffer::make((size_t)n * LUPIN_RAY_RECORD_FLOATS * 4, d_rec));
        HIP_TRY(DeviceBuffer::make((size_t)n * 4, d_texel));
        hipLaunchKernelGGL(k_lm_emit, dim3(texel_blocks), dim3(LP_BLOCK), 0, st, scene->dev, d_charts.as<LmChartDev>(), num_charts, W, H,
                           d_owner.as<uint32_t>(), d_totals.as<uint32_t>(), flags, counter, surface_offset, d_rec->as<float4>(), d_texel->as<uint32_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
    }
    *compact_ms = lm_ms_since(t0);
    return LUPIN_OK;
}

// What the radiance query refuses in a descriptor, refused by the two path-traced bakes as well: an atlas without an owned texel
// never reaches the query.
static int lightmap_refuse_query(const LupinLightmapDesc *desc)
{
    if (desc->pathtrace_type > LUPIN_PATHTRACE_DIRECT) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown pathtrace_type");
    if (desc->samples == 0 || desc->samples > LP_RAYS_MAX_CHUNK_SLOTS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "samples must be in [1, 2^27]");
    if (desc->max_bounces >= META_BOUNCE_MASK) return fail(LUPIN_ERR_INVALID_ARGUMENT, "max_bounces must be < 4095");
    return LUPIN_OK;
}

int lupin_hip_bake_lightmap(LupinContext *ctx, const LupinScene *scene, const LupinLightmapDesc *desc, const LupinLightmapChart *charts,
                            uint32_t num_charts, float *out_rgba, float *out_records, uint64_t *out_num_covered)
{
    const char *who = "lupin_hip_bake_lightmap";
    if (int rc = query_refuse(ctx, scene, desc && charts && out_rgba)) return rc;
    const uint32_t W = desc->width, H = desc->height;
    if (int rc = lightmap_refuse_atlas(W, H, num_charts, desc->flags & ~(uint32_t)LUPIN_LIGHTMAP_SMOOTH_NORMALS, desc->dilate, desc->surface_offset)) return rc;
    if (int rc = lightmap_refuse_query(desc)) return rc;
    if (int rc = query_refuse_hierarchy(ctx, scene, true)) return rc;
    std::vector<LmChartDev> h_charts;
    uint64_t total_keys = 0;
    if (int rc = lightmap_host_charts(scene, charts, num_charts, &h_charts, &total_keys)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = join_primary(ctx)) return rc;   // recorded calls run first
    hipStream_t st = ctx->lanes[0].stream;   // the primary stream, the query's own
    using clk = LmClock;
    auto ms_since = lm_ms_since;
    LupinLightmapStats stats = {0, (uint32_t)total_keys, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};

    const uint32_t texels = W * H;
    const uint32_t texel_blocks = (texels + LP_BLOCK - 1) / LP_BLOCK;
    uint32_t n = 0;
    DeviceBuffer d_rec, d_texel, d_mean;
    if (int rc = lightmap_emit_records(scene, st, who, W, H, h_charts, total_keys, desc->flags, desc->counter, desc->surface_offset, &n, &d_rec, &d_texel,
                                       &stats.raster_ms, &stats.compact_ms))
        return rc;
    stats.covered_texels = n;
    if (n == 0)
    {
        memset(out_rgba, 0, (size_t)texels * 16);
        if (out_records) memset(out_records, 0, (size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4);
        if (out_num_covered) *out_num_covered = 0;
        g_lightmap_stats = stats;
        return LUPIN_OK;
    }
    HIP_TRY(DeviceBuffer::make((size_t)n * LUPIN_RAY_RESULT_FLOATS * 4, &d_mean));

    // one query on the device records: its validation, its chunks
    auto t0 = clk::now();
    const LupinRayQueryDesc q{desc->pathtrace_type, desc->max_bounces, desc->samples, LUPIN_RAYS_DEVICE_POINTERS, desc->max_slots, desc->advanced};
    if (int rc = lupin_hip_pathtrace_rays(ctx, scene, &q, n, d_rec.as<float>(), d_mean.as<float>(), nullptr)) return rc;
    stats.trace_ms = ms_since(t0);

    t0 = clk::now();
    DeviceBuffer d_rgba[2], d_filled[2], d_plane;
    const int planes = desc->dilate ? 2 : 1;
    for (int k = 0; k < planes; k++)
    {
        HIP_TRY(DeviceBuffer::make((size_t)texels * 16, &d_rgba[k]));
        HIP_TRY(DeviceBuffer::make((size_t)texels, &d_filled[k]));
    }
    HIP_TRY(hipMemsetAsync(d_rgba[0].get(), 0, (size_t)texels * 16, st));
    HIP_TRY(hipMemsetAsync(d_filled[0].get(), 0, (size_t)texels, st));
    if (out_records)
    {
        HIP_TRY(DeviceBuffer::make((size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4, &d_plane));
        HIP_TRY(hipMemsetAsync(d_plane.get(), 0, (size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4, st));
    }
    hipLaunchKernelGGL(k_lm_scatter, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, n, d_texel.as<uint32_t>(), d_mean.as<float4>(),
                       d_rec.as<float4>(), d_rgba[0].as<float4>(), d_filled[0].as<uint8_t>(), d_plane.as<float4>());
    int cur = 0;
    for (uint32_t pass = 0; pass < desc->dilate; pass++, cur ^= 1)
        hipLaunchKernelGGL(k_lm_dilate, dim3(texel_blocks), dim3(LP_BLOCK), 0, st, W, H, d_rgba[cur].as<float4>(), d_filled[cur].as<uint8_t>(),
                           d_rgba[cur ^ 1].as<float4>(), d_filled[cur ^ 1].as<uint8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    stats.scatter_dilate_ms = ms_since(t0);

    t0 = clk::now();
    HIP_TRY(hipMemcpyAsync(out_rgba, d_rgba[cur].get(), (size_t)texels * 16, hipMemcpyDeviceToHost, st));
    if (out_records) HIP_TRY(hipMemcpyAsync(out_records, d_plane.get(), (size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4, hipMemcpyDeviceToHost, st));
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(LUPIN_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    stats.download_ms = ms_since(t0);
    if (out_num_covered) *out_num_covered = n;
    g_lightmap_stats = stats;
    return LUPIN_OK;
}

// ---- directional lightmaps (kernels: lupin_lightmap_directional.hpp) ----

int lupin_hip_bake_lightmap_directional(LupinContext *ctx, const LupinScene *scene, const LupinLightmapDesc *desc, const LupinLightmapChart *charts,
                                        uint32_t num_charts, float *out_sh, float *out_records, uint64_t *out_num_covered)
{
    const char *who = "lupin_hip_bake_lightmap_directional";
    if (int rc = query_refuse(ctx, scene, desc && charts && out_sh)) return rc;
    const uint32_t W = desc->width, H = desc->height;
    if (int rc = lightmap_refuse_atlas(W, H, num_charts, desc->flags & ~(uint32_t)LUPIN_LIGHTMAP_SMOOTH_NORMALS, desc->dilate, desc->surface_offset)) return rc;
    if (int rc = lightmap_refuse_query(desc)) return rc;
    if (int rc = query_refuse_hierarchy(ctx, scene, true)) return rc;
    std::vector<LmChartDev> h_charts;
    uint64_t total_keys = 0;
    if (int rc = lightmap_host_charts(scene, charts, num_charts, &h_charts, &total_keys)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = join_primary(ctx)) return rc;   // recorded calls run first
    hipStream_t st = ctx->lanes[0].stream;   // the primary stream, the query's own

    const uint32_t texels = W * H;
    const uint32_t texel_blocks = (texels + LP_BLOCK - 1) / LP_BLOCK;
    const size_t plane_bytes = (size_t)texels * 16, planes_bytes = plane_bytes * LP_LM_SH;
    // the planes before anything is launched: a refusal for want of memory leaves the outputs untouched and the device idle
    DeviceBuffer d_planes[2], d_filled[2], d_plane;
    const int sets = desc->dilate ? 2 : 1;
    for (int k = 0; k < sets; k++)
        if (DeviceBuffer::make(planes_bytes, &d_planes[k]) != hipSuccess || DeviceBuffer::make((size_t)texels, &d_filled[k]) != hipSuccess)
        {
            (void)hipGetLastError();
            return fail(LUPIN_ERR_OUT_OF_MEMORY, std::string(who) + ": no device memory for the coefficient planes");
        }
    uint32_t n = 0;
    DeviceBuffer d_rec, d_texel, d_coef;
    float raster_ms, compact_ms;
    if (int rc = lightmap_emit_records(scene, st, who, W, H, h_charts, total_keys, desc->flags, desc->counter, desc->surface_offset, &n, &d_rec, &d_texel,
                                       &raster_ms, &compact_ms))
        return rc;
    if (n == 0)
    {
        memset(out_sh, 0, planes_bytes);
        if (out_records) memset(out_records, 0, (size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4);
        if (out_num_covered) *out_num_covered = 0;
        return LUPIN_OK;
    }
    HIP_TRY(DeviceBuffer::make((size_t)n * LP_LM_SH * 16, &d_coef));

    // one query on the device records: its validation, its chunks (whole records), its wavefront; the resolve is this bake's
    const PathQuery q = {who, desc->pathtrace_type, LUPIN_RAYS_DEVICE_POINTERS, desc->samples, desc->max_bounces, desc->max_slots, &desc->advanced,
                         LP_LM_SH * 4u};
    if (int rc = path_query<RayRecordRule>(ctx, scene, q, n, d_rec.as<float>(), d_coef.as<float>(), nullptr, [ctx, scene](const PathChunk &c) -> int {
            const RayBegin rb{c.d_records, c.samples, c.d_rays};
            HIP_TRY(enqueue_wavefront(ctx, c.ln, scene, c.pathtrace_type, c.slots, c.sh, c.iterations, nullptr, &rb));
            hipLaunchKernelGGL(k_resolve_lightmap_sh, dim3((c.records + LP_LM_SH_RECORDS_PER_BLOCK - 1) / LP_LM_SH_RECORDS_PER_BLOCK), dim3(LP_BLOCK), 0,
                               c.ln->stream, c.ln->pb, c.records, c.d_records, c.samples, c.d_out);
            HIP_TRY(hipGetLastError());
            return LUPIN_OK;
        }))
        return rc;

    HIP_TRY(hipMemsetAsync(d_planes[0].get(), 0, planes_bytes, st));
    HIP_TRY(hipMemsetAsync(d_filled[0].get(), 0, (size_t)texels, st));
    if (out_records)
    {
        HIP_TRY(DeviceBuffer::make((size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4, &d_plane));
        HIP_TRY(hipMemsetAsync(d_plane.get(), 0, (size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4, st));
    }
    hipLaunchKernelGGL(k_lm_sh_scatter, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, n, d_texel.as<uint32_t>(), d_coef.as<float4>(),
                       d_rec.as<float4>(), texels, d_planes[0].as<float4>(), d_filled[0].as<uint8_t>(), d_plane.as<float4>());
    // the gutter passes of lupin_hip_bake_lightmap on each plane (the filled bytes are the same for all four)
    int cur = 0;
    for (uint32_t pass = 0; pass < desc->dilate; pass++, cur ^= 1)
        for (uint32_t j = 0; j < LP_LM_SH; j++)
            hipLaunchKernelGGL(k_lm_dilate, dim3(texel_blocks), dim3(LP_BLOCK), 0, st, W, H, d_planes[cur].as<float4>() + (size_t)j * texels,
                               d_filled[cur].as<uint8_t>(), d_planes[cur ^ 1].as<float4>() + (size_t)j * texels, d_filled[cur ^ 1].as<uint8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_sh, d_planes[cur].get(), planes_bytes, hipMemcpyDeviceToHost, st));
    if (out_records) HIP_TRY(hipMemcpyAsync(out_records, d_plane.get(), (size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4, hipMemcpyDeviceToHost, st));
    if (int rc = query_end(ctx, who)) return rc;
    if (out_num_covered) *out_num_covered = n;
    return LUPIN_OK;
}

// ---- adaptive lightmap baking (kernels: lupin_lightmap_adaptive.hpp) ----

static thread_local LupinLightmapAdaptiveStats g_lightmap_adaptive_stats = {0, 0, 0, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
void lupin_hip_lightmap_adaptive_stats(LupinLightmapAdaptiveStats *out) { if (out) *out = g_lightmap_adaptive_stats; }

int lupin_hip_bake_lightmap_adaptive(LupinContext *ctx, const LupinScene *scene, const LupinLightmapDesc *desc, const LupinLightmapAdaptiveDesc *ad,
                                     const LupinLightmapChart *charts, uint32_t num_charts, float *out_rgba, float *out_stats, float *out_records,
                                     uint64_t *out_num_covered)
{
    const char *who = "lupin_hip_bake_lightmap_adaptive";
    if (int rc = query_refuse(ctx, scene, desc && ad && charts && out_rgba)) return rc;
    const uint32_t W = desc->width, H = desc->height;
    if (int rc = lightmap_refuse_atlas(W, H, num_charts, desc->flags & ~(uint32_t)LUPIN_LIGHTMAP_SMOOTH_NORMALS, desc->dilate, desc->surface_offset)) return rc;
    if (int rc = lightmap_refuse_query(desc)) return rc;
    if (!(std::isfinite(ad->threshold) && ad->threshold >= 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "threshold must be finite and not negative");
    if (ad->min_rounds == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "min_rounds must be >= 1");
    if (ad->max_rounds < ad->min_rounds || ad->max_rounds > LUPIN_LIGHTMAP_ADAPTIVE_MAX_ROUNDS)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "max_rounds must be in [min_rounds, 4096]");
    if ((uint64_t)desc->samples * ad->max_rounds > (1ull << 24))   // (float)n_i is exact
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "samples * max_rounds must not exceed 2^24");
    if (ad->flags) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown adaptive flag");
    if (int rc = query_refuse_hierarchy(ctx, scene, true)) return rc;
    std::vector<LmChartDev> h_charts;
    uint64_t total_keys = 0;
    if (int rc = lightmap_host_charts(scene, charts, num_charts, &h_charts, &total_keys)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = join_primary(ctx)) return rc;   // recorded calls run first
    hipStream_t st = ctx->lanes[0].stream;   // the primary stream, the query's own
    LupinLightmapAdaptiveStats stats = {0, 0, 0, 0, 0, (uint32_t)total_keys, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};

    const uint32_t texels = W * H;
    const uint32_t texel_blocks = (texels + LP_BLOCK - 1) / LP_BLOCK;
    const size_t plane_bytes = (size_t)texels * 16, record_plane_bytes = (size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4;
    // the planes before anything is launched: a refusal for want of memory leaves the outputs untouched and the device idle
    DeviceBuffer d_rgba[2], d_filled[2], d_stats, d_plane, d_want, d_counts;
    {
        bool ok = true;
        for (int k = 0; k < (desc->dilate ? 2 : 1); k++)
            ok = ok && DeviceBuffer::make(plane_bytes, &d_rgba[k]) == hipSuccess && DeviceBuffer::make((size_t)texels, &d_filled[k]) == hipSuccess;
        ok = ok && DeviceBuffer::make(plane_bytes, &d_stats) == hipSuccess && DeviceBuffer::make((size_t)texels, &d_want) == hipSuccess;
        ok = ok && DeviceBuffer::make(2 * sizeof(unsigned long long), &d_counts) == hipSuccess;
        if (out_records) ok = ok && DeviceBuffer::make(record_plane_bytes, &d_plane) == hipSuccess;
        if (!ok)
        {
            (void)hipGetLastError();
            return fail(LUPIN_ERR_OUT_OF_MEMORY, std::string(who) + ": no device memory for the atlas planes");
        }
    }
    uint32_t n = 0;
    DeviceBuffer d_rec, d_texel;
    if (int rc = lightmap_emit_records(scene, st, who, W, H, h_charts, total_keys, desc->flags, desc->counter, desc->surface_offset, &n, &d_rec, &d_texel,
                                       &stats.raster_ms, &stats.compact_ms))
        return rc;
    stats.covered_texels = n;
    if (n == 0)
    {
        memset(out_rgba, 0, plane_bytes);
        if (out_stats) memset(out_stats, 0, plane_bytes);
        if (out_records) memset(out_records, 0, record_plane_bytes);
        if (out_num_covered) *out_num_covered = 0;
        g_lightmap_adaptive_stats = stats;
        return LUPIN_OK;
    }

    // per record: the state, the active bytes; per round (sized for a round of all records): its records, their indices, their moments
    const uint32_t S = desc->samples;
    const uint32_t rec_blocks = (n + LP_BLOCK - 1) / LP_BLOCK;
    DeviceBuffer d_samples, d_rounds, d_mean, d_m2, d_active, d_totals, d_round_rec, d_index, d_moments;
    HIP_TRY(DeviceBuffer::make((size_t)n * 4, &d_samples));
    HIP_TRY(DeviceBuffer::make((size_t)n * 4, &d_rounds));
    HIP_TRY(DeviceBuffer::make((size_t)n * 16, &d_mean));
    HIP_TRY(DeviceBuffer::make((size_t)n * 4, &d_m2));
    HIP_TRY(DeviceBuffer::make((size_t)n, &d_active));
    HIP_TRY(DeviceBuffer::make(((size_t)rec_blocks + 1) * 4, &d_totals));
    HIP_TRY(DeviceBuffer::make((size_t)n * LUPIN_RAY_RECORD_FLOATS * 4, &d_round_rec));
    HIP_TRY(DeviceBuffer::make((size_t)n * 4, &d_index));
    HIP_TRY(DeviceBuffer::make((size_t)n * LUPIN_RAY_MOMENTS_FLOATS * 4, &d_moments));
    const LmAdaptiveDev state{d_samples.as<uint32_t>(), d_rounds.as<uint32_t>(), d_mean.as<float4>(), d_m2.as<float>()};
    HIP_TRY(hipMemsetAsync(d_samples.get(), 0, (size_t)n * 4, st));
    HIP_TRY(hipMemsetAsync(d_rounds.get(), 0, (size_t)n * 4, st));
    HIP_TRY(hipMemsetAsync(d_mean.get(), 0, (size_t)n * 16, st));
    HIP_TRY(hipMemsetAsync(d_m2.get(), 0, (size_t)n * 4, st));
    HIP_TRY(hipMemsetAsync(d_active.get(), 1, (size_t)n, st));   // round 0: every record
    HIP_TRY(hipMemsetAsync(d_want.get(), 0, (size_t)texels, st));
    HIP_TRY(hipMemsetAsync(d_counts.get(), 0, 2 * sizeof(unsigned long long), st));

    // Every round pays the query's validation of its records and its synchronisation: the price of running the wavefront
    // through path_query unchanged.  The loop ends when no record is active.  Every round that traces adds one to rounds_i of
    // each of its records and no record is active at max_rounds, so it ends; a record that a neighbour woke late is behind the
    // call's round count, so the call may run more than max_rounds rounds.
    const PathQuery q = {who, desc->pathtrace_type, LUPIN_RAYS_DEVICE_POINTERS, S, desc->max_bounces, desc->max_slots, &desc->advanced, LUPIN_RAY_MOMENTS_FLOATS};
    for (uint32_t round = 0;; round++)
    {
        auto t0 = LmClock::now();
        hipLaunchKernelGGL(k_lm_ad_count, dim3(rec_blocks), dim3(LP_BLOCK), 0, st, d_active.as<uint8_t>(), n, d_totals.as<uint32_t>());
        hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(LP_LM_SCAN_THREADS), 0, st, d_totals.as<uint32_t>(), rec_blocks);
        HIP_TRY(hipGetLastError());
        uint32_t n_active = 0;
        HIP_TRY(hipMemcpyAsync(&n_active, d_totals.as<uint32_t>() + rec_blocks, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (n_active > n) return fail(LUPIN_ERR_HIP, std::string(who) + ": the compaction counted more records than the atlas owns");
        if (n_active == 0)
        {
            stats.compact_ms += lm_ms_since(t0);
            break;
        }
        hipLaunchKernelGGL(k_lm_ad_emit, dim3(rec_blocks), dim3(LP_BLOCK), 0, st, d_active.as<uint8_t>(), n, d_totals.as<uint32_t>(), d_rec.as<float4>(), round,
                           d_round_rec.as<float4>(), d_index.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        stats.compact_ms += lm_ms_since(t0);

        t0 = LmClock::now();
        if (int rc = path_query<RayRecordRule>(ctx, scene, q, n_active, d_round_rec.as<float>(), d_moments.as<float>(), nullptr,
                                               [ctx, scene](const PathChunk &c) -> int { return launch_moments_chunk(ctx, scene, c); }))
            return rc;
        stats.trace_ms += lm_ms_since(t0);
        stats.rounds++;
        stats.paths += (uint64_t)n_active * S;

        t0 = LmClock::now();
        hipLaunchKernelGGL(k_lm_ad_merge, dim3((n_active + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, n_active, d_index.as<uint32_t>(),
                           d_moments.as<float4>(), S, state, d_texel.as<uint32_t>(), ad->threshold, ad->min_rounds, ad->max_rounds, d_want.as<uint8_t>());
        hipLaunchKernelGGL(k_lm_ad_mask, dim3(rec_blocks), dim3(LP_BLOCK), 0, st, n, d_texel.as<uint32_t>(), W, H, d_want.as<uint8_t>(),
                           d_rounds.as<uint32_t>(), ad->max_rounds, d_active.as<uint8_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));
        stats.merge_mask_ms += lm_ms_since(t0);
    }

    // the plain bake's scatter (it reads the means' r, g, b) and gutter passes; the statistics are not dilated
    auto t0 = LmClock::now();
    HIP_TRY(hipMemsetAsync(d_rgba[0].get(), 0, plane_bytes, st));
    HIP_TRY(hipMemsetAsync(d_filled[0].get(), 0, (size_t)texels, st));
    HIP_TRY(hipMemsetAsync(d_stats.get(), 0, plane_bytes, st));
    if (out_records) HIP_TRY(hipMemsetAsync(d_plane.get(), 0, record_plane_bytes, st));
    hipLaunchKernelGGL(k_lm_scatter, dim3(rec_blocks), dim3(LP_BLOCK), 0, st, n, d_texel.as<uint32_t>(), d_mean.as<float4>(), d_rec.as<float4>(),
                       d_rgba[0].as<float4>(), d_filled[0].as<uint8_t>(), d_plane.as<float4>());
    hipLaunchKernelGGL(k_lm_ad_stats, dim3(rec_blocks), dim3(LP_BLOCK), 0, st, n, d_texel.as<uint32_t>(), state, ad->threshold, ad->min_rounds, ad->max_rounds,
                       d_stats.as<float4>(), d_counts.as<unsigned long long>());
    int cur = 0;
    for (uint32_t pass = 0; pass < desc->dilate; pass++, cur ^= 1)
        hipLaunchKernelGGL(k_lm_dilate, dim3(texel_blocks), dim3(LP_BLOCK), 0, st, W, H, d_rgba[cur].as<float4>(), d_filled[cur].as<uint8_t>(),
                           d_rgba[cur ^ 1].as<float4>(), d_filled[cur ^ 1].as<uint8_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    stats.scatter_dilate_ms = lm_ms_since(t0);

    t0 = LmClock::now();
    unsigned long long counts[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(out_rgba, d_rgba[cur].get(), plane_bytes, hipMemcpyDeviceToHost, st));
    if (out_stats) HIP_TRY(hipMemcpyAsync(out_stats, d_stats.get(), plane_bytes, hipMemcpyDeviceToHost, st));
    if (out_records) HIP_TRY(hipMemcpyAsync(out_records, d_plane.get(), record_plane_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(counts, d_counts.get(), sizeof(counts), hipMemcpyDeviceToHost, st));
    if (int rc = query_end(ctx, who)) return rc;
    stats.download_ms = lm_ms_since(t0);
    stats.converged_texels = counts[0];
    stats.capped_texels = counts[1];
    if (out_num_covered) *out_num_covered = n;
    g_lightmap_adaptive_stats = stats;
    return LUPIN_OK;
}

// ---- ambient-occlusion and bent-normal atlases (kernels: lupin_lightmap.hpp, lupin_bent_normal.hpp) ----

int lupin_hip_bake_lightmap_ao(LupinContext *ctx, const LupinScene *scene, const LupinLightmapAoDesc *desc, const LupinLightmapChart *charts,
                               uint32_t num_charts, float *out_ao, float *out_bent, float *out_records, uint64_t *out_num_covered)
{
    const char *who = "lupin_hip_bake_lightmap_ao";
    if (int rc = query_refuse(ctx, scene, desc && charts && out_ao)) return rc;
    const uint32_t W = desc->width, H = desc->height;
    if (int rc = lightmap_refuse_atlas(W, H, num_charts, desc->flags & ~(uint32_t)(LUPIN_LIGHTMAP_SMOOTH_NORMALS | LUPIN_LIGHTMAP_AO_OPACITY), desc->dilate,
                                       desc->surface_offset))
        return rc;
    // what the query refuses in a descriptor, here as well: an atlas without an owned texel never reaches the query
    if (int rc = bent_normal_refuse(desc->samples, desc->ray_epsilon)) return rc;
    if (!(desc->max_distance > 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "max_distance must be positive (+inf: unbounded)");   // (NaN > 0 is false)
    if (int rc = query_refuse_hierarchy(ctx, scene, false)) return rc;
    std::vector<LmChartDev> h_charts;
    uint64_t total_keys = 0;
    if (int rc = lightmap_host_charts(scene, charts, num_charts, &h_charts, &total_keys)) return rc;
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = join_primary(ctx)) return rc;   // recorded calls run first
    hipStream_t st = ctx->lanes[0].stream;   // the primary stream, the query's own

    const uint32_t texels = W * H;
    const uint32_t texel_blocks = (texels + LP_BLOCK - 1) / LP_BLOCK;
    uint32_t n = 0;
    DeviceBuffer d_rec, d_texel, d_sums;
    float raster_ms, compact_ms;
    if (int rc = lightmap_emit_records(scene, st, who, W, H, h_charts, total_keys, desc->flags & LUPIN_LIGHTMAP_SMOOTH_NORMALS, desc->counter,
                                       desc->surface_offset, &n, &d_rec, &d_texel, &raster_ms, &compact_ms))
        return rc;
    if (n == 0)
    {
        memset(out_ao, 0, (size_t)texels * 16);
        if (out_bent) memset(out_bent, 0, (size_t)texels * 16);
        if (out_records) memset(out_records, 0, (size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4);
        if (out_num_covered) *out_num_covered = 0;
        return LUPIN_OK;
    }
    // one query on the device records (the radiance query's: word [7] is its mode, the slots' tmax is max_distance)
    HIP_TRY(DeviceBuffer::make((size_t)n * LUPIN_BENT_NORMAL_RESULT_FLOATS * 4, &d_sums));
    const BentNormalQuery q = {who, desc->samples, desc->max_slots, (desc->flags & LUPIN_LIGHTMAP_AO_OPACITY) != 0, true, desc->ray_epsilon, true,
                               desc->max_distance};
    if (int rc = bent_normal_query<RayRecordRule>(ctx, scene, q, n, d_rec.as<float>(), d_sums.as<float>())) return rc;

    // both planes: the per-texel formulas, then the gutter passes of lupin_hip_bake_lightmap (the filled bytes are the same for both)
    DeviceBuffer d_ao[2], d_bent[2], d_filled[2], d_plane;
    const int planes = desc->dilate ? 2 : 1;
    for (int k = 0; k < planes; k++)
    {
        HIP_TRY(DeviceBuffer::make((size_t)texels * 16, &d_ao[k]));
        if (out_bent) HIP_TRY(DeviceBuffer::make((size_t)texels * 16, &d_bent[k]));
        HIP_TRY(DeviceBuffer::make((size_t)texels, &d_filled[k]));
    }
    HIP_TRY(hipMemsetAsync(d_ao[0].get(), 0, (size_t)texels * 16, st));
    if (out_bent) HIP_TRY(hipMemsetAsync(d_bent[0].get(), 0, (size_t)texels * 16, st));
    HIP_TRY(hipMemsetAsync(d_filled[0].get(), 0, (size_t)texels, st));
    if (out_records)
    {
        HIP_TRY(DeviceBuffer::make((size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4, &d_plane));
        HIP_TRY(hipMemsetAsync(d_plane.get(), 0, (size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4, st));
    }
    hipLaunchKernelGGL(k_lm_ao_scatter, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, n, d_texel.as<uint32_t>(), d_sums.as<float4>(),
                       d_rec.as<float4>(), (float)desc->samples, d_ao[0].as<float4>(), d_bent[0].as<float4>(), d_filled[0].as<uint8_t>(),
                       d_plane.as<float4>());
    int cur = 0;
    for (uint32_t pass = 0; pass < desc->dilate; pass++, cur ^= 1)
    {
        if (out_bent)
            hipLaunchKernelGGL(k_lm_dilate, dim3(texel_blocks), dim3(LP_BLOCK), 0, st, W, H, d_bent[cur].as<float4>(), d_filled[cur].as<uint8_t>(),
                               d_bent[cur ^ 1].as<float4>(), d_filled[cur ^ 1].as<uint8_t>());
        hipLaunchKernelGGL(k_lm_dilate, dim3(texel_blocks), dim3(LP_BLOCK), 0, st, W, H, d_ao[cur].as<float4>(), d_filled[cur].as<uint8_t>(),
                           d_ao[cur ^ 1].as<float4>(), d_filled[cur ^ 1].as<uint8_t>());
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_ao, d_ao[cur].get(), (size_t)texels * 16, hipMemcpyDeviceToHost, st));
    if (out_bent) HIP_TRY(hipMemcpyAsync(out_bent, d_bent[cur].get(), (size_t)texels * 16, hipMemcpyDeviceToHost, st));
    if (out_records) HIP_TRY(hipMemcpyAsync(out_records, d_plane.get(), (size_t)texels * LUPIN_RAY_RECORD_FLOATS * 4, hipMemcpyDeviceToHost, st));
    if (int rc = query_end(ctx, who)) return rc;
    if (out_num_covered) *out_num_covered = n;
    return LUPIN_OK;
}

// ---- lightmap UV sets (no reference counterpart; kernels: lupin_unwrap.hpp, packer: include/lupin_pack.hpp) ----

int lupin_hip_scene_set_lightmap_uvs(LupinScene *scene, uint32_t mesh_idx, const float *uvs, uint64_t num_corners)
{
    if (!scene) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    LupinContext *ctx = scene->ctx;
    CTX_ALIVE_TRY(ctx);
    if (mesh_idx >= scene->mesh_tri_count.size()) return fail(LUPIN_ERR_INVALID_ARGUMENT, "set_lightmap_uvs: mesh index out of range");
    const uint64_t want = (uint64_t)scene->mesh_tri_count[mesh_idx] * 3;
    if (uvs && num_corners != want)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "set_lightmap_uvs: " + std::to_string(num_corners) + " corners for a mesh of " + std::to_string(want));
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = flush_pending(ctx)) return rc;   // calls recorded so far see the previous set (no frame reads one: only the order is kept)
    DeviceBuffer fresh;
    if (uvs)
    {
        // (an empty mesh keeps a 16-byte set, so that "has a set" stays "has a buffer")
        HIP_TRY(DeviceBuffer::make(std::max<size_t>((size_t)want * sizeof(float2), 16), &fresh));
        if (want) HIP_TRY(hipMemcpyAsync(fresh.get(), uvs, (size_t)want * sizeof(float2), hipMemcpyHostToDevice, ctx->stream));
    }
    // every consumer of a set ends synchronised on the primary stream; the copy has landed and the old set is free to go
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    scene->lightmap_uvs[mesh_idx].swap(fresh);
    return LUPIN_OK;
}

int64_t lupin_hip_scene_mesh_triangle_count(const LupinScene *scene, uint32_t mesh_idx)
{
    if (!scene) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (mesh_idx >= scene->mesh_tri_count.size()) return fail(LUPIN_ERR_INVALID_ARGUMENT, "mesh index out of range");
    return (int64_t)scene->mesh_tri_count[mesh_idx];
}

// include/lupin_pack.hpp knows no HIP header and restates the two limits: here, where both are seen, they are held together
static_assert(lupin_pack::MAX_SIZE == LUPIN_LIGHTMAP_MAX_SIZE && lupin_pack::MAX_PADDING == LUPIN_UNWRAP_MAX_PADDING, "lupin_pack.hpp and lupin_hip.h disagree");
static_assert(LUPIN_LIGHTMAP_MAX_SIZE == 16384u && LUPIN_UNWRAP_MAX_PADDING == 16u, "the refusals' messages name 16384 and 16");

int lupin_hip_unwrap_lightmap_uvs(LupinContext *ctx, const LupinScene *scene, uint32_t mesh_idx, const LupinUnwrapDesc *desc, float *out_uvs,
                                  uint32_t *out_chart_of_tri, LupinUnwrapInfo *out_info)
{
    const char *who = "lupin_hip_unwrap_lightmap_uvs";
    if (int rc = query_refuse(ctx, scene, desc && out_uvs && out_info)) return rc;
    if (mesh_idx >= scene->mesh_tri_count.size()) return fail(LUPIN_ERR_INVALID_ARGUMENT, "mesh index out of range");
    if (const char *why = lupin_pack::unwrap_desc_refusal(desc->texel_size, desc->padding, desc->flags)) return fail(LUPIN_ERR_INVALID_ARGUMENT, why);
    if (int rc = query_flush(ctx)) return rc;
    if (int rc = join_primary(ctx)) return rc;
    hipStream_t st = ctx->stream;
    const uint32_t T = scene->mesh_tri_count[mesh_idx], V = scene->mesh_vert_count[mesh_idx], pad = desc->padding;
    LupinUnwrapInfo info = {0, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f};
    if (T == 0) { *out_info = info; return LUPIN_OK; }
    const uint32_t tri_offset = scene->mesh_tri_offset[mesh_idx];
    const TriVerts *tris = scene->dev.tris + tri_offset;
    const uint32_t *indices = scene->dev.tri_indices + (size_t)tri_offset * 3;
    const uint32_t blocks = (T + LP_BLOCK - 1) / LP_BLOCK;
    const size_t table_bytes = std::max<size_t>((size_t)6 * V * 4, 16);

    DeviceBuffer d_bucket, d_parent, d_table, d_label, d_roots, d_min, d_max, d_totals, d_dense, d_chart_label, d_chart_box, d_origin, d_uvs, d_chart;
    HIP_TRY(DeviceBuffer::make((size_t)T * 4, &d_bucket));
    HIP_TRY(DeviceBuffer::make((size_t)T * 4, &d_parent));
    HIP_TRY(DeviceBuffer::make(table_bytes, &d_table));
    HIP_TRY(DeviceBuffer::make((size_t)T * 4, &d_label));
    HIP_TRY(DeviceBuffer::make((size_t)T * 4, &d_roots));
    HIP_TRY(DeviceBuffer::make((size_t)T * 8, &d_min));
    HIP_TRY(DeviceBuffer::make((size_t)T * 8, &d_max));
    HIP_TRY(DeviceBuffer::make(((size_t)blocks + 1) * 4, &d_totals));
    HIP_TRY(DeviceBuffer::make((size_t)T * 4, &d_dense));
    HIP_TRY(DeviceBuffer::make((size_t)T * 24, &d_uvs));
    HIP_TRY(DeviceBuffer::make((size_t)T * 4, &d_chart));

    // ---- charts: classify, union, flatten (with the charts' boxes) ----
    auto t0 = LmClock::now();
    HIP_TRY(hipMemsetAsync(d_table.get(), 0xFF, table_bytes, st));
    HIP_TRY(hipMemsetAsync(d_min.get(), 0xFF, (size_t)T * 8, st));
    HIP_TRY(hipMemsetAsync(d_max.get(), 0, (size_t)T * 8, st));
    hipLaunchKernelGGL(k_uw_classify, dim3(blocks), dim3(LP_BLOCK), 0, st, tris, indices, T, V, d_bucket.as<uint32_t>(), d_parent.as<uint32_t>(),
                       d_table.as<uint32_t>());
    hipLaunchKernelGGL(k_uw_union, dim3(blocks), dim3(LP_BLOCK), 0, st, indices, T, V, d_bucket.as<uint32_t>(), d_table.as<uint32_t>(), d_parent.as<uint32_t>());
    hipLaunchKernelGGL(k_uw_flatten, dim3(blocks), dim3(LP_BLOCK), 0, st, tris, T, d_bucket.as<uint32_t>(), d_parent.as<uint32_t>(), d_label.as<uint32_t>(),
                       d_roots.as<uint32_t>(), d_min.as<uint32_t>(), d_max.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    info.charts_ms = lm_ms_since(t0);

    // ---- the charts in ascending label, their boxes to the host ----
    t0 = LmClock::now();
    hipLaunchKernelGGL(k_lm_count, dim3(blocks), dim3(LP_BLOCK), 0, st, d_roots.as<uint32_t>(), T, d_totals.as<uint32_t>());
    hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(LP_LM_SCAN_THREADS), 0, st, d_totals.as<uint32_t>(), blocks);
    HIP_TRY(hipGetLastError());
    uint32_t n = 0;
    HIP_TRY(hipMemcpyAsync(&n, d_totals.as<uint32_t>() + blocks, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n > T) return fail(LUPIN_ERR_HIP, std::string(who) + ": the compaction counted more charts than the mesh has triangles");
    std::vector<uint32_t> h_label(n);
    std::vector<float4> h_box(n);
    if (n != 0)
    {
        HIP_TRY(DeviceBuffer::make((size_t)n * 4, &d_chart_label));
        HIP_TRY(DeviceBuffer::make((size_t)n * 16, &d_chart_box));
        HIP_TRY(DeviceBuffer::make((size_t)n * 8, &d_origin));
        hipLaunchKernelGGL(k_uw_compact, dim3(blocks), dim3(LP_BLOCK), 0, st, T, d_roots.as<uint32_t>(), d_totals.as<uint32_t>(), d_min.as<uint32_t>(),
                           d_max.as<uint32_t>(), d_chart_label.as<uint32_t>(), d_chart_box.as<float4>(), d_dense.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h_label.data(), d_chart_label.get(), (size_t)n * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_box.data(), d_chart_box.get(), (size_t)n * 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    info.rects_ms = lm_ms_since(t0);

    // ---- the rectangles and the shelf packer, on the host ----
    t0 = LmClock::now();
    std::vector<lupin_pack::Rect> rects(n);
    for (uint32_t c = 0; c < n; c++)
    {
        uint32_t ew = 0, eh = 0;
        if (!lupin_pack::extent_texels(h_box[c].x, h_box[c].z, desc->texel_size, &ew) || !lupin_pack::extent_texels(h_box[c].y, h_box[c].w, desc->texel_size, &eh))
            return fail(LUPIN_ERR_INVALID_ARGUMENT, "chart " + std::to_string(c) + " is larger than 16384 texels: choose a larger texel_size");
        rects[c] = lupin_pack::Rect{ew + 2u * pad, eh + 2u * pad, c, 0u, 0u};   // (dense numbers ascend with the labels)
    }
    uint64_t AW = 0, AH = 0;
    lupin_pack::shelf_pack(rects, &AW, &AH);
    if (AW > LUPIN_LIGHTMAP_MAX_SIZE || AH > LUPIN_LIGHTMAP_MAX_SIZE)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "the mesh's atlas would be " + std::to_string(AW) + " x " + std::to_string(AH) + " texels, above 16384: choose a larger texel_size");
    std::vector<float2> h_origin(n);
    for (const lupin_pack::Rect &r : rects) h_origin[r.label] = make_float2((float)(r.x + pad), (float)(r.y + pad));
    info.pack_ms = lm_ms_since(t0);

    // ---- the UVs ----
    t0 = LmClock::now();
    if (n != 0) HIP_TRY(hipMemcpyAsync(d_origin.get(), h_origin.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_uw_uvs, dim3(blocks), dim3(LP_BLOCK), 0, st, tris, T, d_bucket.as<uint32_t>(), d_label.as<uint32_t>(), d_dense.as<uint32_t>(),
                       d_chart_box.as<float4>(), d_origin.as<float2>(), desc->texel_size, d_uvs.as<float2>(), d_chart.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    // staged, so that a failed copy leaves the outputs untouched
    std::vector<float> h_uvs((size_t)T * 6);
    std::vector<uint32_t> h_chart(T);
    HIP_TRY(hipMemcpyAsync(h_uvs.data(), d_uvs.get(), (size_t)T * 24, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_chart.data(), d_chart.get(), (size_t)T * 4, hipMemcpyDeviceToHost, st));
    if (int rc = query_end(ctx, who)) return rc;
    for (uint32_t t = 0; t < T; t++) info.degenerate_tris += h_chart[t] == LP_UW_NONE ? 1u : 0u;
    memcpy(out_uvs, h_uvs.data(), (size_t)T * 24);
    if (out_chart_of_tri) memcpy(out_chart_of_tri, h_chart.data(), (size_t)T * 4);
    info.num_charts = n;
    info.width = (uint32_t)AW;
    info.height = (uint32_t)AH;
    info.uvs_ms = lm_ms_since(t0);
    *out_info = info;
    return LUPIN_OK;
}

// ---- lightmap denoising (no reference counterpart; kernels and rule: lupin_lightmap_denoise.hpp) ----

static thread_local LupinLightmapDenoiseStats g_lightmap_denoise_stats = {0.0f, {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, 0.0f, 0.0f};
void lupin_hip_lightmap_denoise_stats(LupinLightmapDenoiseStats *out) { if (out) *out = g_lightmap_denoise_stats; }

// the launch shape of the filter's kernels: one thread per texel in 16 x 16 blocks, as lupin_hip_denoise
static dim3 lmd_grid(uint32_t W, uint32_t H) { return dim3((W + LP_DN_BX - 1) / LP_DN_BX, (H + LP_DN_BY - 1) / LP_DN_BY); }

int lupin_hip_denoise_lightmap(LupinContext *ctx, const LupinLightmapDenoiseDesc *desc, const float *rgba, const float *records, float *out_rgba)
{
    const char *who = "lupin_hip_denoise_lightmap";
    if (int rc = query_refuse_context(ctx, desc && rgba && records && out_rgba)) return rc;
    const uint32_t W = desc->width, H = desc->height;
    if (W == 0 || H == 0 || W > LUPIN_LIGHTMAP_MAX_SIZE || H > LUPIN_LIGHTMAP_MAX_SIZE)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "width and height must be in [1, 16384]");
    if (desc->passes == 0 || desc->passes > LUPIN_LIGHTMAP_DENOISE_MAX_PASSES) return fail(LUPIN_ERR_INVALID_ARGUMENT, "passes must be in [1, 8]");
    if (desc->normal_squarings > LUPIN_LIGHTMAP_DENOISE_MAX_SQUARINGS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "normal_squarings must be <= 7");
    if (desc->dilate > LUPIN_LIGHTMAP_MAX_DILATE) return fail(LUPIN_ERR_INVALID_ARGUMENT, "dilate must be <= 64");
    if (desc->flags & ~(uint32_t)LUPIN_LIGHTMAP_DENOISE_DEVICE_POINTERS) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown flag");
    if (!(std::isfinite(desc->max_stretch) && desc->max_stretch > 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "max_stretch must be finite and positive");
    const bool on_device = (desc->flags & LUPIN_LIGHTMAP_DENOISE_DEVICE_POINTERS) != 0;
    if (on_device && (((uintptr_t)rgba | (uintptr_t)records | (uintptr_t)out_rgba) & 15u))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "device pointers must be 16-byte aligned");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = join_primary(ctx)) return rc;   // recorded calls run first
    hipStream_t st = ctx->stream;   // the primary stream
    const auto t_call = std::chrono::steady_clock::now();

    const size_t texels = (size_t)W * H;   // <= 2^28
    const uint32_t passes = desc->passes, dilate = desc->dilate;
    size_t want[LupinContext::LMD_BUFFERS] = {};
    if (!on_device) { want[LupinContext::LMD_RGBA] = texels * 16; want[LupinContext::LMD_RECORDS] = texels * LUPIN_RAY_RECORD_FLOATS * 4; }
    want[LupinContext::LMD_IV0] = want[LupinContext::LMD_IV1] = want[LupinContext::LMD_G0] = texels * 16;
    want[LupinContext::LMD_G1] = texels * 8;
    want[LupinContext::LMD_FOOT] = texels * 4;
    if (dilate) want[LupinContext::LMD_FILLED0] = want[LupinContext::LMD_FILLED1] = texels;
    for (int k = 0; k < LupinContext::LMD_BUFFERS; k++)
        if (grow_buffer(&ctx->lmd[k], &ctx->lmd_bytes[k], want[k]) != hipSuccess)
        {
            (void)hipGetLastError();
            return fail(LUPIN_ERR_OUT_OF_MEMORY, std::string(who) + ": no device memory for the filter's scratch");
        }
    const float4 *d_rgba = reinterpret_cast<const float4 *>(rgba), *d_records = reinterpret_cast<const float4 *>(records);
    float4 *d_out = reinterpret_cast<float4 *>(out_rgba);
    if (!on_device)
    {
        HIP_TRY(hipMemcpyAsync(ctx->lmd[LupinContext::LMD_RGBA].get(), rgba, texels * 16, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(ctx->lmd[LupinContext::LMD_RECORDS].get(), records, texels * LUPIN_RAY_RECORD_FLOATS * 4, hipMemcpyHostToDevice, st));
        d_rgba = d_out = ctx->lmd[LupinContext::LMD_RGBA].as<float4>();   // the result lands where the input was: the filter may work in place
        d_records = ctx->lmd[LupinContext::LMD_RECORDS].as<float4>();
    }
    float4 *iv[2] = {ctx->lmd[LupinContext::LMD_IV0].as<float4>(), ctx->lmd[LupinContext::LMD_IV1].as<float4>()};
    uint8_t *filled[2] = {ctx->lmd[LupinContext::LMD_FILLED0].as<uint8_t>(), ctx->lmd[LupinContext::LMD_FILLED1].as<uint8_t>()};
    const float4 *g0 = ctx->lmd[LupinContext::LMD_G0].as<float4>();
    const float2 *g1 = ctx->lmd[LupinContext::LMD_G1].as<float2>();
    const float *foot = ctx->lmd[LupinContext::LMD_FOOT].as<float>();

    // events around the prep pass, every filter pass and the gutter passes together: passes + 3 of them
    hipEvent_t ev[LUPIN_LIGHTMAP_DENOISE_MAX_PASSES + 3];
    const uint32_t num_ev = passes + 3;
    for (uint32_t k = 0; k < num_ev; k++) ev[k] = get_event(ctx);
    struct Return { LupinContext *c; hipEvent_t *e; uint32_t n; ~Return() { for (uint32_t k = 0; k < n; k++) c->ev_pool.push_back(e[k]); } } give_back{ctx, ev, num_ev};
    HIP_TRY(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_lmd_prep, lmd_grid(W, H), dim3(LP_DN_BX, LP_DN_BY), 0, st, d_rgba, d_records, iv[0], const_cast<float4 *>(g0), const_cast<float2 *>(g1),
                       const_cast<float *>(foot), W, H);
    HIP_TRY(hipEventRecord(ev[1], st));
    const float stretch2 = desc->max_stretch * desc->max_stretch;
    for (uint32_t i = 0; i < passes; i++)
    {
        const int step = 1 << i;
        const float stretch = stretch2 * (float)(step * step);   // K_i
        const float4 *src = iv[i & 1];
        float4 *other = iv[(i + 1) & 1];
        auto launch = [&](auto kernel, float4 *dst, float4 *out, uint8_t *out_filled) {
            hipLaunchKernelGGL(kernel, lmd_grid(W, H), dim3(LP_DN_BX, LP_DN_BY), 0, st, src, dst, g0, g1, foot, d_rgba, out, out_filled, W, H, step, stretch,
                               desc->normal_squarings);
        };
        if (i + 1 < passes) launch(k_lmd_pass<false, false>, other, nullptr, nullptr);
        else if (dilate) launch(k_lmd_pass<true, true>, nullptr, other, filled[0]);   // the gutter passes start from the other plane
        else launch(k_lmd_pass<true, false>, nullptr, d_out, nullptr);
        HIP_TRY(hipEventRecord(ev[2 + i], st));
    }
    // the gutter passes ping-pong between the two (irradiance, variance) planes, which the filter no longer needs; the last lands in the output
    const uint32_t texel_blocks = (uint32_t)((texels + LP_BLOCK - 1) / LP_BLOCK);
    for (uint32_t pass = 0, cur = passes & 1; pass < dilate; pass++, cur ^= 1)
        hipLaunchKernelGGL(k_lm_dilate, dim3(texel_blocks), dim3(LP_BLOCK), 0, st, W, H, (const float4 *)iv[cur], (const uint8_t *)filled[pass & 1],
                           pass + 1 < dilate ? iv[cur ^ 1] : d_out, filled[(pass & 1) ^ 1]);
    HIP_TRY(hipEventRecord(ev[2 + passes], st));
    HIP_TRY(hipGetLastError());
    if (!on_device) HIP_TRY(hipMemcpyAsync(out_rgba, d_out, texels * 16, hipMemcpyDeviceToHost, st));
    if (int rc = query_end(ctx, who)) return rc;

    LupinLightmapDenoiseStats stats = {0.0f, {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, 0.0f, 0.0f};
    HIP_TRY(hipEventElapsedTime(&stats.prep_ms, ev[0], ev[1]));
    for (uint32_t i = 0; i < passes; i++) HIP_TRY(hipEventElapsedTime(&stats.pass_ms[i], ev[1 + i], ev[2 + i]));
    HIP_TRY(hipEventElapsedTime(&stats.dilate_ms, ev[1 + passes], ev[2 + passes]));
    stats.call_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_call).count();
    g_lightmap_denoise_stats = stats;
    return LUPIN_OK;
}

// ---- lightmap seam stitching (no reference counterpart; kernels and rule: lupin_lightmap_stitch.hpp) ----

static_assert(lupin_stitch::MAX_SIZE == LUPIN_LIGHTMAP_MAX_SIZE && lupin_stitch::MAX_ITERATIONS == LUPIN_LIGHTMAP_STITCH_MAX_ITERATIONS &&
                  lupin_stitch::DEVICE_POINTERS == LUPIN_LIGHTMAP_STITCH_DEVICE_POINTERS && LP_ST_MAX_EDGE_SAMPLES == LUPIN_LIGHTMAP_STITCH_MAX_EDGE_SAMPLES,
              "lupin_stitch_rules.hpp, lupin_lightmap_stitch.hpp and lupin_hip.h disagree");

static thread_local LupinLightmapStitchStats g_lightmap_stitch_stats = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
int lupin_hip_lightmap_stitch_stats(LupinLightmapStitchStats *out)
{
    if (!out) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    *out = g_lightmap_stitch_stats;
    return LUPIN_OK;
}

// the number of words of `plane` (n of them) that are not LP_LM_NO_OWNER, and in d_totals what the compaction kernels read
static int stitch_count(hipStream_t st, const uint32_t *plane, uint32_t n, DeviceBuffer *d_totals, uint32_t *count)
{
    const uint32_t blocks = (uint32_t)(((uint64_t)n + LP_BLOCK - 1) / LP_BLOCK);
    HIP_TRY(DeviceBuffer::make(((size_t)blocks + 1) * 4, d_totals));
    hipLaunchKernelGGL(k_lm_count, dim3(blocks), dim3(LP_BLOCK), 0, st, plane, n, d_totals->as<uint32_t>());
    hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(LP_LM_SCAN_THREADS), 0, st, d_totals->as<uint32_t>(), blocks);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(count, d_totals->as<uint32_t>() + blocks, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LUPIN_OK;
}

int lupin_hip_stitch_lightmap(LupinContext *ctx, const LupinScene *scene, const LupinLightmapStitchDesc *desc, const LupinLightmapChart *charts,
                              uint32_t num_charts, const float *rgba, float *out_rgba, LupinLightmapStitchInfo *out_info)
{
    const char *who = "lupin_hip_stitch_lightmap";
    if (int rc = query_refuse(ctx, scene, desc && charts && rgba && out_rgba)) return rc;
    if (num_charts == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "no charts");
    if (const char *why = lupin_stitch::desc_refusal(desc->width, desc->height, desc->iterations, desc->samples_per_texel, desc->lambda, desc->flags, desc->reserved))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, why);
    const bool on_device = (desc->flags & LUPIN_LIGHTMAP_STITCH_DEVICE_POINTERS) != 0;
    if (on_device && (((uintptr_t)rgba | (uintptr_t)out_rgba) & 15u)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "device pointers must be 16-byte aligned");
    std::vector<LmChartDev> h_charts;
    uint64_t total_keys = 0;
    if (int rc = lightmap_host_charts(scene, charts, num_charts, &h_charts, &total_keys)) return rc;
    if (!lupin_stitch::half_edges_ok(total_keys)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "the charts hold more than 2^32 - 2 half-edges");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = join_primary(ctx)) return rc;   // recorded calls run first
    hipStream_t st = ctx->stream;                // the primary stream
    const auto t_call = LmClock::now();

    const uint32_t W = desc->width, H = desc->height, texels = W * H;   // <= 2^28
    const float Wf = (float)W, Hf = (float)H;
    const uint32_t N = (uint32_t)(total_keys * 3);   // half-edges
    LupinLightmapStitchInfo info;
    memset(&info, 0, sizeof(info));
    LupinLightmapStitchStats stats = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};

    // host arrays are staged; the atlas the kernels read (d_in) and the one the result lands in (d_out) may be the same memory
    DeviceBuffer d_stage;
    const float4 *d_in = reinterpret_cast<const float4 *>(rgba);
    float4 *d_out = reinterpret_cast<float4 *>(out_rgba);
    if (!on_device)
    {
        HIP_TRY(DeviceBuffer::make((size_t)texels * 16, &d_stage));
        HIP_TRY(hipMemcpyAsync(d_stage.get(), rgba, (size_t)texels * 16, hipMemcpyHostToDevice, st));
        d_in = d_out = d_stage.as<float4>();
    }
    // how every path ends: out = in wherever the solver has not written, the call synchronised, the info and the stats out
    auto finish = [&](bool scattered) -> int {
        if (on_device) { if (d_out != d_in && !scattered) HIP_TRY(hipMemcpyAsync(d_out, d_in, (size_t)texels * 16, hipMemcpyDeviceToDevice, st)); }
        else if (scattered) HIP_TRY(hipMemcpyAsync(out_rgba, d_out, (size_t)texels * 16, hipMemcpyDeviceToHost, st));
        if (int rc = query_end(ctx, who)) return rc;
        if (!on_device && !scattered && out_rgba != rgba) memmove(out_rgba, rgba, (size_t)texels * 16);
        if (out_info) *out_info = info;
        stats.call_ms = lm_ms_since(t_call);
        g_lightmap_stitch_stats = stats;
        return LUPIN_OK;
    };
    if (N == 0) return finish(false);

    // ---- seam edges: keys, the two sorts, runs of exactly two, the seam test ----
    auto t0 = LmClock::now();
    DeviceBuffer d_charts, d_counters, d_partner, d_totals;
    uint32_t E = 0;
    uint32_t h_counters[LP_ST_COUNTERS] = {0u, 0u, 0u, 0u};
    const uint32_t h_blocks = (uint32_t)(((uint64_t)N + LP_BLOCK - 1) / LP_BLOCK);
    HIP_TRY(DeviceBuffer::make(h_charts.size() * sizeof(LmChartDev), &d_charts));
    HIP_TRY(DeviceBuffer::make(LP_ST_COUNTERS * 4, &d_counters));
    HIP_TRY(DeviceBuffer::make((size_t)N * 4, &d_partner));
    HIP_TRY(hipMemcpyAsync(d_charts.get(), h_charts.data(), h_charts.size() * sizeof(LmChartDev), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_counters.get(), 0, LP_ST_COUNTERS * 4, st));
    HIP_TRY(hipMemsetAsync(d_partner.get(), 0xFF, (size_t)N * 4, st));
    {
        DeviceBuffer d_keys, d_keys2, d_vals, d_vals2, d_ckeys, d_ckeys2;
        HIP_TRY(DeviceBuffer::make((size_t)N * 8, &d_keys));
        HIP_TRY(DeviceBuffer::make((size_t)N * 8, &d_keys2));
        HIP_TRY(DeviceBuffer::make((size_t)N * 4, &d_vals));
        HIP_TRY(DeviceBuffer::make((size_t)N * 4, &d_vals2));
        uint32_t max_verts = 1;
        for (const LupinLightmapChart *c = charts; c != charts + num_charts; c++)
            max_verts = std::max(max_verts, scene->mesh_vert_count[scene->host_instances[c->instance_idx].mesh_idx]);
        hipLaunchKernelGGL(k_st_keys, dim3(h_blocks), dim3(LP_BLOCK), 0, st, scene->dev, d_charts.as<LmChartDev>(), num_charts, N,
                           d_keys.as<unsigned long long>(), d_vals.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        if (int rc = lupin_internal_sort_pairs_u64(st, d_keys.as<unsigned long long>(), d_keys2.as<unsigned long long>(), d_vals.as<uint32_t>(), d_vals2.as<uint32_t>(), N,
                                 32 + lupin_stitch::bits_for(max_verts - 1u)))
            return rc;
        const uint32_t *sorted = d_vals2.as<uint32_t>();
        if (num_charts > 1)   // equal (min, max) of different charts are apart after a stable sort by chart
        {
            HIP_TRY(DeviceBuffer::make((size_t)N * 4, &d_ckeys));
            HIP_TRY(DeviceBuffer::make((size_t)N * 4, &d_ckeys2));
            hipLaunchKernelGGL(k_st_chart_keys, dim3(h_blocks), dim3(LP_BLOCK), 0, st, d_charts.as<LmChartDev>(), num_charts, N, d_vals2.as<uint32_t>(),
                               d_ckeys.as<uint32_t>());
            HIP_TRY(hipGetLastError());
            if (int rc = lupin_internal_sort_pairs_u32(st, d_ckeys.as<uint32_t>(), d_ckeys2.as<uint32_t>(), d_vals2.as<uint32_t>(), d_vals.as<uint32_t>(), N,
                                     lupin_stitch::bits_for(num_charts - 1u)))
                return rc;
            sorted = d_vals.as<uint32_t>();
        }
        hipLaunchKernelGGL(k_st_runs, dim3(h_blocks), dim3(LP_BLOCK), 0, st, scene->dev, d_charts.as<LmChartDev>(), num_charts, N, sorted, Wf, Hf,
                           d_partner.as<uint32_t>(), d_counters.as<uint32_t>());
        HIP_TRY(hipGetLastError());
        if (int rc = stitch_count(st, d_partner.as<uint32_t>(), N, &d_totals, &E)) return rc;
        HIP_TRY(hipMemcpyAsync(h_counters, d_counters.get(), sizeof(h_counters), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (E > N) return fail(LUPIN_ERR_HIP, std::string(who) + ": the compaction counted more seams than there are half-edges");
    info.seam_edges = E;
    info.non_manifold_edges = h_counters[LP_ST_NON_MANIFOLD];
    stats.edges_ms = lm_ms_since(t0);
    if (E == 0) return finish(false);

    // ---- sample pairs: the edges in ascending hA, their counts, the scan, the rows ----
    t0 = LmClock::now();
    DeviceBuffer d_edges, d_counts, d_offsets, d_row_wgt, d_inc_keys, d_inc_vals, d_inc_keys2, d_inc_vals2, d_col;
    HIP_TRY(DeviceBuffer::make((size_t)E * 32, &d_edges));
    HIP_TRY(DeviceBuffer::make(((size_t)E + 1) * 8, &d_counts));
    HIP_TRY(DeviceBuffer::make(((size_t)E + 1) * 8, &d_offsets));
    HIP_TRY(hipMemsetAsync(d_counts.get(), 0, ((size_t)E + 1) * 8, st));
    hipLaunchKernelGGL(k_st_edges, dim3(h_blocks), dim3(LP_BLOCK), 0, st, scene->dev, d_charts.as<LmChartDev>(), num_charts, N, d_partner.as<uint32_t>(),
                       d_totals.as<uint32_t>(), Wf, Hf, desc->samples_per_texel, d_edges.as<float4>(), d_counts.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    unsigned long long pairs64 = 0;
    if (int rc = lupin_internal_exclusive_sum_u64(st, d_counts.as<unsigned long long>(), d_offsets.as<unsigned long long>(), (size_t)E + 1)) return rc;
    HIP_TRY(hipMemcpyAsync(&pairs64, d_offsets.as<unsigned long long>() + E, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!lupin_stitch::pairs_ok(pairs64)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "the seams give more than 2^32 - 2 incidence entries (8 a sample pair)");
    const uint32_t P = (uint32_t)pairs64, n8 = 8u * P;   // P >= E >= 1
    const uint32_t p_blocks = (P + LP_BLOCK - 1) / LP_BLOCK, e_blocks = (uint32_t)(((uint64_t)n8 + LP_BLOCK - 1) / LP_BLOCK);
    for (DeviceBuffer *b : {&d_row_wgt, &d_inc_keys, &d_inc_vals, &d_inc_keys2, &d_inc_vals2, &d_col}) HIP_TRY(DeviceBuffer::make((size_t)n8 * 4, b));
    hipLaunchKernelGGL(k_st_pairs, dim3(p_blocks), dim3(LP_BLOCK), 0, st, d_in, W, H, d_edges.as<float4>(), d_offsets.as<unsigned long long>(), E, P,
                       d_row_wgt.as<float>(), d_inc_keys.as<uint32_t>(), d_inc_vals.as<uint32_t>(), d_counters.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_counters, d_counters.get(), sizeof(h_counters), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    info.sample_pairs = P;
    info.dropped_pairs = h_counters[LP_ST_DROPPED];
    stats.samples_ms = lm_ms_since(t0);

    // ---- incidence: (texel, 8 * pair + entry) sorted by texel, the active texels, the columns ----
    t0 = LmClock::now();
    uint32_t A = 0;
    DeviceBuffer d_totals2, d_act_texel, d_act_start, d_x0;
    if (int rc = lupin_internal_sort_pairs_u32(st, d_inc_keys.as<uint32_t>(), d_inc_keys2.as<uint32_t>(), d_inc_vals.as<uint32_t>(), d_inc_vals2.as<uint32_t>(), n8,
                             lupin_stitch::bits_for(texels)))
        return rc;
    uint32_t *heads = d_inc_keys.as<uint32_t>();   // (the unsorted keys are done with)
    hipLaunchKernelGGL(k_st_heads, dim3(e_blocks), dim3(LP_BLOCK), 0, st, d_inc_keys2.as<uint32_t>(), n8, texels, heads, d_counters.as<uint32_t>());
    HIP_TRY(hipGetLastError());
    if (int rc = stitch_count(st, heads, n8, &d_totals2, &A)) return rc;
    if (A > texels) return fail(LUPIN_ERR_HIP, std::string(who) + ": the compaction counted more active texels than the atlas has");
    info.active_texels = A;
    if (A == 0) { stats.incidence_ms = lm_ms_since(t0); return finish(false); }   // every pair was dropped
    const uint32_t a_blocks = (A + LP_BLOCK - 1) / LP_BLOCK;
    HIP_TRY(DeviceBuffer::make((size_t)A * 4, &d_act_texel));
    HIP_TRY(DeviceBuffer::make((size_t)A * 4, &d_act_start));
    HIP_TRY(DeviceBuffer::make((size_t)A * 16, &d_x0));
    hipLaunchKernelGGL(k_st_active, dim3(e_blocks), dim3(LP_BLOCK), 0, st, d_inc_keys2.as<uint32_t>(), n8, heads, d_totals2.as<uint32_t>(),
                       d_act_texel.as<uint32_t>(), d_act_start.as<uint32_t>());
    HIP_TRY(hipMemsetAsync(d_col.get(), 0, (size_t)n8 * 4, st));
    hipLaunchKernelGGL(k_st_columns, dim3(a_blocks), dim3(LP_BLOCK), 0, st, d_in, d_act_texel.as<uint32_t>(), d_act_start.as<uint32_t>(), A,
                       d_counters.as<uint32_t>(), d_inc_vals2.as<uint32_t>(), d_col.as<uint32_t>(), d_x0.as<float4>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    stats.incidence_ms = lm_ms_since(t0);

    // ---- the solve: no host round trip from here to the output ----
    t0 = LmClock::now();
    DeviceBuffer d_d, d_r, d_p, d_q, d_s, d_pp, d_ap, d_scalars;
    for (DeviceBuffer *b : {&d_d, &d_r, &d_p, &d_q}) HIP_TRY(DeviceBuffer::make((size_t)A * 16, b));
    HIP_TRY(DeviceBuffer::make((size_t)P * 16, &d_s));
    HIP_TRY(DeviceBuffer::make((size_t)p_blocks * 16, &d_pp));
    HIP_TRY(DeviceBuffer::make((size_t)a_blocks * 16, &d_ap));
    HIP_TRY(DeviceBuffer::make(sizeof(StScalars), &d_scalars));
    HIP_TRY(hipMemsetAsync(d_scalars.get(), 0, sizeof(StScalars), st));
    const float *wgt = d_row_wgt.as<float>();
    const uint32_t *col = d_col.as<uint32_t>(), *inc = d_inc_vals2.as<uint32_t>(), *start = d_act_start.as<uint32_t>(), *cnt = d_counters.as<uint32_t>();
    float4 *dd = d_d.as<float4>(), *r = d_r.as<float4>(), *p = d_p.as<float4>(), *q = d_q.as<float4>(), *s = d_s.as<float4>();
    float4 *pp = d_pp.as<float4>(), *ap = d_ap.as<float4>();
    StScalars *scal = d_scalars.as<StScalars>();
    const float lambda = desc->lambda;
    auto scalars = [&](uint32_t mode) { hipLaunchKernelGGL(k_st_scalars, dim3(1), dim3(64), 0, st, mode, (const float4 *)pp, p_blocks, (const float4 *)ap, a_blocks, scal); };
    hipLaunchKernelGGL(k_st_apply<true>, dim3(p_blocks), dim3(LP_BLOCK), 0, st, P, wgt, col, (const float4 *)d_x0.as<float4>(), s, pp);
    hipLaunchKernelGGL(k_st_adjoint<true>, dim3(a_blocks), dim3(LP_BLOCK), 0, st, A, start, cnt, inc, wgt, (const float4 *)s, lambda, r, p, dd, q, ap);
    scalars(LP_ST_INIT);
    for (uint32_t it = 0; it < desc->iterations; it++)
    {
        hipLaunchKernelGGL(k_st_apply<false>, dim3(p_blocks), dim3(LP_BLOCK), 0, st, P, wgt, col, (const float4 *)p, s, pp);
        hipLaunchKernelGGL(k_st_adjoint<false>, dim3(a_blocks), dim3(LP_BLOCK), 0, st, A, start, cnt, inc, wgt, (const float4 *)s, lambda, r, p, dd, q, ap);
        scalars(LP_ST_ALPHA);
        hipLaunchKernelGGL(k_st_update, dim3(a_blocks), dim3(LP_BLOCK), 0, st, A, (const StScalars *)scal, (const float4 *)p, (const float4 *)q, dd, r, ap);
        scalars(LP_ST_BETA);
        hipLaunchKernelGGL(k_st_direction, dim3(a_blocks), dim3(LP_BLOCK), 0, st, A, (const StScalars *)scal, (const float4 *)r, p);
    }
    float4 *x = q;   // (q is done with)
    hipLaunchKernelGGL(k_st_result, dim3(a_blocks), dim3(LP_BLOCK), 0, st, A, (const float4 *)d_x0.as<float4>(), (const float4 *)dd, x);
    hipLaunchKernelGGL(k_st_apply<true>, dim3(p_blocks), dim3(LP_BLOCK), 0, st, P, wgt, col, (const float4 *)x, s, pp);
    scalars(LP_ST_AFTER);
    const bool scatter = desc->iterations != 0;
    if (scatter)
    {
        if (d_out != d_in) HIP_TRY(hipMemcpyAsync(d_out, d_in, (size_t)texels * 16, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(k_st_scatter, dim3(a_blocks), dim3(LP_BLOCK), 0, st, A, d_act_texel.as<uint32_t>(), (const float4 *)x, reinterpret_cast<float *>(d_out));
    }
    HIP_TRY(hipGetLastError());
    StScalars h_scal;
    HIP_TRY(hipMemcpyAsync(&h_scal, d_scalars.get(), sizeof(StScalars), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    info.iterations = desc->iterations;
    info.energy_before[0] = h_scal.before.x; info.energy_before[1] = h_scal.before.y; info.energy_before[2] = h_scal.before.z;
    info.energy_after[0] = h_scal.after.x; info.energy_after[1] = h_scal.after.y; info.energy_after[2] = h_scal.after.z;
    stats.solve_ms = lm_ms_since(t0);
    return finish(scatter);
}

static int pack_common(LupinContext *ctx, const LupinTexture *tex, uint32_t tile_size, uint32_t rank, uint32_t world, void *packed, int unpack)
{
    if (!ctx || !tex || !packed || tile_size == 0 || world == 0 || rank >= world) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad pack arguments");
    return lupin_internal_tiles_copy(ctx, tex, packed, tile_size, rank, world, 0, unpack ? 1 : 0);
}
int lupin_hip_pack_tiles(LupinContext *ctx, const LupinTexture *tex, uint32_t tile_size, uint32_t rank, uint32_t world, void *device_dst, uint64_t *out_pixels)
{
    CTX_ALIVE_TRY(ctx);
    int rc = pack_common(ctx, tex, tile_size, rank, world, device_dst, 0);
    if (rc == LUPIN_OK && out_pixels) *out_pixels = lupin_hip_packed_tile_pixels(tex->width, tex->height, tile_size, rank, world);
    return rc;
}
int lupin_hip_unpack_tiles(LupinContext *ctx, LupinTexture *tex, uint32_t tile_size, uint32_t rank, uint32_t world, const void *device_src)
{
    CTX_ALIVE_TRY(ctx);
    return pack_common(ctx, tex, tile_size, rank, world, const_cast<void *>(device_src), 1);
}

int lupin_hip_unpack_gathered_tiles(LupinContext *ctx, LupinTexture *tex, uint32_t tile_size, uint32_t rank, uint32_t world,
                                    const void *device_gathered, uint64_t capacity_pixels)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !tex || !device_gathered || tile_size == 0 || world == 0 || rank >= world) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad unpack arguments");
    return lupin_internal_tiles_copy(ctx, tex, const_cast<void *>(device_gathered), tile_size, rank, world, capacity_pixels, 2);
}

int lupin_hip_tonemap_and_fit_aspect(LupinContext *ctx, const LupinTexture *src, uint8_t *dst_rgba8, uint32_t dst_width, uint32_t dst_height,
                                     const LupinTonemapDesc *desc)
{
    CTX_ALIVE_TRY(ctx);
    if (!ctx || !src || !dst_rgba8 || !desc || dst_width == 0 || dst_height == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad tonemap arguments");
    HIP_TRY(hipSetDevice(ctx->device));
    TonemapArgs a;
    memset(&a, 0, sizeof(a));
    a.src_w = src->width; a.src_h = src->height; a.dst_w = dst_width; a.dst_h = dst_height;
    if (desc->has_viewport) { a.vp_x = desc->viewport_x; a.vp_y = desc->viewport_y; a.vp_w = desc->viewport_w; a.vp_h = desc->viewport_h; }
    else { a.vp_x = 0.0f; a.vp_y = 0.0f; a.vp_w = (float)dst_width; a.vp_h = (float)dst_height; }
    if (!(a.vp_w > 0.0f) || !(a.vp_h > 0.0f) || !(a.vp_x >= 0.0f) || !(a.vp_y >= 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad viewport");
    const float src_aspect = (float)src->width / (float)src->height;      // tonemapping.rs:168-174
    const float dst_aspect = a.vp_w / a.vp_h;
    if (src_aspect > dst_aspect) { a.scale_x = 1.0f; a.scale_y = dst_aspect / src_aspect; }
    else { a.scale_x = src_aspect / dst_aspect; a.scale_y = 1.0f; }
    a.exposure = desc->exposure; a.filmic = desc->filmic ? 1u : 0u; a.srgb = desc->srgb ? 1u : 0u;
    // set_scissor_rect(viewport.x as u32, viewport.y as u32, viewport.w as u32, viewport.h as u32) (:217)
    a.sc_x0 = std::min((uint32_t)a.vp_x, dst_width); a.sc_y0 = std::min((uint32_t)a.vp_y, dst_height);
    a.sc_x1 = (uint32_t)std::min<uint64_t>((uint64_t)a.sc_x0 + (uint32_t)a.vp_w, dst_width);
    a.sc_y1 = (uint32_t)std::min<uint64_t>((uint64_t)a.sc_y0 + (uint32_t)a.vp_h, dst_height);

    const size_t bytes = (size_t)dst_width * dst_height * 4;
    DeviceArray<uint32_t> d;   // freed on every return: each path below ends synchronised or failed
    HIP_TRY(d.alloc((size_t)dst_width * dst_height));
    if (int rc = join_primary(ctx)) return rc;
    hipError_t e;
    if (desc->clear)   // LoadOp::Clear(0, 0, 0, 1) over the whole attachment
    {
        std::vector<uint32_t> clear_px((size_t)dst_width * dst_height, 0xFF000000u);
        e = hipMemcpyAsync(d, clear_px.data(), bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    }
    else e = hipMemcpyAsync(d, dst_rgba8, bytes, hipMemcpyHostToDevice, ctx->stream);   // LoadOp::Load
    if (e == hipSuccess && a.sc_x1 > a.sc_x0 && a.sc_y1 > a.sc_y0)
    {
        dim3 grid((a.sc_x1 - a.sc_x0 + LP_BLOCK - 1) / LP_BLOCK, a.sc_y1 - a.sc_y0, 1);
        hipLaunchKernelGGL(k_tonemap, grid, dim3(LP_BLOCK), 0, ctx->stream, a, src->data, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(dst_rgba8, d, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(LUPIN_ERR_HIP, hipGetErrorString(e));
    return LUPIN_OK;
}


// ---- denoising (denoising.rs:83-306; kernels and algorithm: lupin_denoise.hpp) ----

}  // extern "C"

struct LupinDenoiseResources
{
    LupinContext *ctx;
    int device;
    uint32_t width, height;
    DeviceArray<float4> iv[2];          // (irradiance rgb, variance) ping-pong
    DeviceArray<DenoiseGuide> guide;    // normalised normals + albedo, written by the prep pass
};

template <bool FINAL>
static void launch_denoise_iter(bool has_n, bool has_a, dim3 grid, dim3 block, hipStream_t st, const float4 *src, float4 *dst,
                                const DenoiseGuide *guide, const uint2 *color, uint2 *out, uint32_t W, uint32_t H, int step)
{
    if (has_n && has_a) hipLaunchKernelGGL((k_denoise_iter<FINAL, true, true>), grid, block, 0, st, src, dst, guide, color, out, W, H, step);
    else if (has_n) hipLaunchKernelGGL((k_denoise_iter<FINAL, true, false>), grid, block, 0, st, src, dst, guide, color, out, W, H, step);
    else if (has_a) hipLaunchKernelGGL((k_denoise_iter<FINAL, false, true>), grid, block, 0, st, src, dst, guide, color, out, W, H, step);
    else hipLaunchKernelGGL((k_denoise_iter<FINAL, false, false>), grid, block, 0, st, src, dst, guide, color, out, W, H, step);
}

extern "C" {

int lupin_hip_build_denoise_resources(LupinContext *ctx, uint32_t width, uint32_t height, LupinDenoiseResources **out)
{
    CTX_ALIVE_TRY(ctx);
    if (!out || width == 0 || height == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad denoise resources size");
    if ((uint64_t)width * height > 0xFFFFFFFFull / 2) return fail(LUPIN_ERR_INVALID_ARGUMENT, "denoise size too large");
    HIP_TRY(hipSetDevice(ctx->device));
    LupinDenoiseResources *r = new LupinDenoiseResources();
    r->ctx = ctx; r->device = ctx->device; r->width = width; r->height = height;
    const size_t px = (size_t)width * height;
    hipError_t e = r->iv[0].alloc(px);
    if (e == hipSuccess) e = r->iv[1].alloc(px);
    if (e == hipSuccess) e = r->guide.alloc(px);
    if (e != hipSuccess)
    {
        delete r;
        return fail(LUPIN_ERR_OUT_OF_MEMORY, hipGetErrorString(e));
    }
    *out = r;
    return LUPIN_OK;
}

void lupin_hip_destroy_denoise_resources(LupinDenoiseResources *res)
{
    if (!res) return;
    hipSetDevice(res->device);
    if (ctx_alive(res->ctx)) (void)sync_all(res->ctx);   // a destroyed context has drained its streams already; a batch that fails here is dropped
    delete res;   // frees its buffers: after the synchronisation above
}

int lupin_hip_denoise(LupinContext *ctx, LupinDenoiseResources *res, const LupinDenoiseDesc *desc)
{
    CTX_ALIVE_TRY(ctx);
    if (!res || !desc) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (res->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "denoise resources of another context");
    if (!desc->pathtrace_output || !desc->denoise_output) return fail(LUPIN_ERR_INVALID_ARGUMENT, "pathtrace_output and denoise_output are required");
    if (desc->quality > LUPIN_DENOISE_HIGH) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad denoise quality");
    const LupinTexture *texs[4] = {desc->pathtrace_output, desc->albedo, desc->normals, desc->denoise_output};
    for (const LupinTexture *t : texs)
    {
        if (!t) continue;
        if (t->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "texture of another or a destroyed context");
        // denoising.rs:227-236
        if (t->width != res->width || t->height != res->height) return fail(LUPIN_ERR_INVALID_ARGUMENT, "texture size differs from the denoise resources' size");
    }
    HIP_TRY(hipSetDevice(ctx->device));
    // the inputs may be targets of recorded pathtrace calls: run them, then order the filter after every frame in flight
    if (int rc = join_primary(ctx)) return rc;
    const uint32_t W = res->width, H = res->height;
    const dim3 block(LP_DN_BX, LP_DN_BY), grid((W + LP_DN_BX - 1) / LP_DN_BX, (H + LP_DN_BY - 1) / LP_DN_BY);
    const uint2 *color = (const uint2 *)desc->pathtrace_output->data;
    hipLaunchKernelGGL(k_denoise_prep, grid, block, 0, ctx->stream, color, desc->albedo ? (const uint2 *)desc->albedo->data : nullptr,
                       desc->normals ? (const uint2 *)desc->normals->data : nullptr, res->iv[0], res->guide, W, H);
    const int passes = 3 + (int)desc->quality;   // Low / Medium / High: 3 / 4 / 5
    const bool has_n = desc->normals != nullptr, has_a = desc->albedo != nullptr;
    for (int i = 0; i < passes; i++)
    {
        const float4 *src = res->iv[i & 1];
        if (i + 1 < passes)
            launch_denoise_iter<false>(has_n, has_a, grid, block, ctx->stream, src, res->iv[(i + 1) & 1], res->guide, color, nullptr, W, H, 1 << i);
        else
            launch_denoise_iter<true>(has_n, has_a, grid, block, ctx->stream, src, nullptr, res->guide, color,
                                      (uint2 *)desc->denoise_output->data, W, H, 1 << i);
    }
    HIP_TRY(hipGetLastError());
    desc->denoise_output->accum32_valid = false;
    return LUPIN_OK;
}

}  // extern "C"

// ---- adaptive sampling (no reference counterpart; kernels and rule: lupin_adaptive.hpp) ----

extern "C" {

static void launch_adaptive_reset(LupinContext *ctx, LupinAdaptiveResources *r)
{
    const size_t pixels = (size_t)r->dev.width * r->dev.height;   // >= the block count
    hipLaunchKernelGGL(k_adaptive_reset, dim3((uint32_t)((pixels + LP_BLOCK - 1) / LP_BLOCK)), dim3(LP_BLOCK), 0, ctx->stream, r->dev);
    r->calls = 0;
}

int lupin_hip_build_adaptive_resources(LupinContext *ctx, uint32_t width, uint32_t height, LupinAdaptiveResources **out)
{
    CTX_ALIVE_TRY(ctx);
    if (!out || width == 0 || height == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad adaptive resources size");
    if ((uint64_t)width * height > 0xFFFFFFFFull / 2) return fail(LUPIN_ERR_INVALID_ARGUMENT, "adaptive size too large");
    HIP_TRY(hipSetDevice(ctx->device));
    LupinAdaptiveResources *r = new LupinAdaptiveResources();
    r->ctx = ctx; r->device = ctx->device;
    AdaptiveDev &d = r->dev;
    d.width = width; d.height = height;
    d.blocks_x = (width + LP_AD_BLOCK - 1) / LP_AD_BLOCK; d.blocks_y = (height + LP_AD_BLOCK - 1) / LP_AD_BLOCK;
    const size_t px = (size_t)width * height, nb = (size_t)d.blocks_x * d.blocks_y;
    hipError_t e = device_view(&r->frames, px, &d.frames);
    if (e == hipSuccess) e = device_view(&r->moments, px, &d.moments);
    if (e == hipSuccess) e = device_view(&r->block_error, nb, &d.block_error);
    if (e == hipSuccess) e = device_view(&r->block_flags, nb, &d.block_flags);
    if (e == hipSuccess) e = device_view(&r->block_active, nb, &d.block_active);
    if (e == hipSuccess) e = device_view(&r->block_count, nb, &d.block_count);
    if (e == hipSuccess) e = device_view(&r->stats, 3, &d.stats);
    if (e != hipSuccess)
    {
        delete r;
        return fail(LUPIN_ERR_OUT_OF_MEMORY, hipGetErrorString(e));
    }
    launch_adaptive_reset(ctx, r);   // primary stream: every adaptive call waits for it (flush_pending)
    e = hipGetLastError();
    if (e != hipSuccess)
    {
        hipStreamSynchronize(ctx->stream);
        delete r;
        return fail(LUPIN_ERR_HIP, hipGetErrorString(e));
    }
    *out = r;
    return LUPIN_OK;
}

void lupin_hip_destroy_adaptive_resources(LupinAdaptiveResources *res)
{
    if (!res) return;
    hipSetDevice(res->device);
    if (ctx_alive(res->ctx)) (void)sync_all(res->ctx);   // a destroyed context has drained its streams already; a batch that fails here is dropped
    delete res;   // frees its buffers: after the synchronisation above
}

int lupin_hip_adaptive_reset(LupinContext *ctx, LupinAdaptiveResources *res)
{
    CTX_ALIVE_TRY(ctx);
    if (!res) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (res->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "adaptive resources of another context");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = join_primary(ctx)) return rc;   // after every frame enqueued so far (the latest adaptive call's update among them)
    launch_adaptive_reset(ctx, res);
    HIP_TRY(hipGetLastError());
    return LUPIN_OK;
}

int lupin_hip_pathtrace_scene_adaptive(LupinContext *ctx, const LupinPathtraceResources *res, const LupinScene *scene,
                                       LupinTexture *render_target, uint32_t pathtrace_type, const LupinPathtraceDesc *desc,
                                       LupinAdaptiveResources *ares, const LupinAdaptiveParams *params)
{
    CTX_ALIVE_TRY(ctx);
    if (!res || !scene || !render_target || !desc || !ares || !params) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (!desc->accum_params || !desc->accum_params->prev_frame)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "adaptive sampling needs accum_params.prev_frame (inactive pixels copy it)");
    const LupinTexture *prev = desc->accum_params->prev_frame;
    if (prev == render_target) return fail(LUPIN_ERR_SAME_TARGET, "render_target must differ from accum_params.prev_frame");
    if (desc->tile_params) return fail(LUPIN_ERR_INVALID_ARGUMENT, "adaptive sampling renders whole frames: tile_params must be NULL");
    if (ares->ctx != ctx || render_target->ctx != ctx || prev->ctx != ctx || res->ctx != ctx || scene->ctx != ctx)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "object of another or a destroyed context");
    if (render_target->width != ares->dev.width || render_target->height != ares->dev.height || prev->width != ares->dev.width ||
        prev->height != ares->dev.height)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "render_target, prev_frame and adaptive resources differ in size");
    if (!(params->threshold >= 0.0f)) return fail(LUPIN_ERR_INVALID_ARGUMENT, "threshold must be >= 0 (and not NaN)");
    if (pathtrace_type > LUPIN_PATHTRACE_DIRECT) return fail(LUPIN_ERR_INVALID_ARGUMENT, "unknown pathtrace_type");
    ares->dev.threshold = params->threshold;
    ares->dev.min_frames = params->min_frames;
    ares->dev.max_frames = params->max_frames;
    return pathtrace_impl(ctx, res, scene, render_target, pathtrace_type, desc, false, 0, 0, 1, -1, nullptr, ares);
}

int lupin_hip_adaptive_stats(LupinContext *ctx, const LupinAdaptiveResources *ares, LupinAdaptiveStats *out)
{
    CTX_ALIVE_TRY(ctx);
    if (!ares || !out) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (ares->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "adaptive resources of another context");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = join_primary(ctx)) return rc;
    unsigned long long s[3];
    HIP_TRY(hipMemcpyAsync(s, ares->dev.stats, sizeof(s), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    out->active_pixels = s[0];
    out->pixel_frames = s[1];
    out->calls = ares->calls;
    out->max_frames_taken = (uint32_t)s[2];
    return LUPIN_OK;
}

int lupin_hip_adaptive_download(LupinContext *ctx, const LupinAdaptiveResources *ares, uint32_t *frames, float *moments,
                                float *block_error, uint8_t *block_active)
{
    CTX_ALIVE_TRY(ctx);
    if (!ares) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (ares->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "adaptive resources of another context");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = join_primary(ctx)) return rc;
    const AdaptiveDev &d = ares->dev;
    const size_t px = (size_t)d.width * d.height, nb = (size_t)d.blocks_x * d.blocks_y;
    if (frames) HIP_TRY(hipMemcpyAsync(frames, d.frames, px * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (moments) HIP_TRY(hipMemcpyAsync(moments, d.moments, px * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
    if (block_error) HIP_TRY(hipMemcpyAsync(block_error, d.block_error, nb * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (block_active) HIP_TRY(hipMemcpyAsync(block_active, d.block_active, nb, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return LUPIN_OK;
}

}  // extern "C"

// ---- reprojection of the adaptive history (no reference counterpart; kernels and rule: lupin_reproject.hpp) ----

struct LupinReprojectResources
{
    LupinContext *ctx = nullptr;
    int device = 0;
    uint32_t width = 0, height = 0;
    ReprojectVis vis[2] = {};        // [cur] is written by a call's trace; [cur ^ 1] is the previous call's: the plain views the kernels get
    DeviceBuffer vis_inst[2], vis_tri[2], vis_uv[2], vis_depth[2];   // own what vis[k]'s pointers point to
    int cur = 0;
    DeviceArray<uint32_t> frames;    // the gather's output, swapped with the adaptive resources' arrays after it (swap_gathered)
    DeviceArray<float2> moments;
    bool prev_valid = false;
    LupinPushConstants prev_pc{};    // the previous call's camera
    LupinMat3x4 prev_cam_inv{};
    // previous local -> world rows of every instance: two pinned staging buffers used in turn (a call never waits for the
    // copy of the call before it) and their device copy, allocated by the first call, grown on demand
    PinnedBuffer h_rows[2];
    DeviceArray<float4> d_rows;
    uint32_t rows_capacity = 0;      // instances
    Event rows_copied[2];            // staging buffer k may be rewritten once rows_copied[k] has passed
    int rows_next = 0;
    // LUPIN_STATS_KERNEL_TIMING: events before the trace, between trace and gather, after the gather of the latest call
    Event ev[3];
    bool timed = false;              // the latest call recorded them
};

// The gathered counts and moments become the adaptive state and the old state becomes the next gather's output: the owners
// trade places and the adaptive kernels' view follows, here and nowhere else.
static void swap_gathered(LupinAdaptiveResources *ares, LupinReprojectResources *res)
{
    ares->frames.swap(res->frames); ares->moments.swap(res->moments);
    ares->dev.frames = ares->frames.as<uint32_t>(); ares->dev.moments = ares->moments.as<float2>();
}

extern "C" {

int lupin_hip_build_reproject_resources(LupinContext *ctx, uint32_t width, uint32_t height, LupinReprojectResources **out)
{
    CTX_ALIVE_TRY(ctx);
    if (!out || width == 0 || height == 0) return fail(LUPIN_ERR_INVALID_ARGUMENT, "bad reproject resources size");
    if ((uint64_t)width * height > 0xFFFFFFFFull / 2) return fail(LUPIN_ERR_INVALID_ARGUMENT, "reproject size too large");
    HIP_TRY(hipSetDevice(ctx->device));
    LupinReprojectResources *r = new LupinReprojectResources();
    r->ctx = ctx; r->device = ctx->device; r->width = width; r->height = height;
    const size_t px = (size_t)width * height;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; k++)
    {
        ReprojectVis &v = r->vis[k];
        e = device_view(&r->vis_inst[k], px, &v.inst);
        if (e == hipSuccess) e = device_view(&r->vis_tri[k], px, &v.tri);
        if (e == hipSuccess) e = device_view(&r->vis_uv[k], px, &v.uv);
        if (e == hipSuccess) e = device_view(&r->vis_depth[k], px, &v.depth);
        // a download before the first call reads misses, not uninitialised memory
        if (e == hipSuccess) e = hipMemsetAsync(v.inst, 0xFF, px * sizeof(uint32_t), ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(v.tri, 0, px * sizeof(uint32_t), ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(v.uv, 0, px * sizeof(float2), ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(v.depth, 0, px * sizeof(float), ctx->stream);
    }
    if (e == hipSuccess) e = r->frames.alloc(px);
    if (e == hipSuccess) e = r->moments.alloc(px);
    for (int k = 0; k < 2 && e == hipSuccess; k++) e = r->rows_copied[k].create(hipEventDisableTiming);
    for (int k = 0; k < 3 && e == hipSuccess; k++) e = r->ev[k].create();
    if (e != hipSuccess)
    {
        hipStreamSynchronize(ctx->stream);
        delete r;
        return fail(LUPIN_ERR_OUT_OF_MEMORY, hipGetErrorString(e));
    }
    *out = r;
    return LUPIN_OK;
}

void lupin_hip_destroy_reproject_resources(LupinReprojectResources *res)
{
    if (!res) return;
    hipSetDevice(res->device);
    if (ctx_alive(res->ctx)) (void)sync_all(res->ctx);   // a destroyed context has drained its streams already; a batch that fails here is dropped
    delete res;   // frees its buffers and events: after the synchronisation above
}

int lupin_hip_reproject_invalidate(LupinContext *ctx, LupinReprojectResources *res)
{
    CTX_ALIVE_TRY(ctx);
    if (!res) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (res->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "reproject resources of another context");
    res->prev_valid = false;   // host state only: the next call's gather is launched with prev_valid = 0
    return LUPIN_OK;
}

int lupin_hip_adaptive_reproject(LupinContext *ctx, LupinAdaptiveResources *ares, LupinReprojectResources *res, const LupinScene *scene,
                                 const LupinReprojectDesc *desc, const LupinTexture *history_in, LupinTexture *history_out)
{
    CTX_ALIVE_TRY(ctx);
    if (!ares || !res || !scene || !desc || !history_in || !history_out) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (ares->ctx != ctx || res->ctx != ctx || scene->ctx != ctx || history_in->ctx != ctx || history_out->ctx != ctx)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "object of another or a destroyed context");
    if (history_in == history_out) return fail(LUPIN_ERR_SAME_TARGET, "history_out must differ from history_in");
    const uint32_t W = res->width, H = res->height;
    if (ares->dev.width != W || ares->dev.height != H || history_in->width != W || history_in->height != H || history_out->width != W ||
        history_out->height != H)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "history_in, history_out, adaptive and reproject resources differ in size");
    if (!(desc->depth_tolerance >= 0.0f) || !std::isfinite(desc->depth_tolerance))
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "depth_tolerance must be finite and >= 0");
    if (!scene->has_sw_bvh) return fail(LUPIN_ERR_NO_SW_BVH, "no software BVH was built for this scene");
    const uint32_t ninst = scene->dev.num_instances;
    if (desc->prev_instance_transforms && desc->num_instances != ninst)
        return fail(LUPIN_ERR_INVALID_ARGUMENT, "prev_instance_transforms: " + std::to_string(desc->num_instances) + " transforms for " + std::to_string(ninst) + " instances");
    // previous local -> world of every instance: the inverse of its world -> local rows (Mat3x4::inverse, as the loaders use it)
    std::vector<float4> rows((size_t)ninst * 3u);
    for (uint32_t i = 0; i < ninst; i++)
    {
        LupinMat3x4 w2l, l2w;
        if (desc->prev_instance_transforms)
        {
            const float (*m)[4] = desc->prev_instance_transforms[i].m;
            for (int c = 0; c < 4; c++) for (int r = 0; r < 3; r++) w2l.m[c][r] = m[r][c];
        }
        else
        {
            const InstanceDev &in = scene->host_instances[i];
            const float4 rr[3] = {in.r0, in.r1, in.r2};
            for (int r = 0; r < 3; r++) { w2l.m[0][r] = rr[r].x; w2l.m[1][r] = rr[r].y; w2l.m[2][r] = rr[r].z; w2l.m[3][r] = rr[r].w; }
        }
        lupin_mat3x4_inverse(&w2l, &l2w);
        for (int r = 0; r < 3; r++)
        {
            rows[(size_t)i * 3 + r] = make_float4(l2w.m[0][r], l2w.m[1][r], l2w.m[2][r], l2w.m[3][r]);
            // a caller's transform must invert; the scene's own rows were accepted at upload (a singular one reprojects nowhere: NaN fails every tap)
            if (desc->prev_instance_transforms && !(std::isfinite(l2w.m[0][r]) && std::isfinite(l2w.m[1][r]) && std::isfinite(l2w.m[2][r]) && std::isfinite(l2w.m[3][r])))
                return fail(LUPIN_ERR_INVALID_ARGUMENT, "prev_instance_transforms[" + std::to_string(i) + "] has no finite inverse");
        }
    }
    HIP_TRY(hipSetDevice(ctx->device));
    TraversalLds t;
    if (int rc = traversal_lds(ctx, scene, scene->stack_entries, true, &t)) return rc;
    // history_in may be the target of recorded pathtrace calls: run them, then order the work after every frame in flight
    if (int rc = join_primary(ctx)) return rc;
    hipStream_t st = ctx->stream;
    if (ninst > res->rows_capacity)
    {
        // the first call allocates; only a later call with a scene of more instances finds buffers that an earlier call's
        // copy or gather may still read, and waits for them
        if (res->rows_capacity) HIP_TRY(hipStreamSynchronize(st));
        res->d_rows.reset();
        for (PinnedBuffer &h : res->h_rows) h.reset();
        res->rows_capacity = 0;
        HIP_TRY(res->d_rows.alloc((size_t)ninst * 3));
        for (PinnedBuffer &h : res->h_rows) HIP_TRY(PinnedBuffer::make((size_t)ninst * 3 * sizeof(float4), &h));
        res->rows_capacity = ninst;
    }
    float4 *out32 = nullptr;
    if (ctx->accum_mode == LUPIN_ACCUM_F32)
    {
        if (int rc = ensure_accum32(history_out, st)) return rc;
        out32 = history_out->accum32;
    }
    if (ninst)
    {
        const int k = res->rows_next;
        res->rows_next ^= 1;
        HIP_TRY(hipEventSynchronize(res->rows_copied[k]));   // the copy of the call before the previous one: passed unless three calls are in flight
        memcpy(res->h_rows[k].get(), rows.data(), rows.size() * sizeof(float4));
        HIP_TRY(hipMemcpyAsync(res->d_rows, res->h_rows[k].get(), rows.size() * sizeof(float4), hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(res->rows_copied[k], st));
    }
    res->timed = ctx->timing;

    // ---- step 1: the new view's visibility ----
    FrameParams fp;
    memset(&fp, 0, sizeof(fp));
    LupinPushConstants &pc = fp.pc;
    const LupinMat3x4 &ct = desc->camera_transform;
    set_camera_constants(pc, desc->camera_params, ct);   // the aperture travels along unread: the centre ray is a pinhole's
    pc.ray_epsilon = desc->ray_epsilon;
    fp.width = W; fp.height = H; fp.reg_w = W; fp.reg_h = H;
    LupinMat3x4 cam_inv;
    lupin_mat3x4_inverse(&ct, &cam_inv);
    const uint32_t n = W * H;
    const ReprojectVis cur = res->vis[res->cur], prev = res->vis[res->cur ^ 1];
    if (res->timed) hipEventRecord(res->ev[0], st);
    with_bool(t.geo, [&](auto G) {
        constexpr bool LDSGEO = decltype(G)::value;
        hipLaunchKernelGGL(k_reproject_trace<LDSGEO>, dim3((n + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), t.lds, st, scene->dev, fp, n, cam_inv, cur, t.stack_words);
    });

    if (res->timed) hipEventRecord(res->ev[1], st);

    // ---- step 2: gather the previous view's image and state ----
    ReprojectArgs a;
    memset(&a, 0, sizeof(a));
    a.width = W; a.height = H;
    a.prev_pc = res->prev_pc;
    a.prev_cam_inv = res->prev_cam_inv;
    a.prev_local_to_world = res->d_rows;
    a.tris = scene->dev.tris;
    a.depth_tolerance = desc->depth_tolerance;
    a.max_history = desc->max_history;
    a.prev_valid = res->prev_valid ? 1u : 0u;
    a.cur = cur; a.prev = prev;
    a.frames_in = ares->dev.frames; a.moments_in = ares->dev.moments;
    a.frames_out = res->frames; a.moments_out = res->moments;
    a.hist_in = (const uint2 *)history_in->data;
    a.hist_in32 = (history_in->accum32 && history_in->accum32_valid) ? history_in->accum32 : nullptr;
    a.hist_out = (uint2 *)history_out->data;
    a.hist_out32 = out32;
    hipLaunchKernelGGL(k_reproject_gather, dim3((W + LP_DN_BX - 1) / LP_DN_BX, (H + LP_DN_BY - 1) / LP_DN_BY), dim3(LP_DN_BX, LP_DN_BY), 0, st, a);
    if (res->timed) hipEventRecord(res->ev[2], st);

    // ---- step 3: the gathered counts and moments become the adaptive state; every block active; statistics ----
    swap_gathered(ares, res);
    const AdaptiveDev &ad = ares->dev;
    const uint32_t nblocks = ad.blocks_x * ad.blocks_y;
    HIP_TRY(hipMemsetAsync(ad.stats, 0, 3 * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_reproject_refresh, dim3((nblocks + LP_BLOCK / 64 - 1) / (LP_BLOCK / 64)), dim3(LP_BLOCK), 0, st, ad);
    hipLaunchKernelGGL(k_adaptive_mask, dim3((nblocks + LP_BLOCK - 1) / LP_BLOCK), dim3(LP_BLOCK), 0, st, ad);
    history_out->accum32_valid = out32 != nullptr;
    res->cur ^= 1;
    res->prev_pc = pc;
    res->prev_cam_inv = cam_inv;
    res->prev_valid = true;
    HIP_TRY(hipGetLastError());
    return LUPIN_OK;
}

int lupin_hip_reproject_timings(LupinContext *ctx, const LupinReprojectResources *res, float *trace_ms, float *gather_ms)
{
    CTX_ALIVE_TRY(ctx);
    if (!res || !trace_ms || !gather_ms) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (res->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "reproject resources of another context");
    if (!res->timed) return fail(LUPIN_ERR_INVALID_ARGUMENT, "the latest lupin_hip_adaptive_reproject did not run under LUPIN_STATS_KERNEL_TIMING");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(hipEventSynchronize(res->ev[2]));
    HIP_TRY(hipEventElapsedTime(trace_ms, res->ev[0], res->ev[1]));
    HIP_TRY(hipEventElapsedTime(gather_ms, res->ev[1], res->ev[2]));
    return LUPIN_OK;
}

int lupin_hip_reproject_download(LupinContext *ctx, const LupinReprojectResources *res, int which, uint32_t *inst, uint32_t *tri, float *uv,
                                 float *depth)
{
    CTX_ALIVE_TRY(ctx);
    if (!res) return fail(LUPIN_ERR_INVALID_ARGUMENT, "null argument");
    if (res->ctx != ctx) return fail(LUPIN_ERR_INVALID_ARGUMENT, "reproject resources of another context");
    if (which != 0 && which != 1) return fail(LUPIN_ERR_INVALID_ARGUMENT, "which: 0 = current, 1 = previous");
    HIP_TRY(hipSetDevice(ctx->device));
    if (int rc = join_primary(ctx)) return rc;
    // after a call the buffer its trace wrote is vis[cur ^ 1] (the roles were swapped): that is the current view's
    const ReprojectVis &v = res->vis[res->cur ^ 1 ^ which];
    const size_t px = (size_t)res->width * res->height;
    if (inst) HIP_TRY(hipMemcpyAsync(inst, v.inst, px * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (tri) HIP_TRY(hipMemcpyAsync(tri, v.tri, px * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    if (uv) HIP_TRY(hipMemcpyAsync(uv, v.uv, px * sizeof(float2), hipMemcpyDeviceToHost, ctx->stream));
    if (depth) HIP_TRY(hipMemcpyAsync(depth, v.depth, px * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return LUPIN_OK;
}

}  // extern "C"
