// Shared between the translation units of liblupin_hip.so (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <string>
#include "../../include/lupin_hip.h"
#include "lupin_owned.hpp"

// Every allocation of the library has one of these owners (lupin_owned.hpp); only here are the four calls named.
struct HipStatus { using Error = hipError_t; static constexpr hipError_t success = hipSuccess; };
struct DeviceMemoryApi : HipStatus
{
    static hipError_t alloc(void **p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void *p) { hipFree(p); }
};
struct PinnedMemoryApi : HipStatus
{
    static hipError_t alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes); }
    static void free(void *p) { hipHostFree(p); }
};
using DeviceBuffer = Owned<DeviceMemoryApi>;
using PinnedBuffer = Owned<PinnedMemoryApi>;

// A DeviceBuffer that knows its element type: it converts to T * where a kernel launch or a copy takes one.
template <typename T> struct DeviceArray : DeviceBuffer
{
    hipError_t alloc(size_t count) { return DeviceBuffer::make(count * sizeof(T), this); }
    T *get() const { return as<T>(); }
    operator T *() const { return as<T>(); }
};

// *owner holds `count` elements of T and *view, the plain pointer of a kernel's argument struct, points to them, or both stay as they were
template <typename T> static inline hipError_t device_view(DeviceBuffer *owner, size_t count, T **view)
{
    const hipError_t e = DeviceBuffer::make(count * sizeof(T), owner);
    if (e == hipSuccess) *view = owner->as<T>();
    return e;
}

// An event whose whole life is inside one function or one resource object.
class Event
{
    hipEvent_t e_ = nullptr;

public:
    Event() = default;
    Event(const Event &) = delete;
    Event &operator=(const Event &) = delete;
    ~Event() { if (e_) hipEventDestroy(e_); }
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e_, flags); }
    operator hipEvent_t() const { return e_; }
};

struct LupinTexture
{
    LupinContext *ctx;
    int device;            // the context's device ordinal (valid after the context is gone: a texture may outlive it)
    uint32_t width, height;
    DeviceBuffer data_mem, accum32_mem;   // own what the two views below point to
    __half *data;          // Rgba16Float, row-major, row 0 = top
    float4 *accum32;       // f32 shadow (LUPIN_ACCUM_F32), made by ensure_accum32 for the first frame rendered into it in that mode
    bool accum32_valid;    // the shadow holds the value `data` is the rounded view of
};

int lupin_internal_fail(int code, const char *msg);          // records the message lupin_hip_last_error() returns
// the one error macro of the library's HIP calls: returns LUPIN_ERR_HIP with "<expression>: <HIP's error string>"
#define HIP_TRY(expr) do { hipError_t e__ = (expr); if (e__ != hipSuccess) return lupin_internal_fail(LUPIN_ERR_HIP, (std::string(#expr) + ": " + hipGetErrorString(e__)).c_str()); } while (0)
bool lupin_internal_ctx_alive(const LupinContext *ctx);       // created by lupin_hip_create_context and not destroyed since
int lupin_internal_ctx_device(const LupinContext *ctx);
hipStream_t lupin_internal_ctx_stream(const LupinContext *ctx);   // the primary stream
int lupin_internal_sync_all(LupinContext *ctx);              // recorded calls run (their error is returned, message in place), host waits for every lane
int lupin_internal_tiles_copy(LupinContext *ctx, const LupinTexture *tex, void *packed, uint32_t tile_size, uint32_t rank, uint32_t world,
                              uint64_t capacity_px, int mode);   // k_tiles_copy on the primary stream
// the two ends of build_tlas that lupin_build_tlas and the device builder share (builders.cpp)
int lupin_internal_tlas_leaves(const LupinInstance *instances, uint32_t num_instances, const float *model_aabbs, uint32_t num_meshes,
                               LupinTlasNode *out_leaves);   // LUPIN_OK | LUPIN_ERR_INVALID_ARGUMENT (mesh_idx out of range)
bool lupin_internal_tlas_leaves_finite(const LupinInstance *instances, const LupinTlasNode *leaves, uint32_t num_instances);   // transforms and world boxes
void lupin_internal_tlas_finish(LupinTlasNode *tlas, uint32_t len);   // reversal + child remap
// lightmap seam stitching's sorts and scan (lupin_stitch_sort.hip): hipCUB's stable radix sort of n (key, value) pairs on bits
// [0, end_bit) and its exclusive sum, on stream st, in scratch that lives for the call; each returns synchronised
int lupin_internal_sort_pairs_u64(hipStream_t st, const unsigned long long *keys, unsigned long long *keys_out, const uint32_t *vals, uint32_t *vals_out,
                                  size_t n, int end_bit);
int lupin_internal_sort_pairs_u32(hipStream_t st, const uint32_t *keys, uint32_t *keys_out, const uint32_t *vals, uint32_t *vals_out, size_t n, int end_bit);
int lupin_internal_exclusive_sum_u64(hipStream_t st, const unsigned long long *in, unsigned long long *out, size_t n);
