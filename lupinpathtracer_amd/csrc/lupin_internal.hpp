// Shared between the translation units of liblupin_hip.so (not part of the public ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <utility>
#include "../../include/lupin_hip.h"

// A scratch device allocation that lives as long as its holder: hipMalloc in make(), hipFree in the destructor.  Move-only.
class DeviceBuffer
{
    void *p_ = nullptr;

public:
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { std::swap(p_, o.p_); return *this; }   // o's destructor frees what this held
    ~DeviceBuffer() { if (p_) hipFree(p_); }
    // *out holds `bytes` of device memory, or stays as it was if the allocation fails
    static hipError_t make(size_t bytes, DeviceBuffer *out)
    {
        DeviceBuffer b;
        const hipError_t e = hipMalloc(&b.p_, bytes);
        if (e == hipSuccess) *out = std::move(b);
        return e;
    }
    void *get() const { return p_; }
    template <typename T> T *as() const { return static_cast<T *>(p_); }
};

struct LupinTexture
{
    LupinContext *ctx;
    int device;            // the context's device ordinal (valid after the context is gone: a texture may outlive it)
    uint32_t width, height;
    __half *data;          // Rgba16Float, row-major, row 0 = top
    float4 *accum32;       // f32 shadow (LUPIN_ACCUM_F32), allocated by the first frame rendered into it in that mode
    bool accum32_valid;    // the shadow holds the value `data` is the rounded view of
};

int lupin_internal_fail(int code, const char *msg);          // records the message lupin_hip_last_error() returns
bool lupin_internal_ctx_alive(const LupinContext *ctx);       // created by lupin_hip_create_context and not destroyed since
int lupin_internal_ctx_device(const LupinContext *ctx);
hipStream_t lupin_internal_ctx_stream(const LupinContext *ctx);   // the primary stream
void lupin_internal_join_primary(LupinContext *ctx);         // primary stream waits for the frames enqueued so far
int lupin_internal_sync_all(LupinContext *ctx);              // host waits for every lane
int lupin_internal_tiles_copy(LupinContext *ctx, const LupinTexture *tex, void *packed, uint32_t tile_size, uint32_t rank, uint32_t world,
                              uint64_t capacity_px, int mode);   // k_tiles_copy on the primary stream
// the two ends of build_tlas that lupin_build_tlas and the device builder share (builders.cpp)
int lupin_internal_tlas_leaves(const LupinInstance *instances, uint32_t num_instances, const float *model_aabbs, uint32_t num_meshes,
                               LupinTlasNode *out_leaves);   // LUPIN_OK | LUPIN_ERR_INVALID_ARGUMENT (mesh_idx out of range)
bool lupin_internal_tlas_leaves_finite(const LupinInstance *instances, const LupinTlasNode *leaves, uint32_t num_instances);   // transforms and world boxes
void lupin_internal_tlas_finish(LupinTlasNode *tlas, uint32_t len);   // reversal + child remap
