// The sorts and the scan of lightmap seam stitching: hipCUB's stable radix sort, the one the LBVH builder uses
// (lbvh.hip), and its exclusive sum.  Like the builders they are a translation unit of their own: the code object of
// lupin_hip.hip holds the project's own kernels only, which tools/isa_guard.py holds to zero scratch, while rocPRIM's
// onesweep kernels spill 80 bytes of registers.  Declared in lupin_internal.hpp.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdint>

#include "lupin_internal.hpp"

namespace {

template <typename Key>
int sort_pairs(hipStream_t st, const Key *keys, Key *keys_out, const uint32_t *vals, uint32_t *vals_out, size_t n, int end_bit)
{
    size_t temp_bytes = 0;
    DeviceBuffer d_temp;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, keys, keys_out, vals, vals_out, n, 0, end_bit, st));
    HIP_TRY(DeviceBuffer::make(std::max<size_t>(temp_bytes, 16), &d_temp));
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(d_temp.get(), temp_bytes, keys, keys_out, vals, vals_out, n, 0, end_bit, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the scratch goes when this returns)
    return LUPIN_OK;
}

}  // namespace

int lupin_internal_sort_pairs_u64(hipStream_t st, const unsigned long long *keys, unsigned long long *keys_out, const uint32_t *vals, uint32_t *vals_out,
                                  size_t n, int end_bit)
{
    return sort_pairs(st, keys, keys_out, vals, vals_out, n, end_bit);
}

int lupin_internal_sort_pairs_u32(hipStream_t st, const uint32_t *keys, uint32_t *keys_out, const uint32_t *vals, uint32_t *vals_out, size_t n, int end_bit)
{
    return sort_pairs(st, keys, keys_out, vals, vals_out, n, end_bit);
}

int lupin_internal_exclusive_sum_u64(hipStream_t st, const unsigned long long *in, unsigned long long *out, size_t n)
{
    size_t temp_bytes = 0;
    DeviceBuffer d_temp;
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, in, out, n, st));
    HIP_TRY(DeviceBuffer::make(std::max<size_t>(temp_bytes, 16), &d_temp));
    HIP_TRY(hipcub::DeviceScan::ExclusiveSum(d_temp.get(), temp_bytes, in, out, n, st));
    HIP_TRY(hipStreamSynchronize(st));
    return LUPIN_OK;
}
