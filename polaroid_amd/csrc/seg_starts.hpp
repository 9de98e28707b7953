// A segment-start column (checked by seg_check, plgpu_internal.hpp) as 8-byte
// words from bit 0, for the kernels that read it so (rolling.hip,
// cumulative.hip), and the read of one such word.  fill.hip and ewm.hip read
// the bitmap at its own bit offset instead (fill_bits64, seg_scan.hpp).  The
// repack kernel is why this is a header of its own: only the files that
// include it carry the kernel.
#pragma once
#include <algorithm>

#include "plgpu_internal.hpp"

namespace plgpu {
namespace {

// Bits [off, off + n) of a Boolean column as words from bit 0.
__global__ __launch_bounds__(256) void seg_repack_kernel(DevCol c, int64_t n, uint64_t* __restrict__ out) {
    const int64_t words = (n + 63) / 64;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < words * 64;
         r += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t m = __ballot(r < n && dev_load(c, r) != 0);
        if ((threadIdx.x & 63) == 0) out[r >> 6] = m;
    }
}

// The bitmap of n rows as 8-byte words from bit 0: the column's own buffer
// where it is laid out so (as plgpu_segment_starts writes it), else a copy
// in `own`.
inline int seg_words(const plgpu_column* seg_starts, int64_t n, DevBuf<uint64_t>& own, const uint64_t** seg,
                     hipStream_t s) {
    const uintptr_t at = (uintptr_t)seg_starts->values + (uintptr_t)(seg_starts->offset / 8);
    if (seg_starts->offset % 8 == 0 && at % 8 == 0) {
        *seg = (const uint64_t*)at;
        return PLGPU_OK;
    }
    const int64_t words = (n + 63) / 64;
    const int rc = own.alloc((size_t)words * 8, s);
    if (rc) return rc;
    seg_repack_kernel<<<(unsigned)std::min<int64_t>((words * 64 + 255) / 256, 256 * 64), 256, 0, s>>>(
        dev_col(*seg_starts), n, own);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "segment starts");
    *seg = own;
    return PLGPU_OK;
}

// Word wi of those words; the last, partial one byte by byte (a caller's
// bitmap need not be padded): nbytes = ceil(n / 8).
__device__ __forceinline__ uint64_t seg_word(const uint64_t* seg, int64_t nbytes, int64_t wi) {
    if ((wi + 1) * 8 <= nbytes) return seg[wi];
    uint64_t v = 0;
    const uint8_t* b = (const uint8_t*)seg;
    for (int64_t j = wi * 8; j < nbytes; ++j) v |= (uint64_t)b[j] << (8 * (j - wi * 8));
    return v;
}

}  // namespace
}  // namespace plgpu
