// Bitmap words and row codes shared by the scans that run over validity and
// segment-start bitmaps (fill.hip, ewm.hip): 64 rows of a bitmap at any bit
// offset, the code of the closest set bit, and the workgroup's exclusive
// running maximum of two codes per thread.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace plgpu {
namespace {

constexpr uint64_t kRevTop = 1ull << 62;  // backward codes: kRevTop - row

// 8-byte word k of a bitmap of nbytes bytes, zero past its end (a caller's
// bitmap need not be padded, nor 8-byte aligned).
__device__ __forceinline__ uint64_t fill_bitmap_word(const uint8_t* b, int64_t nbytes, int64_t k) {
    if (k * 8 >= nbytes) return 0ull;
    if ((k + 1) * 8 <= nbytes && ((uintptr_t)b & 7u) == 0) return ((const uint64_t*)b)[k];
    uint64_t v = 0;
    const int64_t hi = std::min<int64_t>((k + 1) * 8, nbytes);
    for (int64_t j = k * 8; j < hi; ++j) v |= (uint64_t)b[j] << (8 * (j - k * 8));
    return v;
}

// Bits [bit0, bit0 + 64) of the bitmap: a funnel shift of two words.
__device__ __forceinline__ uint64_t fill_bits64(const uint8_t* b, int64_t nbytes, int64_t bit0) {
    const int64_t k = bit0 >> 6;
    const int sh = (int)(bit0 & 63);
    const uint64_t lo = fill_bitmap_word(b, nbytes, k);
    if (sh == 0) return lo;
    const uint64_t hi = fill_bitmap_word(b, nbytes, k + 1);
    return (lo >> sh) | (hi << (64 - sh));
}

__device__ __forceinline__ uint64_t fill_lowmask(int64_t c) {
    return c >= 64 ? ~0ull : (c <= 0 ? 0ull : (1ull << c) - 1ull);
}

template <bool REV>
__device__ __forceinline__ uint64_t fill_row_code(int64_t row) {
    return REV ? kRevTop - (uint64_t)row : (uint64_t)row + 1ull;
}

// Code of the set bit of m (rows from r0) closest in the direction of the
// fill: find-last-set forward, find-first-set backward.  0: none.
template <bool REV>
__device__ __forceinline__ uint64_t fill_word_code(uint64_t m, int64_t r0) {
    if (m == 0ull) return 0ull;
    const int pos = REV ? __ffsll((unsigned long long)m) - 1 : 63 - __clzll((long long)m);
    return fill_row_code<REV>(r0 + pos);
}

__device__ __forceinline__ uint64_t fill_max(uint64_t a, uint64_t b) { return a > b ? a : b; }

// Exclusive running maximum of (a, b) over the workgroup's threads, in thread
// order.  wa / wb: one slot per wave.
__device__ __forceinline__ void fill_block_excl_max(uint64_t& a, uint64_t& b, uint64_t* wa, uint64_t* wb) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint64_t x = a, y = b;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint64_t xu = __shfl_up(x, off, 64), yu = __shfl_up(y, off, 64);
        if (lane >= off) {
            x = fill_max(x, xu);
            y = fill_max(y, yu);
        }
    }
    if (lane == 63) {
        wa[wid] = x;
        wb[wid] = y;
    }
    uint64_t px = __shfl_up(x, 1, 64), py = __shfl_up(y, 1, 64);
    if (lane == 0) {
        px = 0ull;
        py = 0ull;
    }
    __syncthreads();
    for (int w = 0; w < wid; ++w) {
        px = fill_max(px, wa[w]);
        py = fill_max(py, wb[w]);
    }
    __syncthreads();
    a = px;
    b = py;
}

}  // namespace
}  // namespace plgpu
