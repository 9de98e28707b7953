// The core shared by the segmented scans (cumulative.hip, fill.hip, ewm.hip, rank.hip):
// the tile geometry, the segmented workgroup scan over an operator type, the
// totals launch's split of the tiles, the 16-byte load of a thread's rows, and
// the bitmap words and row codes of the scans that run over validity and
// segment-start bitmaps (fill.hip, ewm.hip, rank.hip).  Primitives only: each operator
// keeps its own reduce / totals / apply kernels, and the tails of the apply
// kernels stay written out there (profiles/seg_scan_isa.md says why).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

namespace plgpu {
namespace {

// ---------------------------------------------------------------- geometry
// A workgroup takes its tile as kTileBlocks block scans of kTileBlock rows one
// after the other; one more launch of a single workgroup scans the tiles'
// summaries.  (polaroid_amd/_native.py mirrors these as CUM_*.)
constexpr int kTileThreads = 256;
constexpr int kTilePer = 8;                           // consecutive rows per thread
constexpr int kTileBlock = kTileThreads * kTilePer;   // rows of one workgroup scan
constexpr int kTileBlocks = 8;                        // scans a workgroup runs one after the other
constexpr int kTileRows = kTileBlock * kTileBlocks;   // rows per workgroup
constexpr int kTileWords = kTileRows / 64;            // bitmap words of a tile: one per thread
constexpr int kTotalsThreads = 1024;
static_assert(kTileWords == kTileThreads, "one bitmap word per thread");

// The tiles [lo, hi) this thread of the totals launch folds.  (tiles by
// reference: the kernels read it from their parameter block at each use, and
// the compiler orders its loads by that.)
__device__ __forceinline__ void totals_span(const int64_t& tiles, int64_t& lo, int64_t& hi) {
    const int64_t per = (tiles + kTotalsThreads - 1) / kTotalsThreads;
    lo = std::min<int64_t>((int64_t)threadIdx.x * per, tiles);
    hi = std::min<int64_t>(lo + per, tiles);
}

// ------------------------------------------------------- the segmented scan
// Op: `using T`, `static T id()`, `static T comb(const T& l, const T& r)`
// (l, then r) and `static T shfl_up(const T& x, int off)`.

// (flag, value) (+) (flag, value): a segment start replaces the running value.
template <class Op>
__device__ __forceinline__ void seg_comb(bool& lf, typename Op::T& l, bool rf, const typename Op::T& r) {
    l = rf ? r : Op::comb(l, r);
    lf = lf || rf;
}

// Segmented scan of one (flag, value) per thread over the workgroup: the
// exclusive prefix of this thread in (ef, ev), the workgroup's total in
// (tf, tv).  wv / wf: one slot per wave.
template <class Op>
__device__ __forceinline__ void block_seg_scan(bool f, const typename Op::T& v, typename Op::T* wv, uint32_t* wf,
                                               bool& ef, typename Op::T& ev, bool& tf, typename Op::T& tv) {
    using T = typename Op::T;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    T x = v;
    uint32_t xf = f ? 1u : 0u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T y = Op::shfl_up(x, off);
        const uint32_t yf = __shfl_up(xf, off, 64);
        if (lane >= off) {
            if (!xf) x = Op::comb(y, x);
            xf |= yf;
        }
    }
    if (lane == 63) {
        wv[wid] = x;
        wf[wid] = xf;
    }
    T px = Op::shfl_up(x, 1);
    uint32_t pf = __shfl_up(xf, 1, 64);
    if (lane == 0) {
        px = Op::id();
        pf = 0u;
    }
    __syncthreads();
    ef = false;
    ev = Op::id();
    tf = false;
    tv = Op::id();
    for (int w = 0; w < nw; ++w) {
        if (w < wid) seg_comb<Op>(ef, ev, wf[w] != 0u, wv[w]);
        seg_comb<Op>(tf, tv, wf[w] != 0u, wv[w]);
    }
    seg_comb<Op>(ef, ev, pf != 0u, px);
    __syncthreads();
}

// ------------------------------------------------- a thread's kTilePer rows
// src[k] into x[k] by 16-byte loads: src is 16-byte aligned.
template <typename T>
using Rows16 = HIP_vector_type<T, 16 / sizeof(T)>;

template <typename T>
__device__ __forceinline__ void load_vec8(const T* src, T (&x)[kTilePer]) {
    const Rows16<T>* s = (const Rows16<T>*)src;
    if constexpr (sizeof(T) == 8) {
#pragma unroll
        for (int k = 0; k < kTilePer / 2; ++k) {
            const Rows16<T> q = s[k];
            x[2 * k] = q.x;
            x[2 * k + 1] = q.y;
        }
    } else {
        const Rows16<T> q0 = s[0], q1 = s[1];
        x[0] = q0.x; x[1] = q0.y; x[2] = q0.z; x[3] = q0.w;
        x[4] = q1.x; x[5] = q1.y; x[6] = q1.z; x[7] = q1.w;
    }
}

// ------------------------------------------------- bitmap words, row codes
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
