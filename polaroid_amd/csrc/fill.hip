// Forward / backward fill of the nulls of one column, plain or per segment
// (forward_fill / backward_fill / fill_null(strategy="forward" | "backward")).
//
// Reference (paths under the polars crates):
//   polars-core/src/chunked_array/ops/fill_null.rs:58 Series::fill_null, :130 /
//   :160 fill_forward_numeric / fill_backward_numeric, :258 / :304
//   fill_forward_gather_limit / fill_backward_gather_limit; over groups
//   polars-expr/src/expressions/window.rs:356 with GroupsToRows.
//
// MI355X design (DESIGN.md "Fill strategies"): the fill is a scan over bitmaps,
// and the values are touched once.  For row i the answer is j(i), the last row
// <= i whose validity bit is set, and s(i), the last row <= i whose
// segment-start bit is set; the row is filled iff j exists, j >= s(i) and
// i - j <= limit.  Both are plain running maxima of row indices, so no
// segmented operator is needed.  Rows are held as codes, 0 for none: row + 1
// forward; backward kRevTop - row, and the start bitmap is read one bit on (a
// set bit then marks the last row of a segment), so the closest row in the
// direction of the scan always has the largest code and both directions run
// the same maxima and the same test.
//
// Three launches, none of which waits on another workgroup:
// fill_reduce_kernel reads the bitmaps alone, one 64-row word per lane, and
// leaves two codes per tile of kTileRows rows; fill_totals_kernel (one
// workgroup) turns them into every tile's carry, an exclusive running maximum
// in the direction of the fill; fill_apply_kernel scans the per-word codes of
// its tile, adds the carry, and streams the values once: a null row that
// passes the test takes x[j] from the lane's own registers when j lies in the
// lane's rows, else by one load per lane (the line just streamed, or for a
// long run one address for the whole wave).  Values are moved as their bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "plgpu_internal.hpp"
#include "seg_scan.hpp"

namespace plgpu {
namespace {

struct FillParams {
    const void* values;      // the slice's first element is values[voff]
    int64_t voff;
    const uint8_t* valid;    // validity bitmap; row r is bit valid_off + r
    int64_t valid_off;
    int64_t valid_bytes;     // bytes of the bitmap that hold bits of the slice
    const uint8_t* seg;      // segment starts (nullptr: one segment), row r is bit seg_off + r
    int64_t seg_off;
    int64_t seg_bytes;
    int64_t n;
    uint64_t limit;          // largest distance filled
    void* out;
    uint8_t* out_valid;
    uint64_t* cj;            // per tile: code of its last valid row, then the carry
    uint64_t* cs;            // per tile: code of its last start, then the carry
    int64_t tiles;
};

// Validity bits V and segment bits S of rows [64 w, 64 w + 64), zero past the
// column.  Backward S: bit r set when row r + 1 starts a segment.
template <bool REV>
__device__ __forceinline__ void fill_words(const FillParams& p, int64_t w, bool seg, uint64_t& V, uint64_t& S) {
    const int64_t r0 = w * 64;
    V = 0ull;
    S = 0ull;
    if (r0 >= p.n) return;
    V = fill_bits64(p.valid, p.valid_bytes, p.valid_off + r0) & fill_lowmask(p.n - r0);
    if (seg) {
        if constexpr (REV) S = fill_bits64(p.seg, p.seg_bytes, p.seg_off + r0 + 1) & fill_lowmask(p.n - 1 - r0);
        else S = fill_bits64(p.seg, p.seg_bytes, p.seg_off + r0) & fill_lowmask(p.n - r0);
    }
}

template <bool REV>
__global__ __launch_bounds__(kTileThreads) void fill_reduce_kernel(FillParams p) {
    __shared__ uint64_t wa[kTileThreads / 64], wb[kTileThreads / 64];
    const int64_t tile = blockIdx.x;
    const int64_t w = tile * kTileWords + threadIdx.x;
    uint64_t V, S;
    fill_words<REV>(p, w, p.seg != nullptr, V, S);
    uint64_t a = fill_word_code<REV>(V, w * 64), b = fill_word_code<REV>(S, w * 64);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a = fill_max(a, __shfl_xor(a, off, 64));
        b = fill_max(b, __shfl_xor(b, off, 64));
    }
    if ((threadIdx.x & 63) == 0) {
        wa[threadIdx.x >> 6] = a;
        wb[threadIdx.x >> 6] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kTileThreads / 64; ++k) {
            a = fill_max(a, wa[k]);
            b = fill_max(b, wb[k]);
        }
        p.cj[tile] = a;
        p.cs[tile] = b;
    }
}

template <bool REV>
__global__ __launch_bounds__(kTotalsThreads) void fill_totals_kernel(FillParams p) {
    __shared__ uint64_t wa[kTotalsThreads / 64], wb[kTotalsThreads / 64];
    // position q of the scan is tile q forward, tile tiles - 1 - q backward
    int64_t lo, hi;
    totals_span(p.tiles, lo, hi);
    uint64_t a = 0ull, b = 0ull;
    for (int64_t q = lo; q < hi; ++q) {
        const int64_t t = REV ? p.tiles - 1 - q : q;
        a = fill_max(a, p.cj[t]);
        b = fill_max(b, p.cs[t]);
    }
    fill_block_excl_max(a, b, wa, wb);
    // the carry of a tile: the maximum of the tiles before it in scan order
    for (int64_t q = lo; q < hi; ++q) {
        const int64_t t = REV ? p.tiles - 1 - q : q;
        const uint64_t va = p.cj[t], vb = p.cs[t];
        p.cj[t] = a;
        p.cs[t] = b;
        a = fill_max(a, va);
        b = fill_max(b, vb);
    }
}

template <int BYTES, bool REV, bool SEG>
__global__ __launch_bounds__(kTileThreads) void fill_apply_kernel(FillParams p) {
    using T = typename std::conditional<BYTES == 8, uint64_t, uint32_t>::type;
    __shared__ uint64_t sV[kTileWords], sS[kTileWords], sJ[kTileWords], sT[kTileWords];
    __shared__ uint64_t wa[kTileThreads / 64], wb[kTileThreads / 64];
    const int64_t tile = blockIdx.x;
    const int t = threadIdx.x;
    {
        // the codes that enter every word of the tile: thread order is scan order
        const int wi = REV ? kTileWords - 1 - t : t;
        const int64_t w = tile * kTileWords + wi;
        uint64_t V, S;
        fill_words<REV>(p, w, SEG, V, S);
        uint64_t a = fill_word_code<REV>(V, w * 64), b = SEG ? fill_word_code<REV>(S, w * 64) : 0ull;
        fill_block_excl_max(a, b, wa, wb);
        sV[wi] = V;
        sS[wi] = S;
        sJ[wi] = fill_max(a, p.cj[tile]);
        sT[wi] = SEG ? fill_max(b, p.cs[tile]) : 0ull;
    }
    __syncthreads();
    const T* src = (const T*)p.values + p.voff;
    T* dst = (T*)p.out;
    const bool aligned = ((uintptr_t)src & 15u) == 0;
    const int64_t padded = (p.n + 63) / 64 * 64;
    for (int blk = 0; blk < kTileBlocks; ++blk) {
        const int64_t first = tile * kTileRows + (int64_t)blk * kTileBlock;
        if (first >= p.n) break;
        const int64_t base = first + (int64_t)t * kTilePer;
        if (base >= p.n) {  // the rest of the last validity word
            if (base < padded) p.out_valid[base >> 3] = 0;
            continue;
        }
        const int wi = blk * (kTileBlock / 64) + (t >> 3);
        const int b0 = (t & 7) * kTilePer;  // the thread's rows are bits b0 .. b0 + 7 of the word
        const uint64_t V = sV[wi], S = SEG ? sS[wi] : 0ull;
        const uint32_t vb = (uint32_t)(V >> b0) & 0xFFu, sb = (uint32_t)(S >> b0) & 0xFFu;
        (void)sb;
        const bool full = base + kTilePer <= p.n;
        T x[kTilePer];
        if (full && aligned) {
            load_vec8(src + base, x);
        } else {
#pragma unroll
            for (int k = 0; k < kTilePer; ++k) x[k] = base + k < p.n ? src[base + k] : (T)0;
        }
        uint32_t ob = vb;
        if (vb != 0xFFu) {
            // the codes that enter the thread's rows: the word's bits before
            // them in scan order, else the word's own entry codes
            uint64_t mj, ms;
            if constexpr (REV) {
                const uint64_t after = b0 + kTilePer == 64 ? 0ull : ~0ull << (b0 + kTilePer);
                mj = V & after;
                ms = S & after;
            } else {
                const uint64_t before = (1ull << b0) - 1ull;
                mj = V & before;
                ms = S & before;
            }
            const int64_t r0 = (tile * kTileWords + wi) * 64;
            uint64_t jc = mj ? fill_word_code<REV>(mj, r0) : sJ[wi];
            uint64_t sc = 0ull;
            if constexpr (SEG) sc = ms ? fill_word_code<REV>(ms, r0) : sT[wi];
            T val = (T)0;
            bool have = false;  // val holds x[j] of the row code jc
#pragma unroll
            for (int kk = 0; kk < kTilePer; ++kk) {
                const int k = REV ? kTilePer - 1 - kk : kk;
                const int64_t i = base + k;
                const uint64_t ic = fill_row_code<REV>(i);
                if constexpr (SEG) {
                    if ((sb >> k) & 1u) sc = ic;
                }
                if ((vb >> k) & 1u) {
                    jc = ic;
                    val = x[k];
                    have = true;
                } else if (i < p.n && jc != 0ull && jc >= sc && ic - jc <= p.limit) {
                    if (!have) {
                        const int64_t j = REV ? (int64_t)(kRevTop - jc) : (int64_t)(jc - 1ull);
                        val = src[j];
                        have = true;
                    }
                    x[k] = val;
                    ob |= 1u << k;
                }
            }
        }
        if (full) {  // an owned buffer, base a multiple of 8: 16-byte aligned
            if constexpr (BYTES == 8) {
                ulonglong2* d2 = (ulonglong2*)(dst + base);
#pragma unroll
                for (int k = 0; k < kTilePer / 2; ++k) d2[k] = make_ulonglong2(x[2 * k], x[2 * k + 1]);
            } else {
                uint4* d4 = (uint4*)(dst + base);
                d4[0] = make_uint4(x[0], x[1], x[2], x[3]);
                d4[1] = make_uint4(x[4], x[5], x[6], x[7]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kTilePer; ++k)
                if (base + k < p.n) dst[base + k] = x[k];
        }
        p.out_valid[base >> 3] = (uint8_t)ob;  // rows past the column: zero bits
    }
}

template <int BYTES, bool REV>
void fill_launch(const FillParams& p, hipStream_t s) {
    const unsigned g = (unsigned)p.tiles;
    {
        KtScope kt("fill_reduce_kernel", s);
        fill_reduce_kernel<REV><<<g, kTileThreads, 0, s>>>(p);
    }
    {
        KtScope kt("fill_totals_kernel", s);
        fill_totals_kernel<REV><<<1, kTotalsThreads, 0, s>>>(p);
    }
    {
        KtScope kt("fill_apply_kernel", s);
        if (p.seg) fill_apply_kernel<BYTES, REV, true><<<g, kTileThreads, 0, s>>>(p);
        else fill_apply_kernel<BYTES, REV, false><<<g, kTileThreads, 0, s>>>(p);
    }
}

}  // namespace
}  // namespace plgpu

using namespace plgpu;

PLGPU_API int plgpu_fill(const plgpu_column* values, const plgpu_column* seg_starts, int32_t kind, int64_t limit,
                         plgpu_column* out, void* stream) {
    hipStream_t s = as_stream(stream);
    if (values == nullptr || out == nullptr) return fail(PLGPU_ERR_INVALID, "NULL argument");
    std::memset(out, 0, sizeof *out);
    if (kind != PLGPU_FILL_FORWARD && kind != PLGPU_FILL_BACKWARD) return fail(PLGPU_ERR_INVALID, "unknown fill kind");
    if (seg_starts != nullptr) {
        const int rc = seg_check(values, seg_starts, PLGPU_ERR_INVALID, PLGPU_ERR_INVALID);
        if (rc) return rc;
    }
    const int eb = dtype_bytes(values->dtype);
    if (eb != 4 && eb != 8)
        return fail(PLGPU_ERR_SCHEMA, "forward / backward fill input must be a 4- or 8-byte numeric column");
    const int64_t n = values->length;
    const bool nullable = values->validity != nullptr;
    int rc = make_owned_column(out, values->dtype, n, nullable, s);
    if (rc || n == 0) return rc;
    hipError_t e = hipSuccess;
    if (!nullable) {
        // nothing to fill (the reference returns a clone at null_count == 0): the values, no launch
        e = hipMemcpyAsync((void*)out->values, (const uint8_t*)values->values + (size_t)values->offset * eb,
                           (size_t)n * eb, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            plgpu_column_release(out);
            return hip_fail(e, "fill");
        }
        return PLGPU_OK;
    }
    FillParams p;
    std::memset(&p, 0, sizeof p);
    p.values = values->values;
    p.voff = values->offset;
    p.valid = values->validity;
    p.valid_off = values->offset;
    p.valid_bytes = (values->offset + n + 7) / 8;
    if (seg_starts != nullptr) {
        p.seg = (const uint8_t*)seg_starts->values;
        p.seg_off = seg_starts->offset;
        p.seg_bytes = (seg_starts->offset + n + 7) / 8;
    }
    p.n = n;
    p.limit = limit < 0 ? (uint64_t)INT64_MAX : (uint64_t)limit;
    p.out = (void*)out->values;
    p.out_valid = (uint8_t*)out->validity;
    p.tiles = (n + kTileRows - 1) / kTileRows;
    DevBuf<uint64_t> carry;
    rc = carry.alloc((size_t)p.tiles * 8 * 2, s);
    if (!rc) {
        p.cj = carry;
        p.cs = p.cj + p.tiles;
        const bool rev = kind == PLGPU_FILL_BACKWARD;
        if (eb == 8) {
            if (rev) fill_launch<8, true>(p, s);
            else fill_launch<8, false>(p, s);
        } else {
            if (rev) fill_launch<4, true>(p, s);
            else fill_launch<4, false>(p, s);
        }
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "fill");
    }
    if (rc) plgpu_column_release(out);
    else out->null_count = -1;
    return rc;
}
