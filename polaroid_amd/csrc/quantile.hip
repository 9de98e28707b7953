// Quantiles of one column sorted within its segments, one per segment
// (median / quantile, plain, in group_by().agg() and over(keys)).
//
// Reference (paths under the polars crates):
//   polars-core/src/chunked_array/ops/aggregate/quantile.rs:16 quantile_idx,
//   :46 linear_interpol, :54 midpoint_interpol, :106 generic_quantile; over
//   groups polars-core/src/frame/group_by/aggregations/mod.rs:251
//   agg_quantile_generic (the GroupsType::Idx arm).
//
// MI355X design (DESIGN.md "Quantile"): the caller sorts by (group, value) with
// the value's nulls last (plgpu_arg_sort_multi), gathers and marks the segment
// starts (plgpu_segment_starts).  A quantile then reads one or two rows of its
// segment, so what is left is to find every segment's bounds and its non-null
// count from the two bitmaps.  For a segment of `len` rows of which `nc` are
// null, nn = len - nc > 0, all in f64:
//   float_idx = (nn - 1.0) * q + (double)nc       (this order, no fma)
//   nearest       idx = round(float_idx)          (halves away from zero)
//   equiprobable  idx = max(ceil(nn * q) - 1.0, 0.0) + nc
//   lower / midpoint / linear  idx = min((usize)float_idx, len - 1)
//   higher        idx = min((usize)ceil(float_idx), len - 1)
//   top_idx = (usize)ceil(float_idx)
// idx counts from the segment's first row with its nulls first; here the nulls
// are last, so the row read is start + (idx - nc).  nc stays in float_idx: the
// sum's rounding decides floor, round, ceil and the linear proportion.
//
// Four launches, none of which waits on another workgroup, no atomics.
// quantile_count_kernel reads the bitmaps alone, one 64-row word per thread,
// and leaves per tile of kTileRows rows its segment starts and how many of them
// sit on a null row (a segment whose first row is null holds no value);
// quantile_totals_kernel (one workgroup) turns the counts into every tile's
// first segment ordinal and the two totals, which the host reads to size the
// outputs; quantile_starts_kernel stores start[g] = j for every set bit j with
// ordinal g; quantile_apply_kernel, one lane per segment, finds nn by a binary
// search over the segment's validity bits (ones, then zeros), applies the rule
// for each of the nq quantiles and stores; the validity words of the outputs
// are one ballot per 64 segments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "plgpu_internal.hpp"
#include "seg_scan.hpp"

namespace plgpu {
namespace {

constexpr int kQuantileMax = 8;      // quantiles of one call
constexpr int kQuantileThreads = 256;  // segments per workgroup of the apply kernel

struct QuantileParams {
    const void* vals;      // the slice's first element
    const uint8_t* nv;     // validity of sorted_values (nullptr: no nulls); sorted row j is bit nv_off + j
    int64_t nv_off;
    int64_t nv_bytes;
    const uint8_t* seg;    // segment starts (nullptr: one segment); sorted row j is bit seg_off + j
    int64_t seg_off;
    int64_t seg_bytes;
    int64_t n;
    int64_t tiles;
    uint32_t* cnt;         // per tile: its segment starts (count), then its first segment's ordinal (totals)
    uint32_t* cnt_empty;   // per tile: its segment starts on a null row
    uint32_t* total;       // [0] segments, [1] segments without a value
    uint32_t* start;       // G + 1 entries: the first row of segment g; start[G] = n
    int64_t groups;        // G (starts and apply kernels)
    double* out[kQuantileMax];
    uint64_t* out_valid[kQuantileMax];  // whole 8-byte words (make_owned_column); nullptr: no segment is empty
    double q[kQuantileMax];
    int32_t method[kQuantileMax];
    int32_t nq;
};

// Segment-start bits S and validity bits V of sorted rows [64 w, 64 w + 64),
// zero past the column.  Row 0 starts a segment whatever the caller's bitmap says.
__device__ __forceinline__ void quantile_words(const QuantileParams& p, int64_t w, uint64_t& S, uint64_t& V) {
    const int64_t r0 = w * 64;
    S = 0ull;
    V = 0ull;
    if (r0 >= p.n) return;
    const uint64_t m = fill_lowmask(p.n - r0);
    if (p.seg != nullptr) S = fill_bits64(p.seg, p.seg_bytes, p.seg_off + r0) & m;
    if (w == 0) S |= 1ull;
    V = p.nv != nullptr ? fill_bits64(p.nv, p.nv_bytes, p.nv_off + r0) & m : m;
}

// Exclusive running sums of (a, b) over the workgroup's threads, in thread
// order, and the workgroup's totals.  wa / wb: one slot per wave.
__device__ __forceinline__ void quantile_block_excl_sum(uint32_t& a, uint32_t& b, uint32_t& ta, uint32_t& tb,
                                                        uint32_t* wa, uint32_t* wb) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    uint32_t x = a, y = b;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t xu = __shfl_up(x, off, 64), yu = __shfl_up(y, off, 64);
        if (lane >= off) {
            x += xu;
            y += yu;
        }
    }
    if (lane == 63) {
        wa[wid] = x;
        wb[wid] = y;
    }
    uint32_t px = x - a, py = y - b;
    __syncthreads();
    ta = 0u;
    tb = 0u;
    for (int w = 0; w < nw; ++w) {
        if (w < wid) {
            px += wa[w];
            py += wb[w];
        }
        ta += wa[w];
        tb += wb[w];
    }
    __syncthreads();
    a = px;
    b = py;
}

__global__ __launch_bounds__(kTileThreads) void quantile_count_kernel(QuantileParams p) {
    __shared__ uint32_t wa[kTileThreads / 64], wb[kTileThreads / 64];
    const int64_t tile = blockIdx.x;
    uint64_t S, V;
    quantile_words(p, tile * kTileWords + threadIdx.x, S, V);
    uint32_t a = (uint32_t)__popcll(S), b = (uint32_t)__popcll(S & ~V), ta, tb;
    quantile_block_excl_sum(a, b, ta, tb, wa, wb);
    if (threadIdx.x == 0) {
        p.cnt[tile] = ta;
        p.cnt_empty[tile] = tb;
    }
}

__global__ __launch_bounds__(kTotalsThreads) void quantile_totals_kernel(QuantileParams p) {
    __shared__ uint32_t wa[kTotalsThreads / 64], wb[kTotalsThreads / 64];
    int64_t lo, hi;
    totals_span(p.tiles, lo, hi);
    uint32_t a = 0u, b = 0u, ta, tb;
    for (int64_t t = lo; t < hi; ++t) {
        a += p.cnt[t];
        b += p.cnt_empty[t];
    }
    quantile_block_excl_sum(a, b, ta, tb, wa, wb);
    // the first segment ordinal of a tile: the segment starts of the tiles before it
    for (int64_t t = lo; t < hi; ++t) {
        const uint32_t c = p.cnt[t];
        p.cnt[t] = a;
        a += c;
    }
    if (threadIdx.x == 0) {
        p.total[0] = ta;
        p.total[1] = tb;
    }
}

__global__ __launch_bounds__(kTileThreads) void quantile_starts_kernel(QuantileParams p) {
    __shared__ uint32_t wa[kTileThreads / 64], wb[kTileThreads / 64];
    const int64_t tile = blockIdx.x;
    const int64_t w = tile * kTileWords + threadIdx.x;
    uint64_t S, V;
    quantile_words(p, w, S, V);
    uint32_t a = (uint32_t)__popcll(S), b = 0u, ta, tb;
    quantile_block_excl_sum(a, b, ta, tb, wa, wb);
    int64_t g = (int64_t)p.cnt[tile] + a;
    const int64_t r0 = w * 64;
    while (S != 0ull) {
        const int pos = __ffsll((unsigned long long)S) - 1;
        S &= S - 1ull;
        // (an ordinal past the total would come from bitmaps that changed between the launches: never stored)
        if (g < p.groups) p.start[g] = (uint32_t)(r0 + pos);
        ++g;
    }
    if (tile == 0 && threadIdx.x == 0) p.start[p.groups] = (uint32_t)p.n;
}

__device__ __forceinline__ bool quantile_bit(const uint8_t* b, int64_t bit) {
    return (b[bit >> 3] >> (bit & 7)) & 1u;
}

template <typename T>
__global__ __launch_bounds__(kQuantileThreads) void quantile_apply_kernel(QuantileParams p) {
    const int64_t g = (int64_t)blockIdx.x * kQuantileThreads + threadIdx.x;
    const bool live = g < p.groups;
    int64_t s = 0, nn = 0, len = 0;
    if (live) {
        int64_t e = p.n;
        if (p.start != nullptr) {
            s = p.start[g];
            e = p.start[g + 1];
        }
        // (bounds a caller's changed bitmaps cannot move out of the column)
        e = std::min<int64_t>(std::max<int64_t>(e, 0), p.n);
        s = std::min<int64_t>(std::max<int64_t>(s, 0), e);
        len = e - s;
        nn = len;
        if (p.nv != nullptr) {
            // the first row of [s, e) whose bit is clear: the bits are ones, then zeros
            int64_t lo = s, hi = e;
            while (lo < hi) {
                const int64_t mid = lo + ((hi - lo) >> 1);
                if (quantile_bit(p.nv, p.nv_off + mid)) lo = mid + 1;
                else hi = mid;
            }
            nn = lo - s;
        }
    }
    const bool valid = live && nn > 0;
    const uint64_t word = __ballot(valid);
    const T* v = (const T*)p.vals;
    for (int i = 0; i < p.nq; ++i) {
        double r = 0.0;
        if (valid) {
            const double q = p.q[i];
            const int32_t m = p.method[i];
            const int64_t nc = len - nn;
            const double nnf = (double)nn;
            const double fi = (nnf - 1.0) * q + (double)nc;
            uint64_t idx;
            bool interp = false;
            if (m == PLGPU_QUANTILE_NEAREST) {
                idx = (uint64_t)round(fi);
            } else if (m == PLGPU_QUANTILE_EQUIPROBABLE) {
                idx = (uint64_t)fmax(ceil(nnf * q) - 1.0, 0.0) + (uint64_t)nc;
            } else {
                idx = m == PLGPU_QUANTILE_HIGHER ? (uint64_t)ceil(fi) : (uint64_t)fi;
                idx = std::min<uint64_t>(idx, (uint64_t)(len - 1));
                interp = (m == PLGPU_QUANTILE_MIDPOINT || m == PLGPU_QUANTILE_LINEAR) && (uint64_t)ceil(fi) != idx;
            }
            // the row of the segment's non-null values: idx counts the nulls first
            int64_t row = (int64_t)idx - nc;
            row = std::min<int64_t>(std::max<int64_t>(row, 0), nn - 1);
            const double lower = (double)v[s + row];
            r = lower;
            if (interp && row + 1 < nn) {
                const double upper = (double)v[s + row + 1];
                if (!(lower == upper)) {
                    if (m == PLGPU_QUANTILE_MIDPOINT) r = (lower + upper) / 2.0;
                    else r = (fi - (double)idx) * (upper - lower) + lower;
                }
            }
        }
        if (live) p.out[i][g] = r;
        if (p.out_valid[i] != nullptr && (threadIdx.x & 63) == 0 && live) p.out_valid[i][g >> 6] = word;
    }
}

template <typename T>
void quantile_apply_launch(const QuantileParams& p, hipStream_t s) {
    KtScope kt("quantile_apply_kernel", s);
    quantile_apply_kernel<T><<<(unsigned)((p.groups + kQuantileThreads - 1) / kQuantileThreads), kQuantileThreads, 0,
                               s>>>(p);
}

}  // namespace
}  // namespace plgpu

using namespace plgpu;

PLGPU_API int plgpu_segment_quantile(const plgpu_column* sorted_values, const plgpu_column* seg_starts,
                                     const double* quantiles, const int32_t* methods, int32_t nq,
                                     plgpu_column* outs, void* stream) {
    hipStream_t s = as_stream(stream);
    if (sorted_values == nullptr || quantiles == nullptr || methods == nullptr || outs == nullptr)
        return fail(PLGPU_ERR_INVALID, "NULL argument");
    if (nq < 1 || nq > kQuantileMax) return fail(PLGPU_ERR_INVALID, "quantile: between 1 and 8 quantiles per call");
    std::memset(outs, 0, sizeof *outs * (size_t)nq);
    for (int i = 0; i < nq; ++i) {
        if (!(quantiles[i] >= 0.0 && quantiles[i] <= 1.0))
            return fail(PLGPU_ERR_INVALID, "`quantile` should be between 0.0 and 1.0");
        if (methods[i] < PLGPU_QUANTILE_NEAREST || methods[i] > PLGPU_QUANTILE_EQUIPROBABLE)
            return fail(PLGPU_ERR_INVALID, "unknown quantile method");
    }
    const int32_t dt = sorted_values->dtype;
    if (dt != PLGPU_I32 && dt != PLGPU_I64 && dt != PLGPU_U32 && dt != PLGPU_F64)
        return fail(PLGPU_ERR_INVALID, "quantile: the sorted values must be Int32, Int64, UInt32 or Float64");
    const int64_t n = sorted_values->length;
    if (seg_starts != nullptr) {
        if (seg_starts->dtype != PLGPU_BOOL || seg_starts->validity != nullptr)
            return fail(PLGPU_ERR_INVALID, "quantile: segment starts must be a null-free Boolean column");
        if (seg_starts->length != n)
            return fail(PLGPU_ERR_INVALID, "quantile: segment starts and values must have equal lengths");
    }
    if (n < 0 || n > (int64_t)UINT32_MAX) return fail(PLGPU_ERR_INVALID, "quantile: more rows than a UInt32 row id counts");

    QuantileParams p;
    std::memset(&p, 0, sizeof p);
    p.vals = (const uint8_t*)sorted_values->values + sorted_values->offset * dtype_bytes(dt);
    p.nv = sorted_values->validity;
    p.nv_off = sorted_values->offset;
    p.nv_bytes = (sorted_values->offset + n + 7) / 8;
    if (seg_starts != nullptr) {
        p.seg = (const uint8_t*)seg_starts->values;
        p.seg_off = seg_starts->offset;
        p.seg_bytes = (seg_starts->offset + n + 7) / 8;
    }
    p.n = n;
    p.tiles = (n + kTileRows - 1) / kTileRows;
    p.nq = nq;
    for (int i = 0; i < nq; ++i) {
        p.q[i] = quantiles[i];
        p.method[i] = methods[i];
    }

    int rc = PLGPU_OK;
    int64_t groups = 0;
    uint32_t totals[2] = {0u, 0u};
    DevBuf<uint32_t> carry, start;
    if (n == 0) {
        // the plain reduction of an empty column is one null row; no segments otherwise
        groups = seg_starts == nullptr ? 1 : 0;
        totals[1] = (uint32_t)groups;
    } else {
        rc = carry.alloc(((size_t)p.tiles * 2 + 2) * sizeof(uint32_t), s);
        if (rc) return rc;
        p.cnt = carry;
        p.cnt_empty = p.cnt + p.tiles;
        p.total = p.cnt_empty + p.tiles;
        {
            KtScope kt("quantile_count_kernel", s);
            quantile_count_kernel<<<(unsigned)p.tiles, kTileThreads, 0, s>>>(p);
        }
        {
            KtScope kt("quantile_totals_kernel", s);
            quantile_totals_kernel<<<1, kTotalsThreads, 0, s>>>(p);
        }
        hipError_t e = hipGetLastError();
        // the one device-to-host copy: it sizes the outputs
        if (e == hipSuccess) e = hipMemcpyAsync(totals, p.total, sizeof totals, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "quantile");
        groups = totals[0];
        if (groups < 1 || groups > n || (int64_t)totals[1] > groups)
            return fail(PLGPU_ERR_HIP, "quantile: the segment count left the column");
    }
    p.groups = groups;
    for (int i = 0; i < nq && !rc; ++i) {
        rc = make_owned_column(&outs[i], PLGPU_F64, groups, totals[1] != 0u, s);
        if (!rc) {
            p.out[i] = (double*)outs[i].values;
            p.out_valid[i] = (uint64_t*)outs[i].validity;
        }
    }
    hipError_t e = hipSuccess;
    if (!rc && groups > 0) {
        if (n == 0) {
            for (int i = 0; i < nq && e == hipSuccess; ++i) {
                e = hipMemsetAsync((void*)p.out[i], 0, 8, s);
                if (e == hipSuccess) e = hipMemsetAsync((void*)p.out_valid[i], 0, 8, s);
            }
        } else {
            rc = start.alloc(((size_t)groups + 1) * sizeof(uint32_t), s);
            if (!rc) {
                p.start = start;
                {
                    KtScope kt("quantile_starts_kernel", s);
                    quantile_starts_kernel<<<(unsigned)p.tiles, kTileThreads, 0, s>>>(p);
                }
                switch (dt) {
                case PLGPU_I32: quantile_apply_launch<int32_t>(p, s); break;
                case PLGPU_U32: quantile_apply_launch<uint32_t>(p, s); break;
                case PLGPU_I64: quantile_apply_launch<int64_t>(p, s); break;
                default: quantile_apply_launch<double>(p, s); break;
                }
                e = hipGetLastError();
            }
        }
        if (!rc && e == hipSuccess) e = hipStreamSynchronize(s);
        if (!rc && e != hipSuccess) rc = hip_fail(e, "quantile");
    }
    if (rc)
        for (int i = 0; i < nq; ++i)
            if (outs[i].release != nullptr) plgpu_column_release(&outs[i]);
    return rc;
}
