// Cumulative (cum_sum / cum_min / cum_max / cum_count) and lag (shift / diff)
// functions of one column, plain or per segment.
//
// Reference (paths under the polars crates):
//   polars-ops/src/series/ops/cum_agg.rs:340 cum_sum, :378 cum_min, :416
//   cum_max, :420 cum_count and the det_* folds at :14-51 (a null row gives
//   null and leaves the running state as it was; min / max skip NaN once a
//   non-NaN value has been seen); polars-ops/src/series/ops/diff.rs:4 diff;
//   ChunkedArray::shift_and_fill; over groups
//   polars-expr/src/expressions/window.rs:356 with GroupsToRows.
//
// MI355X design (DESIGN.md "Cumulative and lag expressions"): three launches,
// none of which waits on another workgroup.  cum_reduce_kernel: one workgroup
// per tile of kTileRows rows writes the tile's summary (does it hold a segment
// start; the aggregate of the rows after its last start, or of all its rows;
// for f64 sums the non-finite flags and the exponent range).
// cum_totals_kernel: one workgroup scans the summaries with the segmented
// operator (a summary with a start replaces the running value) and leaves
// every tile's carry in their place; for f64 sums it first fixes the column's
// bottom exponent, shifts every tile's sum onto it and checks the span.
// cum_apply_kernel re-reads the tile, scans it and adds the carry to the rows
// before the tile's first start.  A workgroup takes its tile as kTileBlocks
// block scans of kTileBlock rows one after the other, the running value handed
// from one to the next in registers, so the column has an eighth of the
// summaries one scan per workgroup would leave to the single-workgroup launch.
//
// f64 sums are exact: a value is a fixed-point integer on the column's bottom
// (the exponent of its smallest finite non-zero value) held as three
// carry-free 40-bit limbs; prefixes are limb sums, the carry a 192-bit
// integer, and every output is rounded once (fx_to_double).  Integer sums are
// u64 scans modulo 2^64 truncated on store, min / max unsigned maxima of
// order-preserving codes (0 = nothing seen yet), count a scan of validity.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>

#include "plgpu_internal.hpp"
#include "seg_scan.hpp"
#include "seg_starts.hpp"

namespace plgpu {
namespace {

constexpr int kCumSpan = kSumWindowBits - 53;      // binades between the smallest and largest exponent

enum CumK : int { CK_SUMI = 0, CK_SUMF = 1, CK_MM = 2, CK_COUNT = 3 };
constexpr uint32_t kNfNan = 1u, kNfPinf = 2u, kNfNinf = 4u;

// Summary words of tile t (cum_reduce_kernel), replaced by the tile's carry
// (cum_totals_kernel).  meta: bit 0 the tile holds a segment start, bits 1..3
// the non-finite flags, bits 16..27 / 32..43 the smallest / largest biased
// exponent of its finite non-zero values (0x7FF / 0: none).
struct CumParams {
    DevCol c;
    int64_t n;
    const uint64_t* seg;  // segment starts as words from bit 0 (nullptr: one segment)
    int32_t is_max;
    int32_t isf;
    int32_t out_dtype;
    int32_t uns;          // UInt64 input: a value is its own order-preserving code
    void* out;
    uint8_t* out_valid;   // nullptr: cum_count
    uint64_t* w0;
    uint64_t* w1;
    uint64_t* w2;
    uint64_t* meta;
    int64_t tiles;
    int32_t* info;        // [0] 1: span refused, [1] / [2] the column's smallest / largest exponent
};

// The running value.  Integer kinds use `a` alone; f64 sums hold three signed
// limb sums (tile kernels) or a 192-bit two's complement integer (totals
// kernel) in a, b, c and the non-finite flags in f.
struct St {
    uint64_t a, b, c;
    uint32_t f;
};

__device__ __forceinline__ St st_id() { return St{0ull, 0ull, 0ull, 0u}; }

// left (+) right.  WORDS: a, b, c are one 192-bit integer.
template <int K, bool WORDS>
__device__ __forceinline__ St st_comb(const St& l, const St& r) {
    St o = l;
    if constexpr (K == CK_MM) {
        o.a = l.a > r.a ? l.a : r.a;
    } else if constexpr (K == CK_SUMF) {
        if constexpr (WORDS) {
            o.a = l.a + r.a;
            const uint64_t c0 = o.a < l.a ? 1ull : 0ull;
            const uint64_t t = l.b + r.b;
            const uint64_t c1 = t < l.b ? 1ull : 0ull;
            o.b = t + c0;
            const uint64_t c2 = o.b < t ? 1ull : 0ull;
            o.c = l.c + r.c + c1 + c2;
        } else {
            o.a = l.a + r.a;
            o.b = l.b + r.b;
            o.c = l.c + r.c;
        }
        o.f = l.f | r.f;
    } else {
        o.a = l.a + r.a;
    }
    return o;
}

template <int K>
__device__ __forceinline__ St st_shfl_up(const St& x, int off) {
    St y = x;
    y.a = __shfl_up(x.a, off, 64);
    if constexpr (K == CK_SUMF) {
        y.b = __shfl_up(x.b, off, 64);
        y.c = __shfl_up(x.c, off, 64);
        y.f = __shfl_up(x.f, off, 64);
    }
    return y;
}

// The operator of the segmented scan (seg_scan.hpp).
template <int K, bool WORDS>
struct CumOp {
    using T = St;
    static __device__ __forceinline__ St id() { return st_id(); }
    static __device__ __forceinline__ St comb(const St& l, const St& r) { return st_comb<K, WORDS>(l, r); }
    static __device__ __forceinline__ St shfl_up(const St& x, int off) { return st_shfl_up<K>(x, off); }
};

// Smallest / largest of one (lo, hi) pair per thread over the workgroup.
__device__ __forceinline__ void block_minmax(int& lo, int& hi, int* slo, int* shi) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, __shfl_xor(lo, off, 64));
        hi = max(hi, __shfl_xor(hi, off, 64));
    }
    if (lane == 0) {
        slo[wid] = lo;
        shi[wid] = hi;
    }
    __syncthreads();
    lo = slo[0];
    hi = shi[0];
    for (int w = 1; w < nw; ++w) {
        lo = min(lo, slo[w]);
        hi = max(hi, shi[w]);
    }
    __syncthreads();
}

// The thread's kTilePer rows: register forms, validity bits, segment-start bits.
struct CumRows {
    uint64_t x[kTilePer];
    uint32_t vm;  // bit k: row k is inside the column and not null
    uint32_t sb;  // bit k: row k starts a segment
};

template <bool SEG>
__device__ __forceinline__ void cum_load(const CumParams& p, int64_t base, CumRows& r) {
    r.vm = 0u;
    r.sb = 0u;
    const bool full = base + kTilePer <= p.n;
    const bool wide = p.c.dtype == PLGPU_F64 || p.c.dtype == PLGPU_I64 || p.c.dtype == PLGPU_U64;
    const uint64_t* src = (const uint64_t*)p.c.values + p.c.offset + base;
    if (wide && full && ((uintptr_t)src & 15u) == 0) {
        load_vec8(src, r.x);
    } else {
#pragma unroll
        for (int k = 0; k < kTilePer; ++k) r.x[k] = base + k < p.n ? dev_load(p.c, base + k) : 0ull;
    }
#pragma unroll
    for (int k = 0; k < kTilePer; ++k)
        if (base + k < p.n && dev_valid(p.c, base + k)) r.vm |= 1u << k;
    if constexpr (SEG) {
        // base is a multiple of 8: the thread's start bits are one byte of the bitmap
        if (base < p.n) r.sb = ((const uint8_t*)p.seg)[base >> 3];
        if (!full) r.sb &= base < p.n ? (1u << (int)(p.n - base)) - 1u : 0u;
    }
}

// Biased exponent of a finite non-zero value (a subnormal's is 1), else -1.
__device__ __forceinline__ int cum_exponent(uint64_t b) {
    const int ex = (int)((b >> 52) & 0x7FF);
    if (ex == 0x7FF) return -1;
    if (ex == 0) return (b & 0x000FFFFFFFFFFFFFull) ? 1 : -1;
    return ex;
}

// Row value -> running-value element (the identity for a null row).
template <int K>
__device__ __forceinline__ St cum_elem(const CumParams& p, uint64_t b, bool valid, int bottom) {
    St s = st_id();
    if (!valid) return s;
    if constexpr (K == CK_COUNT) {
        s.a = 1ull;
    } else if constexpr (K == CK_SUMI) {
        s.a = b;
    } else if constexpr (K == CK_MM) {
        if (p.isf && (b & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return s;  // NaN: skipped
        const uint64_t code = p.isf ? ord_f64(b) : (p.uns ? b : ord_i64(b));
        s.a = p.is_max ? code : ~code;
    } else {
        if (((b >> 52) & 0x7FF) == 0x7FF) {
            s.f = (b & 0x000FFFFFFFFFFFFFull) ? kNfNan : ((b >> 63) ? kNfNinf : kNfPinf);
        } else {
            uint32_t fl = 0u, ex = 0u;
            uint64_t l0 = 0, l1 = 0, l2 = 0;
            // (exact: the bottom is at or below every value's own; a value
            // that leaves the window belongs to a refused column)
            if (fx_limbs<kSumWindowBits>(b, bottom, l0, l1, l2, fl, ex)) {
                s.a = l0;
                s.b = l1;
                s.c = l2;
            }
        }
    }
    return s;
}

// Fold of the thread's rows from (f, run): (f, run) afterwards.
template <int K>
__device__ __forceinline__ void cum_fold(const CumParams& p, const CumRows& r, int bottom, bool& f, St& run) {
#pragma unroll
    for (int k = 0; k < kTilePer; ++k) {
        const St e = cum_elem<K>(p, r.x[k], (r.vm >> k) & 1u, bottom);
        seg_comb<CumOp<K, false>>(f, run, (r.sb >> k) & 1u, e);
    }
}

// 192-bit w << s, 0 <= s < 128.
__device__ __forceinline__ void shl192(uint64_t& w0, uint64_t& w1, uint64_t& w2, int s) {
    if (s >= 64) {
        w2 = w1;
        w1 = w0;
        w0 = 0;
        s -= 64;
    }
    if (s > 0) {
        w2 = (w2 << s) | (w1 >> (64 - s));
        w1 = (w1 << s) | (w0 >> (64 - s));
        w0 <<= s;
    }
}

// Limb sums -> the 192-bit integer (f64 sums; the other kinds keep `a`).
template <int K>
__device__ __forceinline__ St st_words(const St& l) {
    St w = l;
    if constexpr (K == CK_SUMF) limbs_to_192((int64_t)l.a, (int64_t)l.b, (int64_t)l.c, w.a, w.b, w.c);
    return w;
}

template <int K, bool SEG>
__global__ __launch_bounds__(kTileThreads) void cum_reduce_kernel(CumParams p) {
    __shared__ St wv[kTileThreads / 64];
    __shared__ uint32_t wf[kTileThreads / 64];
    __shared__ int slo[kTileThreads / 64], shi[kTileThreads / 64];
    const int64_t tile = blockIdx.x;
    // the tile's running total over its blocks (f64 sums: 192 bits on the
    // bottom emin - 1075, emin the smallest exponent of the blocks so far)
    bool rf = false;
    St rv = st_id();
    int emin = 0x7FF, emax = 0;
    for (int j = 0; j < kTileBlocks; ++j) {
        const int64_t first = tile * kTileRows + (int64_t)j * kTileBlock;
        if (first >= p.n) break;
        const int64_t base = first + (int64_t)threadIdx.x * kTilePer;
        CumRows r;
        cum_load<SEG>(p, base, r);
        int bmin = 0x7FF, bmax = 0;
        if constexpr (K == CK_SUMF) {
#pragma unroll
            for (int k = 0; k < kTilePer; ++k) {
                const int ex = ((r.vm >> k) & 1u) ? cum_exponent(r.x[k]) : -1;
                if (ex > 0) {
                    bmin = min(bmin, ex);
                    bmax = max(bmax, ex);
                }
            }
            block_minmax(bmin, bmax, slo, shi);
        }
        bool f = false;
        St run = st_id();
        cum_fold<K>(p, r, bmin - 1075, f, run);
        bool ef, tf;
        St ev, tv;
        block_seg_scan<CumOp<K, false>>(f, run, wv, wf, ef, ev, tf, tv);
        St tw = st_words<K>(tv);
        if constexpr (K == CK_SUMF) {
            // (shifts past the span belong to a refused column: its sums are not used)
            if (bmax >= bmin) {
                if (emin != 0x7FF && bmin < emin) shl192(rv.a, rv.b, rv.c, min(emin - bmin, kCumSpan));
                emin = min(emin, bmin);
                emax = max(emax, bmax);
                shl192(tw.a, tw.b, tw.c, min(bmin - emin, kCumSpan));
            }
        }
        seg_comb<CumOp<K, true>>(rf, rv, tf, tw);
    }
    if (threadIdx.x == 0) {
        p.w0[tile] = rv.a;
        if constexpr (K == CK_SUMF) {
            p.w1[tile] = rv.b;
            p.w2[tile] = rv.c;
        }
        p.meta[tile] = (rf ? 1ull : 0ull) | ((uint64_t)rv.f << 1) | ((uint64_t)emin << 16) | ((uint64_t)emax << 32);
    }
}

// Summary of tile t as a (flag, value) of the totals scan; f64 sums shifted
// from the tile's bottom onto the column's (emin).
template <int K>
__device__ __forceinline__ St cum_summary(const CumParams& p, int64_t t, int emin, bool& f) {
    const uint64_t m = p.meta[t];
    f = (m & 1ull) != 0;
    St s = st_id();
    s.a = p.w0[t];
    if constexpr (K == CK_SUMF) {
        s.b = p.w1[t];
        s.c = p.w2[t];
        s.f = (uint32_t)(m >> 1) & 7u;
        const int tmin = (int)((m >> 16) & 0xFFF), tmax = (int)((m >> 32) & 0xFFF);
        // (a tile above the span belongs to a refused column: its sum is not used)
        if (tmax >= tmin) shl192(s.a, s.b, s.c, min(tmin - emin, kCumSpan));
    }
    return s;
}

template <int K>
__global__ __launch_bounds__(kTotalsThreads) void cum_totals_kernel(CumParams p) {
    __shared__ St wv[kTotalsThreads / 64];
    __shared__ uint32_t wf[kTotalsThreads / 64];
    __shared__ int slo[kTotalsThreads / 64], shi[kTotalsThreads / 64];
    int64_t lo, hi;
    totals_span(p.tiles, lo, hi);
    int emin = 0x7FF, emax = 0;
    if constexpr (K == CK_SUMF) {
        for (int64_t t = lo; t < hi; ++t) {
            const uint64_t m = p.meta[t];
            emin = min(emin, (int)((m >> 16) & 0xFFF));
            emax = max(emax, (int)((m >> 32) & 0xFFF));
        }
        block_minmax(emin, emax, slo, shi);
        if (threadIdx.x == 0) {
            p.info[0] = (emax >= emin && emax - emin > kCumSpan) ? 1 : 0;
            p.info[1] = emin;
            p.info[2] = emax;
        }
    }
    bool f = false;
    St run = st_id();
    for (int64_t t = lo; t < hi; ++t) {
        bool sf;
        const St s = cum_summary<K>(p, t, emin, sf);
        seg_comb<CumOp<K, true>>(f, run, sf, s);
    }
    bool ef, tf;
    St ev, tv;
    block_seg_scan<CumOp<K, true>>(f, run, wv, wf, ef, ev, tf, tv);
    // the carry of tile t: the running value before it
    for (int64_t t = lo; t < hi; ++t) {
        bool sf;
        const St s = cum_summary<K>(p, t, emin, sf);
        p.w0[t] = ev.a;
        if constexpr (K == CK_SUMF) {
            p.w1[t] = ev.b;
            p.w2[t] = ev.c;
            p.meta[t] = (uint64_t)ev.f << 1;
        }
        seg_comb<CumOp<K, true>>(ef, ev, sf, s);
    }
}

template <int K, bool SEG>
__global__ __launch_bounds__(kTileThreads) void cum_apply_kernel(CumParams p) {
    __shared__ St wv[kTileThreads / 64];
    __shared__ uint32_t wf[kTileThreads / 64];
    const int64_t tile = blockIdx.x;
    int bottom = 0;
    if constexpr (K == CK_SUMF) bottom = p.info[1] - 1075;
    // the running value before the block: the tile's carry, then the blocks
    // before this one (f64 sums: 192 bits on the column's bottom)
    bool cf = false;
    St cy = st_id();
    cy.a = p.w0[tile];
    if constexpr (K == CK_SUMF) {
        cy.b = p.w1[tile];
        cy.c = p.w2[tile];
        cy.f = (uint32_t)(p.meta[tile] >> 1) & 7u;
    }
    for (int j = 0; j < kTileBlocks; ++j) {
        const int64_t first = tile * kTileRows + (int64_t)j * kTileBlock;
        if (first >= p.n) break;
        const int64_t base = first + (int64_t)threadIdx.x * kTilePer;
        CumRows r;
        cum_load<SEG>(p, base, r);
        bool f = false;
        St run = st_id();
        cum_fold<K>(p, r, bottom, f, run);
        bool seen, tf;
        St ev, tv;
        block_seg_scan<CumOp<K, false>>(f, run, wv, wf, seen, ev, tf, tv);
        // integer kinds fold the carry into the thread's prefix; f64 sums add
        // it (192 bits) to the limb sums of the rows before the first start
        if constexpr (K != CK_SUMF) {
            if (!seen) ev = st_comb<K, false>(cy, ev);
        }
        uint64_t o[kTilePer];
        uint32_t ovm = 0u;
#pragma unroll
        for (int k = 0; k < kTilePer; ++k) {
            const bool valid = (r.vm >> k) & 1u;
            const St e = cum_elem<K>(p, r.x[k], valid, bottom);
            seg_comb<CumOp<K, false>>(seen, ev, (r.sb >> k) & 1u, e);
            uint64_t v = 0ull;
            if constexpr (K == CK_COUNT) {
                v = ev.a;
            } else if (valid) {
                ovm |= 1u << k;
                if constexpr (K == CK_SUMI) {
                    v = ev.a;
                } else if constexpr (K == CK_MM) {
                    const uint64_t code = p.is_max ? ev.a : ~ev.a;
                    if (p.isf) v = ev.a == 0ull ? 0x7ff8000000000000ull : unord_f64(code);
                    else v = p.uns ? code : code ^ 0x8000000000000000ull;
                } else {
                    St w = st_words<K>(ev);
                    if (!seen) w = st_comb<K, true>(cy, w);
                    double d;
                    if ((w.f & kNfNan) || ((w.f & kNfPinf) && (w.f & kNfNinf))) d = __builtin_nan("");
                    else if (w.f & kNfPinf) d = __builtin_inf();
                    else if (w.f & kNfNinf) d = -__builtin_inf();
                    else d = fx_to_double(w.a, w.b, w.c, bottom);
                    v = f64_bits(d);
                }
            }
            o[k] = v;
        }
        seg_comb<CumOp<K, true>>(cf, cy, tf, st_words<K>(tv));  // the carry of the next block
        if (base >= p.n) {  // the rest of the last validity word
            if (p.out_valid != nullptr && base < (p.n + 63) / 64 * 64) p.out_valid[base >> 3] = 0;
            continue;
        }
        if (dtype_bytes(p.out_dtype) == 8 && base + kTilePer <= p.n) {
            ulonglong2* d2 = (ulonglong2*)((uint64_t*)p.out + base);  // an owned buffer, base even: 16-byte aligned
#pragma unroll
            for (int k = 0; k < kTilePer / 2; ++k) d2[k] = make_ulonglong2(o[2 * k], o[2 * k + 1]);
        } else if (dtype_bytes(p.out_dtype) == 4 && base + kTilePer <= p.n) {
            uint4* d4 = (uint4*)((uint32_t*)p.out + base);
            d4[0] = make_uint4((uint32_t)o[0], (uint32_t)o[1], (uint32_t)o[2], (uint32_t)o[3]);
            d4[1] = make_uint4((uint32_t)o[4], (uint32_t)o[5], (uint32_t)o[6], (uint32_t)o[7]);
        } else {
#pragma unroll
            for (int k = 0; k < kTilePer; ++k)
                if (base + k < p.n) {
                    if (dtype_bytes(p.out_dtype) == 8) ((uint64_t*)p.out)[base + k] = o[k];
                    else ((uint32_t*)p.out)[base + k] = (uint32_t)o[k];
                }
        }
        if (p.out_valid != nullptr) p.out_valid[base >> 3] = (uint8_t)ovm;  // rows past the column: zero bits
    }
}

// ------------------------------------------------------------------- lag
struct LagParams {
    DevCol c;
    int64_t n;
    int64_t lag;
    const uint64_t* seg;
    int64_t seg_bytes;
    int32_t diff;
    int32_t has_fill;
    uint64_t fill;
    void* out;
    uint64_t* out_valid;
};

// Is a segment start among rows (lo, hi]?  (0 <= lo <= hi < n.)
__device__ __forceinline__ bool lag_seg_any(const uint64_t* seg, int64_t nbytes, int64_t lo, int64_t hi) {
    const int64_t q = lo + 1;
    for (int64_t wi = q >> 6; (wi << 6) <= hi; ++wi) {
        uint64_t m = seg_word(seg, nbytes, wi);
        if ((wi << 6) < q) m &= ~0ull << (int)(q & 63);
        if (hi - (wi << 6) < 63) m &= ~0ull >> (63 - (int)(hi - (wi << 6)));
        if (m) return true;
    }
    return false;
}

// x[i] - x[j] in the column's own dtype (register forms).
__device__ __forceinline__ uint64_t lag_sub(int32_t dt, uint64_t a, uint64_t b) {
    switch (dt) {
    case PLGPU_F64: return f64_bits(as_f64(a) - as_f64(b));
    case PLGPU_F32: return f64_bits((double)((float)as_f64(a) - (float)as_f64(b)));
    default: return a - b;  // wraps at the width of the store
    }
}

template <bool SEG>
__global__ __launch_bounds__(256) void lag_kernel(LagParams p) {
    const int64_t words = (p.n + 63) / 64;
    const int eb = dtype_bytes(p.c.dtype);
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < words * 64;
         r += (int64_t)gridDim.x * blockDim.x) {
        bool ok = false;
        if (r < p.n) {
            const int64_t src = r - p.lag;
            bool in = src >= 0 && src < p.n;
            if constexpr (SEG) {
                if (in && src != r) in = !lag_seg_any(p.seg, p.seg_bytes, src < r ? src : r, src < r ? r : src);
            }
            uint64_t v = 0ull;
            if (p.diff) {
                ok = in && dev_valid(p.c, r) && dev_valid(p.c, src);
                if (ok) v = lag_sub(p.c.dtype, dev_load(p.c, r), dev_load(p.c, src));
                if (eb == 8) ((uint64_t*)p.out)[r] = v;
                else dev_store(p.out, p.c.dtype, r, v);
            } else {
                // the value's own bits, so a NaN keeps its payload
                if (in) {
                    ok = dev_valid(p.c, src);
                    if (ok) v = eb == 8 ? ((const uint64_t*)p.c.values)[p.c.offset + src]
                                        : (uint64_t)((const uint32_t*)p.c.values)[p.c.offset + src];
                } else if (p.has_fill) {
                    ok = true;
                    v = p.fill;
                }
                if (eb == 8) ((uint64_t*)p.out)[r] = v;
                else ((uint32_t*)p.out)[r] = (uint32_t)v;
            }
        }
        const uint64_t m = __ballot(ok);
        if ((threadIdx.x & 63) == 0) p.out_valid[r >> 6] = m;
    }
}

template <int K>
void cum_launch(const CumParams& p, hipStream_t s) {
    const unsigned g = (unsigned)p.tiles;
    {
        KtScope kt("cum_reduce_kernel", s);
        if (p.seg) cum_reduce_kernel<K, true><<<g, kTileThreads, 0, s>>>(p);
        else cum_reduce_kernel<K, false><<<g, kTileThreads, 0, s>>>(p);
    }
    {
        KtScope kt("cum_totals_kernel", s);
        cum_totals_kernel<K><<<1, kTotalsThreads, 0, s>>>(p);
    }
    {
        KtScope kt("cum_apply_kernel", s);
        if (p.seg) cum_apply_kernel<K, true><<<g, kTileThreads, 0, s>>>(p);
        else cum_apply_kernel<K, false><<<g, kTileThreads, 0, s>>>(p);
    }
}

}  // namespace
}  // namespace plgpu

using namespace plgpu;

PLGPU_API int plgpu_cumulative(const plgpu_column* values, const plgpu_column* seg_starts, int32_t kind,
                               plgpu_column* out, void* stream) {
    hipStream_t s = as_stream(stream);
    if (values == nullptr || out == nullptr) return fail(PLGPU_ERR_INVALID, "NULL argument");
    std::memset(out, 0, sizeof *out);
    if (kind < PLGPU_CUM_SUM || kind > PLGPU_CUM_COUNT) return fail(PLGPU_ERR_INVALID, "unknown cumulative kind");
    const int32_t dt = values->dtype;
    if (kind == PLGPU_CUM_COUNT) {
        if (dt < PLGPU_BOOL || dt > PLGPU_F32) return fail(PLGPU_ERR_SCHEMA, "cum_count: unknown input dtype");
    } else if (dt != PLGPU_F64 && dt != PLGPU_I64 && dt != PLGPU_I32 && dt != PLGPU_U64) {
        return fail(PLGPU_ERR_SCHEMA, "cumulative input must be Float64 / Int64 / Int32 / UInt64");
    }
    if (seg_starts != nullptr) {
        const int rc = seg_check(values, seg_starts, PLGPU_ERR_SCHEMA, PLGPU_ERR_SHAPE);
        if (rc) return rc;
    }
    const int64_t n = values->length;
    const bool count = kind == PLGPU_CUM_COUNT;
    int rc = make_owned_column(out, count ? PLGPU_U32 : dt, n, !count, s);
    if (rc || n == 0) return rc;
    CumParams p;
    std::memset(&p, 0, sizeof p);
    DevBuf<uint64_t> seg_own, words;
    DevBuf<int32_t> info;
    if (seg_starts != nullptr) rc = seg_words(seg_starts, n, seg_own, &p.seg, s);
    p.c = dev_col(*values);
    p.n = n;
    p.is_max = kind == PLGPU_CUM_MAX;
    p.isf = dt == PLGPU_F64;
    p.uns = dt == PLGPU_U64;
    p.out_dtype = out->dtype;
    p.out = (void*)out->values;
    p.out_valid = (uint8_t*)out->validity;
    p.tiles = (n + kTileRows - 1) / kTileRows;
    const bool sumf = kind == PLGPU_CUM_SUM && dt == PLGPU_F64;
    if (!rc) rc = words.alloc((size_t)p.tiles * 8 * 4, s);
    if (!rc) rc = info.alloc(4 * sizeof(int32_t), s);
    hipError_t e = hipSuccess;
    int32_t hinfo[4] = {0, 0, 0, 0};
    if (!rc) {
        p.w0 = words;
        p.w1 = p.w0 + p.tiles;
        p.w2 = p.w1 + p.tiles;
        p.meta = p.w2 + p.tiles;
        p.info = info;
        if (count) cum_launch<CK_COUNT>(p, s);
        else if (kind != PLGPU_CUM_SUM) cum_launch<CK_MM>(p, s);
        else if (sumf) cum_launch<CK_SUMF>(p, s);
        else cum_launch<CK_SUMI>(p, s);
        e = hipGetLastError();
        if (e == hipSuccess && sumf) e = hipMemcpyAsync(hinfo, p.info, sizeof hinfo, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "cumulative");
    }
    if (!rc && sumf && hinfo[0] != 0)
        rc = fail(PLGPU_ERR_SCHEMA,
                  "cum_sum: the column's finite non-zero Float64 values span " + std::to_string(hinfo[2] - hinfo[1]) +
                      " binades; the exact fixed-point accumulator holds at most " + std::to_string(kCumSpan) +
                      " (a sum is never rounded twice)");
    if (rc) plgpu_column_release(out);
    else out->null_count = count ? 0 : -1;
    return rc;
}

PLGPU_API int plgpu_lag(const plgpu_column* values, const plgpu_column* seg_starts, int32_t kind, int64_t n,
                        int32_t has_fill, int64_t fill_bits, plgpu_column* out, void* stream) {
    hipStream_t s = as_stream(stream);
    if (values == nullptr || out == nullptr) return fail(PLGPU_ERR_INVALID, "NULL argument");
    std::memset(out, 0, sizeof *out);
    if (kind != PLGPU_LAG_SHIFT && kind != PLGPU_LAG_DIFF) return fail(PLGPU_ERR_INVALID, "unknown lag kind");
    const int eb = dtype_bytes(values->dtype);
    if (eb != 4 && eb != 8) return fail(PLGPU_ERR_SCHEMA, "shift / diff input must be a 4- or 8-byte numeric column");
    if (kind == PLGPU_LAG_DIFF && (values->dtype == PLGPU_U32 || values->dtype == PLGPU_U64))
        return fail(PLGPU_ERR_SCHEMA, "diff of an unsigned column: cast it to Int64 first");
    if (seg_starts != nullptr) {
        const int rc = seg_check(values, seg_starts, PLGPU_ERR_SCHEMA, PLGPU_ERR_SHAPE);
        if (rc) return rc;
    }
    const int64_t len = values->length;
    int rc = make_owned_column(out, values->dtype, len, true, s);
    if (rc || len == 0) return rc;
    LagParams p;
    std::memset(&p, 0, sizeof p);
    DevBuf<uint64_t> seg_own;
    if (seg_starts != nullptr) rc = seg_words(seg_starts, len, seg_own, &p.seg, s);
    p.seg_bytes = (len + 7) / 8;
    p.c = dev_col(*values);
    p.n = len;
    p.lag = n;
    p.diff = kind == PLGPU_LAG_DIFF;
    p.has_fill = has_fill != 0;
    p.fill = eb == 8 ? (uint64_t)fill_bits : ((uint64_t)fill_bits & 0xFFFFFFFFull);
    p.out = (void*)out->values;
    p.out_valid = (uint64_t*)out->validity;
    if (!rc) {
        const unsigned g = (unsigned)std::min<int64_t>((len + 255) / 256, 256 * 64);
        {
            KtScope kt(p.seg ? "lag_seg_kernel" : "lag_kernel", s);
            if (p.seg) lag_kernel<true><<<g, 256, 0, s>>>(p);
            else lag_kernel<false><<<g, 256, 0, s>>>(p);
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "lag");
    }
    if (rc) plgpu_column_release(out);
    else out->null_count = -1;
    return rc;
}
