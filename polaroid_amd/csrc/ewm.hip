// Exponentially weighted mean of one column, plain or per segment
// (ewm_mean, ewm_mean(...).over(keys)).
//
// Reference (paths under the polars crates):
//   polars-compute/src/ewm/mean.rs:52 EwmMeanState::update_iter, called through
//   polars-ops/src/series/ops/ewm.rs:11 ewm_mean and
//   polars-expr/src/dispatch/misc.rs:887; over groups
//   polars-expr/src/expressions/window.rs:356 with GroupsToRows.
//
// MI355X design (DESIGN.md "Exponentially weighted mean"): the fold is a
// first-order linear recurrence, so every row is an affine map of the running
// state and the column a segmented scan of maps (a segment start replaces the
// running map, it never multiplies it).
//   adjust      state (S, W), one coefficient: S -> a S + x, W -> a W + 1 with
//               a = 1 - alpha at a row that decays, 1 at a null under
//               ignore_nulls; the output is S / W.
//   no adjust   state mean -> mean - F mean + b.  F = alpha / (w + alpha),
//               b = F x, w = (1 - alpha)^(gap + 1), gap the nulls since the
//               previous non-null row (0 under ignore_nulls); the first
//               non-null row of a segment has F = 1.  1 - F is never formed:
//               maps compose as F = F1 + F2 - F1 F2, b = (b1 - F2 b1) + b2.
// Which row is the previous non-null one, and whether a segment start lies
// after it, are running maxima of row codes over the bitmaps, as in fill.hip
// (one 64-row word per thread, then the bits of the thread's own byte).
// A non-finite value never enters a map: it raises a flag that travels with
// the map, and the segmented non-null count travels there too (min_samples).
//
// Three launches, none of which waits on another workgroup.
// ewm_reduce_kernel: one workgroup per tile of kTileRows rows, taken as
// kTileBlocks block scans of kTileBlock rows, leaves the tile's map (after its
// last start, or of all its rows) and, without adjust, its bitmap codes and
// the one row whose map depends on earlier tiles (the tile's first non-null
// row, when no start precedes it).  ewm_totals_kernel: one workgroup scans the
// codes, completes each tile's map with that row and scans the maps; every
// tile's carry takes the place of its summary.  ewm_apply_kernel re-scans the
// tile, composes with the carry and streams the outputs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "plgpu_internal.hpp"
#include "seg_scan.hpp"

namespace plgpu {
namespace {

constexpr int kEwmPowLoop = 8;                    // (1 - alpha)^k by k products up to here, pow() above
constexpr uint32_t kEwmNf = 1u;                   // a non-finite value was seen

struct EwmParams {
    const void* values;    // the slice's first element is values[voff]
    int64_t voff;
    const uint8_t* valid;  // validity bitmap (nullptr: no nulls); row r is bit valid_off + r
    int64_t valid_off;
    int64_t valid_bytes;
    const uint8_t* seg;    // segment starts (nullptr: one segment), row r is bit seg_off + r
    int64_t seg_off;
    int64_t seg_bytes;
    int64_t n;
    double alpha;
    double decay;          // 1 - alpha
    double f0;             // alpha / (decay + alpha): F of a row right after a non-null row
    int32_t ignore_nulls;
    uint64_t min_count;    // max(min_samples, 1)
    void* out;
    uint8_t* out_valid;
    // per tile: the summary (ewm_reduce_kernel), then the carry (ewm_totals_kernel)
    double* sp;
    double* sq;
    double* sr;
    uint64_t* scnt;
    uint64_t* smeta;       // bit 0 the tile holds a segment start, bit 1 non-finite seen
    double* sx1;           // no adjust: value of the row left to the totals launch
    uint64_t* sfirst;      //   and its row code (0: none)
    uint64_t* cj;          // no adjust: code of the tile's last non-null row, then the carry
    uint64_t* cs;          //   code of its last segment start, then the carry
    int64_t tiles;
};

// A map of the running state with what travels along.  adjust: S -> p S + q,
// W -> p W + r.  No adjust: mean -> mean - p mean + q (p is F).
struct Em {
    double p, q, r;
    uint64_t cnt;  // non-null rows
    uint32_t fl;   // kEwmNf
};

template <bool ADJ>
__device__ __forceinline__ Em em_id() {
    return Em{ADJ ? 1.0 : 0.0, 0.0, 0.0, 0ull, 0u};
}

// l, then r.  (fma is asked for by name: the file is built without contraction.)
template <bool ADJ>
__device__ __forceinline__ Em em_comb(const Em& l, const Em& r) {
    Em o;
    if constexpr (ADJ) {
        o.p = l.p * r.p;
        o.q = fma(r.p, l.q, r.q);
        o.r = fma(r.p, l.r, r.r);
    } else {
        o.p = fma(-l.p, r.p, l.p) + r.p;
        o.q = fma(-r.p, l.q, l.q) + r.q;
        o.r = 0.0;
    }
    o.cnt = l.cnt + r.cnt;
    o.fl = l.fl | r.fl;
    return o;
}

template <bool ADJ>
__device__ __forceinline__ Em em_shfl_up(const Em& x, int off) {
    Em y;
    y.p = __shfl_up(x.p, off, 64);
    y.q = __shfl_up(x.q, off, 64);
    y.r = ADJ ? __shfl_up(x.r, off, 64) : 0.0;
    y.cnt = __shfl_up(x.cnt, off, 64);
    y.fl = __shfl_up(x.fl, off, 64);
    return y;
}

// The operator of the segmented scan (seg_scan.hpp).
template <bool ADJ>
struct EmOp {
    using T = Em;
    static __device__ __forceinline__ Em id() { return em_id<ADJ>(); }
    static __device__ __forceinline__ Em comb(const Em& l, const Em& r) { return em_comb<ADJ>(l, r); }
    static __device__ __forceinline__ Em shfl_up(const Em& x, int off) { return em_shfl_up<ADJ>(x, off); }
};

// F of a non-null row that follows `gap` nulls after the previous non-null
// row: the reference's weight there is 1 * d * ... * d, gap + 1 factors.
__device__ __forceinline__ double ewm_gap_f(const EwmParams& p, uint64_t gap) {
    if (gap == 0ull) return p.f0;
    double w = p.decay;
    if (gap < (uint64_t)kEwmPowLoop) {
        for (uint64_t g = 0; g < gap; ++g) w *= p.decay;
    } else {
        w = pow(p.decay, (double)(gap + 1ull));
    }
    return p.alpha / (w + p.alpha);
}

__device__ __forceinline__ bool ewm_finite(double x) {
    return (f64_bits(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// The bitmap words of the tile, one per thread, into sV / sS; without adjust
// also the codes that enter every word (sJ last non-null row, sT last start),
// cj0 / cs0 folded in, and the tile's own last codes in (tj, ts) of the last
// thread.
template <bool ADJ>
__device__ __forceinline__ void ewm_tile_words(const EwmParams& p, int64_t tile, bool seg, uint64_t cj0, uint64_t cs0,
                                               uint64_t* sV, uint64_t* sS, uint64_t* sJ, uint64_t* sT, uint64_t* wa,
                                               uint64_t* wb, uint64_t& tj, uint64_t& ts) {
    const int t = threadIdx.x;
    const int64_t r0 = (tile * kTileWords + t) * 64;
    uint64_t V = 0ull, S = 0ull;
    if (r0 < p.n) {
        const uint64_t in = fill_lowmask(p.n - r0);
        V = p.valid != nullptr ? fill_bits64(p.valid, p.valid_bytes, p.valid_off + r0) & in : in;
        if (seg) S = fill_bits64(p.seg, p.seg_bytes, p.seg_off + r0) & in;
    }
    sV[t] = V;
    sS[t] = S;
    tj = 0ull;
    ts = 0ull;
    if constexpr (!ADJ) {
        const uint64_t wj = fill_word_code<false>(V, r0), wt = fill_word_code<false>(S, r0);
        uint64_t a = wj, b = wt;
        fill_block_excl_max(a, b, wa, wb);
        sJ[t] = fill_max(a, cj0);
        sT[t] = fill_max(b, cs0);
        tj = fill_max(a, wj);
        ts = fill_max(b, wt);
    }
    __syncthreads();
}

// The thread's kTilePer rows of one block scan.
struct EwmRows {
    double x[kTilePer];
    double F[kTilePer];  // no adjust: F of a non-null row (0: the row left to the totals launch)
    uint32_t vb;        // bit k: row k is inside the column and not null
    uint32_t sb;        // bit k: row k starts a segment
    uint32_t nf;        // bit k: row k is non-null and not finite
};

// PEND (ewm_reduce_kernel): the codes know nothing of earlier tiles, so the
// tile's first non-null row, when no start precedes it, is left out of the
// maps (its F depends on them); its code and value go to pcode / px.
template <bool ADJ, bool F32, bool PEND>
__device__ __forceinline__ void ewm_load(const EwmParams& p, int64_t tile, int blk, const uint64_t* sV,
                                         const uint64_t* sS, const uint64_t* sJ, const uint64_t* sT, EwmRows& r,
                                         uint64_t* pcode, double* px) {
    using T = typename std::conditional<F32, float, double>::type;
    const int t = threadIdx.x;
    const int64_t base = tile * kTileRows + (int64_t)blk * kTileBlock + (int64_t)t * kTilePer;
    const int wi = blk * (kTileBlock / 64) + (t >> 3);
    const int b0 = (t & 7) * kTilePer;  // the thread's rows are bits b0 .. b0 + 7 of the word
    const uint64_t V = sV[wi], S = sS[wi];
    r.vb = (uint32_t)(V >> b0) & 0xFFu;
    r.sb = (uint32_t)(S >> b0) & 0xFFu;
    r.nf = 0u;
    const T* src = (const T*)p.values + p.voff;
    if (base + kTilePer <= p.n && ((uintptr_t)src & 15u) == 0) {
        if constexpr (F32) {
            float x[kTilePer];
            load_vec8(src + base, x);
#pragma unroll
            for (int k = 0; k < kTilePer; ++k) r.x[k] = x[k];
        } else {
            load_vec8(src + base, r.x);
        }
    } else {
#pragma unroll
        for (int k = 0; k < kTilePer; ++k) r.x[k] = base + k < p.n ? (double)src[base + k] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kTilePer; ++k) {
        if (!((r.vb >> k) & 1u)) r.x[k] = 0.0;  // a null row's bytes are not a value
        else if (!ewm_finite(r.x[k])) r.nf |= 1u << k;
    }
    if constexpr (!ADJ) {
        // the codes that enter the thread's rows: the word's bits before them, else the word's own entry codes
        const uint64_t before = (1ull << b0) - 1ull;
        const uint64_t mj = V & before, ms = S & before;
        const int64_t r0 = (tile * kTileWords + wi) * 64;
        uint64_t jc = mj ? fill_word_code<false>(mj, r0) : sJ[wi];
        uint64_t sc = ms ? fill_word_code<false>(ms, r0) : sT[wi];
#pragma unroll
        for (int k = 0; k < kTilePer; ++k) {
            const uint64_t ic = fill_row_code<false>(base + k);
            if ((r.sb >> k) & 1u) sc = ic;
            r.F[k] = 0.0;
            if ((r.vb >> k) & 1u) {
                if (jc != 0ull && jc >= sc) {
                    r.F[k] = ewm_gap_f(p, p.ignore_nulls ? 0ull : ic - jc - 1ull);
                } else if (PEND && sc == 0ull) {
                    *pcode = ic;
                    *px = ((r.nf >> k) & 1u) ? 0.0 : r.x[k];
                } else {
                    r.F[k] = 1.0;  // the first non-null row of a segment replaces the state
                }
                jc = ic;
            }
        }
    }
}

// Row k as a map (the identity for a null row under ignore_nulls or without adjust).
template <bool ADJ>
__device__ __forceinline__ Em ewm_elem(const EwmParams& p, const EwmRows& r, int k) {
    Em e = em_id<ADJ>();
    const bool valid = (r.vb >> k) & 1u, nf = (r.nf >> k) & 1u;
    if constexpr (ADJ) {
        if (valid || !p.ignore_nulls) e.p = p.decay;
        if (valid) {
            e.q = nf ? 0.0 : r.x[k];
            e.r = 1.0;
        }
    } else {
        if (valid) {
            e.p = r.F[k];
            e.q = nf ? 0.0 : r.F[k] * r.x[k];
        }
    }
    if (valid) {
        e.cnt = 1ull;
        e.fl = nf ? kEwmNf : 0u;
    }
    return e;
}

template <bool ADJ>
__device__ __forceinline__ void ewm_fold(const EwmParams& p, const EwmRows& r, bool& f, Em& run) {
#pragma unroll
    for (int k = 0; k < kTilePer; ++k) seg_comb<EmOp<ADJ>>(f, run, (r.sb >> k) & 1u, ewm_elem<ADJ>(p, r, k));
}

template <bool ADJ, bool F32>
__global__ __launch_bounds__(kTileThreads) void ewm_reduce_kernel(EwmParams p) {
    __shared__ uint64_t sV[kTileWords], sS[kTileWords], sJ[kTileWords], sT[kTileWords];
    __shared__ uint64_t wa[kTileThreads / 64], wb[kTileThreads / 64];
    __shared__ Em wv[kTileThreads / 64];
    __shared__ uint32_t wf[kTileThreads / 64];
    __shared__ uint64_t pcode;
    __shared__ double px;
    const int64_t tile = blockIdx.x;
    if (threadIdx.x == 0) {
        pcode = 0ull;
        px = 0.0;
    }
    uint64_t tj, ts;
    ewm_tile_words<ADJ>(p, tile, p.seg != nullptr, 0ull, 0ull, sV, sS, sJ, sT, wa, wb, tj, ts);
    bool rf = false;
    Em rv = em_id<ADJ>();
    for (int j = 0; j < kTileBlocks; ++j) {
        if (tile * kTileRows + (int64_t)j * kTileBlock >= p.n) break;
        EwmRows r;
        ewm_load<ADJ, F32, true>(p, tile, j, sV, sS, sJ, sT, r, &pcode, &px);
        bool f = false;
        Em run = em_id<ADJ>();
        ewm_fold<ADJ>(p, r, f, run);
        bool ef, tf;
        Em ev, tv;
        block_seg_scan<EmOp<ADJ>>(f, run, wv, wf, ef, ev, tf, tv);
        seg_comb<EmOp<ADJ>>(rf, rv, tf, tv);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        p.sp[tile] = rv.p;
        p.sq[tile] = rv.q;
        p.sr[tile] = rv.r;
        p.scnt[tile] = rv.cnt;
        p.smeta[tile] = (rf ? 1ull : 0ull) | ((uint64_t)rv.fl << 1);
        if constexpr (!ADJ) {
            p.sfirst[tile] = pcode;
            p.sx1[tile] = px;
        }
    }
    if constexpr (!ADJ) {
        if (threadIdx.x == kTileThreads - 1) {
            p.cj[tile] = tj;
            p.cs[tile] = ts;
        }
    }
}

__device__ __forceinline__ Em ewm_summary(const EwmParams& p, int64_t t, bool& f) {
    const uint64_t m = p.smeta[t];
    f = (m & 1ull) != 0;
    return Em{p.sp[t], p.sq[t], p.sr[t], p.scnt[t], (uint32_t)(m >> 1) & kEwmNf};
}

template <bool ADJ>
__global__ __launch_bounds__(kTotalsThreads) void ewm_totals_kernel(EwmParams p) {
    __shared__ uint64_t wa[kTotalsThreads / 64], wb[kTotalsThreads / 64];
    __shared__ Em wv[kTotalsThreads / 64];
    __shared__ uint32_t wf[kTotalsThreads / 64];
    int64_t lo, hi;
    totals_span(p.tiles, lo, hi);
    uint64_t a = 0ull, b = 0ull;
    if constexpr (!ADJ) {
        for (int64_t t = lo; t < hi; ++t) {
            a = fill_max(a, p.cj[t]);
            b = fill_max(b, p.cs[t]);
        }
        fill_block_excl_max(a, b, wa, wb);
    }
    bool f = false;
    Em run = em_id<ADJ>();
    for (int64_t t = lo; t < hi; ++t) {
        bool sf;
        Em s = ewm_summary(p, t, sf);
        if constexpr (!ADJ) {
            // the codes that enter the tile decide the map of the row the tile left out
            const uint64_t va = p.cj[t], vb = p.cs[t], pc = p.sfirst[t];
            p.cj[t] = a;
            p.cs[t] = b;
            if (!sf && pc != 0ull) {
                Em m = em_id<ADJ>();
                m.p = (a != 0ull && a >= b) ? ewm_gap_f(p, p.ignore_nulls ? 0ull : pc - a - 1ull) : 1.0;
                m.q = m.p * p.sx1[t];
                s = em_comb<ADJ>(m, s);
                p.sp[t] = s.p;
                p.sq[t] = s.q;
            }
            a = fill_max(a, va);
            b = fill_max(b, vb);
        }
        seg_comb<EmOp<ADJ>>(f, run, sf, s);
    }
    bool ef, tf;
    Em ev, tv;
    block_seg_scan<EmOp<ADJ>>(f, run, wv, wf, ef, ev, tf, tv);
    // the carry of tile t: the running map before it
    for (int64_t t = lo; t < hi; ++t) {
        bool sf;
        const Em s = ewm_summary(p, t, sf);
        p.sp[t] = ev.p;
        p.sq[t] = ev.q;
        p.sr[t] = ev.r;
        p.scnt[t] = ev.cnt;
        p.smeta[t] = (uint64_t)ev.fl << 1;
        seg_comb<EmOp<ADJ>>(ef, ev, sf, s);
    }
}

template <bool ADJ, bool F32, bool SEG>
__global__ __launch_bounds__(kTileThreads) void ewm_apply_kernel(EwmParams p) {
    using T = typename std::conditional<F32, float, double>::type;
    __shared__ uint64_t sV[kTileWords], sS[kTileWords], sJ[kTileWords], sT[kTileWords];
    __shared__ uint64_t wa[kTileThreads / 64], wb[kTileThreads / 64];
    __shared__ Em wv[kTileThreads / 64];
    __shared__ uint32_t wf[kTileThreads / 64];
    const int64_t tile = blockIdx.x;
    uint64_t tj, ts;
    ewm_tile_words<ADJ>(p, tile, SEG, ADJ ? 0ull : p.cj[tile], ADJ ? 0ull : p.cs[tile], sV, sS, sJ, sT, wa, wb, tj, ts);
    // the running map before the block: the tile's carry, then the blocks before this one
    bool cf = false, sf0;
    Em cy = ewm_summary(p, tile, sf0);
    T* dst = (T*)p.out;
    const int64_t padded = (p.n + 63) / 64 * 64;
    for (int j = 0; j < kTileBlocks; ++j) {
        const int64_t first = tile * kTileRows + (int64_t)j * kTileBlock;
        if (first >= p.n) break;
        const int64_t base = first + (int64_t)threadIdx.x * kTilePer;
        EwmRows r;
        ewm_load<ADJ, F32, false>(p, tile, j, sV, sS, sJ, sT, r, nullptr, nullptr);
        bool f = false;
        Em run = em_id<ADJ>();
        ewm_fold<ADJ>(p, r, f, run);
        bool seen, tf;
        Em ev, tv;
        block_seg_scan<EmOp<ADJ>>(f, run, wv, wf, seen, ev, tf, tv);
        if (!seen) ev = em_comb<ADJ>(cy, ev);
        T o[kTilePer];
        uint32_t ob = 0u;
#pragma unroll
        for (int k = 0; k < kTilePer; ++k) {
            const bool valid = (r.vb >> k) & 1u, start = (r.sb >> k) & 1u;
            const bool nf_before = !start && (ev.fl & kEwmNf) != 0u;
            seg_comb<EmOp<ADJ>>(seen, ev, start, ewm_elem<ADJ>(p, r, k));
            double d = 0.0;
            if (valid) {
                // the first non-finite value of a segment comes out as itself, every later row as
                // NaN; the first non-null row of a segment as itself
                if (nf_before) d = __builtin_nan("");
                else if (((r.nf >> k) & 1u) || ev.cnt == 1ull) d = r.x[k];
                else d = ADJ ? ev.q / ev.r : ev.q;
                if (ev.cnt >= p.min_count) ob |= 1u << k;
            }
            o[k] = (T)d;  // Float32: computed in f64, rounded once here
        }
        seg_comb<EmOp<ADJ>>(cf, cy, tf, tv);  // the carry of the next block
        if (base >= p.n) {  // the rest of the last validity word
            if (base < padded) p.out_valid[base >> 3] = 0;
            continue;
        }
        if (base + kTilePer <= p.n) {  // an owned buffer, base a multiple of 8: 16-byte aligned
            if constexpr (F32) {
                float4* d4 = (float4*)(dst + base);
                d4[0] = make_float4(o[0], o[1], o[2], o[3]);
                d4[1] = make_float4(o[4], o[5], o[6], o[7]);
            } else {
                double2* d2 = (double2*)(dst + base);
#pragma unroll
                for (int k = 0; k < kTilePer / 2; ++k) d2[k] = make_double2(o[2 * k], o[2 * k + 1]);
            }
        } else {
#pragma unroll
            for (int k = 0; k < kTilePer; ++k)
                if (base + k < p.n) dst[base + k] = o[k];
        }
        p.out_valid[base >> 3] = (uint8_t)ob;  // rows past the column: zero bits
    }
}

template <bool ADJ, bool F32>
void ewm_launch(const EwmParams& p, hipStream_t s) {
    const unsigned g = (unsigned)p.tiles;
    {
        KtScope kt("ewm_reduce_kernel", s);
        ewm_reduce_kernel<ADJ, F32><<<g, kTileThreads, 0, s>>>(p);
    }
    {
        KtScope kt("ewm_totals_kernel", s);
        ewm_totals_kernel<ADJ><<<1, kTotalsThreads, 0, s>>>(p);
    }
    {
        KtScope kt("ewm_apply_kernel", s);
        if (p.seg) ewm_apply_kernel<ADJ, F32, true><<<g, kTileThreads, 0, s>>>(p);
        else ewm_apply_kernel<ADJ, F32, false><<<g, kTileThreads, 0, s>>>(p);
    }
}

}  // namespace
}  // namespace plgpu

using namespace plgpu;

PLGPU_API int plgpu_ewm_mean(const plgpu_column* values, const plgpu_column* seg_starts, double alpha, int32_t adjust,
                             int32_t ignore_nulls, int64_t min_samples, plgpu_column* out, void* stream) {
    hipStream_t s = as_stream(stream);
    if (values == nullptr || out == nullptr) return fail(PLGPU_ERR_INVALID, "NULL argument");
    std::memset(out, 0, sizeof *out);
    if (!(alpha > 0.0 && alpha <= 1.0)) return fail(PLGPU_ERR_INVALID, "ewm_mean: alpha must lie in (0, 1]");
    if (min_samples < 0) return fail(PLGPU_ERR_INVALID, "ewm_mean: min_samples must not be negative");
    if (seg_starts != nullptr) {
        const int rc = seg_check(values, seg_starts, PLGPU_ERR_INVALID, PLGPU_ERR_INVALID);
        if (rc) return rc;
    }
    const int32_t dt = values->dtype;
    if (dt != PLGPU_F32 && dt != PLGPU_F64) return fail(PLGPU_ERR_SCHEMA, "ewm_mean input must be Float32 / Float64");
    const int64_t n = values->length;
    int rc = make_owned_column(out, dt, n, true, s);
    if (rc || n == 0) return rc;
    EwmParams p;
    std::memset(&p, 0, sizeof p);
    p.values = values->values;
    p.voff = values->offset;
    if (values->validity != nullptr) {
        p.valid = values->validity;
        p.valid_off = values->offset;
        p.valid_bytes = (values->offset + n + 7) / 8;
    }
    if (seg_starts != nullptr) {
        p.seg = (const uint8_t*)seg_starts->values;
        p.seg_off = seg_starts->offset;
        p.seg_bytes = (seg_starts->offset + n + 7) / 8;
    }
    p.n = n;
    p.alpha = alpha;
    p.decay = 1.0 - alpha;
    p.f0 = alpha / (p.decay + alpha);
    p.ignore_nulls = ignore_nulls != 0;
    p.min_count = (uint64_t)std::max<int64_t>(min_samples, 1);
    p.out = (void*)out->values;
    p.out_valid = (uint8_t*)out->validity;
    p.tiles = (n + kTileRows - 1) / kTileRows;
    DevBuf<uint64_t> words;
    rc = words.alloc((size_t)p.tiles * 8 * 9, s);
    if (!rc) {
        uint64_t* w = words;
        p.sp = (double*)w;
        p.sq = (double*)(w + p.tiles);
        p.sr = (double*)(w + 2 * p.tiles);
        p.scnt = w + 3 * p.tiles;
        p.smeta = w + 4 * p.tiles;
        p.sx1 = (double*)(w + 5 * p.tiles);
        p.sfirst = w + 6 * p.tiles;
        p.cj = w + 7 * p.tiles;
        p.cs = w + 8 * p.tiles;
        const bool f32 = dt == PLGPU_F32;
        if (adjust) {
            if (f32) ewm_launch<true, true>(p, s);
            else ewm_launch<true, false>(p, s);
        } else {
            if (f32) ewm_launch<false, true>(p, s);
            else ewm_launch<false, false>(p, s);
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "ewm_mean");
    }
    if (rc) plgpu_column_release(out);
    else out->null_count = -1;
    return rc;
}
