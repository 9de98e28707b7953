// Ranks of one column, plain or per segment (rank, rank(...).over(keys)), from
// its stable sort: the five tie methods average / min / max / dense / ordinal.
//
// Reference (paths under the polars crates):
//   polars-ops/src/series/ops/rank.rs:68 rank, :32 rank_impl and the flush
//   closures at :113-:186 (average at :154: 0.5 * (first + last)); the sort is
//   polars-core/src/chunked_array/ops/sort/arg_sort.rs:7 with the stable
//   sort_by of sort/mod.rs:71; over groups
//   polars-expr/src/expressions/window.rs:356 with GroupsToRows.
//
// MI355X design (DESIGN.md "Rank"): the caller sorts (plgpu_arg_sort*), gathers
// and marks the runs of equal values (plgpu_segment_starts); what is left is a
// scan over bitmaps alone, and one scatter.  For sorted row j let s be the last
// segment start <= j, a the last tie start <= j and b the next tie start > j
// (n when there is none); a segment start is a tie start.
//   ordinal  j - s + 1              min      a - s + 1
//   max      b - s                  average  0.5 * ((double)min + (double)max)
//   dense    the tie starts in [s, j]
// s and a are forward running maxima of row codes (row + 1, 0 for none), b a
// backward one (kRevTop - row), as in fill.hip; dense is a segmented sum of
// popcounts.  Every kernel is a template on the method and carries only what
// that method reads: ordinal s alone, dense the sum alone.
//
// Three launches, none of which waits on another workgroup.
// rank_reduce_kernel reads the start bitmaps alone, one 64-row word per
// thread, and leaves the codes and the sum of its tile of kTileRows rows;
// rank_totals_kernel (one workgroup) turns them into every tile's carries, the
// forward ones and the backward one; rank_apply_kernel scans the per-word
// codes of its tile, adds the carries, reads sorted_idx once and writes every
// non-null sorted row's rank at out[sorted_idx[j]]: the scatter to row order
// is the kernel's own store.  The same kernel copies the validity of `values`
// to the output, realigned to bit 0.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>

#include "plgpu_internal.hpp"
#include "seg_scan.hpp"

namespace plgpu {
namespace {

struct RankParams {
    const uint32_t* idx;   // sorted_idx, the slice's first element
    const uint8_t* nv;     // validity of sorted_values (nullptr: no nulls); sorted row j is bit nv_off + j
    int64_t nv_off;
    int64_t nv_bytes;
    const uint8_t* tie;    // tie starts; sorted row j is bit tie_off + j
    int64_t tie_off;
    int64_t tie_bytes;
    const uint8_t* seg;    // segment starts (nullptr: one segment); sorted row j is bit seg_off + j
    int64_t seg_off;
    int64_t seg_bytes;
    const uint8_t* valid;  // validity of values (nullptr: none); row r is bit valid_off + r
    int64_t valid_off;
    int64_t valid_bytes;
    int64_t n;
    void* out;
    uint64_t* out_valid;   // whole 8-byte words (make_owned_column)
    // per tile: the summary (rank_reduce_kernel), then the carry (rank_totals_kernel)
    uint64_t* cs;          // code of the tile's last segment start
    uint64_t* ca;          // code of its last tie start
    uint64_t* cb;          // backward code of its first tie start
    uint32_t* cd;          // dense: tie starts from its last segment start on (of all its rows without one)
    uint32_t* cf;          // dense: the tile holds a segment start
    int64_t tiles;
};

template <int M>
struct RankNeeds {
    static constexpr bool S = M != PLGPU_RANK_DENSE;
    static constexpr bool A = M == PLGPU_RANK_MIN || M == PLGPU_RANK_AVERAGE;
    static constexpr bool B = M == PLGPU_RANK_MAX || M == PLGPU_RANK_AVERAGE;
    static constexpr bool D = M == PLGPU_RANK_DENSE;
};

// The operator of dense's segmented scan (seg_scan.hpp).
struct RankSum {
    using T = uint32_t;
    static __device__ __forceinline__ uint32_t id() { return 0u; }
    static __device__ __forceinline__ uint32_t comb(const uint32_t& l, const uint32_t& r) { return l + r; }
    static __device__ __forceinline__ uint32_t shfl_up(const uint32_t& x, int off) { return __shfl_up(x, off, 64); }
};

// Tie-start bits T and segment-start bits S of sorted rows [64 w, 64 w + 64),
// zero past the column.  Row 0 starts a segment whatever the caller's bitmaps
// say, and a segment start is a tie start.
__device__ __forceinline__ void rank_words(const RankParams& p, int64_t w, uint64_t& T, uint64_t& S) {
    const int64_t r0 = w * 64;
    T = 0ull;
    S = 0ull;
    if (r0 >= p.n) return;
    const uint64_t m = fill_lowmask(p.n - r0);
    if (p.seg != nullptr) S = fill_bits64(p.seg, p.seg_bytes, p.seg_off + r0) & m;
    if (w == 0) S |= 1ull;
    T = (fill_bits64(p.tie, p.tie_bytes, p.tie_off + r0) & m) | S;
}

// The tie starts of a word from its last segment start on (all of them when it
// has none): the word's value in dense's segmented sum.
__device__ __forceinline__ uint32_t rank_word_count(uint64_t T, uint64_t S) {
    return (uint32_t)__popcll(S ? T >> (63 - __clzll((long long)S)) : T);
}

template <int M>
__global__ __launch_bounds__(kTileThreads) void rank_reduce_kernel(RankParams p) {
    using Need = RankNeeds<M>;
    __shared__ uint64_t ws[kTileThreads / 64], wa[kTileThreads / 64], wb[kTileThreads / 64];
    __shared__ uint32_t wv[kTileThreads / 64], wf[kTileThreads / 64];
    const int64_t tile = blockIdx.x;
    const int64_t w = tile * kTileWords + threadIdx.x;
    uint64_t T, S;
    rank_words(p, w, T, S);
    if constexpr (Need::D) {
        bool ef, tf;
        uint32_t ev, tv;
        block_seg_scan<RankSum>(S != 0ull, rank_word_count(T, S), wv, wf, ef, ev, tf, tv);
        if (threadIdx.x == 0) {
            p.cd[tile] = tv;
            p.cf[tile] = tf ? 1u : 0u;
        }
    } else {
        uint64_t s = fill_word_code<false>(S, w * 64);
        uint64_t a = Need::A ? fill_word_code<false>(T, w * 64) : 0ull;
        uint64_t b = Need::B ? fill_word_code<true>(T, w * 64) : 0ull;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            s = fill_max(s, __shfl_xor(s, off, 64));
            if constexpr (Need::A) a = fill_max(a, __shfl_xor(a, off, 64));
            if constexpr (Need::B) b = fill_max(b, __shfl_xor(b, off, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            ws[threadIdx.x >> 6] = s;
            wa[threadIdx.x >> 6] = a;
            wb[threadIdx.x >> 6] = b;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 1; k < kTileThreads / 64; ++k) {
                s = fill_max(s, ws[k]);
                a = fill_max(a, wa[k]);
                b = fill_max(b, wb[k]);
            }
            p.cs[tile] = s;
            if constexpr (Need::A) p.ca[tile] = a;
            if constexpr (Need::B) p.cb[tile] = b;
        }
    }
}

template <int M>
__global__ __launch_bounds__(kTotalsThreads) void rank_totals_kernel(RankParams p) {
    using Need = RankNeeds<M>;
    __shared__ uint64_t wa[kTotalsThreads / 64], wb[kTotalsThreads / 64];
    __shared__ uint32_t wv[kTotalsThreads / 64], wf[kTotalsThreads / 64];
    int64_t lo, hi;
    totals_span(p.tiles, lo, hi);
    if constexpr (Need::D) {
        bool f = false;
        uint32_t v = 0u;
        for (int64_t q = lo; q < hi; ++q) seg_comb<RankSum>(f, v, p.cf[q] != 0u, p.cd[q]);
        bool ef, tf;
        uint32_t c, tv;
        block_seg_scan<RankSum>(f, v, wv, wf, ef, c, tf, tv);
        // the carry of a tile: the tie starts since the last segment start before it
        for (int64_t q = lo; q < hi; ++q) {
            const uint32_t vq = p.cd[q];
            const bool fq = p.cf[q] != 0u;
            p.cd[q] = c;
            c = fq ? vq : c + vq;
        }
    } else {
        // forward: the carry of a tile is the maximum of the tiles before it
        uint64_t s = 0ull, a = 0ull;
        for (int64_t q = lo; q < hi; ++q) {
            s = fill_max(s, p.cs[q]);
            if constexpr (Need::A) a = fill_max(a, p.ca[q]);
        }
        fill_block_excl_max(s, a, wa, wb);
        for (int64_t q = lo; q < hi; ++q) {
            const uint64_t vs = p.cs[q];
            p.cs[q] = s;
            s = fill_max(s, vs);
            if constexpr (Need::A) {
                const uint64_t va = p.ca[q];
                p.ca[q] = a;
                a = fill_max(a, va);
            }
        }
        if constexpr (Need::B) {
            // backward: position q of the scan is tile tiles - 1 - q
            uint64_t b = 0ull, z = 0ull;
            for (int64_t q = lo; q < hi; ++q) b = fill_max(b, p.cb[p.tiles - 1 - q]);
            fill_block_excl_max(b, z, wa, wb);
            for (int64_t q = lo; q < hi; ++q) {
                const int64_t t = p.tiles - 1 - q;
                const uint64_t vb = p.cb[t];
                p.cb[t] = b;
                b = fill_max(b, vb);
            }
        }
    }
}

template <int M>
__global__ __launch_bounds__(kTileThreads) void rank_apply_kernel(RankParams p) {
    using Need = RankNeeds<M>;
    using Out = typename std::conditional<M == PLGPU_RANK_AVERAGE, double, uint32_t>::type;
    __shared__ uint64_t sT[kTileWords], sS[kTileWords], sN[kTileWords];
    __shared__ uint64_t sSc[kTileWords], sA[kTileWords], sB[kTileWords];
    __shared__ uint32_t sD[kTileWords];
    __shared__ uint64_t wa[kTileThreads / 64], wb[kTileThreads / 64];
    __shared__ uint32_t wv[kTileThreads / 64], wf[kTileThreads / 64];
    const int64_t tile = blockIdx.x;
    const int t = threadIdx.x;
    {
        // the codes that enter every word of the tile
        const int64_t w = tile * kTileWords + t;
        const int64_t r0 = w * 64;
        uint64_t T, S;
        rank_words(p, w, T, S);
        sT[t] = T;
        sS[t] = S;
        uint64_t nv = 0ull;
        if (r0 < p.n) {
            const uint64_t m = fill_lowmask(p.n - r0);
            nv = p.nv != nullptr ? fill_bits64(p.nv, p.nv_bytes, p.nv_off + r0) & m : m;
            // the output's validity: that of `values`, from bit 0
            if (p.valid != nullptr) p.out_valid[w] = fill_bits64(p.valid, p.valid_bytes, p.valid_off + r0) & m;
        }
        sN[t] = nv;
        if constexpr (Need::D) {
            bool ef, tf;
            uint32_t ev, tv;
            block_seg_scan<RankSum>(S != 0ull, rank_word_count(T, S), wv, wf, ef, ev, tf, tv);
            sD[t] = ef ? ev : p.cd[tile] + ev;
        } else {
            uint64_t s = fill_word_code<false>(S, r0), a = Need::A ? fill_word_code<false>(T, r0) : 0ull;
            fill_block_excl_max(s, a, wa, wb);
            sSc[t] = fill_max(s, p.cs[tile]);
            if constexpr (Need::A) sA[t] = fill_max(a, p.ca[tile]);
            if constexpr (Need::B) {
                // backward: thread order is scan order (the syncs of the scan above order sT)
                const int wi = kTileWords - 1 - t;
                uint64_t b = fill_word_code<true>(sT[wi], (tile * kTileWords + wi) * 64), z = 0ull;
                fill_block_excl_max(b, z, wa, wb);
                sB[wi] = fill_max(b, p.cb[tile]);
            }
        }
    }
    __syncthreads();
    Out* dst = (Out*)p.out;
    const bool aligned = ((uintptr_t)p.idx & 15u) == 0;
    for (int blk = 0; blk < kTileBlocks; ++blk) {
        const int64_t first = tile * kTileRows + (int64_t)blk * kTileBlock;
        if (first >= p.n) break;
        const int64_t base = first + (int64_t)t * kTilePer;
        const int wi = blk * (kTileBlock / 64) + (t >> 3);
        const int b0 = (t & 7) * kTilePer;  // the thread's rows are bits b0 .. b0 + 7 of the word
        const uint32_t nb = (uint32_t)(sN[wi] >> b0) & 0xFFu;
        if (nb == 0u) continue;  // nulls only, or past the column: nothing to write
        const uint64_t T = sT[wi], S = sS[wi];
        const uint32_t tb = (uint32_t)(T >> b0) & 0xFFu, sb = (uint32_t)(S >> b0) & 0xFFu;
        (void)tb;
        (void)sb;
        uint32_t x[kTilePer];
        if (base + kTilePer <= p.n && aligned) {
            load_vec8(p.idx + base, x);
        } else {
#pragma unroll
            for (int k = 0; k < kTilePer; ++k) x[k] = base + k < p.n ? p.idx[base + k] : 0u;
        }
        const int64_t r0 = (tile * kTileWords + wi) * 64;
        const uint64_t before = (1ull << b0) - 1ull;
        // the rows (and the count) that enter the thread's rows: the word's
        // bits before them in scan order, else the word's own entry codes
        const uint64_t ms = S & before, mt = T & before;
        int64_t srow = 0, arow = 0;
        uint32_t dc = 0u;
        if constexpr (Need::S) srow = (int64_t)(ms ? fill_word_code<false>(ms, r0) : sSc[wi]) - 1;
        if constexpr (Need::A) arow = (int64_t)(mt ? fill_word_code<false>(mt, r0) : sA[wi]) - 1;
        if constexpr (Need::D) dc = ms ? (uint32_t)__popcll(mt >> (63 - __clzll((long long)ms))) : sD[wi] + (uint32_t)__popcll(mt);
        int64_t brow[kTilePer];
        if constexpr (Need::B) {
            const uint64_t after = b0 + kTilePer == 64 ? 0ull : ~0ull << (b0 + kTilePer);
            const uint64_t mb = T & after;
            const uint64_t bc = mb ? fill_word_code<true>(mb, r0) : sB[wi];
            int64_t b = bc ? (int64_t)(kRevTop - bc) : p.n;
#pragma unroll
            for (int k = kTilePer - 1; k >= 0; --k) {
                brow[k] = b;
                if ((tb >> k) & 1u) b = base + k;
            }
        }
#pragma unroll
        for (int k = 0; k < kTilePer; ++k) {
            const int64_t i = base + k;
            if constexpr (Need::S) {
                if ((sb >> k) & 1u) srow = i;
            }
            if constexpr (Need::A) {
                if ((tb >> k) & 1u) arow = i;
            }
            if constexpr (Need::D) {
                if ((sb >> k) & 1u) dc = 0u;
                if ((tb >> k) & 1u) ++dc;
            }
            Out r;
            if constexpr (M == PLGPU_RANK_ORDINAL) r = (uint32_t)(i - srow + 1);
            else if constexpr (M == PLGPU_RANK_MIN) r = (uint32_t)(arow - srow + 1);
            else if constexpr (M == PLGPU_RANK_MAX) r = (uint32_t)(brow[k] - srow);
            else if constexpr (M == PLGPU_RANK_DENSE) r = dc;
            else r = 0.5 * ((double)(uint32_t)(arow - srow + 1) + (double)(uint32_t)(brow[k] - srow));
            // (a row id outside the column is not a permutation's: never stored)
            if (((nb >> k) & 1u) && (int64_t)x[k] < p.n) dst[x[k]] = r;
        }
    }
}

template <int M>
void rank_launch(const RankParams& p, hipStream_t s) {
    const unsigned g = (unsigned)p.tiles;
    {
        KtScope kt("rank_reduce_kernel", s);
        rank_reduce_kernel<M><<<g, kTileThreads, 0, s>>>(p);
    }
    {
        KtScope kt("rank_totals_kernel", s);
        rank_totals_kernel<M><<<1, kTotalsThreads, 0, s>>>(p);
    }
    {
        KtScope kt("rank_apply_kernel", s);
        rank_apply_kernel<M><<<g, kTileThreads, 0, s>>>(p);
    }
}

int rank_starts_check(const plgpu_column* c, int64_t n, const char* what) {
    if (c->dtype != PLGPU_BOOL || c->validity != nullptr)
        return fail(PLGPU_ERR_INVALID, std::string("rank: ") + what + " must be a null-free Boolean column");
    if (c->length != n) return fail(PLGPU_ERR_INVALID, std::string("rank: ") + what + " and values must have equal lengths");
    return PLGPU_OK;
}

}  // namespace
}  // namespace plgpu

using namespace plgpu;

PLGPU_API int plgpu_rank(const plgpu_column* sorted_idx, const plgpu_column* sorted_values,
                         const plgpu_column* tie_starts, const plgpu_column* seg_starts, const plgpu_column* values,
                         int32_t method, plgpu_column* out, void* stream) {
    hipStream_t s = as_stream(stream);
    if (sorted_idx == nullptr || sorted_values == nullptr || tie_starts == nullptr || values == nullptr ||
        out == nullptr)
        return fail(PLGPU_ERR_INVALID, "NULL argument");
    std::memset(out, 0, sizeof *out);
    if (method < PLGPU_RANK_AVERAGE || method > PLGPU_RANK_ORDINAL)
        return fail(PLGPU_ERR_INVALID, "unknown rank method");
    const int64_t n = values->length;
    if (sorted_idx->dtype != PLGPU_U32 || sorted_idx->validity != nullptr)
        return fail(PLGPU_ERR_INVALID, "rank: the sorted index must be a null-free UInt32 column");
    if (sorted_idx->length != n || sorted_values->length != n)
        return fail(PLGPU_ERR_INVALID, "rank: the sorted index, the sorted values and values must have equal lengths");
    int rc = rank_starts_check(tie_starts, n, "tie starts");
    if (rc) return rc;
    if (seg_starts != nullptr && (rc = rank_starts_check(seg_starts, n, "segment starts"))) return rc;
    if (n < 0 || n > (int64_t)UINT32_MAX) return fail(PLGPU_ERR_INVALID, "rank: more rows than a UInt32 rank counts");
    const bool nullable = values->validity != nullptr;
    const bool avg = method == PLGPU_RANK_AVERAGE;
    rc = make_owned_column(out, avg ? PLGPU_F64 : PLGPU_U32, n, nullable, s);
    if (rc || n == 0) return rc;
    RankParams p;
    std::memset(&p, 0, sizeof p);
    p.idx = (const uint32_t*)sorted_idx->values + sorted_idx->offset;
    p.nv = sorted_values->validity;
    p.nv_off = sorted_values->offset;
    p.nv_bytes = (sorted_values->offset + n + 7) / 8;
    p.tie = (const uint8_t*)tie_starts->values;
    p.tie_off = tie_starts->offset;
    p.tie_bytes = (tie_starts->offset + n + 7) / 8;
    if (seg_starts != nullptr) {
        p.seg = (const uint8_t*)seg_starts->values;
        p.seg_off = seg_starts->offset;
        p.seg_bytes = (seg_starts->offset + n + 7) / 8;
    }
    p.valid = values->validity;
    p.valid_off = values->offset;
    p.valid_bytes = (values->offset + n + 7) / 8;
    p.n = n;
    p.out = (void*)out->values;
    p.out_valid = (uint64_t*)out->validity;
    p.tiles = (n + kTileRows - 1) / kTileRows;
    DevBuf<uint64_t> carry;
    rc = carry.alloc((size_t)p.tiles * 8 * 4, s);
    hipError_t e = hipSuccess;
    if (!rc) {
        p.cs = carry;
        p.ca = p.cs + p.tiles;
        p.cb = p.ca + p.tiles;
        p.cd = (uint32_t*)(p.cb + p.tiles);
        p.cf = p.cd + p.tiles;
        // a null row is never stored to: its bytes are zero
        if (p.nv != nullptr || nullable) e = hipMemsetAsync((void*)out->values, 0, (size_t)n * (avg ? 8 : 4), s);
        if (e == hipSuccess) {
            switch (method) {
            case PLGPU_RANK_AVERAGE: rank_launch<PLGPU_RANK_AVERAGE>(p, s); break;
            case PLGPU_RANK_MIN: rank_launch<PLGPU_RANK_MIN>(p, s); break;
            case PLGPU_RANK_MAX: rank_launch<PLGPU_RANK_MAX>(p, s); break;
            case PLGPU_RANK_DENSE: rank_launch<PLGPU_RANK_DENSE>(p, s); break;
            default: rank_launch<PLGPU_RANK_ORDINAL>(p, s); break;
            }
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "rank");
    }
    if (rc) plgpu_column_release(out);
    return rc;
}
