// As-of join: for every left row the one right row whose `on` key is the
// closest at or before (backward), at or after (forward) or on either side
// (nearest) of the left key, optionally inside a per-row range of the right
// column (the `by` groups) and within a tolerance.
//
// Reference (paths under the polars crates):
//   polars-ops/src/frame/join/asof/mod.rs:46-199 the three AsofJoinState
//   machines, default.rs:11 join_asof_impl and :112 join_asof_numeric (the
//   tolerance as a filter), groups.rs:38 asof_in_group.
//
// MI355X design (DESIGN.md "As-of join"): the reference scans both sides with
// one running state; for ascending right keys its answer is a pure function of
// each left key, a lower or an upper bound in the right keys, so every left
// row is searched on its own.  lb(x): the first position whose value is >= x,
// ub(x): the first whose value is > x, both under TotalOrd for floats
// (-0.0 == 0.0, NaN greatest and equal to itself).
//   backward  ub(l) - 1 (allow_eq) or lb(l) - 1
//   forward   lb(l) (allow_eq) or ub(l)
//   nearest   an equal value's last position (allow_eq); else lower =
//             lb(l) - 1 and upper = the last of the run of equal values that
//             begins at ub(l), upper where |l - upper| <= |l - lower|
// and then the tolerance keeps or drops the one match.
//
// asof_staged_kernel (no ranges): one workgroup per tile of kAsofTile left
// rows.  The tile reduces the minimum and maximum of its non-null keys, two
// searches of the right column, one wave each, turn them into the window those
// rows can touch (one below lb(min) through ub(max), nearest one more), a
// window of at most kAsofLds values is copied to LDS with 16-byte loads and
// searched there, a larger one is searched in place.  asof_ranged_kernel (`by`
// groups): every row searches its own clamped [lo, hi).  asof_sorted_kernel:
// one pass that tells whether a column is ascending with its nulls first and
// where its first non-null row is.  No workgroup waits on another; a thread's
// search halves at most 32 times, a wave's takes at most 6 steps.
#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>

#include "plgpu_internal.hpp"

namespace plgpu {
namespace {

constexpr int kAsofThreads = 256;
constexpr int kAsofPer = 8;                          // left rows per thread, kAsofThreads apart
constexpr int kAsofTile = kAsofThreads * kAsofPer;   // left rows per workgroup (_native.py ASOF_TILE_ROWS)
constexpr int kAsofLds = 2048;                       // right values a tile stages (_native.py ASOF_LDS_VALUES)
constexpr int kAsofHalvings = 33;                    // bound of every search loop (a range below 2^32 needs 32)

constexpr uint64_t kSortedDesc = 1ull;               // a non-null value is smaller than the non-null value before it
constexpr uint64_t kSortedNullAfter = 2ull;          // a null follows a non-null row

struct AsofParams {
    const void* left;        // first element of the slice
    const uint8_t* lvalid;   // nullptr: no nulls; row r is bit lvoff + r
    int64_t lvoff;
    int64_t n_left;
    const void* right;       // first element of the slice
    uint32_t n_right;
    const uint64_t* rscan;   // nullptr: the right column has no nulls; else asof_sorted_kernel's words
    const uint32_t* lo;      // ranged: per left row
    const uint32_t* hi;
    const uint32_t* rrows;   // nullptr: a position is the row
    int32_t allow_eq;
    int32_t has_tol;
    uint64_t tol_u;          // |tolerance| of an integer key
    double tol_f;            // |tolerance| of a float key
    int32_t whole;           // staged kernel: 1 every row searches the whole non-null run (asof_path 2)
    uint32_t* out;
    uint64_t* out_valid;
};

// Order, equality and distance of one key type.
template <class K, bool FLT = std::is_floating_point<K>::value>
struct AsofOrd {
    using D = uint64_t;
    static __device__ __forceinline__ bool lt(K a, K b) { return a < b; }
    static __device__ __forceinline__ bool eq(K a, K b) { return a == b; }
    // the exact unsigned difference (num-traits abs_diff of the reference)
    static __device__ __forceinline__ D diff(K a, K b) {
        return a > b ? (uint64_t)a - (uint64_t)b : (uint64_t)b - (uint64_t)a;
    }
    static __device__ __forceinline__ D tol(const AsofParams& p) { return p.tol_u; }
};
template <class K>
struct AsofOrd<K, true> {
    using D = K;
    // TotalOrd: NaN greatest, NaN == NaN, -0.0 == 0.0
    static __device__ __forceinline__ bool lt(K a, K b) { return !__builtin_isnan(a) && (__builtin_isnan(b) || a < b); }
    static __device__ __forceinline__ bool eq(K a, K b) { return __builtin_isnan(a) ? __builtin_isnan(b) : a == b; }
    // |a - b| rounded in the key's own type; a NaN difference passes no `<=`
    static __device__ __forceinline__ D diff(K a, K b) {
        const K d = a - b;
        if constexpr (sizeof(K) == 4) return __builtin_fabsf(d);
        else return __builtin_fabs(d);
    }
    static __device__ __forceinline__ D tol(const AsofParams& p) { return (K)p.tol_f; }
};

// lb (UPPER false) / ub (UPPER true) of x in a[lo, hi).
template <class K, bool UPPER>
__device__ __forceinline__ uint32_t asof_bound(const K* a, uint32_t lo, uint32_t hi, K x) {
    using O = AsofOrd<K>;
    uint32_t n = hi - lo;
    for (int it = 0; it < kAsofHalvings && n != 0u; ++it) {
        const uint32_t half = n >> 1;
        const K v = a[lo + half];
        const bool after = UPPER ? !O::lt(x, v) : O::lt(v, x);
        if (after) {
            lo += half + 1u;
            n -= half + 1u;
        } else {
            n = half;
        }
    }
    return lo;
}

// The same bound found by a whole wave (every lane active, uniform arguments):
// each step 64 lanes probe 64 evenly spaced positions and the ballot keeps one
// of the 65 pieces, so 2^32 positions take at most 6 steps of one load each
// where the halving search takes 32.  On an unsorted column the pieces still
// nest, so every probe stays inside [lo, hi).
constexpr int kAsofWaveSteps = 7;
template <class K, bool UPPER>
__device__ __forceinline__ uint32_t asof_bound_wave(const K* a, uint32_t lo, uint32_t hi, K x) {
    using O = AsofOrd<K>;
    const uint32_t lane = threadIdx.x & 63u;
    for (int it = 0; it < kAsofWaveSteps; ++it) {
        const uint32_t n = hi - lo;
        if (n <= 64u) {
            bool after = false;
            if (lane < n) {
                const K v = a[lo + lane];
                after = UPPER ? !O::lt(x, v) : O::lt(v, x);
            }
            return lo + (uint32_t)__popcll(__ballot(after));
        }
        const K v = a[lo + (uint32_t)(((uint64_t)(lane + 1u) * n) / 65u)];
        const bool after = UPPER ? !O::lt(x, v) : O::lt(v, x);
        const uint32_t c = (uint32_t)__popcll(__ballot(after));  // the answer lies beyond c of the probes
        const uint32_t nlo = c == 0u ? lo : lo + (uint32_t)(((uint64_t)c * n) / 65u) + 1u;
        const uint32_t nhi = c == 64u ? hi : lo + (uint32_t)(((uint64_t)(c + 1u) * n) / 65u);
        lo = nlo;
        hi = nhi;
    }
    return lo;
}

// The match of left key l in a[0, cnt), which is R[g0, g0 + cnt); a run of
// equal values may go on in R up to ext_end (nearest's upper).  pos: the
// match's position in R.
template <class K, int STRAT>
__device__ __forceinline__ bool asof_match(const K* a, uint32_t cnt, uint32_t g0, const K* R, uint32_t ext_end, K l,
                                           const AsofParams& p, uint32_t& pos) {
    using O = AsofOrd<K>;
    const bool eqok = p.allow_eq != 0;
    K rv;
    if constexpr (STRAT == PLGPU_ASOF_BACKWARD) {
        const uint32_t b = eqok ? asof_bound<K, true>(a, 0u, cnt, l) : asof_bound<K, false>(a, 0u, cnt, l);
        if (b == 0u) return false;
        rv = a[b - 1u];
        pos = g0 + b - 1u;
    } else if constexpr (STRAT == PLGPU_ASOF_FORWARD) {
        const uint32_t b = eqok ? asof_bound<K, false>(a, 0u, cnt, l) : asof_bound<K, true>(a, 0u, cnt, l);
        if (b >= cnt) return false;
        rv = a[b];
        pos = g0 + b;
    } else {
        const uint32_t pu = asof_bound<K, true>(a, 0u, cnt, l);
        if (eqok && pu > 0u && O::eq(a[pu - 1u], l)) {
            rv = a[pu - 1u];
            pos = g0 + pu - 1u;
        } else {
            // with allow_eq no value equals l here, so lb(l) == ub(l)
            const uint32_t pl = eqok ? pu : asof_bound<K, false>(a, 0u, cnt, l);
            const bool hl = pl > 0u, hu = pu < cnt;
            if (!hl && !hu) return false;
            const K lv = hl ? a[pl - 1u] : l, uv = hu ? a[pu] : l;
            uint32_t up = 0u;
            if (hu) {
                const uint32_t pe = asof_bound<K, true>(a, pu, cnt, uv);
                // the run reaches the end of what was searched: it may go on in the column
                up = (pe == cnt && g0 + cnt < ext_end) ? asof_bound<K, true>(R, g0 + cnt, ext_end, uv) - 1u
                                                      : g0 + pe - 1u;
            }
            const bool upper = hu && (!hl || O::diff(l, uv) <= O::diff(l, lv));
            rv = upper ? uv : lv;
            pos = upper ? up : g0 + pl - 1u;
        }
    }
    if (p.has_tol && !(O::diff(l, rv) <= O::tol(p))) return false;
    return true;
}

__device__ __forceinline__ bool asof_bit(const uint8_t* b, int64_t i) { return (b[i >> 3] >> (i & 7)) & 1; }

// One index and one validity bit per row of the pass; the wave's 64 bits are one word.
__device__ __forceinline__ void asof_store(const AsofParams& p, int64_t r, bool m, uint32_t pos) {
    const unsigned long long bits = __ballot(m);
    if (r < p.n_left) p.out[r] = m ? (p.rrows != nullptr ? p.rrows[pos] : pos) : 0u;
    const int64_t w0 = r - (threadIdx.x & 63);
    if ((threadIdx.x & 63) == 0 && w0 < p.n_left) p.out_valid[w0 >> 6] = bits;
}

template <class K, int STRAT>
__global__ __launch_bounds__(kAsofThreads) void asof_staged_kernel(AsofParams p) {
    using O = AsofOrd<K>;
    __shared__ K sv[kAsofLds];
    __shared__ K smin[kAsofThreads / 64], smax[kAsofThreads / 64];
    __shared__ uint32_t sany[kAsofThreads / 64];
    __shared__ uint32_t swin[2];
    const int t = threadIdx.x;
    const K* L = (const K*)p.left;
    const K* R = (const K*)p.right;
    const int64_t base = (int64_t)blockIdx.x * kAsofTile;
    // the non-null run of the right column: [r0, n_right)
    uint32_t r0 = 0u;
    if (p.rscan != nullptr) {
        const uint64_t f = p.rscan[1];
        r0 = f != 0ull ? (uint32_t)(f - 1ull) : p.n_right;
    }
    K key[kAsofPer];
    bool ok[kAsofPer];
#pragma unroll
    for (int j = 0; j < kAsofPer; ++j) {
        const int64_t r = base + (int64_t)j * kAsofThreads + t;
        ok[j] = r < p.n_left && (p.lvalid == nullptr || asof_bit(p.lvalid, p.lvoff + r));
        key[j] = ok[j] ? L[r] : K(0);
    }
    uint32_t wlo = r0, whi = p.n_right;
    if (!p.whole) {
        // the minimum and maximum of the tile's non-null keys, not its first and last row: an unsorted left stays correct
        bool any = false;
        K mn = K(0), mx = K(0);
#pragma unroll
        for (int j = 0; j < kAsofPer; ++j) {
            if (!ok[j]) continue;
            if (!any || O::lt(key[j], mn)) mn = key[j];
            if (!any || O::lt(mx, key[j])) mx = key[j];
            any = true;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const K omn = __shfl_xor(mn, off, 64), omx = __shfl_xor(mx, off, 64);
            const bool oany = __shfl_xor((int)any, off, 64) != 0;
            if (oany) {
                if (!any || O::lt(omn, mn)) mn = omn;
                if (!any || O::lt(mx, omx)) mx = omx;
                any = true;
            }
        }
        if ((t & 63) == 0) {
            smin[t >> 6] = mn;
            smax[t >> 6] = mx;
            sany[t >> 6] = any ? 1u : 0u;
        }
        __syncthreads();
        // wave 0 finds lb(min), wave 1 ub(max), each with all its lanes
        if (t < 128) {
            any = false;
            for (int w = 0; w < kAsofThreads / 64; ++w) {
                if (!sany[w]) continue;
                if (!any || O::lt(smin[w], mn)) mn = smin[w];
                if (!any || O::lt(mx, smax[w])) mx = smax[w];
                any = true;
            }
            uint32_t e = r0;
            if (any) {
                if (t < 64) {
                    const uint32_t lbm = asof_bound_wave<K, false>(R, r0, p.n_right, mn);
                    e = lbm > r0 ? lbm - 1u : r0;
                } else {
                    // through ub(max); nearest takes one more, so that a run of equal values which ends
                    // at ub(max) is seen to end inside the window
                    constexpr uint32_t extra = STRAT == PLGPU_ASOF_NEAREST ? 2u : 1u;
                    const uint32_t ubm = asof_bound_wave<K, true>(R, r0, p.n_right, mx);
                    e = p.n_right - ubm > extra ? ubm + extra : p.n_right;
                }
            }
            if ((t & 63) == 0) swin[t >> 6] = e;
        }
        __syncthreads();
        wlo = swin[0];
        whi = swin[1] < wlo ? wlo : swin[1];  // an unsorted right column: nothing is promised but bounds
    }
    const uint32_t cnt = whi - wlo;
    const bool staged = !p.whole && cnt <= (uint32_t)kAsofLds;
    if (staged) {
        // scalar rows up to the first 16-byte boundary, 16-byte loads, scalar rest
        constexpr uint32_t V = 16 / sizeof(K);
        const K* src = R + wlo;
        uint32_t head = (uint32_t)(((16u - ((uintptr_t)src & 15u)) & 15u) / sizeof(K));
        if (head > cnt) head = cnt;
        const uint32_t nvec = (cnt - head) / V;
        if ((uint32_t)t < head) sv[t] = src[t];
        for (uint32_t v = t; v < nvec; v += kAsofThreads) {
            const uint4 q = *(const uint4*)(src + head + v * V);
            K x[V];
            __builtin_memcpy(x, &q, 16);
#pragma unroll
            for (uint32_t c = 0; c < V; ++c) sv[head + v * V + c] = x[c];
        }
        for (uint32_t i = head + nvec * V + t; i < cnt; i += kAsofThreads) sv[i] = src[i];
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < kAsofPer; ++j) {
        const int64_t r = base + (int64_t)j * kAsofThreads + t;
        uint32_t pos = 0u;
        bool m = false;
        if (ok[j]) {
            m = staged ? asof_match<K, STRAT>(sv, cnt, wlo, R, p.n_right, key[j], p, pos)
                       : asof_match<K, STRAT>(R + wlo, cnt, wlo, R, p.n_right, key[j], p, pos);
        }
        asof_store(p, r, m, pos);
    }
}

template <class K, int STRAT>
__global__ __launch_bounds__(kAsofThreads) void asof_ranged_kernel(AsofParams p) {
    const K* L = (const K*)p.left;
    const K* R = (const K*)p.right;
    const int64_t r = (int64_t)blockIdx.x * kAsofThreads + threadIdx.x;
    uint32_t pos = 0u;
    bool m = false;
    if (r < p.n_left && (p.lvalid == nullptr || asof_bit(p.lvalid, p.lvoff + r))) {
        // clamped into [0, n_right]: a bad range cannot read outside the column
        uint32_t lo = p.lo[r], hi = p.hi[r];
        if (lo > p.n_right) lo = p.n_right;
        if (hi > p.n_right) hi = p.n_right;
        if (hi < lo) hi = lo;
        m = asof_match<K, STRAT>(R + lo, hi - lo, lo, R, hi, L[r], p, pos);
    }
    asof_store(p, r, m, pos);
}

// res[0] |= kSortedDesc / kSortedNullAfter; res[1] = 1 + the row of a non-null
// value that has no non-null row before it (the first non-null row when the
// nulls are a prefix; res zeroed before the launch, 0: every row is null).
template <class K>
__global__ __launch_bounds__(kAsofThreads) void asof_sorted_kernel(const K* v, const uint8_t* valid, int64_t voff,
                                                                   int64_t n, unsigned long long* res) {
    using O = AsofOrd<K>;
    const int64_t base = (int64_t)blockIdx.x * kAsofTile;
    unsigned long long bad = 0ull;
#pragma unroll
    for (int j = 0; j < kAsofPer; ++j) {
        const int64_t r = base + (int64_t)j * kAsofThreads + threadIdx.x;
        if (r >= n) continue;
        const bool ok = valid == nullptr || asof_bit(valid, voff + r);
        const bool pok = r > 0 && (valid == nullptr || asof_bit(valid, voff + r - 1));
        if (ok && pok && O::lt(v[r], v[r - 1])) bad |= kSortedDesc;
        if (!ok && pok) bad |= kSortedNullAfter;
        if (ok && !pok) res[1] = (unsigned long long)r + 1ull;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) bad |= __shfl_xor(bad, off, 64);
    if ((threadIdx.x & 63) == 0 && bad != 0ull) atomicOr(&res[0], bad);
}

template <class K>
void sorted_launch(const plgpu_column* c, unsigned long long* res, hipStream_t s) {
    const int64_t n = c->length;
    KtScope kt("asof_sorted_kernel", s);
    asof_sorted_kernel<K><<<(unsigned)((n + kAsofTile - 1) / kAsofTile), kAsofThreads, 0, s>>>(
        (const K*)c->values + c->offset, c->validity, c->offset, n, res);
}

bool asof_dtype(int32_t dt) {
    return dt == PLGPU_I64 || dt == PLGPU_I32 || dt == PLGPU_U32 || dt == PLGPU_U64 || dt == PLGPU_F64 ||
           dt == PLGPU_F32;
}

// Zeroes res (two words) and launches the scan of a non-empty column.
int sorted_scan(const plgpu_column* c, unsigned long long* res, hipStream_t s) {
    PLGPU_HIP(hipMemsetAsync(res, 0, 16, s));
    switch (c->dtype) {
    case PLGPU_I64: sorted_launch<int64_t>(c, res, s); break;
    case PLGPU_I32: sorted_launch<int32_t>(c, res, s); break;
    case PLGPU_U32: sorted_launch<uint32_t>(c, res, s); break;
    case PLGPU_U64: sorted_launch<uint64_t>(c, res, s); break;
    case PLGPU_F64: sorted_launch<double>(c, res, s); break;
    default: sorted_launch<float>(c, res, s); break;
    }
    return PLGPU_OK;
}

template <class K, int STRAT>
void asof_launch(const AsofParams& p, hipStream_t s) {
    if (p.lo != nullptr) {
        KtScope kt("asof_ranged_kernel", s);
        asof_ranged_kernel<K, STRAT><<<(unsigned)((p.n_left + kAsofThreads - 1) / kAsofThreads), kAsofThreads, 0, s>>>(p);
    } else {
        KtScope kt("asof_staged_kernel", s);
        asof_staged_kernel<K, STRAT><<<(unsigned)((p.n_left + kAsofTile - 1) / kAsofTile), kAsofThreads, 0, s>>>(p);
    }
}

template <class K>
void asof_launch_strategy(const AsofParams& p, int32_t strategy, hipStream_t s) {
    if (strategy == PLGPU_ASOF_BACKWARD) asof_launch<K, PLGPU_ASOF_BACKWARD>(p, s);
    else if (strategy == PLGPU_ASOF_FORWARD) asof_launch<K, PLGPU_ASOF_FORWARD>(p, s);
    else asof_launch<K, PLGPU_ASOF_NEAREST>(p, s);
}

int index_arg_check(const plgpu_column* c, int64_t length, const char* what) {
    if (c->dtype != PLGPU_U32) return fail(PLGPU_ERR_INVALID, std::string("join_asof: ") + what + " must be a UInt32 column");
    if (c->validity != nullptr) return fail(PLGPU_ERR_INVALID, std::string("join_asof: ") + what + " must not be nullable");
    if (c->length != length) return fail(PLGPU_ERR_INVALID, std::string("join_asof: ") + what + " has the wrong length");
    return PLGPU_OK;
}

}  // namespace
}  // namespace plgpu

using namespace plgpu;

PLGPU_API int plgpu_is_sorted_asc(const plgpu_column* col, int32_t* out_ascending, int32_t* out_nulls_first,
                                  void* stream) {
    hipStream_t s = as_stream(stream);
    if (col == nullptr || out_ascending == nullptr || out_nulls_first == nullptr)
        return fail(PLGPU_ERR_INVALID, "NULL argument");
    if (!asof_dtype(col->dtype))
        return fail(PLGPU_ERR_SCHEMA, "is_sorted_asc takes Int32 / Int64 / UInt32 / UInt64 / Float32 / Float64");
    *out_ascending = 1;
    *out_nulls_first = 1;
    if (col->length < 2) return PLGPU_OK;
    DevBuf<unsigned long long> res;
    int rc = res.alloc(16, s);
    if (rc) return rc;
    rc = sorted_scan(col, res, s);
    if (rc) return rc;
    unsigned long long h[2] = {0ull, 0ull};
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h, res.get(), 16, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "is_sorted_asc");
    *out_ascending = (h[0] & kSortedDesc) ? 0 : 1;
    *out_nulls_first = (h[0] & kSortedNullAfter) ? 0 : 1;
    return PLGPU_OK;
}

PLGPU_API int plgpu_join_asof(const plgpu_column* left_on, const plgpu_column* right_on, const plgpu_column* lo,
                              const plgpu_column* hi, const plgpu_column* right_rows, int32_t strategy,
                              int32_t allow_eq, int32_t has_tolerance, int64_t tolerance_bits, double tolerance_f64,
                              plgpu_column* out_idx, int32_t* out_path, void* stream) {
    hipStream_t s = as_stream(stream);
    if (left_on == nullptr || right_on == nullptr || out_idx == nullptr) return fail(PLGPU_ERR_INVALID, "NULL argument");
    std::memset(out_idx, 0, sizeof *out_idx);
    if (out_path != nullptr) *out_path = 0;
    if (strategy != PLGPU_ASOF_BACKWARD && strategy != PLGPU_ASOF_FORWARD && strategy != PLGPU_ASOF_NEAREST)
        return fail(PLGPU_ERR_INVALID, "join_asof: unknown strategy");
    if ((lo == nullptr) != (hi == nullptr)) return fail(PLGPU_ERR_INVALID, "join_asof: lo and hi come together");
    const int64_t n = left_on->length, nr = right_on->length;
    int rc;
    if (lo != nullptr) {
        if ((rc = index_arg_check(lo, n, "lo")) != PLGPU_OK) return rc;
        if ((rc = index_arg_check(hi, n, "hi")) != PLGPU_OK) return rc;
        if (right_on->validity != nullptr)
            return fail(PLGPU_ERR_INVALID, "join_asof: ranges search a right column without a validity buffer");
    }
    if (right_rows != nullptr && (rc = index_arg_check(right_rows, nr, "right_rows")) != PLGPU_OK) return rc;
    if (nr < 0 || n < 0 || nr >= 0xFFFFFFFFll)
        return fail(PLGPU_ERR_INVALID, "join_asof: the right side must have fewer than 2^32 - 1 rows");
    const int32_t dt = left_on->dtype;
    if (dt != right_on->dtype) return fail(PLGPU_ERR_SCHEMA, "mismatching key dtypes in asof-join");
    if (!asof_dtype(dt))
        return fail(PLGPU_ERR_SCHEMA, "join_asof keys must be Int32 / Int64 / UInt32 / UInt64 / Float32 / Float64");
    const int path = lo != nullptr ? 3 : (options().asof_path == 2 ? 2 : 1);
    if (out_path != nullptr) *out_path = path;
    rc = make_owned_column(out_idx, PLGPU_U32, n, true, s);
    if (rc || n == 0) return rc;
    const int esz = dtype_bytes(dt);
    AsofParams p;
    std::memset(&p, 0, sizeof p);
    p.left = (const char*)left_on->values + left_on->offset * esz;
    p.lvalid = left_on->validity;
    p.lvoff = left_on->offset;
    p.n_left = n;
    p.right = (const char*)right_on->values + right_on->offset * esz;
    p.n_right = (uint32_t)nr;
    if (lo != nullptr) {
        p.lo = (const uint32_t*)lo->values + lo->offset;
        p.hi = (const uint32_t*)hi->values + hi->offset;
    }
    if (right_rows != nullptr) p.rrows = (const uint32_t*)right_rows->values + right_rows->offset;
    p.allow_eq = allow_eq != 0;
    p.has_tol = has_tolerance != 0;
    if (dt == PLGPU_U64) p.tol_u = (uint64_t)tolerance_bits;
    else p.tol_u = tolerance_bits < 0 ? 0ull - (uint64_t)tolerance_bits : (uint64_t)tolerance_bits;
    p.tol_f = tolerance_f64 < 0.0 ? -tolerance_f64 : tolerance_f64;
    p.whole = path == 2;
    p.out = (uint32_t*)out_idx->values;
    p.out_valid = (uint64_t*)out_idx->validity;
    DevBuf<unsigned long long> rscan;
    if (right_on->validity != nullptr && nr > 0) {
        // where the right column's non-null run begins (its nulls are assumed first)
        rc = rscan.alloc(16, s);
        if (!rc) rc = sorted_scan(right_on, rscan, s);
        p.rscan = (const uint64_t*)rscan.get();
    }
    if (!rc) {
        switch (dt) {
        case PLGPU_I64: asof_launch_strategy<int64_t>(p, strategy, s); break;
        case PLGPU_I32: asof_launch_strategy<int32_t>(p, strategy, s); break;
        case PLGPU_U32: asof_launch_strategy<uint32_t>(p, strategy, s); break;
        case PLGPU_U64: asof_launch_strategy<uint64_t>(p, strategy, s); break;
        case PLGPU_F64: asof_launch_strategy<double>(p, strategy, s); break;
        default: asof_launch_strategy<float>(p, strategy, s); break;
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "join_asof");
    }
    if (rc) plgpu_column_release(out_idx);
    else out_idx->null_count = -1;
    return rc;
}
