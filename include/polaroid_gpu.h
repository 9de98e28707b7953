/*
 * polaroid_gpu.h — C-ABI of the MI355X columnar executor backend.
 *
 * This is the drop-in boundary a Polars host (Rust, via `extern "C"` +
 * bindgen, or Python via ctypes) binds to run the filter / arithmetic /
 * comparison / hash-group-by-aggregation hot path on gfx950.  Only plain C
 * types cross it: device pointers, lengths, Arrow bit-packed validity
 * bitmaps (LSB-first, Arrow offset semantics), status codes.  No torch or
 * HIP types appear in any signature; `stream` is an opaque hipStream_t
 * (NULL = the library's default stream).
 *
 * Each entry point names the reference interface it replaces
 * (paths relative to /root/reference/crates).
 *
 * Column ownership follows the Arrow C data interface: a column produced by
 * the library carries a non-NULL `release` callback that the consumer must
 * call exactly once; borrowed input columns have `release == NULL`.
 */
#ifndef POLAROID_GPU_H
#define POLAROID_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLGPU_ABI_VERSION 1

/* ---------------------------------------------------------------- status */
/* Error classes mirror polars_error::PolarsError variants
 * (polars-error/src/lib.rs) so the host can map them 1:1. */
enum plgpu_status {
    PLGPU_OK = 0,
    PLGPU_ERR_INVALID = -1,        /* InvalidOperation                      */
    PLGPU_ERR_SCHEMA = -2,         /* SchemaMismatch / ComputeError (dtype)  */
    PLGPU_ERR_SHAPE = -3,          /* ShapeMismatch (column lengths differ)  */
    PLGPU_ERR_OOM = -4,            /* device allocation failed               */
    PLGPU_ERR_HIP = -5,            /* HIP runtime error                      */
    PLGPU_ERR_NO_DEVICE = -6,      /* no gfx950 device visible               */
    PLGPU_ERR_CAPACITY = -7        /* internal table overflow (retry failed) */
};

/* ---------------------------------------------------------------- dtypes */
/* Physical types of the path; Arrow format string in the comment. */
enum plgpu_dtype {
    PLGPU_BOOL = 1, /* "b"  bit-packed values, LSB first               */
    PLGPU_I32 = 2,  /* "i"                                             */
    PLGPU_I64 = 3,  /* "l"                                             */
    PLGPU_F64 = 4,  /* "g"                                             */
    PLGPU_U32 = 5,  /* "I"  polars IdxSize (count / len outputs)       */
    PLGPU_STR = 6,  /* "U"  large_string: int64 offsets in `values`,
                       UTF-8 bytes in `data` (polars String / Binary)   */
    PLGPU_I8 = 7,   /* "c"                                             */
    PLGPU_I16 = 8,  /* "s"                                             */
    PLGPU_U8 = 9,   /* "C"                                             */
    PLGPU_U16 = 10, /* "S"                                             */
    PLGPU_U64 = 11, /* "L"                                             */
    PLGPU_F32 = 12  /* "f"                                             */
    /* polars' temporal types travel as their physical integers: Datetime /
     * Duration as PLGPU_I64, Date as PLGPU_I32 (the host keeps the unit). */
};

/* One Arrow array in device memory (Arrow C Device Data Interface,
 * ARROW_DEVICE_ROCM = 10, flattened to the two buffers the path uses). */
typedef struct plgpu_column {
    int32_t dtype;            /* enum plgpu_dtype                                  */
    int32_t device_id;        /* HIP device ordinal                                */
    int64_t length;           /* logical length                                    */
    int64_t offset;           /* Arrow offset (elements; bits for PLGPU_BOOL)      */
    int64_t null_count;       /* -1 = unknown                                      */
    const void* values;       /* device ptr, Arrow buffers[1]                      */
    const uint8_t* validity;  /* device ptr, Arrow buffers[0]; NULL = all valid    */
    void (*release)(struct plgpu_column*); /* NULL for borrowed columns             */
    void* private_data;
    const uint8_t* data;      /* device ptr, Arrow buffers[2] of PLGPU_STR (bytes); */
                              /* NULL for fixed-width columns                       */
} plgpu_column;

/* ------------------------------------------------------- expression ISA */
/* A physical expression (polars-expr/src/expressions/{binary,column,
 * literal}.rs) is lowered to a postfix program evaluated per row on the
 * GPU.  Semantics per op follow the reference kernels cited below. */
enum plgpu_opcode {
    PLGPU_OP_COL = 1,       /* push column[arg]                                 */
    PLGPU_OP_LIT_F64 = 2,   /* push f64 literal imm.f64                         */
    PLGPU_OP_LIT_I64 = 3,   /* push i64 literal imm.i64                         */
    PLGPU_OP_LIT_BOOL = 4,  /* push bool literal imm.i64 != 0                   */
    PLGPU_OP_LIT_NULL = 5,  /* push typed null (arg = plgpu_dtype)              */
    /* arithmetic: polars-compute/src/arithmetic/{signed,unsigned,float}.rs.
     * Operands are coerced to their supertype first
     * (polars-core/src/utils/supertype.rs, dynamic literals included: an
     * integer literal takes the smallest type that holds it, a float
     * literal takes the float column's type or Float64), and integer
     * results wrap at the supertype's width.  LIT_I64 / LIT_F64 are the
     * dynamic (untyped) literals; CAST gives a literal a concrete type. */
    PLGPU_OP_ADD = 10,
    PLGPU_OP_SUB = 11,
    PLGPU_OP_MUL = 12,
    PLGPU_OP_TRUEDIV = 13,  /* ints -> Float64; float / literal = x * (1 / lit)
                               (true_div_scalar, arithmetic/float.rs:113)    */
    PLGPU_OP_NEG = 14,
    PLGPU_OP_ABS = 15,
    PLGPU_OP_CAST_F64 = 16,
    PLGPU_OP_FLOORDIV = 17, /* ints: floor division, x // 0 = null
                               (floor_divmod.rs:39); floats: floor(a / b)    */
    PLGPU_OP_MOD = 18,      /* ints: remainder with the divisor's sign, x % 0
                               = null; floats: a - b * floor(a / b)          */
    PLGPU_OP_DIVIDE = 19,   /* Operator::Divide (legacy_div, arithmetic/mod.rs:40):
                               floor division for ints, true division for floats */
    PLGPU_OP_CAST = 50,     /* cast to dtype `arg`; imm.i64: 0 = non-strict
                               (a value that does not fit -> null), 1 =
                               overflowing (integers wrap)                   */
    PLGPU_OP_XOR = 51,      /* Boolean xor (null if either is null); bitwise on ints */
    PLGPU_OP_FILL_NULL = 52,/* [x, fill] -> x where valid, else fill         */
    PLGPU_OP_IF_ELSE = 53,  /* [cond, then, otherwise] -> when(cond).then().otherwise();
                               a null condition selects `otherwise`
                               (polars-compute/src/if_then_else)             */
    /* comparisons: TotalOrd semantics, polars-utils/src/total_ord.rs:317-368
     * (NaN == NaN, NaN greatest); null in -> null out. */
    PLGPU_OP_EQ = 20,
    PLGPU_OP_NE = 21,
    PLGPU_OP_LT = 22,
    PLGPU_OP_LE = 23,
    PLGPU_OP_GT = 24,
    PLGPU_OP_GE = 25,
    PLGPU_OP_EQ_MISSING = 26, /* null == null, never null out */
    PLGPU_OP_NE_MISSING = 27,
    /* boolean: Kleene logic, polars-compute/src/bitwise + ops::and/or;
     * AND / OR / XOR of integers are bitwise */
    PLGPU_OP_AND = 30,
    PLGPU_OP_OR = 31,
    PLGPU_OP_NOT = 32,
    PLGPU_OP_IS_NULL = 33,
    PLGPU_OP_IS_NOT_NULL = 34,
    PLGPU_OP_IS_NAN = 35,
    PLGPU_OP_IS_FINITE = 36,
    /* String literal pattern tests (plgpu_str_compare only):
     * polars-ops/src/chunked_array/binary/namespace.rs:85 starts_with, :78
     * ends_with, strings/namespace.rs:332 contains_literal */
    PLGPU_OP_STR_STARTS_WITH = 40,
    PLGPU_OP_STR_ENDS_WITH = 41,
    PLGPU_OP_STR_CONTAINS = 42
};

typedef struct plgpu_instr {
    int32_t op;   /* enum plgpu_opcode */
    int32_t arg;  /* column index / dtype */
    union {
        double f64;
        int64_t i64;
    } imm;
} plgpu_instr;

#define PLGPU_MAX_STACK 8
#define PLGPU_MAX_PROGRAM 64
#define PLGPU_MAX_COLS 8

/* -------------------------------------------------------- aggregations */
/* polars-core/src/frame/group_by/aggregations/mod.rs (agg_sum :581,
 * agg_mean :659, agg_min/agg_max) and the streaming reductions the lazy
 * engine actually runs for a partitionable group-by
 * (polars-mem-engine/src/planner/lp.rs:648 -> polars-expr/src/reduce/
 * {sum,mean,min_max,count,len}.rs). */
enum plgpu_agg_kind {
    PLGPU_AGG_SUM = 1,   /* f64: correctly-rounded exact sum; i64: wrapping  */
    PLGPU_AGG_MEAN = 2,  /* f64 out, null if no non-null values              */
    PLGPU_AGG_MIN = 3,   /* NaN ignored unless all NaN (min_ignore_nan)      */
    PLGPU_AGG_MAX = 4,
    PLGPU_AGG_COUNT = 5, /* non-null count, u32 (IdxSize)                    */
    PLGPU_AGG_LEN = 6,   /* group length incl. nulls, u32                    */
    PLGPU_AGG_FIRST = 7, /* value of the group's first row, null included    */
    PLGPU_AGG_LAST = 8,  /* ... last row (reduce/first_last.rs First / Last) */
    PLGPU_AGG_VAR = 9,   /* variance of a Float64 column, f64 out; ddof in bits */
                         /* 8..15 of the kind (plgpu_group_by_agg_ex only)      */
    PLGPU_AGG_STD = 10   /* its square root                                    */
};

typedef struct plgpu_agg {
    int32_t kind; /* enum plgpu_agg_kind */
    int32_t col;  /* input column index */
} plgpu_agg;

/* An aggregation input computed from the columns: the elementwise
 * expression under an aggregation (`(close * volume).sum()`), which the
 * reference's partitionable group-by pre-aggregates directly
 * (polars-plan/src/plans/aexpr/properties/general.rs:335 can_pre_agg).
 * `program` is an expression program over the call's columns. */
typedef struct plgpu_agg_input {
    const plgpu_instr* program;
    int32_t n_instr;
    int32_t _pad;
} plgpu_agg_input;

/* Diagnostics of one group-by call (for tests / bench / rocprof cross-check). */
typedef struct plgpu_groupby_info {
    int64_t rows_in;
    int64_t rows_selected;       /* rows passing the fused predicate            */
    int64_t groups;
    int64_t global_path_rows;    /* rows that missed the LDS table             */
    int32_t reruns;              /* fixed-point window / table-size retries    */
    int32_t lds_slots;           /* per-workgroup LDS hash-table capacity      */
    int32_t grid;                /* workgroups in the main launch              */
    int32_t sum_inexact;         /* bit i: f64 sum acc i rounded below window  */
    int64_t table_capacity;      /* global hash-table slots                    */
    double main_kernel_ms;       /* device time of the aggregation kernel(s)   */
    int32_t path;                /* 0 generic, 1 fast, 2 fast sum-only, 3 partitioned,
                                    4 fast variance triple (one var / std column)   */
    int32_t sum_limbs;           /* 40-bit LDS limbs per f64 sum (2 or 3)      */
    int32_t local_range;         /* 1: range-local fused kernel (clustered keys) */
    int32_t register_runs;       /* 1: fused kernel with per-lane register runs (sorted keys) */
    int32_t key_pack;            /* key columns packed in the fused kernel's registers (0: a key / code column) */
    int32_t part_layout;         /* partitioned path: partition bits | scatter passes << 8 (0: not partitioned) */
    int32_t fused_variant;       /* the gb_fast_kernel instantiation the fused path launched (0: it did not
                                    run, i.e. path 0 or 3): bits 0-2 VAR, 3-4 PACK, 5 NULLS, 6 RUNS, 7 DERIV,
                                    8-9 LIMBS, 10-12 NACC, 13 PRED, 14 SUMONLY, 15 always 1, 16-19 ROWS,
                                    20 a NULLS instantiation read its validity as whole words per wave
                                    (every bitmap 8-byte aligned at a column offset that is a multiple of 64) */
    int32_t _reserved;           /* 0 (keeps the size a multiple of 8 without implicit padding) */
} plgpu_groupby_info;

/* ---------------------------------------------------------------- basics */
int plgpu_abi_version(void);
const char* plgpu_last_error(void);           /* thread-local message        */
int plgpu_device_count(int* out);
int plgpu_set_device(int device);
int plgpu_synchronize(void* stream);

/* Stream-ordered device allocator (native caching pool). */
int plgpu_alloc(void** out_ptr, size_t bytes, void* stream);
int plgpu_free(void* ptr, void* stream);
int plgpu_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int plgpu_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
/* n device -> host copies (dst[i] <- src[i], bytes[i]) with one
 * synchronisation: small ranges go through a library-owned pinned buffer.
 * Returns when every dst holds its bytes (a query's result columns). */
int plgpu_memcpy_d2h_many(int32_t n, void* const* dst, const void* const* src, const size_t* bytes, void* stream);
int plgpu_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream);

/* Test hooks and diagnostics, each read once from the environment variable
 * PLGPU_<NAME> (upper case) when the library loads and settable here:
 *   "ktime"       1: time the named kernels with HIP events (plgpu_ktime_read)
 *   "fuse_keys"   0: multi-key / Categorical group-bys write their packed
 *                 code column instead of forming the codes in the fused kernel
 *   "plan_cache"  0: every group-by samples its inputs (no reuse of the plan
 *                 statistics of a recent group-by over the same columns)
 *   "grid_rounds" > 0: the fused group-by grid in that many rounds of resident
 *                 workgroups (A/B; 0: scaled with the input)
 *   "debug"       per-attempt group-by diagnostics on stderr
 *   "no_pack"     multi-key operators hash their key tuples even when the
 *                 tuples would pack into one Int64 (exercises the hashed path)
 *   "mk_collide"  a 3-bit first tuple hash (forces the collision / re-seed path)
 *   "runs"        -1: the plan decides; 0 / 1 force the sorted-key variant of
 *                 the fused group-by kernel
 *   "local"       -1: the plan decides; 0 keeps the group-by off the
 *                 range-local fused kernel (clustered keys)
 *   "gb_path"     -1: the plan decides; forces the single-key group-by's
 *                 path where its inputs allow it: 0 generic kernel on the
 *                 global table, 1 generic kernel with LDS tables, 2 fused
 *                 kernel, 3 partitioned (results never depend on it)
 *   "part_bits"   partitioned group-by: at least this many partition bits
 *   "part_levels" partitioned group-by: 1 / 2 scatter passes (-1: by the
 *                 partition bits, two above 8)
 * A / B switches of measured kernel variants (results never depend on them):
 *   "part_direct"  1: one-workgroup partitions flush into their own region
 *   "part_lds_kb"  partitioned aggregation's LDS table budget (0: 160 KiB)
 *   "part_threads" partitioned aggregation's threads per workgroup (0: by
 *                  the rows per workgroup)
 *   "rl_stream"    1: rolling windows <= 64 by resident streaming waves
 *   "rl_grid"      the streaming rolling kernel's workgroups per CU
 *   "rl_div"       1: full windows' means by the one-correction quotient
 *   "rl_full"      1: interior null-free rolling waves by the specialised
 *                  scans (sum / mean / var / std)
 *   "filt_pipe"    1: the filter scatter issues the next column's loads
 *                  before this column's stores
 *   "gb_pair"      1: (x * y).sum() next to y.sum() by the fused kernel's
 *                  product-pair variant
 *   "var_pos"      1: the fused variance's x limbs unsigned when the fused
 *                  predicate keeps only x >= 0
 *   "sum_pos"      1: the fused 4-sum kernel's limbs of the predicate's own
 *                  column unsigned when the predicate keeps only x >= 0
 *   "filt_fused"   1: a simple-predicate filter of null-free 8-byte columns
 *                  in one pass (decoupled look-back; off: measured slower)
 *   "part_compact" 1: sum-only one-workgroup partitions write their groups
 *                  densely into a region table, misses go to a small hashed
 *                  overflow table, the finalize reads only the dense runs
 *   "part_null_sentinel" 1: sum-only partitioned runs write a null Int64 key
 *                  as a value outside the non-null keys' range (no null-bits
 *                  column in the partition buffers)
 *   "rl_var128"    1: rolling var / std interior waves form their numerators
 *                  modulo 2^128 where the wave's exponent span bounds them
 *   "rl_var_hot"   1: rolling var / std run their common blocks (interior,
 *                  finite, 128-bit numerators) in a kernel of their own and
 *                  the other blocks from a device-side list afterwards
 *   "rl_mean_hot"  1: the same split for rolling sum / mean (interior,
 *                  finite blocks in the 64-bit form)
 *   "wave_report"  1: the slim fused kernels publish their diagnostics per
 *                  wave instead of once per workgroup
 *   "alloc_skew"   1: device blocks of 256 MiB and more start at rotating
 *                  64 KiB offsets (placement probe; off)
 *   "alloc_contig" 1: device blocks of 256 MiB and more physically
 *                  contiguous where the driver grants it (placement probe; off)
 *   "srt_w4"       1: the sort's packed downsweeps compiled for 4 waves per
 *                  SIMD (off: measured slower)
 *   "srt_up_tiles" tiles per sort upsweep workgroup (1; more measured slower)
 *   "part_rows4"   1: 512-thread partition workgroups take 4 rows per thread
 *   "over_presorted" 1: a caller that plgpu_segment_starts tells the keys
 *                  arrive sorted runs its window expression over groups with
 *                  no sort and no gather; 0: it sorts all the same (same
 *                  results).  Read by the caller choosing the path (the host
 *                  mirror's over()); the entry points do not depend on it
 *   "asof_path"    plgpu_join_asof without ranges: 0 the library decides
 *                  (today: as 1), 1 every tile of left rows searches the
 *                  window of the right column its keys can touch, staged in
 *                  LDS where it fits, 2 every row searches the whole right
 *                  column (tests / A-B; results never depend on it)
 *   "gb_claim"     fused group-by without an explicit "grid_rounds": 1 (the
 *                  default) the resident workgroups' waves claim their rows
 *                  chunk by chunk, 0 the static grid of several rounds (A/B)
 *   "claim_cap_rows" rows per workgroup at which its waves stop claiming, a
 *                  multiple of 1024 (0: the kernel's limit of 2^22; tests
 *                  reach the cap with a small input)
 * An unknown name is PLGPU_ERR_INVALID. */
int plgpu_set_option(const char* name, int64_t value);
int plgpu_get_option(const char* name, int64_t* out);
/* Kernel timer (option "ktime" = 1): HIP-event times of the library's named
 * kernels since the last reset, one "name\tms_total\tlaunches\n" line per
 * kernel into buf (NUL-terminated); waits for pending launches.  reset != 0
 * clears the sums.  A launch that an A/B option selects or shapes carries a
 * name of its own (rl_stream_kernel, srt_downsweep_w4_kernel,
 * gb_part_agg_rows4_kernel, ...), so a test can tell that it ran; the default
 * configuration's names do not change.  Measurement support (no reference counterpart; the
 * reference's equivalent is its profiling via `should_time`,
 * crates/polars-mem-engine/src/executors/scan/python_scan.rs:91). */
int plgpu_ktime_read(char* buf, int64_t cap, int32_t reset);
/* Return the allocator's cached free blocks on the current device to the HIP
 * runtime (waits for the device first), e.g. before another allocator in the
 * process needs the memory.  Live columns are untouched. */
int plgpu_release_cached(void);

/* Checked build only (make CHECKS=1, libpolaroid_gpu_checked.so): the bits of
 * the group-by kernels' index invariants violated since the last call (the
 * violating accesses were skipped), then cleared.  Always 0 in the product
 * build. */
int plgpu_debug_checks(uint32_t* out);

/* Release a library-produced column (no-op for borrowed ones). */
void plgpu_column_release(plgpu_column* col);

/* ---- ingestion: Arrow RecordBatches in host memory -> device columns -------
 * The reference hands a DataFrame to an engine as one Arrow RecordBatch per
 * chunk: crates/polars-python/src/dataframe/export.rs:80 PyDataFrame.to_arrow
 * (what a GPU-engine scan calls on DataFrameScan.df, visitor/nodes.rs:190).
 * plgpu_column_alloc makes an owning column for the concatenated chunks
 * (PLGPU_STR: `str_bytes` bytes of string data).  plgpu_ingest_chunk copies
 * rows [src_offset, src_offset + length) of one chunk's Arrow buffers, as they
 * lie in host memory, into rows [dst_row, dst_row + length) of `dst`:
 *   values    Arrow buffers[1] (fixed width; bit-packed for PLGPU_BOOL;
 *             int64 offsets for PLGPU_STR, rebased so the chunk's first byte
 *             lands at `dst_byte` of dst->data)
 *   validity  Arrow buffers[0] or NULL (all valid; required NULL when dst has
 *             no validity)
 *   str_data  Arrow buffers[2] of a PLGPU_STR chunk
 * Copies are the runtime's staged copies of the pageable buffers,
 * asynchronously on `stream`; bits at any offset are placed by a device
 * kernel.  The host buffers may be reused on return; the device data is
 * complete after plgpu_synchronize. */
int plgpu_column_alloc(int32_t dtype, int64_t length, int32_t with_validity, int64_t str_bytes,
                       plgpu_column* out, void* stream);
int plgpu_ingest_chunk(plgpu_column* dst, int64_t dst_row, int64_t dst_byte, const void* values,
                       const uint8_t* validity, const uint8_t* str_data, int64_t src_offset, int64_t length,
                       void* stream);

/* Result dtype of a program over columns of the given dtypes (only the
 * columns' dtype fields are read; nothing runs on the device): the static
 * typing of polars' type coercion (polars-plan/src/plans/conversion/
 * type_coercion, polars-core/src/utils/supertype.rs) as the executor applies
 * it. */
int plgpu_expr_dtype(const plgpu_column* cols, int32_t ncols, const plgpu_instr* program, int32_t n_instr,
                     int32_t* out_dtype);

/* ------------------------------------------------------------ hot path */

/* Evaluate a physical expression over `ncols` input columns of equal length
 * into a new column (BOOL / I64 / F64).  Replaces PhysicalExpr::evaluate for
 * column/literal/binary expressions (polars-expr/src/expressions/binary.rs)
 * and the broadcast comparison kernels TotalOrdKernel::tot_*_kernel_broadcast
 * (polars-compute/src/comparisons/{scalar,simd}.rs). */
int plgpu_eval(const plgpu_column* cols, int32_t ncols, const plgpu_instr* program,
               int32_t n_instr, plgpu_column* out, void* stream);

/* Filter `ncols` columns by a BOOL mask (null = false) into new columns.
 * Replaces polars-compute/src/filter/mod.rs:18 `filter` (and
 * DataFrame::filter, polars-core/src/frame/mod.rs:2012, which FilterExec
 * calls in polars-mem-engine/src/executors/filter.rs:51). */
int plgpu_filter(const plgpu_column* cols, int32_t ncols, const plgpu_column* mask,
                 plgpu_column* out_cols, int64_t* out_len, void* stream);

/* Fused FilterExec + predicate: evaluate `program` (must yield BOOL) and
 * compact the columns in one pipeline (no materialised mask column). */
int plgpu_filter_expr(const plgpu_column* cols, int32_t ncols, const plgpu_instr* program,
                      int32_t n_instr, plgpu_column* out_cols, int64_t* out_len,
                      void* stream);

/* Hash group-by on one integer key column with aggregations, optionally
 * fused with a filter predicate (`program` may be NULL / n_instr 0).
 * Replaces GroupByExec / GroupByStreamingExec
 * (polars-mem-engine/src/executors/group_by.rs:117,
 * group_by_streaming.rs) for keys = [col(k)], aggs over plain columns.
 * Output: `out_key` (I64, null group allowed) and `out_aggs[naggs]`.
 * maintain_order != 0 orders groups by first occurrence (the reference's
 * `maintain_order=True`); otherwise group order is unspecified, as in the
 * reference. */
int plgpu_group_by_agg(const plgpu_column* key, const plgpu_column* cols, int32_t ncols,
                       const plgpu_instr* program, int32_t n_instr, const plgpu_agg* aggs,
                       int32_t naggs, int32_t maintain_order, plgpu_column* out_key,
                       plgpu_column* out_aggs, plgpu_groupby_info* info, void* stream);

/* Group-by on 1..8 key columns (I64 / I32 / U32 / F64 / BOOL, nullable).
 * Replaces the multi-key branch of DataFrame::group_by_with_series
 * (polars-core/src/frame/group_by/mod.rs:91): the reference row-encodes the
 * keys (chunked_array/ops/row_encode.rs:11) and groups the encoded rows, so
 * groups are distinct key tuples, a null equal only to a null and f64 keys
 * compared by TotalOrd.  Here the tuples are hashed to 64 bits, grouped by
 * the single-key kernels, and every row is verified against its group's first
 * row (a hash collision re-runs with another seed; PLGPU_ERR_CAPACITY after 4
 * seeds).  `out_keys[nkeys]` take the key columns' dtypes and hold each
 * group's first-row tuple; `maintain_order`, aggregations and the fused
 * predicate are as for plgpu_group_by_agg. */
int plgpu_group_by_agg_multi(const plgpu_column* keys, int32_t nkeys, const plgpu_column* cols,
                             int32_t ncols, const plgpu_instr* program, int32_t n_instr,
                             const plgpu_agg* aggs, int32_t naggs, int32_t maintain_order,
                             plgpu_column* out_keys, plgpu_column* out_aggs,
                             plgpu_groupby_info* info, void* stream);

/* The general form of both: 0..8 key columns, and aggregations over the
 * columns or over computed inputs.  An agg.col >= ncols names
 * inputs[agg.col - ncols], an elementwise expression over the columns (see
 * plgpu_agg_input): `x op y` of two Float64 columns or a column and a
 * literal (+ - * /) is computed in registers by the fused kernel; any other
 * expression is evaluated once into a column first.
 * nkeys == 0 is a global reduction, `lf.filter(p).select(aggs)`
 * (polars-expr/src/reduce/sum.rs:112 reduce_ca and its siblings): every
 * selected row in one group, and one output row even when no row is
 * selected (sum / len / count 0, the other aggregations null, as the
 * reference's empty reductions); `out_keys` is not written.  `ncols` must be
 * >= 1 then, to give the length. */
int plgpu_group_by_agg_ex(const plgpu_column* keys, int32_t nkeys, const plgpu_column* cols, int32_t ncols,
                          const plgpu_agg_input* inputs, int32_t ninputs, const plgpu_instr* program,
                          int32_t n_instr, const plgpu_agg* aggs, int32_t naggs, int32_t maintain_order,
                          plgpu_column* out_keys, plgpu_column* out_aggs, plgpu_groupby_info* info,
                          void* stream);


/* ---- hash-partitioned group-by (one process per GPU) ----------------------
 * Mirrors the partitioned sink of the streaming group-by
 * (polars-stream/src/nodes/group_by.rs:216 `combine_locals`): each local
 * builder pre-aggregates, splits its pre-aggregates by a hash partitioner
 * (group_by.rs:85 `add_pre_agg`, :509 HashPartitioner) and each partition
 * folds the pre-aggregates routed to it (group_by.rs:378 `combine_subset`).
 * Here a "local" is one GPU's shard, partitions are ranks, and the
 * pre-aggregates are exact partial states (records) moved by one RCCL
 * all-to-all.  A record is `record_words` u64 words:
 * [kind (0 key, 1 null key, 2 INT64_MIN key), key, state fields...].
 * Each rank aggregates with its own f64 fixed-point windows (`bottoms`,
 * PLGPU_GB_MAX_ACC int32, refitted locally as needed); the windows travel
 * with the record counts, and plgpu_gb_merge_sources shifts every source's
 * exact sum states onto the lowest window before folding them
 * (polaroid_amd/distributed.py).  No collective precedes the exchange. */
typedef struct plgpu_gb_partial plgpu_gb_partial;

#define PLGPU_GB_MAX_ACC 6

/* Words per exported record for this aggregation schema (lengths ignored). */
int plgpu_gb_record_words(const plgpu_column* cols, int32_t ncols, const plgpu_agg* aggs,
                          int32_t naggs, int32_t* out_words);

/* Sampled fixed-point windows of this shard (out_bottoms[PLGPU_GB_MAX_ACC]). */
int plgpu_gb_plan_bottoms(const plgpu_column* key, const plgpu_column* cols, int32_t ncols,
                          const plgpu_agg* aggs, int32_t naggs, int32_t* out_bottoms,
                          void* stream);

/* Filter + pre-aggregate this shard.  `bottoms` NULL: this shard's own
 * windows (sampled, refitted here when a value does not fit); otherwise the
 * fixed windows to use, and whether one must move for an exact sum is
 * reported (*out_refit, new windows in out_bottoms_hint[6]; without a refit
 * the hint equals the used windows).  The windows used come back in
 * out_bottoms_used[6].  Returns a handle holding the partial table and the
 * number of groups (*out_records).  A column whose values need the wide
 * (multi-window) sum keeps exact per-group digit states instead: the ranks
 * agree one digit range per column (plgpu_gb_partial_wide, a max all-reduce,
 * plgpu_gb_partial_set_wide) before the export. */
int plgpu_gb_partial_begin(const plgpu_column* key, const plgpu_column* cols, int32_t ncols,
                           const plgpu_instr* program, int32_t n_instr, const plgpu_agg* aggs,
                           int32_t naggs, const int32_t* bottoms, int32_t world,
                           plgpu_gb_partial** out, int64_t* out_records, int32_t* out_bottoms_used,
                           int32_t* out_refit, int32_t* out_bottoms_hint,
                           plgpu_groupby_info* info, void* stream);

/* Wide f64 sums across ranks (round 5; polars-stream/src/nodes/group_by.rs:85
 * add_pre_agg ships fixed-size pre-aggregates whatever the values): per acc
 * a, out_wide[a] = 1 when this shard's values of that f64 sum span more
 * binades than one fixed-point window, and [out_exmin[a], out_exmax[a]] the
 * biased exponents its values take (the window's range for a non-wide f64
 * sum; 0x7FF / 0 for other accs).  The ranks reduce (max of wide, min of
 * exmin, max of exmax); when any wide[a] is set, every rank calls
 * plgpu_gb_partial_set_wide with the reduced arrays: those columns' states
 * become per-group digit words (24-bit digits in int64 words, the single-GPU
 * wide sum's form) over the agreed range, appended to every record, and
 * plgpu_gb_merge_sources_wide adds them and rounds each group once.  The
 * result is bit-identical to the single-GPU group-by.  Record words then
 * come from plgpu_gb_partial_record_words. */
int plgpu_gb_partial_wide(const plgpu_gb_partial* h, int32_t* out_wide, int32_t* out_exmin,
                          int32_t* out_exmax);
int plgpu_gb_partial_set_wide(plgpu_gb_partial* h, const int32_t* wide, const int32_t* exmin,
                              const int32_t* exmax);
int plgpu_gb_partial_record_words(const plgpu_gb_partial* h, int32_t* out_words);

/* Write the partial groups as records into device buffer `dst_records`
 * (out_records * record_words u64), grouped by destination rank in rank
 * order; out_counts[world] receives the records per destination. */
int plgpu_gb_partial_export(plgpu_gb_partial* h, void* dst_records, int64_t* out_counts,
                            void* stream);

void plgpu_gb_partial_free(plgpu_gb_partial* h);

/* Rows of a key column routed to the rank that owns their key's partial
 * states (the partition function plgpu_gb_partial_export routes records by;
 * the null key and the INT64_MIN key go to rank 0): *out_perm receives a
 * UInt32 row-index column grouped by rank in rank order, out_counts[world]
 * the rows per rank.  Used to move per-rank first() / last() results to the
 * owner of their groups (the partitioned sink's `combine_subset` for
 * reduce/first_last.rs, polars-stream/src/nodes/group_by.rs:378). */
int plgpu_gb_route(const plgpu_column* key, int32_t world, plgpu_column* out_perm,
                   int64_t* out_counts, void* stream);

/* Packed tuple keys agreed across ranks (the multi-key group-by's exact
 * Int64 packing, row_encode.rs:11 semantics: tuple equality, a null distinct
 * from every value).  plgpu_key_ranges writes per key column [min, max,
 * any null] (signed; no valid value: min = INT64_MAX > max = INT64_MIN) into
 * out_ranges[3 * nkeys]; the caller reduces them over the ranks (min / max /
 * max).  plgpu_key_pack packs every row's tuple with the plan those ranges
 * give into *out_codes (Int64, no nulls; *out_ok = 0 and no column when the
 * fields need more than 63 bits); plgpu_key_unpack turns codes back into
 * key columns of `dtypes`.  Keys: integer (not UInt64) or Boolean. */
int plgpu_key_ranges(const plgpu_column* keys, int32_t nkeys, int64_t* out_ranges, void* stream);
int plgpu_key_pack(const plgpu_column* keys, int32_t nkeys, const int64_t* ranges,
                   plgpu_column* out_codes, int32_t* out_ok, void* stream);
int plgpu_key_unpack(const plgpu_column* codes, const int32_t* dtypes, int32_t nkeys,
                     const int64_t* ranges, plgpu_column* out_keys, void* stream);

/* Float64 / Float32 keys across ranks: each key as the Int64 of its
 * canonical bits (-0.0 as 0.0, every NaN as one NaN; polars-utils/src/
 * total_ord.rs TotalEq groups exactly these together), validity carried, so
 * a float key crosses the integer-keyed partitioned group-by (the output
 * key is each group's first value, carried by a first() aggregation). */
int plgpu_float_key_encode(const plgpu_column* keys, plgpu_column* out_codes, void* stream);

/* Fold `n_records` received records (device memory) into this rank's
 * partition and finalize it like plgpu_group_by_agg (`cols` supplies the
 * dtypes only; `key_dtype` is the original key dtype). */
int plgpu_gb_merge(const void* records, int64_t n_records, const plgpu_column* cols,
                   int32_t ncols, const plgpu_agg* aggs, int32_t naggs, const int32_t* bottoms,
                   int32_t key_dtype, plgpu_column* out_key, plgpu_column* out_aggs,
                   plgpu_groupby_info* info, void* stream);

/* Fold the records received from `n_sources` ranks: source j's
 * src_records[j] records lie consecutively, in source order (the layout of
 * an all-to-all's receive buffer), aggregated with that source's windows
 * src_bottoms[j * PLGPU_GB_MAX_ACC + a].  Per column, the sums are shifted
 * onto the lowest window of any source that sent records (exact); a state
 * that would leave the 192-bit range fails with PLGPU_ERR_CAPACITY.  Then
 * finalized like plgpu_gb_merge.  Replaces the window agreement before the
 * partial stage (polars-stream/src/nodes/group_by.rs:378 combine_subset
 * folds pre-aggregates of any origin). */
int plgpu_gb_merge_sources(const void* records, int32_t n_sources, const int64_t* src_records,
                           const int32_t* src_bottoms, const plgpu_column* cols, int32_t ncols,
                           const plgpu_agg* aggs, int32_t naggs, int32_t key_dtype,
                           plgpu_column* out_key, plgpu_column* out_aggs, plgpu_groupby_info* info,
                           void* stream);

/* plgpu_gb_merge_sources for records carrying wide digit states (the
 * reduced wide / exmin / exmax of plgpu_gb_partial_set_wide). */
int plgpu_gb_merge_sources_wide(const void* records, int32_t n_sources, const int64_t* src_records,
                                const int32_t* src_bottoms, const int32_t* wide,
                                const int32_t* wide_exmin, const int32_t* wide_exmax,
                                const plgpu_column* cols, int32_t ncols, const plgpu_agg* aggs,
                                int32_t naggs, int32_t key_dtype, plgpu_column* out_key,
                                plgpu_column* out_aggs, plgpu_groupby_info* info, void* stream);

/* ---- hash join ------------------------------------------------------------
 * maintain_order (polars-ops/src/frame/join/args.rs:100 MaintainOrderJoin)
 * and validate (args.rs JoinValidation). */
enum plgpu_join_order {
    PLGPU_JOIN_ORDER_NONE = 0,        /* unspecified (build on the shorter side) */
    PLGPU_JOIN_ORDER_LEFT = 1,        /* left row order (then right row order)   */
    PLGPU_JOIN_ORDER_RIGHT = 2,       /* right row order (then left row order)   */
    PLGPU_JOIN_ORDER_LEFT_RIGHT = 3,
    PLGPU_JOIN_ORDER_RIGHT_LEFT = 4
};
enum plgpu_join_validate {
    PLGPU_JOIN_VALIDATE_M_M = 0,
    PLGPU_JOIN_VALIDATE_1_M = 1,      /* left keys unique  */
    PLGPU_JOIN_VALIDATE_M_1 = 2,      /* right keys unique */
    PLGPU_JOIN_VALIDATE_1_1 = 3
};

/* Join type (polars-ops/src/frame/join/args.rs JoinType; cross / as-of /
 * IE joins are not on the GPU path). */
enum plgpu_join_how {
    PLGPU_JOIN_INNER = 0,
    PLGPU_JOIN_LEFT = 1,
    PLGPU_JOIN_RIGHT = 2,
    PLGPU_JOIN_FULL = 3,
    PLGPU_JOIN_SEMI = 4,
    PLGPU_JOIN_ANTI = 5
};

/* Equi-join of any type on one integer key (I64 / I32 / U32).  Produces the
 * row pairs as two UInt32 index columns; a row without a partner has a null
 * partner index (left / right / full joins: the reference's
 * NullableIdxSize / ChunkJoinOptIds), and such an index column carries an
 * Arrow validity bitmap.  Semi / anti joins produce the kept left rows in
 * `out_left_idx` (in left-row order) and an empty `out_right_idx`.  Pair
 * order is the reference's for every maintain_order mode (left joins are
 * always in left order; full joins with maintain_order "none" leave the
 * order unspecified, as the reference's hash-table drain does).  Replaces
 *   inner  single_keys_inner.rs:45 hash_join_tuples_inner,
 *   left   single_keys_left.rs:106 hash_join_tuples_left (+ the ordering of
 *          dispatch_left_right.rs:143 maintain_order_idx),
 *   right  dispatch_left_right.rs:19 right_join_from_series,
 *   full   single_keys_outer.rs:181 hash_join_tuples_outer (+ the ordering of
 *          hash_join/mod.rs:164 _full_join_from_series),
 *   semi / anti  single_keys_semi_anti.rs:111 / :95
 * (paths under polars-ops/src/frame/join/). */
int plgpu_join(const plgpu_column* left_key, const plgpu_column* right_key, int32_t how, int32_t nulls_equal,
               int32_t maintain_order, int32_t validate, plgpu_column* out_left_idx, plgpu_column* out_right_idx,
               void* stream);

/* plgpu_join on 1..8 key columns per side (pairwise equal dtypes: I64 / I32
 * / U32 / F64 / BOOL; join/mod.rs:625 prepare_keys_multiple). */
int plgpu_join_multi(const plgpu_column* left_keys, const plgpu_column* right_keys, int32_t nkeys, int32_t how,
                     int32_t nulls_equal, int32_t maintain_order, int32_t validate, plgpu_column* out_left_idx,
                     plgpu_column* out_right_idx, void* stream);

/* Boolean column of a comparison of String column `a` with String column
 * `b`, or (b == NULL) with the literal `lit` (lit_len bytes, host memory):
 * op = PLGPU_OP_EQ .. PLGPU_OP_NE_MISSING; or IS_NULL / IS_NOT_NULL of `a`;
 * or PLGPU_OP_STR_{STARTS_WITH,ENDS_WITH,CONTAINS} against the literal.
 * Bytes compare lexicographically (a proper prefix first); a null operand
 * gives null except for the *_MISSING ops.  Replaces
 * polars-compute/src/comparisons/view.rs TotalEqKernel / TotalOrdKernel for
 * BinaryViewArray (and their _broadcast scalar forms). */
int plgpu_str_compare(const plgpu_column* a, const plgpu_column* b, const uint8_t* lit, int64_t lit_len, int32_t op,
                      plgpu_column* out, void* stream);

/* Group variance / standard deviation from per-group sums of squared
 * deviations (Float64) and non-null counts (UInt32 / Int64): null when
 * count <= ddof, else sum_sq / (count - ddof) (negative clamped to 0), the
 * square root when take_sqrt.  Replaces polars-compute/src/moment.rs:126
 * VarState::finalize as used by polars-expr/src/reduce/var_std.rs.  The
 * executor computes the sums with two exact group-by passes around the
 * per-row group mean (polaroid_amd/frame.py:_group_by_var). */
int plgpu_var_finalize(const plgpu_column* sum_sq, const plgpu_column* count, int32_t ddof, int32_t take_sqrt,
                       plgpu_column* out, void* stream);

/* Per-row squared deviation from the row's group mean, the second pass of
 * var / std for one integer / Boolean key: out[i] = (x[i] - mean[g])^2 with
 * g the row of group_key equal to row_key[i] (group keys unique; a null
 * row key matches the null group).  Null where x is null, the key is not a
 * group or the mean is null.  Same values as the composed join path
 * (x.cast(f64) - mean)^2, without materialising the joined frame. */
int plgpu_group_sq_dev(const plgpu_column* row_key, const plgpu_column* x, const plgpu_column* group_key,
                       const plgpu_column* group_mean, plgpu_column* out, void* stream);

/* Short-string codes: each string of at most 7 bytes as the Int64
 * (length << 56) | bytes (little-endian), exact and injective, so String
 * keys can cross the integer-keyed paths (the multi-GPU group-by's partial
 * states and exchange); *all_short = 0 if some string is longer (its code
 * is then 0).  Validity is carried.  plgpu_str_decode_short is the inverse. */
int plgpu_str_encode_short(const plgpu_column* strs, plgpu_column* out_codes, int32_t* all_short, void* stream);
int plgpu_str_decode_short(const plgpu_column* codes, plgpu_column* out, void* stream);

/* out[i] = a[i] if valid, else b[i] (same dtype and length); the coalesced
 * key columns of a full join with coalesce=True
 * (polars-ops/src/frame/join/general.rs:52 _coalesce_full_join). */
int plgpu_coalesce(const plgpu_column* a, const plgpu_column* b, plgpu_column* out, void* stream);

/* Inner equi-join on one integer key column per side, both of one dtype
 * (PLGPU_ERR_SCHEMA "datatypes of join keys don't match" otherwise, as the
 * reference and plgpu_join_multi; plgpu_join and plgpu_join_inner_take
 * alike).  Produces the matching row pairs as
 * two UInt32 index columns (the reference's IdxSize pairs).  Null keys match
 * only when nulls_equal != 0.  Replaces
 * polars-ops/src/frame/join/hash_join/single_keys_inner.rs:45
 * hash_join_tuples_inner (via _inner_join / JoinDispatch). */
int plgpu_join_inner(const plgpu_column* left_key, const plgpu_column* right_key,
                     int32_t nulls_equal, int32_t maintain_order, int32_t validate,
                     plgpu_column* out_left_idx, plgpu_column* out_right_idx, void* stream);

/* Inner join on one integer key plus the take of both frames' columns: the
 * left frame's `left_cols` and the right frame's `right_cols` (0..8 each,
 * every one as long as its side's key) at the matching pairs, in the pair
 * order of plgpu_join_inner; *out_len rows.  The fused form of
 * polars-ops/src/frame/join/hash_join/single_keys_inner.rs:45
 * hash_join_tuples_inner followed by _finish_join's takes
 * (polars-ops/src/frame/join/general.rs:17).  With one right column, unique
 * right keys and a null-free 8-byte right column the hash table is
 * row-format (each cell {key, payload}) and the emit pass writes the
 * payload and the null-free 8-byte left columns straight to their output
 * rows; other inputs take the pairs + gather route with the same result.
 * With maintain_order "none" (the reference's default), null-free 8-byte
 * integer keys and columns, a long probe side and a build side beyond the
 * L2s, the join is radix-partitioned (round 6): per-partition L2-resident
 * sub-tables (polars-ops/src/frame/join/hash_join/single_keys.rs:16
 * build_tables), the probe rows scattered by partition, rows out in
 * partition order. */
int plgpu_join_inner_take(const plgpu_column* left_key, const plgpu_column* right_key,
                          const plgpu_column* left_cols, int32_t nleft,
                          const plgpu_column* right_cols, int32_t nright, int32_t nulls_equal,
                          int32_t maintain_order, int32_t validate, plgpu_column* out_left,
                          plgpu_column* out_right, int64_t* out_len, void* stream);

/* plgpu_join_inner_take on 1..8 key columns per side (as plgpu_join_inner_multi):
 * integer / Boolean keys whose ranges pack into one exact Int64 take the
 * single-key route on the packed keys (row-format table included); other
 * keys compute the verified pairs and gather. */
int plgpu_join_inner_take_multi(const plgpu_column* left_keys, const plgpu_column* right_keys,
                                int32_t nkeys, const plgpu_column* left_cols, int32_t nleft,
                                const plgpu_column* right_cols, int32_t nright, int32_t nulls_equal,
                                int32_t maintain_order, int32_t validate, plgpu_column* out_left,
                                plgpu_column* out_right, int64_t* out_len, void* stream);

/* Inner join on 1..8 key columns per side (pairwise equal dtypes: I64 / I32 /
 * U32 / F64 / BOOL).  Replaces the multi-key branch of the reference's join
 * (polars-ops/src/frame/join/mod.rs:625 prepare_keys_multiple: both sides'
 * keys row-encoded, then hash-joined as binary keys; a tuple holding a null
 * joins only when nulls_equal).  Here tuples are hashed to 64 bits
 * (tuplehash.hpp), joined with the single-key kernels, and every output pair
 * is verified tuple by tuple (a collision re-runs with another seed).
 * Arguments, output and order modes as plgpu_join_inner. */
int plgpu_join_inner_multi(const plgpu_column* left_keys, const plgpu_column* right_keys,
                           int32_t nkeys, int32_t nulls_equal, int32_t maintain_order,
                           int32_t validate, plgpu_column* out_left_idx,
                           plgpu_column* out_right_idx, void* stream);

/* out_cols[i] = cols[i][idx] (UInt32 indices), validity carried; a null
 * index gathers a null.  Replaces the join materialisation take
 * (polars-core/src/chunked_array/ops/gather.rs, DataFrame::take_unchecked;
 * IdxCa::with_nullable_idx for the outer joins' nullable indices). */
int plgpu_gather(const plgpu_column* cols, int32_t ncols, const plgpu_column* idx,
                 plgpu_column* out_cols, void* stream);

/* ---- row shuffles (multi-GPU join / group-by) -------------------------------
 * Stable hash partitioning of rows by 1..8 key columns into nparts (1..1024)
 * partitions: out_perm (UInt32, library-owned) lists the rows partition by
 * partition, in row order within each; out_counts[p] = rows of partition p.
 * A key tuple holding a null is dropped when nulls_equal == 0 (it cannot
 * join) and routed to partition 0 otherwise.  The partition of a row depends
 * only on its key values, so every rank routes equal keys alike (floats by
 * TotalEq class, -0.0 with 0.0 and every NaN together; String keys by a hash
 * of their bytes).  Replaces
 * polars-utils/src/hashing.rs:101 HashPartitioner::hash_to_partition as
 * used by polars-stream/src/nodes/joins/equi_join.rs:445 / :740
 * (partition_and_sink / partition_and_probe). */
int plgpu_hash_partition(const plgpu_column* keys, int32_t nkeys, int32_t nparts,
                         int32_t nulls_equal, plgpu_column* out_perm, int64_t* out_counts,
                         void* stream);

/* Pack rows into caller-owned flat buffers (e.g. RCCL send tensors):
 * dst_values[i][o] = cols[i][idx[o]] (idx NULL: o), 8 / 4 bytes per value,
 * one byte (0/1) per Boolean value; dst_valid[i] (when dst_valid and
 * dst_valid[i] are non-NULL) gets one validity byte per row.  The
 * send-side half of the reference's per-partition DataFrame::take. */
int plgpu_gather_rows(const plgpu_column* cols, int32_t ncols, const plgpu_column* idx,
                      void* const* dst_values, uint8_t* const* dst_valid, void* stream);

/* Bytes (0 / non-zero) -> Arrow LSB-first bitmap of ceil(n / 64) 8-byte
 * words; *out_zero_count (optional) = number of zero bytes (the null count
 * of a validity mask).  The receive-side inverse of plgpu_gather_rows. */
int plgpu_pack_bits(const uint8_t* bytes, int64_t n, uint8_t* out_bits, int64_t* out_zero_count,
                    void* stream);

/* ---- sort ------------------------------------------------------------------
 * Stable arg-sort of one column (I64 / I32 / U32 / F64) into a UInt32
 * permutation: TotalOrd order (NaN greatest, -0.0 == 0.0), descending
 * reverses the order of distinct values while equal values keep their row
 * order, nulls first unless nulls_last.  Replaces
 * polars-core/src/chunked_array/ops/sort/arg_sort.rs arg_sort with
 * SortOptions { maintain_order: true } (options.rs:32); DataFrame.sort is
 * this permutation followed by plgpu_gather. */
int plgpu_arg_sort(const plgpu_column* key, int32_t descending, int32_t nulls_last,
                   plgpu_column* out_idx, void* stream);

/* Stable arg-sort by 1..8 columns (I64 / I32 / U32 / F64 / BOOL), each with
 * its own `descending[j]` and `nulls_last[j]`.  Replaces
 * polars-core/src/chunked_array/ops/sort/arg_sort_multiple.rs:24
 * arg_sort_multiple_impl (lexicographic compare, column by column, nulls
 * placed per column independently of `descending`; maintain_order = a stable
 * result, which this always is).  LSD over the columns: each column is one
 * stable radix sort of its codes through the running permutation, plus one
 * pass placing its nulls. */
int plgpu_arg_sort_multi(const plgpu_column* keys, int32_t nkeys, const int32_t* descending,
                         const int32_t* nulls_last, plgpu_column* out_idx, void* stream);

/* ---- rolling windows ---------------------------------------------------------
 * Fixed-size window sum / mean (window_size rows, min_periods non-null rows
 * for a valid output, optionally centred), like Series.rolling_sum /
 * rolling_mean.  Float64 (and integer mean) results are the correctly
 * rounded window sums (divided by the non-null count); integer sums wrap.
 * Replaces polars-compute/src/rolling/no_nulls/{sum,mean}.rs rolling_sum /
 * rolling_mean and nulls/{sum,mean}.rs (rolling/sum.rs:7 SumWindow).
 * VAR / STD (ddof in bits 8..15 of kind): Series.rolling_var / rolling_std,
 * replacing polars-compute/src/rolling/{no_nulls,nulls}/moment.rs
 * rolling_var (rolling/moment.rs:138 MomentWindow<VarianceMoment>) and
 * polars-time/src/chunkedarray/rolling_window/dispatch.rs:526 (std = its
 * square root): Float64 output, (RN(c sum x^2 - (sum x)^2) / c) / (c - ddof)
 * with the numerator exact; a non-finite value gives NaN; null below
 * min_periods non-null values or at c <= ddof. */
enum plgpu_rolling_kind {
    PLGPU_ROLLING_SUM = 1,
    PLGPU_ROLLING_MEAN = 2,
    PLGPU_ROLLING_MIN = 3,  /* rolling/no_nulls/min_max.rs MinWindow (NaN propagates) */
    PLGPU_ROLLING_MAX = 4,  /* ... MaxWindow; output dtype = input dtype            */
    PLGPU_ROLLING_VAR = 5,
    PLGPU_ROLLING_STD = 6
};

int plgpu_rolling(const plgpu_column* values, int32_t kind, int64_t window_size,
                  int64_t min_periods, int32_t center, plgpu_column* out, void* stream);

/* ---- window expressions over groups (Expr.over) ------------------------------
 * The device side of polars-expr/src/expressions/window.rs (WindowExpr::evaluate
 * :356 with WindowMapping::GroupsToRows, determine_map_strategy :296) for
 * rolling functions: the function runs on each group's rows in their order
 * and every result goes back to its row.
 *
 * plgpu_segment_starts: one pass over 1..8 key columns (integer, float or
 * Boolean; short String / Categorical keys as their Int64 / UInt32 codes).
 * out_starts is a null-free Boolean column of n rows (library-owned), bit i
 * set when i == 0 or row i's key tuple differs from row i - 1's -- the
 * group-by's equality (TotalEq: -0.0 == 0.0, NaN == NaN; a null equals a null
 * and nothing else).  *out_sorted = 1 when the rows are already non-decreasing
 * in the order plgpu_arg_sort_multi gives with every column ascending and
 * nulls first, so every run of equal tuples is a whole group (replaces
 * window.rs:433 df.group_by_with_series for keys that arrive sorted).
 *
 * plgpu_rolling_segmented: plgpu_rolling (same kinds, ddof bits, dtypes, output
 * dtype and validity rules) with every window also clipped to the segment of
 * its own row, [last set bit of seg_starts at or before the row, next set bit
 * after it): a row's output is bit-identical to plgpu_rolling's for that row
 * over the segment alone as a column.  seg_starts: null-free Boolean column of
 * the values' length (replaces window.rs:500 run_aggregation of a rolling
 * function: its evaluation on every group's rows).
 *
 * plgpu_invert_permutation: out_idx[idx[j]] = j for a null-free UInt32 index
 * column holding a permutation of 0..n-1 (as plgpu_arg_sort_multi returns), so
 * sorted-order results go back to row order through plgpu_gather (replaces
 * window.rs:125 map_by_arg_sort, the MapStrategy::Map branch at :524). */
int plgpu_segment_starts(const plgpu_column* keys, int32_t nkeys, plgpu_column* out_starts,
                         int32_t* out_sorted, void* stream);
int plgpu_rolling_segmented(const plgpu_column* values, const plgpu_column* seg_starts, int32_t kind,
                            int64_t window_size, int64_t min_periods, int32_t center,
                            plgpu_column* out, void* stream);
int plgpu_invert_permutation(const plgpu_column* idx, plgpu_column* out_idx, void* stream);

/* ---- cumulative and lag functions ----------------------------------------------
 * plgpu_cumulative: the running sum / minimum / maximum / non-null count of a
 * column, restarted at every set bit of seg_starts (NULL: one segment; else a
 * null-free Boolean column of the values' length, as plgpu_segment_starts
 * writes it).  Replaces polars-ops/src/series/ops/cum_agg.rs cum_sum :340,
 * cum_min :378, cum_max :416, cum_count :420 (the det_* folds at :14-51) and,
 * with seg_starts, their evaluation on every group's rows
 * (polars-expr/src/expressions/window.rs:356, GroupsToRows).  A null row gives
 * null and leaves the running value as it was.
 *   SUM    Int32 / Int64 / UInt64 wrap at their width; Float64 is the correctly rounded
 *          exact sum of the segment's non-null values so far (rounded once; a
 *          zero sum is +0.0), NaN after a NaN or after both infinities, else
 *          the infinity that occurred.  PLGPU_ERR_SCHEMA when the column's
 *          finite non-zero values span more than 67 binades (the fixed-point
 *          accumulator's window less a significand).  This refusal depends on
 *          the data, not on the schema: it is found on the device, after the
 *          launches, and reported with the code the library uses for polars'
 *          ComputeError (PLGPU_ERR_SCHEMA; plgpu_last_error states the span
 *          and the limit); no output column is returned.
 *   MIN / MAX  Int32 / Int64 / UInt64 / Float64, dtype kept; a NaN is skipped once a
 *          non-NaN value has been seen, before that the output is NaN.
 *   COUNT  any dtype; UInt32 output without nulls.
 * Three launches (tile reduce, scan of the tile totals, apply); no workgroup
 * waits on another.
 *
 * plgpu_lag: SHIFT out[i] = values[i - n] (validity with the value) where row
 * i - n lies in the column and no segment start lies in (i - n, i] (n > 0) or
 * (i, i - n] (n < 0); elsewhere fill_bits (the value's bits in the column's
 * dtype) when has_fill, else null.  Replaces ChunkedArray::shift_and_fill.
 * DIFF out[i] = values[i] - values[i - n] under the same rule (null where
 * either is; has_fill ignored): one IEEE subtraction for floats, wrapping for
 * integers.  Replaces polars-ops/src/series/ops/diff.rs:4 with
 * NullBehavior::Ignore.  4- and 8-byte numeric dtypes (DIFF: signed and float
 * ones); the output keeps the dtype. */
enum plgpu_cum_kind { PLGPU_CUM_SUM = 1, PLGPU_CUM_MIN = 2, PLGPU_CUM_MAX = 3, PLGPU_CUM_COUNT = 4 };
int plgpu_cumulative(const plgpu_column* values, const plgpu_column* seg_starts /* NULL: one segment */,
                     int32_t kind, plgpu_column* out, void* stream);
enum plgpu_lag_kind { PLGPU_LAG_SHIFT = 1, PLGPU_LAG_DIFF = 2 };
int plgpu_lag(const plgpu_column* values, const plgpu_column* seg_starts, int32_t kind, int64_t n,
              int32_t has_fill, int64_t fill_bits /* value bits in the column's dtype */,
              plgpu_column* out, void* stream);

/* ---- forward / backward fill ---------------------------------------------------
 * plgpu_fill: the nulls of a column replaced by the closest non-null value
 * before (FORWARD) or after (BACKWARD) them, at a distance of at most `limit`
 * rows (limit < 0: any distance; 0 fills nothing) and never across a set bit of
 * seg_starts (NULL: one segment; else a null-free Boolean column of the values'
 * length, as plgpu_segment_starts writes it).  Replaces
 * polars-core/src/chunked_array/ops/fill_null.rs:58 Series::fill_null with
 * FillNullStrategy::Forward / Backward: :130 fill_forward_numeric, :160
 * fill_backward_numeric, :258 fill_forward_gather_limit, :304
 * fill_backward_gather_limit, and with seg_starts their evaluation on every
 * group's rows (polars-expr/src/expressions/window.rs:356, GroupsToRows).  A
 * non-null row keeps its value; leading (FORWARD) / trailing (BACKWARD) nulls
 * of a column or segment stay null.  Values are moved as their bits (a NaN
 * keeps its payload, -0.0 stays -0.0).  4- and 8-byte dtypes; the output keeps
 * the dtype.  A column without a validity buffer is copied (no kernel runs).
 * PLGPU_ERR_INVALID: a NULL values / out, an unknown kind, a seg_starts that is
 * not a null-free Boolean column of the values' length; PLGPU_ERR_SCHEMA: any
 * other dtype; both before any device work.  n == 0 is legal.
 * Three launches over the bitmaps and one pass over the values (bitmap reduce
 * per tile, scan of the tile summaries, apply); no workgroup waits on another. */
enum plgpu_fill_kind { PLGPU_FILL_FORWARD = 1, PLGPU_FILL_BACKWARD = 2 };
int plgpu_fill(const plgpu_column* values, const plgpu_column* seg_starts /* NULL: one segment */,
               int32_t kind, int64_t limit /* < 0: no limit */, plgpu_column* out, void* stream);

/* ---- exponentially weighted mean -----------------------------------------------
 * plgpu_ewm_mean: the exponentially weighted mean of a Float32 / Float64
 * column, restarted at every set bit of seg_starts (NULL: one segment; else a
 * null-free Boolean column of the values' length, as plgpu_segment_starts
 * writes it).  Replaces polars-compute/src/ewm/mean.rs:52
 * EwmMeanState::update_iter (through polars-ops/src/series/ops/ewm.rs:11
 * ewm_mean and polars-expr/src/dispatch/misc.rs:887) and, with seg_starts, its
 * evaluation on every group's rows (polars-expr/src/expressions/window.rs:356,
 * GroupsToRows).  The state (mean, weight, count) is zero at the start of a
 * segment; its first non-null row sets mean = x, weight = 1; every other row
 * multiplies weight by 1 - alpha when it is non-null or ignore_nulls is 0, and
 * a non-null row then does mean += (x - mean) * v / (weight + v) with v = 1
 * (adjust; weight += 1) or alpha (no adjust; weight = 1).  A row is non-null
 * in the output when it is non-null in the input and the segment has seen at
 * least max(min_samples, 1) non-null rows.  The dtype is kept; Float32 is
 * computed in double and rounded once.
 * Non-finite values: the first NaN / +inf / -inf among the non-null values of
 * a column or segment comes out as itself, every later non-null row of that
 * segment is NaN (the reference's x - mean); a segment start clears this.
 * The first non-null row of a segment equals its input bit for bit; other rows
 * agree with the reference's sequential fold within the bound DESIGN.md "Float
 * tolerance against the reference" states (a scan rounds in tree order).
 * PLGPU_ERR_INVALID: a NULL values / out, alpha outside (0, 1] or NaN, a
 * negative min_samples, a seg_starts that is not a null-free Boolean column of
 * the values' length; PLGPU_ERR_SCHEMA: any other dtype; both before any
 * device work.  n == 0 is legal.
 * Three launches (tile reduce, scan of the tile summaries, apply); no
 * workgroup waits on another. */
int plgpu_ewm_mean(const plgpu_column* values, const plgpu_column* seg_starts /* NULL: one segment */,
                   double alpha, int32_t adjust, int32_t ignore_nulls, int64_t min_samples,
                   plgpu_column* out, void* stream);

/* ---- rank -------------------------------------------------------------------------
 * plgpu_rank: the ranks of a column from its stable sort, for the whole column
 * or per segment.  The caller has sorted (plgpu_arg_sort / plgpu_arg_sort_multi,
 * which break ties in row order whatever `descending` says, as the reference's
 * stable sort_by does), gathered, and marked the runs (plgpu_segment_starts:
 * TotalEq, so -0.0 ties with 0.0 and NaN with NaN; a null equals a null).
 * Replaces polars-ops/src/series/ops/rank.rs:68 rank (:32 rank_impl and its
 * flush closures) and, with seg_starts, its evaluation on every group's rows
 * (polars-expr/src/expressions/window.rs:356, GroupsToRows).
 *   sorted_idx     null-free UInt32 permutation of 0..n-1: sorted row j is row
 *                  sorted_idx[j] of `values`.
 *   sorted_values  the ranked column gathered through sorted_idx.  Only its
 *                  validity is read; within every segment its nulls are last.
 *   tie_starts     null-free Boolean, n rows: sorted row j begins a run of equal
 *                  (keys, value).
 *   seg_starts     NULL: one segment; else null-free Boolean, n rows, as
 *                  plgpu_segment_starts writes it for the keys.  Row 0 starts a
 *                  segment and every segment start is a tie start, whatever the
 *                  two bitmaps say (they are ORed on the device).
 *   values         the ranked column in row order: only its validity is read,
 *                  and becomes the output's (realigned to offset 0; no validity
 *                  buffer when `values` has none).
 * For sorted row j with s the last segment start <= j, a the last tie start
 * <= j and b the next tie start > j (n when there is none):
 *   ORDINAL j - s + 1     MIN a - s + 1     MAX b - s
 *   AVERAGE 0.5 * ((double)min + (double)max)   (rank.rs:154)
 *   DENSE   the number of tie starts in [s, j]
 * written at out[sorted_idx[j]]: the output is in row order.  Sorted rows
 * whose sorted_values bit is clear write nothing; the value buffer is zeroed
 * first when there are any, so a null row's bytes are defined.  Nulls being
 * last in their segment, a non-null row's rank counts non-null rows only.
 * UInt32 output (the reference's IdxSize), Float64 for AVERAGE.
 * Every input may be sliced and its bitmap unaligned.
 * PLGPU_ERR_INVALID: a NULL argument (seg_starts apart), an unknown method,
 * lengths that differ, a sorted_idx that is not a null-free UInt32 column, a
 * tie_starts / seg_starts that is not a null-free Boolean column, more than
 * 2^32 - 1 rows; all before any device work.  n == 0 is legal.
 * Three launches over the bitmaps and one pass over sorted_idx (bitmap reduce
 * per tile, scan of the tile summaries in both directions, apply with the
 * scatter); no workgroup waits on another. */
enum plgpu_rank_method {
    PLGPU_RANK_AVERAGE = 1,
    PLGPU_RANK_MIN = 2,
    PLGPU_RANK_MAX = 3,
    PLGPU_RANK_DENSE = 4,
    PLGPU_RANK_ORDINAL = 5
};
int plgpu_rank(const plgpu_column* sorted_idx, const plgpu_column* sorted_values, const plgpu_column* tie_starts,
               const plgpu_column* seg_starts /* NULL: one segment */, const plgpu_column* values, int32_t method,
               plgpu_column* out, void* stream);

/* ---- as-of join -----------------------------------------------------------------
 * plgpu_join_asof: for every left row the row of the right side whose `on` key
 * is the closest at or before (BACKWARD), at or after (FORWARD) or on either
 * side (NEAREST) of the left key: a left join in left-row order, as one UInt32
 * index column with validity, the form plgpu_join writes for a left join and
 * plgpu_gather takes.  Replaces polars-ops/src/frame/join/asof/mod.rs:46-199
 * (AsofJoinForwardState / BackwardState / NearestState::next), default.rs:11
 * join_asof_impl and :112 join_asof_numeric, and with ranges groups.rs:38
 * asof_in_group.  The reference walks both sides with one running state; for
 * ascending right keys its answer is a function of each left key alone, which
 * is what is computed here.  With lb(x) the first position of the non-null
 * right keys whose value is >= x and ub(x) the first whose value is > x:
 *   BACKWARD  ub(l) - 1 (allow_eq: the last of a run of equal values), else
 *             lb(l) - 1; nothing before the first value.
 *   FORWARD   lb(l) (allow_eq: the first of a run), else ub(l); nothing past
 *             the end.
 *   NEAREST   with allow_eq and a value equal to l, ub(l) - 1.  Otherwise
 *             lower = lb(l) - 1 and upper = the last of the run of equal
 *             values that begins at ub(l); one side missing takes the other;
 *             upper when abs_diff(l, upper) <= abs_diff(l, lower), else lower.
 *   tolerance (has_tolerance != 0): the one match chosen above is kept only if
 *             abs_diff(l, r) <= |tolerance|; no other candidate is looked for.
 *             Integer keys take tolerance_bits (an Int64; the bits of a UInt64
 *             for UInt64 keys), float keys tolerance_f64 (rounded to the key's
 *             type).
 *   abs_diff  integers: the exact unsigned difference; floats: |l - r| in the
 *             key's own type (a NaN difference passes no tolerance).
 * Floats compare by TotalOrd (-0.0 == 0.0, NaN greatest and equal to itself);
 * the reference's partial_cmp stalls its scan at a NaN.  A null left key, and
 * every row when all right keys are null, gets no match.  The right keys are
 * taken to be ascending with their nulls first; on other input the result is
 * unspecified, and every index is still null or a row of the right side.
 * lo / hi (both or neither; null-free UInt32 columns of the left length): left
 * row i searches positions [lo[i], hi[i]) of the right column only, clamped
 * into [0, length] (a reversed range is empty); the right column then has no
 * validity buffer.  right_rows (a null-free UInt32 column of the right length,
 * or NULL): the index written is right_rows[position].  *out_path (optional):
 * 1 the window search (option "asof_path"), 2 the whole-column search, 3 ranges.
 * Keys: Int32 / Int64 / UInt32 / UInt64 / Float32 / Float64, both sides alike.
 * PLGPU_ERR_INVALID: a NULL left_on / right_on / out_idx, an unknown strategy,
 * lo without hi, lo / hi / right_rows of another dtype or length or with a
 * validity buffer, ranges with a nullable right column, a right side of
 * 2^32 - 1 rows or more; PLGPU_ERR_SCHEMA: unequal or other key dtypes; all
 * before any device work.  Empty sides are legal.
 * One launch (two when the right column has a validity buffer: its first
 * non-null row is found first); no workgroup waits on another.
 *
 * plgpu_is_sorted_asc: one pass over a column of those dtypes.
 * *out_nulls_first = 1 when no null follows a non-null row; *out_ascending = 1
 * when no non-null value is smaller (TotalOrd) than a non-null value right
 * before it.  Both together are the reference's ensure_sorted_arg with the
 * default SortOptions (polars-ops/src/series/ops/various.rs:69). */
enum plgpu_asof_strategy { PLGPU_ASOF_BACKWARD = 0, PLGPU_ASOF_FORWARD = 1, PLGPU_ASOF_NEAREST = 2 };
int plgpu_join_asof(const plgpu_column* left_on, const plgpu_column* right_on,
                    const plgpu_column* lo /* NULL: the whole right column */, const plgpu_column* hi,
                    const plgpu_column* right_rows /* NULL: positions are rows */, int32_t strategy,
                    int32_t allow_eq, int32_t has_tolerance, int64_t tolerance_bits, double tolerance_f64,
                    plgpu_column* out_idx, int32_t* out_path, void* stream);
int plgpu_is_sorted_asc(const plgpu_column* col, int32_t* out_ascending, int32_t* out_nulls_first, void* stream);

/* ---- quantile ---------------------------------------------------------------------
 * plgpu_segment_quantile: nq quantiles of every segment of a column that is
 * sorted within its segments: median / quantile, plain, per group and over
 * keys.  The caller has sorted by (group, value) with the value's nulls last
 * (plgpu_arg_sort_multi), gathered, and marked the segment starts of the
 * gathered groups (plgpu_segment_starts).  Replaces
 * polars-core/src/chunked_array/ops/aggregate/quantile.rs:106 generic_quantile
 * (:16 quantile_idx, :46 linear_interpol, :54 midpoint_interpol) and over groups
 * polars-core/src/frame/group_by/aggregations/mod.rs:251 agg_quantile_generic.
 *   sorted_values  Int32 / Int64 / UInt32 / Float64; within every segment
 *                  ascending in TotalOrd (NaN greatest) with its nulls last.
 *   seg_starts     NULL: one segment (also of an empty column: one null row);
 *                  else null-free Boolean, n rows; row 0 starts a segment
 *                  whatever its bit says.  With n == 0 the outputs have no rows.
 *   quantiles      nq values in [0, 1].
 *   methods        nq values of plgpu_quantile_method.
 *   outs           nq owned Float64 columns, one row per segment in segment
 *                  order.  They carry a validity buffer only when some segment
 *                  holds no non-null value; such a row is null and its bytes
 *                  are zero.
 * For a segment of len rows, nc of them null, nn = len - nc > 0, in f64:
 *   float_idx = (nn - 1.0) * q + (double)nc
 *   NEAREST       idx = round(float_idx), halves away from zero
 *   EQUIPROBABLE  idx = max(ceil(nn * q) - 1.0, 0.0) + nc
 *   LOWER / MIDPOINT / LINEAR  idx = min((size_t)float_idx, len - 1)
 *   HIGHER        idx = min((size_t)ceil(float_idx), len - 1)
 * idx counts the segment's rows with its nulls first, so the row read is
 * start + (idx - nc); lower = (double)sorted[idx] is the result, except that
 * MIDPOINT and LINEAR with ceil(float_idx) != idx take upper = (double)sorted[idx + 1]
 * and give, when lower != upper (IEEE), (lower + upper) / 2.0 and
 * (float_idx - (double)idx) * (upper - lower) + lower.
 * Every input may be sliced and its bitmap unaligned.
 * PLGPU_ERR_INVALID: a NULL argument (seg_starts apart), nq outside 1..8, a
 * quantile outside [0, 1] or NaN, an unknown method, another dtype, a
 * seg_starts that is not a null-free Boolean column of the values' length, more
 * than 2^32 - 1 rows; all before any device work.
 * Four launches (segment starts per tile, scan of the tile counts, the starts
 * as row ids, one lane per segment), one device-to-host copy of the segment
 * count between them; no workgroup waits on another. */
enum plgpu_quantile_method {
    PLGPU_QUANTILE_NEAREST = 1,
    PLGPU_QUANTILE_HIGHER = 2,
    PLGPU_QUANTILE_LOWER = 3,
    PLGPU_QUANTILE_MIDPOINT = 4,
    PLGPU_QUANTILE_LINEAR = 5,
    PLGPU_QUANTILE_EQUIPROBABLE = 6
};
int plgpu_segment_quantile(const plgpu_column* sorted_values, const plgpu_column* seg_starts /* NULL: one segment */,
                           const double* quantiles, const int32_t* methods, int32_t nq, plgpu_column* outs,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POLAROID_GPU_H */
