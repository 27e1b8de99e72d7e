/*
 * strawboat_hip.h — C ABI of the MI355X-native page encode/decode path of strawboat.
 *
 * This is the drop-in boundary a host (the Rust crate, or the C++/Python host layer in
 * this repo) binds: plain pointers and sizes, no C++/torch types, `extern "C"`, int32
 * status codes, errors as strings per context.  Every entry point names the reference
 * seam it replaces (file:line under the sundy-li/strawboat tree).
 *
 * Unit of work: the *pages of leaf columns*.  A call takes a batch of columns; every
 * (column, page) is an independent work item scheduled over the GPU.
 * All work is enqueued on the context's HIP stream; nothing is valid on the host until
 * sb_ctx_synchronize() returned SB_OK.
 *
 * Memory: buffers marked DEVICE are HBM pointers (hipMalloc / torch tensors on the
 * context's device) when `mem == SB_MEM_DEVICE` — the measured configuration — or host
 * pointers when `mem == SB_MEM_HOST` (the library stages them over PCIe itself; this is
 * the shape the reference's `&[u8]` / `Vec<T>` callers have).
 */
#ifndef STRAWBOAT_HIP_H
#define STRAWBOAT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes: arrow2::error::Error variants used on this path
 *      (src/errors.rs:19-31, src/compression/mod.rs:78-80, basic.rs:104,116,129) */
#define SB_OK 0
#define SB_ERR_OUT_OF_SPEC (-1)  /* Error::OutOfSpec: unknown codec, corrupt page, size mismatch */
#define SB_ERR_EXTERNAL (-2)     /* Error::External: LZ4/Zstd stream rejected, HIP runtime failure */
#define SB_ERR_IO (-3)           /* Error::Io(UnexpectedEof): page shorter than its headers say */
#define SB_ERR_NYI (-4)          /* Error::NotYetImplemented: codec/type not handled on the device */
#define SB_ERR_INVALID (-5)      /* bad argument at the boundary (null pointer, capacity too small) */

/* ---- on-disk codec ids: enum Compression (src/compression/mod.rs:37-51,92-108) */
#define SB_CODEC_NONE 0
#define SB_CODEC_LZ4 1
#define SB_CODEC_ZSTD 2
#define SB_CODEC_SNAPPY 3
#define SB_CODEC_RLE 10
#define SB_CODEC_DICT 11
#define SB_CODEC_ONEVALUE 12
#define SB_CODEC_FREQ 13
#define SB_CODEC_BITPACKING 14
#define SB_CODEC_DELTA_BITPACKING 15
#define SB_CODEC_PATAS 16

/* ---- physical kinds: the dispatch key of batch_read::read_simple
 *      (src/read/batch_read.rs:37-63) and write_simple (src/write/serialize.rs:62-129).
 *      Utf8/LargeUtf8 are written as Binary/LargeBinary (serialize.rs:92-121). */
#define SB_TYPE_BOOLEAN 0
#define SB_TYPE_INT8 1
#define SB_TYPE_INT16 2
#define SB_TYPE_INT32 3
#define SB_TYPE_INT64 4
#define SB_TYPE_UINT8 5
#define SB_TYPE_UINT16 6
#define SB_TYPE_UINT32 7
#define SB_TYPE_UINT64 8
#define SB_TYPE_INT128 9
#define SB_TYPE_INT256 10
#define SB_TYPE_FLOAT32 11
#define SB_TYPE_FLOAT64 12
#define SB_TYPE_BINARY 13       /* i32 offsets: Binary, Utf8 */
#define SB_TYPE_LARGE_BINARY 14 /* i64 offsets: LargeBinary, LargeUtf8 */
#define SB_TYPE_NULL 15

#define SB_MEM_DEVICE 0
#define SB_MEM_HOST 1

/* PageMeta (src/lib.rs:75-80): bytes of the page in the file, rows (flat columns) */
typedef struct sb_page_meta {
    uint64_t length;
    uint64_t num_values;
} sb_page_meta;

/* WriteOptions (src/write/common.rs:37-45) plus the two knobs a deterministic build needs
 * (SURVEY.md App. B#1): a forced codec (the reference only has debug-build env switches,
 * src/util/env.rs:20-24) and a seed for the sampling in compress_sample_ratio
 * (src/compression/integer/mod.rs:310-347 uses thread_rng()). */
typedef struct sb_write_options {
    int32_t default_compression;       /* CommonCompression: SB_CODEC_NONE/LZ4/ZSTD/SNAPPY */
    int32_t has_default_compress_ratio;/* Option<f64> discriminant */
    double default_compress_ratio;
    uint64_t max_page_size;            /* 0 = None */
    uint32_t forbidden_compressions;   /* bit (1u << codec id) set = forbidden */
    int32_t force_codec;               /* -1 = choose; else the page codec */
    int32_t force_index_codec;         /* -1 = choose; else codec of Dict indices / Freq exceptions */
    uint32_t flags;                    /* SB_WRITE_* bits, 0 = defaults */
    uint64_t rng_seed;                 /* column-level seed; page p uses mix64(seed ^ p*K) */
} sb_write_options;

/* sb_write_options.flags.
 * SB_WRITE_LZ4_EXACT: LZ4 blocks byte-identical to liblz4's LZ4_compress_default (what the reference's lz4 crate calls,
 * src/compression/basic.rs:108-120) — the serial greedy parse, ~10x slower on the device.  Default: a parallel
 * parse that emits a format-valid block every LZ4 decoder (hence the reference) reads back to the same bytes;
 * compressed-byte identity is library-version dependent upstream (no lockfile) and not part of the page layout. */
#define SB_WRITE_LZ4_EXACT 1u
/* SB_WRITE_DEBUG_VERIFY_FAIL (tests only): the string check behind the adaptive binary selector's hashed key count reports a
 * collision on every page, so that the exact re-selection and the exact dictionary build run; the bytes written are the same. */
#define SB_WRITE_DEBUG_VERIFY_FAIL (1u << 30)

typedef struct sb_ctx sb_ctx;

/* One context per host thread / stream, like one NativeWriter or column reader per thread
 * upstream (src/read/deserialize.rs:28: iterators are Send + Sync, no shared state).
 * `hip_stream` may be NULL (the context then creates its own non-blocking stream). */
int32_t sb_ctx_create(int32_t device, void* hip_stream, sb_ctx** out);
void sb_ctx_destroy(sb_ctx* ctx);
/* waits for all enqueued work; returns the first error raised by a kernel since the last
 * synchronize (status word in HBM) or by the runtime */
int32_t sb_ctx_synchronize(sb_ctx* ctx);
const char* sb_ctx_last_error(sb_ctx* ctx);
void* sb_ctx_stream(sb_ctx* ctx);

/* ------------------------------------------------------------------ decode
 * Replaces, per leaf column, batch_read::read_simple -> read_integer / read_double /
 * read_boolean / read_binary (src/read/batch_read.rs:27-64; src/read/array/integer.rs:210-238,
 * boolean.rs:191-219, binary.rs:223-265), i.e. per page read_validity
 * (src/read/read_basic.rs:36-63) + decompress_integer|double|boolean|binary
 * (src/compression/integer/mod.rs:72-117, double/mod.rs:69-114, boolean/mod.rs:63-102,
 * binary/mod.rs:95-183).  Output buffers receive the pages back to back, exactly what the
 * reference appends to its Vec<T> / MutableBitmap / offsets+values Vecs. */
typedef struct sb_column_read {
    int32_t physical_type;   /* SB_TYPE_* */
    int32_t is_nullable;     /* schema field nullable => pages carry a def-level section */
    const uint8_t* pages;    /* DEVICE: the column's pages, concatenated as in the file */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST: ColumnMeta.pages */
    uint64_t n_pages;
    /* outputs (DEVICE).  Capacities in bytes; bitmaps are written in 32-bit words, so their buffers are
     * 4-byte aligned with a capacity of 4*ceil(rows/32) (SB_ERR_INVALID otherwise).
     * Alignment: `pages` may start at any byte (a pointer into a file buffer); `values` of a primitive column and `offsets`
     * at the element's natural alignment (16 bytes for Int128 / Int256), the value bytes of a binary column at any byte.
     * Nothing is written outside the capacities given, and no result depends on bytes outside a page's own. */
    void* values;            /* primitives: rows*w; boolean: ceil(rows/8) bitmap bytes; binary: value bytes */
    uint64_t values_capacity;
    uint8_t* validity;       /* ceil(rows/8) bitmap bytes, LSB-first; required iff is_nullable */
    uint64_t validity_capacity;
    void* offsets;           /* binary: (rows+1) offsets of i32/i64 */
    uint64_t offsets_capacity;
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;           /* sum of num_values */
    uint64_t values_len;     /* bytes produced in `values` */
    /* optional (HOST, n_pages entries): byte offset of every page's data inside `pages`.  NULL =
     * the pages are back to back.  Used for the leaf blocks of nested pages, which sit behind
     * their level sections (sb_nested_read_levels reports the offsets).  The offsets need not ascend; a page that does
     * not lie inside [0, pages_len) is refused at the call (SB_ERR_IO, nothing enqueued). */
    const uint64_t* page_offsets;
} sb_column_read;

/* Enqueue the decode of `n` columns.  Binary columns whose value bytes are not known in
 * advance: call sb_read_columns_sizes first, or pass a capacity that is large enough
 * (the reference guesses 4x the page bytes, src/read/array/binary.rs:241). */
int32_t sb_read_columns(sb_ctx* ctx, sb_column_read* cols, uint64_t n, int32_t mem);
/* Parses only the page headers on the device and fills rows / values_len (synchronous). */
int32_t sb_read_columns_sizes(sb_ctx* ctx, sb_column_read* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ filter
 * What a query engine does first with the filter columns of a block (databend: read the columns of a
 * WHERE clause, evaluate it, then decide which rows of the other columns it needs): the pages of a
 * primitive column go in, one bit per row comes out.  The values are compared where the decoder
 * would have stored them (one compare per run of an RLE page, per entry of a Dict page, per OneValue
 * page), so `rows / 8` bytes are written instead of `rows * width`.
 *
 * Comparisons (EQ .. GE): INT8..INT64, UINT8..UINT64 (signedness from the physical type), FLOAT32,
 * FLOAT64.  A null row never satisfies a comparison.  Floats compare as IEEE 754: NaN satisfies only
 * NE, -0.0 == 0.0.  IS_NULL / IS_NOT_NULL: every physical type (only the def-level section of a page
 * is looked at; a non-nullable column has no null row, every row of a SB_TYPE_NULL column is null).
 * A comparison on any other type: SB_ERR_NYI at the call, the selection is not touched (Binary / LargeBinary columns:
 * sb_filter_columns_var below, whose literal is a pointer and a length). */
#define SB_PRED_EQ 0
#define SB_PRED_NE 1
#define SB_PRED_LT 2
#define SB_PRED_LE 3
#define SB_PRED_GT 4
#define SB_PRED_GE 5
#define SB_PRED_IS_NULL 6
#define SB_PRED_IS_NOT_NULL 7

#define SB_SEL_SET 0 /* selection  = result; bits at positions >= rows of the last word are written as 0 */
#define SB_SEL_AND 1 /* selection &= result; bits at positions >= rows stay as they are */
#define SB_SEL_OR 2  /* selection |= result; bits at positions >= rows stay as they are */

typedef struct sb_column_filter {
    int32_t physical_type;   /* SB_TYPE_* */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE: as in sb_column_read, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST), as in sb_column_read */
    int32_t op;              /* SB_PRED_* */
    int32_t combine;         /* SB_SEL_* */
    uint8_t literal[8];      /* a value of the column's own type, little endian; ignored by IS_[NOT_]NULL */
    uint8_t* selection;      /* DEVICE: LSB-first bitmap, 4-byte aligned */
    uint64_t selection_capacity; /* >= 4*ceil(rows/32) bytes */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;           /* sum of num_values */
    uint64_t selected;       /* bits set in `selection` below `rows`, after combining */
} sb_column_filter;

/* Enqueue the filter of `n` columns, like sb_read_columns: results and errors (the codes the decoder raises for the
 * same corrupt page) at sb_ctx_synchronize.  With SB_SEL_AND / SB_SEL_OR the buffer's contents are an input: chain
 * predicates with one call after the other on the context's stream; two columns of ONE call whose selection buffers
 * overlap are refused (SB_ERR_INVALID).  The call is part of its synchronize interval like a read call: when the
 * interval is issued again (sb_ctx_replays) it is issued again in its place, which gives the same bits for all three
 * modes.  Its own kernels are launched without consulting the launch hints of the read path.
 * `mem`: SB_MEM_DEVICE.  SB_MEM_HOST is not implemented (SB_ERR_NYI): stage the pages and the bitmap yourself. */
int32_t sb_filter_columns(sb_ctx* ctx, sb_column_filter* cols, uint64_t n, int32_t mem);

/* The same call with a literal of any length: what a predicate on a Binary / LargeBinary column (Utf8 / LargeUtf8 are
 * stored as these) needs.  Numeric columns, IS_[NOT_]NULL, SET / AND / OR, `rows` / `selected`, errors and replays are
 * those of sb_filter_columns bit for bit, and numeric and binary columns may share one call.
 *
 * Binary columns, EQ .. GE: values compare as byte strings — bytes unsigned, lexicographic, a proper prefix is less
 * than the longer string (Rust's `<[u8] as Ord>`, what arrow2 compares Binary and Utf8 with).  The empty string is a
 * value like any other.  STARTS_WITH: the value has at least literal_len bytes and its first literal_len bytes equal
 * the literal; an empty literal selects every non-null row.  A null row satisfies nothing.
 * The predicate is evaluated once per entry of a Dict page (and of a Freq page, which is read as one), once per
 * OneValue page and once per row of a plain page; no offsets and no value bytes are written.  The value blocks of
 * LZ4 / Zstd / Snappy pages are inflated into a staging area of the context first: `stage_capacity` bounds the bytes
 * this column may take there (the sum of the uncompressed sizes of those blocks; 0 = 4 * pages_len, the reference's
 * guess for a binary read, src/read/array/binary.rs:241).  A column that needs more raises SB_ERR_INVALID at the
 * synchronize, as sb_read_columns does for a `values` buffer that is too small.
 *
 * Binary columns, ENDS_WITH / CONTAINS / NOT_STARTS_WITH / NOT_ENDS_WITH / NOT_CONTAINS (`LIKE '%lit'`, `LIKE '%lit%'`,
 * `NOT LIKE ...`): everything works on bytes, which for valid UTF-8 equals a search by characters.  CONTAINS: there is
 * an i with value[i .. i + literal_len) equal to the literal.  ENDS_WITH: the value has at least literal_len bytes and
 * its last literal_len bytes equal the literal.  A NOT_ op selects exactly the non-null rows whose positive form is
 * false (SET / AND / OR have no complement, and a null row must satisfy neither form, so these are ops of their own).
 * A null row satisfies none of the five, whatever bytes its slot holds.  An empty literal: the positive forms select
 * every non-null row, the negated forms none.  Once per Dict / Freq entry as above; on a plain page CONTAINS scans the
 * value bytes of 4096 rows at a time, so its cost follows the bytes and not the rows.  Struct, combine modes, the zero
 * bits behind `rows` after SET, page_offsets, stage_capacity, page errors and replays are those of STARTS_WITH.
 *
 * Refused at the call (nothing enqueued, no selection touched): STARTS_WITH or one of ops 11 .. 15 on a type that is
 * not binary, ops 9 and 10 (sb_filter_columns_in) and every op above 15, a numeric literal_len that is not the type's
 * width, a binary literal of more than 2^30 bytes, a null literal with literal_len > 0 (SB_ERR_INVALID); comparisons
 * on Boolean / Int128 / Int256 / Null, SB_MEM_HOST (SB_ERR_NYI).  sb_filter_columns refuses ops 8 and above, and
 * sb_filter_columns_in everything but 9 and 10. */
#define SB_PRED_STARTS_WITH 8
#define SB_PRED_ENDS_WITH 11          /* (9 and 10: SB_PRED_IN / SB_PRED_NOT_IN below) */
#define SB_PRED_CONTAINS 12
#define SB_PRED_NOT_STARTS_WITH 13
#define SB_PRED_NOT_ENDS_WITH 14
#define SB_PRED_NOT_CONTAINS 15

typedef struct sb_column_filter_var {
    int32_t physical_type;   /* SB_TYPE_* */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST) */
    int32_t op;              /* SB_PRED_* */
    int32_t combine;         /* SB_SEL_* */
    const uint8_t* literal;  /* HOST, literal_len bytes; must stay valid until sb_ctx_synchronize (a replay reads it again) */
    uint64_t literal_len;    /* numbers: exactly the type's width; binary: any length, 0 included; ignored by IS_[NOT_]NULL */
    uint8_t* selection;      /* DEVICE: LSB-first bitmap, 4-byte aligned */
    uint64_t selection_capacity; /* >= 4*ceil(rows/32) bytes */
    uint64_t stage_capacity; /* binary comparison columns: see above; 0 = 4 * pages_len */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;
    uint64_t selected;
} sb_column_filter_var;      /* 112 bytes */

int32_t sb_filter_columns_var(sb_ctx* ctx, sb_column_filter_var* cols, uint64_t n, int32_t mem);

/* Set membership: `WHERE c IN (v0, v1, ...)` / `NOT IN` with up to SB_IN_MAX_VALUES literals per column, evaluated on the
 * pages in ONE walk of them (n chained EQ / OR calls walk and inflate them n times).  A non-null row satisfies IN when
 * its value equals at least one literal and NOT_IN when it equals none; a null row satisfies neither.
 *
 * Numbers (INT8..INT64, UINT8..UINT64, FLOAT32, FLOAT64) compare as SB_PRED_EQ does: signedness from the physical type,
 * floats as IEEE 754 (-0.0 matches 0.0 either way round; a NaN row is in no list and so satisfies NOT_IN; a NaN literal
 * is accepted and matches nothing).  Binary / LargeBinary values compare as byte strings, as SB_PRED_EQ of
 * sb_filter_columns_var; the empty string is a literal like any other.  The literals may come in any order and repeat.
 * n_values == 0: IN selects nothing, NOT_IN every non-null row; `values` may be null then.
 * The list is searched once per run of an RLE page, per entry of a Dict page (strings included), per OneValue page and
 * per row of every other page.
 *
 * combine, `rows` / `selected`, the zero bits behind `rows` after SET, page errors (the decoder's codes, at the
 * synchronize), page_offsets, stage_capacity, replays and the rule that two columns of one call may not share a selection
 * are those of sb_filter_columns_var.  Numeric and binary columns may share a call.  `values` and `value_offsets` must
 * stay valid and unmodified until sb_ctx_synchronize: a replay reads them again.
 *
 * Refused at the call (nothing enqueued, no selection touched): Boolean / Int128 / Int256 / Null columns, SB_MEM_HOST
 * (SB_ERR_NYI); an op other than IN / NOT_IN, n_values > SB_IN_MAX_VALUES, `values` null with literal bytes to read,
 * value_offsets on a numeric column, no value_offsets on a binary column with n_values > 0, offsets that do not start
 * at 0 or that descend, more than 2^30 literal bytes, the selection refusals of sb_filter_columns (SB_ERR_INVALID); a
 * page outside [0, pages_len) (SB_ERR_IO).
 *
 * Offsets: physical_type 0, is_nullable 4, pages 8, pages_len 16, metas 24, n_pages 32, page_offsets 40, op 48,
 * combine 52, values 56, value_offsets 64, n_values 72, selection 80, selection_capacity 88, stage_capacity 96, rows 104,
 * selected 112. */
#define SB_PRED_IN 9
#define SB_PRED_NOT_IN 10
#define SB_IN_MAX_VALUES 1024u

typedef struct sb_column_filter_in {
    int32_t physical_type;   /* SB_TYPE_* */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST) */
    int32_t op;              /* SB_PRED_IN | SB_PRED_NOT_IN */
    int32_t combine;         /* SB_SEL_* */
    const uint8_t* values;   /* HOST: numbers: n_values values of the column's type, little endian, back to back;
                                binary: the literals' bytes back to back */
    const uint64_t* value_offsets; /* HOST: binary: n_values + 1 ascending offsets into `values`, [0] == 0; numbers: NULL */
    uint64_t n_values;       /* 0 .. SB_IN_MAX_VALUES */
    uint8_t* selection;      /* DEVICE: LSB-first bitmap, 4-byte aligned */
    uint64_t selection_capacity; /* >= 4*ceil(rows/32) bytes */
    uint64_t stage_capacity; /* binary columns: as in sb_column_filter_var; 0 = 4 * pages_len */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;
    uint64_t selected;
} sb_column_filter_in;       /* 120 bytes */

int32_t sb_filter_columns_in(sb_ctx* ctx, sb_column_filter_in* cols, uint64_t n, int32_t mem);

/* Column against column: `WHERE a < b`, `l_commitdate < l_receiptdate`, `end_ts >= start_ts`, `price > cost`.  The pages
 * of a primitive column y go in with a dense DEVICE array `other`: one value of `other_type` per row of the column (a
 * column decoded earlier in the interval by sb_read_columns, or any per-row expression of the engine's), optionally with
 * a validity bitmap.  Bit `row` of the result is  y[row] op other[row] ; it is combined into `selection` exactly as
 * sb_filter_columns combines its result.  Nothing of y is written, nothing of `other` is modified.
 *
 * Ops: SB_PRED_EQ .. SB_PRED_GE.  Types: y and `other` are each one of INT8..INT64, UINT8..UINT64, FLOAT32, FLOAT64,
 * chosen independently (the pairing rule of sb_aggregate_weighted):
 *   integer vs integer   both are extended by their own signedness and compared EXACTLY as mathematical integers,
 *                        whatever the widths: a negative signed value is below every unsigned value, UINT64 2^63 is
 *                        above INT64's maximum.
 *   a float on a side    both are converted to double (integers round to nearest, ties to even) and compared as IEEE
 *                        754: a NaN on either side satisfies only NE, -0.0 == +0.0, -inf and +inf are ordered like any
 *                        value.  An INT64 / UINT64 above 2^53 in magnitude is compared AFTER that rounding: 2^53 + 1
 *                        equals the double 2^53.
 * Nulls: a row satisfies nothing, NE included, when y is null at that row or bit `row` of `other_validity` is 0.
 * other_validity == NULL: every operand is valid.  Bits behind `rows` are ignored, and so is whatever the slot of an
 * invalid operand holds.
 *
 * `other`: aligned to the width of other_type, other_capacity >= rows * width bytes.  `other_validity`: 4-byte aligned,
 * LSB first as sb_read_columns writes it, other_validity_capacity >= 4*ceil(rows/32) bytes.  Both are INPUTS that must
 * stay valid and unmodified until sb_ctx_synchronize: a replay reads them again.
 *
 * `selection`, combine, `rows` / `selected`, the zero bits behind `rows` after SET, page errors (the decoder's codes, at
 * the synchronize), page_offsets and the place in the synchronize interval are those of sb_filter_columns bit for bit:
 * on a replay the call is issued again in its place and gives the same bits in all three modes; a column with a
 * primitive Freq page asks for the replay itself and is then compared from the decoded staging area.  No launch hint of
 * the read path is consulted or fed.  Per codec: plain and inflated pages load y and the operand once per row; a OneValue
 * page keeps y in a register; an RLE page hands every row its run's value; a Dict page gathers the row's entry (an index
 * beyond the dictionary raises what a read raises); bit-packed pages are unpacked in LDS.  No run and no dictionary entry
 * can be decided once any more: the cost follows the rows.
 *
 * Refused at the call (nothing enqueued, no result field and no selection byte touched): y or `other` of Boolean /
 * Int128 / Int256 / Binary / LargeBinary / Null, SB_MEM_HOST (SB_ERR_NYI); an op outside EQ .. GE, a bad combine, a
 * physical_type or other_type outside the enum, `other` null, not aligned to its width or shorter than rows * width,
 * `other_validity` misaligned or short, a validity capacity without a pointer, flags != 0, reserved != 0, a `selection`
 * that overlaps `other` or `other_validity` of its own column, two columns of one call whose selections overlap, and
 * every argument refusal of sb_filter_columns (SB_ERR_INVALID); a page outside [0, pages_len) (SB_ERR_IO; like its
 * siblings' this one refusal is also what the next sb_ctx_synchronize returns).
 *
 * Layout (pinned by tests/test_filter_cmp_host.py): sb_column_filter_cmp 136 bytes; physical_type 0, is_nullable 4,
 * pages 8, pages_len 16, metas 24, n_pages 32, page_offsets 40, op 48, combine 52, other 56, other_capacity 64,
 * other_validity 72, other_validity_capacity 80, other_type 88, flags 92, reserved 96, selection 104,
 * selection_capacity 112, rows 120, selected 128.  The first 56 bytes are sb_column_filter's. */
typedef struct sb_column_filter_cmp {
    int32_t physical_type;   /* SB_TYPE_* of y */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST) */
    int32_t op;              /* SB_PRED_EQ .. SB_PRED_GE */
    int32_t combine;         /* SB_SEL_* */
    const uint8_t* other;    /* DEVICE (input): one value of other_type per row, aligned to its width */
    uint64_t other_capacity; /* >= rows * width bytes */
    const uint8_t* other_validity; /* DEVICE (input), optional: LSB-first bitmap, 4-byte aligned */
    uint64_t other_validity_capacity; /* >= 4*ceil(rows/32) bytes when other_validity is given, else 0 */
    int32_t other_type;      /* SB_TYPE_* of `other` */
    uint32_t flags;          /* 0 */
    uint64_t reserved;       /* 0 */
    uint8_t* selection;      /* DEVICE: LSB-first bitmap, 4-byte aligned */
    uint64_t selection_capacity; /* >= 4*ceil(rows/32) bytes */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;
    uint64_t selected;
} sb_column_filter_cmp;      /* 136 bytes */

int32_t sb_filter_columns_cmp(sb_ctx* ctx, sb_column_filter_cmp* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ selected read
 * The second half of the filter: the pages of a payload column and a selection bitmap go in, the selected rows come
 * out packed.  Output row k is the column's row at the k-th set bit of `selection` below `rows`: its `values` are the
 * bytes sb_read_columns writes for that row (the slot of a null row included), its validity bit is bit k of `validity`.
 * Selection bits at positions >= rows are ignored.  Bits >= selected of the last validity word written are 0; validity
 * words behind it and `values` bytes behind values_len are not touched.
 *
 * Types: INT8..INT64, UINT8..UINT64, FLOAT32, FLOAT64.  Boolean, Int128, Int256, Binary, LargeBinary and Null:
 * SB_ERR_NYI at the call, nothing is enqueued and no buffer is touched.
 *
 * `selected` is not known at the call when the bitmap comes from a filter call of the same interval, so the output
 * capacities are checked on the device: a column whose values_capacity < selected * width or (nullable) whose
 * validity_capacity < 4*ceil(selected/32) raises SB_ERR_INVALID at the synchronize, and nothing is written outside the
 * capacities given.  rows * width and 4*ceil(rows/32) are always enough.  `selected` and `values_len` are filled in
 * even then: they say what the buffers have to hold.
 *
 * Refused at the call (SB_ERR_INVALID, nothing enqueued): a null or misaligned `selection`, selection_capacity below
 * 4*ceil(rows/32), a nullable column without `validity`, `values` / `validity` buffers of one call that overlap each
 * other or any `selection` of the call (columns may share ONE selection: that is the usual case).  SB_MEM_HOST: SB_ERR_NYI.
 *
 * Enqueued like sb_read_columns and sb_filter_columns; page errors are the decoder's, with its codes, at the
 * synchronize (a corrupt page without a selected row may or may not raise).  The call is part of its synchronize
 * interval: when the interval is issued again (sb_ctx_replays) it is issued again in its place, behind the filter calls
 * that write its bitmap, and gives the same bytes.  `selection` is an INPUT: like the pages it must stay unmodified by
 * the caller until the synchronize.  The call consults no launch hint of the read path and leaves its counters alone. */
typedef struct sb_column_read_selected {
    int32_t physical_type;   /* SB_TYPE_* */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST) */
    const uint8_t* selection;     /* DEVICE, input: LSB-first bitmap, 4-byte aligned, as the filter calls write it */
    uint64_t selection_capacity;  /* >= 4*ceil(rows/32) bytes */
    void* values;            /* DEVICE, aligned to the type's width: selected * width bytes are written */
    uint64_t values_capacity;
    uint8_t* validity;       /* DEVICE, 4-byte aligned: ceil(selected/8) bytes, written in 32-bit words; required iff is_nullable */
    uint64_t validity_capacity;
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;           /* sum of num_values */
    uint64_t selected;       /* bits set in `selection` below `rows` */
    uint64_t values_len;     /* selected * width */
} sb_column_read_selected;   /* 120 bytes */

int32_t sb_read_selected(sb_ctx* ctx, sb_column_read_selected* cols, uint64_t n, int32_t mem);

/* The same call for Binary / LargeBinary columns (Utf8 / LargeUtf8 are stored as these): a string payload column
 * behind a filter.  Output row k is the column's row at the k-th set bit of `selection` below `rows`:
 *   offsets[0] = 0 (written whenever the call is accepted, also with selected == 0);
 *   offsets[k+1] - offsets[k] is the byte length sb_read_columns gives that row — the difference of its two offsets,
 *   for a null row too, whatever the writer put there; offsets are int32 (Binary) or int64 (LargeBinary);
 *   values[offsets[k] .. offsets[k+1]) are the row's bytes, back to back;
 *   validity bit k as in sb_read_selected, the zero bits >= selected of the last word included.
 * What is written, and where:
 *   - nothing outside offsets_capacity, values_capacity and validity_capacity, ever;
 *   - nothing behind (selected+1)*sizeof(offset), values_len or 4*ceil(selected/32) in an interval that runs once;
 *   - EXCEPTION: an interval that is issued again (sb_ctx_replays) runs this call twice.  Where its bitmap is written
 *     by a filter call of the same interval, the first run goes by the bitmap of the first pass — which can have more
 *     bits set, a filter column with a primitive Freq page being left alone there — and what that run wrote INSIDE the
 *     capacities stays behind the three marks above: the second run cannot restore bytes it does not know.  Below the
 *     marks everything is the second run's.  A caller that needs the bytes behind the marks untouched hands in
 *     capacities it can afford to have written, or reads the bitmap in an interval of its own.  (sb_read_selected
 *     has the same property for values_len and its validity words.)
 *
 * Neither `selected` nor `values_len` is known at the call, so every capacity is checked on the device:
 * offsets_capacity < (selected+1)*sizeof(offset) or (nullable) validity_capacity < 4*ceil(selected/32) raises
 * SB_ERR_INVALID at the synchronize (site 500), values_capacity < values_len raises it too (site 510); a Binary column
 * whose selected bytes exceed INT32_MAX raises SB_ERR_OUT_OF_SPEC (site 511).  Nothing outside the capacities given is
 * written in any of these cases, and `selected` and `values_len` are filled in all the same: they say what to allocate.
 * Always enough: (rows+1)*sizeof(offset), 4*ceil(rows/32), and the column's values_len from sb_read_columns_sizes.
 * The value blocks of LZ4 / Zstd / Snappy pages are inflated into the context's staging area first, whatever the
 * selection: `stage_capacity` as in sb_column_filter_var (0 = 4 * pages_len).
 *
 * Refused at the call, nothing enqueued and no byte touched: a type that is not Binary / LargeBinary (numeric columns:
 * sb_read_selected on the same stream) and SB_MEM_HOST (SB_ERR_NYI); a null or misaligned `selection`, a short
 * selection_capacity, a nullable column without `validity`, `offsets` null, not aligned to its entries or smaller than
 * one entry, values_capacity > 0 with null `values`, any two of the call's `values` / `validity` / `offsets` buffers
 * that overlap each other or a selection of the call (SB_ERR_INVALID).  Columns may share ONE selection.
 *
 * Enqueued, replayed and reported like sb_read_selected: part of its synchronize interval, issued again in its place
 * when the interval is (sb_ctx_replays) and the same bytes then; it never asks for a replay itself (a Freq page of
 * strings is read as a Dict page); no launch hint consulted, the read path's counters left alone.  Page errors are the
 * decoder's; a Dict index beyond the dictionary on a SELECTED row is SB_ERR_OUT_OF_SPEC, on another row this call's
 * own kernels do not look at it (a corrupt page without a selected row may or may not raise, as in sb_read_selected).
 * The selected rows of a page that raised get the length 0. */
typedef struct sb_column_read_selected_var {
    int32_t physical_type;   /* SB_TYPE_BINARY | SB_TYPE_LARGE_BINARY */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST), as in sb_column_read */
    const uint8_t* selection;     /* DEVICE, input: as in sb_column_read_selected */
    uint64_t selection_capacity;  /* >= 4*ceil(rows/32) bytes */
    uint8_t* values;         /* DEVICE, any byte alignment: the selected rows' bytes, back to back */
    uint64_t values_capacity;
    uint8_t* validity;       /* DEVICE, 4-byte aligned: ceil(selected/8) bytes, written in 32-bit words; required iff is_nullable */
    uint64_t validity_capacity;
    void* offsets;           /* DEVICE, aligned to int32 / int64: selected + 1 offsets */
    uint64_t offsets_capacity;
    uint64_t stage_capacity; /* as in sb_column_filter_var; 0 = 4 * pages_len */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;           /* sum of num_values */
    uint64_t selected;       /* bits set in `selection` below `rows` */
    uint64_t values_len;     /* bytes of the selected rows */
} sb_column_read_selected_var;   /* 144 bytes */

int32_t sb_read_selected_var(sb_ctx* ctx, sb_column_read_selected_var* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ aggregate
 * The third thing a scan does with a block: SELECT count(y), min(y), max(y), sum(y) ... WHERE x < 5 wants no row, only a
 * few scalars per column.  The pages of a column and (optionally) a selection bitmap go in; count, min, max and sum of the
 * LIVE rows come back in the struct.  A row is live if its selection bit is set and it is not null.  Selection bits at
 * positions >= rows are ignored; `selection` == NULL selects every row; a non-nullable column has no null row; every row
 * of a SB_TYPE_NULL column is null.
 *
 * rows / selected / count / nans are always filled (SB_AGG_COUNT asks for nothing more); the other fields are written as
 * 0 where `ops` lacks their bit.
 *   MIN / MAX  over the live rows that are not NaN.  Integers compare by the physical type's signedness; floats compare
 *              numerically with -0.0 < +0.0, so the result's bits are determined.  The stored bytes are the bytes of a
 *              row that has that value, little endian, in the first `width` bytes; the bytes behind `width` are 0, and
 *              with no such row (count - nans == 0) all 8 bytes are 0.
 *   SUM        integers: the exact sum of the live rows as a 128-bit two's-complement number (values sign- or
 *              zero-extended by type; sum_hi is the high word).  Float32 / Float64: the sum of ALL live rows, NaN and
 *              +-inf included, accumulated in double: its bits in sum_lo, sum_hi = 0.  No floating-point atomics: partial
 *              sums are combined in an order fixed by the launch shape, so the same call gives the same bits every time
 *              it is issued, a replayed interval included: the order of the double additions of a column's sum is a
 *              function of the column's own page layout, data and selection alone, whatever other columns the call and
 *              other calls the interval have.  Only a column that has a primitive Freq page itself is decoded in a
 *              replayed interval, and such a column is decoded in every interval it is part of.
 *   nans       the live rows that are NaN (0 for integers, and 0 where `ops` has none of MIN / MAX / SUM: no value is
 *              looked at then).
 *
 * Types: MIN / MAX / SUM on INT8..INT64, UINT8..UINT64, FLOAT32, FLOAT64.  With `ops` of 0 or SB_AGG_COUNT alone every
 * physical type is accepted, and only the def-level section of a page is looked at, as SB_PRED_IS_NULL does it.
 *
 * Refused at the call, nothing enqueued and no result field touched: MIN / MAX / SUM on Boolean, Int128, Int256, Binary,
 * LargeBinary or Null, and SB_MEM_HOST (SB_ERR_NYI); unknown `ops` bits, `reserved` != 0, a bad physical_type, a non-null
 * `selection` that is not 4-byte aligned or shorter than 4*ceil(rows/32), `metas` null with n_pages > 0 (SB_ERR_INVALID);
 * a page outside [0, pages_len) (SB_ERR_IO).
 *
 * Enqueued like sb_read_selected: page errors are the decoder's, with its codes, at the synchronize (a corrupt page
 * without a selected row may or may not raise); `rows` and `selected` are delivered even when the interval failed, the
 * other results are unspecified then.  The call is part of its synchronize interval: when the interval is issued again
 * (sb_ctx_replays) it is issued again in its place, behind the filter calls that write its bitmap.  A column with a
 * primitive Freq page and MIN / MAX / SUM asks for that replay itself, as a filter comparison does.  `selection` is an
 * INPUT: it must stay unmodified until the synchronize.  The call consults no launch hint of the read path and leaves its
 * counters alone.
 *
 * Layout (pinned by tests/test_aggregate_host.py): 136 bytes; physical_type 0, is_nullable 4, pages 8, pages_len 16,
 * metas 24, n_pages 32, page_offsets 40, selection 48, selection_capacity 56, ops 64, reserved 68, rows 72, selected 80,
 * count 88, nans 96, min 104, max 112, sum_lo 120, sum_hi 128. */
#define SB_AGG_COUNT 1u   /* rows / selected / count / nans: always filled, this bit asks for nothing more */
#define SB_AGG_MIN   2u
#define SB_AGG_MAX   4u
#define SB_AGG_SUM   8u

typedef struct sb_column_aggregate {
    int32_t physical_type;   /* SB_TYPE_* */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST), as in sb_column_read */
    const uint8_t* selection;     /* DEVICE, input: LSB-first bitmap, 4-byte aligned; NULL = every row */
    uint64_t selection_capacity;  /* >= 4*ceil(rows/32) bytes when selection != NULL */
    uint32_t ops;            /* SB_AGG_* bits */
    uint32_t reserved;       /* must be 0 */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;           /* sum of num_values */
    uint64_t selected;       /* bits set in `selection` below `rows` (== rows without a selection) */
    uint64_t count;          /* selected rows that are not null */
    uint64_t nans;           /* of those, float NaNs */
    uint8_t min[8], max[8];  /* a value of the column's own type, little endian, in the first `width` bytes */
    uint64_t sum_lo, sum_hi;
} sb_column_aggregate;       /* 136 bytes */

int32_t sb_aggregate_columns(sb_ctx* ctx, sb_column_aggregate* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ aggregate, grouped
 * SELECT k, count(*), count(y), min(y), max(y), sum(y) ... WHERE x < 5 GROUP BY k.  sb_aggregate_columns with one more
 * input: `group_ids`, one unsigned integer of `group_id_width` bytes per row of the column, on the device.  It is a key
 * column read by sb_read_columns earlier in the interval, or ids the caller computed.  Row r belongs to group
 * group_ids[r]; every group gets a record of its own in `groups` (HOST), filled at the synchronize.
 *
 * Everything not said here is sb_aggregate_columns' word for word: live rows, NaNs, the order of min / max with
 * -0.0 < +0.0, 128-bit integer sums, float sums in double, the bytes of min / max, fields written as 0 where `ops` lacks
 * their bit, the accepted types, what a count-only column looks at.
 *   membership    a selected row whose id is >= n_groups is aggregated nowhere and counted in `out_of_range`; no error is
 *                 raised (0xFF.. can mark a null key).  Ids of unselected rows are never interpreted.
 *   counts        groups[g].selected: the selected rows of the group, null or not (count(*)); groups[g].count: the live
 *                 ones (count(y)).  The sum of groups[g].selected over g, plus out_of_range, is `selected`.
 *   empty groups  all counts 0, min / max all zero bytes, sum 0.
 *   float sums    no floating-point atomics, neither in LDS nor in HBM: the order of the double additions of a group's
 *                 sum is a function of the column's shape and data alone, so the same call gives the same bits every time
 *                 it is issued, also in an interval that is issued again on another call's account: only a column that
 *                 has a Freq page itself is decoded for the replay, and such a column is decoded in every interval.
 *
 * Refused at the call, nothing enqueued, no result field and no byte of `groups` touched: n_groups 0 or above
 * SB_AGG_MAX_GROUPS, group_id_width not 1 / 2 / 4, `group_ids` null with rows > 0 or not aligned to its width or shorter
 * than rows * group_id_width, `groups` null, and every refusal of sb_aggregate_columns with its code.
 *
 * Enqueued like sb_aggregate_columns and part of its synchronize interval in the same way: on a replay it is issued again
 * in its place, behind the filter calls that write its bitmap and the read calls that write its ids.  `selection` and
 * `group_ids` are INPUTS: they stay unmodified until the synchronize.  `rows` and `selected` are delivered even when the
 * interval failed; `groups` and `out_of_range` are unspecified then.
 *
 * Layout (pinned by tests/test_aggregate_grouped_host.py): sb_agg_group 64 bytes; selected 0, count 8, nans 16, min 24,
 * max 32, sum_lo 40, sum_hi 48, reserved 56.  sb_column_aggregate_grouped 128 bytes; physical_type 0, is_nullable 4,
 * pages 8, pages_len 16, metas 24, n_pages 32, page_offsets 40, selection 48, selection_capacity 56, group_ids 64,
 * group_ids_capacity 72, group_id_width 80, n_groups 84, ops 88, reserved 92, groups 96, rows 104, selected 112,
 * out_of_range 120. */
#define SB_AGG_MAX_GROUPS 256u

typedef struct sb_agg_group {
    uint64_t selected;       /* selected rows of this group, null or not */
    uint64_t count;          /* of those, not null */
    uint64_t nans;           /* of those, float NaNs */
    uint8_t min[8], max[8];  /* as in sb_column_aggregate */
    uint64_t sum_lo, sum_hi;
    uint64_t reserved;       /* written as 0 */
} sb_agg_group;              /* 64 bytes */

typedef struct sb_column_aggregate_grouped {
    int32_t physical_type;   /* SB_TYPE_* */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST), as in sb_column_read */
    const uint8_t* selection;     /* DEVICE, input: as in sb_column_aggregate; NULL = every row */
    uint64_t selection_capacity;
    const void* group_ids;        /* DEVICE, input: one unsigned id per row of the column, aligned to its width */
    uint64_t group_ids_capacity;  /* >= rows * group_id_width bytes */
    uint32_t group_id_width;      /* 1, 2 or 4 */
    uint32_t n_groups;            /* 1 .. SB_AGG_MAX_GROUPS (sb_aggregate_grouped), 1 .. SB_AGG_LARGE_MAX_GROUPS (sb_aggregate_grouped_large) */
    uint32_t ops;            /* SB_AGG_* bits */
    uint32_t reserved;       /* must be 0 */
    sb_agg_group* groups;    /* HOST, n_groups entries, filled at the synchronize; must live until then */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;           /* sum of num_values */
    uint64_t selected;       /* bits set in `selection` below `rows` (== rows without a selection) */
    uint64_t out_of_range;   /* selected rows whose id is >= n_groups */
} sb_column_aggregate_grouped;   /* 128 bytes */

int32_t sb_aggregate_grouped(sb_ctx* ctx, sb_column_aggregate_grouped* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ aggregate, grouped, up to 1024 groups
 * sb_aggregate_grouped for key columns of 257 .. 1024 distinct values: every id sb_key_ids / sb_key_ids_var hands out
 * (SB_KEY_MAX_KEYS) has a group here.  The same struct (sb_column_aggregate_grouped, layout unchanged), the same
 * sb_agg_group records, n_groups 1 .. SB_AGG_LARGE_MAX_GROUPS.
 *
 * Everything said for sb_aggregate_grouped holds word for word with SB_AGG_LARGE_MAX_GROUPS in the limit's place: live rows,
 * out_of_range, counts, empty groups, the order and bytes of min / max, 128-bit integer sums, float sums in double, the
 * accepted types, the count-only route on every physical type, the refusals with their codes (nothing enqueued, no result
 * field and no byte of `groups` touched), `rows` / `selected` delivered on a failed interval, membership in the
 * synchronize interval and its replays.
 *   float sums    one thing differs: the bits of a float sum are this call's own.  Its rows meet other tables in another
 *                 order than sb_aggregate_grouped's (a table lives for 16 tiles of the column, not one), so the two calls
 *                 need not give the same bits for the same input.  This call gives the same bits every time it is issued,
 *                 a replayed interval included: no floating-point atomics, and the order of the double additions of a
 *                 group's sum is a function of the column's own page layout and data alone, whatever other columns the
 *                 call has. */
#define SB_AGG_LARGE_MAX_GROUPS 1024u      /* == SB_KEY_MAX_KEYS */

int32_t sb_aggregate_grouped_large(sb_ctx* ctx, sb_column_aggregate_grouped* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ aggregate, weighted: sum(y * w) per group
 * SELECT k, count(y), sum(y * w) ... WHERE x < 5 GROUP BY k.  sb_aggregate_grouped_large with one more dense per-row
 * input beside `group_ids`: `weights` (DEVICE), one value of `weight_type` per row of the column -- a column that
 * sb_read_columns decoded earlier in the interval, or any per-row expression the caller computed.  With SB_WGT_SQUARE the
 * weight of a row is its own y: the sum of squares.  The results are sb_agg_group records, index-aligned with those of the
 * grouped calls: min / max are written as zero bytes, sum_lo / sum_hi hold the sum of products, nans counts NaN products.
 *
 *   operands      y from the pages and w from `weights`, each of INT8..INT64, UINT8..UINT64, FLOAT32, FLOAT64,
 *                 independently chosen.  `weights`: aligned to the type's width, weights_capacity >= rows * width.
 *                 `weights_validity` (optional, DEVICE): an LSB-first bitmap as sb_read_columns writes it, 4-byte aligned,
 *                 >= 4*ceil(rows/32) bytes; NULL: every weight is valid.  Bits behind `rows` are ignored.
 *   SB_WGT_SQUARE weights, weights_validity and their capacities must be NULL / 0 and weight_type 0.
 *   groups        group_ids / group_id_width / n_groups as for sb_aggregate_grouped_large, n_groups 1 .. 1024.  group_ids
 *                 NULL is allowed only with n_groups == 1, group_id_width == 0 and group_ids_capacity == 0: every selected
 *                 row is in group 0 (the ungrouped case).
 *   live rows     selected, id < n_groups, y not null, weight valid.  Weights, validity bits and ids of unselected rows
 *                 are never loaded.  groups[g].selected: the group's selected rows; groups[g].count: its live rows; the
 *                 sum of groups[g].selected over g, plus out_of_range, is `selected`.
 *   ops           SB_AGG_COUNT and SB_AGG_SUM; MIN / MAX are refused (SB_ERR_INVALID).  Without SUM only def levels, ids
 *                 and weight validity are read, sum / nans are 0, every physical type is accepted.
 *   int x int     both operands extended by their own signedness, multiplied exactly; the group's sum is the true sum
 *                 modulo 2^128 (two's complement in sum_lo / sum_hi), the same in any order.  nans 0.
 *   otherwise     the product is (double)y * (double)w (integer to double: round to nearest), summed in double over all
 *                 live rows, NaN and +-inf included; the bits in sum_lo, sum_hi 0; nans: live rows whose product is NaN.
 *                 No floating-point atomics: the order of a group's additions is a function of the column's own page
 *                 layout, data, ids and selection alone, a replayed interval included.  The bits are this call's own.
 *
 * Refused at the call, nothing enqueued, no result field and no byte of `groups` touched: SB_ERR_NYI for SUM on Boolean /
 * Int128 / Int256 / Binary / LargeBinary / Null and for SB_MEM_HOST; SB_ERR_INVALID for a bad weight_type, null,
 * misaligned or short weights, misaligned or short weights_validity, an inconsistent SB_WGT_SQUARE or ungrouped form,
 * unknown flags, reserved != 0, n_groups 0 or above 1024, and every argument refusal of sb_aggregate_grouped; SB_ERR_IO for
 * a page outside [0, pages_len).
 *
 * Enqueued like sb_aggregate_grouped; `selection`, `group_ids`, `weights` and `weights_validity` are INPUTS that stay
 * unmodified until the synchronize.  `rows` and `selected` are delivered even when the interval failed.
 *
 * Layout (pinned by tests/test_aggregate_weighted_host.py): 168 bytes; the first 92 bytes are sb_column_aggregate_grouped's,
 * then flags 92, weights 96, weights_capacity 104, weights_validity 112, weights_validity_capacity 120, weight_type 128,
 * reserved 132, groups 136, rows 144, selected 152, out_of_range 160. */
#define SB_WGT_SQUARE 1u   /* flags bit 0: the weight of a row is its own y */

typedef struct sb_column_aggregate_weighted {
    int32_t physical_type;   /* SB_TYPE_* */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST), as in sb_column_read */
    const uint8_t* selection;     /* DEVICE, input; NULL = every row */
    uint64_t selection_capacity;
    const void* group_ids;        /* DEVICE, input; NULL: the ungrouped form (n_groups 1, width and capacity 0) */
    uint64_t group_ids_capacity;
    uint32_t group_id_width;      /* 1, 2 or 4 (0 in the ungrouped form) */
    uint32_t n_groups;            /* 1 .. SB_AGG_LARGE_MAX_GROUPS */
    uint32_t ops;                 /* SB_AGG_COUNT | SB_AGG_SUM */
    uint32_t flags;               /* SB_WGT_* bits */
    const void* weights;          /* DEVICE, input: one value of weight_type per row, aligned to its width */
    uint64_t weights_capacity;    /* >= rows * width bytes */
    const uint8_t* weights_validity;     /* DEVICE, input, optional: LSB-first bitmap, 4-byte aligned */
    uint64_t weights_validity_capacity;  /* >= 4*ceil(rows/32) bytes */
    int32_t weight_type;          /* SB_TYPE_* of `weights` (0 with SB_WGT_SQUARE) */
    uint32_t reserved;            /* must be 0 */
    sb_agg_group* groups;         /* HOST, n_groups entries, filled at the synchronize; must live until then */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;
    uint64_t selected;
    uint64_t out_of_range;
} sb_column_aggregate_weighted;   /* 168 bytes */

int32_t sb_aggregate_weighted(sb_ctx* ctx, sb_column_aggregate_weighted* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ top-k
 * SELECT ... WHERE x < 5 ORDER BY y [DESC] LIMIT k.  The pages of a column and (optionally) a selection bitmap go in; the
 * k best of the selected rows come back in `out` (HOST) with their row numbers, with which sb_read_selected fetches the
 * other columns of the winners.  No selected value is stored on the way.
 *
 *   live rows     a row is live if its selection bit is set and it is not null, exactly as for sb_aggregate_columns;
 *                 rows / selected / count / nans mean what they mean there.
 *   candidates    the live rows that are not NaN.  found = min(k, count - nans).
 *   order         by value in the aggregate's order: integers by the physical type's signedness; floats numerically with
 *                 -0.0 < +0.0, +-inf included.  Ascending for SB_TOPK_SMALLEST, descending for SB_TOPK_LARGEST.  TIES ARE
 *                 BROKEN BY THE LOWER ROW NUMBER, IN BOTH ORDERS.  That is a total order on (value, row), so the result
 *                 is unique: the same bytes every time the call is issued, a replayed interval included, whatever the
 *                 schedule.
 *   out           out[0 .. found) holds the winners in that order: `row` is the row's number in the column, `value` the
 *                 bytes of that row's value, little endian, in the first `width` bytes, and 0 behind them.
 *                 out[found .. k) is written as all zero.  No byte behind out[k) is touched.
 *
 * Types: INT8..INT64, UINT8..UINT64, FLOAT32, FLOAT64.
 *
 * Refused at the call, nothing enqueued and no result field or byte of `out` touched: another physical type and
 * SB_MEM_HOST (SB_ERR_NYI); k of 0 or above SB_TOPK_MAX_K, an unknown `order`, `reserved` != 0, `out` null, and every
 * argument refusal of sb_aggregate_columns, with its code.
 *
 * Enqueued like sb_aggregate_columns and part of its synchronize interval in the same way: on a replay it is issued again
 * in its place, behind the filter calls that write its bitmap.  A column with a primitive Freq page asks for that replay
 * itself.  `selection` is an INPUT: it stays unmodified until the synchronize.  `rows` and `selected` are delivered even
 * when the interval failed; the other results and `out` are unspecified then.  The call consults no launch hint of the read
 * path and leaves its counters alone.
 *
 * Layout (pinned by tests/test_topk_host.py): sb_topk_row 16 bytes; row 0, value 8.  sb_column_topk 128 bytes;
 * physical_type 0, is_nullable 4, pages 8, pages_len 16, metas 24, n_pages 32, page_offsets 40, selection 48,
 * selection_capacity 56, k 64, order 68, out 72, reserved 80, rows 88, selected 96, count 104, nans 112, found 120. */
#define SB_TOPK_MAX_K 256u
#define SB_TOPK_SMALLEST 0u
#define SB_TOPK_LARGEST  1u

typedef struct sb_topk_row {
    uint64_t row;            /* the row's number in the column */
    uint8_t value[8];        /* as min / max in sb_column_aggregate */
} sb_topk_row;               /* 16 bytes */

typedef struct sb_column_topk {
    int32_t physical_type;   /* SB_TYPE_* */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST), as in sb_column_read */
    const uint8_t* selection;     /* DEVICE, input: as in sb_column_aggregate; NULL = every row */
    uint64_t selection_capacity;
    uint32_t k;              /* 1 .. SB_TOPK_MAX_K */
    uint32_t order;          /* SB_TOPK_SMALLEST / SB_TOPK_LARGEST */
    sb_topk_row* out;        /* HOST, k entries, filled at the synchronize; must live until then */
    uint64_t reserved;       /* must be 0 */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;           /* sum of num_values */
    uint64_t selected;       /* bits set in `selection` below `rows` (== rows without a selection) */
    uint64_t count;          /* selected rows that are not null */
    uint64_t nans;           /* of those, float NaNs */
    uint64_t found;          /* min(k, count - nans): the entries of `out` that hold a row */
} sb_column_topk;            /* 128 bytes */

int32_t sb_topk_columns(sb_ctx* ctx, sb_column_topk* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ key ids
 * SELECT ... GROUP BY k / SELECT DISTINCT k WHERE ...  The pages of an INTEGER key column and (optionally) a selection
 * bitmap go in; the distinct values of the live rows come back in `keys` (HOST), and every row of the column gets a dense
 * id in `ids` (DEVICE): the link between sb_filter_columns* and sb_aggregate_grouped, whose group ids these are.
 *
 *   live rows     a row is live if its selection bit is set and it is not null, exactly as for sb_aggregate_columns;
 *                 rows / selected / count mean what they mean there.
 *   keys          the distinct values of the live rows, ascending by the physical type's signedness; n_keys of them.  Key i
 *                 is written like sb_topk_row.value: the value's bytes, little endian, in the first `width` bytes of the
 *                 8-byte slot keys[8 * i ..], and 0 behind them.  keys[n_keys .. max_keys) is written as zero.
 *   ids           one unsigned integer of id_width bytes per row of the column, all `rows` of them written: the position
 *                 of the row's value in `keys`, or all ones (SB_KEY_ID_NONE truncated to id_width) for a row that is not
 *                 live.  The sorted order makes the ids a function of the data alone: the same bytes every time the call
 *                 is issued, a replayed interval included, whatever the schedule.  Handed to sb_aggregate_grouped
 *                 unchanged (group_id_width = id_width, n_groups >= n_keys), its out_of_range counts the selected rows
 *                 that are null.
 *   max_keys      1 .. min(SB_KEY_MAX_KEYS, 2^(8 * id_width) - 1): with id_width 1 at most 255, so that all ones is no id.
 *   overflow      the live rows have more than max_keys distinct values: overflow = 1 and the synchronize still returns
 *                 SB_OK (an engine probes a column's cardinality this way and falls back); n_keys, `keys` and `ids` are
 *                 unspecified then.  Otherwise 0.  Either way no byte behind keys[max_keys) or behind ids_capacity is
 *                 touched.
 *
 * Types: INT8..INT64, UINT8..UINT64.
 *
 * Refused at the call, nothing enqueued and no result field, byte of `keys` or byte of `ids` touched: Float32 / Float64
 * (NaN and +-0 need a grouping rule of their own), Boolean, Int128 / Int256, Binary / LargeBinary, Null and SB_MEM_HOST
 * (SB_ERR_NYI); id_width not 1 / 2 / 4, max_keys 0 or above its limit, `ids` null with rows > 0, misaligned or smaller
 * than rows * id_width, `keys` null, `reserved` != 0, two columns of one call whose `ids` overlap (SB_ERR_INVALID), and
 * every argument refusal of sb_aggregate_columns, with its code.
 *
 * Enqueued like sb_aggregate_columns and part of its synchronize interval in the same way: on a replay it is issued again
 * in its place, behind the filter calls that write its bitmap and in front of the sb_aggregate_grouped calls that read its
 * ids.  A column with a primitive Freq page asks for that replay itself.  `selection` is an INPUT: it stays unmodified
 * until the synchronize.  Page errors are the decoder's, with its codes, at the synchronize; `rows` and `selected` are
 * delivered even when the interval failed, the other results, `keys` and `ids` are unspecified then.  The call consults no
 * launch hint of the read path and leaves its counters alone.
 *
 * Layout (pinned by tests/test_key_ids_host.py): sb_column_key_ids 144 bytes; physical_type 0, is_nullable 4, pages 8,
 * pages_len 16, metas 24, n_pages 32, page_offsets 40, selection 48, selection_capacity 56, ids 64, ids_capacity 72,
 * id_width 80, max_keys 84, keys 88, reserved 96, rows 104, selected 112, count 120, n_keys 128, overflow 136. */
#define SB_KEY_MAX_KEYS 1024u
#define SB_KEY_ID_NONE 0xFFFFFFFFu

typedef struct sb_column_key_ids {
    int32_t physical_type;   /* SB_TYPE_* */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST), as in sb_column_read */
    const uint8_t* selection;     /* DEVICE, input: as in sb_column_aggregate; NULL = every row */
    uint64_t selection_capacity;
    void* ids;               /* DEVICE, output: one id per row, aligned to id_width */
    uint64_t ids_capacity;   /* >= rows * id_width bytes */
    uint32_t id_width;       /* 1, 2 or 4 */
    uint32_t max_keys;       /* 1 .. min(SB_KEY_MAX_KEYS, 2^(8 * id_width) - 1) */
    uint8_t* keys;           /* HOST, 8 * max_keys bytes, filled at the synchronize; must live until then */
    uint64_t reserved;       /* must be 0 */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;           /* sum of num_values */
    uint64_t selected;       /* bits set in `selection` below `rows` (== rows without a selection) */
    uint64_t count;          /* selected rows that are not null */
    uint64_t n_keys;         /* distinct values among them */
    uint64_t overflow;       /* 1: more than max_keys of them; n_keys, keys and ids are unspecified */
} sb_column_key_ids;         /* 144 bytes */

int32_t sb_key_ids(sb_ctx* ctx, sb_column_key_ids* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ key ids of Binary / Utf8 columns
 * sb_key_ids for SB_TYPE_BINARY / SB_TYPE_LARGE_BINARY key columns: GROUP BY country / status / host, SELECT DISTINCT of
 * a string column.  Live rows, rows / selected / count, `ids`, id_width, max_keys, the enqueueing, replays and page
 * errors are those of sb_key_ids; what differs is how the keys come back.
 *
 *   keys          the distinct byte strings of the live rows, n_keys of them.  Distinct as byte strings, whatever their
 *                 hashes; ascending in the order of SB_PRED_LT of sb_filter_columns_var: bytes compare unsigned, a proper
 *                 prefix is less than the longer string.  The empty string is a key like any other; a null row gives no
 *                 key, whatever bytes the writer left in it.
 *   key_offsets   HOST, max_keys + 1 entries, filled at the synchronize: key_offsets[0] == 0, key i is
 *                 keys[key_offsets[i] .. key_offsets[i + 1]), the entries behind n_keys repeat keys_len.
 *   keys          HOST, keys_capacity bytes (at most SB_KEY_VAR_MAX_BYTES): the keys' bytes back to back, and zero in
 *                 [keys_len, keys_capacity).  key_offsets / keys are the value_offsets / values of sb_column_filter_in:
 *                 a semi-join hands both over unchanged.
 *   overflow      a bit set; the synchronize returns SB_OK either way.
 *                 SB_KEY_OVERFLOW_KEYS: more than max_keys distinct live strings; n_keys, keys_len, key_offsets, `keys`
 *                 and `ids` are unspecified.
 *                 SB_KEY_OVERFLOW_BYTES: the keys fit max_keys but their bytes exceed keys_capacity: n_keys, keys_len,
 *                 key_offsets and `ids` are valid, only the bytes of `keys` are not delivered (they are written as
 *                 zero); keys_len says what to allocate.
 *                 In no case is a byte written outside ids_capacity, key_offsets[0 .. max_keys] and keys[0 .. keys_capacity).
 *   stage_capacity  as in sb_column_filter_var: the column's share of the staging area for LZ4 / Zstd / Snappy value
 *                 blocks; 0 = 4 * pages_len.
 *
 * A Dict / Freq page costs one insertion and one search per dictionary entry that a live row points at (an entry no
 * live row points at is no key), a OneValue page one per tile, a Basic page one per live row.  A Dict index beyond the
 * dictionary on a live row is SB_ERR_OUT_OF_SPEC; offsets that leave a values block are cut to it.  The call never asks
 * for a replay itself (a Freq page of strings is a virtual Dict page) and consults no launch hint.
 *
 * Refused at the call, nothing enqueued and no result field or output byte touched: every refusal of sb_key_ids with
 * its code (`keys` null is refused only with keys_capacity > 0); a type that is not Binary / LargeBinary and SB_MEM_HOST
 * (SB_ERR_NYI); key_offsets null, keys_capacity above SB_KEY_VAR_MAX_BYTES (SB_ERR_INVALID); a call of 2^28 pages or
 * more, a page of more than 2^26 rows or of 2^29 bytes or more (SB_ERR_NYI: page and row / entry number are fields of
 * the 64-bit word a slot of the distinct set holds).
 *
 * Layout (pinned by tests/test_key_ids_var_host.py): sb_column_key_ids_var 176 bytes; physical_type 0, is_nullable 4,
 * pages 8, pages_len 16, metas 24, n_pages 32, page_offsets 40, selection 48, selection_capacity 56, ids 64,
 * ids_capacity 72, id_width 80, max_keys 84, key_offsets 88, keys 96, keys_capacity 104, stage_capacity 112,
 * reserved 120, rows 128, selected 136, count 144, n_keys 152, keys_len 160, overflow 168. */
#define SB_KEY_VAR_MAX_BYTES (1u << 20)
#define SB_KEY_OVERFLOW_KEYS 1u
#define SB_KEY_OVERFLOW_BYTES 2u

typedef struct sb_column_key_ids_var {
    int32_t physical_type;   /* SB_TYPE_BINARY | SB_TYPE_LARGE_BINARY */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST), as in sb_column_read */
    const uint8_t* selection;     /* DEVICE, input: as in sb_column_aggregate; NULL = every row */
    uint64_t selection_capacity;
    void* ids;               /* DEVICE, output: one id per row, aligned to id_width */
    uint64_t ids_capacity;   /* >= rows * id_width bytes */
    uint32_t id_width;       /* 1, 2 or 4 */
    uint32_t max_keys;       /* 1 .. min(SB_KEY_MAX_KEYS, 2^(8 * id_width) - 1) */
    uint64_t* key_offsets;   /* HOST, max_keys + 1 entries, filled at the synchronize; must live until then */
    uint8_t* keys;           /* HOST, keys_capacity bytes, likewise */
    uint64_t keys_capacity;  /* 0 .. SB_KEY_VAR_MAX_BYTES */
    uint64_t stage_capacity; /* see above; 0 = 4 * pages_len */
    uint64_t reserved;       /* must be 0 */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;           /* sum of num_values */
    uint64_t selected;       /* bits set in `selection` below `rows` (== rows without a selection) */
    uint64_t count;          /* selected rows that are not null */
    uint64_t n_keys;         /* distinct strings among them */
    uint64_t keys_len;       /* their bytes together */
    uint64_t overflow;       /* SB_KEY_OVERFLOW_* bits */
} sb_column_key_ids_var;     /* 176 bytes */

int32_t sb_key_ids_var(sb_ctx* ctx, sb_column_key_ids_var* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ ids of composite keys
 * SELECT ... GROUP BY a, b / SELECT DISTINCT a, b.  Every key column goes through sb_key_ids / sb_key_ids_var first; the
 * 2 .. 4 id arrays they wrote (DEVICE) go in here, and one call turns them into the sorted distinct tuples of part ids
 * (`tuples`, HOST) and a dense tuple id per row (`ids`, DEVICE), which sb_aggregate_grouped / _large take as group ids.
 * No page is read and the call takes no selection: the part ids carry it.
 *
 *   parts         part p is part_ids[p]: `rows` unsigned integers of part_width[p] bytes, inside part_capacity[p] bytes.
 *                 part_keys[p] (1 .. SB_KEY_MAX_KEYS) is the exclusive bound of a valid id of that part: the max_keys of
 *                 the call that wrote it, since its n_keys is not known before the synchronize.  The fields of the parts
 *                 at and behind n_parts are ignored.
 *   live rows     a row is live if every part id is below its part's bound.  All ones — what sb_key_ids* write for a row
 *                 that is not selected or null — is therefore not live, and neither is any other id at or above the bound;
 *                 no error is raised for one.  `live` counts the live rows.  A row with a null in any key column has no
 *                 tuple: under sb_aggregate_grouped it ends in out_of_range, as with a single key.
 *   tuples        the distinct tuples of the live rows, n_keys of them, ascending lexicographically by part id with part 0
 *                 most significant; the part ids of sb_key_ids* preserve the order of the key values, so this is the order
 *                 of the key values too.  Tuple i is tuples[4 * i .. 4 * i + 4), the parts at and behind n_parts written
 *                 as 0; tuples[4 * n_keys .. 4 * max_keys) is written as 0.
 *   ids           one unsigned integer of id_width bytes per row, all `rows` of them written: the position of the row's
 *                 tuple in `tuples`, or all ones (SB_KEY_ID_NONE truncated to id_width) for a row that is not live.  A
 *                 function of the data alone: the same bytes whatever the schedule, a replayed interval included.
 *   max_keys      1 .. min(SB_KEY_MAX_KEYS, 2^(8 * id_width) - 1), as in sb_key_ids.
 *   overflow      more than max_keys distinct tuples: overflow = 1 and the synchronize still returns SB_OK; n_keys,
 *                 `tuples` and `ids` are unspecified then.  Otherwise 0.  Either way nothing is written outside
 *                 tuples[0 .. 4 * max_keys) and ids_capacity.
 *   rows == 0     is valid: live and n_keys are 0.
 *
 * Whatever bits the part arrays hold (the ids of a part that itself overflowed are unspecified), no access leaves
 * rows * part_width[p] bytes of a part, rows * id_width bytes of `ids` or the call's workspace: an id is compared with its
 * bound before anything else is done with it, and it is never an index.
 *
 * Refused at the call, nothing enqueued and no result field or output byte touched: SB_MEM_HOST and more than 65535 items
 * (SB_ERR_NYI); n_parts outside 2 .. 4, a part_width or id_width that is not 1 / 2 / 4, part_keys[p] 0 or above
 * SB_KEY_MAX_KEYS, a part pointer or `ids` that is null with rows > 0, misaligned to its width or shorter than
 * rows * width bytes, max_keys 0 or above its limit, `tuples` null, `reserved` != 0, `ids` overlapping any part of any
 * item of the call, the `ids` of two items overlapping (SB_ERR_INVALID).  The part arrays are INPUTS: they stay
 * unmodified until the synchronize.
 *
 * Part of the synchronize interval like sb_key_ids: on a replay it is issued again in its place, behind the sb_key_ids*
 * calls that write its parts and in front of the grouped aggregates that read its ids.  It never asks for a replay itself,
 * consults no launch hint of the read path and leaves its counters alone.  On a failed interval its results are
 * unspecified.
 *
 * Layout (pinned by tests/test_key_combine_host.py): sb_key_combine_item 168 bytes; rows 0, n_parts 8, id_width 12,
 * part_ids 16, part_capacity 48, part_width 80, part_keys 96, ids 112, ids_capacity 120, max_keys 128, reserved 132,
 * tuples 136, live 144, n_keys 152, overflow 160. */
#define SB_KEY_COMBINE_MAX_PARTS 4u

typedef struct sb_key_combine_item {
    uint64_t rows;
    uint32_t n_parts;        /* 2 .. SB_KEY_COMBINE_MAX_PARTS */
    uint32_t id_width;       /* of `ids`: 1, 2 or 4 */
    const void* part_ids[SB_KEY_COMBINE_MAX_PARTS];   /* DEVICE, input: one id per row, aligned to part_width[p] */
    uint64_t part_capacity[SB_KEY_COMBINE_MAX_PARTS]; /* >= rows * part_width[p] bytes */
    uint32_t part_width[SB_KEY_COMBINE_MAX_PARTS];    /* 1, 2 or 4 */
    uint32_t part_keys[SB_KEY_COMBINE_MAX_PARTS];     /* 1 .. SB_KEY_MAX_KEYS: ids at or above it are not live */
    void* ids;               /* DEVICE, output: one id per row, aligned to id_width */
    uint64_t ids_capacity;   /* >= rows * id_width bytes */
    uint32_t max_keys;       /* 1 .. min(SB_KEY_MAX_KEYS, 2^(8 * id_width) - 1) */
    uint32_t reserved;       /* must be 0 */
    uint32_t* tuples;        /* HOST, 4 * max_keys entries, filled at the synchronize; must live until then */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t live;           /* rows whose part ids are all below their bounds */
    uint64_t n_keys;         /* distinct tuples among them */
    uint64_t overflow;       /* 1: more than max_keys of them; n_keys, tuples and ids are unspecified */
} sb_key_combine_item;       /* 168 bytes */

int32_t sb_key_combine(sb_ctx* ctx, sb_key_combine_item* items, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ ids of a key column's rows against a given list
 * fact.fk = dim.pk with a small dimension; GROUP BY over a key set that is known (the dates of a month, status codes, the
 * keys of the previous batch); ids that mean the same in every call, so that the grouped results of two row groups, two
 * files or two ranks are index-aligned and can be added.  The pages of a key column, (optionally) a selection bitmap and a
 * list of up to SB_KEY_MAX_KEYS values on the HOST go in; every row gets the id the list assigns to its value.  Nothing is
 * discovered: one walk over the pages, no table, no sort.
 *
 *   live rows     a row is live if its selection bit is set and it is not null, exactly as for sb_key_ids; rows /
 *                 selected / count mean what they mean there.
 *   ids           one unsigned integer of id_width bytes per row of the column, all `rows` of them written.  A live row
 *                 whose value equals values[i] gets value_ids[i], or i when value_ids is null.  Every other row gets all
 *                 ones (SB_KEY_ID_NONE truncated to id_width): a row that is not selected, a null row (whatever bytes the
 *                 page stores for it), and a live row whose value is not in the list.  Handed to sb_aggregate_grouped /
 *                 sb_aggregate_grouped_large unchanged, the rows without an id end in out_of_range: inner-join semantics.
 *   matched       the live rows that got an id; count - matched are the live rows the list does not know.
 *   the list      in any order.  Numeric columns: n_values values of the column's width back to back in `values`,
 *                 value_offsets null.  Binary columns: value i is values[value_offsets[i] .. value_offsets[i + 1]), exactly
 *                 the fields of sb_column_filter_in.  A value that repeats takes the id of its first occurrence.  Several
 *                 values may carry the same value_ids[i] (nation -> region: the ids are group ids directly).  Every id the
 *                 list can hand out is below all ones of id_width: each value_ids[i], or n_values - 1 without value_ids.
 *                 n_values == 0 is valid: every id is all ones and matched is 0.
 *   comparison    integers by value with the type's signedness; binary values as byte strings, exactly as SB_PRED_EQ of
 *                 sb_filter_columns_var: the empty string is a value, a trailing zero byte makes a different string.  A
 *                 value between two entries of the list, below the first or above the last has no id.
 *   determinism   the ids are a function of the pages, the selection and the list alone: the same bytes every time the
 *                 call is issued, a replayed interval included; count and matched are sums of integers.
 *   cost          one search per run of an RLE page and one per dictionary entry of a Dict / Freq page (strings too,
 *                 through the page's id table), one per OneValue tile, one per row elsewhere.  A tile of 4096 rows without
 *                 a selected row loads no value.
 *
 * Types: INT8..INT64, UINT8..UINT64, BINARY, LARGE_BINARY; the columns of a call may mix them, each with its own id_width.
 *
 * Refused at the call, nothing enqueued and no result field or byte of `ids` touched: Float32 / Float64, Boolean, Int128 /
 * Int256, Null and SB_MEM_HOST (SB_ERR_NYI); id_width not 1 / 2 / 4, `ids` null with rows > 0, misaligned or smaller than
 * rows * id_width, reserved0 or reserved != 0, two columns of one call whose `ids` overlap, n_values above
 * SB_KEY_MAX_KEYS, an id that is all ones of id_width or does not fit it (SB_ERR_INVALID); the values / value_offsets
 * refusals of sb_filter_columns_in and every argument refusal of sb_aggregate_columns, with their codes; for binary
 * columns the page and row limits of sb_key_ids_var (SB_ERR_NYI).
 *
 * Enqueued like sb_key_ids and part of its synchronize interval in the same way, as a call of its own kind: on a replay it
 * is issued again in its place, behind the filter calls that write its bitmap and in front of the sb_key_combine and
 * aggregate calls that read its ids.  A numeric column with a Freq page asks for that replay itself and is then served
 * from the decoded column; a binary Freq page is a virtual Dict page.  `selection`, `values`, `value_offsets` and
 * `value_ids` are INPUTS: they stay valid and unmodified until the synchronize.  Page errors are the decoder's, with its
 * codes, at the synchronize; `rows` and `selected` are delivered even when the interval failed, the other results and
 * `ids` are unspecified then.  The call consults no launch hint of the read path and leaves its counters alone.
 *
 * Layout (pinned by tests/test_key_lookup_host.py): sb_column_key_lookup 168 bytes; physical_type 0, is_nullable 4,
 * pages 8, pages_len 16, metas 24, n_pages 32, page_offsets 40, selection 48, selection_capacity 56, ids 64,
 * ids_capacity 72, id_width 80, reserved0 84, values 88, value_offsets 96, value_ids 104, n_values 112,
 * stage_capacity 120, reserved 128, rows 136, selected 144, count 152, matched 160. */
typedef struct sb_column_key_lookup {
    int32_t physical_type;   /* INT8..INT64, UINT8..UINT64, BINARY, LARGE_BINARY */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST), as in sb_column_read */
    const uint8_t* selection;     /* DEVICE, input: as in sb_column_key_ids; NULL = every row */
    uint64_t selection_capacity;
    void* ids;               /* DEVICE, output: one id per row, aligned to id_width */
    uint64_t ids_capacity;   /* >= rows * id_width bytes */
    uint32_t id_width;       /* 1, 2 or 4 */
    uint32_t reserved0;      /* must be 0 */
    const uint8_t* values;         /* HOST: exactly sb_column_filter_in.values */
    const uint64_t* value_offsets; /* HOST: binary columns only, exactly sb_column_filter_in.value_offsets */
    const uint32_t* value_ids;     /* HOST, optional: n_values ids; NULL = the value's position in the list */
    uint64_t n_values;       /* 0 .. SB_KEY_MAX_KEYS */
    uint64_t stage_capacity; /* binary columns: as in sb_column_filter_var; 0 = 4 * pages_len */
    uint64_t reserved;       /* must be 0 */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;           /* sum of num_values */
    uint64_t selected;       /* bits set in `selection` below `rows` (== rows without a selection) */
    uint64_t count;          /* selected rows that are not null */
    uint64_t matched;        /* ... whose value is in the list */
} sb_column_key_lookup;      /* 168 bytes */

int32_t sb_key_lookup(sb_ctx* ctx, sb_column_key_lookup* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ range-bucket ids of a numeric key column
 * GROUP BY date_trunc('month', d) over a Date32 or timestamp column; price, age or latency bands (CASE WHEN x < 10 ..,
 * width_bucket); histograms; any GROUP BY over a Float32 / Float64 column.  The key calls above are equality; here a row's
 * id says WHERE its value falls.  The pages of a numeric key column, (optionally) a selection bitmap and up to
 * SB_BUCKET_MAX_BOUNDS bounds on the HOST go in; every row gets the id of its bucket.  One walk over the pages, the walk of
 * sb_key_lookup with the lower bound kept.
 *
 *   live rows     a row is live if its selection bit is set and it is not null, exactly as for sb_key_lookup; rows /
 *                 selected / count mean what they mean there.  All `rows` ids are written.
 *   bounds        n_bounds (0 .. SB_BUCKET_MAX_BOUNDS) values of the column's width back to back, strictly increasing under
 *                 the column's comparison: integers by value with the type's signedness, floats by IEEE value with
 *                 -0.0 == +0.0 (so { -0.0, +0.0 } is not increasing).  -inf and +inf are bounds like any other; a NaN
 *                 bound is refused.
 *   bucket of x   b(x) = the number of bounds <= x: bucket 0 is below bounds[0], bucket i is [bounds[i - 1], bounds[i]),
 *                 bucket n_bounds is [bounds[n_bounds - 1], ..).  With SB_BUCKET_RIGHT_CLOSED in `flags`, b(x) = the number
 *                 of bounds < x: bucket i is (bounds[i - 1], bounds[i]].  n_bounds == 0: every value is in bucket 0.
 *   ids           a live row that is not a NaN gets bucket_ids[b(x)], or b(x) when bucket_ids is null.  bucket_ids has
 *                 n_bounds + 1 entries; several buckets may share an id; an entry equal to SB_KEY_ID_NONE means "no id"
 *                 (to drop the open-ended buckets, for instance); every other entry is below all ones of id_width, and so
 *                 is n_bounds when bucket_ids is null.
 *   NaN           a live NaN of either sign and any payload gets nan_id truncated to id_width; nan_id == SB_KEY_ID_NONE
 *                 means all ones, any other nan_id is below all ones of id_width.  For integer columns nan_id must be
 *                 SB_KEY_ID_NONE.  Every live NaN is counted in `nans`.
 *   other rows    a row that is not selected, a null row (whatever bytes the page stores for it) and a live row whose
 *                 bucket is mapped to "no id" get all ones of id_width.
 *   matched       the live rows whose id is not all ones; a NaN row with a real nan_id counts.
 *   determinism   the ids are a function of the pages, the selection and the struct alone: the same bytes every time the
 *                 call is issued, a replayed interval included; count, matched and nans are sums of integers.
 *   cost          one search per run of an RLE page, one per dictionary entry of a Dict page, one per OneValue tile, one
 *                 per row elsewhere.  A tile of 4096 rows without a selected row loads no value.
 *
 * Types: INT8..INT64, UINT8..UINT64, FLOAT32, FLOAT64; the columns of a call may mix them, each with its own id_width.
 *
 * Refused at the call, nothing enqueued and no result field or byte of `ids` touched: Binary, Boolean, Int128 / Int256,
 * Null and SB_MEM_HOST (SB_ERR_NYI); id_width not 1 / 2 / 4, `ids` null with rows > 0, misaligned or smaller than
 * rows * id_width, reserved0 or reserved != 0, two columns of one call whose `ids` overlap, an unknown flags bit, n_bounds
 * above SB_BUCKET_MAX_BOUNDS, bounds null with n_bounds > 0, bounds that are not strictly increasing or hold a NaN, an id
 * that does not fit id_width, nan_id set on an integer column (SB_ERR_INVALID); every argument refusal of
 * sb_aggregate_columns, with its code.
 *
 * Enqueued like sb_key_lookup and part of its synchronize interval in the same way, as a call of its own kind: on a replay
 * it is issued again in its place.  A column with a Freq page asks for that replay itself and is then served from the
 * decoded column.  `selection`, `bounds` and `bucket_ids` are INPUTS: they stay valid and unmodified until the
 * synchronize.  Page errors are the decoder's, with its codes, at the synchronize (a Float32 Patas page among them, as for
 * sb_read_columns); `rows` and `selected` are delivered even when the interval failed, the other results and `ids` are
 * unspecified then.  The call consults no launch hint of the read path and leaves its counters alone.
 *
 * Layout (pinned by tests/test_key_buckets_host.py): sb_column_key_buckets 168 bytes; physical_type 0, is_nullable 4,
 * pages 8, pages_len 16, metas 24, n_pages 32, page_offsets 40, selection 48, selection_capacity 56, ids 64,
 * ids_capacity 72, id_width 80, flags 84, bounds 88, bucket_ids 96, n_bounds 104, nan_id 112, reserved0 116,
 * reserved 120, rows 128, selected 136, count 144, matched 152, nans 160. */
#define SB_BUCKET_MAX_BOUNDS 1023u    /* 1024 buckets == SB_AGG_LARGE_MAX_GROUPS */
#define SB_BUCKET_RIGHT_CLOSED 1u     /* flags bit 0 */

typedef struct sb_column_key_buckets {
    int32_t physical_type;   /* INT8..INT64, UINT8..UINT64, FLOAT32, FLOAT64 */
    int32_t is_nullable;
    const uint8_t* pages;    /* DEVICE, at any byte alignment */
    uint64_t pages_len;
    const sb_page_meta* metas; /* HOST */
    uint64_t n_pages;
    const uint64_t* page_offsets; /* optional (HOST), as in sb_column_read */
    const uint8_t* selection;     /* DEVICE, input: as in sb_column_key_ids; NULL = every row */
    uint64_t selection_capacity;
    void* ids;               /* DEVICE, output: one id per row, aligned to id_width */
    uint64_t ids_capacity;   /* >= rows * id_width bytes */
    uint32_t id_width;       /* 1, 2 or 4 */
    uint32_t flags;          /* SB_BUCKET_RIGHT_CLOSED or 0 */
    const uint8_t* bounds;         /* HOST: n_bounds values of the column's width, strictly increasing */
    const uint32_t* bucket_ids;    /* HOST, optional: n_bounds + 1 ids; NULL = the bucket's number */
    uint64_t n_bounds;       /* 0 .. SB_BUCKET_MAX_BOUNDS */
    uint32_t nan_id;         /* the id of a live NaN; SB_KEY_ID_NONE = all ones (required for integer columns) */
    uint32_t reserved0;      /* must be 0 */
    uint64_t reserved;       /* must be 0 */
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t rows;           /* sum of num_values */
    uint64_t selected;       /* bits set in `selection` below `rows` (== rows without a selection) */
    uint64_t count;          /* selected rows that are not null */
    uint64_t matched;        /* ... whose id is not all ones */
    uint64_t nans;           /* ... that are NaN */
} sb_column_key_buckets;     /* 168 bytes */

int32_t sb_key_buckets(sb_ctx* ctx, sb_column_key_buckets* cols, uint64_t n, int32_t mem);

/* ------------------------------------------------------------------ encode
 * Replaces, per leaf column, the page loop of NativeWriter::encode_chunk
 * (src/write/common.rs:54-109): page slicing, then per page write::write -> write_simple
 * (src/write/serialize.rs:36-132): write_validity (:200-215) + compress_integer|double|
 * boolean|binary (src/compression/integer/mod.rs:35-70, double/mod.rs:32-67,
 * boolean/mod.rs:23-61, binary/mod.rs:26-93), and the PageMeta bookkeeping (:102-107).
 * Output: the column's pages back to back (the bytes NativeWriter would write_all) and
 * one sb_page_meta per page.
 *
 * Slices.  A column may be a slice of a longer Arrow array, presented without copying:
 *  - validity: row i is bit validity_bit_offset + i of `validity`.  The offset may be 8 or more (a Bitmap whose pointer
 *    was not advanced).  The library reads at most ceil((validity_bit_offset + rows) / 8) bytes from `validity`, and
 *    nothing outside bits [validity_bit_offset, validity_bit_offset + rows) reaches the pages.
 *  - Boolean values: row i is bit values_bit_offset + i of `values`, chosen independently of the validity offset; at most
 *    ceil((values_bit_offset + rows) / 8) bytes are read.  A page of a Basic codec (None / LZ4 / Zstd / Snappy) whose first
 *    value bit is byte aligned holds the bitmap's bytes as they stand (boolean/mod.rs:44-54): the spare bits of its last
 *    byte are whatever follows the page in the buffer (the next page's rows, or for the last page the bits behind the
 *    slice inside that byte).  At an unaligned first bit the page is re-packed from bit 0 and padded with zeros.  RLE and
 *    OneValue pages never depend on bits outside the slice.
 *  - Binary / LargeBinary: `offsets` holds rows + 1 entries and offsets[0] may be non-zero: entries [start, start + rows]
 *    of the parent array.  `values` is then the parent's whole values buffer and `values_len` its whole length
 *    (array.values().len(), which enters the selector and the hdr9 of Dict / Freq / OneValue pages); only bytes
 *    [offsets[0], offsets[rows]) are page content.
 *  - primitives: `values` points at row 0 of the slice, start * width bytes into its buffer; it needs the alignment of
 *    the type at most (none is required), rows * width bytes are read.
 * With SB_MEM_HOST exactly these byte counts are staged: (offset + rows + 7) / 8, values_len, (rows + 1) * width. */
typedef struct sb_column_write {
    int32_t physical_type;
    int32_t is_nullable;
    uint64_t rows;
    const void* values;          /* DEVICE: values buffer / boolean bitmap / binary value bytes */
    uint64_t values_bit_offset;  /* boolean: bit offset of row 0 in `values` (any value; see Slices above) */
    uint64_t values_len;         /* binary: byte length of the whole values buffer (array.values().len()) */
    const uint8_t* validity;     /* DEVICE or NULL (no validity bitmap) */
    uint64_t validity_bit_offset; /* bit of row 0 in `validity`; may be >= 8 */
    const void* offsets;         /* DEVICE: binary offsets, rows+1 entries; offsets[0] may be non-zero */
    /* outputs */
    uint8_t* out_pages;          /* DEVICE, capacity >= sb_write_bound() */
    uint64_t out_capacity;
    sb_page_meta* out_metas;     /* HOST, capacity n_pages_capacity; valid after synchronize */
    uint64_t n_pages_capacity;
    /* results (HOST, valid after sb_ctx_synchronize) */
    uint64_t n_pages;
    uint64_t out_len;
    /* optional explicit paging (nested leaves): rows of every page instead of max_page_size, and
     * a head (the page's level section, produced by sb_nested_write_levels) that is placed in
     * front of every page's block.  page_rows / page_head_bytes: HOST arrays of n_pages_in
     * entries; page_heads: DEVICE, the heads back to back. */
    const uint64_t* page_rows;
    const uint64_t* page_head_bytes;
    const uint8_t* page_heads;
    uint64_t n_pages_in;
    /* index of this call's first page inside its column (0 for a whole column).  A rank that encodes pages
     * [first, first + n) of a column (SURVEY §8e work items) passes `first`, so that the per-page sampling seeds — and
     * hence the adaptive codec choice — are those of a single writer. */
    uint64_t first_page_index;
    /* binary columns: byte length of the COLUMN's whole values buffer when `values` holds only the bytes of this page
     * range (0 = values_len).  Upstream slices arrays page by page without slicing the values buffer, so
     * array.values().len() — which enters the selector's total_bytes (binary/mod.rs:270) and the hdr9 of Dict / Freq /
     * OneValue pages (binary/mod.rs:88) — is the length of the whole column's buffer. */
    uint64_t column_values_len;
} sb_column_write;

/* upper bound of the encoded size of a column, and its page count (A.4 page arithmetic) */
uint64_t sb_write_bound(int32_t physical_type, int32_t is_nullable, uint64_t rows, uint64_t values_len,
                        const sb_write_options* opts, uint64_t* n_pages);
int32_t sb_write_columns(sb_ctx* ctx, sb_column_write* cols, uint64_t n, const sb_write_options* opts,
                         int32_t mem);

/* ------------------------------------------------------------------ nested level sections
 * A nested page is `u32 page_rows | u32 rep_len | u32 def_len | rep | def | leaf BLOCK`
 * (src/write/serialize.rs:135-198).  The level sections are produced / consumed here; the leaf
 * BLOCK goes through sb_write_columns / sb_read_columns with explicit paging (page_rows +
 * page_heads on write, page_offsets on read), so every codec of the flat path applies.
 *
 * sb_nested_level describes one node on the path root -> leaf (arrow2 `Nested`, to_nested in
 * src/write/serialize.rs:135): kind 0 primitive leaf, 1 list (i32 offsets), 2 large list (i64
 * offsets), 3 struct.  All pointers are DEVICE memory.
 *
 * A path has at most SB_NESTED_MAX_DEPTH nodes, the leaf included.  Every write and read call below
 * returns SB_ERR_INVALID for n_levels == 0 or n_levels > SB_NESTED_MAX_DEPTH: the call is refused
 * before anything is launched, and no output is touched. */
#define SB_NESTED_PRIMITIVE 0
#define SB_NESTED_LIST 1
#define SB_NESTED_LARGE_LIST 2
#define SB_NESTED_STRUCT 3
#define SB_NESTED_MAX_DEPTH 8
typedef struct sb_nested_level {
    const uint8_t* validity;      /* LSB-first bitmap or NULL (all valid) */
    const void* offsets;          /* lists: length + 1 entries */
    uint64_t validity_bit_offset;
    uint64_t length;              /* elements at this level (levels[0].length == rows) */
    int32_t kind;
    int32_t is_optional;
} sb_nested_level;
typedef struct sb_nested_page {
    uint64_t level_bytes;  /* 12 + rep_len + def_len */
    uint64_t num_values;   /* PageMeta.num_values of a nested page = level entries (write/common.rs:84-92) */
    uint64_t leaf_start;   /* slice of the leaf array this page carries (slice_parquet_array) */
    uint64_t leaf_count;
} sb_nested_page;
/* replaces write_nested_validity (src/write/serialize.rs:217-232) + the page cut of
 * write/common.rs:79-107 for one nested leaf column.  Writes every page's level section back to
 * back into out_levels (DEVICE) and fills pages[] (HOST).  Synchronises the context. */
uint64_t sb_nested_levels_bound(const sb_nested_level* levels, uint32_t n_levels, uint64_t rows,
                                uint64_t max_page_size);
int32_t sb_nested_write_levels(sb_ctx* ctx, const sb_nested_level* levels, uint32_t n_levels, uint64_t rows,
                               uint64_t max_page_size, uint8_t* out_levels, uint64_t out_capacity,
                               sb_nested_page* pages, uint64_t n_pages_capacity, uint64_t* n_pages_out);

/* The same for the leaf columns of a whole call (every leaf of every nested array of a chunk — encode_chunk's loop over
 * the leaves, src/write/common.rs:60-116): ONE set of launches over all pages of all leaves and ONE host round trip for
 * the page cut of the batch (32 bytes per page), instead of one per leaf column. */
typedef struct sb_nested_levels_write {
    const sb_nested_level* levels;  /* root -> leaf */
    uint32_t n_levels;
    uint32_t reserved;
    uint64_t rows;                  /* top-level rows (levels[0].length) */
    uint8_t* out_levels;            /* DEVICE: the level sections of the pages, back to back */
    uint64_t out_capacity;          /* >= sb_nested_levels_bound() */
    sb_nested_page* pages;          /* HOST, n_pages_capacity entries */
    uint64_t n_pages_capacity;
    uint64_t n_pages;               /* result */
} sb_nested_levels_write;
int32_t sb_nested_write_levels_batch(sb_ctx* ctx, sb_nested_levels_write* items, uint64_t n, uint64_t max_page_size);
/* The same without the round trip: enqueues the kernels and returns; items[].n_pages is set at once (host arithmetic),
 * items[].pages[] are filled by the next sb_ctx_synchronize.  `items` and what it points to must live until then.  A writer
 * that encodes chunk after chunk of one shape enqueues the level call and the leaf call (sb_write_columns with the page
 * cut of the chunk before) together and checks the cut afterwards (src/write/serialize.rs:217-232 runs them back to back). */
int32_t sb_nested_write_levels_enqueue(sb_ctx* ctx, sb_nested_levels_write* items, uint64_t n, uint64_t max_page_size);

/* replaces read_validity_nested (src/read/read_basic.rs:65-173) over all pages of one nested leaf
 * column.  Per level the caller passes DEVICE outputs: `offsets` (lists: column-level i64 offsets,
 * elements + 1 entries) and `validity` (nullable list/struct levels: LSB-first bitmap; 4-byte
 * aligned, capacity a multiple of 4 bytes); `length` returns the elements decoded at that level.
 * leaf_validity (DEVICE, same alignment rule) receives the leaf's validity when the leaf is
 * nullable.  page_leaf_counts / page_block_offsets (HOST, n_pages entries) return the number of
 * leaf slots of every page and the byte offset of its leaf BLOCK inside `pages`: feed them to
 * sb_read_columns as metas[].num_values / page_offsets.  Synchronises the context. */
typedef struct sb_nested_level_out {
    int64_t* offsets;
    uint8_t* validity;
    uint64_t offsets_capacity;   /* entries */
    uint64_t validity_capacity;  /* bytes */
    uint64_t length;             /* result */
    int32_t kind;
    int32_t is_nullable;
} sb_nested_level_out;
/* the leaf columns of a whole call: the arguments of sb_nested_read_levels per item, one set of launches, one round trip */
typedef struct sb_nested_levels_read {
    const uint8_t* pages;           /* DEVICE: the column's pages back to back */
    uint64_t pages_len;
    const sb_page_meta* metas;      /* HOST */
    uint64_t n_pages;
    sb_nested_level_out* levels;    /* HOST array of n_levels entries (DEVICE outputs inside); .length returns */
    uint32_t n_levels;
    uint32_t reserved;
    uint8_t* leaf_validity;         /* DEVICE or NULL */
    uint64_t leaf_validity_capacity;
    uint64_t* page_leaf_counts;     /* HOST, n_pages entries, or NULL */
    uint64_t* page_block_offsets;   /* HOST, n_pages entries, or NULL */
} sb_nested_levels_read;
int32_t sb_nested_read_levels_batch(sb_ctx* ctx, sb_nested_levels_read* items, uint64_t n);
/* The same without the round trip: levels[].length, page_leaf_counts and page_block_offsets are filled by the next
 * sb_ctx_synchronize; `items` and what it points to must live until then.  A reader that knows the page cut (a second
 * pass over the same pages) enqueues the level call and sb_read_columns together and compares afterwards. */
int32_t sb_nested_read_levels_enqueue(sb_ctx* ctx, sb_nested_levels_read* items, uint64_t n);
int32_t sb_nested_read_levels(sb_ctx* ctx, const uint8_t* pages, uint64_t pages_len, const sb_page_meta* metas,
                              uint64_t n_pages, sb_nested_level_out* levels, uint32_t n_levels,
                              uint8_t* leaf_validity, uint64_t leaf_validity_capacity,
                              uint64_t* page_leaf_counts, uint64_t* page_block_offsets);

/* ------------------------------------------------------------------ file framing (host only)
 * "ARROW2" 00 00 | column pages ... | schema bytes | metas | u32 schema_size | u32 meta_size | EOS
 * (SURVEY App. A.1).  Writer: NativeWriter::start / write / finish (src/write/writer.rs:91-167);
 * one sb_file_writer_write_column per leaf column in leaf order, with the pages and PageMeta that
 * sb_write_columns produced (copied to HOST memory).  The schema is an opaque Arrow IPC Schema
 * message flatbuffer (arrow2 schema_to_bytes upstream).  Errors carry the reference's messages;
 * sb_file_last_error() is thread-local. */
typedef struct sb_file_writer sb_file_writer;
typedef struct sb_file_reader sb_file_reader;
const char* sb_file_last_error(void);
int32_t sb_file_writer_open(const char* path, sb_file_writer** out);
int32_t sb_file_writer_start(sb_file_writer* w);
int32_t sb_file_writer_write_column(sb_file_writer* w, const uint8_t* pages, uint64_t pages_len,
                                    const sb_page_meta* metas, uint64_t n_pages);
int32_t sb_file_writer_finish(sb_file_writer* w, const uint8_t* schema_bytes, uint64_t schema_len,
                              uint64_t* total_size);
void sb_file_writer_close(sb_file_writer* w);
/* Reader: read_meta / deserialize_meta (src/read/reader.rs:148-178), the schema bytes of
 * infer_schema (:227-241), and page ranges of a column (ColumnMeta::slice src/lib.rs:47-61 +
 * NativeReader::next src/read/reader.rs:117-127) into HOST memory. */
int32_t sb_file_reader_open(const char* path, sb_file_reader** out);
uint64_t sb_file_reader_n_columns(const sb_file_reader* r);
int32_t sb_file_reader_column(const sb_file_reader* r, uint64_t col, uint64_t* offset, uint64_t* n_pages,
                              const sb_page_meta** pages);
int32_t sb_file_reader_schema(const sb_file_reader* r, const uint8_t** bytes, uint64_t* len);
int32_t sb_file_reader_read_pages(sb_file_reader* r, uint64_t col, uint64_t first_page, uint64_t n_pages,
                                  uint8_t* dst, uint64_t capacity, uint64_t* bytes_read);
void sb_file_reader_close(sb_file_reader* r);

/* ------------------------------------------------------------------ schema bytes of the footer (host only)
 * NativeWriter::finish stores arrow2's schema_to_bytes(&schema, &default_ipc_fields(..)) (src/write/writer.rs:137-139):
 * the bare Arrow IPC Message flatbuffer with a Schema header (version V5, little endian, body_length 0); infer_schema
 * feeds it to deserialize_schema (src/read/reader.rs:227-241).  These two calls write / read that flatbuffer without
 * another Arrow implementation.  A schema is passed as its fields flattened in PRE-ORDER: every entry is followed by
 * its n_children children (List / LargeList / FixedSizeList: the item field; Struct: its fields; Map: the non-null
 * "entries" struct with the key and value fields).  type_id is the `Type` union tag of Schema.fbs. */
#define SB_ARROW_NULL 1
#define SB_ARROW_INT 2              /* bit_width 8/16/32/64, is_signed */
#define SB_ARROW_FLOATING_POINT 3   /* precision: 0 half, 1 single, 2 double */
#define SB_ARROW_BINARY 4
#define SB_ARROW_UTF8 5
#define SB_ARROW_BOOL 6
#define SB_ARROW_DECIMAL 7          /* precision, scale, bit_width 128 / 256 */
#define SB_ARROW_DATE 8             /* unit: 0 day (Date32), 1 millisecond (Date64) */
#define SB_ARROW_TIME 9             /* unit (TimeUnit), bit_width 32 / 64 */
#define SB_ARROW_TIMESTAMP 10       /* unit: 0 s, 1 ms, 2 us, 3 ns; timezone or NULL */
#define SB_ARROW_INTERVAL 11        /* unit: 0 year_month, 1 day_time, 2 month_day_nano */
#define SB_ARROW_LIST 12
#define SB_ARROW_STRUCT 13
#define SB_ARROW_FIXED_SIZE_BINARY 15 /* bit_width = byte width */
#define SB_ARROW_FIXED_SIZE_LIST 16   /* bit_width = list size */
#define SB_ARROW_MAP 17             /* is_signed = keys_sorted */
#define SB_ARROW_DURATION 18        /* unit (TimeUnit) */
#define SB_ARROW_LARGE_BINARY 19
#define SB_ARROW_LARGE_UTF8 20
#define SB_ARROW_LARGE_LIST 21
typedef struct sb_schema_field {
    const char* name;     /* UTF-8, NUL terminated */
    const char* timezone; /* Timestamp only; NULL = none */
    int32_t type_id;      /* SB_ARROW_* */
    int32_t nullable;
    int32_t n_children;
    int32_t bit_width;
    int32_t is_signed;
    int32_t precision;
    int32_t scale;
    int32_t unit;
    const char* metadata; /* Field.custom_metadata: n_metadata pairs packed as "key\0value\0key\0value\0..."; NULL = none */
    uint64_t n_metadata;
} sb_schema_field;
const char* sb_schema_last_error(void);
/* metadata: 2 * n_metadata strings (key, value, key, value ...) of Schema.custom_metadata, or NULL.  *len returns the
 * size of the flatbuffer (also when `capacity` is too small: SB_ERR_INVALID, call again). */
int32_t sb_schema_to_bytes(const sb_schema_field* fields, uint64_t n_fields, uint64_t n_top, const char* const* metadata,
                           uint64_t n_metadata, uint8_t* out, uint64_t capacity, uint64_t* len);
/* Parses schema bytes written by this library, arrow2 or any other Arrow implementation.  Field names / timezones are
 * copied into `strings`; the out[].name pointers point there.  *n_fields / *strings_len return the sizes needed. */
int32_t sb_schema_from_bytes(const uint8_t* bytes, uint64_t len, sb_schema_field* out, uint64_t capacity, uint64_t* n_fields,
                             uint64_t* n_top, char* strings, uint64_t strings_capacity, uint64_t* strings_len);
/* Schema.custom_metadata of the same bytes (arrow2's deserialize_schema keeps it, src/read/reader.rs:227-241): *n_pairs
 * pairs packed into `strings` as "key\0value\0..." (*strings_len bytes; SB_ERR_INVALID + sizes when it does not fit). */
int32_t sb_schema_metadata_from_bytes(const uint8_t* bytes, uint64_t len, char* strings, uint64_t strings_capacity,
                                      uint64_t* n_pairs, uint64_t* strings_len);

/* ------------------------------------------------------------------ page inspector (host only)
 * Replaces stat::stat_simple / stat_body / stat_dict_body / stat_freq_body (src/stat.rs:61-152): the
 * block structure of one page without decoding it.  `out` receives a chain: out[0] is the page's block,
 * out[k + 1] the block nested in out[k] (the u32 indices of a Dict block, the exceptions of a primitive
 * Freq block), PageInfo / DictPageBody / FreqPageBody flattened. */
typedef struct sb_page_info {
    int32_t codec;                   /* SB_CODEC_*: PageBody variant */
    int32_t has_validity_size;       /* PageInfo.validity_size is Some (nullable field, out[0] only) */
    uint32_t validity_size;          /* as upstream reports it: the u32 FOLLOWING the def-level section, i.e. the
                                        first 4 bytes of the block header (src/stat.rs:72-76), not the section's size */
    uint32_t compressed_size;
    uint32_t uncompressed_size;
    uint32_t unique_num;             /* Dict: DictPageBody.unique_num */
    uint32_t exceptions_bitmap_size; /* Freq: FreqPageBody.exceptions_bitmap_size */
    int32_t has_nested;              /* the next entry of `out` describes this block's nested block */
} sb_page_info;
/* Returns SB_OK and the chain length in *n_out (<= capacity); SB_ERR_IO when the page is shorter than
 * its headers say (upstream: slice panic), SB_ERR_OUT_OF_SPEC for an unknown codec id. */
int32_t sb_stat_page(const uint8_t* page, uint64_t length, int32_t physical_type, int32_t is_nullable,
                     sb_page_info* out, uint32_t capacity, uint32_t* n_out);

/* ------------------------------------------------------------------ measurement
 * Optional per-kernel timing with HIP events recorded on the context's stream around every
 * kernel launch (used by bench.py for the roofline figure).  Totals are accumulated at
 * sb_ctx_synchronize(). */
typedef struct sb_kernel_stat {
    const char* name;   /* kernel name as it appears in rocprofv3 traces (without namespace) */
    uint64_t launches;
    double total_ms;
} sb_kernel_stat;
int32_t sb_ctx_profile(sb_ctx* ctx, int32_t enable);  /* enable/disable; resets the totals */
uint32_t sb_ctx_profile_read(sb_ctx* ctx, sb_kernel_stat* out, uint32_t cap);
/* Totals of the block-parallel Zstd decoder (basic.rs:93-97: libzstd frames are decoded block by block, all blocks of a
 * call at once) since the context was created: out[0] frames it decoded, out[1] frames handed back to the frame-serial
 * decoder (pools exhausted, or a malformed stream whose error that decoder names), out[2] blocks, out[3] sequences.
 * Synchronises the context. */
int32_t sb_ctx_zstd_block_stats(sb_ctx* ctx, uint64_t out[4]);

/* Calls since the context was created whose kernels were spread over side streams next to the call's stream (a mixed
 * schema in one adaptive sb_write_columns call: the binary chain beside the primitive kinds; sb_read_columns with
 * primitive and binary pages; the Zstd block pipeline).  Diagnostics only: the parity tests use it to show that the
 * multi-stream path — whose kernels exchange a page's scratch areas across streams through fork / join events — is
 * the one that ran.  Does not synchronise. */
uint64_t sb_ctx_side_forks(sb_ctx* ctx);

/* Synchronize intervals since the context was created that were issued a second time: a call skips kernels that the
 * previous calls of the same shape did not need (long-page Dict / Freq writers, the block-parallel LZ4 reader, emitters of
 * codecs no page chose); when a page needs one after all it is left undone, and sb_ctx_synchronize re-issues the
 * interval's sb_write_columns / sb_read_columns calls with everything launched before it returns.  Results are the same
 * either way; the counter lets tests show which path ran.  Does not synchronise.  A sb_read_columns_sizes call made
 * inside an open interval closes it with its own synchronize: it is issued again with the interval's other calls, and
 * both its values_len and theirs are delivered before it returns. */
uint64_t sb_ctx_replays(sb_ctx* ctx);

/* version / build info string ("strawboat-hip <ver> gfx950") */
const char* sb_version(void);

#ifdef __cplusplus
}
#endif
#endif /* STRAWBOAT_HIP_H */
