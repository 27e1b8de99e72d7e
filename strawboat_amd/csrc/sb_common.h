// strawboat-hip: structures shared by host code and gfx950 kernels.
//
// Data layout in HBM: a call works on a batch of leaf columns.  The host
// uploads one ColDesc per column and one PageTask per page; the parse kernel turns each
// page's headers into a PageDesc and fills the tile table; every later kernel is indexed
// either by page (plan kernels, one workgroup per page) or by tile (expand kernels, one
// workgroup per TILE_ROWS rows of one page).
//
// MEMORY-ORDER CONTRACT for scratch areas in HBM (slot tables, row hashes, tag tables, run records, tile entries).
// Fences inside the page kernels are WORKGROUP scope (an agent-scope release / acquire writes back and invalidates the
// XCD's L2: ~100 us per fence once the chip is busy).  Workgroup scope orders the accesses of the waves of ONE workgroup —
// they share a CU and its vector L1 — and says nothing to another CU.  So every scratch area obeys one of two rules:
//   (1) SINGLE OWNER inside a kernel: between two kernel boundaries, the bytes of a scratch area that one workgroup
//       writes are read by that workgroup only.  The owner is fixed by the launch geometry: blockIdx.x = page for the page
//       kernels, (blockIdx.x, blockIdx.y) = (page, tile / section) for the tile- and section-parallel ones, whose
//       areas are indexed by that pair.  A workgroup never reads another (page, tile)'s scratch inside the kernel
//       that wrote it.
//   (2) KERNEL BOUNDARY between owners: a consumer with another geometry (k_enc_bin_hash's (page, tile) grid -> the
//       page selector -> k_enc_bin_verify's grid -> the page emitters; k_sel_big_count -> _merge -> _sec; k_rle_big_count
//       -> _plan -> _emit; k_parse -> k_plan -> k_expand*) is a LATER KERNEL, ordered after the producer by stream order
//       or by a fork / join event edge when the chain runs on a side stream (side_fork / side_join, sb_api.hip): the
//       end-of-kernel release and start-of-kernel acquire are agent scope and do what the in-kernel fences do not.
// What workgroups of ONE launch do share is touched with AGENT-scope operations only, and says so where it stands: job
// queues and counters (atomicAdd / __hip_atomic_fetch_add, push_job_if), the key tables in HBM that all sections of a long
// page insert into (SlotTable / k_sel_big_count: agent-scope load, CAS and fetch_min — a table is complete at the kernel
// boundary; the one in-kernel read of shared progress is the relaxed agent-scope load of the distinct counter by which
// sections stop early once Dict's limit is passed), and last_workgroup_done (sb_decode.hip: __threadfence() = agent-scope
// release before the counter, acquire after it in the workgroup that finds itself last).
// tests/test_gpu_configs.py::test_c4_all_columns_in_one_call runs the binary chain on the side stream next to the
// primitive kinds (sb_ctx_side_forks shows it did) and compares every page with the oracle's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/strawboat_hip.h"

namespace sb {

constexpr int TILE_ROWS = 4096;  // rows of one page handled by one workgroup
constexpr int WG = 256;          // threads per workgroup = 4 wave64
constexpr int ROWS_PER_THREAD = TILE_ROWS / WG;

struct ColDesc {
    const uint8_t* pages;  // concatenated pages of the column
    uint64_t pages_len;
    uint8_t* values;
    uint64_t values_cap;
    uint8_t* validity;
    uint8_t* offsets;
    uint64_t offsets_cap;
    uint64_t rows;
    int32_t ptype;
    int32_t nullable;
    uint32_t width;       // bytes per value (primitives), 4/8 for binary offsets, 0 bool
    uint32_t first_page;  // index into the page tables
    uint32_t n_pages;
    uint32_t bits_aligned;  // every page starts at a multiple of 32 rows: bitmap words are never shared
};

struct PageTask {
    uint64_t in_off;      // byte offset of the page in ColDesc.pages
    uint64_t length;      // PageMeta.length
    uint64_t num_values;  // PageMeta.num_values
    uint64_t out_row;     // first row of the page in the column's output
    uint64_t aux_off;     // byte offset of the page's u32 aux area in the scratch buffer
    uint64_t infl_off;    // byte offset of the page's inflate area in the scratch buffer
    uint32_t col;
    uint32_t first_tile;
};

struct TileTask {
    uint32_t page;
    uint32_t tile;
    uint32_t col;  // = tasks[page].col: lets k_expand fetch its three descriptors in one round trip
    uint32_t k0;   // RLE pages (k_plan): first run of the tile ...
    uint32_t kend; // ... and one past its last run; 0 / 0 otherwise
    uint32_t pad;
};

// result of parsing one page's headers (hdr9 = u8 codec | u32 compressed | u32 uncompressed,
// reference src/read/read_basic.rs:181-189)
struct PageDesc {
    const uint8_t* def_bits;  // validity bits of the def-level section (NULL: not nullable)
    const uint8_t* body;      // body of the page's (first) block
    const uint8_t* ibody;     // Dict: body of the nested u32 index block
    const uint8_t* dict;      // Dict: first entry; binary OneValue: value bytes
    const uint8_t* vbody;     // binary Basic: body of the values block
    const uint8_t* src;       // where the expand step reads "plain" data from (body or inflated copy)
    const uint8_t* isrc;      // same for nested indices
    uint32_t csize, usize;    // of the first block
    uint32_t icsize;          // nested block compressed size
    uint32_t dict_n;          // Dict: entries; binary OneValue: value length
    uint32_t vcsize, vusize;  // binary Basic values block
    uint8_t codec;            // page codec
    uint8_t icodec;           // nested codec (Dict) or 255
    uint8_t ok;               // 1 = parsed, expand may run
    uint8_t pad;
    uint32_t n_runs;          // RLE: number of runs (filled by plan)
    uint32_t tile_base;       // first entry of the page in the compact tile list (k_parse)
    uint32_t pad2;
    uint64_t val_bytes;       // binary: value bytes this page produces
    uint64_t val_base;        // binary: first value byte of the page in the column output (colscan)
    uint64_t off_last;        // binary: last offset of the page as decoded (page relative)
    uint64_t off_base;        // binary: offset base of the page (colscan)
};

struct Status {
    int32_t code;   // first error (SB_ERR_*), 0 = ok
    uint32_t page;  // page index within the call
    uint32_t where; // kernel-specific tag
    uint32_t kinds; // KIND_* bits of what the calls have met so far (never cleared: the host sizes later calls by it)
};
constexpr uint32_t KIND_ZSTD = 1u;   // a Zstd buffer was queued
constexpr uint32_t KIND_LZ4_GIANT = 4u;   // an LZ4 block of >= LZG_MIN compressed bytes was queued (sb_lz4_giant.h is launched for contexts that meet them)
constexpr uint32_t KIND_REPLAY = 8u;      // a page was left undone because a kernel it needed was not launched on a hint: sb_ctx_synchronize re-issues the interval's calls with everything launched
constexpr uint32_t KIND_REPLAY_LZG = 16u; // ... and it was an LZ4 block of megabytes that asked (the context turns the block-parallel chain on again)
constexpr uint32_t KIND_QUEUE_A = 32u;    // a read call queued inflate jobs for queue A (Basic blocks of primitive pages, index / offset blocks)
constexpr uint32_t KIND_TILES = 64u;      // a read call had tile tasks (k_expand / k_expand_binary)
constexpr uint32_t KIND_FILTER_FREQ = 128u; // a filter call met a primitive Freq page (with KIND_REPLAY): the replay decodes that call's columns into the staging area (sb_filter.h)
constexpr uint32_t KIND_ZSEQ_LONG = 2u;   // a Zstd block of >= 8192 sequences was met (zb_hdr): the sequence chains are the long pole

// one general-purpose block (LZ4 / Zstd / Snappy) to inflate: src -> dst
struct InflateJob {
    const uint8_t* src;
    uint8_t* dst;
    uint32_t csize;
    uint32_t out_len;
    uint32_t codec;     // codec id | JOB_REL
    uint32_t page;
};
constexpr uint32_t JOB_REL = 0x100;   // dst is a byte offset from the page's value base (cols[col].values + descs[page].val_base)

// one Freq page (integer/freq.rs:90-127), logged by k_parse: its exceptions block is an ordinary
// BLOCK<T> that a second decode pass expands, then k_freq_scatter puts the values in place
struct FreqEntry {
    const uint8_t* roaring;  // serialized RoaringBitmap of the exception rows
    const uint8_t* nested;   // BLOCK<T exceptions>
    uint8_t* out;            // the page's values in the column output
    uint64_t nested_len;     // bytes from `nested` to the end of the page
    uint64_t rows;
    uint32_t roaring_len;
    uint32_t n_exceptions;
    uint32_t ptype, width;
    uint32_t page, pad;
};

// ---- the block-parallel Zstd pipeline (sb_zstd_blocks.h): descriptors and pools of one call
struct ZbBlock {
    const uint8_t* src;     // block content (after the 3-byte block header)
    uint32_t bsize;         // content bytes in the stream (RLE block: 1)
    uint32_t frame;
    uint32_t btype;         // 0 raw, 1 RLE, 2 compressed
    uint32_t out_size;      // raw / RLE: from the header; compressed: literals + match bytes (zb_seq; nseq == 0: regen)
    uint32_t ltype, lstreams, regen, lcsize, lpay;   // literals section: type, streams, regenerated / compressed size, payload offset
    uint32_t huf_def;       // block whose literal payload starts with the Huffman tree in use
    uint32_t nseq, modes, seq_off;                   // sequences: count, modes byte, offset of the byte after it
    uint32_t def[3];        // LL, OF, ML: block whose description defines the table in use; ZB_NONE: predefined
    uint32_t desc[3];       // zb_hdr: offsets (in this block) of its own descriptions (modes 1 and 2)
    uint32_t bits_off;      // zb_hdr: offset of the sequence bit stream
    uint64_t lit_pos;       // the block's literals in the literal pool (types 1, 2, 3)
    uint64_t rec_pos;       // the block's records in the record pool
};
struct ZbFrame {
    uint8_t* dst;
    uint32_t out_len;
    uint32_t first, nblocks;
    uint32_t job;           // queue entry
    uint32_t page;
    uint32_t punt;          // != 0: the one-wave decoder takes the frame
    uint32_t avail;         // bytes of the queue entry's buffer (loads never reach beyond it)
    uint32_t queue;         // 0: queue A, 1: queue Z (executed after k_colscan)
    uint32_t rel;           // dst is relative to the page's value base (JOB_REL)
    uint32_t wg;            // executed by zb_exec_wg (many short sequences) instead of zb_exec
    const uint8_t* base;    // the queue entry's buffer
};
struct ZbPools {             // (the defaults: the pipeline is not launched)
    ZbBlock* blocks = nullptr;
    ZbFrame* frames = nullptr;
    uint8_t* lit = nullptr;
    uint64_t* rec = nullptr;          // 12 bytes per sequence: literal length, match length, offset value (rec_pos counts sequences)
    uint32_t* counters = nullptr;     // [0] blocks, [1] frames, [4..5] literal bytes, [6..7] records, [8..11] blocks with sequences per size class
    uint32_t* lists = nullptr;        // zb_hdr: the blocks with sequences, by size class (4 x block_cap indices)
    uint32_t block_cap = 0, frame_cap = 0;
    uint64_t lit_cap = 0, rec_cap = 0;
    uint32_t min_csize = 0;     // frames shorter than this stay with the one-wave / lane-per-frame paths
    uint32_t wg_exec = 0;       // 0: every frame through the wave executor (SB_ZSTD_BLOCKS_WG=0)
    unsigned long long* stats = nullptr;   // totals of the context: [0] frames decoded, [1] frames handed back, [2] blocks, [3] sequences
    uint32_t* kinds = nullptr;             // Status.kinds of the call
};


// the pool of inflate waves (k_inflate) and its per-wave areas
constexpr uint32_t INFLATE_POOL = 2048;          // waves
constexpr uint32_t ZREC_PER_WAVE = 128 * 1024;   // pre-decoded Zstd sequence records (8 bytes each) per pool wave
// a LONG Zstd buffer (compressed bytes): the host launches the frame scan for calls with a page this long, or marks the call
// zb_skipped when the block pipeline is left out on a hint; k_zstd_split then leaves such a buffer undone and asks for the replay
constexpr uint32_t ZSTD_LONG_MIN = 1u << 20;

// one LZ4 block of megabytes decoded by the whole chip (sb_lz4_giant.h)
constexpr uint32_t LZG_MIN = 2u << 20;     // compressed bytes
constexpr uint32_t LZG_JOBS = 16;
constexpr uint32_t LZG_CH = 4096;          // positions per chunk
constexpr uint32_t LZG_GROUP = 64;         // chunks per group
constexpr uint32_t LZG_WIN = 8192;         // entries per window of k_lzg_jump
constexpr uint32_t LZG_LITS = 4096, LZG_LIT_MIN = 32768;
struct LzgJob {
    const uint8_t* src;
    uint8_t* dst;
    uint32_t n, out_len, page, nchunks, ngroups, nwin;
    uint32_t err, left;     // first error (0: none); windows with unresolved entries
    uint32_t queue, slot;   // where the job came from
    uint32_t* eo;           // [n][2]: exit of the chunk from the position, output bytes up to there
    uint32_t* gtab;         // [n][2]: exit of the GROUP from the position, output bytes up to there (k_lzg_groups)
    uint32_t* gent;         // [ngroups][2]: the chain's entry position / output position (LZG_NONE: the chain skips the group)
    uint32_t* cent;         // [nchunks][2]
    uint32_t* ent;          // [out_len] entries
    uint32_t* wdone;        // [nwin]
    uint32_t* lits;         // [LZG_LITS][4]: literal runs of >= LZG_LIT_MIN bytes (source position, output position, length), copied by all workgroups
    uint32_t nlits, pad0;
};
struct LzgArgs {
    LzgJob* jobs = nullptr;           // LZG_JOBS
    uint32_t* njobs = nullptr;
    uint8_t* pool = nullptr;
    uint64_t pool_bytes = 0;
    Status* st = nullptr;
};


struct DecodeArgs {
    const ColDesc* cols = nullptr;
    const PageTask* tasks = nullptr;
    PageDesc* descs = nullptr;
    TileTask* tiles = nullptr;
    uint8_t* scratch = nullptr;
    Status* status = nullptr;
    InflateJob* jobs_a = nullptr;  // capacity job_cap_a
    InflateJob* jobs_b = nullptr;  // capacity job_cap_b
    // queue Z (calls with binary columns): the Zstd payloads nothing in the planning steps waits for — Basic pages of
    // primitives (absolute dst) and the VALUE blocks of Basic binary pages, whose place in the column's values buffer is only
    // known after k_colscan (JOB_REL: dst is an offset from the page's value base).  k_parse fills it, so the block-parallel
    // Zstd pipeline runs its entropy stages for queue A and queue Z in ONE pass, before k_plan; the frames of queue Z are
    // executed after k_colscan.  null: no such queue in this call.
    InflateJob* jobs_z = nullptr;
    uint32_t* job_counts = nullptr;  // [0] = queue A, [1] = queue B, [2] tiles, [3] planned pages, [4] page-level RLE, [5] / [6] workgroups of k_parse / k_colscan that are done, [8] / [9] / [11] lengths of A / B / Z when complete, [10] = queue Z, [12] = binary Dict pages whose tile totals k_plan left to k_bin_tile_sums
    uint8_t* zlit = nullptr;         // Zstd literal buffers, one per inflate wave
    uint64_t* zrec = nullptr;        // Zstd sequence records, one arena per inflate wave (k_inflate's lane-per-frame pre-decode)
    uint32_t n_pages = 0;
    uint32_t n_cols = 0;
    uint32_t n_tiles = 0;
    FreqEntry* freq_log = nullptr;   // Freq pages found by k_parse (shared by the calls of one synchronize interval)
    uint32_t* freq_count = nullptr;
    uint32_t freq_cap = 0;
    uint32_t no_freq = 0;      // second pass: an exceptions block never holds a Freq block (freq.rs:78-79)
    uint32_t sizes_only = 0;   // sb_read_columns_sizes: only what values_len depends on is inflated (nested index blocks)
    uint32_t defer_payloads = 0;  // the call has binary columns (queue B runs): Basic payloads nothing waits for go there too
    uint32_t job_cap_a = 0, job_cap_b = 0;  // entries of the two job queues (2 * n_pages + room for the frames of split Zstd buffers)
    uint32_t lz4_big_min = 0xFFFFFFFFu;  // LZ4 blocks of at least this many compressed bytes go to k_inflate_lz4_big (0xFFFFFFFF: the call has no page that long)
    ZbPools zb;            // block-parallel Zstd pipeline (zb.blocks == nullptr: not launched for this call)
    // frame split of LONG multi-frame Zstd buffers (k_zsplit_scan / k_zsplit_chain; null: every buffer is walked by one lane):
    // zs_hdr[0] = entries listed, [1] = segment records handed out, [16 + 2 i], [17 + 2 i] = (queue entry, first record) of
    // listed entry i; zs_segs: records of 8 words (count | 7 positions of the frame magic inside a 16 KiB segment)
    uint32_t* zs_hdr = nullptr;
    uint32_t* zs_segs = nullptr;
    uint32_t zs_seg_cap = 0;
    // long RLE pages (a call with few pages of >= 2^18 rows): `rle_parts` workgroups per page, rle_sums[page * parts + part]
    uint32_t rle_parts = 0;
    uint64_t* rle_sums = nullptr;
    // long bit-packed pages (the same calls): bp_guess[page] = blocks from the first on that share its width (k_bp_guess)
    uint32_t* bp_guess = nullptr;
    // LZ4 blocks of LZG_MIN compressed bytes and more, block-parallel (sb_lz4_giant.h); lzg.jobs == nullptr: not in this call
    LzgArgs lzg;
    uint32_t lzg_chunks = 0, lzg_wins = 0, lzg_rounds = 0, lzg_jobs = 0;   // grid sizes: the longest page / the largest output of the call / pages long enough
    uint32_t zb_skipped = 0;    // the block-parallel Zstd pipeline was left out on a hint (the context's last intervals read no Zstd buffer): a Zstd buffer of a megabyte or more asks for the replay instead of going frame by frame through the one-wave decoder (20 ms for a 96 MB page against 1.3)
    uint32_t read_skips = 0;    // RSKIP_* bits: kernels left out because the context's last read interval had no work for them (k_plan asks for the replay when this call has)
    uint32_t lzg_skipped = 0;   // the call has pages long enough but the context's last intervals met no such block: the chain is not launched, a block that shows up after all asks for a replay (KIND_REPLAY)
};
// (passed to the kernels by value: the member initialisers above are the "off" state of a call and change nothing in that)
static_assert(sizeof(DecodeArgs) == 368 && __is_trivially_copyable(DecodeArgs), "DecodeArgs is a kernel argument");
// one column of a filter call (sb_filter_columns, sb_filter.h), next to its ColDesc
struct FilterCol {
    uint32_t* sel;     // the selection bitmap, in 32-bit words
    uint64_t lit;      // the literal: zero- / sign-extended to 64 bits, floats as the bits of a double; FK_BYTES: the DEVICE
                       // address of its lit_len bytes, followed by at least 8 zero bytes (sb_filter_bin.h)
    uint32_t kind;     // how values compare: FK_*
    uint32_t mask;     // bit r set: relation r (0 less, 1 equal, 2 greater, 3 unordered) satisfies the predicate
    uint32_t op;       // SB_PRED_*
    uint32_t combine;  // SB_SEL_*
    int32_t ptype;     // the column's physical type (an IS_[NOT_]NULL column is parsed as SB_TYPE_NULL: no page body is looked at)
    uint32_t lit_len;  // FK_BYTES: bytes of the literal
};
struct FilterLaunch {   // what launch_decode needs to end a call with the filter kernels instead of the expand kernels
    const FilterCol* fcols;
    uint64_t* counts;      // [n_cols]: bits set per column
    bool any_cmp, any_null, any_set;
    bool any_bin;          // comparison columns of a binary type: k_filter_bin_base / _entries / k_filter_bin (sb_filter_bin.h)
    bool any_sub = false;  // ... with a FILTER_MASK_SUB bit among them: k_filter_sub_entries / k_filter_sub as well (sb_filter_sub.h)
};
// one column of an IN / NOT IN call (sb_filter_columns_in, sb_filter_in.h), next to its FilterCol: the literals as a sorted
// set without duplicates, in the call's tables.  FilterCol.op is SB_PRED_IN / SB_PRED_NOT_IN, FilterCol.kind as ever.
constexpr uint32_t IN_MAX_VALUES = 1024;   // SB_IN_MAX_VALUES
struct InCol {
    const uint64_t* keys;   // numeric: n order keys (in_key), ascending; FK_BYTES: n + 1 ascending offsets into `bytes`
    const uint8_t* bytes;   // FK_BYTES: the literals back to back in byte-string order, followed by 8 zero bytes
    uint32_t n;             // 0 .. IN_MAX_VALUES
    uint32_t steps;         // ceil(log2(n + 1)): the trip count of the search
    uint32_t negate;        // NOT IN
    uint32_t pad;
};
// The order key of a numeric value (agg_key's mapping, sb_aggregate.h: unsigned as is, signed with the sign bit flipped,
// floats in the total order), with -0.0 folded onto +0.0: equal keys <=> values that compare equal, for everything that
// is not a NaN.  A NaN's key is no other value's, and the host keeps NaN literals out of the set.
__host__ __device__ inline uint64_t in_key(uint32_t kind, uint32_t w, uint64_t raw) {
    if (kind == 0u /* FK_UNSIGNED */) return raw;
    if (kind == 1u /* FK_SIGNED */) {
        const uint32_t sh = 64 - 8 * w;
        return (uint64_t)((int64_t)(raw << sh) >> sh) ^ (1ull << 63);
    }
    if (kind == 2u /* FK_F32 */) {
        uint32_t b = (uint32_t)raw;
        if ((b << 1) == 0) b = 0;
        return (b >> 31) ? (uint32_t)~b : (b | 0x80000000u);
    }
    if ((raw << 1) == 0) raw = 0;
    return (raw >> 63) ? ~raw : (raw | (1ull << 63));
}
// The keys below x among n ascending keys: in_member's loop (sb_filter_in.h) returning the position.  `steps` =
// ceil(log2(n + 1)) probes whatever x is, and no branch; n = 0 has 0 steps and the position 0.  Where x is one of the keys
// the position is its index.
__host__ __device__ inline uint32_t key_steps(uint32_t n) {
    uint32_t s = 0;
    while ((1ull << s) < (uint64_t)n + 1) s++;
    return s;
}
__host__ __device__ inline uint32_t key_lower_bound(const uint64_t* keys, uint32_t n, uint32_t steps, uint64_t x) {
    uint32_t pos = 0;
    for (uint32_t s = steps; s-- > 0;) {
        const uint32_t p = pos + (1u << s);
        const uint64_t k = keys[(p < n ? p : n) - 1];   // (steps > 0: n >= 1, and p >= 1)
        pos = (p <= n && k < x) ? p : pos;
    }
    return pos;
}
// one column of a key-id call (sb_key_ids, sb_key_ids.h), next to its AggCol (of which sel, rows, kind and w are used).
// The distinct set of a column is an open-addressing table of order keys (in_key) in the call's scratch: `tab_mask` + 1
// slots, a power of two >= 4 * max_keys, 0 = empty; the key 0 itself is KeyState.has_zero.
constexpr uint32_t KEY_MAX_KEYS = 1024;            // SB_KEY_MAX_KEYS (= IN_MAX_VALUES: 8 KiB of LDS, 11 probes)
struct KeyCol {
    uint8_t* ids;          // the caller's ids: one unsigned integer of `idw` bytes per row of the column (output)
    uint64_t tab0;         // the column's first slot in KeyLaunch.tabs
    uint32_t tab_mask;
    uint32_t max_keys;     // 1 .. min(KEY_MAX_KEYS, 2^(8 * idw) - 1)
    uint32_t idw;          // 1, 2 or 4
    uint32_t pad;
};
struct KeyState {          // 32 bytes per column, zeroed with the tables before the collect walk
    uint64_t count;        // live rows (one integer add per tile / page part)
    uint32_t inserted;     // keys that won a slot of the table
    uint32_t overflow;     // collect: more than max_keys keys are in, nothing more is inserted; k_key_finish: the verdict
    uint32_t has_zero;     // the order key 0 is among the live rows
    uint32_t n_keys;       // k_key_finish: the sorted keys of the column ...
    uint32_t steps;        // ... and the trip count of the search over them
    uint32_t pad;
};
// the result of a column: { selected, count, n_keys, overflow, 0, 0, 0, 0 }, then kmax key slots of 8 bytes (the call's
// largest max_keys), of which the column's own max_keys are handed over
__host__ __device__ inline uint64_t key_result_words(uint32_t kmax) { return 8 + (uint64_t)kmax; }
__host__ __device__ inline uint32_t key_table_slots(uint32_t max_keys) {
    uint32_t s = 64;
    while (s < 4 * max_keys) s <<= 1;
    return s;
}
struct AggCol;
struct KeyLaunch {   // what launch_decode needs to end a call with the collect kernels; the finish and assign kernels take it too
    const AggCol* acols;
    const KeyCol* kcols;
    KeyState* st;          // [n_cols], and behind them the tables: one area, zeroed by launch_key_zero
    uint64_t* tabs;
    uint64_t* sorted;      // [n_cols * KEY_MAX_KEYS]: k_key_finish's sorted order keys, for the assign walk
    uint64_t zero_bytes;   // of the area at `st`
    uint32_t kmax;
    uint32_t n_cols;
};
// one column of a key-lookup call (sb_key_lookup, sb_key_lookup.h), next to its AggCol (of which sel, rows, kind and w are
// used).  The caller's list as the kernels search it: InCol's two forms -- numeric: n order keys (in_key), ascending;
// binary: n + 1 ascending offsets into `bytes`, the literals back to back in byte-string order with 8 zero bytes behind
// them -- without duplicates, and beside it the id the list gives each sorted position.
struct LookCol {
    uint8_t* ids;           // the caller's ids: one unsigned integer of `idw` bytes per row of the column (output)
    const uint64_t* keys;
    const uint32_t* kid;    // n ids, each below all ones of `idw`: kid[i] belongs to keys[i]
    const uint8_t* bytes;   // binary columns
    uint32_t n;             // 0 .. KEY_MAX_KEYS
    uint32_t steps;         // key_steps(n)
    uint32_t idw;           // 1, 2 or 4
    uint32_t pad;
};
struct LookState {          // 16 bytes per column, zeroed before the walk; one integer add per tile / page part into each
    uint64_t count;         // live rows
    uint64_t matched;       // ... whose value is in the list
};
constexpr uint32_t LOOK_RESULT_WORDS = 4;   // { selected, count, matched, 0 }
struct LookLaunch {   // what launch_decode needs to end a call with the lookup kernels
    const AggCol* acols;
    const LookCol* lcols;
    LookState* st;         // [n_cols]
    uint32_t n_cols;
    bool any_num, any_bin;
};
// one column of a key-buckets call (sb_key_buckets, sb_key_buckets.h), next to its AggCol (of which sel, rows, kind and w are
// used).  The caller's bounds as order keys (in_key), strictly ascending, and the id of each of the n + 1 buckets: bucket 0
// below keys[0], bucket i from keys[i - 1] to keys[i].  A float whose order key is below nan_lo or above nan_hi is a NaN
// (the keys of -inf and +inf); an integer column has 0 and all ones there, which no key is outside of.
constexpr uint32_t BUCK_MAX_BOUNDS = 1023;   // SB_BUCKET_MAX_BOUNDS: n + 1 <= KEY_MAX_KEYS ids, 4 KiB of LDS
struct BuckCol {
    uint8_t* ids;           // the caller's ids: one unsigned integer of `idw` bytes per row of the column (output)
    const uint64_t* keys;   // n order keys
    const uint32_t* bid;    // n + 1 ids, each below all ones of `idw` or 0xFFFFFFFF ("no id")
    uint64_t nan_lo, nan_hi;
    uint32_t n;             // 0 .. BUCK_MAX_BOUNDS
    uint32_t steps;         // key_steps(n)
    uint32_t idw;           // 1, 2 or 4
    uint32_t right_closed;  // SB_BUCKET_RIGHT_CLOSED: a value equal to a bound stays below it
    uint32_t nan_id;        // the id of a live NaN; 0xFFFFFFFF: all ones
    uint32_t pad;
};
struct BuckState {          // 32 bytes per column, zeroed before the walk; one integer add per tile / page part into each
    uint64_t count;         // live rows
    uint64_t matched;       // ... whose id is not all ones
    uint64_t nans;          // ... that are NaN
    uint64_t pad;
};
constexpr uint32_t BUCK_RESULT_WORDS = 4;   // { selected, count, matched, nans }
struct BuckLaunch {   // what launch_decode needs to end a call with the bucket kernels
    const AggCol* acols;
    const BuckCol* bcols;
    BuckState* st;         // [n_cols]
    uint32_t n_cols;
};
// ---- sb_key_combine (sb_key_combine.h): the key of a row is a tuple of 2 .. 4 part ids, each below KEY_MAX_KEYS.  Its
// code is a 64-bit word with one COMB_FIELD_BITS field per part, part 0 highest, so that codes order as the tuples do
// lexicographically.  The host's delivery, the kernels and tests/test_key_combine_host.py use these two functions.
constexpr uint32_t COMB_MAX_PARTS = 4;             // SB_KEY_COMBINE_MAX_PARTS
constexpr uint32_t COMB_FIELD_BITS = 10;           // 2^10 == KEY_MAX_KEYS: a valid part id fits a field
static_assert((1u << COMB_FIELD_BITS) == KEY_MAX_KEYS && COMB_MAX_PARTS * COMB_FIELD_BITS <= 64, "a field per part id");
__host__ __device__ inline uint64_t comb_pack(const uint32_t* part_id, uint32_t n_parts) {
    uint64_t code = 0;
    for (uint32_t p = 0; p < n_parts; p++) code = (code << COMB_FIELD_BITS) | (uint64_t)(part_id[p] & (KEY_MAX_KEYS - 1));
    return code;
}
// the n_parts part ids of a code into out[0 .. n_parts), 0 into out[n_parts .. COMB_MAX_PARTS)
__host__ __device__ inline void comb_unpack(uint64_t code, uint32_t n_parts, uint32_t* out) {
    for (uint32_t p = COMB_MAX_PARTS; p-- > 0;) {
        if (p >= n_parts) {
            out[p] = 0;
            continue;
        }
        out[p] = (uint32_t)(code & (KEY_MAX_KEYS - 1));
        code >>= COMB_FIELD_BITS;
    }
}
// one item of a key-combine call, next to its AggCol (rows; no selection; the codes are a FK_UNSIGNED column of 8-byte
// values) and its KeyCol (ids, the table, max_keys), which k_key_finish and key_stage take as they are
struct CombItem {
    const uint8_t* part[COMB_MAX_PARTS];   // the part id arrays (input)
    uint32_t width[COMB_MAX_PARTS];        // 1, 2 or 4 bytes per id
    uint32_t bound[COMB_MAX_PARTS];        // an id at or above it: the row is not live
    uint32_t n_parts;                      // 2 .. COMB_MAX_PARTS
    uint32_t pad;
};
struct CombLaunch {
    const CombItem* items;
    KeyLaunch kl;          // acols / kcols / st / tabs / sorted of the call's items, as for sb_key_ids
    uint64_t max_rows;     // of the call's items
};
// ---- sb_key_ids_var (sb_key_ids_bin.h): the keys are byte strings.  The order is sb_filter_columns_var's (bin_rel_prefix):
// bytes unsigned, a proper prefix less than the longer string.  The helpers below are the host's and the device's alike
// (tests/test_key_ids_var_host.py runs them against std::lexicographical_compare / std::lower_bound); a load never touches
// a byte before a string's first or behind its last (the rule at the head of sb_filter_bin.h).
#if defined(__HIP_DEVICE_COMPILE__)
#define SB_KV_PTR(T) __attribute__((address_space(1))) const T*   // strings live in HBM: global_load, not flat_load
#else
#define SB_KV_PTR(T) const T*
#endif
__host__ __device__ inline uint64_t kv_ld64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, (SB_KV_PTR(uint8_t))p, 8);
    return v;
}
// the n (0 .. 7) bytes at p as a little-endian number
__host__ __device__ inline uint64_t kv_ld_short(const uint8_t* p, uint32_t n) {
    SB_KV_PTR(uint8_t) g = (SB_KV_PTR(uint8_t))p;
    if (n >= 4) {
        uint32_t a, b;
        __builtin_memcpy(&a, g, 4);
        __builtin_memcpy(&b, g + n - 4, 4);
        return (uint64_t)a | ((uint64_t)b << (8 * (n - 4)));
    }
    if (n >= 2) {
        uint16_t a, b;
        __builtin_memcpy(&a, g, 2);
        __builtin_memcpy(&b, g + n - 2, 2);
        return (uint64_t)a | ((uint64_t)b << (8 * (n - 2)));
    }
    return n ? (uint64_t)*g : 0ull;
}
#undef SB_KV_PTR
// the first min(n, 8) bytes, zero padded, as a little-endian number / as a number that orders like the bytes.  Two strings
// whose prefixes differ order as their prefixes do; equal prefixes decide nothing.
__host__ __device__ inline uint64_t kv_first8(const uint8_t* p, uint32_t n) { return n >= 8 ? kv_ld64(p) : kv_ld_short(p, n); }
__host__ __device__ inline uint64_t kv_prefix(const uint8_t* p, uint32_t n) { return __builtin_bswap64(kv_first8(p, n)); }
// a against b: 0 less, 1 equal, 2 greater
__host__ __device__ inline uint32_t kv_rel(const uint8_t* a, uint32_t n, const uint8_t* b, uint32_t m) {
    const uint32_t k = n < m ? n : m;
    if (k < 8) {
        const uint64_t x = kv_ld_short(a, k), y = kv_ld_short(b, k);
        if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? 0u : 2u;
    } else {
        uint32_t i = 0;
        for (; i + 8 <= k; i += 8) {
            const uint64_t x = kv_ld64(a + i), y = kv_ld64(b + i);
            if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? 0u : 2u;
        }
        if (i < k) {   // the tail once more at its last 8 bytes: the bytes read twice are equal
            const uint64_t x = kv_ld64(a + k - 8), y = kv_ld64(b + k - 8);
            if (x != y) return __builtin_bswap64(x) < __builtin_bswap64(y) ? 0u : 2u;
        }
    }
    return n < m ? 0u : n == m ? 1u : 2u;
}
__host__ __device__ inline bool kv_equal(const uint8_t* a, uint32_t n, const uint8_t* b, uint32_t m) { return n == m && kv_rel(a, n, b, m) == 1u; }
// a function of the bytes alone; the low bits pick the slot, the top KEYV_TAG_BITS are the tag
__host__ __device__ inline uint64_t kv_mix(uint64_t h, uint64_t w) {
    h = (h ^ w) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}
__host__ __device__ inline uint64_t kv_hash(const uint8_t* p, uint32_t n) {
    uint64_t h = ((uint64_t)n + 1) * 0xD6E8FEB86659FD93ull;
    if (n < 8) {
        h = kv_mix(h, kv_ld_short(p, n));
    } else {
        uint32_t i = 0;
        for (; i + 8 <= n; i += 8) h = kv_mix(h, kv_ld64(p + i));
        if (i < n) h = kv_mix(h, kv_ld64(p + n - 8));
    }
    h *= 0xFF51AFD7ED558CCDull;
    return h ^ (h >> 32);
}
// The keys below x among n keys ascending by bytes: key_lower_bound's loop.  Key i is len[i] bytes at ptr[i] with the
// prefix pre[i]; a probe whose prefix differs from x's loads no byte of the key.
__host__ __device__ inline uint32_t kv_lower_bound(const uint64_t* pre, const uint64_t* ptr, const uint32_t* len, uint32_t n, uint32_t steps,
                                                   const uint8_t* x, uint32_t xn) {
    const uint64_t xpre = kv_prefix(x, xn);
    uint32_t pos = 0;
    for (uint32_t s = steps; s-- > 0;) {
        const uint32_t p = pos + (1u << s);
        const uint32_t i = (p < n ? p : n) - 1;   // (steps > 0: n >= 1, and p >= 1)
        const uint64_t kp = pre[i];
        const bool below = kp != xpre ? kp < xpre : kv_rel((const uint8_t*)(uintptr_t)ptr[i], len[i], x, xn) == 0u;
        pos = (p <= n && below) ? p : pos;
    }
    return pos;
}
// The slot of a table or set is one 64-bit word, complete the moment a compare-and-swap makes it visible:
//   bits 0 .. 7 the tag | 8 .. 9 the form (1 .. 3: never 0, the empty slot) | 10 .. 35 the index | 36 .. 63 the page
// and names a string that memory no kernel of the call writes any more resolves to (pointer, length):
//   KEYV_ENTRY  entry `index` of the Dict / Freq page   KEYV_ROW  row `index` of the Basic page   KEYV_ONE  the OneValue page's value
constexpr uint32_t KEYV_TAG_BITS = 8, KEYV_INDEX_BITS = 26, KEYV_PAGE_BITS = 28;
constexpr uint32_t KEYV_ENTRY = 1, KEYV_ROW = 2, KEYV_ONE = 3;
__host__ __device__ inline uint64_t kv_word(uint32_t form, uint32_t page, uint32_t index, uint64_t hash) {
    return ((uint64_t)page << 36) | ((uint64_t)index << 10) | ((uint64_t)form << 8) | (hash >> (64 - KEYV_TAG_BITS));
}
constexpr uint32_t KEYV_MAX_BYTES = 1u << 20;      // SB_KEY_VAR_MAX_BYTES
// one column of the call, next to its AggCol (sel, rows); the table as KeyCol has it, of reference words
struct KeyVarCol {
    uint8_t* ids;          // as KeyCol.ids
    uint64_t tab0;
    uint32_t tab_mask;
    uint32_t max_keys;
    uint32_t idw;
    uint32_t pad;
    uint64_t keys_cap;     // keys_capacity
};
struct KeyVarState {       // 32 bytes per column, zeroed with the tables before the collect walk
    uint64_t count;
    uint32_t inserted;
    uint32_t overflow;     // collect: the early flag; k_keyv_finish: the SB_KEY_OVERFLOW_* bits
    uint32_t n_keys;
    uint32_t steps;
    uint64_t keys_len;
};
static_assert(sizeof(KeyVarState) == sizeof(KeyState), "read_layout places either behind the call's tables");
// the result of a column: { selected, count, n_keys, overflow, keys_len, 0, 0, 0 }, then kmax + 1 offsets (behind n_keys:
// keys_len), then the keys' bytes in kbytes (the call's largest keys_capacity) rounded up to words
__host__ __device__ inline uint64_t keyv_result_words(uint32_t kmax, uint64_t kbytes) { return 8 + (uint64_t)kmax + 1 + (kbytes + 7) / 8; }
// what k_keyv_finish leaves for the assign walk, per column: KEY_MAX_KEYS pointers, prefixes (8 bytes each) and lengths (4)
constexpr uint64_t KEYV_SORTED_BYTES = (uint64_t)KEY_MAX_KEYS * 20;
// words of the 16-bit id table (an id per dictionary entry) that the call reserves in front of the bit table of
// filter_bin_table_words at the end of a page's aux area: at most L / 8 entries in a page of L bytes
__host__ __device__ inline uint64_t keyv_id_table_words(uint64_t page_len) { return (page_len / 16 + 4) & ~3ull; }
struct KeyVarLaunch {   // what launch_decode needs to end a call with the collect kernels; the finish and assign kernels take it too
    const AggCol* acols;
    const KeyVarCol* kcols;
    KeyVarState* st;       // [n_cols], and behind them the tables: one area, zeroed by launch_keyv_zero
    uint64_t* tabs;
    uint8_t* sorted;       // [n_cols * KEYV_SORTED_BYTES]
    uint64_t zero_bytes;
    uint64_t kbytes;
    uint32_t kmax;
    uint32_t n_cols;
};
// one column of a selected read (sb_read_selected, sb_read_sel.h), next to its ColDesc
constexpr uint32_t RSEL_RANK_BLOCKS = 64;   // workgroups per column of the rank scan (k_rsel_sums / k_rsel_rank)
struct SelCol {
    const uint32_t* sel;   // the selection bitmap (input)
    uint8_t* values;       // the caller's outputs ...
    uint32_t* validity;    // ... (null: not nullable)
    uint64_t* rank;        // [ceil(rows/32) + 1] bits set below each selection word (the last entry: below `rows`), then
                           // RSEL_RANK_BLOCKS block sums
    uint64_t rows;
    uint64_t cap_rows;     // values_capacity / width: output rows the values buffer holds
    uint64_t cap_words;    // validity_capacity / 4
    uint32_t w;            // bytes per value
    uint32_t pad;
};
__host__ __device__ inline uint64_t rsel_rank_words(uint64_t rows) { return (rows + 31) / 32 + 1 + RSEL_RANK_BLOCKS; }
// ... and what a column of sb_read_selected_var (sb_read_sel_bin.h) has beside its SelCol, whose `values` are the
// caller's value bytes, whose cap_rows is offsets_capacity / osize - 1 and whose w is osize
struct SelBin {
    uint8_t* offsets;      // the caller's offsets: selected + 1 entries of osize bytes
    uint64_t* sums;        // RSEL_RANK_BLOCKS block sums of the length scan, then one word (zeroed by the call): the bytes of
                           // the selected rows at and behind cap_rows, which have no offset to be counted through
    uint64_t values_cap;   // values_capacity
    uint32_t osize;        // 4 (Binary) or 8 (LargeBinary)
    uint32_t pad;
};
constexpr uint32_t RSEL_BIN_SUM_WORDS = RSEL_RANK_BLOCKS + 1;
struct SelLaunch {   // what launch_decode needs to end a call with the selected-read kernels
    const SelCol* scols;
    uint64_t* counts;      // [n_cols]: bits set per column
    bool any_nullable;
    const SelBin* bcols = nullptr;   // sb_read_selected_var: one per column (null: sb_read_selected)
    uint64_t* results = nullptr;     // ... [n_cols][2]: { selected, values_len }
};
// one column of an aggregate call (sb_aggregate_columns, sb_aggregate.h), next to its ColDesc.  The kernels write partial
// records (AggPart) into slots of one array of the call: a slot per (page, part of a long RLE page) — the RLE walk and the
// count-only route — and a slot per tile; k_agg_finish combines a column's slots, in slot order, into its result record.
constexpr uint32_t AGG_VALUE_OPS = 2u | 4u | 8u;   // SB_AGG_MIN | SB_AGG_MAX | SB_AGG_SUM: the column's values are looked at
constexpr uint32_t AGG_RESULT_WORDS = 8;           // { selected, count, nans, min, max, sum_lo, sum_hi, the column met a Freq page }
struct AggCol {
    const uint32_t* sel;   // the selection bitmap (input) or null: every row
    uint64_t rows;
    uint64_t page_slot0, page_slots;   // the column's slots in the call's array of partial records
    uint64_t tile_slot0, tile_slots;
    uint32_t ops;          // SB_AGG_*
    uint32_t kind;         // how values order and add: FK_UNSIGNED / FK_SIGNED / FK_F32 / FK_F64
    int32_t ptype;         // the column's physical type (a column without a value op is parsed as SB_TYPE_NULL: no page body is looked at)
    uint32_t w;            // bytes per value
};
struct AggPart {           // 64 bytes; all zero: the slot was not written (a page that failed, a tile without a selected row)
    uint64_t live;         // 1: written; AGG_PART_FREQ: no record, the mark of a Freq page in the slot of its first tile
    uint64_t cnt, nans;    // live rows, NaNs among them
    uint64_t kmin, kmax;   // order keys (agg_key) of the live rows that are not NaN; ~0 / 0: none
    uint64_t s0, s1;       // integers: the 128-bit sum; floats: the bits of the double sum, 0
    uint64_t pad;
};
constexpr uint64_t AGG_PART_FREQ = 2;
struct AggLaunch {   // what launch_decode needs to end a call with the aggregate kernels
    const AggCol* acols;
    AggPart* parts;
    uint64_t tile_base;    // the slot of the call's first tile (the page slots come first)
    bool any_val, any_null;
    bool replayed;         // the call is issued again (a replay): the columns that met a Freq page are not on this route
};
// one column of a grouped aggregate call (sb_aggregate_grouped, sb_aggregate_grouped.h), next to its AggCol.  The slots are
// the AggCol's; a slot holds `gmax` records (the call's largest n_groups), record g of slot s at index s * gmax + g, and a
// flag word says whether the slot was written: the records themselves are never zeroed.
constexpr uint32_t GRP_MAX_GROUPS = 256;           // SB_AGG_MAX_GROUPS
struct GrpCol {
    const uint8_t* ids;    // one unsigned id of `idw` bytes per row of the column (input)
    uint32_t idw;          // 1, 2 or 4
    uint32_t n_groups;     // 1 .. GRP_MAX_GROUPS (sb_aggregate_grouped_large: 1 .. GRPL_MAX_GROUPS)
};
struct GrpPart {           // 64 bytes: a group's share of a slot
    uint64_t sel;          // selected rows of the group, null or not
    uint64_t cnt, nans;    // as in AggPart
    uint64_t kmin, kmax;
    uint64_t s0, s1;
    uint64_t pad;
};
// the result of a column: a header { selected, out_of_range, met a Freq page, 0... } of 8 words, then a record per group in the layout of
// sb_agg_group, `gmax` of them reserved
__host__ __device__ inline uint64_t grp_result_words(uint32_t gmax) { return 8ull * (1 + gmax); }
struct GrpLaunch {   // what launch_decode needs to end a call with the grouped aggregate kernels
    const AggCol* acols;
    const GrpCol* gcols;
    uint64_t* flags;       // [slots]: 1 = the slot's records were written; behind them [n_cols]: rows with an id >= n_groups;
                           // behind those [n_cols]: 1 = the column met a primitive Freq page under a value op
    GrpPart* recs;         // [slots * gmax]
    uint64_t slots;
    uint64_t tile_base;    // the slot of the call's first tile (the page slots come first)
    uint32_t gmax;
    bool any_val, any_null;
    uint32_t n_cols;
    bool replayed;         // the call is issued again: its columns with a Freq page are not on this route (an error if one is)
};
// sb_aggregate_grouped_large (sb_aggregate_grouped_large.h): the same structs with up to GRPL_MAX_GROUPS groups.  Its
// AggCol's tile_slot0 / tile_slots are not a slot per tile but one per CHUNK of GRPL_CHUNK_TILES tiles of the column:
// tile j of the column (its tiles numbered from 0 through its pages, in page order) belongs to chunk j / GRPL_CHUNK_TILES.
constexpr uint32_t GRPL_MAX_GROUPS = 1024;         // SB_AGG_LARGE_MAX_GROUPS (== KEY_MAX_KEYS)
constexpr uint32_t GRPL_CHUNK_TILES = 16;          // 65 536 rows at the most share a table
__host__ __device__ inline uint64_t grpl_chunks(uint64_t tiles) { return (tiles + GRPL_CHUNK_TILES - 1) / GRPL_CHUNK_TILES; }
// The page that holds tile `gt` (numbered through the call, as PageTask::first_tile is) among pages [p0, p0 + n) of one
// column, n > 0, whose first_tile values ascend: the LAST page whose first_tile is <= gt, so that a page without rows,
// which shares its first_tile with the page behind it, is never the answer for a tile that exists.  gt is at least the
// first page's first_tile.  A binary search of ceil(log2(n)) steps.
__host__ __device__ inline uint32_t grpl_page_of(const PageTask* tasks, uint32_t p0, uint32_t n, uint32_t gt) {
    uint32_t lo = 0, hi = n;   // tasks[p0 + lo].first_tile <= gt; hi == n or tasks[p0 + hi].first_tile > gt
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tasks[p0 + mid].first_tile <= gt) lo = mid;
        else hi = mid;
    }
    return p0 + lo;
}
// sb_aggregate_weighted (sb_aggregate_weighted.h): sum(y * w) per group.  The structs, slots and chunks of
// sb_aggregate_grouped_large, and beside a column's AggCol and GrpCol (whose ids are null in the ungrouped form: every
// selected row is in group 0) its weights:
struct WgtCol {
    const uint8_t* w;      // one value of `ww` bytes per row of the column (input); null: the row's own y (SB_WGT_SQUARE)
    const uint8_t* wv;     // the weights' validity, LSB first, or null: every weight is valid
    uint32_t wkind;        // FK_* of the weights
    uint32_t ww;           // bytes per weight
    uint32_t flt;          // 1: either operand is a float, the products are added in double; 0: exact 128-bit products
    uint32_t pad;
};
struct WgtLaunch {   // what launch_decode needs to end a call with the weighted aggregate kernels
    GrpLaunch gl;
    const WgtCol* wcols;
};
// The low 128 bits of x * y, each a 64-bit word that stands for a signed (x_signed: two's complement) or unsigned integer.
// With xu, yu the words read as unsigned: x = xu - 2^64 [x < 0], so x * y = xu * yu - 2^64 ([x < 0] yu + [y < 0] xu) mod 2^128.
__host__ __device__ inline uint64_t wgt_umulhi(uint64_t x, uint64_t y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(x, y);
#else
    const uint64_t x0 = x & 0xFFFFFFFFull, x1 = x >> 32, y0 = y & 0xFFFFFFFFull, y1 = y >> 32;
    const uint64_t p00 = x0 * y0, p01 = x0 * y1, p10 = x1 * y0, p11 = x1 * y1;
    const uint64_t mid = (p00 >> 32) + (p01 & 0xFFFFFFFFull) + (p10 & 0xFFFFFFFFull);   // (< 3 * 2^32: no overflow)
    return p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32);
#endif
}
__host__ __device__ inline void wgt_mul128(uint64_t x, bool x_signed, uint64_t y, bool y_signed, uint64_t& lo, uint64_t& hi) {
    lo = x * y;
    hi = wgt_umulhi(x, y);
    if (x_signed && (x >> 63)) hi -= y;
    if (y_signed && (y >> 63)) hi -= x;
}
// one column of a top-k call (sb_topk_columns, sb_topk.h), next to its AggCol, whose slots it uses.  A slot is a header and
// `kmax` records (the call's largest k), record i of slot s at index s * kmax + i; the headers are zeroed, the records
// are not, and a record is read only below its header's n.
constexpr uint32_t TOPK_MAX_K = 256;               // SB_TOPK_MAX_K
struct TopkCol {
    uint32_t k;            // 1 .. TOPK_MAX_K
    uint32_t largest;      // SB_TOPK_LARGEST: descending by value
};
struct TopkRec {           // smaller (key, row) wins
    uint64_t key;          // the value's order key (agg_key), complemented for `largest`
    uint64_t row;          // the row's number in the column
};
struct TopkHead {          // all zero: the slot was not written
    uint64_t written;
    uint64_t cnt, nans;    // as in AggPart
    uint64_t n;            // records of the slot: its best min(k, cnt - nans)
};
// the result of a column: { selected, count, nans, found, 0, 0, 0, 0 }, then kmax entries in the layout of sb_topk_row,
// of which the column's own k are written
__host__ __device__ inline uint64_t topk_result_words(uint32_t kmax) { return 8 + 2ull * kmax; }
struct TopkLaunch {   // what launch_decode needs to end a call with the top-k kernels
    const AggCol* acols;
    const TopkCol* tcols;
    TopkHead* heads;       // [slots]
    TopkRec* recs;         // [slots * kmax]
    uint64_t slots;
    uint64_t tile_base;    // the slot of the call's first tile (the page slots come first)
    uint32_t kmax;
};
constexpr uint32_t FK_UNSIGNED = 0, FK_SIGNED = 1, FK_F32 = 2, FK_F64 = 3, FK_BYTES = 4;
constexpr uint32_t FILTER_MASK_PREFIX = 16u;   // FilterCol.mask of SB_PRED_STARTS_WITH (the four relation bits are clear)
// ... of SB_PRED_ENDS_WITH, SB_PRED_CONTAINS and, ORed onto one of the three, of the NOT_ forms (sb_filter_sub.h)
constexpr uint32_t FILTER_MASK_SUFFIX = 32u, FILTER_MASK_SUBSTR = 64u, FILTER_MASK_NOT = 128u;
constexpr uint32_t FILTER_MASK_SUB = FILTER_MASK_SUFFIX | FILTER_MASK_SUBSTR | FILTER_MASK_NOT;   // a column of sb_filter_sub.h
// words of the bit table (a bit per dictionary entry) that a filter call reserves at the END of the aux area of every page
// of a binary comparison column: an entry is a u64 length and its bytes, so a page of L bytes has at most L / 8 of them
__host__ __device__ inline uint64_t filter_bin_table_words(uint64_t page_len) { return (page_len / 256 + 4) & ~3ull; }
// one column of a column-against-column call (sb_filter_columns_cmp, sb_filter_cmp.h), next to its FilterCol (sel, kind =
// how y compares, mask, combine).  Nothing of it is written.
struct CmpCol {
    const uint8_t* other;   // one value of `ow` bytes per row of the column (input)
    const uint32_t* ov;     // the operands' validity, LSB first in 32-bit words, or null: every operand is valid
    uint32_t okind;         // FK_* of the operands
    uint32_t ow;            // bytes per operand
};
// The relation of y to o (0 less, 1 equal, 2 greater, 3 unordered), whose bit of FilterCol.mask is the row's result.  The
// host's and the device's alike (tests/test_filter_cmp_host.py runs them on the edge values of every type pair).
// Integers: each word extended by its own signedness; where the signs differ the negative one is below, where they agree
// the words order as unsigned ones do (two's complement keeps the order of two negatives).
__host__ __device__ inline uint64_t cmp_ext(bool is_signed, uint32_t w, uint64_t raw) {
    const uint32_t sh = 64 - 8 * w;
    return is_signed ? (uint64_t)((int64_t)(raw << sh) >> sh) : raw;
}
__host__ __device__ inline uint32_t cmp_rel_int(uint64_t y, bool y_signed, uint64_t o, bool o_signed) {
    const bool yn = y_signed && (y >> 63), on = o_signed && (o >> 63);
    const uint32_t r = y < o ? 0u : y == o ? 1u : 2u;
    return yn != on ? (yn ? 0u : 2u) : r;
}
// a value of kind K (FK_*) as a double: integers round to nearest even
template <uint32_t K>
__host__ __device__ inline double cmp_dbl(uint32_t w, uint64_t raw) {
    if (K == FK_F32) return (double)__builtin_bit_cast(float, (uint32_t)raw);
    if (K == FK_F64) return __builtin_bit_cast(double, raw);
    if (K == FK_SIGNED) return (double)(int64_t)cmp_ext(true, w, raw);
    return (double)raw;
}
__host__ __device__ inline uint32_t cmp_rel_dbl(double y, double o) { return y < o ? 0u : y == o ? 1u : y > o ? 2u : 3u; }
// y (kind YK, yw bytes) against o (kind OK, ow bytes): a pair of integers exactly, any pair with a float as doubles
template <uint32_t YK, uint32_t OK>
__host__ __device__ inline uint32_t cmp_rel(uint32_t yw, uint64_t y, uint32_t ow, uint64_t o) {
    if (YK <= FK_SIGNED && OK <= FK_SIGNED) return cmp_rel_int(cmp_ext(YK == FK_SIGNED, yw, y), YK == FK_SIGNED, cmp_ext(OK == FK_SIGNED, ow, o), OK == FK_SIGNED);
    return cmp_rel_dbl(cmp_dbl<YK>(yw, y), cmp_dbl<OK>(ow, o));
}
// the type pair resolved once, outside the loops over rows: f(integral_constant yk, integral_constant ok)
template <uint32_t YK, class F>
__host__ __device__ __forceinline__ void cmp_pair_o(uint32_t okind, F&& f) {
    switch (okind) {
        case FK_UNSIGNED: f(std::integral_constant<uint32_t, YK>{}, std::integral_constant<uint32_t, FK_UNSIGNED>{}); break;
        case FK_SIGNED: f(std::integral_constant<uint32_t, YK>{}, std::integral_constant<uint32_t, FK_SIGNED>{}); break;
        case FK_F32: f(std::integral_constant<uint32_t, YK>{}, std::integral_constant<uint32_t, FK_F32>{}); break;
        default: f(std::integral_constant<uint32_t, YK>{}, std::integral_constant<uint32_t, FK_F64>{}); break;
    }
}
template <class F>
__host__ __device__ __forceinline__ void cmp_pair(uint32_t ykind, uint32_t okind, F&& f) {
    switch (ykind) {
        case FK_UNSIGNED: cmp_pair_o<FK_UNSIGNED>(okind, f); break;
        case FK_SIGNED: cmp_pair_o<FK_SIGNED>(okind, f); break;
        case FK_F32: cmp_pair_o<FK_F32>(okind, f); break;
        default: cmp_pair_o<FK_F64>(okind, f); break;
    }
}
constexpr uint32_t LZ4_BIG_MIN = 64u << 10;
constexpr uint32_t RSKIP_QUEUE_A = 1u, RSKIP_TILES = 2u;   // k_zstd_split + k_inflate + k_inflate_lz4 of queue A / k_expand

}  // namespace sb

// ------------------------------------------------------------------ device helpers
#if defined(__HIPCC__)
namespace sb {

// unaligned little-endian loads: page bytes sit at arbitrary byte offsets (9-byte headers,
// def-level sections); gfx950 global loads handle unaligned addresses in hardware.
// All page bytes and Arrow buffers live in HBM: casting to the global address space makes the
// compiler emit global_load/global_store instead of flat_* (pointers read from descriptor tables
// are otherwise "generic", and flat accesses tie up the LDS counter as well).
typedef __attribute__((address_space(1))) const uint8_t* gcptr;
typedef __attribute__((address_space(1))) uint8_t* gptr;
__device__ __forceinline__ uint8_t ldu8(const uint8_t* p) { return *(gcptr)p; }
__device__ __forceinline__ uint16_t ldu16(const uint8_t* p) {
    uint16_t v;
    __builtin_memcpy(&v, (gcptr)p, 2);
    return v;
}
__device__ __forceinline__ uint32_t ldu32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, (gcptr)p, 4);
    return v;
}
__device__ __forceinline__ uint64_t ldu64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, (gcptr)p, 8);
    return v;
}
// aligned u32 / u64 accesses to HBM through generic pointers (workspace arrays handed around as plain pointers): the
// cast makes them global_load / global_store — a flat access also counts on lgkmcnt, so every wait for an LDS result
// would wait for the outstanding HBM accesses too and nothing overlaps
typedef __attribute__((address_space(1))) const uint32_t* gc32p;
typedef __attribute__((address_space(1))) uint32_t* g32p;
typedef __attribute__((address_space(1))) const uint64_t* gc64p;
typedef __attribute__((address_space(1))) uint64_t* g64p;
typedef __attribute__((address_space(3))) uint32_t* l32p;
__device__ __forceinline__ uint32_t gld32(const uint32_t* p) { return *(gc32p)p; }
__device__ __forceinline__ void gst32(uint32_t* p, uint32_t v) { *(g32p)p = v; }
__device__ __forceinline__ uint64_t gld64(const uint64_t* p) { return *(gc64p)p; }
__device__ __forceinline__ void gst64(uint64_t* p, uint64_t v) { *(g64p)p = v; }
// A table of u32 slots that lives in LDS or in HBM (chosen at run time): every access names its address space.
struct SlotTable {
    uint32_t* p;
    bool in_lds;
    __device__ __forceinline__ uint32_t ld(uint32_t h) const {
        return in_lds ? *((l32p)p + h) : __hip_atomic_load((g32p)p + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void st(uint32_t h, uint32_t v) const {
        if (in_lds) *((l32p)p + h) = v;
        else *((g32p)p + h) = v;
    }
    // returns the value found (== cmp: the slot now holds val)
    __device__ __forceinline__ uint32_t cas(uint32_t h, uint32_t cmp, uint32_t val) const {
        uint32_t e = cmp;
        if (in_lds)
            __hip_atomic_compare_exchange_strong((l32p)p + h, &e, val, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else
            __hip_atomic_compare_exchange_strong((g32p)p + h, &e, val, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return e;
    }
    __device__ __forceinline__ void amin(uint32_t h, uint32_t v) const {
        if (in_lds) __hip_atomic_fetch_min((l32p)p + h, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_fetch_min((g32p)p + h, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};
__device__ __forceinline__ void stu32(uint8_t* p, uint32_t v) { __builtin_memcpy((gptr)p, &v, 4); }
__device__ __forceinline__ void stu64(uint8_t* p, uint64_t v) { __builtin_memcpy((gptr)p, &v, 8); }

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
struct __attribute__((packed, aligned(1))) U16B {
    u32x4 v;
};
__device__ __forceinline__ u32x4 ldu128(const uint8_t* p) {
    u32x4 v;
    __builtin_memcpy(&v, (gcptr)p, 16);
    return v;
}
__device__ __forceinline__ void stu128(uint8_t* p, u32x4 v) { __builtin_memcpy((gptr)p, &v, 16); }

// value of W bytes as a register bundle
template <int W>
struct Val;
template <>
struct Val<1> {
    uint8_t x;
};
template <>
struct Val<2> {
    uint16_t x;
};
template <>
struct Val<4> {
    uint32_t x;
};
template <>
struct Val<8> {
    uint64_t x;
};
template <>
struct Val<16> {
    u32x4 x;
};
template <>
struct Val<32> {
    u32x4 x, y;
};
template <int W>
__device__ __forceinline__ Val<W> ld_val(const uint8_t* p) {  // unaligned
    Val<W> v;
    __builtin_memcpy(&v, (gcptr)p, W);
    return v;
}
template <int W>
__device__ __forceinline__ void st_val(uint8_t* p, Val<W> v) {  // p aligned to min(W,16)
    __builtin_memcpy((gptr)p, &v, W);
}

__device__ __forceinline__ void raise(Status* st, int32_t code, uint32_t page, uint32_t where) {
    if (atomicCAS(&st->code, 0, code) == 0) {
        st->page = page;
        st->where = where;
    }
}

// padded index into a TILE_ROWS-entry LDS array: one pad word per 16 entries so that a
// thread owning 16 consecutive entries (the scan layout) hits distinct banks
__device__ __forceinline__ int sidx(int i) { return i + (i >> 4); }
constexpr int SIDX_WORDS = TILE_ROWS + TILE_ROWS / 16;

// wave64 inclusive scan (u32 wrapping add)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_incl_scan64(uint64_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint64_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// exclusive scan on top of `carry` (wave-uniform), which leaves with the wave's total added: one step of a scan that a wave
// makes 64 entries at a time
__device__ __forceinline__ uint64_t wave_excl_scan64(uint64_t v, uint64_t& carry) {
    const uint64_t incl = wave_incl_scan64(v);
    const uint64_t excl = carry + incl - v;
    carry += __shfl(incl, 63, 64);
    return excl;
}

// Inclusive scan of the TILE_ROWS u32 entries of `a` (sidx layout), in place.  Thread t owns
// entries [16t, 16t+16).  `wsum` is a 4-entry LDS scratch.  Returns the tile total.
__device__ __forceinline__ uint32_t tile_incl_scan(uint32_t* a, uint32_t* wsum) {
    const int t = threadIdx.x;
    uint32_t loc[ROWS_PER_THREAD];
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD; j++) {
        run += a[sidx(t * ROWS_PER_THREAD + j)];
        loc[j] = run;
    }
    uint32_t incl = wave_incl_scan(run);
    if ((t & 63) == 63) wsum[t >> 6] = incl;
    __syncthreads();
    uint32_t base = incl - run;
    const int w = t >> 6;
    uint32_t w0 = wsum[0], w1 = wsum[1], w2 = wsum[2], w3 = wsum[3];
    if (w > 0) base += w0;
    if (w > 1) base += w1;
    if (w > 2) base += w2;
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD; j++) a[sidx(t * ROWS_PER_THREAD + j)] = base + loc[j];
    __syncthreads();
    return w0 + w1 + w2 + w3;
}

// inclusive max-scan over the TILE_ROWS entries of `a` (sidx layout), in place
__device__ __forceinline__ void tile_incl_scan_max(uint32_t* a, uint32_t* wsum) {
    const int t = threadIdx.x;
    uint32_t loc[ROWS_PER_THREAD];
    uint32_t run = 0;
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD; j++) {
        run = max(run, a[sidx(t * ROWS_PER_THREAD + j)]);
        loc[j] = run;
    }
    uint32_t incl = run;
    const int lane = t & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t o = __shfl_up(incl, d, 64);
        if (lane >= d) incl = max(incl, o);
    }
    uint32_t excl = __shfl_up(incl, 1, 64);
    if (lane == 0) excl = 0;
    __syncthreads();
    if (lane == 63) wsum[t >> 6] = incl;
    __syncthreads();
    const int w = t >> 6;
    uint32_t base = excl;
    if (w > 0) base = max(base, wsum[0]);
    if (w > 1) base = max(base, wsum[1]);
    if (w > 2) base = max(base, wsum[2]);
#pragma unroll
    for (int j = 0; j < ROWS_PER_THREAD; j++) a[sidx(t * ROWS_PER_THREAD + j)] = max(base, loc[j]);
    __syncthreads();
}

// workgroup sum of one u32 / u64 per thread
__device__ __forceinline__ uint64_t wg_sum64(uint64_t v, uint64_t* wsum4) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) wsum4[threadIdx.x >> 6] = v;
    __syncthreads();
    return wsum4[0] + wsum4[1] + wsum4[2] + wsum4[3];
}

// BitPacker4x geometry: value j of a 128-block lives in lane (j&3) at slot (j>>2);
// slot i of width nb starts at bit i*nb of the lane's stream; word k of lane l is the
// u32 at index 4k+l of the block payload.
__device__ __forceinline__ uint32_t bp4x_extract(const uint8_t* payload, uint32_t nb, int j) {
    if (nb == 0) return 0;
    const int l = j & 3, i = j >> 2;
    const uint32_t bitpos = (uint32_t)i * nb, word = bitpos >> 5, sh = bitpos & 31;
    uint32_t v = ldu32(payload + 4 * (4 * word + l)) >> sh;
    if (sh + nb > 32) v |= ldu32(payload + 4 * (4 * (word + 1) + l)) << (32 - sh);
    if (nb < 32) v &= (1u << nb) - 1;
    return v;
}

}  // namespace sb
#endif
