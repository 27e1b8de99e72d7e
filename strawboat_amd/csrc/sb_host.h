// strawboat-hip: host-side context (workspace, staging ring, error plumbing).
#pragma once
#include <string>
#include <algorithm>
#include <deque>
#include <vector>

#include "sb_common.h"

namespace sb {

struct DevBuf {
    uint8_t* p = nullptr;
    size_t cap = 0;
};

// pinned host staging slot: uploads (tables) and readbacks (status, sizes, metas)
struct StageSlot {
    uint8_t* host = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool in_flight = false;
};

// A result to hand back to the caller's structs at synchronize (sb_api.hip: deliver_pending), read back into pinned memory:
//   kind        user                          host                                        n               bytes
//   READ_COL    sb_column_read*               8 bytes: values_len                         0               -
//   FILTER_COL  the caller's `selected`       8 bytes: the bits set                       0               -
//   RSEL_COL    sb_column_read_selected*      8 bytes: the bits set (values_len follows)  0               -
//   RSEL_VAR_COL sb_column_read_selected_var* 16 bytes: the bits set, values_len          0               -
//   AGG_COL     sb_column_aggregate*          64 bytes: the result record (AGG_RESULT_WORDS; word 7: the column met a Freq page)  0   -
//   AGG_GRP_COL sb_column_aggregate_grouped*  64 bytes { selected, out_of_range }, then 64 per group  0       of header + groups
//   AGG_GRPL_COL  the same, of an sb_aggregate_grouped_large call (a kind of its own: the Freq marks of the two calls are kept apart)
//   AGG_WGT_COL sb_column_aggregate_weighted*  the same record, of an sb_aggregate_weighted call (its own struct, its own Freq marks)
//   TOPK_COL    sb_column_topk*               64 bytes { selected, count, nans, found }, then 16 per entry of `out`  0   of header + kmax entries
//   KEY_COL     sb_column_key_ids*            64 bytes { selected, count, n_keys, overflow }, then 8 per slot of `keys`  0   of header + kmax slots
//   KEY_VAR_COL sb_column_key_ids_var*        64 bytes { selected, count, n_keys, overflow, keys_len }, then kmax + 1 offsets, then the keys' bytes  0   of the record
//   KEY_LOOK_COL sb_column_key_lookup*        32 bytes { selected, count, matched, 0 }    0               -
//   KEY_BUCKET_COL sb_column_key_buckets*     32 bytes { selected, count, matched, nans } 0               -
//   FILTER_CMP_COL the caller's `selected`    8 bytes: the bits set (sb_filter_columns_cmp) 0             -
//   COMB_ITEM   sb_key_combine_item*          64 bytes { rows, live, n_keys, overflow }, then 8 per sorted code (unpacked into `tuples`)  0   of header + kmax codes
//   WRITE_COL   sb_column_write*              u64 [n lengths][n num_values][out_len]      pages           -
//   ENC_HINT    null                          32 words: pages per codec of a write call   the plan's key  -
//   NESTED_W    sb_nested_levels_write[n]     the page records of an enqueued level call  items           of the records
//   NESTED_R    sb_nested_levels_read[n]      the page records of an enqueued level call  items           of the records
// (acquire_slot sizes what it moves out of a recycled slot by this table)
struct Pending {
    enum Kind { READ_COL, WRITE_COL, ENC_HINT, NESTED_W, NESTED_R, FILTER_COL, RSEL_COL, RSEL_VAR_COL, AGG_COL, AGG_GRP_COL, AGG_GRPL_COL, TOPK_COL, KEY_COL, KEY_VAR_COL, COMB_ITEM, KEY_LOOK_COL, AGG_WGT_COL, KEY_BUCKET_COL, FILTER_CMP_COL } kind;
    void* user;
    const uint8_t* host;
    uint64_t n;
    uint64_t bytes = 0;
};

enum KernelId {
    K_PARSE, K_INFLATE_A, K_PLAN, K_COLSCAN, K_INFLATE_B, K_EXPAND, K_EXPAND_BIN,
    K_ENC_TILES, K_ENC_PAGES, K_ENC_LAYOUT, K_ENC_COMPACT, K_ENC_SELECT, K_ENC_LZ4,
    K_ENC_PAGES_DICT, K_ENC_PAGES_ONEVALUE, K_ENC_PAGES_BP, K_EXPAND_RLE, K_ENC_PAGES_PATAS, K_ENC_FREQ, K_ENC_SELECT_ROWS, K_COUNT
};
struct ProfSpan {
    int id;
    hipEvent_t a, b;
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// bytes per value (binary types: per offset; Boolean and Null: 0)
inline uint32_t type_width(int32_t t) {
    switch (t) {
        case SB_TYPE_INT8:
        case SB_TYPE_UINT8:
            return 1;
        case SB_TYPE_INT16:
        case SB_TYPE_UINT16:
            return 2;
        case SB_TYPE_INT32:
        case SB_TYPE_UINT32:
        case SB_TYPE_FLOAT32:
        case SB_TYPE_BINARY:
            return 4;
        case SB_TYPE_INT64:
        case SB_TYPE_UINT64:
        case SB_TYPE_FLOAT64:
        case SB_TYPE_LARGE_BINARY:
            return 8;
        case SB_TYPE_INT128:
            return 16;
        case SB_TYPE_INT256:
            return 32;
    }
    return 0;
}
inline bool is_binary_t(int32_t t) { return t == SB_TYPE_BINARY || t == SB_TYPE_LARGE_BINARY; }

}  // namespace sb

struct sb_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string last_error;

    int lzg_state = 0;        // sb_lz4_giant.h: 0 = not known yet, 1 = this context meets LZ4 blocks of megabytes, 2 = it does not
    bool lzg_long_pages = false;   // a call since the last synchronize had pages long enough
    uint32_t lzg_idle = 0;         // intervals in a row with long pages and no LZ4 block of megabytes
    sb::DevBuf lzg_pool;   // sb_lz4_giant.h: tables and entries of LZ4 blocks of megabytes
    sb::DevBuf tables;   // ColDesc / PageTask / PageDesc / TileTask / jobs / counters
    sb::DevBuf scratch;  // per-page aux + inflate areas, encode slots
    sb::DevBuf staging;  // device staging for SB_MEM_HOST callers
    sb::DevBuf combine;  // sb_key_combine: the call's descriptors, results, states, tables and sorted codes
    sb::DevBuf filter_stage;   // sb_filter_columns: where the inflate queues put the values of LZ4 / Zstd / Snappy / Patas pages (no caller's buffer to inflate into)
    std::vector<const void*> agg_freq_users;   // ... the same for the sb_column_aggregate structs of sb_aggregate_columns calls
    std::vector<const void*> wgt_freq_users;   // ... the same for the columns of sb_aggregate_weighted calls
    std::vector<const void*> grpl_freq_users;  // ... the same for the columns of sb_aggregate_grouped_large calls
    std::vector<const void*> grp_freq_users;   // during a replay: the sb_column_aggregate_grouped structs whose column met a Freq page in the first pass
    bool filter_freq = false;  // replay of an interval in which a filter or selected-read call met a Freq page: such calls decode into filter_stage first
    sb::DevBuf zlit;     // Zstd literal buffers (fixed pool of inflate waves)
    sb::DevBuf zrec;     // Zstd sequence records (one arena per inflate wave; allocated by the first batch-sized read)
    sb::Status* d_status = nullptr;
    sb::Status* h_status = nullptr;  // pinned
    // the block-parallel Zstd pipeline (sb_zstd_blocks.h): pools sized per call once the context has met Zstd pages
    // (Status.kinds, read back at every synchronize); SB_ZSTD_BLOCKS = 0 / 1 in the environment forces it off / on
    sb::DevBuf zb_blocks, zb_lit, zb_rec;
    unsigned long long* zb_stats = nullptr;   // device: sb_ctx_zstd_block_stats
    uint32_t kinds_seen = 0;
    bool zstd_recent = false;   // the read calls of the last synchronize interval met a Zstd buffer
    uint32_t read_calls = 0;     // read calls since the last synchronize
    uint32_t qa_idle = 0, tiles_idle = 0;   // read intervals in a row that queued no inflate job for queue A / no tile task: from two
                                            // on the next read calls leave those kernels out (a reader that alternates column kinds keeps them)
    uint32_t zstd_idle = 0;      // read intervals in a row that met no Zstd buffer
    bool zb_seq_long = false;    // the last Zstd calls held blocks of >= 8192 sequences: zb_seq is submitted before zb_lit
    int zb_mode = 2;             // 0 off, 1 always, 2 once Zstd has been seen
    uint32_t zb_wg_exec = 1;     // SB_ZSTD_BLOCKS_WG=0: frames of many short sequences through the wave executor too
    uint32_t zb_pool_div = 1;    // SB_ZSTD_BLOCKS_POOL_DIV (tests): pool estimates divided by this
    uint32_t zb_min_csize = 0;   // SB_ZSTD_BLOCKS_MIN: frames shorter than this keep the one-wave / lane-per-frame paths

    static constexpr int NSLOTS = 8;
    sb::StageSlot slots[NSLOTS];
    int next_slot = 0;
    size_t slot_cap_max = 0;                // largest staging request so far: a slot that grows, grows to this

    // SB_MEM_HOST copies to hand back after the stream drains: (host dst, device src, bytes)
    struct Copyback {
        void* host;
        const void* dev;
        size_t n;
        const uint64_t* used = nullptr;  // when set: only the first min(n, *used) bytes are copied (pages: out_len)
        bool issued = false;             // already on its way (copy stream): a call of many columns is cut into groups whose
                                         // copies back overlap the next group's copies in — the link's two directions are independent
    };
    uint32_t host_groups_max = 8;        // SB_HOST_GROUPS (1: SB_MEM_HOST calls are never cut into groups)
    hipStream_t copy_stream = nullptr;   // D2H copies of SB_MEM_HOST calls
    std::vector<hipEvent_t> pipe_ev;     // "group's kernels done" events (iv.pipe_ev_used of them belong to the open interval)
    hipEvent_t next_pipe_event() {
        if (iv.pipe_ev_used == pipe_ev.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return nullptr;
            pipe_ev.push_back(e);
        }
        return pipe_ev[iv.pipe_ev_used++];
    }
    hipStream_t copy_stream_get() {
        if (!copy_stream && hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking) != hipSuccess) copy_stream = nullptr;
        return copy_stream;
    }
    // SB_MEM_HOST staging areas: carved out of chunks that stay allocated (hipMalloc / hipFree per buffer and call
    // cost more than the PCIe copies); every carve-out lives until the next synchronize, which rewinds the chunks
    struct StageChunk {
        uint8_t* p;
        size_t cap, used;
    };
    std::vector<StageChunk> stage_chunks;
    size_t stage_hint = 0;  // capacity of the set of chunks that was last merged
    uint8_t* stage_alloc(size_t bytes) {
        bytes = (bytes + 64 + 255) & ~(size_t)255;
        for (auto& c : stage_chunks)
            if (c.cap - c.used >= bytes) {
                uint8_t* r = c.p + c.used;
                c.used += bytes;
                return r;
            }
        size_t total = 0;
        for (auto& c : stage_chunks) total += c.cap;
        const size_t cap = std::max<size_t>(std::max<size_t>(bytes, stage_hint), std::max<size_t>(total, (size_t)256 << 20));  // doubling growth
        uint8_t* p = nullptr;
        if (hipMalloc((void**)&p, cap) != hipSuccess) return nullptr;
        stage_chunks.push_back({p, cap, bytes});
        return p;
    }
    void stage_rewind() {  // after the stream has drained: one chunk of the total size replaces a fragmented set
        if (stage_chunks.size() > 2) {
            stage_hint = 0;
            for (auto& c : stage_chunks) {
                stage_hint += c.cap;
                (void)hipFree(c.p);
            }
            stage_chunks.clear();
        }
        for (auto& c : stage_chunks) c.used = 0;
    }
    void stage_release() {
        for (auto& c : stage_chunks) (void)hipFree(c.p);
        stage_chunks.clear();
    }
    // Freq pages logged by the decode calls since the last synchronize: [u32 count | pad][FreqEntry...]
    struct FreqLog {
        uint8_t* dev = nullptr;
        uint32_t cap = 0, reserved = 0;
    };
    std::vector<FreqLog> freq_logs;

    // optional per-kernel HIP-event timing (sb_ctx_profile)
    bool profile = false;
    std::vector<hipEvent_t> free_events;
    // The page table of the last write call (sb_write_columns): page arithmetic, scratch layout and launch shape depend only
    // on the columns' types, row counts, paging and the options — not on their buffers — so a writer that sends chunk after
    // chunk of one schema (or a benchmark that repeats a call) re-uses the device-resident table and the plan instead of
    // building and uploading ~170 bytes per page again (65 536 pages of 8192 booleans: 2 ms of host work per call).
    struct EncPlan {
        bool valid = false;
        uint64_t key = 0, n = 0;
        uint64_t P = 0, max_tiles = 1, max_chunks = 1, lz_cap = 0, lz_chunk = 0;
        bool any_tiles = false, any_pages = false, any_compact = false, any_lz4 = false;
        size_t scratch_total = 0, lz_pool_off = 0, zpar_off = 0;
        std::vector<uint64_t> key_words;   // the words the key was hashed from (compared on a hit)
        std::vector<uint32_t> col_first, col_pages;
        std::vector<uint64_t> hro;
        sb::DevBuf pages;   // EncPage[P] on the device
        // long pages of 4- / 8-byte values (adaptive calls): selected section-parallel (sb_select_big.h); page indices on
        // the device as [1-byte | 2-byte | 4-byte | 8-byte pages], grid.x = the most sections any page of a width has
        std::vector<uint32_t> bigw[5];          // by log2(width): 1-, 2-, 4-, 8-byte values; [4]: binary pages
        uint32_t big_secs[5] = {0, 0, 0, 0, 0};
        sb::DevBuf big;
        // pages per codec the last TWO completed calls with this plan chose (element-wise maximum; read back with the results):
        // a call leaves out the launches neither of them needed — a page that needs one after all stays unwritten and the
        // interval is replayed (k_enc_layout, sb_ctx_synchronize).  Two calls, not one: a writer that alternates two kinds
        // of data under one plan keeps the kernels of both instead of replaying every other call.
        uint32_t last_counts[32] = {0}, prev_counts[32] = {0};
        bool counts_valid = false;
        // binary pages of an adaptive call: any of them, and any that k_enc_bin_page (sb_bin_page.h) does not take (too
        // short / long): only those still need the hash -> select -> verify chain
        bool bin_pages = false, bin_unfused = false;
    } enc_plan;
    // Calls of the open synchronize interval, kept so that they can be issued again: kernels whose work the last calls did
    // not need are skipped on that hint (the long-page Dict / Freq chains, the block-parallel LZ4 reader, emitters of
    // codecs nobody chose); a page that needed one after all is left undone, the device says so (KIND_REPLAY) and
    // sb_ctx_synchronize re-issues the interval's calls with every kernel launched — a wrong guess costs one extra pass,
    // never a one-workgroup walk over a million-row page.  (The callers' column arrays and buffers live until the
    // synchronize anyway: the results are written into them there.)
    struct Call {
        enum Kind { READ, WRITE, FILTER, FILTER_VAR, FILTER_IN, READ_SEL, READ_SEL_VAR, AGGREGATE, AGG_GROUPED, AGG_GROUPED_LARGE, TOPK, KEY_IDS, KEY_IDS_VAR, KEY_COMBINE, SIZES, KEY_LOOKUP, AGG_WEIGHTED, KEY_BUCKETS, FILTER_CMP } kind;   // sb_read_columns, sb_write_columns, sb_filter_columns, sb_filter_columns_var, sb_filter_columns_in, sb_read_selected, sb_read_selected_var, sb_aggregate_columns, sb_aggregate_grouped, sb_aggregate_grouped_large, sb_topk_columns, sb_key_ids, sb_key_ids_var, sb_key_combine, sb_read_columns_sizes (its enqueue: the call's own synchronize may be the one that replays), sb_key_lookup, sb_aggregate_weighted, sb_key_buckets, sb_filter_columns_cmp
        void* cols;
        uint64_t n;
        sb_write_options opts;
        int32_t mem;
    };
    // The open synchronize interval: everything that lives from the first enqueue after a synchronize to the end of the next
    // one.  reset() is the only place that ends these lifetimes, and it resets nothing else; what survives intervals on
    // purpose (the hint counters with read_calls / lzg_long_pages, which update_read_hints consumes; enc_plan; the pools;
    // free_events; pipe_ev; the Freq logs' buffers) stays outside.
    struct Interval {
        int32_t sticky = 0;                        // first host-side error since the last synchronize
        std::vector<Call> calls;                   // (above)
        std::vector<sb::Pending> pending;
        std::deque<std::vector<uint8_t>> rescued;  // readbacks moved out of a recycled staging slot (acquire_slot) or kept for a replay
        std::vector<Copyback> copybacks;
        std::vector<void*> temp_dev;               // device temporaries
        std::vector<void*> stale_host;             // outgrown staging buffers (hipHostFree drains the device: not inside an enqueue)
        std::deque<std::vector<sb_column_read>> filter_tmp;   // the read columns of a filter replay's decodes (filter_freq)
        size_t pipe_ev_used = 0;
        sb::StageSlot* last_slot = nullptr;        // the staging slot of the last enqueued write call (its `done` event = results are back)
        bool freq_pass_ran = false;                // this synchronize ran the Freq second pass (copies issued early are repeated)
        std::vector<sb_column_read> freq_cols;     // the second pass's one-page columns (their READ_COL pendings point here)
        std::vector<sb_page_meta> freq_metas;
        std::vector<sb::ProfSpan> spans;           // (sb_ctx_profile) the launches to time; recycle_spans hands their events back

        // END: the interval is over, its results are delivered.  REPLAY: its calls are about to be issued again (the caller has
        // taken `calls` out): the page records of enqueued level calls stay pending, because those calls are not issued again
        // -- copied into `rescued`, since the staging slots are free to be reused -- and every other pending result is dropped;
        // `rescued` therefore stays too.  That is the whole difference.  (sticky is 0 in a replay: an interval that failed on the
        // host is not replayed.)  Called with the stream and the copy stream drained.
        enum Reset { END, REPLAY };
        void reset(Reset how) {
            if (how == REPLAY) {
                std::vector<sb::Pending> keep;
                for (auto& p : pending)
                    if (p.kind == sb::Pending::NESTED_W || p.kind == sb::Pending::NESTED_R) {
                        rescued.emplace_back(p.host, p.host + p.bytes);
                        p.host = rescued.back().data();
                        keep.push_back(p);
                    }
                pending.swap(keep);
            } else {
                pending.clear();
                rescued.clear();
            }
            sticky = 0;
            calls.clear();
            for (void* p : stale_host) (void)hipHostFree(p);
            stale_host.clear();
            copybacks.clear();
            pipe_ev_used = 0;
            for (void* p : temp_dev) (void)hipFree(p);
            temp_dev.clear();
            filter_tmp.clear();
            last_slot = nullptr;
            freq_pass_ran = false;
            freq_cols.clear();
            freq_metas.clear();
            spans.clear();   // (empty already: recycle_spans has handed the events back)
        }
    } iv;
    bool no_hints = false, in_replay = false;   // no_hints: SB_NO_HINTS=1, and during a replay
    uint64_t replays = 0;                       // sb_ctx_replays
    bool bin_fused = true;   // SB_BIN_FUSED=0: binary pages through the round-3 chain (A/B measurements, tests)
    std::vector<uint64_t> enc_plan_probe;   // the key words of the call at hand
    // side streams: kernels of a call that work on disjoint pages (the selector / emit chains of different column kinds, the
    // three expand kernels of a read) run side by side between a fork and a join on `stream`; seen from outside the call is
    // still one span of work on `stream`.  Not used while profiling (the per-kernel events bracket launches on `stream`).
    static constexpr int NSIDE = 3;
    hipStream_t side[NSIDE] = {nullptr, nullptr, nullptr};
    hipEvent_t fork_ev = nullptr, join_ev[NSIDE] = {nullptr, nullptr, nullptr};
    uint64_t side_forks = 0;   // calls whose kernels ran on side streams next to the call's stream (sb_ctx_side_forks)
    bool side_ready = false;
    struct ProfEntry {
        std::string name;  // the kernel's name as rocprofv3 prints it, without "void sb::" and the argument list
        double ms = 0;
        uint64_t n = 0;
    };
    std::vector<ProfEntry> prof;  // [0, K_COUNT): the KernelId entries; template instances are added by name
    int prof_id(const char* name) {
        for (size_t i = 0; i < prof.size(); i++)
            if (prof[i].name == name) return (int)i;
        ProfEntry e;
        e.name = name;
        prof.push_back(e);
        return (int)prof.size() - 1;
    }

    int32_t fail(int32_t code, const std::string& msg) {
        last_error = msg;
        if (!iv.sticky) iv.sticky = code;
        return code;
    }
};

// the enqueue of sb_read_columns_sizes without its synchronize (sb_api.hip)
int32_t enqueue_read_sizes(sb_ctx* ctx, sb_column_read* cols, uint64_t n, int32_t mem);

// issues a call of the interval again (a replay: sb_api.hip, replay_interval)
inline int32_t reissue(sb_ctx* ctx, sb_ctx::Call& cl) {
    switch (cl.kind) {
        case sb_ctx::Call::SIZES: return enqueue_read_sizes(ctx, (sb_column_read*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::READ: return sb_read_columns(ctx, (sb_column_read*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::WRITE: return sb_write_columns(ctx, (sb_column_write*)cl.cols, cl.n, &cl.opts, cl.mem);
        case sb_ctx::Call::FILTER: return sb_filter_columns(ctx, (sb_column_filter*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::FILTER_VAR: return sb_filter_columns_var(ctx, (sb_column_filter_var*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::FILTER_IN: return sb_filter_columns_in(ctx, (sb_column_filter_in*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::READ_SEL: return sb_read_selected(ctx, (sb_column_read_selected*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::READ_SEL_VAR: return sb_read_selected_var(ctx, (sb_column_read_selected_var*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::AGGREGATE: return sb_aggregate_columns(ctx, (sb_column_aggregate*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::AGG_GROUPED: return sb_aggregate_grouped(ctx, (sb_column_aggregate_grouped*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::AGG_GROUPED_LARGE: return sb_aggregate_grouped_large(ctx, (sb_column_aggregate_grouped*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::AGG_WEIGHTED: return sb_aggregate_weighted(ctx, (sb_column_aggregate_weighted*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::TOPK: return sb_topk_columns(ctx, (sb_column_topk*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::KEY_IDS: return sb_key_ids(ctx, (sb_column_key_ids*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::KEY_IDS_VAR: return sb_key_ids_var(ctx, (sb_column_key_ids_var*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::KEY_COMBINE: return sb_key_combine(ctx, (sb_key_combine_item*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::KEY_LOOKUP: return sb_key_lookup(ctx, (sb_column_key_lookup*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::KEY_BUCKETS: return sb_key_buckets(ctx, (sb_column_key_buckets*)cl.cols, cl.n, cl.mem);
        case sb_ctx::Call::FILTER_CMP: return sb_filter_columns_cmp(ctx, (sb_column_filter_cmp*)cl.cols, cl.n, cl.mem);
    }
    return SB_ERR_INVALID;
}

namespace sb {
// brackets one kernel launch with events when profiling is on
struct KScope {
    sb_ctx* ctx;
    ProfSpan sp;
    KScope(sb_ctx* c, const char* name) : KScope(c, c->profile ? c->prof_id(name) : 0) {}
    KScope(sb_ctx* c, int id) : ctx(c) {
        if (!ctx->profile) return;
        sp.id = id;
        auto get = [&]() {
            hipEvent_t e;
            if (!ctx->free_events.empty()) {
                e = ctx->free_events.back();
                ctx->free_events.pop_back();
            } else {
                (void)hipEventCreate(&e);
            }
            return e;
        };
        sp.a = get();
        sp.b = get();
        (void)hipEventRecord(sp.a, ctx->stream);
    }
    ~KScope() {
        if (!ctx->profile) return;
        (void)hipEventRecord(sp.b, ctx->stream);
        ctx->iv.spans.push_back(sp);
    }
};
bool ensure(sb_ctx* ctx, DevBuf& b, size_t need);
// side streams (created on first use); fork: they wait for everything queued on ctx->stream so far; join: ctx->stream waits
// for the side streams listed in `used_mask`
bool side_streams(sb_ctx* ctx);
void side_fork(sb_ctx* ctx, uint32_t used_mask);
void side_join(sb_ctx* ctx, uint32_t used_mask);
StageSlot* acquire_slot(sb_ctx* ctx, size_t need);
int32_t check_hip(sb_ctx* ctx, hipError_t e, const char* what);
}  // namespace sb

// sb_nested.hip: the page records of an enqueued level call -> the caller's structs (Pending::NESTED_W / _R)
void nested_write_finish(sb_nested_levels_write* items, uint64_t n, const uint8_t* host);
void nested_read_finish(sb_nested_levels_read* items, uint64_t n, const uint8_t* host);
