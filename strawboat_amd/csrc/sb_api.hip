// strawboat-hip: C ABI (include/strawboat_hip.h) — context management and the decode entry
// points.  Host logic only: page bookkeeping (the arithmetic of read_integer & co: running row
// offset per page, src/read/array/integer.rs:210-238), table upload, kernel launches.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "sb_host.h"
#include "sb_key_buckets_prep.h"
#include "sb_key_lookup_prep.h"
#include "sb_span.h"

namespace sb {

void launch_decode(sb_ctx* ctx, const DecodeArgs& a, bool any_binary, bool any_prim, bool lzg_on, uint64_t* col_values_len, const FilterLaunch* flt,
                   const SelLaunch* rsel, const AggLaunch* agg, const GrpLaunch* grp = nullptr, const InCol* icols = nullptr,
                   const TopkLaunch* topk = nullptr, const KeyLaunch* keys = nullptr, const KeyVarLaunch* keyv = nullptr,
                   const GrpLaunch* grpl = nullptr, const LookLaunch* look = nullptr, const WgtLaunch* wgt = nullptr,
                   const BuckLaunch* buck = nullptr, const CmpCol* ccols = nullptr);
void launch_filter_cmp_plain(sb_ctx* ctx, const FilterCol& f, const CmpCol& cc, const uint8_t* values, const uint8_t* validity, uint64_t rows, uint32_t w,
                             uint64_t* count);
void launch_buck_zero(sb_ctx* ctx, const BuckLaunch& bl);
void launch_buck_finish(sb_ctx* ctx, const BuckLaunch& bl, uint64_t* results);
void launch_key_buckets_plain(sb_ctx* ctx, const BuckLaunch& bl, const uint64_t* rows, const uint8_t* const* values, const uint8_t* const* validity);
void launch_look_zero(sb_ctx* ctx, const LookLaunch& ll);
void launch_look_finish(sb_ctx* ctx, const LookLaunch& ll, uint64_t* results);
void launch_key_lookup_plain(sb_ctx* ctx, const LookLaunch& ll, const uint64_t* rows, const uint8_t* const* values, const uint8_t* const* validity);
void launch_key_zero(sb_ctx* ctx, const KeyLaunch& kl);
void launch_key_finish(sb_ctx* ctx, const KeyLaunch& kl, uint64_t* results);
void launch_key_assign(sb_ctx* ctx, const DecodeArgs& a, const KeyLaunch& kl);
void launch_key_collect_plain(sb_ctx* ctx, const KeyLaunch& kl, const uint64_t* rows, const uint8_t* const* values, const uint8_t* const* validity);
void launch_key_assign_plain(sb_ctx* ctx, const KeyLaunch& kl, const uint64_t* rows, const uint8_t* const* values, const uint8_t* const* validity);
void launch_keyv_zero(sb_ctx* ctx, const KeyVarLaunch& kl);
void launch_keyv_finish(sb_ctx* ctx, const DecodeArgs& a, const KeyVarLaunch& kl, uint64_t* results);
void launch_keyv_assign(sb_ctx* ctx, const DecodeArgs& a, const KeyVarLaunch& kl);
void launch_key_combine(sb_ctx* ctx, const CombLaunch& cl, uint64_t* results);
void launch_topk_zero(sb_ctx* ctx, const TopkLaunch& tl);
void launch_topk_finish(sb_ctx* ctx, const TopkLaunch& tl, uint64_t* results, uint32_t n_cols);
void launch_topk_plain(sb_ctx* ctx, const TopkLaunch& tl, uint32_t n_cols, const uint64_t* rows, const uint8_t* const* values,
                       const uint8_t* const* validity);
void launch_grp_zero(sb_ctx* ctx, const GrpLaunch& gl, uint32_t n_cols);
void launch_grp_finish(sb_ctx* ctx, const GrpLaunch& gl, uint64_t* results, uint32_t n_cols);
void launch_grp_plain(sb_ctx* ctx, const GrpLaunch& gl, uint32_t n_cols, const uint64_t* rows, const uint8_t* const* values,
                      const uint8_t* const* validity);
void launch_grpl_zero(sb_ctx* ctx, const GrpLaunch& gl, uint32_t n_cols);
void launch_grpl_finish(sb_ctx* ctx, const GrpLaunch& gl, uint64_t* results, uint32_t n_cols);
void launch_grpl_plain(sb_ctx* ctx, const GrpLaunch& gl, uint32_t n_cols, const uint64_t* rows, const uint8_t* const* values,
                       const uint8_t* const* validity);
void launch_wgt_zero(sb_ctx* ctx, const WgtLaunch& wl, uint32_t n_cols);
void launch_wgt_finish(sb_ctx* ctx, const WgtLaunch& wl, uint64_t* results, uint32_t n_cols);
void launch_wgt_plain(sb_ctx* ctx, const WgtLaunch& wl, uint32_t n_cols, const uint64_t* rows, const uint8_t* const* values,
                      const uint8_t* const* validity);
void launch_agg_finish(sb_ctx* ctx, const AggCol* acols, const AggPart* parts, uint64_t* results, uint32_t n_cols);
void launch_agg_plain(sb_ctx* ctx, const AggCol* acols, uint32_t n_cols, AggPart* parts, const uint64_t* rows, const uint8_t* const* values,
                      const uint8_t* const* validity);
void launch_rsel_plain(sb_ctx* ctx, const SelCol* scols, uint32_t n_cols, uint64_t* counts, bool any_nullable, const uint64_t* rows,
                       const uint8_t* const* values, const uint8_t* const* validity);
void launch_rsel_bin(sb_ctx* ctx, const DecodeArgs& a, const SelLaunch& sl);
void launch_filter_plain(sb_ctx* ctx, const FilterCol& f, const uint8_t* values, const uint8_t* validity, uint64_t rows, uint32_t w, uint64_t* count);
void launch_filter_in_plain(sb_ctx* ctx, const FilterCol& f, const InCol& ic, const uint8_t* values, const uint8_t* validity, uint64_t rows, uint32_t w,
                            uint64_t* count);
void launch_parse_sizes(sb_ctx* ctx, const DecodeArgs& a, uint64_t* col_values_len);
void launch_freq_scatter(sb_ctx* ctx, const FreqEntry* entries, uint32_t n, const uint64_t* ex_off, const uint8_t* ex_base);

// names as rocprofv3 prints them (template instances are registered by name at their launch sites)
static const char* const KERNEL_NAMES[K_COUNT] = {"k_parse", "k_inflate", "k_plan", "k_colscan", "k_inflate(values)",
                                                  "k_expand", "k_expand_binary", "k_enc_emit_tiles",
                                                  "k_enc_emit_pages<RLE>", "k_enc_layout", "k_enc_compact", "k_enc_select", "k_enc_emit_lz4",
                                                  "k_enc_emit_pages<Dict>", "k_enc_emit_pages<OneValue>",
                                                  "k_enc_emit_pages<Bitpacking>", "k_expand_rle", "k_enc_emit_pages<Patas>", "k_enc_freq_prep/finish", "k_enc_select_rle"};

int32_t check_hip(sb_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return SB_OK;
    return ctx->fail(SB_ERR_EXTERNAL, std::string(what) + ": " + hipGetErrorString(e));
}

bool ensure(sb_ctx* ctx, DevBuf& b, size_t need) {
    if (need <= b.cap) return true;
    // earlier launches may still use the old buffer
    if (b.p) {
        if (hipStreamSynchronize(ctx->stream) != hipSuccess) return false;
        (void)hipFree(b.p);
        b.p = nullptr;
        b.cap = 0;
    }
    size_t cap = need + need / 4 + 4096;
    if (hipMalloc((void**)&b.p, cap) != hipSuccess) {
        b.p = nullptr;
        return false;
    }
    b.cap = cap;
    return true;
}

bool side_streams(sb_ctx* ctx) {
    if (ctx->side_ready) return true;
    int lo_prio = 0, hi_prio = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo_prio, &hi_prio);
    for (int i = 0; i < sb_ctx::NSIDE; i++) {
        // side[0] carries the longest chain of a mixed call (binary columns): highest priority, so that its workgroups are
        // placed first when several kernels compete for the CUs
        if (hipStreamCreateWithPriority(&ctx->side[i], hipStreamNonBlocking, i == 0 ? hi_prio : lo_prio) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&ctx->join_ev[i], hipEventDisableTiming) != hipSuccess) return false;
    }
    if (hipEventCreateWithFlags(&ctx->fork_ev, hipEventDisableTiming) != hipSuccess) return false;
    ctx->side_ready = true;
    return true;
}
void side_fork(sb_ctx* ctx, uint32_t used_mask) {
    if (used_mask) ctx->side_forks++;
    (void)hipEventRecord(ctx->fork_ev, ctx->stream);
    for (int i = 0; i < sb_ctx::NSIDE; i++)
        if ((used_mask >> i) & 1) (void)hipStreamWaitEvent(ctx->side[i], ctx->fork_ev, 0);
}
void side_join(sb_ctx* ctx, uint32_t used_mask) {
    for (int i = 0; i < sb_ctx::NSIDE; i++)
        if ((used_mask >> i) & 1) {
            (void)hipEventRecord(ctx->join_ev[i], ctx->side[i]);
            (void)hipStreamWaitEvent(ctx->stream, ctx->join_ev[i], 0);
        }
}

StageSlot* acquire_slot(sb_ctx* ctx, size_t need) {
    StageSlot& s = ctx->slots[ctx->next_slot];
    ctx->next_slot = (ctx->next_slot + 1) % sb_ctx::NSLOTS;
    if (s.in_flight) {
        (void)hipEventSynchronize(s.done);
        s.in_flight = false;
    }
    // Results of earlier calls that were read back into this slot and not yet handed to their callers
    // (more than NSLOTS calls since the last synchronize): move them to heap storage owned by the
    // Pending entry before the slot is rewritten or freed.
    if (s.host)
        for (auto& p : ctx->iv.pending) {
            if (p.host < s.host || p.host >= s.host + s.cap) continue;
            const size_t nb = (p.kind == Pending::READ_COL || p.kind == Pending::FILTER_COL || p.kind == Pending::FILTER_CMP_COL || p.kind == Pending::RSEL_COL) ? 8 : p.kind == Pending::RSEL_VAR_COL ? 16 : p.kind == Pending::AGG_COL ? AGG_RESULT_WORDS * 8 : p.kind == Pending::ENC_HINT ? 128 : (p.kind == Pending::NESTED_W || p.kind == Pending::NESTED_R || p.kind == Pending::AGG_GRP_COL || p.kind == Pending::AGG_GRPL_COL || p.kind == Pending::AGG_WGT_COL || p.kind == Pending::TOPK_COL || p.kind == Pending::KEY_COL || p.kind == Pending::KEY_VAR_COL || p.kind == Pending::COMB_ITEM || p.kind == Pending::KEY_LOOK_COL || p.kind == Pending::KEY_BUCKET_COL) ? (size_t)p.bytes
                                                                                                   : (size_t)(2 * p.n + 1) * 8;
            ctx->iv.rescued.emplace_back(p.host, p.host + nb);
            p.host = ctx->iv.rescued.back().data();
        }
    if (s.cap < need) {
        // hipHostFree waits for the device: inside an enqueue it would drain the pipeline once per slot whenever a context
        // moves on to larger calls (the eight slots outgrown one after the other: +0.25 ms on each of the next eight calls)
        if (s.host) ctx->iv.stale_host.push_back(s.host);
        ctx->slot_cap_max = std::max(ctx->slot_cap_max, need + need / 4 + 4096);
        size_t cap = ctx->slot_cap_max;
        if (hipHostMalloc((void**)&s.host, cap, hipHostMallocDefault) != hipSuccess) {
            s.host = nullptr;
            s.cap = 0;
            return nullptr;
        }
        s.cap = cap;
    }
    if (!s.done) (void)hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
    return &s;
}

static const char* status_text(const Status& s, char* buf, size_t n) {
    const char* kind = s.code == SB_ERR_OUT_OF_SPEC ? "OutOfSpec"
                       : s.code == SB_ERR_EXTERNAL  ? "External"
                       : s.code == SB_ERR_IO        ? "Io(UnexpectedEof)"
                       : s.code == SB_ERR_NYI       ? "NotYetImplemented"
                                                    : "InvalidArgument";
    snprintf(buf, n, "%s raised on the device: page %u, site %u", kind, s.page, s.where);
    return buf;
}

}  // namespace sb

using namespace sb;

extern "C" {

const char* sb_version(void) { return "strawboat-hip 0.1 gfx950"; }

int32_t sb_ctx_create(int32_t device, void* hip_stream, sb_ctx** out) {
    if (!out) return SB_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return SB_ERR_EXTERNAL;
    if (hipSetDevice(device) != hipSuccess) return SB_ERR_EXTERNAL;
    sb_ctx* ctx = new sb_ctx();
    ctx->device = device;
    for (int i = 0; i < K_COUNT; i++) ctx->prof_id(KERNEL_NAMES[i]);
    if (hip_stream) {
        ctx->stream = (hipStream_t)hip_stream;
    } else {
        if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
            delete ctx;
            return SB_ERR_EXTERNAL;
        }
        ctx->own_stream = true;
    }
    if (hipMalloc((void**)&ctx->d_status, sizeof(Status)) != hipSuccess ||
        hipHostMalloc((void**)&ctx->h_status, sizeof(Status), hipHostMallocDefault) != hipSuccess) {
        sb_ctx_destroy(ctx);
        return SB_ERR_EXTERNAL;
    }
    (void)hipMemsetAsync(ctx->d_status, 0, sizeof(Status), ctx->stream);
    if (hipMalloc((void**)&ctx->zb_stats, 16 * sizeof(unsigned long long)) != hipSuccess) {
        sb_ctx_destroy(ctx);
        return SB_ERR_EXTERNAL;
    }
    (void)hipMemsetAsync(ctx->zb_stats, 0, 16 * sizeof(unsigned long long), ctx->stream);
    if (const char* e = getenv("SB_ZSTD_BLOCKS")) ctx->zb_mode = e[0] == '0' ? 0 : e[0] == '1' ? 1 : 2;
    if (const char* e = getenv("SB_ZSTD_BLOCKS_WG")) ctx->zb_wg_exec = e[0] != '0';
    if (const char* e = getenv("SB_BIN_FUSED")) ctx->bin_fused = e[0] != '0';
    if (const char* e = getenv("SB_NO_HINTS")) ctx->no_hints = e[0] != '0';
    if (const char* e = getenv("SB_HOST_GROUPS")) ctx->host_groups_max = std::max<uint32_t>(1, (uint32_t)strtoul(e, nullptr, 10));
    if (const char* e = getenv("SB_ZSTD_BLOCKS_MIN")) ctx->zb_min_csize = (uint32_t)strtoul(e, nullptr, 10);
    // tests: divide the block pipeline's pool estimates so that a call runs out of pool space part-way (frames that do not
    // fit go back to the frame-serial decoder)
    if (const char* e = getenv("SB_ZSTD_BLOCKS_POOL_DIV")) ctx->zb_pool_div = std::max<uint32_t>(1, (uint32_t)strtoul(e, nullptr, 10));
    *out = ctx;
    return SB_OK;
}

void sb_ctx_destroy(sb_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto& s : ctx->slots) {
        if (s.host) (void)hipHostFree(s.host);
        if (s.done) (void)hipEventDestroy(s.done);
    }
    for (void* p : ctx->iv.stale_host) (void)hipHostFree(p);
    for (void* p : ctx->iv.temp_dev) (void)hipFree(p);
    ctx->stage_release();
    for (auto& sp : ctx->iv.spans) {
        (void)hipEventDestroy(sp.a);
        (void)hipEventDestroy(sp.b);
    }
    for (auto e : ctx->free_events) (void)hipEventDestroy(e);
    for (auto& l : ctx->freq_logs) (void)hipFree(l.dev);
    if (ctx->tables.p) (void)hipFree(ctx->tables.p);
    if (ctx->scratch.p) (void)hipFree(ctx->scratch.p);
    if (ctx->staging.p) (void)hipFree(ctx->staging.p);
    if (ctx->filter_stage.p) (void)hipFree(ctx->filter_stage.p);
    if (ctx->combine.p) (void)hipFree(ctx->combine.p);
    if (ctx->zlit.p) (void)hipFree(ctx->zlit.p);
    if (ctx->zrec.p) (void)hipFree(ctx->zrec.p);
    if (ctx->zb_stats) (void)hipFree(ctx->zb_stats);
    if (ctx->zb_blocks.p) (void)hipFree(ctx->zb_blocks.p);
    if (ctx->zb_lit.p) (void)hipFree(ctx->zb_lit.p);
    if (ctx->lzg_pool.p) (void)hipFree(ctx->lzg_pool.p);
    if (ctx->zb_rec.p) (void)hipFree(ctx->zb_rec.p);
    if (ctx->enc_plan.pages.p) (void)hipFree(ctx->enc_plan.pages.p);
    if (ctx->d_status) (void)hipFree(ctx->d_status);
    if (ctx->h_status) (void)hipHostFree(ctx->h_status);
    for (int i = 0; i < sb_ctx::NSIDE; i++) {
        if (ctx->side[i]) (void)hipStreamDestroy(ctx->side[i]);
        if (ctx->join_ev[i]) (void)hipEventDestroy(ctx->join_ev[i]);
    }
    if (ctx->fork_ev) (void)hipEventDestroy(ctx->fork_ev);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    for (hipEvent_t e : ctx->pipe_ev) (void)hipEventDestroy(e);
    if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char* sb_ctx_last_error(sb_ctx* ctx) { return ctx ? ctx->last_error.c_str() : "null context"; }
void* sb_ctx_stream(sb_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

// What kind of call read_columns_impl serves: built at the entry points, read by every step of the call
struct ReadMode {
    // sb_read_columns (and the decode of a filter replay) / sb_read_columns_sizes / the Freq second pass, from inside a
    // synchronize / sb_filter_columns[_var], whose columns end in the filter kernels / sb_read_selected, whose columns end
    // in the selected-read kernels / sb_read_selected_var, whose binary columns end in those of sb_read_sel_bin.h /
    // sb_aggregate_columns, whose columns end in the aggregate kernels
    // / sb_aggregate_grouped, an aggregate call whose columns end in the grouped aggregate kernels
    // / sb_aggregate_grouped_large, the same with up to 1024 groups: a slot per chunk of 16 tiles instead of a slot per tile
    // / sb_aggregate_weighted, the same slots and chunks, a WgtCol per column beside its GrpCol, the weighted kernels
    // / sb_topk_columns, an aggregate call whose columns end in the top-k kernels
    // / sb_key_ids, an aggregate call whose columns end in the key kernels: two walks, the finish between them
    // / sb_key_ids_var, the same for binary columns, whose value blocks are staged as a filter call stages them
    // / sb_key_lookup, an aggregate call whose columns end in the lookup kernels: one walk, numeric and binary columns alike
    // / sb_key_buckets, an aggregate call whose columns end in the bucket kernels: the same walk over numeric columns
    // / sb_filter_columns_cmp, a filter call whose columns end in the kernels of sb_filter_cmp.h: a CmpCol beside every FilterCol
    enum Kind { READ, SIZES, FREQ_PASS, FILTER, SELECTED, SELECTED_VAR, AGGREGATE, AGG_GROUPED, AGG_GROUPED_LARGE, TOPK, KEY_IDS, KEY_IDS_VAR, KEY_LOOKUP, AGG_WEIGHTED, KEY_BUCKETS, FILTER_CMP } kind;
    const FilterCol* filt = nullptr;             // FILTER: one per column
    const std::vector<uint8_t>* lits = nullptr;  // ... the literals of the FK_BYTES columns, FilterCol.lit being the offset of each
    bool in_list = false;                        // ... sb_filter_columns_in: `lits` begins with an InCol per column, whose pointers are offsets in `lits`
                                                 // FILTER_CMP: `filt` as for FILTER, and `lits` is a CmpCol per column
    bool sizes() const { return kind == SIZES; }
    bool freq_pass() const { return kind == FREQ_PASS; }
    const SelCol* selc = nullptr;                // SELECTED: one per column (rank: filled in with the call's tables)
    const SelBin* selb = nullptr;                // SELECTED_VAR: one per column beside selc (sums: filled in with the call's tables)
    const AggCol* aggc = nullptr;                // AGGREGATE: one per column (the slots: filled in with the call's tables)
    const GrpCol* grpc = nullptr;                // AGG_GROUPED, AGG_GROUPED_LARGE: one per column beside aggc
    uint32_t grp_gmax = 0;                       // ... the largest n_groups of the call: records per slot
    const WgtCol* wgtc = nullptr;                // AGG_WEIGHTED: one per column beside aggc and grpc
    const TopkCol* topkc = nullptr;              // TOPK: one per column beside aggc
    uint32_t topk_kmax = 0;                      // ... the largest k of the call: records per slot
    const KeyCol* keyc = nullptr;                // KEY_IDS: one per column beside aggc
    uint32_t key_kmax = 0;                       // ... the largest max_keys of the call: key slots per result
    uint64_t key_slots = 0;                      // ... the slots of the columns' tables together
    const KeyVarCol* keyvc = nullptr;            // KEY_IDS_VAR: one per column beside aggc (key_kmax and key_slots as above)
    uint64_t key_kbytes = 0;                     // ... the largest keys_capacity of the call: bytes per result
    const LookCol* lookc = nullptr;              // KEY_LOOKUP: one per column beside aggc, whose pointers are offsets in `lits` (the lists)
    const BuckCol* buckc = nullptr;              // KEY_BUCKETS: one per column beside aggc, whose pointers are offsets in `lits` (the bounds and ids)
    // Where a column's result goes at the synchronize, as Pending has it (sb_host.h): users[i] beside pending_kind.  Set by
    // the entry points of the sinks: the callers' structs, for a filter call the caller's `selected` (results[i] + 1).
    // Null for the other kinds of call, whose results go to the sb_column_read structs of the call itself.
    void* const* users = nullptr;
    Pending::Kind pending_kind = Pending::READ_COL;
    bool aggregate() const { return kind == AGGREGATE || kind == AGG_GROUPED || kind == AGG_GROUPED_LARGE || kind == AGG_WEIGHTED || kind == TOPK || kind == KEY_IDS || kind == KEY_IDS_VAR || kind == KEY_LOOKUP || kind == KEY_BUCKETS; }   // an AggCol per column, slots per page part and tile
    bool grouped() const { return kind == AGG_GROUPED || kind == AGG_GROUPED_LARGE || kind == AGG_WEIGHTED; }   // a GrpCol per column, flags and gmax records per slot
    bool grouped_large() const { return kind == AGG_GROUPED_LARGE || kind == AGG_WEIGHTED; }   // ... whose tile slots are a slot per chunk of GRPL_CHUNK_TILES tiles
    bool weighted() const { return kind == AGG_WEIGHTED; }                            // ... and a WgtCol per column behind the GrpCols
    bool topk() const { return kind == TOPK; }
    bool key_ids() const { return kind == KEY_IDS; }
    bool key_var() const { return kind == KEY_IDS_VAR; }
    bool key_lookup() const { return kind == KEY_LOOKUP; }
    bool key_buckets() const { return kind == KEY_BUCKETS; }
    bool bin_id_tables() const { return kind == KEY_IDS_VAR || kind == KEY_LOOKUP; }   // a 16-bit id table and a bit table per binary Dict / Freq page
    bool filter() const { return kind == FILTER || kind == FILTER_CMP; }
    bool filter_cmp() const { return kind == FILTER_CMP; }
    bool selected() const { return kind == SELECTED; }
    bool selected_var() const { return kind == SELECTED_VAR; }
    bool ranked() const { return kind == SELECTED || kind == SELECTED_VAR; }   // a SelCol and a rank table per column
    // binary columns whose value blocks are staged and compared or gathered: no offsets are written by the read's kernels
    bool bin_staged() const { return filter() || kind == SELECTED_VAR || kind == KEY_IDS_VAR || kind == KEY_LOOKUP; }
    // the columns end in a sink of their own: `values` is a share of the staging area, there is no validity buffer, and
    // the call neither consults nor feeds the launch hints of the read path
    bool sink() const { return filter() || kind == SELECTED || kind == SELECTED_VAR || aggregate(); }
    // words of 8 bytes that come back per column: { selected, values_len } for a SELECTED_VAR call, the result record of
    // an AGGREGATE call, the header and the gmax group records of an AGG_GROUPED call, the header and the kmax entries of
    // a TOPK call, the header and the kmax key slots of a KEY_IDS call, the header, offsets and bytes of a KEY_IDS_VAR call
    uint64_t result_words() const {
        return kind == SELECTED_VAR ? 2 : kind == AGGREGATE ? AGG_RESULT_WORDS : grouped() ? grp_result_words(grp_gmax) : kind == TOPK ? topk_result_words(topk_kmax) : kind == KEY_IDS ? key_result_words(key_kmax) : kind == KEY_IDS_VAR ? keyv_result_words(key_kmax, key_kbytes) : kind == KEY_LOOKUP ? LOOK_RESULT_WORDS : kind == KEY_BUCKETS ? BUCK_RESULT_WORDS : 1;
    }
};
static int32_t read_columns_impl(sb_ctx* ctx, sb_column_read* cols, uint64_t n, int32_t mem, const ReadMode& mode);
static void update_read_hints(sb_ctx* ctx, uint32_t kinds);   // (next to read_hints, its reader)

// ---- sb_ctx_synchronize, step by step: status read -> replay? -> the interval's result -> Freq second pass -> profile ->
// results to the callers -> SB_MEM_HOST copies back -> release.  

// The status word travels with the stream: d_status -> h_status once everything queued has run.  The device only ever sets
// bits of `kinds`: the word is cleared here so that it describes the calls of ONE interval (the host's kinds_seen keeps what
// must stay).  feed_hints: the read at the end of an interval, whose kinds the next read calls go by; the Freq second pass
// reads the word too, and what that pass met is not what the next interval's calls met.
static hipError_t read_status(sb_ctx* ctx, bool feed_hints) {
    hipError_t e = hipMemcpyAsync(ctx->h_status, ctx->d_status, sizeof(Status), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return e;
    if (feed_hints) update_read_hints(ctx, ctx->h_status->kinds);
    if (ctx->h_status->kinds) (void)hipMemsetAsync(&ctx->d_status->kinds, 0, sizeof ctx->d_status->kinds, ctx->stream);
    return hipSuccess;
}

// The device raised an error (h_status->code): it becomes the result and last_error unless the host failed first (`rc`, whose
// text stays); the device's word is cleared either way.  Returns the result.
static int32_t take_device_error(sb_ctx* ctx, int32_t rc) {
    if (ctx->h_status->code == 0) return rc;
    if (rc == SB_OK) {
        char buf[160];
        rc = ctx->h_status->code;
        ctx->last_error = status_text(*ctx->h_status, buf, sizeof buf);
    }
    (void)hipMemsetAsync(ctx->d_status, 0, sizeof(Status), ctx->stream);
    return rc;
}

// Freq pages (integer/freq.rs:90-127) found by the decode calls of this synchronize interval: their
// exception blocks are ordinary BLOCK<T>s, so they go through the decoder once more as one-page
// columns that land in a temporary buffer; k_freq_scatter then writes them over the top value.
// Only runs when k_parse logged a Freq page; costs one 4-byte readback per log otherwise.
struct FreqBatch {   // the entries of one log that met Freq pages, and where their exceptions are decoded to
    const FreqEntry* d_entries;
    uint32_t n;
    uint8_t* ex_base;
    uint64_t* d_off;
};
// ... the logs read back: a batch per log, and every entry's exception block as a one-page column (iv.freq_cols / freq_metas)
static int32_t read_freq_logs(sb_ctx* ctx, std::vector<FreqBatch>& batches) {
    ctx->iv.freq_cols.clear();
    ctx->iv.freq_metas.clear();
    for (auto& log : ctx->freq_logs) {
        if (!log.reserved) continue;
        log.reserved = 0;
        uint32_t cnt = 0;
        if (hipMemcpy(&cnt, log.dev, 4, hipMemcpyDeviceToHost) != hipSuccess) return ctx->fail(SB_ERR_EXTERNAL, "freq log readback failed");
        if (cnt == 0) continue;
        (void)hipMemsetAsync(log.dev, 0, 16, ctx->stream);
        cnt = std::min(cnt, log.cap);
        std::vector<FreqEntry> ents(cnt);
        if (hipMemcpy(ents.data(), log.dev + 16, (size_t)cnt * sizeof(FreqEntry), hipMemcpyDeviceToHost) != hipSuccess)
            return ctx->fail(SB_ERR_EXTERNAL, "freq log readback failed");
        std::vector<uint64_t> ex_off(cnt);
        uint64_t total = 0;
        for (uint32_t i = 0; i < cnt; i++) {
            ex_off[i] = total;
            total += ((uint64_t)ents[i].n_exceptions * ents[i].width + 15) / 16 * 16;
        }
        FreqBatch b;
        b.d_entries = (const FreqEntry*)(log.dev + 16);
        b.n = cnt;
        if (hipMalloc((void**)&b.ex_base, total + 64) != hipSuccess) return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(freq exceptions) failed");
        ctx->iv.temp_dev.push_back(b.ex_base);
        if (hipMalloc((void**)&b.d_off, (size_t)cnt * 8) != hipSuccess) return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(freq offsets) failed");
        ctx->iv.temp_dev.push_back(b.d_off);
        if (hipMemcpy(b.d_off, ex_off.data(), (size_t)cnt * 8, hipMemcpyHostToDevice) != hipSuccess)
            return ctx->fail(SB_ERR_EXTERNAL, "freq offsets upload failed");
        for (uint32_t i = 0; i < cnt; i++) {
            sb_column_read c;
            memset(&c, 0, sizeof c);
            c.physical_type = (int32_t)ents[i].ptype;
            c.is_nullable = 0;
            c.pages = ents[i].nested;
            c.pages_len = ents[i].nested_len;
            c.n_pages = 1;
            c.values = b.ex_base + ex_off[i];
            c.values_capacity = (uint64_t)ents[i].n_exceptions * ents[i].width;
            ctx->iv.freq_cols.push_back(c);
            sb_page_meta m;
            m.length = ents[i].nested_len;
            m.num_values = ents[i].n_exceptions;
            ctx->iv.freq_metas.push_back(m);
        }
        batches.push_back(b);
    }
    for (size_t i = 0; i < ctx->iv.freq_cols.size(); i++) ctx->iv.freq_cols[i].metas = &ctx->iv.freq_metas[i];
    return SB_OK;
}
// ... and the pass proper: decode the exception blocks, scatter them, see what the device says.  Also called by a filter
// replay's decode (filter_columns_decoded), between its read and its comparison.
static int32_t freq_second_pass(sb_ctx* ctx) {
    std::vector<FreqBatch> batches;
    int32_t rc = read_freq_logs(ctx, batches);
    if (rc != SB_OK || batches.empty()) return rc;
    ctx->iv.freq_pass_ran = true;
    rc = read_columns_impl(ctx, ctx->iv.freq_cols.data(), ctx->iv.freq_cols.size(), SB_MEM_DEVICE, ReadMode{ReadMode::FREQ_PASS});
    if (rc != SB_OK) return rc;
    for (const FreqBatch& b : batches) launch_freq_scatter(ctx, b.d_entries, b.n, b.d_off, b.ex_base);
    const hipError_t e = read_status(ctx, false);
    if (e != hipSuccess) return check_hip(ctx, e, "freq second pass");
    // The pass goes by no launch hint (read_hints), so nothing of it may have been left undone: there is no call to issue
    // again from inside a synchronize, and the scatter above has read the exceptions already.  Never SB_OK over that.
    if (ctx->h_status->kinds & KIND_REPLAY) {
        (void)take_device_error(ctx, SB_ERR_EXTERNAL);   // (clears the device's word)
        return ctx->fail(SB_ERR_EXTERNAL, "freq second pass: an exceptions block was left undone on a launch hint");
    }
    return take_device_error(ctx, SB_OK);
}

// the Freq records of the interval point into buffers the caller may reuse: drop them all
static void clear_freq_logs(sb_ctx* ctx) {
    for (auto& log : ctx->freq_logs) {
        log.reserved = 0;
        (void)hipMemsetAsync(log.dev, 0, 16, ctx->stream);
    }
}
// What the end of an interval and the start of its replay share, once the stream (and the copy stream) is drained and
// nothing reads the interval's buffers any more: the interval's own state (Interval::reset says what a replay keeps) and
// the context's staging, which the next calls use from the start again
static void release_interval(sb_ctx* ctx, sb_ctx::Interval::Reset how) {
    for (auto& s : ctx->slots) s.in_flight = false;
    ctx->iv.reset(how);
    ctx->stage_rewind();
}

// The events of the profiled launches go back to the pool; timed: their spans are added to the profile first
static void recycle_spans(sb_ctx* ctx, bool timed) {
    for (auto& sp : ctx->iv.spans) {
        float ms = 0;
        if (timed && hipEventElapsedTime(&ms, sp.a, sp.b) == hipSuccess) {
            ctx->prof[sp.id].ms += ms;
            ctx->prof[sp.id].n += 1;
        }
        ctx->free_events.push_back(sp.a);
        ctx->free_events.push_back(sp.b);
    }
    ctx->iv.spans.clear();
}

// A page was left undone because a kernel it needed had been skipped on a hint (KIND_REPLAY): one extra pass with every
// kernel launched instead of a one-workgroup walk.  Not for an interval that failed on the host, not twice in a row, and
// only if there is a call to issue again (enqueued level calls are not kept).
static bool needs_replay(const sb_ctx* ctx, hipError_t e, int32_t rc) {
    return e == hipSuccess && (ctx->h_status->kinds & KIND_REPLAY) && rc == SB_OK && !ctx->in_replay && !ctx->iv.calls.empty();
}
// Drops what the interval produced and issues its calls again, without launch hints, then synchronizes for good.
// (an error code of such an interval is not looked at: kernels behind a skipped one may have met what it did not produce;
// a real error shows again in the replay)
static int32_t replay_interval(sb_ctx* ctx) {
    if (ctx->h_status->code != 0) (void)hipMemsetAsync(ctx->d_status, 0, sizeof(Status), ctx->stream);
    recycle_spans(ctx, false);
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);   // (copies of groups that ran: overwritten by the replay's)
    std::vector<sb_ctx::Call> calls;
    calls.swap(ctx->iv.calls);
    // the grouped aggregate columns that met a Freq page say so in their result header (k_grp_finish): they alone take the
    // decoded route below, so that a column's route does not depend on what else the interval holds
    // (the two grouped calls keep their marks apart: one struct may be handed to both in one interval)
    // (the columns of sb_aggregate_columns likewise, in the last word of their result record: k_agg_finish)
    ctx->grp_freq_users.clear();
    ctx->grpl_freq_users.clear();
    ctx->wgt_freq_users.clear();
    ctx->agg_freq_users.clear();
    for (const auto& p : ctx->iv.pending)
        if (p.kind == Pending::AGG_GRP_COL || p.kind == Pending::AGG_GRPL_COL || p.kind == Pending::AGG_WGT_COL) {
            uint64_t met = 0;
            memcpy(&met, p.host + 2 * sizeof(uint64_t), sizeof met);
            if (met) (p.kind == Pending::AGG_GRP_COL ? ctx->grp_freq_users : p.kind == Pending::AGG_GRPL_COL ? ctx->grpl_freq_users : ctx->wgt_freq_users).push_back(p.user);
        } else if (p.kind == Pending::AGG_COL) {
            uint64_t met = 0;
            memcpy(&met, p.host + (AGG_RESULT_WORDS - 1) * sizeof(uint64_t), sizeof met);
            if (met) ctx->agg_freq_users.push_back(p.user);
        }
    release_interval(ctx, sb_ctx::Interval::REPLAY);
    clear_freq_logs(ctx);
    ctx->filter_freq = (ctx->h_status->kinds & KIND_FILTER_FREQ) != 0;
    const bool saved = ctx->no_hints;
    ctx->no_hints = true;
    ctx->in_replay = true;   // (the entry points: such a call is not recorded again)
    ctx->replays++;
    if (ctx->h_status->kinds & KIND_REPLAY_LZG) ctx->lzg_state = 1;
    int32_t rc = SB_OK;
    for (auto& cl : calls)
        if ((rc = reissue(ctx, cl)) != SB_OK) break;
    ctx->no_hints = saved;
    ctx->filter_freq = false;
    ctx->grp_freq_users.clear();
    ctx->grpl_freq_users.clear();
    ctx->wgt_freq_users.clear();
    ctx->agg_freq_users.clear();
    if (rc != SB_OK) ctx->iv.sticky = rc;
    rc = sb_ctx_synchronize(ctx);   // (in_replay: this one ends the interval whatever the device says)
    ctx->in_replay = false;
    return rc;
}

// ---- the results of the interval's calls -> the callers' structs, by Pending::Kind (the table in sb_host.h)
static void deliver_read_col(const Pending& p) {
    uint64_t v;
    memcpy(&v, p.host, 8);
    ((sb_column_read*)p.user)->values_len = v;
}
static void deliver_filter_col(const Pending& p) { memcpy(p.user, p.host, 8); }
static void deliver_rsel_col(const Pending& p) {
    uint64_t v;
    memcpy(&v, p.host, 8);
    sb_column_read_selected* c = (sb_column_read_selected*)p.user;
    c->selected = v;
    c->values_len = v * type_width(c->physical_type);
}
static void deliver_rsel_var_col(const Pending& p) {
    uint64_t v[2];
    memcpy(v, p.host, 16);
    sb_column_read_selected_var* c = (sb_column_read_selected_var*)p.user;
    c->selected = v[0];
    c->values_len = v[1];
}
static void deliver_agg_col(const Pending& p) {   // (k_agg_finish's record: sb_aggregate.h)
    uint64_t v[AGG_RESULT_WORDS];
    memcpy(v, p.host, sizeof v);
    sb_column_aggregate* c = (sb_column_aggregate*)p.user;
    c->selected = v[0];
    c->count = v[1];
    c->nans = v[2];
    memcpy(c->min, &v[3], 8);
    memcpy(c->max, &v[4], 8);
    c->sum_lo = v[5];
    c->sum_hi = v[6];
}
// k_grp_finish's header and group records (sb_aggregate_grouped.h); `ok` false: the interval failed, selected alone
static void deliver_agg_grp_col(const Pending& p, bool ok) {
    uint64_t head[8];
    memcpy(head, p.host, sizeof head);
    sb_column_aggregate_grouped* c = (sb_column_aggregate_grouped*)p.user;
    c->selected = head[0];
    if (!ok) return;
    c->out_of_range = head[1];
    memcpy(c->groups, p.host + sizeof head, (size_t)p.bytes - sizeof head);
}
// k_wgt_finish's header and group records (sb_aggregate_weighted.h); `ok` false: the interval failed, selected alone
static void deliver_agg_wgt_col(const Pending& p, bool ok) {
    uint64_t head[8];
    memcpy(head, p.host, sizeof head);
    sb_column_aggregate_weighted* c = (sb_column_aggregate_weighted*)p.user;
    c->selected = head[0];
    if (!ok) return;
    c->out_of_range = head[1];
    memcpy(c->groups, p.host + sizeof head, (size_t)p.bytes - sizeof head);
}
// k_topk_finish's header and entries (sb_topk.h); `ok` false: the interval failed, selected alone
static void deliver_topk_col(const Pending& p, bool ok) {
    uint64_t head[8];
    memcpy(head, p.host, sizeof head);
    sb_column_topk* c = (sb_column_topk*)p.user;
    c->selected = head[0];
    if (!ok) return;
    c->count = head[1];
    c->nans = head[2];
    c->found = head[3];
    // (k as the struct has it now, but never more than the record that was enqueued holds: header + kmax entries)
    memcpy(c->out, p.host + sizeof head, std::min<size_t>((size_t)c->k * sizeof(sb_topk_row), (size_t)p.bytes - sizeof head));
}
// k_key_finish's header and key slots (sb_key_ids.h); `ok` false: the interval failed, selected alone
static void deliver_key_col(const Pending& p, bool ok) {
    uint64_t head[8];
    memcpy(head, p.host, sizeof head);
    sb_column_key_ids* c = (sb_column_key_ids*)p.user;
    c->selected = head[0];
    if (!ok) return;
    c->count = head[1];
    c->n_keys = head[2];
    c->overflow = head[3];
    // (max_keys as the struct has it now, but never more than the record that was enqueued holds: header + kmax slots)
    memcpy(c->keys, p.host + sizeof head, std::min<size_t>((size_t)c->max_keys * 8, (size_t)p.bytes - sizeof head));
}
// k_keyv_finish's header, offsets and bytes (sb_key_ids_bin.h); `ok` false: the interval failed, selected alone.  The
// record holds kmax + 1 offsets in front of the bytes, kmax being the largest max_keys of the call it was enqueued with.
static void deliver_key_var_col(const Pending& p, bool ok) {
    uint64_t head[8];
    memcpy(head, p.host, sizeof head);
    sb_column_key_ids_var* c = (sb_column_key_ids_var*)p.user;
    c->selected = head[0];
    if (!ok) return;
    c->count = head[1];
    c->n_keys = head[2];
    c->overflow = head[3];
    c->keys_len = head[4];
    const size_t kmax = (size_t)p.n, room = (size_t)p.bytes - sizeof head;
    const size_t n_off = std::min<size_t>((size_t)c->max_keys, kmax) + 1;
    memcpy(c->key_offsets, p.host + sizeof head, n_off * 8);
    const size_t cap = std::min<size_t>((size_t)c->keys_capacity, room - (kmax + 1) * 8);
    const size_t len = head[3] == 0 ? std::min<size_t>((size_t)head[4], cap) : 0;   // (an overflow of either kind: no bytes)
    if (len) memcpy(c->keys, p.host + sizeof head + (kmax + 1) * 8, len);
    if (cap > len) memset(c->keys + len, 0, cap - len);
}
// k_key_lookup_finish's record (sb_key_lookup.h); `ok` false: the interval failed, selected alone
static void deliver_key_look_col(const Pending& p, bool ok) {
    uint64_t v[LOOK_RESULT_WORDS];
    memcpy(v, p.host, sizeof v);
    sb_column_key_lookup* c = (sb_column_key_lookup*)p.user;
    c->selected = v[0];
    if (!ok) return;
    c->count = v[1];
    c->matched = v[2];
}
// k_key_buckets_finish's record (sb_key_buckets.h); `ok` false: the interval failed, selected alone
static void deliver_key_bucket_col(const Pending& p, bool ok) {
    uint64_t v[BUCK_RESULT_WORDS];
    memcpy(v, p.host, sizeof v);
    sb_column_key_buckets* c = (sb_column_key_buckets*)p.user;
    c->selected = v[0];
    if (!ok) return;
    c->count = v[1];
    c->matched = v[2];
    c->nans = v[3];
}
// k_key_finish's header and sorted codes of a key-combine item (sb_key_combine.h): { rows, live, n_keys, overflow, 0 .. },
// then kmax codes, of which the first n_keys are unpacked into `tuples`; a failed interval delivers nothing
static void deliver_comb_item(const Pending& p, bool ok) {
    if (!ok) return;
    uint64_t head[8];
    memcpy(head, p.host, sizeof head);
    sb_key_combine_item* c = (sb_key_combine_item*)p.user;
    c->live = head[1];
    c->n_keys = head[2];
    c->overflow = head[3];
    // (max_keys and n_parts as the struct has them now, but never more codes than the record that was enqueued holds)
    const size_t room = ((size_t)p.bytes - sizeof head) / 8, cap = std::min<size_t>((size_t)c->max_keys, room);
    const size_t nk = head[3] ? 0 : std::min<size_t>((size_t)head[2], cap);
    const uint32_t parts = std::min<uint32_t>(c->n_parts, COMB_MAX_PARTS);
    for (size_t i = 0; i < nk; i++) {
        uint64_t code;
        memcpy(&code, p.host + sizeof head + i * 8, 8);
        comb_unpack(code, parts, c->tuples + COMB_MAX_PARTS * i);
    }
    memset(c->tuples + COMB_MAX_PARTS * nk, 0, ((size_t)c->max_keys - nk) * COMB_MAX_PARTS * sizeof(uint32_t));
}
static void deliver_write_col(const Pending& p) {
    sb_column_write* c = (sb_column_write*)p.user;
    const uint64_t* lens = (const uint64_t*)p.host;  // [n_pages lengths][n_pages num_values][total]
    for (uint64_t i = 0; i < p.n && i < c->n_pages_capacity; i++) {
        c->out_metas[i].length = lens[i];
        c->out_metas[i].num_values = lens[p.n + i];
    }
    c->n_pages = p.n;
    c->out_len = lens[2 * p.n];
}
// the pages per codec of a write call, for the next call with its plan (EncPlan::last_counts): only if that plan is still
// the context's
static void apply_enc_hint(sb_ctx* ctx, const Pending& p) {
    if (!ctx->enc_plan.valid || ctx->enc_plan.key != p.n) return;
    uint32_t now[32];
    memcpy(now, p.host, 128);
    for (int i = 0; i < 32; i++) ctx->enc_plan.last_counts[i] = std::max(now[i], ctx->enc_plan.prev_counts[i]);
    memcpy(ctx->enc_plan.prev_counts, now, 128);
    ctx->enc_plan.counts_valid = true;
}
// `rc`: the interval's result; sizes and lengths are handed over even when it failed, hints and page records are not
static void deliver_pending(sb_ctx* ctx, const Pending& p, int32_t rc) {
    switch (p.kind) {
        case Pending::READ_COL: deliver_read_col(p); break;
        case Pending::FILTER_COL:
        case Pending::FILTER_CMP_COL: deliver_filter_col(p); break;
        case Pending::RSEL_COL: deliver_rsel_col(p); break;
        case Pending::RSEL_VAR_COL: deliver_rsel_var_col(p); break;
        case Pending::AGG_COL: deliver_agg_col(p); break;
        case Pending::AGG_GRP_COL:
        case Pending::AGG_GRPL_COL: deliver_agg_grp_col(p, rc == SB_OK); break;
        case Pending::AGG_WGT_COL: deliver_agg_wgt_col(p, rc == SB_OK); break;
        case Pending::TOPK_COL: deliver_topk_col(p, rc == SB_OK); break;
        case Pending::KEY_COL: deliver_key_col(p, rc == SB_OK); break;
        case Pending::KEY_VAR_COL: deliver_key_var_col(p, rc == SB_OK); break;
        case Pending::COMB_ITEM: deliver_comb_item(p, rc == SB_OK); break;
        case Pending::KEY_LOOK_COL: deliver_key_look_col(p, rc == SB_OK); break;
        case Pending::KEY_BUCKET_COL: deliver_key_bucket_col(p, rc == SB_OK); break;
        case Pending::WRITE_COL: deliver_write_col(p); break;
        case Pending::ENC_HINT:
            if (rc == SB_OK) apply_enc_hint(ctx, p);
            break;
        case Pending::NESTED_W:
            if (rc == SB_OK) nested_write_finish((sb_nested_levels_write*)p.user, p.n, p.host);
            break;
        case Pending::NESTED_R:
            if (rc == SB_OK) nested_read_finish((sb_nested_levels_read*)p.user, p.n, p.host);
            break;
    }
}

// SB_MEM_HOST: what was not sent back while the interval ran (all copies on the copy stream, one wait).  A copy that a group
// issued early is repeated if the Freq second pass ran, which wrote the buffers after it.  Returns the interval's result.
static int32_t finish_copybacks(sb_ctx* ctx, int32_t rc) {
    // (the stream exists only in contexts that serve host-memory calls: one more stream in the process changes how the
    // runtime maps streams to hardware queues — C4's side streams lost their overlap, 1.03 -> 1.55 ms per read)
    hipStream_t cs = ctx->iv.copybacks.empty() ? ctx->copy_stream : ctx->copy_stream_get();
    bool any = false;
    for (auto& cb : ctx->iv.copybacks) {
        if (cb.issued && !ctx->iv.freq_pass_ran) {
            any = true;
            continue;
        }
        const size_t nb = cb.used ? (size_t)std::min<uint64_t>(cb.n, *cb.used) : cb.n;
        if (rc == SB_OK && nb) {
            hipError_t ce = cs ? hipMemcpyAsync(cb.host, cb.dev, nb, hipMemcpyDeviceToHost, cs) : hipMemcpy(cb.host, cb.dev, nb, hipMemcpyDeviceToHost);
            if (ce != hipSuccess) rc = check_hip(ctx, ce, "copy back");
            any = true;
        }
    }
    if (any && cs) {
        hipError_t ce = hipStreamSynchronize(cs);
        if (ce != hipSuccess && rc == SB_OK) rc = check_hip(ctx, ce, "copy back");
    }
    return rc;
}

int32_t sb_ctx_synchronize(sb_ctx* ctx) {
    if (!ctx) return SB_ERR_INVALID;
    (void)hipSetDevice(ctx->device);
    int32_t rc = ctx->iv.sticky;   // a call of the interval failed on the host
    const hipError_t e = read_status(ctx, true);
    if (needs_replay(ctx, e, rc)) return replay_interval(ctx);
    if (e != hipSuccess)
        rc = check_hip(ctx, e, "sb_ctx_synchronize");
    else
        rc = take_device_error(ctx, rc);
    if (rc == SB_OK) rc = freq_second_pass(ctx);
    if (rc != SB_OK) {   // a failed interval
        clear_freq_logs(ctx);
        (void)hipStreamSynchronize(ctx->stream);
    }
    recycle_spans(ctx, true);
    for (const Pending& p : ctx->iv.pending) deliver_pending(ctx, p, rc);
    rc = finish_copybacks(ctx, rc);
    release_interval(ctx, sb_ctx::Interval::END);
    return rc;
}

uint64_t sb_ctx_side_forks(sb_ctx* ctx) { return ctx ? ctx->side_forks : 0; }
uint64_t sb_ctx_replays(sb_ctx* ctx) { return ctx ? ctx->replays : 0; }

int32_t sb_ctx_zstd_block_stats(sb_ctx* ctx, uint64_t out[4]) {
    if (!ctx || !out) return SB_ERR_INVALID;
    const int32_t rc = sb_ctx_synchronize(ctx);
    if (hipMemcpy(out, ctx->zb_stats, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return SB_ERR_EXTERNAL;
    return rc;
}

#ifdef ZB_TL
extern "C++" { namespace sb { void debug_lzx_timers(uint64_t* out8); } }
extern "C" int32_t sb_debug_zb_timers(sb_ctx* ctx, uint64_t out[20]) {   // development only (not in the header)
    (void)sb_ctx_synchronize(ctx);
    if (hipMemcpy(out, ctx->zb_stats + 4, 12 * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return SB_ERR_EXTERNAL;
    sb::debug_lzx_timers(out + 12);
    return SB_OK;
}
#endif

int32_t sb_ctx_profile(sb_ctx* ctx, int32_t enable) {
    if (!ctx) return SB_ERR_INVALID;
    int32_t rc = sb_ctx_synchronize(ctx);
    ctx->profile = enable != 0;
    for (auto& e : ctx->prof) {
        e.ms = 0;
        e.n = 0;
    }
    return rc;
}

uint32_t sb_ctx_profile_read(sb_ctx* ctx, sb_kernel_stat* out, uint32_t cap) {
    if (!ctx) return 0;
    uint32_t n = 0;
    for (size_t i = 0; i < ctx->prof.size() && n < cap; i++) {
        if (!ctx->prof[i].n) continue;
        out[n].name = ctx->prof[i].name.c_str();
        out[n].launches = ctx->prof[i].n;
        out[n].total_ms = ctx->prof[i].ms;
        n++;
    }
    return n;
}

// ------------------------------------------------------------------------------------ decode
// ---- read_columns_impl, step by step: checks and call shape -> launch hints -> table layout -> host staging -> tables ->
// pools -> upload -> arguments -> launches -> readbacks.  Every step reads the call's ReadMode.

// What the columns and their page lists decide for the whole call
struct ReadShape {
    uint64_t P = 0, T = 0;   // pages, tiles
    uint64_t C = 0;          // chunks of GRPL_CHUNK_TILES tiles, column by column (the tile slots of an AGG_GROUPED_LARGE call)
    uint64_t max_page_len = 0, max_page_rows = 0, pages_bytes = 0;
    uint64_t lzg_pages = 0;  // blocks that may go block-parallel: sb_lz4_giant.h
    bool any_binary = false, any_prim = false;
};

// The checks of every call; fills in cols[i].rows and clears cols[i].values_len
static int32_t read_shape(sb_ctx* ctx, sb_column_read* cols, uint64_t n, const ReadMode& mode, ReadShape& sh) {
    ReadShape a;   // (a local: the page loop's sums stay in registers)
    for (uint64_t i = 0; i < n; i++) {
        sb_column_read& c = cols[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return ctx->fail(SB_ERR_INVALID, "bad physical_type");
        if (c.n_pages && !c.metas) return ctx->fail(SB_ERR_INVALID, "metas is null");
        if (c.pages_len && !c.pages && c.physical_type != SB_TYPE_NULL) return ctx->fail(SB_ERR_INVALID, "pages is null");
        uint64_t rows = 0;
        const uint64_t tiles0 = a.T;
        for (uint64_t p = 0; p < c.n_pages; p++) {
            rows += c.metas[p].num_values;
            a.T += (c.metas[p].num_values + TILE_ROWS - 1) / TILE_ROWS;
            a.max_page_len = std::max<uint64_t>(a.max_page_len, c.metas[p].length);
            if (c.metas[p].length >= LZG_MIN) a.lzg_pages += is_binary_t(c.physical_type) ? 2 : 1;
            a.max_page_rows = std::max<uint64_t>(a.max_page_rows, c.metas[p].num_values);
        }
        c.rows = rows;
        c.values_len = 0;
        a.C += grpl_chunks(a.T - tiles0);
        a.P += c.n_pages;
        a.pages_bytes += c.pages_len;
        if (is_binary_t(c.physical_type))
            a.any_binary = true;
        else if (c.physical_type != SB_TYPE_NULL)
            a.any_prim = true;
        if (!mode.sizes() && c.physical_type != SB_TYPE_NULL && rows) {
            const uint32_t w = type_width(c.physical_type);
            if (!c.values) return ctx->fail(SB_ERR_INVALID, "values is null");
            if (c.is_nullable && !mode.sink() && (!c.validity || c.validity_capacity < (rows + 31) / 32 * 4))
                return ctx->fail(SB_ERR_INVALID, "validity buffer missing or smaller than 4*ceil(rows/32) bytes");
            if (is_binary_t(c.physical_type) && mode.bin_staged()) {
                // (a filter call writes no offsets, a selected read its own; `values` is the column's share of the staging area)
            } else if (is_binary_t(c.physical_type)) {
                if (!c.offsets || c.offsets_capacity < (rows + 1) * w)
                    return ctx->fail(SB_ERR_INVALID, "offsets buffer missing or too small");
            } else if (c.physical_type == SB_TYPE_BOOLEAN) {
                if (c.values_capacity < (rows + 31) / 32 * 4)
                    return ctx->fail(SB_ERR_INVALID, "boolean values buffer smaller than 4*ceil(rows/32) bytes");
            } else if (c.values_capacity < rows * w) {
                return ctx->fail(SB_ERR_INVALID, "values buffer too small");
            }
        }
    }
    sh = a;
    if (sh.P >= 0x7FFFFFFFull || sh.T >= 0x7FFFFFFFull) return ctx->fail(SB_ERR_INVALID, "too many pages in one call");
    return SB_OK;
}

// ---- launch hints: what a call launches, sizes or leaves out because of what the context's earlier intervals met.  The
// state has one writer (update_read_hints, from sb_ctx_synchronize) and one reader (read_hints, once per call); a page that
// needed a kernel which was left out stays undone and the interval is replayed with no_hints set (KIND_REPLAY).
struct ReadHints {
    bool zb_on = false;         // the block-parallel Zstd pipeline is launched
    bool zs_on = false;         // ... and the frame scan of long multi-frame Zstd buffers (sb_decode.hip)
    bool zrec_wanted = false;   // the lane-per-frame record arena
    uint32_t zb_skipped = 0;    // DecodeArgs.zb_skipped
    uint32_t read_skips = 0;    // DecodeArgs.read_skips
    enum { LZG_NONE, LZG_SKIPPED, LZG_POOL } lzg = LZG_NONE;   // no page long enough / left out on the hint / pool sized and grids set
    bool lzg_launch = false;    // launch_lzg launches the chain
};

// The producer: `kinds` is Status.kinds of the interval that a synchronize has just closed
static void update_read_hints(sb_ctx* ctx, uint32_t kinds) {
    ctx->kinds_seen |= kinds & KIND_ZSTD;
    // what the LAST interval's read calls met decides what the next ones launch: a context that read Zstd pages once and
    // LZ4 / plain pages ever since stops paying for the block pipeline's launches (7 kernels, ~40 us of a 0.6 ms call)
    // (two read intervals in a row without one: a nested reader alternates level calls — no Zstd — and leaf calls)
    if (kinds & KIND_ZSTD) {
        ctx->zstd_recent = true;
        ctx->zstd_idle = 0;
    } else if (ctx->read_calls && ++ctx->zstd_idle >= 2) {
        ctx->zstd_recent = false;
    }
    if (ctx->read_calls) {
        ctx->qa_idle = (kinds & KIND_QUEUE_A) ? 0 : ctx->qa_idle + 1;
        ctx->tiles_idle = (kinds & KIND_TILES) ? 0 : ctx->tiles_idle + 1;
    }
    ctx->read_calls = 0;
    // (three intervals with long pages and no such block before the chain is dropped: a reader that alternates giant-LZ4
    // columns with long plain ones keeps it; a wrong 2 costs a replay, not a one-workgroup walk)
    if (kinds & KIND_LZ4_GIANT) {
        ctx->lzg_state = 1;
        ctx->lzg_idle = 0;
    } else if (ctx->lzg_long_pages && ctx->lzg_state == 0) {
        ctx->lzg_state = 2;
    } else if (ctx->lzg_long_pages && ctx->lzg_state == 1 && ++ctx->lzg_idle >= 3) {
        ctx->lzg_state = 2;
    }
    ctx->lzg_long_pages = false;
    // (not sticky: what the calls since the last synchronize looked like decides the order of the next call's entropy kernels)
    if (kinds & KIND_ZSTD) ctx->zb_seq_long = (kinds & KIND_ZSEQ_LONG) != 0;
}

// The consumer.  Only a READ call consults every hint and counts as a call of its interval: a sizes call launches what
// values_len depends on, a filter call consults no launch hint and leaves the read calls' hint state alone.  The Freq
// second pass runs inside a synchronize, where nothing can be issued again: it goes by no hint at all (as if no_hints
// were set), and it is not a call of the next interval, whose state it leaves alone.
static ReadHints read_hints(sb_ctx* ctx, const ReadMode& mode, const ReadShape& sh) {
    ReadHints h;
    const bool no_hints = ctx->no_hints || mode.freq_pass();
    // the block-parallel Zstd pipeline: in a context whose last read intervals met Zstd buffers
    h.zb_on = ctx->zb_mode == 1 || (ctx->zb_mode == 2 && (ctx->zstd_recent || no_hints || mode.sink()));
    if (!mode.freq_pass() && !mode.sink()) ctx->read_calls++;
    // long multi-frame Zstd buffers (a one-page column written by this library): frames found by a scan (sb_decode.hip)
    h.zs_on = h.zb_on && !mode.sizes() && sh.max_page_len >= ZSTD_LONG_MIN;
    h.zb_skipped = (!h.zb_on && ctx->zb_mode == 2 && !mode.sizes() && sh.max_page_len >= ZSTD_LONG_MIN) ? 1u : 0u;
    // (the lane-per-frame record arena only for calls that can hold >= 4 x INFLATE_POOL frames of 16 KiB, and only in a
    // context that has met Zstd pages: LZ4 / plain / Dict-only readers never pay for it)
    h.zrec_wanted = sh.pages_bytes >= (48ull << 20) && (ctx->zb_mode == 1 || ctx->zstd_recent);
    // the inflate kernels of queue A / the tile kernel of primitives are left out when the last read interval queued nothing
    // for them (C2: four launches that found nothing to do, ~30 us of a 0.9 ms read); k_plan asks for the replay otherwise
    if (!ctx->no_hints && mode.kind == ReadMode::READ) {
        if (ctx->qa_idle >= 2) h.read_skips |= RSKIP_QUEUE_A;
        if (ctx->tiles_idle >= 2) h.read_skips |= RSKIP_TILES;
    }
    // LZ4 blocks of megabytes (a one-page column): block-parallel (sb_lz4_giant.h) — tables and entries in a pool of their own
    if (!mode.sizes() && sh.max_page_len >= LZG_MIN) {
        const bool none_met = ctx->lzg_state == 2 && !no_hints;   // the context's last intervals met no LZ4 block of megabytes
        // none met: no pool, no launches; k_inflate_lz4_big leaves such a block alone and asks for the replay (it used to
        // walk it with one workgroup: 0.8 s for 68 MB)
        h.lzg = none_met && !mode.sink() ? ReadHints::LZG_SKIPPED : ReadHints::LZG_POOL;
        // OPEN POINT, kept as it was found: a filter call in such a context sizes the pool and sets the grids, is NOT marked
        // lzg_skipped, and launches nothing all the same (launch_lzg used to read lzg_state for itself)
        h.lzg_launch = h.lzg == ReadHints::LZG_POOL && !none_met;
        // (noted here, before anything of the call can fail: a call that fails later — tables, staging, page_offsets, pools,
        // upload, or the giant-LZ4 pool itself — has still shown its long pages; it used to be noted after all of those)
        if (!mode.sink() && !mode.freq_pass()) ctx->lzg_long_pages = true;
    }
    return h;
}

// Where the call's tables sit, on the device (ctx->tables) and — up to `upload` — in the staging slot, whose next n words
// receive the results.  A pure function of shape, hints and mode.
struct ReadLayout {
    size_t cols, tasks, fcols, bcols, wcols, lits, upload, descs, tiles, jobs_a, jobs_b, jobs_z, counts, vlen, zb_counts, zb_frames, zs, rle, bpg, aggp, grp_recs, topk_recs, key_sorted, total;
    size_t job_cap;        // queue entries: 2 per page + room for the frames of Zstd buffers that are several frames (one entry per frame)
    bool want_z;           // queue Z (calls with binary columns that produce values): Zstd payloads known to k_parse, entropy stages with queue A's
    uint64_t zs_seg_cap;
    uint32_t rle_parts;    // long RLE pages: few pages of many rows are shared by several workgroups each (sb_decode.hip: k_rle_sums)
};
static ReadLayout read_layout(uint64_t n, const ReadShape& sh, const ReadHints& h, const ReadMode& mode) {
    ReadLayout L;
    const uint64_t P = sh.P;
    const size_t zs_extra = (size_t)std::min<uint64_t>(1u << 20, sh.pages_bytes / 256 + 64);
    size_t off = 0;
    L.cols = off;
    off = align_up(off + n * sizeof(ColDesc), 64);
    L.tasks = off;
    off = align_up(off + P * sizeof(PageTask), 64);
    L.fcols = off;
    if (mode.filter()) off = align_up(off + n * sizeof(FilterCol), 64);
    if (mode.ranked()) off = align_up(off + n * sizeof(SelCol), 64);   // (in the filter columns' place)
    if (mode.aggregate()) off = align_up(off + n * sizeof(AggCol), 64);   // (likewise)
    L.bcols = off;
    if (mode.selected_var()) off = align_up(off + n * sizeof(SelBin), 64);
    if (mode.grouped()) off = align_up(off + n * sizeof(GrpCol), 64);   // (in the SelBins' place)
    L.wcols = off;
    if (mode.weighted()) off = align_up(off + n * sizeof(WgtCol), 64);   // (behind the GrpCols)
    if (mode.topk()) off = align_up(off + n * sizeof(TopkCol), 64);     // (likewise)
    if (mode.key_ids()) off = align_up(off + n * sizeof(KeyCol), 64);   // (likewise)
    if (mode.key_var()) off = align_up(off + n * sizeof(KeyVarCol), 64);   // (likewise)
    if (mode.key_lookup()) off = align_up(off + n * sizeof(LookCol), 64);  // (likewise)
    if (mode.key_buckets()) off = align_up(off + n * sizeof(BuckCol), 64);  // (likewise)
    L.lits = off;
    if (mode.lits) off = align_up(off + mode.lits->size(), 64);
    L.upload = off;
    L.descs = off;
    off = align_up(off + P * sizeof(PageDesc), 64);
    L.tiles = off;
    off = align_up(off + sh.T * sizeof(TileTask), 64);
    L.job_cap = 2 * P + zs_extra;
    L.jobs_a = off;
    off = align_up(off + L.job_cap * sizeof(InflateJob), 64);
    L.jobs_b = off;
    off = align_up(off + L.job_cap * sizeof(InflateJob), 64);
    L.want_z = sh.any_binary && !mode.sizes();
    L.jobs_z = off;
    if (L.want_z) off = align_up(off + L.job_cap * sizeof(InflateJob), 64);
    L.counts = off;
    off = align_up(off + 64, 64);
    L.vlen = off;   // (a SELECTED_VAR call: the n bit counts of the rank kernels, then its { selected, values_len } per column)
    off = align_up(off + n * sizeof(uint64_t) * (mode.selected_var() ? 3 : mode.result_words()), 64);
    // the block-parallel Zstd pipeline: frames + counters here, blocks / literals / records in pools of their own
    L.zb_counts = off;
    if (h.zb_on) off = align_up(off + 64, 64);
    L.zb_frames = off;
    if (h.zb_on) off = align_up(off + L.job_cap * sizeof(ZbFrame), 64);
    L.zs_seg_cap = h.zs_on ? sh.pages_bytes / 16384 + 2 * P + 64 : 0;
    L.zs = off;
    if (h.zs_on) off = align_up(off + 256 + L.zs_seg_cap * 32, 64);
    L.rle_parts = (!mode.sizes() && sh.max_page_rows >= (1u << 18) && P > 0 && P <= 1024) ? (uint32_t)std::min<uint64_t>(256, 2048 / P) : 1u;
    L.rle = off;
    if (L.rle_parts > 1) off = align_up(off + P * L.rle_parts * sizeof(uint64_t), 64);
    L.bpg = off;
    if (L.rle_parts > 1) off = align_up(off + P * sizeof(uint32_t), 64);
    L.aggp = off;   // an AGGREGATE call's partial records: a slot per (page, RLE part), then a slot per tile
    if (mode.kind == ReadMode::AGGREGATE) off = align_up(off + (P * L.rle_parts + sh.T) * sizeof(AggPart), 64);
    if (mode.key_lookup()) off = align_up(off + n * sizeof(LookState), 64);   // a KEY_LOOKUP call: a state per column (zeroed)
    if (mode.key_buckets()) off = align_up(off + n * sizeof(BuckState), 64);  // a KEY_BUCKETS call: likewise
    // an AGG_GROUPED call: a flag word per slot, a counter and a Freq mark per column (zeroed), then gmax records per slot (not zeroed)
    // (an AGG_GROUPED_LARGE call: the same with a slot per chunk in the tile slots' place)
    const uint64_t grp_tile_slots = mode.grouped_large() ? sh.C : sh.T;
    L.grp_recs = align_up(off + (P * L.rle_parts + grp_tile_slots + 2 * n) * sizeof(uint64_t), 64);
    if (mode.grouped()) off = align_up(L.grp_recs + (P * L.rle_parts + grp_tile_slots) * mode.grp_gmax * sizeof(GrpPart), 64);
    // a TOPK call: a header per slot (zeroed), then kmax records per slot (not zeroed)
    L.topk_recs = align_up(off + (P * L.rle_parts + sh.T) * sizeof(TopkHead), 64);
    if (mode.topk()) off = align_up(L.topk_recs + (P * L.rle_parts + sh.T) * mode.topk_kmax * sizeof(TopkRec), 64);
    // a KEY_IDS call: a state per column and the columns' tables (zeroed), then KEY_MAX_KEYS sorted keys per column (not zeroed)
    L.key_sorted = align_up(off + n * sizeof(KeyState) + mode.key_slots * sizeof(uint64_t), 64);
    if (mode.key_ids()) off = align_up(L.key_sorted + n * KEY_MAX_KEYS * sizeof(uint64_t), 64);
    // a KEY_IDS_VAR call: the same area, of KeyVarStates and reference words; then the sorted keys of sb_key_ids_bin.h
    if (mode.key_var()) off = align_up(L.key_sorted + n * KEYV_SORTED_BYTES, 64);
    L.total = off;
    return L;
}

// The device buffers of each column: the caller's own (SB_MEM_DEVICE), or, for SB_MEM_HOST, device temporaries: the pages
// are staged over PCIe here, the outputs are copied back once they are written (queue_copybacks)
struct ReadBufs {
    const uint8_t* pages;
    uint8_t *values, *validity, *offsets;
};
static int32_t stage_read_cols(sb_ctx* ctx, hipStream_t s, const sb_column_read* cols, uint64_t n, int32_t mem, const ReadMode& mode,
                               std::vector<ReadBufs>& bufs) {
    bufs.assign(n, ReadBufs{});
    if (mem != SB_MEM_HOST) {
        for (uint64_t i = 0; i < n; i++) bufs[i] = {cols[i].pages, (uint8_t*)cols[i].values, cols[i].validity, (uint8_t*)cols[i].offsets};
        return SB_OK;
    }
    auto alloc = [&](size_t bytes, uint8_t** out) -> bool {
        *out = nullptr;
        if (!bytes) return true;
        return (*out = ctx->stage_alloc(bytes)) != nullptr;
    };
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_read& c = cols[i];
        ReadBufs& b = bufs[i];
        uint8_t* pages = nullptr;
        if (!alloc(c.pages_len, &pages)) return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(pages) failed");
        b.pages = pages;
        if (c.pages_len && hipMemcpyAsync(pages, c.pages, c.pages_len, hipMemcpyHostToDevice, s) != hipSuccess)
            return ctx->fail(SB_ERR_EXTERNAL, "H2D pages failed");
        if (mode.sizes()) continue;
        if (!alloc(c.values_capacity, &b.values) || !alloc(c.is_nullable ? c.validity_capacity : 0, &b.validity) ||
            !alloc(is_binary_t(c.physical_type) ? c.offsets_capacity : 0, &b.offsets))
            return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(outputs) failed");
    }
    return SB_OK;
}
// ... and what goes back from them (SB_MEM_HOST calls that produce values; sb_ctx_synchronize and the groups of
// sb_read_columns issue the copies)
static void queue_copybacks(sb_ctx* ctx, sb_column_read* cols, uint64_t n, const std::vector<ReadBufs>& bufs) {
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_read& c = cols[i];
        const ReadBufs& b = bufs[i];
        const uint32_t w = type_width(c.physical_type);
        if (c.is_nullable && c.rows) ctx->iv.copybacks.push_back({c.validity, b.validity, (size_t)((c.rows + 7) / 8)});
        if (is_binary_t(c.physical_type)) {
            ctx->iv.copybacks.push_back({c.offsets, b.offsets, (size_t)((c.rows + 1) * w)});
            ctx->iv.copybacks.push_back({c.values, b.values, (size_t)c.values_capacity, &cols[i].values_len});  // (set just before, from `pending`)
        } else if (c.physical_type == SB_TYPE_BOOLEAN) {
            ctx->iv.copybacks.push_back({c.values, b.values, (size_t)((c.rows + 7) / 8)});
        } else if (c.physical_type != SB_TYPE_NULL) {
            ctx->iv.copybacks.push_back({c.values, b.values, (size_t)(c.rows * w)});
        }
    }
}

// The list structs of the sinks carry offsets into the call's blob (in_set_append, look_list_append, buck_list_append)
// until the blob has a device address: `base`, in the call's tables on the page route, in a ReplayArena on the decoded one.
extern "C++" {   // (overloads: not inside the C linkage of the entry points)
static void rebase(InCol& c, const uint8_t* base) {
    c.keys = (const uint64_t*)(base + (size_t)(uintptr_t)c.keys);
    c.bytes = base + (size_t)(uintptr_t)c.bytes;
}
static void rebase(LookCol& c, const uint8_t* base) {
    c.keys = (const uint64_t*)(base + (size_t)(uintptr_t)c.keys);
    c.kid = (const uint32_t*)(base + (size_t)(uintptr_t)c.kid);
    c.bytes = base + (size_t)(uintptr_t)c.bytes;
}
static void rebase(BuckCol& c, const uint8_t* base) {
    c.keys = (const uint64_t*)(base + (size_t)(uintptr_t)c.keys);
    c.bid = (const uint32_t*)(base + (size_t)(uintptr_t)c.bid);
}
}   // extern "C++"

// The call's tables in the staging slot: ColDesc per column, PageTask per page (with the page's share of the scratch
// buffer, which is grown to fit), and for a filter call its FilterCol per column and the literals
static int32_t fill_read_tables(sb_ctx* ctx, uint8_t* host, const ReadLayout& L, const sb_column_read* cols, uint64_t n,
                                const std::vector<ReadBufs>& bufs, const ReadMode& mode) {
    ColDesc* hc = (ColDesc*)(host + L.cols);
    PageTask* ht = (PageTask*)(host + L.tasks);
    size_t scratch_off = 0;
    uint64_t page_i = 0, tile_i = 0;
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_read& c = cols[i];
        ColDesc& d = hc[i];
        memset(&d, 0, sizeof d);
        d.pages = bufs[i].pages;
        d.pages_len = c.pages_len;
        d.values = bufs[i].values;
        d.values_cap = mode.sizes() ? ~0ull : c.values_capacity;
        d.validity = bufs[i].validity;
        d.offsets = bufs[i].offsets;
        d.offsets_cap = c.offsets_capacity;
        d.rows = c.rows;
        d.ptype = c.physical_type;
        d.nullable = c.is_nullable;
        d.width = type_width(c.physical_type);
        d.first_page = (uint32_t)page_i;
        d.n_pages = (uint32_t)c.n_pages;
        uint64_t in_off = 0, out_row = 0;
        d.bits_aligned = 1;
        for (uint64_t p = 0; p + 1 < c.n_pages; p++)
            if (c.metas[p].num_values % 32) d.bits_aligned = 0;
        for (uint64_t p = 0; p < c.n_pages; p++, page_i++) {
            PageTask& t = ht[page_i];
            const uint64_t N = c.metas[p].num_values, len = c.metas[p].length;
            const uint64_t ntiles = (N + TILE_ROWS - 1) / TILE_ROWS;
            t.in_off = c.page_offsets ? c.page_offsets[p] : in_off;
            t.length = len;
            // (every page, with or without page_offsets; in_off is the sum of the lengths before the page in both cases)
            if (c.page_offsets && !page_span_ok(t.in_off, len, c.pages_len)) return ctx->fail(SB_ERR_IO, "page_offsets + length exceeds pages_len");
            if (!page_span_ok(in_off, len, c.pages_len)) return ctx->fail(SB_ERR_IO, "sum of PageMeta.length exceeds pages_len");
            t.num_values = N;
            t.out_row = out_row;
            t.col = (uint32_t)i;
            t.first_tile = (uint32_t)tile_i;
            t.aux_off = scratch_off;
            scratch_off += align_up((len / 4 + N / 128 + 4 * ntiles + 16) * 4, 16);   // (4 * ntiles: tile_k0 / tile_base + tile_bytes, and the u64 tile totals of a long binary Dict page)
            if (mode.bin_id_tables() && is_binary_t(c.physical_type)) scratch_off += keyv_id_table_words(len) * 4;    // (a 16-bit id per dictionary entry, in front of the bits: sb_key_ids_bin.h)
            if ((mode.filter() || mode.bin_id_tables()) && is_binary_t(c.physical_type)) scratch_off += filter_bin_table_words(len) * 4;   // (a bit per dictionary entry: sb_filter_bin.h)
            t.infl_off = scratch_off;
            scratch_off += align_up((N + 1) * 8 + 16, 16);
            in_off += len;
            out_row += N;
            tile_i += ntiles;
        }
    }
    if (mode.filter()) {
        FilterCol* hfc = (FilterCol*)(host + L.fcols);
        memcpy(hfc, mode.filt, n * sizeof(FilterCol));
        if (mode.lits && !mode.lits->empty()) memcpy(host + L.lits, mode.lits->data(), mode.lits->size());
        for (uint64_t i = 0; i < n; i++)
            if (hfc[i].kind == FK_BYTES) hfc[i].lit += (uint64_t)(uintptr_t)(ctx->tables.p + L.lits);
        InCol* hic = mode.in_list ? (InCol*)(host + L.lits) : nullptr;
        for (uint64_t i = 0; hic && i < n; i++) rebase(hic[i], ctx->tables.p + L.lits);
    }
    if (mode.aggregate()) {   // the columns' slots among the call's partial records (read_layout: L.aggp)
        AggCol* hac = (AggCol*)(host + L.fcols);
        memcpy(hac, mode.aggc, n * sizeof(AggCol));
        uint64_t tile0 = 0;
        for (uint64_t i = 0; i < n; i++) {
            uint64_t ntiles = 0;
            for (uint64_t p = 0; p < cols[i].n_pages; p++) ntiles += (cols[i].metas[p].num_values + TILE_ROWS - 1) / TILE_ROWS;
            hac[i].page_slot0 = (uint64_t)hc[i].first_page * L.rle_parts;
            hac[i].page_slots = cols[i].n_pages * L.rle_parts;
            if (mode.grouped_large()) ntiles = grpl_chunks(ntiles);   // (a slot per chunk of the column's tiles)
            hac[i].tile_slot0 = page_i * L.rle_parts + tile0;
            hac[i].tile_slots = ntiles;
            tile0 += ntiles;
        }
        if (mode.grouped()) memcpy(host + L.bcols, mode.grpc, n * sizeof(GrpCol));
        if (mode.weighted()) memcpy(host + L.wcols, mode.wgtc, n * sizeof(WgtCol));
        if (mode.topk()) memcpy(host + L.bcols, mode.topkc, n * sizeof(TopkCol));
        if (mode.key_ids()) memcpy(host + L.bcols, mode.keyc, n * sizeof(KeyCol));
        if (mode.key_var()) memcpy(host + L.bcols, mode.keyvc, n * sizeof(KeyVarCol));
        if (mode.key_lookup()) {   // the lists travel with the tables; the columns' pointers get their place
            LookCol* hl = (LookCol*)(host + L.bcols);
            memcpy(hl, mode.lookc, n * sizeof(LookCol));
            if (mode.lits && !mode.lits->empty()) memcpy(host + L.lits, mode.lits->data(), mode.lits->size());
            for (uint64_t i = 0; i < n; i++) rebase(hl[i], ctx->tables.p + L.lits);
        }
        if (mode.key_buckets()) {   // likewise: the bounds and ids travel with the tables
            BuckCol* hb = (BuckCol*)(host + L.bcols);
            memcpy(hb, mode.buckc, n * sizeof(BuckCol));
            if (mode.lits && !mode.lits->empty()) memcpy(host + L.lits, mode.lits->data(), mode.lits->size());
            for (uint64_t i = 0; i < n; i++) rebase(hb[i], ctx->tables.p + L.lits);
        }
    }
    SelCol* hsc = mode.ranked() ? (SelCol*)(host + L.fcols) : nullptr;
    for (uint64_t i = 0; hsc && i < n; i++) {   // the rank tables: behind the pages' areas, sized by the rows
        hsc[i] = mode.selc[i];
        hsc[i].rank = (uint64_t*)scratch_off;   // (an offset until the buffer is known)
        scratch_off += align_up(rsel_rank_words(cols[i].rows) * 8, 16);
    }
    SelBin* hsb = mode.selected_var() ? (SelBin*)(host + L.bcols) : nullptr;
    for (uint64_t i = 0; hsb && i < n; i++) {   // ... and behind them the sums of the length scan, the columns' back to back
        hsb[i] = mode.selb[i];
        hsb[i].sums = (uint64_t*)scratch_off;
        scratch_off += RSEL_BIN_SUM_WORDS * 8;
    }
    if (!ensure(ctx, ctx->scratch, scratch_off + 64)) return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(scratch) failed");
    for (uint64_t i = 0; hsc && i < n; i++) hsc[i].rank = (uint64_t*)(ctx->scratch.p + (size_t)hsc[i].rank);
    for (uint64_t i = 0; hsb && i < n; i++) hsb[i].sums = (uint64_t*)(ctx->scratch.p + (size_t)hsb[i].sums);
    return SB_OK;
}

// The Zstd decoders' areas: the per-wave literal buffers of the inflate pool (every call), the block pipeline's pools (sized
// per call; all zero: not launched) and the lane-per-frame record arena
struct ZbCaps {
    uint64_t block = 0, lit = 0, rec = 0;
};
static int32_t size_zb_pools(sb_ctx* ctx, const sb_column_read* cols, uint64_t n, const ReadMode& mode, const ReadShape& sh,
                             const ReadHints& h, size_t job_cap, ZbCaps& zb) {
    // the inflate pool's per-wave areas: a literal buffer of one block, and (calls with at least 4 queue entries per pool
    // wave: batches) the arena of pre-decoded Zstd sequences
    if (!ensure(ctx, ctx->zlit, (size_t)INFLATE_POOL * (128 * 1024 + 64))) return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(zlit) failed");
    if (h.zb_on) {
        // blocks: libzstd's are 128 KiB of content (sub-blocks of a few KiB when it splits them); literals: at most the
        // output (a Huffman stream expands <= 8 x); records: one per >= 3 output bytes, in practice one per >= 2 stream bytes.
        // A frame that does not fit is decoded by the one-wave path.
        const uint64_t pages_bytes = sh.pages_bytes;
        uint64_t out_bytes = 0;
        for (uint64_t i = 0; i < n; i++) {
            const uint64_t rows = cols[i].rows;
            out_bytes += mode.sizes() ? rows * 8 + 64 : cols[i].values_capacity + (is_binary_t(cols[i].physical_type) ? cols[i].offsets_capacity : 0) + rows * 8 + 64;
        }
        // Sized from the OUTPUT, not from the stream: a 128 KiB block of repetitive data is a few hundred stream bytes, RLE
        // literals expand 1 byte to 128 KiB, RLE / repeat-mode tables spend well under a byte per sequence.
        zb.block = std::min<uint64_t>(std::max<uint64_t>(pages_bytes / 2048, out_bytes / 8192) + 2 * job_cap + 64, 1u << 23);
        // ... with a ceiling all the same: a C2-shaped read (4 GB out of 250 MB of pages) asked for ~20 GB.  Literals at most
        // 8 x the pages + 256 MB (what Huffman streams expand to; blocks of RLE literals beyond that overflow the pool), records
        // at most 2^28 (3 GB; a cap by the stream's bytes is wrong: small integers in repeat mode are several sequences per stream
        // byte); what does not fit goes to the frame-serial decoder (ZbCounts, tests/test_gpu_zstd_blocks.py).
        zb.lit = std::min<uint64_t>(out_bytes, 8 * pages_bytes + (256ull << 20)) + 16 * zb.block + (1u << 16);
        zb.rec = std::min<uint64_t>(std::min<uint64_t>(4 * pages_bytes, out_bytes / 3), 1ull << 28) + (1u << 14);
        if (ctx->zb_pool_div > 1) {
            zb.block = std::max<uint64_t>(zb.block / ctx->zb_pool_div, 4);
            zb.lit = std::max<uint64_t>(zb.lit / ctx->zb_pool_div, 4096);
            zb.rec = std::max<uint64_t>(zb.rec / ctx->zb_pool_div, 64);
        }
        if (!ensure(ctx, ctx->zb_blocks, zb.block * (sizeof(ZbBlock) + 16)) || !ensure(ctx, ctx->zb_lit, zb.lit + 64) ||
            !ensure(ctx, ctx->zb_rec, zb.rec * 12 + 16))
            return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(zstd block pools) failed");
    }
    if (h.zrec_wanted && !ensure(ctx, ctx->zrec, (size_t)INFLATE_POOL * ZREC_PER_WAVE * 8))
        return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(zrec) failed");
    return SB_OK;
}

// The pool of the giant-LZ4 chain and the grids of its kernels (all zero: not in this call — also when the pool cannot be had)
struct LzgPool {
    LzgArgs lzg;
    uint32_t chunks = 0, wins = 0, rounds = 0, jobs = 0;
};
static LzgPool size_lzg_pool(sb_ctx* ctx, const sb_column_read* cols, uint64_t n, const ReadShape& sh, const ReadHints& h) {
    LzgPool g;
    if (h.lzg != ReadHints::LZG_POOL) return g;
    // the pool holds what the (at most LZG_JOBS) picked blocks need: 16 bytes per compressed byte and 4 per output byte of
    // the largest candidate pages — not of every page of the call (128 plain 1 M-row columns pinned 27 GB that way)
    uint64_t out_max = 0;
    std::vector<std::pair<uint64_t, uint64_t>> cand;   // (page bytes, output bytes of its column's share)
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t o = std::max<uint64_t>(cols[i].values_capacity, (cols[i].rows + 1) * 8);
        out_max = std::max(out_max, o);
        for (uint64_t k = 0; k < cols[i].n_pages; k++)
            if (cols[i].metas[k].length >= LZG_MIN) cand.push_back({cols[i].metas[k].length, o + (is_binary_t(cols[i].physical_type) ? (cols[i].rows + 1) * 8 : 0)});
    }
    std::sort(cand.begin(), cand.end(), [](const std::pair<uint64_t, uint64_t>& x, const std::pair<uint64_t, uint64_t>& y) { return x.first + x.second > y.first + y.second; });
    uint64_t pages_sel = 0, out_sel = 0;
    for (size_t q = 0; q < cand.size() && q < 2 * LZG_JOBS; q++) {   // (a page holds up to two blocks: queue A and queue B)
        pages_sel += cand[q].first;
        out_sel += cand[q].second;
    }
    const uint64_t pool = pages_sel * 16 + pages_sel / 512 + LZG_JOBS * (uint64_t)LZG_LITS * 16 + out_sel * 4 + out_sel / 2048 + (LZG_JOBS + 1) * (6 * 256 + (uint64_t)LZG_CH * 8 + 4096) +
                          LZG_JOBS * sizeof(LzgJob) + 1024;
    if (!ensure(ctx, ctx->lzg_pool, pool)) return g;
    g.lzg.jobs = (LzgJob*)ctx->lzg_pool.p;
    g.lzg.njobs = (uint32_t*)(ctx->lzg_pool.p + LZG_JOBS * sizeof(LzgJob));
    const uint64_t head = (LZG_JOBS * sizeof(LzgJob) + 64 + 255) & ~255ull;
    g.lzg.pool = ctx->lzg_pool.p + head;
    g.lzg.pool_bytes = pool - head;
    g.lzg.st = ctx->d_status;
    g.chunks = (uint32_t)((sh.max_page_len + LZG_CH - 1) / LZG_CH);
    g.jobs = (uint32_t)std::min<uint64_t>(sh.lzg_pages, LZG_JOBS);
    g.wins = (uint32_t)std::min<uint64_t>((out_max + LZG_WIN - 1) / LZG_WIN, 0x7FFFFFFFu);
    uint32_t bits = 1;
    while ((1ull << bits) < out_max + 1 && bits < 32) bits++;
    g.rounds = bits / 4 + 2;   // (a launch of k_lzg_jump is LZG_PASSES passes; a chain halves per pass at least — in practice a launch or two)
    return g;
}

// Room in the interval's Freq log for every page of this call to be a Freq page (null: the call logs none)
static int32_t reserve_freq_log(sb_ctx* ctx, hipStream_t s, const ReadMode& mode, uint64_t P, sb_ctx::FreqLog*& log) {
    log = nullptr;
    if (mode.sizes() || mode.freq_pass() || !P) return SB_OK;
    log = ctx->freq_logs.empty() ? nullptr : &ctx->freq_logs.back();
    if (!log || (uint64_t)log->reserved + P > log->cap) {
        sb_ctx::FreqLog nl;
        nl.cap = (uint32_t)std::max<uint64_t>(8192, 2 * P);
        if (hipMalloc((void**)&nl.dev, 16 + (size_t)nl.cap * sizeof(FreqEntry)) != hipSuccess)
            return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(freq log) failed");
        (void)hipMemsetAsync(nl.dev, 0, 16, s);
        ctx->freq_logs.push_back(nl);
        log = &ctx->freq_logs.back();
    }
    log->reserved += (uint32_t)P;
    return SB_OK;
}

// The kernels' arguments, from layout, hints and pools (what a call does not use keeps DecodeArgs' defaults)
static DecodeArgs fill_decode_args(sb_ctx* ctx, uint64_t n, const ReadMode& mode, const ReadShape& sh, const ReadHints& h, const ReadLayout& L,
                                   const ZbCaps& zb, const LzgPool& g, const sb_ctx::FreqLog* log) {
    uint8_t* tb = ctx->tables.p;
    DecodeArgs a;
    a.zlit = ctx->zlit.p;
    if (h.zrec_wanted) a.zrec = (uint64_t*)ctx->zrec.p;
    a.cols = (const ColDesc*)(tb + L.cols);
    a.tasks = (const PageTask*)(tb + L.tasks);
    a.descs = (PageDesc*)(tb + L.descs);
    a.tiles = (TileTask*)(tb + L.tiles);
    a.scratch = ctx->scratch.p;
    a.status = ctx->d_status;
    a.jobs_a = (InflateJob*)(tb + L.jobs_a);
    a.jobs_b = (InflateJob*)(tb + L.jobs_b);
    if (L.want_z) a.jobs_z = (InflateJob*)(tb + L.jobs_z);
    a.job_counts = (uint32_t*)(tb + L.counts);
    a.job_cap_a = a.job_cap_b = (uint32_t)L.job_cap;
    a.n_pages = (uint32_t)sh.P;
    a.n_cols = (uint32_t)n;
    a.n_tiles = (uint32_t)sh.T;
    a.sizes_only = mode.sizes() ? 1u : 0u;
    a.defer_payloads = (!mode.sizes() && sh.any_binary) ? 1u : 0u;
    a.no_freq = mode.freq_pass() ? 1u : 0u;
    // LZ4 blocks for the workgroup decoder: in a call with few blocks every block of 16 KiB and more (a lone wave's latency
    // is what the call waits for); in a call that fills the one-wave pool several times over only the blocks of 128 KiB and
    // more (64 KiB pages of incompressible values — the reference's bench shape — stay with the one-wave copy path)
    const uint32_t big_min = 2 * sh.P >= 4096 ? 2 * LZ4_BIG_MIN : LZ4_BIG_MIN / 4;
    a.lz4_big_min = sh.max_page_len >= big_min ? big_min : 0xFFFFFFFFu;
    a.read_skips = h.read_skips;
    a.zb_skipped = h.zb_skipped;
    a.lzg_skipped = h.lzg == ReadHints::LZG_SKIPPED ? 1u : 0u;
    a.lzg = g.lzg;
    a.lzg_chunks = g.chunks;
    a.lzg_wins = g.wins;
    a.lzg_rounds = g.rounds;
    a.lzg_jobs = g.jobs;
    a.rle_parts = L.rle_parts;
    if (L.rle_parts > 1) {
        a.rle_sums = (uint64_t*)(tb + L.rle);
        a.bp_guess = (uint32_t*)(tb + L.bpg);
    }
    if (h.zs_on) {
        a.zs_hdr = (uint32_t*)(tb + L.zs);
        a.zs_segs = (uint32_t*)(tb + L.zs + 256);
        a.zs_seg_cap = (uint32_t)std::min<uint64_t>(L.zs_seg_cap, 0x7FFFFFFFu);
    }
    if (h.zb_on) {
        a.zb.blocks = (ZbBlock*)ctx->zb_blocks.p;
        a.zb.lists = (uint32_t*)(ctx->zb_blocks.p + zb.block * sizeof(ZbBlock));
        a.zb.frames = (ZbFrame*)(tb + L.zb_frames);
        a.zb.lit = ctx->zb_lit.p;
        a.zb.rec = (uint64_t*)ctx->zb_rec.p;
        a.zb.counters = (uint32_t*)(tb + L.zb_counts);
        a.zb.block_cap = (uint32_t)zb.block;
        a.zb.frame_cap = (uint32_t)std::min<uint64_t>(L.job_cap, 0x7FFFFFFFu);
        a.zb.lit_cap = zb.lit;
        a.zb.rec_cap = zb.rec;
        a.zb.min_csize = ctx->zb_min_csize;
        a.zb.wg_exec = ctx->zb_wg_exec;
        a.zb.stats = ctx->zb_stats;
        a.zb.kinds = &ctx->d_status->kinds;
    }
    if (log) {
        a.freq_count = (uint32_t*)log->dev;
        a.freq_log = (FreqEntry*)(log->dev + 16);
        a.freq_cap = log->cap;
    }
    return a;
}

// The launches of the kinds of call (hc: the call's columns, host copy; hb: the SelBin of a SELECTED_VAR call, host copy)
static void launch_read(sb_ctx* ctx, const ReadMode& mode, const ReadShape& sh, const ReadHints& h, const ReadLayout& L, const DecodeArgs& a,
                        const ColDesc* hc, const SelBin* hb, uint64_t n) {
    const hipStream_t s = ctx->stream;
    uint64_t* d_vlen = (uint64_t*)(ctx->tables.p + L.vlen);   // values_len / bits set per column
    if (mode.sizes()) {
        if (sh.P) launch_parse_sizes(ctx, a, d_vlen);
    } else if (mode.filter()) {
        FilterLaunch fl{(const FilterCol*)(ctx->tables.p + L.fcols), d_vlen, false, false, false, false};
        for (uint64_t i = 0; i < n; i++) {
            const bool null_op = !mode.in_list && mode.filt[i].op >= SB_PRED_IS_NULL;   // (IN / NOT_IN: searched, sb_filter_in.h)
            (null_op ? fl.any_null : mode.filt[i].kind == FK_BYTES ? fl.any_bin : fl.any_cmp) = true;
            if (!null_op && !mode.in_list && mode.filt[i].kind == FK_BYTES && (mode.filt[i].mask & FILTER_MASK_SUB)) fl.any_sub = true;
            if (mode.filt[i].combine == SB_SEL_SET) fl.any_set = true;
        }
        const InCol* icols = mode.in_list ? (const InCol*)(ctx->tables.p + L.lits) : nullptr;
        const CmpCol* ccols = mode.filter_cmp() ? (const CmpCol*)(ctx->tables.p + L.lits) : nullptr;
        if (sh.P)
            launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, &fl, nullptr, nullptr, nullptr, icols, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, nullptr, ccols);
    } else if (mode.selected()) {
        SelLaunch sl{(const SelCol*)(ctx->tables.p + L.fcols), d_vlen, false};
        for (uint64_t i = 0; i < n; i++)
            if (mode.selc[i].validity) sl.any_nullable = true;
        if (sh.P) launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, &sl, nullptr);
    } else if (mode.selected_var()) {
        SelLaunch sl{(const SelCol*)(ctx->tables.p + L.fcols), d_vlen, false, (const SelBin*)(ctx->tables.p + L.bcols), d_vlen + n};
        for (uint64_t i = 0; i < n; i++)
            if (mode.selc[i].validity) sl.any_nullable = true;
        // (the columns' sums are one area: fill_read_tables; what is zeroed is the byte count of the rows without an offset)
        (void)hipMemsetAsync(hb[0].sums, 0, n * RSEL_BIN_SUM_WORDS * 8, s);
        // a call without a page still has a result: offsets[0] = 0, selected = values_len = 0
        if (sh.P) launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, &sl, nullptr);
        else launch_rsel_bin(ctx, a, sl);
    } else if (mode.grouped()) {
        const bool large = mode.grouped_large();
        const uint64_t slots = sh.P * L.rle_parts + (large ? sh.C : sh.T);
        GrpLaunch gl{(const AggCol*)(ctx->tables.p + L.fcols), (const GrpCol*)(ctx->tables.p + L.bcols), (uint64_t*)(ctx->tables.p + L.aggp),
                     (GrpPart*)(ctx->tables.p + L.grp_recs), slots, sh.P * L.rle_parts, mode.grp_gmax, false, false, (uint32_t)n, ctx->in_replay};
        for (uint64_t i = 0; i < n; i++) ((mode.aggc[i].ops & AGG_VALUE_OPS) ? gl.any_val : gl.any_null) = true;
        if (mode.weighted()) {
            const WgtLaunch wl{gl, (const WgtCol*)(ctx->tables.p + L.wcols)};
            launch_wgt_zero(ctx, wl, (uint32_t)n);
            if (sh.P)
                launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &wl);
            // (a call without a page still has a result: selected, and empty groups)
            launch_wgt_finish(ctx, wl, d_vlen, (uint32_t)n);
            return;
        }
        if (large) launch_grpl_zero(ctx, gl, (uint32_t)n);
        else launch_grp_zero(ctx, gl, (uint32_t)n);
        if (sh.P && large)
            launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &gl);
        else if (sh.P) launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, nullptr, nullptr, &gl);
        // (a call without a page still has a result: selected, and empty groups)
        if (large) launch_grpl_finish(ctx, gl, d_vlen, (uint32_t)n);
        else launch_grp_finish(ctx, gl, d_vlen, (uint32_t)n);
    } else if (mode.topk()) {
        TopkLaunch tl{(const AggCol*)(ctx->tables.p + L.fcols), (const TopkCol*)(ctx->tables.p + L.bcols), (TopkHead*)(ctx->tables.p + L.aggp),
                      (TopkRec*)(ctx->tables.p + L.topk_recs), sh.P * L.rle_parts + sh.T, sh.P * L.rle_parts, mode.topk_kmax};
        launch_topk_zero(ctx, tl);
        if (sh.P) launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, nullptr, nullptr, nullptr, nullptr, &tl);
        // (a call without a page still has a result: selected, and an `out` of zeros)
        launch_topk_finish(ctx, tl, d_vlen, (uint32_t)n);
    } else if (mode.key_ids()) {
        KeyLaunch kl{(const AggCol*)(ctx->tables.p + L.fcols), (const KeyCol*)(ctx->tables.p + L.bcols), (KeyState*)(ctx->tables.p + L.aggp),
                     (uint64_t*)(ctx->tables.p + L.aggp + n * sizeof(KeyState)), (uint64_t*)(ctx->tables.p + L.key_sorted),
                     n * sizeof(KeyState) + mode.key_slots * sizeof(uint64_t), mode.key_kmax, (uint32_t)n};
        launch_key_zero(ctx, kl);
        if (sh.P) launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &kl);
        // (a call without a page still has a result: selected, and `keys` of zeros)
        launch_key_finish(ctx, kl, d_vlen);
        if (sh.P) launch_key_assign(ctx, a, kl);
    } else if (mode.key_var()) {
        KeyVarLaunch kl{(const AggCol*)(ctx->tables.p + L.fcols), (const KeyVarCol*)(ctx->tables.p + L.bcols), (KeyVarState*)(ctx->tables.p + L.aggp),
                        (uint64_t*)(ctx->tables.p + L.aggp + n * sizeof(KeyVarState)), ctx->tables.p + L.key_sorted,
                        n * sizeof(KeyVarState) + mode.key_slots * sizeof(uint64_t), mode.key_kbytes, mode.key_kmax, (uint32_t)n};
        launch_keyv_zero(ctx, kl);
        if (sh.P) launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &kl);
        // (a call without a page still has a result: selected, offsets of zero)
        launch_keyv_finish(ctx, a, kl, d_vlen);
        if (sh.P) launch_keyv_assign(ctx, a, kl);
    } else if (mode.key_lookup()) {
        LookLaunch ll{(const AggCol*)(ctx->tables.p + L.fcols), (const LookCol*)(ctx->tables.p + L.bcols), (LookState*)(ctx->tables.p + L.aggp), (uint32_t)n,
                      sh.any_prim, sh.any_binary};
        launch_look_zero(ctx, ll);
        if (sh.P)
            launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &ll);
        // (a call without a page still has a result: selected, and zeros)
        launch_look_finish(ctx, ll, d_vlen);
    } else if (mode.key_buckets()) {
        BuckLaunch bl{(const AggCol*)(ctx->tables.p + L.fcols), (const BuckCol*)(ctx->tables.p + L.bcols), (BuckState*)(ctx->tables.p + L.aggp), (uint32_t)n};
        launch_buck_zero(ctx, bl);
        if (sh.P)
            launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                          nullptr, &bl);
        // (a call without a page still has a result: selected, and zeros)
        launch_buck_finish(ctx, bl, d_vlen);
    } else if (mode.aggregate()) {
        AggLaunch al{(const AggCol*)(ctx->tables.p + L.fcols), (AggPart*)(ctx->tables.p + L.aggp), sh.P * L.rle_parts, false, false, ctx->in_replay};
        for (uint64_t i = 0; i < n; i++) ((mode.aggc[i].ops & AGG_VALUE_OPS) ? al.any_val : al.any_null) = true;
        // an empty slot is all zero: a page that failed or a tile without a selected row writes none
        const size_t slots = (size_t)(sh.P * L.rle_parts + sh.T);
        if (slots) (void)hipMemsetAsync(al.parts, 0, slots * sizeof(AggPart), s);
        if (sh.P) launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, nullptr, &al);
        // (a call without a page still has a result: selected, and zeros)
        launch_agg_finish(ctx, al.acols, al.parts, d_vlen, (uint32_t)n);
    } else {
        // bitmaps are assembled with OR at page seams: start from zero
        for (uint64_t i = 0; i < n; i++) {
            const ColDesc& d = hc[i];
            if (d.bits_aligned) continue;  // no bitmap word is shared between pages: plain stores only
            if (d.nullable && d.validity && d.rows) (void)hipMemsetAsync(d.validity, 0, (d.rows + 31) / 32 * 4, s);
            if (d.ptype == SB_TYPE_BOOLEAN && d.values && d.rows) (void)hipMemsetAsync(d.values, 0, (d.rows + 31) / 32 * 4, s);
        }
        if (sh.P) launch_decode(ctx, a, sh.any_binary, sh.any_prim, h.lzg_launch, d_vlen, nullptr, nullptr, nullptr);
    }
}

// One Pending per column of a call whose results are on their way to `host`, `stride` bytes apart.  grpc: the columns of a
// grouped aggregate, of whose record the header and the column's own groups are handed over.
static void push_pending(sb_ctx* ctx, Pending::Kind kind, void* const* users, const uint8_t* host, size_t stride, uint64_t n,
                         const GrpCol* grpc = nullptr, uint32_t kmax = 0 /* KEY_VAR_COL: the call's largest max_keys */) {
    for (uint64_t i = 0; i < n; i++) {
        Pending pd;
        pd.kind = kind;
        pd.user = users[i];
        pd.host = host + i * stride;
        pd.n = 0;
        if (grpc) pd.bytes = sizeof(uint64_t) * grp_result_words(grpc[i].n_groups);
        if (kind == Pending::TOPK_COL) pd.bytes = stride;   // (the header and kmax entries: the column's own k is in its struct)
        if (kind == Pending::KEY_COL || kind == Pending::COMB_ITEM) pd.bytes = stride;    // (likewise: the header and kmax key slots / codes)
        if (kind == Pending::KEY_VAR_COL) pd.bytes = stride, pd.n = kmax;   // (the header, kmax + 1 offsets, the bytes)
        if (kind == Pending::KEY_LOOK_COL || kind == Pending::KEY_BUCKET_COL) pd.bytes = stride;
        ctx->iv.pending.push_back(pd);
    }
}

// Results: values_len per column (a filter call: the bits set per column) into the slot's n words behind the upload;
// sb_ctx_synchronize hands them to the callers' structs
static int32_t queue_read_results(sb_ctx* ctx, StageSlot* slot, const ReadLayout& L, const ReadMode& mode, const ReadShape& sh,
                                  sb_column_read* cols, uint64_t n) {
    const hipStream_t s = ctx->stream;
    const ColDesc* hc = (const ColDesc*)(slot->host + L.cols);
    uint8_t* hv = slot->host + L.upload;
    if (mode.aggregate()) {   // the result records, also of a call without a page
        hipError_t e = hipMemcpyAsync(hv, ctx->tables.p + L.vlen, n * mode.result_words() * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return check_hip(ctx, e, "aggregate readback");
    } else if (mode.selected_var()) {   // { selected, values_len } per column, behind the n bit counts; also of a call without a page
        hipError_t e = hipMemcpyAsync(hv, ctx->tables.p + L.vlen + n * sizeof(uint64_t), 2 * n * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return check_hip(ctx, e, "values_len readback");
    } else if (sh.P && (sh.any_binary || mode.sizes() || mode.sink())) {
        hipError_t e = hipMemcpyAsync(hv, ctx->tables.p + L.vlen, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return check_hip(ctx, e, "values_len readback");
    } else {
        for (uint64_t i = 0; i < n; i++) {  // fixed-width columns: rows * width (booleans: bitmap bytes)
            const uint64_t v = !sh.P ? 0 : hc[i].ptype == SB_TYPE_BOOLEAN ? (hc[i].rows + 7) / 8 : hc[i].rows * hc[i].width;
            memcpy(hv + i * sizeof(uint64_t), &v, sizeof v);
        }
    }
    (void)hipEventRecord(slot->done, s);
    slot->in_flight = true;
    std::vector<void*> own;   // (the results of a call that is no sink go to its own columns)
    if (!mode.users) {
        own.resize(n);
        for (uint64_t i = 0; i < n; i++) own[i] = &cols[i];
    }
    push_pending(ctx, mode.pending_kind, mode.users ? mode.users : own.data(), hv, sizeof(uint64_t) * mode.result_words(), n,
                 mode.grouped() ? mode.grpc : nullptr, mode.key_kmax);
    return SB_OK;
}

static int32_t read_columns_impl(sb_ctx* ctx, sb_column_read* cols, uint64_t n, int32_t mem, const ReadMode& mode) {
    if (!ctx || (!cols && n)) return SB_ERR_INVALID;
    if (n == 0) return SB_OK;
    (void)hipSetDevice(ctx->device);
    const hipStream_t s = ctx->stream;
    ReadShape sh;
    int32_t rc = read_shape(ctx, cols, n, mode, sh);
    if (rc != SB_OK) return rc;
    const ReadHints h = read_hints(ctx, mode, sh);
    const ReadLayout L = read_layout(n, sh, h, mode);
    if (!ensure(ctx, ctx->tables, L.total)) return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(tables) failed");
    StageSlot* slot = acquire_slot(ctx, L.upload + n * sizeof(uint64_t) * mode.result_words());
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    std::vector<ReadBufs> bufs;
    if ((rc = stage_read_cols(ctx, s, cols, n, mem, mode, bufs)) != SB_OK) return rc;
    if ((rc = fill_read_tables(ctx, slot->host, L, cols, n, bufs, mode)) != SB_OK) return rc;
    ZbCaps zb;
    if ((rc = size_zb_pools(ctx, cols, n, mode, sh, h, L.job_cap, zb)) != SB_OK) return rc;
    uint8_t* tb = ctx->tables.p;
    hipError_t e = hipMemcpyAsync(tb, slot->host, L.upload, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return check_hip(ctx, e, "table upload");
    const LzgPool lzg = size_lzg_pool(ctx, cols, n, sh, h);
    if (h.zs_on) (void)hipMemsetAsync(tb + L.zs, 0, 256 + L.zs_seg_cap * 32, s);
    sb_ctx::FreqLog* log = nullptr;
    if ((rc = reserve_freq_log(ctx, s, mode, sh.P, log)) != SB_OK) return rc;
    const DecodeArgs a = fill_decode_args(ctx, n, mode, sh, h, L, zb, lzg, log);
    launch_read(ctx, mode, sh, h, L, a, (const ColDesc*)(slot->host + L.cols), (const SelBin*)(slot->host + L.bcols), n);
    e = hipGetLastError();
    if (e != hipSuccess) return check_hip(ctx, e, "decode launch");
    if ((rc = queue_read_results(ctx, slot, L, mode, sh, cols, n)) != SB_OK) return rc;
    if (mem == SB_MEM_HOST && !mode.sizes()) queue_copybacks(ctx, cols, n, bufs);
    return SB_OK;
}

// SB_MEM_HOST calls of many columns are cut into groups: while group g + 1's pages travel to the device, group g's Arrow
// buffers travel back on the copy stream — PCIe's two directions are independent, and a call that ran them one after the
// other (all copies in, kernels, all copies out at the synchronize) used half of the link.  Fixed-size outputs are sent as
// soon as the group's kernels are done; values of binary columns (length known with the results) at the synchronize.
static uint64_t host_groups(sb_ctx* ctx, uint64_t n, uint64_t bytes) {
    if (n < 4 || bytes < (32ull << 20)) return 1;
    return std::min<uint64_t>(ctx->host_groups_max, n / 2);
}
int32_t sb_read_columns(sb_ctx* ctx, sb_column_read* cols, uint64_t n, int32_t mem) {
    int32_t rc = SB_OK;
    uint64_t groups = 1;
    if (ctx && cols && mem == SB_MEM_HOST && n >= 4) {
        uint64_t bytes = 0;
        for (uint64_t i = 0; i < n; i++) bytes += cols[i].pages_len + cols[i].values_capacity;
        groups = host_groups(ctx, n, bytes);
    }
    hipStream_t cs = groups > 1 ? ctx->copy_stream_get() : nullptr;
    if (!cs) {
        rc = read_columns_impl(ctx, cols, n, mem, ReadMode{ReadMode::READ});
    } else {
        const uint64_t per = (n + groups - 1) / groups;
        for (uint64_t g0 = 0; g0 < n && rc == SB_OK; g0 += per) {
            const size_t cb0 = ctx->iv.copybacks.size();
            rc = read_columns_impl(ctx, cols + g0, std::min<uint64_t>(per, n - g0), mem, ReadMode{ReadMode::READ});
            if (rc != SB_OK) break;
            hipEvent_t ev = ctx->next_pipe_event();
            if (!ev || hipEventRecord(ev, ctx->stream) != hipSuccess || hipStreamWaitEvent(cs, ev, 0) != hipSuccess) continue;   // (copied at the synchronize)
            for (size_t k = cb0; k < ctx->iv.copybacks.size(); k++) {
                auto& cb = ctx->iv.copybacks[k];
                if (cb.used || !cb.n) continue;
                if (hipMemcpyAsync(cb.host, cb.dev, cb.n, hipMemcpyDeviceToHost, cs) == hipSuccess) cb.issued = true;
            }
        }
    }
    if (rc == SB_OK && ctx && n && !ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::READ, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ sinks: the steps their entry points share
static bool filter_comparable(int32_t t) {
    return (t >= SB_TYPE_INT8 && t <= SB_TYPE_UINT64) || t == SB_TYPE_FLOAT32 || t == SB_TYPE_FLOAT64;
}

// how the sink kernels compare, order and add the values of a numeric type
static uint32_t value_kind(int32_t t) {
    return t == SB_TYPE_FLOAT32 ? FK_F32 : t == SB_TYPE_FLOAT64 ? FK_F64 : t <= SB_TYPE_INT64 ? FK_SIGNED : FK_UNSIGNED;
}

// what an entry point refuses itself is refused before anything is enqueued or written, and does not show again at the synchronize
static int32_t refuse(sb_ctx* ctx, int32_t code, const char* msg) {
    ctx->last_error = msg;
    return code;
}

// How every sink entry point begins.  False: the call ends here, with *rc.
static bool sink_entry(sb_ctx* ctx, const void* cols, uint64_t n, int32_t mem, const char* name, int32_t* rc) {
    *rc = SB_OK;
    if (!ctx || (!cols && n)) {
        *rc = SB_ERR_INVALID;
    } else if (n && mem != SB_MEM_DEVICE) {
        ctx->last_error = std::string(name) + ": SB_MEM_HOST is not implemented";
        *rc = SB_ERR_NYI;
    }
    return *rc == SB_OK && n;
}

extern "C++" {   // (templates: not inside the C linkage of the entry points)
// The column structs of the sinks begin alike, with the pages of the column as sb_column_filter has them
template <class Col>
constexpr bool has_pages_prefix() {
    return offsetof(Col, physical_type) == offsetof(sb_column_filter, physical_type) && offsetof(Col, is_nullable) == offsetof(sb_column_filter, is_nullable) &&
           offsetof(Col, pages) == offsetof(sb_column_filter, pages) && offsetof(Col, pages_len) == offsetof(sb_column_filter, pages_len) &&
           offsetof(Col, metas) == offsetof(sb_column_filter, metas) && offsetof(Col, n_pages) == offsetof(sb_column_filter, n_pages) &&
           offsetof(Col, page_offsets) == offsetof(sb_column_filter, page_offsets);
}
static_assert(offsetof(sb_column_filter, page_offsets) == 40, "the pages of a sink column: 48 bytes");
static_assert(has_pages_prefix<sb_column_filter_var>() && has_pages_prefix<sb_column_read_selected>() && has_pages_prefix<sb_column_read_selected_var>() &&
                  has_pages_prefix<sb_column_aggregate>() && has_pages_prefix<sb_column_aggregate_grouped>() && has_pages_prefix<sb_column_topk>() &&
                  has_pages_prefix<sb_column_key_ids>() && has_pages_prefix<sb_column_key_ids_var>() && has_pages_prefix<sb_column_key_lookup>() &&
                  has_pages_prefix<sb_column_key_buckets>() && has_pages_prefix<sb_column_filter_cmp>(),
              "every sink column begins with the seven fields of sb_column_filter, at its offsets");

// The pages of a sink column as a read column (outputs: none yet)
template <class Col>
static sb_column_read read_col_of(const Col& u) {
    sb_column_read r;
    memset(&r, 0, sizeof r);
    r.physical_type = u.physical_type;
    r.is_nullable = u.is_nullable;
    r.pages = u.pages;
    r.pages_len = u.pages_len;
    r.metas = u.metas;
    r.n_pages = u.n_pages;
    r.page_offsets = u.page_offsets;
    return r;
}

// The rows of a column: what its pages' metas say.  False: it has pages and no metas ("metas is null").
template <class Col>
static bool column_rows(const Col& c, uint64_t* rows) {
    if (c.n_pages && !c.metas) return false;
    uint64_t r = 0;
    for (uint64_t p = 0; p < c.n_pages; p++) r += c.metas[p].num_values;
    *rows = r;
    return true;
}

// The elements of v whose dec[i] is set, taken out of v; both parts keep their order.  (A replayed call splits its columns'
// parallel vectors with it: those that go through a full decode, and the rest.)
template <class T>
static std::vector<T> take_if(std::vector<T>& v, const std::vector<bool>& dec) {
    std::vector<T> taken, rest;
    for (size_t i = 0; i < v.size(); i++) (dec[i] ? taken : rest).push_back(v[i]);
    v.swap(rest);
    return taken;
}

// The last part of an entry point begins with the call's columns as read columns, and the callers' structs as the users of
// their results
template <class Col>
static void read_cols_of(Col* cols, uint64_t n, std::vector<sb_column_read>& rc_cols, std::vector<void*>& users) {
    rc_cols.resize(n);
    users.resize(n);
    for (uint64_t i = 0; i < n; i++) {
        rc_cols[i] = read_col_of(cols[i]);
        users[i] = &cols[i];
    }
}

// The `ids` output of a key sink (id_width, ids, ids_capacity), in two steps as the aggregate check has them: the width,
// which the limits an entry point checks next go by, and -- once the rows are known -- the buffer.  The message of the
// refusal (SB_ERR_INVALID) or null.
template <class Col>
static const char* ids_check_width(const Col& c) {
    return c.id_width != 1 && c.id_width != 2 && c.id_width != 4 ? "id_width is not 1, 2 or 4" : nullptr;
}
template <class Col>
static const char* ids_check_buffer(const Col& c, uint64_t rows) {
    if (rows && !c.ids) return "ids is null";
    if (c.ids && (((uintptr_t)c.ids & (c.id_width - 1)) || c.ids_capacity < rows * c.id_width))
        return "ids not aligned to id_width or smaller than rows * id_width bytes";
    return nullptr;
}
// ... and of the columns of one call together: the bytes a column writes are rows * id_width (hs[i].rows: agg_check_fill's)
template <class Col>
static const char* ids_check_overlaps(const Col* cols, const std::vector<AggCol>& hs) {
    for (size_t i = 0; i < hs.size(); i++)
        for (size_t j = i + 1; j < hs.size(); j++) {
            const uintptr_t a0 = (uintptr_t)cols[i].ids, a1 = a0 + hs[i].rows * cols[i].id_width;
            const uintptr_t b0 = (uintptr_t)cols[j].ids, b1 = b0 + hs[j].rows * cols[j].id_width;
            if (a0 < b1 && b0 < a1) return "ids of two columns of one call overlap";
        }
    return nullptr;
}
}   // extern "C++"

// The normal route: column i's share of the staging area, cap[i] bytes at a multiple of 64, as the `values` of its read
// column.  NO_SHARE: no page body of the column is parsed, queued or planned (a null test, a count) -- it is read as SB_TYPE_NULL.
static const uint64_t NO_SHARE = ~0ull;
static int32_t stage_shares(sb_ctx* ctx, sb_column_read* rc_cols, const uint64_t* cap, uint64_t n) {
    size_t stage = 0;
    for (uint64_t i = 0; i < n; i++)
        if (cap[i] != NO_SHARE) stage += align_up(cap[i], 64);
    if (!ensure(ctx, ctx->filter_stage, stage + 64)) return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(filter staging) failed");
    size_t so = 0;
    for (uint64_t i = 0; i < n; i++) {
        sb_column_read& r = rc_cols[i];
        if (cap[i] == NO_SHARE) {
            r.physical_type = SB_TYPE_NULL;
            continue;
        }
        r.values = ctx->filter_stage.p + so;
        r.values_capacity = cap[i];
        so += align_up(cap[i], 64);
    }
    return SB_OK;
}

// The replay of an interval in which a sink call met a primitive Freq page (KIND_FILTER_FREQ), first half: the columns are
// decoded like a read -- values and validity into the staging area, the exceptions of Freq pages by the second pass, which
// needs the host and so cannot run inside the enqueue-only call -- and the sink's plain kernels take them from there.
// pages: the columns as read_col_of gives them; they live in iv.filter_tmp until the interval ends, and *out is where.
// what: the sink, for the error texts.
static int32_t decode_for_replay(sb_ctx* ctx, std::vector<sb_column_read>&& pages, const uint64_t* rows, const char* what, const sb_column_read** out) {
    ctx->iv.filter_tmp.push_back(std::move(pages));
    std::vector<sb_column_read>& rr = ctx->iv.filter_tmp.back();
    const uint64_t n = rr.size();
    size_t total = 0;
    for (uint64_t i = 0; i < n; i++)
        total += align_up(rows[i] * type_width(rr[i].physical_type), 64) + align_up((rows[i] + 31) / 32 * 4, 64);
    if (!ensure(ctx, ctx->filter_stage, total + 64)) return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(filter staging) failed");
    size_t so = 0;
    for (uint64_t i = 0; i < n; i++) {
        sb_column_read& r = rr[i];
        r.values = ctx->filter_stage.p + so;
        r.values_capacity = rows[i] * type_width(r.physical_type);
        so += align_up(r.values_capacity, 64);
        r.validity = ctx->filter_stage.p + so;
        r.validity_capacity = (rows[i] + 31) / 32 * 4;
        so += align_up(r.validity_capacity, 64);
    }
    int32_t rc = read_columns_impl(ctx, rr.data(), n, SB_MEM_DEVICE, ReadMode{ReadMode::READ});
    if (rc != SB_OK) return rc;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return ctx->fail(SB_ERR_EXTERNAL, std::string(what) + " replay: synchronize failed");
    *out = rr.data();
    return freq_second_pass(ctx);
}

// ... as the aggregate and key sinks begin their replay: the rows from the columns' AggCols, the decode, and the decoded
// columns as the plain kernels take them -- values and validity of each, and its slots in its AggCol: one per TILE_ROWS
// rows, the columns' back to back.
struct ReplayCols {
    std::vector<uint64_t> rows;
    std::vector<const uint8_t*> vals, bits;
    uint64_t slots = 0;
};
static int32_t open_replay(sb_ctx* ctx, std::vector<sb_column_read>&& pages, std::vector<AggCol>& hs, const char* what, ReplayCols& rp) {
    const size_t n = hs.size();
    rp.rows.resize(n);
    for (size_t i = 0; i < n; i++) rp.rows[i] = hs[i].rows;
    const sb_column_read* rr = nullptr;
    int32_t rc = decode_for_replay(ctx, std::move(pages), rp.rows.data(), what, &rr);
    if (rc != SB_OK) return rc;
    rp.vals.resize(n);
    rp.bits.resize(n);
    for (size_t i = 0; i < n; i++) {
        rp.vals[i] = (const uint8_t*)rr[i].values;
        rp.bits[i] = rr[i].is_nullable ? rr[i].validity : nullptr;
        hs[i].page_slot0 = hs[i].page_slots = 0;
        hs[i].tile_slot0 = rp.slots;
        hs[i].tile_slots = (rp.rows[i] + TILE_ROWS - 1) / TILE_ROWS;
        rp.slots += hs[i].tile_slots;
    }
    return SB_OK;
}
// ... the large grouped and the weighted sink: the columns' chunks back to back, in the tile slots' place.  Returns the slots.
static uint64_t chunk_slots(std::vector<AggCol>& hs) {
    uint64_t slots = 0;
    for (AggCol& g : hs) {
        g.tile_slot0 = slots;
        g.tile_slots = grpl_chunks(g.tile_slots);
        slots += g.tile_slots;
    }
    return slots;
}

// The temporary device buffer of one decoded call: sections at multiples of 64 in the order they are added, those with a
// host source uploaded once the buffer exists.  It belongs to the interval (iv.temp_dev) and is freed when that ends.
// what: the buffer, for the error texts.
extern "C++" {   // (a member template: not inside the C linkage of the entry points)
struct ReplayArena {
    struct Upload {
        size_t off;
        const void* host;
        size_t bytes;
    };
    uint8_t* dev = nullptr;
    size_t total = 0;
    std::vector<Upload> uploads;
    size_t add(size_t bytes) {
        const size_t off = align_up(total, 64);
        total = off + bytes;
        return off;
    }
    // (the source is read at the upload, not here.  A section of no bytes is not uploaded: the routes' struct arrays never
    // are one, a decoded call having a column at least, so only an empty blob of lists meets this)
    size_t add(const void* host, size_t bytes) {
        const size_t off = add(bytes);
        if (bytes) uploads.push_back(Upload{off, host, bytes});
        return off;
    }
    int32_t alloc(sb_ctx* ctx, const char* what) {
        if (hipMalloc((void**)&dev, total + 64) != hipSuccess) return ctx->fail(SB_ERR_EXTERNAL, std::string("hipMalloc(") + what + ") failed");
        ctx->iv.temp_dev.push_back(dev);
        return SB_OK;
    }
    // (copies that have ended when they return: their sources do not outlive the call)
    int32_t upload(sb_ctx* ctx, const std::string& failed) {
        for (const Upload& u : uploads)
            if (hipMemcpy(dev + u.off, u.host, u.bytes, hipMemcpyHostToDevice) != hipSuccess) return ctx->fail(SB_ERR_EXTERNAL, failed);
        return SB_OK;
    }
    // both; a call whose sections hold addresses of the buffer itself takes the two steps apart
    int32_t commit(sb_ctx* ctx, const char* what) {
        const int32_t rc = alloc(ctx, what);
        return rc != SB_OK ? rc : upload(ctx, std::string(what) + ": upload failed");
    }
    template <class T>
    T* at(size_t off) const {
        return (T*)(dev + off);
    }
};
}   // extern "C++"

// ... second half: the plain kernels are launched, and their results -- `stride` bytes per column at d_res -- travel to
// the slot, which was acquired before the launches, and from there to the callers at the synchronize.
static int32_t queue_sink_results(sb_ctx* ctx, StageSlot* slot, const void* d_res, size_t stride, uint64_t n, Pending::Kind kind, void* const* users,
                                  const GrpCol* grpc, const char* what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(slot->host, d_res, n * stride, hipMemcpyDeviceToHost, ctx->stream);
    if (e != hipSuccess) return check_hip(ctx, e, (std::string(what) + " replay").c_str());
    (void)hipEventRecord(slot->done, ctx->stream);
    slot->in_flight = true;
    push_pending(ctx, kind, users, slot->host, stride, n, grpc);
    return SB_OK;
}

// ------------------------------------------------------------------------------------ filter
// The numeric comparison columns of a replayed filter call: decoded, and compared from the staging area.
static int32_t filter_columns_decoded(sb_ctx* ctx, std::vector<sb_column_read>&& pages, const uint64_t* rows, const FilterCol* hf, void* const* sel_out) {
    hipStream_t s = ctx->stream;
    const uint64_t m = pages.size();
    const sb_column_read* rr = nullptr;
    int32_t rc = decode_for_replay(ctx, std::move(pages), rows, "filter", &rr);
    if (rc != SB_OK) return rc;
    // [bits set per column]
    ReplayArena a;
    const size_t o_counts = a.add(m * sizeof(uint64_t));
    if ((rc = a.commit(ctx, "filter counts")) != SB_OK) return rc;
    StageSlot* slot = acquire_slot(ctx, m * sizeof(uint64_t));
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    uint64_t* d_counts = a.at<uint64_t>(o_counts);
    for (uint64_t i = 0; i < m; i++) {
        if (hf[i].combine == SB_SEL_SET && rows[i]) (void)hipMemsetAsync(hf[i].sel, 0, (rows[i] + 31) / 32 * 4, s);
        launch_filter_plain(ctx, hf[i], (const uint8_t*)rr[i].values, rr[i].is_nullable ? rr[i].validity : nullptr, rows[i],
                            type_width(rr[i].physical_type), d_counts + i);
    }
    return queue_sink_results(ctx, slot, d_counts, sizeof(uint64_t), m, Pending::FILTER_COL, sel_out, nullptr, "filter");
}

// FilterCol.mask of the string ops (sb_filter_bin.h, sb_filter_sub.h); 0: not one of them
static uint32_t filter_str_mask(int32_t op) {
    switch (op) {
        case SB_PRED_STARTS_WITH:
            return FILTER_MASK_PREFIX;
        case SB_PRED_ENDS_WITH:
            return FILTER_MASK_SUFFIX;
        case SB_PRED_CONTAINS:
            return FILTER_MASK_SUBSTR;
        case SB_PRED_NOT_STARTS_WITH:
            return FILTER_MASK_PREFIX | FILTER_MASK_NOT;
        case SB_PRED_NOT_ENDS_WITH:
            return FILTER_MASK_SUFFIX | FILTER_MASK_NOT;
        case SB_PRED_NOT_CONTAINS:
            return FILTER_MASK_SUBSTR | FILTER_MASK_NOT;
        default:
            return 0;
    }
}

// Both entry points end here.  `cols` is the call in the var layout (sb_filter_columns copies its columns into one that
// lives for the call); results[i] are the caller's own { rows, selected } words, which outlive the call.
static int32_t filter_impl(sb_ctx* ctx, const sb_column_filter_var* cols, uint64_t* const* results, uint64_t n) {
    std::vector<FilterCol> hf(n);
    std::vector<sb_column_filter_var> work(cols, cols + n);   // (with rows and the default stage_capacity filled in)
    std::vector<uint8_t> lits;   // the binary literals, each at a multiple of 8 and followed by 8 zero bytes
    for (uint64_t i = 0; i < n; i++) {
        sb_column_filter_var& c = work[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
        const bool str_op = c.op == SB_PRED_STARTS_WITH || (c.op >= SB_PRED_ENDS_WITH && c.op <= SB_PRED_NOT_CONTAINS);
        if (c.op < SB_PRED_EQ || (c.op > SB_PRED_IS_NOT_NULL && !str_op)) return refuse(ctx, SB_ERR_INVALID, "bad op");
        if (c.combine < SB_SEL_SET || c.combine > SB_SEL_OR) return refuse(ctx, SB_ERR_INVALID, "bad combine");
        const bool null_op = c.op == SB_PRED_IS_NULL || c.op == SB_PRED_IS_NOT_NULL;
        const bool bin = is_binary_t(c.physical_type);
        if (str_op && !bin) return refuse(ctx, SB_ERR_INVALID, "STARTS_WITH / ENDS_WITH / CONTAINS and their NOT_ forms need a Binary / LargeBinary column");
        if (!null_op && !bin && !filter_comparable(c.physical_type))
            return refuse(ctx, SB_ERR_NYI, "comparison predicates are implemented for 8- to 64-bit integers, floats and binary types");
        if (!null_op) {
            if (!bin && c.literal_len != type_width(c.physical_type)) return refuse(ctx, SB_ERR_INVALID, "literal_len is not the width of the column's type");
            if (bin && c.literal_len > (1ull << 30)) return refuse(ctx, SB_ERR_INVALID, "a binary literal has at most 2^30 bytes");
            if (c.literal_len && !c.literal) return refuse(ctx, SB_ERR_INVALID, "literal is null");
        }
        uint64_t rows = 0;
        if (!column_rows(c, &rows)) return refuse(ctx, SB_ERR_INVALID, "metas is null");
        const uint64_t sel_bytes = (rows + 31) / 32 * 4;
        if (rows && (!c.selection || ((uintptr_t)c.selection & 3) || c.selection_capacity < sel_bytes))
            return refuse(ctx, SB_ERR_INVALID, "selection missing, not 4-byte aligned or smaller than 4*ceil(rows/32) bytes");
        for (uint64_t j = 0; j < i && rows; j++)
            if (work[j].rows && c.selection < work[j].selection + (work[j].rows + 31) / 32 * 4 && work[j].selection < c.selection + sel_bytes)
                return refuse(ctx, SB_ERR_INVALID, "two columns of one call share a selection buffer: chain them with two calls");
        c.rows = rows;
    }
    std::vector<sb_column_read> rc_cols(n);
    std::vector<uint64_t> rows(n), cap(n);   // (cap: the column's share of the staging area)
    std::vector<void*> sel_out(n);           // the callers' `selected`
    for (uint64_t i = 0; i < n; i++) {
        sb_column_filter_var& c = work[i];
        const bool null_op = c.op == SB_PRED_IS_NULL || c.op == SB_PRED_IS_NOT_NULL;
        results[i][0] = c.rows;
        results[i][1] = 0;
        sel_out[i] = results[i] + 1;
        rc_cols[i] = read_col_of(c);
        rows[i] = c.rows;
        cap[i] = NO_SHARE;
        FilterCol& f = hf[i];
        memset(&f, 0, sizeof f);
        f.sel = (uint32_t*)c.selection;
        const uint32_t str_mask = filter_str_mask(c.op);
        f.op = str_mask ? (uint32_t)SB_PRED_EQ : (uint32_t)c.op;   // (the kernels tell null tests by op >= IS_NULL; a prefix / suffix / substring test by its mask)
        f.combine = (uint32_t)c.combine;
        f.ptype = c.physical_type;
        if (null_op) continue;
        static const uint32_t MASKS[6] = {2u, 13u, 1u, 3u, 4u, 6u};   // EQ NE LT LE GT GE over (less, equal, greater, unordered)
        f.mask = str_mask ? str_mask : MASKS[c.op];
        if (is_binary_t(c.physical_type)) {
            f.kind = FK_BYTES;
            f.lit_len = (uint32_t)c.literal_len;
            lits.resize(align_up(lits.size(), 8));
            f.lit = lits.size();   // (offset in `lits`; read_columns_impl makes it the device address)
            if (c.literal_len) lits.insert(lits.end(), c.literal, c.literal + c.literal_len);
            lits.insert(lits.end(), 8, (uint8_t)0);
            if (!c.stage_capacity) c.stage_capacity = 4 * c.pages_len;
            cap[i] = c.stage_capacity;
            continue;
        }
        // the literal widened to the 8 bytes the kernels compare: floats as doubles, signed integers sign-extended
        const uint32_t w = type_width(c.physical_type);
        uint64_t raw = 0;
        memcpy(&raw, c.literal, w);
        f.kind = value_kind(c.physical_type);
        f.lit = raw;
        if (f.kind == FK_F32) {
            float v;
            memcpy(&v, c.literal, 4);
            const double dv = (double)v;
            memcpy(&f.lit, &dv, 8);
        } else if (f.kind == FK_SIGNED) {
            const uint32_t sh = 64 - 8 * w;
            f.lit = (uint64_t)((int64_t)(raw << sh) >> sh);
        }
        cap[i] = c.rows * w;
    }
    (void)hipSetDevice(ctx->device);
    int32_t rc = SB_OK;
    if (ctx->in_replay && ctx->filter_freq) {
        // IS_[NOT_]NULL and binary columns as ever; the numeric comparison columns through a full decode
        std::vector<bool> dec(n);
        for (uint64_t i = 0; i < n; i++) dec[i] = hf[i].op < SB_PRED_IS_NULL && hf[i].kind != FK_BYTES;
        std::vector<sb_column_read> r_cmp = take_if(rc_cols, dec);
        const std::vector<uint64_t> n_cmp = take_if(rows, dec);
        const std::vector<FilterCol> f_cmp = take_if(hf, dec);
        const std::vector<void*> s_cmp = take_if(sel_out, dec);
        take_if(cap, dec);
        if (!r_cmp.empty()) rc = filter_columns_decoded(ctx, std::move(r_cmp), n_cmp.data(), f_cmp.data(), s_cmp.data());
        if (rc != SB_OK || rc_cols.empty()) return rc;
    }
    if ((rc = stage_shares(ctx, rc_cols.data(), cap.data(), rc_cols.size())) != SB_OK) return rc;
    ReadMode mode{ReadMode::FILTER};
    mode.filt = hf.data();
    mode.lits = &lits;
    mode.users = sel_out.data();
    mode.pending_kind = Pending::FILTER_COL;
    return read_columns_impl(ctx, rc_cols.data(), rc_cols.size(), SB_MEM_DEVICE, mode);
}

int32_t sb_filter_columns_var(sb_ctx* ctx, sb_column_filter_var* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_filter_columns_var", &rc)) return rc;
    std::vector<uint64_t*> results(n);
    for (uint64_t i = 0; i < n; i++) results[i] = &cols[i].rows;   // { rows, selected }
    rc = filter_impl(ctx, cols, results.data(), n);
    if (rc == SB_OK && !ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::FILTER_VAR, cols, n, sb_write_options{}, mem});
    return rc;
}

int32_t sb_filter_columns(sb_ctx* ctx, sb_column_filter* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_filter_columns", &rc)) return rc;
    // the eight inline literal bytes hold numbers only: everything else this entry point refused before stays refused
    std::vector<sb_column_filter_var> v(n);
    std::vector<uint64_t*> results(n);
    for (uint64_t i = 0; i < n; i++) {
        sb_column_filter& c = cols[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
        if (c.op < SB_PRED_EQ || c.op > SB_PRED_IS_NOT_NULL) return refuse(ctx, SB_ERR_INVALID, "bad op");
        if (c.op < SB_PRED_IS_NULL && !filter_comparable(c.physical_type))
            return refuse(ctx, SB_ERR_NYI, "comparison predicates are implemented for 8- to 64-bit integers and floats");
        sb_column_filter_var& d = v[i];
        memset(&d, 0, sizeof d);
        d.physical_type = c.physical_type;
        d.is_nullable = c.is_nullable;
        d.pages = c.pages;
        d.pages_len = c.pages_len;
        d.metas = c.metas;
        d.n_pages = c.n_pages;
        d.page_offsets = c.page_offsets;
        d.op = c.op;
        d.combine = c.combine;
        d.literal = c.literal;
        d.literal_len = c.op < SB_PRED_IS_NULL ? type_width(c.physical_type) : 0;
        d.selection = c.selection;
        d.selection_capacity = c.selection_capacity;
        static_assert(offsetof(sb_column_filter, selected) == offsetof(sb_column_filter, rows) + 8, "{ rows, selected }");
        results[i] = &c.rows;
    }
    rc = filter_impl(ctx, v.data(), results.data(), n);
    if (rc == SB_OK && !ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::FILTER, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ IN / NOT IN
// The list of a column as the kernels search it (sb_filter_in.h), appended to `blob` at a multiple of 8; ic's pointers are
// offsets in `blob` until the tables have their place.  Numbers: order keys, sorted, without duplicates and without NaNs.
// Binary: the literals sorted as byte strings, without duplicates, as [n + 1 offsets | bytes | 8 zero bytes].
static void in_set_append(const sb_column_filter_in& c, uint32_t kind, std::vector<uint8_t>& blob, InCol* ic) {
    blob.resize(align_up(blob.size(), 8));
    memset(ic, 0, sizeof *ic);
    ic->negate = c.op == SB_PRED_NOT_IN;
    std::vector<uint64_t> words;   // the keys, or the offsets
    std::vector<uint8_t> bytes;
    if (kind == FK_BYTES) {
        struct Lit {
            const uint8_t* p;
            uint64_t len;
        };
        std::vector<Lit> lits(c.n_values);
        for (uint64_t j = 0; j < c.n_values; j++) lits[j] = Lit{c.values + c.value_offsets[j], c.value_offsets[j + 1] - c.value_offsets[j]};
        auto cmp3 = [](const Lit& a, const Lit& b) {
            const uint64_t m = std::min(a.len, b.len);
            const int r = m ? memcmp(a.p, b.p, m) : 0;
            return r ? r : a.len < b.len ? -1 : a.len > b.len ? 1 : 0;
        };
        std::sort(lits.begin(), lits.end(), [&](const Lit& a, const Lit& b) { return cmp3(a, b) < 0; });
        lits.erase(std::unique(lits.begin(), lits.end(), [&](const Lit& a, const Lit& b) { return cmp3(a, b) == 0; }), lits.end());
        words.push_back(0);
        for (const Lit& l : lits) {
            if (l.len) bytes.insert(bytes.end(), l.p, l.p + l.len);
            words.push_back(bytes.size());
        }
        bytes.insert(bytes.end(), 8, (uint8_t)0);
        ic->n = (uint32_t)lits.size();
    } else {
        const uint32_t w = type_width(c.physical_type);
        for (uint64_t j = 0; j < c.n_values; j++) {
            uint64_t raw = 0;
            memcpy(&raw, c.values + j * w, w);
            if (kind == FK_F32 && (raw & 0x7FFFFFFFull) > 0x7F800000ull) continue;   // NaN: matches nothing
            if (kind == FK_F64 && (raw & ~(1ull << 63)) > 0x7FF0000000000000ull) continue;
            words.push_back(in_key(kind, w, raw));
        }
        std::sort(words.begin(), words.end());
        words.erase(std::unique(words.begin(), words.end()), words.end());
        ic->n = (uint32_t)words.size();
    }
    while ((1ull << ic->steps) < (uint64_t)ic->n + 1) ic->steps++;
    ic->keys = (const uint64_t*)(uintptr_t)blob.size();
    blob.insert(blob.end(), (const uint8_t*)words.data(), (const uint8_t*)(words.data() + words.size()));
    ic->bytes = (const uint8_t*)(uintptr_t)blob.size();
    blob.insert(blob.end(), bytes.begin(), bytes.end());
}

// The numeric columns of a replayed IN call: decoded, and searched from the staging area (filter_columns_decoded with the
// sets, which go to the device in a buffer of the interval's)
static int32_t filter_in_columns_decoded(sb_ctx* ctx, std::vector<sb_column_read>&& pages, const uint64_t* rows, const FilterCol* hf,
                                         const InCol* hic, const std::vector<uint8_t>& blob, void* const* sel_out) {
    hipStream_t s = ctx->stream;
    const uint64_t m = pages.size();
    const sb_column_read* rr = nullptr;
    int32_t rc = decode_for_replay(ctx, std::move(pages), rows, "filter", &rr);
    if (rc != SB_OK) return rc;
    // [bits set per column][the sets]
    ReplayArena a;
    const size_t o_counts = a.add(m * sizeof(uint64_t));
    const size_t o_sets = a.add(blob.data(), blob.size());
    if ((rc = a.alloc(ctx, "filter counts")) != SB_OK || (rc = a.upload(ctx, "H2D of the lists failed")) != SB_OK) return rc;
    StageSlot* slot = acquire_slot(ctx, m * sizeof(uint64_t));
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    uint64_t* d_counts = a.at<uint64_t>(o_counts);
    for (uint64_t i = 0; i < m; i++) {
        if (hf[i].combine == SB_SEL_SET && rows[i]) (void)hipMemsetAsync(hf[i].sel, 0, (rows[i] + 31) / 32 * 4, s);
        InCol ic = hic[i];
        rebase(ic, a.at<uint8_t>(o_sets));
        launch_filter_in_plain(ctx, hf[i], ic, (const uint8_t*)rr[i].values, rr[i].is_nullable ? rr[i].validity : nullptr, rows[i],
                               type_width(rr[i].physical_type), d_counts + i);
    }
    return queue_sink_results(ctx, slot, d_counts, sizeof(uint64_t), m, Pending::FILTER_COL, sel_out, nullptr, "filter");
}

static_assert(sizeof(sb_column_filter_in) == 120 && offsetof(sb_column_filter_in, op) == 48 && offsetof(sb_column_filter_in, values) == 56 &&
                  offsetof(sb_column_filter_in, value_offsets) == 64 && offsetof(sb_column_filter_in, n_values) == 72 &&
                  offsetof(sb_column_filter_in, selection) == 80 && offsetof(sb_column_filter_in, stage_capacity) == 96 &&
                  offsetof(sb_column_filter_in, rows) == 104 && offsetof(sb_column_filter_in, selected) == 112 && has_pages_prefix<sb_column_filter_in>(),
              "sb_column_filter_in: the offsets the header states");

int32_t sb_filter_columns_in(sb_ctx* ctx, sb_column_filter_in* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_filter_columns_in", &rc)) return rc;
    std::vector<uint64_t> rows(n), cap(n);
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_filter_in& c = cols[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
        if (c.op != SB_PRED_IN && c.op != SB_PRED_NOT_IN) return refuse(ctx, SB_ERR_INVALID, "bad op: SB_PRED_IN or SB_PRED_NOT_IN");
        if (c.combine < SB_SEL_SET || c.combine > SB_SEL_OR) return refuse(ctx, SB_ERR_INVALID, "bad combine");
        const bool bin = is_binary_t(c.physical_type);
        if (!bin && !filter_comparable(c.physical_type))
            return refuse(ctx, SB_ERR_NYI, "IN lists are implemented for 8- to 64-bit integers, floats and binary types");
        if (c.n_values > SB_IN_MAX_VALUES) return refuse(ctx, SB_ERR_INVALID, "n_values exceeds SB_IN_MAX_VALUES");
        if (!bin) {
            if (c.value_offsets) return refuse(ctx, SB_ERR_INVALID, "value_offsets on a numeric column");
            if (c.n_values && !c.values) return refuse(ctx, SB_ERR_INVALID, "values is null");
        } else if (c.n_values) {
            if (!c.value_offsets) return refuse(ctx, SB_ERR_INVALID, "value_offsets is null");
            if (c.value_offsets[0] != 0) return refuse(ctx, SB_ERR_INVALID, "value_offsets[0] is not 0");
            for (uint64_t j = 0; j < c.n_values; j++)
                if (c.value_offsets[j + 1] < c.value_offsets[j]) return refuse(ctx, SB_ERR_INVALID, "value_offsets descend");
            if (c.value_offsets[c.n_values] > (1ull << 30)) return refuse(ctx, SB_ERR_INVALID, "the literals of a column have at most 2^30 bytes");
            if (c.value_offsets[c.n_values] && !c.values) return refuse(ctx, SB_ERR_INVALID, "values is null");
        }
        if (!column_rows(c, &rows[i])) return refuse(ctx, SB_ERR_INVALID, "metas is null");
        const uint64_t sel_bytes = (rows[i] + 31) / 32 * 4;
        if (rows[i] && (!c.selection || ((uintptr_t)c.selection & 3) || c.selection_capacity < sel_bytes))
            return refuse(ctx, SB_ERR_INVALID, "selection missing, not 4-byte aligned or smaller than 4*ceil(rows/32) bytes");
        for (uint64_t j = 0; j < i && rows[i]; j++)
            if (rows[j] && c.selection < cols[j].selection + (rows[j] + 31) / 32 * 4 && cols[j].selection < c.selection + sel_bytes)
                return refuse(ctx, SB_ERR_INVALID, "two columns of one call share a selection buffer: chain them with two calls");
    }
    // [InCol per column | the sets], FilterCol per column beside
    std::vector<uint8_t> blob(align_up(n * sizeof(InCol), 64));
    std::vector<InCol> hic(n);
    std::vector<FilterCol> hf(n);
    std::vector<sb_column_read> rc_cols(n);
    std::vector<void*> sel_out(n);
    for (uint64_t i = 0; i < n; i++) {
        sb_column_filter_in& c = cols[i];
        c.rows = rows[i];
        c.selected = 0;
        static_assert(offsetof(sb_column_filter_in, selected) == offsetof(sb_column_filter_in, rows) + 8, "{ rows, selected }");
        sel_out[i] = &c.selected;
        rc_cols[i] = read_col_of(c);
        const bool bin = is_binary_t(c.physical_type);
        FilterCol& f = hf[i];
        memset(&f, 0, sizeof f);
        f.sel = (uint32_t*)c.selection;
        f.op = (uint32_t)c.op;
        f.combine = (uint32_t)c.combine;
        f.ptype = c.physical_type;
        f.kind = bin ? FK_BYTES : value_kind(c.physical_type);
        in_set_append(c, f.kind, blob, &hic[i]);
        // the share of the staging area a comparison column has (the caller's stage_capacity stays as given: a replay reads it again)
        cap[i] = bin ? (c.stage_capacity ? c.stage_capacity : 4 * c.pages_len) : rows[i] * type_width(c.physical_type);
    }
    (void)hipSetDevice(ctx->device);
    const bool first_issue = !ctx->in_replay;
    if (ctx->in_replay && ctx->filter_freq) {
        // binary columns as ever; the numeric columns through a full decode
        std::vector<bool> dec(n);
        for (uint64_t i = 0; i < n; i++) dec[i] = hf[i].kind != FK_BYTES;
        std::vector<sb_column_read> r_cmp = take_if(rc_cols, dec);
        const std::vector<uint64_t> n_cmp = take_if(rows, dec);
        const std::vector<FilterCol> f_cmp = take_if(hf, dec);
        const std::vector<InCol> i_cmp = take_if(hic, dec);
        const std::vector<void*> s_cmp = take_if(sel_out, dec);
        take_if(cap, dec);
        if (!r_cmp.empty()) rc = filter_in_columns_decoded(ctx, std::move(r_cmp), n_cmp.data(), f_cmp.data(), i_cmp.data(), blob, s_cmp.data());
        if (rc != SB_OK || rc_cols.empty()) return rc;
    }
    const uint64_t m = rc_cols.size();
    memcpy(blob.data(), hic.data(), m * sizeof(InCol));
    if ((rc = stage_shares(ctx, rc_cols.data(), cap.data(), m)) != SB_OK) return rc;
    ReadMode mode{ReadMode::FILTER};
    mode.filt = hf.data();
    mode.lits = &blob;
    mode.in_list = true;
    mode.users = sel_out.data();
    mode.pending_kind = Pending::FILTER_COL;
    rc = read_columns_impl(ctx, rc_cols.data(), m, SB_MEM_DEVICE, mode);
    if (rc == SB_OK && first_issue) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::FILTER_IN, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ column against column
static_assert(sizeof(sb_column_filter_cmp) == 136 && offsetof(sb_column_filter_cmp, op) == 48 && offsetof(sb_column_filter_cmp, combine) == 52 &&
                  offsetof(sb_column_filter_cmp, other) == 56 && offsetof(sb_column_filter_cmp, other_capacity) == 64 &&
                  offsetof(sb_column_filter_cmp, other_validity) == 72 && offsetof(sb_column_filter_cmp, other_validity_capacity) == 80 &&
                  offsetof(sb_column_filter_cmp, other_type) == 88 && offsetof(sb_column_filter_cmp, flags) == 92 &&
                  offsetof(sb_column_filter_cmp, reserved) == 96 && offsetof(sb_column_filter_cmp, selection) == 104 &&
                  offsetof(sb_column_filter_cmp, selection_capacity) == 112 && offsetof(sb_column_filter_cmp, rows) == 120 &&
                  offsetof(sb_column_filter_cmp, selected) == 128,
              "sb_column_filter_cmp: the offsets the header states");
static_assert(offsetof(sb_column_filter_cmp, op) == offsetof(sb_column_filter, op) && offsetof(sb_column_filter_cmp, combine) == offsetof(sb_column_filter, combine) &&
                  offsetof(sb_column_filter, literal) == 56,
              "the first 56 bytes are sb_column_filter's");

// The columns of a replayed call: decoded, and compared from the staging area (filter_columns_decoded with the operands,
// which are the callers' own device buffers)
static int32_t filter_cmp_columns_decoded(sb_ctx* ctx, std::vector<sb_column_read>&& pages, const uint64_t* rows, const FilterCol* hf, const CmpCol* hcc,
                                          void* const* sel_out) {
    hipStream_t s = ctx->stream;
    const uint64_t m = pages.size();
    const sb_column_read* rr = nullptr;
    int32_t rc = decode_for_replay(ctx, std::move(pages), rows, "filter", &rr);
    if (rc != SB_OK) return rc;
    // [bits set per column]
    ReplayArena a;
    const size_t o_counts = a.add(m * sizeof(uint64_t));
    if ((rc = a.commit(ctx, "filter counts")) != SB_OK) return rc;
    StageSlot* slot = acquire_slot(ctx, m * sizeof(uint64_t));
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    uint64_t* d_counts = a.at<uint64_t>(o_counts);
    for (uint64_t i = 0; i < m; i++) {
        if (hf[i].combine == SB_SEL_SET && rows[i]) (void)hipMemsetAsync(hf[i].sel, 0, (rows[i] + 31) / 32 * 4, s);
        launch_filter_cmp_plain(ctx, hf[i], hcc[i], (const uint8_t*)rr[i].values, rr[i].is_nullable ? rr[i].validity : nullptr, rows[i],
                                type_width(rr[i].physical_type), d_counts + i);
    }
    return queue_sink_results(ctx, slot, d_counts, sizeof(uint64_t), m, Pending::FILTER_CMP_COL, sel_out, nullptr, "filter");
}

int32_t sb_filter_columns_cmp(sb_ctx* ctx, sb_column_filter_cmp* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_filter_columns_cmp", &rc)) return rc;
    std::vector<uint64_t> rows(n), cap(n);
    auto overlap = [](const uint8_t* a, uint64_t an, const uint8_t* b, uint64_t bn) { return an && bn && a < b + bn && b < a + an; };
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_filter_cmp& c = cols[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
        if (c.other_type < 0 || c.other_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad other_type");
        if (c.op < SB_PRED_EQ || c.op > SB_PRED_GE) return refuse(ctx, SB_ERR_INVALID, "bad op: SB_PRED_EQ .. SB_PRED_GE");
        if (c.combine < SB_SEL_SET || c.combine > SB_SEL_OR) return refuse(ctx, SB_ERR_INVALID, "bad combine");
        if (c.flags) return refuse(ctx, SB_ERR_INVALID, "flags is not 0");
        if (c.reserved) return refuse(ctx, SB_ERR_INVALID, "reserved is not 0");
        if (!filter_comparable(c.physical_type) || !filter_comparable(c.other_type))
            return refuse(ctx, SB_ERR_NYI, "column comparisons are implemented for 8- to 64-bit integers and floats on both sides");
        if (!column_rows(c, &rows[i])) return refuse(ctx, SB_ERR_INVALID, "metas is null");
        const uint64_t r = rows[i], sel_bytes = (r + 31) / 32 * 4, ow = type_width(c.other_type);
        if (r && (!c.selection || ((uintptr_t)c.selection & 3) || c.selection_capacity < sel_bytes))
            return refuse(ctx, SB_ERR_INVALID, "selection missing, not 4-byte aligned or smaller than 4*ceil(rows/32) bytes");
        if (r && !c.other) return refuse(ctx, SB_ERR_INVALID, "other is null");
        if (c.other && (((uintptr_t)c.other & (ow - 1)) || c.other_capacity < r * ow))
            return refuse(ctx, SB_ERR_INVALID, "other not aligned to its width or smaller than rows * width bytes");
        if (!c.other_validity && c.other_validity_capacity) return refuse(ctx, SB_ERR_INVALID, "other_validity_capacity without other_validity");
        if (c.other_validity && (((uintptr_t)c.other_validity & 3) || c.other_validity_capacity < sel_bytes))
            return refuse(ctx, SB_ERR_INVALID, "other_validity not 4-byte aligned or smaller than 4*ceil(rows/32) bytes");
        if (overlap(c.selection, sel_bytes, c.other, r * ow) || (c.other_validity && overlap(c.selection, sel_bytes, c.other_validity, sel_bytes)))
            return refuse(ctx, SB_ERR_INVALID, "selection overlaps other or other_validity");
        for (uint64_t j = 0; j < i; j++)
            if (overlap(c.selection, sel_bytes, cols[j].selection, (rows[j] + 31) / 32 * 4))
                return refuse(ctx, SB_ERR_INVALID, "two columns of one call share a selection buffer: chain them with two calls");
        cap[i] = r * type_width(c.physical_type);   // the share of the staging area a comparison column has
    }
    // [CmpCol per column] in the literals' place, FilterCol per column beside
    std::vector<uint8_t> blob(n * sizeof(CmpCol));
    std::vector<CmpCol> hcc(n);
    std::vector<FilterCol> hf(n);
    std::vector<sb_column_read> rc_cols(n);
    std::vector<void*> sel_out(n);
    for (uint64_t i = 0; i < n; i++) {
        sb_column_filter_cmp& c = cols[i];
        static_assert(offsetof(sb_column_filter_cmp, selected) == offsetof(sb_column_filter_cmp, rows) + 8, "{ rows, selected }");
        sel_out[i] = &c.selected;
        rc_cols[i] = read_col_of(c);
        FilterCol& f = hf[i];
        memset(&f, 0, sizeof f);
        static const uint32_t MASKS[6] = {2u, 13u, 1u, 3u, 4u, 6u};   // EQ NE LT LE GT GE over (less, equal, greater, unordered)
        f.sel = (uint32_t*)c.selection;
        f.kind = value_kind(c.physical_type);
        f.mask = MASKS[c.op];
        f.op = (uint32_t)c.op;
        f.combine = (uint32_t)c.combine;
        f.ptype = c.physical_type;
        hcc[i] = CmpCol{c.other, (const uint32_t*)c.other_validity, value_kind(c.other_type), type_width(c.other_type)};
    }
    if (n) memcpy(blob.data(), hcc.data(), n * sizeof(CmpCol));
    (void)hipSetDevice(ctx->device);
    if (ctx->in_replay && ctx->filter_freq) {
        // every column through a full decode, as sb_filter_columns has its comparison columns.  The bits are a function of
        // the data and the struct alone, so the route does not show in them.
        rc = filter_cmp_columns_decoded(ctx, std::move(rc_cols), rows.data(), hf.data(), hcc.data(), sel_out.data());
    } else {
        if ((rc = stage_shares(ctx, rc_cols.data(), cap.data(), n)) != SB_OK) return rc;
        ReadMode mode{ReadMode::FILTER_CMP};
        mode.filt = hf.data();
        mode.lits = &blob;
        mode.users = sel_out.data();
        mode.pending_kind = Pending::FILTER_CMP_COL;
        rc = read_columns_impl(ctx, rc_cols.data(), n, SB_MEM_DEVICE, mode);
    }
    if (rc != SB_OK) return rc;
    for (uint64_t i = 0; i < n; i++) {   // (after the last thing that can refuse the call: a page outside pages_len)
        cols[i].rows = rows[i];
        cols[i].selected = 0;
    }
    if (!ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::FILTER_CMP, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ selected read
// The columns of a replayed call: decoded, and compacted from the staging area by k_rsel_plain with the same sink.
static int32_t rsel_columns_decoded(sb_ctx* ctx, std::vector<sb_column_read>&& pages, const uint64_t* rows, std::vector<SelCol>& hs, void* const* users) {
    const uint64_t n = pages.size();
    const sb_column_read* rr = nullptr;
    int32_t rc = decode_for_replay(ctx, std::move(pages), rows, "selected-read", &rr);
    if (rc != SB_OK) return rc;
    // [SelCol per column][bits set per column][the rank tables, each at a multiple of 16]
    std::vector<size_t> rank_off(n);
    size_t rank_bytes = 0;
    for (uint64_t i = 0; i < n; i++) {
        rank_off[i] = rank_bytes;
        rank_bytes += align_up(rsel_rank_words(rows[i]) * 8, 16);
    }
    ReplayArena a;
    const size_t o_sc = a.add(hs.data(), n * sizeof(SelCol));
    const size_t o_counts = a.add(n * sizeof(uint64_t));
    const size_t o_rank = a.add(rank_bytes);
    if ((rc = a.alloc(ctx, "selected-read replay")) != SB_OK) return rc;
    std::vector<const uint8_t*> vals(n), bits(n);
    bool any_nullable = false;
    for (uint64_t i = 0; i < n; i++) {
        hs[i].rank = a.at<uint64_t>(o_rank + rank_off[i]);
        vals[i] = (const uint8_t*)rr[i].values;
        bits[i] = rr[i].is_nullable ? rr[i].validity : nullptr;
        if (hs[i].validity) any_nullable = true;
    }
    if ((rc = a.upload(ctx, "selected-read replay: upload failed")) != SB_OK) return rc;
    StageSlot* slot = acquire_slot(ctx, n * sizeof(uint64_t));
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    uint64_t* d_counts = a.at<uint64_t>(o_counts);
    launch_rsel_plain(ctx, a.at<const SelCol>(o_sc), (uint32_t)n, d_counts, any_nullable, rows, vals.data(), bits.data());
    return queue_sink_results(ctx, slot, d_counts, sizeof(uint64_t), n, Pending::RSEL_COL, users, nullptr, "selected-read");
}

// What sb_read_selected and sb_read_selected_var check of a column's arguments behind their own type checks, and of
// the call's buffers together: one definition, so that the two entry points refuse the same things.  The message of the
// refusal (SB_ERR_INVALID) or null.
extern "C++" {   // (a template: not inside the C linkage of the entry points)
struct SelSpan {
    const uint8_t* p;
    uint64_t len;
};
struct SelSpans {
    std::vector<SelSpan> outs, sels;   // the outputs and the selections of the call (an entry point adds outputs of its own)
};
template <class Col>
static const char* sel_check_column(const Col& c, SelSpans& sp, uint64_t* rows) {
    if (!column_rows(c, rows)) return "metas is null";
    const uint64_t r = *rows;
    const uint64_t sel_bytes = (r + 31) / 32 * 4;
    if (r && (!c.selection || ((uintptr_t)c.selection & 3) || c.selection_capacity < sel_bytes))
        return "selection missing, not 4-byte aligned or smaller than 4*ceil(rows/32) bytes";
    if (c.values_capacity && !c.values) return "values is null";
    if (r && c.is_nullable && (!c.validity || ((uintptr_t)c.validity & 3))) return "validity buffer of a nullable column missing or not 4-byte aligned";
    if (r) sp.sels.push_back({c.selection, sel_bytes});
    if (c.values && c.values_capacity) sp.outs.push_back({(const uint8_t*)c.values, c.values_capacity});
    if (c.is_nullable && c.validity && c.validity_capacity) sp.outs.push_back({c.validity, c.validity_capacity});
    return nullptr;
}
static const char* sel_check_overlaps(const SelSpans& sp) {
    auto overlap = [](const SelSpan& a, const SelSpan& b) { return a.p < b.p + b.len && b.p < a.p + a.len; };
    for (size_t i = 0; i < sp.outs.size(); i++) {
        for (size_t j = 0; j < i; j++)
            if (overlap(sp.outs[i], sp.outs[j])) return "output buffers of one call overlap";
        for (const SelSpan& s : sp.sels)
            if (overlap(sp.outs[i], s)) return "an output buffer overlaps a selection of the call";
    }
    return nullptr;
}
}   // extern "C++"

int32_t sb_read_selected(sb_ctx* ctx, sb_column_read_selected* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_read_selected", &rc)) return rc;
    std::vector<uint64_t> rows(n);
    SelSpans sp;
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_read_selected& c = cols[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
        if (!filter_comparable(c.physical_type))
            return refuse(ctx, SB_ERR_NYI, "sb_read_selected is implemented for 8- to 64-bit integers and floats");
        if (const char* msg = sel_check_column(c, sp, &rows[i])) return refuse(ctx, SB_ERR_INVALID, msg);
    }
    if (const char* msg = sel_check_overlaps(sp)) return refuse(ctx, SB_ERR_INVALID, msg);
    std::vector<SelCol> hs(n);
    std::vector<sb_column_read> rc_cols(n);
    std::vector<void*> users(n);
    std::vector<uint64_t> cap(n);
    for (uint64_t i = 0; i < n; i++) {
        sb_column_read_selected& c = cols[i];
        c.rows = rows[i];
        c.selected = 0;
        c.values_len = 0;
        users[i] = &c;
        rc_cols[i] = read_col_of(c);
        SelCol& sc = hs[i];
        memset(&sc, 0, sizeof sc);
        sc.w = type_width(c.physical_type);
        sc.sel = (const uint32_t*)c.selection;
        sc.values = (uint8_t*)c.values;
        sc.validity = c.is_nullable ? (uint32_t*)c.validity : nullptr;
        sc.rows = rows[i];
        sc.cap_rows = c.values ? c.values_capacity / sc.w : 0;
        sc.cap_words = sc.validity ? c.validity_capacity / 4 : 0;
        cap[i] = rows[i] * sc.w;   // (the share of the staging area a filter comparison column has)
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->in_replay && ctx->filter_freq) {
        rc = rsel_columns_decoded(ctx, std::move(rc_cols), rows.data(), hs, users.data());
    } else {
        if ((rc = stage_shares(ctx, rc_cols.data(), cap.data(), n)) != SB_OK) return rc;
        ReadMode mode{ReadMode::SELECTED};
        mode.selc = hs.data();
        mode.users = users.data();
        mode.pending_kind = Pending::RSEL_COL;
        rc = read_columns_impl(ctx, rc_cols.data(), n, SB_MEM_DEVICE, mode);
    }
    if (rc == SB_OK && !ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::READ_SEL, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ selected read, binary columns
// The binary columns of a selected read are what the binary columns of a filter call are up to k_plan: a share of the
// staging area for the inflated value blocks, Freq pages as virtual Dict pages.  So the call never asks for the Freq
// replay, and in an interval that is replayed for someone else's primitive Freq page (ctx->filter_freq) it takes this
// same path, as filter_impl does for its binary columns.
int32_t sb_read_selected_var(sb_ctx* ctx, sb_column_read_selected_var* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_read_selected_var", &rc)) return rc;
    std::vector<uint64_t> rows(n);
    SelSpans sp;
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_read_selected_var& c = cols[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
        if (!is_binary_t(c.physical_type))
            return refuse(ctx, SB_ERR_NYI, "sb_read_selected_var is implemented for Binary and LargeBinary: numbers go through sb_read_selected");
        if (const char* msg = sel_check_column(c, sp, &rows[i])) return refuse(ctx, SB_ERR_INVALID, msg);
        const uint32_t osize = type_width(c.physical_type);
        // (offsets[0] is written by every accepted call, so a buffer without room for it counts as missing)
        if (!c.offsets || ((uintptr_t)c.offsets & (osize - 1)) || c.offsets_capacity < osize)
            return refuse(ctx, SB_ERR_INVALID, "offsets missing, not aligned to its entries or smaller than one entry");
        sp.outs.push_back({(const uint8_t*)c.offsets, c.offsets_capacity});
    }
    if (const char* msg = sel_check_overlaps(sp)) return refuse(ctx, SB_ERR_INVALID, msg);
    std::vector<SelCol> hs(n);
    std::vector<SelBin> hb(n);
    std::vector<sb_column_read> rc_cols(n);
    std::vector<void*> users(n);
    std::vector<uint64_t> cap(n);
    for (uint64_t i = 0; i < n; i++) {
        sb_column_read_selected_var& c = cols[i];
        c.rows = rows[i];
        c.selected = 0;
        c.values_len = 0;
        users[i] = &c;
        rc_cols[i] = read_col_of(c);
        SelCol& sc = hs[i];
        memset(&sc, 0, sizeof sc);
        sc.w = type_width(c.physical_type);
        sc.sel = (const uint32_t*)c.selection;
        sc.values = c.values;
        sc.validity = c.is_nullable ? (uint32_t*)c.validity : nullptr;
        sc.rows = rows[i];
        sc.cap_rows = c.offsets_capacity / sc.w - 1;
        sc.cap_words = sc.validity ? c.validity_capacity / 4 : 0;
        SelBin& bc = hb[i];
        memset(&bc, 0, sizeof bc);
        bc.offsets = (uint8_t*)c.offsets;
        bc.values_cap = c.values ? c.values_capacity : 0;
        bc.osize = sc.w;
        // the share of the staging area a binary filter column has (the caller's field stays as given: a replay reads it again)
        cap[i] = c.stage_capacity ? c.stage_capacity : 4 * c.pages_len;
    }
    (void)hipSetDevice(ctx->device);
    if ((rc = stage_shares(ctx, rc_cols.data(), cap.data(), n)) != SB_OK) return rc;
    ReadMode mode{ReadMode::SELECTED_VAR};
    mode.selc = hs.data();
    mode.selb = hb.data();
    mode.users = users.data();
    mode.pending_kind = Pending::RSEL_VAR_COL;
    rc = read_columns_impl(ctx, rc_cols.data(), n, SB_MEM_DEVICE, mode);
    if (rc == SB_OK && !ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::READ_SEL_VAR, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ aggregate
extern "C++" {
// What both aggregate entry points check of a column, in two steps (sb_aggregate_grouped checks its group fields behind
// each), and the column's AggCol
template <class Col>
static int32_t agg_check_ops(sb_ctx* ctx, const Col& c) {
    if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
    if (c.ops & ~(SB_AGG_COUNT | SB_AGG_MIN | SB_AGG_MAX | SB_AGG_SUM)) return refuse(ctx, SB_ERR_INVALID, "unknown ops bits");
    if (c.reserved) return refuse(ctx, SB_ERR_INVALID, "reserved is not 0");
    return SB_OK;
}
template <class Col>
static int32_t agg_check_fill(sb_ctx* ctx, const Col& c, uint32_t ops, AggCol& g,   // (ops: the column's, or a top-k column's SB_AGG_MIN)
                              const char* nyi = "min / max / sum are implemented for 8- to 64-bit integers and floats") {
    if ((ops & AGG_VALUE_OPS) && !filter_comparable(c.physical_type)) return refuse(ctx, SB_ERR_NYI, nyi);
    uint64_t rows = 0;
    if (!column_rows(c, &rows)) return refuse(ctx, SB_ERR_INVALID, "metas is null");
    if (c.selection && (((uintptr_t)c.selection & 3) || c.selection_capacity < (rows + 31) / 32 * 4))
        return refuse(ctx, SB_ERR_INVALID, "selection not 4-byte aligned or smaller than 4*ceil(rows/32) bytes");
    memset(&g, 0, sizeof g);
    g.sel = (const uint32_t*)c.selection;
    g.rows = rows;
    g.ops = ops;
    g.ptype = c.physical_type;
    g.w = type_width(c.physical_type);
    g.kind = value_kind(c.physical_type);
    return SB_OK;
}
}   // extern "C++"

// the share of the staging area a filter comparison column has; none for a column without a value op
static std::vector<uint64_t> agg_stage_caps(const std::vector<AggCol>& hs) {
    std::vector<uint64_t> cap(hs.size());
    for (size_t i = 0; i < hs.size(); i++) cap[i] = (hs[i].ops & AGG_VALUE_OPS) ? hs[i].rows * hs[i].w : NO_SHARE;
    return cap;
}

// The columns with a value op of a replayed call: decoded, and reduced from the staging area by k_agg_plain with the same
// sink: a slot per TILE_ROWS rows.
static int32_t agg_columns_decoded(sb_ctx* ctx, std::vector<sb_column_read>&& pages, std::vector<AggCol>& hs, void* const* users) {
    const uint64_t n = pages.size();
    ReplayCols rp;
    int32_t rc = open_replay(ctx, std::move(pages), hs, "aggregate", rp);
    if (rc != SB_OK) return rc;
    // [AggCol per column][the result records][the partial records: a slot per TILE_ROWS rows]
    const size_t res_stride = AGG_RESULT_WORDS * sizeof(uint64_t);
    ReplayArena a;
    const size_t o_ac = a.add(hs.data(), n * sizeof(AggCol));
    const size_t o_res = a.add(n * res_stride);
    const size_t o_parts = a.add((size_t)rp.slots * sizeof(AggPart));
    if ((rc = a.commit(ctx, "aggregate replay")) != SB_OK) return rc;
    StageSlot* slot = acquire_slot(ctx, n * res_stride);
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    uint64_t* d_res = a.at<uint64_t>(o_res);
    launch_agg_plain(ctx, a.at<const AggCol>(o_ac), (uint32_t)n, a.at<AggPart>(o_parts), rp.rows.data(), rp.vals.data(), rp.bits.data());
    launch_agg_finish(ctx, a.at<const AggCol>(o_ac), a.at<const AggPart>(o_parts), d_res, (uint32_t)n);
    return queue_sink_results(ctx, slot, d_res, res_stride, n, Pending::AGG_COL, users, nullptr, "aggregate");
}

int32_t sb_aggregate_columns(sb_ctx* ctx, sb_column_aggregate* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_aggregate_columns", &rc)) return rc;
    std::vector<AggCol> hs(n);
    for (uint64_t i = 0; i < n; i++)
        if ((rc = agg_check_ops(ctx, cols[i])) != SB_OK || (rc = agg_check_fill(ctx, cols[i], cols[i].ops, hs[i])) != SB_OK) return rc;
    (void)hipSetDevice(ctx->device);
    std::vector<sb_column_read> rc_cols;
    std::vector<void*> users;
    read_cols_of(cols, n, rc_cols, users);
    if (ctx->in_replay && ctx->filter_freq) {
        // The columns that met a Freq page in the first pass (and so asked for this replay, or would have) through a full
        // decode; the others as ever, on the page route, whose slots -- and float bits -- are those of an interval that is
        // not replayed (aggregate_grouped_impl has the same rule).
        const std::vector<const void*>& freq_users = ctx->agg_freq_users;
        std::vector<bool> dec(n);
        for (uint64_t i = 0; i < n; i++)
            dec[i] = (hs[i].ops & AGG_VALUE_OPS) != 0 &&
                     std::find(freq_users.begin(), freq_users.end(), (const void*)users[i]) != freq_users.end();
        std::vector<sb_column_read> r_val = take_if(rc_cols, dec);
        std::vector<AggCol> g_val = take_if(hs, dec);
        const std::vector<void*> u_val = take_if(users, dec);
        if (!r_val.empty()) rc = agg_columns_decoded(ctx, std::move(r_val), g_val, u_val.data());
    }
    if (rc == SB_OK && !rc_cols.empty()) {
        if ((rc = stage_shares(ctx, rc_cols.data(), agg_stage_caps(hs).data(), rc_cols.size())) != SB_OK) return rc;
        ReadMode mode{ReadMode::AGGREGATE};
        mode.aggc = hs.data();
        mode.users = users.data();
        mode.pending_kind = Pending::AGG_COL;
        rc = read_columns_impl(ctx, rc_cols.data(), rc_cols.size(), SB_MEM_DEVICE, mode);
    }
    if (rc != SB_OK) return rc;
    for (uint64_t i = 0; i < n; i++) {   // (after the last thing that can refuse the call: a page outside pages_len)
        sb_column_aggregate& c = cols[i];
        column_rows(c, &c.rows);
        c.selected = c.count = c.nans = c.sum_lo = c.sum_hi = 0;
        memset(c.min, 0, sizeof c.min);
        memset(c.max, 0, sizeof c.max);
    }
    if (!ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::AGGREGATE, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ aggregate, grouped
// The sibling of agg_columns_decoded: reduced from the staging area by k_grp_plain into a slot per TILE_ROWS rows, combined
// by k_grp_finish.  large (sb_aggregate_grouped_large): by k_grpl_plain into a slot per GRPL_CHUNK_TILES * TILE_ROWS rows,
// combined by k_grpl_finish.
static int32_t grp_columns_decoded(sb_ctx* ctx, std::vector<sb_column_read>&& pages, std::vector<AggCol>& hs, const std::vector<GrpCol>& hg,
                                   void* const* users, bool large) {
    const uint64_t n = pages.size();
    ReplayCols rp;
    int32_t rc = open_replay(ctx, std::move(pages), hs, "grouped aggregate", rp);
    if (rc != SB_OK) return rc;
    uint32_t gmax = 1;
    for (const GrpCol& g : hg) gmax = std::max(gmax, g.n_groups);
    const uint64_t slots = large ? chunk_slots(hs) : rp.slots;
    // [AggCol per column][GrpCol per column][the results][the slots' flags, the columns' counters and Freq marks][the slots' records]
    const size_t res_stride = grp_result_words(gmax) * sizeof(uint64_t);
    ReplayArena a;
    const size_t o_ac = a.add(hs.data(), n * sizeof(AggCol));
    const size_t o_gc = a.add(hg.data(), n * sizeof(GrpCol));
    const size_t o_res = a.add(n * res_stride);
    const size_t o_flags = a.add((size_t)(slots + 2 * n) * sizeof(uint64_t));
    const size_t o_recs = a.add((size_t)slots * gmax * sizeof(GrpPart));
    if ((rc = a.commit(ctx, "grouped aggregate replay")) != SB_OK) return rc;
    StageSlot* slot = acquire_slot(ctx, n * res_stride);
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    uint64_t* d_res = a.at<uint64_t>(o_res);
    GrpLaunch gl{a.at<const AggCol>(o_ac), a.at<const GrpCol>(o_gc), a.at<uint64_t>(o_flags), a.at<GrpPart>(o_recs), slots, 0, gmax, true, false, (uint32_t)n, true};
    if (large) {
        launch_grpl_zero(ctx, gl, (uint32_t)n);
        launch_grpl_plain(ctx, gl, (uint32_t)n, rp.rows.data(), rp.vals.data(), rp.bits.data());
        launch_grpl_finish(ctx, gl, d_res, (uint32_t)n);
    } else {
        launch_grp_zero(ctx, gl, (uint32_t)n);
        launch_grp_plain(ctx, gl, (uint32_t)n, rp.rows.data(), rp.vals.data(), rp.bits.data());
        launch_grp_finish(ctx, gl, d_res, (uint32_t)n);
    }
    return queue_sink_results(ctx, slot, d_res, res_stride, n, large ? Pending::AGG_GRPL_COL : Pending::AGG_GRP_COL, users, hg.data(), "grouped aggregate");
}

// sb_aggregate_grouped and, with `large`, sb_aggregate_grouped_large: the same checks with the call's own limit, the same
// Freq rule with the call's own marks, the kernels of sb_aggregate_grouped.h or of sb_aggregate_grouped_large.h
static int32_t aggregate_grouped_impl(sb_ctx* ctx, sb_column_aggregate_grouped* cols, uint64_t n, int32_t mem, bool large) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, large ? "sb_aggregate_grouped_large" : "sb_aggregate_grouped", &rc)) return rc;
    const std::vector<const void*>& freq_users = large ? ctx->grpl_freq_users : ctx->grp_freq_users;
    std::vector<AggCol> hs(n);
    std::vector<GrpCol> hg(n);
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_aggregate_grouped& c = cols[i];
        if ((rc = agg_check_ops(ctx, c)) != SB_OK) return rc;
        if (!large && (c.n_groups == 0 || c.n_groups > SB_AGG_MAX_GROUPS)) return refuse(ctx, SB_ERR_INVALID, "n_groups is not in 1 .. SB_AGG_MAX_GROUPS");
        if (large && (c.n_groups == 0 || c.n_groups > SB_AGG_LARGE_MAX_GROUPS))
            return refuse(ctx, SB_ERR_INVALID, "n_groups is not in 1 .. SB_AGG_LARGE_MAX_GROUPS");
        if (c.group_id_width != 1 && c.group_id_width != 2 && c.group_id_width != 4) return refuse(ctx, SB_ERR_INVALID, "group_id_width is not 1, 2 or 4");
        if (!c.groups) return refuse(ctx, SB_ERR_INVALID, "groups is null");
        if ((rc = agg_check_fill(ctx, c, c.ops, hs[i])) != SB_OK) return rc;
        const uint64_t rows = hs[i].rows;
        if (rows && !c.group_ids) return refuse(ctx, SB_ERR_INVALID, "group_ids is null");
        if (c.group_ids && (((uintptr_t)c.group_ids & (c.group_id_width - 1)) || c.group_ids_capacity < rows * c.group_id_width))
            return refuse(ctx, SB_ERR_INVALID, "group_ids not aligned to group_id_width or smaller than rows * group_id_width bytes");
        hg[i] = GrpCol{(const uint8_t*)c.group_ids, c.group_id_width, c.n_groups};
    }
    (void)hipSetDevice(ctx->device);
    std::vector<sb_column_read> rc_cols;
    std::vector<void*> users;
    read_cols_of(cols, n, rc_cols, users);
    if (ctx->in_replay && ctx->filter_freq) {
        // The columns that met a Freq page in the first pass (and so asked for this replay, or would have) through a full
        // decode; the others as ever, on the page route, whose slots -- and float bits -- are those of an interval that is
        // not replayed.
        std::vector<bool> dec(n);
        for (uint64_t i = 0; i < n; i++)
            dec[i] = (hs[i].ops & AGG_VALUE_OPS) != 0 &&
                     std::find(freq_users.begin(), freq_users.end(), (const void*)users[i]) != freq_users.end();
        std::vector<sb_column_read> r_val = take_if(rc_cols, dec);
        std::vector<AggCol> g_val = take_if(hs, dec);
        const std::vector<GrpCol> c_val = take_if(hg, dec);
        const std::vector<void*> u_val = take_if(users, dec);
        if (!r_val.empty()) rc = grp_columns_decoded(ctx, std::move(r_val), g_val, c_val, u_val.data(), large);
    }
    if (rc == SB_OK && !rc_cols.empty()) {
        if ((rc = stage_shares(ctx, rc_cols.data(), agg_stage_caps(hs).data(), rc_cols.size())) != SB_OK) return rc;
        ReadMode mode{large ? ReadMode::AGG_GROUPED_LARGE : ReadMode::AGG_GROUPED};
        for (const GrpCol& g : hg) mode.grp_gmax = std::max(mode.grp_gmax, g.n_groups);
        mode.aggc = hs.data();
        mode.grpc = hg.data();
        mode.users = users.data();
        mode.pending_kind = large ? Pending::AGG_GRPL_COL : Pending::AGG_GRP_COL;
        rc = read_columns_impl(ctx, rc_cols.data(), rc_cols.size(), SB_MEM_DEVICE, mode);
    }
    if (rc != SB_OK) return rc;
    for (uint64_t i = 0; i < n; i++) {   // (after the last thing that can refuse the call: a page outside pages_len)
        sb_column_aggregate_grouped& c = cols[i];
        column_rows(c, &c.rows);
        c.selected = c.out_of_range = 0;
    }
    if (!ctx->in_replay)
        ctx->iv.calls.push_back(sb_ctx::Call{large ? sb_ctx::Call::AGG_GROUPED_LARGE : sb_ctx::Call::AGG_GROUPED, cols, n, sb_write_options{}, mem});
    return rc;
}

int32_t sb_aggregate_grouped(sb_ctx* ctx, sb_column_aggregate_grouped* cols, uint64_t n, int32_t mem) {
    return aggregate_grouped_impl(ctx, cols, n, mem, false);
}
int32_t sb_aggregate_grouped_large(sb_ctx* ctx, sb_column_aggregate_grouped* cols, uint64_t n, int32_t mem) {
    return aggregate_grouped_impl(ctx, cols, n, mem, true);
}

// ------------------------------------------------------------------------------------ aggregate, weighted
static_assert(sizeof(sb_column_aggregate_weighted) == 168 && offsetof(sb_column_aggregate_weighted, ops) == offsetof(sb_column_aggregate_grouped, ops) &&
                  offsetof(sb_column_aggregate_weighted, group_ids) == offsetof(sb_column_aggregate_grouped, group_ids) &&
                  has_pages_prefix<sb_column_aggregate_weighted>(),
              "sb_column_aggregate_weighted begins with the first 92 bytes of sb_column_aggregate_grouped");

// The sibling of grp_columns_decoded: reduced from the staging area by k_wgt_plain into a slot per GRPL_CHUNK_TILES *
// TILE_ROWS rows, combined by k_wgt_finish.
static int32_t wgt_columns_decoded(sb_ctx* ctx, std::vector<sb_column_read>&& pages, std::vector<AggCol>& hs, const std::vector<GrpCol>& hg,
                                   const std::vector<WgtCol>& hw, void* const* users) {
    const uint64_t n = pages.size();
    ReplayCols rp;
    int32_t rc = open_replay(ctx, std::move(pages), hs, "weighted aggregate", rp);
    if (rc != SB_OK) return rc;
    uint32_t gmax = 1;
    for (const GrpCol& g : hg) gmax = std::max(gmax, g.n_groups);
    const uint64_t slots = chunk_slots(hs);
    // [AggCol per column][GrpCol per column][WgtCol per column][the results][the slots' flags, the columns' counters and Freq marks][the slots' records]
    const size_t res_stride = grp_result_words(gmax) * sizeof(uint64_t);
    ReplayArena a;
    const size_t o_ac = a.add(hs.data(), n * sizeof(AggCol));
    const size_t o_gc = a.add(hg.data(), n * sizeof(GrpCol));
    const size_t o_wc = a.add(hw.data(), n * sizeof(WgtCol));
    const size_t o_res = a.add(n * res_stride);
    const size_t o_flags = a.add((size_t)(slots + 2 * n) * sizeof(uint64_t));
    const size_t o_recs = a.add((size_t)slots * gmax * sizeof(GrpPart));
    if ((rc = a.commit(ctx, "weighted aggregate replay")) != SB_OK) return rc;
    StageSlot* slot = acquire_slot(ctx, n * res_stride);
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    uint64_t* d_res = a.at<uint64_t>(o_res);
    const WgtLaunch wl{GrpLaunch{a.at<const AggCol>(o_ac), a.at<const GrpCol>(o_gc), a.at<uint64_t>(o_flags), a.at<GrpPart>(o_recs), slots, 0, gmax, true, false,
                                 (uint32_t)n, true},
                       a.at<const WgtCol>(o_wc)};
    launch_wgt_zero(ctx, wl, (uint32_t)n);
    launch_wgt_plain(ctx, wl, (uint32_t)n, rp.rows.data(), rp.vals.data(), rp.bits.data());
    launch_wgt_finish(ctx, wl, d_res, (uint32_t)n);
    return queue_sink_results(ctx, slot, d_res, res_stride, n, Pending::AGG_WGT_COL, users, hg.data(), "weighted aggregate");
}

int32_t sb_aggregate_weighted(sb_ctx* ctx, sb_column_aggregate_weighted* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_aggregate_weighted", &rc)) return rc;
    std::vector<AggCol> hs(n);
    std::vector<GrpCol> hg(n);
    std::vector<WgtCol> hw(n);
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_aggregate_weighted& c = cols[i];
        if ((rc = agg_check_ops(ctx, c)) != SB_OK) return rc;
        if (c.ops & (SB_AGG_MIN | SB_AGG_MAX)) return refuse(ctx, SB_ERR_INVALID, "min / max of a product are not offered: ops is SB_AGG_COUNT | SB_AGG_SUM");
        if (c.flags & ~SB_WGT_SQUARE) return refuse(ctx, SB_ERR_INVALID, "unknown flags bits");
        if (c.n_groups == 0 || c.n_groups > SB_AGG_LARGE_MAX_GROUPS) return refuse(ctx, SB_ERR_INVALID, "n_groups is not in 1 .. SB_AGG_LARGE_MAX_GROUPS");
        if (!c.group_ids) {   // the ungrouped form
            if (c.n_groups != 1 || c.group_id_width != 0 || c.group_ids_capacity != 0)
                return refuse(ctx, SB_ERR_INVALID, "group_ids is null: n_groups must be 1, group_id_width and group_ids_capacity 0");
        } else if (c.group_id_width != 1 && c.group_id_width != 2 && c.group_id_width != 4) {
            return refuse(ctx, SB_ERR_INVALID, "group_id_width is not 1, 2 or 4");
        }
        if (!c.groups) return refuse(ctx, SB_ERR_INVALID, "groups is null");
        const bool square = (c.flags & SB_WGT_SQUARE) != 0;
        if (square && (c.weights || c.weights_capacity || c.weights_validity || c.weights_validity_capacity || c.weight_type != 0))
            return refuse(ctx, SB_ERR_INVALID, "SB_WGT_SQUARE: weights, weights_validity and their capacities must be null / 0 and weight_type 0");
        if (!square && !filter_comparable(c.weight_type)) return refuse(ctx, SB_ERR_INVALID, "weight_type is not an 8- to 64-bit integer or a float");
        if ((rc = agg_check_fill(ctx, c, c.ops, hs[i], "sum(y * w) is implemented for 8- to 64-bit integers and floats")) != SB_OK) return rc;
        const uint64_t rows = hs[i].rows;
        if (c.group_ids && (((uintptr_t)c.group_ids & (c.group_id_width - 1)) || c.group_ids_capacity < rows * c.group_id_width))
            return refuse(ctx, SB_ERR_INVALID, "group_ids not aligned to group_id_width or smaller than rows * group_id_width bytes");
        const uint32_t ww = square ? hs[i].w : type_width(c.weight_type);
        if (!square) {
            if (!c.weights) return refuse(ctx, SB_ERR_INVALID, "weights is null");
            if (((uintptr_t)c.weights & (ww - 1)) || c.weights_capacity < rows * ww)
                return refuse(ctx, SB_ERR_INVALID, "weights not aligned to the width of weight_type or smaller than rows * width bytes");
            if (c.weights_validity && (((uintptr_t)c.weights_validity & 3) || c.weights_validity_capacity < (rows + 31) / 32 * 4))
                return refuse(ctx, SB_ERR_INVALID, "weights_validity not 4-byte aligned or smaller than 4*ceil(rows/32) bytes");
        }
        hg[i] = GrpCol{(const uint8_t*)c.group_ids, c.group_id_width, c.n_groups};
        const uint32_t wkind = square ? hs[i].kind : value_kind(c.weight_type);
        const bool flt = hs[i].kind == FK_F32 || hs[i].kind == FK_F64 || wkind == FK_F32 || wkind == FK_F64;
        hw[i] = WgtCol{square ? nullptr : (const uint8_t*)c.weights, square ? nullptr : c.weights_validity, wkind, ww, flt ? 1u : 0u, 0u};
    }
    (void)hipSetDevice(ctx->device);
    std::vector<sb_column_read> rc_cols;
    std::vector<void*> users;
    read_cols_of(cols, n, rc_cols, users);
    if (ctx->in_replay && ctx->filter_freq) {
        // the columns that met a Freq page in the first pass through a full decode, the others on the page route
        // (aggregate_grouped_impl has the same rule); the marks are this call's own
        const std::vector<const void*>& freq_users = ctx->wgt_freq_users;
        std::vector<bool> dec(n);
        for (uint64_t i = 0; i < n; i++)
            dec[i] = (hs[i].ops & AGG_VALUE_OPS) != 0 &&
                     std::find(freq_users.begin(), freq_users.end(), (const void*)users[i]) != freq_users.end();
        std::vector<sb_column_read> r_val = take_if(rc_cols, dec);
        std::vector<AggCol> g_val = take_if(hs, dec);
        const std::vector<GrpCol> c_val = take_if(hg, dec);
        const std::vector<WgtCol> w_val = take_if(hw, dec);
        const std::vector<void*> u_val = take_if(users, dec);
        if (!r_val.empty()) rc = wgt_columns_decoded(ctx, std::move(r_val), g_val, c_val, w_val, u_val.data());
    }
    if (rc == SB_OK && !rc_cols.empty()) {
        if ((rc = stage_shares(ctx, rc_cols.data(), agg_stage_caps(hs).data(), rc_cols.size())) != SB_OK) return rc;
        ReadMode mode{ReadMode::AGG_WEIGHTED};
        for (const GrpCol& g : hg) mode.grp_gmax = std::max(mode.grp_gmax, g.n_groups);
        mode.aggc = hs.data();
        mode.grpc = hg.data();
        mode.wgtc = hw.data();
        mode.users = users.data();
        mode.pending_kind = Pending::AGG_WGT_COL;
        rc = read_columns_impl(ctx, rc_cols.data(), rc_cols.size(), SB_MEM_DEVICE, mode);
    }
    if (rc != SB_OK) return rc;
    for (uint64_t i = 0; i < n; i++) {   // (after the last thing that can refuse the call: a page outside pages_len)
        sb_column_aggregate_weighted& c = cols[i];
        column_rows(c, &c.rows);
        c.selected = c.out_of_range = 0;
    }
    if (!ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::AGG_WEIGHTED, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ top-k
// The sibling of agg_columns_decoded: ordered from the staging area by k_topk_plain into a slot per TILE_ROWS rows, combined
// by k_topk_finish.
static int32_t topk_columns_decoded(sb_ctx* ctx, std::vector<sb_column_read>&& pages, std::vector<AggCol>& hs, const std::vector<TopkCol>& ht,
                                    void* const* users) {
    const uint64_t n = pages.size();
    ReplayCols rp;
    int32_t rc = open_replay(ctx, std::move(pages), hs, "top-k", rp);
    if (rc != SB_OK) return rc;
    uint32_t kmax = 1;
    for (const TopkCol& t : ht) kmax = std::max(kmax, t.k);
    // [AggCol per column][TopkCol per column][the results][the slots' headers][the slots' records]
    const size_t res_stride = topk_result_words(kmax) * sizeof(uint64_t);
    ReplayArena a;
    const size_t o_ac = a.add(hs.data(), n * sizeof(AggCol));
    const size_t o_tc = a.add(ht.data(), n * sizeof(TopkCol));
    const size_t o_res = a.add(n * res_stride);
    const size_t o_heads = a.add((size_t)rp.slots * sizeof(TopkHead));
    const size_t o_recs = a.add((size_t)rp.slots * kmax * sizeof(TopkRec));
    if ((rc = a.commit(ctx, "top-k replay")) != SB_OK) return rc;
    StageSlot* slot = acquire_slot(ctx, n * res_stride);
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    uint64_t* d_res = a.at<uint64_t>(o_res);
    TopkLaunch tl{a.at<const AggCol>(o_ac), a.at<const TopkCol>(o_tc), a.at<TopkHead>(o_heads), a.at<TopkRec>(o_recs), rp.slots, 0, kmax};
    launch_topk_zero(ctx, tl);
    launch_topk_plain(ctx, tl, (uint32_t)n, rp.rows.data(), rp.vals.data(), rp.bits.data());
    launch_topk_finish(ctx, tl, d_res, (uint32_t)n);
    return queue_sink_results(ctx, slot, d_res, res_stride, n, Pending::TOPK_COL, users, nullptr, "top-k");
}

int32_t sb_topk_columns(sb_ctx* ctx, sb_column_topk* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_topk_columns", &rc)) return rc;
    std::vector<AggCol> hs(n);
    std::vector<TopkCol> ht(n);
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_topk& c = cols[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
        if (c.k == 0 || c.k > SB_TOPK_MAX_K) return refuse(ctx, SB_ERR_INVALID, "k is not in 1 .. SB_TOPK_MAX_K");
        if (c.order != SB_TOPK_SMALLEST && c.order != SB_TOPK_LARGEST) return refuse(ctx, SB_ERR_INVALID, "unknown order");
        if (c.reserved) return refuse(ctx, SB_ERR_INVALID, "reserved is not 0");
        if (!c.out) return refuse(ctx, SB_ERR_INVALID, "out is null");
        // (ordered like a minimum: every value is looked at)
        if ((rc = agg_check_fill(ctx, c, SB_AGG_MIN, hs[i], "top-k is implemented for 8- to 64-bit integers and floats")) != SB_OK) return rc;
        ht[i] = TopkCol{c.k, c.order == SB_TOPK_LARGEST ? 1u : 0u};
    }
    (void)hipSetDevice(ctx->device);
    std::vector<sb_column_read> rc_cols;
    std::vector<void*> users;
    read_cols_of(cols, n, rc_cols, users);
    if (ctx->in_replay && ctx->filter_freq) {
        // Every column through a full decode, as sb_aggregate_columns has it.  The result is one set in one sequence on
        // either route, so which interval a column is decoded in does not show in its bytes.
        rc = topk_columns_decoded(ctx, std::move(rc_cols), hs, ht, users.data());
    } else {
        if ((rc = stage_shares(ctx, rc_cols.data(), agg_stage_caps(hs).data(), n)) != SB_OK) return rc;
        ReadMode mode{ReadMode::TOPK};
        for (const TopkCol& t : ht) mode.topk_kmax = std::max(mode.topk_kmax, t.k);
        mode.aggc = hs.data();
        mode.topkc = ht.data();
        mode.users = users.data();
        mode.pending_kind = Pending::TOPK_COL;
        rc = read_columns_impl(ctx, rc_cols.data(), n, SB_MEM_DEVICE, mode);
    }
    if (rc != SB_OK) return rc;
    for (uint64_t i = 0; i < n; i++) {   // (after the last thing that can refuse the call: a page outside pages_len)
        sb_column_topk& c = cols[i];
        column_rows(c, &c.rows);
        c.selected = c.count = c.nans = c.found = 0;
    }
    if (!ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::TOPK, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ key ids
static KeyLaunch key_launch_at(uint8_t* acols, uint8_t* kcols, uint8_t* state, uint8_t* sorted, uint64_t n, uint64_t slots, uint32_t kmax) {
    return KeyLaunch{(const AggCol*)acols, (const KeyCol*)kcols, (KeyState*)state, (uint64_t*)(state + n * sizeof(KeyState)), (uint64_t*)sorted,
                     n * sizeof(KeyState) + slots * sizeof(uint64_t), kmax, (uint32_t)n};
}

// The sibling of topk_columns_decoded: the three phases from the staging area, k_key_collect_plain and k_key_assign_plain
// around the same k_key_finish.
static int32_t key_ids_decoded(sb_ctx* ctx, std::vector<sb_column_read>&& pages, std::vector<AggCol>& hs, const std::vector<KeyCol>& hk, uint64_t slots,
                               uint32_t kmax, void* const* users) {
    const uint64_t n = pages.size();
    ReplayCols rp;
    int32_t rc = open_replay(ctx, std::move(pages), hs, "key ids", rp);
    if (rc != SB_OK) return rc;
    // [AggCol per column][KeyCol per column][the results][the columns' states, their tables][the sorted keys]
    const size_t res_stride = key_result_words(kmax) * sizeof(uint64_t);
    ReplayArena a;
    const size_t o_ac = a.add(hs.data(), n * sizeof(AggCol));
    const size_t o_kc = a.add(hk.data(), n * sizeof(KeyCol));
    const size_t o_res = a.add(n * res_stride);
    const size_t o_state = a.add(n * sizeof(KeyState) + (size_t)slots * sizeof(uint64_t));
    const size_t o_sorted = a.add(n * KEY_MAX_KEYS * sizeof(uint64_t));
    if ((rc = a.commit(ctx, "key ids replay")) != SB_OK) return rc;
    StageSlot* slot = acquire_slot(ctx, n * res_stride);
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    uint64_t* d_res = a.at<uint64_t>(o_res);
    const KeyLaunch kl = key_launch_at(a.at<uint8_t>(o_ac), a.at<uint8_t>(o_kc), a.at<uint8_t>(o_state), a.at<uint8_t>(o_sorted), n, slots, kmax);
    launch_key_zero(ctx, kl);
    launch_key_collect_plain(ctx, kl, rp.rows.data(), rp.vals.data(), rp.bits.data());
    launch_key_finish(ctx, kl, d_res);
    launch_key_assign_plain(ctx, kl, rp.rows.data(), rp.vals.data(), rp.bits.data());
    return queue_sink_results(ctx, slot, d_res, res_stride, n, Pending::KEY_COL, users, nullptr, "key ids");
}

int32_t sb_key_ids(sb_ctx* ctx, sb_column_key_ids* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_key_ids", &rc)) return rc;
    std::vector<AggCol> hs(n);
    std::vector<KeyCol> hk(n);
    uint64_t slots = 0;
    uint32_t kmax = 0;
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_key_ids& c = cols[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
        if (c.physical_type < SB_TYPE_INT8 || c.physical_type > SB_TYPE_UINT64)
            return refuse(ctx, SB_ERR_NYI, "key ids are implemented for 8- to 64-bit integers");
        if (const char* why = ids_check_width(c)) return refuse(ctx, SB_ERR_INVALID, why);
        const uint64_t limit = std::min<uint64_t>(SB_KEY_MAX_KEYS, (1ull << (8 * c.id_width)) - 1);
        if (c.max_keys == 0 || c.max_keys > limit) return refuse(ctx, SB_ERR_INVALID, "max_keys is not in 1 .. min(SB_KEY_MAX_KEYS, 2^(8 * id_width) - 1)");
        if (c.reserved) return refuse(ctx, SB_ERR_INVALID, "reserved is not 0");
        if (!c.keys) return refuse(ctx, SB_ERR_INVALID, "keys is null");
        // (collected like a minimum: every live value is looked at)
        if ((rc = agg_check_fill(ctx, c, SB_AGG_MIN, hs[i], "key ids are implemented for 8- to 64-bit integers")) != SB_OK) return rc;
        if (const char* why = ids_check_buffer(c, hs[i].rows)) return refuse(ctx, SB_ERR_INVALID, why);
        hk[i] = KeyCol{(uint8_t*)c.ids, slots, key_table_slots(c.max_keys) - 1, c.max_keys, c.id_width, 0};
        slots += key_table_slots(c.max_keys);
        kmax = std::max(kmax, c.max_keys);
    }
    if (const char* why = ids_check_overlaps(cols, hs)) return refuse(ctx, SB_ERR_INVALID, why);
    (void)hipSetDevice(ctx->device);
    std::vector<sb_column_read> rc_cols;
    std::vector<void*> users;
    read_cols_of(cols, n, rc_cols, users);
    if (ctx->in_replay && ctx->filter_freq) {
        // Every column through a full decode, as sb_aggregate_columns has it.  Keys and ids are functions of the data alone,
        // so which interval a column is decoded in does not show in its bytes.
        rc = key_ids_decoded(ctx, std::move(rc_cols), hs, hk, slots, kmax, users.data());
    } else {
        if ((rc = stage_shares(ctx, rc_cols.data(), agg_stage_caps(hs).data(), n)) != SB_OK) return rc;
        ReadMode mode{ReadMode::KEY_IDS};
        mode.aggc = hs.data();
        mode.keyc = hk.data();
        mode.key_kmax = kmax;
        mode.key_slots = slots;
        mode.users = users.data();
        mode.pending_kind = Pending::KEY_COL;
        rc = read_columns_impl(ctx, rc_cols.data(), n, SB_MEM_DEVICE, mode);
    }
    if (rc != SB_OK) return rc;
    for (uint64_t i = 0; i < n; i++) {   // (after the last thing that can refuse the call: a page outside pages_len)
        sb_column_key_ids& c = cols[i];
        column_rows(c, &c.rows);
        c.selected = c.count = c.n_keys = c.overflow = 0;
    }
    if (!ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::KEY_IDS, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ key ids of binary columns
static_assert(sizeof(sb_column_key_ids_var) == 176 && offsetof(sb_column_key_ids_var, selection) == 48 && offsetof(sb_column_key_ids_var, ids) == 64 &&
                  offsetof(sb_column_key_ids_var, id_width) == 80 && offsetof(sb_column_key_ids_var, max_keys) == 84 &&
                  offsetof(sb_column_key_ids_var, key_offsets) == 88 && offsetof(sb_column_key_ids_var, keys) == 96 &&
                  offsetof(sb_column_key_ids_var, keys_capacity) == 104 && offsetof(sb_column_key_ids_var, stage_capacity) == 112 &&
                  offsetof(sb_column_key_ids_var, reserved) == 120 && offsetof(sb_column_key_ids_var, rows) == 128 &&
                  offsetof(sb_column_key_ids_var, keys_len) == 160 && offsetof(sb_column_key_ids_var, overflow) == 168,
              "the layout the header pins");
static_assert(SB_KEY_VAR_MAX_BYTES == KEYV_MAX_BYTES && KEYV_TAG_BITS + 2 + KEYV_INDEX_BITS + KEYV_PAGE_BITS == 64, "the header's limit; the slot's word");

// One route, also on a replay: a Freq page of strings is a virtual Dict page, so no column is decoded first.
int32_t sb_key_ids_var(sb_ctx* ctx, sb_column_key_ids_var* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_key_ids_var", &rc)) return rc;
    std::vector<AggCol> hs(n);
    std::vector<KeyVarCol> hk(n);
    std::vector<uint64_t> cap(n);
    uint64_t slots = 0, kbytes = 0, pages = 0;
    uint32_t kmax = 0;
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_key_ids_var& c = cols[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
        if (!is_binary_t(c.physical_type)) return refuse(ctx, SB_ERR_NYI, "sb_key_ids_var takes Binary / LargeBinary columns (integers: sb_key_ids)");
        if (const char* why = ids_check_width(c)) return refuse(ctx, SB_ERR_INVALID, why);
        const uint64_t limit = std::min<uint64_t>(SB_KEY_MAX_KEYS, (1ull << (8 * c.id_width)) - 1);
        if (c.max_keys == 0 || c.max_keys > limit) return refuse(ctx, SB_ERR_INVALID, "max_keys is not in 1 .. min(SB_KEY_MAX_KEYS, 2^(8 * id_width) - 1)");
        if (c.reserved) return refuse(ctx, SB_ERR_INVALID, "reserved is not 0");
        if (!c.key_offsets) return refuse(ctx, SB_ERR_INVALID, "key_offsets is null");
        if (c.keys_capacity > SB_KEY_VAR_MAX_BYTES) return refuse(ctx, SB_ERR_INVALID, "keys_capacity exceeds SB_KEY_VAR_MAX_BYTES");
        if (!c.keys && c.keys_capacity) return refuse(ctx, SB_ERR_INVALID, "keys is null");
        if ((rc = agg_check_fill(ctx, c, 0u, hs[i])) != SB_OK) return rc;
        if (const char* why = ids_check_buffer(c, hs[i].rows)) return refuse(ctx, SB_ERR_INVALID, why);
        // page and row / entry number are fields of the word a slot holds (kv_word, sb_common.h)
        for (uint64_t p = 0; p < c.n_pages; p++)
            if (c.metas[p].num_values > (1ull << KEYV_INDEX_BITS) || c.metas[p].length / 8 >= (1ull << KEYV_INDEX_BITS))
                return refuse(ctx, SB_ERR_NYI, "sb_key_ids_var: a page of more than 2^26 rows or of 2^29 bytes or more");
        pages += c.n_pages;
        hk[i] = KeyVarCol{(uint8_t*)c.ids, slots, key_table_slots(c.max_keys) - 1, c.max_keys, c.id_width, 0, c.keys_capacity};
        slots += key_table_slots(c.max_keys);
        kmax = std::max(kmax, c.max_keys);
        kbytes = std::max<uint64_t>(kbytes, c.keys_capacity);
        cap[i] = c.stage_capacity ? c.stage_capacity : 4 * c.pages_len;   // (the caller's field stays as given: a replay reads it again)
    }
    if (pages >= (1ull << KEYV_PAGE_BITS)) return refuse(ctx, SB_ERR_NYI, "sb_key_ids_var: 2^28 pages or more in one call");
    if (const char* why = ids_check_overlaps(cols, hs)) return refuse(ctx, SB_ERR_INVALID, why);
    (void)hipSetDevice(ctx->device);
    std::vector<sb_column_read> rc_cols;
    std::vector<void*> users;
    read_cols_of(cols, n, rc_cols, users);
    if ((rc = stage_shares(ctx, rc_cols.data(), cap.data(), n)) != SB_OK) return rc;
    ReadMode mode{ReadMode::KEY_IDS_VAR};
    mode.aggc = hs.data();
    mode.keyvc = hk.data();
    mode.key_kmax = kmax;
    mode.key_slots = slots;
    mode.key_kbytes = kbytes;
    mode.users = users.data();
    mode.pending_kind = Pending::KEY_VAR_COL;
    if ((rc = read_columns_impl(ctx, rc_cols.data(), n, SB_MEM_DEVICE, mode)) != SB_OK) return rc;
    for (uint64_t i = 0; i < n; i++) {   // (after the last thing that can refuse the call: a page outside pages_len)
        sb_column_key_ids_var& c = cols[i];
        column_rows(c, &c.rows);
        c.selected = c.count = c.n_keys = c.keys_len = c.overflow = 0;
    }
    if (!ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::KEY_IDS_VAR, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ ids of composite keys
static_assert(sizeof(sb_key_combine_item) == 168 && offsetof(sb_key_combine_item, n_parts) == 8 && offsetof(sb_key_combine_item, id_width) == 12 &&
                  offsetof(sb_key_combine_item, part_ids) == 16 && offsetof(sb_key_combine_item, part_capacity) == 48 &&
                  offsetof(sb_key_combine_item, part_width) == 80 && offsetof(sb_key_combine_item, part_keys) == 96 &&
                  offsetof(sb_key_combine_item, ids) == 112 && offsetof(sb_key_combine_item, ids_capacity) == 120 &&
                  offsetof(sb_key_combine_item, max_keys) == 128 && offsetof(sb_key_combine_item, reserved) == 132 &&
                  offsetof(sb_key_combine_item, tuples) == 136 && offsetof(sb_key_combine_item, live) == 144 &&
                  offsetof(sb_key_combine_item, n_keys) == 152 && offsetof(sb_key_combine_item, overflow) == 160,
              "the layout the header pins");
static_assert(SB_KEY_COMBINE_MAX_PARTS == COMB_MAX_PARTS, "the header's limit");

// No page is read, so no read_columns_impl: the call's workspace is carved out of a buffer of the context's that grows
// (ctx->combine), as read_columns_impl carves ctx->tables --
//   [AggCol per item][KeyCol per item][CombItem per item]   uploaded from the staging slot
//   [k_key_finish's records]                                read back into the slot, behind the upload
//   [KeyState per item, the items' tables]                  zeroed
//   [KEY_MAX_KEYS sorted codes per item]
// -- and everything travels on the context's stream, behind the calls that write the parts.
int32_t sb_key_combine(sb_ctx* ctx, sb_key_combine_item* items, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, items, n, mem, "sb_key_combine", &rc)) return rc;
    if (n > 65535) return refuse(ctx, SB_ERR_NYI, "sb_key_combine: more than 65535 items in one call");
    std::vector<AggCol> hs(n);
    std::vector<KeyCol> hk(n);
    std::vector<CombItem> hc(n);
    uint64_t slots = 0, max_rows = 0;
    uint32_t kmax = 0;
    for (uint64_t i = 0; i < n; i++) {
        const sb_key_combine_item& c = items[i];
        if (c.n_parts < 2 || c.n_parts > SB_KEY_COMBINE_MAX_PARTS) return refuse(ctx, SB_ERR_INVALID, "n_parts is not in 2 .. SB_KEY_COMBINE_MAX_PARTS");
        if (const char* why = ids_check_width(c)) return refuse(ctx, SB_ERR_INVALID, why);
        const uint64_t limit = std::min<uint64_t>(SB_KEY_MAX_KEYS, (1ull << (8 * c.id_width)) - 1);
        if (c.max_keys == 0 || c.max_keys > limit) return refuse(ctx, SB_ERR_INVALID, "max_keys is not in 1 .. min(SB_KEY_MAX_KEYS, 2^(8 * id_width) - 1)");
        if (c.reserved) return refuse(ctx, SB_ERR_INVALID, "reserved is not 0");
        if (!c.tuples) return refuse(ctx, SB_ERR_INVALID, "tuples is null");
        if (c.rows > (1ull << 60)) return refuse(ctx, SB_ERR_INVALID, "rows * width overflows");
        memset(&hc[i], 0, sizeof hc[i]);
        for (uint32_t p = 0; p < c.n_parts; p++) {
            const uint32_t w = c.part_width[p];
            if (w != 1 && w != 2 && w != 4) return refuse(ctx, SB_ERR_INVALID, "part_width is not 1, 2 or 4");
            if (c.part_keys[p] == 0 || c.part_keys[p] > SB_KEY_MAX_KEYS) return refuse(ctx, SB_ERR_INVALID, "part_keys is not in 1 .. SB_KEY_MAX_KEYS");
            if (c.rows && !c.part_ids[p]) return refuse(ctx, SB_ERR_INVALID, "a part's ids are null");
            if (c.part_ids[p] && (((uintptr_t)c.part_ids[p] & (w - 1)) || c.part_capacity[p] < c.rows * w))
                return refuse(ctx, SB_ERR_INVALID, "a part's ids are not aligned to part_width or smaller than rows * part_width bytes");
            hc[i].part[p] = (const uint8_t*)c.part_ids[p];
            hc[i].width[p] = w;
            hc[i].bound[p] = c.part_keys[p];
        }
        hc[i].n_parts = c.n_parts;
        if (const char* why = ids_check_buffer(c, c.rows)) return refuse(ctx, SB_ERR_INVALID, why);
        memset(&hs[i], 0, sizeof hs[i]);
        hs[i].rows = c.rows;
        hs[i].kind = FK_UNSIGNED;   // (the codes order and come back as they are)
        hs[i].ptype = SB_TYPE_UINT64;
        hs[i].w = 8;
        hk[i] = KeyCol{(uint8_t*)c.ids, slots, key_table_slots(c.max_keys) - 1, c.max_keys, c.id_width, 0};
        slots += key_table_slots(c.max_keys);
        kmax = std::max(kmax, c.max_keys);
        max_rows = std::max(max_rows, c.rows);
    }
    for (uint64_t i = 0; i < n; i++) {   // (the bytes an item writes: rows * id_width; the inputs must survive until a replay)
        const uintptr_t a0 = (uintptr_t)items[i].ids, a1 = a0 + items[i].rows * items[i].id_width;
        if (a0 == a1) continue;   // (no byte is written)
        for (uint64_t j = 0; j < n; j++) {
            if (items[j].rows == 0) continue;
            for (uint32_t p = 0; p < items[j].n_parts; p++) {
                const uintptr_t b0 = (uintptr_t)items[j].part_ids[p], b1 = b0 + items[j].rows * items[j].part_width[p];
                if (a0 < b1 && b0 < a1) return refuse(ctx, SB_ERR_INVALID, "ids overlaps a part of an item of the call");
            }
            if (j <= i) continue;
            const uintptr_t b0 = (uintptr_t)items[j].ids, b1 = b0 + items[j].rows * items[j].id_width;
            if (a0 < b1 && b0 < a1) return refuse(ctx, SB_ERR_INVALID, "ids of two items of one call overlap");
        }
    }
    (void)hipSetDevice(ctx->device);
    const size_t res_stride = key_result_words(kmax) * sizeof(uint64_t);
    size_t off = align_up(n * sizeof(AggCol), 64);
    const size_t o_kc = off;
    off = align_up(off + n * sizeof(KeyCol), 64);
    const size_t o_items = off;
    off = align_up(off + n * sizeof(CombItem), 64);
    const size_t upload = off, o_res = off;
    off = align_up(off + n * res_stride, 64);
    const size_t o_state = off;
    off = align_up(off + n * sizeof(KeyState) + (size_t)slots * sizeof(uint64_t), 64);
    const size_t o_sorted = off;
    off += n * KEY_MAX_KEYS * sizeof(uint64_t);
    if (!ensure(ctx, ctx->combine, off + 64)) return ctx->fail(SB_ERR_EXTERNAL, "hipMalloc(key combine workspace) failed");
    StageSlot* slot = acquire_slot(ctx, upload + n * res_stride);
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    memset(slot->host, 0, upload);
    memcpy(slot->host, hs.data(), n * sizeof(AggCol));
    memcpy(slot->host + o_kc, hk.data(), n * sizeof(KeyCol));
    memcpy(slot->host + o_items, hc.data(), n * sizeof(CombItem));
    uint8_t* dev = ctx->combine.p;
    hipError_t e = hipMemcpyAsync(dev, slot->host, upload, hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) return check_hip(ctx, e, "key combine upload");
    const CombLaunch cl{(const CombItem*)(dev + o_items), key_launch_at(dev, dev + o_kc, dev + o_state, dev + o_sorted, n, slots, kmax), max_rows};
    launch_key_combine(ctx, cl, (uint64_t*)(dev + o_res));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(slot->host + upload, dev + o_res, n * res_stride, hipMemcpyDeviceToHost, ctx->stream);
    if (e != hipSuccess) return check_hip(ctx, e, "key combine");
    (void)hipEventRecord(slot->done, ctx->stream);
    slot->in_flight = true;
    std::vector<void*> users(n);
    for (uint64_t i = 0; i < n; i++) {
        users[i] = &items[i];
        items[i].live = items[i].n_keys = items[i].overflow = 0;
    }
    push_pending(ctx, Pending::COMB_ITEM, users.data(), slot->host + upload, res_stride, n);
    if (!ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::KEY_COMBINE, items, n, sb_write_options{}, mem});
    return SB_OK;
}

// ------------------------------------------------------------------------------------ ids against a given list
static_assert(sizeof(sb_column_key_lookup) == 168 && offsetof(sb_column_key_lookup, selection) == 48 && offsetof(sb_column_key_lookup, ids) == 64 &&
                  offsetof(sb_column_key_lookup, id_width) == 80 && offsetof(sb_column_key_lookup, reserved0) == 84 &&
                  offsetof(sb_column_key_lookup, values) == 88 && offsetof(sb_column_key_lookup, value_offsets) == 96 &&
                  offsetof(sb_column_key_lookup, value_ids) == 104 && offsetof(sb_column_key_lookup, n_values) == 112 &&
                  offsetof(sb_column_key_lookup, stage_capacity) == 120 && offsetof(sb_column_key_lookup, reserved) == 128 &&
                  offsetof(sb_column_key_lookup, rows) == 136 && offsetof(sb_column_key_lookup, matched) == 160,
              "sb_column_key_lookup: the offsets the header states");
static_assert(sb_lookup::MAX_VALUES == SB_KEY_MAX_KEYS && SB_KEY_MAX_KEYS == KEY_MAX_KEYS, "the header's limit");

// The prepared list of a column (sb_key_lookup_prep.h) appended to `blob` at a multiple of 8, as [words | ids | bytes]; lc's
// pointers are offsets in `blob` until the lists have their place on the device.
static void look_list_append(const sb_lookup::Prepared& pr, std::vector<uint8_t>& blob, LookCol* lc) {
    blob.resize(align_up(blob.size(), 8));
    lc->keys = (const uint64_t*)(uintptr_t)blob.size();
    blob.insert(blob.end(), (const uint8_t*)pr.words.data(), (const uint8_t*)(pr.words.data() + pr.words.size()));
    lc->kid = (const uint32_t*)(uintptr_t)blob.size();
    blob.insert(blob.end(), (const uint8_t*)pr.ids.data(), (const uint8_t*)(pr.ids.data() + pr.ids.size()));
    blob.resize(align_up(blob.size(), 8));
    lc->bytes = (const uint8_t*)(uintptr_t)blob.size();
    blob.insert(blob.end(), pr.bytes.begin(), pr.bytes.end());
    lc->n = pr.n;
    lc->steps = pr.steps;
}

// The sibling of key_ids_decoded for the numeric columns of a replayed call: searched from the staging area by
// k_key_lookup_plain.  The lists go to the device in a buffer of the interval's, as filter_in_columns_decoded has it.
static int32_t key_lookup_decoded(sb_ctx* ctx, std::vector<sb_column_read>&& pages, std::vector<AggCol>& hs, std::vector<LookCol>& hl,
                                  const std::vector<uint8_t>& blob, void* const* users) {
    const uint64_t n = pages.size();
    ReplayCols rp;
    int32_t rc = open_replay(ctx, std::move(pages), hs, "key lookup", rp);
    if (rc != SB_OK) return rc;
    // [AggCol per column][LookCol per column][the results][the columns' states][the lists]
    const size_t res_stride = LOOK_RESULT_WORDS * sizeof(uint64_t);
    ReplayArena a;
    const size_t o_ac = a.add(hs.data(), n * sizeof(AggCol));
    const size_t o_lc = a.add(hl.data(), n * sizeof(LookCol));
    const size_t o_res = a.add(n * res_stride);
    const size_t o_state = a.add(n * sizeof(LookState));
    const size_t o_lists = a.add(blob.data(), blob.size());
    if ((rc = a.alloc(ctx, "key lookup replay")) != SB_OK) return rc;
    for (LookCol& lc : hl) rebase(lc, a.at<uint8_t>(o_lists));
    if ((rc = a.upload(ctx, "key lookup replay: upload failed")) != SB_OK) return rc;
    StageSlot* slot = acquire_slot(ctx, n * res_stride);
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    uint64_t* d_res = a.at<uint64_t>(o_res);
    const LookLaunch ll{a.at<const AggCol>(o_ac), a.at<const LookCol>(o_lc), a.at<LookState>(o_state), (uint32_t)n, true, false};
    launch_look_zero(ctx, ll);
    launch_key_lookup_plain(ctx, ll, rp.rows.data(), rp.vals.data(), rp.bits.data());
    launch_look_finish(ctx, ll, d_res);
    return queue_sink_results(ctx, slot, d_res, res_stride, n, Pending::KEY_LOOK_COL, users, nullptr, "key lookup");
}

int32_t sb_key_lookup(sb_ctx* ctx, sb_column_key_lookup* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_key_lookup", &rc)) return rc;
    std::vector<AggCol> hs(n);
    std::vector<uint64_t> cap(n);
    uint64_t pages = 0;
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_key_lookup& c = cols[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
        const bool bin = is_binary_t(c.physical_type);
        if (!bin && (c.physical_type < SB_TYPE_INT8 || c.physical_type > SB_TYPE_UINT64))
            return refuse(ctx, SB_ERR_NYI, "key lookup is implemented for 8- to 64-bit integers and binary types");
        if (const char* why = ids_check_width(c)) return refuse(ctx, SB_ERR_INVALID, why);
        if (c.reserved0 || c.reserved) return refuse(ctx, SB_ERR_INVALID, "reserved is not 0");
        const char* why = sb_lookup::check_list(bin, c.values, c.value_offsets, c.n_values);
        if (!why) why = sb_lookup::check_ids(c.value_ids, c.n_values, c.id_width);
        if (why) return refuse(ctx, SB_ERR_INVALID, why);
        // (numbers: searched like a minimum is taken, every live value is looked at; strings: as sb_key_ids_var has them)
        if ((rc = agg_check_fill(ctx, c, bin ? 0u : (uint32_t)SB_AGG_MIN, hs[i])) != SB_OK) return rc;
        const uint64_t rows = hs[i].rows;
        if ((why = ids_check_buffer(c, rows))) return refuse(ctx, SB_ERR_INVALID, why);
        for (uint64_t p = 0; bin && p < c.n_pages; p++)   // (the limits of sb_key_ids_var: its id tables and entry records)
            if (c.metas[p].num_values > (1ull << KEYV_INDEX_BITS) || c.metas[p].length / 8 >= (1ull << KEYV_INDEX_BITS))
                return refuse(ctx, SB_ERR_NYI, "sb_key_lookup: a binary page of more than 2^26 rows or of 2^29 bytes or more");
        if (bin) pages += c.n_pages;
        // the share of the staging area a filter column has (the caller's stage_capacity stays as given: a replay reads it again)
        cap[i] = bin ? (c.stage_capacity ? c.stage_capacity : 4 * c.pages_len) : rows * type_width(c.physical_type);
    }
    if (pages >= (1ull << KEYV_PAGE_BITS)) return refuse(ctx, SB_ERR_NYI, "sb_key_lookup: 2^28 binary pages or more in one call");
    if (const char* why = ids_check_overlaps(cols, hs)) return refuse(ctx, SB_ERR_INVALID, why);
    // the lists as the kernels search them, one blob for the call
    std::vector<LookCol> hl(n);
    std::vector<uint8_t> blob;
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_key_lookup& c = cols[i];
        memset(&hl[i], 0, sizeof hl[i]);
        hl[i].ids = (uint8_t*)c.ids;
        hl[i].idw = c.id_width;
        const sb_lookup::Prepared pr = is_binary_t(c.physical_type)
                                           ? sb_lookup::prepare_binary(c.values, c.value_offsets, c.value_ids, c.n_values)
                                           : sb_lookup::prepare_numeric(c.values, hs[i].w, hs[i].kind == FK_SIGNED, c.value_ids, c.n_values);
        look_list_append(pr, blob, &hl[i]);
    }
    (void)hipSetDevice(ctx->device);
    std::vector<sb_column_read> rc_cols;
    std::vector<void*> users;
    read_cols_of(cols, n, rc_cols, users);
    if (ctx->in_replay && ctx->filter_freq) {
        // The numeric columns through a full decode, as sb_key_ids has it; the binary columns as ever (a binary Freq page is
        // a virtual Dict page).  The ids are a function of the data and the list alone, so the route does not show in them.
        std::vector<bool> dec(n);
        for (uint64_t i = 0; i < n; i++) dec[i] = !is_binary_t(rc_cols[i].physical_type);
        std::vector<sb_column_read> r_num = take_if(rc_cols, dec);
        std::vector<AggCol> g_num = take_if(hs, dec);
        std::vector<LookCol> l_num = take_if(hl, dec);
        const std::vector<void*> u_num = take_if(users, dec);
        take_if(cap, dec);
        if (!r_num.empty()) rc = key_lookup_decoded(ctx, std::move(r_num), g_num, l_num, blob, u_num.data());
    }
    if (rc == SB_OK && !rc_cols.empty()) {
        if ((rc = stage_shares(ctx, rc_cols.data(), cap.data(), rc_cols.size())) != SB_OK) return rc;
        ReadMode mode{ReadMode::KEY_LOOKUP};
        mode.aggc = hs.data();
        mode.lookc = hl.data();
        mode.lits = &blob;
        mode.users = users.data();
        mode.pending_kind = Pending::KEY_LOOK_COL;
        rc = read_columns_impl(ctx, rc_cols.data(), rc_cols.size(), SB_MEM_DEVICE, mode);
    }
    if (rc != SB_OK) return rc;
    for (uint64_t i = 0; i < n; i++) {   // (after the last thing that can refuse the call: a page outside pages_len)
        sb_column_key_lookup& c = cols[i];
        column_rows(c, &c.rows);
        c.selected = c.count = c.matched = 0;
    }
    if (!ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::KEY_LOOKUP, cols, n, sb_write_options{}, mem});
    return rc;
}

// ------------------------------------------------------------------------------------ range-bucket ids
static_assert(sizeof(sb_column_key_buckets) == 168 && offsetof(sb_column_key_buckets, selection) == 48 &&
                  offsetof(sb_column_key_buckets, selection_capacity) == 56 && offsetof(sb_column_key_buckets, ids) == 64 &&
                  offsetof(sb_column_key_buckets, ids_capacity) == 72 && offsetof(sb_column_key_buckets, id_width) == 80 &&
                  offsetof(sb_column_key_buckets, flags) == 84 && offsetof(sb_column_key_buckets, bounds) == 88 &&
                  offsetof(sb_column_key_buckets, bucket_ids) == 96 && offsetof(sb_column_key_buckets, n_bounds) == 104 &&
                  offsetof(sb_column_key_buckets, nan_id) == 112 && offsetof(sb_column_key_buckets, reserved0) == 116 &&
                  offsetof(sb_column_key_buckets, reserved) == 120 && offsetof(sb_column_key_buckets, rows) == 128 &&
                  offsetof(sb_column_key_buckets, selected) == 136 && offsetof(sb_column_key_buckets, count) == 144 &&
                  offsetof(sb_column_key_buckets, matched) == 152 && offsetof(sb_column_key_buckets, nans) == 160,
              "sb_column_key_buckets: the offsets the header states");
static_assert(offsetof(sb_column_key_buckets, id_width) == offsetof(sb_column_key_lookup, id_width) &&
                  offsetof(sb_column_key_buckets, ids_capacity) == offsetof(sb_column_key_lookup, ids_capacity),
              "the first 84 bytes are sb_column_key_lookup's");
static_assert(sb_buckets::MAX_BOUNDS == SB_BUCKET_MAX_BOUNDS && SB_BUCKET_MAX_BOUNDS == BUCK_MAX_BOUNDS && SB_BUCKET_MAX_BOUNDS + 1 == SB_AGG_LARGE_MAX_GROUPS &&
                  sb_buckets::RIGHT_CLOSED == SB_BUCKET_RIGHT_CLOSED && sb_buckets::ID_NONE == SB_KEY_ID_NONE,
              "the header's limits");
static_assert(sb_buckets::UNSIGNED == FK_UNSIGNED && sb_buckets::SIGNED == FK_SIGNED && sb_buckets::F32 == FK_F32 && sb_buckets::F64 == FK_F64,
              "the preparation's kinds are the kernels'");

// The prepared bounds of a column (sb_key_buckets_prep.h) appended to `blob` at a multiple of 8, as [keys | ids]; bc's
// pointers are offsets in `blob` until the lists have their place on the device.
static void buck_list_append(const sb_buckets::Prepared& pr, std::vector<uint8_t>& blob, BuckCol* bc) {
    blob.resize(align_up(blob.size(), 8));
    bc->keys = (const uint64_t*)(uintptr_t)blob.size();
    blob.insert(blob.end(), (const uint8_t*)pr.keys.data(), (const uint8_t*)(pr.keys.data() + pr.keys.size()));
    bc->bid = (const uint32_t*)(uintptr_t)blob.size();
    blob.insert(blob.end(), (const uint8_t*)pr.ids.data(), (const uint8_t*)(pr.ids.data() + pr.ids.size()));
    bc->nan_lo = pr.nan_lo;
    bc->nan_hi = pr.nan_hi;
    bc->n = pr.n;
    bc->steps = pr.steps;
}

// key_lookup_decoded's sibling: the columns of a replayed call searched from the staging area by k_key_buckets_plain
static int32_t key_buckets_decoded(sb_ctx* ctx, std::vector<sb_column_read>&& pages, std::vector<AggCol>& hs, std::vector<BuckCol>& hb,
                                   const std::vector<uint8_t>& blob, void* const* users) {
    const uint64_t n = pages.size();
    ReplayCols rp;
    int32_t rc = open_replay(ctx, std::move(pages), hs, "key buckets", rp);
    if (rc != SB_OK) return rc;
    // [AggCol per column][BuckCol per column][the results][the columns' states][the lists]
    const size_t res_stride = BUCK_RESULT_WORDS * sizeof(uint64_t);
    ReplayArena a;
    const size_t o_ac = a.add(hs.data(), n * sizeof(AggCol));
    const size_t o_bc = a.add(hb.data(), n * sizeof(BuckCol));
    const size_t o_res = a.add(n * res_stride);
    const size_t o_state = a.add(n * sizeof(BuckState));
    const size_t o_lists = a.add(blob.data(), blob.size());
    if ((rc = a.alloc(ctx, "key buckets replay")) != SB_OK) return rc;
    for (BuckCol& bc : hb) rebase(bc, a.at<uint8_t>(o_lists));
    if ((rc = a.upload(ctx, "key buckets replay: upload failed")) != SB_OK) return rc;
    StageSlot* slot = acquire_slot(ctx, n * res_stride);
    if (!slot) return ctx->fail(SB_ERR_EXTERNAL, "hipHostMalloc(staging) failed");
    uint64_t* d_res = a.at<uint64_t>(o_res);
    const BuckLaunch bl{a.at<const AggCol>(o_ac), a.at<const BuckCol>(o_bc), a.at<BuckState>(o_state), (uint32_t)n};
    launch_buck_zero(ctx, bl);
    launch_key_buckets_plain(ctx, bl, rp.rows.data(), rp.vals.data(), rp.bits.data());
    launch_buck_finish(ctx, bl, d_res);
    return queue_sink_results(ctx, slot, d_res, res_stride, n, Pending::KEY_BUCKET_COL, users, nullptr, "key buckets");
}

int32_t sb_key_buckets(sb_ctx* ctx, sb_column_key_buckets* cols, uint64_t n, int32_t mem) {
    int32_t rc;
    if (!sink_entry(ctx, cols, n, mem, "sb_key_buckets", &rc)) return rc;
    std::vector<AggCol> hs(n);
    std::vector<uint64_t> cap(n);
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_key_buckets& c = cols[i];
        if (c.physical_type < 0 || c.physical_type > SB_TYPE_NULL) return refuse(ctx, SB_ERR_INVALID, "bad physical_type");
        const bool is_int = c.physical_type >= SB_TYPE_INT8 && c.physical_type <= SB_TYPE_UINT64;
        if (!is_int && c.physical_type != SB_TYPE_FLOAT32 && c.physical_type != SB_TYPE_FLOAT64)
            return refuse(ctx, SB_ERR_NYI, "key buckets are implemented for 8- to 64-bit integers and floats");
        if (const char* why = ids_check_width(c)) return refuse(ctx, SB_ERR_INVALID, why);
        if (c.reserved0 || c.reserved) return refuse(ctx, SB_ERR_INVALID, "reserved is not 0");
        const uint32_t kind = value_kind(c.physical_type), w = type_width(c.physical_type);
        const char* why = sb_buckets::check_bounds(kind, w, c.flags, c.bounds, c.n_bounds);
        if (!why) why = sb_buckets::check_ids(kind, c.bucket_ids, c.n_bounds, c.id_width, c.nan_id);
        if (why) return refuse(ctx, SB_ERR_INVALID, why);
        // (searched like a minimum is taken: every live value is looked at)
        if ((rc = agg_check_fill(ctx, c, (uint32_t)SB_AGG_MIN, hs[i])) != SB_OK) return rc;
        const uint64_t rows = hs[i].rows;
        if ((why = ids_check_buffer(c, rows))) return refuse(ctx, SB_ERR_INVALID, why);
        cap[i] = rows * w;   // the share of the staging area a filter column has
    }
    if (const char* why = ids_check_overlaps(cols, hs)) return refuse(ctx, SB_ERR_INVALID, why);
    // the bounds as the kernels search them, one blob for the call
    std::vector<BuckCol> hb(n);
    std::vector<uint8_t> blob;
    for (uint64_t i = 0; i < n; i++) {
        const sb_column_key_buckets& c = cols[i];
        memset(&hb[i], 0, sizeof hb[i]);
        hb[i].ids = (uint8_t*)c.ids;
        hb[i].idw = c.id_width;
        hb[i].right_closed = c.flags & SB_BUCKET_RIGHT_CLOSED;
        hb[i].nan_id = c.nan_id;
        buck_list_append(sb_buckets::prepare(hs[i].kind, hs[i].w, c.bounds, c.bucket_ids, c.n_bounds), blob, &hb[i]);
    }
    (void)hipSetDevice(ctx->device);
    std::vector<sb_column_read> rc_cols;
    std::vector<void*> users;
    read_cols_of(cols, n, rc_cols, users);
    if (ctx->in_replay && ctx->filter_freq) {
        // Every column through a full decode, as sb_key_lookup has its numeric columns.  The ids are a function of the data
        // and the struct alone, so the route does not show in them.
        rc = key_buckets_decoded(ctx, std::move(rc_cols), hs, hb, blob, users.data());
    } else {
        if ((rc = stage_shares(ctx, rc_cols.data(), cap.data(), rc_cols.size())) != SB_OK) return rc;
        ReadMode mode{ReadMode::KEY_BUCKETS};
        mode.aggc = hs.data();
        mode.buckc = hb.data();
        mode.lits = &blob;
        mode.users = users.data();
        mode.pending_kind = Pending::KEY_BUCKET_COL;
        rc = read_columns_impl(ctx, rc_cols.data(), rc_cols.size(), SB_MEM_DEVICE, mode);
    }
    if (rc != SB_OK) return rc;
    for (uint64_t i = 0; i < n; i++) {   // (after the last thing that can refuse the call: a page outside pages_len)
        sb_column_key_buckets& c = cols[i];
        column_rows(c, &c.rows);
        c.selected = c.count = c.matched = c.nans = 0;
    }
    if (!ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::KEY_BUCKETS, cols, n, sb_write_options{}, mem});
    return rc;
}


// The call synchronizes, and the interval it closes may hold earlier calls of which one asks for a replay: the replay
// drops every pending result and issues the recorded calls again, so the sizes call is recorded with them (its
// values_len would stay unwritten otherwise).  By itself a sizes call never asks for one: it goes by no launch hint.
int32_t sb_read_columns_sizes(sb_ctx* ctx, sb_column_read* cols, uint64_t n, int32_t mem) {
    int32_t rc = enqueue_read_sizes(ctx, cols, n, mem);
    if (rc != SB_OK) return rc;
    if (ctx && n && !ctx->in_replay) ctx->iv.calls.push_back(sb_ctx::Call{sb_ctx::Call::SIZES, cols, n, sb_write_options{}, mem});
    return sb_ctx_synchronize(ctx);
}

}  // extern "C"

int32_t enqueue_read_sizes(sb_ctx* ctx, sb_column_read* cols, uint64_t n, int32_t mem) {
    return read_columns_impl(ctx, cols, n, mem, ReadMode{ReadMode::SIZES});
}
