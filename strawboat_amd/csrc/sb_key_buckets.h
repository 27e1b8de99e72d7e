// strawboat-hip: sb_key_buckets — the range bucket of every row of a numeric key column (included by sb_decode.hip behind
// sb_key_lookup.h: the sink, the span, the store and the staging order are its LookSink / look_span / look_store, the id
// store sb_key_ids.h's key_id_store, the search sb_common.h's key_lower_bound over in_key order keys).
//
// GROUP BY date_trunc('month', d), price bands, histograms, GROUP BY over a float column: the pages of a key column, a
// selection bitmap (or none) and up to BUCK_MAX_BOUNDS strictly increasing bounds go in; every row gets the id of the
// bucket its value falls in, all ones where the row is not live or its bucket has no id.  The host hands every column its
// bounds as order keys and the id of each of the n + 1 buckets (BuckCol, sb_common.h).  The chain is sb_key_lookup's: a read
// call up to k_plan, then ONE walk with the same work items:
//   buck_zero                   the columns' states start from zero (one memset of 32 bytes per column)
//   k_key_buckets               the tiles.  None / LZ4 / Zstd / Snappy / Patas (from the staged column) / 4-byte bit-packed
//                               and delta: one search per row; OneValue: one per tile; Dict: one per entry into an LDS
//                               table of 16-bit bucket codes (<= FILTER_DICT_BITS entries), else one per row on the
//                               gathered entry; Freq: asks for the replay (KIND_REPLAY | KIND_FILTER_FREQ)
//   k_key_buckets_rle           rle_page_walk with RleKeyBuckets: one search per run, floats included
//   k_key_buckets_plain         the Freq replay: from the decoded column, one search per row
//   k_key_buckets_finish        one workgroup per column: `selected` counted, { selected, count, matched, nans } written
// A tile without a selected row loads no value and no index: its ids are all ones.
//
// The search keeps what sb_key_lookup's throws away: pos = key_lower_bound(keys, n, steps, key(x)) is the number of bounds
// below x, and a left-closed bucket adds 1 where keys[pos] == key(x).  The bucket code indexes the 4 KiB of ids in LDS.  A
// float whose order key lies outside [key(-inf), key(+inf)] is a NaN: its code is BUCK_NAN, its id the column's nan_id.
// -0.0 and +0.0 have one key (in_key), so both fall where 0.0 falls.
//
// The counts are look_span's scheme.  Integer columns go through look_span itself with two ballots per step; float columns
// through buck_span_f with a third ballot for the NaNs.  The column's kind is the same for every row of a tile or page, so
// the two are instances of one template chosen before the row loop: an integer column never pays the third ballot.
//
// The tile switch is written beside key_lookup_tile's, not shared with it by a template parameter, so that the kernels of
// sb_key_lookup.h keep their resource figures by construction.  Folding the two is a follow-up.
//
// Resources (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch 0 and no vector register spilled for
// every kernel):
//                             LDS bytes   VGPRs   workgroups per CU
//   k_key_buckets                 46384      93   3  (by its LDS, as k_key_lookup: 17 KiB index tile + 16 KiB bucket codes + 8 KiB
//                                                    keys + 4 KiB ids; the registers allow 5)
//   k_key_buckets_rle             33872     115   4  (17 KiB flags + 4 KiB run ids / codes + 8 KiB keys + 4 KiB ids; LDS and
//                                                    registers both allow 4)
//   k_key_buckets_plain           12568      18   8  (the 32 waves of a CU)
//   k_key_buckets_finish             32      12   8
#pragma once

namespace sb {

constexpr uint32_t BUCK_NAN = 0xFFFFu;   // the bucket code of a NaN (a bucket is at most BUCK_MAX_BOUNDS)
constexpr uint32_t BUCK_BAD = 0xFFFEu;   // ... of a row whose dictionary index is outside the dictionary: no id
static_assert(BUCK_MAX_BOUNDS + 1 <= KEY_MAX_KEYS && BUCK_MAX_BOUNDS < BUCK_BAD, "a bucket code fits 16 bits beside the markers");

struct BuckFind {
    const uint64_t* keys;   // LDS
    const uint32_t* bid;    // LDS: n + 1 ids
    uint64_t nan_lo, nan_hi;
    uint32_t n, steps, kind, w, rc, nan_id;
};
// the bucket code of a value: 0 .. n, BUCK_NAN for a NaN of a float column
template <bool FLT>
__device__ __forceinline__ uint32_t buck_code(const BuckFind& f, uint64_t raw) {
    const uint64_t x = in_key(f.kind, f.w, raw);
    uint32_t pos = key_lower_bound(f.keys, f.n, f.steps, x);
    if (!f.rc && pos < f.n && f.keys[pos] == x) pos++;   // (left-closed: the bound itself opens the next bucket)
    if (FLT && (x < f.nan_lo || x > f.nan_hi)) pos = BUCK_NAN;
    return pos;
}
__device__ __forceinline__ uint32_t buck_id(const BuckFind& f, uint32_t code) {
    return code <= f.n ? f.bid[code] : code == BUCK_NAN ? f.nan_id : LOOK_NONE;
}
// the column's keys and ids into LDS; the caller's barrier follows
__device__ __forceinline__ BuckFind buck_stage(const BuckCol& bc, const AggCol& g, uint64_t* s_keys, uint32_t* s_bid) {
    const uint32_t n = min(bc.n, BUCK_MAX_BOUNDS);
    for (uint32_t i = threadIdx.x; i < n; i += WG) s_keys[i] = bc.keys[i];
    for (uint32_t i = threadIdx.x; i <= n; i += WG) s_bid[i] = bc.bid[i];
    return BuckFind{s_keys, s_bid, bc.nan_lo, bc.nan_hi, n, bc.steps, g.kind, g.w, bc.right_closed, bc.nan_id};
}

// LookSink's sibling with the third count
struct BuckSink {
    LookSink k;
    uint32_t nan = 0;
};
// look_span for a float column: code_of(row) gives a live row's bucket code; every row of the span is stored
template <class F>
__device__ __forceinline__ void buck_span_f(BuckSink& b, const BuckFind& f, uint64_t lo, uint64_t hi, F code_of) {
    LookSink& k = b.k;
    for (uint64_t base = lo; base < hi; base += WG) {
        const uint64_t r = base + threadIdx.x, c = k.out_row + r;
        const bool in = r < hi;
        bool on = in;
        if (on && k.sel) on = (gld32(k.sel + (c >> 5)) >> (uint32_t)(c & 31)) & 1u;
        if (on && k.def_bits) on = (ldu8(k.def_bits + (r >> 3)) >> (uint32_t)(r & 7)) & 1u;
        const uint32_t code = on ? code_of(r) : BUCK_BAD;
        const uint32_t id = buck_id(f, code);
        if (in) key_id_store(k.ids, k.idw, c, id);
        k.live += (uint32_t)__popcll(__ballot(on));
        k.hit += (uint32_t)__popcll(__ballot(on && id != LOOK_NONE));
        b.nan += (uint32_t)__popcll(__ballot(on && code == BUCK_NAN));
    }
}
// The rows of a span whatever the column's kind: integers through look_span itself
template <bool FLT, class F>
__device__ __forceinline__ void buck_span(BuckSink& b, const BuckFind& f, uint64_t lo, uint64_t hi, F code_of) {
    if (FLT) buck_span_f(b, f, lo, hi, code_of);
    else look_span(b.k, lo, hi, [&](uint64_t r) { return buck_id(f, code_of(r)); });
}
// look_store with the NaNs of a float column behind it (flt: the same for the whole workgroup); s_cnt: 3 words of LDS
// that nothing else uses
__device__ __forceinline__ void buck_store(BuckSink& b, bool flt, BuckState* st, unsigned long long* s_cnt) {
    const uint32_t nan = b.nan;
    if (threadIdx.x == 0) s_cnt[2] = 0;
    look_store(b.k, (LookState*)st, s_cnt);   // (count and matched: the first 16 bytes of the state; its barriers cover s_cnt[2])
    b.nan = 0;
    if (!flt) return;
    if ((threadIdx.x & 63) == 0 && nan) atomicAdd(&s_cnt[2], (unsigned long long)nan);
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt[2]) atomicAdd((unsigned long long*)&st->nans, s_cnt[2]);
}
static_assert(offsetof(BuckState, count) == offsetof(LookState, count) && offsetof(BuckState, matched) == offsetof(LookState, matched),
              "a BuckState begins as a LookState");

template <bool FLT>
__device__ __forceinline__ void key_buckets_rows(const DecodeArgs& a, const TileTask& tt, const PageDesc& d, const PageTask& t, const ColDesc& c,
                                                 BuckSink& b, const BuckFind& f, uint64_t lo, uint32_t rows, uint32_t* s_a, uint32_t* s_w, uint16_t* s_pos) {
    const uint32_t w = c.width;
    const uint64_t hi = lo + rows;
    switch (d.codec) {
        case SB_CODEC_NONE: {
            const uint8_t* src = d.src;
            buck_span<FLT>(b, f, lo, hi, [&](uint64_t r) { return buck_code<FLT>(f, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {   // inflated into the staging area
            const uint8_t* src = c.values + t.out_row * w;
            buck_span<FLT>(b, f, lo, hi, [&](uint64_t r) { return buck_code<FLT>(f, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_ONEVALUE: {
            const uint32_t code = buck_code<FLT>(f, flt_load(d.body, w));
            buck_span<FLT>(b, f, lo, hi, [&](uint64_t) { return code; });
            break;
        }
        case SB_CODEC_DICT: {
            U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
            u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
            const uint8_t* dict = d.dict;
            const uint32_t D = d.dict_n;
            bool bad = false;
            if (D <= FILTER_DICT_BITS) {   // one search per entry into the tile's table of bucket codes
                for (uint32_t e = threadIdx.x; e < D; e += WG) s_pos[e] = (uint16_t)buck_code<FLT>(f, flt_load(dict + (uint64_t)e * w, w));
                __syncthreads();
                buck_span<FLT>(b, f, lo, hi, [&](uint64_t r) {
                    const uint32_t e = s_a[sidx((int)(r - lo))];
                    if (e >= D) {
                        bad = true;
                        return BUCK_BAD;
                    }
                    return (uint32_t)s_pos[e];
                });
            } else {
                buck_span<FLT>(b, f, lo, hi, [&](uint64_t r) {
                    const uint32_t e = s_a[sidx((int)(r - lo))];
                    if (e >= D) {
                        bad = true;
                        return BUCK_BAD;
                    }
                    return buck_code<FLT>(f, flt_load(dict + (uint64_t)e * w, w));
                });
            }
            if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 400);   // (where the key-id walk finds it)
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            u32_tile_to_lds(vs, tt.tile, rows, s_a, s_w);
            buck_span<FLT>(b, f, lo, hi, [&](uint64_t r) { return buck_code<FLT>(f, (uint64_t)s_a[sidx((int)(r - lo))]); });
            break;
        }
        default:
            break;
    }
}

__device__ void key_buckets_tile(const DecodeArgs& a, const BuckLaunch& bl, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint16_t* s_pos, uint64_t* s_keys,
                                 uint32_t* s_bid, unsigned long long* s_cnt, uint32_t* staged) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;   // (the interval fails)
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    // a Freq page asks for the replay whatever the selection, as in agg_tile
    if (d.codec == SB_CODEC_FREQ) {
        if (threadIdx.x == 0 && tt.tile == 0) atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
        return;
    }
    switch (d.codec) {   // (RLE pages of <= 8-byte values have no tiles: k_key_buckets_rle)
        case SB_CODEC_NONE:
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS:
        case SB_CODEC_ONEVALUE:
        case SB_CODEC_DICT: break;
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING:
            if (c.width != 4) return;
            break;
        default: return;
    }
    const AggCol g = bl.acols[tt.col];
    const BuckCol bc = bl.bcols[tt.col];
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    BuckSink b{LookSink{g.sel, d.def_bits, t.out_row, bc.ids, bc.idw}};
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) {   // no value and no index is loaded, nothing is counted
        look_span(b.k, lo, hi, [&](uint64_t) { return LOOK_NONE; });
        return;
    }
    if (*staged != tt.col) {   // (the same for every lane: the tile's column)
        __syncthreads();
        (void)buck_stage(bc, g, s_keys, s_bid);
        *staged = tt.col;
        __syncthreads();
    }
    const BuckFind f{s_keys, s_bid, bc.nan_lo, bc.nan_hi, min(bc.n, BUCK_MAX_BOUNDS), bc.steps, g.kind, c.width, bc.right_closed, bc.nan_id};
    const bool flt = g.kind == FK_F32 || g.kind == FK_F64;
    if (flt) key_buckets_rows<true>(a, tt, d, t, c, b, f, lo, rows, s_a, s_w, s_pos);
    else key_buckets_rows<false>(a, tt, d, t, c, b, f, lo, rows, s_a, s_w, s_pos);
    buck_store(b, flt, bl.st + tt.col, s_cnt);
}

__global__ void __launch_bounds__(WG) k_key_buckets(DecodeArgs a, BuckLaunch bl) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ unsigned long long s_cnt[3];
    __shared__ uint16_t s_pos[FILTER_DICT_BITS];
    __shared__ uint64_t s_keys[KEY_MAX_KEYS];
    __shared__ uint32_t s_bid[KEY_MAX_KEYS];
    const uint32_t count = a.job_counts[2];
    uint32_t staged = 0xFFFFFFFFu;
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        key_buckets_tile(a, bl, ti, s_a, s_w, s_pos, s_keys, s_bid, s_cnt, &staged);
        __syncthreads();
    }
}

// RLE pages: one search per run.  An integer run keeps its id, a float run its bucket code (the NaN runs are counted by row)
template <bool FLT>
struct RleKeyBuckets {
    using Rec = uint32_t;
    uint32_t* s_rec;
    BuckSink* b;
    BuckFind f;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + f.w; }
    __device__ __forceinline__ uint32_t load(const uint8_t* v, bool in) const {
        if (!in) return FLT ? BUCK_BAD : LOOK_NONE;
        const uint32_t code = buck_code<FLT>(f, flt_load(v, f.w));
        return FLT ? code : buck_id(f, code);
    }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        if (FLT) buck_span_f(*b, f, lo, hi, [&](uint64_t r) { return s_rec[A + s_flag[sidx((int)(r - tile_lo))]]; });
        else look_span(b->k, lo, hi, [&](uint64_t r) { return s_rec[A + s_flag[sidx((int)(r - tile_lo))]]; });
    }
};

__global__ void __launch_bounds__(WG) k_key_buckets_rle(DecodeArgs a, BuckLaunch bl) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint32_t s_run[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ unsigned long long s_cnt[3];
    __shared__ uint64_t s_keys[KEY_MAX_KEYS];
    __shared__ uint32_t s_bid[KEY_MAX_KEYS];
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    const AggCol g = bl.acols[t.col];
    const BuckCol bc = bl.bcols[t.col];
    const BuckFind f = buck_stage(bc, g, s_keys, s_bid);
    __syncthreads();   // (the walk's first loads search the keys)
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    BuckSink b{LookSink{g.sel, d.def_bits, t.out_row, bc.ids, bc.idw}};
    const bool flt = g.kind == FK_F32 || g.kind == FK_F64;
    if (flt) {
        const RleKeyBuckets<true> pol{s_run, &b, f};
        rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
    } else {
        const RleKeyBuckets<false> pol{s_run, &b, f};
        rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
    }
    __syncthreads();
    buck_store(b, flt, bl.st + t.col, s_cnt);
}

// the Freq replay: from the decoded column, one search per row; one launch per column, a workgroup per TILE_ROWS rows
__global__ void __launch_bounds__(WG) k_key_buckets_plain(BuckLaunch bl, uint32_t col, const uint8_t* values, const uint8_t* validity) {
    __shared__ uint64_t s_keys[KEY_MAX_KEYS];
    __shared__ uint32_t s_bid[KEY_MAX_KEYS];
    __shared__ unsigned long long s_cnt[3];
    const AggCol g = bl.acols[col];
    const BuckCol bc = bl.bcols[col];
    const uint64_t lo = (uint64_t)blockIdx.x * TILE_ROWS, hi = min(g.rows, lo + TILE_ROWS);
    BuckSink b{LookSink{g.sel, validity, 0, bc.ids, bc.idw}};
    if (!agg_any_selected(g.sel, lo, hi)) {
        look_span(b.k, lo, hi, [&](uint64_t) { return LOOK_NONE; });
        return;
    }
    const BuckFind f = buck_stage(bc, g, s_keys, s_bid);
    __syncthreads();
    const uint32_t w = g.w;
    const bool flt = g.kind == FK_F32 || g.kind == FK_F64;
    if (flt) buck_span<true>(b, f, lo, hi, [&](uint64_t r) { return buck_code<true>(f, flt_load(values + r * w, w)); });
    else buck_span<false>(b, f, lo, hi, [&](uint64_t r) { return buck_code<false>(f, flt_load(values + r * w, w)); });
    buck_store(b, flt, bl.st + col, s_cnt);
}

// ---- one workgroup per column: `selected` as k_key_lookup_finish counts it, and the column's record
__global__ void __launch_bounds__(WG) k_key_buckets_finish(BuckLaunch bl, uint64_t* results) {
    __shared__ uint64_t s_w64[4];
    const AggCol g = bl.acols[blockIdx.x];
    uint64_t nsel = 0;
    if (g.sel) {
        const uint64_t nwords = (g.rows + 31) / 32;
        for (uint64_t i = threadIdx.x; i < nwords; i += WG) {
            uint32_t v = gld32(g.sel + i);
            if (i == nwords - 1 && (g.rows & 31)) v &= (1u << (g.rows & 31)) - 1;   // bits behind `rows` are ignored
            nsel += (uint64_t)__popc(v);
        }
        nsel = wg_sum64(nsel, s_w64);
    } else {
        nsel = g.rows;
    }
    if (threadIdx.x == 0) {
        const BuckState* st = bl.st + blockIdx.x;   // (written by the walk's kernels: final here)
        uint64_t* r = results + (uint64_t)blockIdx.x * BUCK_RESULT_WORDS;
        r[0] = nsel, r[1] = st->count, r[2] = st->matched, r[3] = st->nans;
    }
}

// the states start from zero; timed under a name of its own
void launch_buck_zero(sb_ctx* ctx, const BuckLaunch& bl) {
    KScope k(ctx, "buck_zero(memset)");
    if (bl.n_cols) (void)hipMemsetAsync(bl.st, 0, (size_t)bl.n_cols * sizeof(BuckState), ctx->stream);
}

// The end of a buckets call, in launch_key_lookup's place: the pages are parsed, inflated and planned
void launch_key_buckets(sb_ctx* ctx, const DecodeArgs& a, const BuckLaunch& bl) {
    hipStream_t s = ctx->stream;
    {
        KScope k(ctx, "k_key_buckets_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_key_buckets_rle<<<dim3(a.n_pages, std::max<uint32_t>(1u, a.rle_parts)), WG, 0, s>>>(a, bl);
    }
    if (a.n_tiles) {
        KScope k(ctx, "k_key_buckets");
        k_key_buckets<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, bl);
    }
}

void launch_buck_finish(sb_ctx* ctx, const BuckLaunch& bl, uint64_t* results) {
    KScope k(ctx, "k_key_buckets_finish");
    k_key_buckets_finish<<<bl.n_cols, WG, 0, ctx->stream>>>(bl, results);
}

// `rows[i]`, `values[i]`, `validity[i]` (host arrays): the decoded columns of the replay
void launch_key_buckets_plain(sb_ctx* ctx, const BuckLaunch& bl, const uint64_t* rows, const uint8_t* const* values, const uint8_t* const* validity) {
    KScope k(ctx, "k_key_buckets_plain");
    for (uint32_t i = 0; i < bl.n_cols; i++)
        if (rows[i]) k_key_buckets_plain<<<(uint32_t)((rows[i] + TILE_ROWS - 1) / TILE_ROWS), WG, 0, ctx->stream>>>(bl, i, values[i], validity[i]);
}

}  // namespace sb
