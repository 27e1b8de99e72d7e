// strawboat-hip: sb_key_lookup — the ids a given list assigns to the rows of a key column (included by sb_decode.hip behind
// sb_key_ids_bin.h: the id store is sb_key_ids.h's key_id_store, the searches sb_common.h's key_lower_bound and the order of
// sb_filter_bin.h's bin_rel_prefix, the entries of Dict / Freq pages sb_filter_bin.h's bin_dict and sb_key_ids_bin.h's
// kv_entry / kv_row / kv_id_table).
//
// fact.fk = dim.pk with a small dimension, GROUP BY over a key set that is known, ids that mean the same in every call:
// the pages of a key column, a selection bitmap (or none) and a list of up to KEY_MAX_KEYS values go in; every row gets the
// id the list gives its value, all ones where the row is not live or its value is not in the list.  The host hands every
// column its list sorted and without duplicates (LookCol, sb_common.h) with the id of each sorted position beside it.
// The chain is a read call up to k_plan (binary columns: up to the staged value blocks, k_keyv_base and queues B / Z), then
// ONE walk -- there is nothing to discover, so no table, no sort and no second pass:
//   look_zero                 the columns' states start from zero (one memset of 16 bytes per column)
//   numbers  k_key_lookup       the tiles.  None / LZ4 / Zstd / Snappy / Patas (from the staged column) / 4-byte bit-packed
//                               and delta: one search per row; OneValue: one per tile; Dict: one per entry into an LDS
//                               table (<= FILTER_DICT_BITS entries), else one per row on the gathered entry; Freq: asks
//                               for the replay (KIND_REPLAY | KIND_FILTER_FREQ)
//            k_key_lookup_rle   rle_page_walk with RleKeyLookup: one search per run
//            k_key_lookup_plain the Freq replay: from the decoded column, one search per row
//   binary   k_key_lookup_bin_entries  grid (pages, FILTER_BIN_EY), a lane per entry of every Dict / Freq page: the entry's
//                               sorted position (0xFFFF: not in the list) into the page's 16-bit id table
//            k_key_lookup_bin   the tiles.  Dict / Freq: the table (LDS up to FILTER_DICT_BITS entries, gathered beyond);
//                               OneValue: one search per tile; Basic: one per row
//   k_key_lookup_finish       one workgroup per column: `selected` counted, { selected, count, matched, 0 } written
// A tile without a selected row loads no value and no index: its ids are all ones.
//
// A hit is the lower bound followed by an equality test: a value between two entries of the list, below the first or above
// the last gets all ones.  The numeric search is key_lower_bound over the keys in LDS: branch-free, with the trip count of
// the column for every lane.  The binary search is in_bin_eval's (sb_filter_in.h) returning the position: the first word
// of a literal is one load, which stays inside the set because 8 zero bytes follow the literals; the loads of the strings
// stay inside their buffers by the rule at the head of sb_filter_bin.h.
//
// The Dict table holds SORTED POSITIONS in 16 bits (they are below KEY_MAX_KEYS; 0xFFFF = no match) and the row's store
// maps the position to the list's 32-bit id through the 4 KiB of ids in LDS: 16 KiB for the table instead of 32, which
// keeps a third workgroup on the CU.
//
// count and matched are integer counts: a ballot and a popcount per step of a wave, one LDS add per wave and tile (or page
// part), one global integer atomic per tile / part and counter.  No atomic per row, and sums of integers do not depend on
// the order they arrive in: the results are the same every time.
//
// Resources (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage; scratch 0 for every kernel):
//                             LDS bytes   VGPRs   workgroups per CU
//   k_key_lookup                  46368      86   3  (by its LDS: 17 KiB index tile + 16 KiB positions + 8 KiB keys + 4 KiB ids;
//                                                    the registers allow 5)
//   k_key_lookup_rle              33856     110   4  (17 KiB flags + 4 KiB run ids + 8 KiB keys + 4 KiB ids; LDS and registers
//                                                    both allow 4)
//   k_key_lookup_plain            12560      18   8  (the 32 waves of a CU)
//   k_key_lookup_bin_entries          0      28   8
//   k_key_lookup_bin              34080      99   4  (17 KiB index tile + 16 KiB positions; LDS and registers both allow 4)
//   k_key_lookup_finish              32      12   8
#pragma once

namespace sb {

constexpr uint32_t LOOK_NONE = 0xFFFFFFFFu;   // SB_KEY_ID_NONE
constexpr uint32_t LOOK_NOPOS = 0xFFFFu;      // a Dict table's "not in the list" (a position is below KEY_MAX_KEYS)
static_assert(KEY_MAX_KEYS <= LOOK_NOPOS, "a sorted position fits 16 bits beside the marker");

// What the rows of a tile / page part end in: the ids, and the wave's share of the two counts (the same number in every
// lane of a wave: look_span adds popcounts of ballots)
struct LookSink {
    const uint32_t* sel;       // as in AggSink
    const uint8_t* def_bits;
    uint64_t out_row;
    uint8_t* ids;
    uint32_t idw;
    uint32_t live = 0, hit = 0;
};
// Rows [lo, hi) of a page by the whole workgroup, a lane per row and the same number of steps for every lane (the ballots).
// id_of(row) gives a live row's id, LOOK_NONE where its value is not in the list; every row of the span is stored.
template <class F>
__device__ __forceinline__ void look_span(LookSink& k, uint64_t lo, uint64_t hi, F id_of) {
    for (uint64_t base = lo; base < hi; base += WG) {
        const uint64_t r = base + threadIdx.x, c = k.out_row + r;
        const bool in = r < hi;
        bool on = in;
        if (on && k.sel) on = (gld32(k.sel + (c >> 5)) >> (uint32_t)(c & 31)) & 1u;
        if (on && k.def_bits) on = (ldu8(k.def_bits + (r >> 3)) >> (uint32_t)(r & 7)) & 1u;
        const uint32_t id = on ? id_of(r) : LOOK_NONE;
        if (in) key_id_store(k.ids, k.idw, c, id);
        k.live += (uint32_t)__popcll(__ballot(on));
        k.hit += (uint32_t)__popcll(__ballot(on && id != LOOK_NONE));
    }
}
// The end of a tile or page part: the waves' counts into LDS, their sums into the column's state; by the whole workgroup.
// s_cnt: 2 words of LDS that nothing else uses.
__device__ __forceinline__ void look_store(LookSink& k, LookState* st, unsigned long long* s_cnt) {
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        if (k.live) atomicAdd(&s_cnt[0], (unsigned long long)k.live);
        if (k.hit) atomicAdd(&s_cnt[1], (unsigned long long)k.hit);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_cnt[0]) atomicAdd((unsigned long long*)&st->count, s_cnt[0]);
        if (s_cnt[1]) atomicAdd((unsigned long long*)&st->matched, s_cnt[1]);
    }
    k.live = k.hit = 0;
}

// ---- numbers
struct LookFind {
    const uint64_t* keys;   // LDS
    const uint32_t* kid;    // LDS
    uint32_t n, steps, kind, w;
};
// the sorted position of the value, LOOK_NOPOS where it is not one of the keys
__device__ __forceinline__ uint32_t look_pos(const LookFind& f, uint64_t raw) {
    const uint64_t x = in_key(f.kind, f.w, raw);
    const uint32_t pos = key_lower_bound(f.keys, f.n, f.steps, x);
    return (f.n != 0 && pos < f.n && f.keys[min(pos, f.n - 1)] == x) ? pos : LOOK_NOPOS;
}
__device__ __forceinline__ uint32_t look_id_at(const uint32_t* kid, uint32_t n, uint32_t pos) { return pos < n ? kid[pos] : LOOK_NONE; }
__device__ __forceinline__ uint32_t look_find(const LookFind& f, uint64_t raw) { return look_id_at(f.kid, f.n, look_pos(f, raw)); }
// the column's keys and their ids into LDS, as in_stage does it; the caller's barrier follows
__device__ __forceinline__ LookFind look_stage(const LookCol& lc, const AggCol& g, uint64_t* s_keys, uint32_t* s_kid) {
    const uint32_t n = min(lc.n, KEY_MAX_KEYS);
    for (uint32_t i = threadIdx.x; i < n; i += WG) s_keys[i] = lc.keys[i], s_kid[i] = lc.kid[i];
    return LookFind{s_keys, s_kid, n, lc.steps, g.kind, g.w};
}

__device__ void key_lookup_tile(const DecodeArgs& a, const LookLaunch& ll, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint16_t* s_pos, uint64_t* s_keys,
                                uint32_t* s_kid, unsigned long long* s_cnt, uint32_t* staged) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;   // (the interval fails)
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    if (is_binary(c.ptype)) return;   // (k_key_lookup_bin)
    // a Freq page asks for the replay whatever the selection, as in agg_tile
    if (d.codec == SB_CODEC_FREQ) {
        if (threadIdx.x == 0 && tt.tile == 0) atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
        return;
    }
    const AggCol g = ll.acols[tt.col];
    const LookCol lc = ll.lcols[tt.col];
    const uint32_t w = c.width;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    LookSink k{g.sel, d.def_bits, t.out_row, lc.ids, lc.idw};
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) {   // no value and no index is loaded, nothing is counted
        look_span(k, lo, hi, [&](uint64_t) { return LOOK_NONE; });
        return;
    }
    if (*staged != tt.col) {   // (the same for every lane: the tile's column)
        __syncthreads();
        (void)look_stage(lc, g, s_keys, s_kid);
        *staged = tt.col;
        __syncthreads();
    }
    const LookFind f{s_keys, s_kid, min(lc.n, KEY_MAX_KEYS), lc.steps, g.kind, w};
    switch (d.codec) {
        case SB_CODEC_NONE: {
            const uint8_t* src = d.src;
            look_span(k, lo, hi, [&](uint64_t r) { return look_find(f, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {   // inflated into the staging area
            const uint8_t* src = c.values + t.out_row * w;
            look_span(k, lo, hi, [&](uint64_t r) { return look_find(f, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_ONEVALUE: {
            const uint32_t id = look_find(f, flt_load(d.body, w));
            look_span(k, lo, hi, [&](uint64_t) { return id; });
            break;
        }
        case SB_CODEC_DICT: {
            U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
            u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
            const uint8_t* dict = d.dict;
            const uint32_t D = d.dict_n;
            bool bad = false;
            if (D <= FILTER_DICT_BITS) {   // one search per entry into the tile's table of sorted positions
                for (uint32_t e = threadIdx.x; e < D; e += WG) s_pos[e] = (uint16_t)look_pos(f, flt_load(dict + (uint64_t)e * w, w));
                __syncthreads();
                look_span(k, lo, hi, [&](uint64_t r) {
                    const uint32_t e = s_a[sidx((int)(r - lo))];
                    if (e >= D) {
                        bad = true;
                        return LOOK_NONE;
                    }
                    return look_id_at(f.kid, f.n, s_pos[e]);
                });
            } else {
                look_span(k, lo, hi, [&](uint64_t r) {
                    const uint32_t e = s_a[sidx((int)(r - lo))];
                    if (e >= D) {
                        bad = true;
                        return LOOK_NONE;
                    }
                    return look_find(f, flt_load(dict + (uint64_t)e * w, w));
                });
            }
            if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 400);   // (where the key-id walk finds it)
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            if (w != 4) return;
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            u32_tile_to_lds(vs, tt.tile, rows, s_a, s_w);
            look_span(k, lo, hi, [&](uint64_t r) { return look_find(f, (uint64_t)s_a[sidx((int)(r - lo))]); });
            break;
        }
        default:   // (RLE pages of <= 8-byte values have no tiles: k_key_lookup_rle)
            return;
    }
    look_store(k, ll.st + tt.col, s_cnt);
}

__global__ void __launch_bounds__(WG) k_key_lookup(DecodeArgs a, LookLaunch ll) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ unsigned long long s_cnt[2];
    __shared__ uint16_t s_pos[FILTER_DICT_BITS];
    __shared__ uint64_t s_keys[KEY_MAX_KEYS];
    __shared__ uint32_t s_kid[KEY_MAX_KEYS];
    const uint32_t count = a.job_counts[2];
    uint32_t staged = 0xFFFFFFFFu;
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        key_lookup_tile(a, ll, ti, s_a, s_w, s_pos, s_keys, s_kid, s_cnt, &staged);
        __syncthreads();
    }
}

// RLE pages: one search per run into its id
struct RleKeyLookup {
    using Rec = uint32_t;
    uint32_t* s_rec;
    LookSink* k;
    LookFind f;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + f.w; }
    __device__ __forceinline__ uint32_t load(const uint8_t* v, bool in) const { return in ? look_find(f, flt_load(v, f.w)) : LOOK_NONE; }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        look_span(*k, lo, hi, [&](uint64_t r) { return s_rec[A + s_flag[sidx((int)(r - tile_lo))]]; });
    }
};

__global__ void __launch_bounds__(WG) k_key_lookup_rle(DecodeArgs a, LookLaunch ll) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint32_t s_run[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ unsigned long long s_cnt[2];
    __shared__ uint64_t s_keys[KEY_MAX_KEYS];
    __shared__ uint32_t s_kid[KEY_MAX_KEYS];
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    const AggCol g = ll.acols[t.col];
    const LookCol lc = ll.lcols[t.col];
    const LookFind f = look_stage(lc, g, s_keys, s_kid);
    __syncthreads();   // (the walk's first loads search the keys)
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    LookSink k{g.sel, d.def_bits, t.out_row, lc.ids, lc.idw};
    const RleKeyLookup pol{s_run, &k, f};
    rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
    __syncthreads();
    look_store(k, ll.st + t.col, s_cnt);
}

// the Freq replay: from the decoded column, one search per row; one launch per column, a workgroup per TILE_ROWS rows
__global__ void __launch_bounds__(WG) k_key_lookup_plain(LookLaunch ll, uint32_t col, const uint8_t* values, const uint8_t* validity) {
    __shared__ uint64_t s_keys[KEY_MAX_KEYS];
    __shared__ uint32_t s_kid[KEY_MAX_KEYS];
    __shared__ unsigned long long s_cnt[2];
    const AggCol g = ll.acols[col];
    const LookCol lc = ll.lcols[col];
    const uint64_t lo = (uint64_t)blockIdx.x * TILE_ROWS, hi = min(g.rows, lo + TILE_ROWS);
    LookSink k{g.sel, validity, 0, lc.ids, lc.idw};
    if (!agg_any_selected(g.sel, lo, hi)) {
        look_span(k, lo, hi, [&](uint64_t) { return LOOK_NONE; });
        return;
    }
    const LookFind f = look_stage(lc, g, s_keys, s_kid);
    __syncthreads();
    const uint32_t w = g.w;
    look_span(k, lo, hi, [&](uint64_t r) { return look_find(f, flt_load(values + r * w, w)); });
    look_store(k, ll.st + col, s_cnt);
}

// ---- binary columns
// The string's sorted position among the literals, LOOK_NOPOS where it is none of them: in_bin_eval's search with its
// three-way order, returning where it ends
__device__ __forceinline__ uint32_t look_bin_pos(const LookCol& lc, const uint8_t* v, uint32_t len) {
    uint32_t lo = 0, hi = min(lc.n, KEY_MAX_KEYS);
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint64_t o0 = lc.keys[mid], o1 = lc.keys[mid + 1];
        const uint8_t* p = lc.bytes + o0;
        const BinLit l{p, ldu64(p), (uint32_t)(o1 - o0), 0u};
        uint32_t r = bin_rel_prefix(v, l, min(len, l.len));
        if (r == 1u) r = len < l.len ? 0u : len == l.len ? 1u : 2u;
        if (r == 1u) return mid;
        if (r == 0u) hi = mid;
        else lo = mid + 1;
    }
    return LOOK_NOPOS;
}
__device__ __forceinline__ uint32_t look_bin_find(const LookCol& lc, const KvStr& s) {
    return look_id_at(lc.kid, min(lc.n, KEY_MAX_KEYS), look_bin_pos(lc, s.p, s.len));
}

// grid (pages, FILTER_BIN_EY): the sorted position of every entry into the page's id table
__global__ void __launch_bounds__(WG) k_key_lookup_bin_entries(DecodeArgs a, LookLaunch ll) {
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    if (!d.ok || (d.codec != SB_CODEC_DICT && d.codec != SB_CODEC_FREQ)) return;
    const PageTask t = a.tasks[p];
    if (!is_binary(a.cols[t.col].ptype)) return;
    BinDict bd;
    uint16_t* ids = nullptr;
    if (!bin_dict(a, t, d, &bd) || !kv_id_table(t, bd, &ids)) {
        if (threadIdx.x == 0 && blockIdx.y == 0) raise(a.status, SB_ERR_INVALID, p, 220);
        return;
    }
    const LookCol lc = ll.lcols[t.col];
    for (uint32_t e0 = blockIdx.y * WG; e0 < bd.D; e0 += gridDim.y * WG) {
        const uint32_t e = e0 + threadIdx.x;
        if (e >= bd.D) continue;
        const KvStr s = kv_entry(d.dict, bd, e);
        ids[e] = (uint16_t)look_bin_pos(lc, s.p, s.len);
    }
}

__device__ void key_lookup_bin_tile(const DecodeArgs& a, const LookLaunch& ll, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint16_t* s_pos,
                                    unsigned long long* s_cnt) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;   // (the interval fails)
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    if (!is_binary(c.ptype)) return;   // (k_key_lookup)
    const AggCol g = ll.acols[tt.col];
    const LookCol lc = ll.lcols[tt.col];
    const uint32_t n = min(lc.n, KEY_MAX_KEYS);
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    LookSink k{g.sel, d.def_bits, t.out_row, lc.ids, lc.idw};
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) {   // no value and no index is loaded, nothing is counted
        look_span(k, lo, hi, [&](uint64_t) { return LOOK_NONE; });
        return;
    }
    if (d.codec == SB_CODEC_DICT || d.codec == SB_CODEC_FREQ) {
        BinDict bd;
        uint16_t* ids = nullptr;
        if (!bin_dict(a, t, d, &bd) || !kv_id_table(t, bd, &ids)) return;   // (raised by k_key_lookup_bin_entries)
        U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
        u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
        const uint32_t D = bd.D;
        const uint32_t* kid = lc.kid;
        bool bad = false;
        if (D <= FILTER_DICT_BITS) {
            for (uint32_t e = threadIdx.x; e < D; e += WG) s_pos[e] = ids[e];
            __syncthreads();
            look_span(k, lo, hi, [&](uint64_t r) {
                const uint32_t e = s_a[sidx((int)(r - lo))];
                if (e >= D) {
                    bad = true;
                    return LOOK_NONE;
                }
                return look_id_at(kid, n, s_pos[e]);
            });
        } else {
            look_span(k, lo, hi, [&](uint64_t r) {
                const uint32_t e = s_a[sidx((int)(r - lo))];
                if (e >= D) {
                    bad = true;
                    return LOOK_NONE;
                }
                return look_id_at(kid, n, ids[e]);
            });
        }
        if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 222);   // (where the var filter finds it)
    } else if (is_basic(d.codec)) {
        const uint8_t* vals = kv_vals(c, d);
        look_span(k, lo, hi, [&](uint64_t r) { return look_bin_find(lc, kv_row(c.ptype, d.src, vals, d.vusize, r)); });
    } else if (d.codec == SB_CODEC_ONEVALUE) {
        const uint32_t id = look_bin_find(lc, KvStr{d.dict, d.dict_n});
        look_span(k, lo, hi, [&](uint64_t) { return id; });
    } else {
        return;
    }
    look_store(k, ll.st + tt.col, s_cnt);
}

__global__ void __launch_bounds__(WG) k_key_lookup_bin(DecodeArgs a, LookLaunch ll) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ unsigned long long s_cnt[2];
    __shared__ uint16_t s_pos[FILTER_DICT_BITS];
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        key_lookup_bin_tile(a, ll, ti, s_a, s_w, s_pos, s_cnt);
        __syncthreads();
    }
}

// ---- one workgroup per column: `selected` as k_key_finish counts it, and the column's record { selected, count, matched, 0 }
__global__ void __launch_bounds__(WG) k_key_lookup_finish(LookLaunch ll, uint64_t* results) {
    __shared__ uint64_t s_w64[4];
    const AggCol g = ll.acols[blockIdx.x];
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
        const LookState* st = ll.st + blockIdx.x;   // (written by the walk's kernels: final here)
        uint64_t* r = results + (uint64_t)blockIdx.x * LOOK_RESULT_WORDS;
        r[0] = nsel, r[1] = st->count, r[2] = st->matched, r[3] = 0;
    }
}

// the states start from zero; timed under a name of its own
void launch_look_zero(sb_ctx* ctx, const LookLaunch& ll) {
    KScope k(ctx, "look_zero(memset)");
    if (ll.n_cols) (void)hipMemsetAsync(ll.st, 0, (size_t)ll.n_cols * sizeof(LookState), ctx->stream);
}

// The end of a lookup call, in launch_key_collect's place: the pages are parsed, inflated and planned
void launch_key_lookup(sb_ctx* ctx, const DecodeArgs& a, const LookLaunch& ll) {
    hipStream_t s = ctx->stream;
    if (ll.any_num) {
        KScope k(ctx, "k_key_lookup_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_key_lookup_rle<<<dim3(a.n_pages, std::max<uint32_t>(1u, a.rle_parts)), WG, 0, s>>>(a, ll);
    }
    if (ll.any_num && a.n_tiles) {
        KScope k(ctx, "k_key_lookup");
        k_key_lookup<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, ll);
    }
    if (ll.any_bin) {
        KScope k(ctx, "k_key_lookup_bin_entries");
        k_key_lookup_bin_entries<<<dim3(a.n_pages, FILTER_BIN_EY), WG, 0, s>>>(a, ll);
    }
    if (ll.any_bin && a.n_tiles) {
        KScope k(ctx, "k_key_lookup_bin");
        k_key_lookup_bin<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, ll);
    }
}

void launch_look_finish(sb_ctx* ctx, const LookLaunch& ll, uint64_t* results) {
    KScope k(ctx, "k_key_lookup_finish");
    k_key_lookup_finish<<<ll.n_cols, WG, 0, ctx->stream>>>(ll, results);
}

// `rows[i]`, `values[i]`, `validity[i]` (host arrays): the decoded columns of the replay
void launch_key_lookup_plain(sb_ctx* ctx, const LookLaunch& ll, const uint64_t* rows, const uint8_t* const* values, const uint8_t* const* validity) {
    KScope k(ctx, "k_key_lookup_plain");
    for (uint32_t i = 0; i < ll.n_cols; i++)
        if (rows[i]) k_key_lookup_plain<<<(uint32_t)((rows[i] + TILE_ROWS - 1) / TILE_ROWS), WG, 0, ctx->stream>>>(ll, i, values[i], validity[i]);
}

}  // namespace sb
