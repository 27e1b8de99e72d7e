// strawboat-hip: sb_filter_columns_in — IN / NOT IN lists evaluated on the pages (included by sb_decode.hip behind
// sb_filter_bin.h; every kernel here ends in the sink of sb_filter.h: filter_span / sel_put).
//
// The host hands every column its literals as a sorted set without duplicates (InCol, sb_common.h): numbers as order keys
// (in_key: -0.0 and +0.0 share a key, NaN literals are left out), binary literals in byte-string order.  A row is in the
// list when a binary search finds its key; NOT IN negates that, and the sink ANDs either with the row's validity, so a
// null row satisfies neither.  The kernels are those of sb_filter.h / sb_filter_bin.h with the compare replaced by the
// search, beside them and not inside them: no kernel of a comparison call is touched.
//   numbers   k_filter_in        None / LZ4 / Zstd / Snappy / Patas / bit-packed: one search per row; OneValue: per tile;
//                                Dict: per entry into the LDS bit table (<= FILTER_DICT_BITS entries), else per row on the
//                                gathered entry; Freq: asks for the replay (KIND_REPLAY | KIND_FILTER_FREQ)
//             k_filter_in_rle    rle_page_walk with RleFilterIn: one search per run into the predicate bytes
//             k_filter_in_plain  the Freq replay: the column decoded into the staging area, one search per row
//   The column's keys are staged into LDS (n * 8 bytes, at most 8 KiB) and searched there: branch-free, with the trip
//   count of the column, ceil(log2(n + 1)), so every lane of a wave issues the same number of LDS loads.
//   binary    k_filter_in_bin_entries   one search per entry of Dict / Freq pages into the page's bit table (bin_dict)
//             k_filter_in_bin           Dict / Freq: a bit per row; OneValue: one search per tile; basic: one per row
//   The search is over the literals themselves with the order of bin_rel_prefix; the literals are followed by 8 zero bytes,
//   so the first word of each is one load that stays inside the set (the rule at the head of sb_filter_bin.h).
#pragma once

namespace sb {

// ---- numbers
struct InEval {
    const uint64_t* keys;   // LDS
    uint32_t n, steps, negate, kind, w;
};
// true when x is one of the n ascending keys: `steps` probes, whatever x is
__device__ __forceinline__ bool in_member(const uint64_t* keys, uint32_t n, uint32_t steps, uint64_t x) {
    uint32_t pos = 0;   // keys below x
    for (uint32_t s = steps; s-- > 0;) {
        const uint32_t p = pos + (1u << s);
        const uint64_t k = keys[min(p, n) - 1];   // (steps > 0: n >= 1, and p >= 1)
        pos = (p <= n && k < x) ? p : pos;
    }
    return n != 0 && pos < n && keys[min(pos, n - 1)] == x;
}
__device__ __forceinline__ bool in_eval(const InEval& k, uint64_t raw) {
    return in_member(k.keys, k.n, k.steps, in_key(k.kind, k.w, raw)) != (k.negate != 0);
}
// the column's keys into LDS, by the whole workgroup; the caller's barrier follows
__device__ __forceinline__ void in_stage(const InCol& ic, uint64_t* s_keys) {
    const uint32_t n = min(ic.n, IN_MAX_VALUES);
    for (uint32_t i = threadIdx.x; i < n; i += WG) s_keys[i] = ic.keys[i];
}
__device__ __forceinline__ InEval in_eval_of(const FilterCol& f, const InCol& ic, const uint64_t* s_keys, uint32_t w) {
    return InEval{s_keys, min(ic.n, IN_MAX_VALUES), ic.steps, ic.negate, f.kind, w};
}

// the tiles k_filter has: filter_tile with the search in the compare's place.  `staged` is the column whose keys s_keys holds.
__device__ void filter_in_tile(const DecodeArgs& a, const FilterCol* fcols, const InCol* icols, uint32_t ti, uint32_t* s_a, uint32_t* s_w,
                               uint32_t* s_tab, uint64_t* s_keys, uint32_t* staged) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    if (!d.ok) return;
    if (is_binary(c.ptype)) return;   // (k_filter_in_bin)
    const FilterCol f = fcols[tt.col];
    const InCol ic = icols[tt.col];
    if (*staged != tt.col) {   // (the same for every lane: the tile's column)
        in_stage(ic, s_keys);
        *staged = tt.col;
        __syncthreads();
    }
    const uint32_t w = c.width;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    const FilterSink k{f.sel, d.def_bits, t.out_row, t.num_values, f.combine};
    const InEval ev = in_eval_of(f, ic, s_keys, w);
    switch (d.codec) {
        case SB_CODEC_NONE: {
            const uint8_t* src = d.src;
            filter_span(k, lo, hi, [&](uint64_t r) { return in_eval(ev, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {   // inflated into the staging area
            const uint8_t* src = c.values + t.out_row * w;
            filter_span(k, lo, hi, [&](uint64_t r) { return in_eval(ev, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_FREQ:   // the replay puts the rows (k_filter_in_plain)
            if (threadIdx.x == 0 && tt.tile == 0) atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
            break;
        case SB_CODEC_ONEVALUE: {
            const bool v = in_eval(ev, flt_load(d.body, w));
            filter_span(k, lo, hi, [&](uint64_t) { return v; });
            break;
        }
        case SB_CODEC_DICT: {
            U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
            u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
            const uint8_t* dict = d.dict;
            const uint32_t D = d.dict_n;
            bool bad;
            if (D <= FILTER_DICT_BITS) {
                for (uint32_t e0 = 0; e0 < D; e0 += WG) {
                    const uint32_t e = e0 + threadIdx.x;
                    const uint64_t m = __ballot(e < D && in_eval(ev, flt_load(dict + (uint64_t)e * w, w)));
                    if ((threadIdx.x & 31) == 0 && e < D) s_tab[e >> 5] = ballot_half(m);
                }
                __syncthreads();
                bad = filter_dict_rows(k, lo, hi, s_a, D, [&](uint32_t e) { return tab_bit(s_tab, e); });
            } else {
                bad = filter_dict_rows(k, lo, hi, s_a, D, [&](uint32_t e) { return in_eval(ev, flt_load(dict + (uint64_t)e * w, w)); });
            }
            if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 400);
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            if (w != 4) break;
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            u32_tile_to_lds(vs, tt.tile, rows, s_a, s_w);
            filter_span(k, lo, hi, [&](uint64_t r) { return in_eval(ev, s_a[sidx((int)(r - lo))]); });
            break;
        }
        default:   // (RLE pages of <= 8-byte values have no tiles: k_filter_in_rle)
            break;
    }
}

// 26 KB of LDS: k_filter's 18 KB and the keys (8 KB); 160 KB per CU hold 6 such workgroups
__global__ void __launch_bounds__(WG) k_filter_in(DecodeArgs a, const FilterCol* fcols, const InCol* icols) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_tab[FILTER_DICT_BITS / 32];
    __shared__ uint64_t s_keys[IN_MAX_VALUES];
    const uint32_t count = a.job_counts[2];
    uint32_t staged = 0xFFFFFFFFu;
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        filter_in_tile(a, fcols, icols, ti, s_a, s_w, s_tab, s_keys, &staged);
        __syncthreads();
    }
}

// ---- RLE pages: RleFilter with the search per run
struct RleFilterIn {
    using Rec = uint8_t;
    uint8_t* s_rec;
    FilterSink k;
    InEval ev;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + ev.w; }
    __device__ __forceinline__ uint8_t load(const uint8_t* v, bool in) const { return in && in_eval(ev, flt_load(v, ev.w)); }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        filter_span(k, lo, hi, [&](uint64_t r) { return s_rec[A + s_flag[sidx((int)(r - tile_lo))]] != 0; });
    }
};

__global__ void __launch_bounds__(WG) k_filter_in_rle(DecodeArgs a, const FilterCol* fcols, const InCol* icols) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint8_t s_pred[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_keys[IN_MAX_VALUES];
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    const FilterCol f = fcols[t.col];
    const InCol ic = icols[t.col];
    in_stage(ic, s_keys);
    __syncthreads();   // (the walk's first loads search the keys)
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    const RleFilterIn pol{s_pred, FilterSink{f.sel, d.def_bits, t.out_row, t.num_values, f.combine}, in_eval_of(f, ic, s_keys, c.width)};
    rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
}

// ---- the replay of a call that met a Freq page: k_filter_plain with the search
__global__ void __launch_bounds__(WG) k_filter_in_plain(FilterCol f, InCol ic, const uint8_t* values, const uint8_t* validity, uint64_t rows, uint32_t w) {
    __shared__ uint64_t s_keys[IN_MAX_VALUES];
    in_stage(ic, s_keys);
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * TILE_ROWS, hi = min(rows, lo + TILE_ROWS);
    const FilterSink k{f.sel, validity, 0, rows, f.combine};
    const InEval ev = in_eval_of(f, ic, s_keys, w);
    filter_span(k, lo, hi, [&](uint64_t r) { return in_eval(ev, flt_load(values + r * w, w)); });
}

// ---- binary columns
// the value's place among the literals: a binary search with the three-way order of bin_eval
__device__ __forceinline__ bool in_bin_eval(const InCol& ic, const uint8_t* v, uint32_t len) {
    uint32_t lo = 0, hi = min(ic.n, IN_MAX_VALUES);
    bool found = false;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        const uint64_t o0 = ic.keys[mid], o1 = ic.keys[mid + 1];
        const uint8_t* p = ic.bytes + o0;
        const BinLit l{p, ldu64(p), (uint32_t)(o1 - o0), 0u};
        uint32_t r = bin_rel_prefix(v, l, min(len, l.len));
        if (r == 1u) r = len < l.len ? 0u : len == l.len ? 1u : 2u;
        if (r == 1u) {
            found = true;
            break;
        }
        if (r == 0u) hi = mid;
        else lo = mid + 1;
    }
    return found != (ic.negate != 0);
}

// grid (pages, FILTER_BIN_EY): k_filter_bin_entries with the search
__global__ void __launch_bounds__(WG) k_filter_in_bin_entries(DecodeArgs a, const FilterCol* fcols, const InCol* icols) {
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    if (!d.ok || (d.codec != SB_CODEC_DICT && d.codec != SB_CODEC_FREQ)) return;
    const PageTask t = a.tasks[p];
    if (!is_binary(a.cols[t.col].ptype)) return;
    if (fcols[t.col].kind != FK_BYTES) return;
    BinDict bd;
    if (!bin_dict(a, t, d, &bd)) {
        if (threadIdx.x == 0 && blockIdx.y == 0) raise(a.status, SB_ERR_INVALID, p, 220);
        return;
    }
    const InCol ic = icols[t.col];
    for (uint32_t e0 = blockIdx.y * WG; e0 < bd.D; e0 += gridDim.y * WG) {
        const uint32_t e = e0 + threadIdx.x;
        bool b = false;
        if (e < bd.D) {
            const uint64_t pr = ldu64((const uint8_t*)(bd.ent_off + e));
            const uint32_t eo = (uint32_t)pr;
            const uint32_t len = (uint32_t)(pr >> 32) - eo - 8 - (e == 0 ? bd.gap : 0);
            b = in_bin_eval(ic, d.dict + eo + 8, len);
        }
        const uint64_t m = __ballot(b);
        if ((threadIdx.x & 31) == 0 && e < bd.D) gst32(bd.bits + (e >> 5), ballot_half(m));
    }
}

template <class O>
__device__ __forceinline__ void filter_in_bin_basic(const FilterSink& k, uint64_t lo, uint64_t hi, const uint8_t* offs, const uint8_t* vals,
                                                    uint32_t vsize, const InCol& ic) {
    filter_span(k, lo, hi, [&](uint64_t r) {
        uint64_t o0, o1;
        if constexpr (sizeof(O) == 4) {
            const uint64_t pr = ldu64(offs + r * 4);
            o0 = (uint32_t)pr;
            o1 = pr >> 32;
        } else {
            o0 = ldu64(offs + r * 8);
            o1 = ldu64(offs + r * 8 + 8);
        }
        // offsets that leave the values block are cut to it, as filter_bin_basic cuts them: nothing outside is loaded
        o1 = min(o1, (uint64_t)vsize);
        o0 = min(o0, o1);
        return in_bin_eval(ic, vals + o0, (uint32_t)(o1 - o0));
    });
}
__device__ void filter_in_bin_tile(const DecodeArgs& a, const FilterCol* fcols, const InCol* icols, uint32_t ti, uint32_t* s_a, uint32_t* s_w,
                                   uint32_t* s_tab) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    if (!is_binary(c.ptype)) return;   // (k_filter_in)
    const FilterCol f = fcols[tt.col];
    if (f.kind != FK_BYTES) return;
    const InCol ic = icols[tt.col];
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    const FilterSink k{f.sel, d.def_bits, t.out_row, t.num_values, f.combine};
    if (is_basic(d.codec)) {
        const uint8_t* vals = d.codec == SB_CODEC_NONE ? d.vbody : c.values + d.val_base;
        if (c.ptype == SB_TYPE_BINARY) filter_in_bin_basic<int32_t>(k, lo, hi, d.src, vals, d.vusize, ic);
        else filter_in_bin_basic<int64_t>(k, lo, hi, d.src, vals, d.vusize, ic);
    } else if (d.codec == SB_CODEC_ONEVALUE) {
        const bool v = in_bin_eval(ic, d.dict, d.dict_n);
        filter_span(k, lo, hi, [&](uint64_t) { return v; });
    } else if (d.codec == SB_CODEC_DICT || d.codec == SB_CODEC_FREQ) {
        BinDict bd;
        if (!bin_dict(a, t, d, &bd)) return;   // (raised by k_filter_in_bin_entries)
        U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
        u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
        const uint32_t D = bd.D;
        bool bad;
        if (D <= FILTER_DICT_BITS) {
            for (uint32_t g = threadIdx.x; g < (D + 31) / 32; g += WG) s_tab[g] = gld32(bd.bits + g);
            __syncthreads();
            bad = filter_dict_rows(k, lo, hi, s_a, D, [&](uint32_t e) { return tab_bit(s_tab, e); });
        } else {
            const uint32_t* bits = bd.bits;
            bad = filter_dict_rows(k, lo, hi, s_a, D, [&](uint32_t e) { return ((gld32(bits + (e >> 5)) >> (e & 31)) & 1u) != 0; });
        }
        if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 222);
    }
}

// 18 KB of LDS like k_filter_bin
__global__ void __launch_bounds__(WG) k_filter_in_bin(DecodeArgs a, const FilterCol* fcols, const InCol* icols) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_tab[FILTER_DICT_BITS / 32];
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        filter_in_bin_tile(a, fcols, icols, ti, s_a, s_w, s_tab);
        __syncthreads();
    }
}

// The end of an IN call, in launch_filter's place: the clear and the count are the comparison call's own kernels
void launch_filter_in(sb_ctx* ctx, const DecodeArgs& a, const FilterLaunch& fl, const InCol* icols) {
    hipStream_t s = ctx->stream;
    const FilterCol* fcols = fl.fcols;
    if (fl.any_set) {
        KScope k(ctx, "k_filter_clear");
        k_filter_clear<<<dim3(a.n_cols, 16), WG, 0, s>>>(a.cols, fcols);
    }
    if (fl.any_cmp) {
        KScope k(ctx, "k_filter_in_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_filter_in_rle<<<dim3(a.n_pages, std::max<uint32_t>(1u, a.rle_parts)), WG, 0, s>>>(a, fcols, icols);
    }
    if (fl.any_cmp && a.n_tiles) {
        KScope k(ctx, "k_filter_in");
        k_filter_in<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, fcols, icols);
    }
    if (fl.any_bin) {
        KScope k(ctx, "k_filter_in_bin_entries");
        k_filter_in_bin_entries<<<dim3(a.n_pages, FILTER_BIN_EY), WG, 0, s>>>(a, fcols, icols);
    }
    if (fl.any_bin && a.n_tiles) {
        KScope k(ctx, "k_filter_in_bin");
        k_filter_in_bin<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, fcols, icols);
    }
    KScope k(ctx, "k_filter_count");
    k_filter_count<<<a.n_cols, WG, 0, s>>>(a.cols, fcols, fl.counts);
}

void launch_filter_in_plain(sb_ctx* ctx, const FilterCol& f, const InCol& ic, const uint8_t* values, const uint8_t* validity, uint64_t rows,
                            uint32_t w, uint64_t* count) {
    hipStream_t s = ctx->stream;
    if (rows) k_filter_in_plain<<<(uint32_t)((rows + TILE_ROWS - 1) / TILE_ROWS), WG, 0, s>>>(f, ic, values, validity, rows, w);
    k_filter_count_one<<<1, WG, 0, s>>>(f.sel, rows, count);
}

}  // namespace sb
