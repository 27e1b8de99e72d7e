// strawboat-hip: sb_aggregate_columns — the reducing sink on the decoder's walks (included by sb_decode.hip behind
// sb_read_sel.h).
//
// A read call stores every row, a filter call a bit per row, a selected read the rows whose bit is set; this call stores
// nothing per row: count / min / max / sum of the rows whose selection bit is set and that are not null come back as a few
// dozen bytes per column.  The chain is a read call up to k_plan (same tables, k_parse, inflate queues, plan), then
//   k_agg_null               columns without MIN / MAX / SUM, of every type: popcount of selection & def levels, per page
//   k_agg_rle / k_agg        the walks of k_expand_rle / k_expand with agg_span as the sink (below)
//   k_agg_finish             one workgroup per column: the bits set below `rows`, and the column's partial records combined
//   k_agg_plain              the replay of a call that met a Freq page: the column decoded like a read into the staging
//                            area, reduced from there
// No rank table, no cleared output, no capacity: a lane's bit is selection(row) & valid(row), and a lane that has it adds
// its row to accumulators it keeps in registers for the whole tile (the whole page part in the RLE walk).  The workgroup
// reduces ONCE per tile — shuffles across the wave, LDS across the four waves — and writes one partial record into the
// tile's own slot.  Nothing is accumulated with atomics: the slots are combined in slot order, so the order of the double
// additions of a float sum is fixed by the launch shape and the same call gives the same bits every time.  That holds for
// an interval that is issued again too: a column without a Freq page stays on the page route there, and a column with one
// takes the decoded route in every interval it is part of (agg_tile marks it, the host goes by the mark).
#pragma once

namespace sb {

// A lane's accumulators.  kmin / kmax are order keys (agg_key), so one unsigned min / max serves every type; integers are
// summed as 128-bit two's-complement numbers (s1 carries), floats in double (its bits in s0).
struct AggAcc {
    uint64_t cnt = 0, nans = 0, kmin = ~0ull, kmax = 0, s0 = 0, s1 = 0;
};
__device__ __forceinline__ bool agg_is_float(uint32_t kind) { return kind == FK_F32 || kind == FK_F64; }
__device__ __forceinline__ double agg_dbl(uint64_t b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ uint64_t agg_bits(double v) { return (uint64_t)__double_as_longlong(v); }
__device__ __forceinline__ uint64_t agg_sext(uint64_t raw, uint32_t w) {
    const uint32_t sh = 64 - 8 * w;
    return (uint64_t)((int64_t)(raw << sh) >> sh);
}
// The order of FilterCmp (unsigned, signed, numeric) as an unsigned key; floats in the total order -inf < ... < -0.0 <
// +0.0 < ... < +inf (NaNs never get here), so the key gives the value's bits back (agg_unkey).
__device__ __forceinline__ uint64_t agg_key(uint32_t kind, uint32_t w, uint64_t raw) {
    if (kind == FK_UNSIGNED) return raw;
    if (kind == FK_SIGNED) return agg_sext(raw, w) ^ (1ull << 63);
    if (kind == FK_F32) {
        const uint32_t b = (uint32_t)raw;
        return (b >> 31) ? (uint32_t)~b : (b | 0x80000000u);
    }
    return (raw >> 63) ? ~raw : (raw | (1ull << 63));
}
__device__ __forceinline__ uint64_t agg_unkey(uint32_t kind, uint32_t w, uint64_t key) {
    if (kind == FK_UNSIGNED) return key;
    if (kind == FK_SIGNED) return (key ^ (1ull << 63)) & (w == 8 ? ~0ull : (1ull << (8 * w)) - 1);
    if (kind == FK_F32) {
        const uint32_t k = (uint32_t)key;
        return (k >> 31) ? (k & 0x7FFFFFFFu) : (uint32_t)~k;
    }
    return (key >> 63) ? (key & ~(1ull << 63)) : ~key;
}
// one live row
__device__ __forceinline__ void agg_add(AggAcc& a, uint32_t kind, uint32_t w, uint64_t raw) {
    a.cnt++;
    if (agg_is_float(kind)) {
        const double v = kind == FK_F32 ? (double)__uint_as_float((uint32_t)raw) : agg_dbl(raw);
        a.s0 = agg_bits(agg_dbl(a.s0) + v);
        if (v != v) {
            a.nans++;
            return;
        }
    } else {
        const uint64_t v = kind == FK_SIGNED ? agg_sext(raw, w) : raw;
        a.s0 += v;
        a.s1 += (a.s0 < v ? 1ull : 0ull) + (kind == FK_SIGNED ? (uint64_t)((int64_t)v >> 63) : 0ull);
    }
    const uint64_t k = agg_key(kind, w, raw);
    a.kmin = min(a.kmin, k);
    a.kmax = max(a.kmax, k);
}
// n > 0 live rows of one value (OneValue pages): the product instead of n additions
__device__ __forceinline__ void agg_add_n(AggAcc& a, uint32_t kind, uint32_t w, uint64_t raw, uint64_t n) {
    a.cnt += n;
    if (agg_is_float(kind)) {
        const double v = kind == FK_F32 ? (double)__uint_as_float((uint32_t)raw) : agg_dbl(raw);
        a.s0 = agg_bits(agg_dbl(a.s0) + v * (double)n);
        if (v != v) {
            a.nans += n;
            return;
        }
    } else if (kind == FK_SIGNED) {
        const int64_t v = (int64_t)agg_sext(raw, w);
        const uint64_t lo = (uint64_t)v * n;
        a.s0 += lo;
        a.s1 += (uint64_t)__mul64hi((long long)v, (long long)n) + (a.s0 < lo ? 1ull : 0ull);
    } else {
        const uint64_t lo = raw * n;
        a.s0 += lo;
        a.s1 += __umul64hi(raw, n) + (a.s0 < lo ? 1ull : 0ull);
    }
    const uint64_t k = agg_key(kind, w, raw);
    a.kmin = min(a.kmin, k);
    a.kmax = max(a.kmax, k);
}
// a + b, in this order (a float sum depends on it)
__device__ __forceinline__ AggAcc agg_merge(const AggAcc& a, const AggAcc& b, bool flt) {
    AggAcc r;
    r.cnt = a.cnt + b.cnt;
    r.nans = a.nans + b.nans;
    r.kmin = min(a.kmin, b.kmin);
    r.kmax = max(a.kmax, b.kmax);
    if (flt) {
        r.s0 = agg_bits(agg_dbl(a.s0) + agg_dbl(b.s0));
        r.s1 = 0;
    } else {
        r.s0 = a.s0 + b.s0;
        r.s1 = a.s1 + b.s1 + (r.s0 < a.s0 ? 1ull : 0ull);
    }
    return r;
}
// The workgroup's accumulators as one, in thread 0: a shuffle tree per wave, then waves 0..3 in order through s_red
// (AGG_RED_WORDS words; the caller keeps a barrier between two uses).
constexpr uint32_t AGG_RED_WORDS = 4 * 6;
__device__ __forceinline__ AggAcc agg_wg_reduce(AggAcc a, bool flt, uint64_t* s_red) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        AggAcc b;
        b.cnt = __shfl_down(a.cnt, d, 64);
        b.nans = __shfl_down(a.nans, d, 64);
        b.kmin = __shfl_down(a.kmin, d, 64);
        b.kmax = __shfl_down(a.kmax, d, 64);
        b.s0 = __shfl_down(a.s0, d, 64);
        b.s1 = __shfl_down(a.s1, d, 64);
        a = agg_merge(a, b, flt);
    }
    if ((threadIdx.x & 63) == 0) {
        uint64_t* r = s_red + (threadIdx.x >> 6) * 6;
        r[0] = a.cnt, r[1] = a.nans, r[2] = a.kmin, r[3] = a.kmax, r[4] = a.s0, r[5] = a.s1;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t wv = 1; wv < WG / 64; wv++) {
            const uint64_t* r = s_red + wv * 6;
            AggAcc b;
            b.cnt = r[0], b.nans = r[1], b.kmin = r[2], b.kmax = r[3], b.s0 = r[4], b.s1 = r[5];
            a = agg_merge(a, b, flt);
        }
    return a;
}
__device__ __forceinline__ void agg_store(AggPart* p, const AggAcc& a) {
    p->live = 1;
    p->cnt = a.cnt;
    p->nans = a.nans;
    p->kmin = a.kmin;
    p->kmax = a.kmax;
    p->s0 = a.s0;
    p->s1 = a.s1;
    p->pad = 0;
}

struct AggSink {
    const uint32_t* sel;       // the column's selection words or null: every row
    const uint8_t* def_bits;   // the page's validity bits (bit 0 = row 0 of the page) or null: every row valid
    uint64_t out_row;          // the page's first row in the column
};
// Rows [lo, hi) of a page, live(row) by every lane whose row is selected and not null, by the whole workgroup: a lane per
// row.  No barrier, no ballot: a lane without its bit moves on to its next row.
template <class F>
__device__ __forceinline__ void agg_rows(const AggSink& k, uint64_t lo, uint64_t hi, F live) {
    for (uint64_t r = lo + threadIdx.x; r < hi; r += WG) {
        const uint64_t c = k.out_row + r;
        bool on = true;
        if (k.sel) on = (gld32(k.sel + (c >> 5)) >> (uint32_t)(c & 31)) & 1u;
        if (on && k.def_bits) on = (ldu8(k.def_bits + (r >> 3)) >> (uint32_t)(r & 7)) & 1u;
        if (on) live(r);
    }
}
// the reducing counterpart of filter_span / sel_span: value_of(row) of every live row into the lane's accumulators
template <class V>
__device__ __forceinline__ void agg_span(const AggSink& k, AggAcc& acc, uint32_t kind, uint32_t w, uint64_t lo, uint64_t hi, V value_of) {
    agg_rows(k, lo, hi, [&](uint64_t r) { agg_add(acc, kind, w, value_of(r)); });
}
// Is a bit set among rows [c0, c1) of the column, c1 - c0 <= TILE_ROWS?  From the <= 129 selection words alone, a word
// per lane, by the whole workgroup (a barrier inside).
__device__ __forceinline__ bool agg_any_selected(const uint32_t* sel, uint64_t c0, uint64_t c1) {
    static_assert(TILE_ROWS / 32 + 1 <= WG, "a selection word per lane");
    if (!sel) return true;
    const uint64_t w0 = c0 >> 5, w1 = (c1 - 1) >> 5, g = w0 + threadIdx.x;
    uint32_t v = 0;
    if (g <= w1) {
        v = gld32(sel + g);
        if (g == w0) v &= 0xFFFFFFFFu << (uint32_t)(c0 & 31);
        if (g == w1 && (c1 & 31)) v &= (1u << (uint32_t)(c1 & 31)) - 1;
    }
    return __syncthreads_or(v != 0) != 0;
}

// ---- tiles of None / OneValue / Dict / bit-packed / inflated pages (the pages k_expand, k_filter and k_rsel have tiles for)
__device__ void agg_tile(const DecodeArgs& a, const AggLaunch& al, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint64_t* s_red) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    const AggCol g = al.acols[tt.col];
    if (!(g.ops & AGG_VALUE_OPS)) return;   // (k_agg_null)
    const uint32_t w = c.width, kind = g.kind;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    // A Freq page asks for the replay whatever the selection, as in filter_tile and rsel_tile: k_parse has logged the page
    // for the second decode pass, and only the replay drops that record (see the head of sb_filter.h).  It marks its column
    // (the slot of its first tile, which holds no record: k_agg_finish hands the mark to the host): the replay takes the
    // decoded route for the marked columns alone, so the route of a column -- and with it the order of its float additions --
    // is a matter of the column's own pages, not of what else the interval holds.  A marked column is not issued on this
    // route again; if one is, the call fails instead of leaving the page out.
    if (d.codec == SB_CODEC_FREQ) {
        if (threadIdx.x == 0 && tt.tile == 0) {
            gst64(&al.parts[al.tile_base + t.first_tile].live, AGG_PART_FREQ);
            if (al.replayed) raise(a.status, SB_ERR_NYI, tt.page, 411);
            else atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
        }
        return;
    }
    // a tile without a selected row: no value and no index is loaded, and its slot stays empty
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) return;
    const AggSink k{g.sel, d.def_bits, t.out_row};
    AggAcc acc;
    switch (d.codec) {
        case SB_CODEC_NONE: {
            const uint8_t* src = d.src;
            agg_span(k, acc, kind, w, lo, hi, [&](uint64_t r) { return flt_load(src + r * w, w); });
            break;
        }
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {   // inflated into the staging area, where a read call has the column's values
            const uint8_t* src = c.values + t.out_row * w;
            agg_span(k, acc, kind, w, lo, hi, [&](uint64_t r) { return flt_load(src + r * w, w); });
            break;
        }
        case SB_CODEC_ONEVALUE: {   // the value times the lane's live rows: no load per row
            uint64_t n = 0;
            agg_rows(k, lo, hi, [&](uint64_t) { n++; });
            if (n) agg_add_n(acc, kind, w, flt_load(d.body, w), n);
            break;
        }
        case SB_CODEC_DICT: {
            U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
            u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
            const uint8_t* dict = d.dict;
            const uint32_t D = d.dict_n;
            bool bad = false;
            agg_rows(k, lo, hi, [&](uint64_t r) {   // the row's entry is gathered, as the decoder gathers it
                const uint32_t e = s_a[sidx((int)(r - lo))];
                if (e >= D) {
                    bad = true;
                    return;
                }
                agg_add(acc, kind, w, flt_load(dict + (uint64_t)e * w, w));
            });
            if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 400);
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            if (w != 4) break;
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            u32_tile_to_lds(vs, tt.tile, rows, s_a, s_w);
            agg_span(k, acc, kind, w, lo, hi, [&](uint64_t r) { return (uint64_t)s_a[sidx((int)(r - lo))]; });
            break;
        }
        default:   // (RLE pages of <= 8-byte values have no tiles: k_agg_rle)
            return;
    }
    acc = agg_wg_reduce(acc, agg_is_float(kind), s_red);
    if (threadIdx.x == 0) agg_store(al.parts + al.tile_base + t.first_tile + tt.tile, acc);
}

// 17 KB of LDS (k_expand's, and 192 bytes for the reduction): 8 workgroups per CU like k_expand
__global__ void __launch_bounds__(WG) k_agg(DecodeArgs a, AggLaunch al) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_red[AGG_RED_WORDS];
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        agg_tile(a, al, ti, s_a, s_w, s_red);
        __syncthreads();
    }
}

// ---- RLE pages, one workgroup per page (or per part of a long page): rle_page_walk (sb_decode.hip) with this policy.
// The chunk's run values are staged in LDS as 64-bit words like RleSelect's; live rows gather their run's value.  The
// lanes keep their accumulators across the chunks and tiles of the whole page part: one reduction, one record.
struct RleAggregate {
    using Rec = uint64_t;
    uint64_t* s_rec;
    AggSink k;
    AggAcc* acc;
    uint32_t kind, w;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + w; }
    __device__ __forceinline__ uint64_t load(const uint8_t* v, bool in) const { return in ? flt_load(v, w) : 0ull; }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        agg_span(k, *acc, kind, w, lo, hi, [&](uint64_t r) { return s_rec[A + s_flag[sidx((int)(r - tile_lo))]]; });
    }
};

__global__ void __launch_bounds__(WG) k_agg_rle(DecodeArgs a, AggLaunch al) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint64_t s_vals[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_red[AGG_RED_WORDS];
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    const AggCol g = al.acols[t.col];
    if (!(g.ops & AGG_VALUE_OPS)) return;
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    AggAcc acc;
    const RleAggregate pol{s_vals, AggSink{g.sel, d.def_bits, t.out_row}, &acc, g.kind, c.width};
    rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
    __syncthreads();
    acc = agg_wg_reduce(acc, agg_is_float(g.kind), s_red);
    if (threadIdx.x == 0) agg_store(al.parts + (uint64_t)p * parts + part, acc);
}

// ---- columns without MIN / MAX / SUM, of every physical type: the live rows of a page are the set bits of its def-level
// section (parse_def_levels, as k_filter_null reads it) under the selection; no page body is looked at
__device__ __forceinline__ uint32_t agg_sel_bits32(const uint32_t* sel, uint64_t pos, uint64_t col_rows) {
    const uint64_t i = pos >> 5;
    const uint32_t sh = (uint32_t)(pos & 31);
    uint32_t v = gld32(sel + i) >> sh;
    if (sh && i + 1 < (col_rows + 31) / 32) v |= gld32(sel + i + 1) << (32 - sh);
    return v;
}
__global__ void __launch_bounds__(WG) k_agg_null(DecodeArgs a, AggLaunch al, uint32_t parts) {
    __shared__ uint64_t s_w64[4];
    const uint32_t p = blockIdx.x;
    const PageTask t = a.tasks[p];
    const AggCol g = al.acols[t.col];
    if (g.ops & AGG_VALUE_OPS) return;
    const ColDesc c = a.cols[t.col];
    const uint64_t N = t.num_values;
    if (!N) return;
    const uint8_t* def = nullptr;
    if (g.ptype != SB_TYPE_NULL && c.nullable) {
        DefLevels dl{nullptr, nullptr, SB_ERR_IO, 1};   // (site 1 is k_parse's as well: the page lies in the column's bytes)
        if (t.in_off + t.length <= c.pages_len) dl = parse_def_levels(c.pages + t.in_off, c.pages + t.in_off + t.length, N);
        if (dl.code) {
            if (threadIdx.x == 0) raise(a.status, dl.code, p, dl.site);
            return;
        }
        def = dl.bits;
    }
    const uint32_t none = g.ptype == SB_TYPE_NULL ? 0u : 0xFFFFFFFFu;   // validity of a page without a def-level section
    const uint64_t nwords = (N + 31) / 32;
    uint64_t n = 0;
    for (uint64_t i = threadIdx.x; i < nwords; i += WG) {
        uint32_t v = def ? tile_bits_load(def, i * 32, N) : none;
        const uint64_t left = N - i * 32;
        if (left < 32) v &= (1u << (uint32_t)left) - 1;
        if (v && g.sel) v &= agg_sel_bits32(g.sel, t.out_row + i * 32, g.rows);
        n += (uint64_t)__popc(v);
    }
    n = wg_sum64(n, s_w64);
    if (threadIdx.x == 0) {
        AggAcc acc;
        acc.cnt = n;
        agg_store(al.parts + (uint64_t)p * parts, acc);
    }
}

// ---- one workgroup per column: `selected` (the bits set below `rows`: delivered whatever became of the pages) and the
// column's partial records — page slots, then tile slots, a thread taking every WG-th — as its result record
__global__ void __launch_bounds__(WG) k_agg_finish(const AggCol* acols, const AggPart* parts, uint64_t* results) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_red[AGG_RED_WORDS];
    const AggCol g = acols[blockIdx.x];
    const bool flt = agg_is_float(g.kind);
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
    AggAcc acc;
    bool freq = false;   // a Freq page's mark among the tile slots (agg_tile)
    auto take = [&](const AggPart& p) {
        if (!p.live) return;
        if (p.live == AGG_PART_FREQ) {
            freq = true;
            return;
        }
        AggAcc b;
        b.cnt = p.cnt, b.nans = p.nans, b.kmin = p.kmin, b.kmax = p.kmax, b.s0 = p.s0, b.s1 = p.s1;
        acc = agg_merge(acc, b, flt);
    };
    for (uint64_t i = threadIdx.x; i < g.page_slots; i += WG) take(parts[g.page_slot0 + i]);
    for (uint64_t i = threadIdx.x; i < g.tile_slots; i += WG) take(parts[g.tile_slot0 + i]);
    acc = agg_wg_reduce(acc, flt, s_red);
    freq = __syncthreads_or(freq) != 0;
    if (threadIdx.x == 0) {
        uint64_t* r = results + (uint64_t)blockIdx.x * AGG_RESULT_WORDS;
        const bool any = acc.cnt > acc.nans && (g.ops & AGG_VALUE_OPS);
        r[0] = nsel;
        r[1] = acc.cnt;
        r[2] = acc.nans;
        r[3] = any && (g.ops & 2u) ? agg_unkey(g.kind, g.w, acc.kmin) : 0;
        r[4] = any && (g.ops & 4u) ? agg_unkey(g.kind, g.w, acc.kmax) : 0;
        r[5] = (g.ops & 8u) ? acc.s0 : 0;
        r[6] = (g.ops & 8u) ? acc.s1 : 0;
        r[7] = freq ? 1 : 0;   // for the host's replay (replay_interval)
    }
}

// ---- the replay of a call that met a Freq page: the column was decoded like a read (values and validity in the staging
// area, exceptions scattered by the second pass); one launch per column, a workgroup and a slot per TILE_ROWS rows
__global__ void __launch_bounds__(WG) k_agg_plain(const AggCol* acols, uint32_t col, AggPart* parts, const uint8_t* values, const uint8_t* validity) {
    __shared__ uint64_t s_red[AGG_RED_WORDS];
    const AggCol g = acols[col];
    const uint64_t lo = (uint64_t)blockIdx.x * TILE_ROWS, hi = min(g.rows, lo + TILE_ROWS);
    AggAcc acc;
    if (agg_any_selected(g.sel, lo, hi)) {
        const uint32_t w = g.w;
        agg_span(AggSink{g.sel, validity, 0}, acc, g.kind, w, lo, hi, [&](uint64_t r) { return flt_load(values + r * w, w); });
    }
    acc = agg_wg_reduce(acc, agg_is_float(g.kind), s_red);
    if (threadIdx.x == 0) agg_store(parts + g.tile_slot0 + blockIdx.x, acc);
}

void launch_agg(sb_ctx* ctx, const DecodeArgs& a, const AggLaunch& al) {
    hipStream_t s = ctx->stream;
    const uint32_t parts = std::max<uint32_t>(1u, a.rle_parts);
    if (al.any_null) {
        KScope k(ctx, "k_agg_null");
        k_agg_null<<<a.n_pages, WG, 0, s>>>(a, al, parts);
    }
    if (al.any_val) {
        KScope k(ctx, "k_agg_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_agg_rle<<<dim3(a.n_pages, parts), WG, 0, s>>>(a, al);
    }
    if (al.any_val && a.n_tiles) {
        KScope k(ctx, "k_agg");
        k_agg<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, al);
    }
}

void launch_agg_finish(sb_ctx* ctx, const AggCol* acols, const AggPart* parts, uint64_t* results, uint32_t n_cols) {
    KScope k(ctx, "k_agg_finish");
    k_agg_finish<<<n_cols, WG, 0, ctx->stream>>>(acols, parts, results);
}

// `rows[i]`, `values[i]`, `validity[i]` (host arrays): the decoded columns of the replay
void launch_agg_plain(sb_ctx* ctx, const AggCol* acols, uint32_t n_cols, AggPart* parts, const uint64_t* rows, const uint8_t* const* values,
                      const uint8_t* const* validity) {
    KScope k(ctx, "k_agg_plain");
    for (uint32_t i = 0; i < n_cols; i++)
        if (rows[i]) k_agg_plain<<<(uint32_t)((rows[i] + TILE_ROWS - 1) / TILE_ROWS), WG, 0, ctx->stream>>>(acols, i, parts, values[i], validity[i]);
}

}  // namespace sb
