// strawboat-hip: sb_filter_columns — the value sink of a filter call and its kernels (included by sb_decode.hip behind
// the expand kernels, whose page walk they share).
//
// A filter call runs k_parse, the inflate queues and k_plan exactly as a read call does; where the read call launches
// k_expand_rle / k_expand, it launches k_filter_rle / k_filter: the same walk over runs, indices and tiles, but every
// value is compared with the column's literal and the outcome of 32 rows goes into a word of the selection bitmap.
//   None                     one load per row, compared in registers
//   OneValue                 one compare per tile
//   RLE                      one compare per run: the chunk's runs become predicate BYTES in LDS, rows gather those
//   Dict                     one compare per entry into an LDS bit table (<= FILTER_DICT_BITS entries), rows look bits up;
//                            longer dictionaries: the row's entry is gathered and compared, as the decoder gathers it
//   Bitpacking / Delta       unpacked into LDS by u32_tile_to_lds as for a read, compared from there
//   LZ4 / Zstd / Snappy / Patas   inflated by the queues into the call's staging area (ColDesc.values), compared from there
//   Freq                     the exceptions are a block of their own that a second decode pass expands at the synchronize:
//                            the page is left alone here and the interval is issued again (KIND_REPLAY | KIND_FILTER_FREQ)
//                            with this call decoded into the staging area and compared by k_filter_plain
// k_filter_null serves IS_NULL / IS_NOT_NULL from the def-level section alone; k_filter_count counts the bits at the end.
// Comparison columns of a binary type (sb_filter_columns_var) share the sink and have kernels of their own: sb_filter_bin.h.
#pragma once

namespace sb {

constexpr uint32_t FILTER_DICT_BITS = 8192;   // entries of the LDS bit table (1 KiB): at most two compares per row of a full
                                              // tile, read coalesced; beyond that a gather per row is less work

struct FilterCmp {
    uint64_t lit;
    uint32_t kind, mask, w;
};
__device__ __forceinline__ FilterCmp filter_cmp(const FilterCol& f, uint32_t w) { return FilterCmp{f.lit, f.kind, f.mask, w}; }
__device__ __forceinline__ uint64_t flt_load(const uint8_t* p, uint32_t w) {
    switch (w) {
        case 1:
            return ldu8(p);
        case 2:
            return ldu16(p);
        case 4:
            return ldu32(p);
        default:
            return ldu64(p);
    }
}
// the relation of the value to the literal (0 less, 1 equal, 2 greater, 3 unordered) picks a bit of the predicate's mask
__device__ __forceinline__ bool flt_eval(const FilterCmp& k, uint64_t raw) {
    uint32_t rel;
    if (k.kind == FK_UNSIGNED) {
        rel = raw < k.lit ? 0u : raw == k.lit ? 1u : 2u;
    } else if (k.kind == FK_SIGNED) {
        const uint32_t sh = 64 - 8 * k.w;
        const int64_t v = (int64_t)(raw << sh) >> sh, l = (int64_t)k.lit;
        rel = v < l ? 0u : v == l ? 1u : 2u;
    } else {
        const double v = k.kind == FK_F32 ? (double)__uint_as_float((uint32_t)raw) : __longlong_as_double((long long)raw);
        const double l = __longlong_as_double((long long)k.lit);
        rel = v < l ? 0u : v == l ? 1u : v > l ? 2u : 3u;
    }
    return (k.mask >> rel) & 1u;
}

// `b` are the result bits of the positions `m` of one selection word.  A word whose 32 positions come from one put is
// owned by the lane that puts it: plain accesses.  A word shared by puts (page seams, chunk seams of an RLE page, the
// column's last word) is touched with atomics only: OR into the word the call cleared (SET) or that holds the earlier
// selection (OR), AND with the positions outside `m` set (AND).
__device__ __forceinline__ void sel_word(uint32_t* w, uint32_t m, uint32_t b, uint32_t combine) {
    if (m == 0xFFFFFFFFu) {
        if (combine == SB_SEL_SET) gst32(w, b);
        else if (combine == SB_SEL_AND) gst32(w, gld32(w) & b);
        else gst32(w, gld32(w) | b);
    } else if (combine == SB_SEL_AND) {
        if (~b & m) atomicAnd(w, b | ~m);
    } else if (b) {
        atomicOr(w, b);
    }
}
// the result of rows [pos, pos + nbits) of the column, nbits <= 32
__device__ __forceinline__ void sel_put(uint32_t* sel, uint64_t pos, uint32_t bits, uint32_t nbits, uint32_t combine) {
    const uint32_t m = nbits < 32 ? (1u << nbits) - 1 : 0xFFFFFFFFu;
    bits &= m;
    uint32_t* w = sel + (pos >> 5);
    const uint32_t sh = (uint32_t)(pos & 31);
    sel_word(w, m << sh, bits << sh, combine);
    if (sh && (m >> (32 - sh))) sel_word(w + 1, m >> (32 - sh), bits >> (32 - sh), combine);
}

struct FilterSink {
    uint32_t* sel;
    const uint8_t* def_bits;   // the page's validity bits (bit 0 = row 0 of the page) or null
    uint64_t out_row;          // the page's first row in the column
    uint64_t N;                // rows of the page
    uint32_t combine;
};
// Rows [lo, hi) of a page, pred(row) per row, by the whole workgroup: a lane per row, a ballot per wave, and the two
// 32-row halves of the ballot — ANDed with the rows' validity: a null row satisfies nothing — put by lanes 0 and 32.
// The halves start at multiples of 32 rows OF THE PAGE, so that the validity bits are a byte-aligned load.
template <class P>
__device__ __forceinline__ void filter_span(const FilterSink& k, uint64_t lo, uint64_t hi, P pred) {
    constexpr int U = 4;   // rows per lane whose loads are issued before the first ballot
    const uint32_t tid = threadIdx.x;
    for (uint64_t g0 = lo & ~31ull; g0 < hi; g0 += (uint64_t)U * WG) {
        bool bit[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t row = g0 + (uint64_t)u * WG + tid;
            bit[u] = row >= lo && row < hi && pred(row);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint64_t row = g0 + (uint64_t)u * WG + tid;
            const uint64_t m = __ballot(bit[u]);
            if ((tid & 31) == 0 && row < hi && row + 32 > lo) {
                uint32_t half = ballot_half(m);
                if (k.def_bits) half &= tile_bits_load(k.def_bits, row, k.N);
                const uint64_t glo = max(row, lo), ghi = min(row + 32, hi);
                sel_put(k.sel, k.out_row + glo, half >> (uint32_t)(glo - row), (uint32_t)(ghi - glo), k.combine);
            }
        }
    }
}

// Rows [lo, hi) of a tile whose dictionary indices are in s_a (u32_tile_to_lds): a row whose index e is below D satisfies
// what look(e) says — a bit of a table (tab_bit) or the compare of the gathered entry — and a row whose index is not
// satisfies nothing.  True when there was such a row: the caller raises it at the site where a read finds it.
__device__ __forceinline__ bool tab_bit(const uint32_t* tab, uint32_t e) { return (tab[e >> 5] >> (e & 31)) & 1u; }
template <class L>
__device__ __forceinline__ bool filter_dict_rows(const FilterSink& k, uint64_t lo, uint64_t hi, const uint32_t* s_a, uint32_t D, L look) {
    bool bad = false;
    filter_span(k, lo, hi, [&](uint64_t r) {
        const uint32_t e = s_a[sidx((int)(r - lo))];
        if (e >= D) {
            bad = true;
            return false;
        }
        return look(e);
    });
    return bad;
}

// ---- tiles of None / OneValue / Dict / bit-packed / inflated pages (the pages k_expand has tiles for)
__device__ void filter_tile(const DecodeArgs& a, const FilterCol* fcols, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint32_t* s_tab) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    if (!d.ok) return;
    if (is_binary(c.ptype)) return;   // (k_filter_bin)
    const FilterCol f = fcols[tt.col];
    if (f.op >= SB_PRED_IS_NULL) return;   // (k_filter_null)
    const uint32_t w = c.width;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    const FilterSink k{f.sel, d.def_bits, t.out_row, t.num_values, f.combine};
    const FilterCmp cmp = filter_cmp(f, w);
    switch (d.codec) {
        case SB_CODEC_NONE: {
            const uint8_t* src = d.src;
            filter_span(k, lo, hi, [&](uint64_t r) { return flt_eval(cmp, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {   // inflated into the staging area, where a read call has the column's values
            const uint8_t* src = c.values + t.out_row * w;
            filter_span(k, lo, hi, [&](uint64_t r) { return flt_eval(cmp, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_FREQ:   // SET: the rows stay cleared; AND / OR: untouched.  The replay puts them (see the head of the file)
            if (threadIdx.x == 0 && tt.tile == 0) atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
            break;
        case SB_CODEC_ONEVALUE: {
            const bool v = flt_eval(cmp, flt_load(d.body, w));
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
                    const uint64_t m = __ballot(e < D && flt_eval(cmp, flt_load(dict + (uint64_t)e * w, w)));
                    if ((threadIdx.x & 31) == 0 && e < D) s_tab[e >> 5] = ballot_half(m);
                }
                __syncthreads();
                bad = filter_dict_rows(k, lo, hi, s_a, D, [&](uint32_t e) { return tab_bit(s_tab, e); });
            } else {   // the row's entry is gathered and compared, as the decoder gathers it
                bad = filter_dict_rows(k, lo, hi, s_a, D, [&](uint32_t e) { return flt_eval(cmp, flt_load(dict + (uint64_t)e * w, w)); });
            }
            if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 400);
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            if (w != 4) break;
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            u32_tile_to_lds(vs, tt.tile, rows, s_a, s_w);
            filter_span(k, lo, hi, [&](uint64_t r) { return flt_eval(cmp, s_a[sidx((int)(r - lo))]); });
            break;
        }
        default:   // (RLE pages of <= 8-byte values have no tiles: k_filter_rle)
            break;
    }
}

// 18 KB of LDS (k_expand's 17 KB and the Dict bit table): 8 workgroups per CU like k_expand
__global__ void __launch_bounds__(WG) k_filter(DecodeArgs a, const FilterCol* fcols) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_tab[FILTER_DICT_BITS / 32];
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        filter_tile(a, fcols, ti, s_a, s_w, s_tab);
        __syncthreads();
    }
}

// ---- RLE pages, one workgroup per page (or per part of a long page): rle_page_walk (sb_decode.hip) with this policy.
// A run is one predicate BYTE, its value compared once; rows gather their run's byte.  The rows of a chunk start and end
// anywhere in a selection word, which filter_span and sel_put allow for.
struct RleFilter {
    using Rec = uint8_t;
    uint8_t* s_rec;
    FilterSink k;
    FilterCmp cmp;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + cmp.w; }
    __device__ __forceinline__ uint8_t load(const uint8_t* v, bool in) const { return in && flt_eval(cmp, flt_load(v, cmp.w)); }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        filter_span(k, lo, hi, [&](uint64_t r) { return s_rec[A + s_flag[sidx((int)(r - tile_lo))]] != 0; });
    }
};

__global__ void __launch_bounds__(WG) k_filter_rle(DecodeArgs a, const FilterCol* fcols) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint8_t s_pred[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    const FilterCol f = fcols[t.col];
    if (f.op >= SB_PRED_IS_NULL) return;
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    const RleFilter pol{s_pred, FilterSink{f.sel, d.def_bits, t.out_row, t.num_values, f.combine}, filter_cmp(f, c.width)};
    rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
}

// ---- IS_NULL / IS_NOT_NULL: the def-level section of every page of such a column (u32 def_len | ULEB128 | bits,
// parse_def_levels, which k_parse reads it with as well), one workgroup per page
__global__ void __launch_bounds__(WG) k_filter_null(DecodeArgs a, const FilterCol* fcols) {
    const uint32_t p = blockIdx.x;
    const PageTask t = a.tasks[p];
    const FilterCol f = fcols[t.col];
    if (f.op < SB_PRED_IS_NULL) return;
    const ColDesc c = a.cols[t.col];
    const uint64_t N = t.num_values;
    if (!N) return;
    const uint8_t* def = nullptr;
    if (f.ptype != SB_TYPE_NULL && c.nullable) {
        DefLevels dl{nullptr, nullptr, SB_ERR_IO, 1};   // (site 1 is k_parse's as well: the page lies in the column's bytes)
        if (t.in_off + t.length <= c.pages_len) dl = parse_def_levels(c.pages + t.in_off, c.pages + t.in_off + t.length, N);
        if (dl.code) {
            if (threadIdx.x == 0) raise(a.status, dl.code, p, dl.site);
            return;
        }
        def = dl.bits;
    }
    const uint32_t none = f.ptype == SB_TYPE_NULL ? 0u : 0xFFFFFFFFu;   // validity of a page without a def-level section
    const uint64_t nwords = (N + 31) / 32;
    for (uint64_t g = threadIdx.x; g < nwords; g += WG) {
        uint32_t v = def ? tile_bits_load(def, g * 32, N) : none;
        if (f.op == SB_PRED_IS_NULL) v = ~v;
        sel_put(f.sel, t.out_row + g * 32, v, (uint32_t)min((uint64_t)32, N - g * 32), f.combine);
    }
}

// ---- bits set below `rows`, one workgroup per column
__device__ void filter_count(const uint32_t* sel, uint64_t rows, uint64_t* out, uint64_t* s_w64) {
    const uint64_t nwords = (rows + 31) / 32;
    uint64_t n = 0;
    for (uint64_t g = threadIdx.x; g < nwords; g += WG) {
        uint32_t v = gld32(sel + g);
        if (g == nwords - 1 && (rows & 31)) v &= (1u << (rows & 31)) - 1;
        n += (uint64_t)__popc(v);
    }
    n = wg_sum64(n, s_w64);
    if (threadIdx.x == 0) *out = n;
}
__global__ void __launch_bounds__(WG) k_filter_count(const ColDesc* cols, const FilterCol* fcols, uint64_t* counts) {
    __shared__ uint64_t s_w64[4];
    filter_count(fcols[blockIdx.x].sel, cols[blockIdx.x].rows, counts + blockIdx.x, s_w64);
}

// ---- the replay of a call that met a Freq page: the column was decoded like a read (values and validity in the staging
// area, exceptions scattered by the second pass); one launch per column, a workgroup per TILE_ROWS rows, then the count
__global__ void __launch_bounds__(WG) k_filter_plain(FilterCol f, const uint8_t* values, const uint8_t* validity, uint64_t rows, uint32_t w) {
    const uint64_t lo = (uint64_t)blockIdx.x * TILE_ROWS, hi = min(rows, lo + TILE_ROWS);
    const FilterSink k{f.sel, validity, 0, rows, f.combine};
    const FilterCmp cmp = filter_cmp(f, w);
    filter_span(k, lo, hi, [&](uint64_t r) { return flt_eval(cmp, flt_load(values + r * w, w)); });
}
__global__ void __launch_bounds__(WG) k_filter_count_one(const uint32_t* sel, uint64_t rows, uint64_t* out) {
    __shared__ uint64_t s_w64[4];
    filter_count(sel, rows, out, s_w64);
}

// SET columns start from zero: shared words are assembled with OR, and the bits behind the last row are written as 0
// (one launch for the call's columns: a memset per column costs a 64-column call more than its kernels)
__global__ void __launch_bounds__(WG) k_filter_clear(const ColDesc* cols, const FilterCol* fcols) {
    const FilterCol f = fcols[blockIdx.x];
    if (f.combine != SB_SEL_SET) return;
    const uint64_t nwords = (cols[blockIdx.x].rows + 31) / 32;
    for (uint64_t g = (uint64_t)blockIdx.y * WG + threadIdx.x; g < nwords; g += (uint64_t)gridDim.y * WG) gst32(f.sel + g, 0u);
}

void launch_filter_bin(sb_ctx* ctx, const DecodeArgs& a, const FilterCol* fcols);   // sb_filter_bin.h
void launch_filter_sub_entries(sb_ctx* ctx, const DecodeArgs& a, const FilterCol* fcols);   // sb_filter_sub.h
void launch_filter_sub(sb_ctx* ctx, const DecodeArgs& a, const FilterCol* fcols);
void launch_filter(sb_ctx* ctx, const DecodeArgs& a, const FilterLaunch& fl) {
    hipStream_t s = ctx->stream;
    const FilterCol* fcols = fl.fcols;
    const bool any_cmp = fl.any_cmp, any_null = fl.any_null, any_set = fl.any_set;
    uint64_t* counts = fl.counts;
    if (any_set) {
        KScope k(ctx, "k_filter_clear");
        k_filter_clear<<<dim3(a.n_cols, 16), WG, 0, s>>>(a.cols, fcols);
    }
    if (any_null) {
        KScope k(ctx, "k_filter_null");
        k_filter_null<<<a.n_pages, WG, 0, s>>>(a, fcols);
    }
    if (any_cmp) {
        KScope k(ctx, "k_filter_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_filter_rle<<<dim3(a.n_pages, std::max<uint32_t>(1u, a.rle_parts)), WG, 0, s>>>(a, fcols);
    }
    if (any_cmp && a.n_tiles) {
        KScope k(ctx, "k_filter");
        k_filter<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, fcols);
    }
    if (fl.any_sub) launch_filter_sub_entries(ctx, a, fcols);   // (the bit tables k_filter_bin reads)
    if (fl.any_bin) launch_filter_bin(ctx, a, fcols);
    if (fl.any_sub) launch_filter_sub(ctx, a, fcols);
    KScope k(ctx, "k_filter_count");
    k_filter_count<<<a.n_cols, WG, 0, s>>>(a.cols, fcols, counts);
}

void launch_filter_plain(sb_ctx* ctx, const FilterCol& f, const uint8_t* values, const uint8_t* validity, uint64_t rows, uint32_t w,
                         uint64_t* count) {
    hipStream_t s = ctx->stream;
    if (rows) k_filter_plain<<<(uint32_t)((rows + TILE_ROWS - 1) / TILE_ROWS), WG, 0, s>>>(f, values, validity, rows, w);
    k_filter_count_one<<<1, WG, 0, s>>>(f.sel, rows, count);
}

}  // namespace sb
