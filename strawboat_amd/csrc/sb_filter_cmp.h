// strawboat-hip: sb_filter_columns_cmp — the pages of a column compared row by row with a second, dense column (included
// by sb_decode.hip behind sb_filter.h; every kernel here ends in the sink of sb_filter.h: filter_span / sel_put).
//
// `WHERE a < b`: y comes from the pages, the operand of row r of the column is other[r] (CmpCol, sb_common.h), a value of
// a type of its own with an optional validity bit.  The kernels are those of sb_filter.h over the same parse / inflate /
// plan chain and the same tile list, beside them and not inside them: no kernel of a literal call is touched.  What
// differs is that nothing can be decided once per run or per dictionary entry any more -- every row has its own operand:
//   None / LZ4 / Zstd / Snappy / Patas   one load of y (the page, or the staging area the queues inflated into), one of
//                                        the operand, compared in registers
//   OneValue                             y is a register for the tile, one load of the operand per row
//   RLE                                  rle_page_walk with RleFilterCmp: the chunk's run VALUES in LDS (no predicate
//                                        bytes), every row gathers its run's value
//   Dict                                 the row's entry is gathered from the dictionary, whatever its size (no LDS bit
//                                        table); an index beyond the dictionary raises where a read raises
//   Bitpacking / Delta                   unpacked into LDS by u32_tile_to_lds, compared from there
//   Freq                                 left alone: the interval is issued again (KIND_REPLAY | KIND_FILTER_FREQ) with this
//                                        call decoded into the staging area and compared by k_filter_cmp_plain
// The comparison is cmp_rel (sb_common.h): the relation of y to the operand picks a bit of the op's mask, as flt_eval has
// it.  The type pair is a template argument of the span: cmp_pair resolves it once per tile / chunk / launch, outside
// the loop over rows.  The operand loads are the coalesced stream of these kernels; they are issued inside filter_span's
// predicate, that is with the y loads of its U rows per lane and before the first ballot.  A null row of y is masked by
// the sink as ever; an invalid operand masks its row in the predicate.  Nothing of `other` is written.
#pragma once

namespace sb {

struct CmpEval {
    const uint8_t* other;
    const uint32_t* ov;
    uint32_t mask, ykind, yw, okind, ow;
};
__device__ __forceinline__ CmpEval cmp_eval_of(const FilterCol& f, const CmpCol& cc, uint32_t yw) {
    return CmpEval{cc.other, cc.ov, f.mask, f.kind, yw, cc.okind, cc.ow};
}

// Rows [lo, hi) of a page by the whole workgroup: y_of(row, y) gives the row's value, or false for a row that has none (a
// Dict index beyond the dictionary: the caller raises).  Row `row` of the page is row k.out_row + row of the column, which
// is where its operand and its validity bit are: both lie below the column's rows, the capacities the entry point checked.
template <class Y>
__device__ __forceinline__ void cmp_span(const FilterSink& k, const CmpEval& ev, uint64_t lo, uint64_t hi, Y y_of) {
    cmp_pair(ev.ykind, ev.okind, [&](auto yk, auto ok) __attribute__((always_inline)) {
        constexpr uint32_t YK = decltype(yk)::value, OK = decltype(ok)::value;
        filter_span(k, lo, hi, [&](uint64_t r) __attribute__((always_inline)) {
            uint64_t y;
            if (!y_of(r, y)) return false;
            const uint64_t c = k.out_row + r;
            const uint64_t o = flt_load(ev.other + c * ev.ow, ev.ow);
            bool b = (ev.mask >> cmp_rel<YK, OK>(ev.yw, y, ev.ow, o)) & 1u;
            if (ev.ov) b = b && ((gld32(ev.ov + (c >> 5)) >> (uint32_t)(c & 31)) & 1u);
            return b;
        });
    });
}

// ---- tiles of None / OneValue / Dict / bit-packed / inflated pages: filter_tile's switch with cmp_span as the sink
__device__ __forceinline__ void filter_cmp_tile(const DecodeArgs& a, const FilterCol* fcols, const CmpCol* ccols, uint32_t ti, uint32_t* s_a, uint32_t* s_w) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    if (!d.ok) return;
    if (is_binary(c.ptype)) return;   // (refused at the call)
    const FilterCol f = fcols[tt.col];
    const uint32_t w = c.width;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    const FilterSink k{f.sel, d.def_bits, t.out_row, t.num_values, f.combine};
    const CmpEval ev = cmp_eval_of(f, ccols[tt.col], w);
    // (this function and the unpacking below are inlined by force: a kernel of sixty-four spans is past the inliner's size,
    // and a call would keep `a` or the stream it is handed in scratch memory)
    switch (d.codec) {
        case SB_CODEC_NONE:
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {   // the page itself, or the staging area, where a read call has the column's values
            const uint8_t* src = d.codec == SB_CODEC_NONE ? d.src : c.values + t.out_row * w;
            cmp_span(k, ev, lo, hi, [&](uint64_t r, uint64_t& y) { return y = flt_load(src + r * w, w), true; });
            break;
        }
        case SB_CODEC_FREQ:   // SET: the rows stay cleared; AND / OR: untouched.  The replay puts them (see the head of the file)
            if (threadIdx.x == 0 && tt.tile == 0) atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
            break;
        case SB_CODEC_ONEVALUE: {
            const uint64_t one = flt_load(d.body, w);
            cmp_span(k, ev, lo, hi, [&](uint64_t, uint64_t& y) { return y = one, true; });
            break;
        }
        case SB_CODEC_DICT: {
            U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
            [[clang::always_inline]] u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
            const uint8_t* dict = d.dict;
            const uint32_t D = d.dict_n;
            bool bad = false;
            cmp_span(k, ev, lo, hi, [&](uint64_t r, uint64_t& y) {
                const uint32_t e = s_a[sidx((int)(r - lo))];
                if (e >= D) {
                    bad = true;
                    return false;
                }
                y = flt_load(dict + (uint64_t)e * w, w);
                return true;
            });
            if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 400);
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            if (w != 4) break;
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            [[clang::always_inline]] u32_tile_to_lds(vs, tt.tile, rows, s_a, s_w);
            cmp_span(k, ev, lo, hi, [&](uint64_t r, uint64_t& y) { return y = (uint64_t)s_a[sidx((int)(r - lo))], true; });
            break;
        }
        default:   // (RLE pages of <= 8-byte values have no tiles: k_filter_cmp_rle)
            break;
    }
}

// 17 KB of LDS like k_expand (no Dict bit table): 8 workgroups per CU
__global__ void __launch_bounds__(WG) k_filter_cmp(DecodeArgs a, const FilterCol* fcols, const CmpCol* ccols) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        filter_cmp_tile(a, fcols, ccols, ti, s_a, s_w);
        __syncthreads();
    }
}

// ---- RLE pages: rle_page_walk with this policy.  A run is its value (RleWeighted's staging); rows gather their run's
// value and meet their own operand.  The rows of a chunk start and end anywhere in a selection word, as for RleFilter.
struct RleFilterCmp {
    using Rec = uint64_t;
    uint64_t* s_rec;
    FilterSink k;
    CmpEval ev;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + ev.yw; }
    __device__ __forceinline__ uint64_t load(const uint8_t* v, bool in) const { return in ? flt_load(v, ev.yw) : 0ull; }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        cmp_span(k, ev, lo, hi, [&](uint64_t r, uint64_t& y) { return y = s_rec[A + s_flag[sidx((int)(r - tile_lo))]], true; });
    }
};

// 25 KB of LDS: the flags and the chunk's run values
__global__ void __launch_bounds__(WG) k_filter_cmp_rle(DecodeArgs a, const FilterCol* fcols, const CmpCol* ccols) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint64_t s_vals[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    const FilterCol f = fcols[t.col];
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    const RleFilterCmp pol{s_vals, FilterSink{f.sel, d.def_bits, t.out_row, t.num_values, f.combine}, cmp_eval_of(f, ccols[t.col], c.width)};
    // (the walk with sixteen spans in it is past the inliner's size: left as a call, `pol` would live in scratch memory)
    [[clang::always_inline]] rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
}

// ---- the replay of a call that met a Freq page: k_filter_plain with the operand
__global__ void __launch_bounds__(WG) k_filter_cmp_plain(FilterCol f, CmpCol cc, const uint8_t* values, const uint8_t* validity, uint64_t rows, uint32_t w) {
    const uint64_t lo = (uint64_t)blockIdx.x * TILE_ROWS, hi = min(rows, lo + TILE_ROWS);
    const FilterSink k{f.sel, validity, 0, rows, f.combine};
    cmp_span(k, cmp_eval_of(f, cc, w), lo, hi, [&](uint64_t r, uint64_t& y) { return y = flt_load(values + r * w, w), true; });
}

// The end of a column-against-column call, in launch_filter's place: the clear and the count are the literal call's own kernels
void launch_filter_cmp(sb_ctx* ctx, const DecodeArgs& a, const FilterLaunch& fl, const CmpCol* ccols) {
    hipStream_t s = ctx->stream;
    const FilterCol* fcols = fl.fcols;
    if (fl.any_set) {
        KScope k(ctx, "k_filter_clear");
        k_filter_clear<<<dim3(a.n_cols, 16), WG, 0, s>>>(a.cols, fcols);
    }
    {
        KScope k(ctx, "k_filter_cmp_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_filter_cmp_rle<<<dim3(a.n_pages, std::max<uint32_t>(1u, a.rle_parts)), WG, 0, s>>>(a, fcols, ccols);
    }
    if (a.n_tiles) {
        KScope k(ctx, "k_filter_cmp");
        k_filter_cmp<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, fcols, ccols);
    }
    KScope k(ctx, "k_filter_count");
    k_filter_count<<<a.n_cols, WG, 0, s>>>(a.cols, fcols, fl.counts);
}

void launch_filter_cmp_plain(sb_ctx* ctx, const FilterCol& f, const CmpCol& cc, const uint8_t* values, const uint8_t* validity, uint64_t rows,
                             uint32_t w, uint64_t* count) {
    hipStream_t s = ctx->stream;
    if (rows) k_filter_cmp_plain<<<(uint32_t)((rows + TILE_ROWS - 1) / TILE_ROWS), WG, 0, s>>>(f, cc, values, validity, rows, w);
    k_filter_count_one<<<1, WG, 0, s>>>(f.sel, rows, count);
}

}  // namespace sb
