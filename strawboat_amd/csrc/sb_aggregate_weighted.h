// strawboat-hip: sb_aggregate_weighted — sum(y * w) per group: the grouping sink of sb_aggregate_grouped_large with a second
// dense per-row input beside the ids, a weight (included by sb_decode.hip behind sb_aggregate_grouped_large.h, whose slots,
// flags, records, chunk rule and page walks it uses).
//
// The chain is k_grpl's with a sibling per kernel:
//   k_wgt_null     columns without SUM, of every physical type: selection, def levels, ids and weight validity, per page
//   k_wgt_rle      rle_page_walk with wgt_span as the sink: one table and one slot per (page, part)
//   k_wgt          a CHUNK of GRPL_CHUNK_TILES tiles of the column per workgroup, found from blockIdx as k_grpl finds it
//   k_wgt_plain    the replay of a column that met a Freq page, from the decoded column: a table per 16 * TILE_ROWS rows
//   k_wgt_finish   grid (columns, ceil(gmax / 256)): k_grpl_finish without min / max, float or not by the pair of types
// What is new is the sink, wgt_span: grp_span's selected / id / def-bit steps, then the weight's validity bit and the weight
// itself at the row's place in the column, then the product:
//   integer x integer   wgt_mul128, the exact low 128 bits, added with integer LDS atomics: the low word with a returning
//                       add, whose old value tells the carry; the carry and the product's high word go to the high field
//   otherwise           (double)y * (double)w, rounded once (no fused multiply-add), added by grp_span's scheme: a fixed
//                       shuffle tree for the first GRP_TREE_IDS ids of a wave's step, rank rounds in lane order for the
//                       rest, into the wave's own row; the four rows in wave order at the store
// Determinism of the float sums: DESIGN 4k's argument word for word.  Which rows share a table and in which order they meet
// it is a function of the column's own page layout; within a table the additions are a function of the rows' ids, selection
// and liveness (the weights' validity included); k_wgt_finish adds the slots in slot order.  No float atomic anywhere.
// The table has no kmin / kmax: 7 fields x 1024 groups x 8 bytes = 56 KB, at one stride (GRPL_MAX_GROUPS) for every n_groups.
#pragma once

namespace sb {

constexpr uint32_t WF_SEL = 0, WF_CNT = 1, WF_NANS = 2, WF_SUM = 3;   // the table: field f of group g at s_g[f * GRPL_MAX_GROUPS + g]
constexpr uint32_t WGT_FIELDS = WF_SUM + WG / 64;                      // fields 3..: the two words of an integer sum, or the four waves' rows
constexpr uint32_t WGT_LDS_WORDS = WGT_FIELDS * GRPL_MAX_GROUPS;       // 56 KB

__device__ __forceinline__ uint64_t* wgt_field(uint64_t* s_g, uint32_t f) { return s_g + f * GRPL_MAX_GROUPS; }

// by the whole workgroup, followed by a barrier
__device__ __forceinline__ void wgt_table_clear(uint64_t* s_g, uint32_t G) {
    for (uint32_t i = threadIdx.x; i < G; i += WG) {
#pragma unroll
        for (uint32_t f = 0; f < WGT_FIELDS; f++) wgt_field(s_g, f)[i] = 0ull;
    }
    __syncthreads();
}

// a value of `kind` as the 64-bit word its own signedness extends it to / as a double (integers: round to nearest)
__device__ __forceinline__ uint64_t wgt_ext(uint32_t kind, uint32_t w, uint64_t raw) { return kind == FK_SIGNED ? agg_sext(raw, w) : raw; }
__device__ __forceinline__ double wgt_dbl(uint32_t kind, uint32_t w, uint64_t raw) {
    return kind == FK_F32 ? (double)__uint_as_float((uint32_t)raw) : kind == FK_F64 ? agg_dbl(raw) : kind == FK_SIGNED ? (double)(int64_t)agg_sext(raw, w) : (double)raw;
}

// Rows [lo, hi) of a page, by the whole workgroup, a lane per row and the same number of steps for every lane: grp_span
// with the weight.  k.ids null: every selected row is in group 0.  value_of(row, raw) gives y, or false for a row that has
// none (a Dict index beyond the dictionary: the caller raises).  Nothing of an unselected row is loaded but its selection
// bit; the weight of a row that is not live is not loaded either.
template <bool VAL, class V>
__device__ __forceinline__ void wgt_span(const GrpSink& k, const WgtCol& wc, uint64_t& oor, uint32_t kind, uint32_t w, uint64_t lo, uint64_t hi, V value_of) {
    const bool flt = VAL && wc.flt;
    uint64_t* const s_g = k.s_g;
    for (uint64_t base = lo; base < hi; base += WG) {
        const uint64_t r = base + threadIdx.x, c = k.out_row + r;
        bool on = r < hi;
        if (on && k.sel) on = (gld32(k.sel + (c >> 5)) >> (uint32_t)(c & 31)) & 1u;
        uint32_t id = 0;
        if (on) {   // (the id of an unselected row is never loaded)
            if (k.ids) id = grp_id(k.ids, k.idw, c);
            if (id >= k.G) {
                oor++;
                on = false;
            } else {
                grp_lds_add(wgt_field(s_g, WF_SEL) + id, 1);
            }
        }
        if (on && k.all_null) on = false;
        if (on && k.def_bits) on = (ldu8(k.def_bits + (r >> 3)) >> (uint32_t)(r & 7)) & 1u;
        if (on && wc.wv) on = (ldu8(wc.wv + (c >> 3)) >> (uint32_t)(c & 7)) & 1u;
        uint64_t raw = 0;
        if (VAL && on) on = value_of(r, raw);
        if (on) grp_lds_add(wgt_field(s_g, WF_CNT) + id, 1);
        if (!VAL) continue;
        uint64_t wraw = raw;   // (SB_WGT_SQUARE: wkind / ww are the column's own)
        if (on && wc.w) wraw = flt_load(wc.w + c * wc.ww, wc.ww);
        if (flt) {
            double v = 0.0;
            if (on) v = __dmul_rn(wgt_dbl(kind, w, raw), wgt_dbl(wc.wkind, wc.ww, wraw));
            // grp_span's float scheme applied to the product (the comments there): trees for the first ids, rank rounds
            // for the rest, into the wave's own row
            uint64_t* const row = wgt_field(s_g, WF_SUM + (threadIdx.x >> 6));
            const uint32_t lane = threadIdx.x & 63;
            uint64_t left = __ballot(on);
            for (uint32_t it = 0; left && it < GRP_TREE_IDS; it++) {
                const int lead = __ffsll((unsigned long long)left) - 1;
                const uint32_t gid = (uint32_t)__shfl((int)id, lead, 64);
                const bool mine = on && id == gid;
                double x = mine ? v : 0.0;
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
                if (lane == 0) {
                    l64p slot = (l64p)(row + gid);
                    *slot = agg_bits(agg_dbl(*slot) + x);
                }
                left &= ~__ballot(mine);
            }
            __builtin_amdgcn_wave_barrier();
            if (left) {
                const bool rem = on && ((left >> lane) & 1ull);
                uint32_t rank = 0, rounds = 0;
                while (left) {
                    const int lead = __ffsll((unsigned long long)left) - 1;
                    const uint32_t gid = (uint32_t)__shfl((int)id, lead, 64);
                    const bool mine = rem && id == gid;
                    const uint64_t b = __ballot(mine);
                    if (mine) rank = (uint32_t)__popcll(b & ((1ull << lane) - 1));
                    rounds = max(rounds, (uint32_t)__popcll(b));
                    left &= ~b;
                }
                for (uint32_t q = 0; q < rounds; q++) {
                    if (rem && rank == q) {
                        l64p slot = (l64p)(row + id);
                        *slot = agg_bits(agg_dbl(*slot) + v);
                    }
                    __builtin_amdgcn_wave_barrier();   // (keeps the rounds apart)
                }
            }
            if (on && v != v) grp_lds_add(wgt_field(s_g, WF_NANS) + id, 1);
        } else if (on) {   // the exact product into the 128-bit sum: the low word's old value tells the carry
            uint64_t plo, phi;
            wgt_mul128(wgt_ext(kind, w, raw), kind == FK_SIGNED, wgt_ext(wc.wkind, wc.ww, wraw), wc.wkind == FK_SIGNED, plo, phi);
            const uint64_t old = __hip_atomic_fetch_add((l64p)(wgt_field(s_g, WF_SUM) + id), plo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint64_t up = phi + (old + plo < plo ? 1ull : 0ull);
            if (up) grp_lds_add(wgt_field(s_g, WF_SUM + 1) + id, up);
        }
    }
}

// The table into the records of `slot` (grp_store without min / max), its flag set, and the workgroup's out-of-range rows
// added to the column's counter.  By the whole workgroup; barriers inside.
__device__ __forceinline__ void wgt_store(const GrpLaunch& gl, uint32_t col, uint64_t slot, uint32_t G, bool flt, uint64_t* s_g, uint64_t oor, uint64_t* s_w64) {
    __syncthreads();
    GrpPart* out = gl.recs + slot * gl.gmax;
    for (uint32_t g = threadIdx.x; g < G; g += WG) {
        GrpPart p;
        p.sel = wgt_field(s_g, WF_SEL)[g];
        p.cnt = wgt_field(s_g, WF_CNT)[g];
        p.nans = wgt_field(s_g, WF_NANS)[g];
        p.kmin = ~0ull;
        p.kmax = 0;
        if (flt) {   // the waves' rows, in wave order
            double s = agg_dbl(wgt_field(s_g, WF_SUM)[g]);
#pragma unroll
            for (uint32_t wv = 1; wv < WG / 64; wv++) s += agg_dbl(wgt_field(s_g, WF_SUM + wv)[g]);
            p.s0 = agg_bits(s);
            p.s1 = 0;
        } else {
            p.s0 = wgt_field(s_g, WF_SUM)[g];
            p.s1 = wgt_field(s_g, WF_SUM + 1)[g];
        }
        p.pad = 0;
        out[g] = p;
    }
    oor = wg_sum64(oor, s_w64);
    if (threadIdx.x == 0) {
        gst64(gl.flags + slot, 1);
        if (oor) atomicAdd((unsigned long long*)(gl.flags + gl.slots + col), (unsigned long long)oor);
    }
}

// Rows [lo, hi) of tile `tile` of page `page` into the table of `k`: grp_tile_rows' codec switch with wgt_span as the sink
__device__ __forceinline__ void wgt_tile_rows(const DecodeArgs& a, const PageDesc& d, const PageTask& t, const ColDesc& c, const GrpSink& k, const WgtCol& wc,
                                              uint64_t& oor, uint32_t kind, uint32_t page, uint32_t tile, uint64_t lo, uint64_t hi, uint32_t* s_a, uint32_t* s_w) {
    const uint32_t w = c.width, rows = (uint32_t)(hi - lo);
    switch (d.codec) {
        case SB_CODEC_NONE: {
            const uint8_t* src = d.src;
            wgt_span<true>(k, wc, oor, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = flt_load(src + r * w, w), true; });
            break;
        }
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {   // inflated into the staging area
            const uint8_t* src = c.values + t.out_row * w;
            wgt_span<true>(k, wc, oor, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = flt_load(src + r * w, w), true; });
            break;
        }
        case SB_CODEC_ONEVALUE: {
            const uint64_t one = flt_load(d.body, w);
            wgt_span<true>(k, wc, oor, kind, w, lo, hi, [&](uint64_t, uint64_t& raw) { return raw = one, true; });
            break;
        }
        case SB_CODEC_DICT: {
            U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
            u32_tile_to_lds(is, tile, rows, s_a, s_w);
            const uint8_t* dict = d.dict;
            const uint32_t D = d.dict_n;
            bool bad = false;
            wgt_span<true>(k, wc, oor, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) {
                const uint32_t e = s_a[sidx((int)(r - lo))];
                if (e >= D) {
                    bad = true;
                    return false;
                }
                raw = flt_load(dict + (uint64_t)e * w, w);
                return true;
            });
            if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, page, 420);
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            if (w != 4) break;
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            u32_tile_to_lds(vs, tile, rows, s_a, s_w);
            wgt_span<true>(k, wc, oor, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = (uint64_t)s_a[sidx((int)(r - lo))], true; });
            break;
        }
        default:   // (RLE pages of <= 8-byte values have no tiles: k_wgt_rle)
            break;
    }
}

// One tile of a chunk: grpl_tile's checks.  By the whole workgroup, every branch uniform.
__device__ __forceinline__ void wgt_tile(const DecodeArgs& a, const GrpLaunch& gl, uint32_t col, const ColDesc& c, const AggCol& g, const GrpCol& gc, const WgtCol& wc,
                                         uint32_t page, uint32_t tile, bool& live, uint64_t& oor, uint32_t* s_a, uint32_t* s_w, uint64_t* s_g) {
    const PageDesc d = a.descs[page];
    if (!d.ok) return;
    const PageTask t = a.tasks[page];
    const uint64_t lo = (uint64_t)tile * TILE_ROWS;
    if (lo >= t.num_values) return;
    const uint64_t hi = min(t.num_values, lo + TILE_ROWS);
    // a Freq page: the rule of grp_tile.  The column is marked and the replay asked for; the tile is passed over
    if (d.codec == SB_CODEC_FREQ) {
        if (threadIdx.x == 0 && tile == 0) {
            gst64(gl.flags + gl.slots + gl.n_cols + col, 1);
            if (gl.replayed) raise(a.status, SB_ERR_NYI, page, 421);
            else atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
        }
        return;
    }
    if (rle_by_page(c, d)) return;   // (k_wgt_rle)
    // a tile without a selected row: no value, no index, no id and no weight is loaded
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) return;
    if (!live) {
        wgt_table_clear(s_g, gc.n_groups);
        live = true;
    }
    const GrpSink k{g.sel, d.def_bits, t.out_row, gc.ids, gc.idw, gc.n_groups, s_g, false};
    wgt_tile_rows(a, d, t, c, k, wc, oor, g.kind, page, tile, lo, hi, s_a, s_w);
    __syncthreads();   // (s_a is filled again by the next tile)
}

// 73 KB of LDS (k_agg's 17 KB and the table): 2 workgroups per CU
__global__ void __launch_bounds__(WG) k_wgt(DecodeArgs a, WgtLaunch wl) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[WGT_LDS_WORDS];
    const GrpLaunch& gl = wl.gl;
    // the chunk's slot names its column (k_grpl)
    const uint64_t slot = gl.tile_base + blockIdx.x;
    uint32_t lo = 0, hi = gl.n_cols;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (gl.acols[mid].tile_slot0 <= slot) lo = mid;
        else hi = mid;
    }
    const uint32_t col = lo;
    const AggCol g = gl.acols[col];
    if (slot < g.tile_slot0 || slot - g.tile_slot0 >= g.tile_slots) return;
    if (!(g.ops & AGG_VALUE_OPS)) return;   // (k_wgt_null)
    const ColDesc c = a.cols[col];
    if (!c.n_pages) return;
    const GrpCol gc = gl.gcols[col];
    const WgtCol wc = wl.wcols[col];
    // the column's tiles, numbered through the call: [t0, t1)
    const PageTask last = a.tasks[c.first_page + c.n_pages - 1];
    const uint64_t t0 = a.tasks[c.first_page].first_tile;
    const uint64_t t1 = (uint64_t)last.first_tile + (last.num_values + TILE_ROWS - 1) / TILE_ROWS;
    const uint64_t j0 = (slot - g.tile_slot0) * GRPL_CHUNK_TILES;
    const uint64_t j1 = min(t1 - t0, j0 + GRPL_CHUNK_TILES);
    bool live = false;
    uint64_t oor = 0;
    for (uint64_t j = j0; j < j1; j++) {
        const uint32_t gt = (uint32_t)(t0 + j);
        const uint32_t page = grpl_page_of(a.tasks, c.first_page, c.n_pages, gt);
        wgt_tile(a, gl, col, c, g, gc, wc, page, gt - a.tasks[page].first_tile, live, oor, s_a, s_w, s_g);
    }
    // a chunk without a selected row stores nothing: its flag stays 0
    if (live) wgt_store(gl, col, slot, gc.n_groups, wc.flt, s_g, oor, s_w64);
}

// ---- RLE pages: rle_page_walk with this policy (RleGroupedLarge's staging of the run values)
struct RleWeighted {
    using Rec = uint64_t;
    uint64_t* s_rec;
    GrpSink k;
    WgtCol wc;
    uint64_t* oor;
    uint32_t kind, w;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + w; }
    __device__ __forceinline__ uint64_t load(const uint8_t* v, bool in) const { return in ? flt_load(v, w) : 0ull; }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        wgt_span<true>(k, wc, *oor, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = s_rec[A + s_flag[sidx((int)(r - tile_lo))]], true; });
    }
};

// 82 KB of LDS: 1 workgroup per CU
__global__ void __launch_bounds__(WG) k_wgt_rle(DecodeArgs a, WgtLaunch wl) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint64_t s_vals[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[WGT_LDS_WORDS];
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const GrpLaunch& gl = wl.gl;
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    const AggCol g = gl.acols[t.col];
    if (!(g.ops & AGG_VALUE_OPS)) return;
    const GrpCol gc = gl.gcols[t.col];
    const WgtCol wc = wl.wcols[t.col];
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    wgt_table_clear(s_g, gc.n_groups);
    uint64_t oor = 0;
    const RleWeighted pol{s_vals, GrpSink{g.sel, d.def_bits, t.out_row, gc.ids, gc.idw, gc.n_groups, s_g, false}, wc, &oor, g.kind, c.width};
    rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
    wgt_store(gl, t.col, (uint64_t)p * parts + part, gc.n_groups, wc.flt, s_g, oor, s_w64);
}

// ---- columns without SUM, of every physical type: k_grpl_null with the weights' validity
__global__ void __launch_bounds__(WG) k_wgt_null(DecodeArgs a, WgtLaunch wl, uint32_t parts) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[WGT_LDS_WORDS];
    const GrpLaunch& gl = wl.gl;
    const uint32_t p = blockIdx.x;
    const PageTask t = a.tasks[p];
    const AggCol g = gl.acols[t.col];
    if (g.ops & AGG_VALUE_OPS) return;
    const GrpCol gc = gl.gcols[t.col];
    const WgtCol wc = wl.wcols[t.col];
    const ColDesc c = a.cols[t.col];
    const uint64_t N = t.num_values;
    if (!N) return;
    const uint8_t* def = nullptr;
    if (g.ptype != SB_TYPE_NULL && c.nullable) {
        DefLevels dl{nullptr, nullptr, SB_ERR_IO, 1};
        if (t.in_off + t.length <= c.pages_len) dl = parse_def_levels(c.pages + t.in_off, c.pages + t.in_off + t.length, N);
        if (dl.code) {
            if (threadIdx.x == 0) raise(a.status, dl.code, p, dl.site);
            return;
        }
        def = dl.bits;
    }
    wgt_table_clear(s_g, gc.n_groups);
    uint64_t oor = 0;
    const GrpSink k{g.sel, def, t.out_row, gc.ids, gc.idw, gc.n_groups, s_g, g.ptype == SB_TYPE_NULL};
    wgt_span<false>(k, wc, oor, 0, 0, 0, N, [](uint64_t, uint64_t&) { return true; });
    wgt_store(gl, t.col, (uint64_t)p * parts, gc.n_groups, false, s_g, oor, s_w64);
}

// ---- grid (columns, ceil(gmax / GRPL_FINISH_GROUPS)): k_grpl_finish's stripes, without min / max; a column's sums are
// doubles if either of its operands is a float
__global__ void __launch_bounds__(WG) k_wgt_finish(const AggCol* acols, const GrpCol* gcols, const WgtCol* wcols, const uint64_t* flags, const GrpPart* recs,
                                                   uint64_t slots, uint32_t gmax, uint64_t* results) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_m[5 * WG];
    const AggCol g = acols[blockIdx.x];
    const GrpCol gc = gcols[blockIdx.x];
    const uint32_t g0 = blockIdx.y * GRPL_FINISH_GROUPS;
    if (g0 >= gc.n_groups) return;   // (uniform; workgroup 0 always has groups: n_groups >= 1)
    const bool sum = (g.ops & AGG_VALUE_OPS) != 0;
    const bool flt = wcols[blockIdx.x].flt && sum;
    uint64_t* res = results + (uint64_t)blockIdx.x * grp_result_words(gmax);
    if (blockIdx.y == 0) {
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
            res[0] = nsel;
            res[1] = gld64(flags + slots + blockIdx.x);
            res[2] = gld64(flags + slots + gridDim.x + blockIdx.x);   // the column met a Freq page (wgt_tile): for the host's replay
            for (int i = 3; i < 8; i++) res[i] = 0;
        }
    }
    const uint32_t G = min(GRPL_FINISH_GROUPS, gc.n_groups - g0);
    uint32_t Gp = 1;
    while (Gp < G) Gp <<= 1;
    const uint32_t stripes = WG / Gp, grp = threadIdx.x & (Gp - 1), stripe = threadIdx.x / Gp;
    uint64_t sel = 0, cnt = 0, nans = 0, s0 = 0, s1 = 0;
    auto take = [&](uint64_t psel, uint64_t pcnt, uint64_t pnans, uint64_t p0, uint64_t p1) {   // acc + p, in this order
        sel += psel, cnt += pcnt, nans += pnans;
        if (flt) {
            s0 = agg_bits(agg_dbl(s0) + agg_dbl(p0));
        } else {
            const uint64_t old = s0;
            s0 += p0;
            s1 += p1 + (s0 < old ? 1ull : 0ull);
        }
    };
    if (grp < G) {
        const uint64_t total = g.page_slots + g.tile_slots;
        for (uint64_t j = stripe; j < total; j += stripes) {
            const uint64_t slot = j < g.page_slots ? g.page_slot0 + j : g.tile_slot0 + (j - g.page_slots);
            if (!gld64(flags + slot)) continue;
            const GrpPart p = recs[slot * gmax + g0 + grp];
            take(p.sel, p.cnt, p.nans, p.s0, p.s1);
        }
    }
    uint64_t* m = s_m + threadIdx.x;
    m[0 * WG] = sel, m[1 * WG] = cnt, m[2 * WG] = nans, m[3 * WG] = s0, m[4 * WG] = s1;
    __syncthreads();
    if (stripe == 0 && grp < G) {
        for (uint32_t st = 1; st < stripes; st++) {
            const uint64_t* o = s_m + st * Gp + grp;
            take(o[0 * WG], o[1 * WG], o[2 * WG], o[3 * WG], o[4 * WG]);
        }
        uint64_t* r = res + 8 + (uint64_t)(g0 + grp) * 8;
        r[0] = sel;
        r[1] = cnt;
        r[2] = sum ? nans : 0;
        r[3] = 0;
        r[4] = 0;
        r[5] = sum ? s0 : 0;
        r[6] = sum ? s1 : 0;
        r[7] = 0;
    }
}

// ---- the replay of a column that met a Freq page: k_grpl_plain with the weight, a slot per chunk of
// GRPL_CHUNK_TILES * TILE_ROWS rows, walked tile by tile as k_wgt walks them
__global__ void __launch_bounds__(WG) k_wgt_plain(WgtLaunch wl, uint32_t col, const uint8_t* values, const uint8_t* validity) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[WGT_LDS_WORDS];
    const GrpLaunch& gl = wl.gl;
    const AggCol g = gl.acols[col];
    const GrpCol gc = gl.gcols[col];
    const WgtCol wc = wl.wcols[col];
    const uint64_t c0 = (uint64_t)blockIdx.x * GRPL_CHUNK_TILES * TILE_ROWS, c1 = min(g.rows, c0 + (uint64_t)GRPL_CHUNK_TILES * TILE_ROWS);
    const uint32_t w = g.w;
    const GrpSink k{g.sel, validity, 0, gc.ids, gc.idw, gc.n_groups, s_g, false};
    bool live = false;
    uint64_t oor = 0;
    for (uint64_t lo = c0; lo < c1; lo += TILE_ROWS) {
        const uint64_t hi = min(c1, lo + TILE_ROWS);
        if (!agg_any_selected(g.sel, lo, hi)) continue;
        if (!live) {
            wgt_table_clear(s_g, gc.n_groups);
            live = true;
        }
        wgt_span<true>(k, wc, oor, g.kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = flt_load(values + r * w, w), true; });
    }
    if (live) wgt_store(gl, col, g.tile_slot0 + blockIdx.x, gc.n_groups, wc.flt, s_g, oor, s_w64);
}

// the flags, the out-of-range counters and the Freq marks start from zero; timed under a name of its own
void launch_wgt_zero(sb_ctx* ctx, const WgtLaunch& wl, uint32_t n_cols) {
    KScope k(ctx, "wgt_zero(memset)");
    (void)hipMemsetAsync(wl.gl.flags, 0, (size_t)(wl.gl.slots + 2 * n_cols) * sizeof(uint64_t), ctx->stream);
}

// gl.tile_base: the slot of the call's first chunk; the chunk slots are the rest of gl.slots
void launch_wgt(sb_ctx* ctx, const DecodeArgs& a, const WgtLaunch& wl) {
    hipStream_t s = ctx->stream;
    const GrpLaunch& gl = wl.gl;
    const uint32_t parts = std::max<uint32_t>(1u, a.rle_parts);
    if (gl.any_null) {
        KScope k(ctx, "k_wgt_null");
        k_wgt_null<<<a.n_pages, WG, 0, s>>>(a, wl, parts);
    }
    if (gl.any_val) {
        KScope k(ctx, "k_wgt_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_wgt_rle<<<dim3(a.n_pages, parts), WG, 0, s>>>(a, wl);
    }
    const uint64_t chunks = gl.slots - gl.tile_base;
    if (gl.any_val && chunks) {
        KScope k(ctx, "k_wgt");
        k_wgt<<<(uint32_t)chunks, WG, 0, s>>>(a, wl);
    }
}

void launch_wgt_finish(sb_ctx* ctx, const WgtLaunch& wl, uint64_t* results, uint32_t n_cols) {
    KScope k(ctx, "k_wgt_finish");
    const GrpLaunch& gl = wl.gl;
    k_wgt_finish<<<dim3(n_cols, (gl.gmax + GRPL_FINISH_GROUPS - 1) / GRPL_FINISH_GROUPS), WG, 0, ctx->stream>>>(gl.acols, gl.gcols, wl.wcols, gl.flags, gl.recs,
                                                                                                                gl.slots, gl.gmax, results);
}

// `rows[i]`, `values[i]`, `validity[i]` (host arrays): the decoded columns of the replay
void launch_wgt_plain(sb_ctx* ctx, const WgtLaunch& wl, uint32_t n_cols, const uint64_t* rows, const uint8_t* const* values, const uint8_t* const* validity) {
    KScope k(ctx, "k_wgt_plain");
    for (uint32_t i = 0; i < n_cols; i++)
        if (rows[i]) k_wgt_plain<<<(uint32_t)grpl_chunks((rows[i] + TILE_ROWS - 1) / TILE_ROWS), WG, 0, ctx->stream>>>(wl, i, values[i], validity[i]);
}

}  // namespace sb
