// strawboat-hip: sb_aggregate_grouped — the grouping sink on the decoder's walks (included by sb_decode.hip behind
// sb_aggregate.h, whose accumulators, order keys and selection helpers it uses).
//
// sb_aggregate_columns sends every live row to one accumulator; this call sends it to the accumulator of its group: row r
// of the column belongs to group ids[r], an array the caller read or computed before.  The chain is sb_aggregate_columns'
// with a sibling per kernel:
//   k_grp_null               columns without MIN / MAX / SUM, of every type: selection, def levels and ids, per page
//   k_grp_rle / k_grp        the walks of k_agg_rle / k_agg with grp_span as the sink (below)
//   k_grp_finish             one workgroup per column: the bits set below `rows`, and the column's slots combined per group
//   k_grp_plain              the replay of a call that met a Freq page, from the decoded column
// A workgroup keeps one table of n_groups accumulators in LDS for a tile (a page part in the RLE walk).  What is exact in
// any order — the counts, the order keys of min / max, the two words of an integer sum — is updated with integer LDS
// atomics.  A float sum is not: a wave loops over the distinct ids its 64 lanes hold, adds the lanes of one id with a fixed
// shuffle tree (the first few ids) or in lane order (the rest, by rank: grp_span) into the wave's own row of the table,
// without an atomic.  The four rows are added in wave order when the table is written out, into the records of the tile's
// slot; k_grp_finish adds a group's records in an order that is a function of the slot numbers alone.  So the order of the
// double additions of every group's sum is fixed by the column's shape and data: the same call gives the same bits every
// time.  That holds for an interval that is issued again too: a column without a Freq page stays on the page route there,
// and a column with one takes the decoded route in every interval it is part of (grp_tile marks it, the host goes by the mark).
// A slot holds `gmax` records and has a flag word; only the flags are zeroed, an unwritten slot's records are never read.
#pragma once

namespace sb {

typedef __attribute__((address_space(3))) uint64_t* l64p;
// the table: field f of group g at s_g[f * S + g], S the table's stride (GRP_MAX_GROUPS for this call's kernels).  Fields 5.. are the two words of an integer sum, or the
// four waves' rows of a float sum
constexpr uint32_t GF_SEL = 0, GF_CNT = 1, GF_NANS = 2, GF_KMIN = 3, GF_KMAX = 4, GF_SUM = 5;
// distinct ids of a wave's step that get a shuffle tree each; the rest go by rank (grp_span).  A tree is six dependent
// 64-bit shuffles, a rank round one LDS add for every id at once: past a handful of ids the rounds are cheaper
constexpr uint32_t GRP_TREE_IDS = 4;
constexpr uint32_t GRP_LDS_WORDS =(GF_SUM + WG / 64) * GRP_MAX_GROUPS;   // 18 KB
// (S: the table's stride, the most groups it holds: GRP_MAX_GROUPS here, GRPL_MAX_GROUPS in sb_aggregate_grouped_large.h)
template <uint32_t S = GRP_MAX_GROUPS>
__device__ __forceinline__ uint64_t* grp_field(uint64_t* s_g, uint32_t f) { return s_g + f * S; }
__device__ __forceinline__ void grp_lds_add(uint64_t* p, uint64_t v) {
    (void)__hip_atomic_fetch_add((l64p)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

struct GrpSink {
    const uint32_t* sel;       // as in AggSink
    const uint8_t* def_bits;
    uint64_t out_row;
    const uint8_t* ids;        // the column's ids
    uint32_t idw, G;           // bytes per id; n_groups
    uint64_t* s_g;             // the workgroup's table
    bool all_null;             // a SB_TYPE_NULL column: no row is live
};
__device__ __forceinline__ uint32_t grp_id(const uint8_t* ids, uint32_t w, uint64_t c) {
    return w == 1 ? (uint32_t)ldu8(ids + c) : w == 2 ? (uint32_t)ldu16(ids + 2 * c) : ldu32(ids + 4 * c);
}
// by the whole workgroup, followed by a barrier
template <uint32_t S = GRP_MAX_GROUPS>
__device__ __forceinline__ void grp_table_clear(uint64_t* s_g, uint32_t G) {
    for (uint32_t i = threadIdx.x; i < G; i += WG) {
#pragma unroll
        for (uint32_t f = 0; f < GF_SUM + WG / 64; f++) grp_field<S>(s_g, f)[i] = f == GF_KMIN ? ~0ull : 0ull;
    }
    __syncthreads();
}

// Rows [lo, hi) of a page, by the whole workgroup, a lane per row and the same number of steps for every lane (the float
// sum is a matter of the whole wave).  A selected row is counted in its group or, with an id >= n_groups, in `oor`; a live
// one (VAL) is aggregated there: value_of(row, raw) gives its value, or false for a row that has none (a Dict index beyond
// the dictionary: the caller raises).
template <bool VAL, uint32_t S = GRP_MAX_GROUPS, class V>
__device__ __forceinline__ void grp_span(const GrpSink& k, uint64_t& oor, uint32_t kind, uint32_t w, uint64_t lo, uint64_t hi, V value_of) {
    const bool flt = VAL && agg_is_float(kind);
    uint64_t* const s_g = k.s_g;
    for (uint64_t base = lo; base < hi; base += WG) {
        const uint64_t r = base + threadIdx.x, c = k.out_row + r;
        bool on = r < hi;
        if (on && k.sel) on = (gld32(k.sel + (c >> 5)) >> (uint32_t)(c & 31)) & 1u;
        uint32_t id = 0;
        if (on) {   // (the id of an unselected row is never loaded)
            id = grp_id(k.ids, k.idw, c);
            if (id >= k.G) {
                oor++;
                on = false;
            } else {
                grp_lds_add(grp_field<S>(s_g, GF_SEL) + id, 1);
            }
        }
        if (on && k.all_null) on = false;
        if (on && k.def_bits) on = (ldu8(k.def_bits + (r >> 3)) >> (uint32_t)(r & 7)) & 1u;
        uint64_t raw = 0;
        if (VAL && on) on = value_of(r, raw);
        if (on) grp_lds_add(grp_field<S>(s_g, GF_CNT) + id, 1);
        if (!VAL) continue;
        double v = 0.0;
        if (flt) {
            if (on) v = kind == FK_F32 ? (double)__uint_as_float((uint32_t)raw) : agg_dbl(raw);
            // the wave's lanes by id: the lowest remaining lane names it, its lanes are added by a fixed tree (the other
            // lanes add 0.0), lane 0 adds the result into the wave's row
            uint64_t* const row = grp_field<S>(s_g, GF_SUM + (threadIdx.x >> 6));
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
            // What follows, and the next step, read and write the same row from other lanes with plain accesses.  That is
            // safe on this hardware: a wave's LDS operations execute in the order they are issued, and the compiler keeps
            // the order of accesses that may alias.  It is not something the language promises across lanes, so the wave
            // barriers below pin the phases for the compiler, and test_float_sums_that_are_exact_in_no_order with 96 groups
            // and test_group_counts_and_id_patterns catch a lost update (a rank loop collapsed into one add) as a wrong sum.
            __builtin_amdgcn_wave_barrier();
            if (left) {
                // Many ids in this step (high-cardinality keys): a tree per id would cost more than the rows.  Each of the
                // remaining lanes learns its rank among the remaining lanes of its id, from ballots alone; round k then adds
                // the lanes of rank k into the wave's row.  No two lanes of a round share an id, so the adds need no atomic,
                // and an id's lanes are added in lane order (the LDS operations of a wave execute in program order).
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
                for (uint32_t k = 0; k < rounds; k++) {
                    if (rem && rank == k) {
                        l64p slot = (l64p)(row + id);
                        *slot = agg_bits(agg_dbl(*slot) + v);
                    }
                    __builtin_amdgcn_wave_barrier();   // (keeps the rounds apart: a lane's add is not moved out of its round)
                }
            }
            if (on && v != v) {
                grp_lds_add(grp_field<S>(s_g, GF_NANS) + id, 1);
                on = false;   // a NaN has no place in min / max
            }
        } else if (on) {   // the 128-bit sum: the low word's old value tells the carry
            const uint64_t x = kind == FK_SIGNED ? agg_sext(raw, w) : raw;
            const uint64_t old = __hip_atomic_fetch_add((l64p)(grp_field<S>(s_g, GF_SUM) + id), x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const uint64_t up = (old + x < x ? 1ull : 0ull) + (kind == FK_SIGNED ? (uint64_t)((int64_t)x >> 63) : 0ull);
            if (up) grp_lds_add(grp_field<S>(s_g, GF_SUM + 1) + id, up);
        }
        if (on) {
            const uint64_t key = agg_key(kind, w, raw);
            (void)__hip_atomic_fetch_min((l64p)(grp_field<S>(s_g, GF_KMIN) + id), key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            (void)__hip_atomic_fetch_max((l64p)(grp_field<S>(s_g, GF_KMAX) + id), key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// The table into the records of `slot`, its flag set, and the workgroup's out-of-range rows added to the column's counter
// (integers: exact in any order).  By the whole workgroup; barriers inside.
template <uint32_t S = GRP_MAX_GROUPS>
__device__ __forceinline__ void grp_store(const GrpLaunch& gl, uint32_t col, uint64_t slot, uint32_t G, bool flt, uint64_t* s_g, uint64_t oor,
                                          uint64_t* s_w64) {
    __syncthreads();
    GrpPart* out = gl.recs + slot * gl.gmax;
    for (uint32_t g = threadIdx.x; g < G; g += WG) {
        GrpPart p;
        p.sel = grp_field<S>(s_g, GF_SEL)[g];
        p.cnt = grp_field<S>(s_g, GF_CNT)[g];
        p.nans = grp_field<S>(s_g, GF_NANS)[g];
        p.kmin = grp_field<S>(s_g, GF_KMIN)[g];
        p.kmax = grp_field<S>(s_g, GF_KMAX)[g];
        if (flt) {   // the waves' rows, in wave order
            double s = agg_dbl(grp_field<S>(s_g, GF_SUM)[g]);
#pragma unroll
            for (uint32_t wv = 1; wv < WG / 64; wv++) s += agg_dbl(grp_field<S>(s_g, GF_SUM + wv)[g]);
            p.s0 = agg_bits(s);
            p.s1 = 0;
        } else {
            p.s0 = grp_field<S>(s_g, GF_SUM)[g];
            p.s1 = grp_field<S>(s_g, GF_SUM + 1)[g];
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

// ---- tiles of None / OneValue / Dict / bit-packed / inflated pages: agg_tile with the grouping sink
// Rows [lo, hi) of tile `tile` of page `page` into the table of `k`, by the page's codec.  False: a page that has no tiles
// (RLE pages of <= 8-byte values: k_grp_rle), nothing was looked at.
template <uint32_t S = GRP_MAX_GROUPS>
__device__ __forceinline__ bool grp_tile_rows(const DecodeArgs& a, const PageDesc& d, const PageTask& t, const ColDesc& c, const GrpSink& k, uint64_t& oor,
                                              uint32_t kind, uint32_t page, uint32_t tile, uint64_t lo, uint64_t hi, uint32_t* s_a, uint32_t* s_w) {
    const uint32_t w = c.width, rows = (uint32_t)(hi - lo);
    switch (d.codec) {
        case SB_CODEC_NONE: {
            const uint8_t* src = d.src;
            grp_span<true, S>(k, oor, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = flt_load(src + r * w, w), true; });
            break;
        }
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {   // inflated into the staging area
            const uint8_t* src = c.values + t.out_row * w;
            grp_span<true, S>(k, oor, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = flt_load(src + r * w, w), true; });
            break;
        }
        case SB_CODEC_ONEVALUE: {   // one load for the page: a row brings its id alone
            const uint64_t one = flt_load(d.body, w);
            grp_span<true, S>(k, oor, kind, w, lo, hi, [&](uint64_t, uint64_t& raw) { return raw = one, true; });
            break;
        }
        case SB_CODEC_DICT: {
            U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
            u32_tile_to_lds(is, tile, rows, s_a, s_w);
            const uint8_t* dict = d.dict;
            const uint32_t D = d.dict_n;
            bool bad = false;
            grp_span<true, S>(k, oor, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) {
                const uint32_t e = s_a[sidx((int)(r - lo))];
                if (e >= D) {
                    bad = true;
                    return false;
                }
                raw = flt_load(dict + (uint64_t)e * w, w);
                return true;
            });
            if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, page, 400);
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            if (w != 4) break;
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            u32_tile_to_lds(vs, tile, rows, s_a, s_w);
            grp_span<true, S>(k, oor, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = (uint64_t)s_a[sidx((int)(r - lo))], true; });
            break;
        }
        default:   // (RLE pages of <= 8-byte values have no tiles: k_grp_rle)
            return false;
    }
    return true;
}

__device__ void grp_tile(const DecodeArgs& a, const GrpLaunch& gl, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint64_t* s_g, uint64_t* s_w64) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    const AggCol g = gl.acols[tt.col];
    if (!(g.ops & AGG_VALUE_OPS)) return;   // (k_grp_null)
    const GrpCol gc = gl.gcols[tt.col];
    const uint32_t kind = g.kind;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    // A Freq page asks for the replay whatever the selection (agg_tile), and marks its column: the replay takes the decoded
    // route for the marked columns alone, so the route of a column -- and with it the order of its float additions -- is a
    // matter of the column's own pages, not of what else the interval holds.  A marked column is not issued on this route
    // again; if one is, the call fails instead of leaving the page out.
    if (d.codec == SB_CODEC_FREQ) {
        if (threadIdx.x == 0 && tt.tile == 0) {
            gst64(gl.flags + gl.slots + gl.n_cols + tt.col, 1);
            if (gl.replayed) raise(a.status, SB_ERR_NYI, tt.page, 410);
            else atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
        }
        return;
    }
    // a tile without a selected row: no value, no index and no id is loaded, and its slot stays unwritten
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) return;
    grp_table_clear(s_g, gc.n_groups);
    const GrpSink k{g.sel, d.def_bits, t.out_row, gc.ids, gc.idw, gc.n_groups, s_g, false};
    uint64_t oor = 0;
    if (!grp_tile_rows(a, d, t, c, k, oor, kind, tt.page, tt.tile, lo, hi, s_a, s_w)) return;
    grp_store(gl, tt.col, gl.tile_base + t.first_tile + tt.tile, gc.n_groups, agg_is_float(kind), s_g, oor, s_w64);
}

// 35 KB of LDS (k_agg's 17 KB and the table): 4 workgroups per CU
__global__ void __launch_bounds__(WG) k_grp(DecodeArgs a, GrpLaunch gl) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[GRP_LDS_WORDS];
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        grp_tile(a, gl, ti, s_a, s_w, s_g, s_w64);
        __syncthreads();
    }
}

// ---- RLE pages: rle_page_walk with this policy (RleAggregate's staging of the run values).  The table lives for the
// whole page part: one write-out, one slot.
struct RleGrouped {
    using Rec = uint64_t;
    uint64_t* s_rec;
    GrpSink k;
    uint64_t* oor;
    uint32_t kind, w;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + w; }
    __device__ __forceinline__ uint64_t load(const uint8_t* v, bool in) const { return in ? flt_load(v, w) : 0ull; }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        grp_span<true>(k, *oor, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = s_rec[A + s_flag[sidx((int)(r - tile_lo))]], true; });
    }
};

__global__ void __launch_bounds__(WG) k_grp_rle(DecodeArgs a, GrpLaunch gl) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint64_t s_vals[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[GRP_LDS_WORDS];
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    const AggCol g = gl.acols[t.col];
    if (!(g.ops & AGG_VALUE_OPS)) return;
    const GrpCol gc = gl.gcols[t.col];
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    grp_table_clear(s_g, gc.n_groups);
    uint64_t oor = 0;
    const RleGrouped pol{s_vals, GrpSink{g.sel, d.def_bits, t.out_row, gc.ids, gc.idw, gc.n_groups, s_g, false}, &oor, g.kind, c.width};
    rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
    grp_store(gl, t.col, (uint64_t)p * parts + part, gc.n_groups, agg_is_float(g.kind), s_g, oor, s_w64);
}

// ---- columns without MIN / MAX / SUM, of every physical type: the def-level section of k_agg_null, a lane per row
__global__ void __launch_bounds__(WG) k_grp_null(DecodeArgs a, GrpLaunch gl, uint32_t parts) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[GRP_LDS_WORDS];
    const uint32_t p = blockIdx.x;
    const PageTask t = a.tasks[p];
    const AggCol g = gl.acols[t.col];
    if (g.ops & AGG_VALUE_OPS) return;
    const GrpCol gc = gl.gcols[t.col];
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
    grp_table_clear(s_g, gc.n_groups);
    uint64_t oor = 0;
    const GrpSink k{g.sel, def, t.out_row, gc.ids, gc.idw, gc.n_groups, s_g, g.ptype == SB_TYPE_NULL};
    grp_span<false>(k, oor, 0, 0, 0, N, [](uint64_t, uint64_t&) { return true; });
    grp_store(gl, t.col, (uint64_t)p * parts, gc.n_groups, false, s_g, oor, s_w64);
}

// ---- one workgroup per column.  A thread has one group and one stripe of the column's slots: with G groups, rounded up
// to a power of two Gp, there are WG / Gp stripes, stripe s takes slots s, s + WG / Gp, ... of the column (page slots
// first, then tile slots) in rising order, and stripe 0's thread then adds the stripes' records in stripe order.
__global__ void __launch_bounds__(WG) k_grp_finish(const AggCol* acols, const GrpCol* gcols, const uint64_t* flags, const GrpPart* recs,
                                                   uint64_t slots, uint32_t gmax, uint64_t* results) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_m[7 * WG];
    const AggCol g = acols[blockIdx.x];
    const GrpCol gc = gcols[blockIdx.x];
    const bool flt = agg_is_float(g.kind) && (g.ops & AGG_VALUE_OPS);
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
    const uint32_t G = gc.n_groups;
    uint32_t Gp = 1;
    while (Gp < G) Gp <<= 1;
    const uint32_t stripes = WG / Gp, grp = threadIdx.x & (Gp - 1), stripe = threadIdx.x / Gp;
    AggAcc acc;
    uint64_t sel = 0;
    auto take = [&](const GrpPart& p) {
        AggAcc b;
        b.cnt = p.cnt, b.nans = p.nans, b.kmin = p.kmin, b.kmax = p.kmax, b.s0 = p.s0, b.s1 = p.s1;
        acc = agg_merge(acc, b, flt);
        sel += p.sel;
    };
    if (grp < G) {
        const uint64_t total = g.page_slots + g.tile_slots;
        for (uint64_t j = stripe; j < total; j += stripes) {
            const uint64_t slot = j < g.page_slots ? g.page_slot0 + j : g.tile_slot0 + (j - g.page_slots);
            if (!gld64(flags + slot)) continue;
            take(recs[slot * gmax + grp]);
        }
    }
    uint64_t* m = s_m + threadIdx.x;
    m[0 * WG] = sel, m[1 * WG] = acc.cnt, m[2 * WG] = acc.nans, m[3 * WG] = acc.kmin, m[4 * WG] = acc.kmax, m[5 * WG] = acc.s0, m[6 * WG] = acc.s1;
    __syncthreads();
    uint64_t* res = results + (uint64_t)blockIdx.x * grp_result_words(gmax);
    if (threadIdx.x == 0) {
        res[0] = nsel;
        res[1] = gld64(flags + slots + blockIdx.x);
        res[2] = gld64(flags + slots + gridDim.x + blockIdx.x);   // the column met a Freq page (grp_tile): for the host's replay
        for (int i = 3; i < 8; i++) res[i] = 0;
    }
    if (stripe == 0 && grp < G) {
        for (uint32_t st = 1; st < stripes; st++) {
            const uint64_t* o = s_m + st * Gp + grp;
            GrpPart p;
            p.sel = o[0 * WG], p.cnt = o[1 * WG], p.nans = o[2 * WG], p.kmin = o[3 * WG], p.kmax = o[4 * WG], p.s0 = o[5 * WG], p.s1 = o[6 * WG];
            take(p);
        }
        uint64_t* r = res + 8 + (uint64_t)grp * 8;
        const bool any = acc.cnt > acc.nans && (g.ops & AGG_VALUE_OPS);
        r[0] = sel;
        r[1] = acc.cnt;
        r[2] = acc.nans;
        r[3] = any && (g.ops & 2u) ? agg_unkey(g.kind, g.w, acc.kmin) : 0;
        r[4] = any && (g.ops & 4u) ? agg_unkey(g.kind, g.w, acc.kmax) : 0;
        r[5] = (g.ops & 8u) ? acc.s0 : 0;
        r[6] = (g.ops & 8u) ? acc.s1 : 0;
        r[7] = 0;
    }
}

// ---- the replay of a call that met a Freq page: k_agg_plain with the grouping sink, a slot per TILE_ROWS rows
__global__ void __launch_bounds__(WG) k_grp_plain(GrpLaunch gl, uint32_t col, const uint8_t* values, const uint8_t* validity) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[GRP_LDS_WORDS];
    const AggCol g = gl.acols[col];
    const GrpCol gc = gl.gcols[col];
    const uint64_t lo = (uint64_t)blockIdx.x * TILE_ROWS, hi = min(g.rows, lo + TILE_ROWS);
    if (!agg_any_selected(g.sel, lo, hi)) return;
    grp_table_clear(s_g, gc.n_groups);
    uint64_t oor = 0;
    const uint32_t w = g.w;
    const GrpSink k{g.sel, validity, 0, gc.ids, gc.idw, gc.n_groups, s_g, false};
    grp_span<true>(k, oor, g.kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = flt_load(values + r * w, w), true; });
    grp_store(gl, col, g.tile_slot0 + blockIdx.x, gc.n_groups, agg_is_float(g.kind), s_g, oor, s_w64);
}

// the flags, the out-of-range counters and the Freq marks start from zero; timed under a name of its own
void launch_grp_zero(sb_ctx* ctx, const GrpLaunch& gl, uint32_t n_cols) {
    KScope k(ctx, "grp_zero(memset)");
    (void)hipMemsetAsync(gl.flags, 0, (size_t)(gl.slots + 2 * n_cols) * sizeof(uint64_t), ctx->stream);
}

void launch_grp(sb_ctx* ctx, const DecodeArgs& a, const GrpLaunch& gl) {
    hipStream_t s = ctx->stream;
    const uint32_t parts = std::max<uint32_t>(1u, a.rle_parts);
    if (gl.any_null) {
        KScope k(ctx, "k_grp_null");
        k_grp_null<<<a.n_pages, WG, 0, s>>>(a, gl, parts);
    }
    if (gl.any_val) {
        KScope k(ctx, "k_grp_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_grp_rle<<<dim3(a.n_pages, parts), WG, 0, s>>>(a, gl);
    }
    if (gl.any_val && a.n_tiles) {
        KScope k(ctx, "k_grp");
        k_grp<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, gl);
    }
}

void launch_grp_finish(sb_ctx* ctx, const GrpLaunch& gl, uint64_t* results, uint32_t n_cols) {
    KScope k(ctx, "k_grp_finish");
    k_grp_finish<<<n_cols, WG, 0, ctx->stream>>>(gl.acols, gl.gcols, gl.flags, gl.recs, gl.slots, gl.gmax, results);
}

// `rows[i]`, `values[i]`, `validity[i]` (host arrays): the decoded columns of the replay
void launch_grp_plain(sb_ctx* ctx, const GrpLaunch& gl, uint32_t n_cols, const uint64_t* rows, const uint8_t* const* values,
                      const uint8_t* const* validity) {
    KScope k(ctx, "k_grp_plain");
    for (uint32_t i = 0; i < n_cols; i++)
        if (rows[i]) k_grp_plain<<<(uint32_t)((rows[i] + TILE_ROWS - 1) / TILE_ROWS), WG, 0, ctx->stream>>>(gl, i, values[i], validity[i]);
}

}  // namespace sb
