// strawboat-hip: sb_aggregate_grouped_large — the grouping sink with up to GRPL_MAX_GROUPS (1024) groups (included by
// sb_decode.hip behind sb_aggregate_grouped.h, whose sink -- grp_span, grp_table_clear, grp_store, grp_tile_rows -- it uses
// with a table stride of GRPL_MAX_GROUPS).
//
// What the 256-group call does per tile does not stretch to 1024 groups: a record block of 64 KB per 4096-row tile is more
// than the tile's own values.  So what is new here is how long a table lives and where its records go:
//   k_grpl         tiles of None / OneValue / Dict / bit-packed / inflated pages.  A work item is a CHUNK of a column:
//                  GRPL_CHUNK_TILES (16) consecutive tiles of the column's own numbering (tile j of the column is in chunk
//                  j / 16).  One workgroup clears the table once, walks the chunk's tiles in rising j and stores once, into
//                  the chunk's slot.  The work does not come from the compact a.tiles list (k_parse appends to it with an
//                  atomicAdd: its order differs from run to run) but from blockIdx: the grid is the sum of the columns'
//                  chunks, known on the host, and a tile's page is found from PageTask::first_tile (grpl_page_of).
//   k_grpl_rle     k_grp_rle with the wide table: one table and one slot per (page, part)
//   k_grpl_null    k_grp_null with the wide table: one table and one slot per page
//   k_grpl_plain   the replay of a column that met a Freq page, from the decoded column: a table per 16 * TILE_ROWS rows
//   k_grpl_finish  grid (columns, ceil(gmax / 256)): a workgroup combines 256 groups of a column as k_grp_finish does;
//                  workgroup (col, 0) also writes the header words
// Determinism of the float sums: within a table the additions are grp_span's (fixed trees, then rank rounds in
// lane order, the four waves' rows added in wave order at the store).  Which rows share a table, and in which order they
// meet it, is a function of the column's own page layout alone: its chunk is made of its own tiles in rising order, the
// tiles of RLE pages and of pages that failed are passed over, whatever other columns the call has and whatever an
// interval that is issued again holds.  k_grpl_finish adds a group's records in an order that is a function of the slot
// numbers alone.  No float atomic anywhere.
// LDS: the table is 9 fields x 1024 groups x 8 bytes = 72 KB on top of the walk's 17 to 26 KB: one workgroup per CU.
#pragma once

namespace sb {

constexpr uint32_t GRPL_LDS_WORDS = (GF_SUM + WG / 64) * GRPL_MAX_GROUPS;   // 72 KB
constexpr uint32_t GRPL_FINISH_GROUPS = 256;                                 // groups per workgroup of k_grpl_finish

// One tile of a chunk: grp_tile's checks.  True: the tile's rows went into the table (which is cleared before the first
// such tile of the chunk: `live`).  By the whole workgroup, every branch uniform.
__device__ __forceinline__ bool grpl_tile(const DecodeArgs& a, const GrpLaunch& gl, uint32_t col, const ColDesc& c, const AggCol& g, const GrpCol& gc,
                                          uint32_t page, uint32_t tile, bool& live, uint64_t& oor, uint32_t* s_a, uint32_t* s_w, uint64_t* s_g) {
    const PageDesc d = a.descs[page];
    if (!d.ok) return false;
    const PageTask t = a.tasks[page];
    const uint64_t lo = (uint64_t)tile * TILE_ROWS;
    if (lo >= t.num_values) return false;
    const uint64_t hi = min(t.num_values, lo + TILE_ROWS);
    // a Freq page: the rule of grp_tile.  The column is marked and the replay asked for; the tile is passed over
    if (d.codec == SB_CODEC_FREQ) {
        if (threadIdx.x == 0 && tile == 0) {
            gst64(gl.flags + gl.slots + gl.n_cols + col, 1);
            if (gl.replayed) raise(a.status, SB_ERR_NYI, page, 411);
            else atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
        }
        return false;
    }
    if (rle_by_page(c, d)) return false;   // (k_grpl_rle)
    // a tile without a selected row: no value, no index and no id is loaded
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) return false;
    if (!live) {
        grp_table_clear<GRPL_MAX_GROUPS>(s_g, gc.n_groups);
        live = true;
    }
    const GrpSink k{g.sel, d.def_bits, t.out_row, gc.ids, gc.idw, gc.n_groups, s_g, false};
    (void)grp_tile_rows<GRPL_MAX_GROUPS>(a, d, t, c, k, oor, g.kind, page, tile, lo, hi, s_a, s_w);
    __syncthreads();   // (s_a is filled again by the next tile)
    return true;
}

// 89 KB of LDS (k_agg's 17 KB and the table): 1 workgroup per CU
__global__ void __launch_bounds__(WG) k_grpl(DecodeArgs a, GrpLaunch gl) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[GRPL_LDS_WORDS];
    // the chunk's slot names its column: the last column whose first chunk slot is not behind it (a column without a
    // chunk shares its slot0 with the column behind it and is never the answer)
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
    if (!(g.ops & AGG_VALUE_OPS)) return;   // (k_grpl_null)
    const ColDesc c = a.cols[col];
    if (!c.n_pages) return;
    const GrpCol gc = gl.gcols[col];
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
        (void)grpl_tile(a, gl, col, c, g, gc, page, gt - a.tasks[page].first_tile, live, oor, s_a, s_w, s_g);
    }
    // a chunk without a selected row stores nothing: its flag stays 0
    if (live) grp_store<GRPL_MAX_GROUPS>(gl, col, slot, gc.n_groups, agg_is_float(g.kind), s_g, oor, s_w64);
}

// ---- RLE pages: k_grp_rle with the wide table
struct RleGroupedLarge {
    using Rec = uint64_t;
    uint64_t* s_rec;
    GrpSink k;
    uint64_t* oor;
    uint32_t kind, w;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + w; }
    __device__ __forceinline__ uint64_t load(const uint8_t* v, bool in) const { return in ? flt_load(v, w) : 0ull; }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        grp_span<true, GRPL_MAX_GROUPS>(k, *oor, kind, w, lo, hi,
                                        [&](uint64_t r, uint64_t& raw) { return raw = s_rec[A + s_flag[sidx((int)(r - tile_lo))]], true; });
    }
};

// 98 KB of LDS: 1 workgroup per CU
__global__ void __launch_bounds__(WG) k_grpl_rle(DecodeArgs a, GrpLaunch gl) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint64_t s_vals[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[GRPL_LDS_WORDS];
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
    grp_table_clear<GRPL_MAX_GROUPS>(s_g, gc.n_groups);
    uint64_t oor = 0;
    const RleGroupedLarge pol{s_vals, GrpSink{g.sel, d.def_bits, t.out_row, gc.ids, gc.idw, gc.n_groups, s_g, false}, &oor, g.kind, c.width};
    rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
    grp_store<GRPL_MAX_GROUPS>(gl, t.col, (uint64_t)p * parts + part, gc.n_groups, agg_is_float(g.kind), s_g, oor, s_w64);
}

// ---- columns without MIN / MAX / SUM, of every physical type: k_grp_null with the wide table
__global__ void __launch_bounds__(WG) k_grpl_null(DecodeArgs a, GrpLaunch gl, uint32_t parts) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[GRPL_LDS_WORDS];
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
    grp_table_clear<GRPL_MAX_GROUPS>(s_g, gc.n_groups);
    uint64_t oor = 0;
    const GrpSink k{g.sel, def, t.out_row, gc.ids, gc.idw, gc.n_groups, s_g, g.ptype == SB_TYPE_NULL};
    grp_span<false, GRPL_MAX_GROUPS>(k, oor, 0, 0, 0, N, [](uint64_t, uint64_t&) { return true; });
    grp_store<GRPL_MAX_GROUPS>(gl, t.col, (uint64_t)p * parts, gc.n_groups, false, s_g, oor, s_w64);
}

// ---- grid (columns, ceil(gmax / GRPL_FINISH_GROUPS)).  Workgroup (col, y) has groups [256 y, 256 y + 256) of the column:
// k_grp_finish's stripes over them (with G' groups in this workgroup, rounded up to a power of two Gp, stripe s takes
// slots s, s + WG / Gp, ... of the column -- page slots first, then chunk slots -- in rising order, and stripe 0's thread
// adds the stripes' records in stripe order).  The header words are written by workgroup (col, 0) alone.
__global__ void __launch_bounds__(WG) k_grpl_finish(const AggCol* acols, const GrpCol* gcols, const uint64_t* flags, const GrpPart* recs,
                                                    uint64_t slots, uint32_t gmax, uint64_t* results) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_m[7 * WG];
    const AggCol g = acols[blockIdx.x];
    const GrpCol gc = gcols[blockIdx.x];
    const uint32_t g0 = blockIdx.y * GRPL_FINISH_GROUPS;
    if (g0 >= gc.n_groups) return;   // (uniform; workgroup 0 always has groups: n_groups >= 1)
    const bool flt = agg_is_float(g.kind) && (g.ops & AGG_VALUE_OPS);
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
            res[2] = gld64(flags + slots + gridDim.x + blockIdx.x);   // the column met a Freq page (grpl_tile): for the host's replay
            for (int i = 3; i < 8; i++) res[i] = 0;
        }
    }
    const uint32_t G = min(GRPL_FINISH_GROUPS, gc.n_groups - g0);
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
            take(recs[slot * gmax + g0 + grp]);
        }
    }
    uint64_t* m = s_m + threadIdx.x;
    m[0 * WG] = sel, m[1 * WG] = acc.cnt, m[2 * WG] = acc.nans, m[3 * WG] = acc.kmin, m[4 * WG] = acc.kmax, m[5 * WG] = acc.s0, m[6 * WG] = acc.s1;
    __syncthreads();
    if (stripe == 0 && grp < G) {
        for (uint32_t st = 1; st < stripes; st++) {
            const uint64_t* o = s_m + st * Gp + grp;
            GrpPart p;
            p.sel = o[0 * WG], p.cnt = o[1 * WG], p.nans = o[2 * WG], p.kmin = o[3 * WG], p.kmax = o[4 * WG], p.s0 = o[5 * WG], p.s1 = o[6 * WG];
            take(p);
        }
        uint64_t* r = res + 8 + (uint64_t)(g0 + grp) * 8;
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

// ---- the replay of a column that met a Freq page: k_grp_plain with the wide table, a slot per chunk of
// GRPL_CHUNK_TILES * TILE_ROWS rows, walked tile by tile as k_grpl walks them
__global__ void __launch_bounds__(WG) k_grpl_plain(GrpLaunch gl, uint32_t col, const uint8_t* values, const uint8_t* validity) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_g[GRPL_LDS_WORDS];
    const AggCol g = gl.acols[col];
    const GrpCol gc = gl.gcols[col];
    const uint64_t c0 = (uint64_t)blockIdx.x * GRPL_CHUNK_TILES * TILE_ROWS, c1 = min(g.rows, c0 + (uint64_t)GRPL_CHUNK_TILES * TILE_ROWS);
    const uint32_t w = g.w;
    const GrpSink k{g.sel, validity, 0, gc.ids, gc.idw, gc.n_groups, s_g, false};
    bool live = false;
    uint64_t oor = 0;
    for (uint64_t lo = c0; lo < c1; lo += TILE_ROWS) {
        const uint64_t hi = min(c1, lo + TILE_ROWS);
        if (!agg_any_selected(g.sel, lo, hi)) continue;
        if (!live) {
            grp_table_clear<GRPL_MAX_GROUPS>(s_g, gc.n_groups);
            live = true;
        }
        grp_span<true, GRPL_MAX_GROUPS>(k, oor, g.kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = flt_load(values + r * w, w), true; });
    }
    if (live) grp_store<GRPL_MAX_GROUPS>(gl, col, g.tile_slot0 + blockIdx.x, gc.n_groups, agg_is_float(g.kind), s_g, oor, s_w64);
}

// the flags, the out-of-range counters and the Freq marks start from zero; timed under a name of its own
void launch_grpl_zero(sb_ctx* ctx, const GrpLaunch& gl, uint32_t n_cols) {
    KScope k(ctx, "grpl_zero(memset)");
    (void)hipMemsetAsync(gl.flags, 0, (size_t)(gl.slots + 2 * n_cols) * sizeof(uint64_t), ctx->stream);
}

// gl.tile_base: the slot of the call's first chunk; the chunk slots are the rest of gl.slots
void launch_grpl(sb_ctx* ctx, const DecodeArgs& a, const GrpLaunch& gl) {
    hipStream_t s = ctx->stream;
    const uint32_t parts = std::max<uint32_t>(1u, a.rle_parts);
    if (gl.any_null) {
        KScope k(ctx, "k_grpl_null");
        k_grpl_null<<<a.n_pages, WG, 0, s>>>(a, gl, parts);
    }
    if (gl.any_val) {
        KScope k(ctx, "k_grpl_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_grpl_rle<<<dim3(a.n_pages, parts), WG, 0, s>>>(a, gl);
    }
    const uint64_t chunks = gl.slots - gl.tile_base;
    if (gl.any_val && chunks) {
        KScope k(ctx, "k_grpl");
        k_grpl<<<(uint32_t)chunks, WG, 0, s>>>(a, gl);
    }
}

void launch_grpl_finish(sb_ctx* ctx, const GrpLaunch& gl, uint64_t* results, uint32_t n_cols) {
    KScope k(ctx, "k_grpl_finish");
    k_grpl_finish<<<dim3(n_cols, (gl.gmax + GRPL_FINISH_GROUPS - 1) / GRPL_FINISH_GROUPS), WG, 0, ctx->stream>>>(gl.acols, gl.gcols, gl.flags, gl.recs,
                                                                                                                 gl.slots, gl.gmax, results);
}

// `rows[i]`, `values[i]`, `validity[i]` (host arrays): the decoded columns of the replay
void launch_grpl_plain(sb_ctx* ctx, const GrpLaunch& gl, uint32_t n_cols, const uint64_t* rows, const uint8_t* const* values,
                       const uint8_t* const* validity) {
    KScope k(ctx, "k_grpl_plain");
    for (uint32_t i = 0; i < n_cols; i++)
        if (rows[i]) k_grpl_plain<<<(uint32_t)grpl_chunks((rows[i] + TILE_ROWS - 1) / TILE_ROWS), WG, 0, ctx->stream>>>(gl, i, values[i], validity[i]);
}

}  // namespace sb
