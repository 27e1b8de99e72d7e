// strawboat-hip: sb_filter_columns_var — comparison columns of a binary type (included by sb_decode.hip behind sb_filter.h,
// whose sink — filter_span / sel_put — every kernel here ends in).
//
// Values compare with the column's literal as byte strings: bytes unsigned, lexicographic, a proper prefix less than the
// longer string; STARTS_WITH beside the six orderings (FilterCol.mask == FILTER_MASK_PREFIX).  ENDS_WITH, CONTAINS and the
// NOT_ forms (a FILTER_MASK_SUB bit in the mask) have kernels of their own, sb_filter_sub.h: only the row lookups of their
// Dict / Freq pages are done here.
//   Dict, Freq (a virtual Dict page,  k_filter_bin_entries evaluates the predicate ONCE PER ENTRY of every such page of the
//   k_plan)                           call (a lane per entry, the entry found through k_plan's offset table) into a bit table
//                                     at the end of the page's aux area; k_filter_bin then looks a bit up per row: the tile's
//                                     indices through u32_tile_to_lds, the table from LDS (<= FILTER_DICT_BITS entries) or HBM
//   OneValue                          one compare per tile
//   Basic, values None                a lane per row: the offset pair from d.src, the bytes from d.vbody
//   Basic, values LZ4 / Zstd / Snappy the same with the bytes in the column's share of the staging area (ColDesc.values),
//                                     where queues B / Z inflate them once k_filter_bin_base has given every such page its
//                                     place: a scan of vusize over the column's pages, 0 for the pages that need no staging
// A read's k_bin_tile_sums / k_bin_tile_scan / k_colscan / k_expand_binary are not launched: no offsets, no value bytes and
// no per-tile byte totals are needed for a bit per row.
//
// LOADS STAY INSIDE THEIR BUFFER.  A string of n >= 8 bytes is read in 8-byte steps from its first byte and, for the tail,
// once more at its last 8 bytes (the bytes read twice are known to be equal by then); a string of n < 8 bytes by two
// overlapping 4- / 2-byte loads or one byte load — never a byte before the string's first or behind its last.  The literal
// is followed by 8 zero bytes in the call's tables (sb_api.hip), so its first word is one load whatever its length.
#pragma once

namespace sb {

struct BinLit {
    const uint8_t* p;   // lit_len bytes + 8 zero bytes
    uint64_t w0;        // its first 8 bytes (zero padded): most compares end there
    uint32_t len, mask;
};
__device__ __forceinline__ BinLit bin_lit(const FilterCol& f) {
    const uint8_t* p = (const uint8_t*)(uintptr_t)f.lit;
    return BinLit{p, ldu64(p), f.lit_len, f.mask};
}
// the n (1 .. 7) bytes at p as a little-endian number
__device__ __forceinline__ uint64_t bin_ld_short(const uint8_t* p, uint32_t n) {
    if (n >= 4) return (uint64_t)ldu32(p) | ((uint64_t)ldu32(p + n - 4) << (8 * (n - 4)));
    if (n >= 2) return (uint64_t)ldu16(p) | ((uint64_t)ldu16(p + n - 2) << (8 * (n - 2)));
    return ldu8(p);
}
__device__ __forceinline__ uint32_t bin_order(uint64_t a, uint64_t b) {   // of two 8-byte groups that differ
    return __builtin_bswap64(a) < __builtin_bswap64(b) ? 0u : 2u;
}
// the first n bytes of the value against the first n bytes of the literal (n <= both lengths): 0 less, 1 equal, 2 greater
__device__ __forceinline__ uint32_t bin_rel_prefix(const uint8_t* v, const BinLit& l, uint32_t n) {
    if (n < 8) {
        if (n == 0) return 1u;
        const uint64_t a = bin_ld_short(v, n), b = l.w0 & ((1ull << (8 * n)) - 1);
        return a == b ? 1u : bin_order(a, b);
    }
    uint64_t a = ldu64(v);
    if (a != l.w0) return bin_order(a, l.w0);
    uint32_t i = 8;
    for (; i + 8 <= n; i += 8) {
        a = ldu64(v + i);
        const uint64_t b = ldu64(l.p + i);
        if (a != b) return bin_order(a, b);
    }
    if (i < n) {
        a = ldu64(v + n - 8);
        const uint64_t b = ldu64(l.p + n - 8);
        if (a != b) return bin_order(a, b);
    }
    return 1u;
}
__device__ __forceinline__ bool bin_eval(const uint8_t* v, uint32_t len, const BinLit& l) {
    if (l.mask & FILTER_MASK_PREFIX) return len >= l.len && bin_rel_prefix(v, l, l.len) == 1u;
    uint32_t r = bin_rel_prefix(v, l, min(len, l.len));
    if (r == 1u) r = len < l.len ? 0u : len == l.len ? 1u : 2u;
    return (l.mask >> r) & 1u;
}

// ---- where the inflated value blocks of a column go: one wave per column, scan_column_pages (sb_decode.hip) summing vusize
// for the pages whose values block is compressed and 0 for the others; no offset bases, no values_len.  (bin_base_column /
// bin_base_done: the body, which the selected read of binary columns launches for itself — k_rsel_bin_base, sb_read_sel_bin.h)
__device__ __forceinline__ void bin_base_column(const DecodeArgs& a, const ColDesc& c) {
    auto staged = [](const PageDesc& d) { return is_basic(d.codec) && d.codec != SB_CODEC_NONE; };
    scan_column_pages(
        a, c, [&](const PageDesc& d) { return staged(d) ? d.vusize : 0u; },
        [&](uint32_t p, const PageDesc& d, bool in, uint64_t base, bool fits) {
            if (!(in && d.ok && staged(d))) return;
            a.descs[p].val_base = base;
            if (!fits) a.descs[p].ok = 0;   // (nothing is inflated or compared; the column raises)
        });
}
__device__ __forceinline__ void bin_base_done(const DecodeArgs& a) {
    if (last_workgroup_done(&a.job_counts[6]) && threadIdx.x == 0)   // queue B is complete: its length for k_zstd_split
        a.job_counts[9] = __hip_atomic_load(&a.job_counts[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__global__ void __launch_bounds__(64) k_filter_bin_base(DecodeArgs a, const FilterCol* fcols) {
    const uint32_t ci = blockIdx.x;
    const ColDesc c = a.cols[ci];
    if (is_binary(c.ptype) && fcols[ci].kind == FK_BYTES) bin_base_column(a, c);
    bin_base_done(a);
}

// ---- Dict / Freq pages: k_plan's entry offsets and the page's bit table
struct BinDict {
    const uint32_t* ent_off;   // D + 1 offsets of the entries' records (u64 length | bytes) from d.dict
    uint32_t* bits;            // bit e: entry e satisfies the predicate
    uint32_t D, gap;           // gap: bytes between entry 0 and entry 1 of a Freq page (its bitmap)
};
__device__ __forceinline__ bool bin_dict(const DecodeArgs& a, const PageTask& t, const PageDesc& d, BinDict* out) {
    uint32_t* aux = (uint32_t*)(a.scratch + t.aux_off);
    const bool freq = d.codec == SB_CODEC_FREQ;
    const uint32_t used = freq ? 0 : idx_aux_words(d.icodec, d.n_runs, t.num_values);
    const uint64_t tw = filter_bin_table_words(t.length);
    uint32_t* bits = (uint32_t*)(a.scratch + t.infl_off) - tw;
    out->ent_off = aux + used;
    out->bits = bits;
    out->D = d.dict_n;
    out->gap = freq ? 4 + d.vcsize : 0;
    // (k_plan walked the D entries inside the page, so D <= length / 8 and the table holds them; its own words end below)
    return ((uint64_t)d.dict_n + 31) / 32 <= tw && aux + used + (uint64_t)d.dict_n + 1 <= bits;
}
// grid (pages, FILTER_BIN_EY): a lane per entry, 32 entries per word of the table
constexpr uint32_t FILTER_BIN_EY = 4;
__global__ void __launch_bounds__(WG) k_filter_bin_entries(DecodeArgs a, const FilterCol* fcols) {
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    if (!d.ok || (d.codec != SB_CODEC_DICT && d.codec != SB_CODEC_FREQ)) return;
    const PageTask t = a.tasks[p];
    if (!is_binary(a.cols[t.col].ptype)) return;
    const FilterCol f = fcols[t.col];
    if (f.kind != FK_BYTES) return;
    if (f.mask & FILTER_MASK_SUB) return;   // (k_filter_sub_entries)
    BinDict bd;
    if (!bin_dict(a, t, d, &bd)) {
        if (threadIdx.x == 0 && blockIdx.y == 0) raise(a.status, SB_ERR_INVALID, p, 220);
        return;
    }
    const BinLit lit = bin_lit(f);
    for (uint32_t e0 = blockIdx.y * WG; e0 < bd.D; e0 += gridDim.y * WG) {
        const uint32_t e = e0 + threadIdx.x;
        bool b = false;
        if (e < bd.D) {
            const uint64_t pr = ldu64((const uint8_t*)(bd.ent_off + e));
            const uint32_t eo = (uint32_t)pr;
            const uint32_t len = (uint32_t)(pr >> 32) - eo - 8 - (e == 0 ? bd.gap : 0);
            b = bin_eval(d.dict + eo + 8, len, lit);
        }
        const uint64_t m = __ballot(b);
        if ((threadIdx.x & 31) == 0 && e < bd.D) gst32(bd.bits + (e >> 5), ballot_half(m));
    }
}

// ---- the tiles of the binary comparison columns
template <class O>
__device__ __forceinline__ void filter_bin_basic(const FilterSink& k, uint64_t lo, uint64_t hi, const uint8_t* offs, const uint8_t* vals,
                                                 uint32_t vsize, const BinLit& lit) {
    filter_span(k, lo, hi, [&](uint64_t r) {
        uint64_t o0, o1;
        if constexpr (sizeof(O) == 4) {   // (the pair with one load)
            const uint64_t pr = ldu64(offs + r * 4);
            o0 = (uint32_t)pr;
            o1 = pr >> 32;
        } else {
            o0 = ldu64(offs + r * 8);
            o1 = ldu64(offs + r * 8 + 8);
        }
        // offsets that leave the values block (a read hands them on as they are) are cut to it: nothing outside is loaded
        o1 = min(o1, (uint64_t)vsize);
        o0 = min(o0, o1);
        return bin_eval(vals + o0, (uint32_t)(o1 - o0), lit);
    });
}
__device__ void filter_bin_tile(const DecodeArgs& a, const FilterCol* fcols, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint32_t* s_tab) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    if (!is_binary(c.ptype)) return;   // (k_filter)
    const FilterCol f = fcols[tt.col];
    if (f.kind != FK_BYTES) return;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    const FilterSink k{f.sel, d.def_bits, t.out_row, t.num_values, f.combine};
    const BinLit lit = bin_lit(f);
    if (is_basic(d.codec)) {
        if (lit.mask & FILTER_MASK_SUB) return;   // (k_filter_sub)
        const uint8_t* vals = d.codec == SB_CODEC_NONE ? d.vbody : c.values + d.val_base;
        if (c.ptype == SB_TYPE_BINARY) filter_bin_basic<int32_t>(k, lo, hi, d.src, vals, d.vusize, lit);
        else filter_bin_basic<int64_t>(k, lo, hi, d.src, vals, d.vusize, lit);
    } else if (d.codec == SB_CODEC_ONEVALUE) {
        if (lit.mask & FILTER_MASK_SUB) return;   // (k_filter_sub)
        const bool v = bin_eval(d.dict, d.dict_n, lit);
        filter_span(k, lo, hi, [&](uint64_t) { return v; });
    } else if (d.codec == SB_CODEC_DICT || d.codec == SB_CODEC_FREQ) {
        BinDict bd;
        if (!bin_dict(a, t, d, &bd)) return;   // (raised by k_filter_bin_entries)
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
        if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 222);   // (where a read finds it: plan_bin_dict / k_bin_tile_sums)
    }
}

// 18 KB of LDS like k_filter: the tile's indices and the Dict bit table
__global__ void __launch_bounds__(WG) k_filter_bin(DecodeArgs a, const FilterCol* fcols) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_tab[FILTER_DICT_BITS / 32];
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        filter_bin_tile(a, fcols, ti, s_a, s_w, s_tab);
        __syncthreads();
    }
}

void launch_filter_bin_base(sb_ctx* ctx, const DecodeArgs& a, const FilterCol* fcols) {
    KScope k(ctx, "k_filter_bin_base");
    k_filter_bin_base<<<a.n_cols, 64, 0, ctx->stream>>>(a, fcols);
}
void launch_filter_bin(sb_ctx* ctx, const DecodeArgs& a, const FilterCol* fcols) {
    hipStream_t s = ctx->stream;
    {
        KScope k(ctx, "k_filter_bin_entries");
        k_filter_bin_entries<<<dim3(a.n_pages, FILTER_BIN_EY), WG, 0, s>>>(a, fcols);
    }
    if (a.n_tiles) {
        KScope k(ctx, "k_filter_bin");
        k_filter_bin<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, fcols);
    }
}

}  // namespace sb
