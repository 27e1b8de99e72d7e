// strawboat-hip: sb_read_selected_var — the selected rows of Binary / LargeBinary columns (included by sb_decode.hip behind
// sb_read_sel.h, whose rank table and sink — sel_rank_at, sel_rows / sel_validity — every kernel here uses).
//
// Output row k is the column's row at the k-th set bit: offsets[k + 1] - offsets[k] is the row's byte length, the bytes sit
// back to back in `values`.  The chain is that of a binary filter column up to k_plan (Freq pages as virtual Dict pages, no
// k_bin_tile_sums / k_bin_tile_scan / k_colscan), then
//   k_rsel_bin_base                 k_filter_bin_base's scan for every column of the call: the inflated value blocks of
//                                   LZ4 / Zstd / Snappy pages get their place in the column's share of the staging area
//   k_rsel_sums + k_rsel_rank       unchanged, with cap_rows = offsets_capacity / sizeof(O) - 1;  k_rsel_clear
//   k_rsel_bin_len                  the tile list: a selected lane stores its row's LENGTH to offsets[k + 1]
//   k_rsel_bin_sums + _scan         offsets[1 .. selected] summed in place, in 64 bits, over RSEL_RANK_BLOCKS workgroups per
//                                   column like the rank scan; offsets[0] = 0, values_len, the values_capacity check
//   k_rsel_bin                      the tile list again: a selected lane reads offsets[k] and copies its row's bytes
// A row's place and length, by codec, as the filter finds them (sb_filter_bin.h):
//   Basic (None or staged)          the offset pair from d.src, cut to the values block as filter_bin_basic cuts it
//   OneValue                        d.dict, d.dict_n
//   Dict / Freq                     the tile's indices through u32_tile_to_lds, the entry through k_plan's ent_off as
//                                   expand_binary computes it (the Freq gap behind entry 0 included); an index >= D on a
//                                   SELECTED row raises OutOfSpec (site 410), on any other row it is not looked at
// Both walks keep rsel_tile's early-out: a tile without a selected row returns after two rank lookups, before an offset, an
// index or an entry is loaded.  The length is computed again in the second walk rather than kept: per hit Dict tile that
// is one more u32_tile_to_lds, and nothing is stored between the walks but the offsets themselves.
//
// The rows of a page that is not ok (its parse or plan raised, or its value blocks do not fit the staging share) have no
// tiles or are skipped by them: k_rsel_bin_len gives their selected rows the length 0, so that the scan never reads a word
// nobody wrote.  Selected rows at and behind cap_rows have no offset: their lengths are added to a counter of the column
// (only such a call pays the atomics), so that values_len is what the caller has to allocate also when `offsets` was short.
//
// LOADS STAY INSIDE THEIR BUFFER (the rule at the head of sb_filter_bin.h): bin_move reads a string of n >= 16 bytes in
// 16-byte steps from its first byte and once more at its last 16, shorter ones by two overlapping 8- / 4- / 2-byte moves
// or one byte.  Stores are guarded by the capacities: offsets below cap_rows, bytes below values_capacity.
#pragma once

namespace sb {

// `len` bytes from sp to dp, both at any alignment: the overlapping moves of expand_binary (sb_decode.hip), whose Dict
// branch has the same ladder inline — a copy, so that the decoder's code generation stays what it was; a change to one
// belongs in the other
__device__ __forceinline__ void bin_move(uint8_t* dp, const uint8_t* sp, uint32_t len) {
    if (len >= 16) {
        uint32_t b = 0;
        for (; b + 16 <= len; b += 16) stu128(dp + b, ldu128(sp + b));
        if (b < len) stu128(dp + len - 16, ldu128(sp + len - 16));
    } else if (len >= 8) {
        const uint64_t v0 = ldu64(sp), v1 = ldu64(sp + len - 8);
        stu64(dp, v0);
        stu64(dp + len - 8, v1);
    } else if (len >= 4) {
        const uint32_t v0 = ldu32(sp), v1 = ldu32(sp + len - 4);
        stu32(dp, v0);
        stu32(dp + len - 4, v1);
    } else if (len >= 2) {
        const uint16_t v0 = ldu16(sp), v1 = ldu16(sp + len - 2);
        __builtin_memcpy((gptr)dp, &v0, 2);
        __builtin_memcpy((gptr)(dp + len - 2), &v1, 2);
    } else if (len == 1) {
        *(gptr)dp = ldu8(sp);
    }
}

// entry i of the caller's offsets (aligned to osize)
__device__ __forceinline__ uint64_t bin_off_ld(const SelBin& b, uint64_t i) {
    return b.osize == 4 ? (uint64_t)gld32((const uint32_t*)b.offsets + i) : gld64((const uint64_t*)b.offsets + i);
}
__device__ __forceinline__ void bin_off_st(const SelBin& b, uint64_t i, uint64_t v) {
    if (b.osize == 4) gst32((uint32_t*)b.offsets + i, (uint32_t)v);
    else gst64((uint64_t*)b.offsets + i, v);
}

// where the inflated value blocks go: k_filter_bin_base for every (binary) column of the call
__global__ void __launch_bounds__(64) k_rsel_bin_base(DecodeArgs a) {
    const ColDesc c = a.cols[blockIdx.x];
    if (is_binary(c.ptype)) bin_base_column(a, c);
    bin_base_done(a);
}

// ---- one tile of the list.  COPY false: the length of every selected row to offsets[k + 1] (k_rsel_bin_len); true: its
// bytes to values + offsets[k], and its validity bit (k_rsel_bin)
template <bool COPY>
__device__ void rsel_bin_tile(const DecodeArgs& a, const SelCol* scols, const SelBin* bcols, uint32_t ti, uint32_t* s_a, uint32_t* s_w,
                              uint32_t* s_strip) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;   // (rsel_bin_bad_page)
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    if (!is_binary(c.ptype)) return;
    SelCol s = scols[tt.col];
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    // a tile without a selected row: two rank lookups, and no offset, index or entry is loaded
    if (sel_rank_at(s, t.out_row + lo) == sel_rank_at(s, t.out_row + hi)) return;
    const SelBin b = bcols[tt.col];
    if (!COPY) s.validity = nullptr;   // (the validity bits go with the bytes)
    const SelSink k{s, d.def_bits, t.out_row, s_strip};
    auto put = [&](uint64_t ko, const uint8_t* p, uint32_t len) {
        if constexpr (COPY) {
            if (ko >= s.cap_rows) return;
            const uint64_t o0 = bin_off_ld(b, ko);
            if (o0 + len <= b.values_cap) bin_move(s.values + o0, p, len);
        } else {
            if (ko < s.cap_rows) bin_off_st(b, ko + 1, len);
            else if (len) atomicAdd((unsigned long long*)(b.sums + RSEL_RANK_BLOCKS), (unsigned long long)len);
        }
    };
    if (is_basic(d.codec)) {
        const uint8_t* offs = d.src;
        const uint8_t* vals = d.codec == SB_CODEC_NONE ? d.vbody : c.values + d.val_base;
        const uint64_t vsize = d.vusize;
        const bool o32 = c.ptype == SB_TYPE_BINARY;
        sel_rows(k, lo, hi, [&](uint64_t r, uint64_t ko) {
            uint64_t o0, o1;
            if (o32) {   // (the pair with one load)
                const uint64_t pr = ldu64(offs + r * 4);
                o0 = (uint32_t)pr;
                o1 = pr >> 32;
            } else {
                o0 = ldu64(offs + r * 8);
                o1 = ldu64(offs + r * 8 + 8);
            }
            // offsets that leave the values block are cut to it, as filter_bin_basic cuts them: nothing outside is loaded
            o1 = min(o1, vsize);
            o0 = min(o0, o1);
            put(ko, vals + o0, (uint32_t)(o1 - o0));
        });
    } else if (d.codec == SB_CODEC_ONEVALUE) {
        const uint8_t* v = d.dict;
        const uint32_t len = d.dict_n;
        sel_rows(k, lo, hi, [&](uint64_t, uint64_t ko) { put(ko, v, len); });
    } else if (d.codec == SB_CODEC_DICT || d.codec == SB_CODEC_FREQ) {
        const uint32_t* aux = (const uint32_t*)(a.scratch + t.aux_off);
        const bool freq = d.codec == SB_CODEC_FREQ;
        const uint32_t gap = freq ? 4 + d.vcsize : 0;
        const uint32_t* ent_off = aux + (freq ? 0u : idx_aux_words(d.icodec, d.n_runs, t.num_values));
        U32Stream is{d.isrc, aux, d.icodec, d.n_runs, t.num_values};
        u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
        const uint8_t* dict = d.dict;
        const uint32_t D = d.dict_n;
        bool bad = false;
        sel_rows(k, lo, hi, [&](uint64_t r, uint64_t ko) {
            const uint32_t e = s_a[sidx((int)(r - lo))];
            if (e >= D) {
                bad = true;
                put(ko, dict, 0);
                return;
            }
            const uint64_t pr = ldu64((const uint8_t*)(ent_off + e));   // the entry's offset pair with one load
            const uint32_t eo = (uint32_t)pr;
            put(ko, dict + eo + 8, (uint32_t)(pr >> 32) - eo - 8 - (e == 0 ? gap : 0));
        });
        if (bad && !COPY) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 410);
    } else {   // (k_parse lets no other codec of a binary page through; if one came, its rows would still get a length)
        sel_rows(k, lo, hi, [&](uint64_t, uint64_t ko) { put(ko, nullptr, 0); });
    }
}

// the selected rows of a page that is not ok: length 0
__device__ void rsel_bin_bad_page(const DecodeArgs& a, const SelCol* scols, const SelBin* bcols, uint32_t p, uint32_t* s_strip) {
    if (a.descs[p].ok) return;
    const PageTask t = a.tasks[p];
    if (!is_binary(a.cols[t.col].ptype)) return;
    SelCol s = scols[t.col];
    if (sel_rank_at(s, t.out_row) == sel_rank_at(s, t.out_row + t.num_values)) return;
    const SelBin b = bcols[t.col];
    s.validity = nullptr;
    const SelSink k{s, nullptr, t.out_row, s_strip};
    sel_rows(k, 0, t.num_values, [&](uint64_t, uint64_t ko) {
        if (ko < s.cap_rows) bin_off_st(b, ko + 1, 0);
    });
}

// 17 KB of LDS (the tile's indices): 8 workgroups per CU like k_expand
__global__ void __launch_bounds__(WG) k_rsel_bin_len(DecodeArgs a, const SelCol* scols, const SelBin* bcols) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        rsel_bin_tile<false>(a, scols, bcols, ti, s_a, s_w, nullptr);
        __syncthreads();
    }
    for (uint32_t p = blockIdx.x; p < a.n_pages; p += gridDim.x) rsel_bin_bad_page(a, scols, bcols, p, nullptr);
}
// 18 KB of LDS like k_rsel: the tile's indices and the validity strip
__global__ void __launch_bounds__(WG) k_rsel_bin(DecodeArgs a, const SelCol* scols, const SelBin* bcols) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_strip[WG];
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        rsel_bin_tile<true>(a, scols, bcols, ti, s_a, s_w, s_strip);
        __syncthreads();
    }
}

// ---- lengths -> offsets.  grid (columns, RSEL_RANK_BLOCKS): block y owns offsets[1 + y * per, 1 + (y + 1) * per) of the
// m = min(selected, cap_rows) lengths that were stored
struct BinScanSpan {
    uint64_t m, i0, i1;
};
__device__ __forceinline__ BinScanSpan bin_scan_span(const SelCol& s) {
    const uint64_t selected = gld64(s.rank + (s.rows + 31) / 32);
    const uint64_t m = min(selected, s.cap_rows), per = (m + RSEL_RANK_BLOCKS - 1) / RSEL_RANK_BLOCKS;
    const uint64_t i0 = min(m, blockIdx.y * per);
    return BinScanSpan{m, i0, min(m, i0 + per)};
}
__global__ void __launch_bounds__(WG) k_rsel_bin_sums(const SelCol* scols, const SelBin* bcols) {
    __shared__ uint64_t s_w64[4];
    const SelCol s = scols[blockIdx.x];
    const SelBin b = bcols[blockIdx.x];
    const BinScanSpan sp = bin_scan_span(s);
    uint64_t n = 0;
    for (uint64_t i = sp.i0 + threadIdx.x; i < sp.i1; i += WG) n += bin_off_ld(b, i + 1);
    n = wg_sum64(n, s_w64);
    if (threadIdx.x == 0) gst64(b.sums + blockIdx.y, n);
}
// ... and the running sums on top of the sums of the blocks before.  Block 0 also writes offsets[0] = 0 and has the
// column's total: the values_len result, the values_capacity check (site 510, `page` = the column) and the range of a
// Binary column's 32-bit offsets (OutOfSpec, site 511)
__global__ void __launch_bounds__(WG) k_rsel_bin_scan(const SelCol* scols, const SelBin* bcols, uint64_t* results, Status* st) {
    __shared__ uint64_t s_w64[4];
    const SelCol s = scols[blockIdx.x];
    const SelBin b = bcols[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const BinScanSpan sp = bin_scan_span(s);
    const uint64_t mine = tid < RSEL_RANK_BLOCKS ? gld64(b.sums + tid) : 0;
    uint64_t base = wg_sum64(tid < blockIdx.y ? mine : 0, s_w64);
    if (blockIdx.y == 0) {
        const uint64_t total = wg_sum64(mine, s_w64) + gld64(b.sums + RSEL_RANK_BLOCKS);
        if (tid == 0) {
            bin_off_st(b, 0, 0);
            results[2 * blockIdx.x] = gld64(s.rank + (s.rows + 31) / 32);
            results[2 * blockIdx.x + 1] = total;
            if (total > b.values_cap) raise(st, SB_ERR_INVALID, blockIdx.x, 510);
            else if (b.osize == 4 && total > 0x7FFFFFFFull) raise(st, SB_ERR_OUT_OF_SPEC, blockIdx.x, 511);
        }
    }
    for (uint64_t c0 = sp.i0; c0 < sp.i1; c0 += WG) {
        const uint64_t i = c0 + tid;
        const uint64_t len = i < sp.i1 ? bin_off_ld(b, i + 1) : 0;
        const uint64_t incl = wave_incl_scan64(len);
        __syncthreads();   // the readers of s_w64 of the chunk before (and of the sums above) are done
        if ((tid & 63) == 63) s_w64[tid >> 6] = incl;
        __syncthreads();
        uint64_t pre = incl;
        const uint32_t wv = tid >> 6;
        if (wv > 0) pre += s_w64[0];
        if (wv > 1) pre += s_w64[1];
        if (wv > 2) pre += s_w64[2];
        if (i < sp.i1) bin_off_st(b, i + 1, base + pre);
        base += s_w64[0] + s_w64[1] + s_w64[2] + s_w64[3];
    }
}

// everything behind k_plan and the inflate of the value blocks (a call without a page: the rank, the scan, offsets[0])
void launch_rsel_bin(sb_ctx* ctx, const DecodeArgs& a, const SelLaunch& sl) {
    hipStream_t s = ctx->stream;
    launch_rsel_rank(ctx, sl.scols, a.n_cols, sl.counts, sl.any_nullable);
    const uint32_t grid = std::max<uint32_t>(1u, min(a.n_tiles, TILE_GRID));
    if (a.n_pages) {
        KScope k(ctx, "k_rsel_bin_len");
        k_rsel_bin_len<<<grid, WG, 0, s>>>(a, sl.scols, sl.bcols);
    }
    {
        KScope k(ctx, "k_rsel_bin_scan");
        k_rsel_bin_sums<<<dim3(a.n_cols, RSEL_RANK_BLOCKS), WG, 0, s>>>(sl.scols, sl.bcols);
        k_rsel_bin_scan<<<dim3(a.n_cols, RSEL_RANK_BLOCKS), WG, 0, s>>>(sl.scols, sl.bcols, sl.results, ctx->d_status);
    }
    if (a.n_tiles) {
        KScope k(ctx, "k_rsel_bin");
        k_rsel_bin<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, sl.scols, sl.bcols);
    }
}
void launch_rsel_bin_base(sb_ctx* ctx, const DecodeArgs& a) {
    KScope k(ctx, "k_rsel_bin_base");
    k_rsel_bin_base<<<a.n_cols, 64, 0, ctx->stream>>>(a);
}

}  // namespace sb
