// strawboat-hip: sb_filter_columns_var — ENDS_WITH, CONTAINS and the three NOT_ forms on columns of a binary type (included
// by sb_decode.hip behind sb_filter_bin.h, whose literal, compares and Dict bit table the kernels here share).
//
// The host maps the five ops onto FilterCol.mask bits beside FILTER_MASK_PREFIX (FILTER_MASK_SUFFIX / _SUBSTR / _NOT,
// sb_common.h); a column that carries one of the three new bits (FILTER_MASK_SUB) is served here:
//   Dict, Freq                        k_filter_sub_entries evaluates the predicate once per entry, a lane per entry and a
//                                     plain search, and writes the FINAL bit (negation applied) into the page's bit table
//                                     (bin_dict); the rows are then looked up by k_filter_bin like those of any column
//   Basic (None or staged), OneValue  k_filter_sub.  Prefix and suffix tests are a lane per row.  CONTAINS is
//                                     POSITION-parallel: the tile's rows are one byte range [off[lo], off[hi]) of the values
//                                     block, which the workgroup streams once with 16-byte loads per lane (a wave reads
//                                     1 KiB per instruction); every byte position is tested against the literal's first
//                                     min(len, 8) bytes, and a position that passes finds its row by an upper-bound search
//                                     of the tile's offsets in LDS, checks that the literal fits into the row, compares
//                                     the rest and sets the row's bit in an LDS bitmap, which filter_span then reads.
//                                     The cost follows the bytes, not the rows: a 70 KB value is no lane's own job.
// sub_eval is the definition of every predicate here, per row; the scan computes the same bits for a tile whose offsets
// ascend inside the values block, and a tile whose offsets do not is served per row with filter_bin_basic's cut rule.
//
// LOADS STAY INSIDE THEIR BUFFER.  The scan's 16-byte slots lie on the 16-byte grid of the ADDRESS SPACE; a slot (and the
// 8 bytes behind it that the slot's last positions look into) that lies inside the tile's byte range whole is loaded
// whole, one that straddles the range's first or last byte is loaded byte by byte, the inside bytes only.  A candidate's
// remaining bytes are compared after p + len <= off[r + 1] is known.
#pragma once

namespace sb {

// does the literal (1 <= l.len <= len) occur in the len bytes at v?  A plain search: first byte, then the whole literal
__device__ __forceinline__ bool sub_find(const uint8_t* v, uint32_t len, const BinLit& l) {
    const uint8_t b0 = (uint8_t)l.w0;
    for (uint32_t i = 0; i + l.len <= len; i++)
        if (ldu8(v + i) == b0 && bin_rel_prefix(v + i, l, l.len) == 1u) return true;
    return false;
}
// THE DEFINITION of the predicates of a FILTER_MASK_SUB column, negation applied (the validity is the sink's)
__device__ __forceinline__ bool sub_eval(const uint8_t* v, uint32_t len, const BinLit& l) {
    bool r = false;
    if (len >= l.len) {
        if (l.mask & FILTER_MASK_SUBSTR) r = l.len == 0 || sub_find(v, len, l);
        else r = bin_rel_prefix((l.mask & FILTER_MASK_SUFFIX) ? v + (len - l.len) : v, l, l.len) == 1u;
    }
    return r != ((l.mask & FILTER_MASK_NOT) != 0);
}

// ---- Dict / Freq pages: k_filter_bin_entries for the columns it skips.  grid (pages, FILTER_BIN_EY)
__global__ void __launch_bounds__(WG) k_filter_sub_entries(DecodeArgs a, const FilterCol* fcols) {
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    if (!d.ok || (d.codec != SB_CODEC_DICT && d.codec != SB_CODEC_FREQ)) return;
    const PageTask t = a.tasks[p];
    if (!is_binary(a.cols[t.col].ptype)) return;
    const FilterCol f = fcols[t.col];
    if (f.kind != FK_BYTES || !(f.mask & FILTER_MASK_SUB)) return;
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
            b = sub_eval(d.dict + eo + 8, len, lit);
        }
        const uint64_t m = __ballot(b);
        if ((threadIdx.x & 31) == 0 && e < bd.D) gst32(bd.bits + (e >> 5), ballot_half(m));
    }
}

// ---- plain tiles
// 8 bytes at A + q of the range A .. A + n, the bytes outside it as zero: the inside bytes one by one
__device__ __forceinline__ uint64_t sub_ld_edge(const uint8_t* A, int64_t q, uint32_t n) {
    uint64_t v = 0;
    for (int j = 0; j < 8; j++) {
        const int64_t r = q + j;
        if (r >= 0 && r < (int64_t)n) v |= (uint64_t)ldu8(A + r) << (8 * j);
    }
    return v;
}

constexpr uint32_t SUB_SLOT = 16;   // bytes of the range per lane and step

// The rows of s_off[0 .. rows] (ascending, the last one <= the block's size) whose bytes hold the literal (len >= 1) get
// their bit in s_bits (zeroed by the caller, who also puts the barrier behind this).  By the whole workgroup.
__device__ __forceinline__ void sub_scan(const uint8_t* vals, const uint32_t* s_off, uint32_t rows, const BinLit& lit, uint32_t* s_bits) {
    const uint32_t b0 = s_off[0], n = s_off[rows] - b0;
    if (lit.len > n) return;
    const uint8_t* A = vals + b0;
    const uint32_t mis = (uint32_t)((uintptr_t)A & (SUB_SLOT - 1));
    const uint64_t nslots = ((uint64_t)mis + n + SUB_SLOT - 1) / SUB_SLOT;
    const int64_t last = (int64_t)n - lit.len;   // the last position a match can start at
    const uint64_t lmask = lit.len >= 8 ? ~0ull : (1ull << (8 * lit.len)) - 1;
    const uint64_t w0 = lit.w0 & lmask;
    for (uint64_t s = threadIdx.x; s < nslots; s += WG) {
        const int64_t q = (int64_t)(s * SUB_SLOT) - mis;   // the slot's first byte, from A
        uint64_t x0, x1, x2;
        if (q >= 0 && q + 24 <= (int64_t)n) {
            const u32x4 v = ldu128(A + q);   // (16-byte aligned)
            x0 = v.x | ((uint64_t)v.y << 32);
            x1 = v.z | ((uint64_t)v.w << 32);
            x2 = ldu64(A + q + 16);
        } else {
            x0 = sub_ld_edge(A, q, n);
            x1 = sub_ld_edge(A, q + 8, n);
            x2 = sub_ld_edge(A, q + 16, n);
        }
        uint32_t cand = 0;   // bit i: the literal's first bytes stand at q + i
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint64_t lo = i < 8 ? x0 : x1, hi = i < 8 ? x1 : x2;
            const int sh = 8 * (i & 7);
            const uint64_t w = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
            if (((w ^ w0) & lmask) == 0) cand |= 1u << i;
        }
        uint32_t r_lo = 1, r_hi = 0;   // the byte range (from the block's start) of the row the last match set: its bit is set
        while (cand) {
            const int i = __builtin_ctz(cand);
            cand &= cand - 1;
            const int64_t pq = q + i;
            if (pq < 0 || pq > last) continue;
            const uint32_t p = b0 + (uint32_t)pq;
            if (p >= r_lo && p < r_hi) continue;
            // the last row r with off[r] <= p (rows that are empty are stepped over; off[rows] > p)
            uint32_t l = 0, h = rows;
            while (h - l > 1) {
                const uint32_t m = (l + h) >> 1;
                if (s_off[m] <= p) l = m;
                else h = m;
            }
            const uint32_t end = s_off[l + 1];
            if ((uint64_t)p + lit.len > end) continue;   // (before any further load: every load stays inside the row)
            if (lit.len > 8 && bin_rel_prefix(vals + p, lit, lit.len) != 1u) continue;
            atomicOr(&s_bits[l >> 5], 1u << (l & 31));
            r_lo = s_off[l];
            r_hi = end;
        }
    }
}

// the offsets of rows [lo, hi] of the page into s_off, cut to the block; true (for every lane) when they ascend inside it
template <class O>
__device__ __forceinline__ bool sub_offsets(const uint8_t* offs, uint64_t lo, uint32_t rows, uint32_t vsize, uint32_t* s_off) {
    bool bad = false;
    for (uint32_t i = threadIdx.x; i <= rows; i += WG) {
        uint64_t o;
        if constexpr (sizeof(O) == 4) o = ldu32(offs + (lo + i) * 4);
        else o = ldu64(offs + (lo + i) * 8);
        bad |= o > vsize;
        s_off[i] = (uint32_t)min(o, (uint64_t)vsize);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < rows; i += WG) bad |= s_off[i] > s_off[i + 1];
    return !__syncthreads_or(bad);
}

template <class O>
__device__ __forceinline__ void filter_sub_basic(const FilterSink& k, uint64_t lo, uint64_t hi, const uint8_t* offs, const uint8_t* vals,
                                                 uint32_t vsize, const BinLit& lit, uint32_t* s_off, uint32_t* s_bits) {
#ifndef SB_FILTER_SUB_PER_ROW   // (the build that the scan was measured against: every tile per row)
    if ((lit.mask & FILTER_MASK_SUBSTR) && lit.len) {
        const uint32_t neg = (lit.mask & FILTER_MASK_NOT) ? 1u : 0u;
        const uint32_t rows = (uint32_t)(hi - lo);
        for (uint32_t g = threadIdx.x; g < TILE_ROWS / 32; g += WG) s_bits[g] = 0;
        if (sub_offsets<O>(offs, lo, rows, vsize, s_off)) {
            sub_scan(vals, s_off, rows, lit, s_bits);
            __syncthreads();
            filter_span(k, lo, hi, [&](uint64_t r) { return (uint32_t)tab_bit(s_bits, (uint32_t)(r - lo)) != neg; });
            return;
        }
    }
#endif
    // a lane per row, with filter_bin_basic's cut rule
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
        o1 = min(o1, (uint64_t)vsize);
        o0 = min(o0, o1);
        return sub_eval(vals + o0, (uint32_t)(o1 - o0), lit);
    });
}

__device__ void filter_sub_tile(const DecodeArgs& a, const FilterCol* fcols, uint32_t ti, uint32_t* s_off, uint32_t* s_bits) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok || !(is_basic(d.codec) || d.codec == SB_CODEC_ONEVALUE)) return;   // (Dict, Freq: k_filter_bin)
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    if (!is_binary(c.ptype)) return;
    const FilterCol f = fcols[tt.col];
    if (f.kind != FK_BYTES || !(f.mask & FILTER_MASK_SUB)) return;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint64_t hi = lo + min((uint64_t)TILE_ROWS, t.num_values - lo);
    const FilterSink k{f.sel, d.def_bits, t.out_row, t.num_values, f.combine};
    const BinLit lit = bin_lit(f);
    if (is_basic(d.codec)) {
        const uint8_t* vals = d.codec == SB_CODEC_NONE ? d.vbody : c.values + d.val_base;
        if (c.ptype == SB_TYPE_BINARY) filter_sub_basic<int32_t>(k, lo, hi, d.src, vals, d.vusize, lit, s_off, s_bits);
        else filter_sub_basic<int64_t>(k, lo, hi, d.src, vals, d.vusize, lit, s_off, s_bits);
        return;
    }
    // OneValue: the same scan with a one-row map
    bool v;
#ifndef SB_FILTER_SUB_PER_ROW
    if ((lit.mask & FILTER_MASK_SUBSTR) && lit.len) {
        if (threadIdx.x == 0) {
            s_off[0] = 0;
            s_off[1] = d.dict_n;
            s_bits[0] = 0;
        }
        __syncthreads();
        sub_scan(d.dict, s_off, 1, lit, s_bits);
        __syncthreads();
        v = (s_bits[0] & 1u) != ((lit.mask & FILTER_MASK_NOT) ? 1u : 0u);
    } else
#endif
        v = sub_eval(d.dict, d.dict_n, lit);
    filter_span(k, lo, hi, [&](uint64_t) { return v; });
}

// 16.5 KB of LDS: the tile's offsets and its row bitmap
__global__ void __launch_bounds__(WG) k_filter_sub(DecodeArgs a, const FilterCol* fcols) {
    __shared__ uint32_t s_off[TILE_ROWS + 1];
    __shared__ uint32_t s_bits[TILE_ROWS / 32];
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        filter_sub_tile(a, fcols, ti, s_off, s_bits);
        __syncthreads();
    }
}

// for a call with a FILTER_MASK_SUB column (FilterLaunch.any_sub): the entries before k_filter_bin, which reads their bits
void launch_filter_sub_entries(sb_ctx* ctx, const DecodeArgs& a, const FilterCol* fcols) {
    KScope k(ctx, "k_filter_sub_entries");
    k_filter_sub_entries<<<dim3(a.n_pages, FILTER_BIN_EY), WG, 0, ctx->stream>>>(a, fcols);
}
void launch_filter_sub(sb_ctx* ctx, const DecodeArgs& a, const FilterCol* fcols) {
    if (!a.n_tiles) return;
    KScope k(ctx, "k_filter_sub");
    k_filter_sub<<<min(a.n_tiles, TILE_GRID), WG, 0, ctx->stream>>>(a, fcols);
}

}  // namespace sb
