// strawboat-hip: sb_read_selected — the third sink on the decoder's walks (included by sb_decode.hip behind sb_filter.h).
//
// A read call stores every row, a filter call stores a bit per row; this call stores the rows whose bit is set in a
// selection bitmap, packed: output row k is the column's row at the k-th set bit.  The chain is a read call up to k_plan
// (same tables, k_parse, inflate queues, plan), then
//   k_rsel_sums + k_rsel_rank   bits set below every 32-bit selection word (SelCol.rank) and the column's total, over
//                               RSEL_RANK_BLOCKS workgroups per column: block sums, then each block scans its words on top
//                               of the sums before it.  The total is the `selected` result; the capacity check is made here.
//   k_rsel_clear                zeroes the ceil(selected/32) validity words that the sink assembles with OR
//   k_rsel_rle / k_rsel         the walks of k_expand_rle / k_expand with sel_span as the sink (below)
//   k_rsel_plain                the replay of a call that met a Freq page: the column decoded like a read into the staging
//                               area, compacted from there
// (Binary / LargeBinary columns — sb_read_selected_var — use the rank kernels and sel_rows / sel_validity from here and
// have their own sinks: sb_read_sel_bin.h)
// A rank per WORD (8 bytes per 32 rows, a quarter of a byte per row) rather than a rank per TILE_ROWS block: pages start
// anywhere in a word and RLE chunks anywhere in a tile, so a block rank would leave every lane a popcount over up to 128
// words; with the word rank a lane's output row is one load and one popcount, and a tile's "any row selected?" is two.
#pragma once

namespace sb {

// bits set below row `c` of the column (c <= rows: the entry behind the last word holds the total)
__device__ __forceinline__ uint64_t sel_rank_at(const SelCol& s, uint64_t c) {
    const uint64_t g = c >> 5;
    const uint32_t b = (uint32_t)(c & 31);
    uint64_t r = gld64(s.rank + g);
    if (b) r += (uint64_t)__popc(gld32(s.sel + g) & ((1u << b) - 1));
    return r;
}

__device__ __forceinline__ void sel_store(uint8_t* p, uint64_t v, uint32_t w) {
    switch (w) {
        case 1:
            *(gptr)p = (uint8_t)v;
            break;
        case 2: {
            const uint16_t x = (uint16_t)v;
            __builtin_memcpy((gptr)p, &x, 2);
            break;
        }
        case 4:
            stu32(p, (uint32_t)v);
            break;
        default:
            stu64(p, v);
            break;
    }
}

struct SelSink {
    SelCol s;
    const uint8_t* def_bits;   // the page's validity bits (bit 0 = row 0 of the page) or null: every row valid
    uint64_t out_row;          // the page's first row in the column
    uint32_t* s_strip;         // WG words of LDS: 64 per wave
};

// word `j` (0..2) of the 96-bit value x << sh, sh < 32
__device__ __forceinline__ uint32_t sel_word96(uint64_t x, uint32_t sh, uint32_t j) {
    if (j == 0) return (uint32_t)(x << sh);
    if (j == 1) return (uint32_t)(x >> (32 - sh));
    return sh ? (uint32_t)(x >> (64 - sh)) : 0u;
}

// Rows [lo, hi) of a page, put(row, output row) by every SELECTED lane, by the whole workgroup: a lane per row.  The lane
// loads its row's selection word; its output row is the word's rank plus the set bits below its own.  The selected lanes
// of a wave own consecutive output rows, so what they store is one contiguous range.  Validity (sel_validity) follows when
// the column has a validity buffer.  No barrier inside: a wave without a selected row moves on at once.
//
// sel_validity, the validity half, by the whole wave and without an atomic per row: the selected lanes write their bit to
// popc-compacted positions of the wave's LDS strip, every lane reads back its own position, the ballot of that is the
// <= 64 validity bits of output rows [k0, k0 + n), and lanes 0..2 put the (at most three) words they touch — a word wholly
// inside the range with a plain store, a word shared with another wave, tile or page with atomicOr into the buffer
// k_rsel_clear zeroed (the discipline of sel_put).  Guarded by the capacity of the validity buffer.
__device__ __forceinline__ void sel_validity(const SelSink& k, uint32_t* strip, uint32_t lane, bool on, uint64_t m, uint64_t ko, uint64_t r) {
    uint32_t v = 0;
    if (on) v = k.def_bits ? (uint32_t)(ldu8(k.def_bits + (r >> 3)) >> (r & 7)) & 1u : 1u;
    const uint32_t pos = (uint32_t)__popcll(m & ((1ull << lane) - 1)), n = (uint32_t)__popcll(m);
    const uint64_t k0 = __shfl(ko, __ffsll((long long)m) - 1, 64);
    __builtin_amdgcn_wave_barrier();
    if (on) strip[pos] = v;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const uint64_t bits = __ballot(lane < n && strip[lane] != 0);
    __builtin_amdgcn_wave_barrier();
    if (lane < 3) {
        const uint32_t sh = (uint32_t)(k0 & 31);
        const uint64_t wi = (k0 >> 5) + lane;
        const uint32_t wm = sel_word96(n == 64 ? ~0ull : (1ull << n) - 1, sh, lane), wb = sel_word96(bits, sh, lane);
        if (wm && wi < k.s.cap_words) {
            if (wm == 0xFFFFFFFFu) gst32(k.s.validity + wi, wb);
            else if (wb) atomicOr(k.s.validity + wi, wb);
        }
    }
}
template <class P>
__device__ __forceinline__ void sel_rows(const SelSink& k, uint64_t lo, uint64_t hi, P put) {
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    uint32_t* strip = k.s_strip + (tid & ~63u);
    for (uint64_t g0 = lo; g0 < hi; g0 += WG) {
        const uint64_t r = g0 + tid, c = k.out_row + r;
        const uint32_t b = (uint32_t)(c & 31);
        uint32_t word = 0;
        if (r < hi) word = gld32(k.s.sel + (c >> 5));
        const bool on = (word >> b) & 1u;
        const uint64_t m = __ballot(on);
        if (m == 0) continue;
        uint64_t ko = 0;
        if (on) {
            ko = gld64(k.s.rank + (c >> 5)) + (uint64_t)__popc(word & ((1u << b) - 1));
            put(r, ko);
        }
        if (!k.s.validity) continue;
        sel_validity(k, strip, lane, on, m, ko, r);
    }
}
// the sink of the fixed-width columns: value_of(row), stored with one w-byte store below the capacity of the values buffer
template <class V>
__device__ __forceinline__ void sel_span(const SelSink& k, uint64_t lo, uint64_t hi, V value_of) {
    sel_rows(k, lo, hi, [&](uint64_t r, uint64_t ko) {
        if (ko < k.s.cap_rows) sel_store(k.s.values + ko * k.s.w, value_of(r), k.s.w);
    });
}

// ---- tiles of None / OneValue / Dict / bit-packed / inflated pages (the pages k_expand and k_filter have tiles for)
__device__ void rsel_tile(const DecodeArgs& a, const SelCol* scols, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint32_t* s_strip) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    const SelCol s = scols[tt.col];
    const uint32_t w = c.width;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    // A Freq page asks for the replay whatever the selection, as in filter_tile: k_parse has logged the page for the second
    // decode pass, whose scatter writes through the staging area, and only the replay drops that record (it clears the logs
    // and decodes the column itself: see the head of sb_filter.h).  A page left alone here without the replay would be
    // scattered at the synchronize into a staging area that a later call of the interval may have outgrown and freed.
    if (d.codec == SB_CODEC_FREQ) {
        if (threadIdx.x == 0 && tt.tile == 0) atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
        return;
    }
    // a tile without a selected row: two rank lookups, and no value or index is loaded
    if (sel_rank_at(s, t.out_row + lo) == sel_rank_at(s, t.out_row + hi)) return;
    const SelSink k{s, d.def_bits, t.out_row, s_strip};
    switch (d.codec) {
        case SB_CODEC_NONE: {
            const uint8_t* src = d.src;
            sel_span(k, lo, hi, [&](uint64_t r) { return flt_load(src + r * w, w); });
            break;
        }
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {   // inflated into the staging area, where a read call has the column's values
            const uint8_t* src = c.values + t.out_row * w;
            sel_span(k, lo, hi, [&](uint64_t r) { return flt_load(src + r * w, w); });
            break;
        }
        case SB_CODEC_ONEVALUE: {
            const uint64_t v = flt_load(d.body, w);
            sel_span(k, lo, hi, [&](uint64_t) { return v; });
            break;
        }
        case SB_CODEC_DICT: {
            U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
            u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
            const uint8_t* dict = d.dict;
            const uint32_t D = d.dict_n;
            bool bad = false;
            sel_span(k, lo, hi, [&](uint64_t r) -> uint64_t {   // the row's entry is gathered, as the decoder gathers it
                const uint32_t e = s_a[sidx((int)(r - lo))];
                if (e >= D) {
                    bad = true;
                    return 0;
                }
                return flt_load(dict + (uint64_t)e * w, w);
            });
            if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 400);
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            if (w != 4) break;
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            u32_tile_to_lds(vs, tt.tile, rows, s_a, s_w);
            sel_span(k, lo, hi, [&](uint64_t r) { return (uint64_t)s_a[sidx((int)(r - lo))]; });
            break;
        }
        default:   // (RLE pages of <= 8-byte values have no tiles: k_rsel_rle)
            break;
    }
}

// 18 KB of LDS (k_expand's 17 KB and the validity strip): 8 workgroups per CU like k_expand
__global__ void __launch_bounds__(WG) k_rsel(DecodeArgs a, const SelCol* scols) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint32_t s_strip[WG];
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        rsel_tile(a, scols, ti, s_a, s_w, s_strip);
        __syncthreads();
    }
}

// ---- RLE pages, one workgroup per page (or per part of a long page): rle_page_walk (sb_decode.hip) with this policy.
// The chunk's run values are staged in LDS as the decoder stages them (as 64-bit words, whatever the width: one
// instance of the walk); rows gather their run's value and hand it to sel_span.
struct RleSelect {
    using Rec = uint64_t;
    uint64_t* s_rec;
    SelSink k;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + k.s.w; }
    __device__ __forceinline__ uint64_t load(const uint8_t* v, bool in) const { return in ? flt_load(v, k.s.w) : 0ull; }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        if (sel_rank_at(k.s, k.out_row + lo) == sel_rank_at(k.s, k.out_row + hi)) return;
        sel_span(k, lo, hi, [&](uint64_t r) { return s_rec[A + s_flag[sidx((int)(r - tile_lo))]]; });
    }
};

__global__ void __launch_bounds__(WG) k_rsel_rle(DecodeArgs a, const SelCol* scols) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint64_t s_vals[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint32_t s_strip[WG];
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    const RleSelect pol{s_vals, SelSink{scols[t.col], d.def_bits, t.out_row, s_strip}};
    rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
}

// ---- the rank table.  grid (columns, RSEL_RANK_BLOCKS): block y owns words [y * per, (y + 1) * per)
__device__ __forceinline__ uint32_t rsel_popc(const SelCol& s, uint64_t g, uint64_t nwords) {
    uint32_t v = gld32(s.sel + g);
    if (g == nwords - 1 && (s.rows & 31)) v &= (1u << (s.rows & 31)) - 1;   // bits behind `rows` are ignored
    return (uint32_t)__popc(v);
}
__global__ void __launch_bounds__(WG) k_rsel_sums(const SelCol* scols) {
    __shared__ uint64_t s_w64[4];
    const SelCol s = scols[blockIdx.x];
    const uint64_t nwords = (s.rows + 31) / 32, per = (nwords + RSEL_RANK_BLOCKS - 1) / RSEL_RANK_BLOCKS;
    const uint64_t w0 = min(nwords, blockIdx.y * per), w1 = min(nwords, w0 + per);
    uint64_t n = 0;
    for (uint64_t g = w0 + threadIdx.x; g < w1; g += WG) n += rsel_popc(s, g, nwords);
    n = wg_sum64(n, s_w64);
    if (threadIdx.x == 0) gst64(s.rank + nwords + 1 + blockIdx.y, n);
}
// ... and the ranks on top of the sums of the blocks before.  Block 0 also has the column's total: the `selected` result,
// the entry behind the last word, and the capacity check (site 500, `page` = the column)
__global__ void __launch_bounds__(WG) k_rsel_rank(const SelCol* scols, uint64_t* counts, Status* st) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint32_t s_w[4];
    const SelCol s = scols[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint64_t nwords = (s.rows + 31) / 32, per = (nwords + RSEL_RANK_BLOCKS - 1) / RSEL_RANK_BLOCKS;
    const uint64_t w0 = min(nwords, blockIdx.y * per), w1 = min(nwords, w0 + per);
    const uint64_t mine = tid < RSEL_RANK_BLOCKS ? gld64(s.rank + nwords + 1 + tid) : 0;
    uint64_t base = wg_sum64(tid < blockIdx.y ? mine : 0, s_w64);
    if (blockIdx.y == 0) {
        const uint64_t total = wg_sum64(mine, s_w64);
        if (tid == 0) {
            gst64(s.rank + nwords, total);
            counts[blockIdx.x] = total;
            if (total > s.cap_rows || (s.validity && (total + 31) / 32 > s.cap_words)) raise(st, SB_ERR_INVALID, blockIdx.x, 500);
        }
    }
    for (uint64_t c0 = w0; c0 < w1; c0 += WG) {
        const uint64_t g = c0 + tid;
        const uint32_t p = g < w1 ? rsel_popc(s, g, nwords) : 0;
        const uint32_t incl = wave_incl_scan(p);
        __syncthreads();   // the readers of s_w of the chunk before are done
        if ((tid & 63) == 63) s_w[tid >> 6] = incl;
        __syncthreads();
        uint32_t pre = incl - p;
        const uint32_t wv = tid >> 6;
        if (wv > 0) pre += s_w[0];
        if (wv > 1) pre += s_w[1];
        if (wv > 2) pre += s_w[2];
        if (g < w1) gst64(s.rank + g, base + pre);
        base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    }
}

// the validity words the sink assembles with OR start from zero; this also writes the bits >= selected of the last word
// as 0 (one launch for the call's columns, like k_filter_clear).  Never beyond the capacity given.
__global__ void __launch_bounds__(WG) k_rsel_clear(const SelCol* scols, const uint64_t* counts) {
    const SelCol s = scols[blockIdx.x];
    if (!s.validity) return;
    const uint64_t nwords = min((counts[blockIdx.x] + 31) / 32, s.cap_words);
    for (uint64_t g = (uint64_t)blockIdx.y * WG + threadIdx.x; g < nwords; g += (uint64_t)gridDim.y * WG) gst32(s.validity + g, 0u);
}

// ---- the replay of a call that met a Freq page: the column was decoded like a read (values and validity in the staging
// area, exceptions scattered by the second pass); one launch per column, a workgroup per TILE_ROWS rows
__global__ void __launch_bounds__(WG) k_rsel_plain(const SelCol* scols, uint32_t col, const uint8_t* values, const uint8_t* validity) {
    __shared__ uint32_t s_strip[WG];
    const SelCol s = scols[col];
    const uint64_t lo = (uint64_t)blockIdx.x * TILE_ROWS, hi = min(s.rows, lo + TILE_ROWS);
    if (sel_rank_at(s, lo) == sel_rank_at(s, hi)) return;
    const SelSink k{s, validity, 0, s_strip};
    const uint32_t w = s.w;
    sel_span(k, lo, hi, [&](uint64_t r) { return flt_load(values + r * w, w); });
}

static void launch_rsel_rank(sb_ctx* ctx, const SelCol* scols, uint32_t n_cols, uint64_t* counts, bool any_nullable) {
    hipStream_t s = ctx->stream;
    {
        KScope k(ctx, "k_rsel_rank");
        k_rsel_sums<<<dim3(n_cols, RSEL_RANK_BLOCKS), WG, 0, s>>>(scols);
        k_rsel_rank<<<dim3(n_cols, RSEL_RANK_BLOCKS), WG, 0, s>>>(scols, counts, ctx->d_status);
    }
    if (any_nullable) {
        KScope k(ctx, "k_rsel_clear");
        k_rsel_clear<<<dim3(n_cols, 16), WG, 0, s>>>(scols, counts);
    }
}

void launch_rsel(sb_ctx* ctx, const DecodeArgs& a, const SelLaunch& sl) {
    hipStream_t s = ctx->stream;
    launch_rsel_rank(ctx, sl.scols, a.n_cols, sl.counts, sl.any_nullable);
    {
        KScope k(ctx, "k_rsel_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_rsel_rle<<<dim3(a.n_pages, std::max<uint32_t>(1u, a.rle_parts)), WG, 0, s>>>(a, sl.scols);
    }
    if (a.n_tiles) {
        KScope k(ctx, "k_rsel");
        k_rsel<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, sl.scols);
    }
}

// `rows[i]`, `values[i]`, `validity[i]` (host arrays): the decoded columns of the replay
void launch_rsel_plain(sb_ctx* ctx, const SelCol* scols, uint32_t n_cols, uint64_t* counts, bool any_nullable, const uint64_t* rows,
                       const uint8_t* const* values, const uint8_t* const* validity) {
    launch_rsel_rank(ctx, scols, n_cols, counts, any_nullable);
    KScope k(ctx, "k_rsel_plain");
    for (uint32_t i = 0; i < n_cols; i++)
        if (rows[i]) k_rsel_plain<<<(uint32_t)((rows[i] + TILE_ROWS - 1) / TILE_ROWS), WG, 0, ctx->stream>>>(scols, i, values[i], validity[i]);
}

}  // namespace sb
