// strawboat-hip: sb_topk_columns — the ordering sink on the decoder's walks (included by sb_decode.hip behind
// sb_aggregate_grouped.h; the order keys, the selection helpers and the slot numbering are sb_aggregate.h's).
//
// SELECT ... WHERE ... ORDER BY y [DESC] LIMIT k: of the live rows that are not NaN, the k best by (value, row number) come
// back with their row numbers, and nothing else is stored.  The chain is sb_aggregate_columns' with a sibling per kernel:
//   topk_zero                the slots' headers start from zero (one memset)
//   k_topk_rle / k_topk      the walks of k_agg_rle / k_agg with topk_span as the sink (below)
//   k_topk_finish            one workgroup per column: the bits set below `rows`, the slots' counts summed, and the slots'
//                            records through the same sink once more: the column's k best, as sb_topk_row
//   k_topk_plain             the replay of an interval in which a sink call met a Freq page, from the decoded column
//
// The sink.  A record is { key, row }: key = agg_key(value), complemented for LARGEST, row = the row's number in the
// column.  "Smaller (key, row) wins" is the only comparison there is, and (key, row) is a total order on the candidates,
// since no two have one row: the k best are one set in one sequence, whatever walk, tile, slot or schedule brought them in.
// That is the whole argument for "the same bytes every time"; no order of arrival is ever looked at.
// A workgroup keeps a candidate buffer of TOPK_CAP records in LDS and a bound: the k-th best record it holds, or none
// (all ones, which no candidate reaches: its row would be 2^64 - 1) while it holds fewer than k.  A step is one row per lane.
// A live lane that is no NaN and beats the bound appends its record: its place is its rank among the wave's appending
// lanes (a ballot) behind one LDS integer add per wave.  When a whole further step may no longer fit -- and once before
// that, as soon as k records are held -- the workgroup prunes:
// a bitonic sort of the buffer on the full (key, row) record, the best k kept, the bound set to the k-th.  How many steps
// still fit is counted down in a register, so the barriers that make the buffer's fill a workgroup-uniform fact are paid
// once per refill, not per step.  The lanes count live rows and NaNs in registers, reduced once per slot.
//
// Sizes.  TOPK_CAP = 1024 records = SB_TOPK_MAX_K kept + 3 steps of WG = 256 appended (one row per lane and step: the
// span is not unrolled), a power of two for the sort.  16 bytes per record: 16 KiB, and 24 bytes of fill and bound.
//   kernel          LDS                                                     workgroups per CU (160 KiB)
//   k_topk          17 KiB (k_agg's index tile) + 16 KiB = 33.3 KiB         4
//   k_topk_rle      17 KiB + 8 KiB (k_agg_rle's flags and run values) + 16 KiB = 41.1 KiB   3
//   k_topk_plain    16.1 KiB                                                8 (the 32 waves of a CU)
//   k_topk_finish   16.1 KiB                                                8 (one workgroup per column is launched)
// A slot -- AggCol's numbering: a slot per (page, RLE part), then a slot per tile -- is a header { written, cnt, nans, n }
// and `kmax` records, the call's largest k.  Only the headers are zeroed; a record is read only below its header's n.
// No float is ever added, so there is no float atomic; the only atomics are the integer adds on the buffer's fill in LDS,
// and every write to HBM is a plain vector store.
#pragma once

namespace sb {

constexpr uint32_t TOPK_CAP = 1024;
constexpr uint32_t TOPK_FINISH_STEPS = (TOPK_CAP - TOPK_MAX_K) / WG;   // steps that fit behind any prune
static_assert((TOPK_CAP & (TOPK_CAP - 1)) == 0 && TOPK_CAP >= TOPK_MAX_K + WG, "a power of two that holds k records and a step");
static_assert(TOPK_MAX_K <= WG, "k_topk_finish takes a slot's records in one step");

struct TopkBuf {   // LDS
    uint64_t key[TOPK_CAP], row[TOPK_CAP];
    uint64_t bkey, brow;   // the bound
    uint32_t n, pad;       // records held
};

struct TopkSink {
    const uint32_t* sel;       // as in AggSink
    const uint8_t* def_bits;
    uint64_t out_row;
    TopkBuf* b;
    uint32_t k;
    uint64_t flip;             // ~0 for LARGEST: the key is complemented
    // the lane's own
    uint64_t cnt = 0, nans = 0;
    uint64_t bkey = ~0ull, brow = ~0ull;   // the bound, as of the last prune
    uint32_t room = 1;                     // steps that fit whatever they append (the same number in every lane); the
                                           // empty buffer has room for more, and is looked at after one: topk_reserve
};

__device__ __forceinline__ bool topk_less(uint64_t ka, uint64_t ra, uint64_t kb, uint64_t rb) { return ka < kb || (ka == kb && ra < rb); }
__device__ __forceinline__ bool topk_is_nan(uint32_t kind, uint64_t raw) {
    if (kind == FK_F32) return ((uint32_t)raw & 0x7FFFFFFFu) > 0x7F800000u;
    if (kind == FK_F64) return (raw & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull;
    return false;
}

// an empty buffer without a bound; by the whole workgroup, a barrier behind it
__device__ __forceinline__ TopkSink topk_begin(TopkBuf* b, const uint32_t* sel, const uint8_t* def_bits, uint64_t out_row, const TopkCol& tc) {
    __syncthreads();   // (the buffer's last readers are done)
    if (threadIdx.x == 0) {
        b->n = 0;
        b->bkey = b->brow = ~0ull;
    }
    __syncthreads();
    return TopkSink{sel, def_bits, out_row, b, tc.k, tc.largest ? ~0ull : 0ull};
}

// The n records of the buffer sorted, the best min(n, k) kept (that number is returned), the bound set if there are k.
// By the whole workgroup, between two barriers of its own; the caller has one between the last append and this, and every
// thread passes the n it read behind that barrier.
__device__ __noinline__ uint32_t topk_prune(TopkBuf* b, uint32_t n, uint32_t k) {
    uint32_t P = 2;
    while (P < n) P <<= 1;
    for (uint32_t i = n + threadIdx.x; i < P; i += WG) b->key[i] = b->row[i] = ~0ull;   // behind every record
    __syncthreads();
    for (uint32_t size = 2; size <= P; size <<= 1)
        for (uint32_t stride = size >> 1; stride; stride >>= 1) {
            for (uint32_t i = threadIdx.x; i < P / 2; i += WG) {
                const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t ka = b->key[lo], ra = b->row[lo], kb = b->key[hi], rb = b->row[hi];
                if (topk_less(kb, rb, ka, ra) == up) {
                    b->key[lo] = kb, b->row[lo] = rb;
                    b->key[hi] = ka, b->row[hi] = ra;
                }
            }
            __syncthreads();
        }
    const uint32_t kept = min(n, k);
    if (threadIdx.x == 0) {
        b->n = kept;
        if (n >= k) b->bkey = b->key[k - 1], b->brow = b->row[k - 1];
    }
    __syncthreads();
    return kept;
}

// Room for a further step, by the whole workgroup.  Nothing happens while the count says so.  The buffer is pruned when a
// step may no longer fit -- and once before that, as soon as it holds k records: the first bound is what turns most rows
// of a tile away, and the sort that finds it is the shorter the earlier it comes.
__device__ __forceinline__ void topk_reserve(TopkSink& s) {
    if (s.room) return;
    __syncthreads();   // the appends so far are in
    uint32_t n = s.b->n;
    __syncthreads();   // ... and every thread has read the fill before a faster wave's next append moves it
    const bool unbound = (s.bkey & s.brow) == ~0ull;
    if (TOPK_CAP - n < WG || (unbound && n >= s.k)) {
        n = topk_prune(s.b, n, s.k);
        s.bkey = s.b->bkey;   // (changes in topk_prune alone, whose last barrier is behind us)
        s.brow = s.b->brow;
    }
    s.room = (TOPK_CAP - n) / WG;
}

// One step: every lane of the workgroup calls it, with `on` for a candidate.  Reserved before.
__device__ __forceinline__ void topk_offer(TopkSink& s, bool on, uint64_t key, uint64_t row) {
    on = on && topk_less(key, row, s.bkey, s.brow);
    const uint64_t m = __ballot(on);
    if (m) {
        const uint32_t lane = threadIdx.x & 63;
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(&s.b->n, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, 0, 64);
        if (on) {
            const uint32_t i = base + (uint32_t)__popcll(m & ((1ull << lane) - 1));
            s.b->key[i] = key;
            s.b->row[i] = row;
        }
    }
    s.room--;
}

// The ordering counterpart of agg_span: rows [lo, hi) of a page by the whole workgroup, a lane per row and the same number
// of steps for every lane.  value_of(row, raw) gives a live row's value, or false for a row that has none (a Dict index
// beyond the dictionary: the caller raises).
template <class V>
__device__ __forceinline__ void topk_span(TopkSink& s, uint32_t kind, uint32_t w, uint64_t lo, uint64_t hi, V value_of) {
    for (uint64_t base = lo; base < hi; base += WG) {
        topk_reserve(s);
        const uint64_t r = base + threadIdx.x, c = s.out_row + r;
        bool on = r < hi;
        if (on && s.sel) on = (gld32(s.sel + (c >> 5)) >> (uint32_t)(c & 31)) & 1u;
        if (on && s.def_bits) on = (ldu8(s.def_bits + (r >> 3)) >> (uint32_t)(r & 7)) & 1u;
        uint64_t raw = 0;
        if (on) on = value_of(r, raw);
        if (on) {
            s.cnt++;
            if (topk_is_nan(kind, raw)) {
                s.nans++;
                on = false;
            }
        }
        topk_offer(s, on, agg_key(kind, w, raw) ^ s.flip, c);
    }
}

// The workgroup's best k into `slot`, with its counts; by the whole workgroup, barriers inside.
__device__ __forceinline__ void topk_store(TopkSink& s, const TopkLaunch& tl, uint64_t slot, uint64_t* s_w64) {
    __syncthreads();
    uint32_t n = s.b->n;
    if (n > s.k) n = topk_prune(s.b, n, s.k);
    TopkRec* out = tl.recs + slot * tl.kmax;
    for (uint32_t i = threadIdx.x; i < n; i += WG) out[i] = TopkRec{s.b->key[i], s.b->row[i]};
    const uint64_t cnt = wg_sum64(s.cnt, s_w64);
    const uint64_t nans = wg_sum64(s.nans, s_w64);
    if (threadIdx.x == 0) tl.heads[slot] = TopkHead{1, cnt, nans, n};
}

// ---- tiles of None / OneValue / Dict / bit-packed / inflated pages: agg_tile with the ordering sink
__device__ void topk_tile(const DecodeArgs& a, const TopkLaunch& tl, uint32_t ti, uint32_t* s_a, uint32_t* s_w, TopkBuf* s_t, uint64_t* s_w64) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    const AggCol g = tl.acols[tt.col];
    const uint32_t w = c.width, kind = g.kind;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    // a Freq page asks for the replay whatever the selection, as in agg_tile
    if (d.codec == SB_CODEC_FREQ) {
        if (threadIdx.x == 0 && tt.tile == 0) atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
        return;
    }
    // a tile without a selected row: no value and no index is loaded, and its slot stays unwritten
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) return;
    TopkSink s = topk_begin(s_t, g.sel, d.def_bits, t.out_row, tl.tcols[tt.col]);
    switch (d.codec) {
        case SB_CODEC_NONE: {
            const uint8_t* src = d.src;
            topk_span(s, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = flt_load(src + r * w, w), true; });
            break;
        }
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {   // inflated into the staging area
            const uint8_t* src = c.values + t.out_row * w;
            topk_span(s, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = flt_load(src + r * w, w), true; });
            break;
        }
        case SB_CODEC_ONEVALUE: {   // one load for the page; behind the first prune the bound is (the value, its k-th live row)
            const uint64_t one = flt_load(d.body, w);
            topk_span(s, kind, w, lo, hi, [&](uint64_t, uint64_t& raw) { return raw = one, true; });
            break;
        }
        case SB_CODEC_DICT: {
            U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
            u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
            const uint8_t* dict = d.dict;
            const uint32_t D = d.dict_n;
            bool bad = false;
            topk_span(s, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) {
                const uint32_t e = s_a[sidx((int)(r - lo))];
                if (e >= D) {
                    bad = true;
                    return false;
                }
                raw = flt_load(dict + (uint64_t)e * w, w);
                return true;
            });
            if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 400);
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            if (w != 4) break;
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            u32_tile_to_lds(vs, tt.tile, rows, s_a, s_w);
            topk_span(s, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = (uint64_t)s_a[sidx((int)(r - lo))], true; });
            break;
        }
        default:   // (RLE pages of <= 8-byte values have no tiles: k_topk_rle)
            return;
    }
    topk_store(s, tl, tl.tile_base + t.first_tile + tt.tile, s_w64);
}

__global__ void __launch_bounds__(WG) k_topk(DecodeArgs a, TopkLaunch tl) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ TopkBuf s_t;
    const uint32_t count = a.job_counts[2];
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        topk_tile(a, tl, ti, s_a, s_w, &s_t, s_w64);
        __syncthreads();
    }
}

// ---- RLE pages: rle_page_walk with this policy (RleAggregate's staging of the run values).  The buffer and the bound live
// for the whole page part: one slot.
struct RleTopk {
    using Rec = uint64_t;
    uint64_t* s_rec;
    TopkSink* k;
    uint32_t kind, w;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + w; }
    __device__ __forceinline__ uint64_t load(const uint8_t* v, bool in) const { return in ? flt_load(v, w) : 0ull; }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        topk_span(*k, kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = s_rec[A + s_flag[sidx((int)(r - tile_lo))]], true; });
    }
};

__global__ void __launch_bounds__(WG) k_topk_rle(DecodeArgs a, TopkLaunch tl) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint64_t s_vals[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ TopkBuf s_t;
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    const AggCol g = tl.acols[t.col];
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    TopkSink s = topk_begin(&s_t, g.sel, d.def_bits, t.out_row, tl.tcols[t.col]);
    const RleTopk pol{s_vals, &s, g.kind, c.width};
    rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
    topk_store(s, tl, (uint64_t)p * parts + part, s_w64);
}

// ---- one workgroup per column: `selected` as k_agg_finish counts it, the counts of the column's slots, and their
// records -- page slots first, then tile slots; WG / (k rounded up to a power of two) slots per step, a lane per record,
// TOPK_FINISH_STEPS steps loaded at once -- through the sink.  The result: { selected, count, nans, found, 0 .. } in 8
// words, then k entries of sb_topk_row, zeros behind `found`.
__global__ void __launch_bounds__(WG) k_topk_finish(TopkLaunch tl, uint64_t* results) {
    __shared__ uint64_t s_w64[4];
    __shared__ TopkBuf s_t;
    const AggCol g = tl.acols[blockIdx.x];
    const TopkCol tc = tl.tcols[blockIdx.x];
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
    TopkSink s = topk_begin(&s_t, nullptr, nullptr, 0, tc);
    uint32_t kp = 1;
    while (kp < tc.k) kp <<= 1;
    const uint32_t per = WG / kp, sub = threadIdx.x / kp, ri = threadIdx.x & (kp - 1);
    const uint64_t total = g.page_slots + g.tile_slots;
    constexpr uint32_t U = TOPK_FINISH_STEPS;
    for (uint64_t j0 = 0; j0 < total;) {
        topk_reserve(s);
        const uint32_t steps = min(s.room, U);   // as many steps as fit, their loads issued together
        uint64_t slot[U];
        uint32_t n[U];
        TopkRec rec[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            const uint64_t j = j0 + (uint64_t)u * per + sub;
            slot[u] = j < g.page_slots ? g.page_slot0 + j : g.tile_slot0 + (j - g.page_slots);
            TopkHead h{0, 0, 0, 0};
            if (u < steps && j < total) h = tl.heads[slot[u]];
            n[u] = h.written ? (uint32_t)h.n : 0u;
            if (h.written && ri == 0) s.cnt += h.cnt, s.nans += h.nans;
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            rec[u] = TopkRec{0, 0};
            if (ri < n[u]) rec[u] = tl.recs[slot[u] * tl.kmax + ri];
        }
#pragma unroll
        for (uint32_t u = 0; u < U; u++)
            if (u < steps) topk_offer(s, ri < n[u], rec[u].key, rec[u].row);
        j0 += (uint64_t)steps * per;
    }
    __syncthreads();
    const uint32_t found = topk_prune(&s_t, s_t.n, tc.k);   // (sorted also where nothing has to go)
    const uint64_t cnt = wg_sum64(s.cnt, s_w64);
    const uint64_t nans = wg_sum64(s.nans, s_w64);
    uint64_t* r = results + (uint64_t)blockIdx.x * topk_result_words(tl.kmax);
    if (threadIdx.x == 0) {
        r[0] = nsel, r[1] = cnt, r[2] = nans, r[3] = found;
        r[4] = r[5] = r[6] = r[7] = 0;
    }
    for (uint32_t i = threadIdx.x; i < tc.k; i += WG) {
        const bool in = i < found;
        r[8 + 2 * i] = in ? s_t.row[i] : 0;
        r[8 + 2 * i + 1] = in ? agg_unkey(g.kind, g.w, s_t.key[i] ^ s.flip) : 0;
    }
}

// ---- the replay of an interval in which a sink call met a Freq page: the column was decoded like a read (k_agg_plain);
// one launch per column, a workgroup and a slot per TILE_ROWS rows
__global__ void __launch_bounds__(WG) k_topk_plain(TopkLaunch tl, uint32_t col, const uint8_t* values, const uint8_t* validity) {
    __shared__ uint64_t s_w64[4];
    __shared__ TopkBuf s_t;
    const AggCol g = tl.acols[col];
    const uint64_t lo = (uint64_t)blockIdx.x * TILE_ROWS, hi = min(g.rows, lo + TILE_ROWS);
    if (!agg_any_selected(g.sel, lo, hi)) return;
    TopkSink s = topk_begin(&s_t, g.sel, validity, 0, tl.tcols[col]);
    const uint32_t w = g.w;
    topk_span(s, g.kind, w, lo, hi, [&](uint64_t r, uint64_t& raw) { return raw = flt_load(values + r * w, w), true; });
    topk_store(s, tl, g.tile_slot0 + blockIdx.x, s_w64);
}

// the headers start from zero; timed under a name of its own
void launch_topk_zero(sb_ctx* ctx, const TopkLaunch& tl) {
    KScope k(ctx, "topk_zero(memset)");
    if (tl.slots) (void)hipMemsetAsync(tl.heads, 0, (size_t)tl.slots * sizeof(TopkHead), ctx->stream);
}

void launch_topk(sb_ctx* ctx, const DecodeArgs& a, const TopkLaunch& tl) {
    hipStream_t s = ctx->stream;
    {
        KScope k(ctx, "k_topk_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_topk_rle<<<dim3(a.n_pages, std::max<uint32_t>(1u, a.rle_parts)), WG, 0, s>>>(a, tl);
    }
    if (a.n_tiles) {
        KScope k(ctx, "k_topk");
        k_topk<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, tl);
    }
}

void launch_topk_finish(sb_ctx* ctx, const TopkLaunch& tl, uint64_t* results, uint32_t n_cols) {
    KScope k(ctx, "k_topk_finish");
    k_topk_finish<<<n_cols, WG, 0, ctx->stream>>>(tl, results);
}

// `rows[i]`, `values[i]`, `validity[i]` (host arrays): the decoded columns of the replay
void launch_topk_plain(sb_ctx* ctx, const TopkLaunch& tl, uint32_t n_cols, const uint64_t* rows, const uint8_t* const* values,
                       const uint8_t* const* validity) {
    KScope k(ctx, "k_topk_plain");
    for (uint32_t i = 0; i < n_cols; i++)
        if (rows[i]) k_topk_plain<<<(uint32_t)((rows[i] + TILE_ROWS - 1) / TILE_ROWS), WG, 0, ctx->stream>>>(tl, i, values[i], validity[i]);
}

}  // namespace sb
