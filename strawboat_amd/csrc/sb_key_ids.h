// strawboat-hip: sb_key_ids — distinct keys and dense group ids of an integer key column (included by sb_decode.hip behind
// sb_topk.h; the selection helpers are sb_aggregate.h's, the order keys and the search sb_common.h's: in_key, key_lower_bound).
//
// GROUP BY k / SELECT DISTINCT k WHERE ...: the pages of a key column and a selection bitmap (or none) go in; the sorted
// distinct values of the live rows come back on the host, and every row gets the position of its value among them (all
// ones for a row that is not live).  The chain is a read call up to k_plan, then three phases on the stream:
//   key_zero                    the columns' states and tables start from zero (one memset)
//   1. collect   k_key_collect_rle / k_key_collect   the walks of k_agg_rle / k_agg: the order keys of the live rows into
//                               the column's table
//                k_key_collect_plain                 the Freq replay, from the decoded column
//   2. finish    k_key_finish   one workgroup per column: the table's keys sorted in LDS, stored for phase 3 and, as value
//                               bytes, into the result record with selected / count / n_keys / overflow
//   3. assign    k_key_assign_rle / k_key_assign / k_key_assign_plain   the same walks again over the pages that are parsed,
//                               inflated and planned already: key_lower_bound over the column's keys in LDS, one id per row
//
// The distinct set.  Two levels, and no global atomic per row:
//   * a workgroup keeps the keys it has met in an LDS set (KEY_SET_SLOTS slots, linear probing, 0 = empty).  A row probes
//     it with LDS loads; only a key that is new to the workgroup takes an LDS compare-and-swap, and only such a key goes on
//     to the global table.  A lane whose key is its lower neighbour's is dropped before either (one shuffle).  The set
//     lives as long as the workgroup stays on one column: the tiles of k_key_collect, a page part of the RLE walk.
//   * the column's table in the call's scratch (KeyCol): probed with relaxed agent-scope loads, a 64-bit compare-and-swap
//     only on an empty slot.  A lane that wins a slot counts it (KeyState.inserted); the count passing max_keys raises
//     KeyState.overflow, which every step looks at first: from then on rows are counted and nothing is inserted, so neither
//     level fills up and no probe sequence is longer than its table.
//   The order key 0 is the empty slot's value and is kept as a flag (KeyState.has_zero).  k_key_finish counts the table's
//   keys and the flag itself: `overflow` is exact, the early flag only ends the work sooner.
// Candidates are fewer than rows where the page allows it: a Dict page of up to FILTER_DICT_BITS entries marks the entries
// its live rows point at in an LDS bit table and offers the marked entries (an entry no live row points at is no key);
// a OneValue tile offers one key if it has a live row; an RLE run is converted to its key once (RleKeyCollect::load) and
// offered by at most one lane per wave and unbroken stretch of live rows.  A tile without a selected row loads no value.
// The ids are a function of the sorted keys alone, so the same call gives the same bytes whatever the schedule.
//
// LDS:  k_key_collect      17 KiB index tile + 1 KiB bit table + 16 KiB set = 35120 B       4 workgroups per CU (160 KiB)
//       k_key_collect_rle  17 KiB flags + 8 KiB run keys + 16 KiB set = 42288 B             3
//       k_key_collect_plain 16672 B                                                         8 (the 32 waves of a CU)
//       k_key_finish       8232 B                                                           (one workgroup per column)
//       k_key_assign       17 KiB index tile + 16 KiB id table + 8 KiB keys = 42256 B       3
//       k_key_assign_rle   17 KiB flags + 4 KiB run ids + 8 KiB keys = 29744 B              4 (by its 106 VGPRs; LDS allows 5)
//       k_key_assign_plain 8192 B                                                           8
// (DESIGN 4i has the registers, and what the probe measured)
#pragma once

namespace sb {

constexpr uint32_t KEY_SET_SLOTS = 2048;   // the workgroup's set: at most max_keys + a step's WG keys are ever in it
static_assert(KEY_SET_SLOTS >= KEY_MAX_KEYS + 2 * WG && (KEY_SET_SLOTS & (KEY_SET_SLOTS - 1)) == 0, "never full; a power of two");

__device__ __forceinline__ uint32_t key_hash(uint64_t key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 40); }
__device__ __forceinline__ uint32_t key_over(const KeyState* st) {
    return __hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct KeySink {
    const uint32_t* sel;       // as in AggSink
    const uint8_t* def_bits;
    uint64_t out_row;
    uint64_t* set;             // LDS, KEY_SET_SLOTS
    KeyState* st;
    uint64_t* tab;             // the column's table
    uint32_t mask, max_keys;
    // the lane's own
    uint64_t cnt = 0;
    uint32_t zero = 0;
};
__device__ __forceinline__ KeySink key_sink(const KeyLaunch& kl, uint32_t col, uint64_t* set, const uint32_t* sel, const uint8_t* def_bits, uint64_t out_row) {
    const KeyCol kc = kl.kcols[col];
    return KeySink{sel, def_bits, out_row, set, kl.st + col, kl.tabs + kc.tab0, kc.tab_mask, kc.max_keys};
}
// the set empty, by the whole workgroup; the caller's barrier follows
__device__ __forceinline__ void key_set_clear(uint64_t* set) {
    for (uint32_t i = threadIdx.x; i < KEY_SET_SLOTS; i += WG) set[i] = 0;
}

// true: the key is new to the workgroup and this lane put it in (a set that is full says so too: the table decides then)
__device__ __forceinline__ bool key_set_put(uint64_t* set, uint64_t key) {
    uint32_t h = key_hash(key) & (KEY_SET_SLOTS - 1);
    for (uint32_t i = 0; i < KEY_SET_SLOTS; i++, h = (h + 1) & (KEY_SET_SLOTS - 1)) {
        uint64_t v = set[h];
        if (v == key) return false;
        if (v == 0) {
            v = atomicCAS((unsigned long long*)&set[h], 0ull, (unsigned long long)key);
            if (v == 0) return true;
            if (v == key) return false;
        }
    }
    return true;
}
// the key into the column's table: loads until an empty slot, one compare-and-swap there
__device__ __forceinline__ void key_tab_put(const KeySink& s, uint64_t key) {
    uint32_t h = key_hash(key) & s.mask;
    for (uint32_t i = 0; i <= s.mask; i++, h = (h + 1) & s.mask) {
        uint64_t v = __hip_atomic_load(s.tab + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == key) return;
        if (v == 0) {
            v = atomicCAS((unsigned long long*)(s.tab + h), 0ull, (unsigned long long)key);
            if (v == 0) {
                if (atomicAdd(&s.st->inserted, 1u) >= s.max_keys) __hip_atomic_store(&s.st->overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            if (v == key) return;
        }
    }
    __hip_atomic_store(&s.st->overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // no slot left: more than max_keys keys
}
// One step: every lane of the wave calls it, `on` for a candidate.
__device__ __forceinline__ void key_offer(KeySink& s, bool on, uint64_t key) {
    const uint64_t pk = __shfl_up(key, 1, 64);
    const int pon = __shfl_up((int)on, 1, 64);
    if (on && (threadIdx.x & 63) && pon && pk == key) on = false;   // my lower neighbour offers it
    if (!on) return;
    if (key == 0) {
        s.zero = 1;
        return;
    }
    if (key_set_put(s.set, key)) key_tab_put(s, key);
}

// The collecting counterpart of agg_span: rows [lo, hi) of a page by the whole workgroup, a lane per row and the same
// number of steps for every lane.  key_of(row) gives a live row's order key.  Behind the overflow the rows are counted only.
template <class V>
__device__ __forceinline__ void key_span(KeySink& s, uint64_t lo, uint64_t hi, V key_of) {
    for (uint64_t base = lo; base < hi; base += WG) {
        const uint64_t r = base + threadIdx.x, c = s.out_row + r;
        bool on = r < hi;
        if (on && s.sel) on = (gld32(s.sel + (c >> 5)) >> (uint32_t)(c & 31)) & 1u;
        if (on && s.def_bits) on = (ldu8(s.def_bits + (r >> 3)) >> (uint32_t)(r & 7)) & 1u;
        if (on) s.cnt++;
        if (key_over(s.st)) on = false;
        uint64_t key = 0;
        if (on) key = key_of(r);
        key_offer(s, on, key);
    }
}
// the live rows of [lo, hi) counted, nothing offered
__device__ __forceinline__ void key_count(KeySink& s, uint64_t lo, uint64_t hi) {
    agg_rows(AggSink{s.sel, s.def_bits, s.out_row}, lo, hi, [&](uint64_t) { s.cnt++; });
}
// The end of a tile or page part: the lanes' counts and zero flags into the column's state; by the whole workgroup.
__device__ __forceinline__ void key_store(KeySink& s, uint64_t* s_w64) {
    const uint64_t cnt = wg_sum64(s.cnt, s_w64);
    const int zero = __syncthreads_or((int)s.zero);
    if (threadIdx.x == 0) {
        if (cnt) atomicAdd((unsigned long long*)&s.st->count, (unsigned long long)cnt);
        if (zero) s.st->has_zero = 1;   // (read by k_key_finish, a later kernel)
    }
    s.cnt = 0;
    s.zero = 0;
}

// ---- phase 1, tiles of None / OneValue / Dict / bit-packed / inflated pages.  `owner` is the column whose keys the set holds.
__device__ void key_collect_tile(const DecodeArgs& a, const KeyLaunch& kl, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint32_t* s_tab, uint64_t* s_set,
                                 uint64_t* s_w64, uint32_t* owner) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    const AggCol g = kl.acols[tt.col];
    const uint32_t w = c.width, kind = g.kind;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    // a Freq page asks for the replay whatever the selection, as in agg_tile
    if (d.codec == SB_CODEC_FREQ) {
        if (threadIdx.x == 0 && tt.tile == 0) atomicOr(&a.status->kinds, KIND_REPLAY | KIND_FILTER_FREQ);
        return;
    }
    // a tile without a selected row: no value and no index is loaded
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) return;
    if (*owner != tt.col) {   // (the same for every lane: the tile's column)
        __syncthreads();
        key_set_clear(s_set);
        *owner = tt.col;
        __syncthreads();
    }
    KeySink s = key_sink(kl, tt.col, s_set, g.sel, d.def_bits, t.out_row);
    switch (d.codec) {
        case SB_CODEC_NONE: {
            const uint8_t* src = d.src;
            key_span(s, lo, hi, [&](uint64_t r) { return in_key(kind, w, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {   // inflated into the staging area
            const uint8_t* src = c.values + t.out_row * w;
            key_span(s, lo, hi, [&](uint64_t r) { return in_key(kind, w, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_ONEVALUE: {   // one candidate for the tile, if a row of it is live
            key_count(s, lo, hi);
            const bool any = __syncthreads_or(s.cnt != 0) != 0;
            const bool on = any && threadIdx.x == 0 && !key_over(s.st);
            key_offer(s, on, on ? in_key(kind, w, flt_load(d.body, w)) : 0ull);
            break;
        }
        case SB_CODEC_DICT: {
            U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
            u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
            const uint8_t* dict = d.dict;
            const uint32_t D = d.dict_n;
            bool bad = false;
            if (D <= FILTER_DICT_BITS) {   // the entries the live rows point at are marked, the marked entries offered
                for (uint32_t i = threadIdx.x; i < (D + 31) / 32; i += WG) s_tab[i] = 0;
                __syncthreads();
                agg_rows(AggSink{s.sel, s.def_bits, s.out_row}, lo, hi, [&](uint64_t r) {
                    s.cnt++;
                    const uint32_t e = s_a[sidx((int)(r - lo))];
                    if (e >= D) bad = true;
                    else atomicOr(&s_tab[e >> 5], 1u << (e & 31));
                });
                __syncthreads();
                for (uint32_t e0 = 0; e0 < D; e0 += WG) {
                    const uint32_t e = e0 + threadIdx.x;
                    const bool on = e < D && tab_bit(s_tab, e) && !key_over(s.st);
                    key_offer(s, on, on ? in_key(kind, w, flt_load(dict + (uint64_t)e * w, w)) : 0ull);
                }
            } else {
                key_span(s, lo, hi, [&](uint64_t r) {
                    uint32_t e = s_a[sidx((int)(r - lo))];
                    if (e >= D) bad = true, e = 0;   // (raised below; entry 0 is inside the dictionary)
                    return in_key(kind, w, flt_load(dict + (uint64_t)e * w, w));
                });
            }
            if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 400);
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            if (w != 4) break;
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            u32_tile_to_lds(vs, tt.tile, rows, s_a, s_w);
            key_span(s, lo, hi, [&](uint64_t r) { return in_key(kind, w, (uint64_t)s_a[sidx((int)(r - lo))]); });
            break;
        }
        default:   // (RLE pages of <= 8-byte values have no tiles: k_key_collect_rle)
            return;
    }
    key_store(s, s_w64);
}

__global__ void __launch_bounds__(WG) k_key_collect(DecodeArgs a, KeyLaunch kl) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint32_t s_tab[FILTER_DICT_BITS / 32];
    __shared__ uint64_t s_set[KEY_SET_SLOTS];
    const uint32_t count = a.job_counts[2];
    uint32_t owner = 0xFFFFFFFFu;
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        key_collect_tile(a, kl, ti, s_a, s_w, s_tab, s_set, s_w64, &owner);
        __syncthreads();
    }
}

// ---- phase 1, RLE pages: rle_page_walk with this policy.  A run is its order key, converted once; the set lives for the
// whole page part.
struct RleKeyCollect {
    using Rec = uint64_t;
    uint64_t* s_rec;
    KeySink* k;
    uint32_t kind, w;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + w; }
    __device__ __forceinline__ uint64_t load(const uint8_t* v, bool in) const { return in ? in_key(kind, w, flt_load(v, w)) : 0ull; }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        key_span(*k, lo, hi, [&](uint64_t r) { return s_rec[A + s_flag[sidx((int)(r - tile_lo))]]; });
    }
};

__global__ void __launch_bounds__(WG) k_key_collect_rle(DecodeArgs a, KeyLaunch kl) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint64_t s_vals[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_set[KEY_SET_SLOTS];
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    const AggCol g = kl.acols[t.col];
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    key_set_clear(s_set);
    __syncthreads();
    KeySink s = key_sink(kl, t.col, s_set, g.sel, d.def_bits, t.out_row);
    const RleKeyCollect pol{s_vals, &s, g.kind, c.width};
    rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
    key_store(s, s_w64);
}

// ---- phase 1, the replay of an interval in which a sink call met a Freq page: the column was decoded like a read; one
// launch per column, a workgroup per TILE_ROWS rows
__global__ void __launch_bounds__(WG) k_key_collect_plain(KeyLaunch kl, uint32_t col, const uint8_t* values, const uint8_t* validity) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_set[KEY_SET_SLOTS];
    const AggCol g = kl.acols[col];
    const uint64_t lo = (uint64_t)blockIdx.x * TILE_ROWS, hi = min(g.rows, lo + TILE_ROWS);
    if (!agg_any_selected(g.sel, lo, hi)) return;
    key_set_clear(s_set);
    __syncthreads();
    KeySink s = key_sink(kl, col, s_set, g.sel, validity, 0);
    const uint32_t w = g.w, kind = g.kind;
    key_span(s, lo, hi, [&](uint64_t r) { return in_key(kind, w, flt_load(values + r * w, w)); });
    key_store(s, s_w64);
}

// ---- phase 2, one workgroup per column: `selected` as k_agg_finish counts it; the table's keys (and the key 0, if its
// flag is up) gathered in LDS, sorted ascending by a bitonic network, stored for the assign walk, and written as value
// bytes into the result: { selected, count, n_keys, overflow, 0 .. } in 8 words, then kmax key slots, zeros behind n_keys.
__global__ void __launch_bounds__(WG) k_key_finish(KeyLaunch kl, uint64_t* results) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_keys[KEY_MAX_KEYS];
    __shared__ uint32_t s_n;
    const AggCol g = kl.acols[blockIdx.x];
    const KeyCol kc = kl.kcols[blockIdx.x];
    KeyState* st = kl.st + blockIdx.x;
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
    // the key 0, if flagged, takes place 0 and the gather starts behind it: both written before the barrier, by the
    // thread whose fill touches s_keys[0], so no lane's atomicAdd or store meets them
    const bool has_zero = st->has_zero != 0;   // (written by the collect kernels: final here)
    for (uint32_t i = threadIdx.x; i < KEY_MAX_KEYS; i += WG) s_keys[i] = ~0ull;   // behind every key: the sort's padding
    if (threadIdx.x == 0) {
        s_n = has_zero ? 1u : 0u;
        if (has_zero) s_keys[0] = 0;
    }
    __syncthreads();
    const uint64_t* tab = kl.tabs + kc.tab0;
    for (uint32_t i = threadIdx.x; i <= kc.tab_mask; i += WG) {
        const uint64_t v = tab[i];
        if (v) {
            const uint32_t at = atomicAdd(&s_n, 1u);
            if (at < KEY_MAX_KEYS) s_keys[at] = v;
        }
    }
    __syncthreads();
    const uint32_t total = s_n;
    const bool over = total > kc.max_keys || st->overflow != 0;   // (the early flag is raised by a count above max_keys alone)
    const uint32_t n = over ? 0u : total;
    uint32_t P = 2;
    while (P < n) P <<= 1;
    for (uint32_t size = 2; size <= P; size <<= 1)
        for (uint32_t stride = size >> 1; stride; stride >>= 1) {
            for (uint32_t i = threadIdx.x; i < P / 2; i += WG) {
                const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t ka = s_keys[lo], kb = s_keys[hi];
                if ((kb < ka) == up && ka != kb) s_keys[lo] = kb, s_keys[hi] = ka;
            }
            __syncthreads();
        }
    uint64_t* sorted = kl.sorted + (uint64_t)blockIdx.x * KEY_MAX_KEYS;
    for (uint32_t i = threadIdx.x; i < n; i += WG) sorted[i] = s_keys[i];
    uint64_t* r = results + (uint64_t)blockIdx.x * key_result_words(kl.kmax);
    if (threadIdx.x == 0) {
        st->overflow = over ? 1u : 0u;
        st->n_keys = n;
        st->steps = key_steps(n);
        r[0] = nsel, r[1] = st->count, r[2] = n, r[3] = over ? 1u : 0u;
        r[4] = r[5] = r[6] = r[7] = 0;
    }
    for (uint32_t i = threadIdx.x; i < kc.max_keys; i += WG) r[8 + i] = i < n ? agg_unkey(g.kind, g.w, s_keys[i]) : 0;
}

// ---- phase 3.  The id of every row: key_lower_bound over the column's keys in LDS, all ones where the row is not live;
// one lane per row, so a wave stores 64 neighbouring ids.
struct KeyIdSink {
    const uint32_t* sel;
    const uint8_t* def_bits;
    uint64_t out_row;
    uint8_t* ids;
    uint32_t idw;
};
__device__ __forceinline__ void key_id_store(uint8_t* ids, uint32_t idw, uint64_t row, uint32_t id) {
    if (idw == 1) ids[row] = (uint8_t)id;
    else if (idw == 2) ((uint16_t*)ids)[row] = (uint16_t)id;
    else ((uint32_t*)ids)[row] = id;
}
template <class F>
__device__ __forceinline__ void key_id_span(const KeyIdSink& k, uint64_t lo, uint64_t hi, F id_of) {
    for (uint64_t r = lo + threadIdx.x; r < hi; r += WG) {
        const uint64_t c = k.out_row + r;
        bool on = true;
        if (k.sel) on = (gld32(k.sel + (c >> 5)) >> (uint32_t)(c & 31)) & 1u;
        if (on && k.def_bits) on = (ldu8(k.def_bits + (r >> 3)) >> (uint32_t)(r & 7)) & 1u;
        key_id_store(k.ids, k.idw, c, on ? id_of(r) : 0xFFFFFFFFu);
    }
}
struct KeyFind {
    const uint64_t* keys;   // LDS
    uint32_t n, steps, kind, w;
};
__device__ __forceinline__ uint32_t key_find(const KeyFind& f, uint64_t raw) { return key_lower_bound(f.keys, f.n, f.steps, in_key(f.kind, f.w, raw)); }
// the column's sorted keys into LDS, as in_stage does it; the caller's barrier follows
__device__ __forceinline__ KeyFind key_stage(const KeyLaunch& kl, uint32_t col, const AggCol& g, uint64_t* s_keys) {
    const KeyState* st = kl.st + col;
    const uint32_t n = min(st->n_keys, KEY_MAX_KEYS);
    const uint64_t* sorted = kl.sorted + (uint64_t)col * KEY_MAX_KEYS;
    for (uint32_t i = threadIdx.x; i < n; i += WG) s_keys[i] = sorted[i];
    return KeyFind{s_keys, n, st->steps, g.kind, g.w};
}

__device__ void key_assign_tile(const DecodeArgs& a, const KeyLaunch& kl, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint16_t* s_ids, uint64_t* s_keys,
                                uint32_t* staged) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok || d.codec == SB_CODEC_FREQ) return;   // (the interval fails / is replayed)
    if (kl.st[tt.col].overflow) return;
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    const AggCol g = kl.acols[tt.col];
    const KeyCol kc = kl.kcols[tt.col];
    const uint32_t w = c.width;
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    const KeyIdSink k{g.sel, d.def_bits, t.out_row, kc.ids, kc.idw};
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) {   // no value and no index is loaded
        key_id_span(k, lo, hi, [&](uint64_t) { return 0xFFFFFFFFu; });
        return;
    }
    if (*staged != tt.col) {   // (the same for every lane: the tile's column)
        __syncthreads();
        (void)key_stage(kl, tt.col, g, s_keys);
        *staged = tt.col;
        __syncthreads();
    }
    const KeyState* st = kl.st + tt.col;
    const KeyFind f{s_keys, min(st->n_keys, KEY_MAX_KEYS), st->steps, g.kind, w};
    switch (d.codec) {
        case SB_CODEC_NONE: {
            const uint8_t* src = d.src;
            key_id_span(k, lo, hi, [&](uint64_t r) { return key_find(f, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_LZ4:
        case SB_CODEC_ZSTD:
        case SB_CODEC_SNAPPY:
        case SB_CODEC_PATAS: {
            const uint8_t* src = c.values + t.out_row * w;
            key_id_span(k, lo, hi, [&](uint64_t r) { return key_find(f, flt_load(src + r * w, w)); });
            break;
        }
        case SB_CODEC_ONEVALUE: {
            const uint32_t id = key_find(f, flt_load(d.body, w));
            key_id_span(k, lo, hi, [&](uint64_t) { return id; });
            break;
        }
        case SB_CODEC_DICT: {
            U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
            u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
            const uint8_t* dict = d.dict;
            const uint32_t D = d.dict_n;
            if (D <= FILTER_DICT_BITS) {   // one search per entry into the page's id table (an id is below KEY_MAX_KEYS)
                for (uint32_t e = threadIdx.x; e < D; e += WG) s_ids[e] = (uint16_t)key_find(f, flt_load(dict + (uint64_t)e * w, w));
                __syncthreads();
                key_id_span(k, lo, hi, [&](uint64_t r) {
                    const uint32_t e = s_a[sidx((int)(r - lo))];
                    return e < D ? (uint32_t)s_ids[e] : 0xFFFFFFFFu;   // (an index beyond the dictionary was raised by the collect walk)
                });
            } else {
                key_id_span(k, lo, hi, [&](uint64_t r) {
                    const uint32_t e = s_a[sidx((int)(r - lo))];
                    return e < D ? key_find(f, flt_load(dict + (uint64_t)e * w, w)) : 0xFFFFFFFFu;
                });
            }
            break;
        }
        case SB_CODEC_BITPACKING:
        case SB_CODEC_DELTA_BITPACKING: {
            if (w != 4) break;
            U32Stream vs{d.body, (const uint32_t*)(a.scratch + t.aux_off), d.codec, 0, t.num_values};
            u32_tile_to_lds(vs, tt.tile, rows, s_a, s_w);
            key_id_span(k, lo, hi, [&](uint64_t r) { return key_find(f, (uint64_t)s_a[sidx((int)(r - lo))]); });
            break;
        }
        default:   // (k_key_assign_rle)
            break;
    }
}

__global__ void __launch_bounds__(WG) k_key_assign(DecodeArgs a, KeyLaunch kl) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint16_t s_ids[FILTER_DICT_BITS];
    __shared__ uint64_t s_keys[KEY_MAX_KEYS];
    const uint32_t count = a.job_counts[2];
    uint32_t staged = 0xFFFFFFFFu;
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        key_assign_tile(a, kl, ti, s_a, s_w, s_ids, s_keys, &staged);
        __syncthreads();
    }
}

// RLE pages: one search per run into its id
struct RleKeyAssign {
    using Rec = uint32_t;
    uint32_t* s_rec;
    KeyIdSink k;
    KeyFind f;
    __device__ __forceinline__ uint32_t rec_bytes() const { return 4 + f.w; }
    __device__ __forceinline__ uint32_t load(const uint8_t* v, bool in) const { return in ? key_find(f, flt_load(v, f.w)) : 0u; }
    __device__ __forceinline__ void rows(uint64_t tile_lo, uint64_t lo, uint64_t hi, uint32_t A, const uint32_t* s_flag) const {
        key_id_span(k, lo, hi, [&](uint64_t r) { return s_rec[A + s_flag[sidx((int)(r - tile_lo))]]; });
    }
};

__global__ void __launch_bounds__(WG) k_key_assign_rle(DecodeArgs a, KeyLaunch kl) {
    __shared__ __attribute__((aligned(16))) uint32_t s_flag[SIDX_WORDS];
    __shared__ uint32_t s_run[RLE_CHUNK];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_keys[KEY_MAX_KEYS];
    if (a.job_counts[4] == 0) return;  // no RLE page in this call
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    const PageTask t = a.tasks[p];
    const ColDesc c = a.cols[t.col];
    if (!rle_by_page(c, d)) return;
    if (kl.st[t.col].overflow) return;
    const AggCol g = kl.acols[t.col];
    const KeyCol kc = kl.kcols[t.col];
    const KeyFind f = key_stage(kl, t.col, g, s_keys);
    __syncthreads();   // (the walk's first loads search the keys)
    const uint32_t part = blockIdx.y, parts = gridDim.y;
    const uint64_t* sums = parts > 1 ? a.rle_sums + (uint64_t)p * parts : nullptr;
    const RleKeyAssign pol{s_run, KeyIdSink{g.sel, d.def_bits, t.out_row, kc.ids, kc.idw}, f};
    rle_page_walk(pol, c, t, d, s_flag, s_w, s_w64, a.status, p, part, parts, sums);
}

// the Freq replay: from the decoded column, one search per row
__global__ void __launch_bounds__(WG) k_key_assign_plain(KeyLaunch kl, uint32_t col, const uint8_t* values, const uint8_t* validity) {
    __shared__ uint64_t s_keys[KEY_MAX_KEYS];
    if (kl.st[col].overflow) return;
    const AggCol g = kl.acols[col];
    const KeyCol kc = kl.kcols[col];
    const KeyFind f = key_stage(kl, col, g, s_keys);
    __syncthreads();
    const uint64_t lo = (uint64_t)blockIdx.x * TILE_ROWS, hi = min(g.rows, lo + TILE_ROWS);
    const KeyIdSink k{g.sel, validity, 0, kc.ids, kc.idw};
    const uint32_t w = g.w;
    key_id_span(k, lo, hi, [&](uint64_t r) { return key_find(f, flt_load(values + r * w, w)); });
}

// the states and the tables start from zero; timed under a name of its own
void launch_key_zero(sb_ctx* ctx, const KeyLaunch& kl) {
    KScope k(ctx, "key_zero(memset)");
    if (kl.zero_bytes) (void)hipMemsetAsync(kl.st, 0, (size_t)kl.zero_bytes, ctx->stream);
}

void launch_key_collect(sb_ctx* ctx, const DecodeArgs& a, const KeyLaunch& kl) {
    hipStream_t s = ctx->stream;
    {
        KScope k(ctx, "k_key_collect_rle");
        if (a.rle_parts > 1) k_rle_sums<<<dim3(a.n_pages, a.rle_parts), WG, 0, s>>>(a);
        k_key_collect_rle<<<dim3(a.n_pages, std::max<uint32_t>(1u, a.rle_parts)), WG, 0, s>>>(a, kl);
    }
    if (a.n_tiles) {
        KScope k(ctx, "k_key_collect");
        k_key_collect<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, kl);
    }
}

void launch_key_finish(sb_ctx* ctx, const KeyLaunch& kl, uint64_t* results) {
    KScope k(ctx, "k_key_finish");
    k_key_finish<<<kl.n_cols, WG, 0, ctx->stream>>>(kl, results);
}

// the second walk: the pages are parsed, inflated and planned, and the parts' sums (k_rle_sums) are where the first left them
void launch_key_assign(sb_ctx* ctx, const DecodeArgs& a, const KeyLaunch& kl) {
    hipStream_t s = ctx->stream;
    {
        KScope k(ctx, "k_key_assign_rle");
        k_key_assign_rle<<<dim3(a.n_pages, std::max<uint32_t>(1u, a.rle_parts)), WG, 0, s>>>(a, kl);
    }
    if (a.n_tiles) {
        KScope k(ctx, "k_key_assign");
        k_key_assign<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, kl);
    }
}

// `rows[i]`, `values[i]`, `validity[i]` (host arrays): the decoded columns of the replay
void launch_key_collect_plain(sb_ctx* ctx, const KeyLaunch& kl, const uint64_t* rows, const uint8_t* const* values, const uint8_t* const* validity) {
    KScope k(ctx, "k_key_collect_plain");
    for (uint32_t i = 0; i < kl.n_cols; i++)
        if (rows[i]) k_key_collect_plain<<<(uint32_t)((rows[i] + TILE_ROWS - 1) / TILE_ROWS), WG, 0, ctx->stream>>>(kl, i, values[i], validity[i]);
}
void launch_key_assign_plain(sb_ctx* ctx, const KeyLaunch& kl, const uint64_t* rows, const uint8_t* const* values, const uint8_t* const* validity) {
    KScope k(ctx, "k_key_assign_plain");
    for (uint32_t i = 0; i < kl.n_cols; i++)
        if (rows[i]) k_key_assign_plain<<<(uint32_t)((rows[i] + TILE_ROWS - 1) / TILE_ROWS), WG, 0, ctx->stream>>>(kl, i, values[i], validity[i]);
}

}  // namespace sb
