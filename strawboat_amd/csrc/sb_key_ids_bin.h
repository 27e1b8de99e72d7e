// strawboat-hip: sb_key_ids_var — distinct keys and dense group ids of a Binary / Utf8 key column (included by sb_decode.hip
// behind sb_key_ids.h, whose id sink — key_id_span / key_id_store — the assign kernels end in, and behind sb_filter_bin.h,
// whose bin_dict / bin_base_column find the entries of Dict / Freq pages and place the value blocks to inflate).
//
// The chain is a filter call's up to the staged value blocks (k_parse .. k_plan, k_keyv_base, queues B / Z), then three
// phases on the stream, the pages parsed, inflated and planned once:
//   keyv_zero                 the columns' states and tables start from zero (one memset)
//   1. collect  k_keyv_clear    the bit table of every Dict / Freq page (a bit per entry, at the end of its aux area) to zero
//               k_keyv_collect  the tiles.  Dict / Freq: the entries that live rows point at are marked, through an LDS bit
//                               table per tile (<= FILTER_DICT_BITS entries) and atomicOr of its non-zero words.  OneValue:
//                               one candidate per tile with a live row.  Basic: a candidate per live row, less the lanes whose
//                               string is their lower neighbour's.  `count` is one integer add per tile.
//               k_keyv_entries  grid (pages, FILTER_BIN_EY), a lane per entry: the marked entries are the candidates
//   2. finish   k_keyv_finish   one workgroup per column: the table's references gathered and counted, resolved, sorted by
//                               bytes (a bitonic network over prefix | pointer | length; no ties), the lengths scanned into
//                               key_offsets, the bytes copied into the result record, the sorted keys left for phase 3
//   3. assign   k_keyv_entry_ids  a search per marked entry into the page's 16-bit id table (in front of its bit table)
//               k_keyv_assign     the tiles: Dict / Freq rows look their entry up (the id table in LDS up to
//                                 FILTER_DICT_BITS entries, gathered beyond), OneValue one search per tile, Basic one per
//                                 row; one lane per row stores id_width bytes, all ones where the row is not live
//
// THE DISTINCT SET IS EXACT, AND NO LANE WAITS FOR ANOTHER.  A slot of either level is one 64-bit word, `tag | reference`
// (kv_word, sb_common.h), written by one compare-and-swap and complete the moment it is visible: the reference names a
// string that memory no kernel writes any more resolves to (kv_resolve: a.descs, bin_dict(...).ent_off, d.src / d.vbody /
// c.values + d.val_base).  A probe that meets its tag resolves the reference and compares lengths, then bytes: equal, it is
// done; not, it goes on to the next slot.  0 is the empty slot.  Two strings never merge, whatever their hashes; a probe
// loop is bounded by its table and spins on nothing.  The two levels, the early overflow flag and the counting of winners
// are sb_key_ids.h's: an LDS set per workgroup (KEY_SET_SLOTS), the column's table in the call's tables (>= 4 * max_keys
// slots, relaxed agent-scope loads: the XCDs' L2s are not coherent, and a stale empty slot only costs the compare-and-swap).
//
// LOADS STAY INSIDE THEIR BUFFERS by the rule at the head of sb_filter_bin.h (kv_rel / kv_hash / kv_first8, sb_common.h);
// offsets that leave a values block are cut to it as filter_bin_basic cuts them.
//
// LDS:  k_keyv_collect    17 KiB index tile + 1 KiB bit table + 16 KiB set = 35120 B          4 workgroups per CU (160 KiB)
//       k_keyv_entries    16 KiB set = 16384 B                                              8 (the 32 waves of a CU)
//       k_keyv_finish     8 + 8 + 4 KiB keys, 2 KiB scan = 22568 B                          (one workgroup per column)
//       k_keyv_entry_ids  8 KiB prefixes = 8192 B                                           8
//       k_keyv_assign     17 KiB index tile + 16 KiB id table + 8 KiB prefixes = 42256 B    3
// (DESIGN 4j has the registers, and what the probe measured)
#pragma once

namespace sb {

struct KvStr {
    const uint8_t* p;
    uint32_t len;
};
__device__ __forceinline__ uint32_t kv_over(const KeyVarState* st) {
    return __hip_atomic_load(&st->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// entry e of a Dict / Freq page: k_plan's offset pair, as k_filter_bin_entries reads it
__device__ __forceinline__ KvStr kv_entry(const uint8_t* dict, const BinDict& bd, uint32_t e) {
    const uint64_t pr = ldu64((const uint8_t*)(bd.ent_off + e));
    const uint32_t eo = (uint32_t)pr;
    return KvStr{dict + eo + 8, (uint32_t)(pr >> 32) - eo - 8 - (e == 0 ? bd.gap : 0)};
}
// row r of a Basic page: the offset pair cut to the values block
__device__ __forceinline__ KvStr kv_row(int32_t ptype, const uint8_t* offs, const uint8_t* vals, uint32_t vsize, uint64_t r) {
    uint64_t o0, o1;
    if (ptype == SB_TYPE_BINARY) {   // (the pair with one load)
        const uint64_t pr = ldu64(offs + r * 4);
        o0 = (uint32_t)pr;
        o1 = pr >> 32;
    } else {
        o0 = ldu64(offs + r * 8);
        o1 = ldu64(offs + r * 8 + 8);
    }
    o1 = min(o1, (uint64_t)vsize);
    o0 = min(o0, o1);
    return KvStr{vals + o0, (uint32_t)(o1 - o0)};
}
__device__ __forceinline__ const uint8_t* kv_vals(const ColDesc& c, const PageDesc& d) { return d.codec == SB_CODEC_NONE ? d.vbody : c.values + d.val_base; }
// the string a slot's word names
__device__ __forceinline__ KvStr kv_resolve(const DecodeArgs& a, uint64_t word) {
    const uint32_t page = (uint32_t)(word >> 36), index = (uint32_t)(word >> 10) & ((1u << KEYV_INDEX_BITS) - 1), form = (uint32_t)(word >> 8) & 3u;
    const PageDesc& d = a.descs[page];
    if (form == KEYV_ONE) return KvStr{d.dict, d.dict_n};
    const PageTask t = a.tasks[page];
    if (form == KEYV_ENTRY) {
        BinDict bd;
        (void)bin_dict(a, t, d, &bd);   // (checked by the kernel that made the word)
        return kv_entry(d.dict, bd, index);
    }
    const ColDesc& c = a.cols[t.col];
    return kv_row(c.ptype, d.src, kv_vals(c, d), d.vusize, index);
}
__device__ __forceinline__ bool kv_same(const DecodeArgs& a, uint64_t v, uint64_t word, const KvStr& s) {
    if ((uint8_t)v != (uint8_t)word) return false;   // the tags
    if (v == word) return true;
    const KvStr o = kv_resolve(a, v);
    return kv_equal(o.p, o.len, s.p, s.len);
}

struct KvSink {
    uint64_t* set;             // LDS, KEY_SET_SLOTS
    KeyVarState* st;
    uint64_t* tab;             // the column's table
    uint32_t mask, max_keys;
};
__device__ __forceinline__ KvSink kv_sink(const KeyVarLaunch& kl, uint32_t col, uint64_t* set) {
    const KeyVarCol kc = kl.kcols[col];
    return KvSink{set, kl.st + col, kl.tabs + kc.tab0, kc.tab_mask, kc.max_keys};
}
// true: the string is new to the workgroup and this lane put it in (a set that is full says so too: the table decides then)
__device__ __forceinline__ bool kv_set_put(const DecodeArgs& a, uint64_t* set, uint64_t hash, uint64_t word, const KvStr& s) {
    uint32_t h = (uint32_t)hash & (KEY_SET_SLOTS - 1);
    for (uint32_t i = 0; i < KEY_SET_SLOTS; i++, h = (h + 1) & (KEY_SET_SLOTS - 1)) {
        uint64_t v = set[h];
        if (v == 0) {
            v = atomicCAS((unsigned long long*)&set[h], 0ull, (unsigned long long)word);
            if (v == 0) return true;
        }
        if (kv_same(a, v, word, s)) return false;
    }
    return true;
}
// the string into the column's table: loads until an empty slot, one compare-and-swap there
__device__ __forceinline__ void kv_tab_put(const DecodeArgs& a, const KvSink& k, uint64_t hash, uint64_t word, const KvStr& s) {
    uint32_t h = (uint32_t)hash & k.mask;
    for (uint32_t i = 0; i <= k.mask; i++, h = (h + 1) & k.mask) {
        uint64_t v = __hip_atomic_load(k.tab + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == 0) {
            v = atomicCAS((unsigned long long*)(k.tab + h), 0ull, (unsigned long long)word);
            if (v == 0) {
                if (atomicAdd(&k.st->inserted, 1u) >= k.max_keys) __hip_atomic_store(&k.st->overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
        }
        if (kv_same(a, v, word, s)) return;
    }
    __hip_atomic_store(&k.st->overflow, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // no slot left: more than max_keys keys
}
// a candidate: `form` / `page` / `index` say where memory keeps it
__device__ __forceinline__ void kv_offer(const DecodeArgs& a, const KvSink& k, const KvStr& s, uint32_t form, uint32_t page, uint32_t index) {
    const uint64_t hash = kv_hash(s.p, s.len);
    const uint64_t word = kv_word(form, page, index, hash);
    if (kv_set_put(a, k.set, hash, word, s)) kv_tab_put(a, k, hash, word, s);
}
// the set empty, by the whole workgroup; the caller's barrier follows
__device__ __forceinline__ void kv_set_clear(uint64_t* set) {
    for (uint32_t i = threadIdx.x; i < KEY_SET_SLOTS; i += WG) set[i] = 0;
}

// ---- where the inflated value blocks go: k_filter_bin_base for every binary column of the call
__global__ void __launch_bounds__(64) k_keyv_base(DecodeArgs a) {
    const ColDesc c = a.cols[blockIdx.x];
    if (is_binary(c.ptype)) bin_base_column(a, c);
    bin_base_done(a);
}

// ---- phase 1.  The bit tables of the Dict / Freq pages: bit e set = a live row points at entry e
__global__ void __launch_bounds__(WG) k_keyv_clear(DecodeArgs a) {
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    if (!d.ok || (d.codec != SB_CODEC_DICT && d.codec != SB_CODEC_FREQ)) return;
    const PageTask t = a.tasks[p];
    if (!is_binary(a.cols[t.col].ptype)) return;
    BinDict bd;
    if (!bin_dict(a, t, d, &bd)) {
        if (threadIdx.x == 0) raise(a.status, SB_ERR_INVALID, p, 220);
        return;
    }
    for (uint32_t g = threadIdx.x; g < (bd.D + 31) / 32; g += WG) gst32(bd.bits + g, 0u);
}
// the page's 16-bit id table, in front of its bit table; false: the entry offsets reach into it (raised by k_keyv_clear's
// check of the bit table, or here)
__device__ __forceinline__ bool kv_id_table(const PageTask& t, const BinDict& bd, uint16_t** ids) {
    uint32_t* tab = bd.bits - keyv_id_table_words(t.length);
    *ids = (uint16_t*)tab;
    return (uint64_t)bd.D <= 2 * keyv_id_table_words(t.length) && bd.ent_off + (uint64_t)bd.D + 1 <= tab;
}

__device__ void keyv_collect_tile(const DecodeArgs& a, const KeyVarLaunch& kl, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint32_t* s_tab, uint64_t* s_set,
                                  uint64_t* s_w64, uint32_t* owner) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    if (!is_binary(c.ptype)) return;
    const AggCol g = kl.acols[tt.col];
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    // a tile without a selected row: no value and no index is loaded
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) return;
    if (*owner != tt.col) {   // (the same for every lane: the tile's column)
        __syncthreads();
        kv_set_clear(s_set);
        *owner = tt.col;
        __syncthreads();
    }
    const KvSink k = kv_sink(kl, tt.col, s_set);
    const AggSink rs{g.sel, d.def_bits, t.out_row};
    uint64_t cnt = 0;
    if (is_basic(d.codec)) {
        const uint8_t* vals = kv_vals(c, d);
        const uint32_t lane = threadIdx.x & 63;
        for (uint64_t base = lo; base < hi; base += WG) {   // the same number of steps for every lane: the shuffles
            const uint64_t r = base + threadIdx.x, cr = t.out_row + r;
            bool on = r < hi;
            if (on && g.sel) on = (gld32(g.sel + (cr >> 5)) >> (uint32_t)(cr & 31)) & 1u;
            if (on && d.def_bits) on = (ldu8(d.def_bits + (r >> 3)) >> (uint32_t)(r & 7)) & 1u;
            if (on) cnt++;
            if (kv_over(k.st)) on = false;
            KvStr s{vals, 0};
            if (on) s = kv_row(c.ptype, d.src, vals, d.vusize, r);
            const uint64_t f8 = on ? kv_first8(s.p, s.len) : 0ull;
            // a lane whose string is its lower neighbour's is dropped before either level sees it: the lengths and the
            // first 8 bytes decide nearly always, the rest of the bytes where they agree
            const uint64_t pf8 = __shfl_up(f8, 1, 64), pp = __shfl_up((uint64_t)(uintptr_t)s.p, 1, 64);
            const uint32_t plen = __shfl_up(s.len, 1, 64);
            const int pon = __shfl_up((int)on, 1, 64);
            if (on && lane && pon && plen == s.len && pf8 == f8 && (s.len <= 8 || kv_equal((const uint8_t*)(uintptr_t)pp, plen, s.p, s.len))) on = false;
            if (on) kv_offer(a, k, s, KEYV_ROW, tt.page, (uint32_t)r);
        }
    } else if (d.codec == SB_CODEC_ONEVALUE) {   // one candidate for the tile, if a row of it is live
        agg_rows(rs, lo, hi, [&](uint64_t) { cnt++; });
        const bool any = __syncthreads_or(cnt != 0) != 0;
        if (any && threadIdx.x == 0 && !kv_over(k.st)) kv_offer(a, k, KvStr{d.dict, d.dict_n}, KEYV_ONE, tt.page, 0u);
    } else if (d.codec == SB_CODEC_DICT || d.codec == SB_CODEC_FREQ) {
        BinDict bd;
        if (!bin_dict(a, t, d, &bd)) return;   // (raised by k_keyv_clear)
        U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
        u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
        const uint32_t D = bd.D;
        bool bad = false;
        if (D <= FILTER_DICT_BITS) {
            const uint32_t words = (D + 31) / 32;
            for (uint32_t i = threadIdx.x; i < words; i += WG) s_tab[i] = 0;
            __syncthreads();
            agg_rows(rs, lo, hi, [&](uint64_t r) {
                cnt++;
                const uint32_t e = s_a[sidx((int)(r - lo))];
                if (e >= D) bad = true;
                else atomicOr(&s_tab[e >> 5], 1u << (e & 31));
            });
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < words; i += WG)
                if (s_tab[i]) atomicOr(bd.bits + i, s_tab[i]);
        } else {   // a bit per row, where it is not up yet (a stale word only costs the atomic)
            uint32_t* bits = bd.bits;
            agg_rows(rs, lo, hi, [&](uint64_t r) {
                cnt++;
                const uint32_t e = s_a[sidx((int)(r - lo))];
                if (e >= D) bad = true;
                else if (!((gld32(bits + (e >> 5)) >> (e & 31)) & 1u)) atomicOr(bits + (e >> 5), 1u << (e & 31));
            });
        }
        if (bad) raise(a.status, SB_ERR_OUT_OF_SPEC, tt.page, 222);   // (where the var filter finds it)
    } else {
        return;
    }
    cnt = wg_sum64(cnt, s_w64);
    if (threadIdx.x == 0 && cnt) atomicAdd((unsigned long long*)&k.st->count, (unsigned long long)cnt);
}

__global__ void __launch_bounds__(WG) k_keyv_collect(DecodeArgs a, KeyVarLaunch kl) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint64_t s_w64[4];
    __shared__ uint32_t s_tab[FILTER_DICT_BITS / 32];
    __shared__ uint64_t s_set[KEY_SET_SLOTS];
    const uint32_t count = a.job_counts[2];
    uint32_t owner = 0xFFFFFFFFu;
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        keyv_collect_tile(a, kl, ti, s_a, s_w, s_tab, s_set, s_w64, &owner);
        __syncthreads();
    }
}

// grid (pages, FILTER_BIN_EY): a lane per entry, the marked ones offered
__global__ void __launch_bounds__(WG) k_keyv_entries(DecodeArgs a, KeyVarLaunch kl) {
    __shared__ uint64_t s_set[KEY_SET_SLOTS];
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    if (!d.ok || (d.codec != SB_CODEC_DICT && d.codec != SB_CODEC_FREQ)) return;
    const PageTask t = a.tasks[p];
    if (!is_binary(a.cols[t.col].ptype)) return;
    BinDict bd;
    if (!bin_dict(a, t, d, &bd)) return;   // (raised by k_keyv_clear)
    kv_set_clear(s_set);
    __syncthreads();
    const KvSink k = kv_sink(kl, t.col, s_set);
    for (uint32_t e0 = blockIdx.y * WG; e0 < bd.D; e0 += gridDim.y * WG) {
        const uint32_t e = e0 + threadIdx.x;
        if (e < bd.D && ((gld32(bd.bits + (e >> 5)) >> (e & 31)) & 1u) && !kv_over(k.st)) kv_offer(a, k, kv_entry(d.dict, bd, e), KEYV_ENTRY, p, e);
    }
}

// ---- phase 2, one workgroup per column
constexpr uint32_t KEYV_PAD = 0xFFFFFFFFu;   // the length of the sort's padding: behind every key
__device__ __forceinline__ bool kv_sort_less(uint64_t pa, uint64_t qa, uint32_t la, uint64_t pb, uint64_t qb, uint32_t lb) {
    if (la == KEYV_PAD) return false;
    if (lb == KEYV_PAD) return true;
    if (pa != pb) return pa < pb;
    return kv_rel((const uint8_t*)(uintptr_t)qa, la, (const uint8_t*)(uintptr_t)qb, lb) == 0u;
}
__global__ void __launch_bounds__(WG) k_keyv_finish(DecodeArgs a, KeyVarLaunch kl, uint64_t* results) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_pre[KEY_MAX_KEYS];   // the prefixes; behind the sort the offsets
    __shared__ uint64_t s_ptr[KEY_MAX_KEYS];   // the gathered words, then what they resolve to
    __shared__ uint32_t s_len[KEY_MAX_KEYS];
    __shared__ uint64_t s_scan[WG];
    __shared__ uint32_t s_n;
    const AggCol g = kl.acols[blockIdx.x];
    const KeyVarCol kc = kl.kcols[blockIdx.x];
    KeyVarState* st = kl.st + blockIdx.x;
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
    for (uint32_t i = threadIdx.x; i < KEY_MAX_KEYS; i += WG) s_len[i] = KEYV_PAD, s_pre[i] = ~0ull, s_ptr[i] = 0;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const uint64_t* tab = kl.tabs + kc.tab0;
    for (uint32_t i = threadIdx.x; i <= kc.tab_mask; i += WG) {
        const uint64_t v = tab[i];
        if (v) {
            const uint32_t at = atomicAdd(&s_n, 1u);
            if (at < KEY_MAX_KEYS) s_ptr[at] = v;
        }
    }
    __syncthreads();
    const uint32_t total = s_n;   // exact: every winner of a slot is in the table (the early flag only ended the work sooner)
    const bool over = total > kc.max_keys;
    const uint32_t n = over ? 0u : total;
    for (uint32_t i = threadIdx.x; i < n; i += WG) {
        const KvStr s = kv_resolve(a, s_ptr[i]);
        s_ptr[i] = (uint64_t)(uintptr_t)s.p;
        s_len[i] = s.len;
        s_pre[i] = kv_prefix(s.p, s.len);
    }
    __syncthreads();
    uint32_t P = 2;
    while (P < n) P <<= 1;
    for (uint32_t size = 2; size <= P; size <<= 1)
        for (uint32_t stride = size >> 1; stride; stride >>= 1) {
            for (uint32_t i = threadIdx.x; i < P / 2; i += WG) {
                const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const uint64_t pa = s_pre[lo], pb = s_pre[hi], qa = s_ptr[lo], qb = s_ptr[hi];
                const uint32_t la = s_len[lo], lb = s_len[hi];
                const bool swap = up ? kv_sort_less(pb, qb, lb, pa, qa, la) : kv_sort_less(pa, qa, la, pb, qb, lb);
                if (swap) s_pre[lo] = pb, s_pre[hi] = pa, s_ptr[lo] = qb, s_ptr[hi] = qa, s_len[lo] = lb, s_len[hi] = la;
            }
            __syncthreads();
        }
    // the sorted keys for the assign walk
    uint8_t* sorted = kl.sorted + (uint64_t)blockIdx.x * KEYV_SORTED_BYTES;
    uint64_t* o_ptr = (uint64_t*)sorted;
    uint64_t* o_pre = o_ptr + KEY_MAX_KEYS;
    uint32_t* o_len = (uint32_t*)(o_pre + KEY_MAX_KEYS);
    for (uint32_t i = threadIdx.x; i < n; i += WG) o_ptr[i] = s_ptr[i], o_pre[i] = s_pre[i], o_len[i] = s_len[i];
    // the lengths scanned: a thread has KEY_MAX_KEYS / WG neighbouring keys
    constexpr uint32_t PER = KEY_MAX_KEYS / WG;
    uint64_t mine = 0;
    for (uint32_t j = 0; j < PER; j++) {
        const uint32_t i = threadIdx.x * PER + j;
        if (i < n) mine += s_len[i];
    }
    s_scan[threadIdx.x] = mine;
    __syncthreads();
    for (uint32_t dd = 1; dd < WG; dd <<= 1) {
        const uint64_t v = threadIdx.x >= dd ? s_scan[threadIdx.x - dd] : 0;
        __syncthreads();
        s_scan[threadIdx.x] += v;
        __syncthreads();
    }
    const uint64_t keys_len = s_scan[WG - 1];
    uint64_t off = s_scan[threadIdx.x] - mine;
    for (uint32_t j = 0; j < PER; j++) {   // (s_pre: stored for phase 3 above, by this thread's own lanes or others' — the barriers of the scan lie between)
        const uint32_t i = threadIdx.x * PER + j;
        s_pre[i] = off;
        if (i < n) off += s_len[i];
    }
    __syncthreads();
    const bool fits = keys_len <= kc.keys_cap;
    uint64_t* r = results + (uint64_t)blockIdx.x * keyv_result_words(kl.kmax, kl.kbytes);
    if (threadIdx.x == 0) {
        const uint32_t bits = over ? 1u : fits ? 0u : 2u;
        st->overflow = bits;
        st->n_keys = n;
        st->steps = key_steps(n);
        st->keys_len = keys_len;
        r[0] = nsel, r[1] = st->count, r[2] = n, r[3] = bits, r[4] = keys_len;
        r[5] = r[6] = r[7] = 0;
    }
    for (uint32_t i = threadIdx.x; i <= kl.kmax; i += WG) r[8 + i] = i < n ? s_pre[i] : keys_len;
    if (!fits) return;
    uint8_t* bytes = (uint8_t*)(r + 8 + kl.kmax + 1);   // keys_len <= keys_cap <= kbytes
    for (uint32_t i = threadIdx.x >> 6; i < n; i += WG / 64) {   // a wave per key
        const uint8_t* src = (const uint8_t*)(uintptr_t)s_ptr[i];
        uint8_t* dst = bytes + s_pre[i];
        for (uint32_t b = threadIdx.x & 63; b < s_len[i]; b += 64) dst[b] = ldu8(src + b);
    }
}

// ---- phase 3
struct KvFind {
    const uint64_t* pre;   // LDS
    const uint64_t* ptr;   // the call's tables
    const uint32_t* len;
    uint32_t n, steps;
};
__device__ __forceinline__ uint32_t kv_find(const KvFind& f, const KvStr& s) { return kv_lower_bound(f.pre, f.ptr, f.len, f.n, f.steps, s.p, s.len); }
// the column's prefixes into LDS; the caller's barrier follows
__device__ __forceinline__ KvFind kv_stage(const KeyVarLaunch& kl, uint32_t col, uint64_t* s_pre) {
    const KeyVarState* st = kl.st + col;
    const uint32_t n = min(st->n_keys, KEY_MAX_KEYS);
    const uint64_t* o_ptr = (const uint64_t*)(kl.sorted + (uint64_t)col * KEYV_SORTED_BYTES);
    const uint64_t* o_pre = o_ptr + KEY_MAX_KEYS;
    for (uint32_t i = threadIdx.x; i < n; i += WG) s_pre[i] = o_pre[i];
    return KvFind{s_pre, o_ptr, (const uint32_t*)(o_pre + KEY_MAX_KEYS), n, st->steps};
}

// grid (pages, FILTER_BIN_EY): the id of every marked entry into the page's id table
__global__ void __launch_bounds__(WG) k_keyv_entry_ids(DecodeArgs a, KeyVarLaunch kl) {
    __shared__ uint64_t s_pre[KEY_MAX_KEYS];
    const uint32_t p = blockIdx.x;
    const PageDesc d = a.descs[p];
    if (!d.ok || (d.codec != SB_CODEC_DICT && d.codec != SB_CODEC_FREQ)) return;
    const PageTask t = a.tasks[p];
    if (!is_binary(a.cols[t.col].ptype)) return;
    if (kl.st[t.col].overflow & 1u) return;
    BinDict bd;
    if (!bin_dict(a, t, d, &bd)) return;
    uint16_t* ids;
    if (!kv_id_table(t, bd, &ids)) {
        if (threadIdx.x == 0 && blockIdx.y == 0) raise(a.status, SB_ERR_INVALID, p, 220);
        return;
    }
    const KvFind f = kv_stage(kl, t.col, s_pre);
    __syncthreads();
    for (uint32_t e0 = blockIdx.y * WG; e0 < bd.D; e0 += gridDim.y * WG) {
        const uint32_t e = e0 + threadIdx.x;
        if (e >= bd.D) continue;
        const bool marked = (gld32(bd.bits + (e >> 5)) >> (e & 31)) & 1u;
        ids[e] = marked ? (uint16_t)kv_find(f, kv_entry(d.dict, bd, e)) : (uint16_t)0xFFFFu;
    }
}

__device__ void keyv_assign_tile(const DecodeArgs& a, const KeyVarLaunch& kl, uint32_t ti, uint32_t* s_a, uint32_t* s_w, uint16_t* s_ids, uint64_t* s_pre,
                                 uint32_t* staged) {
    const TileTask tt = a.tiles[ti];
    const PageDesc d = a.descs[tt.page];
    if (!d.ok) return;   // (the interval fails)
    if (kl.st[tt.col].overflow & 1u) return;
    const PageTask t = a.tasks[tt.page];
    const ColDesc c = a.cols[tt.col];
    if (!is_binary(c.ptype)) return;
    const AggCol g = kl.acols[tt.col];
    const KeyVarCol kc = kl.kcols[tt.col];
    const uint64_t lo = (uint64_t)tt.tile * TILE_ROWS;
    const uint32_t rows = (uint32_t)min((uint64_t)TILE_ROWS, t.num_values - lo);
    const uint64_t hi = lo + rows;
    const KeyIdSink k{g.sel, d.def_bits, t.out_row, kc.ids, kc.idw};
    if (!agg_any_selected(g.sel, t.out_row + lo, t.out_row + hi)) {   // no value and no index is loaded
        key_id_span(k, lo, hi, [&](uint64_t) { return 0xFFFFFFFFu; });
        return;
    }
    if (d.codec == SB_CODEC_DICT || d.codec == SB_CODEC_FREQ) {
        BinDict bd;
        uint16_t* ids = nullptr;
        if (!bin_dict(a, t, d, &bd) || !kv_id_table(t, bd, &ids)) return;   // (raised)
        U32Stream is{d.isrc, (const uint32_t*)(a.scratch + t.aux_off), d.icodec, d.n_runs, t.num_values};
        u32_tile_to_lds(is, tt.tile, rows, s_a, s_w);
        const uint32_t D = bd.D;
        if (D <= FILTER_DICT_BITS) {
            for (uint32_t e = threadIdx.x; e < D; e += WG) s_ids[e] = ids[e];
            __syncthreads();
            key_id_span(k, lo, hi, [&](uint64_t r) {
                const uint32_t e = s_a[sidx((int)(r - lo))];
                return e < D ? (uint32_t)s_ids[e] : 0xFFFFFFFFu;   // (an index beyond the dictionary was raised by the collect walk)
            });
        } else {
            key_id_span(k, lo, hi, [&](uint64_t r) {
                const uint32_t e = s_a[sidx((int)(r - lo))];
                return e < D ? (uint32_t)ids[e] : 0xFFFFFFFFu;
            });
        }
        return;
    }
    if (*staged != tt.col) {   // (the same for every lane: the tile's column)
        __syncthreads();
        (void)kv_stage(kl, tt.col, s_pre);
        *staged = tt.col;
        __syncthreads();
    }
    const KeyVarState* st = kl.st + tt.col;
    const uint64_t* o_ptr = (const uint64_t*)(kl.sorted + (uint64_t)tt.col * KEYV_SORTED_BYTES);
    const KvFind f{s_pre, o_ptr, (const uint32_t*)(o_ptr + 2 * KEY_MAX_KEYS), min(st->n_keys, KEY_MAX_KEYS), st->steps};
    if (is_basic(d.codec)) {
        const uint8_t* vals = kv_vals(c, d);
        key_id_span(k, lo, hi, [&](uint64_t r) { return kv_find(f, kv_row(c.ptype, d.src, vals, d.vusize, r)); });
    } else if (d.codec == SB_CODEC_ONEVALUE) {
        const uint32_t id = kv_find(f, KvStr{d.dict, d.dict_n});
        key_id_span(k, lo, hi, [&](uint64_t) { return id; });
    }
}

__global__ void __launch_bounds__(WG) k_keyv_assign(DecodeArgs a, KeyVarLaunch kl) {
    __shared__ uint32_t s_a[SIDX_WORDS];
    __shared__ uint32_t s_w[4];
    __shared__ uint16_t s_ids[FILTER_DICT_BITS];
    __shared__ uint64_t s_pre[KEY_MAX_KEYS];
    const uint32_t count = a.job_counts[2];
    uint32_t staged = 0xFFFFFFFFu;
    for (uint32_t ti = blockIdx.x; ti < count; ti += gridDim.x) {
        keyv_assign_tile(a, kl, ti, s_a, s_w, s_ids, s_pre, &staged);
        __syncthreads();
    }
}

void launch_keyv_base(sb_ctx* ctx, const DecodeArgs& a) {
    KScope k(ctx, "k_keyv_base");
    k_keyv_base<<<a.n_cols, 64, 0, ctx->stream>>>(a);
}
// the states and the tables start from zero; timed under a name of its own
void launch_keyv_zero(sb_ctx* ctx, const KeyVarLaunch& kl) {
    KScope k(ctx, "keyv_zero(memset)");
    if (kl.zero_bytes) (void)hipMemsetAsync(kl.st, 0, (size_t)kl.zero_bytes, ctx->stream);
}
void launch_keyv_collect(sb_ctx* ctx, const DecodeArgs& a, const KeyVarLaunch& kl) {
    hipStream_t s = ctx->stream;
    {
        KScope k(ctx, "k_keyv_clear");
        k_keyv_clear<<<a.n_pages, WG, 0, s>>>(a);
    }
    if (a.n_tiles) {
        KScope k(ctx, "k_keyv_collect");
        k_keyv_collect<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, kl);
    }
    KScope k(ctx, "k_keyv_entries");
    k_keyv_entries<<<dim3(a.n_pages, FILTER_BIN_EY), WG, 0, s>>>(a, kl);
}
void launch_keyv_finish(sb_ctx* ctx, const DecodeArgs& a, const KeyVarLaunch& kl, uint64_t* results) {
    KScope k(ctx, "k_keyv_finish");
    k_keyv_finish<<<kl.n_cols, WG, 0, ctx->stream>>>(a, kl, results);
}
// the second walk: the pages are parsed, inflated and planned, the bit tables say which entries are keys
void launch_keyv_assign(sb_ctx* ctx, const DecodeArgs& a, const KeyVarLaunch& kl) {
    hipStream_t s = ctx->stream;
    {
        KScope k(ctx, "k_keyv_entry_ids");
        k_keyv_entry_ids<<<dim3(a.n_pages, FILTER_BIN_EY), WG, 0, s>>>(a, kl);
    }
    if (a.n_tiles) {
        KScope k(ctx, "k_keyv_assign");
        k_keyv_assign<<<min(a.n_tiles, TILE_GRID), WG, 0, s>>>(a, kl);
    }
}

}  // namespace sb
