// strawboat-hip: sb_key_combine — dense ids of composite keys (included by sb_decode.hip behind sb_key_ids_bin.h; the distinct
// set, the finish and the search are sb_key_ids.h's: KeySink, key_offer, key_store, k_key_finish, key_stage, key_find,
// key_id_store; the code word is sb_common.h's: comb_pack).
//
// GROUP BY a, b / SELECT DISTINCT a, b: 2 .. 4 arrays of part ids (what sb_key_ids* wrote) go in; the sorted distinct
// tuples of the live rows come back on the host, and every row gets the position of its tuple among them (all ones for a
// row that is not live).  No page is read: two passes over the id arrays and a finish between them, on the stream:
//   comb_zero                 the items' states and tables start from zero (launch_key_zero's memset)
//   1. collect  k_comb_collect   persistent workgroups stride over the rows, a lane per row: the codes of the live rows
//                             into the workgroup's LDS set, a code new to the workgroup into the item's table
//   2. finish   k_key_finish  unchanged: the codes are presented as a UINT64 column (kind FK_UNSIGNED, w 8, no selection),
//                             so the record is { rows, live, n_keys, overflow, 0 .. } and kmax sorted codes
//   3. assign   k_comb_assign the same stride again: key_lower_bound over the item's codes in LDS, one id per row
// The item is the grid's y dimension: the items of a call share the three launches.
//
// A row is live when every part id is below its part's bound; the id is compared before it is used for anything, and it is
// never an index: it only becomes a field of the code.  Whatever bits the part arrays hold, loads stay inside
// rows * width bytes of each part and stores inside rows * id_width bytes of `ids`.
// The code 0 — the tuple of all zeros — is the empty slot's value and goes through the existing flag (KeyState.has_zero,
// raised by key_offer / key_store, placed first by k_key_finish); codes are not offset by one.
// The set lives as long as the workgroup: a tuple reaches the global table once per workgroup, not once per 256 rows, and
// there is no global atomic per row.  Behind the overflow flag rows are only counted.  A lane loads its row's id from each
// part: a wave reads 64 neighbouring ids per part and load, coalesced at every width.
//
// LDS:  k_comb_collect  16 KiB set + the reduction's words = 16672 B     8 workgroups per CU (the 32 waves of a CU; LDS allows 9)
//       k_comb_assign   8 KiB codes = 8192 B                              8
// VGPRs (the compiler's resource-usage remarks, gfx950): k_comb_collect 24, k_comb_assign 10; no scratch, no spills.
// (DESIGN 4l has what the probe measured)
#pragma once

namespace sb {

constexpr uint32_t COMB_GRID = 2048;   // workgroups per item at most: 8 per CU, each with a set of its own

__device__ __forceinline__ uint32_t comb_load(const uint8_t* p, uint32_t w, uint64_t row) {
    if (w == 1) return p[row];
    if (w == 2) return ((const uint16_t*)p)[row];
    return ((const uint32_t*)p)[row];
}
// the code of row `row`; false: a part id is at or above its bound, the row is not live
__device__ __forceinline__ bool comb_row_code(const CombItem& it, uint64_t row, uint64_t* code) {
    uint32_t id[COMB_MAX_PARTS];
    bool live = true;
#pragma unroll
    for (uint32_t p = 0; p < COMB_MAX_PARTS; p++) {
        id[p] = 0;
        if (p < it.n_parts) {
            id[p] = comb_load(it.part[p], it.width[p], row);
            live = live && id[p] < it.bound[p];
        }
    }
    // (comb_pack's shifts, with the unused trailing parts left out)
    uint64_t c = 0;
#pragma unroll
    for (uint32_t p = 0; p < COMB_MAX_PARTS; p++)
        if (p < it.n_parts) c = (c << COMB_FIELD_BITS) | (uint64_t)(id[p] & (KEY_MAX_KEYS - 1));
    *code = c;
    return live;
}

__global__ void __launch_bounds__(WG) k_comb_collect(CombLaunch cl) {
    __shared__ uint64_t s_w64[4];
    __shared__ uint64_t s_set[KEY_SET_SLOTS];
    const uint32_t item = blockIdx.y;
    const CombItem it = cl.items[item];
    const uint64_t rows = cl.kl.acols[item].rows;
    key_set_clear(s_set);
    __syncthreads();
    KeySink s = key_sink(cl.kl, item, s_set, nullptr, nullptr, 0);
    // (base is the workgroup's: every lane of a wave takes the same number of steps, as key_offer's shuffle needs)
    for (uint64_t base = (uint64_t)blockIdx.x * WG; base < rows; base += (uint64_t)gridDim.x * WG) {
        const uint64_t r = base + threadIdx.x;
        uint64_t code = 0;
        bool on = r < rows && comb_row_code(it, r, &code);
        if (on) s.cnt++;
        if (key_over(s.st)) on = false;
        key_offer(s, on, on ? code : 0ull);
    }
    key_store(s, s_w64);
}

__global__ void __launch_bounds__(WG) k_comb_assign(CombLaunch cl) {
    __shared__ uint64_t s_keys[KEY_MAX_KEYS];
    const uint32_t item = blockIdx.y;
    if (cl.kl.st[item].overflow) return;   // (the ids are unspecified then)
    const CombItem it = cl.items[item];
    const AggCol g = cl.kl.acols[item];
    const KeyCol kc = cl.kl.kcols[item];
    const KeyFind f = key_stage(cl.kl, item, g, s_keys);
    __syncthreads();
    for (uint64_t r = (uint64_t)blockIdx.x * WG + threadIdx.x; r < g.rows; r += (uint64_t)gridDim.x * WG) {
        uint64_t code = 0;
        const bool on = comb_row_code(it, r, &code);
        key_id_store(kc.ids, kc.idw, r, on ? key_find(f, code) : 0xFFFFFFFFu);
    }
}

static uint32_t comb_grid(uint64_t max_rows) { return (uint32_t)std::min<uint64_t>(COMB_GRID, std::max<uint64_t>(1, (max_rows + WG - 1) / WG)); }

// the three phases of a call, between launch_key_zero and the readback of `results` (k_key_finish's records)
void launch_key_combine(sb_ctx* ctx, const CombLaunch& cl, uint64_t* results) {
    hipStream_t s = ctx->stream;
    launch_key_zero(ctx, cl.kl);
    const dim3 grid(comb_grid(cl.max_rows), cl.kl.n_cols);
    {
        KScope k(ctx, "k_comb_collect");
        k_comb_collect<<<grid, WG, 0, s>>>(cl);
    }
    launch_key_finish(ctx, cl.kl, results);
    {
        KScope k(ctx, "k_comb_assign");
        k_comb_assign<<<grid, WG, 0, s>>>(cl);
    }
}

}  // namespace sb
