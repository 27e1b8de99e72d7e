"""sb_topk_columns on the GPU: pages written by the CPU oracle, the k best of the selected rows found on the device,
compared with the ORACLE's decode of the pages ordered by numpy (tests/topk_ref.py: np.lexsort on (row, key), checked on
its own against a brute-force sort in tests/test_topk_host.py).  Nothing here is compared with what the device's own
decoder or sb_read_selected give, except in the end-to-end test, which says so.

Every comparison is exact: the row numbers, the value bytes, found / count / nans / selected, and the zeroed tail of
`out`.  Unless a test says otherwise a column has 10 000 rows and runs under a random ~0.35 selection, a sparse one that
leaves whole tiles and pages out, and no selection at all, in both orders and at k = 1, 7, 64 and 256: 24 columns of one
call."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import sbo as S
from tests import gen
from tests import topk_ref as T
from tests.test_gpu_aggregate import bitmap
from tests.test_gpu_decode import LONG_RLE_ROWS
from tests.test_gpu_read_selected import PAGES, TYPES, oracle_code, read_code, two_masks, upload

pytestmark = pytest.mark.gpu

NP = gen.NP_OF
SENTINEL = 0x5A
WORD = 0x5A5A5A5A5A5A5A5A
RESULTS = ("rows", "selected", "count", "nans", "found")


def run(ctx, cps, masks, refs, ks, orders, what=""):
    """the columns of ONE call, each under its own selection (None: no selection), k and order, against their references"""
    import strawboat_amd as sb
    res = sb.topk_columns(ctx, cps, list(ks), list(orders), [bitmap(ctx, m) for m in masks])
    ctx.synchronize()
    for i, (r, ref, m, k, lg) in enumerate(zip(res, refs, masks, ks, orders)):
        T.check(r, T.want(ref, m, k, lg), "%s column %d (k %d, %s)" % (what, i, k, "largest" if lg else "smallest"))
    return res


def check_pages(ctx, col, pages, metas, masks=None, ks=T.KS, what=""):
    ref = T.Ref(col, pages, metas)
    if masks is None:
        masks = two_masks(ref.rows, 11) + [None]
    cp = upload(ctx, col, pages, metas)
    combos = [(m, k, lg) for m in masks for lg in (False, True) for k in ks]
    n = len(combos)
    return run(ctx, [cp] * n, [c[0] for c in combos], [ref] * n, [c[1] for c in combos], [c[2] for c in combos], what)


def check(ctx, col, codec=None, masks=None, ks=T.KS, **opt):
    pages, metas = gen.oracle_write(col, **opt)
    if codec is not None:
        seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
        assert seen == {codec}, (seen, codec)
    return check_pages(ctx, col, pages, metas, masks, ks, what="codec %r %r" % (codec, opt))


def _column(ptype, values, validity=None):
    values = np.asarray(values, NP[ptype])
    return dict(ptype=ptype, nullable=validity is not None, rows=values.size, values=values,
                validity=None if validity is None else gen.pack_bits(validity), offsets=None)


# ---- 1: codecs x types
@pytest.mark.parametrize("ptype", TYPES)
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT, S.ONEVALUE])
def test_prim_codecs(gpu_ctx, ptype, codec):
    uniq = 1 if codec == S.ONEVALUE else 100
    for nd, page in ((0.2, 4100), (None, 2050)):
        col = gen.prim(ptype, 10_000, uniq=uniq, null_density=nd, runs=8 if nd else 3, seed=page)
        check(gpu_ctx, col, codec=codec, max_page_size=page, force_codec=codec)


@pytest.mark.parametrize("ptype", [S.T_I32, S.T_U32])
@pytest.mark.parametrize("codec", [S.BITPACK, S.DELTABP])
def test_bitpacking(gpu_ctx, ptype, codec):
    col = gen.prim(ptype, 128 * 100, uniq=1 << 13, sorted_=(codec == S.DELTABP))
    check(gpu_ctx, col, codec=codec, max_page_size=128 * 40, force_codec=codec)


@pytest.mark.parametrize("icodec", [S.NONE, S.RLE, S.BITPACK, S.DELTABP, S.ONEVALUE, S.LZ4])
def test_dict_index_codecs(gpu_ctx, icodec):
    uniq = 1 if icodec == S.ONEVALUE else 200
    col = gen.prim(S.T_F64, 128 * 100, uniq=uniq, null_density=0.1, runs=16, sorted_=(icodec == S.DELTABP))
    check(gpu_ctx, col, codec=S.DICT, max_page_size=128 * 40, force_codec=S.DICT, force_index_codec=icodec)


@pytest.mark.parametrize("ptype", [S.T_I16, S.T_I64, S.T_F64])
@pytest.mark.parametrize("codec", [S.LZ4, S.ZSTD, S.SNAPPY])
def test_basic_pages_are_staged(gpu_ctx, ptype, codec):
    col = gen.prim(ptype, 10_000, uniq=300, null_density=0.2, runs=5, seed=codec)
    check(gpu_ctx, col, codec=codec, max_page_size=2050, force_codec=codec)


def test_patas_pages(gpu_ctx):
    rng = np.random.default_rng(3)
    v = np.round(rng.normal(100, 20, 10_000), 2)
    col = dict(ptype=S.T_F64, nullable=True, rows=v.size, values=v, validity=gen.make_validity(rng, v.size, 0.2), offsets=None)
    check(gpu_ctx, col, codec=S.PATAS, max_page_size=2050, force_codec=S.PATAS)


# ---- 2: ties
@pytest.mark.parametrize("codec", [S.ONEVALUE, S.NONE, S.RLE, S.DICT])
def test_ties_go_to_the_lowest_rows(gpu_ctx, codec):
    """one value everywhere, and three values: the winners are the lowest live row numbers of the best value"""
    uniq = 1 if codec == S.ONEVALUE else 3
    for ptype in (S.T_I32, S.T_F64):
        col = gen.prim(ptype, 10_000, uniq=uniq, null_density=0.2, seed=uniq)
        res = check(gpu_ctx, col, codec=codec, max_page_size=4100, force_codec=codec)
        for r in res:
            ids = r.row_ids.astype(np.int64)
            same = np.all(r.value_bytes == r.value_bytes[:1], axis=1)   # the winners that have the best value
            assert np.all(np.diff(ids[same]) > 0), "the best value's rows come in row order"
            if uniq == 1:
                assert same.all()


@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
@pytest.mark.parametrize("largest", [False, True])
def test_a_tie_group_that_straddles_the_kth_place_across_a_tile_seam_and_a_page_seam(gpu_ctx, codec, largest):
    rng = np.random.default_rng(codec)
    v = rng.integers(100, 1000, 8200).astype(np.int64)
    v[4090:4101] = 5000 if largest else 0   # rows 4090 .. 4100: the tile seam is at 4096, the page seam at 4100
    col = _column(S.T_I64, v)
    pages, metas = gen.oracle_write(col, max_page_size=4100, force_codec=codec)
    assert [int(n) for n in metas[:, 1]] == [4100, 4100]
    ref = T.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    ks = (1, 5, 6, 7, 10, 11, 12, 64)   # inside the group on either side of both seams, its last row, and beyond it
    odd = np.ones(8200, bool)
    odd[4091:4101:2] = False   # ... and with every other row of the group left out
    for mask in (None, odd):
        res = run(gpu_ctx, [cp] * len(ks), [mask] * len(ks), [ref] * len(ks), ks, [largest] * len(ks), what="tie group")
        group = [r for r in range(4090, 4101) if mask is None or mask[r]]
        for r, k in zip(res, ks):
            assert r.row_ids[:len(group)].tolist() == group[:k]


def test_long_rle_runs_and_the_parts_of_a_long_rle_page(gpu_ctx):
    # runs of three rows -- 1367 runs in a page of 4100 rows, two chunks of 1024 -- and one run of the best value that lies
    # across the chunk border, the tile seam and the page seam
    rng = np.random.default_rng(2)
    v = np.repeat(rng.integers(100, 1000, 3334), 3)[:10_000].astype(np.int32)
    v[3000:4700] = 7
    col = _column(S.T_I32, v, rng.random(10_000) >= 0.1)
    check(gpu_ctx, col, codec=S.RLE, max_page_size=4100, force_codec=S.RLE)
    v[3000:4700] = 5000
    check(gpu_ctx, _column(S.T_I32, v), codec=S.RLE, max_page_size=4100, force_codec=S.RLE)
    # one page that several workgroups share: a slot per part
    col = gen.prim(S.T_F64, LONG_RLE_ROWS, uniq=256, null_density=0.1, runs=32, seed=4)
    pages, metas = gen.oracle_write(col, force_codec=S.RLE)
    assert metas.shape[0] == 1
    check_pages(gpu_ctx, col, pages, metas, [rng.random(LONG_RLE_ROWS) < 0.002, None], ks=(7, 256), what="long page")


# ---- 3: fewer than k candidates
def test_fewer_candidates_than_k(gpu_ctx):
    rng = np.random.default_rng(3)
    for codec in (S.NONE, S.RLE, S.DICT):
        v = np.repeat(rng.normal(0, 50, 2500), 4)
        v[::3] = np.nan
        col = _column(S.T_F64, v, rng.random(10_000) >= 0.5)
        few = np.zeros(10_000, bool)
        few[rng.integers(0, 10_000, 90)] = True   # about 30 candidates: found < k for k = 64 and 256
        res = check(gpu_ctx, col, codec=codec, masks=[few, np.zeros(10_000, bool)], max_page_size=2050, force_codec=codec)
        assert any(0 < r.found < r.k for r in res) and all(r.out_bytes[16 * r.found:] == bytes(16 * (r.k - r.found)) for r in res)
        assert all(r.found == 0 and r.selected == 0 for r in res[len(res) // 2:])
        # every row null
        res = check(gpu_ctx, _column(S.T_F64, v, np.zeros(10_000, bool)), masks=[few, None], max_page_size=2050, force_codec=codec)
        assert all((r.count, r.found) == (0, 0) and r.out_bytes == bytes(16 * r.k) for r in res)


def test_columns_without_rows_or_pages_and_a_canary_behind_out(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd import _native as N
    from strawboat_amd import read
    dev = gpu_ctx.torch_device
    empty = read.ColumnPages(S.T_I64, True, torch.zeros(0, dtype=torch.uint8, device=dev), np.zeros((0, 2), np.uint64))
    for sel in (None, torch.zeros(0, dtype=torch.uint8, device=dev)):
        r = sb.topk_columns(gpu_ctx, [empty], 7, True, sel)[0]
        gpu_ctx.synchronize()
        assert (r.rows, r.selected, r.count, r.nans, r.found) == (0, 0, 0, 0, 0) and r.out_bytes == bytes(16 * 7)
    col = gen.prim(S.T_I32, 3000, uniq=500, null_density=0.3, seed=4)
    pages, metas = gen.oracle_write(col, max_page_size=777, force_codec=S.NONE)
    ref = T.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(1).random(3000) < 0.5
    res = sb.topk_columns(gpu_ctx, [empty, cp, empty], [3, 64, 256], False, [None, bitmap(gpu_ctx, mask), None])
    gpu_ctx.synchronize()
    assert (res[0].rows, res[0].found, res[2].selected) == (0, 0, 0) and res[2].out_bytes == bytes(16 * 256)
    T.check(res[1], T.want(ref, mask, 64, False), "next to empty columns")
    # the caller's array is longer than k: the entries behind out[k) keep their bytes, found or not
    for k, m in ((5, mask), (64, np.zeros(3000, bool)), (256, None)):
        batch = sb.TopKBatch(gpu_ctx, [cp], k, True, bitmap(gpu_ctx, m))
        out = (N.TopKRowC * (k + 3))()
        C.memset(out, SENTINEL, C.sizeof(out))
        batch._arr[0].out = out
        batch.enqueue()
        gpu_ctx.synchronize()
        w = T.want(ref, m, k, True)
        assert bytes(out)[:16 * k] == w.out_bytes and bytes(out)[16 * k:] == bytes([SENTINEL]) * 48
        assert batch._arr[0].found == w.found


# ---- 4: adversarial order: every step beats the bound
@pytest.mark.parametrize("codec", [S.NONE, S.RLE])
def test_values_sorted_against_the_requested_order(gpu_ctx, codec):
    rows = 10_000
    rep = 2 if codec == S.RLE else 1
    asc = np.repeat(np.arange(rows // rep, dtype=np.int64) * 3 - 7000, rep)
    for v, largest in ((asc, True), (asc[::-1].copy(), False)):
        col = _column(S.T_I64, v)
        pages, metas = gen.oracle_write(col, max_page_size=4100, force_codec=codec)
        ref = T.Ref(col, pages, metas)
        cp = upload(gpu_ctx, col, pages, metas)
        masks = two_masks(rows, 4) + [None]
        for k in T.KS:
            res = run(gpu_ctx, [cp] * 3, masks, [ref] * 3, [k] * 3, [largest] * 3, what="against the order")
            assert res[2].row_ids[0] == (rows - rep if codec == S.RLE else rows - 1)


# ---- 5: extremes
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_integer_extremes(gpu_ctx, codec):
    rng = np.random.default_rng(codec + 7)
    opt = dict(max_page_size=4100, force_codec=codec)
    runs = np.repeat(np.arange(10_000 // 5 + 1), 5)[:10_000]
    pool = np.array([-2 ** 63, 2 ** 63 - 1, -1, 0, 1, -2 ** 63 + 1, 2 ** 63 - 2], np.int64)
    v = pool[rng.integers(0, pool.size, 10_000)[runs]]
    res = check(gpu_ctx, _column(S.T_I64, v, rng.random(10_000) >= 0.2), codec=codec, **opt)
    assert int(res[-1].values[0]) == 2 ** 63 - 1 and int(res[-5].values[0]) == -2 ** 63   # (no selection: largest, smallest)
    v = (np.uint64(2 ** 64 - 1) - rng.integers(0, 50, 10_000).astype(np.uint64))[runs]
    res = check(gpu_ctx, _column(S.T_U64, v, rng.random(10_000) >= 0.1), codec=codec, **opt)
    assert int(res[-1].values[0]) > 2 ** 64 - 51
    for ptype, lo, hi in ((S.T_I8, -128, 127), (S.T_I16, -32768, 32767)):
        v = rng.integers(lo, lo // 2, 10_000)[runs]
        v[::97] = lo
        v[5::101] = hi
        res = check(gpu_ctx, _column(ptype, v, rng.random(10_000) >= 0.2), codec=codec, **opt)
        assert int(res[-5].values[0]) == lo and int(res[-1].values[0]) == hi
        assert not res[-5].value_bytes[:, np.dtype(NP[ptype]).itemsize:].any(), "zeros behind the value's width"


@pytest.mark.parametrize("ptype", [S.T_F32, S.T_F64])
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_float_specials(gpu_ctx, ptype, codec):
    dtype = NP[ptype]
    w = np.dtype(dtype).itemsize
    rng = np.random.default_rng(ptype)
    rows = 10_000
    v = np.repeat(rng.normal(0, 50, rows // 4 + 1), 4)[:rows].astype(dtype)
    nan_neg = np.array([(0xFFC00001 if w == 4 else 0xFFF8000000000001)], "<u%d" % w).view(dtype)[0]
    tiny = np.finfo(dtype).smallest_subnormal
    at = {10: np.nan, 4097: np.nan, 9000: np.nan, 11: nan_neg, 8300: nan_neg, 500: np.inf, 4095: np.inf, 4096: -np.inf,
          20: 0.0, 21: 0.0, 22: 0.0, 23: -0.0, 24: -0.0, 30: tiny, 31: -tiny}
    special = np.zeros(rows, bool)
    for r, x in at.items():
        v[r] = x
        special[r] = True
    valid = rng.random(rows) >= 0.1
    valid[special] = True
    col = _column(ptype, v, valid)
    pages, metas = gen.oracle_write(col, max_page_size=4100, force_codec=codec)
    ref = T.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    with_all = special | (rng.random(rows) < 0.3)
    zeros_only = np.zeros(rows, bool)
    zeros_only[20:25] = True
    nans_only = np.zeros(rows, bool)
    nans_only[[10, 4097, 9000, 11, 8300]] = True
    masks = [with_all, zeros_only, nans_only, None]
    for largest in (False, True):
        for k in (7, 256):
            res = run(gpu_ctx, [cp] * 4, masks, [ref] * 4, [k] * 4, [largest] * 4, what="float specials")
            assert res[0].nans == 5 and res[3].nans == 5 and not np.isnan(res[0].values).any()
            assert res[0].values[0] == (np.inf if largest else -np.inf)
            assert (res[2].count, res[2].nans, res[2].found) == (5, 5, 0) and res[2].out_bytes == bytes(16 * k)
            assert res[1].found == 5
            if np.signbit(ref.vals[23]) and not np.signbit(ref.vals[20]):   # (the pages kept the zeros' signs)
                assert res[1].row_ids.tolist() == ([20, 21, 22, 23, 24] if largest else [23, 24, 20, 21, 22])


# ---- 6: Freq pages: the interval is issued again, the call's columns decoded and ordered
@pytest.mark.parametrize("ptype", [S.T_I32, S.T_I64])
def test_freq_pages(gpu_ctx, ptype):
    from tests.test_gpu_freq import sparse
    rows = 10_000
    f = sparse(ptype, rows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    assert S.FREQ in set(int(x) for x in S.stat_column(f["ptype"], f["nullable"], fp, fm)[0].tolist())
    b = gen.prim(S.T_I64, rows, uniq=100, null_density=0.2, runs=6, seed=2)
    bp, bm = gen.oracle_write(b, max_page_size=4100, force_codec=S.RLE)
    fref, bref = T.Ref(f, fp, fm), T.Ref(b, bp, bm)
    fcp, bcp = upload(gpu_ctx, f, fp, fm), upload(gpu_ctx, b, bp, bm)
    mask = np.random.default_rng(ptype).random(rows) < 0.3
    for k, largest in ((7, False), (256, True)):
        r0 = gpu_ctx.replays()
        run(gpu_ctx, [fcp, bcp, fcp], [mask, mask, None], [fref, bref, fref], [k, 64, k], [largest, not largest, largest], what="freq")
        assert gpu_ctx.replays() == r0 + 1
    # a Freq column without a selected row: the replay all the same
    r0 = gpu_ctx.replays()
    run(gpu_ctx, [fcp, bcp], [np.zeros(rows, bool), mask], [fref, bref], [7, 7], [False, False], what="freq, nothing selected")
    assert gpu_ctx.replays() == r0 + 1


# ---- 7: the same bytes every time
def test_the_same_bytes_every_time(gpu_ctx):
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows = 10_000
    rng = np.random.default_rng(7)
    cols = [(gen.prim(S.T_F64, rows, uniq=40, null_density=0.2, seed=1), S.NONE), (gen.prim(S.T_I16, rows, uniq=3, seed=2), S.DICT),
            (gen.prim(S.T_I64, rows, uniq=20, null_density=0.1, runs=6, seed=3), S.RLE)]
    cps, refs = [], []
    for col, codec in cols:
        pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
        cps.append(upload(gpu_ctx, col, pages, metas))
        refs.append(T.Ref(col, pages, metas))
    mask = rng.random(rows) < 0.35
    ks, orders = [256, 64, 7], [True, False, True]
    batch = sb.TopKBatch(gpu_ctx, cps, ks, orders, bitmap(gpu_ctx, mask))
    seen = []
    for _ in range(3):   # fresh intervals
        res = batch.enqueue()
        gpu_ctx.synchronize()
        seen.append([r.out_bytes for r in res])
    # ... and in an interval that a filter call's Freq column causes to be issued again
    x = sparse(S.T_I32, rows, 0.05, 2, null_density=0.1)
    xp, xm = gen.oracle_write(x, max_page_size=2050, force_codec=S.FREQ)
    r0 = gpu_ctx.replays()
    sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("ne", 7)])
    res = batch.enqueue()
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    seen.append([r.out_bytes for r in res])
    assert all(s == seen[0] for s in seen[1:])
    for r, ref, k, lg in zip(res, refs, ks, orders):
        T.check(r, T.want(ref, mask, k, lg), "in the replayed interval")


# ---- 8: several columns with their own k and order in one call (the slots hold the largest k)
def test_columns_with_different_k_and_order_in_one_call(gpu_ctx):
    rng = np.random.default_rng(8)
    cps, refs = [], []
    for ptype, codec, page in ((S.T_I64, S.NONE, 4100), (S.T_F32, S.DICT, 2050), (S.T_U16, S.RLE, 2050), (S.T_F64, S.LZ4, 2050)):
        col = gen.prim(ptype, 10_000, uniq=300, null_density=0.2, runs=5, seed=page + ptype)
        pages, metas = gen.oracle_write(col, max_page_size=page, force_codec=codec)
        cps.append(upload(gpu_ctx, col, pages, metas))
        refs.append(T.Ref(col, pages, metas))
    masks = [rng.random(10_000) < 0.35, None, two_masks(10_000, 3)[1], rng.random(10_000) < 0.9]
    for ks, orders in (([1, 256, 7, 64], [True, False, False, True]), ([200, 3, 3, 2], [False, True, True, False]),
                       ([5, 5, 5, 5], [True, True, False, False])):
        run(gpu_ctx, cps, masks, refs, ks, orders, what="k %r" % (ks,))
        run(gpu_ctx, cps[::-1], masks[::-1], refs[::-1], ks, orders, what="k %r, the columns turned round" % (ks,))


# ---- 9: the filter call that writes the selection is earlier in the same interval
def test_filter_then_topk_in_one_interval(gpu_ctx):
    import strawboat_amd as sb
    rows = 10_007
    x = gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    y = gen.prim(S.T_F64, rows, uniq=5000, null_density=0.1, seed=2)
    xp, xm = gen.oracle_write(x, max_page_size=2050, force_codec=S.RLE)
    yp, ym = gen.oracle_write(y, max_page_size=4100, force_codec=S.NONE)
    xr, yr = T.Ref(x, xp, xm), T.Ref(y, yp, ym)
    mask = (xr.vals < 60) & xr.valid
    assert 0 < mask.sum() < rows
    ycp = upload(gpu_ctx, y, yp, ym)
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("lt", 60)])
    res = sb.topk_columns(gpu_ctx, [ycp, ycp], [10, 256], [True, False], sel[0])
    gpu_ctx.synchronize()   # (the only one)
    assert np.array_equal(sel[0].numpy(), mask)
    T.check(res[0], T.want(yr, mask, 10, True), "behind the filter")
    T.check(res[1], T.want(yr, mask, 256, False), "behind the filter")


# ---- 10: filter -> top-k -> the winners' bitmap -> the selected read of another column
def test_end_to_end_the_other_columns_of_the_winners(gpu_ctx):
    import strawboat_amd as sb
    rows = 10_000
    x = gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    y = gen.prim(S.T_F64, rows, uniq=400, null_density=0.1, seed=2)   # (ties among the winners)
    z = gen.prim(S.T_I64, rows, uniq=1 << 40, null_density=0.1, seed=3)
    xp, xm = gen.oracle_write(x, max_page_size=2050, force_codec=S.RLE)
    yp, ym = gen.oracle_write(y, max_page_size=4100, force_codec=S.DICT)
    zp, zm = gen.oracle_write(z, max_page_size=2050, force_codec=S.NONE)
    xr, yr, zr = T.Ref(x, xp, xm), T.Ref(y, yp, ym), T.Ref(z, zp, zm)
    mask = (xr.vals >= 30) & xr.valid
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("ge", 30)])
    top = sb.topk_columns(gpu_ctx, [upload(gpu_ctx, y, yp, ym)], 50, True, sel[0])[0]
    gpu_ctx.synchronize()
    want = T.want(yr, mask, 50, True)
    T.check(top, want, "order by y desc limit 50")
    winners = sb.selection_of_rows(gpu_ctx, rows, top.row_ids)
    arr = sb.read_selected(gpu_ctx, [upload(gpu_ctx, z, zp, zm)], winners)[0]
    gpu_ctx.synchronize()
    vals, valid = arr.numpy()
    ids = want.row_ids.astype(np.int64)
    assert arr.selected == 50 and winners.selected == 50
    in_rank = np.argsort(np.argsort(ids))   # row order -> rank order, as selection_of_rows' docstring has it
    assert np.array_equal(valid[in_rank], zr.valid[ids])
    assert np.array_equal(vals[in_rank][zr.valid[ids]], zr.vals[ids][zr.valid[ids]])


# ---- 11: refusals through the raw C call
def _raw(ctx, cps, bitmaps, k=7):
    import strawboat_amd as sb
    from strawboat_amd import _native as N
    batch = sb.TopKBatch(ctx, cps, k, False, bitmaps)
    batch._outs = []
    for i in range(len(cps)):
        out = (N.TopKRowC * k)()
        C.memset(out, SENTINEL, C.sizeof(out))
        batch._arr[i].out = out
        batch._outs.append(out)
        for f in RESULTS:
            setattr(batch._arr[i], f, WORD)
    return batch


def _sentinels_kept(batch):
    for c, out in zip(batch._arr, batch._outs):
        assert all(getattr(c, f) == WORD for f in RESULTS)
        assert bytes(out) == bytes([SENTINEL]) * C.sizeof(out)


def test_refusals_at_the_call(gpu_ctx):
    from strawboat_amd import _native as N
    col = gen.prim(S.T_I64, 5000, uniq=10, null_density=0.2)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.NONE)
    ref = T.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(9).random(5000) < 0.5
    bm = bitmap(gpu_ctx, mask)

    def fresh(cps=None):
        return _raw(gpu_ctx, cps or [cp, cp], [bm, bm])

    def refused(batch, code, what, mem=N.SB_MEM_DEVICE):
        assert gpu_ctx._lib.sb_topk_columns(gpu_ctx._h, batch._arr, 2, mem) == code, what
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        _sentinels_kept(batch)

    for k in (0, 257, 1 << 31):
        batch = fresh()
        batch._arr[1].k = k
        refused(batch, N.SB_ERR_INVALID, "k %d" % k)
    for order in (2, 0xFFFFFFFF):
        batch = fresh()
        batch._arr[1].order = order
        refused(batch, N.SB_ERR_INVALID, "unknown order")
    batch = fresh()
    batch._arr[1].reserved = 1
    refused(batch, N.SB_ERR_INVALID, "reserved != 0")
    batch = fresh()
    batch._arr[0].out = None
    refused(batch, N.SB_ERR_INVALID, "out null")
    for bad in (-1, S.T_NULL + 1, 99):
        batch = fresh()
        batch._arr[0].physical_type = bad
        refused(batch, N.SB_ERR_INVALID, "bad physical_type %d" % bad)
    batch = fresh()
    batch._arr[1].selection += 1
    refused(batch, N.SB_ERR_INVALID, "misaligned selection")
    batch = fresh()
    batch._arr[1].selection_capacity = (5000 + 31) // 32 * 4 - 4
    refused(batch, N.SB_ERR_INVALID, "short selection_capacity")
    batch = fresh()
    batch._arr[0].metas = None
    refused(batch, N.SB_ERR_INVALID, "metas null with n_pages > 0")
    for ptype in (S.T_BOOL, S.T_I128, S.T_I256, S.T_BIN32, S.T_BIN64, S.T_NULL):
        batch = fresh()
        batch._arr[1].physical_type = ptype
        refused(batch, N.SB_ERR_NYI, "type %d" % ptype)
    batch = fresh()
    refused(batch, N.SB_ERR_NYI, "SB_MEM_HOST", mem=N.SB_MEM_HOST)
    # a page outside [0, pages_len): the span check of the read calls' host tables
    batch = fresh()
    batch._arr[1].pages_len -= 1
    assert gpu_ctx._lib.sb_topk_columns(gpu_ctx._h, batch._arr, 2, N.SB_MEM_DEVICE) == N.SB_ERR_IO
    _sentinels_kept(batch)
    with pytest.raises(N.NativeError) as e:   # (like its siblings', this refusal is the interval's result as well)
        gpu_ctx.synchronize()
    assert e.value.code == N.SB_ERR_IO
    # the same batch, as it was built, then succeeds
    batch = fresh()
    res = batch.enqueue()
    gpu_ctx.synchronize()
    for r, out in zip(res, batch._outs):
        assert bytes(out) == T.want(ref, mask, 7, False).out_bytes and r.found == 7


# ---- 12: errors at the synchronize
def topk_code(ctx, cp, rows, sel=True):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    try:
        sb.topk_columns(ctx, [cp], 7, False, bitmap(ctx, np.ones(rows, bool)) if sel else None)
        ctx.synchronize()
    except NativeError as e:
        try:
            ctx.synchronize()
        except NativeError:
            pass
        return e.code
    return 0


def test_a_truncated_page_raises_what_the_decoder_raises(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    for codec in (S.NONE, S.RLE, S.DICT, S.LZ4):
        col = gen.prim(S.T_I64, 9000, uniq=60, null_density=0.1, runs=6)
        pages, metas = gen.oracle_write(col, max_page_size=3000, force_codec=codec)
        m = np.array(metas, np.uint64).copy()
        cut = int(m[-1, 0]) // 2
        m[-1, 0] -= cut
        bad = pages[:pages.size - cut].copy()
        cp = upload(gpu_ctx, col, bad, m)
        want = read_code(gpu_ctx, cp)
        oc = oracle_code(col, bad, m)
        assert want != 0 and oc != 0 and (oc is None or oc == want), (codec, want, oc)
        assert topk_code(gpu_ctx, cp, 9000) == want, codec
        assert topk_code(gpu_ctx, cp, 9000, sel=False) == want, codec
        # rows and selected are delivered even when the interval failed
        sel = np.random.default_rng(12).random(9000) < 0.5
        res = sb.topk_columns(gpu_ctx, [cp], 7, True, bitmap(gpu_ctx, sel))
        with pytest.raises(NativeError):
            gpu_ctx.synchronize()
        assert res[0].rows == 9000 and res[0].selected == int(sel.sum())
    # the context still works
    check(gpu_ctx, gen.prim(S.T_I64, 9000, uniq=60), max_page_size=3000, force_codec=S.DICT)


# ---- 13: a context whose read path holds launch hints
def test_on_a_context_that_holds_launch_hints(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd import read
    ctx = sb.Context(0)
    try:
        col = gen.prim(S.T_F64, 200_000, uniq=50, null_density=0.1, runs=40, seed=5)
        pages, metas = gen.oracle_write(col, max_page_size=65536, force_codec=S.RLE)
        plain = gen.prim(S.T_I64, 50_000, uniq=1 << 40, seed=6)
        pp, pm = gen.oracle_write(plain, max_page_size=65536, force_codec=S.NONE)
        ref, pref = T.Ref(col, pages, metas), T.Ref(plain, pp, pm)
        cp, pcp = upload(ctx, col, pages, metas), upload(ctx, plain, pp, pm)
        mask = np.random.default_rng(13).random(200_000) < 0.35
        for _ in range(3):   # the hints now say: RLE pages alone, no tiles
            read.read_simple(ctx, cp)
        r0 = ctx.replays()
        # a column of tiles: a read call would be issued again for it; this call goes by no hint
        run(ctx, [cp, pcp], [mask, None], [ref, pref], [64, 7], [True, False], what="behind reads")
        assert ctx.replays() == r0
        # ... and feeds none: the read path still holds "RLE pages alone", so the same RLE read is right without a replay,
        # and the first read of the column of tiles is the one that is issued again
        want, pwant = gen.oracle_read(col, pages, metas), gen.oracle_read(plain, pp, pm)
        got = read.read_simple(ctx, cp)
        assert np.array_equal(got.values_numpy(), want["values"]) and ctx.replays() == r0
        if os.environ.get("SB_NO_HINTS", "0") == "0":
            got = read.read_simple(ctx, pcp)
            assert np.array_equal(got.values_numpy(), pwant["values"]) and ctx.replays() == r0 + 1
    finally:
        ctx.close()
