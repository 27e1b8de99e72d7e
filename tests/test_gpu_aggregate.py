"""sb_aggregate_columns on the GPU: pages written by the CPU oracle (hand-built where noted), count / min / max / sum of the
selected rows computed on the device, compared with the ORACLE's decode of the pages reduced by numpy and Python
(tests/aggregate_ref.py: Python ints for integer sums, math.fsum for float sums).  Nothing here is compared with what the
device's own decoder or sb_read_selected give.

Every case checks all of rows / selected / count / nans / min / max / sum.  Integers, the counts and the bytes of float
min / max are compared exactly; a float sum over finite data must lie within n * 2^-52 * sum|x| of math.fsum, n = count:
the bound any order of double additions satisfies (derived in aggregate_ref.float_sum_bound, not measured).  Unless a test
says otherwise every column runs under a random ~0.35 selection, a sparse one that leaves whole tiles and pages out, and
no selection at all, as three columns of one call."""
import ctypes as C

import numpy as np
import pytest

from oracle import sbo as S
from tests import aggregate_ref as R
from tests import buffer_cases, gen
from tests.test_gpu_decode import LONG_RLE_ROWS, RLE_OVERSHOOT, RLE_SHORT, _rle_page
from tests.test_gpu_read_selected import PAGES, TYPES, oracle_code, read_code, to_dev, two_masks, upload
from tests.test_read_selected_host import PAGE_ROWS, ROWS, bitmap_of, patterns

pytestmark = pytest.mark.gpu

NP = gen.NP_OF
SENTINEL = 0x5A


def bitmap(ctx, mask, tail=False):
    return None if mask is None else to_dev(ctx, bitmap_of(mask, tail))


def run(ctx, cps, masks, refs, ops=R.ALL, what="", tails=None):
    """the columns of ONE call, each under its own selection (None: no selection), checked against their references"""
    import strawboat_amd as sb
    tails = tails or [False] * len(cps)
    res = sb.aggregate_columns(ctx, cps, [bitmap(ctx, m, t) for m, t in zip(masks, tails)], ops=ops)
    ctx.synchronize()
    for i, (r, ref, m) in enumerate(zip(res, refs, masks)):
        R.check(r, ref.want(m, ops), "%s column %d" % (what, i))
    return res


def check_pages(ctx, col, pages, metas, masks=None, ops=R.ALL, what=""):
    ref = R.Ref(col, pages, metas)
    if masks is None:
        masks = two_masks(ref.rows, 11) + [None]
    cp = upload(ctx, col, pages, metas)
    return run(ctx, [cp] * len(masks), masks, [ref] * len(masks), ops, what)


def check(ctx, col, codec=None, masks=None, ops=R.ALL, **opt):
    pages, metas = gen.oracle_write(col, **opt)
    if codec is not None:
        seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
        assert seen == {codec}, (seen, codec)
    return check_pages(ctx, col, pages, metas, masks, ops, what="codec %r %r" % (codec, opt))


# ---- 1: codecs x types
@pytest.mark.parametrize("ptype", TYPES)
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT, S.ONEVALUE])
def test_prim_codecs(gpu_ctx, ptype, codec):
    uniq = 1 if codec == S.ONEVALUE else 100
    for nd, page in [(nd, page) for nd in (0.2, None) for page in PAGES]:
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


# ---- 2: selection patterns (the list is pinned on the CPU: tests/test_read_selected_host.py)
@pytest.mark.parametrize("page_rows,codec", [(PAGE_ROWS[1], S.RLE), (PAGE_ROWS[0], S.NONE), (PAGE_ROWS[1], S.NONE), (PAGE_ROWS[1], S.DICT)])
def test_selection_patterns(gpu_ctx, page_rows, codec):
    col = gen.prim(S.T_I64, ROWS, uniq=100, null_density=0.2, runs=6 if codec == S.RLE else None, seed=page_rows)
    pages, metas = gen.oracle_write(col, max_page_size=page_rows, force_codec=codec)
    assert [int(n) for n in metas[:-1, 1]] == [page_rows] * (metas.shape[0] - 1)
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    pats = patterns(ROWS, page_rows)
    masks = [m for _, m, _ in pats] + [None]
    res = run(gpu_ctx, [cp] * len(masks), masks, [ref] * len(masks), what="patterns", tails=[t for _, _, t in pats] + [False])
    by_name = dict((name, r) for (name, _, _), r in zip(pats, res))
    for name in ("zeros", "zeros, bits behind the rows set"):
        r = by_name[name]
        assert (r.selected, r.count, r.nans) == (0, 0, 0) and r.min_bytes == r.max_bytes == bytes(8), name
        assert (r._c.sum_lo, r._c.sum_hi) == (0, 0) and r.min is None and r.max is None and r.sum == 0, name
    ones, none = by_name["ones"], res[-1]   # "ones" equals no selection
    assert ones.selected == none.selected == ROWS
    assert (ones.count, ones.min_bytes, ones.max_bytes, ones.sum) == (none.count, none.min_bytes, none.max_bytes, none.sum)
    assert by_name["bits behind the rows set"].selected == int(pats[13][1].sum())   # tail bits behind `rows` are ignored


# ---- 3: extremes
def _column(ptype, values, validity=None):
    values = np.asarray(values, NP[ptype])
    return dict(ptype=ptype, nullable=validity is not None, rows=values.size, values=values,
                validity=None if validity is None else gen.pack_bits(validity), offsets=None)


@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_extremes(gpu_ctx, codec):
    rng = np.random.default_rng(codec + 7)
    opt = dict(max_page_size=4100, force_codec=codec)
    runs = np.repeat(np.arange(10_000 // 5 + 1), 5)[:10_000]
    # the 64-bit sum wraps, the 128-bit sum does not
    pool = np.array([-2 ** 63, 2 ** 63 - 1, -1, 0], np.int64)
    v = pool[rng.integers(0, 4, 10_000)[runs]]
    res = check(gpu_ctx, _column(S.T_I64, v, rng.random(10_000) >= 0.2), codec=codec, **opt)
    assert res[2].min == -2 ** 63 and res[2].max == 2 ** 63 - 1
    mostly_min = np.where(rng.random(10_000)[runs] < 0.9, -2 ** 63, 2 ** 63 - 1).astype(np.int64)
    res = check(gpu_ctx, _column(S.T_I64, mostly_min), codec=codec, **opt)
    assert res[2].sum < -2 ** 64 and res[2].min == -2 ** 63   # below what 64 bits hold
    # U64 near 2^64 - 1
    v = (np.uint64(2 ** 64 - 1) - rng.integers(0, 50, 10_000).astype(np.uint64))[runs]
    res = check(gpu_ctx, _column(S.T_U64, v, rng.random(10_000) >= 0.1), codec=codec, **opt)
    assert res[2].sum > 2 ** 64 * 8000 and res[2].max > 2 ** 63
    # I8 / I16 with negative minima: sign extension in min / max / sum
    for ptype, lo, hi in ((S.T_I8, -128, 127), (S.T_I16, -32768, 32767)):
        v = rng.integers(lo, lo // 2, 10_000)[runs]
        v[::97] = lo
        v[5::101] = hi
        res = check(gpu_ctx, _column(ptype, v, rng.random(10_000) >= 0.2), codec=codec, **opt)
        assert res[2].min == lo and res[2].max == hi and res[2].sum < 0
        res = check(gpu_ctx, _column(ptype, np.minimum(v, -1)), codec=codec, **opt)
        assert res[2].max < 0 and res[2].sum < 0


@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_selected_rows_that_are_all_null(gpu_ctx, codec):
    rng = np.random.default_rng(3)
    valid = rng.random(10_000) >= 0.3
    valid[4000:4300] = False
    col = _column(S.T_I32, np.repeat(rng.integers(-1000, 1000, 2000), 5), valid)
    only_nulls = ~valid & (rng.random(10_000) < 0.5)
    stretch = np.zeros(10_000, bool)
    stretch[4050:4250] = True   # across the tile seam of the first page
    res = check(gpu_ctx, col, codec=codec, masks=[only_nulls, stretch], max_page_size=4100, force_codec=codec)
    for r in res:
        assert r.selected > 0 and r.count == 0 and r.min is None and r.max is None and r.sum == 0
        assert r.min_bytes == r.max_bytes == bytes(8)


# ---- 4: floats
def _specials(dtype):
    w = np.dtype(dtype).itemsize
    nan_neg = np.array([(0xFFC00001 if w == 4 else 0xFFF8000000000001)], "<u%d" % w).view(dtype)[0]
    tiny = np.finfo(dtype).smallest_subnormal
    return [np.nan, nan_neg, np.inf, -np.inf, 0.0, -0.0, tiny, -tiny]


@pytest.mark.parametrize("ptype", [S.T_F32, S.T_F64])
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_float_specials(gpu_ctx, ptype, codec):
    dtype = NP[ptype]
    rng = np.random.default_rng(ptype)
    rows = 10_000
    v = np.repeat(rng.normal(0, 50, rows // 4 + 1), 4)[:rows].astype(dtype)
    at = {"nan": [10, 4097, 9000], "nan_neg": [11, 8300], "inf": [500, 4095], "-inf": [4096], "zero": [20, 21, 22], "-zero": [23, 24],
          "tiny": [30], "-tiny": [31]}
    sp = dict(zip(("nan", "nan_neg", "inf", "-inf", "zero", "-zero", "tiny", "-tiny"), _specials(dtype)))
    special = np.zeros(rows, bool)
    for name, idx in at.items():
        v[idx] = sp[name]
        special[idx] = True
    valid = rng.random(rows) >= 0.1
    valid[special] = True
    col = _column(ptype, v, valid)
    pages, metas = gen.oracle_write(col, max_page_size=4100, force_codec=codec)
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    with_all = special | (rng.random(rows) < 0.3)
    without = ~special & (rng.random(rows) < 0.3)
    zeros_only = np.zeros(rows, bool)
    zeros_only[20:25] = True
    pos_inf = without.copy()
    pos_inf[at["inf"]] = True
    neg_inf = without.copy()
    neg_inf[at["-inf"]] = True
    nans_only = np.zeros(rows, bool)
    nans_only[at["nan"] + at["nan_neg"]] = True
    masks = [with_all, without, zeros_only, pos_inf, neg_inf, nans_only, None]
    res = run(gpu_ctx, [cp] * len(masks), masks, [ref] * len(masks), what="float specials")
    w = np.dtype(dtype).itemsize
    assert res[0].nans == 5 and res[0].sum != res[0].sum and res[0].min == -np.inf and res[0].max == np.inf
    assert res[1].nans == 0 and np.isfinite(res[1].sum)
    assert res[2].count == 5
    if np.signbit(ref.vals[23]) and not np.signbit(ref.vals[20]):   # (the pages kept the zeros' signs)
        assert res[2].min_bytes[:w] == dtype(-0.0).tobytes() and res[2].max_bytes[:w] == dtype(0.0).tobytes()
    assert res[3].sum == np.inf and res[3].max == np.inf and res[4].sum == -np.inf and res[4].min == -np.inf
    assert res[5].count == 5 and res[5].nans == 5 and res[5].min is None and res[5].max is None and res[5].sum != res[5].sum
    assert res[5].min_bytes == res[5].max_bytes == bytes(8)


@pytest.mark.parametrize("ptype", [S.T_F32, S.T_F64])
@pytest.mark.parametrize("codec", [S.NONE, S.DICT, S.RLE])
def test_float_sums_that_are_exact_in_no_order(gpu_ctx, ptype, codec):
    import strawboat_amd as sb
    rng = np.random.default_rng(codec * 10 + ptype)
    rows = 10_000
    x = rng.normal(size=rows // 2) * 10.0 ** rng.integers(-3, 6, rows // 2)
    v = np.repeat(x, 2).astype(NP[ptype])   # (runs of two, so that RLE and Dict pages can hold it)
    col = _column(ptype, v, rng.random(rows) >= 0.1)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
    assert set(int(c) for c in S.stat_column(ptype, True, pages, metas)[0].tolist()) == {codec}
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    masks = two_masks(rows, 11) + [None]
    res = run(gpu_ctx, [cp] * 3, masks, [ref] * 3, what="inexact float sums")
    # the identical call issued twice gives the identical bits
    batch = sb.AggregateBatch(gpu_ctx, [cp] * 3, [bitmap(gpu_ctx, m) for m in masks])
    first = [(r._c.sum_lo, r.min_bytes, r.max_bytes) for r in res]
    for _ in range(2):
        again = batch.enqueue()
        gpu_ctx.synchronize()
        assert [(r._c.sum_lo, r.min_bytes, r.max_bytes) for r in again] == first


@pytest.mark.parametrize("ptype", [S.T_F32, S.T_F64])
def test_a_float_freq_column_gives_the_same_bits_in_every_interval(gpu_ctx, ptype):
    """A column with a Freq page takes the decoded route whenever it is issued: alone, twice, next to another aggregate call
    and next to a filter call.  (A column without one stays on the page route next to it: tests/test_gpu_replay_routes.py.)"""
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows = 10_000
    f = sparse(ptype, rows, 0.05, 2, null_density=0.1)
    f["values"] = f["values"] * NP[ptype](0.1)   # (sums that are exact in no order: 0.7 on 95 % of the rows)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    if S.FREQ not in set(int(x) for x in S.stat_column(f["ptype"], f["nullable"], fp, fm)[0].tolist()):
        pytest.fail("the oracle wrote no Freq page for type %d" % ptype)
    fref = R.Ref(f, fp, fm)
    fcp = upload(gpu_ctx, f, fp, fm)
    b = gen.prim(S.T_F64, rows, uniq=100, null_density=0.2, runs=6, seed=2)
    bp, bm = gen.oracle_write(b, max_page_size=4100, force_codec=S.RLE)
    bcp = upload(gpu_ctx, b, bp, bm)
    mask = np.random.default_rng(ptype).random(rows) < 0.4
    bmp = bitmap(gpu_ctx, mask)
    batch = sb.AggregateBatch(gpu_ctx, [fcp, fcp], [bmp, None])
    seen = []
    for others in (0, 0, 1, 2):
        r0 = gpu_ctx.replays()
        if others == 1:
            sb.aggregate_columns(gpu_ctx, [bcp], bmp)
        if others == 2:
            sb.filter_columns(gpu_ctx, [fcp], [sb.Predicate("is_not_null")])
        res = batch.enqueue()
        gpu_ctx.synchronize()
        assert gpu_ctx.replays() == r0 + 1
        R.check(res[0], fref.want(mask), "Freq float column, selection")
        R.check(res[1], fref.want(None), "Freq float column, every row")
        seen.append([(r._c.sum_lo, r.min_bytes, r.max_bytes) for r in res])
    assert seen[1:] == seen[:1] * 3


# ---- 5: one long page (several workgroups share an RLE page)
@pytest.mark.parametrize("codec", [S.RLE, S.DICT])
def test_one_long_page(gpu_ctx, codec):
    col = gen.prim(S.T_F64, LONG_RLE_ROWS, uniq=256, null_density=0.1, runs=32, seed=4)
    pages, metas = gen.oracle_write(col, force_codec=codec)
    assert metas.shape[0] == 1
    rng = np.random.default_rng(codec)
    check_pages(gpu_ctx, col, pages, metas, [rng.random(LONG_RLE_ROWS) < 0.002], what="long page")
    col = gen.prim(S.T_I64, LONG_RLE_ROWS, uniq=256, null_density=0.1, runs=32, seed=5)
    pages, metas = gen.oracle_write(col, force_codec=codec)
    check_pages(gpu_ctx, col, pages, metas, [rng.random(LONG_RLE_ROWS) < 0.002, None], what="long page, i64")


# ---- 6: Freq pages: the interval is issued again, the call's columns decoded and reduced
@pytest.mark.parametrize("ptype", [S.T_I32, S.T_I64])
def test_freq_pages(gpu_ctx, ptype):
    from tests.test_gpu_freq import sparse
    rows = 10_000
    f = sparse(ptype, rows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    assert S.FREQ in set(int(x) for x in S.stat_column(f["ptype"], f["nullable"], fp, fm)[0].tolist())
    b = gen.prim(S.T_I64, rows, uniq=100, null_density=0.2, runs=6, seed=2)
    bp, bm = gen.oracle_write(b, max_page_size=4100, force_codec=S.RLE)
    fref, bref = R.Ref(f, fp, fm), R.Ref(b, bp, bm)
    fcp, bcp = upload(gpu_ctx, f, fp, fm), upload(gpu_ctx, b, bp, bm)
    mask = np.random.default_rng(ptype).random(rows) < 0.3
    r0 = gpu_ctx.replays()
    run(gpu_ctx, [fcp, bcp, fcp], [mask, mask, None], [fref, bref, fref], what="freq")
    assert gpu_ctx.replays() == r0 + 1
    # a sparse selection, and a Freq column without a selected row: the replay all the same
    for m in (two_masks(rows, 5)[1], np.zeros(rows, bool)):
        r0 = gpu_ctx.replays()
        run(gpu_ctx, [fcp, bcp], [m, mask], [fref, bref], what="freq, %d selected" % int(m.sum()))
        assert gpu_ctx.replays() == r0 + 1
    # count alone looks at no page body: no replay
    r0 = gpu_ctx.replays()
    run(gpu_ctx, [fcp], [mask], [fref], ops=("count",), what="freq, count only")
    assert gpu_ctx.replays() == r0


def test_ops_are_per_column_also_in_a_replayed_call(gpu_ctx):
    """`ops` is a field of the column: one call holds columns with all four ops, with count alone and with single ops; the
    fields whose bit is missing come back as 0.  With a Freq column among them the interval is issued again: the columns
    with a value op are decoded, the count-only column keeps its own route."""
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows = 10_000
    f = sparse(S.T_I64, rows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    b = gen.prim(S.T_F64, rows, uniq=100, null_density=0.2, runs=6, seed=2)
    bp, bm = gen.oracle_write(b, max_page_size=4100, force_codec=S.RLE)
    fref, bref = R.Ref(f, fp, fm), R.Ref(b, bp, bm)
    fcp, bcp = upload(gpu_ctx, f, fp, fm), upload(gpu_ctx, b, bp, bm)
    mask = np.random.default_rng(21).random(rows) < 0.3
    each = [("count", "min", "max", "sum"), ("count",), ("sum",), ("min",), ("count", "max"), ()]
    for cp, ref, replays in ((bcp, bref, 0), (fcp, fref, 1)):
        batch = sb.AggregateBatch(gpu_ctx, [cp] * len(each) + [bcp], bitmap(gpu_ctx, mask))
        for i, ops in enumerate(each):
            batch._arr[i].ops = sum(R.OPS[o] for o in ops)
        r0 = gpu_ctx.replays()
        res = batch.enqueue()
        gpu_ctx.synchronize()
        assert gpu_ctx.replays() == r0 + replays
        for i, ops in enumerate(each):
            R.check(res[i], ref.want(mask, ops), "ops %r" % (ops,))
        R.check(res[-1], bref.want(mask), "the column behind them")


# ---- 7: filter -> aggregate (and read_selected) in one interval
@pytest.mark.parametrize("freq", [False, True])
def test_filter_then_aggregate_in_one_interval(gpu_ctx, freq):
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows = 10_007
    x = sparse(S.T_I32, rows, 0.05, 2, null_density=0.1) if freq else gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    y = gen.prim(S.T_F64, rows, uniq=100, runs=6, seed=2)
    xp, xm = gen.oracle_write(x, max_page_size=2050, force_codec=S.FREQ if freq else S.RLE)
    yp, ym = gen.oracle_write(y, max_page_size=777, force_codec=S.DICT)
    xlit = 7 if freq else 60
    xr, yr = R.Ref(x, xp, xm), R.Ref(y, yp, ym)
    mask = ((xr.vals != xlit) & xr.valid) & ((yr.vals >= 30.0) & yr.valid)
    assert 0 < mask.sum() < rows
    a = gen.prim(S.T_I64, rows, uniq=100, null_density=0.2, runs=6, seed=3)
    b = gen.prim(S.T_U16, rows, uniq=100, null_density=0.1, seed=4)
    ap, am = gen.oracle_write(a, max_page_size=4100, force_codec=S.RLE)
    bp, bm = gen.oracle_write(b, max_page_size=2050, force_codec=S.DICT)
    ar, br = R.Ref(a, ap, am), R.Ref(b, bp, bm)
    acp, bcp = upload(gpu_ctx, a, ap, am), upload(gpu_ctx, b, bp, bm)
    r0 = gpu_ctx.replays()
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("ne", xlit)])
    sb.filter_columns(gpu_ctx, [upload(gpu_ctx, y, yp, ym)], [sb.Predicate("ge", 30.0)], combine="and", out=sel)
    res = sb.aggregate_columns(gpu_ctx, [acp, bcp], sel[0])
    arrs = sb.read_selected(gpu_ctx, [acp, bcp], sel[0])
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + (1 if freq else 0)
    assert np.array_equal(sel[0].numpy(), mask)
    R.check(res[0], ar.want(mask), "a behind the filter")
    R.check(res[1], br.want(mask), "b behind the filter")
    for ref, arr in ((ar, arrs[0]), (br, arrs[1])):   # the selected read next to it is the oracle's rows too
        got_vals, got_valid = arr.numpy()
        assert arr.selected == int(mask.sum())
        assert np.array_equal(got_valid, ref.valid[mask])
        assert np.array_equal(got_vals[got_valid], ref.vals[mask][ref.valid[mask]])


# ---- 8: count alone works on every type
def _every_type_columns():
    return [gen.boolean(3000, null_density=0.2), gen.binary(3000, uniq=10, null_density=0.3), gen.binary(3000, uniq=10, large=True),
            gen.prim(S.T_I128, 3000, uniq=10, null_density=0.1), gen.prim(S.T_I256, 3000, uniq=10),
            dict(ptype=S.T_NULL, nullable=True, rows=3000, values=None, validity=None, offsets=None)]


def _raw_array(ctx, cps, bitmaps, ops):
    from strawboat_amd.aggregate import AggregateBatch
    from strawboat_amd import _native as N
    batch = AggregateBatch(ctx, cps, bitmaps, ops=("count",))
    for i in range(len(cps)):
        batch._arr[i].ops = ops
        for f in ("rows", "selected", "count", "nans", "sum_lo", "sum_hi"):
            setattr(batch._arr[i], f, 0x5A5A5A5A5A5A5A5A)
        C.memset(C.addressof(batch._arr[i]) + N.ColumnAggregateC.min.offset, SENTINEL, 16)
    return batch


def _sentinels_kept(arr):
    for c in arr:
        assert all(getattr(c, f) == 0x5A5A5A5A5A5A5A5A for f in ("rows", "selected", "count", "nans", "sum_lo", "sum_hi"))
        assert bytes(c.min) == bytes(c.max) == bytes([SENTINEL]) * 8


def test_count_only_on_every_type(gpu_ctx):
    from strawboat_amd import _native as N
    rng = np.random.default_rng(8)
    for col in _every_type_columns():
        pages, metas = gen.oracle_write(col, max_page_size=777)
        ref = R.Ref(col, pages, metas)
        cp = upload(gpu_ctx, col, pages, metas)
        masks = [rng.random(3000) < 0.35, two_masks(3000, 3)[1], None]
        for ops in (("count",), ()):
            res = run(gpu_ctx, [cp] * 3, masks, [ref] * 3, ops=ops, what="count only, type %d" % col["ptype"])
            assert all(r.min is None and r.max is None and r.sum is None for r in res)
        if col["ptype"] == S.T_NULL:
            assert [r.count for r in res] == [0, 0, 0] and res[2].selected == 3000
        # the same column with MIN: refused at the call, nothing enqueued, and the synchronize raises nothing
        batch = _raw_array(gpu_ctx, [cp], [bitmap(gpu_ctx, masks[0])], N.SB_AGG_COUNT | N.SB_AGG_MIN)
        assert gpu_ctx._lib.sb_aggregate_columns(gpu_ctx._h, batch._arr, 1, N.SB_MEM_DEVICE) == N.SB_ERR_NYI, col["ptype"]
        gpu_ctx.synchronize()
        _sentinels_kept(batch._arr)
    # ... and on the ten numeric types, Dict and RLE pages included: no page body is looked at
    for ptype in (S.T_I16, S.T_F64):
        for codec in (S.RLE, S.DICT):
            col = gen.prim(ptype, 10_000, uniq=50, null_density=0.2, runs=5)
            check(gpu_ctx, col, codec=codec, ops=("count",), max_page_size=2050, force_codec=codec)


# ---- 9: refusals at the call
def test_refusals_at_the_call(gpu_ctx):
    from strawboat_amd import _native as N
    col = gen.prim(S.T_I64, 5000, uniq=10, null_density=0.2)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.NONE)
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(9).random(5000) < 0.5
    bm = bitmap(gpu_ctx, mask)
    boolean = gen.boolean(5000)
    bpages, bmetas = gen.oracle_write(boolean)
    bcp = upload(gpu_ctx, boolean, bpages, bmetas)

    def fresh(cps=None):
        return _raw_array(gpu_ctx, cps or [cp, cp], [bm, bm], 15)

    def refused(batch, code, what, mem=N.SB_MEM_DEVICE):
        assert gpu_ctx._lib.sb_aggregate_columns(gpu_ctx._h, batch._arr, 2, mem) == code, what
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        _sentinels_kept(batch._arr)

    batch = fresh()
    batch._arr[1].ops = 16 | 1
    refused(batch, N.SB_ERR_INVALID, "unknown ops bits")
    batch = fresh()
    batch._arr[1].reserved = 1
    refused(batch, N.SB_ERR_INVALID, "reserved != 0")
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
    for ops in (N.SB_AGG_MIN, N.SB_AGG_MAX, N.SB_AGG_SUM, 15):
        batch = fresh([cp, bcp])
        batch._arr[1].ops = ops
        refused(batch, N.SB_ERR_NYI, "min / max / sum on Boolean")
    batch = fresh()
    refused(batch, N.SB_ERR_NYI, "SB_MEM_HOST", mem=N.SB_MEM_HOST)
    # a page outside [0, pages_len): the span check of the read calls' host tables
    batch = fresh()
    batch._arr[1].pages_len -= 1
    assert gpu_ctx._lib.sb_aggregate_columns(gpu_ctx._h, batch._arr, 2, N.SB_MEM_DEVICE) == N.SB_ERR_IO
    _sentinels_kept(batch._arr)
    with pytest.raises(N.NativeError) as e:   # (like its siblings', this refusal is the interval's result as well)
        gpu_ctx.synchronize()
    assert e.value.code == N.SB_ERR_IO
    # the same batch, as it was built, then succeeds
    batch = fresh()
    res = batch.enqueue()
    gpu_ctx.synchronize()
    for r in res:
        R.check(r, ref.want(mask), "after the refusals")


# ---- 10: pages anywhere
def test_pages_at_any_byte_offset_and_in_any_order(gpu_ctx):
    from strawboat_amd import read
    rng = np.random.default_rng(10)
    for codec in (S.NONE, S.RLE, S.DICT, S.LZ4):
        col = gen.prim(S.T_I64, 10_000, uniq=100, null_density=0.2, runs=6, seed=codec)
        pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
        ref = R.Ref(col, pages, metas)
        masks = [rng.random(10_000) < 0.35, None]
        cps = []
        for shift in (1, 7, 15):
            buf, start = buffer_cases.place(pages, shift, 0x5A)
            dev = to_dev(gpu_ctx, buf)
            cps.append(read.ColumnPages(col["ptype"], True, dev[start:start + pages.size], metas))
        buf, offs = buffer_cases.scatter(pages, metas, order="descending")
        cps.append(read.ColumnPages(col["ptype"], True, to_dev(gpu_ctx, buf), metas, page_offsets=offs))
        for m in masks:
            run(gpu_ctx, cps, [m] * 4, [ref] * 4, what="placed pages, codec %d" % codec)


# ---- 11: empty and tiny
def test_empty_and_tiny(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    dev = gpu_ctx.torch_device
    empty = read.ColumnPages(S.T_I64, True, torch.zeros(0, dtype=torch.uint8, device=dev), np.zeros((0, 2), np.uint64))
    for sel in (None, torch.zeros(0, dtype=torch.uint8, device=dev)):
        res = sb.aggregate_columns(gpu_ctx, [empty], sel)
        gpu_ctx.synchronize()
        r = res[0]
        assert (r.rows, r.selected, r.count, r.nans, r.min, r.max, r.sum) == (0, 0, 0, 0, None, None, 0)
    # ... and as one column of a call that has pages
    col = gen.prim(S.T_I32, 3000, uniq=5, null_density=0.3, seed=4)
    pages, metas = gen.oracle_write(col, max_page_size=777, force_codec=S.NONE)
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(1).random(3000) < 0.5
    res = sb.aggregate_columns(gpu_ctx, [empty, cp, empty], [None, bitmap(gpu_ctx, mask), None])
    gpu_ctx.synchronize()
    assert (res[0].rows, res[0].count, res[0].sum, res[2].selected) == (0, 0, 0, 0)
    R.check(res[1], ref.want(mask), "next to empty columns")
    # one-row columns: the row selected / unselected / unselected by absence, null / not null
    for nd in (None, 0.5):
        for seed in (1, 2, 3, 4):
            col = gen.prim(S.T_I32, 1, uniq=5, null_density=nd, seed=seed)
            check(gpu_ctx, col, masks=[np.array([True]), np.array([False]), None])
            check(gpu_ctx, col, masks=[np.array([True]), np.array([False]), None], force_codec=S.NONE)
    col = gen.prim(S.T_I32, 2051, uniq=5, seed=4)   # a one-row page behind two others
    for codec in (S.RLE, S.NONE, S.DICT):
        check(gpu_ctx, col, codec=codec, max_page_size=1025, force_codec=codec)
        last = np.zeros(2051, bool)
        last[2050] = True
        check(gpu_ctx, col, masks=[last], max_page_size=1025, force_codec=codec)


# ---- 12: corrupt pages raise what the decoder raises
def aggregate_code(ctx, cp, rows, sel=True):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    try:
        sb.aggregate_columns(ctx, [cp], to_dev(ctx, bitmap_of(np.ones(rows, bool))) if sel else None)
        ctx.synchronize()
    except NativeError as e:
        try:
            ctx.synchronize()
        except NativeError:
            pass
        return e.code
    return 0


def test_corrupt_pages_raise_what_the_decoder_raises(gpu_ctx):
    # a truncated last page
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
        assert aggregate_code(gpu_ctx, cp, 9000) == want, codec
        assert aggregate_code(gpu_ctx, cp, 9000, sel=False) == want, codec
    # a Dict page with an index >= D: plain u32 indices behind hdr9 Dict | hdr9 None
    col = gen.prim(S.T_I64, 40_000, uniq=50, seed=50)
    pages, metas = gen.oracle_write(col, max_page_size=40_000, force_codec=S.DICT, force_index_codec=S.NONE)
    bad = pages.copy()
    pos = 9 + 9 + 25_000 * 4
    bad[pos:pos + 4] = np.frombuffer(np.uint32(1 << 30).tobytes(), np.uint8)
    cp = upload(gpu_ctx, col, bad, metas)
    assert read_code(gpu_ctx, cp) == -1 and oracle_code(col, bad, metas) != 0
    assert aggregate_code(gpu_ctx, cp, 40_000) == -1
    # hand-built RLE pages: a run that overshoots the page, runs that end before the page is full
    for (ptype, dtype, w, runs, rows), code in ((RLE_OVERSHOOT, -1), (RLE_SHORT, -3)):
        page = _rle_page(runs, w, dtype).copy()
        cp = upload(gpu_ctx, dict(ptype=ptype, nullable=False), page, np.array([[page.size, rows]], np.uint64))
        assert read_code(gpu_ctx, cp) == code
        assert aggregate_code(gpu_ctx, cp, rows) == code
    # rows and selected are delivered even when the interval failed
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    sel = np.random.default_rng(12).random(rows) < 0.5
    res = sb.aggregate_columns(gpu_ctx, [cp], bitmap(gpu_ctx, sel))
    with pytest.raises(NativeError):
        gpu_ctx.synchronize()
    assert res[0].rows == rows and res[0].selected == int(sel.sum())
    # the context still works
    col = gen.prim(S.T_I64, 9000, uniq=60)
    check(gpu_ctx, col, max_page_size=3000, force_codec=S.DICT)


# ---- 13: a seeded sweep
SWEEP_SEED = 20241019
SWEEP_CASES = 60


def test_random_sweep(gpu_ctx):
    rng = np.random.default_rng(SWEEP_SEED)
    codecs = [-1, S.NONE, S.RLE, S.DICT, S.LZ4, S.ZSTD, S.SNAPPY, S.ONEVALUE]
    for case in range(SWEEP_CASES):
        ptype = TYPES[int(rng.integers(0, len(TYPES)))]
        codec = codecs[int(rng.integers(0, len(codecs)))]
        rows = int(rng.integers(1, 10_001))
        page = int(rng.choice(PAGES))
        nd = [None, 0.05, 0.5][int(rng.integers(0, 3))]
        uniq = 1 if codec == S.ONEVALUE else int(rng.choice([2, 100, 100_000]))
        runs = [None, 3, 50][int(rng.integers(0, 3))]
        p = float(rng.choice([0.0, 0.001, 0.01, 0.1, 0.5, 0.999, 1.0]))
        kind = int(rng.integers(0, 3))
        col = gen.prim(ptype, rows, uniq=uniq, null_density=nd, runs=runs, seed=int(rng.integers(0, 1 << 30)))
        if kind == 0:
            mask = rng.random(rows) < p
        elif kind == 1:   # clustered: the bits of one stretch of the column
            mask = np.zeros(rows, bool)
            at = int(rng.integers(0, rows))
            mask[at:at + max(1, int(rows * p))] = True
        else:
            mask = (np.arange(rows) % int(rng.integers(2, 70))) == 0
        opt = dict(max_page_size=page)
        if codec >= 0:
            opt["force_codec"] = codec
        try:
            pages, metas = gen.oracle_write(col, **opt)
            ref = R.Ref(col, pages, metas)
            cp = upload(gpu_ctx, col, pages, metas)
            run(gpu_ctx, [cp, cp], [mask, None], [ref, ref], what="sweep", tails=[bool(case & 1), False])
        except AssertionError as e:
            raise AssertionError("seed %d case %d: type %d codec %d rows %d page %d nulls %r uniq %d runs %r p %r kind %d: %s" % (
                SWEEP_SEED, case, ptype, codec, rows, page, nd, uniq, runs, p, kind, e))
