"""sb_aggregate_grouped on the GPU: pages written by the CPU oracle, count / min / max / sum of the selected rows per group
computed on the device, compared with the ORACLE's decode of the pages reduced per group by numpy and Python
(tests/aggregate_grouped_ref.py on tests/aggregate_ref.py).  Nothing here is compared with what the device's own decoder,
sb_read_selected or sb_aggregate_columns give.

Every case checks rows / selected / out_of_range of the column and selected / count / nans / min / max / sum of every group.
Integers, the counts and the bytes of min / max are compared exactly; a group's float sum over finite data must lie within
count_g * 2^-52 * sum_g|x| of math.fsum (aggregate_ref.float_sum_bound: derived, not measured).  Unless a test says otherwise
every column runs under a random ~0.35 selection, a sparse one that leaves whole tiles and pages out, and no selection at
all, as three columns of one call."""
import ctypes as C

import numpy as np
import pytest

from oracle import sbo as S
from tests import aggregate_grouped_ref as G
from tests import aggregate_ref as R
from tests import buffer_cases, gen
from tests.test_gpu_aggregate import _column, _every_type_columns, _specials, bitmap
from tests.test_gpu_decode import LONG_RLE_ROWS, RLE_OVERSHOOT, RLE_SHORT, _rle_page
from tests.test_gpu_read_selected import PAGES, TYPES, oracle_code, read_code, to_dev, two_masks, upload
from tests.test_read_selected_host import bitmap_of

pytestmark = pytest.mark.gpu

NP = gen.NP_OF
SENTINEL = 0x5A
ID_DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def ids_dev(ctx, ids, width=4):
    return to_dev(ctx, np.asarray(ids).astype(ID_DTYPE[width]))


def run(ctx, cps, masks, refs, ids, n_groups, ops=R.ALL, what="", width=4):
    """the columns of ONE call, each under its own selection (None: none), its own ids (or one array for all) and its own
    n_groups (or one for all), checked against their references"""
    import strawboat_amd as sb
    n = len(cps)
    ids_list = list(ids) if isinstance(ids, (list, tuple)) else [ids] * n
    ng_list = list(n_groups) if isinstance(n_groups, (list, tuple)) else [n_groups] * n
    shared = {}
    devs = [shared.setdefault(id(a), ids_dev(ctx, a, width)) for a in ids_list]
    res = sb.aggregate_grouped(ctx, cps, devs if isinstance(ids, (list, tuple)) else devs[0], ng_list, [bitmap(ctx, m) for m in masks], ops=ops)
    ctx.synchronize()
    for i, (r, ref, m) in enumerate(zip(res, refs, masks)):
        G.check(r, G.want(ref, ids_list[i], ng_list[i], m, ops), "%s column %d" % (what, i))
    return res


def some_ids(rows, n_groups, seed=0):
    return np.random.default_rng(1000 + seed).integers(0, n_groups, rows)


def check_pages(ctx, col, pages, metas, ids=None, n_groups=5, masks=None, ops=R.ALL, what="", width=4):
    ref = R.Ref(col, pages, metas)
    if masks is None:
        masks = two_masks(ref.rows, 11) + [None]
    if ids is None:
        ids = some_ids(ref.rows, n_groups)
    cp = upload(ctx, col, pages, metas)
    return run(ctx, [cp] * len(masks), masks, [ref] * len(masks), ids, n_groups, ops, what, width)


def check(ctx, col, codec=None, ids=None, n_groups=5, masks=None, ops=R.ALL, width=4, **opt):
    pages, metas = gen.oracle_write(col, **opt)
    if codec is not None:
        seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
        assert seen == {codec}, (seen, codec)
    return check_pages(ctx, col, pages, metas, ids, n_groups, masks, ops, "codec %r %r" % (codec, opt), width)


# ---- 1: codecs x types
@pytest.mark.parametrize("ptype", TYPES)
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT, S.ONEVALUE])
def test_prim_codecs(gpu_ctx, ptype, codec):
    uniq = 1 if codec == S.ONEVALUE else 100
    for nd, page in ((0.2, PAGES[0]), (None, PAGES[1]), (0.2, PAGES[2]), (None, PAGES[3])):
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


@pytest.mark.parametrize("codec", [S.RLE, S.DICT])
def test_one_long_page(gpu_ctx, codec):
    """several workgroups share an RLE page (the parts route); a long Dict page has many tiles"""
    rng = np.random.default_rng(codec)
    ids = np.repeat(rng.integers(0, 4, LONG_RLE_ROWS // 1000 + 1), 1000)[:LONG_RLE_ROWS]
    ids[::4099] = 7   # (out of range)
    for ptype, seed in ((S.T_F64, 4), (S.T_I64, 5)):
        col = gen.prim(ptype, LONG_RLE_ROWS, uniq=256, null_density=0.1, runs=32, seed=seed)
        pages, metas = gen.oracle_write(col, force_codec=codec)
        assert metas.shape[0] == 1
        check_pages(gpu_ctx, col, pages, metas, ids, 4, [rng.random(LONG_RLE_ROWS) < 0.002, None], what="long page")


@pytest.mark.parametrize("ptype", [S.T_I32, S.T_I64])
def test_freq_pages(gpu_ctx, ptype):
    """the interval is issued again, the call's columns decoded and reduced per group"""
    from tests.test_gpu_freq import sparse
    rows = 10_000
    f = sparse(ptype, rows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    assert S.FREQ in set(int(x) for x in S.stat_column(f["ptype"], f["nullable"], fp, fm)[0].tolist())
    b = gen.prim(S.T_F64, rows, uniq=100, null_density=0.2, runs=6, seed=2)
    bp, bm = gen.oracle_write(b, max_page_size=4100, force_codec=S.RLE)
    fref, bref = R.Ref(f, fp, fm), R.Ref(b, bp, bm)
    fcp, bcp = upload(gpu_ctx, f, fp, fm), upload(gpu_ctx, b, bp, bm)
    mask = np.random.default_rng(ptype).random(rows) < 0.3
    ids = some_ids(rows, 7)   # (two ids out of range)
    r0 = gpu_ctx.replays()
    run(gpu_ctx, [fcp, bcp, fcp], [mask, mask, None], [fref, bref, fref], ids, 5, what="freq")
    assert gpu_ctx.replays() == r0 + 1
    # a sparse selection, and a Freq column without a selected row: the replay all the same
    for m in (two_masks(rows, 5)[1], np.zeros(rows, bool)):
        r0 = gpu_ctx.replays()
        run(gpu_ctx, [fcp, bcp], [m, mask], [fref, bref], ids, [5, 256], what="freq, %d selected" % int(m.sum()))
        assert gpu_ctx.replays() == r0 + 1
    # count alone looks at no page body: no replay
    r0 = gpu_ctx.replays()
    run(gpu_ctx, [fcp], [mask], [fref], ids, 5, ops=("count",), what="freq, count only")
    assert gpu_ctx.replays() == r0


def test_ops_are_per_column_also_in_a_replayed_call(gpu_ctx):
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
    ids = some_ids(rows, 4)
    each = [("count", "min", "max", "sum"), ("count",), ("sum",), ("min",), ("count", "max"), ()]
    for cp, ref, replays in ((bcp, bref, 0), (fcp, fref, 1)):
        batch = sb.GroupedAggregateBatch(gpu_ctx, [cp] * len(each) + [bcp], ids_dev(gpu_ctx, ids), 3, bitmap(gpu_ctx, mask))
        for i, ops in enumerate(each):
            batch._arr[i].ops = sum(R.OPS[o] for o in ops)
            batch.results[i].ops = batch._arr[i].ops
        r0 = gpu_ctx.replays()
        res = batch.enqueue()
        gpu_ctx.synchronize()
        assert gpu_ctx.replays() == r0 + replays
        for i, ops in enumerate(each):
            G.check(res[i], G.want(ref, ids, 3, mask, ops), "ops %r" % (ops,))
        G.check(res[-1], G.want(bref, ids, 3, mask), "the column behind them")


# ---- 2: group shapes
GROUP_COUNTS = (1, 2, 3, 64, 65, 255, 256)


def _shape_columns():
    rows = 10_000
    out = []
    for ptype, codec, page in ((S.T_F64, S.NONE, 4100), (S.T_I64, S.RLE, 2050), (S.T_F32, S.DICT, 2048), (S.T_I16, S.NONE, 777)):
        col = gen.prim(ptype, rows, uniq=100, null_density=0.2, runs=4, seed=page)
        pages, metas = gen.oracle_write(col, max_page_size=page, force_codec=codec)
        out.append((col, pages, metas, R.Ref(col, pages, metas)))
    return out


@pytest.fixture(scope="module")
def shape_columns():
    return _shape_columns()


@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
def test_group_counts_and_id_patterns(gpu_ctx, shape_columns, n_groups):
    rows = 10_000
    rng = np.random.default_rng(n_groups)
    r = np.arange(rows)
    patterns = {"constant": np.full(rows, n_groups - 1), "r % n": r % n_groups, "random": rng.integers(0, n_groups, rows)}
    for run_len in (63, 64, 65, 256, 4096):
        patterns["runs of %d" % run_len] = (r // run_len) % n_groups
    masks = two_masks(rows, 11) + [None]
    for k, (name, ids) in enumerate(patterns.items()):
        col, pages, metas, ref = shape_columns[k % len(shape_columns)]
        cp = upload(gpu_ctx, col, pages, metas)
        run(gpu_ctx, [cp] * 3, masks, [ref] * 3, ids, n_groups, what="%d groups, ids %s" % (n_groups, name),
            width=1 if n_groups < 256 and k % 2 else 4)


@pytest.mark.parametrize("width", [1, 2, 4])
def test_id_widths_and_ids_out_of_range(gpu_ctx, shape_columns, width):
    """ids >= n_groups, the all-ones id included, among selected and among unselected rows: the selected ones are counted
    in out_of_range, the unselected ones are never interpreted"""
    rows = 10_000
    rng = np.random.default_rng(width)
    ones = int(np.iinfo(ID_DTYPE[width]).max)
    masks = two_masks(rows, 11) + [None]
    for n_groups in (3, 200):
        ids = rng.integers(0, n_groups, rows)
        ids[rng.random(rows) < 0.05] = ones
        ids[rng.random(rows) < 0.05] = n_groups
        ids[rng.random(rows) < 0.02] = min(ones, n_groups + 50)
        wild = ids.copy()
        wild[~masks[0]] = ones   # (column 0: every unselected row carries the all-ones id)
        for col, pages, metas, ref in shape_columns[:3]:
            cp = upload(gpu_ctx, col, pages, metas)
            res = run(gpu_ctx, [cp] * 3, masks, [ref] * 3, [wild, ids, ids], n_groups, what="width %d" % width, width=width)
            assert 0 < res[0].out_of_range < res[2].out_of_range


def test_a_group_whose_only_row_is_the_last_of_a_page_and_of_a_tile(gpu_ctx):
    rows = 3 * 4096
    for ptype, codec in ((S.T_F64, S.NONE), (S.T_I64, S.RLE), (S.T_I32, S.DICT)):
        col = gen.prim(ptype, rows, uniq=50, runs=4, seed=3)
        pages, metas = gen.oracle_write(col, max_page_size=4096, force_codec=codec)
        assert [int(n) for n in metas[:, 1]] == [4096] * 3
        ids = np.zeros(rows, np.int64)
        ids[4095] = 1       # the last row of page 0 (and of its tile)
        ids[rows - 1] = 2   # the last row of the column
        res = check_pages(gpu_ctx, col, pages, metas, ids, 3, masks=[None, np.arange(rows) % 4096 == 4095], what="last rows")
        assert [g.selected for g in res[0].groups] == [rows - 2, 1, 1] and [g.selected for g in res[1].groups] == [1, 1, 1]


def test_group_ids_shared_and_per_column_with_their_own_n_groups(gpu_ctx, shape_columns):
    rows = 10_000
    rng = np.random.default_rng(5)
    a, b = rng.integers(0, 4, rows), rng.integers(0, 300, rows)
    cps = [upload(gpu_ctx, c, p, m) for c, p, m, _ in shape_columns]
    refs = [ref for _, _, _, ref in shape_columns]
    masks = [two_masks(rows, 3)[0], None, two_masks(rows, 3)[1], two_masks(rows, 4)[0]]
    run(gpu_ctx, cps, masks, refs, a, 4, what="one ids array for all")
    run(gpu_ctx, cps, masks, refs, [a, b, b, a], [4, 256, 17, 2], what="ids and n_groups per column")


# ---- 3: extremes
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_extremes(gpu_ctx, codec):
    rng = np.random.default_rng(codec + 7)
    rows = 10_000
    opt = dict(max_page_size=4100, force_codec=codec)
    runs = np.repeat(np.arange(rows // 5 + 1), 5)[:rows]
    ids = rng.integers(0, 3, rows)[runs]   # (runs of five, so that RLE and Dict pages can hold the values below)
    # INT64 min / max repeated inside one group: the 64-bit sum wraps, the 128-bit sum does not
    v = np.where(ids == 0, -2 ** 63, np.where(ids == 1, 2 ** 63 - 1, rng.integers(-5, 5, rows)[runs])).astype(np.int64)
    res = check(gpu_ctx, _column(S.T_I64, v, rng.random(rows) >= 0.2), codec=codec, ids=ids, n_groups=3, **opt)
    g = res[2].groups
    assert g[0].sum == -2 ** 63 * g[0].count < -2 ** 64 and g[0].min == g[0].max == -2 ** 63
    assert g[1].sum == (2 ** 63 - 1) * g[1].count > 2 ** 64 and g[1].max == 2 ** 63 - 1
    # UINT64 max repeated inside one group
    v = np.where(ids == 2, np.uint64(2 ** 64 - 1), rng.integers(0, 50, rows)[runs].astype(np.uint64))
    res = check(gpu_ctx, _column(S.T_U64, v, rng.random(rows) >= 0.1), codec=codec, ids=ids, n_groups=3, **opt)
    g = res[2].groups[2]
    assert g.sum == (2 ** 64 - 1) * g.count and g.count > 2000 and g.min == g.max == 2 ** 64 - 1
    # I8 / I16 with negative minima: sign extension in min / max / sum
    for ptype, lo, hi in ((S.T_I8, -128, 127), (S.T_I16, -32768, 32767)):
        v = rng.integers(lo, lo // 2, rows)[runs]
        v[::97] = lo
        v[5::101] = hi
        res = check(gpu_ctx, _column(ptype, v, rng.random(rows) >= 0.2), codec=codec, ids=ids, n_groups=3, **opt)
        assert all(g.sum < 0 for g in res[2].groups) and min(g.min for g in res[2].groups) == lo


@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_selected_rows_of_a_group_that_are_all_null(gpu_ctx, codec):
    rng = np.random.default_rng(3)
    rows = 10_000
    ids = rng.integers(0, 4, rows)
    valid = rng.random(rows) >= 0.3
    valid[ids == 2] = False   # every row of group 2 is null
    col = _column(S.T_I32, np.repeat(rng.integers(-1000, 1000, 2000), 5), valid)
    res = check(gpu_ctx, col, codec=codec, ids=ids, n_groups=4, max_page_size=4100, force_codec=codec)
    for r in res:
        g = r.groups[2]
        assert g.selected > 0 and g.count == 0 and g.min is None and g.max is None and g.sum == 0
        assert g.min_bytes == g.max_bytes == bytes(8)
    only_nulls = ~valid & (rng.random(rows) < 0.5)
    res = check(gpu_ctx, col, codec=codec, ids=ids, n_groups=4, masks=[only_nulls], max_page_size=4100, force_codec=codec)
    assert all(g.selected > 0 and g.count == 0 and g.sum == 0 for g in res[0].groups)


@pytest.mark.parametrize("ptype", [S.T_F32, S.T_F64])
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_float_specials(gpu_ctx, ptype, codec):
    """group 0: NaNs of both signs among finite rows; 1: +inf; 2: -inf; 3: the zeros alone; 4: NaNs alone; 5: finite rows"""
    dtype = NP[ptype]
    rng = np.random.default_rng(ptype)
    rows = 10_000
    v = np.repeat(rng.normal(0, 50, rows // 4 + 1), 4)[:rows].astype(dtype)
    nan, nan_neg, inf, ninf, zero, nzero, tiny, ntiny = _specials(dtype)
    ids = rng.integers(0, 3, rows) * 0 + 5
    ids[rng.random(rows) < 0.5] = 0
    ids[rng.random(rows) < 0.2] = 1
    ids[rng.random(rows) < 0.2] = 2
    special = np.zeros(rows, bool)
    for at, value, group in (([10, 4097, 9000], nan, 0), ([11, 8300], nan_neg, 0), ([500, 4095], inf, 1), ([4096], ninf, 2),
                             ([20, 21, 22], zero, 3), ([23, 24], nzero, 3), ([30, 31, 5000], nan, 4), ([32], nan_neg, 4),
                             ([40], tiny, 5), ([41], ntiny, 5)):
        v[at] = value
        ids[at] = group
        special[at] = True
    valid = rng.random(rows) >= 0.1
    valid[special] = True
    col = _column(ptype, v, valid)
    pages, metas = gen.oracle_write(col, max_page_size=4100, force_codec=codec)
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    masks = [special | (rng.random(rows) < 0.3), None]
    res = run(gpu_ctx, [cp] * 2, masks, [ref] * 2, ids, 6, what="float specials")
    w = np.dtype(dtype).itemsize
    for r in res:
        g = r.groups
        assert g[0].nans == 5 and g[0].sum != g[0].sum and g[0].min is not None
        assert g[1].sum == np.inf and g[1].max == np.inf and g[2].sum == -np.inf and g[2].min == -np.inf
        assert g[3].count == 5 and g[3].sum == 0.0
        if np.signbit(ref.vals[23]) and not np.signbit(ref.vals[20]):   # (the pages kept the zeros' signs)
            assert g[3].min_bytes[:w] == dtype(-0.0).tobytes() and g[3].max_bytes[:w] == dtype(0.0).tobytes()
        assert g[4].count == 4 and g[4].nans == 4 and g[4].min is None and g[4].max is None and g[4].sum != g[4].sum
        assert g[4].min_bytes == g[4].max_bytes == bytes(8)
        assert g[5].nans == 0 and np.isfinite(g[5].sum)


# ---- 4: the order of the float additions: the same bits every time, a replayed interval included
@pytest.mark.parametrize("n_groups", G.ORDER_TEST_GROUPS)
@pytest.mark.parametrize("ptype", [S.T_F32, S.T_F64])
@pytest.mark.parametrize("codec", [S.NONE, S.DICT, S.RLE])
def test_float_sums_that_are_exact_in_no_order(gpu_ctx, ptype, codec, n_groups):
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows = 10_000
    v, ids = G.inexact_values(rows, n_groups, seed=17)   # (pinned on the CPU: tests/test_aggregate_grouped_host.py)
    rng = np.random.default_rng(codec * 10 + ptype)
    col = _column(ptype, v.astype(NP[ptype]), rng.random(rows) >= 0.1)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
    assert set(int(c) for c in S.stat_column(ptype, True, pages, metas)[0].tolist()) == {codec}
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    masks = two_masks(rows, 11) + [None]
    res = run(gpu_ctx, [cp] * 3, masks, [ref] * 3, ids, n_groups, what="inexact float sums")
    first = [[(g._c.sum_lo, g.min_bytes, g.max_bytes) for g in r.groups] for r in res]
    # the same call three times in fresh intervals
    dev = ids_dev(gpu_ctx, ids)
    bitmaps = [bitmap(gpu_ctx, m) for m in masks]
    batch = sb.GroupedAggregateBatch(gpu_ctx, [cp] * 3, dev, n_groups, bitmaps)
    for _ in range(3):
        again = batch.enqueue()
        gpu_ctx.synchronize()
        assert [[(g._c.sum_lo, g.min_bytes, g.max_bytes) for g in r.groups] for r in again] == first
    # ... and the unchanged call in intervals that are issued again on another call's account: a filter on a Freq column, a
    # grouped aggregate of a Freq column, and both.  The bits are those of the fresh intervals.
    f = sparse(S.T_I64, rows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    fcp = upload(gpu_ctx, f, fp, fm)
    fref = R.Ref(f, fp, fm)
    for others in ("filter", "grouped", "both"):
        r0 = gpu_ctx.replays()
        if others != "grouped":
            sb.filter_columns(gpu_ctx, [fcp], [sb.Predicate("ne", 7)])
        if others != "filter":
            fres = sb.aggregate_grouped(gpu_ctx, [fcp], dev, n_groups, bitmaps[0])
        again = batch.enqueue()
        gpu_ctx.synchronize()
        assert gpu_ctx.replays() == r0 + 1, others
        assert [[(g._c.sum_lo, g.min_bytes, g.max_bytes) for g in r.groups] for r in again] == first, others
        if others != "filter":
            G.check(fres[0], G.want(fref, ids, n_groups, masks[0]), "the Freq column next to it")
    # ... and as columns of one call with a Freq column: the Freq column is decoded, the others stay where they were
    r0 = gpu_ctx.replays()
    both = sb.GroupedAggregateBatch(gpu_ctx, [cp] * 3 + [fcp], dev, n_groups, bitmaps + [None]).enqueue()
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    assert [[(g._c.sum_lo, g.min_bytes, g.max_bytes) for g in r.groups] for r in both[:3]] == first
    G.check(both[3], G.want(fref, ids, n_groups, None), "the Freq column of the call")


@pytest.mark.parametrize("ptype", [S.T_F32, S.T_F64])
def test_a_float_freq_column_gives_the_same_bits_in_every_interval(gpu_ctx, ptype):
    """A column with a Freq page takes the decoded route whenever it is issued: alone, twice, and next to other calls."""
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows, n_groups = 10_000, 7
    f = sparse(ptype, rows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    if S.FREQ not in set(int(x) for x in S.stat_column(f["ptype"], f["nullable"], fp, fm)[0].tolist()):
        pytest.fail("the oracle wrote no Freq page for type %d" % ptype)
    fref = R.Ref(f, fp, fm)
    fcp = upload(gpu_ctx, f, fp, fm)
    b = gen.prim(S.T_I64, rows, uniq=100, null_density=0.2, runs=6, seed=2)
    bp, bm = gen.oracle_write(b, max_page_size=4100, force_codec=S.RLE)
    bcp = upload(gpu_ctx, b, bp, bm)
    ids = some_ids(rows, n_groups)
    dev = ids_dev(gpu_ctx, ids)
    mask = np.random.default_rng(ptype).random(rows) < 0.4
    bmp = bitmap(gpu_ctx, mask)
    batch = sb.GroupedAggregateBatch(gpu_ctx, [fcp, fcp], dev, n_groups, [bmp, None])
    seen = []
    for others in (0, 0, 1, 2):
        r0 = gpu_ctx.replays()
        if others == 1:
            sb.aggregate_grouped(gpu_ctx, [bcp], dev, n_groups, bmp)
        if others == 2:
            sb.filter_columns(gpu_ctx, [fcp], [sb.Predicate("is_not_null")])
        res = batch.enqueue()
        gpu_ctx.synchronize()
        assert gpu_ctx.replays() == r0 + 1
        G.check(res[0], G.want(fref, ids, n_groups, mask), "Freq float column, selection")
        G.check(res[1], G.want(fref, ids, n_groups, None), "Freq float column, every row")
        seen.append([[g._c.sum_lo for g in r.groups] for r in res])
    assert seen[1:] == seen[:1] * 3


# ---- 5: count alone works on every type
def _raw_array(ctx, cps, bitmaps, dev_ids, n_groups, ops):
    from strawboat_amd.aggregate_grouped import GroupedAggregateBatch
    batch = GroupedAggregateBatch(ctx, cps, dev_ids, n_groups, bitmaps, ops=("count",))
    for i in range(len(cps)):
        batch._arr[i].ops = ops
        for f in ("rows", "selected", "out_of_range"):
            setattr(batch._arr[i], f, 0x5A5A5A5A5A5A5A5A)
        C.memset(batch.results[i]._groups, SENTINEL, 64 * n_groups)
    return batch


def _sentinels_kept(batch):
    for c, r in zip(batch._arr, batch.results):
        assert all(getattr(c, f) == 0x5A5A5A5A5A5A5A5A for f in ("rows", "selected", "out_of_range"))
        assert bytes(r._groups) == bytes([SENTINEL]) * (64 * len(r.groups))


def test_count_only_on_every_type(gpu_ctx):
    from strawboat_amd import _native as N
    rng = np.random.default_rng(8)
    ids = rng.integers(0, 6, 3000)   # (id 5 is out of range)
    for col in _every_type_columns():
        pages, metas = gen.oracle_write(col, max_page_size=777)
        ref = R.Ref(col, pages, metas)
        cp = upload(gpu_ctx, col, pages, metas)
        masks = [rng.random(3000) < 0.35, two_masks(3000, 3)[1], None]
        for ops in (("count",), ()):
            res = run(gpu_ctx, [cp] * 3, masks, [ref] * 3, ids, 5, ops=ops, what="count only, type %d" % col["ptype"], width=1)
            assert all(g.min is None and g.max is None and g.sum is None for r in res for g in r.groups)
        if col["ptype"] == S.T_NULL:
            assert [g.count for g in res[2].groups] == [0] * 5 and sum(g.selected for g in res[2].groups) + res[2].out_of_range == 3000
        # the same column with MIN: refused at the call, nothing enqueued, and the synchronize raises nothing
        batch = _raw_array(gpu_ctx, [cp], [bitmap(gpu_ctx, masks[0])], ids_dev(gpu_ctx, ids, 1), 5, N.SB_AGG_COUNT | N.SB_AGG_MIN)
        assert gpu_ctx._lib.sb_aggregate_grouped(gpu_ctx._h, batch._arr, 1, N.SB_MEM_DEVICE) == N.SB_ERR_NYI, col["ptype"]
        gpu_ctx.synchronize()
        _sentinels_kept(batch)
    # ... and on numeric types, Dict and RLE pages included: no page body is looked at
    for ptype in (S.T_I16, S.T_F64):
        for codec in (S.RLE, S.DICT):
            col = gen.prim(ptype, 10_000, uniq=50, null_density=0.2, runs=5)
            check(gpu_ctx, col, codec=codec, ops=("count",), max_page_size=2050, force_codec=codec)


# ---- 6: read the keys, filter, aggregate per group: one interval, replayed and not
@pytest.mark.parametrize("freq", [False, True])
def test_read_keys_filter_then_aggregate_in_one_interval(gpu_ctx, freq):
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    from tests.test_gpu_freq import sparse
    rows = 10_007
    rng = np.random.default_rng(6)
    k32 = dict(ptype=S.T_U32, nullable=False, rows=rows, values=np.repeat(rng.integers(0, 6, rows // 3 + 1), 3)[:rows].astype(np.uint32),
               validity=None, offsets=None)
    k8 = dict(ptype=S.T_U8, nullable=False, rows=rows, values=rng.integers(0, 256, rows).astype(np.uint8), validity=None, offsets=None)
    k32p, k32m = gen.oracle_write(k32, max_page_size=2050)
    k8p, k8m = gen.oracle_write(k8, max_page_size=4100)
    x = sparse(S.T_I32, rows, 0.05, 2, null_density=0.1) if freq else gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    xp, xm = gen.oracle_write(x, max_page_size=2050, force_codec=S.FREQ if freq else S.RLE)
    xlit = 7 if freq else 60
    xr = R.Ref(x, xp, xm)
    mask = (xr.vals != xlit) & xr.valid
    assert 0 < mask.sum() < rows
    a = gen.prim(S.T_I64, rows, uniq=100, null_density=0.2, runs=6, seed=3)
    b = gen.prim(S.T_F64, rows, uniq=100, null_density=0.1, seed=4)
    ap, am = gen.oracle_write(a, max_page_size=4100, force_codec=S.RLE)
    bp, bm = gen.oracle_write(b, max_page_size=2050, force_codec=S.DICT)
    ar, br = R.Ref(a, ap, am), R.Ref(b, bp, bm)
    acp, bcp = upload(gpu_ctx, a, ap, am), upload(gpu_ctx, b, bp, bm)
    ids32 = R.Ref(k32, k32p, k32m).vals   # (the oracle's decode of the key pages)
    ids8 = R.Ref(k8, k8p, k8m).vals
    kcps = [upload(gpu_ctx, k32, k32p, k32m), upload(gpu_ctx, k8, k8p, k8m)]
    read.batch_read_columns(gpu_ctx, kcps)
    gpu_ctx.synchronize()   # (the read path's launch hints have seen these columns: no replay on the key read's account below)
    r0 = gpu_ctx.replays()
    keys = read.batch_read_columns(gpu_ctx, kcps)
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("ne", xlit)])
    dev32 = keys[0].values[:rows * 4].view(torch.uint32)
    dev8 = keys[1].values[:rows]
    res = sb.aggregate_grouped(gpu_ctx, [acp, bcp, bcp], [dev32, dev8, dev32], [5, 256, 6], sel[0])
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + (1 if freq else 0)
    assert np.array_equal(sel[0].numpy(), mask)
    G.check(res[0], G.want(ar, ids32, 5, mask), "a by the UInt32 key")
    G.check(res[1], G.want(br, ids8, 256, mask), "b by the UInt8 key")
    G.check(res[2], G.want(br, ids32, 6, mask), "b by the UInt32 key")
    assert res[0].out_of_range > 0 and res[2].out_of_range == 0


# ---- 7: refusals at the call
def test_refusals_at_the_call(gpu_ctx):
    from strawboat_amd import _native as N
    rows = 5000
    col = gen.prim(S.T_I64, rows, uniq=10, null_density=0.2)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.NONE)
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(9).random(rows) < 0.5
    bm = bitmap(gpu_ctx, mask)
    ids = some_ids(rows, 4)
    dev = ids_dev(gpu_ctx, ids, 4)
    boolean = gen.boolean(rows)
    bpages, bmetas = gen.oracle_write(boolean)
    bcp = upload(gpu_ctx, boolean, bpages, bmetas)

    def fresh(cps=None):
        return _raw_array(gpu_ctx, cps or [cp, cp], [bm, bm], dev, 4, 15)

    def refused(batch, code, what, mem=N.SB_MEM_DEVICE):
        assert gpu_ctx._lib.sb_aggregate_grouped(gpu_ctx._h, batch._arr, 2, mem) == code, what
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        _sentinels_kept(batch)

    def tweak(what, code=N.SB_ERR_INVALID, col=1, **fields):
        batch = fresh()
        for f, v in fields.items():
            setattr(batch._arr[col], f, v)
        refused(batch, code, what)

    for n_groups in (0, 257, 1 << 16):
        tweak("n_groups %d" % n_groups, n_groups=n_groups)
    for width in (0, 3, 8):
        tweak("group_id_width %d" % width, group_id_width=width)
    tweak("group_ids null with rows > 0", group_ids=None)
    tweak("group_ids misaligned", group_ids=dev.data_ptr() + 2)
    tweak("group_ids misaligned, width 2", group_ids=dev.data_ptr() + 1, group_id_width=2)
    tweak("group_ids too short", group_ids_capacity=rows * 4 - 1)
    tweak("groups null", groups=None)
    tweak("unknown ops bits", ops=16 | 1)
    tweak("reserved != 0", reserved=1)
    for bad in (-1, S.T_NULL + 1, 99):
        tweak("bad physical_type %d" % bad, col=0, physical_type=bad)
    tweak("misaligned selection", selection=bm.data_ptr() + 1)
    tweak("short selection_capacity", selection_capacity=(rows + 31) // 32 * 4 - 4)
    tweak("metas null with n_pages > 0", col=0, metas=None)
    for ops in (N.SB_AGG_MIN, N.SB_AGG_MAX, N.SB_AGG_SUM, 15):
        batch = fresh([cp, bcp])
        batch._arr[1].ops = ops
        refused(batch, N.SB_ERR_NYI, "min / max / sum on Boolean")
    refused(fresh(), N.SB_ERR_NYI, "SB_MEM_HOST", mem=N.SB_MEM_HOST)
    # a page outside [0, pages_len): the span check of the read calls' host tables
    batch = fresh()
    batch._arr[1].pages_len -= 1
    assert gpu_ctx._lib.sb_aggregate_grouped(gpu_ctx._h, batch._arr, 2, N.SB_MEM_DEVICE) == N.SB_ERR_IO
    _sentinels_kept(batch)
    with pytest.raises(N.NativeError) as e:   # (like its siblings', this refusal is the interval's result as well)
        gpu_ctx.synchronize()
    assert e.value.code == N.SB_ERR_IO
    # the same batch, as it was built, then succeeds
    batch = fresh()
    for r in batch.results:
        r.ops = 15
    res = batch.enqueue()
    gpu_ctx.synchronize()
    for r in res:
        G.check(r, G.want(ref, ids, 4, mask), "after the refusals")


# ---- 8: pages anywhere, empty and tiny columns, corrupt pages
def test_pages_at_any_byte_offset_and_in_any_order(gpu_ctx):
    from strawboat_amd import read
    rng = np.random.default_rng(10)
    ids = some_ids(10_000, 9)
    for codec in (S.NONE, S.RLE, S.DICT, S.LZ4):
        col = gen.prim(S.T_I64, 10_000, uniq=100, null_density=0.2, runs=6, seed=codec)
        pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
        ref = R.Ref(col, pages, metas)
        cps = []
        for shift in (1, 7, 15):
            buf, start = buffer_cases.place(pages, shift, 0x5A)
            dev = to_dev(gpu_ctx, buf)
            cps.append(read.ColumnPages(col["ptype"], True, dev[start:start + pages.size], metas))
        buf, offs = buffer_cases.scatter(pages, metas, order="descending")
        cps.append(read.ColumnPages(col["ptype"], True, to_dev(gpu_ctx, buf), metas, page_offsets=offs))
        for m in (rng.random(10_000) < 0.35, None):
            run(gpu_ctx, cps, [m] * 4, [ref] * 4, ids, 8, what="placed pages, codec %d" % codec, width=2)


def test_empty_and_tiny(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    dev = gpu_ctx.torch_device
    empty = read.ColumnPages(S.T_I64, True, torch.zeros(0, dtype=torch.uint8, device=dev), np.zeros((0, 2), np.uint64))
    no_ids = torch.zeros(0, dtype=torch.uint8, device=dev)
    for sel in (None, torch.zeros(0, dtype=torch.uint8, device=dev)):
        res = sb.aggregate_grouped(gpu_ctx, [empty], no_ids, 3, sel)
        gpu_ctx.synchronize()
        r = res[0]
        assert (r.rows, r.selected, r.out_of_range, len(r.groups)) == (0, 0, 0, 3)
        assert all(bytes(g._c) == bytes(64) and g.min is None and g.sum == 0 for g in r.groups)
    # ... and as one column of a call that has pages
    col = gen.prim(S.T_I32, 3000, uniq=5, null_density=0.3, seed=4)
    pages, metas = gen.oracle_write(col, max_page_size=777, force_codec=S.NONE)
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(1).random(3000) < 0.5
    ids = some_ids(3000, 4)
    res = sb.aggregate_grouped(gpu_ctx, [empty, cp, empty], [no_ids, ids_dev(gpu_ctx, ids, 1), no_ids], [2, 4, 256],
                               [None, bitmap(gpu_ctx, mask), None])
    gpu_ctx.synchronize()
    assert (res[0].rows, res[0].selected, res[2].selected, len(res[2].groups)) == (0, 0, 0, 256)
    assert all(bytes(g._c) == bytes(64) for g in res[2].groups)
    G.check(res[1], G.want(ref, ids, 4, mask), "next to empty columns")
    # one-row columns: the row selected / unselected / unselected by absence, null / not null, in / out of range
    for nd in (None, 0.5):
        for seed in (1, 2, 3, 4):
            col = gen.prim(S.T_I32, 1, uniq=5, null_density=nd, seed=seed)
            for one_id in (0, 1, 2):
                check(gpu_ctx, col, ids=np.array([one_id]), n_groups=2, masks=[np.array([True]), np.array([False]), None])
                check(gpu_ctx, col, ids=np.array([one_id]), n_groups=2, masks=[np.array([True]), np.array([False]), None], force_codec=S.NONE)
    col = gen.prim(S.T_I32, 2051, uniq=5, seed=4)   # a one-row page behind two others
    last = np.zeros(2051, bool)
    last[2050] = True
    for codec in (S.RLE, S.NONE, S.DICT):
        check(gpu_ctx, col, codec=codec, max_page_size=1025, force_codec=codec)
        check(gpu_ctx, col, masks=[last], max_page_size=1025, force_codec=codec)


def grouped_code(ctx, cp, rows, sel=True):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    try:
        sb.aggregate_grouped(ctx, [cp], ids_dev(ctx, np.arange(rows) % 3, 1), 3, to_dev(ctx, bitmap_of(np.ones(rows, bool))) if sel else None)
        ctx.synchronize()
    except NativeError as e:
        try:
            ctx.synchronize()
        except NativeError:
            pass
        return e.code
    return 0


def test_corrupt_pages_raise_what_the_decoder_raises(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
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
        assert grouped_code(gpu_ctx, cp, 9000) == want, codec
        assert grouped_code(gpu_ctx, cp, 9000, sel=False) == want, codec
    # a Dict page with an index >= D on a live row: plain u32 indices behind hdr9 Dict | hdr9 None
    col = gen.prim(S.T_I64, 40_000, uniq=50, seed=50)
    pages, metas = gen.oracle_write(col, max_page_size=40_000, force_codec=S.DICT, force_index_codec=S.NONE)
    bad = pages.copy()
    pos = 9 + 9 + 25_000 * 4
    bad[pos:pos + 4] = np.frombuffer(np.uint32(1 << 30).tobytes(), np.uint8)
    cp = upload(gpu_ctx, col, bad, metas)
    assert read_code(gpu_ctx, cp) == -1 and oracle_code(col, bad, metas) != 0
    assert grouped_code(gpu_ctx, cp, 40_000) == -1
    # hand-built RLE pages: a run that overshoots the page, runs that end before the page is full
    for (ptype, dtype, w, runs, rows), code in ((RLE_OVERSHOOT, -1), (RLE_SHORT, -3)):
        page = _rle_page(runs, w, dtype).copy()
        cp = upload(gpu_ctx, dict(ptype=ptype, nullable=False), page, np.array([[page.size, rows]], np.uint64))
        assert read_code(gpu_ctx, cp) == code
        assert grouped_code(gpu_ctx, cp, rows) == code
    # rows and selected are delivered even when the interval failed
    sel = np.random.default_rng(12).random(rows) < 0.5
    res = sb.aggregate_grouped(gpu_ctx, [cp], ids_dev(gpu_ctx, np.arange(rows) % 3, 1), 3, bitmap(gpu_ctx, sel))
    with pytest.raises(NativeError):
        gpu_ctx.synchronize()
    assert res[0].rows == rows and res[0].selected == int(sel.sum())
    # the context still works
    col = gen.prim(S.T_I64, 9000, uniq=60)
    check(gpu_ctx, col, max_page_size=3000, force_codec=S.DICT)


# ---- 9: a seeded sweep
SWEEP_SEED = 20261019
SWEEP_CASES = 40


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
        n_groups = int(rng.choice([1, 2, 3, 7, 64, 65, 255, 256]))
        width = int(rng.choice([1, 2, 4]))
        shape = int(rng.integers(0, 4))
        ops = [R.ALL, ("sum",), ("count",), ("min", "max")][int(rng.integers(0, 4))]
        col = gen.prim(ptype, rows, uniq=uniq, null_density=nd, runs=runs, seed=int(rng.integers(0, 1 << 30)))
        if kind == 0:
            mask = rng.random(rows) < p
        elif kind == 1:   # clustered: the bits of one stretch of the column
            mask = np.zeros(rows, bool)
            at = int(rng.integers(0, rows))
            mask[at:at + max(1, int(rows * p))] = True
        else:
            mask = (np.arange(rows) % int(rng.integers(2, 70))) == 0
        top = min(n_groups + (2 if case % 3 == 0 else 0), 256 if width == 1 else 1 << 16)   # (every third case: ids out of range)
        if shape == 0:
            ids = rng.integers(0, top, rows)
        elif shape == 1:
            ids = (np.arange(rows) // int(rng.choice([1, 63, 64, 65, 256, 4096]))) % top
        elif shape == 2:
            ids = np.full(rows, int(rng.integers(0, top)))
        else:
            ids = np.sort(rng.integers(0, top, rows))
        opt = dict(max_page_size=page)
        if codec >= 0:
            opt["force_codec"] = codec
        try:
            pages, metas = gen.oracle_write(col, **opt)
            ref = R.Ref(col, pages, metas)
            cp = upload(gpu_ctx, col, pages, metas)
            run(gpu_ctx, [cp, cp], [mask, None], [ref, ref], ids, n_groups, ops=ops, what="sweep", width=width)
        except AssertionError as e:
            raise AssertionError("seed %d case %d: type %d codec %d rows %d page %d nulls %r uniq %d runs %r p %r kind %d groups %d "
                                 "width %d ids %d ops %r: %s" % (SWEEP_SEED, case, ptype, codec, rows, page, nd, uniq, runs, p, kind,
                                                                 n_groups, width, shape, ops, e))
