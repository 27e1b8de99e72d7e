"""sb_aggregate_weighted and group_by_weighted on the GPU: pages written by the CPU oracle, count and sum(y * w) of the
selected rows per group computed on the device and compared with tests/aggregate_weighted_ref.py: the ORACLE's decode of the
pages reduced per group by Python ints (integer x integer: exact mod 2^128) and by exact rationals (float mode: within
(count_g + 2) * 2^-52 * sum_g|y w|, derived there).  Nothing here is compared with what the device's own decoder gives,
except where a test says so (SB_WGT_SQUARE against the same call with the decoded y as weights).

Shapes are the smallest that reach the edge: a tile is 4096 rows, a chunk -- the rows that share one table -- 16 tiles."""
import ctypes as C

import numpy as np
import pytest

from oracle import sbo as S
from tests import aggregate_grouped_ref as G
from tests import aggregate_ref as R
from tests import aggregate_weighted_ref as W
from tests import gen
from tests.test_gpu_aggregate import _column, _every_type_columns, bitmap
from tests.test_gpu_decode import LONG_RLE_ROWS, RLE_OVERSHOOT, _rle_page
from tests.test_gpu_read_selected import TYPES, oracle_code, read_code, to_dev, two_masks, upload
from tests.test_read_selected_host import bitmap_of

pytestmark = pytest.mark.gpu

NP = gen.NP_OF
SENTINEL = 0x5A
WORD = 0x5A5A5A5A5A5A5A5A
ID_DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32}
TILE, CHUNK = 4096, 16 * 4096
OPS = ("count", "sum")
I64_MIN, U64_MAX = -2 ** 63, 2 ** 64 - 1


def weights_of(dtype, rows, seed=0):
    """weights of a type: integers over the type's whole range, its extremes among them; floats with random mantissas"""
    rng = np.random.default_rng(3000 + seed)
    dt = np.dtype(dtype)
    if dt.kind == "f":
        return (rng.choice([-1.0, 1.0], rows) * (1.0 + rng.random(rows)) * rng.choice([1e-3, 1.0, 1e3], rows)).astype(dt)
    info = np.iinfo(dt)
    w = rng.integers(info.min, info.max, rows, dtype=dt, endpoint=True)
    w[rng.random(rows) < 0.05] = info.min
    w[rng.random(rows) < 0.05] = info.max
    return w


def some_ids(rows, top, seed=0):
    return np.random.default_rng(2000 + seed).integers(0, top, rows)


def dev_weights(ctx, w, wv=None, tail=False):
    return to_dev(ctx, w) if wv is None else (to_dev(ctx, w), to_dev(ctx, bitmap_of(wv, tail)))


def bits(res):
    return [[(g._c.sum_lo, g._c.sum_hi, g._c.count, g._c.nans) for g in r.groups] for r in res]


def records(res):
    return [bytes(r._groups) for r in res]


def run(ctx, cps, refs, ws, masks, ids, n_groups, ops=OPS, what="", width=4, wvs=None, square=False, tail=False):
    """the columns of ONE call, each with its own weights, weights' validity (None: all valid) and selection, one ids array
    (None: the ungrouped form) for all; checked against the reference"""
    import strawboat_amd as sb
    n = len(cps)
    wvs = wvs or [None] * n
    weights = None if square else [dev_weights(ctx, w, wv, tail) for w, wv in zip(ws, wvs)]
    dev_ids = None if ids is None else to_dev(ctx, np.asarray(ids).astype(ID_DTYPE[width]))
    res = sb.aggregate_weighted(ctx, cps, weights, dev_ids, n_groups, [bitmap(ctx, m, tail) for m in masks], ops=ops, square=square)
    ctx.synchronize()
    for i, (r, ref, m) in enumerate(zip(res, refs, masks)):
        W.check(r, W.want(ref, None if square else ws[i], wvs[i], ids, n_groups, m, ops), "%s column %d" % (what, i))
    return res


def codecs_of(col, pages, metas):
    return set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())


def check_pages(ctx, col, pages, metas, wtypes=(np.int64, np.float64), ids=None, n_groups=300, masks=None, what="", width=2, **kw):
    """a column under a random selection, a sparse one and none, once per weight type, all as columns of one call"""
    ref = R.Ref(col, pages, metas)
    rows = ref.rows
    if masks is None:
        masks = two_masks(rows, 11) + [None] if rows else [None]
    if ids is None and n_groups > 1:
        ids = some_ids(rows, n_groups + 3)
    cp = upload(ctx, col, pages, metas)
    ws = [weights_of(t, rows, k) for k, t in enumerate(wtypes) for _ in masks]
    return run(ctx, [cp] * len(ws), [ref] * len(ws), ws, list(masks) * len(wtypes), ids, n_groups, what=what, width=width, **kw)


def check(ctx, col, codec=None, **kw):
    opt = {k: kw.pop(k) for k in list(kw) if k in ("max_page_size", "force_codec", "force_index_codec", "ratio", "forbidden")}
    pages, metas = gen.oracle_write(col, **opt)
    if codec is not None:
        assert codecs_of(col, pages, metas) == {codec}, (codecs_of(col, pages, metas), codec)
    return check_pages(ctx, col, pages, metas, what="codec %r %r" % (codec, opt), **kw)


# ---- 1: a route per numeric codec of y
@pytest.mark.parametrize("codec,ptype", [(S.NONE, S.T_I64), (S.NONE, S.T_F32), (S.RLE, S.T_I32), (S.RLE, S.T_F64), (S.DICT, S.T_U16),
                                         (S.ONEVALUE, S.T_I8), (S.LZ4, S.T_I16), (S.ZSTD, S.T_I64), (S.SNAPPY, S.T_F64)])
def test_routes(gpu_ctx, codec, ptype):
    uniq = 1 if codec == S.ONEVALUE else 100
    col = gen.prim(ptype, 9000, uniq=uniq, null_density=0.2, runs=6, seed=codec)
    check(gpu_ctx, col, codec=codec, max_page_size=2050, force_codec=codec)


@pytest.mark.parametrize("uniq", [8192, 8193])
def test_dict_route_at_the_lds_dictionary_limit(gpu_ctx, uniq):
    rng = np.random.default_rng(uniq)
    rows = 9000
    v = np.concatenate([rng.permutation(uniq), rng.integers(0, uniq, rows - uniq)]).astype(np.int64) * 1_000_003 - 2 ** 40
    col = _column(S.T_I64, v, rng.random(rows) >= 0.1)
    pages, metas = gen.oracle_write(col, max_page_size=1 << 20, force_codec=S.DICT)
    assert metas.shape[0] == 1 and codecs_of(col, pages, metas) == {S.DICT}
    check_pages(gpu_ctx, col, pages, metas, what="dict %d" % uniq)


@pytest.mark.parametrize("ptype", [S.T_I32, S.T_U32])
@pytest.mark.parametrize("codec", [S.BITPACK, S.DELTABP])
def test_bitpacking_routes(gpu_ctx, ptype, codec):
    col = gen.prim(ptype, 128 * 70, uniq=1 << 13, sorted_=(codec == S.DELTABP))
    check(gpu_ctx, col, codec=codec, max_page_size=128 * 40, force_codec=codec)


def test_patas_route(gpu_ctx):
    rng = np.random.default_rng(3)
    v = np.round(rng.normal(100, 20, 9000), 2)
    col = dict(ptype=S.T_F64, nullable=True, rows=v.size, values=v, validity=gen.make_validity(rng, v.size, 0.2), offsets=None)
    check(gpu_ctx, col, codec=S.PATAS, max_page_size=2050, force_codec=S.PATAS)


# ---- 2: type pairings
@pytest.fixture(scope="module")
def typed_columns():
    out = {}
    for ptype in TYPES:
        rng = np.random.default_rng(ptype)
        rows = 5000
        v = weights_of(NP[ptype], rows, 50 + ptype)   # (the type's whole range)
        col = _column(ptype, v, rng.random(rows) >= 0.15)
        pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.NONE if ptype % 2 else S.RLE)
        out[ptype] = (col, pages, metas)
    return out


@pytest.mark.parametrize("ptype", TYPES)
def test_every_y_type_with_int64_and_float64_weights(gpu_ctx, typed_columns, ptype):
    col, pages, metas = typed_columns[ptype]
    check_pages(gpu_ctx, col, pages, metas, wtypes=(np.int64, np.float64), what="y type %d" % ptype)


def test_every_weight_type_with_an_int64_y(gpu_ctx, typed_columns):
    col, pages, metas = typed_columns[S.T_I64]
    check_pages(gpu_ctx, col, pages, metas, wtypes=tuple(NP[t] for t in TYPES), masks=[two_masks(5000, 3)[0]], what="weight types")
    col, pages, metas = typed_columns[S.T_U64]
    check_pages(gpu_ctx, col, pages, metas, wtypes=(np.uint64, np.int8, np.uint8), masks=[None], what="weight types, u64 y")


def test_float32_y_with_float32_weights(gpu_ctx, typed_columns):
    col, pages, metas = typed_columns[S.T_F32]
    check_pages(gpu_ctx, col, pages, metas, wtypes=(np.float32,), what="f32 x f32")


# ---- 3: row counts at the tile and chunk edges
EDGE_ROWS = (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 65535, 65536, 65537)


def test_zero_rows(gpu_ctx):
    """a column without a page (the oracle writes no empty chunk), alone and next to a column that has pages"""
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    dev = gpu_ctx.torch_device
    empty = read.ColumnPages(S.T_I64, True, torch.zeros(0, dtype=torch.uint8, device=dev), np.zeros((0, 2), np.uint64))
    no_ids = torch.zeros(0, dtype=torch.uint8, device=dev)
    no_w = torch.zeros(0, dtype=torch.float64, device=dev)
    for sel in (None, torch.zeros(0, dtype=torch.uint8, device=dev)):
        for kw in (dict(weights=[no_w], group_ids=no_ids, n_groups=3), dict(weights=[no_w]), dict(weights=None, square=True)):
            r = sb.aggregate_weighted(gpu_ctx, [empty], selection=sel, **kw)[0]
            gpu_ctx.synchronize()
            assert (r.rows, r.selected, r.out_of_range, len(r.groups)) == (0, 0, 0, kw.get("n_groups", 1))
            assert all(bytes(g._c) == bytes(64) and g.sum == 0 for g in r.groups)
    col = gen.prim(S.T_I32, 3000, uniq=5, null_density=0.3, seed=4)
    pages, metas = gen.oracle_write(col, max_page_size=777, force_codec=S.NONE)
    ref = R.Ref(col, pages, metas)
    mask = np.random.default_rng(1).random(3000) < 0.5
    ids, w = some_ids(3000, 5), weights_of(np.int16, 3000)
    res = sb.aggregate_weighted(gpu_ctx, [empty, upload(gpu_ctx, col, pages, metas), empty], [no_w, to_dev(gpu_ctx, w), no_w],
                                [no_ids, to_dev(gpu_ctx, ids.astype(np.uint8)), no_ids], [2, 4, 1024], [None, bitmap(gpu_ctx, mask), None])
    gpu_ctx.synchronize()
    assert (res[0].rows, res[0].selected, res[2].selected, len(res[2].groups)) == (0, 0, 0, 1024)
    assert all(bytes(g._c) == bytes(64) for g in res[2].groups)
    W.check(res[1], W.want(ref, w, None, ids, 4, mask), "next to empty columns")


@pytest.mark.parametrize("rows", EDGE_ROWS)
def test_row_counts_one_page(gpu_ctx, rows):
    for ptype, codec in ((S.T_I64, S.NONE), (S.T_F64, S.DICT)):
        col = gen.prim(ptype, rows, uniq=200, null_density=0.1, runs=3, seed=rows % 1000)
        pages, metas = gen.oracle_write(col, max_page_size=1 << 20, force_codec=codec)
        assert metas.shape[0] == 1
        ids = some_ids(rows, 303, rows)
        ids[rows - 1] = 299   # (the last row of the column has a group of its own)
        ids[:rows - 1][ids[:rows - 1] == 299] = 0
        res = check_pages(gpu_ctx, col, pages, metas, wtypes=(np.int64 if ptype == S.T_I64 else np.float64,), ids=ids, n_groups=300,
                          what="%d rows in one page" % rows)
        assert res[-1].groups[299].selected == 1


@pytest.mark.parametrize("rows", [4097, 65537])
def test_row_counts_short_pages(gpu_ctx, rows):
    """pages shorter than a tile: 16 of them to a chunk, the page of a tile found from first_tile"""
    col = gen.prim(S.T_F64, rows, uniq=500, null_density=0.1, runs=3, seed=rows % 1000)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.DICT)
    assert int(metas[:, 1].max()) <= TILE and metas.shape[0] > rows // TILE
    check_pages(gpu_ctx, col, pages, metas, what="short pages")


def test_one_long_rle_page_in_parts(gpu_ctx):
    rng = np.random.default_rng(4)
    ids = np.repeat(rng.integers(0, 1024, LONG_RLE_ROWS // 100 + 1), 100)[:LONG_RLE_ROWS]
    ids[::4099] = 1027   # (out of range)
    col = gen.prim(S.T_I64, LONG_RLE_ROWS, uniq=256, null_density=0.1, runs=32, seed=8)
    pages, metas = gen.oracle_write(col, force_codec=S.RLE)
    assert metas.shape[0] == 1 and codecs_of(col, pages, metas) == {S.RLE}
    res = check_pages(gpu_ctx, col, pages, metas, wtypes=(np.int64, np.float32), ids=ids, n_groups=1024,
                      masks=[rng.random(LONG_RLE_ROWS) < 0.01, None], what="long RLE page")
    assert res[1].out_of_range == len(range(0, LONG_RLE_ROWS, 4099))


# ---- 4: selections
def test_selections(gpu_ctx):
    rows = 2 * CHUNK + TILE + 5
    r = np.arange(rows)
    masks = [None, np.ones(rows, bool), np.zeros(rows, bool), (r % CHUNK) == 4097, (r % TILE == 0) | (r % TILE == TILE - 1) | (r == rows - 1)]
    for ptype, codec, page in ((S.T_I64, S.NONE, 1 << 20), (S.T_F64, S.DICT, 2050 * 4)):
        col = gen.prim(ptype, rows, uniq=500, null_density=0.1, runs=3, seed=7)
        pages, metas = gen.oracle_write(col, max_page_size=page, force_codec=codec)
        res = check_pages(gpu_ctx, col, pages, metas, wtypes=(np.float64 if ptype == S.T_F64 else np.int64,), masks=masks, what="selections")
        assert [x.selected for x in res] == [rows, rows, 0, 3, int(masks[4].sum())]


def test_selection_and_validity_bits_behind_rows_are_ignored(gpu_ctx):
    rows = 4097 + 13   # (not a multiple of 32)
    col = gen.prim(S.T_I64, rows, uniq=500, null_density=0.1, seed=9)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.NONE)
    ref = R.Ref(col, pages, metas)
    rng = np.random.default_rng(1)
    masks = [rng.random(rows) < 0.5, rng.random(rows) < 0.9]
    wvs = [rng.random(rows) < 0.8, rng.random(rows) < 0.5]
    ws = [weights_of(np.int64, rows), weights_of(np.float64, rows)]
    assert bitmap_of(wvs[0], True)[-1] & 0x80   # (the bits behind `rows` are set)
    run(gpu_ctx, [upload(gpu_ctx, col, pages, metas)] * 2, [ref] * 2, ws, masks, some_ids(rows, 40), 37, wvs=wvs, tail=True, what="tails")


# ---- 5: groups
@pytest.fixture(scope="module")
def shape_columns():
    out = []
    for ptype, codec, page in ((S.T_F64, S.NONE, 4100), (S.T_I64, S.RLE, 2050), (S.T_F32, S.DICT, 2048)):
        col = gen.prim(ptype, 6000, uniq=100, null_density=0.2, runs=4, seed=page)
        pages, metas = gen.oracle_write(col, max_page_size=page, force_codec=codec)
        out.append((col, pages, metas, R.Ref(col, pages, metas)))
    return out


@pytest.mark.parametrize("n_groups", [1, 2, 255, 256, 257, 1023, 1024])
def test_group_counts_and_id_widths(gpu_ctx, shape_columns, n_groups):
    """ids cover [0, n_groups + 3) and 0xFF.. markers: every group has rows, three ids and the markers are out of range"""
    rows = 6000
    rng = np.random.default_rng(n_groups)
    masks = two_masks(rows, 11) + [None]
    for k, (col, pages, metas, ref) in enumerate(shape_columns):
        width = (4, 2, 1)[k] if n_groups <= 250 else (4, 2, 4)[k]
        ids = rng.integers(0, n_groups + 3, rows)
        marker = (1 << (8 * width)) - 1
        ids[rng.random(rows) < 0.03] = marker
        ids[rng.permutation(rows)[:n_groups + 3]] = np.arange(n_groups + 3)
        cp = upload(gpu_ctx, col, pages, metas)
        ws = [weights_of(np.int64 if k == 1 else np.float64, rows, k)] * 3
        res = run(gpu_ctx, [cp] * 3, [ref] * 3, ws, masks, ids, n_groups, what="%d groups, width %d" % (n_groups, width), width=width)
        assert res[2].out_of_range >= int((ids == marker).sum()) > 0 and all(g.selected > 0 for g in res[2].groups)


def test_the_ungrouped_form(gpu_ctx, shape_columns):
    """group_ids NULL with n_groups 1 gives what ids of zeros give: the integer records identical, the float sums' bits too
    (the same rows meet the same table in the same order)"""
    rows = 6000
    masks = two_masks(rows, 5) + [None]
    for k, (col, pages, metas, ref) in enumerate(shape_columns):
        cp = upload(gpu_ctx, col, pages, metas)
        ws = [weights_of(np.int64 if k == 1 else np.float64, rows, k)] * 3
        none = run(gpu_ctx, [cp] * 3, [ref] * 3, ws, masks, None, 1, what="ungrouped")
        zeros = run(gpu_ctx, [cp] * 3, [ref] * 3, ws, masks, np.zeros(rows, np.int64), 1, what="ids of zeros", width=1)
        assert records(none) == records(zeros)
        assert all(r.out_of_range == 0 and r.groups[0].selected == r.selected for r in none)


# ---- 6: null weights, null y
def test_null_weights_and_null_y(gpu_ctx):
    rows = 9000
    rng = np.random.default_rng(6)
    yv = rng.random(rows) >= 0.3
    wv = rng.random(rows) >= 0.3
    both = ~yv & ~wv
    assert both.sum() > 300 and (yv & ~wv).sum() > 300 and (~yv & wv).sum() > 300
    ids = some_ids(rows, 13)
    for ptype, codec in ((S.T_I64, S.NONE), (S.T_F64, S.RLE), (S.T_I32, S.DICT)):
        col = _column(ptype, gen.prim(ptype, rows, uniq=300, runs=4)["values"], yv)
        pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
        ref = R.Ref(col, pages, metas)
        cp = upload(gpu_ctx, col, pages, metas)
        ws = [weights_of(np.int64, rows), weights_of(np.float64, rows), weights_of(np.int16, rows)]
        masks = [None, rng.random(rows) < 0.5, both | (rng.random(rows) < 0.1)]
        res = run(gpu_ctx, [cp] * 3, [ref] * 3, ws, masks, ids, 10, wvs=[wv, wv, wv], what="nulls")
        assert sum(g.count for g in res[0].groups) == int((yv & wv & (ids < 10)).sum())
        # all weights null: no live row, every selected row still counted
        res = run(gpu_ctx, [cp], [ref], ws[:1], [None], ids, 10, wvs=[np.zeros(rows, bool)], what="all weights null")
        assert all(g.count == 0 and g.sum == 0 for g in res[0].groups) and sum(g.selected for g in res[0].groups) + res[0].out_of_range == rows


def test_weights_and_validity_written_by_read_columns_in_the_same_interval(gpu_ctx):
    """sum(y * w) with w a nullable column: its DeviceArray -- `values` and the validity bitmap sb_read_columns writes -- handed
    in directly, read and aggregate in one interval"""
    import strawboat_amd as sb
    from strawboat_amd import read
    rows = 9001
    y = gen.prim(S.T_I64, rows, uniq=5000, null_density=0.1, seed=1)
    yp, ym = gen.oracle_write(y, max_page_size=2050, force_codec=S.NONE)
    yref = R.Ref(y, yp, ym)
    ids = some_ids(rows, 33)
    dev_ids = to_dev(gpu_ctx, ids.astype(np.uint8))
    mask = np.random.default_rng(2).random(rows) < 0.6
    for wtype, codec in ((S.T_I32, S.DICT), (S.T_F64, S.RLE)):
        w = gen.prim(wtype, rows, uniq=700, null_density=0.25, runs=3, seed=2)
        wp, wm = gen.oracle_write(w, max_page_size=4100, force_codec=codec)
        wref = R.Ref(w, wp, wm)
        arr = read.batch_read_columns(gpu_ctx, [upload(gpu_ctx, w, wp, wm)])[0]
        res = sb.aggregate_weighted(gpu_ctx, [upload(gpu_ctx, y, yp, ym)], [arr], dev_ids, 30, bitmap(gpu_ctx, mask))
        gpu_ctx.synchronize()   # (the only one)
        W.check(res[0], W.want(yref, wref.vals, wref.valid, ids, 30, mask), "weights from read_columns, type %d" % wtype)


# ---- 7: integer edges
def test_integer_edges(gpu_ctx):
    def one(ptype, v, wdtype, w, ids, n_groups, codec=S.NONE):
        col = _column(ptype, v)
        pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
        ref = R.Ref(col, pages, metas)
        return run(gpu_ctx, [upload(gpu_ctx, col, pages, metas)], [ref], [np.asarray(w, wdtype)], [None], ids, n_groups, what="integer edges")[0]

    # four rows of INT64_MIN * INT64_MIN in one group: 4 * 2^126 wraps to 0; three of them do not
    v = np.full(7, I64_MIN, np.int64)
    r = one(S.T_I64, v, np.int64, v, np.array([0, 0, 0, 0, 1, 1, 1]), 2)
    assert (r.groups[0]._c.sum_lo, r.groups[0]._c.sum_hi, r.groups[0].count) == (0, 0, 4)
    assert (r.groups[1]._c.sum_lo, r.groups[1]._c.sum_hi) == (0, 3 << 62)
    # UINT64_MAX^2 repeated, in both routes
    for codec in (S.NONE, S.RLE):
        n = 5000
        u = np.full(n, U64_MAX, np.uint64)
        r = one(S.T_U64, u, np.uint64, u, np.zeros(n, np.int64), 1, codec)
        assert (r.groups[0]._c.sum_hi << 64) | r.groups[0]._c.sum_lo == (n * U64_MAX * U64_MAX) % (1 << 128)
    # INT64_MIN * UINT64_MAX and the other way round
    r = one(S.T_I64, np.full(3, I64_MIN, np.int64), np.uint64, np.full(3, U64_MAX, np.uint64), np.zeros(3, np.int64), 1)
    assert (r.groups[0]._c.sum_hi << 64) | r.groups[0]._c.sum_lo == (3 * I64_MIN * U64_MAX) % (1 << 128)
    r = one(S.T_U64, np.full(3, U64_MAX, np.uint64), np.int64, np.full(3, I64_MIN, np.int64), np.zeros(3, np.int64), 1)
    assert (r.groups[0]._c.sum_hi << 64) | r.groups[0]._c.sum_lo == (3 * I64_MIN * U64_MAX) % (1 << 128)
    # mixed signs that cancel; sums that cross 2^64 and -2^64
    rng = np.random.default_rng(5)
    n = 6000
    y = rng.integers(-2 ** 62, 2 ** 62, n // 2)
    w = rng.integers(-2 ** 31, 2 ** 31, n // 2)
    r = one(S.T_I64, np.concatenate([y, y]), np.int64, np.concatenate([w, -w]), rng.integers(0, 1, n), 1)
    assert r.groups[0].sum == 0 and r.groups[0].count == n
    y = np.full(n, 2 ** 40, np.int64)
    w = np.where(np.arange(n) % 2 == 0, 2 ** 30, -2 ** 30).astype(np.int64)
    ids = np.arange(n) % 2
    r = one(S.T_I64, y, np.int64, w, ids, 2)
    assert r.groups[0].sum == (n // 2) * 2 ** 70 > 2 ** 64 and r.groups[1].sum == -(n // 2) * 2 ** 70 < -2 ** 64
    # narrow types extend by their own signedness: -128 * 255, 255 * 255, -128 * -128
    r = one(S.T_I8, np.array([-128, -128, 127], np.int8), np.uint8, np.array([255, 0, 255], np.uint8), np.array([0, 1, 2]), 3)
    assert [g.sum for g in r.groups] == [-128 * 255, 0, 127 * 255]
    r = one(S.T_U8, np.array([255, 255], np.uint8), np.int8, np.array([-128, 127], np.int8), np.array([0, 1]), 2)
    assert [g.sum for g in r.groups] == [255 * -128, 255 * 127]


# ---- 8: float specials
def test_float_specials(gpu_ctx):
    """group 0: NaN * 0 among finite rows; 1: inf * 0; 2: inf * -1 next to inf * 1; 3: inf * 1 alone; 4: -0.0 and 0.0;
    5: an integer y times inf; the rest finite"""
    rng = np.random.default_rng(8)
    rows = 9000
    for ptype, wdtype, codec in ((S.T_F64, np.float64, S.NONE), (S.T_F32, np.float32, S.RLE), (S.T_F64, np.int64, S.DICT)):
        dt = NP[ptype]
        v = np.repeat(rng.normal(0, 50, rows // 4 + 1), 4)[:rows].astype(dt)
        w = weights_of(wdtype, rows) if np.dtype(wdtype).kind == "f" else rng.integers(-1000, 1000, rows).astype(wdtype)
        ids = rng.integers(6, 40, rows)
        special = np.zeros(rows, bool)
        for at, yv, wv, group in (([10, 4097], np.nan, 0, 0), ([11], 1.5, 2, 0), ([500, 4095], np.inf, 0, 1), ([600], np.inf, -1, 2), ([601], np.inf, 1, 2),
                                  ([700, 8000], np.inf, 1, 3), ([20, 21], -0.0, 3, 4), ([22], 0.0, -3, 4)):
            v[at], w[at], ids[at], special[at] = yv, wv, group, True
        valid = rng.random(rows) >= 0.1
        valid[special] = True
        col = _column(ptype, v, valid)
        pages, metas = gen.oracle_write(col, max_page_size=4100, force_codec=codec)
        ref = R.Ref(col, pages, metas)
        cp = upload(gpu_ctx, col, pages, metas)
        masks = [special | (rng.random(rows) < 0.3), None]
        res = run(gpu_ctx, [cp] * 2, [ref] * 2, [w, w], masks, ids, 40, what="float specials")
        for r in res:
            g = r.groups
            assert g[0].nans == 2 and g[0].count == 3 and g[0].sum != g[0].sum
            assert g[1].nans == 2 and g[1].sum != g[1].sum                    # inf * 0 is NaN
            assert g[2].nans == 0 and g[2].sum != g[2].sum                    # -inf + inf
            assert g[3].nans == 0 and g[3].sum == np.inf
            assert g[4].count == 3 and g[4].sum == 0.0
    # an integer y with float weights that are infinite
    col = _column(S.T_I64, np.array([5, -5, 0, 7], np.int64))
    pages, metas = gen.oracle_write(col, force_codec=S.NONE)
    res = run(gpu_ctx, [upload(gpu_ctx, col, pages, metas)], [R.Ref(col, pages, metas)], [np.array([np.inf, np.inf, np.inf, 1.0])], [None],
              np.array([0, 1, 2, 3]), 4, what="integer y, infinite weights")
    assert [g.sum for g in res[0].groups[:2]] == [np.inf, -np.inf] and res[0].groups[2].nans == 1 and res[0].groups[3].sum == 7.0


# ---- 9: SB_WGT_SQUARE
@pytest.mark.parametrize("ptype,codec", [(S.T_I64, S.NONE), (S.T_U16, S.DICT), (S.T_I8, S.RLE), (S.T_F64, S.RLE), (S.T_F32, S.NONE)])
def test_square(gpu_ctx, typed_columns, ptype, codec):
    """against the reference, and against the same call with the decoded y as weights: integer records identical, float sums
    within the bound of the same reference (and here bit-identical: the same products meet the same table in the same order)"""
    col, _, _ = typed_columns[ptype]
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
    ref = R.Ref(col, pages, metas)
    rows = ref.rows
    cp = upload(gpu_ctx, col, pages, metas)
    masks = two_masks(rows, 11) + [None]
    ids = some_ids(rows, 23)
    if ptype in (S.T_F32, S.T_F64):   # (keep the squares far from overflow)
        small = np.abs(ref.vals.astype(np.float64)) < 1e100
        masks = [small & m if m is not None else small for m in masks]
    sq = run(gpu_ctx, [cp] * 3, [ref] * 3, None, masks, ids, 20, square=True, what="square")
    y = ref.vals.copy()
    y[~ref.valid] = 0
    same = run(gpu_ctx, [cp] * 3, [ref] * 3, [y] * 3, masks, ids, 20, wvs=[ref.valid] * 3, what="decoded y as weights")
    assert records(sq) == records(same)
    assert any(g.count for g in sq[0].groups)


# ---- 10: count only, on every physical type
def test_count_only_on_every_type(gpu_ctx):
    rng = np.random.default_rng(8)
    rows = 3000
    ids = rng.integers(0, 603, rows)
    wv = rng.random(rows) < 0.7
    cols = _every_type_columns() + [gen.prim(S.T_I64, rows, uniq=10, null_density=0.2), gen.prim(S.T_F32, rows, uniq=10)]
    for col in cols:
        pages, metas = gen.oracle_write(col, max_page_size=777)
        ref = R.Ref(col, pages, metas)
        cp = upload(gpu_ctx, col, pages, metas)
        masks = [rng.random(rows) < 0.35, two_masks(rows, 3)[1], None]
        for ops in (("count",), ()):
            res = run(gpu_ctx, [cp] * 3, [ref] * 3, [weights_of(np.float32, rows)] * 3, masks, ids, 600, ops=ops, wvs=[wv, None, wv],
                      what="count only, type %d" % col["ptype"], width=2)
            assert all(g.sum is None and g._c.sum_lo == 0 and g._c.nans == 0 for r in res for g in r.groups)
        if col["ptype"] == S.T_NULL:
            assert sum(g.count for g in res[2].groups) == 0 and sum(g.selected for g in res[2].groups) + res[2].out_of_range == rows


# ---- 11: the order of the float additions: the same bits every time, a replayed interval included
def _freq_column(ctx, ptype, rows=10_000):
    from tests.test_gpu_freq import sparse
    f = sparse(ptype, rows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    assert S.FREQ in codecs_of(f, fp, fm)
    return f, fp, fm, R.Ref(f, fp, fm), upload(ctx, f, fp, fm)


@pytest.mark.parametrize("n_groups", [5, 96])
@pytest.mark.parametrize("ptype,codec", [(S.T_F64, S.NONE), (S.T_F32, S.DICT), (S.T_F64, S.RLE)])
def test_float_sums_that_are_exact_in_no_order(gpu_ctx, ptype, codec, n_groups):
    import strawboat_amd as sb
    rows = CHUNK + TILE + 77   # (two chunks on the tile route)
    v, ids = G.inexact_values(rows, n_groups, seed=17)
    rng = np.random.default_rng(codec * 10 + ptype)
    w = 1.0 + rng.random(rows)   # (random mantissas)
    col = _column(ptype, v.astype(NP[ptype]), rng.random(rows) >= 0.1)
    pages, metas = gen.oracle_write(col, max_page_size=2050 * 9, force_codec=codec)
    assert codecs_of(col, pages, metas) == {codec}
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    masks = two_masks(rows, 11) + [None]
    res = run(gpu_ctx, [cp] * 3, [ref] * 3, [w] * 3, masks, ids, n_groups, what="inexact float sums", width=1)
    first = bits(res)
    dev_ids = to_dev(gpu_ctx, ids.astype(np.uint8))
    dw = to_dev(gpu_ctx, w)
    bitmaps = [bitmap(gpu_ctx, m) for m in masks]
    batch = sb.WeightedAggregateBatch(gpu_ctx, [cp] * 3, [dw] * 3, dev_ids, n_groups, bitmaps)
    for _ in range(3):   # fresh intervals
        again = batch.enqueue()
        gpu_ctx.synchronize()
        assert bits(again) == first
    # intervals that are issued again on another call's account: a filter on a Freq column, another weighted call on one
    f, fp, fm, fref, fcp = _freq_column(gpu_ctx, S.T_I64)
    fids = some_ids(fref.rows, 200)
    fdev = to_dev(gpu_ctx, fids.astype(np.uint32))
    fw = weights_of(np.float64, fref.rows, 9)
    fdw = to_dev(gpu_ctx, fw)
    fwant = W.want(fref, fw, None, fids, 200, None)
    for others in ("filter", "weighted"):
        r0 = gpu_ctx.replays()
        if others == "filter":
            sb.filter_columns(gpu_ctx, [fcp], [sb.Predicate("ne", 7)])
        else:
            fres = sb.aggregate_weighted(gpu_ctx, [fcp], [fdw], fdev, 200)
        again = batch.enqueue()
        gpu_ctx.synchronize()
        assert gpu_ctx.replays() == r0 + 1, others   # (a Freq page under a sink asks for the replay with or without hints)
        assert bits(again) == first, others
        if others == "weighted":
            W.check(fres[0], fwant, "the Freq column next to it")
    # ... and as columns of one call with a Freq column: the Freq column is decoded, the others stay where they were
    r0 = gpu_ctx.replays()
    both = sb.WeightedAggregateBatch(gpu_ctx, [cp] * 3 + [fcp], [dw] * 3 + [fdw], [dev_ids] * 3 + [fdev], [n_groups] * 3 + [200], bitmaps + [None]).enqueue()
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    assert bits(both[:3]) == first
    W.check(both[3], fwant, "the Freq column of the call")


@pytest.mark.parametrize("ptype", [S.T_I32, S.T_F64, S.T_F32])
def test_freq_pages_take_the_replay_route(gpu_ctx, ptype):
    """a Freq column against the reference and against plain pages of the same values; a float Freq column gives the same
    bits in every interval; count only looks at no page body and asks for no replay"""
    import strawboat_amd as sb
    f, fp, fm, fref, fcp = _freq_column(gpu_ctx, ptype)
    rows = fref.rows
    pp, pm = gen.oracle_write(f, max_page_size=2050, force_codec=S.NONE)
    pref, pcp = R.Ref(f, pp, pm), upload(gpu_ctx, f, pp, pm)
    assert np.array_equal(pref.valid, fref.valid) and np.array_equal(pref.vals[pref.valid], fref.vals[fref.valid])
    ids = some_ids(rows, 103)
    mask = np.random.default_rng(ptype).random(rows) < 0.4
    wf, wi = weights_of(np.float64, rows, 1), weights_of(np.int32, rows, 2)
    r0 = gpu_ctx.replays()
    res = run(gpu_ctx, [fcp, pcp, fcp, pcp], [fref, pref, fref, pref], [wf, wf, wi, wi], [mask, mask, None, None], ids, 100, what="freq")
    assert gpu_ctx.replays() == r0 + 1
    if ptype == S.T_I32:   # integer x integer: the records of the Freq pages are those of the plain pages
        assert records(res[2:3]) == records(res[3:4])
    first = bits(res)
    for _ in range(2):
        again = run(gpu_ctx, [fcp, pcp, fcp, pcp], [fref, pref, fref, pref], [wf, wf, wi, wi], [mask, mask, None, None], ids, 100, what="freq again")
        assert bits(again) == first
    # square on the decoded route
    run(gpu_ctx, [fcp], [fref], None, [mask], ids, 100, square=True, what="freq, square")
    # nothing selected: the replay all the same; count only: none
    r0 = gpu_ctx.replays()
    run(gpu_ctx, [fcp], [fref], [wf], [np.zeros(rows, bool)], ids, 100, what="freq, nothing selected")
    assert gpu_ctx.replays() == r0 + 1
    r0 = gpu_ctx.replays()
    run(gpu_ctx, [fcp], [fref], [wf], [mask], ids, 100, ops=("count",), what="freq, count only")
    assert gpu_ctx.replays() == r0


def test_next_to_the_large_call_on_the_same_inputs_the_marks_do_not_mix(gpu_ctx):
    """one interval: sb_aggregate_grouped_large and sb_aggregate_weighted over a Freq column and an RLE column each, in
    opposite orders; each call's Freq column is decoded for the replay, each call's RLE column stays on the page route"""
    import strawboat_amd as sb
    from tests.test_gpu_aggregate_grouped_large import bits as large_bits
    f, fp, fm, fref, fcp = _freq_column(gpu_ctx, S.T_I64)
    rows = fref.rows
    b = gen.prim(S.T_F64, rows, uniq=100, null_density=0.2, runs=6, seed=2)
    bp, bm = gen.oracle_write(b, max_page_size=4100, force_codec=S.RLE)
    bref, bcp = R.Ref(b, bp, bm), upload(gpu_ctx, b, bp, bm)
    ids = some_ids(rows, 703)
    dev = to_dev(gpu_ctx, ids.astype(np.uint32))
    mask = np.random.default_rng(1).random(rows) < 0.3
    bmp = bitmap(gpu_ctx, mask)
    w = weights_of(np.float64, rows)
    dw = to_dev(gpu_ctx, w)
    alone_w = sb.aggregate_weighted(gpu_ctx, [bcp], [dw], dev, 700, bmp)
    alone_l = sb.aggregate_grouped_large(gpu_ctx, [bcp], dev, 700, bmp)
    gpu_ctx.synchronize()
    r0 = gpu_ctx.replays()
    large = sb.aggregate_grouped_large(gpu_ctx, [fcp, bcp], dev, 700, bmp)
    wgt = sb.aggregate_weighted(gpu_ctx, [bcp, fcp], [dw, dw], dev, 700, bmp)
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    G.check(large[0], G.want(fref, ids, 700, mask), "the large call's Freq column")
    G.check(large[1], G.want(bref, ids, 700, mask), "the large call's RLE column")
    W.check(wgt[0], W.want(bref, w, None, ids, 700, mask), "the weighted call's RLE column")
    W.check(wgt[1], W.want(fref, w, None, ids, 700, mask), "the weighted call's Freq column")
    assert bits(wgt[:1]) == bits(alone_w) and large_bits(large[1:]) == large_bits(alone_l)


# ---- 12: buffers
def test_buffers_at_exactly_their_capacity(gpu_ctx):
    """`groups` of exactly n_groups records between two 4096-byte guards; weights, validity, ids and the selection at exactly
    their capacity, each at the end of a guarded device buffer; pages at an odd byte offset with scattered page_offsets"""
    import torch
    from strawboat_amd import _native as N
    from strawboat_amd.aggregate_grouped import GroupedAggregate
    from strawboat_amd.aggregate_weighted import WeightedAggregateBatch
    from strawboat_amd.read import ColumnPages
    rows, n_groups = 4097 + 33, 37
    rng = np.random.default_rng(12)
    col = gen.prim(S.T_I64, rows, uniq=500, null_density=0.1, seed=3)
    pages, metas = gen.oracle_write(col, max_page_size=1000, force_codec=S.NONE)
    ref = R.Ref(col, pages, metas)
    # the pages in reverse order, three bytes of filler in front of each, behind an odd offset
    m = np.array(metas, np.uint64)
    starts = np.concatenate([[0], np.cumsum(m[:, 0])[:-1]]).astype(np.int64)
    blob, offs, at = [np.full(1, 0xEE, np.uint8)], np.zeros(m.shape[0], np.uint64), 1
    for p in reversed(range(m.shape[0])):
        blob.append(np.full(3, 0xEE, np.uint8))
        at += 3
        offs[p] = at
        blob.append(pages[starts[p]:starts[p] + int(m[p, 0])])
        at += int(m[p, 0])
    blob = np.concatenate(blob)
    cp = ColumnPages(col["ptype"], col["nullable"], to_dev(gpu_ctx, blob), metas, page_offsets=offs)
    ids = some_ids(rows, n_groups + 2)
    w = weights_of(np.int32, rows)
    wv = rng.random(rows) < 0.8
    mask = rng.random(rows) < 0.6

    def at_the_end(a):
        """`a` as the last bytes of a device buffer (aligned to 8 inside it)"""
        raw = np.ascontiguousarray(a).view(np.uint8)
        pad = (-raw.size) % 8
        whole = to_dev(gpu_ctx, np.concatenate([np.full(64 + pad, 0xA5, np.uint8), raw]))
        return whole[64 + pad:].view(getattr(torch, str(np.ascontiguousarray(a).dtype)))

    d_ids = at_the_end(ids.astype(np.uint16))
    d_w = at_the_end(w)
    d_wv = at_the_end(bitmap_of(wv))
    d_sel = at_the_end(bitmap_of(mask))
    batch = WeightedAggregateBatch(gpu_ctx, [cp], [(d_w, d_wv)], d_ids, n_groups, d_sel)
    c = batch._arr[0]
    assert c.weights_capacity == rows * 4 and c.group_ids_capacity == rows * 2 and c.weights_validity_capacity == (rows + 31) // 32 * 4
    guard = 4096
    buf = (C.c_uint8 * (2 * guard + 64 * n_groups))()
    C.memset(buf, SENTINEL, C.sizeof(buf))
    garr = (N.AggGroupC * n_groups).from_buffer(buf, guard)
    c.groups = garr
    batch.enqueue()
    gpu_ctx.synchronize()
    raw = bytes(buf)
    assert raw[:guard] == bytes([SENTINEL]) * guard and raw[guard + 64 * n_groups:] == bytes([SENTINEL]) * guard
    got = GroupedAggregate(col["ptype"], 9, c, [garr[i] for i in range(n_groups)])
    W.check(got, W.want(ref, w, wv, ids, n_groups, mask), "buffers")


# ---- 13: chains in one interval
def test_filter_key_ids_and_aggregate_weighted_in_one_interval(gpu_ctx):
    import strawboat_amd as sb
    from tests.key_ids_ref import Ref as KeyRef
    rows = 12_011
    rng = np.random.default_rng(13)
    x = gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    xp, xm = gen.oracle_write(x, max_page_size=2050, force_codec=S.RLE)
    xr = R.Ref(x, xp, xm)
    y = gen.prim(S.T_I64, rows, uniq=5000, null_density=0.1, seed=2)
    yp, ym = gen.oracle_write(y, max_page_size=4100, force_codec=S.NONE)
    yr = R.Ref(y, yp, ym)
    pool = rng.choice(np.arange(-10 ** 15, 10 ** 15, 10 ** 9 + 7), 300, replace=False)
    k = _column(S.T_I64, pool[rng.integers(0, 300, rows)], rng.random(rows) >= 0.1)
    kp, km = gen.oracle_write(k, max_page_size=4100)
    kr = KeyRef(k, kp, km)
    w = weights_of(np.int64, rows)
    mask = (xr.vals < 60) & xr.valid
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("lt", 60)])
    keys = sb.key_ids(gpu_ctx, [upload(gpu_ctx, k, kp, km)], sel[0], max_keys=512)[0]
    res = sb.aggregate_weighted(gpu_ctx, [upload(gpu_ctx, y, yp, ym)], [to_dev(gpu_ctx, w)], keys.ids, 512, sel[0])
    gpu_ctx.synchronize()   # (the only one)
    order = sorted(set(kr.vals[mask & kr.valid].tolist()))
    assert keys.n_keys == len(order) and not keys.overflow
    dense = np.full(rows, 0xFFFFFFFF, np.int64)
    live_key = mask & kr.valid
    dense[live_key] = np.searchsorted(np.array(order), kr.vals[live_key])
    W.check(res[0], W.want(yr, w, None, dense, 512, mask), "filter -> key_ids -> aggregate_weighted")


def _dict_weighted(keys, key_valid, mask, ref, w):
    groups = {}
    for i in np.flatnonzero(mask & key_valid):
        g = groups.setdefault(keys[i], [0, []])
        g[0] += 1
        if ref.valid[i]:
            g[1].append((ref.vals[i].item(), w[i].item()))
    return groups


def _check_group_by_weighted(kres, agg, groups, mask, key_valid, max_keys, flt):
    from fractions import Fraction
    from strawboat_amd.group_by import trim
    order = sorted(groups)
    assert not kres.overflow and kres.n_keys == len(order)
    assert list(kres.keys.tolist() if hasattr(kres.keys, "tolist") else kres.keys) == order
    trimmed = trim(kres, [agg])[0]
    assert len(agg.groups) == max_keys and len(trimmed) == len(order)
    assert agg.selected == int(mask.sum()) and agg.out_of_range == int((mask & ~key_valid).sum())
    for g, key in enumerate(order):
        n_sel, terms = groups[key]
        got = trimmed[g]
        assert (got.selected, got.count) == (n_sel, len(terms)), g
        if not flt:
            assert got.sum == sum(a * b for a, b in terms), g
        else:
            exact = sum((Fraction(a) * Fraction(b) for a, b in terms), Fraction(0))
            bound = (len(terms) + 2) * Fraction(1, 2 ** 52) * sum((abs(Fraction(a) * Fraction(b)) for a, b in terms), Fraction(0))
            assert abs(Fraction(got.sum) - exact) <= bound, g
    for g in range(len(order), max_keys):
        assert bytes(agg.groups[g]._c) == bytes(64), g


def test_group_by_weighted(gpu_ctx):
    """an integer key, a Utf8 key and a two-column key, against a dict-based reference; group_by itself behaves as before"""
    import strawboat_amd as sb
    from tests import key_ids_var_ref as K
    from tests.key_ids_ref import Ref as KeyRef
    from tests.test_gpu_key_ids_var import pick, vocab
    rows = 9011
    rng = np.random.default_rng(14)
    y = gen.prim(S.T_I64, rows, uniq=5000, null_density=0.1, seed=2)
    yp, ym = gen.oracle_write(y, max_page_size=4100, force_codec=S.NONE)
    yr, ycp = R.Ref(y, yp, ym), upload(gpu_ctx, y, yp, ym)
    z = gen.prim(S.T_F64, rows, uniq=3000, null_density=0.2, runs=3, seed=3)
    zp, zm = gen.oracle_write(z, max_page_size=2050, force_codec=S.DICT)
    zr, zcp = R.Ref(z, zp, zm), upload(gpu_ctx, z, zp, zm)
    wi, wf = weights_of(np.int32, rows), weights_of(np.float64, rows)
    mask = rng.random(rows) < 0.7
    bmp = bitmap(gpu_ctx, mask)
    # an integer key, 300 distinct
    pool = rng.choice(np.arange(-10 ** 15, 10 ** 15, 10 ** 9 + 7), 300, replace=False)
    k = _column(S.T_I64, pool[rng.integers(0, 300, rows)], rng.random(rows) >= 0.1)
    kp, km = gen.oracle_write(k, max_page_size=4100)
    kr, kcp = KeyRef(k, kp, km), upload(gpu_ctx, k, kp, km)
    kres, aggs = sb.group_by_weighted(gpu_ctx, kcp, [ycp, zcp], [to_dev(gpu_ctx, wi), to_dev(gpu_ctx, wf)], bmp, max_keys=400)
    gpu_ctx.synchronize()
    _check_group_by_weighted(kres, aggs[0], _dict_weighted(kr.vals.tolist(), kr.valid, mask, yr, wi), mask, kr.valid, 400, False)
    _check_group_by_weighted(kres, aggs[1], _dict_weighted(kr.vals.tolist(), kr.valid, mask, zr, wf), mask, kr.valid, 400, True)
    # square through group_by_weighted
    kres, aggs = sb.group_by_weighted(gpu_ctx, kcp, [ycp], None, bmp, max_keys=400, square=True)
    gpu_ctx.synchronize()
    _check_group_by_weighted(kres, aggs[0], _dict_weighted(kr.vals.tolist(), kr.valid, mask, yr, yr.vals), mask, kr.valid, 400, False)
    # a Utf8 key
    voc = vocab(200, 10, maxlen=20)
    s = K.column(pick(voc, rows, 10), rng.random(rows) >= 0.15)
    sp, sm = gen.oracle_write(s, max_page_size=4100)
    sr, scp = K.Ref(s, sp, sm), upload(gpu_ctx, s, sp, sm)
    kres, aggs = sb.group_by_weighted(gpu_ctx, scp, [ycp], [to_dev(gpu_ctx, wi)], bmp, max_keys=1024)
    gpu_ctx.synchronize()
    _check_group_by_weighted(kres, aggs[0], _dict_weighted(sr.strs, sr.valid, mask, yr, wi), mask, sr.valid, 1024, False)
    # a two-column key: a small integer and the strings
    a = _column(S.T_I8, rng.integers(-1, 2, rows), rng.random(rows) >= 0.05)
    ap, am = gen.oracle_write(a, max_page_size=4100)
    ar, acp = KeyRef(a, ap, am), upload(gpu_ctx, a, ap, am)
    kres, aggs = sb.group_by_weighted(gpu_ctx, [acp, scp], [zcp], [to_dev(gpu_ctx, wf)], bmp, max_keys=1024)
    gpu_ctx.synchronize()
    both_valid = ar.valid & sr.valid
    tuples = list(zip(ar.vals.tolist(), sr.strs.tolist()))
    _check_group_by_weighted(kres, aggs[0], _dict_weighted(tuples, both_valid, mask, zr, wf), mask, both_valid, 1024, True)


def test_a_context_with_launch_hints_and_the_same_call_four_times(gpu_ctx, shape_columns):
    """reads first, so that the context holds launch hints (or none, under SB_NO_HINTS=1); then the same weighted call four
    times in one interval, and more calls than the context has staging slots"""
    import strawboat_amd as sb
    from strawboat_amd import read
    rows = 6000
    cps = [upload(gpu_ctx, col, pages, metas) for col, pages, metas, _ in shape_columns]
    refs = [r for _, _, _, r in shape_columns]
    for _ in range(3):
        read.batch_read_columns(gpu_ctx, cps)
        gpu_ctx.synchronize()
    ids = some_ids(rows, 70)
    dev = to_dev(gpu_ctx, ids.astype(np.uint8))
    ws = [weights_of(np.float64, rows, 1), weights_of(np.int64, rows, 2), weights_of(np.float32, rows, 3)]
    dws = [to_dev(gpu_ctx, w) for w in ws]
    mask = two_masks(rows, 4)[0]
    bmp = bitmap(gpu_ctx, mask)
    wants = [W.want(r, w, None, ids, 64, mask) for r, w in zip(refs, ws)]
    batch = sb.WeightedAggregateBatch(gpu_ctx, cps, dws, dev, 64, bmp)
    once = batch.enqueue()
    gpu_ctx.synchronize()
    for got, wanted in zip(once, wants):
        W.check(got, wanted, "once")
    first = bits(once)
    all_res = [sb.aggregate_weighted(gpu_ctx, cps, dws, dev, 64, bmp) for _ in range(4)]
    read.batch_read_columns(gpu_ctx, cps)
    all_res += [sb.aggregate_weighted(gpu_ctx, cps, dws, dev, 64, bmp) for _ in range(8)]
    gpu_ctx.synchronize()
    for res in all_res:
        assert bits(res) == first
        for got, wanted in zip(res, wants):
            W.check(got, wanted, "the same call again")


# ---- 14: refusals and errors
def _raw_array(ctx, cps, weights, bitmaps, dev_ids, n_groups, ops, extra=0, square=False):
    """a batch whose result fields and `groups` records (n_groups + extra of them) hold a sentinel"""
    from strawboat_amd import _native as N
    from strawboat_amd.aggregate_weighted import WeightedAggregateBatch
    batch = WeightedAggregateBatch(ctx, cps, weights, dev_ids, n_groups, bitmaps, ops=("count",), square=square)
    batch._garrs = []
    for i in range(len(cps)):
        batch._arr[i].ops = ops
        for f in ("rows", "selected", "out_of_range"):
            setattr(batch._arr[i], f, WORD)
        garr = (N.AggGroupC * (n_groups + extra))()
        C.memset(garr, SENTINEL, 64 * (n_groups + extra))
        batch._garrs.append(garr)
        batch._arr[i].groups = garr
    return batch


def _sentinels_kept(batch):
    for c, garr in zip(batch._arr, batch._garrs):
        assert all(getattr(c, f) == WORD for f in ("rows", "selected", "out_of_range"))
        assert bytes(garr) == bytes([SENTINEL]) * C.sizeof(garr)


def test_refusals_at_the_call(gpu_ctx):
    from strawboat_amd import _native as N
    from strawboat_amd.aggregate_grouped import GroupedAggregate
    rows = 5000
    col = gen.prim(S.T_I64, rows, uniq=10, null_density=0.2)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.NONE)
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(9).random(rows) < 0.5
    bm = bitmap(gpu_ctx, mask)
    ids = some_ids(rows, 600)
    dev = to_dev(gpu_ctx, ids.astype(np.uint32))
    w = weights_of(np.int64, rows)
    wv = np.random.default_rng(10).random(rows) < 0.8
    dw, dwv = to_dev(gpu_ctx, w), to_dev(gpu_ctx, bitmap_of(wv))
    others = []
    for other in (gen.boolean(rows), gen.binary(rows, uniq=20), gen.binary(rows, uniq=20, large=True), gen.prim(S.T_I128, rows, uniq=10),
                  gen.prim(S.T_I256, rows, uniq=10), dict(ptype=S.T_NULL, nullable=True, rows=rows, values=None, validity=None, offsets=None)):
        op, om = gen.oracle_write(other)
        others.append(upload(gpu_ctx, other, op, om))

    def fresh(cps=None):
        return _raw_array(gpu_ctx, cps or [cp, cp], [(dw, dwv), (dw, dwv)], [bm, bm], dev, 600, 9)

    def refused(batch, code, what, mem=N.SB_MEM_DEVICE):
        assert gpu_ctx._lib.sb_aggregate_weighted(gpu_ctx._h, batch._arr, 2, mem) == code, what
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        _sentinels_kept(batch)

    def tweak(what, code=N.SB_ERR_INVALID, **fields):
        batch = fresh()
        for f, v in fields.items():
            setattr(batch._arr[1], f, v)
        refused(batch, code, what)

    for n_groups in (0, 1025, 1 << 16):
        tweak("n_groups %d" % n_groups, n_groups=n_groups)
    for width in (0, 3, 8):
        tweak("group_id_width %d" % width, group_id_width=width)
    tweak("group_ids null with n_groups 600", group_ids=None)
    tweak("group_ids null with a width", group_ids=None, n_groups=1, group_ids_capacity=0)
    tweak("group_ids null with a capacity", group_ids=None, n_groups=1, group_id_width=0)
    tweak("group_ids misaligned", group_ids=dev.data_ptr() + 2)
    tweak("group_ids too short", group_ids_capacity=rows * 4 - 1)
    tweak("groups null", groups=None)
    tweak("unknown ops bits", ops=16 | 1)
    for ops in (N.SB_AGG_MIN, N.SB_AGG_MAX, 15):
        tweak("min / max", ops=ops)
    tweak("reserved != 0", reserved=1)
    tweak("unknown flags", flags=2)
    tweak("unknown flags beside square", flags=3)
    tweak("misaligned selection", selection=bm.data_ptr() + 1)
    tweak("short selection", selection_capacity=(rows + 31) // 32 * 4 - 1)
    for wt in (0, 9, 10, 13, 14, 15, 16, -1):   # Boolean, Int128, Int256, Binary, LargeBinary, Null, none
        tweak("weight_type %d" % wt, weight_type=wt)
    tweak("weights null", weights=None)
    tweak("weights misaligned", weights=dw.data_ptr() + 4)
    tweak("weights short", weights_capacity=rows * 8 - 1)
    tweak("weights short for a wider type", weight_type=12, weights_capacity=rows * 4)
    tweak("weights_validity misaligned", weights_validity=dwv.data_ptr() + 2)
    tweak("weights_validity short", weights_validity_capacity=(rows + 31) // 32 * 4 - 1)
    tweak("square with weights", flags=1)
    tweak("square with a weight_type", flags=1, weights=None, weights_capacity=0, weights_validity=None, weights_validity_capacity=0)
    tweak("square with a validity", flags=1, weights=None, weights_capacity=0, weight_type=0)
    tweak("square with a capacity", flags=1, weights=None, weights_validity=None, weights_validity_capacity=0, weight_type=0)
    for other in others:   # SUM on Boolean / Binary / LargeBinary / Int128 / Int256 / Null
        batch = fresh([cp, other])
        refused(batch, N.SB_ERR_NYI, "sum on a type that has none")
    refused(fresh(), N.SB_ERR_NYI, "SB_MEM_HOST", mem=N.SB_MEM_HOST)
    batch = fresh()   # a page outside [0, pages_len): the span check of the read calls' host tables
    batch._arr[1].pages_len -= 1
    assert gpu_ctx._lib.sb_aggregate_weighted(gpu_ctx._h, batch._arr, 2, N.SB_MEM_DEVICE) == N.SB_ERR_IO
    _sentinels_kept(batch)
    with pytest.raises(N.NativeError) as e:   # (like its siblings', this refusal is the interval's result as well)
        gpu_ctx.synchronize()
    assert e.value.code == N.SB_ERR_IO
    # the batch as it was built then succeeds; a `groups` array longer than n_groups keeps its sentinel behind record n_groups
    batch = _raw_array(gpu_ctx, [cp, cp], [(dw, dwv), dw], [bm, None], dev, 600, 9, extra=3)
    assert gpu_ctx._lib.sb_aggregate_weighted(gpu_ctx._h, batch._arr, 2, N.SB_MEM_DEVICE) == 0
    gpu_ctx.synchronize()
    for c, garr, m, v in zip(batch._arr, batch._garrs, (mask, None), (wv, None)):
        assert bytes(garr)[64 * 600:] == bytes([SENTINEL]) * (64 * 3)
        got = GroupedAggregate(col["ptype"], 9, c, [garr[i] for i in range(600)])
        W.check(got, W.want(ref, w, v, ids, 600, m), "after the refusals")
    # square and the ungrouped form in their consistent shapes are taken
    batch = _raw_array(gpu_ctx, [cp, cp], None, [bm, None], None, 1, 9, square=True)
    assert all(c.flags == N.SB_WGT_SQUARE and not c.weights and not c.group_ids and c.group_id_width == 0 for c in batch._arr)
    assert gpu_ctx._lib.sb_aggregate_weighted(gpu_ctx._h, batch._arr, 2, N.SB_MEM_DEVICE) == 0
    gpu_ctx.synchronize()
    for c, garr, m in zip(batch._arr, batch._garrs, (mask, None)):
        W.check(GroupedAggregate(col["ptype"], 9, c, [garr[0]]), W.want(ref, None, None, None, 1, m), "square, ungrouped")


def test_corrupt_pages_raise_what_the_decoder_raises(gpu_ctx):
    """the inputs of tests/test_gpu_aggregate_grouped_large.py::test_corrupt_pages_raise_what_the_decoder_raises"""
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError

    def code_of(cp, rows, sel):
        try:
            sb.aggregate_weighted(gpu_ctx, [cp], [to_dev(gpu_ctx, np.ones(rows, np.int64))], to_dev(gpu_ctx, (np.arange(rows) % 1000).astype(np.uint16)),
                                  1000, bitmap(gpu_ctx, np.ones(rows, bool)) if sel else None)
            gpu_ctx.synchronize()
        except NativeError as e:
            try:
                gpu_ctx.synchronize()
            except NativeError:
                pass
            return e.code
        return 0

    for codec in (S.NONE, S.RLE, S.DICT, S.LZ4):   # a truncated last page
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
        assert code_of(cp, 9000, True) == want, codec
        assert code_of(cp, 9000, False) == want, codec
    # a Dict page with an index >= D on a live row: plain u32 indices behind hdr9 Dict | hdr9 None
    col = gen.prim(S.T_I64, 40_000, uniq=50, seed=50)
    pages, metas = gen.oracle_write(col, max_page_size=40_000, force_codec=S.DICT, force_index_codec=S.NONE)
    bad = pages.copy()
    pos = 9 + 9 + 25_000 * 4
    bad[pos:pos + 4] = np.frombuffer(np.uint32(1 << 30).tobytes(), np.uint8)
    cp = upload(gpu_ctx, col, bad, metas)
    assert read_code(gpu_ctx, cp) == -1 and oracle_code(col, bad, metas) != 0
    assert code_of(cp, 40_000, True) == -1
    # a hand-built RLE page whose run overshoots the page; rows and selected are delivered even when the interval failed
    ptype, dtype, w, runs, rows = RLE_OVERSHOOT
    page = _rle_page(runs, w, dtype).copy()
    cp = upload(gpu_ctx, dict(ptype=ptype, nullable=False), page, np.array([[page.size, rows]], np.uint64))
    assert read_code(gpu_ctx, cp) == -1 and code_of(cp, rows, True) == -1
    sel = np.random.default_rng(12).random(rows) < 0.5
    res = sb.aggregate_weighted(gpu_ctx, [cp], [to_dev(gpu_ctx, np.ones(rows))], to_dev(gpu_ctx, (np.arange(rows) % 3).astype(np.uint8)), 1024,
                                bitmap(gpu_ctx, sel))
    with pytest.raises(NativeError):
        gpu_ctx.synchronize()
    assert res[0].rows == rows and res[0].selected == int(sel.sum())
    # the context still works
    check(gpu_ctx, gen.prim(S.T_I64, 9000, uniq=60), n_groups=1024, max_page_size=3000, force_codec=S.DICT)
