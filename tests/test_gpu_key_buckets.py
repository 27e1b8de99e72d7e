"""sb_key_buckets on the GPU: the range-bucket ids of a numeric key column, compared BYTE FOR BYTE, with rows / selected /
count / matched / nans, against tests/key_buckets_ref.py over the ORACLE's decode of the pages (the reference is checked on
its own against a plain Python loop in tests/test_key_buckets_host.py).  Nothing here is compared with what the device's
own decoder gives.

Every column comes from tests/key_buckets_cases.py (build(name) asserts the codec of every page; the host test walks the
whole table).  Unless a test says otherwise a column runs with no selection, with every 7th row selected and under a mask
that leaves whole tiles of 4096 rows unselected, left-closed and right-closed.  Null rows keep their stored bytes in the
pages, and the default bounds are drawn from ALL the values the oracle decodes, so a null row whose stored bytes lie in a
bucket, rows that equal a bound, rows between two bounds, below the first and above the last are in every case.

The identities of section 8 need no reference: with a column's own keys as bounds the ids are key_ids' ids + 1, halves of
a column against one list of bounds give the halves of the whole, and the count / sum records of group_by_buckets on the
halves add up."""
import os

import numpy as np
import pytest

from oracle import sbo as S
from tests import key_buckets_cases as Bc
from tests import key_buckets_ref as R
from tests.test_gpu_aggregate import bitmap
from tests.test_gpu_read_selected import oracle_code, read_code, to_dev, upload

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_BYTES = 4096
WORD = 0x5A5A5A5A5A5A5A5A
RESULTS = ("rows", "selected", "count", "matched", "nans")
TILE = 4096
NONE = R.NONE


def three_masks(rows, seed=0):
    """no selection, every 7th row, and a mask that leaves whole tiles unselected (every second tile, the first among them)"""
    r = np.arange(rows)
    tiles = ((r // TILE) % 2 == 1) & (np.random.default_rng(seed).random(rows) < 0.5)
    return [None, r % 7 == 0, tiles]


def is_float(b):
    return b.ref.vals.dtype.kind == "f"


def distinct(b, live_only=False):
    """the distinct values of the column that are no NaN, ascending under the column's comparison (-0.0 == +0.0)"""
    v = b.ref.vals[:b.rows]
    if live_only:
        v = v[b.ref.valid]
    if is_float(b):
        v = v[~np.isnan(v)]
    return np.unique(v)


def default_bounds(b, limit=1023):
    """every other distinct value of the column (null rows' stored values too) without the two smallest and the two
    largest: rows equal to a bound, between two bounds, below the first and above the last"""
    have = distinct(b)
    out = have[2:-2:2] if have.size >= 6 else have[::2]
    return np.ascontiguousarray(out[:limit])


def run(ctx, builts, bounds, bids=None, masks=None, widths=None, closed=False, nan_ids=None, what="", cps=None):
    """the columns of ONE call, each with its own bounds, bucket ids, selection, closedness, nan_id and id_width (None: the
    narrowest)"""
    import strawboat_amd as sb
    n = len(builts)
    bids = [None] * n if bids is None else bids
    masks = [None] * n if masks is None else masks
    widths = [None] * n if widths is None else widths
    closed = [closed] * n if isinstance(closed, bool) else closed
    nan_ids = [None] * n if nan_ids is None else nan_ids
    cps = [upload(ctx, b.col, b.pages, b.metas) for b in builts] if cps is None else cps
    res = sb.key_buckets(ctx, cps, bounds, None if all(v is None for v in bids) else bids, [bitmap(ctx, m) for m in masks], list(closed),
                         list(nan_ids), list(widths))
    ctx.synchronize()
    for i, (r, b) in enumerate(zip(res, builts)):
        R.check(r, R.want(b.ref, masks[i], bounds[i], bids[i], closed[i], nan_ids[i], r.id_width),
                "%s column %d (id_width %d, %s-closed)" % (what, i, r.id_width, "right" if closed[i] else "left"))
    return res


def sweep(ctx, name):
    """one column under its three masks x the three widths, left- and right-closed, with the buckets' numbers and with
    merged / dropped buckets (floats: with a nan_id): four calls of nine columns"""
    b = Bc.build(name)
    bounds = default_bounds(b)
    masks = three_masks(b.rows, len(name))
    cp = upload(ctx, b.col, b.pages, b.metas)
    combos = [(m, w) for m in masks for w in (1, 2, 4)]
    lists = [bounds[:200] if w == 1 else bounds for _, w in combos]   # (ids of one byte name at most 255 buckets)
    ms, ws = [m for m, _ in combos], [w for _, w in combos]
    res = None
    for closed in (False, True):
        res = run(ctx, [b] * 9, lists, None, ms, ws, closed, None, name, cps=[cp] * 9)
        # buckets merged five to an id, the open-ended ones dropped
        bids = [[NONE] + [(i * 7) % 5 for i in range(len(lx) - 1)] + [NONE] if len(lx) else [3] for lx in lists]
        nan_ids = [6 if is_float(b) else None] * 9
        run(ctx, [b] * 9, lists, bids, ms, ws, closed, nan_ids, name + ", merged", cps=[cp] * 9)
    return res


# ---- 1: the codec routes
INT_ROUTES = [n for n in Bc.INT_CASES if n.startswith("route_") and "freq" not in n] + ["dict_8192", "dict_8193"] + \
    [n for n in Bc.INT_CASES if n.startswith("rle_hand_")]
FLOAT_ROUTES = ["f64_none", "f64_lz4", "f64_zstd", "f64_snappy", "f64_rle", "f64_dict", "f64_patas", "f64_onevalue", "f64_onevalue_nan",
                "f64_dict_8192", "f64_dict_8193", "f32_none", "f32_rle", "f32_dict"]
assert "route_bitpack_i32" in INT_ROUTES and "route_deltabp_u32" in INT_ROUTES and "rle_hand_i64" in INT_ROUTES and "route_onevalue" in INT_ROUTES
assert set(FLOAT_ROUTES) <= set(Bc.CASES)


@pytest.mark.parametrize("name", INT_ROUTES + FLOAT_ROUTES)
def test_codec_routes(gpu_ctx, name):
    res = sweep(gpu_ctx, name)
    b = Bc.build(name)
    if "onevalue" not in name:   # the cases are shaped so that the live rows fall in more than two buckets
        assert len(set(R.ids_numpy(res[2]).tolist())) > 3, name
    if is_float(b) and name not in ("f64_onevalue",):
        assert res[2].nans > 0, name


@pytest.mark.parametrize("name", ["rle_long", "f64_rle_long"])
def test_rle_long_page_in_parts(gpu_ctx, name):
    b = Bc.build(name)
    bounds = default_bounds(b)
    masks = three_masks(b.rows, 3)
    run(gpu_ctx, [b] * 3, [bounds] * 3, None, masks, [2, 4, 2], False, None, "long RLE page")
    run(gpu_ctx, [b] * 3, [bounds] * 3, None, masks, [4, 2, 4], True, [None, 9, None] if is_float(b) else None, "long RLE page")


@pytest.mark.parametrize("f,p", [("route_freq_i32", "freq_plain_i32"), ("route_freq_i64", "freq_plain_i64"), ("route_freq_u8", "freq_plain_u8"),
                                 ("f64_freq", "f64_freq_plain")])
def test_freq_pages_are_the_replay_and_equal_plain_pages(gpu_ctx, f, p):
    f, p = Bc.build(f), Bc.build(p)
    bounds = default_bounds(f, 200)
    masks = three_masks(f.rows, 5)
    for closed in (False, True):   # ... and the same column again in the next interval
        r0 = gpu_ctx.replays()
        got = run(gpu_ctx, [f] * 3, [bounds] * 3, None, masks, [1, 2, 4], closed, None, "freq")
        assert gpu_ctx.replays() == r0 + 1
        r0 = gpu_ctx.replays()
        plain = run(gpu_ctx, [p] * 3, [bounds] * 3, None, masks, [1, 2, 4], closed, None, "plain pages of the same values")
        assert gpu_ctx.replays() == r0
        for a, c in zip(got, plain):
            assert a.ids.cpu().numpy().tobytes() == c.ids.cpu().numpy().tobytes()
            assert (a.count, a.matched, a.nans) == (c.count, c.matched, c.nans)


# ---- 2: all ten types, bounds and values at the extremes, values equal to a bound and one step to either side
@pytest.mark.parametrize("t", list(Bc.TYPE_NAME.values()))
def test_types_with_bounds_and_values_at_the_extremes(gpu_ctx, t):
    ptype = {v: k for k, v in Bc.TYPE_NAME.items()}[t]
    bounds = Bc.edge_bounds(ptype)
    for codec in ("none", "rle", "dict"):
        b = Bc.build("edge_%s_%s" % (t, codec))
        live = b.ref.vals[:b.rows][b.ref.valid]
        live = live[~np.isnan(live)] if is_float(b) else live
        assert np.isin(bounds, live).all()   # every bound is a live row's value, and so are its two neighbours
        masks = three_masks(b.rows, 1)
        for closed in (False, True):
            res = run(gpu_ctx, [b] * 3, [bounds] * 3, None, masks, [1, 2, 4], closed, [5, None, 0xFFFFFFFE] if is_float(b) else None,
                      "edges %s %s" % (t, codec))
            ids = R.ids_numpy(res[0])[b.ref.valid]
            assert set(ids.tolist()) >= set(range(1, bounds.size))   # every inner bucket has rows
    if not is_float(Bc.build("edge_%s_none" % t)):   # ... and the spread columns of the lookup tests, on the three walks
        for codec in ("none", "rle", "dict"):
            b = Bc.build("type_%s_%s" % (t, codec))
            run(gpu_ctx, [b] * 3, [default_bounds(b)] * 3, None, three_masks(b.rows, 2), [1, 2, 4], codec == "rle", None, "type %s %s" % (t, codec))


# ---- 3: row counts
@pytest.mark.parametrize("pages", [2, 9])
def test_row_counts(gpu_ctx, pages):
    bs = [Bc.build("rows_%d_%d" % (r, pages)) for r in Bc.ROW_COUNTS] + [Bc.build("f64_rows_%d" % r) for r in Bc.ROW_COUNTS]
    for k, mask_of in enumerate((lambda b: None, lambda b: np.arange(b.rows) % 7 == 0, lambda b: np.arange(b.rows) >= TILE)):
        run(gpu_ctx, bs, [default_bounds(b) for b in bs], None, [mask_of(b) for b in bs], [(1, 2, 4)[(i + k) % 3] for i in range(len(bs))],
            [bool((i + k) % 2) for i in range(len(bs))], [7 if is_float(b) and k else None for b in bs], "row counts, %d pages" % pages)


def test_one_column_of_more_than_tile_grid_tiles(gpu_ctx):
    b = Bc.build("big_u8")
    assert b.rows == 4096 * 4096 + 1
    bounds = np.array([0, 7, 100, 199, 201, 255], np.uint8)
    mask = three_masks(b.rows, 9)[2]
    res = run(gpu_ctx, [b, b], [bounds, bounds], [None, [NONE, 1, 1, 0, 0, 1, NONE]], [None, mask], [1, 1], [False, True], None,
              "the grid's second sweep")
    assert res[0].matched == res[0].count == b.rows and 0 < res[1].matched < res[1].count and 0 < res[1].selected < b.rows


# ---- 4: the number of bounds
def _padded_bounds(b, n):
    """n bounds: the column's own, and beyond them values it does not hold"""
    have = default_bounds(b)
    if is_float(b):
        extra = np.arange(1, 1100, dtype=have.dtype) * 0.5 + 1_000_000.25
    else:
        extra = np.arange(1, 1100).astype(have.dtype) * 2 + 1_000_001
    full = np.unique(np.concatenate([have, extra]))
    return np.ascontiguousarray(full[:n])


@pytest.mark.parametrize("name", ["dict_8192", "route_none", "route_rle", "f64_dict", "f64_rle", "f64_lz4"])
def test_0_1_2_3_1022_and_1023_bounds(gpu_ctx, name):
    b = Bc.build(name)
    masks = three_masks(b.rows, 8)
    for n in (0, 1, 2, 3, 1022, 1023):
        bounds = _padded_bounds(b, n)
        assert bounds.size == n
        for closed in (False, True):
            res = run(gpu_ctx, [b] * 3, [bounds] * 3, None, masks, [2, 4, 2], closed, None, "%s, %d bounds" % (name, n))
            if n == 0:   # every value falls in bucket 0
                ids = R.ids_numpy(res[0])
                nan = np.isnan(b.ref.vals[:b.rows]) if is_float(b) else np.zeros(b.rows, bool)
                assert (ids[b.ref.valid & ~nan] == 0).all() and (ids[~b.ref.valid | nan] == 65535).all()
                assert res[0].matched == res[0].count - res[0].nans


# ---- 5: closedness and float specials
@pytest.mark.parametrize("name", ["route_none", "route_rle", "route_dict", "route_zstd", "dict_8193", "route_bitpack_i32", "route_deltabp_u32",
                                  "f64_none", "f64_rle", "f64_dict", "f64_patas", "f32_dict", "edge_f64_none", "edge_i64_rle"])
def test_the_closedness_flags_differ_exactly_on_the_rows_that_equal_a_bound(gpu_ctx, name):
    b = Bc.build(name)
    bounds = Bc.edge_bounds(b.col["ptype"]) if name.startswith("edge_") else default_bounds(b)
    left, right = run(gpu_ctx, [b, b], [bounds, bounds], None, None, [4, 4], [False, True], None, name + ", closedness")
    li, ri = R.ids_numpy(left).astype(np.int64), R.ids_numpy(right).astype(np.int64)
    on_bound = b.ref.valid & np.isin(b.ref.vals[:b.rows], bounds)
    assert on_bound.any() and ((li != ri) == on_bound).all() and (li[on_bound] == ri[on_bound] + 1).all()
    vals = b.ref.vals[:b.rows]
    if not name.startswith("edge_"):   # (the edge bounds begin and end with the extremes of the type)
        below, above = b.ref.valid & (vals < bounds[0]), b.ref.valid & (vals > bounds[-1])
        assert below.any() and above.any() and (li[below] == 0).all() and (ri[below] == 0).all()
        assert (li[above] == bounds.size).all() and (ri[above] == bounds.size).all()


@pytest.mark.parametrize("name", ["f64_none", "f64_rle", "f64_dict", "f64_lz4", "f64_patas", "f32_none", "f32_rle", "f32_dict"])
def test_zeros_infinities_and_nans(gpu_ctx, name):
    b = Bc.build(name)
    dt = b.ref.vals.dtype
    v, ok = b.ref.vals[:b.rows], b.ref.valid
    nan = ok & np.isnan(v)
    neg0, pos0 = ok & (v == 0) & np.signbit(v), ok & (v == 0) & ~np.signbit(v)
    assert nan.any() and neg0.any() and pos0.any() and (ok & np.isposinf(v)).any() and (ok & np.isneginf(v)).any()
    assert (np.signbit(v) & nan).any() and (~np.signbit(v) & nan).any()   # NaNs of both signs
    zero = [np.array([0.0], dt), np.array([-0.0], dt)]                      # +-0.0 against a bound of either zero
    infs = np.array([-np.inf, -1.0, 1.0, np.inf], dt)                       # +-inf as bounds (and as values)
    res = run(gpu_ctx, [b] * 6, zero + zero + [infs, infs], None, None, [1] * 6, [False, False, True, True, False, True],
              [None, 9, None, 9, 254, None], name + ", specials")
    for r, closed in zip(res[:4], (False, False, True, True)):
        ids = R.ids_numpy(r)
        assert (ids[neg0] == (0 if closed else 1)).all() and (ids[pos0] == (0 if closed else 1)).all()
    for r, nan_id in zip(res, (None, 9, None, 9, 254, None)):
        ids = R.ids_numpy(r)
        assert r.nans == int(nan.sum()) and (ids[nan] == (255 if nan_id is None else nan_id)).all()
        assert r.matched == r.count - (r.nans if nan_id is None else 0)
    li, ri = R.ids_numpy(res[4]), R.ids_numpy(res[5])
    assert (li[ok & np.isneginf(v)] == 1).all() and (ri[ok & np.isneginf(v)] == 0).all()   # -inf equals the first bound
    assert (li[ok & np.isposinf(v)] == 4).all() and (ri[ok & np.isposinf(v)] == 3).all()
    assert (li[ok & (v == np.finfo(dt).max)] == 3).all()


def test_a_page_of_nothing_but_nans(gpu_ctx):
    b = Bc.build("f64_onevalue_nan")
    bounds = np.array([-1.0, 1.0])
    res = run(gpu_ctx, [b] * 3, [bounds] * 3, [None, [0, 1, 2], None], three_masks(b.rows, 1), [1, 2, 4], [False, True, False], [None, 3, 0xFFFFFFFE],
              "nothing but NaNs")
    assert res[0].matched == 0 and res[0].nans == res[0].count > 0 and res[1].matched == res[1].count == res[1].nans > 0


# ---- 6: ids, nulls and selections
@pytest.mark.parametrize("width,largest", [(1, 254), (2, 65534), (4, 0xFFFFFFFE)])
def test_the_largest_id_each_width_allows(gpu_ctx, width, largest):
    for name in ("route_none", "route_rle", "route_dict", "f64_none", "f64_rle", "f64_dict"):
        b = Bc.build(name)
        bounds = default_bounds(b)[:3]
        res = run(gpu_ctx, [b], [bounds], [[largest, 0, largest, 1]], [None], [width], False, [largest if is_float(b) else None],
                  "%s, id %d" % (name, largest))[0]
        ids = R.ids_numpy(res)
        assert int(ids.astype(np.uint64)[b.ref.valid].min()) == 0 and largest in ids.tolist() and res.matched == res.count


def test_bucket_ids_that_merge_buckets_and_drop_the_open_ended_ones(gpu_ctx):
    for name in ("route_dict", "route_rle", "route_lz4", "f64_dict", "f64_rle", "f64_snappy"):
        b = Bc.build(name)
        bounds = default_bounds(b)[:6]
        bids = [None, 4, 4, 2, 2, 4, NONE]   # below the first and above the last: no id; three and two buckets share one
        res = run(gpu_ctx, [b, b], [bounds, bounds], [bids, None], None, [1, 1], False, None, name + ", merged")
        ids, plain = R.ids_numpy(res[0]), R.ids_numpy(res[1])
        assert set(ids.tolist()) == {2, 4, 255} and (ids[np.isin(plain, (0, 6))] == 255).all() and (ids[np.isin(plain, (1, 2, 5))] == 4).all()
        assert res[0].matched == int(np.isin(plain, (1, 2, 3, 4, 5)).sum()) < res[0].count


def test_a_null_row_whose_stored_bytes_lie_in_a_bucket_gets_all_ones(gpu_ctx):
    for name in ("route_none", "route_rle", "route_dict", "f64_none", "f64_dict"):
        b = Bc.build(name)
        assert (~b.ref.valid).any(), name
        res = run(gpu_ctx, [b], [default_bounds(b)], None, [None], [2], False, None, name + ", nulls")[0]
        assert (R.ids_numpy(res)[~b.ref.valid] == 65535).all() and res.count == int(b.ref.valid.sum())


def test_validity_and_selection_bits_behind_rows_are_ignored(gpu_ctx):
    import strawboat_amd as sb
    from tests.test_read_selected_host import bitmap_of
    for name in ("rows_4097_2", "f64_rows_4097", "edge_i64_none", "edge_f64_rle", "edge_u8_dict"):
        b = Bc.with_validity_bits_behind_rows(name)
        assert b.rows % 32
        bounds = default_bounds(b)
        mask = np.random.default_rng(3).random(b.rows) < 0.6
        tail = bitmap_of(mask, True)
        assert tail[-1] & 0x80   # (the bits behind `rows` are set)
        cp = upload(gpu_ctx, b.col, b.pages, b.metas)
        res = sb.key_buckets(gpu_ctx, [cp, cp], [bounds, bounds], selection=[to_dev(gpu_ctx, tail), None], id_width=[2, 2])
        gpu_ctx.synchronize()
        R.check(res[0], R.want(b.ref, mask, bounds), name + ", tails")
        R.check(res[1], R.want(b.ref, None, bounds), name + ", validity tails")


# ---- 7: where the output lands
def _guarded(ctx, nbytes, align=1):
    import torch
    whole = torch.full((2 * GUARD_BYTES + nbytes,), GUARD, dtype=torch.uint8, device=ctx.torch_device)
    assert whole.data_ptr() % 4 == 0 and GUARD_BYTES % align == 0
    return whole[GUARD_BYTES:GUARD_BYTES + nbytes], whole


def _guards_intact(whole, nbytes):
    h = whole.cpu().numpy()
    return bool((h[:GUARD_BYTES] == GUARD).all() and (h[GUARD_BYTES + nbytes:] == GUARD).all())


@pytest.mark.parametrize("id_width", [1, 2, 4])
def test_ids_of_exactly_their_size_between_guards(gpu_ctx, id_width):
    import torch
    import strawboat_amd as sb
    from strawboat_amd.key_ids import ID_DTYPES
    for name in ("route_none", "route_rle", "route_dict", "route_lz4", "rows_4097_2", "rows_8193_9", "f64_none", "f64_rle", "f64_rows_4097",
                 "f64_freq"):
        b = Bc.build(name)
        bounds = default_bounds(b, 100)
        cp = upload(gpu_ctx, b.col, b.pages, b.metas)
        for mask in three_masks(b.rows, id_width):
            ids_bytes, whole = _guarded(gpu_ctx, b.rows * id_width, id_width)
            ids = ids_bytes.view(getattr(torch, ID_DTYPES[id_width]))
            batch = sb.KeyBucketsBatch(gpu_ctx, [cp], [bounds], None, bitmap(gpu_ctx, mask), id_width=id_width, out=[ids])
            assert batch._arr[0].ids_capacity == b.rows * id_width
            res = batch.enqueue()
            gpu_ctx.synchronize()
            assert _guards_intact(whole, b.rows * id_width), "a byte outside ids was written"
            R.check(res[0], R.want(b.ref, mask, bounds, id_width=id_width), name + ", between guards")


def test_pages_at_odd_byte_offsets_and_scattered_page_offsets(gpu_ctx):
    import torch
    from strawboat_amd import read
    for name in ("route_none", "route_rle", "route_dict", "route_lz4", "f64_none", "f64_rle", "f64_dict", "f64_patas"):
        b = Bc.build(name)
        col, pages, metas = b.col, b.pages, b.metas
        cps = []
        for off in (1, 3, 7):
            buf = torch.zeros(off + pages.size, dtype=torch.uint8, device=gpu_ctx.torch_device)
            buf[off:] = torch.from_numpy(np.ascontiguousarray(pages)).to(gpu_ctx.torch_device)
            cps.append(read.ColumnPages(col["ptype"], col["nullable"], buf[off:], metas))
        # the pages in descending order in the buffer, with gaps of odd lengths between them
        lens = [int(x) for x in metas[:, 0]]
        starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
        offs, at = [0] * len(lens), 5
        for p in range(len(lens) - 1, -1, -1):
            offs[p] = at
            at += lens[p] + 3 + 2 * p
        buf = np.full(at, 0xEE, np.uint8)
        for p in range(len(lens)):
            buf[offs[p]:offs[p] + lens[p]] = pages[starts[p]:starts[p] + lens[p]]
        cps.append(read.ColumnPages(col["ptype"], col["nullable"], to_dev(gpu_ctx, buf), metas, page_offsets=np.array(offs, np.uint64)))
        bounds = default_bounds(b, 200)
        for mask in three_masks(b.rows, 7):
            run(gpu_ctx, [b] * 4, [bounds] * 4, None, [mask] * 4, [1, 2, 4, 1], [False, True, False, True], None, name + ", offsets", cps=cps)


# ---- 8: identities that need no reference
def _halves(ctx, b):
    """the column's pages as one column and as two: the first pages and the rest"""
    from strawboat_amd import read
    k = b.metas.shape[0] // 2
    cut = int(b.metas[:k, 0].sum())
    rows0 = int(b.metas[:k, 1].sum())
    assert 0 < rows0 < b.rows
    mk = lambda pg, mt: read.ColumnPages(b.col["ptype"], b.col["nullable"], to_dev(ctx, pg), mt)   # noqa: E731
    return mk(b.pages, b.metas), mk(b.pages[:cut], b.metas[:k]), mk(b.pages[cut:], b.metas[k:]), rows0


@pytest.mark.parametrize("name", ["route_none", "route_rle", "route_dict", "route_zstd", "type_u8_dict", "type_i16_rle"])
def test_a_columns_own_keys_as_bounds_give_the_ids_of_key_ids_plus_one(gpu_ctx, name):
    import strawboat_amd as sb
    b = Bc.build(name)
    whole, first, rest, rows0 = _halves(gpu_ctx, b)
    for mask in three_masks(b.rows, 2):
        bm = bitmap(gpu_ctx, mask)
        kid = sb.key_ids(gpu_ctx, [whole], bm, max_keys=1024, id_width=2)[0]
        gpu_ctx.synchronize()
        assert not kid.overflow and kid.n_keys <= 1023
        keys = np.ascontiguousarray(kid.keys)
        got = sb.key_buckets(gpu_ctx, [whole], [keys], selection=bm, id_width=2)[0]
        gpu_ctx.synchronize()
        want = kid.ids.cpu().numpy().view(np.uint16).astype(np.int64)
        ids = R.ids_numpy(got).astype(np.int64)
        live = want != 65535
        assert (ids[live] == want[live] + 1).all() and (ids[~live] == 65535).all(), name
        assert (got.rows, got.selected, got.count, got.matched, got.nans) == (kid.rows, kid.selected, kid.count, kid.count, 0)
        # the two halves of the pages against the same bounds: the two halves of the whole column's ids
        m0, m1 = (None, None) if mask is None else (mask[:rows0], mask[rows0:])
        parts = sb.key_buckets(gpu_ctx, [first, rest], [keys, keys], selection=[bitmap(gpu_ctx, m0), bitmap(gpu_ctx, m1)], id_width=2)
        gpu_ctx.synchronize()
        assert parts[0].ids.cpu().numpy().tobytes() + parts[1].ids.cpu().numpy().tobytes() == got.ids.cpu().numpy().tobytes(), name
        assert parts[0].count + parts[1].count == kid.count and parts[0].rows == rows0


@pytest.mark.parametrize("name", ["route_none", "route_rle", "dict_8192", "f64_none", "f64_rle", "f64_dict", "f32_dict", "f64_patas", "f64_freq"])
def test_histogram_gives_the_counts_of_the_reference(gpu_ctx, name):
    import strawboat_amd as sb
    b = Bc.build(name)
    cp = upload(gpu_ctx, b.col, b.pages, b.metas)
    bounds = default_bounds(b)
    for mask in three_masks(b.rows, 4):
        for closed in (False, True):
            h = sb.histogram(gpu_ctx, cp, bounds, bitmap(gpu_ctx, mask), closed)
            gpu_ctx.synchronize()
            want = R.histogram(b.ref, mask, bounds, closed)
            assert h.counts.tolist() == want.tolist() and h.counts.size == bounds.size + 1, (name, closed)
            w = R.want(b.ref, mask, bounds, None, closed)
            assert h.nans == w.nans and int(h.counts.sum()) == w.count - w.nans == h.buckets.matched
            assert h.aggregate.out_of_range == w.selected - w.matched


@pytest.mark.parametrize("name,n_bounds", [("route_dict", 20), ("f64_rle", 30), ("keys_700_dict", 300), ("f64_dict_8193", 600)])
def test_group_records_of_the_halves_add_up_to_the_wholes(gpu_ctx, name, n_bounds):
    """integer count / sum records are index-aligned under one list of bounds: adding them is the merge"""
    import strawboat_amd as sb
    from tests import gen
    b = Bc.build(name)
    rng = np.random.default_rng(3)
    whole_cp = upload(gpu_ctx, b.col, b.pages, b.metas)
    if b.metas.shape[0] > 1:
        _, first, rest, rows0 = _halves(gpu_ctx, b)
    else:   # (one page: the halves of its rows, written again)
        rows0 = b.rows // 2 + 5
        valid = np.unpackbits(b.col["validity"], bitorder="little")[:b.rows].astype(bool)
        parts = []
        for lo, hi in ((0, rows0), (rows0, b.rows)):
            part = Bc.floats(b.col["ptype"], b.col["values"][lo:hi], valid[lo:hi])
            pg, mt = gen.oracle_write(part, max_page_size=3000, force_codec=S.NONE)
            parts.append(upload(gpu_ctx, part, pg, mt))
        first, rest = parts
    y = Bc.Kc.ints(S.T_I64, rng.integers(-10 ** 12, 10 ** 12, b.rows), rng.random(b.rows) >= 0.1)
    ys = []
    for lo, hi in ((0, b.rows), (0, rows0), (rows0, b.rows)):
        part = Bc.Kc.ints(S.T_I64, y["values"][lo:hi], np.unpackbits(y["validity"], bitorder="little")[lo:hi].astype(bool))
        pg, mt = gen.oracle_write(part, max_page_size=3000, force_codec=S.NONE)
        ys.append(upload(gpu_ctx, part, pg, mt))
    mask = rng.random(b.rows) < 0.6
    bounds = _padded_bounds(b, n_bounds)
    nan_id = n_bounds + 1 if is_float(b) else None
    kres, aggs = sb.group_by_buckets(gpu_ctx, whole_cp, bounds, [ys[0]], bitmap(gpu_ctx, mask), ops=("count", "sum"), nan_id=nan_id)
    gpu_ctx.synchronize()
    R.check(kres, R.want(b.ref, mask, bounds, None, False, nan_id, kres.id_width), name + ", group_by_buckets")
    n_groups = n_bounds + (2 if is_float(b) else 1)
    assert aggs[0].n_groups == n_groups
    halves = []
    for cp, ycp, m in ((first, ys[1], mask[:rows0]), (rest, ys[2], mask[rows0:])):
        look, agg = sb.group_by_buckets(gpu_ctx, cp, bounds, [ycp], bitmap(gpu_ctx, m), ops=("count", "sum"), nan_id=nan_id)
        gpu_ctx.synchronize()
        halves.append((look, agg[0]))
    assert halves[0][0].matched + halves[1][0].matched == kres.matched and halves[0][0].nans + halves[1][0].nans == kres.nans
    ids = R.ids_numpy(kres).astype(np.int64)
    yv = np.unpackbits(y["validity"], bitorder="little")[:b.rows].astype(bool)
    for g in range(n_groups):
        a, h0, h1 = aggs[0][g], halves[0][1][g], halves[1][1][g]
        assert (h0.selected + h1.selected, h0.count + h1.count, h0.sum + h1.sum) == (a.selected, a.count, a.sum), (name, g)
        in_group = ids == g
        assert a.selected == int(in_group.sum()) and a.count == int((in_group & yv).sum()), (name, g)
        if a.count:
            assert a.sum == int(y["values"][in_group & yv].astype(object).sum()), (name, g)
    assert halves[0][1].out_of_range + halves[1][1].out_of_range == aggs[0].out_of_range


def test_the_same_call_four_times_gives_the_same_bytes(gpu_ctx):
    import strawboat_amd as sb
    names = ["route_none", "route_rle", "route_dict", "route_lz4", "route_onevalue", "route_bitpack_i32", "rle_hand_i16", "f64_none", "f64_rle",
             "f64_dict", "f64_patas", "f32_dict", "f64_onevalue_nan"]
    bs = [Bc.build(n) for n in names]
    cps = [upload(gpu_ctx, b.col, b.pages, b.metas) for b in bs]
    bounds = [default_bounds(b, 250) for b in bs]
    masks = [three_masks(b.rows, i)[i % 3] for i, b in enumerate(bs)]
    closed = [bool(i % 2) for i in range(len(bs))]
    nan_ids = [3 if is_float(b) and i % 3 else None for i, b in enumerate(bs)]
    batch = sb.KeyBucketsBatch(gpu_ctx, cps, bounds, None, [bitmap(gpu_ctx, m) for m in masks], closed, nan_ids, [2, 4] * 6 + [2])
    seen = []
    for _ in range(4):   # fresh intervals
        res = batch.enqueue()
        gpu_ctx.synchronize()
        seen.append([(r.ids.cpu().numpy().tobytes(), r.rows, r.selected, r.count, r.matched, r.nans) for r in res])
    assert all(s == seen[0] for s in seen[1:])
    for i, (r, b) in enumerate(zip(res, bs)):
        R.check(r, R.want(b.ref, masks[i], bounds[i], None, closed[i], nan_ids[i], r.id_width), names[i] + ", again")


# ---- 9: intervals
@pytest.mark.parametrize("name", ["dict_8192", "f64_dict_8192"])
def test_filter_then_key_buckets_then_every_grouped_aggregate_in_one_interval(gpu_ctx, name):
    import strawboat_amd as sb
    from tests import gen
    from tests.aggregate_ref import Ref, reduce_values
    kb = Bc.build(name)
    xcol = gen.prim(S.T_I32, kb.rows, uniq=100, null_density=0.2, runs=4, seed=1)
    xp, xm = gen.oracle_write(xcol, max_page_size=2050, force_codec=S.RLE)
    xr = Ref(xcol, xp, xm)
    ycol = gen.prim(S.T_I64, kb.rows, uniq=5000, null_density=0.1, seed=2)
    yp, ym = gen.oracle_write(ycol, max_page_size=4100, force_codec=S.NONE)
    yr = Ref(ycol, yp, ym)
    wv = np.random.default_rng(5).integers(-9, 10, kb.rows).astype(np.int64)
    mask = (xr.vals[:kb.rows] < 60) & xr.valid
    have = distinct(kb, True)

    def weighted(ctx, cols, ids, n_groups, sel):
        import torch
        return sb.aggregate_weighted(ctx, cols, [to_dev(ctx, wv.view(np.uint8)).view(torch.int64)], ids, n_groups, sel)

    for n_groups, call in ((40, sb.aggregate_grouped), (1000, sb.aggregate_grouped_large), (300, weighted)):
        bounds = np.ascontiguousarray(have[::8][:n_groups - 1])
        sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, xcol, xp, xm)], [sb.Predicate("lt", 60)])
        got = sb.key_buckets(gpu_ctx, [upload(gpu_ctx, kb.col, kb.pages, kb.metas)], [bounds], selection=sel[0])[0]
        agg = call(gpu_ctx, [upload(gpu_ctx, ycol, yp, ym)], got.ids, n_groups, sel[0])[0]
        gpu_ctx.synchronize()   # (the only one)
        assert np.array_equal(sel[0].numpy(), mask)
        w = R.want(kb.ref, mask, bounds, None, False, None, got.id_width)
        R.check(got, w, "behind the filter")
        assert agg.out_of_range == w.selected - w.matched
        for g in (0, 1, n_groups // 2, bounds.size):
            in_group = w.ids == g
            assert agg[g].selected == int(in_group.sum()), g
            if call is weighted:
                live = in_group & yr.valid
                assert agg[g].count == int(live.sum()) and agg[g].sum == int((yr.vals[:kb.rows][live].astype(object) * wv[live].astype(object)).sum()), g
            else:
                r = reduce_values(S.T_I64, yr.vals, in_group & yr.valid, int(in_group.sum()))
                assert agg[g].count == r.count, g
                if r.count:
                    assert agg[g].sum == int(yr.vals[:kb.rows][in_group & yr.valid].astype(object).sum()), g


def test_key_buckets_ids_beside_key_ids_ids_in_key_combine(gpu_ctx):
    import strawboat_amd as sb
    a, f = Bc.build("route_dict"), Bc.build("f64_rle")
    assert a.rows == f.rows
    bounds = default_bounds(f)[:20]
    mask = three_masks(a.rows, 4)[1]
    bm = bitmap(gpu_ctx, mask)
    kid = sb.key_ids(gpu_ctx, [upload(gpu_ctx, a.col, a.pages, a.metas)], bm, max_keys=1024, id_width=2)[0]
    got = sb.key_buckets(gpu_ctx, [upload(gpu_ctx, f.col, f.pages, f.metas)], [bounds], selection=bm)[0]
    comb = sb.key_combine(gpu_ctx, [(kid.ids, 1024), (got.ids, bounds.size + 1)], max_keys=1024)
    gpu_ctx.synchronize()
    w = R.want(f.ref, mask, bounds, None, False, None, got.id_width)
    R.check(got, w, "the buckets part")
    ka = kid.ids.cpu().numpy().view(np.uint16)
    both = (ka != 65535) & (w.ids != 255)
    tuples = sorted(set(zip(ka[both].tolist(), w.ids[both].tolist())))
    assert not comb.overflow and comb.live == int(both.sum()) and [tuple(t) for t in comb.tuples.tolist()] == tuples
    cid = comb.ids.cpu().numpy().view(R.ID_NP[comb.id_width])
    place = {t: i for i, t in enumerate(tuples)}
    want = np.array([place[(x, y)] if ok else (1 << (8 * comb.id_width)) - 1 for x, y, ok in zip(ka.tolist(), w.ids.tolist(), both.tolist())])
    assert np.array_equal(cid, want)


def test_inside_an_interval_that_another_call_causes_to_be_replayed(gpu_ctx):
    import strawboat_amd as sb
    x = Bc.build("route_freq_i32")
    names = ["route_none", "route_rle", "route_dict", "route_lz4", "f64_none", "f64_rle", "f64_dict", "f64_patas"]
    bs = [Bc.build(n) for n in names]
    bounds = [default_bounds(b, 100) for b in bs]
    masks = [three_masks(b.rows, 2)[i % 3] for i, b in enumerate(bs)]
    cps = [upload(gpu_ctx, b.col, b.pages, b.metas) for b in bs]
    closed = [False, True] * 4
    r0 = gpu_ctx.replays()
    sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x.col, x.pages, x.metas)], [sb.Predicate("ne", 7)])
    res = sb.key_buckets(gpu_ctx, cps, bounds, selection=[bitmap(gpu_ctx, m) for m in masks], right_closed=closed, id_width=[1, 2, 4, 1, 2, 4, 1, 2])
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    for i, (r, b) in enumerate(zip(res, bs)):
        R.check(r, R.want(b.ref, masks[i], bounds[i], None, closed[i], None, r.id_width), names[i] + ", in a replayed interval")


def test_columns_of_different_types_and_widths_in_one_call(gpu_ctx):
    names = ["route_none", "f64_dict", "type_u8_rle", "f32_none", "route_onevalue", "f64_onevalue_nan", "type_i16_dict", "f64_lz4",
             "route_freq_i64", "f64_freq", "type_u64_none", "f32_rle"]
    bs = [Bc.build(n) for n in names]
    bounds = [default_bounds(b, 150) for b in bs]
    masks = [three_masks(b.rows, 3)[i % 3] for i, b in enumerate(bs)]
    widths = [1, 4, 2, 1, 4, 2, 1, 2, 4, 1, 2, 4]
    closed = [bool(i % 2) for i in range(len(bs))]
    nan_ids = [200 if is_float(b) and i % 4 else None for i, b in enumerate(bs)]
    r0 = gpu_ctx.replays()
    run(gpu_ctx, bs, bounds, None, masks, widths, closed, nan_ids, "mixed")
    assert gpu_ctx.replays() == r0 + 1   # (the Freq columns)
    run(gpu_ctx, bs[::-1], bounds[::-1], None, masks[::-1], widths[::-1], closed[::-1], nan_ids[::-1], "mixed, the columns turned round")


def test_on_a_context_that_holds_launch_hints(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd import read
    from tests import gen
    ctx = sb.Context(0)
    try:
        rle, plain, flt = Bc.build("rle_long"), Bc.build("route_none"), Bc.build("f64_dict")
        cp = upload(ctx, rle.col, rle.pages, rle.metas)
        for _ in range(3):   # the hints now say: RLE pages alone, no tiles
            read.read_simple(ctx, cp)
        r0 = ctx.replays()
        # columns of tiles: a read call would be issued again for them; this call goes by no hint
        bs = [rle, plain, flt]
        run(ctx, bs, [default_bounds(b) for b in bs], None, [three_masks(b.rows, 1)[1] for b in bs], [2, 1, 4], [False, True, False], None, "behind reads")
        assert ctx.replays() == r0
        # ... and feeds none: the same RLE read is right without a replay, the first read of the column of tiles is issued again
        want = gen.oracle_read(rle.col, rle.pages, rle.metas)
        got = read.read_simple(ctx, cp)
        assert np.array_equal(got.values_numpy(), want["values"]) and ctx.replays() == r0
        if os.environ.get("SB_NO_HINTS", "0") == "0":
            pcp = upload(ctx, plain.col, plain.pages, plain.metas)
            got = read.read_simple(ctx, pcp)
            assert np.array_equal(got.values_numpy(), gen.oracle_read(plain.col, plain.pages, plain.metas)["values"]) and ctx.replays() == r0 + 1
    finally:
        ctx.close()


# ---- 10: refusals through the raw C call
def _raw(ctx, cps, bounds, bitmaps, rows, id_width=2, bids=None, nan_id=None):
    import torch
    import strawboat_amd as sb
    batch = sb.KeyBucketsBatch(ctx, cps, bounds, bids, bitmaps, False, nan_id, id_width)
    batch._ids = []
    for i in range(len(cps)):
        ids = torch.full((rows * id_width + 8,), GUARD, dtype=torch.uint8, device=ctx.torch_device)
        batch._arr[i].ids = ids.data_ptr()
        batch._arr[i].ids_capacity = rows * id_width + 8
        batch._ids.append(ids)
        for f in RESULTS:
            setattr(batch._arr[i], f, WORD)
    return batch


def _canaries_kept(batch):
    for c, ids in zip(batch._arr, batch._ids):
        assert all(getattr(c, f) == WORD for f in RESULTS)
        assert bool((ids == GUARD).all())


def test_refusals_at_the_call(gpu_ctx):
    from strawboat_amd import _native as N
    ib, fb = Bc.build("route_none"), Bc.build("f64_none")
    rows = ib.rows
    assert fb.rows == rows
    icp, fcp = upload(gpu_ctx, ib.col, ib.pages, ib.metas), upload(gpu_ctx, fb.col, fb.pages, fb.metas)
    mask = three_masks(rows, 9)[1]
    bm = bitmap(gpu_ctx, mask)
    il, fl = default_bounds(ib, 50), default_bounds(fb, 50)
    bids = [list(range(len(il) + 1)), list(range(len(fl) + 1))]

    def fresh(**kw):
        return _raw(gpu_ctx, [icp, fcp], [il, fl], [bm, bm], rows, bids=bids, **kw)

    def refused(batch, code, what, mem=N.SB_MEM_DEVICE):
        assert gpu_ctx._lib.sb_key_buckets(gpu_ctx._h, batch._arr, 2, mem) == code, what
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        _canaries_kept(batch)

    def each(change, code, what):
        for i in (0, 1):
            batch = fresh()
            change(batch._arr[i])
            refused(batch, code, "%s (column %d)" % (what, i))

    for w in (0, 3, 8, 0xFFFFFFFF):
        each(lambda c, w=w: setattr(c, "id_width", w), N.SB_ERR_INVALID, "id_width %d" % w)
    each(lambda c: setattr(c, "ids", None), N.SB_ERR_INVALID, "ids null")
    each(lambda c: setattr(c, "ids", c.ids + 1), N.SB_ERR_INVALID, "ids misaligned")
    each(lambda c: setattr(c, "ids_capacity", rows * 2 - 1), N.SB_ERR_INVALID, "ids too small")
    each(lambda c: setattr(c, "reserved0", 1), N.SB_ERR_INVALID, "reserved0 != 0")
    each(lambda c: setattr(c, "reserved", 1), N.SB_ERR_INVALID, "reserved != 0")
    batch = fresh()
    batch._arr[1].ids = batch._arr[0].ids + rows * 2 - 2   # the last id of column 0 is the first of column 1
    refused(batch, N.SB_ERR_INVALID, "ids of two columns overlap")
    for bad in (-1, S.T_NULL + 1, 99):
        each(lambda c, bad=bad: setattr(c, "physical_type", bad), N.SB_ERR_INVALID, "bad physical_type %d" % bad)
    each(lambda c: setattr(c, "selection", c.selection + 1), N.SB_ERR_INVALID, "misaligned selection")
    each(lambda c: setattr(c, "selection_capacity", (rows + 31) // 32 * 4 - 4), N.SB_ERR_INVALID, "short selection_capacity")
    each(lambda c: setattr(c, "metas", None), N.SB_ERR_INVALID, "metas null with n_pages > 0")
    for ptype in (S.T_BIN32, S.T_BIN64, S.T_BOOL, S.T_I128, S.T_I256, S.T_NULL):
        each(lambda c, ptype=ptype: setattr(c, "physical_type", ptype), N.SB_ERR_NYI, "type %d" % ptype)
    batch = fresh()
    refused(batch, N.SB_ERR_NYI, "SB_MEM_HOST", mem=N.SB_MEM_HOST)
    # the flags and the bounds
    for bit in (2, 4, 0x80000000, 3):
        each(lambda c, bit=bit: setattr(c, "flags", bit), N.SB_ERR_INVALID, "flags %#x" % bit)
    each(lambda c: setattr(c, "n_bounds", 1024), N.SB_ERR_INVALID, "n_bounds above SB_BUCKET_MAX_BOUNDS")
    each(lambda c: setattr(c, "bounds", None), N.SB_ERR_INVALID, "bounds null")
    keep = []

    def bounds_of(i, arr):
        def change(c):
            a = np.ascontiguousarray(arr, (il, fl)[i].dtype)
            keep.append(a)
            c.bounds, c.n_bounds, c.bucket_ids = a.ctypes.data, a.size, None
        return change

    for i, lists in ((0, ([1, 1], [2, 1], [1, 2, 3, 3], [5, 4, 3])), (1, ([1.0, 1.0], [2.0, 1.0], [-0.0, 0.0], [0.0, -0.0], [np.nan, 1.0], [1.0, np.nan],
                                                                      [-np.nan, 1.0], [np.inf, -np.inf]))):
        for arr in lists:
            batch = fresh()
            bounds_of(i, arr)(batch._arr[i])
            refused(batch, N.SB_ERR_INVALID, "bounds %r" % (arr,))
    # the ids the call hands out
    for w, bad in ((1, 255), (1, 256), (2, 65535), (2, 1 << 20)):
        for i in (0, 1):
            batch = fresh(id_width=w)
            ids = np.arange(len((il, fl)[i]) + 1, dtype=np.uint32)
            ids[2] = bad
            batch._arr[i].bucket_ids = ids.ctypes.data
            refused(batch, N.SB_ERR_INVALID, "bucket id %d at id_width %d" % (bad, w))
        batch = fresh(id_width=w)
        batch._arr[1].nan_id = bad
        refused(batch, N.SB_ERR_INVALID, "nan_id %d at id_width %d" % (bad, w))
    for nan_id in (0, 5, 0xFFFFFFFE):
        batch = fresh(id_width=4)
        batch._arr[0].nan_id = nan_id
        refused(batch, N.SB_ERR_INVALID, "nan_id on an integer column")
    big = np.arange(300, dtype=ib.ref.vals.dtype)
    batch = _raw(gpu_ctx, [icp, icp], [big[:200], big[:200]], [bm, bm], rows, id_width=1)
    keep.append(np.ascontiguousarray(big))
    batch._arr[1].bounds, batch._arr[1].n_bounds = keep[-1].ctypes.data, 255
    refused(batch, N.SB_ERR_INVALID, "n_bounds == 255 at id_width 1, no bucket_ids")
    # the same batch, as it was built, then succeeds
    batch = fresh()
    res = batch.enqueue()
    gpu_ctx.synchronize()
    for r, b, lst, v, ids in zip(res, (ib, fb), (il, fl), bids, batch._ids):
        w = R.want(b.ref, mask, lst, v, False, None, 2)
        assert (r.rows, r.selected, r.count, r.matched, r.nans) == (w.rows, w.selected, w.count, w.matched, w.nans)
        h = ids.cpu().numpy()
        assert np.array_equal(h[:rows * 2].view(np.uint16), w.ids) and (h[rows * 2:] == GUARD).all()


# ---- 11: errors at the synchronize
def test_a_truncated_page_raises_what_the_decoder_raises(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    for name in ("route_none", "route_rle", "route_dict", "route_lz4", "f64_none", "f64_rle", "f64_dict", "f64_patas"):
        b = Bc.build(name)
        m = np.array(b.metas, np.uint64).copy()
        cut = int(m[-1, 0]) // 2
        m[-1, 0] -= cut
        bad = b.pages[:b.pages.size - cut].copy()
        cp = upload(gpu_ctx, b.col, bad, m)
        want = read_code(gpu_ctx, cp)
        oc = oracle_code(b.col, bad, m)
        assert want != 0 and oc != 0 and (oc is None or oc == want), (name, want, oc)
        sel = three_masks(b.rows, 12)[1]
        for mask in (sel, None):
            res = sb.key_buckets(gpu_ctx, [cp], [default_bounds(b, 100)], selection=bitmap(gpu_ctx, mask))
            with pytest.raises(NativeError) as e:
                gpu_ctx.synchronize()
            assert e.value.code == want, name
            # rows and selected are delivered even when the interval failed
            assert res[0].rows == b.rows and res[0].selected == (b.rows if mask is None else int(sel.sum()))
    # the context still works
    sweep(gpu_ctx, "f64_dict")


def test_a_float32_patas_page_fails_with_the_decoders_code(gpu_ctx):
    """the oracle writes no Float32 Patas page; a Float64 Patas page read as Float32 is one to the decoder"""
    import strawboat_amd as sb
    from strawboat_amd import read
    from strawboat_amd._native import NativeError
    b = Bc.build("f64_patas")
    col = dict(b.col, ptype=S.T_F32)
    cp = read.ColumnPages(S.T_F32, col["nullable"], to_dev(gpu_ctx, b.pages), b.metas)
    want = read_code(gpu_ctx, cp)
    assert want != 0
    res = sb.key_buckets(gpu_ctx, [cp], [np.array([0.0], np.float32)])
    with pytest.raises(NativeError) as e:
        gpu_ctx.synchronize()
    assert e.value.code == want and res[0].rows == b.rows and res[0].selected == b.rows
