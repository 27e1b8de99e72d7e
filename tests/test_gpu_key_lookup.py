"""sb_key_lookup on the GPU: the ids a given list assigns to the rows of a key column, compared BYTE FOR BYTE, with rows /
selected / count / matched, against tests/key_lookup_ref.py over the ORACLE's decode of the pages (the reference is checked
on its own against a dict-based lookup in tests/test_key_lookup_host.py).  Nothing here is compared with what the device's
own decoder gives.

Every column comes from tests/key_lookup_cases.py (build(name) asserts the codec of every page; the host test walks the
whole table).  Unless a test says otherwise a column runs with no selection, with every 7th row selected and under a mask
that leaves whole tiles of 4096 rows unselected.  Null rows keep their stored bytes in the pages, and the default list is
drawn from ALL the values the oracle decodes, so a null row whose stored bytes are in the list is in every case with nulls.

The identities of section 8 need no reference: key_lookup against a column's own keys writes key_ids' bytes, halves of a
column against one list give the halves of the whole, and the count / sum records of group_by_keys on the halves add up."""
import os

import numpy as np
import pytest

from oracle import sbo as S
from tests import key_lookup_cases as Kc
from tests import key_lookup_ref as L
from tests.test_gpu_aggregate import bitmap
from tests.test_gpu_read_selected import oracle_code, read_code, to_dev, upload

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_BYTES = 4096
WORD = 0x5A5A5A5A5A5A5A5A
RESULTS = ("rows", "selected", "count", "matched")
TILE = 4096


def three_masks(rows, seed=0):
    """no selection, every 7th row, and a mask that leaves whole tiles unselected (every second tile, the first among them)"""
    r = np.arange(rows)
    tiles = ((r // TILE) % 2 == 1) & (np.random.default_rng(seed).random(rows) < 0.5)
    return [None, r % 7 == 0, tiles]


def default_list(b, seed=0, limit=1024):
    """every other distinct value of the column (null rows' stored values too), so that values between the entries are
    missing; values below and above all of them that the column does not hold; one entry twice; in a random order"""
    rng = np.random.default_rng(seed)
    if b.binary:
        have = sorted(set(b.ref.strs.tolist()))
        lst = have[::2][:limit - 4] + [b"\x00\x00nope", b"\xff\xff\xffnope", b"abcdefg\x00"]
    else:
        info = np.iinfo(b.ref.vals.dtype)
        have = np.unique(b.ref.vals[:b.rows]).tolist()
        lst = have[::2][:limit - 4] + [v for v in (info.min, info.max) if v not in have]
    if lst:
        lst.append(lst[0])
    lst = [lst[i] for i in rng.permutation(len(lst))]
    return lst if b.binary else np.array(lst, b.ref.vals.dtype)


def run(ctx, builts, lists, vids=None, masks=None, widths=None, what="", cps=None):
    """the columns of ONE call, each with its own list, value ids, selection and id_width (None: the narrowest)"""
    import strawboat_amd as sb
    n = len(builts)
    vids = [None] * n if vids is None else vids
    masks = [None] * n if masks is None else masks
    widths = [None] * n if widths is None else widths
    cps = [upload(ctx, b.col, b.pages, b.metas) for b in builts] if cps is None else cps
    res = sb.key_lookup(ctx, cps, lists, None if all(v is None for v in vids) else vids, [bitmap(ctx, m) for m in masks], list(widths))
    ctx.synchronize()
    for i, (r, b) in enumerate(zip(res, builts)):
        L.check(r, L.want(b.ref, masks[i], lists[i], vids[i], r.id_width), "%s column %d (id_width %d)" % (what, i, r.id_width))
    return res


def sweep(ctx, name, seed=0):
    """one column under its three masks x the three widths, position ids and many-to-one ids: two calls of nine columns"""
    b = Kc.build(name)
    lst = default_list(b, seed)
    masks = three_masks(b.rows, seed)
    cp = upload(ctx, b.col, b.pages, b.metas)
    combos = [(m, w) for m in masks for w in (1, 2, 4)]
    # (ids of one byte name at most 255 positions)
    lists = [lst[:200] if w == 1 else lst for _, w in combos]
    res = run(ctx, [b] * 9, lists, None, [m for m, _ in combos], [w for _, w in combos], name, cps=[cp] * 9)
    vids = [[(i * 7) % 5 for i in range(len(lx))] for lx in lists]
    run(ctx, [b] * 9, lists, vids, [m for m, _ in combos], [w for _, w in combos], name + ", many to one", cps=[cp] * 9)
    if b.rows > 300 and "onevalue" not in name:   # the cases are shaped so that the list knows some live rows and misses others
        assert 0 < res[2].matched < res[2].count, (name, res[2].matched, res[2].count)
    return res


# ---- 1: the codec routes of numeric columns
NUM_ROUTES = [n for n in Kc.CASES if n.startswith("route_") and "freq" not in n] + ["dict_8192", "dict_8193"] + \
    [n for n in Kc.CASES if n.startswith("rle_hand_")]


@pytest.mark.parametrize("name", NUM_ROUTES)
def test_numeric_codec_routes(gpu_ctx, name):
    sweep(gpu_ctx, name, seed=len(name))


def test_rle_long_page_in_parts(gpu_ctx):
    b = Kc.build("rle_long")
    lst = default_list(b, 3)
    masks = three_masks(b.rows, 3)
    run(gpu_ctx, [b] * 3, [lst] * 3, None, masks, [2, 4, 2], "long RLE page")


@pytest.mark.parametrize("t", ["i32", "i64", "u8"])
def test_freq_pages_are_the_replay_and_equal_plain_pages(gpu_ctx, t):
    f, p = Kc.build("route_freq_" + t), Kc.build("freq_plain_" + t)
    lst = default_list(f, 5, limit=200)
    masks = three_masks(f.rows, 5)
    for _ in range(2):   # ... and the same column again in the next interval
        r0 = gpu_ctx.replays()
        got = run(gpu_ctx, [f] * 3, [lst] * 3, None, masks, [1, 2, 4], "freq " + t)
        assert gpu_ctx.replays() == r0 + 1
    r0 = gpu_ctx.replays()
    plain = run(gpu_ctx, [p] * 3, [lst] * 3, None, masks, [1, 2, 4], "plain pages of the same values")
    assert gpu_ctx.replays() == r0
    for a, c in zip(got, plain):
        assert a.ids.cpu().numpy().tobytes() == c.ids.cpu().numpy().tobytes() and (a.count, a.matched) == (c.count, c.matched)


# ---- 2: all eight integer types, with the extremes of the signedness in the list
@pytest.mark.parametrize("t", list(Kc.TYPE_NAME.values()))
def test_integer_types_and_the_extremes_of_the_signedness(gpu_ctx, t):
    for codec in ("none", "rle", "dict"):
        b = Kc.build("type_%s_%s" % (t, codec))
        info = np.iinfo(b.ref.vals.dtype)
        have = np.unique(b.ref.vals[:b.rows]).tolist()
        # in the order of the signedness info.min is the first key and info.max the last; -1 / 0 / 1 sit at the sign's seam
        lst = np.array([info.max, info.min, 0, 1] + ([-1] if info.min < 0 else [info.max - 1]) + have[1::3], b.ref.vals.dtype)
        masks = three_masks(b.rows, 1)
        run(gpu_ctx, [b] * 3, [lst] * 3, None, masks, [1, 2, 4], "type %s %s" % (t, codec))


# ---- 3: the codec routes of binary columns
BIN_ROUTES = [n for n in Kc.CASES if n.split("_")[0] in ("bin", "large") and n.split("_")[1] in ("none", "lz4", "dict", "freq", "onevalue")]
assert "bin_dict_8192" in BIN_ROUTES and "bin_dict_8193" in BIN_ROUTES and "large_freq" in BIN_ROUTES


@pytest.mark.parametrize("name", BIN_ROUTES)
def test_binary_codec_routes(gpu_ctx, name):
    r0 = gpu_ctx.replays()
    sweep(gpu_ctx, name, seed=len(name))
    assert gpu_ctx.replays() == r0   # (a binary Freq page is a virtual Dict page: no replay)


# ---- 4: row counts
@pytest.mark.parametrize("pages", [2, 9])
def test_row_counts(gpu_ctx, pages):
    bs = [Kc.build("rows_%d_%d" % (r, pages)) for r in Kc.ROW_COUNTS]
    for k, mask_of in enumerate((lambda b: None, lambda b: np.arange(b.rows) % 7 == 0, lambda b: np.arange(b.rows) >= TILE)):
        run(gpu_ctx, bs, [default_list(b, 2) for b in bs], None, [mask_of(b) for b in bs], [(1, 2, 4)[(i + k) % 3] for i in range(len(bs))],
            "row counts, %d pages" % pages)


def test_row_counts_of_strings(gpu_ctx):
    bs = [Kc.build("bin_rows_%d" % r) for r in Kc.ROW_COUNTS]
    for k, mask_of in enumerate((lambda b: None, lambda b: np.arange(b.rows) % 7 == 0, lambda b: np.arange(b.rows) >= TILE)):
        run(gpu_ctx, bs, [default_list(b, 4) for b in bs], None, [mask_of(b) for b in bs], [(1, 2, 4)[(i + k) % 3] for i in range(len(bs))],
            "row counts of strings")


def test_one_column_of_more_than_tile_grid_tiles(gpu_ctx):
    b = Kc.build("big_u8")
    assert b.rows == 4096 * 4096 + 1
    lst = np.array([199, 0, 7, 100, 255, 201], np.uint8)
    mask = three_masks(b.rows, 9)[2]
    res = run(gpu_ctx, [b, b], [lst, lst], [None, [1, 1, 0, 0, 1, 0]], [None, mask], [1, 1], "the grid's second sweep")
    assert 0 < res[0].matched < res[0].count == b.rows and 0 < res[1].selected < b.rows


# ---- 5: lists
@pytest.mark.parametrize("name", ["dict_8192", "route_none", "route_rle", "bin_dict_8192", "bin_none"])
def test_lists_of_0_1_2_3_1023_and_1024_values(gpu_ctx, name):
    b = Kc.build(name)
    full = default_list(b, 8)
    if len(full) < 1024:   # the column has fewer distinct values: the rest of the list are values it does not hold
        extra = [b"miss-%04d" % i for i in range(1024)] if b.binary else [int(v) for v in np.arange(1024) * 2 + 1_000_001]
        full = (list(full) + extra)[:1024]
        full = full if b.binary else np.array(full, b.ref.vals.dtype)
    masks = three_masks(b.rows, 8)
    for n in (0, 1, 2, 3, 1023, 1024):
        lst = full[:n]
        res = run(gpu_ctx, [b] * 3, [lst] * 3, None, masks, [2, 4, 2], "%s, %d values" % (name, n))
        if n == 0:
            assert all(r.matched == 0 for r in res) and (L.ids_numpy(res[0]) == 65535).all()


def test_duplicates_take_the_first_occurrence_and_ids_may_be_shared(gpu_ctx):
    for name in ("route_dict", "route_rle", "route_lz4", "bin_dict", "large_none"):
        b = Kc.build(name)
        have = sorted(set(b.ref.strs.tolist())) if b.binary else np.unique(b.ref.vals[:b.rows]).tolist()
        lst = [have[3], have[0], have[3], have[5], have[0], have[0], have[7]]
        vids = [9, 8, 7, 6, 5, 4, 9]   # have[3] -> 9, have[0] -> 8, have[7] -> 9 as well
        lst = lst if b.binary else np.array(lst, b.ref.vals.dtype)
        res = run(gpu_ctx, [b, b], [lst, lst], [vids, None], [None, None], [1, 1], name + ", duplicates")
        ids = L.ids_numpy(res[0])
        assert set(ids.tolist()) <= {9, 8, 6, 255} and 7 not in ids and 5 not in ids and 4 not in ids
        assert set(L.ids_numpy(res[1]).tolist()) <= {0, 1, 3, 6, 255}


def test_the_lower_bound_alone_is_no_match(gpu_ctx):
    """values between, below and above the list's entries get all ones, on every walk"""
    for name in ("route_none", "route_rle", "route_dict", "route_zstd", "route_snappy", "dict_8193", "route_bitpack_i32", "route_deltabp_u32"):
        b = Kc.build(name)
        have = np.unique(b.ref.vals[b.ref.valid]).tolist()
        assert len(have) >= 6
        lst = np.array(have[2:-2:2][:1000], b.ref.vals.dtype)   # misses below the first, above the last and between every two
        res = run(gpu_ctx, [b], [lst], None, [None], [4], name + ", misses")[0]
        ids = L.ids_numpy(res)
        for miss in (have[0], have[1], have[3], have[-1]):
            assert (ids[b.ref.valid & (b.ref.vals[:b.rows] == miss)] == 0xFFFFFFFF).all(), (name, miss)
        assert 0 < res.matched < res.count


@pytest.mark.parametrize("width,largest", [(1, 254), (2, 65534), (4, 0xFFFFFFFE)])
def test_the_largest_id_each_width_allows(gpu_ctx, width, largest):
    for name in ("route_none", "route_rle", "route_dict", "bin_none", "bin_dict"):
        b = Kc.build(name)
        have = sorted(set(b.ref.strs[b.ref.valid].tolist())) if b.binary else np.unique(b.ref.vals[b.ref.valid]).tolist()
        lst = have[:4] if b.binary else np.array(have[:4], b.ref.vals.dtype)
        res = run(gpu_ctx, [b], [lst], [[largest, 0, largest, 1]], [None], [width], "%s, id %d" % (name, largest))[0]
        assert int(L.ids_numpy(res).astype(np.uint64)[b.ref.valid].min()) == 0 and largest in L.ids_numpy(res).tolist()


def test_strings_at_the_edges_of_the_compare(gpu_ctx):
    edge = Kc.edge_strings()
    lists = [
        [b"", b"abcdefg", b"abcdefgh", b"abcdefghi", b"0123456789" * 4],          # 0, 7, 8, 9 and 40 bytes
        [b"abcdefgh" + b"q" * 32, b"abcdefgX", b"abcdefghZZ"],                     # strings sharing their first 8 bytes
        [b"abcdefgh"],                                                             # a proper prefix of other rows' strings
        [b"abcdefgh\x00", b"abcdefgh" + b"q" * 31 + b"r"],
        [b"a"],                                                                    # "a" against "a\0"
        [b"a\x00"],
        [b"a\x00\x00", b"a", b"\x00", b"\xff" * 9, b"\x80"],
        [b"abcdef", b"abcdefghij", b"b", b"\xff" * 8, b"\xff" * 10],               # near misses only: nothing matches
    ]
    for name in ("bin_none", "bin_lz4", "bin_dict", "large_none", "large_dict", "bin_freq"):
        b = Kc.build(name)
        assert set(edge) <= set(b.ref.strs[b.ref.valid].tolist())
        res = run(gpu_ctx, [b] * len(lists), lists, None, [None] * len(lists), [1] * len(lists), name + ", edges")
        assert res[-1].matched == 0 and res[4].matched == int((b.ref.strs[b.ref.valid] == b"a").sum()) > 0
        assert res[0].matched == sum(x in set(lists[0]) for x in b.ref.strs[b.ref.valid].tolist())
        # the empty string is a value: rows of it get its id
        ids = L.ids_numpy(res[0])
        assert (ids[b.ref.valid & (b.ref.strs == b"")] == 0).all() and (b.ref.valid & (b.ref.strs == b"")).any()


# ---- 6: selections and nulls
def test_a_null_row_whose_stored_bytes_are_in_the_list_gets_all_ones(gpu_ctx):
    for name in ("route_none", "route_rle", "route_dict", "bin_none", "bin_dict"):
        b = Kc.build(name)
        vals = b.ref.strs if b.binary else b.ref.vals[:b.rows]
        null_vals = set(vals[~b.ref.valid].tolist())
        assert null_vals, name
        lst = sorted(null_vals)[:50]   # what the null rows hold, as the oracle decodes them
        lst = lst if b.binary else np.array(lst, b.ref.vals.dtype)
        res = run(gpu_ctx, [b], [lst], None, [None], [1], name + ", nulls")[0]
        assert (L.ids_numpy(res)[~b.ref.valid] == 255).all() and res.count == int(b.ref.valid.sum())


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
    for name in ("route_none", "route_rle", "route_dict", "route_lz4", "rows_4097_2", "rows_8193_9", "bin_none", "bin_dict", "bin_rows_4097"):
        b = Kc.build(name)
        lst = default_list(b, 6, limit=100)
        cp = upload(gpu_ctx, b.col, b.pages, b.metas)
        for mask in three_masks(b.rows, id_width):
            ids_bytes, whole = _guarded(gpu_ctx, b.rows * id_width, id_width)
            ids = ids_bytes.view(getattr(torch, ID_DTYPES[id_width]))
            batch = sb.KeyLookupBatch(gpu_ctx, [cp], [lst], None, bitmap(gpu_ctx, mask), id_width, out=[ids])
            assert batch._arr[0].ids_capacity == b.rows * id_width
            res = batch.enqueue()
            gpu_ctx.synchronize()
            assert _guards_intact(whole, b.rows * id_width), "a byte outside ids was written"
            L.check(res[0], L.want(b.ref, mask, lst, None, id_width), name + ", between guards")


def test_pages_at_odd_byte_offsets_and_scattered_page_offsets(gpu_ctx):
    import torch
    from strawboat_amd import read
    for name in ("route_none", "route_rle", "route_dict", "route_lz4", "bin_none", "bin_dict", "bin_lz4"):
        b = Kc.build(name)
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
        lst = default_list(b, 7, limit=200)
        for mask in three_masks(b.rows, 7):
            run(gpu_ctx, [b] * 4, [lst] * 4, None, [mask] * 4, [1, 2, 4, 1], name + ", offsets", cps=cps)


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


@pytest.mark.parametrize("name", ["route_none", "route_rle", "route_dict", "route_zstd", "type_u8_dict", "type_i16_rle", "bin_none", "bin_dict",
                                  "large_lz4", "bin_freq"])
def test_lookup_of_a_columns_own_keys_writes_the_bytes_of_key_ids(gpu_ctx, name):
    import strawboat_amd as sb
    b = Kc.build(name)
    whole, first, rest, rows0 = _halves(gpu_ctx, b)
    for mask in three_masks(b.rows, 2):
        bm = bitmap(gpu_ctx, mask)
        kid = (sb.key_ids_var if b.binary else sb.key_ids)(gpu_ctx, [whole], bm, max_keys=1024, id_width=2)[0]
        gpu_ctx.synchronize()
        assert not kid.overflow
        # a finished KeyIds / KeyIdsVar is a list: its keys, sorted, so a value's position is key_ids' id
        look = sb.key_lookup(gpu_ctx, [whole], [kid], selection=bm, id_width=2)[0]
        gpu_ctx.synchronize()
        want = kid.ids.cpu().numpy().tobytes()
        assert look.ids.cpu().numpy().tobytes() == want, name
        assert (look.rows, look.selected, look.count, look.matched) == (kid.rows, kid.selected, kid.count, kid.count)
        if b.binary:   # ... and through as_in_list()
            again = sb.key_lookup(gpu_ctx, [whole], [kid.as_in_list()], selection=bm, id_width=2)[0]
            gpu_ctx.synchronize()
            assert again.ids.cpu().numpy().tobytes() == want
        # the two halves of the pages against the whole column's keys: the two halves of the whole column's ids
        m0, m1 = (None, None) if mask is None else (mask[:rows0], mask[rows0:])
        parts = sb.key_lookup(gpu_ctx, [first, rest], [kid, kid], selection=[bitmap(gpu_ctx, m0), bitmap(gpu_ctx, m1)], id_width=2)
        gpu_ctx.synchronize()
        assert parts[0].ids.cpu().numpy().tobytes() + parts[1].ids.cpu().numpy().tobytes() == want, name
        assert parts[0].count + parts[1].count == kid.count and parts[0].rows == rows0


@pytest.mark.parametrize("name,n_keys", [("route_dict", 60), ("route_rle", 60), ("bin_dict", None), ("keys_700_dict", 700)])
def test_group_records_of_the_halves_add_up_to_group_by_on_the_whole(gpu_ctx, name, n_keys):
    """integer count / sum records are index-aligned under one list: adding them is the merge"""
    import strawboat_amd as sb
    b = Kc.build(name)
    whole, first, rest, rows0 = _halves(gpu_ctx, b)
    rng = np.random.default_rng(3)
    y = Kc.ints(S.T_I64, rng.integers(-10 ** 12, 10 ** 12, b.rows), rng.random(b.rows) >= 0.1)
    from tests import gen
    # the value column, whole and in the two parts of the key column's rows
    ys = []
    for lo, hi in ((0, b.rows), (0, rows0), (rows0, b.rows)):
        part = Kc.ints(S.T_I64, y["values"][lo:hi], np.unpackbits(y["validity"], bitorder="little")[lo:hi].astype(bool))
        pg, mt = gen.oracle_write(part, max_page_size=3000, force_codec=S.NONE)
        ys.append(upload(gpu_ctx, part, pg, mt))
    mask = rng.random(b.rows) < 0.6
    max_keys = 1024 if n_keys is None or n_keys > 256 else 256   # (more than 256 groups: the large aggregate)
    kres, aggs = sb.group_by(gpu_ctx, whole, [ys[0]], bitmap(gpu_ctx, mask), ops=("count", "sum"), max_keys=max_keys)
    gpu_ctx.synchronize()
    assert not kres.overflow and kres.n_keys > 3
    keys = kres.keys
    halves = []
    for cp, ycp, m in ((first, ys[1], mask[:rows0]), (rest, ys[2], mask[rows0:])):
        look, agg = sb.group_by_keys(gpu_ctx, cp, keys, [ycp], bitmap(gpu_ctx, m), ops=("count", "sum"))
        gpu_ctx.synchronize()
        halves.append((look, agg[0]))
    assert halves[0][0].matched + halves[1][0].matched == kres.count
    for g in range(kres.n_keys):
        a, h0, h1 = aggs[0][g], halves[0][1][g], halves[1][1][g]
        assert (h0.selected + h1.selected, h0.count + h1.count, h0.sum + h1.sum) == (a.selected, a.count, a.sum), (name, g)
    assert halves[0][1].out_of_range + halves[1][1].out_of_range == aggs[0].out_of_range


def test_the_same_call_twice_gives_the_same_bytes(gpu_ctx):
    import strawboat_amd as sb
    names = ["route_none", "route_rle", "route_dict", "route_lz4", "route_onevalue", "route_bitpack_i32", "rle_hand_i16", "bin_none", "bin_dict",
             "large_lz4", "bin_freq", "bin_onevalue"]
    bs = [Kc.build(n) for n in names]
    cps = [upload(gpu_ctx, b.col, b.pages, b.metas) for b in bs]
    lists = [default_list(b, 11) for b in bs]
    masks = [three_masks(b.rows, i)[i % 3] for i, b in enumerate(bs)]
    batch = sb.KeyLookupBatch(gpu_ctx, cps, lists, None, [bitmap(gpu_ctx, m) for m in masks], [(1, 2, 4)[i % 3] if len(lists[i]) < 255 else 2 for i in range(len(bs))])
    seen = []
    for _ in range(4):   # fresh intervals
        res = batch.enqueue()
        gpu_ctx.synchronize()
        seen.append([(r.ids.cpu().numpy().tobytes(), r.rows, r.selected, r.count, r.matched) for r in res])
    assert all(s == seen[0] for s in seen[1:])
    for i, (r, b) in enumerate(zip(res, bs)):
        L.check(r, L.want(b.ref, masks[i], lists[i], None, r.id_width), names[i] + ", again")


# ---- 9: intervals
def test_filter_then_key_lookup_then_grouped_aggregates_in_one_interval(gpu_ctx):
    import strawboat_amd as sb
    from tests import gen
    from tests.aggregate_ref import reduce_values
    kb = Kc.build("dict_8192")
    xcol = gen.prim(S.T_I32, kb.rows, uniq=100, null_density=0.2, runs=4, seed=1)
    xp, xm = gen.oracle_write(xcol, max_page_size=2050, force_codec=S.RLE)
    xr = L.Ref(xcol, xp, xm)
    ycol = gen.prim(S.T_I64, kb.rows, uniq=5000, null_density=0.1, seed=2)
    yp, ym = gen.oracle_write(ycol, max_page_size=4100, force_codec=S.NONE)
    yr = L.Ref(ycol, yp, ym)
    mask = (xr.vals[:kb.rows] < 60) & xr.valid
    have = np.unique(kb.ref.vals[kb.ref.valid])
    for n_groups, call in ((40, sb.aggregate_grouped), (1000, sb.aggregate_grouped_large)):
        lst = have[::5][:n_groups][::-1].copy()                   # the list in descending order: the ids are the list's, not ranks
        sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, xcol, xp, xm)], [sb.Predicate("lt", 60)])
        look = sb.key_lookup(gpu_ctx, [upload(gpu_ctx, kb.col, kb.pages, kb.metas)], [lst], selection=sel[0])[0]
        agg = call(gpu_ctx, [upload(gpu_ctx, ycol, yp, ym)], look.ids, n_groups, sel[0])[0]
        gpu_ctx.synchronize()   # (the only one)
        assert np.array_equal(sel[0].numpy(), mask)
        L.check(look, L.want(kb.ref, mask, lst, None, look.id_width), "behind the filter")
        live = mask & kb.ref.valid
        in_list = np.isin(kb.ref.vals[:kb.rows], lst)
        assert look.matched == int((live & in_list).sum()) and agg.out_of_range == int((mask & ~(kb.ref.valid & in_list)).sum())
        for g in (0, 1, n_groups // 2, n_groups - 1):
            in_group = live & (kb.ref.vals[:kb.rows] == lst[g])
            w = reduce_values(S.T_I64, yr.vals, in_group & yr.valid, int(in_group.sum()))
            assert (agg[g].selected, agg[g].count) == (int(in_group.sum()), w.count), g
            if w.count:
                assert agg[g].sum == int(yr.vals[:kb.rows][in_group & yr.valid].astype(object).sum()), g


def test_key_lookup_ids_as_a_part_of_key_combine(gpu_ctx):
    import strawboat_amd as sb
    a, s = Kc.build("route_dict"), Kc.build("bin_dict")
    assert a.rows == s.rows
    la, ls = default_list(a, 1, limit=30), default_list(s, 1, limit=30)
    mask = three_masks(a.rows, 4)[1]
    bm = bitmap(gpu_ctx, mask)
    look = sb.key_lookup(gpu_ctx, [upload(gpu_ctx, a.col, a.pages, a.metas), upload(gpu_ctx, s.col, s.pages, s.metas)], [la, ls], selection=bm)
    comb = sb.key_combine(gpu_ctx, [(look[0].ids, len(la)), (look[1].ids, len(ls))], max_keys=1024)
    gpu_ctx.synchronize()
    wa, ws = L.want(a.ref, mask, la, None, look[0].id_width), L.want(s.ref, mask, ls, None, look[1].id_width)
    L.check(look[0], wa, "part 0")
    L.check(look[1], ws, "part 1")
    both = (wa.ids != 255) & (ws.ids != 255)
    tuples = sorted(set(zip(wa.ids[both].tolist(), ws.ids[both].tolist())))
    assert not comb.overflow and comb.live == int(both.sum()) and [tuple(t) for t in comb.tuples.tolist()] == tuples
    cid = comb.ids.cpu().numpy().view(L.ID_NP[comb.id_width])
    place = {t: i for i, t in enumerate(tuples)}
    want = np.array([place[(x, y)] if ok else (1 << (8 * comb.id_width)) - 1 for x, y, ok in zip(wa.ids.tolist(), ws.ids.tolist(), both.tolist())])
    assert np.array_equal(cid, want)


def test_inside_an_interval_that_another_call_causes_to_be_replayed(gpu_ctx):
    import strawboat_amd as sb
    x = Kc.build("route_freq_i32")
    names = ["route_none", "route_rle", "route_dict", "route_lz4", "bin_none", "bin_dict", "bin_freq"]
    bs = [Kc.build(n) for n in names]
    lists = [default_list(b, 2, limit=100) for b in bs]
    masks = [three_masks(b.rows, 2)[i % 3] for i, b in enumerate(bs)]
    cps = [upload(gpu_ctx, b.col, b.pages, b.metas) for b in bs]
    r0 = gpu_ctx.replays()
    sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x.col, x.pages, x.metas)], [sb.Predicate("ne", 7)])
    res = sb.key_lookup(gpu_ctx, cps, lists, selection=[bitmap(gpu_ctx, m) for m in masks], id_width=[1, 2, 4, 1, 2, 4, 1])
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    for i, (r, b) in enumerate(zip(res, bs)):
        L.check(r, L.want(b.ref, masks[i], lists[i], None, r.id_width), names[i] + ", in a replayed interval")


def test_numeric_and_binary_columns_with_different_widths_in_one_call(gpu_ctx):
    names = ["route_none", "bin_dict", "type_u8_rle", "large_none", "route_onevalue", "bin_onevalue", "type_i16_dict", "bin_lz4",
             "route_freq_i64", "large_freq"]
    bs = [Kc.build(n) for n in names]
    lists = [default_list(b, 3, limit=150) for b in bs]
    masks = [three_masks(b.rows, 3)[i % 3] for i, b in enumerate(bs)]
    widths = [1, 4, 2, 1, 4, 2, 1, 2, 4, 1]
    r0 = gpu_ctx.replays()
    run(gpu_ctx, bs, lists, None, masks, widths, "mixed")
    assert gpu_ctx.replays() == r0 + 1   # (the numeric Freq column; the binary columns of the call stay on their pages)
    run(gpu_ctx, bs[::-1], lists[::-1], None, masks[::-1], widths, "mixed, the columns turned round")


def test_on_a_context_that_holds_launch_hints(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd import read
    from tests import gen
    ctx = sb.Context(0)
    try:
        rle, plain, strs = Kc.build("rle_long"), Kc.build("route_none"), Kc.build("bin_dict")
        cp = upload(ctx, rle.col, rle.pages, rle.metas)
        for _ in range(3):   # the hints now say: RLE pages alone, no tiles
            read.read_simple(ctx, cp)
        r0 = ctx.replays()
        # columns of tiles: a read call would be issued again for them; this call goes by no hint
        bs = [rle, plain, strs]
        run(ctx, bs, [default_list(b, 1) for b in bs], None, [three_masks(b.rows, 1)[1] for b in bs], [2, 1, 4], "behind reads")
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
def _raw(ctx, cps, lists, bitmaps, rows, id_width=2, vids=None):
    import torch
    import strawboat_amd as sb
    batch = sb.KeyLookupBatch(ctx, cps, lists, vids, bitmaps, id_width)
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
    nb, sb_ = Kc.build("route_none"), Kc.build("bin_none")
    rows = nb.rows
    assert sb_.rows == rows
    ncp, scp = upload(gpu_ctx, nb.col, nb.pages, nb.metas), upload(gpu_ctx, sb_.col, sb_.pages, sb_.metas)
    mask = three_masks(rows, 9)[1]
    bm = bitmap(gpu_ctx, mask)
    nl, sl = default_list(nb, 9, limit=50), default_list(sb_, 9, limit=50)
    vids = [list(range(len(nl))), list(range(len(sl)))]

    def fresh(**kw):
        return _raw(gpu_ctx, [ncp, scp], [nl, sl], [bm, bm], rows, vids=vids, **kw)

    def refused(batch, code, what, mem=N.SB_MEM_DEVICE):
        assert gpu_ctx._lib.sb_key_lookup(gpu_ctx._h, batch._arr, 2, mem) == code, what
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
    for ptype in (S.T_F32, S.T_F64, S.T_BOOL, S.T_I128, S.T_I256, S.T_NULL):
        each(lambda c, ptype=ptype: setattr(c, "physical_type", ptype), N.SB_ERR_NYI, "type %d" % ptype)
    batch = fresh()
    refused(batch, N.SB_ERR_NYI, "SB_MEM_HOST", mem=N.SB_MEM_HOST)
    # the list
    each(lambda c: setattr(c, "n_values", 1025), N.SB_ERR_INVALID, "n_values above SB_KEY_MAX_KEYS")
    each(lambda c: setattr(c, "values", None), N.SB_ERR_INVALID, "values null")
    batch = fresh()
    batch._arr[0].value_offsets = batch._arr[1].value_offsets
    refused(batch, N.SB_ERR_INVALID, "value_offsets on a numeric column")
    batch = fresh()
    batch._arr[1].value_offsets = None
    refused(batch, N.SB_ERR_INVALID, "value_offsets null on a binary column")
    offs = np.zeros(len(sl) + 1, np.uint64)
    offs[1:] = np.cumsum([len(s) for s in sl])
    for what, change in (("value_offsets[0] != 0", lambda o: o.__setitem__(0, 1)), ("value_offsets descend", lambda o: o.__setitem__(3, int(o[2]) - 1)),
                         ("more than 2^30 bytes of values", lambda o: o.__setitem__(len(sl), (1 << 30) + 1))):
        o = offs.copy()
        if what == "value_offsets descend":
            o[2] = max(int(o[2]), 1)
        change(o)
        batch = fresh()
        batch._arr[1].value_offsets = o.ctypes.data
        refused(batch, N.SB_ERR_INVALID, what)
    # the ids the list hands out
    for w, bad in ((1, 255), (1, 256), (2, 65535), (2, 1 << 20), (4, 0xFFFFFFFF)):
        for i in (0, 1):
            batch = fresh(id_width=w)
            ids = np.arange(len((nl, sl)[i]), dtype=np.uint32)
            ids[2] = bad
            batch._arr[i].value_ids = ids.ctypes.data
            refused(batch, N.SB_ERR_INVALID, "value id %d at id_width %d" % (bad, w))
    big = np.arange(300, dtype=nb.ref.vals.dtype)
    batch = _raw(gpu_ctx, [ncp, ncp], [big[:200], big[:200]], [bm, bm], rows, id_width=1)
    batch._keepalive = np.ascontiguousarray(big)
    batch._arr[1].values, batch._arr[1].n_values = batch._keepalive.ctypes.data, 256
    refused(batch, N.SB_ERR_INVALID, "n_values - 1 == 255 at id_width 1, no value_ids")
    # the same batch, as it was built, then succeeds
    batch = fresh()
    res = batch.enqueue()
    gpu_ctx.synchronize()
    for r, b, lst, v, ids in zip(res, (nb, sb_), (nl, sl), vids, batch._ids):
        w = L.want(b.ref, mask, lst, v, 2)
        assert (r.rows, r.selected, r.count, r.matched) == (w.rows, w.selected, w.count, w.matched)
        h = ids.cpu().numpy()
        assert np.array_equal(h[:rows * 2].view(np.uint16), w.ids) and (h[rows * 2:] == GUARD).all()


def test_binary_page_limits_are_refused(gpu_ctx):
    """the page and row limits of sb_key_ids_var: a binary page of more than 2^26 rows (by its meta alone)"""
    import strawboat_amd as sb
    from strawboat_amd import _native as N
    b = Kc.build("bin_rows_65")
    cp = upload(gpu_ctx, b.col, b.pages, b.metas)
    batch = sb.KeyLookupBatch(gpu_ctx, [cp], [default_list(b)], None, None, 2)
    metas = (N.PageMetaC * 1)()
    metas[0].length, metas[0].num_values = int(b.metas[0, 0]), (1 << 26) + 1
    c = batch._arr[0]
    c.metas, c.n_pages = metas, 1
    c.ids_capacity = ((1 << 26) + 1) * 2   # (nothing is written: the call is refused)
    for f in RESULTS:
        setattr(c, f, WORD)
    assert gpu_ctx._lib.sb_key_lookup(gpu_ctx._h, batch._arr, 1, N.SB_MEM_DEVICE) == N.SB_ERR_NYI
    gpu_ctx.synchronize()
    assert all(getattr(c, f) == WORD for f in RESULTS)


# ---- 11: errors at the synchronize
def test_a_truncated_page_raises_what_the_decoder_raises(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    for name in ("route_none", "route_rle", "route_dict", "route_lz4", "bin_none", "bin_dict"):
        b = Kc.build(name)
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
            res = sb.key_lookup(gpu_ctx, [cp], [default_list(b, 1, limit=100)], selection=bitmap(gpu_ctx, mask))
            with pytest.raises(NativeError) as e:
                gpu_ctx.synchronize()
            assert e.value.code == want, name
            # rows and selected are delivered even when the interval failed
            assert res[0].rows == b.rows and res[0].selected == (b.rows if mask is None else int(sel.sum()))
    # the context still works
    sweep(gpu_ctx, "route_dict")
