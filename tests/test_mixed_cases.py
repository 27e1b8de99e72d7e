"""The table of the mixed columns (tests/mixed_cases.py) against the CPU oracle alone: it says what it claims.

  * S.stat_column finds exactly the planned (codec, index codec) page by page and `metas` the planned rows; the oracle's
    decode of the stitched pages equals the concatenated inputs,
  * the structure each plan promises: every ordered pair of routes adjacent at a seam that is no multiple of 32 (`pairs`),
    the chunk borders at tiles 16 and 32 inside and right behind an RLE page and an RLE page of two chunks of runs (`tiles`),
    pages of whole words (`aligned`), four codecs chosen by the writer itself (`adaptive`), disjoint value ranges of
    neighbouring pages and at most 1024 distinct values,
  * the inputs can show a fault: the random selection holds a valid selected row on both sides of every seam, the word of
    every unaligned seam holds a 0 and a 1 on each side of two rows or more under `ne median`, and a float column's sum
    differs between the slot order and the row order,
  * the references of every sink kind can be computed under every selection and are not trivial.

About `ne`: the pages' value ranges are disjoint, so an ordering against ONE literal gives every valid row of a page the
same answer -- no column of this layout can mix the bits of `lt` .. `ge` within a page.  `ne median` is 1 on every valid row
but the median's own, and the table puts a null and a valid row on each side of every seam word.

tests/test_gpu_mixed_columns.py sends the same columns through the device."""
import struct

import numpy as np
import pytest

from oracle import sbo as S
from tests import mixed_cases as M

KEY_IDS = [M.key_id(k) for k in M.KEYS]
NUMERIC = [k for k in M.KEYS if not M.is_binary(k)]
BINARY = [k for k in M.KEYS if M.is_binary(k)]
INTS = [k for k in NUMERIC if k[1] not in M.FLOATS]
ids_of = lambda keys: [M.key_id(k) for k in keys]


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _valid(col):
    return np.unpackbits(col["validity"], bitorder="little")[:col["rows"]].astype(bool)


def test_long_rle_rows_is_the_suites_shape():
    from tests.test_gpu_decode import LONG_RLE_ROWS
    assert M.LONG_RLE_ROWS == LONG_RLE_ROWS and LONG_RLE_ROWS > 64 * M.TILE_ROWS


def test_the_table_holds_every_plan_it_is_meant_to():
    names = {}
    for plan, ptype in M.KEYS:
        names.setdefault(plan, set()).add(ptype)
    assert names["pairs"] == {S.T_I32, S.T_U32, S.T_I64, S.T_F64, S.T_F32, S.T_U16, S.T_I8, S.T_BIN32, S.T_BIN64}
    assert names["tiles"] == {S.T_I32, S.T_I64, S.T_F64, S.T_BIN32}
    assert names["aligned"] == {S.T_I32, S.T_F64}
    assert names["adaptive"] == {S.T_I32, S.T_F64, S.T_BIN32}
    for plan in ("pairs_freq_mid", "pairs_freq_last", "tiles_freq_mid", "tiles_freq_last"):
        assert names[plan] == {S.T_I32, S.T_I64}
    assert len(set(KEY_IDS)) == len(KEY_IDS)


# ---------------------------------------------------------------- 1, 2: the pages are the plan, and decode to the inputs
@pytest.mark.parametrize("key", M.KEYS, ids=KEY_IDS)
def test_pages_are_the_plan_and_decode_to_the_inputs(key):
    col, pages, metas = M.stitched(key)
    plan, found = M.plan_of(key), M.page_codecs(key)
    print("%s: %s" % (M.key_id(key), M.sequence(key)))
    if plan is not None:
        assert len(found) == len(plan) == metas.shape[0]
        for p, (s, (codec, inner)) in enumerate(zip(plan, found)):
            assert codec == s.codec, "page %d: codec %d, planned %d" % (p, codec, s.codec)
            if s.icodec is not None:
                assert inner == s.icodec, "page %d: index codec %d, planned %d" % (p, inner, s.icodec)
        assert [int(n) for n in metas[:, 1]] == [s.rows for s in plan]
    assert int(metas[:, 0].sum()) == pages.size and int(metas[:, 1].sum()) == col["rows"]
    ref, valid = M.ref_of(key), _valid(col)
    assert ref.rows == col["rows"] and np.array_equal(ref.valid, valid)
    if M.is_binary(key):
        # offsets and bytes: the decoded offsets run from 0 to the number of decoded bytes, and every valid row holds its
        # input's bytes (a null row's bytes are dropped by the pages of some codecs, so the offsets behind one may differ)
        want = S.read_column(col["ptype"], True, pages, metas)
        offs = np.ascontiguousarray(want["offsets"]).view(np.uint8).view(col["offsets"].dtype)[:col["rows"] + 1]
        assert offs[0] == 0 and (np.diff(offs) >= 0).all() and int(offs[-1]) == np.asarray(want["values"]).size, "offsets"
        o, d = col["offsets"].astype(np.int64), col["values"].tobytes()
        mine = [d[o[i]:o[i + 1]] for i in range(col["rows"])]
        assert [x for x, ok in zip(mine, valid) if ok] == ref.strs[valid].tolist(), "bytes where valid"
    else:
        assert ref.vals[valid].tobytes() == col["values"][valid].tobytes(), "values where valid"
    assert 0.05 < 1 - valid.mean() < 0.25


# ---------------------------------------------------------------- 3: the structure the plans promise
def _seams(key):
    return M.edges_of(key)[1:-1]


@pytest.mark.parametrize("key", [k for k in M.KEYS if k[0].startswith("pairs")], ids=lambda k: M.key_id(k))
def test_pairs_every_ordered_route_pair_at_an_unaligned_seam(key):
    rts, seams = M.routes(key), _seams(key)
    assert all(s % 32 for s in seams), "every seam of a pairs plan lies inside a selection word"
    assert any(s % 8 for s in seams)
    have = {(a, b) for a, b in zip(rts[:-1], rts[1:])}
    plain = [r for r in M.routes_of(key[1]) if r != "F"] if not M.is_binary(key) else list(M.routes_of(key[1]))
    assert {(a, b) for a in plain for b in plain} <= have, sorted({(a, b) for a in plain for b in plain} - have)
    n = len(M.routes_of(key[1]))   # (37 pages for the six routes of Int32 / UInt32, 26 for five, one Dict page more for binary)
    assert len(rts) == n * n + 1 + (1 if M.is_binary(key) else 0) + {"pairs": 0, "pairs_freq_mid": 2, "pairs_freq_last": 1}[key[0]]
    assert 2000 < M.edges_of(key)[-1] < 5000
    # every codec and index codec the type takes
    found = M.page_codecs(key)
    codecs, inner = {c for c, _ in found}, {i for c, i in found if c == S.DICT}
    if M.is_binary(key):
        assert codecs == {S.NONE, S.LZ4, S.ZSTD, S.SNAPPY, S.DICT, S.ONEVALUE, S.FREQ} and inner == set(M.DICT_INDEX_BIN)
    else:
        want = {S.NONE, S.LZ4, S.ZSTD, S.SNAPPY, S.RLE, S.DICT, S.ONEVALUE}
        want |= {S.BITPACK, S.DELTABP} if key[1] in (S.T_I32, S.T_U32) else set()
        want |= {S.PATAS} if key[1] == S.T_F64 else set()
        want |= {S.FREQ} if "freq" in key[0] else set()
        assert codecs == want and inner == set(M.DICT_INDEX_NUM)
    assert sum(s.recipe == "null" for s in M.plan_of(key)) == 1
    if "freq" in key[0]:
        at = rts.index("F")
        assert rts.count("F") == 1 and (at == len(rts) - 1 if key[0].endswith("last") else 5 < at < len(rts) - 5)


@pytest.mark.parametrize("key", [k for k in NUMERIC if k[0].startswith("tiles")], ids=lambda k: M.key_id(k))
def test_tiles_chunk_borders_and_long_pages(key):
    rts, edges = M.routes(key), M.edges_of(key)
    rows = np.diff(edges)
    allowed = {4095, 4096, 4097, 4100, 8197, 2050, 128 * 33, 1}
    assert set(rows.tolist()) <= allowed
    tiles = -(-rows // M.TILE_ROWS)
    first = np.concatenate([[0], np.cumsum(tiles)])
    assert first[-1] >= 33
    page_of = lambda t: int(np.searchsorted(first, t, side="right")) - 1
    p16, p32 = page_of(16), page_of(32)
    assert rts[p16] == "R" and first[p16] < 16 < first[p16 + 1], "the border at tile 16 falls inside an RLE page"
    assert first[p32] == 32 and rts[p32] != "R" and rts[p32 - 1] == "R", "the border at tile 32: the first tile of a page behind an RLE page"
    ref = M.ref_of(key)
    plan = M.plan_of(key)
    # an RLE page of more than 1024 runs (two RLE_CHUNKs): the values change more than 1024 times within the page
    many = [p for p, s in enumerate(plan) if s.recipe == "short_runs"]
    assert len(many) == 1 and rts[many[0]] == "R"
    a, b = edges[many[0]], edges[many[0] + 1]
    v = M.stitched(key)[0]["values"][a:b]
    assert int((v[1:] != v[:-1]).sum()) > 1024
    found = M.page_codecs(key)
    assert any(c == S.ONEVALUE and n == 4097 for (c, _), n in zip(found, rows)) and any(n == 1 for n in rows)
    assert (S.DICT, S.RLE) in found and {S.LZ4, S.ZSTD, S.SNAPPY} & {c for c, _ in found}
    null = [p for p, s in enumerate(plan) if s.recipe == "null"]
    assert len(null) == 1 and rts[null[0]] == "R" and not ref.valid[edges[null[0]]:edges[null[0] + 1]].any()
    assert ref.rows <= 140_000
    if "freq" in key[0]:
        assert rts.count("F") == 1 and (rts[-1] == "F") == key[0].endswith("last")


def test_tiles_binary_has_long_pages_on_each_route():
    key = ("tiles", S.T_BIN32)
    rows = np.diff(M.edges_of(key))
    assert set(M.routes(key)) == {"N", "D", "O", "I", "F"} and ((rows >= 4097) & (rows <= 9000)).all()


@pytest.mark.parametrize("key", [k for k in M.KEYS if k[0] == "aligned"], ids=lambda k: M.key_id(k))
def test_aligned_every_page_is_whole_words(key):
    assert all(int(n) % 32 == 0 for n in np.diff(M.edges_of(key)))
    want = {"R", "N", "I", "O", "D"} | ({"P"} if key[1] == S.T_I32 else set())
    assert set(M.routes(key)) == want


@pytest.mark.parametrize("key", [k for k in M.KEYS if k[0] == "adaptive"], ids=lambda k: M.key_id(k))
def test_adaptive_the_writer_chose_four_codecs(key):
    codecs = {c for c, _ in M.page_codecs(key)}
    assert len(codecs) >= 4, M.sequence(key)
    if not M.is_binary(key):
        assert S.FREQ not in codecs, "no replay in the adaptive columns"
    rts = M.routes(key)
    assert any(a != b for a, b in zip(rts[:-1], rts[1:]))


@pytest.mark.parametrize("key", [k for k in M.KEYS if k[0] != "adaptive"], ids=lambda k: M.key_id(k))
def test_neighbouring_pages_hold_disjoint_values(key):
    ref, edges = M.ref_of(key), M.edges_of(key)
    vals = ref.strs if M.is_binary(key) else ref.vals
    prev = None
    for p, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        v = vals[a:b][ref.valid[a:b]]
        if M.is_binary(key):
            mine = set(v.tolist()) - {b""}
            assert all(s.startswith(b"p%02d:" % p) for s in mine), p
        elif v.size:
            lo, hi = v.min().item(), v.max().item()
            if prev is not None:
                assert lo > prev, "page %d: [%r, %r] does not lie above %r" % (p, lo, hi, prev)
            prev = hi
    if M.is_binary(key):
        assert b"" in set(vals[ref.valid].tolist()), "empty strings among the values"


@pytest.mark.parametrize("key", INTS + BINARY, ids=ids_of(INTS + BINARY))
def test_at_most_1024_distinct_values(key):
    ref = M.ref_of(key)
    vals = ref.strs if M.is_binary(key) else ref.vals
    n = len(set(vals[ref.valid].tolist()))
    if key == ("adaptive", S.T_BIN32):   # (its None pages hold a string of their own per row: key_ids_var overflows, as its reference says)
        assert n > M.MAX_KEYS
    else:
        assert 4 < n <= M.MAX_KEYS


# ---------------------------------------------------------------- 4: the inputs can show a fault
@pytest.mark.parametrize("key", M.KEYS, ids=KEY_IDS)
def test_selections_are_what_they_claim(key):
    ref, edges = M.ref_of(key), M.edges_of(key)
    rand, sparse, none, seams = M.masks(key)
    assert none is None
    for m in (rand, sparse, seams):
        assert m.size == ref.rows and not m.flags.writeable
    assert 0 < rand.sum() < ref.rows and 0.3 < rand.mean() < 0.45
    assert sparse[-1] and sparse.sum() <= 71
    hit = {int(np.searchsorted(edges, r, side="right")) - 1 for r in np.flatnonzero(sparse)}
    assert len(hit) < len(edges) - 1, "the sparse selection leaves whole pages out"
    if ref.rows > 3 * M.TILE_ROWS:
        assert len({int(r) // M.TILE_ROWS for r in np.flatnonzero(sparse)}) < ref.rows // M.TILE_ROWS, "... and whole tiles"
    want = np.zeros(ref.rows, bool)
    want[edges[:-1]] = want[edges[1:] - 1] = True
    assert np.array_equal(seams, want)
    # a valid selected row on both sides of every seam (a page without a valid row has none to give)
    live = rand & ref.valid
    for a, b in zip(edges[:-1], edges[1:]):
        assert live[a:b].any() == ref.valid[a:b].any()
    assert sum(not ref.valid[a:b].any() for a, b in zip(edges[:-1], edges[1:])) <= 1


@pytest.mark.parametrize("key", NUMERIC, ids=ids_of(NUMERIC))
def test_seam_words_hold_both_bits_on_both_sides(key):
    from tests.test_gpu_filter import expected
    col = M.stitched(key)[0]
    ref, edges = M.ref_of(key), M.edges_of(key)
    bits = expected(col, ref.vals, ref.valid, "ne", M.median(key))
    seen = 0
    for a, s, b in zip(edges[:-2], edges[1:-1], edges[2:]):
        if s % 32 == 0:
            continue
        w0 = s - s % 32
        for lo, hi, page in ((max(a, w0), s, (a, s)), (s, min(b, w0 + 32), (s, b))):
            if hi - lo >= 2 and ref.valid[page[0]:page[1]].any():
                side = bits[lo:hi]
                assert side.any() and not side.all(), "seam %d: the side [%d, %d) holds one bit only" % (s, lo, hi)
                seen += 1
    if key[0] not in ("aligned", "adaptive"):   # (their seams lie between words)
        assert seen >= len(edges) - 3


FLOAT_KEYS = [k for k in NUMERIC if k[1] in M.FLOATS]


def test_a_float_sum_differs_between_slot_order_and_row_order():
    """page slots first, then tile slots, against the rows in their order: different double bits under at least one
    selection, for every float plan that holds RLE pages among others"""
    told = {}
    for key in FLOAT_KEYS:
        if "R" not in M.routes(key):
            continue
        pairs = [M.sums_by_order(key, m) for m in M.masks(key)]
        told[M.key_id(key)] = any(_bits(a) != _bits(b) for a, b in pairs)
    print(told)
    # (Float32: a few thousand values of 24 bits add up exactly in double, so no order can show; its bytes are compared all the same)
    assert all(v == (M.TYPE_NAMES[S.T_F64] in k) for k, v in told.items()) and any(told.values()), told


# ---------------------------------------------------------------- 5: every reference can be computed, and is not trivial
N_SMALL, N_LARGE = 5, 700


@pytest.mark.parametrize("key", NUMERIC, ids=ids_of(NUMERIC))
def test_numeric_references(key):
    from tests import aggregate_grouped_ref as G
    from tests import aggregate_weighted_ref as W
    from tests import key_buckets_ref as B
    from tests import key_ids_ref as K
    from tests import key_lookup_ref as L
    from tests import topk_ref as T
    from tests.test_gpu_filter import expected
    from tests.test_gpu_filter_in import want_in
    col = M.stitched(key)[0]
    ref = M.ref_of(key)
    is_int = key[1] not in M.FLOATS
    med = M.median(key)
    lo, hi = M.outside(key)
    assert 0 < expected(col, ref.vals, ref.valid, "le", med).sum() < ref.valid.sum() or ref.rows < 3
    assert not expected(col, ref.vals, ref.valid, "lt", lo).any() and np.array_equal(expected(col, ref.vals, ref.valid, "lt", hi), ref.valid)
    lits = M.in_list(key)
    assert 0 < want_in(col, ref.vals, ref.valid, lits, False).sum() < ref.valid.sum()
    bounds = M.bucket_bounds(key)
    assert bounds.size >= len(M.edges_of(key)) - 2 and (np.diff(bounds) > 0).all()
    small, large = M.group_ids(key, N_SMALL), M.group_ids(key, N_LARGE)
    assert (small == N_SMALL).any() and (large == N_LARGE).any(), "one id out of range"
    for name, mask in zip(M.SELECTIONS, M.masks(key)):
        w = ref.want(mask)
        assert w.rows == ref.rows
        if name == "random":
            assert 0 < w.selected < ref.rows and 0 < w.count < w.selected
        g = G.want(ref, small, N_SMALL, mask)
        if name in ("random", "none"):
            assert all(x.count > 0 for x in g.groups), "every one of the five groups is hit"
        if name == "random" or ref.rows < 20_000:
            gl = G.want(ref, large, N_LARGE, mask)
            if name == "none" and ref.rows > 10 * N_LARGE:
                assert all(x.selected > 0 for x in gl.groups)
        T.want(ref, mask, 7, True)
        assert T.want(ref, mask, 256, False).found > 0
        B.want(ref, mask, bounds, None, False, None, 2)
        if is_int:
            k = K.want(ref, mask, M.MAX_KEYS, 2)
            assert not k.overflow and k.n_keys > 0
            if name in ("random", "none"):
                assert K.want(ref, mask, 4, 1).overflow
            lw = L.want(ref, mask, M.lookup_list(key), None, 2)
            if name in ("random", "none"):
                assert 0 < lw.matched < lw.count
    if ref.rows < 20_000:
        rng = np.random.default_rng(1)
        W.want(ref, rng.integers(-5, 5, ref.rows), None, large, N_LARGE, M.masks(key)[0])


@pytest.mark.parametrize("key", BINARY, ids=ids_of(BINARY))
def test_binary_references(key):
    from tests import key_ids_var_ref as KV
    from tests import key_lookup_ref as L
    from tests.substring_ref import sub_expected
    from tests.test_gpu_filter_binary import expected
    from tests.test_gpu_filter_in import want_in_bin
    ref = M.ref_of(key)
    strs = ref.strs.tolist()
    med = M.median(key)
    for op in ("eq", "lt", "starts_with"):
        assert 0 < expected(strs, ref.valid, op, med[:4] if op == "starts_with" else med).sum() < ref.valid.sum()
    assert 0 < sub_expected(strs, ref.valid, "contains", med[1:5]).sum() < ref.valid.sum()
    assert 0 < want_in_bin(strs, ref.valid, M.in_list(key), False).sum() < ref.valid.sum()
    for name, mask in zip(M.SELECTIONS, M.masks(key)):
        k = KV.want(ref, mask, M.MAX_KEYS, 2)
        assert bool(k.overflow) == (key == ("adaptive", S.T_BIN32) and name in ("random", "none")) and (k.overflow or k.n_keys > 0)
        lw = L.want(ref, mask, M.lookup_list(key), None, 2)
        if name in ("random", "none"):
            assert 0 < lw.matched < lw.count
