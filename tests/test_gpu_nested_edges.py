"""The nested edge table (tests/nested_cases.py) on the device, against the CPU oracle.  Everything is integers and bits:
the tolerance is zero.
  * write: sb_nested_write_levels == S.nested_write_levels page by page (num_values, leaf_start, leaf_count, level_bytes and
    the section bytes), for every case and every cut of it;
  * read: oracle-written pages (I32 leaf, uncompressed; one case with an RLE leaf) through nested.read_nested rebuild the
    Arrow buffers the levels came from;
  * one batched call with a fast-path, a generic and a depth-8 column side by side (per-item map and scratch offsets);
  * whole pages through write_nested (page_heads of very different sizes);
  * n_levels = 9 is refused by the write and the read call.
Every input is a well-formed column; corrupt sections stay with tests/test_gpu_robustness.py.  tests/test_nested_cases.py
checks the same table, and the oracle at these shapes, on the CPU."""
import functools

import numpy as np
import pytest

from oracle import sbo as S
from tests import nested_cases as NC
from tests.test_gpu_nested import check_decoded, device_levels, leaf_values, oracle_pages, up

pytestmark = pytest.mark.gpu


def dev_levels(ctx, levels):
    dl = device_levels(ctx, levels)
    for d, lv in zip(dl, levels):
        d.validity_bit_offset = lv.get("validity_off", 0)
    return dl


@functools.lru_cache(maxsize=None)
def oracle_sections(name, cut):
    """[(section bytes, num_values, leaf_start, leaf_count)] per page: computed once, shared, never modified"""
    c = NC.by_name(name)
    return [S.nested_write_levels(c.levels, r0, ln) for r0, ln in NC.page_ranges(c.rows, cut)]


def assert_sections(got, want, where):
    assert got.n_pages == len(want), where
    sec = got.sections.cpu().numpy()
    off = 0
    for p, (b, nv, ls, lc) in enumerate(want):
        b = np.asarray(b)
        assert (int(got.num_values[p]), int(got.leaf_start[p]), int(got.leaf_count[p])) == (nv, ls, lc), "%s, page %d" % (where, p)
        assert int(got.level_bytes[p]) == b.size, "%s, page %d: level_bytes" % (where, p)
        g = sec[off:off + b.size]
        if not np.array_equal(g, b):
            at = int(np.argmax(g != b))
            rep_len = int.from_bytes(bytes(b[4:8]), "little")
            part = "header" if at < 12 else "rep stream, byte %d" % (at - 12) if at < 12 + rep_len else "def stream, byte %d" % (at - 12 - rep_len)
            raise AssertionError("%s, page %d (%d entries): first difference at byte %d of %d (%s): got %02x, want %02x"
                                 % (where, p, nv, at, b.size, part, int(g[at]), int(b[at])))
        off += b.size


@pytest.mark.parametrize("name", NC.case_names())
def test_level_sections_match_oracle(gpu_ctx, name):
    from strawboat_amd import nested
    c = NC.by_name(name)
    dl = dev_levels(gpu_ctx, c.levels)
    for cut in c.cuts:
        got = nested.write_levels(gpu_ctx, dl, c.rows, cut)
        assert_sections(got, oracle_sections(name, cut), "%s cut at %s" % (name, cut))


def check_decoded_np(arr, levels, rows, values, w):
    """check_decoded of tests/test_gpu_nested.py with numpy arrays (pages of hundreds of thousands of entries)"""
    want = NC.expected_arrays(levels, 0, rows)
    assert arr.lengths == want["lengths"]
    for k, lv in enumerate(levels):
        if lv["kind"] in (S.K_LIST, S.K_LARGE_LIST):
            offs = arr.offsets_numpy(k)
            assert np.array_equal(offs[:-1], want["offsets"][k]), "offsets of level %d" % k
            assert int(offs[-1]) == want["lengths"][k + 1]
        if lv["is_optional"] and lv["kind"] != S.K_PRIMITIVE:
            bits = np.unpackbits(arr.validity_numpy(k), bitorder="little")[:want["lengths"][k]]
            assert np.array_equal(bits, want["validity"][k]), "validity of level %d" % k
    if levels[-1]["is_optional"]:
        bits = np.unpackbits(arr.leaf.validity_numpy(), bitorder="little")[:want["leaf_count"]]
        assert np.array_equal(bits, want["leaf_validity"])
    got = arr.leaf.values[:want["leaf_count"] * w].cpu().numpy()
    assert np.array_equal(got, np.ascontiguousarray(values).view(np.uint8)[:want["leaf_count"] * w])


def _kinds(levels):
    return [lv["kind"] for lv in levels], [bool(lv["is_optional"]) for lv in levels]


@pytest.mark.parametrize("name", NC.case_names())
def test_read_oracle_written_pages(gpu_ctx, name):
    from strawboat_amd import nested
    from strawboat_amd.read import ColumnPages
    c = NC.by_name(name)
    values, w = leaf_values(c.levels, S.T_I32, 11)
    kinds, opt = _kinds(c.levels)
    for cut in c.cuts:
        pages, metas = oracle_pages(c.levels, S.T_I32, values, c.rows, c.rows if cut is None else cut, force_codec=S.NONE)
        assert [int(m) for m in metas[:, 1]] == [nv for _, nv, _, _ in oracle_sections(name, cut)]
        arr = nested.read_nested(gpu_ctx, ColumnPages(S.T_I32, False, up(gpu_ctx, pages), metas), kinds, opt)
        (check_decoded_np if c.big else check_decoded)(arr, c.levels, c.rows, values, w)


def test_read_pages_with_an_rle_leaf(gpu_ctx):
    """the leaf BLOCKs behind long level sections through a codec that is not a plain copy.  The RLE writer sees the leaf
    validity and lets a run go on through null slots, so the values to expect are the oracle's own reading of every BLOCK;
    at the valid slots they are the input's."""
    from strawboat_amd import nested
    from strawboat_amd.read import ColumnPages
    c = NC.by_name("long_fast_list_struct")
    values, w = leaf_values(c.levels, S.T_I64, 5, runs=6)
    kinds, opt = _kinds(c.levels)
    pages, metas = oracle_pages(c.levels, S.T_I64, values, c.rows, c.cuts[1], force_codec=S.RLE)
    want, off = [], 0
    for (length, _), (b, _, ls, lc) in zip(metas, oracle_sections(c.name, c.cuts[1])):
        blk = pages[off + len(b):off + int(length)].copy()
        got = S.read_column(S.T_I64, False, blk, np.array([[blk.size, lc]], np.uint64))["values"]
        want.append(np.ascontiguousarray(got).view(np.int64)[:lc])
        off += int(length)
    want = np.concatenate(want)
    leaf = c.levels[-1]
    valid = np.unpackbits(leaf["validity"], bitorder="little")[:leaf["length"]].astype(bool)
    assert want.size == values.size and np.array_equal(want[valid], values[valid]) and not np.array_equal(want, values)
    arr = nested.read_nested(gpu_ctx, ColumnPages(S.T_I64, False, up(gpu_ctx, pages), metas), kinds, opt)
    check_decoded(arr, c.levels, c.rows, want, w)


BATCH = ("long_fast_list", "long_generic_bottom", "depth8_mixed")   # a fast-path, a generic and a depth-8 column
BATCH_CUT = 300                                                      # 6, 4 and 2 pages


def test_one_batched_call_over_both_paths(gpu_ctx):
    """write_levels_batch / read_nested_leaves with the k_nested_emit and the k_nested_pack columns in ONE call: the
    per-item map and scratch offsets, each column with its own page count"""
    from strawboat_amd import nested
    from strawboat_amd.read import ColumnPages
    cs = [NC.by_name(n) for n in BATCH]
    assert NC.is_fast_path(cs[0].levels) and not NC.is_fast_path(cs[1].levels) and len(cs[2].levels) == 8
    assert len({len(NC.page_ranges(c.rows, BATCH_CUT)) for c in cs}) == 3
    got = nested.write_levels_batch(gpu_ctx, [dev_levels(gpu_ctx, c.levels) for c in cs], BATCH_CUT)
    assert len(got) == 3
    for g, c in zip(got, cs):
        assert_sections(g, oracle_sections(c.name, BATCH_CUT), "%s in the batch" % c.name)
    cps, kinds, opts, vals = [], [], [], []
    for c in cs:
        values, w = leaf_values(c.levels, S.T_I32, 11)
        pages, metas = oracle_pages(c.levels, S.T_I32, values, c.rows, BATCH_CUT, force_codec=S.NONE)
        cps.append(ColumnPages(S.T_I32, False, up(gpu_ctx, pages), metas))
        k, o = _kinds(c.levels)
        kinds.append(k)
        opts.append(o)
        vals.append((values, w))
    arrs = nested.read_nested_leaves(gpu_ctx, cps, kinds, opts)
    assert len(arrs) == 3
    for arr, c, (values, w) in zip(arrs, cs, vals):
        check_decoded(arr, c.levels, c.rows, values, w)


@pytest.mark.parametrize("name,page_rows", [("long_fast_list", 300), ("long_fast_list_struct", 300), ("long_generic_top", 300),
                                            ("long_generic_bottom", 300), ("depth8_mixed", 150), ("depth8_optional_lists", 150)])
def test_whole_pages_match_oracle(gpu_ctx, name, page_rows):
    """write_nested: level sections of a few bytes next to sections of several KiB in front of their leaf BLOCKs
    (page_heads placement)"""
    from strawboat_amd import WriteOptions, nested
    from strawboat_amd.write import DeviceColumn
    c = NC.by_name(name)
    values, w = leaf_values(c.levels, S.T_I32, 7)
    leaf = c.levels[-1]
    want_pages, want_metas = oracle_pages(c.levels, S.T_I32, values, c.rows, page_rows, force_codec=S.NONE)
    if name.startswith("long_"):
        heads = [len(b) for b, _, _, _ in oracle_sections(name, page_rows)]
        assert max(heads) >= 20 * min(heads)
    dcol = DeviceColumn(S.T_I32, False, leaf["length"], up(gpu_ctx, values), up(gpu_ctx, leaf.get("validity")))
    enc = nested.write_nested(gpu_ctx, dev_levels(gpu_ctx, c.levels), dcol, WriteOptions(max_page_size=page_rows, force_codec=S.NONE))
    assert np.array_equal(enc.metas_array(), want_metas)
    got = enc.pages_numpy()
    assert got.size == want_pages.size
    if not np.array_equal(got, want_pages):
        at = int(np.argmax(got != want_pages))
        ends = np.cumsum(want_metas[:, 0].astype(np.int64))
        raise AssertionError("first difference at byte %d (page %d)" % (at, int(np.searchsorted(ends, at, side="right"))))


def test_nine_levels_are_refused(gpu_ctx):
    """include/strawboat_hip.h: n_levels > SB_NESTED_MAX_DEPTH is SB_ERR_INVALID for the write and the read call — at the call,
    before any launch — and the context keeps working"""
    from strawboat_amd import nested
    from strawboat_amd._native import NativeError, SB_ERR_INVALID
    from strawboat_amd.read import ColumnPages
    lv9 = NC.build_path(((NC.STRUCT, False),) * 8, False, 100, lambda k, n, rng: np.zeros(n, np.int64), seed=1)
    assert len(lv9) == 9
    with pytest.raises(NativeError) as e:
        nested.write_levels(gpu_ctx, dev_levels(gpu_ctx, lv9), 100, None)
    assert e.value.code == SB_ERR_INVALID
    lv8 = lv9[1:]
    values, w = leaf_values(lv8, S.T_I32, 3)
    pages, metas = oracle_pages(lv8, S.T_I32, values, 100, 100, force_codec=S.NONE)
    col = ColumnPages(S.T_I32, False, up(gpu_ctx, pages), metas)
    with pytest.raises(NativeError) as e:
        nested.read_nested(gpu_ctx, col, *_kinds(lv9))
    assert e.value.code == SB_ERR_INVALID
    arr = nested.read_nested(gpu_ctx, col, *_kinds(lv8))
    check_decoded(arr, lv8, 100, values, w)
