"""ENDS_WITH / CONTAINS / NOT_STARTS_WITH / NOT_ENDS_WITH / NOT_CONTAINS of sb_filter_columns_var: pages written by the CPU
oracle, filtered on the device, compared bit for bit with Python's `lit in s` / `s.endswith(lit)` / `s.startswith(lit)` over
the oracle's decode of the same pages, ANDed with the validity (tests/substring_ref.py).  Nothing is compared with a tolerance.
Every fixture asserts ON THE REFERENCE that its predicate selects some but not all valid rows (`selective`), unless the case
is the empty or the over-long literal, or a OneValue page (whose valid rows all hold one value: there the fixture has a
literal that every valid row satisfies and a near miss that none does)."""
import ctypes as C

import numpy as np
import pytest

from oracle import sbo as S
from tests import gen
from tests.substring_ref import OPS6, SUB_OPS, selective, sub_expected
from tests.test_gpu_filter_binary import (CODECS, codec_column, column_of, oracle_strings, raw_var, staged_bytes, strings_of,
                                          unpack, upload, write)

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33, 300)


def run_preds(ctx, cp, strs, valid, preds, chunk=48, **kw):
    """the predicates over the same pages, `chunk` per call (a column entry per predicate), combine = set"""
    import strawboat_amd as sb
    for c0 in range(0, len(preds), chunk):
        part = preds[c0:c0 + chunk]
        sc = dict(stage_capacity=[kw["stage_capacity"]] * len(part)) if "stage_capacity" in kw else {}
        sels = sb.filter_columns(ctx, [cp] * len(part), [sb.Predicate(op, lit) for op, lit in part], **sc)
        ctx.synchronize()
        for (op, lit), sel in zip(part, sels):
            want = sub_expected(strs, valid, op, lit)
            got = sel.numpy()
            assert sel.rows == want.size
            assert np.array_equal(got, want), "%s %r: %d rows differ, first at %d" % (op, lit[:40], int((got != want).sum()), int(np.argmax(got != want)))
            assert sel.selected == int(want.sum()), (op, lit[:40], sel.selected, int(want.sum()))
            tail = np.unpackbits(sel.bitmap.cpu().numpy(), bitorder="little")[sel.rows:]
            assert not tail.any(), "bits behind the last row must be 0 after set"


def check(ctx, col, preds, codec=None, **opt):
    pages, metas = write(col, codec, **opt)
    strs, valid = oracle_strings(col, pages, metas)
    run_preds(ctx, upload(ctx, col, pages, metas), strs, valid, preds)
    return strs, valid


def all_ops(lits):
    return [(op, lit) for lit in lits for op in OPS6]


# ---- 1: codecs x offsets width x nullable x page sizes x 6 ops x the literal lengths
def codec_literals(col):
    """per length of LENGTHS a prefix, a suffix and an inner part of the column's longest value (padded by repeating it when
    the length is beyond it: those literals match nothing), one literal longer than every value and one longer than the block"""
    vals = strings_of(col)
    longest = max(vals, key=len)
    assert len(longest) >= 17
    stretch = longest * (300 // len(longest) + 2)
    lits = {}
    for n in LENGTHS:
        if n <= len(longest):
            k = (len(longest) - n) // 2
            if n == 1:   # (a digit: every value of these columns holds the longest one's first letter)
                k = next(i for i, ch in enumerate(longest) if chr(ch).isdigit())
            lits[n] = (longest[:n], longest[len(longest) - n:], longest[k:k + n])
        else:
            lits[n] = (stretch[:n], stretch[-n:], stretch[1:1 + n])
    over_value = longest + b"~"
    over_block = b"w" * (col["values"].size + 1)
    return lits, over_value, over_block


@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
@pytest.mark.parametrize("name,codec,opt", CODECS, ids=[c[0] for c in CODECS])
def test_codecs(gpu_ctx, large, name, codec, opt):
    for nd, page in ((0.2, 2050), (None, 4100), (0.2, 777), (None, 2048)):
        col = codec_column(codec, large, nd, seed=page)
        if codec == S.ONEVALUE:   # (a value long enough for the lengths up to 17)
            col = gen.binary(10_000, uniq=1, null_density=nd, large=large, seed=page, minlen=20, maxlen=30)
        lits, over_value, over_block = codec_literals(col)
        pages, metas = write(col, codec, max_page_size=page, **opt)
        if codec in (S.LZ4, S.ZSTD, S.SNAPPY):
            assert staged_bytes(col, pages, metas) <= 4 * pages.size
        strs, valid = oracle_strings(col, pages, metas)
        assert valid.any()
        preds = all_ops([lit for n in LENGTHS for lit in lits[n]] + [over_value, over_block])
        for n in (1, 2, 3, 4, 5, 7, 8, 9, 16, 17):
            pre, suf, mid = lits[n]
            if codec == S.ONEVALUE:
                assert np.array_equal(sub_expected(strs, valid, "contains", mid), valid)
                assert not sub_expected(strs, valid, "contains", mid[:-1] + b"~").any()
                preds += all_ops([mid[:-1] + b"~"])
            elif n <= 16:
                assert n == 1 or selective(strs, valid, "starts_with", pre), (n, pre)
                assert selective(strs, valid, "ends_with", suf), (n, suf)
                assert selective(strs, valid, "contains", mid) and selective(strs, valid, "not_contains", mid), (n, mid)
        for lit in (over_value, over_block):
            assert not sub_expected(strs, valid, "contains", lit).any()
            assert np.array_equal(sub_expected(strs, valid, "not_ends_with", lit), valid)
        run_preds(gpu_ctx, upload(gpu_ctx, col, pages, metas), strs, valid, preds, chunk=64)


# ---- 2: row, tile and page borders; empty rows; a null row whose slot holds the literal
def border_column(large):
    rows = 12_300   # three pages of 4100 rows: tiles of 4096 and 4 rows
    rng = np.random.default_rng(2)
    s = [b"z%d" % int(v) for v in rng.integers(0, 50, rows)]
    put = {10: b"xxab", 11: b"cxx",            # a row border
           4095: b"xxab", 4096: b"cxx",        # a tile border of page 0
           4099: b"ab", 4100: b"c",            # a page border
           20: b"", 21: b"abc", 22: b"", 23: b"", 24: b"qabc", 25: b"abcq", 26: b"",   # empty rows before, between and after matches
           50: b"abc",                         # (made null below)
           4097: b"abc", 4098: b"ab", 8198: b"abc",   # the short last tiles of pages 0 and 1
           12_299: b"xabc"}
    for r in range(4101, 4100 + 40):           # a run of empty rows (the one at a tile's start: rows 8200 .. 8232) ...
        put[r] = b""
    put[4100 + 40] = b"abc"
    for r in range(4100 + 4096 - 30, 4100 + 4096):   # ... and at a tile's end, behind a match
        put[r] = b""
    put[4100 + 4096 - 31] = b"xabc"
    put[8199] = b"a"                           # the page border with the split elsewhere, and empty rows in between:
    for r in range(8200, 8200 + 33):           # a page (and tile) that starts with empty rows
        put[r] = b""
    put[8233] = b"bc"                          # `a` | 33 x `` | `bc` is no match
    put[8234] = b"abc"
    for r, v in put.items():
        s[r] = v
    col = column_of(s, rng, 0.05, large)
    valid = np.unpackbits(col["validity"], bitorder="little")[:rows].astype(bool)
    valid[50] = False
    valid[[10, 11, 21, 24, 25, 4095, 4096, 4097, 4099, 4100, 4140, 8198, 8199, 8233, 8234, 12_299, 4100 + 4096 - 31]] = True
    col["validity"] = gen.pack_bits(valid)
    return col


@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
@pytest.mark.parametrize("name,codec,opt", [CODECS[0], CODECS[1], CODECS[4]], ids=["none", "lz4", "dict"])
def test_row_tile_and_page_borders(gpu_ctx, large, name, codec, opt):
    col = border_column(large)
    pages, metas = write(col, codec, max_page_size=4100, **opt)
    assert [int(m[1]) for m in np.asarray(metas).tolist()] == [4100, 4100, 4100]
    strs, valid = oracle_strings(col, pages, metas)
    want = sub_expected(strs, valid, "contains", b"abc")
    assert not valid[50]
    if codec != S.DICT:   # (a Dict page stores an index for the null row, not its bytes)
        assert strs[50] == b"abc", "the null row's slot holds the literal"
    assert not want[50] and not sub_expected(strs, valid, "not_contains", b"abc")[50]
    for r in (10, 11, 4095, 4096, 4099, 4100, 8199, 8233):
        assert valid[r] and not want[r], "no match across a border"
    assert b"abc" in b"".join(strs[4095:4097]) and b"abc" in b"".join(strs[4099:4101]) and b"abc" == b"".join(strs[8199:8234])
    for r in (21, 24, 25, 4097, 4140, 8198, 8234, 12_299, 4100 + 4096 - 31):
        assert want[r]
    assert int(want.sum()) == 9 and selective(strs, valid, "contains", b"abc")
    run_preds(gpu_ctx, upload(gpu_ctx, col, pages, metas), strs, valid, all_ops([b"abc", b"ab", b"c", b"bc", b"z1"]))


# ---- 3: the literal at every byte offset 0 .. 2100 of a values block
def test_every_position(gpu_ctx):
    """page k is [k bytes of padding | the needle row | two short rows]: the needle starts at byte k of the page's values
    block, and the pages themselves sit at ever other alignments in the column's bytes"""
    needle = b"QRSTUVWXY"
    s = []
    for k in range(2101):
        s += [b"." * k, needle, b"Q.", b""]
    col = column_of(s)
    pages, metas = write(col, S.NONE, max_page_size=4, force_codec=S.NONE)
    assert metas.shape[0] == 2101
    strs, valid = oracle_strings(col, pages, metas)
    lits = [needle[:1], needle[:4], needle[:5], needle]
    for lit in lits:
        assert selective(strs, valid, "contains", lit)
    assert selective(strs, valid, "ends_with", needle[4:]) and selective(strs, valid, "not_ends_with", b"Y")
    assert int(sub_expected(strs, valid, "contains", needle[:5]).sum()) == 2101
    preds = [(op, lit) for lit in lits for op in ("contains", "not_contains")] + [("ends_with", needle[4:]), ("not_ends_with", b"Y")]
    run_preds(gpu_ctx, upload(gpu_ctx, col, pages, metas), strs, valid, preds, chunk=5)


# ---- 4: the pages at 16 consecutive byte offsets; the values block ends at the tensor's last byte
@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
def test_alignment(gpu_ctx, large):
    import torch
    from strawboat_amd import read
    col = gen.binary(5000, uniq=80, null_density=0.1, large=large, seed=14, minlen=3, maxlen=45)
    pages, metas = write(col, S.NONE, max_page_size=2050, force_codec=S.NONE)
    strs, valid = oracle_strings(col, pages, metas)
    longest = max(strs, key=len)
    lits = [longest[5:6], longest[3:8], longest[2:11], longest[1:18], longest[-4:]]
    assert all(selective(strs, valid, "contains", lit) for lit in lits) and selective(strs, valid, "ends_with", lits[-1])
    n = pages.size
    for shift in range(16):
        big = torch.full((n + 15,), 0xEE, dtype=torch.uint8, device=gpu_ctx.torch_device)
        big[shift:shift + n] = torch.from_numpy(np.ascontiguousarray(pages)).to(gpu_ctx.torch_device)
        view = big[shift:shift + n]
        assert view.data_ptr() == big.data_ptr() + shift
        if shift == 15:   # the last page's values block is its last section: it ends at the tensor's last byte
            assert view.data_ptr() + n == big.data_ptr() + big.numel()
        cp = read.ColumnPages(col["ptype"], col["nullable"], view, metas)
        run_preds(gpu_ctx, cp, strs, valid, all_ops(lits))


# ---- 5: near misses, overlaps, dense candidates, bytes 0x00 and 0x80 .. 0xFF
@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
@pytest.mark.parametrize("name,codec,opt", [CODECS[0], CODECS[1], CODECS[4]], ids=["none", "lz4", "dict"])
def test_near_misses_overlaps_and_dense_candidates(gpu_ctx, large, name, codec, opt):
    rng = np.random.default_rng(51 + codec)
    L = 37
    vocab = [b"prefix--Y" * k for k in (1, 2, 5)] + [b"prefix--Yprefix--prefix--Y", b"prefix--", b"prefix--prefix--X", b"prefix--X",
             b"prefix--X-tail", b"Xprefix--", b"aaaa", b"aaa", b"aa", b"ababab", b"abab", b"aba", b"bababa", b"needle", b"needle-tail", b"head-needle",
             b"mid-needle-mid", b"needl", b"eedle", b"a" * L, b"a" * (L - 1) + b"b", b"b", b"", b"\0", b"\0\0", b"a\0b", b"\0a\0",
             b"\x80", b"\xff", b"\x80\xff", b"\xff\x80", b"x\x80\xffy", bytes(range(0x80, 0x100)), bytes(range(256)), b"\x7f\x80",
             b"\xfe\xff" * 9]
    strings = [vocab[i] for i in rng.integers(0, len(vocab), 9000)]
    col = column_of(strings, rng, 0.15, large)
    lits = [b"prefix--X", b"prefix--Y", b"aaa", b"abab", b"needle", b"a", b"a" * L, b"a" * (L + 1), b"\0", b"\0\0", b"\x80", b"\x80\xff",
            b"\xff", bytes(range(0x80, 0x100)), bytes(range(0xf0, 0x100)), b"\x7f\x80", b"\xff\xfe\xff", b"b", b"prefix--prefix--X"]
    strs, valid = check(gpu_ctx, col, all_ops(lits), codec=codec, max_page_size=2050, **opt)
    for lit in lits:
        if len(lit) <= L:
            assert selective(strs, valid, "contains", lit), lit
    assert not sub_expected(strs, valid, "contains", b"a" * (L + 1)).any()
    # `aaa` is in `aaaa` and not in `aa`; `abab` in `ababab` and `bababa`, not in `aba`; a signed or a zero-terminated compare differs
    e = sub_expected(strs, np.ones(len(strs), bool), "contains", b"aaa")
    assert e[strs.index(b"aaaa")] and not e[strs.index(b"aa")]
    e = sub_expected(strs, np.ones(len(strs), bool), "contains", b"abab")
    assert e[strs.index(b"ababab")] and e[strs.index(b"bababa")] and not e[strs.index(b"aba")]
    assert sub_expected(strs, valid, "contains", b"\0\0").sum() < sub_expected(strs, valid, "contains", b"\0").sum()
    # the literal as a whole row, at a row's first bytes, at its last bytes
    for lit in (b"needle", b"prefix--X"):
        assert 0 < sub_expected(strs, valid, "ends_with", lit).sum() < sub_expected(strs, valid, "contains", lit).sum()
        assert 0 < sub_expected(strs, valid, "starts_with", lit).sum() < sub_expected(strs, valid, "contains", lit).sum()


# ---- 6: long rows
def long_rows_column(large):
    """rows of 70 000 bytes among short ones, each with the needle at one place: its start, its middle, its end, and across
    every 4096-byte step from the row's first byte; one long row with a near miss only"""
    needle, n = b"NEEDLE", 70_000
    places = [0, 35_000, n - len(needle)] + [4096 * j - 3 for j in range(1, 18)]
    s = []
    for i, p in enumerate(places):
        s += [b"s%d" % i, b"", b"." * p + needle + b"." * (n - p - len(needle)), b"NEEDL", b"EEDLE"]
    s += [b"." * 30_000 + b"NEEDL.EEDLE" + b"." * 39_989, b"tail"]
    return column_of(s, large=large), needle


@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
def test_long_rows(gpu_ctx, large):
    col, needle = long_rows_column(large)
    for codec, opt in ((S.NONE, dict(force_codec=S.NONE)), (S.LZ4, dict(force_codec=S.LZ4))):
        pages, metas = write(col, codec, max_page_size=33, **opt)
        strs, valid = oracle_strings(col, pages, metas)
        assert int(sub_expected(strs, valid, "contains", needle).sum()) == 20 and selective(strs, valid, "contains", needle)
        assert int(sub_expected(strs, valid, "ends_with", needle).sum()) == 1 and int(sub_expected(strs, valid, "starts_with", needle).sum()) == 1
        sc = dict(stage_capacity=staged_bytes(col, pages, metas)) if codec == S.LZ4 else {}
        run_preds(gpu_ctx, upload(gpu_ctx, col, pages, metas), strs, valid, all_ops([needle, b"N", b"NEEDL.E", b".NEEDLE.", b"EEDLE."]), **sc)


def test_a_row_that_is_the_whole_tile(gpu_ctx):
    """4095 empty rows and one row of 5000 bytes in the first tile of a 4100-row page"""
    for at in (0, 2000, 4095):
        s = [b""] * 4100
        s[at] = b"." * 4990 + b"0123456789"
        s[4097] = b"789"
        s[4099] = b"0123456789"
        col = column_of(s)
        pages, metas = write(col, S.NONE, max_page_size=4100, force_codec=S.NONE)
        strs, valid = oracle_strings(col, pages, metas)
        assert sub_expected(strs, valid, "contains", b"3456789").sum() == 2 and sub_expected(strs, valid, "ends_with", b"789").sum() == 3
        run_preds(gpu_ctx, upload(gpu_ctx, col, pages, metas), strs, valid, all_ops([b"3456789", b"789", b".", b"9.", b"0123456789"]))


@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
def test_onevalue_page_with_a_long_value(gpu_ctx, large):
    value = b"." * 40_000 + b"needle-in-the-middle" + b"." * 29_971 + b"the-end!!"
    assert len(value) == 70_000
    rng = np.random.default_rng(6)
    col = column_of([value] * 3000, rng, 0.3, large)
    pages, metas = write(col, S.ONEVALUE, max_page_size=2050, force_codec=S.ONEVALUE)
    strs, valid = oracle_strings(col, pages, metas)
    hits = [b"needle-in-the-middle", b"the-end!!", b"!", b"..", value[:9], value]
    misses = [b"needle-in-the-middlf", b"the-end!!.", b"!.", value + b".", b"x"]
    for lit in hits:
        assert np.array_equal(sub_expected(strs, valid, "contains", lit), valid) and 0 < valid.sum() < valid.size
    for lit in misses:
        assert not sub_expected(strs, valid, "contains", lit).any()
    run_preds(gpu_ctx, upload(gpu_ctx, col, pages, metas), strs, valid, all_ops(hits + misses))


# ---- 7: Dict on both sides of the LDS bit table; a Freq page (entry 0 sits in front of the page's bitmap)
def test_dict_both_sides_of_the_bit_table(gpu_ctx):
    for uniq in (8192, 8193):
        vocab = [b"entry-%06d-%s" % (i, b"x" * (i % 23)) for i in range(uniq)]
        rng = np.random.default_rng(uniq)
        idx = np.concatenate([np.arange(uniq), rng.integers(0, uniq, 20_000)])
        rng.shuffle(idx)
        col = column_of([vocab[i] for i in idx], rng, 0.2)
        v = np.unpackbits(col["validity"], bitorder="little")[:idx.size].astype(bool)
        v[np.isin(idx, [0, 31, 32, 8191, uniq - 1])] = True   # (the entries the literals below single out are not all null)
        col["validity"] = gen.pack_bits(v)
        pages, metas = write(col, S.DICT, max_page_size=col["rows"], force_codec=S.DICT)
        assert metas.shape[0] == 1
        strs, valid = oracle_strings(col, pages, metas)
        lits =[b"-0081", b"91-", b"xxxxxxxxxxxxxxxxxxxxxx", b"-x", vocab[0][3:], vocab[31][1:], vocab[32][:-1], vocab[8191][2:], vocab[uniq - 1][6:]]
        assert all(selective(strs, valid, "contains", lit) for lit in lits)
        assert selective(strs, valid, "ends_with", b"xx") and selective(strs, valid, "not_ends_with", b"-")
        run_preds(gpu_ctx, upload(gpu_ctx, col, pages, metas), strs, valid, all_ops(lits + [b"xx", b"-"]))


@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
def test_freq_page(gpu_ctx, large):
    from tests.test_gpu_freq import sparse_bin
    col = sparse_bin(10_000, 0.05, 71, null_density=0.1, large=large)
    pages, metas = write(col, S.FREQ, max_page_size=4100, force_codec=S.FREQ)
    strs, valid = oracle_strings(col, pages, metas)
    exc = next(s for s, v in zip(strs, valid) if v and len(s) > 8 and not s.startswith(b"the-"))   # an exception's value
    lits = [b"common", b"-value", b"the-", b"the-common-value", exc[:4], exc[1:], b"e", b"-x"]
    for lit in lits:
        assert selective(strs, valid, "contains", lit), lit
    assert selective(strs, valid, "ends_with", b"-value") and selective(strs, valid, "not_starts_with", b"the-")
    run_preds(gpu_ctx, upload(gpu_ctx, col, pages, metas), strs, valid, all_ops(lits + [b"the-common-value!", b""]))


# ---- 8: combine modes, mixed calls, a replayed interval
def state(sel, rows):
    bits = np.unpackbits(sel.bitmap.cpu().numpy(), bitorder="little").astype(bool)
    return bits[:rows], bits[rows:]


def test_combine_modes_and_a_mixed_call(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from tests.test_gpu_filter import expected as num_expected, oracle_column
    from tests.test_gpu_filter_binary import expected as bin_expected
    rows = 10_007   # (the last word holds 23 rows)
    i32 = gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    s1 = gen.binary(rows, uniq=60, null_density=0.1, seed=3, maxlen=20)
    s2 = gen.binary(rows, uniq=500, seed=4, large=True, zipf=1.3, maxlen=30)
    s3 = gen.binary(rows, uniq=90, null_density=0.3, seed=5, maxlen=25)
    ge_lit = sorted(set(strings_of(s1)))[20]
    plan = ((i32, dict(max_page_size=2050, force_codec=S.RLE), ("lt", 60)),
            (s1, dict(max_page_size=4100, force_codec=S.DICT), ("ge", ge_lit)),
            (s1, dict(max_page_size=4100, force_codec=S.DICT), ("not_contains", b"w1")),
            (s2, dict(max_page_size=2048, force_codec=S.LZ4), ("contains", b"2w")),
            (s3, dict(max_page_size=777, force_codec=S.NONE), ("not_ends_with", b"1")),
            (s3, dict(max_page_size=777, force_codec=S.NONE), ("starts_with", b"w3")),
            (s2, dict(max_page_size=2048, force_codec=S.ZSTD), ("ends_with", b"w")))
    cols, preds, want = [], [], []
    for col, opt, (op, lit) in plan:
        pages, metas = gen.oracle_write(col, **opt)
        cols.append(upload(gpu_ctx, col, pages, metas))
        preds.append(sb.Predicate(op, lit))
        if col["offsets"] is None:
            want.append(num_expected(col, *oracle_column(col, pages, metas), op, lit))
        elif op in OPS6:
            want.append(sub_expected(*oracle_strings(col, pages, metas), op, lit))
        else:
            want.append(bin_expected(*oracle_strings(col, pages, metas), op, lit))
    assert all(0 < w.sum() < rows for w in want)
    # ONE call: a number, an old string op and new string ops over Dict, LZ4, None and Zstd pages
    sels = sb.filter_columns(gpu_ctx, cols, preds)
    gpu_ctx.synchronize()
    for sel, w in zip(sels, want):
        assert np.array_equal(sel.numpy(), w) and sel.selected == int(w.sum())
        assert not state(sel, rows)[1].any()
    # one selection, one interval: set contains, and not_contains, or number, and not_ends_with, or ends_with
    sel = sb.filter_columns(gpu_ctx, [cols[3]], [preds[3]])
    sb.filter_columns(gpu_ctx, [cols[2]], [preds[2]], combine="and", out=sel)
    sb.filter_columns(gpu_ctx, [cols[0]], [preds[0]], combine="or", out=sel)
    sb.filter_columns(gpu_ctx, [cols[4]], [preds[4]], combine="and", out=sel)
    last = sb.filter_columns(gpu_ctx, [cols[6]], [preds[6]], combine="or", out=sel)
    gpu_ctx.synchronize()
    final = ((((want[3] & want[2]) | want[0]) & want[4]) | want[6])
    got, tail = state(sel[0], rows)
    assert np.array_equal(got, final) and not tail.any() and last[0].selected == int(final.sum())
    # step by step on a buffer of ones: and / or keep the bits behind the last row, set clears them
    for i in (2, 3, 4, 6):
        with torch.cuda.stream(gpu_ctx.torch_stream):
            sel[0].bitmap.fill_(0xFF)
        a = sb.filter_columns(gpu_ctx, [cols[i]], [preds[i]], combine="and", out=sel)
        gpu_ctx.synchronize()
        got, tail = state(sel[0], rows)
        assert np.array_equal(got, want[i]) and tail.all() and a[0].selected == int(want[i].sum())
        j = 4 if i != 4 else 3
        o = sb.filter_columns(gpu_ctx, [cols[j]], [preds[j]], combine="or", out=sel)
        gpu_ctx.synchronize()
        got, tail = state(sel[0], rows)
        assert np.array_equal(got, want[i] | want[j]) and tail.all() and o[0].selected == int((want[i] | want[j]).sum())
        s = sb.filter_columns(gpu_ctx, [cols[i]], [preds[i]], combine="set", out=sel)
        gpu_ctx.synchronize()
        got, tail = state(sel[0], rows)
        assert np.array_equal(got, want[i]) and not tail.any() and s[0].selected == int(want[i].sum())


def test_mixed_call_with_a_primitive_freq_page(gpu_ctx):
    """a primitive Freq page makes the interval run again: the new string ops of the same call give the same bits"""
    import strawboat_amd as sb
    from tests.test_gpu_filter import expected as num_expected, oracle_column
    from tests.test_gpu_freq import sparse
    rows = 20_000
    f = sparse(S.T_I32, rows, 0.05, 2, null_density=0.1)
    s = gen.binary(rows, uniq=80, null_density=0.1, seed=9, maxlen=16)
    fp, fm = gen.oracle_write(f, max_page_size=5000, force_codec=S.FREQ)
    wf = num_expected(f, *oracle_column(f, fp, fm), "eq", 7)
    cols, preds, wants = [upload(gpu_ctx, f, fp, fm)], [sb.Predicate("eq", 7)], [wf]
    for codec, op, lit in ((S.DICT, "not_ends_with", b"3"), (S.NONE, "contains", b"3w"), (S.LZ4, "not_contains", b"w1"), (S.NONE, "ends_with", b"7")):
        sp, sm = gen.oracle_write(s, max_page_size=4100, force_codec=codec)
        strs, valid = oracle_strings(s, sp, sm)
        assert selective(strs, valid, op, lit), (op, lit)
        cols.append(upload(gpu_ctx, s, sp, sm))
        preds.append(sb.Predicate(op, lit))
        wants.append(sub_expected(strs, valid, op, lit))
    r0 = gpu_ctx.replays()
    sels = sb.filter_columns(gpu_ctx, cols, preds)
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    for sel, w in zip(sels, wants):
        assert np.array_equal(sel.numpy(), w) and sel.selected == int(w.sum())


# ---- 9: offsets that descend or leave the values block: the per-row route with the cut rule
def test_fallback_route_on_patched_offsets(gpu_ctx):
    import strawboat_amd as sb
    from tests.test_gpu_filter import filter_code
    col = gen.binary(6000, uniq=70, seed=19, minlen=2, maxlen=30)   # one page, two tiles: the second one keeps the scan
    pages, metas = write(col, S.NONE, max_page_size=6000, force_codec=S.NONE)
    assert metas.shape[0] == 1
    rows, vusize = col["rows"], int(col["values"].size)
    # hdr9 | offsets block | hdr9 | values block
    offs = np.frombuffer(pages[9:9 + 4 * (rows + 1)].tobytes(), np.int32).copy()
    assert np.array_equal(offs, col["offsets"]) and pages.size == 9 + 4 * (rows + 1) + 9 + vusize
    vals = pages[pages.size - vusize:].tobytes()
    assert vals == col["values"].tobytes()
    strs0 = strings_of(col)
    lit = max(strs0, key=len)[3:9]
    for patch in ("descend", "beyond", "both"):
        o = offs.copy()
        if patch in ("descend", "both"):
            o[1000] = o[1002] + 3          # off[1000] > off[1001]: a pair that descends (and row 999 grows)
        if patch in ("beyond", "both"):
            o[2000] = vusize + 1000        # off[2000] beyond the block
        assert (np.diff(o.astype(np.int64)) < 0).any()
        bad = pages.copy()
        bad[9:9 + 4 * (rows + 1)] = np.frombuffer(o.tobytes(), np.uint8)
        cp = upload(gpu_ctx, col, bad, metas)
        # the cut rule, from the patched offsets: o1 = min(o1, vusize); o0 = min(o0, o1)
        o64 = o.astype(np.int64)
        o1 = np.minimum(o64[1:], vusize)
        o0 = np.minimum(o64[:-1], o1)
        cut = [vals[a:b] for a, b in zip(o0.tolist(), o1.tolist())]
        ones = np.ones(rows, bool)
        assert selective(cut, ones, "contains", lit)
        code = filter_code(gpu_ctx, cp, sb.Predicate("starts_with", lit))
        for op in SUB_OPS:
            assert filter_code(gpu_ctx, cp, sb.Predicate(op, lit)) == code, (patch, op)
        if code == 0:
            run_preds(gpu_ctx, cp, cut, ones, all_ops([lit, lit[:1], lit[:3], b""]))
    # and the same page unpatched: both routes give the reference's bits on the rows the patches touched
    run_preds(gpu_ctx, upload(gpu_ctx, col, pages, metas), strs0, np.ones(rows, bool), all_ops([lit, lit[:1]]))


# ---- 10: stage_capacity
def test_stage_capacity(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    col = gen.binary(20_000, uniq=50, null_density=0.1, seed=11, maxlen=30)
    for codec in (S.LZ4, S.ZSTD, S.SNAPPY):
        pages, metas = write(col, codec, max_page_size=4100, force_codec=codec)
        need = staged_bytes(col, pages, metas)
        assert need == col["values"].size
        cp = upload(gpu_ctx, col, pages, metas)
        strs, valid = oracle_strings(col, pages, metas)
        lit = max(strs, key=len)[2:7]
        assert selective(strs, valid, "contains", lit)
        for op in ("contains", "not_ends_with"):
            with pytest.raises(NativeError) as e:
                sb.filter_columns(gpu_ctx, [cp], [sb.Predicate(op, lit)], stage_capacity=[need - 1])
                gpu_ctx.synchronize()
            assert e.value.code == -5, codec   # (what test_gpu_filter_binary.test_stage_capacity sees for `lt`)
            try:
                gpu_ctx.synchronize()
            except NativeError:
                pass
        run_preds(gpu_ctx, cp, strs, valid, all_ops([lit]), stage_capacity=need)
        run_preds(gpu_ctx, cp, strs, valid, all_ops([lit]))


# ---- 11: the selection buffer at exactly 4*ceil(rows/32) bytes between two guards
def test_selection_buffer_between_guards(gpu_ctx):
    import torch
    import strawboat_amd as sb
    rows = 10_007
    col = gen.binary(rows, uniq=90, null_density=0.2, seed=23, maxlen=25)
    nbytes = 4 * ((rows + 31) // 32)
    for codec in (S.NONE, S.DICT, S.LZ4):
        pages, metas = write(col, codec, max_page_size=2050, force_codec=codec)
        strs, valid = oracle_strings(col, pages, metas)
        cp = upload(gpu_ctx, col, pages, metas)
        for op, lit in (("contains", b"3w"), ("not_contains", b"3w"), ("ends_with", b"1"), ("not_starts_with", b"w2")):
            assert selective(strs, valid, op, lit)
            for combine in ("set", "and", "or"):
                big = torch.full((4096 + nbytes + 4096,), 0xA5, dtype=torch.uint8, device=gpu_ctx.torch_device)
                out = [sb.Selection(big[4096:4096 + nbytes], rows, None)]
                before = unpack(big[4096:4096 + nbytes].cpu().numpy(), rows)
                sel = sb.filter_columns(gpu_ctx, [cp], [sb.Predicate(op, lit)], combine=combine, out=out)
                gpu_ctx.synchronize()
                host = big.cpu().numpy()
                assert (host[:4096] == 0xA5).all() and (host[4096 + nbytes:] == 0xA5).all(), "a guard was written"
                w = sub_expected(strs, valid, op, lit)
                w = w if combine == "set" else (before & w) if combine == "and" else (before | w)
                assert np.array_equal(unpack(host[4096:4096 + nbytes], rows), w) and sel[0].selected == int(w.sum())


# ---- 12: refusals at the call
def test_refusals_at_the_call(gpu_ctx):
    from strawboat_amd import _native as N
    lib, h = gpu_ctx._lib, gpu_ctx._h
    keep = []
    i32, boo, bcol = gen.prim(S.T_I32, 3000, uniq=10), gen.boolean(3000), gen.binary(3000, uniq=10)
    cases = [(col, op, b"\1\0\0\0"[:n], N.SB_ERR_INVALID) for op in range(11, 16) for col, n in ((i32, 4), (boo, 1))]
    cases += [(bcol, 9, b"a", N.SB_ERR_INVALID), (bcol, 10, b"a", N.SB_ERR_INVALID), (bcol, 16, b"a", N.SB_ERR_INVALID)]
    for col, op, lit, code in cases:
        pages, metas = gen.oracle_write(col)
        cp = upload(gpu_ctx, col, pages, metas)
        arr, bitmap, k = raw_var(gpu_ctx, col, cp, op, lit)
        assert lib.sb_filter_columns_var(h, arr, 1, N.SB_MEM_DEVICE) == code, (col["ptype"], op)
        gpu_ctx.synchronize()
        assert (bitmap.cpu().numpy() == 0xA5).all(), "the selection must stay untouched"
        keep.append(k)
    pages, metas = gen.oracle_write(bcol)
    cp = upload(gpu_ctx, bcol, pages, metas)
    strs, valid = oracle_strings(bcol, pages, metas)
    for op in range(11, 16):
        # a null literal with a nonzero length
        arr, bitmap, k = raw_var(gpu_ctx, bcol, cp, op, b"w1")
        arr[0].literal = None
        assert lib.sb_filter_columns_var(h, arr, 1, N.SB_MEM_DEVICE) == N.SB_ERR_INVALID
        gpu_ctx.synchronize()
        assert (bitmap.cpu().numpy() == 0xA5).all()
        # ... and the descriptor is served with its literal
        arr, bitmap, k = raw_var(gpu_ctx, bcol, cp, op, b"w1")
        assert lib.sb_filter_columns_var(h, arr, 1, N.SB_MEM_DEVICE) == 0
        gpu_ctx.synchronize()
        name = {11: "ends_with", 12: "contains", 13: "not_starts_with", 14: "not_ends_with", 15: "not_contains"}[op]
        want = sub_expected(strs, np.ones(len(strs), bool), name, b"w1")
        assert arr[0].rows == 3000 and arr[0].selected == int(want.sum()) and 0 < want.sum() < 3000
        assert np.array_equal(unpack(bitmap.cpu().numpy(), 3000), want)
    # sb_filter_columns_in keeps refusing everything but IN / NOT_IN
    m = cp.metas_array()
    arr_in = (N.ColumnFilterInC * 1)()
    c = arr_in[0]
    c.physical_type, c.is_nullable = bcol["ptype"], 0
    c.pages, c.pages_len = cp.pages.data_ptr(), cp.pages.numel()
    c.metas, c.n_pages = m.ctypes.data_as(C.POINTER(N.PageMetaC)), m.shape[0]
    c.op, c.combine = N.SB_PRED_CONTAINS, N.SB_SEL_SET
    vals = C.create_string_buffer(b"w1", 2)
    voffs = (C.c_uint64 * 2)(0, 2)
    c.values, c.value_offsets, c.n_values = C.addressof(vals), C.addressof(voffs), 1
    bitmap.fill_(0xA5)
    c.selection, c.selection_capacity = bitmap.data_ptr(), bitmap.numel()
    assert lib.sb_filter_columns_in(h, arr_in, 1, N.SB_MEM_DEVICE) == N.SB_ERR_INVALID
    gpu_ctx.synchronize()
    assert (bitmap.cpu().numpy() == 0xA5).all()
    # the old entry point: the new ops behave as STARTS_WITH does there
    codes = {}
    for op in (N.SB_PRED_STARTS_WITH,) + tuple(range(11, 16)):
        arr_old = (N.ColumnFilterC * 1)()
        c = arr_old[0]
        c.physical_type, c.is_nullable = bcol["ptype"], 0
        c.pages, c.pages_len = cp.pages.data_ptr(), cp.pages.numel()
        c.metas, c.n_pages = m.ctypes.data_as(C.POINTER(N.PageMetaC)), m.shape[0]
        c.op, c.combine = op, N.SB_SEL_SET
        c.selection, c.selection_capacity = bitmap.data_ptr(), bitmap.numel()
        codes[op] = lib.sb_filter_columns(h, arr_old, 1, N.SB_MEM_DEVICE)
        gpu_ctx.synchronize()
        assert (bitmap.cpu().numpy() == 0xA5).all()
    assert codes[N.SB_PRED_STARTS_WITH] != 0 and len(set(codes.values())) == 1, codes
