"""sb_filter_columns_var on Binary / LargeBinary (Utf8) columns: pages written by the CPU oracle, filtered on the device,
compared with Python's own `bytes` comparison (`<`, `==`, `.startswith`) of the oracle's decode of the same pages, row by
row, ANDed with the validity.  Nothing here is compared with what the device's own decoder gives; every bit, `selected` and
the bits behind the last row must match."""
import ctypes as C
import operator
import os

import numpy as np
import pytest

from oracle import sbo as S
from tests import gen

pytestmark = pytest.mark.gpu

OPS6 = ["eq", "ne", "lt", "le", "gt", "ge"]
OPS7 = OPS6 + ["starts_with"]
PYOP = {"eq": operator.eq, "ne": operator.ne, "lt": operator.lt, "le": operator.le, "gt": operator.gt, "ge": operator.ge,
        "starts_with": lambda v, lit: v.startswith(lit)}


def unpack(bits, rows):
    return np.unpackbits(np.asarray(bits, np.uint8), bitorder="little")[:rows].astype(bool)


def oracle_strings(col, pages, metas):
    """(list of `bytes`, one per row; validity as bool) from the oracle's decode of the pages"""
    want = gen.oracle_read(col, pages, metas)
    rows = want["rows"]
    valid = unpack(want["validity"], rows) if col["nullable"] else np.ones(rows, bool)
    odt = np.int64 if col["ptype"] == S.T_BIN64 else np.int32
    offs = np.ascontiguousarray(want["offsets"]).view(np.uint8).reshape(-1).view(odt)[:rows + 1].astype(np.int64)
    data = np.asarray(want["values"], np.uint8).tobytes()
    return [data[offs[i]:offs[i + 1]] for i in range(rows)], valid


def as_bytes(lit):
    return lit.encode("utf-8") if isinstance(lit, str) else bytes(lit)


def expected(strs, valid, op, lit):
    if op == "is_null":
        return ~valid
    if op == "is_not_null":
        return valid.copy()
    f, b = PYOP[op], as_bytes(lit)
    # the distinct values once: a page of 2^18 rows has a few hundred of them
    memo = {}
    out = np.zeros(len(strs), bool)
    for i, s in enumerate(strs):
        r = memo.get(s)
        if r is None:
            r = memo[s] = bool(f(s, b))
        out[i] = r
    return out & valid


def upload(ctx, col, pages, metas):
    import torch
    from strawboat_amd import read
    return read.ColumnPages(col["ptype"], col["nullable"], torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device), metas)


def check_pages(ctx, col, pages, metas, preds, chunk=48, **kw):
    """the predicates over the same pages, `chunk` of them per call (one column entry per predicate), combine = set"""
    import strawboat_amd as sb
    strs, valid = oracle_strings(col, pages, metas)
    cp = upload(ctx, col, pages, metas)
    for c0 in range(0, len(preds), chunk):
        part = preds[c0:c0 + chunk]
        sc = dict(stage_capacity=[kw["stage_capacity"]] * len(part)) if "stage_capacity" in kw else {}
        sels = sb.filter_columns(ctx, [cp] * len(part), [sb.Predicate(op, lit) for op, lit in part], **sc)
        ctx.synchronize()
        for (op, lit), sel in zip(part, sels):
            want = expected(strs, valid, op, lit)
            got = sel.numpy()
            assert sel.rows == want.size
            assert np.array_equal(got, want), "%s %r: %d rows differ, first at %d" % (op, lit, int((got != want).sum()), int(np.argmax(got != want)))
            assert sel.selected == int(want.sum()), (op, lit, sel.selected, int(want.sum()))
            tail = np.unpackbits(sel.bitmap.cpu().numpy(), bitorder="little")[sel.rows:]
            assert not tail.any(), "bits behind the last row must be 0 after set"
    return strs, valid


def write(col, codec=None, **opt):
    pages, metas = gen.oracle_write(col, **opt)
    if codec is not None:
        seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
        assert seen == {codec}, (seen, codec)
    return pages, metas


def check(ctx, col, preds, codec=None, **opt):
    pages, metas = write(col, codec, **opt)
    return check_pages(ctx, col, pages, metas, preds)


def column_of(strings, rng=None, null_density=None, large=False):
    """a column of the test's own strings (any bytes)"""
    lens = np.array([len(s) for s in strings], np.int64)
    offs = np.zeros(len(strings) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    data = np.frombuffer(b"".join(strings), np.uint8).copy() if offs[-1] else np.zeros(0, np.uint8)
    validity = gen.make_validity(rng, len(strings), null_density) if null_density is not None else None
    return dict(ptype=S.T_BIN64 if large else S.T_BIN32, nullable=validity is not None, rows=len(strings), values=data,
                validity=validity, offsets=offs.astype(np.int64 if large else np.int32))


def strings_of(col):
    o = col["offsets"].astype(np.int64)
    d = col["values"].tobytes()
    return [d[o[i]:o[i + 1]] for i in range(col["rows"])]


LENGTHS = (1, 7, 8, 9, 15, 16, 17, 33, 300)


def literals_of(col):
    """a value near the median, the minimum, the maximum, b"", a value + b"\\0", a proper prefix of a value, a literal longer
    than every value, an absent value, and literals of the lengths where the compare changes its path"""
    vals = sorted(set(strings_of(col)))
    med, lo, hi = vals[len(vals) // 2], vals[0], vals[-1]
    longest = max(vals, key=len)
    lits = [med, lo, hi, b"", med + b"\0", longest[:max(1, len(longest) // 2)], longest + b"-and-then-some", b"absent~value"]
    base = (longest * (300 // max(1, len(longest)) + 2)) if longest else b"w" * 302
    lits += [base[:n] for n in LENGTHS]
    return lits, lo, hi


def all_preds(col):
    lits, lo, hi = literals_of(col)
    return [(op, lit) for lit in lits for op in OPS7], lo, hi


def check_selective(strs, valid, lo, hi):
    """ "lt min" selects nothing, "ge min" and "le max" every valid row: a constant answer cannot pass"""
    assert not expected(strs, valid, "lt", lo).any()
    assert np.array_equal(expected(strs, valid, "ge", lo), valid) and np.array_equal(expected(strs, valid, "le", hi), valid)
    assert valid.any()


# ---- 1 + 2: codecs x offsets width x nullable x page sizes x 7 predicates x the literal set
CODECS = [("none", S.NONE, dict(force_codec=S.NONE)), ("lz4", S.LZ4, dict(force_codec=S.LZ4)), ("zstd", S.ZSTD, dict(force_codec=S.ZSTD)),
          ("snappy", S.SNAPPY, dict(force_codec=S.SNAPPY)), ("dict", S.DICT, dict(force_codec=S.DICT)),
          ("onevalue", S.ONEVALUE, dict(force_codec=S.ONEVALUE)), ("freq", S.FREQ, dict(force_codec=S.FREQ))]


def codec_column(codec, large, nd, seed):
    if codec == S.ONEVALUE:
        return gen.binary(10_000, uniq=1, null_density=nd, large=large, seed=seed, minlen=5, maxlen=12)
    if codec == S.FREQ:
        from tests.test_gpu_freq import sparse_bin
        return sparse_bin(10_000, 0.05, seed, null_density=nd, large=large)
    return gen.binary(10_000, uniq=100, null_density=nd, large=large, seed=seed, maxlen=40)


@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
@pytest.mark.parametrize("name,codec,opt", CODECS, ids=[c[0] for c in CODECS])
def test_codecs(gpu_ctx, large, name, codec, opt):
    for nd, page in ((0.2, 2050), (None, 4100), (0.2, 777), (None, 2048)):
        col = codec_column(codec, large, nd, seed=page)
        preds, lo, hi = all_preds(col)
        pages, metas = write(col, codec, max_page_size=page, **opt)
        if codec in (S.LZ4, S.ZSTD, S.SNAPPY):   # the default stage_capacity must do for these fixtures
            assert staged_bytes(col, pages, metas) <= 4 * pages.size
        strs, valid = check_pages(gpu_ctx, col, pages, metas, preds)
        check_selective(strs, valid, lo, hi)
        if codec not in (S.ONEVALUE,):
            med = literals_of(col)[0][0]
            assert 0 < expected(strs, valid, "le", med).sum() and expected(strs, valid, "gt", med).sum() > 0


def staged_bytes(col, pages, metas):
    """sum of the uncompressed sizes of the values blocks of a Basic binary column's pages, read from the page bytes:
    [u32 def_len | def] hdr9(offsets) | offsets block | hdr9(values) | values block"""
    total, pos = 0, 0
    buf = np.asarray(pages, np.uint8).tobytes()
    for length, _ in np.asarray(metas, np.uint64).tolist():
        p = pos
        if col["nullable"]:
            p += 4 + int.from_bytes(buf[p:p + 4], "little")
        csize = int.from_bytes(buf[p + 1:p + 5], "little")
        p += 9 + csize
        total += int.from_bytes(buf[p + 5:p + 9], "little")
        pos += int(length)
    return total


# ---- 3: bytes 0x00 and 0x80..0xFF, shared prefixes
@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
@pytest.mark.parametrize("name,codec,opt", CODECS[:5], ids=[c[0] for c in CODECS[:5]])
def test_unsigned_bytes_zero_bytes_and_shared_prefixes(gpu_ctx, large, name, codec, opt):
    rng = np.random.default_rng(31 + codec)
    stems = [b"", b"\0", b"\0\0", b"a", b"a\0", b"a\0b", b"a\x7f", b"a\x80", b"a\xff", b"\x7f", b"\x80", b"\xff", b"\xff\xff",
             b"prefix--", b"prefix--\0", b"prefix--\x80tail", b"prefix--\x7ftail", b"prefix--prefix--", b"prefix--prefix--\xfe",
             b"prefix--prefix--\x01", b"0123456789abcdef", b"0123456789abcdef\0", b"0123456789abcdefg", b"0123456789abcde",
             bytes(range(256)), bytes(range(255, -1, -1)), b"\x80" * 40, b"\x80" * 39 + b"\x7f", b"\x80" * 39 + b"\x81"]
    vocab = stems + [s + bytes([int(rng.integers(0, 256))]) for s in stems for _ in range(3)]
    strings = [vocab[i] for i in rng.integers(0, len(vocab), 9000)]
    col = column_of(strings, rng, 0.15, large)
    lits = sorted(set(vocab)) + [b"prefix-", b"prefix--prefix-", b"\x80" * 41, b"\x7f\xff", b"a\0\0", bytes(range(256))[:17]]
    preds = [(op, lit) for lit in lits for op in OPS7]
    strs, valid = check(gpu_ctx, col, preds, codec=codec, max_page_size=2050, **opt)
    # the fixtures do tell a signed compare and a compare that stops at a zero byte from the right one
    assert expected(strs, valid, "lt", b"a\x80").sum() != sum(1 for s, v in zip(strs, valid) if v and s.replace(b"\x80", b"\x00") < b"a\x00")
    assert expected(strs, valid, "eq", b"a\0b").sum() != expected(strs, valid, "starts_with", b"a").sum()
    assert expected(strs, valid, "gt", b"\x7f").sum() > expected(strs, valid, "gt", b"\x80").sum() > 0


# ---- 4: Dict index codecs, both sides of the LDS bit table, the fallback walk of the entry finder
@pytest.mark.parametrize("icodec", [S.NONE, S.RLE, S.BITPACK, S.ONEVALUE, S.LZ4])
def test_dict_index_codecs(gpu_ctx, icodec):
    uniq = 1 if icodec == S.ONEVALUE else 200
    rng = np.random.default_rng(5)
    base = gen.binary(128 * 300, uniq=uniq, seed=3, maxlen=24, minlen=1)
    strings = strings_of(base)
    if icodec == S.RLE:   # runs
        strings = [s for s in strings[:128 * 300 // 8] for _ in range(8)]
    col = column_of(strings, rng, 0.1)
    pages, metas = write(col, S.DICT, max_page_size=128 * 100, force_codec=S.DICT, force_index_codec=icodec)
    inner = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[1].tolist())
    assert inner == {icodec}, inner
    preds, lo, hi = all_preds(col)
    check_pages(gpu_ctx, col, pages, metas, preds)


def test_dict_both_sides_of_the_bit_table(gpu_ctx):
    for uniq in (8192, 8193, 20_000):
        vocab = [b"entry-%06d-%s" % (i, b"x" * (i % 23)) for i in range(uniq)]
        rng = np.random.default_rng(uniq)
        idx = np.concatenate([np.arange(uniq), rng.integers(0, uniq, 30_000)])
        rng.shuffle(idx)
        col = column_of([vocab[i] for i in idx], rng, 0.2)
        pages, metas = write(col, S.DICT, max_page_size=col["rows"], force_codec=S.DICT)
        assert metas.shape[0] == 1
        preds, lo, hi = all_preds(col)
        preds += [(op, vocab[k]) for k in (0, 31, 32, 8191, uniq - 1) for op in OPS7]
        strs, valid = check_pages(gpu_ctx, col, pages, metas, preds)
        check_selective(strs, valid, lo, hi)


def test_dict_entries_that_look_like_length_fields(gpu_ctx):
    """strings that hold the pattern the parallel entry finder looks for (four zero bytes: the upper half of a u64 length)
    and empty strings: the entry offsets come from the serial walk"""
    rng = np.random.default_rng(8)
    vocab = [b"", b"\0\0\0\0", b"ab\0\0\0\0cd", b"\x05\0\0\0\0\0\0\0hello", b"\0" * 16, b"x" * 70 + b"\0\0\0\0\0\0\0\0", b"plain"]
    vocab += [b"\x03\0\0\0\0\0\0\0" + bytes([65 + i]) * 3 for i in range(20)]
    strings = [vocab[i] for i in rng.integers(0, len(vocab), 12_000)]
    col = column_of(strings, rng, 0.1)
    preds = [(op, lit) for lit in sorted(set(vocab)) + [b"\0\0\0", b"\x03\0\0\0\0\0\0\0"] for op in OPS7]
    check(gpu_ctx, col, preds, codec=S.DICT, max_page_size=5000, force_codec=S.DICT)


# ---- 5: long pages, an empty column, a one-row page behind others, empty strings only
@pytest.mark.parametrize("name,codec,opt", [CODECS[0], CODECS[4], CODECS[6]], ids=["none", "dict", "freq"])
def test_long_pages(gpu_ctx, name, codec, opt):
    rows = (1 << 18) + 12_345
    if codec == S.FREQ:
        from tests.test_gpu_freq import sparse_bin
        col = sparse_bin(rows, 0.03, 77, null_density=0.1)
    else:
        col = gen.binary(rows, uniq=300, null_density=0.1, zipf=1.3, maxlen=30, seed=4)
    pages, metas = write(col, codec, **opt)
    assert metas.shape[0] == 1
    lits, lo, hi = literals_of(col)
    strs, valid = check_pages(gpu_ctx, col, pages, metas, [(op, lit) for lit in lits[:8] for op in OPS7])
    check_selective(strs, valid, lo, hi)


def test_empty_column_one_row_page_and_empty_strings(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    for ptype in (S.T_BIN32, S.T_BIN64):
        cp = read.ColumnPages(ptype, False, torch.zeros(0, dtype=torch.uint8, device=gpu_ctx.torch_device), np.zeros((0, 2), np.uint64))
        sel = sb.filter_columns(gpu_ctx, [cp, cp], [sb.Predicate("lt", b"abc"), sb.Predicate("starts_with", "")])
        gpu_ctx.synchronize()
        assert all(s.rows == 0 and s.selected == 0 and s.numpy().size == 0 for s in sel)
    for large in (False, True):
        col = gen.binary(2051, uniq=7, large=large, seed=4, maxlen=9)   # a one-row page behind two others
        for opt in (dict(force_codec=S.NONE), dict(force_codec=S.DICT), dict(force_codec=S.LZ4)):
            pages, metas = write(col, None, max_page_size=1025, **opt)
            assert [int(m[1]) for m in np.asarray(metas).tolist()] == [1025, 1025, 1]
            check_pages(gpu_ctx, col, pages, metas, all_preds(col)[0])
        for nd in (None, 0.5):
            for seed in (1, 2, 3):
                col = gen.binary(1, uniq=5, null_density=nd, large=large, seed=seed)
                check(gpu_ctx, col, all_preds(col)[0] + [("is_null", None), ("is_not_null", None)])
        rng = np.random.default_rng(12)
        col = column_of([b""] * 5000, rng, 0.3, large)   # empty strings only
        preds = [(op, lit) for lit in (b"", b"\0", b"a") for op in OPS7]
        for opt in (dict(force_codec=S.NONE), dict(force_codec=S.DICT), dict(force_codec=S.ONEVALUE), dict()):
            strs, valid = check(gpu_ctx, col, preds, max_page_size=2050, **opt)
            assert np.array_equal(expected(strs, valid, "eq", b""), valid) and not expected(strs, valid, "gt", b"").any()
            assert np.array_equal(expected(strs, valid, "starts_with", b""), valid)


# ---- 6: numeric and binary columns in one call; and / or chains that alternate them
def test_mixed_call_and_alternating_chain(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from tests.test_gpu_filter import expected as num_expected, oracle_column
    rows = 10_007   # (the last word holds 23 rows)
    i32 = gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    f64 = gen.prim(S.T_F64, rows, uniq=100, runs=6, seed=2)
    s1 = gen.binary(rows, uniq=60, null_density=0.1, seed=3, maxlen=20)
    s2 = gen.binary(rows, uniq=500, seed=4, large=True, zipf=1.3, maxlen=30)
    plan = ((i32, dict(max_page_size=2050, force_codec=S.RLE), ("lt", 60)),
            (f64, dict(max_page_size=777, force_codec=S.LZ4), ("ge", 30.0)),
            (s1, dict(max_page_size=4100, force_codec=S.DICT), ("ge", sorted(set(strings_of(s1)))[20])),
            (s2, dict(max_page_size=2048, force_codec=S.LZ4), ("starts_with", b"w1")))
    cols, preds, want = [], [], []
    for col, opt, (op, lit) in plan:
        pages, metas = gen.oracle_write(col, **opt)
        cols.append(upload(gpu_ctx, col, pages, metas))
        preds.append(sb.Predicate(op, lit))
        if col["offsets"] is None:
            want.append(num_expected(col, *oracle_column(col, pages, metas), op, lit))
        else:
            want.append(expected(*oracle_strings(col, pages, metas), op, lit))
    assert all(0 < w.sum() < rows for w in want)
    # ONE call: Int32, Float64 and two Utf8 columns
    sels = sb.filter_columns(gpu_ctx, cols, preds)
    gpu_ctx.synchronize()
    for sel, w in zip(sels, want):
        assert np.array_equal(sel.numpy(), w) and sel.selected == int(w.sum())
        assert not np.unpackbits(sel.bitmap.cpu().numpy(), bitorder="little")[rows:].any()

    def state(sel):
        bits = np.unpackbits(sel.bitmap.cpu().numpy(), bitorder="little").astype(bool)
        return bits[:rows], bits[rows:]

    # one selection, one synchronize interval: number set, string and, number or, string and
    sel = sb.filter_columns(gpu_ctx, [cols[0]], [preds[0]])
    sb.filter_columns(gpu_ctx, [cols[2]], [preds[2]], combine="and", out=sel)
    sb.filter_columns(gpu_ctx, [cols[1]], [preds[1]], combine="or", out=sel)
    last = sb.filter_columns(gpu_ctx, [cols[3]], [preds[3]], combine="and", out=sel)
    gpu_ctx.synchronize()
    final = ((want[0] & want[2]) | want[1]) & want[3]
    got, tail = state(sel[0])
    assert np.array_equal(got, final) and not tail.any() and last[0].selected == int(final.sum())
    # string set, number or, string or, number and
    sel = sb.filter_columns(gpu_ctx, [cols[3]], [preds[3]])
    sb.filter_columns(gpu_ctx, [cols[0]], [preds[0]], combine="or", out=sel)
    sb.filter_columns(gpu_ctx, [cols[2]], [preds[2]], combine="or", out=sel)
    last = sb.filter_columns(gpu_ctx, [cols[1]], [preds[1]], combine="and", out=sel)
    gpu_ctx.synchronize()
    final = (want[3] | want[0] | want[2]) & want[1]
    got, tail = state(sel[0])
    assert np.array_equal(got, final) and not tail.any() and last[0].selected == int(final.sum())
    # step by step on a buffer of ones: and / or keep the bits behind the last row, set clears them
    with torch.cuda.stream(gpu_ctx.torch_stream):
        sel[0].bitmap.fill_(0xFF)
    a = sb.filter_columns(gpu_ctx, [cols[2]], [preds[2]], combine="and", out=sel)
    gpu_ctx.synchronize()
    got, tail = state(sel[0])
    assert np.array_equal(got, want[2]) and tail.all() and a[0].selected == int(want[2].sum())
    o = sb.filter_columns(gpu_ctx, [cols[3]], [preds[3]], combine="or", out=sel)
    gpu_ctx.synchronize()
    got, tail = state(sel[0])
    assert np.array_equal(got, want[2] | want[3]) and tail.all() and o[0].selected == int((want[2] | want[3]).sum())
    s = sb.filter_columns(gpu_ctx, [cols[3]], [preds[3]], combine="set", out=sel)
    gpu_ctx.synchronize()
    got, tail = state(sel[0])
    assert np.array_equal(got, want[3]) and not tail.any() and s[0].selected == int(want[3].sum())


def test_mixed_call_with_a_primitive_freq_page(gpu_ctx):
    """a primitive Freq page makes the interval run again with the numeric columns decoded first: the string column of the
    same call gives the same bits"""
    import strawboat_amd as sb
    from tests.test_gpu_filter import expected as num_expected, oracle_column
    from tests.test_gpu_freq import sparse
    rows = 20_000
    f = sparse(S.T_I32, rows, 0.05, 2, null_density=0.1)
    s = gen.binary(rows, uniq=80, null_density=0.1, seed=9, maxlen=16)
    fp, fm = gen.oracle_write(f, max_page_size=5000, force_codec=S.FREQ)
    sp, sm = gen.oracle_write(s, max_page_size=4100, force_codec=S.DICT)
    lit = sorted(set(strings_of(s)))[30]
    wf = num_expected(f, *oracle_column(f, fp, fm), "eq", 7)
    ws = expected(*oracle_strings(s, sp, sm), "lt", lit)
    r0 = gpu_ctx.replays()
    sels = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, f, fp, fm), upload(gpu_ctx, s, sp, sm)], [sb.Predicate("eq", 7), sb.Predicate("lt", lit)])
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    assert np.array_equal(sels[0].numpy(), wf) and sels[0].selected == int(wf.sum())
    assert np.array_equal(sels[1].numpy(), ws) and sels[1].selected == int(ws.sum())


# ---- 7: a read whose launch hint misses, in the same interval as a string filter
def test_string_filter_in_an_interval_that_is_replayed():
    if os.environ.get("SB_NO_HINTS", "0") != "0":
        pytest.skip("SB_NO_HINTS: every kernel is launched, nothing to replay")
    import strawboat_amd as sb
    from strawboat_amd import read
    ctx = sb.Context(0)
    try:
        rle = gen.prim(S.T_F64, 200_000, uniq=50, null_density=0.1, runs=40, seed=5)
        plain = gen.prim(S.T_I64, 200_000, uniq=1 << 40, seed=6)
        flt = gen.binary(100_001, uniq=300, null_density=0.2, seed=7, zipf=1.2, maxlen=24)
        rp, rm = gen.oracle_write(rle, max_page_size=65536, force_codec=S.RLE)
        pp, pm = gen.oracle_write(plain, max_page_size=65536, force_codec=S.NONE)
        c_rle, c_plain = upload(ctx, rle, rp, rm), upload(ctx, plain, pp, pm)
        want_rle, want_plain = gen.oracle_read(rle, rp, rm), gen.oracle_read(plain, pp, pm)
        lit = sorted(set(strings_of(flt)))[100]
        for opt in (dict(force_codec=S.DICT), dict(force_codec=S.LZ4)):
            fp, fm = gen.oracle_write(flt, max_page_size=7001, **opt)
            c_flt = upload(ctx, flt, fp, fm)
            strs, valid = oracle_strings(flt, fp, fm)
            wants = [expected(strs, valid, "le", lit), expected(strs, valid, "starts_with", lit[:3])]
            preds = [sb.Predicate("le", lit), sb.Predicate("starts_with", lit[:3])]
            for _ in range(3):   # read intervals that need neither inflate jobs nor tiles: the next read calls leave those kernels out
                read.read_simple(ctx, c_rle)
            r0 = ctx.replays()
            a1 = read.batch_read_columns(ctx, [c_rle])[0]
            sel = sb.filter_columns(ctx, [c_flt, c_flt], preds)
            a2 = read.batch_read_columns(ctx, [c_plain])[0]   # tiles after all: the interval is issued again, the filter call with it
            ctx.synchronize()
            assert ctx.replays() == r0 + 1
            assert np.array_equal(a1.values_numpy(), want_rle["values"]) and np.array_equal(a2.values_numpy(), want_plain["values"])
            for s, w in zip(sel, wants):
                assert np.array_equal(s.numpy(), w) and s.selected == int(w.sum())
    finally:
        ctx.close()


# ---- 8: stage_capacity
def test_stage_capacity(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    col = gen.binary(20_000, uniq=50, null_density=0.1, seed=11, maxlen=30)
    for codec in (S.LZ4, S.ZSTD, S.SNAPPY):
        pages, metas = write(col, codec, max_page_size=4100, force_codec=codec)
        need = staged_bytes(col, pages, metas)
        assert need == col["values"].size
        cp = upload(gpu_ctx, col, pages, metas)
        lit = sorted(set(strings_of(col)))[25]
        with pytest.raises(NativeError) as e:
            sb.filter_columns(gpu_ctx, [cp], [sb.Predicate("lt", lit)], stage_capacity=[need - 1])
            gpu_ctx.synchronize()
        assert e.value.code == -5, codec
        try:
            gpu_ctx.synchronize()
        except NativeError:
            pass
        # exactly enough, and the default
        check_pages(gpu_ctx, col, pages, metas, [("lt", lit), ("starts_with", lit[:2])], stage_capacity=need)
        check_pages(gpu_ctx, col, pages, metas, [("lt", lit), ("starts_with", lit[:2])])
    # a column the default does not do for: one repeated long string compresses more than 4 x
    rep = column_of([b"the same long string again and again " * 4] * 8000)
    pages, metas = write(rep, S.LZ4, max_page_size=8000, force_codec=S.LZ4)
    need = staged_bytes(rep, pages, metas)
    assert need > 4 * pages.size
    cp = upload(gpu_ctx, rep, pages, metas)
    with pytest.raises(NativeError) as e:
        sb.filter_columns(gpu_ctx, [cp], [sb.Predicate("starts_with", b"the same")])
        gpu_ctx.synchronize()
    assert e.value.code == -5
    try:
        gpu_ctx.synchronize()
    except NativeError:
        pass
    check_pages(gpu_ctx, rep, pages, metas, [("starts_with", b"the same"), ("gt", b"the same")], stage_capacity=need)


# ---- 9: corrupt pages
def test_corrupt_pages_raise_what_the_decoder_raises(gpu_ctx):
    import strawboat_amd as sb
    from tests.test_gpu_filter import filter_code, read_code
    pred = sb.Predicate("lt", b"w5")
    # a truncated last page
    for codec in (S.NONE, S.DICT, S.LZ4):
        col = gen.binary(9000, uniq=60, null_density=0.1, seed=codec)
        pages, metas = gen.oracle_write(col, max_page_size=3000, force_codec=codec)
        m = np.array(metas, np.uint64).copy()
        cut = int(m[-1, 0]) // 2
        m[-1, 0] -= cut
        cp = upload(gpu_ctx, col, pages[:pages.size - cut].copy(), m)
        want = read_code(gpu_ctx, cp)
        assert want != 0
        assert filter_code(gpu_ctx, cp, pred) == want, codec
    # a Dict page with an index >= D: plain u32 indices behind hdr9 Dict | hdr9 None
    for uniq in (50, 20_000):   # the bit table in LDS and in HBM
        vocab = [b"v%05d" % i for i in range(uniq)]
        rng = np.random.default_rng(uniq)
        idx = np.concatenate([np.arange(uniq), rng.integers(0, uniq, 40_000 - uniq)])
        col = column_of([vocab[i] for i in idx])
        pages, metas = gen.oracle_write(col, max_page_size=40_000, force_codec=S.DICT, force_index_codec=S.NONE)
        assert metas.shape[0] == 1
        bad = pages.copy()
        pos = 9 + 9 + 25_000 * 4
        bad[pos:pos + 4] = np.frombuffer(np.uint32(1 << 30).tobytes(), np.uint8)
        cp = upload(gpu_ctx, col, bad, metas)
        want = read_code(gpu_ctx, cp)
        assert want == -1
        assert filter_code(gpu_ctx, cp, pred) == want
    # the context still works
    col = gen.binary(9000, uniq=60)
    check(gpu_ctx, col, all_preds(col)[0], max_page_size=3000, force_codec=S.DICT)


# ---- 10: refusals through raw ctypes
def raw_var(ctx, col, cp, op, literal, fill=0xA5, ptype=None):
    import torch
    from strawboat_amd import _native as N
    m = cp.metas_array()
    arr = (N.ColumnFilterVarC * 1)()
    c = arr[0]
    c.physical_type, c.is_nullable = col["ptype"] if ptype is None else ptype, 0
    c.pages, c.pages_len = cp.pages.data_ptr(), cp.pages.numel()
    c.metas, c.n_pages = m.ctypes.data_as(C.POINTER(N.PageMetaC)), m.shape[0]
    c.op, c.combine = op, N.SB_SEL_SET
    buf = C.create_string_buffer(literal, max(1, len(literal)))
    c.literal, c.literal_len = C.addressof(buf), len(literal)
    bitmap = torch.full((((col["rows"] + 31) // 32) * 4,), fill, dtype=torch.uint8, device=ctx.torch_device)
    c.selection, c.selection_capacity = bitmap.data_ptr(), bitmap.numel()
    return arr, bitmap, (m, buf)


def test_refusals_at_the_call(gpu_ctx):
    from strawboat_amd import _native as N
    lib, h = gpu_ctx._lib, gpu_ctx._h
    cases = []
    for col, op, lit, code in ((gen.boolean(3000), N.SB_PRED_LT, b"\1", N.SB_ERR_NYI),
                               (gen.prim(S.T_I128, 3000, uniq=10), N.SB_PRED_EQ, b"\0" * 16, N.SB_ERR_NYI),
                               (gen.prim(S.T_I32, 3000, uniq=10), N.SB_PRED_STARTS_WITH, b"\1\0\0\0", N.SB_ERR_INVALID),
                               (gen.prim(S.T_I32, 3000, uniq=10), N.SB_PRED_LT, b"\1\0\0", N.SB_ERR_INVALID),       # not the type's width
                               (gen.prim(S.T_I32, 3000, uniq=10), N.SB_PRED_LT, b"\1\0\0\0\0\0\0\0", N.SB_ERR_INVALID),
                               (gen.binary(3000, uniq=10), 9, b"a", N.SB_ERR_INVALID)):                              # no such op
        pages, metas = gen.oracle_write(col)
        cp = upload(gpu_ctx, col, pages, metas)
        arr, bitmap, keep = raw_var(gpu_ctx, col, cp, op, lit)
        assert lib.sb_filter_columns_var(h, arr, 1, N.SB_MEM_DEVICE) == code, (col["ptype"], op)
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        assert (bitmap.cpu().numpy() == 0xA5).all(), "the selection must stay untouched"
        cases.append(keep)
    # SB_MEM_HOST
    col = gen.binary(3000, uniq=10)
    pages, metas = gen.oracle_write(col)
    cp = upload(gpu_ctx, col, pages, metas)
    strs, valid = oracle_strings(col, pages, metas)
    lit = max(sorted(set(strs)), key=strs.count)   # a value of the column
    arr, bitmap, keep = raw_var(gpu_ctx, col, cp, N.SB_PRED_EQ, lit)
    assert lib.sb_filter_columns_var(h, arr, 1, N.SB_MEM_HOST) == N.SB_ERR_NYI
    gpu_ctx.synchronize()
    assert (bitmap.cpu().numpy() == 0xA5).all()
    # ... and the same descriptor is served with SB_MEM_DEVICE
    assert lib.sb_filter_columns_var(h, arr, 1, N.SB_MEM_DEVICE) == 0
    gpu_ctx.synchronize()
    want = expected(strs, np.ones(len(strs), bool), "eq", lit)
    assert arr[0].rows == 3000 and arr[0].selected == int(want.sum()) > 0
    assert np.array_equal(unpack(bitmap.cpu().numpy(), 3000), want)
    # the old entry point keeps refusing binary comparisons
    arr_old = (N.ColumnFilterC * 1)()
    c = arr_old[0]
    m = cp.metas_array()
    c.physical_type, c.is_nullable = col["ptype"], 0
    c.pages, c.pages_len = cp.pages.data_ptr(), cp.pages.numel()
    c.metas, c.n_pages = m.ctypes.data_as(C.POINTER(N.PageMetaC)), m.shape[0]
    c.op, c.combine = N.SB_PRED_EQ, N.SB_SEL_SET
    bitmap.fill_(0xA5)
    c.selection, c.selection_capacity = bitmap.data_ptr(), bitmap.numel()
    assert lib.sb_filter_columns(h, arr_old, 1, N.SB_MEM_DEVICE) == N.SB_ERR_NYI
    gpu_ctx.synchronize()
    assert (bitmap.cpu().numpy() == 0xA5).all()
