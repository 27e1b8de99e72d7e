"""sb_filter_columns_in on the GPU: pages written by the CPU oracle, searched on the device, compared with numpy's
`OR over the literals of np.equal(oracle_read(pages).values, literal) & validity` (NOT IN: `validity & ~that`), binary
columns with Python's own `bytes` equality on the oracle's decode.  Nothing here is compared with what the device's own
decoder gives; every row, `selected` and the bits behind the last row are compared in every case."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import sbo as S
from tests import gen
from tests.test_gpu_decode import LONG_RLE_ROWS, RLE_WIDTHS, _rle_hand_built_column, _rle_long_page
from tests.test_gpu_filter import CMP_TYPES, NP, expected as cmp_expected, hand_built, oracle_column, read_code, upload
from tests.test_gpu_filter_binary import column_of, oracle_strings, strings_of
from tests.test_gpu_filter_binary import write as write_bin

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


# ---- the reference
def want_in(col, vals, valid, lits, negate):
    hit = np.zeros(valid.size, bool)
    with np.errstate(invalid="ignore"):
        for lit in lits:
            hit |= np.equal(vals, NP[col["ptype"]](lit))
    hit &= valid
    return valid & ~hit if negate else hit


def want_in_bin(strs, valid, lits, negate):
    have = set(x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in lits)
    hit = np.fromiter((s in have for s in strs), bool, len(strs)) & valid   # (`in` of a set of bytes: bytes equality)
    return valid & ~hit if negate else hit


def compare(sel, want, what="", counted=None):
    """every row of the bitmap, and `selected` of the call that wrote it last (`counted`: that call's Selection when it is
    not `sel` itself, as in a chain on one buffer)"""
    got = sel.numpy()
    assert sel.rows == want.size
    assert np.array_equal(got, want), "%s: %d rows differ, first at %d" % (what, int((got != want).sum()), int(np.argmax(got != want)))
    counted = sel if counted is None else counted
    assert counted.selected == int(want.sum()), (what, counted.selected, int(want.sum()))


def tail_of(sel):
    return np.unpackbits(sel.bitmap.cpu().numpy(), bitorder="little")[sel.rows:]


def check_pages(ctx, col, pages, metas, lists, **kw):
    """lists: (literals, negate) pairs, all over the same pages in ONE call (one column entry per list), combine = set"""
    import strawboat_amd as sb
    binary = col["ptype"] in (S.T_BIN32, S.T_BIN64)
    vals, valid = oracle_strings(col, pages, metas) if binary else oracle_column(col, pages, metas)
    cp = upload(ctx, col, pages, metas)
    sels = sb.filter_in(ctx, [cp] * len(lists), [sb.InList(lits, negate=neg) for lits, neg in lists], **kw)
    ctx.synchronize()
    for (lits, neg), sel in zip(lists, sels):
        want = want_in_bin(vals, valid, lits, neg) if binary else want_in(col, vals, valid, lits, neg)
        compare(sel, want, "%s of %d literals" % ("NOT IN" if neg else "IN", len(lits)))
        assert not tail_of(sel).any(), "bits behind the last row must be 0 after set"
    return vals, valid


def check(ctx, col, lists, codec=None, **opt):
    pages, metas = gen.oracle_write(col, **opt)
    if codec is not None:
        seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
        assert seen == {codec}, (seen, codec)
    return check_pages(ctx, col, pages, metas, lists)


def both(lits):
    return [(lits, False), (lits, True)]


def make_list(rng, values, n, ptype):
    """n literals: the column's minimum and maximum, one value below all of them and one above (where the type has one), half
    of the rest from the column's values and half from outside, with duplicates, shuffled"""
    dt = NP[ptype]
    v = np.unique(values)
    info = np.iinfo(dt) if np.issubdtype(dt, np.integer) else None
    lo, hi = v[0].item(), v[-1].item()
    if info is not None:
        edge = [lo, hi] + ([lo - 1] if lo > info.min else []) + ([hi + 1] if hi < info.max else [])
    else:
        edge = [lo, hi, lo - 1.0, hi + 1.0]
    edge = edge[:n]
    rest = n - len(edge)
    inside = [v[int(i)].item() for i in rng.integers(0, v.size, rest // 2)]
    outside = []
    present = set(v.tolist())
    while len(outside) < rest - len(inside):
        if info is not None:
            x = int(rng.integers(max(info.min, lo - 5000), min(info.max, hi + 5000), endpoint=True))
        else:
            x = float(dt(rng.normal(0, 1000) + 0.123))
        if x not in present:
            outside.append(x)
    lits = edge + inside + outside
    for _ in range(n // 8):   # duplicates
        lits[int(rng.integers(0, n))] = lits[int(rng.integers(0, n))]
    for need in edge:   # (a duplicate may have replaced one of them)
        if need not in lits:
            lits[int(rng.integers(0, n))] = need
    for i, need in enumerate(edge):
        if need not in lits:
            lits[i] = need
    order = rng.permutation(n)
    return [lits[int(i)] for i in order]


# ---- 1: list sizes and edges
LIST_SIZES = [0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024]


@pytest.fixture(scope="module")
def sizes_column():
    """the Int64 column of the list-size cases, its pages per codec and the oracle's decode of each: made once"""
    col = gen.prim(S.T_I64, 10_000, uniq=3000, null_density=0.1, runs=3, seed=11)
    out = {}
    for codec in (S.NONE, S.RLE, S.DICT):
        pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
        out[codec] = (pages, metas, oracle_column(col, pages, metas))
    return col, out


@pytest.mark.parametrize("n", LIST_SIZES)
def test_list_sizes(gpu_ctx, sizes_column, n):
    import strawboat_amd as sb
    col, by_codec = sizes_column
    rng = np.random.default_rng(1000 + n)
    lits = make_list(rng, col["values"], n, S.T_I64)
    assert len(lits) == n
    if n >= 4:
        v = col["values"]
        assert v.min() in lits and v.max() in lits and v.min() - 1 in lits and v.max() + 1 in lits
    if n >= 63:
        assert len(set(lits)) < n, "the list has duplicates"
    for codec, (pages, metas, (vals, valid)) in by_codec.items():
        cp = upload(gpu_ctx, col, pages, metas)
        sels = sb.filter_in(gpu_ctx, [cp, cp], [sb.InList(lits), sb.InList(lits, negate=True)])
        gpu_ctx.synchronize()
        for sel, neg in zip(sels, (False, True)):
            want = want_in(col, vals, valid, lits, neg)
            compare(sel, want, "codec %d n %d negate %r" % (codec, n, neg))
            assert not tail_of(sel).any()
        w_in = want_in(col, vals, valid, lits, False)
        if n == 0:
            assert not w_in.any() and np.array_equal(want_in(col, vals, valid, lits, True), valid)
        elif n >= 63:
            assert 0 < w_in.sum() < valid.sum()   # neither constant answer can pass


# ---- 2: codecs x types
def lists_of(col, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for n in (5, 100):
        out += both(make_list(rng, col["values"], n, col["ptype"]))
    return out


@pytest.mark.parametrize("ptype", CMP_TYPES)
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT, S.ONEVALUE])
def test_prim_codecs(gpu_ctx, ptype, codec):
    uniq = 1 if codec == S.ONEVALUE else 100
    for nd, page in ((0.2, 2050), (None, 4100), (0.2, 777), (None, 2048)):
        col = gen.prim(ptype, 10_000, uniq=uniq, null_density=nd, runs=8 if nd else 3, seed=page)
        lists = lists_of(col, page)
        vals, valid = check(gpu_ctx, col, lists, codec=codec, max_page_size=page, force_codec=codec)
        assert want_in(col, vals, valid, lists[0][0], False).any()   # (the minimum is in every list)


@pytest.mark.parametrize("ptype", [S.T_I32, S.T_U32])
@pytest.mark.parametrize("codec", [S.BITPACK, S.DELTABP])
def test_bitpacking(gpu_ctx, ptype, codec):
    col = gen.prim(ptype, 128 * 100, uniq=1 << 13, sorted_=(codec == S.DELTABP))
    check(gpu_ctx, col, lists_of(col), codec=codec, max_page_size=128 * 40, force_codec=codec)


@pytest.mark.parametrize("ptype", [S.T_I16, S.T_I64, S.T_F64])
@pytest.mark.parametrize("codec", [S.LZ4, S.ZSTD, S.SNAPPY])
def test_basic_pages_are_staged(gpu_ctx, ptype, codec):
    col = gen.prim(ptype, 10_000, uniq=300, null_density=0.2, runs=5, seed=codec)
    check(gpu_ctx, col, lists_of(col), codec=codec, max_page_size=2050, force_codec=codec)


def test_patas_pages(gpu_ctx):
    rng = np.random.default_rng(3)
    v = np.round(rng.normal(100, 20, 10_000), 1)
    col = dict(ptype=S.T_F64, nullable=True, rows=v.size, values=v, validity=gen.make_validity(rng, v.size, 0.2), offsets=None)
    check(gpu_ctx, col, lists_of(col), codec=S.PATAS, max_page_size=2050, force_codec=S.PATAS)


@pytest.mark.parametrize("icodec", [S.NONE, S.RLE, S.BITPACK, S.DELTABP, S.ONEVALUE, S.LZ4])
def test_dict_index_codecs(gpu_ctx, icodec):
    uniq = 1 if icodec == S.ONEVALUE else 200
    col = gen.prim(S.T_F64, 128 * 80, uniq=uniq, null_density=0.1, runs=16, sorted_=(icodec == S.DELTABP))
    check(gpu_ctx, col, lists_of(col), codec=S.DICT, max_page_size=128 * 30, force_codec=S.DICT, force_index_codec=icodec)


def test_dict_both_sides_of_the_bit_table(gpu_ctx):
    for uniq, rows in ((8000, 60_000), (8192 * 4, 70_000)):
        col = gen.prim(S.T_I64, rows, uniq=uniq, null_density=0.2, seed=uniq)
        pages, metas = gen.oracle_write(col, max_page_size=rows, force_codec=S.DICT)
        d = np.unique(col["values"]).size
        assert (d <= 8192) == (uniq == 8000), d
        check_pages(gpu_ctx, col, pages, metas, lists_of(col, uniq))


@pytest.mark.parametrize("ptype", [S.T_U8, S.T_I32, S.T_I64, S.T_F64])
def test_freq_pages_are_replayed(gpu_ctx, ptype):
    from tests.test_gpu_freq import sparse
    col = sparse(ptype, 10_000, 0.05, 2, null_density=0.1)
    r0 = gpu_ctx.replays()
    lists = lists_of(col) + both([7]) + both([])
    check(gpu_ctx, col, lists, codec=S.FREQ, max_page_size=2050, force_codec=S.FREQ)
    assert gpu_ctx.replays() == r0 + 1, "a primitive Freq page asks for the replay"


@pytest.mark.parametrize("ptype,dtype,w", RLE_WIDTHS)
def test_rle_hand_built_pages(gpu_ctx, ptype, dtype, w):
    col, pages, metas = hand_built(ptype, *_rle_hand_built_column(w, dtype))
    check_pages(gpu_ctx, col, pages, metas, lists_of(col))


def test_one_long_rle_page(gpu_ctx):
    col, pages, metas = hand_built(S.T_I64, [_rle_long_page()], [LONG_RLE_ROWS])
    if col is None:   # the oracle's values or the oracle's refusal, never a difference
        cp = upload(gpu_ctx, dict(ptype=S.T_I64, nullable=False), pages, metas)
        assert in_code(gpu_ctx, cp, [0]) != 0
    else:
        check_pages(gpu_ctx, col, pages, metas, lists_of(col))


# ---- 3: floats
@pytest.mark.parametrize("ptype", [S.T_F32, S.T_F64])
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_float_specials(gpu_ctx, ptype, codec):
    rng = np.random.default_rng(9)
    nan, inf = float("nan"), float("inf")
    pool = np.array([nan, 0.0, -0.0, inf, -inf, 1.5, -2.25, 3e30], NP[ptype])
    v = np.repeat(pool[rng.integers(0, pool.size, 3000)], 3)
    col = dict(ptype=ptype, nullable=True, rows=v.size, values=v, validity=gen.make_validity(rng, v.size, 0.2), offsets=None)
    lists = []
    for lits in ([nan], [nan, nan], [0.0], [-0.0], [nan, -0.0, 1.5], [inf, -inf], [3e30, -2.25, nan, 0.0], [-inf, 7.0], []):
        lists += both(lits)
    vals, valid = check(gpu_ctx, col, lists, max_page_size=2050, force_codec=codec)
    isnan = np.isnan(vals) & valid
    assert isnan.any()
    for lits, _ in lists:
        assert not (want_in(col, vals, valid, lits, False) & isnan).any()               # a NaN row is never IN
        assert np.array_equal(want_in(col, vals, valid, lits, True) & isnan, isnan)     # ... and always NOT IN
    zeros = (vals == 0) & valid
    assert np.signbit(vals[zeros]).any() and not np.signbit(vals[zeros]).all()
    assert np.array_equal(want_in(col, vals, valid, [-0.0], False), zeros) and np.array_equal(want_in(col, vals, valid, [0.0], False), zeros)
    for neg in (False, True):   # a NaN-only list behaves like the empty list
        assert np.array_equal(want_in(col, vals, valid, [nan], neg), want_in(col, vals, valid, [], neg))


# ---- 4: signedness
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_signedness_comes_from_the_physical_type(gpu_ctx, codec):
    rng = np.random.default_rng(10)
    b = np.concatenate([np.arange(256), rng.integers(0, 256, 3744)]).astype(np.uint8)   # all 256 byte values
    b = np.repeat(b, 2)
    for ptype, lits in ((S.T_I8, [-128, -1, 0, 127, -100]), (S.T_U8, [0x80, 0xFF, 0, 127, 156])):
        col = dict(ptype=ptype, nullable=False, rows=b.size, values=b.view(NP[ptype]), validity=None, offsets=None)
        info = np.iinfo(NP[ptype])
        every = list(range(info.min, info.max + 1))
        vals, valid = check(gpu_ctx, col, both(lits) + both(every[::2]) + both(every), max_page_size=777, force_codec=codec)
        assert want_in(col, vals, valid, every, False).all()
    v = np.repeat(rng.integers(-1000, 1000, 3000), 2).astype(np.int64)
    v[::97] = I64_MIN
    v[5::89] = -1
    v[7::83] = I64_MAX
    col = dict(ptype=S.T_I64, nullable=False, rows=v.size, values=v, validity=None, offsets=None)
    vals, valid = check(gpu_ctx, col, both([I64_MIN, -1]) + both([I64_MAX, 0, I64_MIN]) + both([-1]), max_page_size=2050, force_codec=codec)
    assert want_in(col, vals, valid, [I64_MIN], False).sum() > 0
    u = np.repeat(rng.integers(0, 1000, 3000), 2).astype(np.uint64)
    u[::97] = 1 << 63
    u[5::89] = (1 << 64) - 1
    u[7::83] = (1 << 63) - 1
    col = dict(ptype=S.T_U64, nullable=False, rows=u.size, values=u, validity=None, offsets=None)
    vals, valid = check(gpu_ctx, col, both([1 << 63, (1 << 64) - 1]) + both([(1 << 63) - 1, 5]) + both([(1 << 64) - 1]), max_page_size=2050,
                        force_codec=codec)
    assert want_in(col, vals, valid, [1 << 63], False).sum() > 0


# ---- 5: binary
SHARED8 = b"prefix08"
SHARED16 = b"prefix08prefix16"
BIN_VALUES = [b"", b"a", b"ab", b"abc", b"abcd", b"1234567", b"12345678", b"123456789", b"x" * 40, SHARED8 + b"A", SHARED8 + b"B", SHARED8,
              SHARED16 + b"A", SHARED16 + b"B", SHARED16, b"\xff\x00", b"\x00", b"\x00\x00", b"Z\xc3\xbcrich", b"y" * 39 + b"z"]
BIN_LISTS = [
    [b""],
    [b"a", b"ab", b"abc"],
    [b"a"], [b"1234567"], [b"12345678"], [b"123456789"], [b"x" * 40],                  # lengths 1, 7, 8, 9 and 40
    [SHARED8 + b"A", SHARED8 + b"C", SHARED8],                                          # literals sharing their first 8 bytes
    [SHARED16 + b"B", SHARED16 + b"C", SHARED16 + b"\x00"],                             # ... and their first 16
    [b"abc", b"", b"x" * 40, b"absent", b"abc", "Zürich", SHARED16, b"\x00", b"x" * 41, b"y" * 39 + b"z", b"12345678"],
    [b"absent", b"abcde", b"\xff"],
    [],
]
BIN_CODECS = [("none", S.NONE, dict(force_codec=S.NONE)), ("lz4", S.LZ4, dict(force_codec=S.LZ4)), ("zstd", S.ZSTD, dict(force_codec=S.ZSTD)),
              ("snappy", S.SNAPPY, dict(force_codec=S.SNAPPY)), ("dict", S.DICT, dict(force_codec=S.DICT)),
              ("onevalue", S.ONEVALUE, dict(force_codec=S.ONEVALUE)), ("freq", S.FREQ, dict(force_codec=S.FREQ))]


def bin_column(codec, large, nd, seed):
    rng = np.random.default_rng(seed)
    n = 10_000
    if codec == S.ONEVALUE:
        idx = np.full(n, int(rng.integers(0, len(BIN_VALUES))))
    elif codec == S.FREQ:   # one frequent value, the others rare
        idx = np.where(rng.random(n) < 0.95, 3, rng.integers(0, len(BIN_VALUES), n))
    else:
        idx = np.repeat(rng.integers(0, len(BIN_VALUES), n // 4 + 1), 4)[:n]
    return column_of([BIN_VALUES[int(i)] for i in idx], rng, nd, large)


@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
@pytest.mark.parametrize("name,codec,opt", BIN_CODECS, ids=[c[0] for c in BIN_CODECS])
def test_binary_codecs(gpu_ctx, large, name, codec, opt):
    lists = [p for lits in BIN_LISTS for p in both(lits)]
    for nd, page in ((0.2, 2050), (None, 4100), (0.2, 777), (None, 2048)):
        col = bin_column(codec, large, nd, seed=page)
        pages, metas = write_bin(col, codec, max_page_size=page, **opt)
        strs, valid = check_pages(gpu_ctx, col, pages, metas, lists)
        if codec != S.ONEVALUE:
            w = want_in_bin(strs, valid, BIN_LISTS[1], False)
            assert 0 < w.sum() < valid.sum()
            assert want_in_bin(strs, valid, [b""], False).any()


def test_binary_long_lists_and_big_dictionaries(gpu_ctx):
    """1024 literals against dictionaries on both sides of the LDS bit table"""
    rng = np.random.default_rng(77)
    for uniq, rows in ((3000, 20_000), (12_000, 40_000)):
        col = gen.binary(rows, uniq=uniq, null_density=0.1, seed=uniq, maxlen=24)
        have = sorted(set(strings_of(col)))
        assert (len(have) <= 8192) == (uniq == 3000)
        lits = [have[int(i)] for i in rng.integers(0, len(have), 600)] + [bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8))
                                                                           for _ in range(424)]
        pages, metas = write_bin(col, S.DICT, max_page_size=rows, force_codec=S.DICT)
        strs, valid = check_pages(gpu_ctx, col, pages, metas, both(lits) + both(lits[:65]))
        assert 0 < want_in_bin(strs, valid, lits, False).sum() < valid.sum()


# ---- 6: combine and chains
def state(sel):
    bits = np.unpackbits(sel.bitmap.cpu().numpy(), bitorder="little").astype(bool)
    return bits[:sel.rows], bits[sel.rows:]


@pytest.fixture(scope="module")
def chain_columns():
    rows = 10_007   # (the last word holds 23 rows)
    a = gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    b = gen.prim(S.T_F64, rows, uniq=100, runs=6, seed=2)
    s = gen.binary(rows, uniq=50, null_density=0.1, seed=3, maxlen=20)
    ap, am = gen.oracle_write(a, max_page_size=2050, force_codec=S.RLE)
    bp, bm = gen.oracle_write(b, max_page_size=777, force_codec=S.DICT)
    sp, sm = gen.oracle_write(s, max_page_size=4100, force_codec=S.DICT)
    return rows, (a, ap, am, oracle_column(a, ap, am)), (b, bp, bm, oracle_column(b, bp, bm)), (s, sp, sm, oracle_strings(s, sp, sm))


def test_combine_modes_chained_with_comparison_calls(gpu_ctx, chain_columns):
    import torch
    import strawboat_amd as sb
    rows, (a, ap, am, (av, avalid)), (b, bp, bm, (bv, bvalid)), (s, sp, sm, (strs, svalid)) = chain_columns
    ca, cb, cs = upload(gpu_ctx, a, ap, am), upload(gpu_ctx, b, bp, bm), upload(gpu_ctx, s, sp, sm)
    la = [int(x) for x in np.unique(av)[::3]]
    ls = sorted(set(strs))[::2]
    w_in_a = want_in(a, av, avalid, la, False)
    w_notin_a = want_in(a, av, avalid, la, True)
    w_ge_b = cmp_expected(b, bv, bvalid, "ge", 30.0)
    w_in_s = want_in_bin(strs, svalid, ls, False)
    assert 0 < w_in_a.sum() < avalid.sum() and 0 < w_in_s.sum() < svalid.sum()
    # one synchronize interval: comparison set, IN and, NOT IN or / IN set, comparison and, IN or
    sel = sb.filter_columns(gpu_ctx, [cb], [sb.Predicate("ge", 30.0)])
    sb.filter_in(gpu_ctx, [ca], [sb.InList(la)], combine="and", out=sel)
    last = sb.filter_in(gpu_ctx, [cs], [sb.InList(ls, negate=True)], combine="or", out=sel)
    gpu_ctx.synchronize()
    final = (w_ge_b & w_in_a) | want_in_bin(strs, svalid, ls, True)
    got, tail = state(sel[0])
    assert np.array_equal(got, final) and not tail.any() and last[0].selected == int(final.sum())
    sel = sb.filter_in(gpu_ctx, [cs], [sb.InList(ls)])
    sb.filter_columns(gpu_ctx, [cb], [sb.Predicate("ge", 30.0)], combine="and", out=sel)
    last = sb.filter_in(gpu_ctx, [ca], [sb.InList(la, negate=True)], combine="or", out=sel)
    gpu_ctx.synchronize()
    final = (w_in_s & w_ge_b) | w_notin_a
    got, tail = state(sel[0])
    assert np.array_equal(got, final) and not tail.any() and last[0].selected == int(final.sum())
    # step by step, the buffer pre-filled with ones: set clears the bits behind the last row, and / or keep them
    with torch.cuda.stream(gpu_ctx.torch_stream):
        sel[0].bitmap.fill_(0xFF)
    s1 = sb.filter_in(gpu_ctx, [ca], [sb.InList(la)], combine="and", out=sel)
    gpu_ctx.synchronize()
    got, tail = state(sel[0])
    assert np.array_equal(got, w_in_a) and tail.all() and s1[0].selected == int(w_in_a.sum())
    s2 = sb.filter_in(gpu_ctx, [cs], [sb.InList(ls)], combine="or", out=sel)
    gpu_ctx.synchronize()
    got, tail = state(sel[0])
    assert np.array_equal(got, w_in_a | w_in_s) and tail.all() and s2[0].selected == int((w_in_a | w_in_s).sum())
    s0 = sb.filter_in(gpu_ctx, [ca], [sb.InList(la, negate=True)], combine="set", out=sel)
    gpu_ctx.synchronize()
    got, tail = state(sel[0])
    assert np.array_equal(got, w_notin_a) and not tail.any() and s0[0].selected == int(w_notin_a.sum())
    # an empty list under and / or: IN clears / keeps everything, NOT IN is the validity
    for neg, mode, fn in ((False, "and", lambda x: x & False), (False, "or", lambda x: x), (True, "and", lambda x: x & avalid), (True, "or", lambda x: x | avalid)):
        sel = sb.filter_columns(gpu_ctx, [cb], [sb.Predicate("ge", 30.0)])
        last = sb.filter_in(gpu_ctx, [ca], [sb.InList([], negate=neg)], combine=mode, out=sel)
        gpu_ctx.synchronize()
        compare(sel[0], fn(w_ge_b), "empty list %r %s" % (neg, mode), counted=last[0])


def test_numeric_and_binary_columns_in_one_call(gpu_ctx, chain_columns):
    import strawboat_amd as sb
    rows, (a, ap, am, (av, avalid)), (b, bp, bm, (bv, bvalid)), (s, sp, sm, (strs, svalid)) = chain_columns
    ca, cb, cs = upload(gpu_ctx, a, ap, am), upload(gpu_ctx, b, bp, bm), upload(gpu_ctx, s, sp, sm)
    la, lb, ls = [int(x) for x in np.unique(av)[::3]], [float(x) for x in np.unique(bv)[::2]], sorted(set(strs))[::2]
    sels = sb.filter_in(gpu_ctx, [cs, ca, cs, cb], [sb.InList(ls), sb.InList(la, negate=True), sb.InList(ls, negate=True), sb.InList(lb)])
    gpu_ctx.synchronize()
    compare(sels[0], want_in_bin(strs, svalid, ls, False), "binary in")
    compare(sels[1], want_in(a, av, avalid, la, True), "i32 not in")
    compare(sels[2], want_in_bin(strs, svalid, ls, True), "binary not in")
    compare(sels[3], want_in(b, bv, bvalid, lb, False), "f64 in")
    assert not any(tail_of(x).any() for x in sels)


def test_mixed_call_with_a_primitive_freq_page(gpu_ctx, chain_columns):
    """the numeric column is replayed through the staging area, the binary column of the same call is issued again as it was"""
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows, _, _, (s, sp, sm, (strs, svalid)) = chain_columns
    f = sparse(S.T_I32, rows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    fv, fvalid = oracle_column(f, fp, fm)
    lf, ls = [7, int(fv[0]), 123456], sorted(set(strs))[::2]
    r0 = gpu_ctx.replays()
    for mode in ("and", "or"):
        sel = sb.filter_in(gpu_ctx, [upload(gpu_ctx, s, sp, sm)], [sb.InList(ls)])
        last = sb.filter_in(gpu_ctx, [upload(gpu_ctx, f, fp, fm)], [sb.InList(lf, negate=True)], combine=mode, out=sel)
        gpu_ctx.synchronize()
        w1, w2 = want_in_bin(strs, svalid, ls, False), want_in(f, fv, fvalid, lf, True)
        want = w1 & w2 if mode == "and" else w1 | w2
        compare(sel[0], want, mode, counted=last[0])
    sels = sb.filter_in(gpu_ctx, [upload(gpu_ctx, s, sp, sm), upload(gpu_ctx, f, fp, fm)], [sb.InList(ls, negate=True), sb.InList(lf)])
    gpu_ctx.synchronize()
    compare(sels[0], want_in_bin(strs, svalid, ls, True), "binary beside freq")
    compare(sels[1], want_in(f, fv, fvalid, lf, False), "freq")
    assert gpu_ctx.replays() == r0 + 3


def test_selected_read_and_aggregate_on_the_bitmap_in_one_interval(gpu_ctx, chain_columns):
    import strawboat_amd as sb
    rows, (a, ap, am, (av, avalid)), (b, bp, bm, (bv, bvalid)), _ = chain_columns
    ca, cb = upload(gpu_ctx, a, ap, am), upload(gpu_ctx, b, bp, bm)
    la = [int(x) for x in np.unique(av)[::3]]
    sel = sb.filter_in(gpu_ctx, [ca], [sb.InList(la)])
    got = sb.read_selected(gpu_ctx, [cb], sel[0])
    agg = sb.aggregate_columns(gpu_ctx, [cb], sel[0])
    gpu_ctx.synchronize()
    want = want_in(a, av, avalid, la, False)
    compare(sel[0], want)
    vals, validity = got[0].numpy()
    assert got[0].selected == int(want.sum()) and validity is None
    assert np.array_equal(vals, bv[want])
    live = bv[want & bvalid]
    assert agg[0].selected == int(want.sum()) and agg[0].count == live.size
    assert agg[0].min == live.min() and agg[0].max == live.max()


def test_in_an_interval_that_is_replayed():
    """the hint-miss construction of the comparison suite: reads whose hints leave kernels out, then a read that needs them"""
    if os.environ.get("SB_NO_HINTS", "0") != "0":
        pytest.skip("SB_NO_HINTS: every kernel is launched, nothing to replay")
    import strawboat_amd as sb
    from strawboat_amd import read
    ctx = sb.Context(0)
    try:
        rle = gen.prim(S.T_F64, 200_000, uniq=50, null_density=0.1, runs=40, seed=5)
        plain = gen.prim(S.T_I64, 200_000, uniq=1 << 40, seed=6)
        flt = gen.prim(S.T_I32, 100_001, uniq=300, null_density=0.2, runs=5, seed=7)
        txt = gen.binary(20_001, uniq=60, null_density=0.1, seed=8, maxlen=20)
        rp, rm = gen.oracle_write(rle, max_page_size=65536, force_codec=S.RLE)
        pp, pm = gen.oracle_write(plain, max_page_size=65536, force_codec=S.NONE)
        fp, fm = gen.oracle_write(flt, max_page_size=7001, force_codec=S.DICT)
        tp, tm = gen.oracle_write(txt, max_page_size=7001, force_codec=S.DICT)
        c_rle, c_plain, c_flt, c_txt = upload(ctx, rle, rp, rm), upload(ctx, plain, pp, pm), upload(ctx, flt, fp, fm), upload(ctx, txt, tp, tm)
        want_rle, want_plain = gen.oracle_read(rle, rp, rm), gen.oracle_read(plain, pp, pm)
        fv, fvalid = oracle_column(flt, fp, fm)
        strs, svalid = oracle_strings(txt, tp, tm)
        lf, lt = [int(x) for x in np.unique(fv)[::4]], sorted(set(strs))[::3]
        w_set, w_not, w_txt = want_in(flt, fv, fvalid, lf, False), want_in(flt, fv, fvalid, lf, True), want_in_bin(strs, svalid, lt, False)

        def same(arr, want):
            return np.array_equal(arr.values_numpy(), want["values"]) and (arr.validity is None or np.array_equal(arr.validity_numpy(), want["validity"]))

        for _ in range(3):
            read.read_simple(ctx, c_rle)
        r0 = ctx.replays()
        sel = sb.filter_in(ctx, [c_flt], [sb.InList(lf)])
        ctx.synchronize()
        assert ctx.replays() == r0, "an IN call consults no launch hint of the read path"
        compare(sel[0], w_set)
        a1 = read.batch_read_columns(ctx, [c_rle])[0]
        sel = sb.filter_in(ctx, [c_flt, c_txt], [sb.InList(lf), sb.InList(lt)])
        sb.filter_columns(ctx, [c_flt], [sb.Predicate("lt", 150)], combine="and", out=[sel[0]])
        last = sb.filter_in(ctx, [c_flt], [sb.InList(lf, negate=True)], combine="or", out=[sel[0]])
        a2 = read.batch_read_columns(ctx, [c_plain])[0]   # tiles after all: the interval is issued again, the IN calls with it
        ctx.synchronize()
        assert ctx.replays() == r0 + 1
        assert same(a1, want_rle) and same(a2, want_plain)
        final = (w_set & cmp_expected(flt, fv, fvalid, "lt", 150)) | w_not
        compare(sel[0], final, counted=last[0])
        compare(sel[1], w_txt)
    finally:
        ctx.close()


# ---- 7: buffers
GUARD = 4096


def raw_in(ctx, ptype, nullable, pages_t, metas, op, values, offsets, n_values, selection_t, sel_cap=None, combine=0, page_offsets=None,
           mem=0, keep=None):
    """one column through the C entry point itself; returns (code, struct)"""
    from strawboat_amd import _native as N
    m = np.ascontiguousarray(metas, np.uint64).reshape(-1, 2)
    arr = (N.ColumnFilterInC * 1)()
    c = arr[0]
    c.physical_type, c.is_nullable = ptype, int(nullable)
    c.pages, c.pages_len = pages_t.data_ptr(), pages_t.numel()
    c.metas, c.n_pages = m.ctypes.data_as(C.POINTER(N.PageMetaC)), m.shape[0]
    if page_offsets is not None:
        po = np.ascontiguousarray(page_offsets, np.uint64)
        c.page_offsets = po.ctypes.data
    c.op, c.combine = op, combine
    vbuf = C.create_string_buffer(values, max(1, len(values))) if values is not None else None
    c.values = C.addressof(vbuf) if vbuf is not None else None
    obuf = np.ascontiguousarray(offsets, np.uint64) if offsets is not None else None
    c.value_offsets = obuf.ctypes.data if obuf is not None else None
    c.n_values = n_values
    c.selection = selection_t.data_ptr() if selection_t is not None else None
    c.selection_capacity = selection_t.numel() if sel_cap is None else sel_cap
    if keep is not None:
        keep += [arr, m, vbuf, obuf, page_offsets if page_offsets is None else po]
    code = ctx._lib.sb_filter_columns_in(ctx._h, arr, 1, mem)
    if keep is None and code == 0:   # the call reads its arguments again at the synchronize
        ctx.synchronize()
    return code, c


def test_selection_between_guards_pages_at_any_byte_offset_and_page_offsets(gpu_ctx):
    import torch
    from strawboat_amd import _native as N
    from strawboat_amd.filter_in import pack_list
    dev = gpu_ctx.torch_device
    for col, codec in ((gen.prim(S.T_I64, 10_007, uniq=200, null_density=0.2, runs=4, seed=1), S.RLE),
                       (gen.prim(S.T_I16, 10_007, uniq=200, null_density=0.2, seed=2), S.NONE),
                       (gen.prim(S.T_F64, 10_007, uniq=200, seed=3), S.DICT),
                       (gen.binary(10_007, uniq=80, null_density=0.2, seed=4, maxlen=20), S.NONE),
                       (gen.binary(10_007, uniq=80, seed=5, maxlen=20), S.DICT)):
        pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
        binary = col["ptype"] in (S.T_BIN32, S.T_BIN64)
        if binary:
            strs, valid = oracle_strings(col, pages, metas)
            lits = sorted(set(strs))[::3] + [b"", b"absent"]
            want = want_in_bin(strs, valid, lits, False)
        else:
            vals, valid = oracle_column(col, pages, metas)
            lits = [x.item() for x in np.unique(vals)[::3]]
            want = want_in(col, vals, valid, lits, False)
        raw, offs = pack_list(col["ptype"], lits)
        rows = want.size
        nsel = 4 * ((rows + 31) // 32)
        # the pages in reverse order, each at its own offset (page_offsets do not ascend), the whole shifted by 0..7 bytes
        m = np.asarray(metas, np.uint64).reshape(-1, 2)
        starts = np.concatenate([[0], np.cumsum(m[:, 0])]).astype(np.int64)
        order = list(range(m.shape[0]))[::-1]
        blob, po, at = [], np.zeros(m.shape[0], np.uint64), 0
        for p in order:
            po[p] = at
            blob.append(pages[starts[p]:starts[p + 1]])
            at += int(m[p, 0])
        scattered = np.concatenate(blob)
        for shift in range(8):
            for layout, page_offsets in ((pages, None), (scattered, po)):
                if page_offsets is not None and shift not in (0, 3):
                    continue
                host = np.full(shift + layout.size, 0xEE, np.uint8)
                host[shift:] = layout
                pages_t = torch.from_numpy(host).to(dev)[shift:]
                buf = torch.full((GUARD + nsel + GUARD,), 0x5A, dtype=torch.uint8, device=dev)
                sel_t = buf[GUARD:GUARD + nsel]
                code, c = raw_in(gpu_ctx, col["ptype"], col["nullable"], pages_t, metas, N.SB_PRED_IN, raw, offs, len(lits), sel_t,
                                 page_offsets=page_offsets)
                assert code == 0
                got = buf.cpu().numpy()
                assert (got[:GUARD] == 0x5A).all() and (got[GUARD + nsel:] == 0x5A).all(), "the guards stay untouched"
                bits = np.unpackbits(got[GUARD:GUARD + nsel], bitorder="little").astype(bool)
                assert np.array_equal(bits[:rows], want) and not bits[rows:].any(), (codec, shift, page_offsets is not None)
                assert c.rows == rows and c.selected == int(want.sum())


# ---- 8: refusals
def test_refusals_at_the_call(gpu_ctx):
    import torch
    from strawboat_amd import _native as N
    from strawboat_amd._native import NativeError
    dev = gpu_ctx.torch_device
    num = gen.prim(S.T_I32, 3000, uniq=10)
    txt = gen.binary(3000, uniq=10)
    npages, nmetas = gen.oracle_write(num, force_codec=S.NONE)
    tpages, tmetas = gen.oracle_write(txt, force_codec=S.NONE)
    nt, tt = torch.from_numpy(npages).to(dev), torch.from_numpy(tpages).to(dev)
    four = np.array([1, 2, 3, 4], np.int32).tobytes()

    def refused(code, ptype, pages_t, metas, op, values, offsets, n_values, sel_bytes=None, sel_off=0, sticky=False, **kw):
        nsel = 4 * ((3000 + 31) // 32) if sel_bytes is None else sel_bytes
        buf = torch.full((8 + nsel,), 0xA5, dtype=torch.uint8, device=dev)
        got, _ = raw_in(gpu_ctx, ptype, False, pages_t, metas, op, values, offsets, n_values, buf[sel_off:sel_off + nsel], **kw)
        assert got == code, (got, code, gpu_ctx.last_error() if hasattr(gpu_ctx, "last_error") else "")
        if sticky:   # (like its siblings', the span refusal of the host tables is the interval's result as well)
            with pytest.raises(NativeError) as e:
                gpu_ctx.synchronize()
            assert e.value.code == code
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        assert (buf.cpu().numpy() == 0xA5).all(), "the selection must stay untouched"

    # SB_ERR_NYI: types without an order of their own here, and host memory
    for col in (gen.boolean(3000), gen.prim(S.T_I128, 3000, uniq=10), gen.prim(S.T_I256, 3000, uniq=10)):
        pages, metas = gen.oracle_write(col)
        refused(N.SB_ERR_NYI, col["ptype"], torch.from_numpy(pages).to(dev), metas, N.SB_PRED_IN, four, None, 1)
    null_col = dict(ptype=S.T_NULL, nullable=True, rows=3000, values=None, validity=None, offsets=None)
    pages, metas = gen.oracle_write(null_col)
    refused(N.SB_ERR_NYI, S.T_NULL, torch.from_numpy(np.ascontiguousarray(pages)).to(dev) if pages.size else torch.zeros(1, dtype=torch.uint8, device=dev),
            metas, N.SB_PRED_IN, four, None, 1)
    refused(N.SB_ERR_NYI, S.T_I32, nt, nmetas, N.SB_PRED_IN, four, None, 4, mem=N.SB_MEM_HOST)
    # SB_ERR_INVALID
    for op in (N.SB_PRED_EQ, N.SB_PRED_IS_NULL, N.SB_PRED_STARTS_WITH, 11, -1):
        refused(N.SB_ERR_INVALID, S.T_I32, nt, nmetas, op, four, None, 4)                                  # an op other than the two
    refused(N.SB_ERR_INVALID, S.T_I32, nt, nmetas, N.SB_PRED_IN, b"\0" * 4100, None, 1025)                 # too many values
    refused(N.SB_ERR_INVALID, S.T_BIN32, tt, tmetas, N.SB_PRED_IN, b"", np.zeros(1026, np.uint64), 1025)
    refused(N.SB_ERR_INVALID, S.T_I32, nt, nmetas, N.SB_PRED_NOT_IN, None, None, 4)                        # values null, numeric
    refused(N.SB_ERR_INVALID, S.T_BIN32, tt, tmetas, N.SB_PRED_IN, None, np.array([0, 1, 2], np.uint64), 2)   # values null, bytes to read
    refused(N.SB_ERR_INVALID, S.T_I32, nt, nmetas, N.SB_PRED_IN, four, np.array([0, 4, 8, 12, 16], np.uint64), 4)   # offsets on a numeric column
    refused(N.SB_ERR_INVALID, S.T_BIN32, tt, tmetas, N.SB_PRED_IN, b"abcd", None, 2)                       # no offsets on a binary column
    refused(N.SB_ERR_INVALID, S.T_BIN32, tt, tmetas, N.SB_PRED_IN, b"abcd", np.array([1, 2, 4], np.uint64), 2)   # do not start at 0
    refused(N.SB_ERR_INVALID, S.T_BIN32, tt, tmetas, N.SB_PRED_IN, b"abcd", np.array([0, 3, 2], np.uint64), 2)   # descend
    refused(N.SB_ERR_INVALID, S.T_BIN32, tt, tmetas, N.SB_PRED_IN, b"abcd", np.array([0, 2, (1 << 30) + 1], np.uint64), 2)   # > 2^30 bytes
    refused(N.SB_ERR_INVALID, S.T_I32, nt, nmetas, N.SB_PRED_IN, four, None, 4, combine=3)
    refused(N.SB_ERR_INVALID, S.T_I32, nt, nmetas, N.SB_PRED_IN, four, None, 4, sel_cap=4 * ((3000 + 31) // 32) - 4)   # selection too small
    refused(N.SB_ERR_INVALID, S.T_I32, nt, nmetas, N.SB_PRED_IN, four, None, 4, sel_off=2)                 # not 4-byte aligned
    buf = torch.full((400,), 0xA5, dtype=torch.uint8, device=dev)
    got, _ = raw_in(gpu_ctx, S.T_I32, False, nt, nmetas, N.SB_PRED_IN, four, None, 4, None, sel_cap=400)   # no selection
    assert got == N.SB_ERR_INVALID
    # two columns of one call on one selection
    import strawboat_amd as sb
    cp = upload(gpu_ctx, num, npages, nmetas)
    sel = sb.filter_in(gpu_ctx, [cp], [sb.InList([1, 2])])
    gpu_ctx.synchronize()
    before = sel[0].bitmap.cpu().numpy().copy()
    with pytest.raises(NativeError) as e:
        sb.filter_in(gpu_ctx, [cp, cp], [sb.InList([3]), sb.InList([4])], combine="and", out=[sel[0], sel[0]])
    assert e.value.code == N.SB_ERR_INVALID
    gpu_ctx.synchronize()
    assert np.array_equal(sel[0].bitmap.cpu().numpy(), before)
    # SB_ERR_IO: a page outside [0, pages_len)
    m = np.asarray(nmetas, np.uint64).reshape(-1, 2)
    refused(N.SB_ERR_IO, S.T_I32, nt[:nt.numel() - 8], nmetas, N.SB_PRED_IN, four, None, 4, sticky=True)
    refused(N.SB_ERR_IO, S.T_I32, nt, nmetas, N.SB_PRED_IN, four, None, 4, sticky=True, page_offsets=np.full(m.shape[0], nt.numel(), np.uint64))
    # what is accepted: values null with no value, and with only empty literals
    vals, valid = oracle_column(num, npages, nmetas)
    nsel = 4 * ((3000 + 31) // 32)
    for ptype, pages_t, metas, offsets, n_values in ((S.T_I32, nt, nmetas, None, 0), (S.T_BIN32, tt, tmetas, None, 0),
                                                     (S.T_BIN32, tt, tmetas, np.zeros(3, np.uint64), 2)):
        buf = torch.full((nsel,), 0xA5, dtype=torch.uint8, device=dev)
        code, c = raw_in(gpu_ctx, ptype, False, pages_t, metas, N.SB_PRED_NOT_IN, None, offsets, n_values, buf)
        assert code == 0 and c.rows == 3000
        bits = np.unpackbits(buf.cpu().numpy(), bitorder="little").astype(bool)
        if n_values == 0:
            assert bits[:3000].all() and not bits[3000:].any() and c.selected == 3000
        else:   # NOT IN (b"", b""): every row that is not the empty string
            strs, _ = oracle_strings(txt, tpages, tmetas)
            want = np.array([s != b"" for s in strs])
            assert np.array_equal(bits[:3000], want) and c.selected == int(want.sum())


# ---- 9: corrupt pages
def in_code(ctx, cp, lits, negate=False):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    try:
        sb.filter_in(ctx, [cp], [sb.InList(lits, negate=negate)])
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
        cp = upload(gpu_ctx, col, pages[:pages.size - cut].copy(), m)
        want = read_code(gpu_ctx, cp)
        assert want != 0
        assert in_code(gpu_ctx, cp, [1, 30, 59]) == want, codec
    # a Dict page with an index >= D: plain u32 indices behind hdr9 Dict | hdr9 None
    for uniq in (50, 20_000):   # the bit table and the gather
        col = gen.prim(S.T_I64, 40_000, uniq=uniq, seed=uniq)
        pages, metas = gen.oracle_write(col, max_page_size=40_000, force_codec=S.DICT, force_index_codec=S.NONE)
        bad = pages.copy()
        pos = 9 + 9 + 25_000 * 4
        bad[pos:pos + 4] = np.frombuffer(np.uint32(1 << 30).tobytes(), np.uint8)
        cp = upload(gpu_ctx, col, bad, metas)
        want = read_code(gpu_ctx, cp)
        assert want == -1
        assert in_code(gpu_ctx, cp, [1, 30], negate=True) == want
    # a binary column: a truncated Dict page
    col = gen.binary(9000, uniq=60, null_density=0.1, seed=3)
    pages, metas = gen.oracle_write(col, max_page_size=3000, force_codec=S.DICT)
    m = np.array(metas, np.uint64).copy()
    cut = int(m[-1, 0]) // 2
    m[-1, 0] -= cut
    cp = upload(gpu_ctx, col, pages[:pages.size - cut].copy(), m)
    want = read_code(gpu_ctx, cp)
    assert want != 0
    assert in_code(gpu_ctx, cp, [b"a", b"b"]) == want
    # the context still works
    col = gen.prim(S.T_I64, 9000, uniq=60)
    check(gpu_ctx, col, lists_of(col), max_page_size=3000, force_codec=S.DICT)


# ---- 10: a seeded sweep
SWEEP_SEED = 20261019
SWEEP_CASES = 300


def test_random_sweep(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd.filter import Selection
    rng = np.random.default_rng(SWEEP_SEED)
    codecs = [-1, S.NONE, S.RLE, S.DICT, S.LZ4, S.ZSTD, S.SNAPPY, S.FREQ]
    modes = ["set", "and", "or"]
    for case in range(SWEEP_CASES):
        binary = case % 5 == 4
        codec = codecs[int(rng.integers(0, len(codecs)))]
        if binary and codec in (S.RLE, S.FREQ):   # (no RLE pages of strings; Freq pages of strings want a frequent value: test_binary_codecs)
            codec = S.DICT
        rows = int(rng.integers(1, 20_001)) if case % 8 == 0 else int(rng.integers(1, 5_000))
        page = int(rng.choice([rows, 777, 2048, 2050, 4100, int(rng.integers(1, rows + 1))]))
        nd = [None, 0.05, 0.5][int(rng.integers(0, 3))]
        uniq = int(rng.choice([2, 100, 100_000]))
        n_lit = int(rng.choice([0, 1, 2, 7, 64, 300, 1024]))
        negate = bool(rng.integers(0, 2))
        mode = modes[int(rng.integers(0, 3))]
        seed = int(rng.integers(0, 1 << 30))
        opt = dict(max_page_size=page)
        if codec >= 0:
            opt["force_codec"] = codec
        what = "case %d: binary %r codec %d rows %d page %d nulls %r uniq %d list %d negate %r combine %s" % (
            case, binary, codec, rows, page, nd, uniq, n_lit, negate, mode)
        try:
            if binary:
                col = gen.binary(rows, uniq=min(uniq, 2000), null_density=nd, large=bool(rng.integers(0, 2)), seed=seed, maxlen=20)
                pages, metas = gen.oracle_write(col, **opt)
                vals, valid = oracle_strings(col, pages, metas)
                have = sorted(set(vals))
                lits = [have[int(i)] if rng.random() < 0.5 else bytes(rng.integers(97, 123, int(rng.integers(0, 12)), dtype=np.uint8))
                        for i in rng.integers(0, len(have), n_lit)]
                want = want_in_bin(vals, valid, lits, negate)
            else:
                ptype = CMP_TYPES[int(rng.integers(0, len(CMP_TYPES)))]
                runs = [None, 3, 50][int(rng.integers(0, 3))]
                col = gen.prim(ptype, rows, uniq=uniq, null_density=nd, runs=runs, seed=seed)
                pages, metas = gen.oracle_write(col, **opt)
                vals, valid = oracle_column(col, pages, metas)
                v = col["values"]
                lits = [v[int(i)].item() if rng.random() < 0.5 else NP[ptype](int(rng.integers(0, 120))).item() for i in rng.integers(0, rows, n_lit)]
                want = want_in(col, vals, valid, lits, negate)
            cp = upload(gpu_ctx, col, pages, metas)
            if mode == "set":
                sel = last = sb.filter_in(gpu_ctx, [cp], [sb.InList(lits, negate=negate)])
                final = want
            else:   # the earlier selection: a random pattern, zero behind the last row
                base = rng.random(want.size) < 0.5
                bits = np.zeros((want.size + 31) // 32 * 32, bool)
                bits[:want.size] = base
                sel = [Selection(torch.from_numpy(np.packbits(bits, bitorder="little")).to(gpu_ctx.torch_device), want.size, None)]
                last = sb.filter_in(gpu_ctx, [cp], [sb.InList(lits, negate=negate)], combine=mode, out=sel)
                final = base & want if mode == "and" else base | want
            gpu_ctx.synchronize()
            compare(sel[0], final, what, counted=last[0])
            assert not tail_of(sel[0]).any()
        except AssertionError as e:
            raise AssertionError("%s: %s" % (what, e))
