"""sb_filter_columns on the GPU: pages written by the CPU oracle, filtered on the device, compared with
`op(oracle_read(pages).values, literal) & validity` computed by numpy.  Nothing here is compared with what the
device's own decoder gives."""
import os

import numpy as np
import pytest

from oracle import sbo as S
from tests import gen
from tests.test_gpu_decode import LONG_RLE_ROWS, RLE_OVERSHOOT, RLE_SHORT, RLE_WIDTHS, _rle_hand_built_column, _rle_long_page, _rle_page

pytestmark = pytest.mark.gpu

NP = gen.NP_OF
CMP_TYPES = [S.T_I8, S.T_I16, S.T_I32, S.T_I64, S.T_U8, S.T_U16, S.T_U32, S.T_U64, S.T_F32, S.T_F64]
OPS6 = ["eq", "ne", "lt", "le", "gt", "ge"]
OPFN = {"eq": np.equal, "ne": np.not_equal, "lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal}


def unpack(bits, rows):
    return np.unpackbits(np.asarray(bits, np.uint8), bitorder="little")[:rows].astype(bool)


def oracle_column(col, pages, metas):
    """(values as the column's dtype or None, validity as bool) from the oracle's decode of the pages"""
    want = gen.oracle_read(col, pages, metas)
    rows = want["rows"]
    valid = unpack(want["validity"], rows) if col["nullable"] and col["ptype"] != S.T_NULL else np.ones(rows, bool)
    if col["ptype"] == S.T_NULL:
        valid = np.zeros(rows, bool)
    vals = None
    if col["ptype"] in NP:
        vals = np.ascontiguousarray(want["values"]).view(np.uint8).reshape(-1).view(NP[col["ptype"]])[:rows]
    return vals, valid


def expected(col, vals, valid, op, lit):
    if op == "is_null":
        return ~valid
    if op == "is_not_null":
        return valid.copy()
    with np.errstate(invalid="ignore"):
        return OPFN[op](vals, NP[col["ptype"]](lit)) & valid


def upload(ctx, col, pages, metas):
    import torch
    from strawboat_amd import read
    return read.ColumnPages(col["ptype"], col["nullable"], torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device), metas)


def check_pages(ctx, col, pages, metas, preds):
    """all predicates over the same pages in ONE call (one column entry per predicate), combine = set"""
    import strawboat_amd as sb
    vals, valid = oracle_column(col, pages, metas)
    cp = upload(ctx, col, pages, metas)
    sels = sb.filter_columns(ctx, [cp] * len(preds), [sb.Predicate(op, lit) for op, lit in preds])
    ctx.synchronize()
    for (op, lit), sel in zip(preds, sels):
        want = expected(col, vals, valid, op, lit)
        got = sel.numpy()
        assert sel.rows == want.size
        assert np.array_equal(got, want), "%s %r: %d rows differ, first at %d" % (op, lit, int((got != want).sum()), int(np.argmax(got != want)))
        assert sel.selected == int(want.sum()), (op, lit, sel.selected, int(want.sum()))
        tail = np.unpackbits(sel.bitmap.cpu().numpy(), bitorder="little")[sel.rows:]
        assert not tail.any(), "bits behind the last row must be 0 after set"
    return vals, valid


def check(ctx, col, preds, codec=None, **opt):
    pages, metas = gen.oracle_write(col, **opt)
    if codec is not None:
        seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
        assert seen == {codec}, (seen, codec)
    return check_pages(ctx, col, pages, metas, preds)


def literals_of(col):
    """a value near the median of the data (selectivities neither 0 nor 1), its minimum and its maximum"""
    v = np.sort(col["values"])
    return [v[v.size // 2].item(), v[0].item(), v[-1].item()]


def six_ops(col):
    return [(op, lit) for lit in literals_of(col) for op in OPS6]


def hand_built(ptype, page_list, rows_list):
    """(col, pages, metas) of hand-built pages of a column without nulls; the literals come from the oracle's decode, or
    col is None where the oracle refuses the pages"""
    pages = np.concatenate(page_list)
    metas = np.array([[p.size, n] for p, n in zip(page_list, rows_list)], np.uint64)
    col = dict(ptype=ptype, nullable=False, rows=sum(rows_list), validity=None, offsets=None)
    try:
        col["values"] = oracle_column(col, pages, metas)[0]
    except Exception:
        col = None
    return col, pages, metas


# ---- 1
@pytest.mark.parametrize("ptype", CMP_TYPES)
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT, S.ONEVALUE])
def test_prim_codecs(gpu_ctx, ptype, codec):
    uniq = 1 if codec == S.ONEVALUE else 100
    for nd, page in ((0.2, 2050), (None, 4100), (0.2, 777), (None, 2048)):
        col = gen.prim(ptype, 10_000, uniq=uniq, null_density=nd, runs=8 if nd else 3, seed=page)
        vals, valid = check(gpu_ctx, col, six_ops(col), codec=codec, max_page_size=page, force_codec=codec)
        if codec != S.ONEVALUE:   # "lt min" selects nothing, "le max" every valid row, the median something in between
            med, lo, hi = literals_of(col)
            assert not expected(col, vals, valid, "lt", lo).any() and np.array_equal(expected(col, vals, valid, "le", hi), valid)
            assert 0 < expected(col, vals, valid, "le", med).sum() and expected(col, vals, valid, "gt", med).sum() > 0


# ---- 2
@pytest.mark.parametrize("ptype,dtype,w", RLE_WIDTHS)
def test_rle_hand_built_pages(gpu_ctx, ptype, dtype, w):
    """the decoder's hand-built column (zero-count runs, a 5000-row run, three chunks of short runs, pages that start at
    odd rows, runs behind a full page) through the filter's policy of the RLE page walk"""
    col, pages, metas = hand_built(ptype, *_rle_hand_built_column(w, dtype))
    check_pages(gpu_ctx, col, pages, metas, six_ops(col))


@pytest.mark.parametrize("ptype", [S.T_I32, S.T_U32])
@pytest.mark.parametrize("codec", [S.BITPACK, S.DELTABP])
def test_bitpacking(gpu_ctx, ptype, codec):
    col = gen.prim(ptype, 128 * 100, uniq=1 << 13, sorted_=(codec == S.DELTABP))
    check(gpu_ctx, col, six_ops(col), codec=codec, max_page_size=128 * 40, force_codec=codec)
    col = gen.prim(ptype, 128 * 1024, uniq=1 << 30, sorted_=(codec == S.DELTABP), seed=7)
    check(gpu_ctx, col, six_ops(col), codec=codec, max_page_size=65536, force_codec=codec)


@pytest.mark.parametrize("icodec", [S.NONE, S.RLE, S.BITPACK, S.DELTABP, S.ONEVALUE, S.LZ4])
def test_dict_index_codecs(gpu_ctx, icodec):
    uniq = 1 if icodec == S.ONEVALUE else 200
    col = gen.prim(S.T_F64, 128 * 300, uniq=uniq, null_density=0.1, runs=16, sorted_=(icodec == S.DELTABP))
    check(gpu_ctx, col, six_ops(col), codec=S.DICT, max_page_size=128 * 100, force_codec=S.DICT, force_index_codec=icodec)


def test_dict_both_sides_of_the_bit_table(gpu_ctx):
    """dictionaries of up to 8192 entries are evaluated into a bit table in LDS; longer ones are gathered and compared per row"""
    for uniq, rows in ((8000, 60_000), (8192 * 4, 70_000)):
        col = gen.prim(S.T_I64, rows, uniq=uniq, null_density=0.2, seed=uniq)
        pages, metas = gen.oracle_write(col, max_page_size=rows, force_codec=S.DICT)
        d = np.unique(col["values"]).size
        assert (d <= 8192) == (uniq == 8000), d
        check_pages(gpu_ctx, col, pages, metas, six_ops(col))


@pytest.mark.parametrize("ptype", [S.T_I16, S.T_I64, S.T_F64])
@pytest.mark.parametrize("codec", [S.LZ4, S.ZSTD, S.SNAPPY])
def test_basic_pages_are_staged(gpu_ctx, ptype, codec):
    col = gen.prim(ptype, 30_000, uniq=300, null_density=0.2, runs=5, seed=codec)
    check(gpu_ctx, col, six_ops(col), codec=codec, max_page_size=7001, force_codec=codec)


def test_patas_pages(gpu_ctx):
    rng = np.random.default_rng(3)
    v = np.round(rng.normal(100, 20, 20_000), 2)
    col = dict(ptype=S.T_F64, nullable=True, rows=v.size, values=v, validity=gen.make_validity(rng, v.size, 0.2), offsets=None)
    check(gpu_ctx, col, six_ops(col), codec=S.PATAS, max_page_size=5000, force_codec=S.PATAS)


@pytest.mark.parametrize("ptype", [S.T_U8, S.T_I32, S.T_I64, S.T_F64])
def test_freq_pages(gpu_ctx, ptype):
    from tests.test_gpu_freq import sparse
    col = sparse(ptype, 20_000, 0.05, 2, null_density=0.1)
    check(gpu_ctx, col, six_ops(col) + [("eq", 7), ("ne", 7)], codec=S.FREQ, max_page_size=5000, force_codec=S.FREQ)


# ---- 3
@pytest.mark.parametrize("ptype", [S.T_F32, S.T_F64])
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_float_specials(gpu_ctx, ptype, codec):
    rng = np.random.default_rng(9)
    pool = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.5, -2.25, 3e30], NP[ptype])
    v = np.repeat(pool[rng.integers(0, pool.size, 3000)], 3)
    col = dict(ptype=ptype, nullable=True, rows=v.size, values=v, validity=gen.make_validity(rng, v.size, 0.2), offsets=None)
    preds = [(op, lit) for lit in (float("nan"), 0.0, -0.0, float("inf"), float("-inf"), 1.5) for op in OPS6]
    vals, valid = check(gpu_ctx, col, preds, max_page_size=2050, force_codec=codec)
    assert np.array_equal(expected(col, vals, valid, "ne", float("nan")), valid)        # NaN satisfies only ne
    assert expected(col, vals, valid, "eq", 0.0).sum() == expected(col, vals, valid, "eq", -0.0).sum() > 0


@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_signedness_comes_from_the_physical_type(gpu_ctx, codec):
    rng = np.random.default_rng(10)
    b = np.repeat(rng.integers(0, 256, 4000).astype(np.uint8), 2)
    for ptype, lits in ((S.T_I8, (-128, -1, 0, 127)), (S.T_U8, (0x80, 0xFF, 0, 127))):
        col = dict(ptype=ptype, nullable=False, rows=b.size, values=b.view(NP[ptype]), validity=None, offsets=None)
        check(gpu_ctx, col, [(op, lit) for lit in lits for op in OPS6], max_page_size=777, force_codec=codec)
    for ptype, npt in ((S.T_I16, np.int16), (S.T_I32, np.int32), (S.T_I64, np.int64)):
        v = np.repeat(rng.integers(-1000, 1000, 3000), 2).astype(npt)
        col = dict(ptype=ptype, nullable=False, rows=v.size, values=v, validity=None, offsets=None)
        check(gpu_ctx, col, [(op, lit) for lit in (-1, 0, -1000, 999) for op in OPS6], max_page_size=2050, force_codec=codec)


# ---- 4
NULL_PREDS = [("is_null", None), ("is_not_null", None)]


@pytest.mark.parametrize("ptype", CMP_TYPES + [S.T_I128, S.T_I256])
def test_null_tests_on_primitives(gpu_ctx, ptype):
    for nd in (0.2, None):
        col = gen.prim(ptype, 10_000, uniq=50, null_density=nd, runs=4)
        for codec in (S.NONE, S.RLE, S.DICT):
            check(gpu_ctx, col, NULL_PREDS, max_page_size=2050, force_codec=codec)


def test_null_tests_on_boolean_binary_and_null_columns(gpu_ctx):
    check(gpu_ctx, gen.boolean(9000, null_density=0.3, runs=7), NULL_PREDS, max_page_size=777)
    check(gpu_ctx, gen.boolean(9000), NULL_PREDS, max_page_size=777)
    for large in (False, True):
        col = gen.binary(6000, uniq=40, null_density=0.25, large=large)
        results = []
        for opt in (dict(force_codec=S.DICT), dict(force_codec=S.LZ4), dict(force_codec=S.NONE)):
            vals, valid = check(gpu_ctx, col, NULL_PREDS, max_page_size=2050, **opt)
            results.append(valid)
        assert all(np.array_equal(results[0], r) for r in results[1:])   # the value codec does not matter
        check(gpu_ctx, gen.binary(3000, uniq=40, large=large), NULL_PREDS, max_page_size=777)
    col = dict(ptype=S.T_NULL, nullable=True, rows=5000, values=None, validity=None, offsets=None)
    check(gpu_ctx, col, NULL_PREDS, max_page_size=2050)


# ---- 5
def test_combine_modes_on_one_stream(gpu_ctx):
    import torch
    import strawboat_amd as sb
    rows = 10_007   # (the last word holds 23 rows)
    a = gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    b = gen.prim(S.T_F64, rows, uniq=100, runs=6, seed=2)
    c = gen.prim(S.T_U16, rows, uniq=100, null_density=0.1, seed=3)
    cols, want = [], []
    for col, codec, page, (op, lit) in ((a, S.RLE, 2050, ("lt", 60)), (b, S.DICT, 777, ("ge", 30.0)), (c, S.NONE, 4100, ("eq", 5))):
        pages, metas = gen.oracle_write(col, max_page_size=page, force_codec=codec)
        vals, valid = oracle_column(col, pages, metas)
        want.append(expected(col, vals, valid, op, lit))
        cols.append((upload(gpu_ctx, col, pages, metas), sb.Predicate(op, lit)))

    def state(sel):
        bits = np.unpackbits(sel.bitmap.cpu().numpy(), bitorder="little").astype(bool)
        return bits[:rows], bits[rows:]

    # one synchronize interval: set, and, or
    sel = sb.filter_columns(gpu_ctx, [cols[0][0]], [cols[0][1]])
    sb.filter_columns(gpu_ctx, [cols[1][0]], [cols[1][1]], combine="and", out=sel)
    s3 = sb.filter_columns(gpu_ctx, [cols[2][0]], [cols[2][1]], combine="or", out=sel)
    gpu_ctx.synchronize()
    got, tail = state(sel[0])
    final = (want[0] & want[1]) | want[2]
    assert np.array_equal(got, final) and not tail.any()
    assert s3[0].selected == int(final.sum())
    # step by step, the buffer pre-filled with ones: set clears the bits behind the last row, and / or keep them
    with torch.cuda.stream(gpu_ctx.torch_stream):
        sel[0].bitmap.fill_(0xFF)
    s1 = sb.filter_columns(gpu_ctx, [cols[1][0]], [cols[1][1]], combine="and", out=sel)
    gpu_ctx.synchronize()
    got, tail = state(sel[0])
    assert np.array_equal(got, want[1]) and tail.all() and s1[0].selected == int(want[1].sum())
    s2 = sb.filter_columns(gpu_ctx, [cols[2][0]], [cols[2][1]], combine="or", out=sel)
    gpu_ctx.synchronize()
    got, tail = state(sel[0])
    assert np.array_equal(got, want[1] | want[2]) and tail.all() and s2[0].selected == int((want[1] | want[2]).sum())
    s0 = sb.filter_columns(gpu_ctx, [cols[0][0]], [cols[0][1]], combine="set", out=sel)
    gpu_ctx.synchronize()
    got, tail = state(sel[0])
    assert np.array_equal(got, want[0]) and not tail.any() and s0[0].selected == int(want[0].sum())


def test_combine_with_a_freq_page_in_the_chain(gpu_ctx):
    """a Freq page makes the interval run a second time (its exceptions are decoded by a pass at the synchronize): set / and / or
    chains give the same bits as without it"""
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows = 20_000
    f = sparse(S.T_I32, rows, 0.05, 2, null_density=0.1)
    b = gen.prim(S.T_I32, rows, uniq=100, runs=6, seed=2)
    fp, fm = gen.oracle_write(f, max_page_size=5000, force_codec=S.FREQ)
    bp, bm = gen.oracle_write(b, max_page_size=4100, force_codec=S.RLE)
    wf = expected(f, *oracle_column(f, fp, fm), "eq", 7)
    wb = expected(b, *oracle_column(b, bp, bm), "lt", 50)
    cf, cb = upload(gpu_ctx, f, fp, fm), upload(gpu_ctx, b, bp, bm)
    pf, pb = sb.Predicate("eq", 7), sb.Predicate("lt", 50)
    for first, second, mode, want in ((cb, cf, "and", wb & wf), (cb, cf, "or", wb | wf), (cf, cb, "and", wf & wb), (cf, cb, "or", wf | wb)):
        sel = sb.filter_columns(gpu_ctx, [first], [pb if first is cb else pf])
        last = sb.filter_columns(gpu_ctx, [second], [pb if second is cb else pf], combine=mode, out=sel)
        gpu_ctx.synchronize()
        assert np.array_equal(sel[0].numpy(), want) and last[0].selected == int(want.sum())
        # ... and with the earlier selection coming from an interval of its own
        sel = sb.filter_columns(gpu_ctx, [first], [pb if first is cb else pf])
        gpu_ctx.synchronize()
        last = sb.filter_columns(gpu_ctx, [second], [pb if second is cb else pf], combine=mode, out=sel)
        gpu_ctx.synchronize()
        assert np.array_equal(sel[0].numpy(), want) and last[0].selected == int(want.sum())


def test_two_columns_of_one_call_may_not_share_a_selection(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    col = gen.prim(S.T_I32, 5000, uniq=10)
    pages, metas = gen.oracle_write(col, force_codec=S.NONE)
    cp = upload(gpu_ctx, col, pages, metas)
    sel = sb.filter_columns(gpu_ctx, [cp], [sb.Predicate("lt", 5)])
    gpu_ctx.synchronize()
    with pytest.raises(NativeError) as e:
        sb.filter_columns(gpu_ctx, [cp, cp], [sb.Predicate("lt", 5)] * 2, combine="and", out=[sel[0], sel[0]])
    assert e.value.code == -5
    gpu_ctx.synchronize()


# ---- 6
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_long_pages(gpu_ctx, codec):
    rows = (1 << 18) + 12_345
    col = gen.prim(S.T_F64, rows, uniq=256, null_density=0.1, runs=32 if codec != S.NONE else None, seed=4)
    pages, metas = gen.oracle_write(col, force_codec=codec)
    assert metas.shape[0] == 1
    check_pages(gpu_ctx, col, pages, metas, six_ops(col))
    if codec == S.RLE:   # hand-built: zero-count runs on both sides of a border between two parts of the page
        col, pages, metas = hand_built(S.T_I64, [_rle_long_page()], [LONG_RLE_ROWS])
        if col is None:   # the oracle's values or the oracle's refusal, never a difference
            import strawboat_amd as sb
            assert filter_code(gpu_ctx, upload(gpu_ctx, dict(ptype=S.T_I64, nullable=False), pages, metas), sb.Predicate("lt", 0)) != 0
        else:
            check_pages(gpu_ctx, col, pages, metas, six_ops(col))


def test_empty_column_and_one_row_page(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    cp = read.ColumnPages(S.T_I64, False, torch.zeros(0, dtype=torch.uint8, device=gpu_ctx.torch_device), np.zeros((0, 2), np.uint64))
    sel = sb.filter_columns(gpu_ctx, [cp], [sb.Predicate("lt", 3)])
    gpu_ctx.synchronize()
    assert sel[0].rows == 0 and sel[0].selected == 0 and sel[0].numpy().size == 0
    for nd in (None, 0.5):
        for seed in (1, 2, 3):
            col = gen.prim(S.T_I32, 1, uniq=5, null_density=nd, seed=seed)
            check(gpu_ctx, col, six_ops(col) + NULL_PREDS)
    col = gen.prim(S.T_I32, 2051, uniq=5, seed=4)   # ... and a one-row page behind two others
    check(gpu_ctx, col, six_ops(col), max_page_size=1025, force_codec=S.RLE)


# ---- 7
def test_comparisons_on_other_types_are_refused_at_the_call(gpu_ctx):
    import ctypes as C
    import torch
    from strawboat_amd import _native as N
    for col in (gen.boolean(3000), gen.prim(S.T_I128, 3000, uniq=10), gen.binary(3000, uniq=10)):
        pages, metas = gen.oracle_write(col)
        cp = upload(gpu_ctx, col, pages, metas)
        m = cp.metas_array()
        arr = (N.ColumnFilterC * 1)()
        c = arr[0]
        c.physical_type, c.is_nullable = col["ptype"], 0
        c.pages, c.pages_len = cp.pages.data_ptr(), cp.pages.numel()
        c.metas, c.n_pages = m.ctypes.data_as(C.POINTER(N.PageMetaC)), m.shape[0]
        c.op, c.combine = N.SB_PRED_LT, N.SB_SEL_SET
        bitmap = torch.full((((col["rows"] + 31) // 32) * 4,), 0xA5, dtype=torch.uint8, device=gpu_ctx.torch_device)
        c.selection, c.selection_capacity = bitmap.data_ptr(), bitmap.numel()
        assert gpu_ctx._lib.sb_filter_columns(gpu_ctx._h, arr, 1, N.SB_MEM_DEVICE) == N.SB_ERR_NYI
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        assert (bitmap.cpu().numpy() == 0xA5).all(), "the selection must stay untouched"


def read_code(ctx, cp):
    from strawboat_amd import read
    from strawboat_amd._native import NativeError
    try:
        read.read_simple(ctx, cp)
    except NativeError as e:
        try:
            ctx.synchronize()
        except NativeError:
            pass
        return e.code
    return 0


def filter_code(ctx, cp, pred):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    try:
        sb.filter_columns(ctx, [cp], [pred])
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
    from strawboat_amd import read
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
        assert filter_code(gpu_ctx, cp, sb.Predicate("lt", 30)) == want, codec
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
        assert filter_code(gpu_ctx, cp, sb.Predicate("lt", 30)) == want
    # hand-built RLE pages: a run that overshoots the page, runs that end before the page is full
    for (ptype, dtype, w, runs, rows), code in ((RLE_OVERSHOOT, -1), (RLE_SHORT, -3)):
        page = _rle_page(runs, w, dtype).copy()
        cp = upload(gpu_ctx, dict(ptype=ptype, nullable=False), page, np.array([[page.size, rows]], np.uint64))
        assert read_code(gpu_ctx, cp) == code
        assert filter_code(gpu_ctx, cp, sb.Predicate("lt", 2)) == code
    # a corrupt def-level section (u32 def_len | ULEB128 | bits): the null tests read it themselves, the comparisons and the
    # decoder through k_parse, and all three refuse it alike
    col = gen.prim(S.T_I64, 3000, uniq=60, null_density=0.2, seed=9)
    pages, metas = gen.oracle_write(col, max_page_size=1 << 20, force_codec=S.NONE)
    assert metas.shape[0] == 1 and int(np.frombuffer(pages[:4].tobytes(), np.uint32)[0]) == 2 + 375 and pages[4] & 0x80
    for what, pos, patch in (("def_len larger than the page", 0, np.uint32(0xFFFFFF00).tobytes()),
                             ("def_len == 0 with rows", 0, np.uint32(0).tobytes()),
                             ("an even ULEB128 indicator", 4, bytes([pages[4] & 0xFE])),
                             ("a bit count below N", 4, bytes([(1 << 1) | 1]))):   # one byte: 8 bits for 3000 rows
        bad = pages.copy()
        bad[pos:pos + len(patch)] = np.frombuffer(patch, np.uint8)
        cp = upload(gpu_ctx, col, bad, metas)
        want = read_code(gpu_ctx, cp)
        assert want != 0, what
        assert filter_code(gpu_ctx, cp, sb.Predicate("is_null")) == want, what
        assert filter_code(gpu_ctx, cp, sb.Predicate("lt", 30)) == want, what
    # the context still works
    col = gen.prim(S.T_I64, 9000, uniq=60)
    check(gpu_ctx, col, six_ops(col), max_page_size=3000, force_codec=S.DICT)


# ---- 8
def test_filter_between_reads_of_one_interval_with_a_hint_that_misses():
    if os.environ.get("SB_NO_HINTS", "0") != "0":
        pytest.skip("SB_NO_HINTS: every kernel is launched, nothing to replay")
    import strawboat_amd as sb
    from strawboat_amd import read
    ctx = sb.Context(0)
    try:
        rle = gen.prim(S.T_F64, 200_000, uniq=50, null_density=0.1, runs=40, seed=5)
        plain = gen.prim(S.T_I64, 200_000, uniq=1 << 40, seed=6)
        flt = gen.prim(S.T_I32, 100_001, uniq=300, null_density=0.2, runs=5, seed=7)
        rp, rm = gen.oracle_write(rle, max_page_size=65536, force_codec=S.RLE)
        pp, pm = gen.oracle_write(plain, max_page_size=65536, force_codec=S.NONE)
        fp, fm = gen.oracle_write(flt, max_page_size=7001, force_codec=S.DICT)
        c_rle, c_plain, c_flt = upload(ctx, rle, rp, rm), upload(ctx, plain, pp, pm), upload(ctx, flt, fp, fm)
        want_rle, want_plain = gen.oracle_read(rle, rp, rm), gen.oracle_read(plain, pp, pm)
        want_sel = expected(flt, *oracle_column(flt, fp, fm), "lt", 150)

        def same(arr, want):
            return np.array_equal(arr.values_numpy(), want["values"]) and (arr.validity is None or np.array_equal(arr.validity_numpy(), want["validity"]))

        for _ in range(3):   # read intervals that need neither inflate jobs nor tiles: the next read calls leave those kernels out
            read.read_simple(ctx, c_rle)
        r0 = ctx.replays()
        # a filter call between two such intervals changes nothing for the reads (its Dict pages queue tiles of its own)
        sel = sb.filter_columns(ctx, [c_flt], [sb.Predicate("lt", 150)])
        ctx.synchronize()
        assert ctx.replays() == r0 and np.array_equal(sel[0].numpy(), want_sel)
        a1 = read.batch_read_columns(ctx, [c_rle])[0]
        sel = sb.filter_columns(ctx, [c_flt], [sb.Predicate("lt", 150)])
        a2 = read.batch_read_columns(ctx, [c_plain])[0]   # tiles after all: the interval is issued again, the filter call with it
        ctx.synchronize()
        assert ctx.replays() == r0 + 1
        assert same(a1, want_rle) and same(a2, want_plain)
        assert np.array_equal(sel[0].numpy(), want_sel) and sel[0].selected == int(want_sel.sum())
        # the same reads with no filter call between them
        ctx2 = sb.Context(0)
        try:
            d1, d2 = read.batch_read_columns(ctx2, [upload(ctx2, rle, rp, rm)])[0], read.batch_read_columns(ctx2, [upload(ctx2, plain, pp, pm)])[0]
            ctx2.synchronize()
            assert np.array_equal(d1.values_numpy(), a1.values_numpy()) and np.array_equal(d1.validity_numpy(), a1.validity_numpy())
            assert np.array_equal(d2.values_numpy(), a2.values_numpy())
        finally:
            ctx2.close()
    finally:
        ctx.close()


# ---- 9
SWEEP_SEED = 20240917
SWEEP_CASES = 200


def test_random_sweep(gpu_ctx):
    rng = np.random.default_rng(SWEEP_SEED)
    codecs = [-1, S.NONE, S.RLE, S.DICT, S.LZ4, S.ZSTD, S.SNAPPY, S.FREQ]
    for case in range(SWEEP_CASES):
        ptype = CMP_TYPES[int(rng.integers(0, len(CMP_TYPES)))]
        codec = codecs[int(rng.integers(0, len(codecs)))]
        rows = int(rng.integers(1, 70_001)) if case % 4 == 0 else int(rng.integers(1, 9_000))
        page = int(rng.choice([rows, 777, 2048, 2050, 4100, 65536, int(rng.integers(1, rows + 1))]))
        nd = [None, 0.05, 0.5][int(rng.integers(0, 3))]
        uniq = int(rng.choice([2, 100, 100_000]))
        runs = [None, 3, 50][int(rng.integers(0, 3))]
        col = gen.prim(ptype, rows, uniq=uniq, null_density=nd, runs=runs, seed=int(rng.integers(0, 1 << 30)))
        v = col["values"]
        lits = [v[int(rng.integers(0, rows))].item(), int(rng.integers(0, 120))]
        preds = [(OPS6[int(rng.integers(0, 6))], lit) for lit in lits] + [NULL_PREDS[int(rng.integers(0, 2))]]
        opt = dict(max_page_size=page)
        if codec >= 0:
            opt["force_codec"] = codec
        try:
            check(gpu_ctx, col, preds, **opt)
        except AssertionError as e:
            raise AssertionError("case %d: type %d codec %d rows %d page %d nulls %r uniq %d runs %r: %s" % (case, ptype, codec, rows, page, nd, uniq, runs, e))
