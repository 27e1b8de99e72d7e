"""sb_read_selected on the GPU: pages written by the CPU oracle (hand-built where noted), the selected rows read on the
device, compared with `oracle_read(pages)` compacted by numpy: `vals[mask]` as bytes and `packbits(valid[mask])`.
Nothing here is compared with what the device's own decoder gives.  Every case checks the value bytes below values_len,
the validity bits below `selected`, the zero bits behind them in the last word, `selected` / `rows`, and that nothing
behind what the call may write was touched (the buffers are pre-filled with a guard pattern)."""
import ctypes as C

import numpy as np
import pytest

from oracle import sbo as S
from tests import gen
from tests.test_gpu_decode import LONG_RLE_ROWS, RLE_OVERSHOOT, RLE_SHORT, RLE_WIDTHS, _rle_hand_built_column, _rle_page
from tests.test_read_selected_host import PAGE_ROWS, ROWS, bitmap_of, patterns

pytestmark = pytest.mark.gpu

NP = gen.NP_OF
TYPES = [S.T_I8, S.T_I16, S.T_I32, S.T_I64, S.T_U8, S.T_U16, S.T_U32, S.T_U64, S.T_F32, S.T_F64]
PAGES = (777, 2048, 2050, 4100)
GUARD = 0xA5
GUARD_BYTES = 256


def unpack(bits, n):
    return np.unpackbits(np.asarray(bits, np.uint8), bitorder="little")[:n].astype(bool)


def oracle_column(col, pages, metas):
    """(the values' bytes as [rows, width], validity as bool or None) from the oracle's decode of the pages"""
    want = gen.oracle_read(col, pages, metas)
    rows = want["rows"]
    w = np.dtype(NP[col["ptype"]]).itemsize
    vals = np.ascontiguousarray(want["values"]).view(np.uint8).reshape(-1)[:rows * w].reshape(rows, w)
    valid = unpack(want["validity"], rows) if col["nullable"] else None
    return vals, valid


def upload(ctx, col, pages, metas):
    import torch
    from strawboat_amd import read
    return read.ColumnPages(col["ptype"], col["nullable"], torch.from_numpy(np.ascontiguousarray(pages)).to(ctx.torch_device), metas)


def to_dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.torch_device)


def guarded(ctx, nbytes):
    """(the buffer handed to the call: `nbytes` of a longer one that is filled with the guard pattern, the whole buffer)"""
    import torch
    with torch.cuda.stream(ctx.torch_stream):   # (the fill is ordered before the call's kernels)
        whole = torch.full((nbytes + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=ctx.torch_device)
    return whole[:nbytes], whole


class Case:
    """one column of a call: its pages, its selection and what the oracle says comes out"""

    def __init__(self, ctx, col, pages, metas, mask, tail=False, values_cap=None, validity_cap=None, oracle=None):
        self.col = col
        self.vals, self.valid = oracle if oracle is not None else oracle_column(col, pages, metas)
        self.rows = self.vals.shape[0]
        self.w = self.vals.shape[1]
        assert mask.size == self.rows
        self.mask = mask
        self.cp = upload(ctx, col, pages, metas)
        self.bitmap = to_dev(ctx, bitmap_of(mask, tail))
        self.values, self.values_whole = guarded(ctx, self.rows * self.w if values_cap is None else values_cap)
        self.validity = self.validity_whole = None
        if col["nullable"]:
            self.validity, self.validity_whole = guarded(ctx, (self.rows + 31) // 32 * 4 if validity_cap is None else validity_cap)

    def out(self):
        return (self.values, self.validity)

    def check(self, arr, what=""):
        sel = int(self.mask.sum())
        assert arr.rows == self.rows and arr.selected == sel, (what, arr.rows, arr.selected, sel)
        assert arr.values_len == sel * self.w, what
        got = self.values_whole.cpu().numpy()
        want = self.vals[self.mask].reshape(-1)
        if not np.array_equal(got[:want.size], want):
            bad = np.flatnonzero(got[:want.size] != want)
            raise AssertionError("%s: %d value bytes differ, first at output row %d" % (what, bad.size, bad[0] // self.w))
        assert (got[want.size:] == GUARD).all(), "%s: bytes behind values_len were written" % what
        if self.validity_whole is None:
            return
        gb = self.validity_whole.cpu().numpy()
        nwords = (sel + 31) // 32
        bits = unpack(gb[:nwords * 4], nwords * 32)
        assert np.array_equal(bits[:sel], self.valid[self.mask]), "%s: validity differs, first at output row %d" % (
            what, int(np.argmax(bits[:sel] != self.valid[self.mask])))
        assert not bits[sel:].any(), "%s: bits >= selected of the last validity word must be 0" % what
        assert (gb[nwords * 4:] == GUARD).all(), "%s: validity words behind the last one were written" % what


def run(ctx, cases, what=""):
    """all cases as the columns of ONE call"""
    import strawboat_amd as sb
    arrs = sb.read_selected(ctx, [c.cp for c in cases], [c.bitmap for c in cases], out=[c.out() for c in cases])
    ctx.synchronize()
    for i, (c, a) in enumerate(zip(cases, arrs)):
        c.check(a, "%s column %d" % (what, i))
    return arrs


def two_masks(rows, seed):
    """a random selection of about a third of the rows, and a sparse one that leaves whole tiles and pages out"""
    rng = np.random.default_rng(seed)
    sparse = np.zeros(rows, bool)
    at = int(rng.integers(0, max(1, rows - 70)))
    sparse[at:at + 70] = rng.random(min(70, rows - at)) < 0.7
    sparse[rows - 1] = True
    return [rng.random(rows) < 0.35, sparse]


def check_pages(ctx, col, pages, metas, masks=None, what=""):
    oracle = oracle_column(col, pages, metas)
    if masks is None:
        masks = two_masks(oracle[0].shape[0], 11)
    return run(ctx, [Case(ctx, col, pages, metas, m, oracle=oracle) for m in masks], what)


def check(ctx, col, codec=None, masks=None, **opt):
    pages, metas = gen.oracle_write(col, **opt)
    if codec is not None:
        seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
        assert seen == {codec}, (seen, codec)
    return check_pages(ctx, col, pages, metas, masks, what="codec %r %r" % (codec, opt))


# ---- 1: codecs x types
@pytest.mark.parametrize("ptype", TYPES)
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT, S.ONEVALUE])
def test_prim_codecs(gpu_ctx, ptype, codec):
    uniq = 1 if codec == S.ONEVALUE else 100
    for nd, page in [(nd, page) for nd in (0.2, None) for page in PAGES]:
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


# ---- 2: selection patterns (the list is pinned on the CPU: tests/test_read_selected_host.py)
# (row 4096 is a tile seam only in a page of more than 4096 rows: in the 4100-row RLE pages it is a seam of the page walk's
# tile loop, in the 4100-row None and Dict pages one of the tile kernel)
@pytest.mark.parametrize("page_rows,codec", [(PAGE_ROWS[0], S.NONE), (PAGE_ROWS[1], S.RLE), (PAGE_ROWS[1], S.NONE), (PAGE_ROWS[1], S.DICT)])
def test_selection_patterns(gpu_ctx, page_rows, codec):
    col = gen.prim(S.T_I64, ROWS, uniq=100, null_density=0.2, runs=6 if codec == S.RLE else None, seed=page_rows)
    pages, metas = gen.oracle_write(col, max_page_size=page_rows, force_codec=codec)
    assert [int(n) for n in metas[:-1, 1]] == [page_rows] * (metas.shape[0] - 1)
    oracle = oracle_column(col, pages, metas)
    pats = patterns(ROWS, page_rows)
    cases = [Case(gpu_ctx, col, pages, metas, mask, tail, oracle=oracle) for _, mask, tail in pats]
    arrs = run(gpu_ctx, cases, "patterns")
    by_name = dict((name, (c, a)) for (name, _, _), c, a in zip(pats, cases, arrs))
    c, a = by_name["zeros"]
    assert a.selected == 0 and (c.values_whole.cpu().numpy() == GUARD).all() and (c.validity_whole.cpu().numpy() == GUARD).all()
    c, a = by_name["zeros, bits behind the rows set"]
    assert a.selected == 0 and (c.values_whole.cpu().numpy() == GUARD).all() and (c.validity_whole.cpu().numpy() == GUARD).all()
    c, a = by_name["ones"]   # equals the full read
    assert a.selected == ROWS and np.array_equal(c.values_whole.cpu().numpy()[:ROWS * 8], oracle[0].reshape(-1))
    assert by_name["bits behind the rows set"][1].selected == int(by_name["bits behind the rows set"][0].mask.sum())


# ---- 3: the decoder's hand-built RLE column
@pytest.mark.parametrize("ptype,dtype,w", RLE_WIDTHS)
def test_rle_hand_built_pages(gpu_ctx, ptype, dtype, w):
    """zero-count runs, a 5000-row run, three chunks of short runs, pages that start at odd rows, runs behind a full page"""
    page_list, rows_list = _rle_hand_built_column(w, dtype)
    pages = np.concatenate(page_list)
    metas = np.array([[p.size, n] for p, n in zip(page_list, rows_list)], np.uint64)
    rows = sum(rows_list)
    col = dict(ptype=ptype, nullable=False, rows=rows, validity=None, offsets=None)
    rng = np.random.default_rng(w)
    check_pages(gpu_ctx, col, pages, metas, [rng.random(rows) < 0.5, np.arange(rows) % 2 == 0, rng.random(rows) < 0.01], "hand-built RLE")


# ---- 4: one long page (several workgroups share an RLE page)
@pytest.mark.parametrize("codec", [S.RLE, S.DICT])
def test_one_long_page(gpu_ctx, codec):
    col = gen.prim(S.T_F64, LONG_RLE_ROWS, uniq=256, null_density=0.1, runs=32, seed=4)
    pages, metas = gen.oracle_write(col, force_codec=codec)
    assert metas.shape[0] == 1
    rng = np.random.default_rng(codec)
    check_pages(gpu_ctx, col, pages, metas, [rng.random(LONG_RLE_ROWS) < 0.002], "long page")


# ---- 5: Freq pages: the interval is issued again, the call's columns decoded and compacted
@pytest.mark.parametrize("ptype", [S.T_I32, S.T_I64])
def test_freq_pages(gpu_ctx, ptype):
    from tests.test_gpu_freq import sparse
    rows = 10_000
    f = sparse(ptype, rows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    assert S.FREQ in set(int(x) for x in S.stat_column(f["ptype"], f["nullable"], fp, fm)[0].tolist())
    b = gen.prim(S.T_I64, rows, uniq=100, null_density=0.2, runs=6, seed=2)
    bp, bm = gen.oracle_write(b, max_page_size=4100, force_codec=S.RLE)
    rng = np.random.default_rng(ptype)
    mask = rng.random(rows) < 0.3
    r0 = gpu_ctx.replays()
    run(gpu_ctx, [Case(gpu_ctx, f, fp, fm, mask), Case(gpu_ctx, b, bp, bm, mask)], "freq")
    assert gpu_ctx.replays() == r0 + 1
    # ... and a sparse selection
    run(gpu_ctx, [Case(gpu_ctx, f, fp, fm, two_masks(rows, 5)[1])], "freq, sparse")


def test_freq_pages_without_a_selected_row_and_a_larger_call_behind_them(gpu_ctx):
    """A Freq page is logged for the second decode pass by the parse step, and that pass writes through the staging area.
    With no selected row in the page the call must still not leave the record to the synchronize: a later, larger call of
    the same interval outgrows the staging area and frees it.  The interval is issued again instead (the filter's route),
    and every byte, guard and count is right."""
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows = 10_000
    f = sparse(S.T_I64, rows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    assert S.FREQ in set(int(x) for x in S.stat_column(f["ptype"], f["nullable"], fp, fm)[0].tolist())
    big_rows = 300_000   # 2.4 MB of staging per column: more than every earlier call of the session's context asked for
    b = gen.prim(S.T_I64, big_rows, uniq=1000, null_density=0.2, seed=12)
    bp, bm = gen.oracle_write(b, max_page_size=65536, force_codec=S.LZ4)
    elsewhere = np.zeros(rows, bool)   # sparse, and in one page only: the other pages hold no selected row
    elsewhere[2050 * 3 + 5:2050 * 3 + 40] = True
    bmask = np.random.default_rng(12).random(big_rows) < 0.01
    for fmask in (np.zeros(rows, bool), elsewhere):
        small = Case(gpu_ctx, f, fp, fm, fmask)
        big = [Case(gpu_ctx, b, bp, bm, bmask) for _ in range(3)]
        r0 = gpu_ctx.replays()
        a_small = sb.read_selected(gpu_ctx, [small.cp], [small.bitmap], out=[small.out()])
        a_big = sb.read_selected(gpu_ctx, [c.cp for c in big], [c.bitmap for c in big], out=[c.out() for c in big])
        gpu_ctx.synchronize()
        assert gpu_ctx.replays() == r0 + 1
        small.check(a_small[0], "freq, %d selected" % int(fmask.sum()))
        for c, a in zip(big, a_big):
            c.check(a, "the larger call behind the freq call")
        big_rows += 50_000   # (the second round's larger call outgrows the first round's as well)
        b = gen.prim(S.T_I64, big_rows, uniq=1000, null_density=0.2, seed=13)
        bp, bm = gen.oracle_write(b, max_page_size=65536, force_codec=S.LZ4)
        bmask = np.random.default_rng(13).random(big_rows) < 0.01


# ---- 6: filter -> read_selected in one interval
@pytest.mark.parametrize("freq", [False, True])
def test_filter_then_read_selected_in_one_interval(gpu_ctx, freq):
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows = 10_007
    x = sparse(S.T_I32, rows, 0.05, 2, null_density=0.1) if freq else gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    y = gen.prim(S.T_F64, rows, uniq=100, runs=6, seed=2)
    xp, xm = gen.oracle_write(x, max_page_size=2050, force_codec=S.FREQ if freq else S.RLE)
    yp, ym = gen.oracle_write(y, max_page_size=777, force_codec=S.DICT)
    xlit = 7 if freq else 60

    def typed(col, pages, metas):
        vals, valid = oracle_column(col, pages, metas)
        return vals.reshape(-1).view(NP[col["ptype"]]), (valid if valid is not None else np.ones(vals.shape[0], bool))

    xv, xvalid = typed(x, xp, xm)
    yv, yvalid = typed(y, yp, ym)
    mask = ((xv != xlit) & xvalid) & ((yv >= 30.0) & yvalid)
    assert 0 < mask.sum() < rows
    a = gen.prim(S.T_I64, rows, uniq=100, null_density=0.2, runs=6, seed=3)
    b = gen.prim(S.T_U16, rows, uniq=100, null_density=0.1, seed=4)
    ap, am = gen.oracle_write(a, max_page_size=4100, force_codec=S.RLE)
    bp, bm = gen.oracle_write(b, max_page_size=2050, force_codec=S.DICT)
    r0 = gpu_ctx.replays()
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("ne", xlit)])
    sb.filter_columns(gpu_ctx, [upload(gpu_ctx, y, yp, ym)], [sb.Predicate("ge", 30.0)], combine="and", out=sel)
    arrs = sb.read_selected(gpu_ctx, [upload(gpu_ctx, a, ap, am), upload(gpu_ctx, b, bp, bm)], sel[0])   # default capacities
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + (1 if freq else 0)
    assert np.array_equal(sel[0].numpy(), mask)
    for col, pages, metas, arr in ((a, ap, am, arrs[0]), (b, bp, bm, arrs[1])):
        vals, valid = typed(col, pages, metas)
        got_vals, got_valid = arr.numpy()
        assert arr.selected == int(mask.sum()) and arr.rows == rows
        assert np.array_equal(got_vals.view(np.uint8), vals[mask].view(np.uint8))
        assert np.array_equal(got_valid, valid[mask])
        assert tuple(arr.values.shape) == (arr.selected,)


# ---- 7: capacities are checked on the device, at the synchronize
def test_capacities(gpu_ctx):
    from strawboat_amd._native import NativeError
    rows = 10_000
    col = gen.prim(S.T_I64, rows, uniq=100, null_density=0.2, runs=6, seed=8)
    mask = np.random.default_rng(8).random(rows) < 0.4
    sel = int(mask.sum())
    vwords = (sel + 31) // 32
    assert sel % 32 != 0
    for codec, page in ((S.RLE, 4100), (S.NONE, 2050)):
        pages, metas = gen.oracle_write(col, max_page_size=page, force_codec=codec)
        oracle = oracle_column(col, pages, metas)
        for vcap, bcap, ok in ((sel * 8, vwords * 4, True), (sel * 8 - 8, vwords * 4, False), (sel * 8, vwords * 4 - 4, False)):
            c = Case(gpu_ctx, col, pages, metas, mask, values_cap=vcap, validity_cap=bcap, oracle=oracle)
            if ok:
                run(gpu_ctx, [c], "exact capacities")
                continue
            import strawboat_amd as sb
            arrs = sb.read_selected(gpu_ctx, [c.cp], [c.bitmap], out=[c.out()])
            with pytest.raises(NativeError) as e:
                gpu_ctx.synchronize()
            assert e.value.code == -5
            assert arrs[0].selected == sel and arrs[0].values_len == sel * 8   # what the buffers have to hold
            assert (c.values_whole.cpu().numpy()[vcap:] == GUARD).all(), "written behind values_capacity"
            assert (c.validity_whole.cpu().numpy()[bcap:] == GUARD).all(), "written behind validity_capacity"
            run(gpu_ctx, [Case(gpu_ctx, col, pages, metas, mask, oracle=oracle)], "the context after a refused capacity")


# ---- 8: refusals at the call
def raw_call(ctx, arr):
    from strawboat_amd import _native as N
    return ctx._lib.sb_read_selected(ctx._h, arr, len(arr), N.SB_MEM_DEVICE)


def test_refusals_at_the_call(gpu_ctx):
    import torch
    from strawboat_amd import _native as N
    from strawboat_amd.read_selected import ReadSelectedBatch
    dev = gpu_ctx.torch_device
    # types
    for col in (gen.boolean(3000), gen.prim(S.T_I128, 3000, uniq=10), gen.prim(S.T_I256, 3000, uniq=10), gen.binary(3000, uniq=10),
                gen.binary(3000, uniq=10, large=True), dict(ptype=S.T_NULL, nullable=True, rows=3000, values=None, validity=None, offsets=None)):
        pages, metas = gen.oracle_write(col)
        cp = upload(gpu_ctx, col, pages, metas)
        m = cp.metas_array()
        arr = (N.ColumnReadSelectedC * 1)()
        c = arr[0]
        c.physical_type, c.is_nullable = col["ptype"], 0
        c.pages, c.pages_len = cp.pages.data_ptr() if cp.pages.numel() else 0, cp.pages.numel()
        c.metas, c.n_pages = m.ctypes.data_as(C.POINTER(N.PageMetaC)), m.shape[0]
        with torch.cuda.stream(gpu_ctx.torch_stream):
            bitmap = torch.full((((col["rows"] + 31) // 32) * 4,), 0xFF, dtype=torch.uint8, device=dev)
            values = torch.full((col["rows"] * 32,), GUARD, dtype=torch.uint8, device=dev)
        c.selection, c.selection_capacity = bitmap.data_ptr(), bitmap.numel()
        c.values, c.values_capacity = values.data_ptr(), values.numel()
        assert raw_call(gpu_ctx, arr) == N.SB_ERR_NYI, col["ptype"]
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        assert (values.cpu().numpy() == GUARD).all()
    # buffers
    col = gen.prim(S.T_I64, 5000, uniq=10, null_density=0.2)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.NONE)
    oracle = oracle_column(col, pages, metas)
    mask = np.ones(5000, bool)

    def fresh():
        a, b = Case(gpu_ctx, col, pages, metas, mask, oracle=oracle), Case(gpu_ctx, col, pages, metas, mask, oracle=oracle)
        return a, b, ReadSelectedBatch(gpu_ctx, [a.cp, b.cp], [a.bitmap, b.bitmap], out=[a.out(), b.out()])

    def refused(a, b, batch, what):
        assert raw_call(gpu_ctx, batch._arr) == N.SB_ERR_INVALID, what
        gpu_ctx.synchronize()
        for c in (a, b):
            assert (c.values_whole.cpu().numpy() == GUARD).all() and (c.validity_whole.cpu().numpy() == GUARD).all(), what

    a, b, batch = fresh()
    batch._arr[1].values = batch._arr[0].values + 8
    refused(a, b, batch, "values of two columns overlap")
    a, b, batch = fresh()
    batch._arr[1].validity = batch._arr[0].values + 64
    refused(a, b, batch, "validity inside another column's values")
    a, b, batch = fresh()
    batch._arr[0].values, batch._arr[0].values_capacity = batch._arr[1].selection, 64
    refused(a, b, batch, "values over a selection of the call")
    a, b, batch = fresh()
    batch._arr[1].selection += 1
    refused(a, b, batch, "misaligned selection")
    a, b, batch = fresh()
    batch._arr[1].selection = 0
    refused(a, b, batch, "null selection")
    a, b, batch = fresh()
    batch._arr[1].selection_capacity = (5000 + 31) // 32 * 4 - 4
    refused(a, b, batch, "short selection_capacity")
    a, b, batch = fresh()
    batch._arr[0].validity = 0
    refused(a, b, batch, "nullable without validity")
    a, b, batch = fresh()
    assert gpu_ctx._lib.sb_read_selected(gpu_ctx._h, batch._arr, 2, N.SB_MEM_HOST) == N.SB_ERR_NYI
    gpu_ctx.synchronize()
    # two columns that share ONE selection are the usual case
    arrs = batch.enqueue()
    gpu_ctx.synchronize()
    a.check(arrs[0], "after the refusals")
    b.check(arrs[1], "after the refusals")


# ---- 9: empty and tiny
def test_empty_and_tiny(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    dev = gpu_ctx.torch_device
    cp = read.ColumnPages(S.T_I64, True, torch.zeros(0, dtype=torch.uint8, device=dev), np.zeros((0, 2), np.uint64))
    arrs = sb.read_selected(gpu_ctx, [cp], torch.zeros(0, dtype=torch.uint8, device=dev))
    gpu_ctx.synchronize()
    assert arrs[0].rows == 0 and arrs[0].selected == 0 and arrs[0].values_len == 0 and arrs[0].numpy()[0].size == 0
    # ... and as one column of a call that has pages
    col = gen.prim(S.T_I32, 3000, uniq=5, null_density=0.3, seed=4)
    pages, metas = gen.oracle_write(col, max_page_size=777, force_codec=S.NONE)
    full = Case(gpu_ctx, col, pages, metas, np.random.default_rng(1).random(3000) < 0.5)
    arrs = sb.read_selected(gpu_ctx, [cp, full.cp], [torch.zeros(0, dtype=torch.uint8, device=dev), full.bitmap],
                            out=[(torch.zeros(0, dtype=torch.uint8, device=dev), torch.zeros(0, dtype=torch.uint8, device=dev)), full.out()])
    gpu_ctx.synchronize()
    assert arrs[0].selected == 0
    full.check(arrs[1], "next to an empty column")
    for nd in (None, 0.5):
        for seed in (1, 2, 3):
            col = gen.prim(S.T_I32, 1, uniq=5, null_density=nd, seed=seed)
            check(gpu_ctx, col, masks=[np.array([True]), np.array([False])])
    col = gen.prim(S.T_I32, 2051, uniq=5, seed=4)   # a one-row page behind two others
    check(gpu_ctx, col, max_page_size=1025, force_codec=S.RLE)
    col = gen.prim(S.T_F64, 10_000, uniq=1, null_density=0.2, seed=5)   # every page OneValue
    check(gpu_ctx, col, codec=S.ONEVALUE, max_page_size=2050, force_codec=S.ONEVALUE)


# ---- 10: corrupt pages raise what the decoder raises
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


def selected_code(ctx, cp, rows):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    try:
        sb.read_selected(ctx, [cp], to_dev(ctx, bitmap_of(np.ones(rows, bool))))
        ctx.synchronize()
    except NativeError as e:
        try:
            ctx.synchronize()
        except NativeError:
            pass
        return e.code
    return 0


def oracle_code(col, pages, metas):
    try:
        gen.oracle_read(col, pages, metas)
    except Exception as e:
        return getattr(e, "code", None)
    return 0


def test_corrupt_pages_raise_what_the_decoder_raises(gpu_ctx):
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
        assert selected_code(gpu_ctx, cp, 9000) == want, codec
    # a Dict page with an index >= D: plain u32 indices behind hdr9 Dict | hdr9 None
    col = gen.prim(S.T_I64, 40_000, uniq=50, seed=50)
    pages, metas = gen.oracle_write(col, max_page_size=40_000, force_codec=S.DICT, force_index_codec=S.NONE)
    bad = pages.copy()
    pos = 9 + 9 + 25_000 * 4
    bad[pos:pos + 4] = np.frombuffer(np.uint32(1 << 30).tobytes(), np.uint8)
    cp = upload(gpu_ctx, col, bad, metas)
    assert read_code(gpu_ctx, cp) == -1 and oracle_code(col, bad, metas) != 0
    assert selected_code(gpu_ctx, cp, 40_000) == -1
    # hand-built RLE pages: a run that overshoots the page, runs that end before the page is full
    for (ptype, dtype, w, runs, rows), code in ((RLE_OVERSHOOT, -1), (RLE_SHORT, -3)):
        page = _rle_page(runs, w, dtype).copy()
        cp = upload(gpu_ctx, dict(ptype=ptype, nullable=False), page, np.array([[page.size, rows]], np.uint64))
        assert read_code(gpu_ctx, cp) == code
        assert selected_code(gpu_ctx, cp, rows) == code
    # the context still works
    col = gen.prim(S.T_I64, 9000, uniq=60)
    check(gpu_ctx, col, max_page_size=3000, force_codec=S.DICT)


# ---- 11: a seeded sweep
SWEEP_SEED = 20241018
SWEEP_CASES = 60


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
        col = gen.prim(ptype, rows, uniq=uniq, null_density=nd, runs=runs, seed=int(rng.integers(0, 1 << 30)))
        if kind == 0:
            mask = rng.random(rows) < p
        elif kind == 1:   # clustered: the bits of one stretch of the column
            mask = np.zeros(rows, bool)
            at = int(rng.integers(0, rows))
            mask[at:at + max(1, int(rows * p))] = True
        else:
            mask = (np.arange(rows) % int(rng.integers(2, 70))) == 0
        opt = dict(max_page_size=page)
        if codec >= 0:
            opt["force_codec"] = codec
        try:
            pages, metas = gen.oracle_write(col, **opt)
            run(gpu_ctx, [Case(gpu_ctx, col, pages, metas, mask, tail=bool(case & 1))], "sweep")
        except AssertionError as e:
            raise AssertionError("seed %d case %d: type %d codec %d rows %d page %d nulls %r uniq %d runs %r p %r kind %d: %s" % (
                SWEEP_SEED, case, ptype, codec, rows, page, nd, uniq, runs, p, kind, e))
