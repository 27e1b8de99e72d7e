"""sb_read_selected_var on the GPU: Binary / LargeBinary pages written by the CPU oracle, the selected rows read on the
device, compared with the oracle's decode of the same pages compacted in Python: `[s for s, m in zip(strs, mask) if m]`.
Nothing here is compared with what the device's own decoder gives.  Every output buffer sits between 0xA5 guards; every
case checks the offsets, the bytes, the validity bits and the zero bits behind them in the last word, `rows` / `selected` /
`values_len`, and that nothing in front of a buffer or behind what the call may write was touched."""
import ctypes as C

import numpy as np
import pytest

from oracle import sbo as S
from tests import gen
from tests.test_gpu_filter_binary import CODECS, codec_column, column_of, oracle_strings, staged_bytes, strings_of, upload, write
from tests.test_gpu_read_selected import two_masks
from tests.test_read_selected_host import ROWS, bitmap_of, patterns

pytestmark = pytest.mark.gpu

GUARD = 0xA5
FRONT = 64          # guard bytes in front of every output (keeps the 8-byte alignment of an offsets buffer)
GUARD_BYTES = 256   # ... and behind it


def unpack(bits, n):
    return np.unpackbits(np.asarray(bits, np.uint8), bitorder="little")[:n].astype(bool)


def to_dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(ctx.torch_device)


class Guarded:
    """`nbytes` handed to the call, `shift` bytes behind an aligned address, inside a longer buffer filled with the guard"""

    def __init__(self, ctx, nbytes, shift=0):
        import torch
        self.front, self.nbytes = FRONT + shift, nbytes
        with torch.cuda.stream(ctx.torch_stream):   # (the fill is ordered before the call's kernels)
            self.whole = torch.full((self.front + nbytes + GUARD_BYTES,), GUARD, dtype=torch.uint8, device=ctx.torch_device)
        self.buf = self.whole[self.front:self.front + nbytes]

    def split(self, used, what, replayed=False):
        """(the first `used` bytes of the buffer; asserts that everything else still holds the guard.  replayed: the call ran
        twice, the first time with the bitmap the interval's first pass left — only the capacity bounds what that wrote)"""
        a = self.whole.cpu().numpy()
        assert (a[:self.front] == GUARD).all(), "%s: bytes in front of the buffer were written" % what
        behind = self.nbytes if replayed else used
        assert (a[self.front + behind:] == GUARD).all(), "%s: bytes behind byte %d of the buffer were written" % (what, behind)
        return a[self.front:self.front + used]

    def untouched(self):
        return bool((self.whole.cpu().numpy() == GUARD).all())


class Case:
    """one column of a call: its pages, its selection and what the oracle says comes out.  Default capacities: the ones
    that are always enough ((rows + 1) offsets, the full read's value bytes, 4*ceil(rows/32))."""

    def __init__(self, ctx, col, pages, metas, mask, tail=False, offsets_cap=None, values_cap=None, validity_cap=None, oracle=None,
                 cp=None, values_shift=0):
        strs, valid = oracle if oracle is not None else oracle_strings(col, pages, metas)
        self.rows = len(strs)
        assert mask.size == self.rows
        self.mask = mask
        self.osize = 8 if col["ptype"] == S.T_BIN64 else 4
        self.odt = np.int64 if self.osize == 8 else np.int32
        self.want = [s for s, m in zip(strs, mask) if m]
        self.want_valid = valid[mask]
        self.nullable = bool(col["nullable"])
        self.cp = cp if cp is not None else upload(ctx, col, pages, metas)
        self.bitmap = to_dev(ctx, bitmap_of(mask, tail))
        self.offsets = Guarded(ctx, (self.rows + 1) * self.osize if offsets_cap is None else offsets_cap)
        self.values = Guarded(ctx, sum(len(s) for s in strs) if values_cap is None else values_cap, values_shift)
        self.validity = None
        if self.nullable:
            self.validity = Guarded(ctx, (self.rows + 31) // 32 * 4 if validity_cap is None else validity_cap)

    def out(self):
        return (self.offsets.buf, self.values.buf, self.validity.buf if self.validity is not None else None)

    @property
    def selected(self):
        return len(self.want)

    @property
    def values_len(self):
        return sum(len(s) for s in self.want)

    def check(self, arr, what="", replayed=False):
        sel, vlen = self.selected, self.values_len
        assert arr.rows == self.rows and arr.selected == sel, (what, arr.rows, arr.selected, sel)
        assert arr.values_len == vlen, (what, arr.values_len, vlen)
        got_off = self.offsets.split((sel + 1) * self.osize, what + " offsets", replayed).view(self.odt)
        want_off = np.concatenate([[0], np.cumsum([len(s) for s in self.want], dtype=np.int64)]).astype(self.odt)
        if not np.array_equal(got_off, want_off):
            bad = np.flatnonzero(got_off != want_off)
            raise AssertionError("%s: %d offsets differ, first at %d: %d, not %d" % (what, bad.size, bad[0], got_off[bad[0]], want_off[bad[0]]))
        got = self.values.split(vlen, what + " values", replayed)
        want = np.frombuffer(b"".join(self.want), np.uint8)
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            k = int(np.searchsorted(want_off.astype(np.int64), bad[0], side="right")) - 1
            raise AssertionError("%s: %d value bytes differ, first at byte %d (output row %d, %d bytes)" % (what, bad.size, bad[0], k, len(self.want[k])))
        if self.validity is None:
            return
        nwords = (sel + 31) // 32
        bits = unpack(self.validity.split(nwords * 4, what + " validity", replayed), nwords * 32)
        assert np.array_equal(bits[:sel], self.want_valid), "%s: validity differs, first at output row %d" % (
            what, int(np.argmax(bits[:sel] != self.want_valid)))
        assert not bits[sel:].any(), "%s: bits >= selected of the last validity word must be 0" % what
        # the Python views agree with the raw buffers
        offs, vals, vbits = arr.numpy()
        assert np.array_equal(offs, want_off) and vals.tobytes() == b"".join(self.want) and np.array_equal(vbits, self.want_valid)

    def outputs_untouched(self):
        return self.offsets.untouched() and self.values.untouched() and (self.validity is None or self.validity.untouched())


def run(ctx, cases, what="", **kw):
    """all cases as the columns of ONE call"""
    import strawboat_amd as sb
    arrs = sb.read_selected_var(ctx, [c.cp for c in cases], [c.bitmap for c in cases], out=[c.out() for c in cases], **kw)
    ctx.synchronize()
    for i, (c, a) in enumerate(zip(cases, arrs)):
        c.check(a, "%s column %d" % (what, i))
    return arrs


def check_pages(ctx, col, pages, metas, masks=None, what="", **kw):
    oracle = oracle_strings(col, pages, metas)
    if masks is None:
        masks = two_masks(len(oracle[0]), 11)
    return run(ctx, [Case(ctx, col, pages, metas, m, oracle=oracle) for m in masks], what, **kw)


# ---- 1: codecs x offsets width x nullable x page sizes; the selection patterns
@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
@pytest.mark.parametrize("name,codec,opt", CODECS, ids=[c[0] for c in CODECS])
def test_codecs(gpu_ctx, large, name, codec, opt):
    for nd, page in ((0.2, 2050), (None, 4100), (0.2, 777), (None, 2048)):
        col = codec_column(codec, large, nd, seed=page)
        pages, metas = write(col, codec, max_page_size=page, **opt)
        if codec in (S.LZ4, S.ZSTD, S.SNAPPY):   # the default stage_capacity must do for these fixtures
            assert staged_bytes(col, pages, metas) <= 4 * pages.size
        arrs = check_pages(gpu_ctx, col, pages, metas, what="%s page %d" % (name, page))
        assert all(0 < a.selected < a.rows for a in arrs)


@pytest.mark.parametrize("page_rows", [2050, 4100])
@pytest.mark.parametrize("name,codec,opt", [CODECS[0], CODECS[4], CODECS[1]], ids=["none", "dict", "lz4"])
def test_selection_patterns(gpu_ctx, page_rows, name, codec, opt):
    col = gen.binary(ROWS, uniq=100, null_density=0.2, seed=page_rows, maxlen=40)
    pages, metas = write(col, codec, max_page_size=page_rows, **opt)
    assert [int(n) for n in metas[:-1, 1]] == [page_rows] * (metas.shape[0] - 1)
    oracle = oracle_strings(col, pages, metas)
    pats = patterns(ROWS, page_rows)
    assert len(pats) == 15
    cases = [Case(gpu_ctx, col, pages, metas, mask, tail, oracle=oracle) for _, mask, tail in pats]
    arrs = run(gpu_ctx, cases, "patterns")
    by_name = dict((n, (c, a)) for (n, _, _), c, a in zip(pats, cases, arrs))
    for n in ("zeros", "zeros, bits behind the rows set"):
        c, a = by_name[n]
        assert a.selected == 0 and a.values_len == 0 and c.values.untouched() and c.validity.untouched()
    c, a = by_name["ones"]   # equals the full read
    assert a.selected == ROWS and a.to_pylist() == [s if v else None for s, v in zip(*oracle)]


# ---- 2: the string-length ladder, empty strings only, one row, no row
LADDER = list(range(66)) + [300]
LONG = 70_000


def ladder_strings(seed):
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(0, 256, n, dtype=np.uint8)) for n in LADDER], bytes(rng.integers(0, 256, LONG, dtype=np.uint8))


@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
@pytest.mark.parametrize("name,codec,opt", [CODECS[0], CODECS[4], CODECS[1]], ids=["none", "dict", "lz4"])
def test_string_length_ladder(gpu_ctx, large, name, codec, opt):
    ladder, long = ladder_strings(codec)
    every = np.ones(len(ladder) + 1, bool)
    cases = []
    for what, strings, mask in (("long first", [long] + ladder, every),
                                ("long last", ladder + [long], every),
                                ("long unselected", ladder[:30] + [long] + ladder[30:], np.arange(len(ladder) + 1) != 30),
                                ("every other row", ladder[:41] + [long] + ladder[41:], np.arange(len(ladder) + 1) % 2 == 1)):
        col = column_of(strings, None, None, large)
        valid = np.array([len(s) not in (5, 17, 40) for s in strings])   # three null rows (what a writer puts there is its own business)
        col["validity"], col["nullable"] = gen.pack_bits(valid), True
        pages, metas = write(col, codec, **opt)
        oracle = oracle_strings(col, pages, metas)
        assert np.array_equal(oracle[1], valid)
        assert sorted(len(s) for s, v in zip(*oracle) if v) == sorted(set(LADDER) - {5, 17, 40}) + [LONG]
        cases.append(Case(gpu_ctx, col, pages, metas, mask, oracle=oracle))
    assert cases[2].values_len < LONG < cases[3].values_len   # (the long string left out / selected)
    run(gpu_ctx, cases, "ladder")


def test_empty_strings_only_one_row_and_no_row(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    for large in (False, True):
        rng = np.random.default_rng(12)
        col = column_of([b""] * 5000, rng, 0.3, large)   # empty strings only: no value byte, `values` may be null
        for opt in (dict(force_codec=S.NONE), dict(force_codec=S.DICT), dict(force_codec=S.ONEVALUE), dict()):
            pages, metas = write(col, None, max_page_size=2050, **opt)
            oracle = oracle_strings(col, pages, metas)
            cases = [Case(gpu_ctx, col, pages, metas, m, values_cap=0, oracle=oracle) for m in two_masks(5000, 3)]
            assert all(c.values.buf.numel() == 0 for c in cases)
            arrs = run(gpu_ctx, cases, "empty strings")
            assert all(a.values_len == 0 and a.selected > 0 for a in arrs)
        for nd in (None, 0.5):   # a one-row column
            for seed in (1, 2, 3):
                col = gen.binary(1, uniq=5, null_density=nd, large=large, seed=seed)
                pages, metas = write(col)
                check_pages(gpu_ctx, col, pages, metas, masks=[np.array([True]), np.array([False])], what="one row")
        # a column without a page: offsets[0] = 0 is still written
        ptype = S.T_BIN64 if large else S.T_BIN32
        dev = gpu_ctx.torch_device
        cp = read.ColumnPages(ptype, True, torch.zeros(0, dtype=torch.uint8, device=dev), np.zeros((0, 2), np.uint64))
        osize = 8 if large else 4
        off, val, bits = Guarded(gpu_ctx, osize), Guarded(gpu_ctx, 0), Guarded(gpu_ctx, 0)
        arrs = sb.read_selected_var(gpu_ctx, [cp], torch.zeros(0, dtype=torch.uint8, device=dev), out=[(off.buf, val.buf, bits.buf)])
        gpu_ctx.synchronize()
        a = arrs[0]
        assert a.rows == 0 and a.selected == 0 and a.values_len == 0 and a.to_pylist() == []
        assert not off.split(osize, "no row").any() and val.untouched() and bits.untouched()
        # ... and as one column of a call that has pages
        col = gen.binary(3000, uniq=30, null_density=0.3, large=large, seed=4)
        pages, metas = write(col, None, max_page_size=777, force_codec=S.NONE)
        full = Case(gpu_ctx, col, pages, metas, np.random.default_rng(1).random(3000) < 0.5)
        off = Guarded(gpu_ctx, osize)
        arrs = sb.read_selected_var(gpu_ctx, [cp, full.cp], [torch.zeros(0, dtype=torch.uint8, device=dev), full.bitmap],
                                    out=[(off.buf, val.buf, bits.buf), full.out()])
        gpu_ctx.synchronize()
        assert arrs[0].selected == 0 and not off.split(osize, "no row, second call").any()
        full.check(arrs[1], "next to a column without a page")


# ---- 3: Dict index codecs
@pytest.mark.parametrize("icodec", [S.NONE, S.RLE, S.BITPACK])
def test_dict_index_codecs(gpu_ctx, icodec):
    rng = np.random.default_rng(5)
    strings = strings_of(gen.binary(128 * 300, uniq=200, seed=3, maxlen=24, minlen=1))
    if icodec == S.RLE:   # runs
        strings = [s for s in strings[:128 * 300 // 8] for _ in range(8)]
    col = column_of(strings, rng, 0.1)
    pages, metas = write(col, S.DICT, max_page_size=128 * 100, force_codec=S.DICT, force_index_codec=icodec)
    inner = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[1].tolist())
    assert inner == {icodec}, inner
    check_pages(gpu_ctx, col, pages, metas, what="index codec %d" % icodec)


# ---- 4: one long page, two of its tiles selected
@pytest.mark.parametrize("name,codec,opt", [CODECS[0], CODECS[4], CODECS[1]], ids=["none", "dict", "lz4"])
def test_long_page_with_two_tiles_selected(gpu_ctx, name, codec, opt):
    rows = 40_000
    col = gen.binary(rows, uniq=300, null_density=0.1, zipf=1.3, maxlen=30, seed=4)
    pages, metas = write(col, codec, max_page_size=rows, **opt)
    assert metas.shape[0] == 1
    mask = np.zeros(rows, bool)
    mask[3 * 4096:4 * 4096] = True
    mask[9 * 4096:] = True   # (the page's last tile: 3136 rows)
    check_pages(gpu_ctx, col, pages, metas, masks=[mask], what="long page")


# ---- 5: capacities are checked on the device, at the synchronize
@pytest.mark.parametrize("large", [False, True], ids=["binary", "large_binary"])
def test_exact_capacities_and_one_unit_short(gpu_ctx, large):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    rows = 10_000
    col = gen.binary(rows, uniq=100, null_density=0.2, large=large, seed=8, maxlen=40)
    mask = np.random.default_rng(8).random(rows) < 0.4
    osize = 8 if large else 4
    for codec, page in ((S.DICT, 4100), (S.NONE, 2050), (S.LZ4, 2050)):
        pages, metas = write(col, codec, max_page_size=page, force_codec=codec)
        oracle = oracle_strings(col, pages, metas)
        probe = Case(gpu_ctx, col, pages, metas, mask, oracle=oracle)
        sel, vlen = probe.selected, probe.values_len
        vwords = (sel + 31) // 32
        assert sel % 32 != 0 and vlen > 0
        exact = ((sel + 1) * osize, vlen, vwords * 4)
        for ocap, vcap, bcap in (exact, (exact[0] - osize, vlen, exact[2]), (exact[0], vlen - 1, exact[2]), (exact[0], vlen, exact[2] - 4)):
            c = Case(gpu_ctx, col, pages, metas, mask, offsets_cap=ocap, values_cap=vcap, validity_cap=bcap, oracle=oracle)
            if (ocap, vcap, bcap) == exact:
                run(gpu_ctx, [c], "exact capacities")
                continue
            arrs = sb.read_selected_var(gpu_ctx, [c.cp], [c.bitmap], out=[c.out()])
            with pytest.raises(NativeError) as e:
                gpu_ctx.synchronize()
            what = "codec %d capacities %r of %r" % (codec, (ocap, vcap, bcap), exact)
            assert e.value.code == -5, what
            assert arrs[0].selected == sel and arrs[0].values_len == vlen, what   # what the buffers have to hold
            c.offsets.split(ocap, what + " offsets")      # (nothing in front of a buffer or behind its capacity)
            c.values.split(vcap, what + " values")
            c.validity.split(bcap, what + " validity")
            run(gpu_ctx, [Case(gpu_ctx, col, pages, metas, mask, oracle=oracle)], "the context after a refused capacity")


# ---- 6: placement: pages at odd addresses, page_offsets scattered and descending, values at odd addresses
@pytest.mark.parametrize("name,codec,opt", [CODECS[0], CODECS[4], CODECS[1]], ids=["none", "dict", "lz4"])
def test_placement(gpu_ctx, name, codec, opt):
    import torch
    from strawboat_amd import read
    rows = 9000
    col = gen.binary(rows, uniq=150, null_density=0.2, seed=21, maxlen=33)
    pages, metas = write(col, codec, max_page_size=2050, **opt)
    oracle = oracle_strings(col, pages, metas)
    dev = gpu_ctx.torch_device
    masks = two_masks(rows, 21)
    cases = []
    for shift, vshift, mask in ((1, 1, masks[0]), (7, 3, masks[1])):   # 1 and 7 bytes behind a 512-byte boundary
        buf = torch.zeros(1024 + pages.size, dtype=torch.uint8, device=dev)
        base = (-buf.data_ptr()) % 512 + shift
        buf[base:base + pages.size] = to_dev(gpu_ctx, pages)
        assert buf[base:].data_ptr() % 512 == shift
        cp = read.ColumnPages(col["ptype"], col["nullable"], buf[base:base + pages.size], metas)
        cases.append(Case(gpu_ctx, col, pages, metas, mask, oracle=oracle, cp=cp, values_shift=vshift))
        assert cases[-1].values.buf.data_ptr() % 2 == 1
    # the pages in descending order, 3 / 5 / 7 ... bytes apart
    lens = [int(m[0]) for m in np.asarray(metas).tolist()]
    starts = np.concatenate([[0], np.cumsum(lens)])
    scattered = np.full(pages.size + 16 * len(lens) + 16, 0xEE, np.uint8)
    page_offsets = np.zeros(len(lens), np.uint64)
    at = scattered.size
    for p, n in enumerate(lens):
        at -= n + 3 + 2 * p
        page_offsets[p] = at
        scattered[at:at + n] = pages[starts[p]:starts[p] + n]
    assert (np.diff(page_offsets.astype(np.int64)) < 0).all()
    cp = read.ColumnPages(col["ptype"], col["nullable"], to_dev(gpu_ctx, scattered), metas, page_offsets=page_offsets)
    cases.append(Case(gpu_ctx, col, pages, metas, masks[0], oracle=oracle, cp=cp, values_shift=5))
    run(gpu_ctx, cases, "placement")


# ---- 7: filter -> read_selected + read_selected_var in one interval, no synchronize in between
@pytest.mark.parametrize("freq", [False, True], ids=["plain", "replayed for a primitive Freq page"])
def test_filter_then_read_selected_var_in_one_interval(gpu_ctx, freq):
    import strawboat_amd as sb
    from tests.test_gpu_filter import expected as num_expected, oracle_column as num_oracle
    from tests.test_gpu_filter_binary import expected
    from tests.test_gpu_freq import sparse
    from tests.test_gpu_read_selected import oracle_column as rsel_oracle
    rows = 10_007   # (the last word holds 23 rows)
    w = gen.binary(rows, uniq=80, null_density=0.1, seed=9, maxlen=16)               # the WHERE column
    wp, wm = gen.oracle_write(w, max_page_size=4100, force_codec=S.DICT)
    lit = sorted(set(strings_of(w)))[50]
    mask = expected(*oracle_strings(w, wp, wm), "lt", lit)
    cols = [upload(gpu_ctx, w, wp, wm)]
    preds = [sb.Predicate("lt", lit)]
    if freq:   # a primitive Freq filter column: the interval is issued again with the numeric columns decoded first
        f = sparse(S.T_I32, rows, 0.05, 2, null_density=0.1)
        fp, fm = gen.oracle_write(f, max_page_size=5000, force_codec=S.FREQ)
        assert S.FREQ in set(int(x) for x in S.stat_column(f["ptype"], f["nullable"], fp, fm)[0].tolist())
        mask = mask & num_expected(f, *num_oracle(f, fp, fm), "eq", 7)
        cols.append(upload(gpu_ctx, f, fp, fm))
        preds.append(sb.Predicate("eq", 7))
    assert 0 < mask.sum() < rows
    n = gen.prim(S.T_I64, rows, uniq=100, null_density=0.2, runs=6, seed=3)           # the payload columns
    s1 = gen.binary(rows, uniq=60, null_density=0.1, seed=3, maxlen=20)
    s2 = gen.binary(rows, uniq=500, seed=4, large=True, zipf=1.3, maxlen=30)
    np_, nm = gen.oracle_write(n, max_page_size=4100, force_codec=S.RLE)
    p1, m1 = gen.oracle_write(s1, max_page_size=2050, force_codec=S.DICT)
    p2, m2 = gen.oracle_write(s2, max_page_size=2048, force_codec=S.LZ4)
    c1, c2 = Case(gpu_ctx, s1, p1, m1, mask), Case(gpu_ctx, s2, p2, m2, mask)
    r0 = gpu_ctx.replays()
    sel = sb.filter_columns(gpu_ctx, cols[:1], preds[:1])
    if freq:
        sb.filter_columns(gpu_ctx, cols[1:], preds[1:], combine="and", out=sel)
    nums = sb.read_selected(gpu_ctx, [upload(gpu_ctx, n, np_, nm)], sel[0])
    strs = sb.read_selected_var(gpu_ctx, [c1.cp, c2.cp], sel[0], out=[c1.out(), c2.out()])   # two columns, one bitmap
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + (1 if freq else 0)
    assert np.array_equal(sel[0].numpy(), mask)
    # (the first pass of a replayed interval ran this call with the bitmap as the Freq column's filter had left it then)
    c1.check(strs[0], "Utf8 behind the filter", replayed=freq)
    c2.check(strs[1], "LargeUtf8 behind the filter", replayed=freq)
    vals, valid = rsel_oracle(n, np_, nm)
    got_vals, got_valid = nums[0].numpy()
    assert nums[0].selected == int(mask.sum())
    assert np.array_equal(got_vals.view(np.uint8), vals[mask].reshape(-1)) and np.array_equal(got_valid, valid[mask])


# ---- 8: corrupt pages
def selected_code(ctx, case):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    try:
        sb.read_selected_var(ctx, [case.cp], [case.bitmap], out=[case.out()])
        ctx.synchronize()
    except NativeError as e:
        try:
            ctx.synchronize()
        except NativeError:
            pass
        return e.code
    return 0


def test_corrupt_pages_return_a_status_and_leave_the_guards(gpu_ctx):
    from tests.test_gpu_read_selected import read_code
    # a truncated last page
    for codec in (S.NONE, S.DICT, S.LZ4):
        col = gen.binary(9000, uniq=60, null_density=0.1, seed=codec)
        pages, metas = gen.oracle_write(col, max_page_size=3000, force_codec=codec)
        oracle = oracle_strings(col, pages, metas)
        m = np.array(metas, np.uint64).copy()
        cut = int(m[-1, 0]) // 2
        m[-1, 0] -= cut
        cp = upload(gpu_ctx, col, pages[:pages.size - cut].copy(), m)
        want = read_code(gpu_ctx, cp)
        assert want != 0
        c = Case(gpu_ctx, col, pages, metas, np.ones(9000, bool), oracle=oracle, cp=cp)
        assert selected_code(gpu_ctx, c) == want, codec
        # only the capacities bound what such a call writes: nothing in front of a buffer, nothing behind it
        c.offsets.split(c.offsets.nbytes, "truncated page, offsets")
        c.values.split(c.values.nbytes, "truncated page, values")
        c.validity.split(c.validity.nbytes, "truncated page, validity")
    # a Dict page with an index >= D: plain u32 indices behind hdr9 Dict | hdr9 None
    for uniq in (50, 20_000):   # (the filter test's two dictionaries: one that any cache holds, one of 260 KB)
        vocab = [b"v%05d" % i for i in range(uniq)]
        rng = np.random.default_rng(uniq)
        idx = np.concatenate([np.arange(uniq), rng.integers(0, uniq, 40_000 - uniq)])
        col = column_of([vocab[i] for i in idx])
        pages, metas = gen.oracle_write(col, max_page_size=40_000, force_codec=S.DICT, force_index_codec=S.NONE)
        assert metas.shape[0] == 1
        oracle = oracle_strings(col, pages, metas)
        bad = pages.copy()
        pos = 9 + 9 + 25_000 * 4
        bad[pos:pos + 4] = np.frombuffer(np.uint32(1 << 30).tobytes(), np.uint8)
        cp = upload(gpu_ctx, col, bad, metas)
        c = Case(gpu_ctx, col, pages, metas, np.ones(40_000, bool), oracle=oracle, cp=cp)
        assert selected_code(gpu_ctx, c) == -1   # SB_ERR_OUT_OF_SPEC: the row is selected
        c.offsets.split(c.offsets.nbytes, "bad index, offsets, D = %d" % uniq)
        c.values.split(c.values.nbytes, "bad index, values, D = %d" % uniq)
        # ... on a row that is not selected the index is not looked at
        mask = np.random.default_rng(1).random(40_000) < 0.5
        mask[24_990:25_010] = True
        mask[25_000] = False
        run(gpu_ctx, [Case(gpu_ctx, col, pages, metas, mask, oracle=oracle, cp=cp)], "bad index on an unselected row")
    # the context still works
    col = gen.binary(9000, uniq=60)
    pages, metas = write(col, S.DICT, max_page_size=3000, force_codec=S.DICT)
    check_pages(gpu_ctx, col, pages, metas, what="after the corrupt pages")


# ---- 9: refusals at the call
def raw_call(ctx, arr, mem=None):
    from strawboat_amd import _native as N
    return ctx._lib.sb_read_selected_var(ctx._h, arr, len(arr), N.SB_MEM_DEVICE if mem is None else mem)


def test_refusals_at_the_call(gpu_ctx):
    import torch
    from strawboat_amd import _native as N
    from strawboat_amd.read_selected_var import ReadSelectedVarBatch
    dev = gpu_ctx.torch_device
    # every type that is not binary
    for col in (gen.boolean(3000), gen.prim(S.T_I32, 3000, uniq=10), gen.prim(S.T_F64, 3000, uniq=10), gen.prim(S.T_I128, 3000, uniq=10),
                dict(ptype=S.T_NULL, nullable=True, rows=3000, values=None, validity=None, offsets=None)):
        pages, metas = gen.oracle_write(col)
        cp = upload(gpu_ctx, col, pages, metas)
        m = cp.metas_array()
        arr = (N.ColumnReadSelectedVarC * 1)()
        c = arr[0]
        c.physical_type, c.is_nullable = col["ptype"], 0
        c.pages, c.pages_len = cp.pages.data_ptr() if cp.pages.numel() else 0, cp.pages.numel()
        c.metas, c.n_pages = m.ctypes.data_as(C.POINTER(N.PageMetaC)), m.shape[0]
        with torch.cuda.stream(gpu_ctx.torch_stream):
            bitmap = torch.full((((col["rows"] + 31) // 32) * 4,), 0xFF, dtype=torch.uint8, device=dev)
        values, offsets = Guarded(gpu_ctx, col["rows"] * 32), Guarded(gpu_ctx, (col["rows"] + 1) * 8)
        c.selection, c.selection_capacity = bitmap.data_ptr(), bitmap.numel()
        c.values, c.values_capacity = values.buf.data_ptr(), values.nbytes
        c.offsets, c.offsets_capacity = offsets.buf.data_ptr(), offsets.nbytes
        assert raw_call(gpu_ctx, arr) == N.SB_ERR_NYI, col["ptype"]
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        assert values.untouched() and offsets.untouched()
    # buffers
    col = gen.binary(5000, uniq=10, null_density=0.2, seed=2)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.NONE)
    oracle = oracle_strings(col, pages, metas)
    mask = np.ones(5000, bool)

    def fresh():
        a, b = Case(gpu_ctx, col, pages, metas, mask, oracle=oracle), Case(gpu_ctx, col, pages, metas, mask, oracle=oracle)
        return a, b, ReadSelectedVarBatch(gpu_ctx, [a.cp, b.cp], a.bitmap, out=[a.out(), b.out()])   # (ONE selection for both)

    def refused(a, b, batch, what, code=N.SB_ERR_INVALID, mem=None):
        assert raw_call(gpu_ctx, batch._arr, mem) == code, what
        gpu_ctx.synchronize()
        assert a.outputs_untouched() and b.outputs_untouched(), what

    a, b, batch = fresh()
    batch._arr[1].values = batch._arr[0].values + 8
    refused(a, b, batch, "values of two columns overlap")
    a, b, batch = fresh()
    batch._arr[1].validity = batch._arr[0].values + 64
    refused(a, b, batch, "validity inside another column's values")
    a, b, batch = fresh()
    batch._arr[1].offsets = batch._arr[0].offsets + 64
    refused(a, b, batch, "offsets of two columns overlap")
    a, b, batch = fresh()
    batch._arr[1].offsets = batch._arr[1].values + 64
    refused(a, b, batch, "offsets inside the column's own values")
    a, b, batch = fresh()
    batch._arr[0].values, batch._arr[0].values_capacity = batch._arr[1].selection, 64
    refused(a, b, batch, "values over a selection of the call")
    a, b, batch = fresh()
    batch._arr[0].offsets, batch._arr[0].offsets_capacity = batch._arr[1].selection, 64
    refused(a, b, batch, "offsets over a selection of the call")
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
    batch._arr[0].offsets = 0
    refused(a, b, batch, "no offsets")
    a, b, batch = fresh()
    batch._arr[0].offsets += 2
    refused(a, b, batch, "misaligned offsets")
    a, b, batch = fresh()
    batch._arr[0].offsets_capacity = 3
    refused(a, b, batch, "offsets without room for offsets[0]")
    a, b, batch = fresh()
    batch._arr[0].values = 0
    refused(a, b, batch, "values_capacity > 0 with null values")
    a, b, batch = fresh()
    refused(a, b, batch, "SB_MEM_HOST", code=N.SB_ERR_NYI, mem=N.SB_MEM_HOST)
    # two columns that share ONE selection are the usual case
    arrs = batch.enqueue()
    gpu_ctx.synchronize()
    a.check(arrs[0], "after the refusals")
    b.check(arrs[1], "after the refusals")
