"""Device calls stay inside the caller's buffers, wherever those lie.

Every output buffer of every call here is `whole[F : F + cap]` of one tensor filled with 0xA5 on the context's stream: `cap`
is exactly the capacity include/strawboat_hip.h documents, 4096 guard bytes lie in front of it and 4096 behind, and F is
4096 plus a shift (the element width, 4 / 12 for bitmaps, 1 / 7 for value bytes).  After the synchronize both guards must
still be 0xA5 and the requested bytes must equal the CPU oracle's decode of the same pages.  The buffers of one call are
neighbours in one tensor, so a store that leaves one of them is seen whichever way it goes.  The inputs get the same
treatment: `pages` at every byte offset inside junk (parts C, D), pages scattered and listed in `page_offsets` (part D).

The case table is tests/buffer_cases.py (tests/test_buffer_cases.py walks it on the CPU); the columns of one (type, option
set) go into ONE call.  A device refusal of a table case is a failure: nothing here catches an exception.
No buffer sits at the end of an allocation, so a stray access is a wrong byte here, never a fault."""
import ctypes as C
import types

import numpy as np
import pytest

from oracle import sbo as S
from tests import buffer_cases as B
from tests.test_gpu_filter_binary import expected as expected_strings, oracle_strings

pytestmark = pytest.mark.gpu

GUARD, FILL = 4096, 0xA5
NUMPY_OF = {S.T_I8: np.int8, S.T_I16: np.int16, S.T_I32: np.int32, S.T_U32: np.uint32, S.T_I64: np.int64,
            S.T_F32: np.float32, S.T_F64: np.float64}
NUMERIC = tuple(NUMPY_OF)            # the types sb_filter_columns compares and sb_read_selected reads
FILTERABLE = NUMERIC + B.BINARIES


class Arena:
    """The output buffers of one call, carved out of one 0xA5 tensor: add() before allocate(), the rest after."""

    def __init__(self, guard=GUARD):
        self.guard, self.size, self.bufs, self.whole, self.host = guard, 0, [], None, None

    def add(self, cap, shift, label):
        f = self.size + self.guard + shift
        self.bufs.append((f, cap, label))
        self.size = -(-(f + cap + self.guard) // 512) * 512
        return len(self.bufs) - 1

    def allocate(self, ctx):
        import torch
        with torch.cuda.stream(ctx.torch_stream):
            self.whole = torch.full((max(self.size, 512),), FILL, dtype=torch.uint8, device=ctx.torch_device)
        assert self.whole.data_ptr() % 512 == 0
        return self

    def view(self, k):
        f, cap, _ = self.bufs[k]
        return self.whole[f:f + cap]

    def ptr(self, k):
        return self.whole.data_ptr() + self.bufs[k][0]

    def fetch(self):
        """after the synchronize: the whole tensor on the host; both guards of every buffer must be untouched"""
        self.host = h = self.whole.cpu().numpy()
        outside = np.ones(h.size, bool)
        for f, cap, _ in self.bufs:
            outside[f:f + cap] = False
        bad = np.flatnonzero(outside & (h != FILL))
        if bad.size:
            at = int(bad[0])
            near = min(self.bufs, key=lambda b: min(abs(at - b[0]), abs(at - (b[0] + b[1]))))
            side = "front guard, %d bytes before the buffer" % (near[0] - at) if at < near[0] else \
                "back guard, %d bytes behind the buffer's %d" % (at - near[0] - near[1], near[1])
            pytest.fail("%d guard bytes overwritten, the first in the %s of %s" % (bad.size, side, near[2]))
        return h

    def bytes(self, k, n=None):
        f, cap, _ = self.bufs[k]
        return self.host[f:f + (cap if n is None else n)]

    def untouched(self, k, start=0):
        return bool((self.bytes(k)[start:] == FILL).all())


class Inputs:
    """The input bytes of one call in one device tensor: add(bytes, shift) puts them `shift` bytes behind a multiple of 512
    with `junk` around them."""

    def __init__(self, junk=0x5A):
        self.junk, self.parts, self.size, self.dev = junk, [], 0, None

    def add(self, data, shift=0):
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        at = self.size + 512 + shift
        self.parts.append((at, data))
        self.size = -(-(at + data.size + 64) // 512) * 512
        return len(self.parts) - 1

    def upload(self, ctx):
        import torch
        host = np.full(self.size + 512, self.junk, np.uint8)
        for at, data in self.parts:
            host[at:at + data.size] = data
        with torch.cuda.stream(ctx.torch_stream):
            self.dev = torch.from_numpy(host).to(ctx.torch_device)
        assert self.dev.data_ptr() % 512 == 0
        return self

    def view(self, k, length=None):
        at, data = self.parts[k]
        return self.dev[at:at + (data.size if length is None else length)]


def value_shifts(ptype):
    if ptype in B.BINARIES:
        return (0, 1, 7)           # value bytes: any byte
    if ptype == S.T_BOOL:
        return (0, 4, 12)          # a bitmap: 32-bit words
    if ptype in (S.T_I128, S.T_I256):
        return (0, 16, 0)
    return (0, S.WIDTH[ptype], 0)  # the element's natural alignment


BITMAP_SHIFTS = (0, 4, 12)


def offsets_shift(ptype, variant):
    return (0, B.width_of(ptype))[variant % 2]


# ================================================================ A. sb_read_columns outputs
class ReadCall:
    """One sb_read_columns call over `items` = [(case, pages tensor, page_offsets or None)] into guarded buffers of exactly
    the documented capacities; check() compares every buffer with the oracle."""

    def __init__(self, ctx, items, variant=0, guard=GUARD):
        from strawboat_amd import read
        self.ctx, self.items = ctx, items
        self.arena = arena = Arena(guard)
        slots = []
        for case, _, _ in items:
            t = case.col["ptype"]
            vcap, ocap, bcap = B.capacities(case)
            slots.append((arena.add(vcap, value_shifts(t)[variant], "values of " + case.name),
                          arena.add(ocap, offsets_shift(t, variant), "offsets of " + case.name) if t in B.BINARIES else None,
                          arena.add(bcap, BITMAP_SHIFTS[variant], "validity of " + case.name) if case.col["nullable"] else None))
        arena.allocate(ctx)
        cols, out = [], []
        for (case, pages, po), (v, o, b) in zip(items, slots):
            col = case.col
            cols.append(read.ColumnPages(col["ptype"], col["nullable"], pages, B.pages_of(case)[1], po))
            out.append(types.SimpleNamespace(values=arena.view(v), offsets=None if o is None else arena.view(o),
                                             validity=None if b is None else arena.view(b)))
        self.slots = slots
        self.batch = read.ReadBatch(ctx, cols, out=out)
        for i, (v, _, _) in enumerate(slots):   # a binary column without a value byte: a buffer of capacity 0 is still a buffer
            if arena.bufs[v][1] == 0:
                self.batch._arr[i].values = arena.ptr(v)

    def run(self):
        self.batch.enqueue()
        self.ctx.synchronize()
        self.arena.fetch()
        return self

    def check(self):
        arena = self.arena
        for i, ((case, _, _), (v, o, b)) in enumerate(zip(self.items, self.slots)):
            col, want = case.col, B.pages_of(case)[2]
            t, rows = col["ptype"], col["rows"]
            c = self.batch._arr[i]
            assert int(c.rows) == rows, case
            if t == S.T_BOOL:
                assert np.array_equal(B.mask_bits(arena.bytes(v), rows), B.mask_bits(want["values"], rows)), "values of %s" % case
            else:
                n = want["values"].size
                assert n == arena.bufs[v][1]
                if t in B.BINARIES:
                    assert int(c.values_len) == n, case
                got = arena.bytes(v)
                assert np.array_equal(got, want["values"]), "values of %s: first difference at byte %d of %d" % (
                    case, int(np.argmax(got != want["values"])), n)
            if o is not None:
                assert np.array_equal(arena.bytes(o), want["offsets"]), "offsets of %s" % case
            if b is not None:
                assert np.array_equal(B.mask_bits(arena.bytes(b), rows), B.mask_bits(want["validity"], rows)), "validity of %s" % case


def back_to_back(ctx, cases, junk=0x5A):
    """[(case, pages tensor, None)]: every case's pages in a tensor slice of its own, 512-byte aligned like a fresh tensor"""
    inp = Inputs(junk)
    ks = [inp.add(B.pages_of(case)[0]) for case in cases]
    inp.upload(ctx)
    return [(case, inp.view(k), None) for case, k in zip(cases, ks)]


@pytest.mark.parametrize("group", B.groups(), ids=B.group_id)
def test_read_outputs_stay_inside_their_buffers(gpu_ctx, group):
    cases = B.table(*group)
    items = back_to_back(gpu_ctx, cases)
    for variant in range(3):
        ReadCall(gpu_ctx, items, variant).run().check()


@pytest.mark.parametrize("group", B.ladder_groups(), ids=B.ladder_group_id)
def test_read_outputs_of_the_string_ladder(gpu_ctx, group):
    cases = B.ladder_table(*group)
    items = back_to_back(gpu_ctx, cases)
    for variant in range(3):
        ReadCall(gpu_ctx, items, variant).run().check()


# ================================================================ B. selection bitmaps and selected reads
# the codecs a filter walks in a way of its own, forced; Rle is no codec of a binary column
PLAIN_SETS = [B.OptionSet("none", dict(force_codec=S.NONE), S.NONE, FILTERABLE),
              B.OptionSet("rle", dict(force_codec=S.RLE), S.RLE, NUMERIC),
              B.OptionSet("dict", dict(force_codec=S.DICT), S.DICT, FILTERABLE),
              B.OptionSet("freq", dict(force_codec=S.FREQ), S.FREQ, FILTERABLE),
              B.OptionSet("lz4", dict(force_codec=S.LZ4), S.LZ4, FILTERABLE)]
SEL_ROWS = (1, 33, 4097, 8193)
_SEL_CASES = {}


def selection_cases(ptypes, osets=PLAIN_SETS, rows_list=SEL_ROWS):
    out = []
    for t in ptypes:
        for oset in osets:
            key = (t, oset.name, rows_list)
            if key not in _SEL_CASES:
                _SEL_CASES[key] = [
                    B.Case("%s-%s-r%d-%s-p%s" % (B.TYPE_NAMES[t], oset.name, rows, "null" if nullable else "req", mps or "one"),
                           B.make_column(t, rows, nullable), dict(oset.opt, max_page_size=mps), oset.forced)
                    for rows in rows_list for nullable in (False, True) for mps in B.pagings(rows)] if oset.applies(t) else []
            out += _SEL_CASES[key]
    return out


def predicate_of(case):
    """one predicate per type that selects some rows and not all: (op, literal)"""
    return ("ge", b"w15") if case.col["ptype"] in B.BINARIES else ("lt", 100)


def wanted_bits(case):
    """bool[rows]: the predicate over the oracle's decode, row by row; null rows satisfy nothing (computed once per case)"""
    if getattr(case, "bits", None) is None:
        col = case.col
        pages, metas, want = B.pages_of(case)
        op, lit = predicate_of(case)
        rows = col["rows"]
        if col["ptype"] in B.BINARIES:
            strs, valid = oracle_strings(col, pages, metas)
            bits = expected_strings(strs, valid, op, lit)
        else:
            valid = np.unpackbits(want["validity"], bitorder="little")[:rows].astype(bool) if col["nullable"] else np.ones(rows, bool)
            vals = want["values"].view(NUMPY_OF[col["ptype"]])
            bits = (vals < NUMPY_OF[col["ptype"]](lit)) & valid
        bits.setflags(write=False)
        case.bits = bits
    return case.bits


def wanted_selection(case, mode):
    """the bytes of the selection buffer (capacity 4*ceil(rows/32)) after a filter call on a buffer of 0xA5 bytes: SET writes
    the bits behind the last row as 0, AND / OR leave them as they are"""
    rows = case.col["rows"]
    bits = np.zeros(B.bitmap_bytes(rows) * 8, bool)
    bits[:rows] = wanted_bits(case)
    prior = np.unpackbits(np.full(B.bitmap_bytes(rows), FILL, np.uint8), bitorder="little").astype(bool)
    if mode == "and":
        res = np.where(np.arange(bits.size) < rows, bits & prior, prior)
    elif mode == "or":
        res = np.where(np.arange(bits.size) < rows, bits | prior, prior)
    else:
        res = bits
    return np.packbits(res, bitorder="little"), int(res[:rows].sum())


class FilterCall:
    """One sb_filter_columns_var (or, fixed=True, sb_filter_columns) call over `items` into guarded selection buffers of
    exactly 4*ceil(rows/32) bytes that hold 0xA5 before the call."""

    def __init__(self, ctx, items, mode, shift, fixed=False, guard=GUARD):
        import strawboat_amd as sb
        from strawboat_amd import _native as N, filter as F, read
        self.ctx, self.items, self.mode, self.fixed = ctx, items, mode, fixed
        self.arena = arena = Arena(guard)
        self.slots = [arena.add(B.bitmap_bytes(case.col["rows"]), shift, "selection of " + case.name) for case, _, _ in items]
        arena.allocate(ctx)
        cols = [read.ColumnPages(case.col["ptype"], case.col["nullable"], pages, B.pages_of(case)[1], po) for case, pages, po in items]
        out = [F.Selection(arena.view(k), case.col["rows"], None) for k, (case, _, _) in zip(self.slots, items)]
        preds = [sb.Predicate(*predicate_of(case)) for case, _, _ in items]
        # (what the value blocks of a binary column's LZ4 / Zstd / Snappy pages inflate to: a bound, no buffer of the caller's)
        stage = [2 * B.pages_of(case)[2]["values"].size + 8 * case.col["rows"] + 4096 if case.col["ptype"] in B.BINARIES else 0
                 for case, _, _ in items]
        self.batch = F.FilterBatch(ctx, cols, preds, combine=mode, out=out, stage_capacity=stage)
        self.arr = self.batch._arr
        if fixed:   # the same descriptors for the call with the 8-byte literal
            self.arr = arr = (N.ColumnFilterC * len(items))()
            for i, (case, _, _) in enumerate(items):
                v, c = self.batch._arr[i], arr[i]
                for f in ("physical_type", "is_nullable", "pages", "pages_len", "metas", "n_pages", "page_offsets", "op", "combine",
                          "selection", "selection_capacity"):
                    setattr(c, f, getattr(v, f))
                lit = F.pack_literal(case.col["ptype"], predicate_of(case)[1])
                C.memmove(c.literal, lit, 8)

    def enqueue(self):
        ctx = self.ctx
        if self.fixed:
            from strawboat_amd import _native as N
            ctx._keep.append(self)
            ctx._check(ctx._lib.sb_filter_columns(ctx._h, self.arr, len(self.items), N.SB_MEM_DEVICE))
        else:
            self.batch.enqueue()
        return self

    def run(self):
        self.enqueue()
        self.ctx.synchronize()
        self.arena.fetch()
        return self

    def check(self):
        for i, ((case, _, _), k) in enumerate(zip(self.items, self.slots)):
            want, selected = wanted_selection(case, self.mode)
            got = self.arena.bytes(k)
            assert np.array_equal(got, want), "selection of %s (%s): first difference in byte %d of %d" % (
                case, self.mode, int(np.argmax(got != want)), want.size)
            assert int(self.arr[i].rows) == case.col["rows"] and int(self.arr[i].selected) == selected, case


@pytest.mark.parametrize("shift", (0, 4, 8, 12))
@pytest.mark.parametrize("mode", ("set", "and", "or"))
def test_selection_bitmaps_stay_inside_their_buffers(gpu_ctx, mode, shift):
    items = back_to_back(gpu_ctx, selection_cases(FILTERABLE))
    FilterCall(gpu_ctx, items, mode, shift).run().check()
    numeric = [it for it in items if it[0].col["ptype"] in NUMERIC]
    FilterCall(gpu_ctx, numeric, mode, shift, fixed=True).run().check()


SELECTIONS = {"none": lambda rows: np.zeros(rows, bool), "all": lambda rows: np.ones(rows, bool),
              "every 7th": lambda rows: np.arange(rows) % 7 == 0}


class SelectedCall:
    """One sb_read_selected call over `items` with the selection `which`: `values` of exactly selected * width bytes and
    `validity` of exactly 4*ceil(selected/32), guarded on both sides; where nothing is selected the buffers have the
    capacities that are always enough (rows * width, 4*ceil(rows/32)) and must stay as they were."""

    def __init__(self, ctx, items, which, variant=0, guard=GUARD):
        from strawboat_amd import read
        from strawboat_amd.read_selected import ReadSelectedBatch
        self.ctx, self.items = ctx, items
        self.arena = arena = Arena(guard)
        inp = Inputs(0xFF)   # (bits behind the last row of a selection are set: they are ignored)
        self.masks, self.slots, sel_k = [], [], []
        for case, _, _ in items:
            col = case.col
            rows, w = col["rows"], S.WIDTH[col["ptype"]]
            mask = SELECTIONS[which](rows)
            bits = np.ones(B.bitmap_bytes(rows) * 8, bool)
            bits[:rows] = mask
            sel_k.append(inp.add(np.packbits(bits, bitorder="little")))
            n = int(mask.sum())
            self.masks.append(mask)
            self.slots.append((arena.add(n * w if n else rows * w, (0, w, 0)[variant], "selected values of " + case.name),
                               arena.add(B.bitmap_bytes(n if n else rows), BITMAP_SHIFTS[variant], "selected validity of " + case.name)
                               if col["nullable"] else None))
        arena.allocate(ctx)
        inp.upload(ctx)
        cols = [read.ColumnPages(case.col["ptype"], case.col["nullable"], pages, B.pages_of(case)[1], po) for case, pages, po in items]
        out = [(arena.view(v), None if b is None else arena.view(b)) for v, b in self.slots]
        self.batch = ReadSelectedBatch(ctx, cols, [inp.view(k) for k in sel_k], out=out)

    def run(self):
        self.batch.enqueue()
        self.ctx.synchronize()
        self.arena.fetch()
        return self

    def check(self):
        arena = self.arena
        for i, ((case, _, _), (v, b), mask) in enumerate(zip(self.items, self.slots, self.masks)):
            col, want = case.col, B.pages_of(case)[2]
            rows, w = col["rows"], S.WIDTH[col["ptype"]]
            n = int(mask.sum())
            c = self.batch._arr[i]
            assert (int(c.rows), int(c.selected), int(c.values_len)) == (rows, n, n * w), case
            assert np.array_equal(arena.bytes(v, n * w), want["values"].reshape(rows, w)[mask].reshape(-1)), "selected values of %s" % case
            assert arena.untouched(v, n * w), "values bytes behind values_len of %s" % case
            if b is not None:
                valid = np.unpackbits(want["validity"], bitorder="little")[:rows].astype(bool)[mask]
                words = B.bitmap_bytes(n)
                bits = np.zeros(words * 8, bool)   # bits >= selected of the last word written are 0
                bits[:n] = valid
                assert np.array_equal(arena.bytes(b, words), np.packbits(bits, bitorder="little")), "selected validity of %s" % case
                assert arena.untouched(b, words), "validity words behind the last of %s" % case


@pytest.mark.parametrize("which", list(SELECTIONS))
def test_selected_reads_stay_inside_their_buffers(gpu_ctx, which):
    items = back_to_back(gpu_ctx, selection_cases(NUMERIC))
    for variant in range(3):
        SelectedCall(gpu_ctx, items, which, variant).run().check()


# ================================================================ C. placement of the input
PLACE_SHIFTS = (1, 2, 3, 4, 7, 8, 15)
PLACE_ROWS = (33, 4097, 8193, 4224)   # (4224: the Bitpacking rows of the table between 4097 and 8193)


def placed(ctx, cases, junk):
    """[(case, pages tensor, None)] x PLACE_SHIFTS: the pages `shift` bytes behind a multiple of 512, junk all around"""
    inp = Inputs(junk)
    ks = [(case, inp.add(B.pages_of(case)[0], shift)) for case in cases for shift in PLACE_SHIFTS]
    inp.upload(ctx)
    items = [(case, inp.view(k), None) for case, k in ks]
    for (_, pages, _), (_, k) in zip(items, ks):
        assert pages.data_ptr() % 16 == inp.parts[k][0] % 16 != 0
    return items


@pytest.mark.parametrize("junk", (0x00, 0xFF))
@pytest.mark.parametrize("ptype", B.TYPES, ids=lambda t: B.TYPE_NAMES[t])
def test_results_do_not_depend_on_where_the_pages_lie(gpu_ctx, ptype, junk):
    """every call may read beyond a page inside the buffer; what it reads there (0x00 or 0xFF) must not show"""
    cases = [c for o in B.OPTION_SETS for c in B.table(ptype, o, PLACE_ROWS)]
    items = placed(gpu_ctx, cases, junk)
    ReadCall(gpu_ctx, items, 0, guard=256).run().check()
    if ptype in FILTERABLE:
        FilterCall(gpu_ctx, items, "set", 0, guard=256).run().check()
    if ptype in NUMERIC:
        FilterCall(gpu_ctx, items, "set", 0, fixed=True, guard=256).run().check()
        SelectedCall(gpu_ctx, items, "every 7th", 0, guard=256).run().check()


# ================================================================ D. page_offsets
OFFSET_TYPES = (S.T_I16, S.T_I32, S.T_I64, S.T_F64, S.T_BIN32, S.T_BIN64)
OFFSET_SETS = PLAIN_SETS + [B.OptionSet("zstd", dict(force_codec=S.ZSTD), S.ZSTD, FILTERABLE)]
OFFSET_PAGING = ((1000, None), (4097, 3000), (8193, 1000))   # columns of 1, 2 and 9 pages
_OFFSET_CASES = []


def offset_cases():
    if not _OFFSET_CASES:
        for t in OFFSET_TYPES:
            for oset in OFFSET_SETS:
                if oset.applies(t):
                    for rows, mps in OFFSET_PAGING:
                        for nullable in (False, True):
                            name = "%s-%s-r%d-%s-p%s" % (B.TYPE_NAMES[t], oset.name, rows, "null" if nullable else "req", mps or "one")
                            _OFFSET_CASES.append(B.Case(name, B.make_column(t, rows, nullable), dict(oset.opt, max_page_size=mps), oset.forced))
        for case in _OFFSET_CASES:
            assert B.pages_of(case)[1].shape[0] == {None: 1, 3000: 2, 1000: 9}[case.opt["max_page_size"]]
    return _OFFSET_CASES


def scattered(ctx, cases, orders=("ascending", "descending")):
    """[(case, buffer tensor, page_offsets)]: every case back to back (page_offsets None) and once per order"""
    inp = Inputs(0x5A)
    plan = []
    for n, case in enumerate(cases):
        pages, metas, _ = B.pages_of(case)
        plan.append((case, inp.add(pages, n % 16), None))
        for order in orders:
            buf, offs = B.scatter(pages, metas, gaps=np.roll((1, 37, 7, 16, 3, 13, 32, 5, 21), n), order=order)
            assert np.array_equal(B.gather(buf, metas, offs), pages)
            plan.append((case, inp.add(buf, (n + 5) % 16), offs))
    inp.upload(ctx)
    return [(case, inp.view(k), po) for case, k, po in plan]


def same_as_back_to_back(call, items, slots_of):
    """the bytes of every scattered entry's buffers equal those of the back-to-back entry of the same case"""
    base = {}
    for i, (case, _, po) in enumerate(items):
        if po is None:
            base[case.name] = i
    for i, (case, _, po) in enumerate(items):
        for a, b in zip(slots_of(i), slots_of(base[case.name])):
            if a is not None:
                assert np.array_equal(call.arena.bytes(a), call.arena.bytes(b)), case


def as_tuple(s):
    return s if isinstance(s, tuple) else (s,)


def test_read_with_page_offsets(gpu_ctx):
    items = scattered(gpu_ctx, offset_cases())
    call = ReadCall(gpu_ctx, items, 0).run()
    call.check()
    same_as_back_to_back(call, items, lambda i: call.slots[i])


def test_filters_with_page_offsets(gpu_ctx):
    items = scattered(gpu_ctx, offset_cases())
    for fixed in (False, True):
        part = [it for it in items if not fixed or it[0].col["ptype"] in NUMERIC]
        call = FilterCall(gpu_ctx, part, "set", 0, fixed=fixed).run()
        call.check()
        same_as_back_to_back(call, part, lambda i: as_tuple(call.slots[i]))


def test_read_selected_with_page_offsets(gpu_ctx):
    items = [it for it in scattered(gpu_ctx, offset_cases()) if it[0].col["ptype"] in NUMERIC]
    call = SelectedCall(gpu_ctx, items, "every 7th", 0).run()
    call.check()
    same_as_back_to_back(call, items, lambda i: call.slots[i])


@pytest.mark.parametrize("over", ("one byte over", "at the end"))
def test_page_offsets_outside_the_buffer_are_refused(gpu_ctx, over):
    """offsets that do not wrap (the wrapping ones: tests/test_buffer_cases.py, on the CPU): SB_ERR_IO at the call, and no
    output buffer of the call is touched"""
    from strawboat_amd import _native as N
    cases = [c for c in offset_cases() if c.name in ("i32-none-r8193-null-p1000", "bin-dict-r4097-null-p3000", "i64-rle-r1000-req-pone")]
    assert len(cases) == 3
    for bad in range(len(cases)):
        items = scattered(gpu_ctx, cases, orders=("ascending",))
        items = [it for it in items if it[2] is not None]
        case, buf, offs = items[bad]
        offs = offs.copy()
        length = int(B.pages_of(case)[1][-1, 0])
        offs[-1] = buf.numel() - length + 1 if over == "one byte over" else buf.numel()
        items[bad] = (case, buf, offs)
        numeric = [it for it in items if it[0].col["ptype"] in NUMERIC]
        calls = [ReadCall(gpu_ctx, items), FilterCall(gpu_ctx, items, "set", 0)]
        if case.col["ptype"] in NUMERIC:
            calls += [FilterCall(gpu_ctx, numeric, "set", 0, fixed=True), SelectedCall(gpu_ctx, numeric, "all")]
        for call in calls:
            with pytest.raises(N.NativeError) as e:
                call.enqueue() if isinstance(call, FilterCall) else call.batch.enqueue()
            assert e.value.code == N.SB_ERR_IO and "page_offsets + length exceeds pages_len" in str(e.value)
            gpu_ctx.synchronize()
            call.arena.fetch()
            assert all(call.arena.untouched(k) for k in range(len(call.arena.bufs)))


# ================================================================ E. the writer and the nested level calls
WRITE_ROWS = (1, 129, 4224, 16896)
WRITE_PAGE = 65536
WRITE_SETS = [   # (name, options, types): Rle is no codec of a binary column, Dict none of a boolean one
    ("ratio2", dict(ratio=2.0), B.TYPES),
    ("lz4-ratio1.1", dict(ratio=1.1, default_compression=S.LZ4), B.TYPES),
    ("lz4", dict(default_compression=S.LZ4), B.TYPES),
    ("zstd", dict(default_compression=S.ZSTD), B.TYPES),
    ("rle", dict(force_codec=S.RLE), B.NOT_BINARY),
    ("dict", dict(force_codec=S.DICT), B.NOT_BOOLEAN),
    ("dict-lz4", dict(force_codec=S.DICT, force_index_codec=S.LZ4), B.NOT_BOOLEAN),
]


@pytest.mark.parametrize("name,opt,ptypes", WRITE_SETS, ids=[w[0] for w in WRITE_SETS])
def test_written_pages_stay_inside_the_write_bound(gpu_ctx, name, opt, ptypes):
    """out_pages of exactly sb_write_bound() bytes; the pages are the oracle's byte for byte (LZ4 blocks with the exact
    parse), Zstd pages are decoded by the oracle instead, as in tests/test_gpu_encode.py"""
    from strawboat_amd import _native as N, write
    from tests.test_gpu_encode import write_options
    ctx = gpu_ctx
    cols = [B.make_column(t, rows, nullable) for t in ptypes for rows in WRITE_ROWS for nullable in (False, True)]
    wo = write_options(max_page_size=WRITE_PAGE, **opt)
    oc = write.options_c(wo)
    inp = Inputs()
    ks = [tuple(None if col[f] is None else inp.add(col[f]) for f in ("values", "validity", "offsets")) for col in cols]
    inp.upload(ctx)
    dcs = [write.DeviceColumn(col["ptype"], col["nullable"], col["rows"], *(None if k is None else inp.view(k) for k in kk))
           for col, kk in zip(cols, ks)]
    arena = Arena()
    slots, out = [], []
    for col, dc in zip(cols, dcs):
        bound, npages = write.write_bound(ctx, dc, oc)
        assert bound > 0 and npages == 1
        slots.append(arena.add(bound, 0, "out_pages of %s rows %d nullable %s" % (B.TYPE_NAMES[col["ptype"]], col["rows"], col["nullable"])))
    arena.allocate(ctx)
    for k in slots:
        out.append(write.EncodedColumn(arena.view(k), (N.PageMetaC * 1)(), None))
    enc = write.WriteBatch(ctx, dcs, wo, out=out).enqueue()
    ctx.synchronize()
    arena.fetch()
    for col, e, k in zip(cols, enc, slots):
        what = arena.bufs[k][2]
        want_pages, want_metas = B.gen.oracle_write(col, max_page_size=WRITE_PAGE, **opt)
        assert e.length <= arena.bufs[k][1], what
        got, metas = arena.bytes(k, e.length), e.metas_array()
        if opt.get("default_compression") == S.ZSTD:
            assert int(metas[:, 1].sum()) == col["rows"] and int(metas[:, 0].sum()) == e.length, what
            back, want = B.gen.oracle_read(col, got, metas), B.gen.oracle_read(col, want_pages, want_metas)
            for f in ("values", "validity", "offsets"):
                assert np.array_equal(back[f], want[f]), "%s: %s decoded by the oracle" % (what, f)
        else:
            assert np.array_equal(metas, want_metas), what
            assert np.array_equal(got, want_pages), what


NESTED_SHAPES = ("list", "list_list", "list_struct", "struct_list")
NESTED_SEEDS = (1, 2)
NESTED_ROWS, NESTED_PAGE = 3000, 900


def nested_columns():
    from tests.nested_gen import make_nested
    return [(shape, seed) + make_nested(shape, NESTED_ROWS, seed) for shape in NESTED_SHAPES for seed in NESTED_SEEDS]


def test_nested_level_sections_stay_inside_the_levels_bound(gpu_ctx):
    """out_levels of exactly sb_nested_levels_bound() bytes: the sections are the oracle's, page by page"""
    from strawboat_amd import nested
    from tests.test_gpu_nested import device_levels
    ctx = gpu_ctx
    cols = nested_columns()
    lw = nested._LevelsWrite(ctx, [device_levels(ctx, levels) for _, _, levels, _ in cols], NESTED_PAGE)
    arena = Arena()
    slots = []
    for k, (shape, seed, levels, rows) in enumerate(cols):
        bound = int(ctx._lib.sb_nested_levels_bound(lw.keep[k][0], len(levels), rows, NESTED_PAGE))
        assert bound > 0
        slots.append(arena.add(bound, 0, "out_levels of %s seed %d" % (shape, seed)))
    arena.allocate(ctx)
    for k, s in enumerate(slots):
        lw.items[k].out_levels, lw.items[k].out_capacity = arena.ptr(s), arena.bufs[s][1]
    lw.call()
    ctx.synchronize()
    arena.fetch()
    for k, ((shape, seed, levels, rows), s) in enumerate(zip(cols, slots)):
        info = lw.info(k)
        want = [S.nested_write_levels(levels, r0, min(NESTED_PAGE, rows - r0)) for r0 in range(0, rows, NESTED_PAGE)]
        assert info.shape[0] == len(want)
        assert [tuple(int(x) for x in row) for row in info] == [(len(b), nv, ls, lc) for b, nv, ls, lc in want], arena.bufs[s][2]
        sections = np.concatenate([np.asarray(b, np.uint8) for b, _, _, _ in want])
        assert sections.size <= arena.bufs[s][1]
        assert np.array_equal(arena.bytes(s, sections.size), sections), arena.bufs[s][2]


def test_nested_level_outputs_stay_inside_their_buffers(gpu_ctx):
    """sb_nested_read_levels_batch: offsets, validity and leaf_validity at exactly the capacities strawboat_amd/nested.py
    gives them ((entries + 1) offsets, 4*ceil(entries/32) bitmap bytes), against the Arrow buffers the levels came from"""
    from strawboat_amd import _native as N
    from tests.nested_gen import expected_state
    from tests.test_gpu_nested import leaf_values, oracle_pages
    ctx = gpu_ctx
    cols = nested_columns()
    inp, arena = Inputs(), Arena()
    n = len(cols)
    items = (N.NestedLevelsReadC * n)()
    keep, plan = [], []
    for j, (shape, seed, levels, rows) in enumerate(cols):
        values, _ = leaf_values(levels, S.T_I32, 11)
        pages, metas = oracle_pages(levels, S.T_I32, values, rows, NESTED_PAGE, force_codec=S.NONE)
        metas = np.ascontiguousarray(metas, np.uint64)
        entries = int(metas[:, 1].sum())
        vbytes = max(B.bitmap_bytes(entries), 4)
        what = "%s seed %d" % (shape, seed)
        lv = (N.NestedLevelOutC * len(levels))()
        slots = []
        for k, l in enumerate(levels):
            lv[k].kind, lv[k].is_nullable = l["kind"], 1 if l["is_optional"] else 0
            o = arena.add((entries + 1) * 8, (0, 8)[(j + k) % 2], "offsets of level %d of %s" % (k, what)) \
                if l["kind"] in (S.K_LIST, S.K_LARGE_LIST) else None
            v = arena.add(vbytes, BITMAP_SHIFTS[(j + k) % 3], "validity of level %d of %s" % (k, what)) \
                if l["is_optional"] and l["kind"] != S.K_PRIMITIVE else None
            slots.append((o, v))
        leaf = arena.add(vbytes, BITMAP_SHIFTS[j % 3], "leaf_validity of " + what) if levels[-1]["is_optional"] else None
        counts, blocks = np.zeros(metas.shape[0], np.uint64), np.zeros(metas.shape[0], np.uint64)
        plan.append((inp.add(pages), metas, entries, lv, slots, leaf, counts, blocks))
    arena.allocate(ctx)
    inp.upload(ctx)
    for j, (pk, metas, entries, lv, slots, leaf, counts, blocks) in enumerate(plan):
        it = items[j]
        pages = inp.view(pk)
        keep.append(pages)
        it.pages, it.pages_len = pages.data_ptr(), pages.numel()
        it.metas, it.n_pages = metas.ctypes.data_as(C.c_void_p), metas.shape[0]
        it.levels, it.n_levels = lv, len(slots)
        for k, (o, v) in enumerate(slots):
            if o is not None:
                lv[k].offsets, lv[k].offsets_capacity = arena.ptr(o), entries + 1
            if v is not None:
                lv[k].validity, lv[k].validity_capacity = arena.ptr(v), arena.bufs[v][1]
        if leaf is not None:
            it.leaf_validity, it.leaf_validity_capacity = arena.ptr(leaf), arena.bufs[leaf][1]
        it.page_leaf_counts, it.page_block_offsets = counts.ctypes.data_as(C.c_void_p), blocks.ctypes.data_as(C.c_void_p)
    ctx._check(ctx._lib.sb_nested_read_levels_batch(ctx._h, items, n))
    ctx.synchronize()
    arena.fetch()

    def bits_of(slot, count):
        return np.unpackbits(arena.bytes(slot), bitorder="little")[:count].tolist()

    for (shape, seed, levels, rows), (pk, metas, entries, lv, slots, leaf, counts, blocks) in zip(cols, plan):
        want = expected_state(levels, 0, rows)
        assert [int(lv[k].length) for k in range(len(levels))] == want["lengths"], (shape, seed)
        assert int(counts.sum()) == want["leaf_count"]
        for k, (o, v) in enumerate(slots):
            if o is not None:
                offs = arena.bytes(o).view(np.int64)[:want["lengths"][k] + 1]
                assert offs[:-1].tolist() == want["offsets"][k] and int(offs[-1]) == want["lengths"][k + 1], arena.bufs[o][2]
            if v is not None:
                assert bits_of(v, want["lengths"][k]) == want["validity"][k], arena.bufs[v][2]
        if leaf is not None:
            assert bits_of(leaf, want["leaf_count"]) == want["leaf_validity"], arena.bufs[leaf][2]
