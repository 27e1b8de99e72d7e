"""The decoded route of the six sink kinds that have one, per codec (the table: tests/replay_cases.py), on the GPU.

Every case issues its victim calls alone in an interval, then in an interval that is issued again on the trigger's account
(a Freq column: in a call of its own before or behind the victim, or as one more column of the victim's call), then alone
once more.  Device outputs are 0xA5-filled buffers of exactly the documented capacities (a selected read's: the capacity
is a slice of a longer poisoned buffer, whose tail must stay untouched).  Every interval is compared with the oracle's
decode through the references of the kinds' suites, and the replay count (sb_ctx_replays) must go up by exactly one with
the trigger and by none without: that is what shows that the decoded routes were reached.  Then the victim's complete
result -- every byte of every device output buffer, poison included, and every host result field -- must be the same in
all three intervals: a column's result does not depend on what else the interval holds.  No expectation comes from the
device, and equality is byte equality; the only bound is aggregate_ref.float_sum_bound inside aggregate_ref.check.

sb_read_selected takes 8- to 64-bit numbers only (Int128 / Int256 are refused at the call), so the table holds no such column.

Measured on an MI355X: the module's 657 cases take 5.7 s, the slowest 0.25 s (the first, which uploads the long RLE page)."""
import ctypes as C

import numpy as np
import pytest

from oracle import sbo as S
from tests import aggregate_ref as R
from tests import key_ids_ref as K
from tests import replay_cases as RC
from tests import topk_ref as T

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD_BYTES = 256


def up(ctx, a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(ctx.torch_device)


def upload(ctx, col, pages, metas):
    from strawboat_amd import read
    return read.ColumnPages(col["ptype"], col["nullable"], up(ctx, pages), metas)


def poisoned(ctx, nbytes):
    import torch
    with torch.cuda.stream(ctx.torch_stream):   # (the fill is ordered before the call's kernels)
        return torch.full((int(nbytes),), POISON, dtype=torch.uint8, device=ctx.torch_device)


def sel_bytes(rows):
    return (rows + 31) // 32 * 4


def bits_of(mask):
    out = np.zeros(sel_bytes(mask.size), np.uint8)
    packed = np.packbits(mask, bitorder="little")
    out[:packed.size] = packed
    return out


def unpack(t, n):
    return np.unpackbits(t.cpu().numpy(), bitorder="little")[:n].astype(bool)


class Interval:
    """the calls of one interval, built before the first of them is enqueued"""

    def __init__(self, ctx, calls, cps):
        self.ctx, self.calls, self.cps = ctx, calls, cps
        self._chain = None
        self.issued = [ISSUE[c.kind](self, c) for c in calls]
        writers = [i for i in self.issued if i.call.kind in RC.FILTER_KINDS and i.call.buffer == "chain"]
        self.last_chain_writer = writers[-1] if writers else None

    def chain(self):
        """the bitmap the prelude writes and the victim reads (or combines into): one per interval"""
        if self._chain is None:
            self._chain = poisoned(self.ctx, sel_bytes(RC.ROWS))
        return self._chain

    def selection(self, sel, rows):
        """the device bitmap of an entry's selection argument: a reference mask, uploaded -- or the chained one"""
        if sel is None:
            return None
        return self.chain() if sel == "chain" else up(self.ctx, bits_of(RC.masks(rows)[sel]))

    def enqueue(self):
        for i in self.issued:
            i.enqueue()

    def check(self, wants, what):
        for n, (i, ws) in enumerate(zip(self.issued, wants)):
            i.check(ws, "%s, call %d (%s, %s)" % (what, n, i.call.kind, i.call.role))

    def snapshot(self):
        """[(label, {field: bytes or int})] of every entry that is not the trigger's"""
        out = []
        for n, i in enumerate(self.issued):
            if i.call.role == "trigger":
                continue
            k = 0
            for e, snap in zip(i.call.entries, i.snapshots()):
                if not e.trigger:
                    out.append(("%s call (%s), column %d" % (i.call.kind, i.call.role, k), snap))
                    k += 1
        return out


class Issued:
    def __init__(self, interval, call):
        self.iv, self.ctx, self.call = interval, interval.ctx, call
        self.cols = [RC.written(e.col)[0] for e in call.entries]
        self.rows = [c["rows"] for c in self.cols]
        self.cps = [interval.cps[e.col] for e in call.entries]

    def enqueue(self):
        self.res = self.batch.enqueue()


class FilterIssued(Issued):
    """sb_filter_columns_var / sb_filter_columns_in: SET into a poisoned buffer, AND / OR onto an uploaded bitmap or the chain"""

    def __init__(self, interval, call):
        import strawboat_amd as sb
        from strawboat_amd.filter import FilterBatch, Selection
        from strawboat_amd.filter_in import FilterInBatch
        super().__init__(interval, call)
        self.bufs = []
        for e, rows in zip(call.entries, self.rows):
            if call.buffer == "chain" and not e.trigger:
                self.bufs.append(interval.chain())
            elif call.buffer == "poison":
                self.bufs.append(poisoned(self.ctx, sel_bytes(rows)))
            else:
                self.bufs.append(up(self.ctx, bits_of(RC.masks(rows)[0])))
        out = [Selection(b, rows, None) for b, rows in zip(self.bufs, self.rows)]
        if call.kind == "filter":
            preds = [sb.Predicate(e.arg[0]) if e.arg[1] is None else sb.Predicate(*e.arg) for e in call.entries]
            self.batch = FilterBatch(self.ctx, self.cps, preds, combine=call.combine, out=out)
        else:
            lists = [sb.InList(list(e.arg[0]), negate=e.arg[1]) for e in call.entries]
            self.batch = FilterInBatch(self.ctx, self.cps, lists, combine=call.combine, out=out)

    def check(self, wants, what):
        for i, (sel, want, rows) in enumerate(zip(self.res, wants, self.rows)):
            assert sel.rows == rows and int(sel._c.rows) == rows, (what, i)
            assert sel.selected == int(want.sum()), "%s column %d: selected %d, want %d" % (what, i, sel.selected, int(want.sum()))
            if sel.bitmap is self.iv._chain and self is not self.iv.last_chain_writer:
                continue   # (a later call of the interval combined into the chained bitmap: its bits are that call's to check)
            got = unpack(sel.bitmap, sel.bitmap.numel() * 8)
            assert np.array_equal(got[:rows], want), "%s column %d: %d rows differ, first at %d" % (
                what, i, int((got[:rows] != want).sum()), int(np.argmax(got[:rows] != want)))
            if self.call.combine == "set":
                assert not got[rows:].any(), "%s column %d: bits behind the last row must be 0 after set" % (what, i)

    def snapshots(self):
        return [dict(bitmap=b.cpu().numpy().tobytes(), rows=int(s._c.rows), selected=s.selected) for b, s in zip(self.bufs, self.res)]


class ReadSelectedIssued(Issued):
    def __init__(self, interval, call):
        import strawboat_amd as sb
        super().__init__(interval, call)
        self.values, self.validity = [], []
        for col, rows in zip(self.cols, self.rows):
            self.values.append(poisoned(self.ctx, rows * S.WIDTH[col["ptype"]] + GUARD_BYTES))
            self.validity.append(poisoned(self.ctx, sel_bytes(rows) + GUARD_BYTES) if col["nullable"] else None)
        out = [(v[:v.numel() - GUARD_BYTES], None if b is None else b[:b.numel() - GUARD_BYTES]) for v, b in zip(self.values, self.validity)]
        sels = [interval.selection(e.arg, rows) for e, rows in zip(call.entries, self.rows)]
        self.batch = sb.ReadSelectedBatch(self.ctx, self.cps, sels, out=out)

    def check(self, wants, what):
        for i, (arr, mask, e) in enumerate(zip(self.res, wants, self.call.entries)):
            ref = RC.ref_of(e.col)
            w = ref.vals.dtype.itemsize
            sel = int(mask.sum())
            assert (arr.rows, arr.selected, arr.values_len) == (ref.rows, sel, sel * w), (what, i, arr.rows, arr.selected, arr.values_len)
            got = self.values[i].cpu().numpy()
            want = np.ascontiguousarray(ref.vals[mask]).view(np.uint8)
            bad = np.flatnonzero(got[:want.size] != want)
            assert bad.size == 0, "%s column %d: %d value bytes differ, first at output row %d" % (what, i, bad.size, bad[0] // w if bad.size else -1)
            assert (got[want.size:] == POISON).all(), "%s column %d: bytes behind values_len were written" % (what, i)
            if self.validity[i] is None:
                continue
            gb = self.validity[i].cpu().numpy()
            nwords = (sel + 31) // 32
            bits = np.unpackbits(gb[:nwords * 4], bitorder="little").astype(bool)
            assert np.array_equal(bits[:sel], ref.valid[mask]), "%s column %d: validity differs" % (what, i)
            assert not bits[sel:].any(), "%s column %d: bits >= selected of the last validity word must be 0" % (what, i)
            assert (gb[nwords * 4:] == POISON).all(), "%s column %d: validity words behind the last one were written" % (what, i)

    def snapshots(self):
        return [dict(values=v.cpu().numpy().tobytes(), validity=b"" if b is None else b.cpu().numpy().tobytes(), rows=a.rows,
                     selected=a.selected, values_len=a.values_len) for v, b, a in zip(self.values, self.validity, self.res)]


class AggregateIssued(Issued):
    def __init__(self, interval, call):
        import strawboat_amd as sb
        super().__init__(interval, call)
        sels = [interval.selection(e.arg, rows) for e, rows in zip(call.entries, self.rows)]
        self.batch = sb.AggregateBatch(self.ctx, self.cps, sels)

    def check(self, wants, what):
        for i, (r, want) in enumerate(zip(self.res, wants)):
            R.check(r, want, "%s column %d" % (what, i))

    def snapshots(self):
        return [dict(rows=r.rows, selected=r.selected, count=r.count, nans=r.nans, sum_lo=int(r._c.sum_lo), sum_hi=int(r._c.sum_hi),
                     min_bytes=r.min_bytes, max_bytes=r.max_bytes) for r in self.res]


class TopkIssued(Issued):
    def __init__(self, interval, call):
        from strawboat_amd.topk import TopKBatch
        super().__init__(interval, call)
        sels = [interval.selection(e.arg[0], rows) for e, rows in zip(call.entries, self.rows)]
        self.batch = TopKBatch(self.ctx, self.cps, [e.arg[1] for e in call.entries], [e.arg[2] for e in call.entries], sels)
        for r in self.batch.results:   # `out` is a host buffer of exactly k entries: every byte of it is written
            C.memset(r._out, POISON, C.sizeof(r._out))

    def check(self, wants, what):
        for i, (r, want) in enumerate(zip(self.res, wants)):
            T.check(r, want, "%s column %d" % (what, i))

    def snapshots(self):
        return [dict(rows=r.rows, selected=r.selected, count=r.count, nans=r.nans, found=r.found, out=r.out_bytes) for r in self.res]


class KeyIdsIssued(Issued):
    ID_TORCH = {1: "uint8", 2: "uint16", 4: "int32"}

    def __init__(self, interval, call):
        import torch
        from strawboat_amd.key_ids import KeyIdsBatch
        super().__init__(interval, call)
        sels = [interval.selection(e.arg[0], rows) for e, rows in zip(call.entries, self.rows)]
        self.ids = [poisoned(self.ctx, rows * e.arg[2]) for e, rows in zip(call.entries, self.rows)]   # exactly `rows` ids
        out = [b.view(getattr(torch, self.ID_TORCH[e.arg[2]])) for b, e in zip(self.ids, call.entries)]
        self.batch = KeyIdsBatch(self.ctx, self.cps, sels, [e.arg[1] for e in call.entries], [e.arg[2] for e in call.entries], out)
        for r in self.batch.results:   # `keys` is a host buffer of exactly 8 * max_keys bytes: every byte of it is written
            C.memset(r._keys, POISON, C.sizeof(r._keys))

    def check(self, wants, what):
        self.wants = wants
        for i, (r, want) in enumerate(zip(self.res, wants)):
            K.check(r, want, "%s column %d" % (what, i))

    def snapshots(self):
        out = []
        for r, b, want in zip(self.res, self.ids, self.wants):
            snap = dict(rows=r.rows, selected=r.selected, count=r.count, overflow=r.overflow)
            if not want.overflow:   # (after an overflow n_keys, keys and ids are unspecified)
                snap.update(n_keys=r.n_keys, keys=r.key_bytes, ids=b.cpu().numpy().tobytes())
            out.append(snap)
        return out


ISSUE = {"filter": FilterIssued, "filter_in": FilterIssued, "read_selected": ReadSelectedIssued, "aggregate": AggregateIssued,
         "topk": TopkIssued, "key_ids": KeyIdsIssued}


def _show(v):
    return v if isinstance(v, int) else "%d bytes" % len(v) if len(v) > 64 else v.hex()


def same_snapshot(alone, other, what):
    assert [label for label, _ in alone] == [label for label, _ in other]
    for (label, a), (_, b) in zip(alone, other):
        for field in a:
            if a[field] == b[field]:
                continue
            at = ""
            if not isinstance(a[field], int) and len(a[field]) == len(b[field]):
                at = ", first at byte %d" % next(i for i, (x, y) in enumerate(zip(a[field], b[field])) if x != y)
            raise AssertionError("%s: %s, %s: alone %s, %s %s%s" % (what, label, field, _show(a[field]), what, _show(b[field]), at))


@pytest.mark.parametrize("case", RC.CASES, ids=repr)
def test_case(gpu_ctx, case):
    ctx = gpu_ctx
    cps = {cid: upload(ctx, *RC.written(cid)) for cid in case.columns()}
    codecs, _ = RC.page_codecs(case.column.id)
    assert codecs == {RC.CODECS[case.column.codec][0]} and S.FREQ in RC.page_codecs(RC.trigger_id(case.column.rows))[0]

    def run(with_trigger, what):
        calls = case.calls(with_trigger)
        wants = RC.wants_of(calls)
        iv = Interval(ctx, calls, cps)
        r0 = ctx.replays()
        iv.enqueue()
        ctx.synchronize()
        replays = ctx.replays() - r0
        assert replays == (1 if with_trigger else 0), "%s: %d replays" % (what, replays)
        iv.check(wants, what)
        return iv.snapshot()

    alone = run(False, "alone")
    same_snapshot(alone, run(True, "next to the trigger"), "next to the trigger")
    same_snapshot(alone, run(False, "alone again"), "alone again")
