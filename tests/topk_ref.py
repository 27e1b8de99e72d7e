"""The reference of sb_topk_columns: the ORACLE's decode of the pages (tests/aggregate_ref.Ref, which is gen.oracle_read
and nothing else), ordered by numpy.  Nothing here touches the device or its decoder.

A row is live if its selection bit is set and it is not null; the candidates are the live rows that are not NaN.  They are
ordered by (value, row number): np.lexsort on (row, key), where `sort_keys` maps the values to integers that order as the
values must -- integers by signedness, floats numerically with -0.0 < +0.0 -- and is complemented for LARGEST, so that ties
go to the lower row number in both orders."""
import numpy as np

from oracle import sbo as S
from tests import gen
from tests.aggregate_ref import Ref  # noqa: F401  (the oracle's decode of a column, computed once)

NP = gen.NP_OF
FLOATS = (S.T_F32, S.T_F64)
KS = (1, 7, 64, 256)


def sort_keys(ptype, vals):
    """Integers (signed or unsigned, of the values' width) whose order is the order of the values.  Integers are their own
    keys.  A float's bits read as a signed integer order the non-negative floats already; the negative ones come out in
    reverse, and flipping their 31 / 63 value bits turns them round while keeping them below zero: -0.0 becomes -1, just
    below +0.0 = 0.  Not for NaNs."""
    vals = np.ascontiguousarray(vals)
    if ptype not in FLOATS:
        return vals
    s = vals.view("<i%d" % vals.dtype.itemsize)
    return np.where(s < 0, s ^ np.iinfo(s.dtype).max, s)


class Want:
    """what one column of a call must give"""

    def __init__(self, rows, selected, count, nans, k, row_ids, value_bytes):
        self.rows, self.selected, self.count, self.nans, self.k = rows, selected, count, nans, k
        self.row_ids = row_ids           # np.uint64[found]
        self.value_bytes = value_bytes   # np.uint8[found, 8]
        self.found = int(row_ids.size)

    @property
    def out_bytes(self):
        """the k entries of `out`: { row, value } of 16 bytes each, zeros behind `found`"""
        out = np.zeros((self.k, 16), np.uint8)
        out[:self.found, :8] = self.row_ids.astype("<u8").view(np.uint8).reshape(self.found, 8)
        out[:self.found, 8:] = self.value_bytes
        return out.tobytes()


def topk_values(ptype, vals, live, selected, k, largest):
    """vals: the column's values as a typed array (any bytes in null slots); live: bool per row"""
    rows = int(live.size)
    vals = np.ascontiguousarray(vals[:rows])
    w = vals.dtype.itemsize
    nan = np.isnan(vals) & live if ptype in FLOATS else np.zeros(rows, bool)
    idx = np.flatnonzero(live & ~nan)
    keys = sort_keys(ptype, vals[idx])
    if largest:
        keys = ~keys   # (-x - 1 for signed keys, max - x for unsigned ones: the order turned round, no overflow)
    best = idx[np.lexsort((idx, keys))[:k]]
    vb = np.zeros((best.size, 8), np.uint8)
    vb[:, :w] = vals[best].view(np.uint8).reshape(best.size, w)
    return Want(rows, selected, int(live.sum()), int(nan.sum()), k, best.astype(np.uint64), vb)


def want(ref, mask, k, largest):
    """the Want of a column (an aggregate_ref.Ref) under a selection (a bool per row, or None: every row)"""
    sel = np.ones(ref.rows, bool) if mask is None else np.asarray(mask, bool)[:ref.rows]
    return topk_values(ref.ptype, ref.vals, sel & ref.valid, int(sel.sum()), k, largest)


def check(got, w, what=""):
    """got: a strawboat_amd.topk.TopK after the synchronize.  Every comparison is exact."""
    head = (got.rows, got.selected, got.count, got.nans, got.found)
    assert head == (w.rows, w.selected, w.count, w.nans, w.found), (
        "%s: rows / selected / count / nans / found %r, want %r" % (what, head, (w.rows, w.selected, w.count, w.nans, w.found)))
    assert w.found == min(w.k, w.count - w.nans), what
    assert np.array_equal(got.row_ids, w.row_ids), "%s: rows %r, want %r" % (what, got.row_ids[:8], w.row_ids[:8])
    assert np.array_equal(got.value_bytes, w.value_bytes), "%s: value bytes differ" % what
    assert got.out_bytes == w.out_bytes, "%s: the bytes of out differ (the tail behind found is zero)" % what
