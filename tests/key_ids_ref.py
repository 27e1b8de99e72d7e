"""The reference of sb_key_ids: the ORACLE's decode of the pages (tests/aggregate_ref.Ref, which is gen.oracle_read and
nothing else), np.unique of the live values for the keys and np.searchsorted for the ids.  Nothing here touches the device
or its decoder.

A row is live if its selection bit is set and it is not null.  The keys are the distinct values of the live rows, ascending
in the order of the column's own numpy dtype (integers by signedness); a row's id is the position of its value among them,
all ones in id_width bytes where the row is not live.  More distinct values than max_keys: overflow, and then n_keys, keys
and ids are unspecified (check() looks at none of them)."""
import numpy as np

from tests import gen
from tests.aggregate_ref import Ref  # noqa: F401  (the oracle's decode of a column, computed once)

NP = gen.NP_OF
ID_NP = {1: np.uint8, 2: np.uint16, 4: np.uint32}


class Want:
    """what one column of a call must give"""

    def __init__(self, rows, selected, count, max_keys, id_width, overflow, keys, ids):
        self.rows, self.selected, self.count = rows, selected, count
        self.max_keys, self.id_width, self.overflow = max_keys, id_width, overflow
        self.keys = keys   # typed array, ascending (None on overflow)
        self.ids = ids     # np.uint8 / uint16 / uint32 per row (None on overflow)
        self.n_keys = None if overflow else int(keys.size)

    @property
    def key_bytes(self):
        """the 8 * max_keys bytes of `keys`: a value's bytes little endian in the first `width` of its slot, zeros elsewhere"""
        out = np.zeros((self.max_keys, 8), np.uint8)
        w = self.keys.dtype.itemsize
        out[:self.n_keys, :w] = np.ascontiguousarray(self.keys).view(np.uint8).reshape(self.n_keys, w)
        return out.tobytes()


def key_ids_values(vals, live, selected, max_keys, id_width):
    """vals: the column's values as a typed array (any bytes in null slots); live: bool per row"""
    rows = int(live.size)
    vals = np.ascontiguousarray(vals[:rows])
    keys = np.unique(vals[live])
    if keys.size > max_keys:
        return Want(rows, selected, int(live.sum()), max_keys, id_width, True, None, None)
    none = (1 << (8 * id_width)) - 1
    ids = np.full(rows, none, ID_NP[id_width])
    ids[live] = np.searchsorted(keys, vals[live]).astype(ID_NP[id_width])
    return Want(rows, selected, int(live.sum()), max_keys, id_width, False, keys, ids)


def want(ref, mask, max_keys, id_width):
    """the Want of a column (an aggregate_ref.Ref) under a selection (a bool per row, or None: every row)"""
    sel = np.ones(ref.rows, bool) if mask is None else np.asarray(mask, bool)[:ref.rows]
    return key_ids_values(ref.vals, sel & ref.valid, int(sel.sum()), max_keys, id_width)


def ids_numpy(got):
    """the ids of a strawboat_amd.key_ids.KeyIds as unsigned integers of their width"""
    return got.ids.cpu().numpy().view(ID_NP[got.id_width])


def check(got, w, what=""):
    """got: a strawboat_amd.key_ids.KeyIds after the synchronize.  Every comparison is exact."""
    head = (got.rows, got.selected, got.count, got.overflow)
    assert head == (w.rows, w.selected, w.count, w.overflow), (
        "%s: rows / selected / count / overflow %r, want %r" % (what, head, (w.rows, w.selected, w.count, w.overflow)))
    if w.overflow:
        return
    assert got.n_keys == w.n_keys, "%s: n_keys %d, want %d" % (what, got.n_keys, w.n_keys)
    assert got.key_bytes == w.key_bytes, "%s: the bytes of keys differ (zeros behind the width and behind n_keys)" % what
    assert np.array_equal(got.keys, w.keys), what
    ids = ids_numpy(got)
    assert ids.size == w.rows
    bad = np.flatnonzero(ids != w.ids)
    assert bad.size == 0, "%s: %d ids differ, the first at row %d: %d, want %d" % (
        what, bad.size, bad[0], ids[bad[0]], w.ids[bad[0]])
