"""The reference of sb_key_buckets: ids and the five counts from decoded values, validity, mask, bounds, bucket ids and
nan_id, in numpy.  The values come from the ORACLE's decode of the pages (tests/aggregate_ref.Ref); nothing here touches
the device or its decoder.

A row is live if its selection bit is set and it is not null.  The bucket of a live value x that is not a NaN is
np.searchsorted(bounds, x, side="right") (the number of bounds <= x), side="left" with right_closed (the number of
bounds < x), both in the column's own dtype: no 64-bit integer goes through a float.  Its id is bucket_ids[bucket] (the
bucket's number without bucket_ids); NONE there means no id.  NaN rows are masked out first and get nan_id (None: no id).
Every other row, and a row without an id, gets all ones of id_width.  `matched` counts the live rows whose id is not all
ones, `nans` the live NaNs."""
import numpy as np

from tests.aggregate_ref import Ref  # noqa: F401  (the oracle's decode of a numeric column: .vals, .valid, .rows)

ID_NP = {1: np.uint8, 2: np.uint16, 4: np.uint32}
NONE = 0xFFFFFFFF


class Want:
    """what one column of a call must give"""

    def __init__(self, rows, selected, count, matched, nans, id_width, ids):
        self.rows, self.selected, self.count, self.matched, self.nans = rows, selected, count, matched, nans
        self.id_width, self.ids = id_width, ids


def bucket_values(vals, live, selected, bounds, bucket_ids, right_closed, nan_id, id_width):
    """vals: one value per row as a typed array (anything in null slots); live: bool per row; bounds: strictly
    increasing, of vals' dtype; bucket_ids: n_bounds + 1 ids (None / NONE: no id) or None"""
    rows = int(live.size)
    none = (1 << (8 * id_width)) - 1
    bounds = np.asarray(bounds)
    assert bounds.dtype == vals.dtype and bounds.ndim == 1, "the bounds are compared in the column's own dtype"
    n = bounds.size
    if bucket_ids is None:
        id_of = np.arange(n + 1, dtype=np.int64)
    else:
        id_of = np.array([NONE if v is None else int(v) for v in bucket_ids], np.int64)
    assert id_of.size == n + 1 and (((0 <= id_of) & (id_of < none)) | (id_of == NONE)).all(), "an id does not fit the width"
    id_of = np.where(id_of == NONE, none, id_of)
    ids = np.full(rows, none, ID_NP[id_width])
    nan = live & np.isnan(vals) if vals.dtype.kind == "f" else np.zeros(rows, bool)
    at = np.flatnonzero(live & ~nan)
    b = np.searchsorted(bounds, vals[at], side="left" if right_closed else "right")
    ids[at] = id_of[b].astype(ID_NP[id_width])
    if nan_id is not None and nan_id != NONE:
        assert vals.dtype.kind == "f" and 0 <= nan_id < none
        ids[nan] = nan_id
    matched = int((ids[live] != none).sum())
    return Want(rows, selected, int(live.sum()), matched, int(nan.sum()), id_width, ids)


def want(ref, mask, bounds, bucket_ids=None, right_closed=False, nan_id=None, id_width=2):
    """the Want of a column (a Ref) under a selection (a bool per row, or None: every row)"""
    sel = np.ones(ref.rows, bool) if mask is None else np.asarray(mask, bool)[:ref.rows]
    return bucket_values(ref.vals[:ref.rows], sel & ref.valid, int(sel.sum()), bounds, bucket_ids, right_closed, nan_id, id_width)


def histogram(ref, mask, bounds, right_closed=False):
    """the n_bounds + 1 counts of the live rows that are not NaN"""
    w = want(ref, mask, bounds, None, right_closed, None, 4)
    live = w.ids != 0xFFFFFFFF
    return np.bincount(w.ids[live].astype(np.int64), minlength=len(bounds) + 1)


def ids_numpy(got):
    """the ids of a strawboat_amd.key_buckets.KeyBuckets as unsigned integers of their width"""
    return got.ids.cpu().numpy().view(ID_NP[got.id_width])


def check(got, w, what=""):
    """got: a KeyBuckets after the synchronize.  Every comparison is exact: the bytes of ids and the five counts."""
    head = (got.rows, got.selected, got.count, got.matched, got.nans)
    print("%s: rows / selected / count / matched / nans %r" % (what, head))
    assert head == (w.rows, w.selected, w.count, w.matched, w.nans), (
        "%s: rows / selected / count / matched / nans %r, want %r" % (what, head, (w.rows, w.selected, w.count, w.matched, w.nans)))
    assert got.id_width == w.id_width, what
    ids = ids_numpy(got)
    assert ids.size == w.rows
    bad = np.flatnonzero(ids != w.ids)
    assert bad.size == 0, "%s: %d ids differ, the first at row %d: %d, want %d" % (what, bad.size, bad[0], ids[bad[0]], w.ids[bad[0]])
    assert ids.tobytes() == w.ids.tobytes(), what
