"""The reference of sb_key_lookup: ids and the four counts from decoded values, validity, mask, list and value_ids, in numpy
and plain Python.  The values come from the ORACLE's decode of the pages (tests/aggregate_ref.Ref for integers,
tests/key_ids_var_ref.Ref for strings); nothing here touches the device or its decoder.

A row is live if its selection bit is set and it is not null.  A live row whose value equals values[i] gets value_ids[i]
(i without value_ids), the FIRST such i where a value repeats; every other row gets all ones of id_width.  `matched`
counts the live rows with an id.  Integers compare as numbers of the column's dtype, strings as Python `bytes`."""
import numpy as np

from tests.aggregate_ref import Ref  # noqa: F401  (the oracle's decode of an integer column)
from tests.key_ids_var_ref import Ref as StrRef  # noqa: F401  (... of a binary column: .strs, .valid)

ID_NP = {1: np.uint8, 2: np.uint16, 4: np.uint32}


class Want:
    """what one column of a call must give"""

    def __init__(self, rows, selected, count, matched, id_width, ids):
        self.rows, self.selected, self.count, self.matched = rows, selected, count, matched
        self.id_width, self.ids = id_width, ids


def lookup_values(vals, live, selected, values, value_ids, id_width):
    """vals: one value per row (a typed array, or an object array of bytes; anything in null slots); live: bool per row;
    values: the list in the caller's order; value_ids: one id per value or None"""
    rows = int(live.size)
    none = (1 << (8 * id_width)) - 1
    ids = np.full(rows, none, ID_NP[id_width])
    n = len(values)
    id_of = np.arange(n, dtype=np.int64) if value_ids is None else np.asarray(value_ids, np.int64)
    assert id_of.size == n and ((0 <= id_of) & (id_of < none)).all(), "the list hands out an id that is all ones or does not fit"
    at = np.flatnonzero(live)
    matched = 0
    if n and at.size:
        strings = isinstance(vals, np.ndarray) and vals.dtype == object
        lst = np.empty(n, object) if strings else np.asarray(values, vals.dtype)
        if strings:
            lst[:] = list(values)
        # sorted distinct values and the index of the FIRST occurrence of each (np.unique's return_index)
        keys, firsts = np.unique(lst, return_index=True)
        probe = vals[at]
        pos = np.searchsorted(keys, probe)
        hit = pos < keys.size
        hit[hit] = keys[pos[hit]] == probe[hit]   # the lower bound alone is no match
        ids[at[hit]] = id_of[firsts[pos[hit]]].astype(ID_NP[id_width])
        matched = int(hit.sum())
    return Want(rows, selected, int(live.sum()), matched, id_width, ids)


def want(ref, mask, values, value_ids, id_width):
    """the Want of a column (a Ref or a StrRef) under a selection (a bool per row, or None: every row)"""
    sel = np.ones(ref.rows, bool) if mask is None else np.asarray(mask, bool)[:ref.rows]
    vals = ref.strs if hasattr(ref, "strs") else ref.vals[:ref.rows]
    return lookup_values(vals, sel & ref.valid, int(sel.sum()), values, value_ids, id_width)


def ids_numpy(got):
    """the ids of a strawboat_amd.key_lookup.KeyLookup as unsigned integers of their width"""
    return got.ids.cpu().numpy().view(ID_NP[got.id_width])


def check(got, w, what=""):
    """got: a KeyLookup after the synchronize.  Every comparison is exact: the bytes of ids and the four counts."""
    head = (got.rows, got.selected, got.count, got.matched)
    print("%s: rows / selected / count / matched %r" % (what, head))
    assert head == (w.rows, w.selected, w.count, w.matched), (
        "%s: rows / selected / count / matched %r, want %r" % (what, head, (w.rows, w.selected, w.count, w.matched)))
    assert got.id_width == w.id_width, what
    ids = ids_numpy(got)
    assert ids.size == w.rows
    bad = np.flatnonzero(ids != w.ids)
    assert bad.size == 0, "%s: %d ids differ, the first at row %d: %d, want %d" % (what, bad.size, bad[0], ids[bad[0]], w.ids[bad[0]])
    assert ids.tobytes() == w.ids.tobytes(), what
