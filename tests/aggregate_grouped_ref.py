"""The reference of sb_aggregate_grouped: the oracle's decode of the pages (tests/aggregate_ref.py, unchanged) reduced per
group on the CPU.  Group g of a column is reduce_values over `live & (ids == g)`; a selected row whose id is >= n_groups
belongs to no group and is counted in out_of_range.  Integers, counts and min / max bytes are exact; a group's float sum is
math.fsum, to be met within float_sum_bound of that group (count_g * 2^-52 * sum_g|x|)."""
import struct

import numpy as np

from tests import aggregate_ref as R


class GroupedWant:
    """what one column of a grouped call must give: the column's rows / selected / out_of_range and a Want per group (whose
    `selected` is the group's: its selected rows, null or not)"""

    def __init__(self, rows, selected, out_of_range, groups):
        self.rows, self.selected, self.out_of_range, self.groups = rows, selected, out_of_range, groups


def reduce_grouped(ptype, vals, valid, sel, ids, n_groups, ops=R.ALL):
    """vals: the column's values as a typed array or None (count only); valid, sel: bool per row; ids: an integer per row"""
    rows = int(valid.size)
    sel = np.asarray(sel, bool)[:rows]
    ids = np.asarray(ids)[:rows].astype(np.uint64)
    value_ops = bool(sum(R.OPS[o] for o in ops) & 14)
    groups = []
    for g in range(n_groups):
        member = sel & (ids == np.uint64(g))
        live = member & valid
        if value_ops:
            groups.append(R.reduce_values(ptype, vals, live, int(member.sum()), ops))
        else:
            groups.append(R.Want(rows, int(member.sum()), int(live.sum())))
    return GroupedWant(rows, int(sel.sum()), int((sel & (ids >= np.uint64(n_groups))).sum()), groups)


ORDER_TEST_GROUPS = (5, 96)   # few groups: every id of a wave gets a shuffle tree; many: most rows go by rank (grp_span)


def inexact_values(rows, n_groups, seed):
    """(values, ids) of the float order tests: runs of two rows of +-1e16-sized, unit-sized and small magnitudes with random
    mantissas, so that a group's sum is exact in no order of additions and different orders give different doubles; ids at
    random"""
    rng = np.random.default_rng(seed)
    pat = np.array([1e16, 1.0, -1e16, 3.0, 1e-3, -1.0])
    half = (rows + 1) // 2
    v = np.repeat(pat[rng.integers(0, pat.size, half)] * (1.0 + rng.random(half)), 2)[:rows]
    return v, rng.integers(0, n_groups, rows)


def want(ref, ids, n_groups, mask=None, ops=R.ALL):
    """ref: an aggregate_ref.Ref; mask: a bool per row or None (every row)"""
    sel = np.ones(ref.rows, bool) if mask is None else np.asarray(mask, bool)[:ref.rows]
    return reduce_grouped(ref.ptype, ref.vals, ref.valid, sel, ids, n_groups, ops)


def check_group(got, w, what=""):
    """got: a strawboat_amd.aggregate_grouped.Group after the synchronize; w: its Want"""
    assert (got.selected, got.count, got.nans) == (w.selected, w.count, w.nans), (
        "%s: selected / count / nans %r, want %r" % (what, (got.selected, got.count, got.nans), (w.selected, w.count, w.nans)))
    assert got.min_bytes == w.min_bytes, "%s: min bytes %s, want %s" % (what, got.min_bytes.hex(), w.min_bytes.hex())
    assert got.max_bytes == w.max_bytes, "%s: max bytes %s, want %s" % (what, got.max_bytes.hex(), w.max_bytes.hex())
    assert int(got._c.reserved) == 0, what
    if w.selected == 0:   # an empty group: every byte of its record is 0
        assert bytes(got._c) == bytes(64), what
    lo, hi = int(got._c.sum_lo), int(got._c.sum_hi)
    if w.fsum is None:
        assert (lo, hi) == (w.sum_lo, w.sum_hi), "%s: sum %d, want %d" % (what, R.join128(lo, hi), R.join128(w.sum_lo, w.sum_hi))
        return
    assert hi == 0, what
    g = struct.unpack("<d", struct.pack("<Q", lo))[0]
    f = w.fsum
    if f != f:
        assert g != g, "%s: sum %r, want NaN" % (what, g)
    elif abs(f) == float("inf"):
        assert g == f, "%s: sum %r, want %r" % (what, g, f)
    else:
        bound = R.float_sum_bound(w)
        assert abs(g - f) <= bound, "%s: sum %r, fsum %r, |diff| %.3g > bound %.3g" % (what, g, f, abs(g - f), bound)


def check(got, w, what=""):
    """got: a strawboat_amd.aggregate_grouped.GroupedAggregate after the synchronize"""
    assert (got.rows, got.selected, got.out_of_range) == (w.rows, w.selected, w.out_of_range), (
        "%s: rows / selected / out_of_range %r, want %r" % (what, (got.rows, got.selected, got.out_of_range),
                                                            (w.rows, w.selected, w.out_of_range)))
    assert len(got.groups) == len(w.groups), what
    assert sum(g.selected for g in got.groups) + got.out_of_range == got.selected, what
    for i, (g, wg) in enumerate(zip(got.groups, w.groups)):
        check_group(g, wg, "%s group %d" % (what, i))
