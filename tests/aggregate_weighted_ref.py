"""The reference of sb_aggregate_weighted: the ORACLE's decode of the pages (tests/aggregate_ref.py, unchanged), reduced per
group on the CPU.  Nothing here touches the device or its decoder.

A row is live if it is selected, its id is below n_groups, y is not null and its weight is valid.
  integer x integer   Python ints, the group's sum taken mod 2^128: compared exactly.
  otherwise           the per-row products in numpy double -- (double)y * (double)w, what the call defines -- classify the
                      group as NaN, +inf, -inf or finite.  A finite group is compared with the exact rational sum of the
                      exact products (fractions.Fraction of the ORIGINAL values, no conversion in between) within
                          (count_g + 2) * 2^-52 * sum_g |y_i * w_i|
                      One rounding of at most 2^-53 relative for each of the two conversions to double and one for the
                      product: 3 * 2^-53 per term to first order.  Then at most count - 1 additions of 2^-53 relative
                      each, in any order: (count + 2) * 2^-53 * sum|y w| together.  Then the factor 2 of slack that
                      aggregate_ref.float_sum_bound already grants for the higher-order terms.  Derived, not measured.
                      The inputs of the tests keep every partial sum far from overflow."""
import struct
from fractions import Fraction

import numpy as np

from tests import aggregate_ref as R

MASK128 = (1 << 128) - 1
INTS = tuple(np.dtype(t) for t in (np.int8, np.int16, np.int32, np.int64, np.uint8, np.uint16, np.uint32, np.uint64))
FLOATS = (np.dtype(np.float32), np.dtype(np.float64))


def is_float_mode(y_dtype, w_dtype):
    return np.dtype(y_dtype) in FLOATS or np.dtype(w_dtype) in FLOATS


class GroupWant:
    def __init__(self, selected=0, count=0):
        self.selected, self.count = selected, count
        self.nans = 0
        self.kind = "none"      # "int", "nan", "+inf", "-inf", "finite" or "none" (sum not asked for)
        self.int_sum = 0        # "int": the sum mod 2^128, as an unsigned Python int
        self.exact = Fraction(0)   # "finite": the exact sum of the exact products
        self.abs_sum = Fraction(0)  # ... and of their magnitudes

    @property
    def bound(self):
        return (self.count + 2) * Fraction(1, 2 ** 52) * self.abs_sum


class Want:
    def __init__(self, rows, selected, out_of_range, groups):
        self.rows, self.selected, self.out_of_range, self.groups = rows, selected, out_of_range, groups


def exact_sums(ys, ws):
    """(sum y_i w_i, sum |y_i w_i|) of finite Python ints / floats as Fractions: every value is an integer over a power of
    two (float.as_integer_ratio, exact), so the products are added as integers over the largest denominator -- what
    sum(Fraction(y) * Fraction(w)) gives, without a gcd per term"""
    nums, dens = [], []
    for a, b in zip(ys, ws):
        na, da = a.as_integer_ratio()
        nb, db = b.as_integer_ratio()
        nums.append(na * nb)
        dens.append(da * db)
    if not nums:
        return Fraction(0), Fraction(0)
    top = max(dens)
    scaled = [n * (top // d) for n, d in zip(nums, dens)]
    return Fraction(sum(scaled), top), Fraction(sum(abs(v) for v in scaled), top)


def reduce(y, y_valid, w, w_valid, ids, n_groups, mask=None, sum_=True):
    """y, w: typed numpy arrays of one length (w None: the row's own y); y_valid, w_valid: bool per row or None (every row);
    ids: integers per row or None (every row in group 0); mask: bool per row or None (every row)."""
    rows = int(len(y))
    sel = np.ones(rows, bool) if mask is None else np.asarray(mask, bool)[:rows]
    idv = np.zeros(rows, np.int64) if ids is None else np.asarray(ids)[:rows].astype(np.int64)
    inr = sel & (idv >= 0) & (idv < n_groups)
    live = inr.copy()
    if y_valid is not None:
        live &= np.asarray(y_valid, bool)[:rows]
    if w is not None and w_valid is not None:
        live &= np.asarray(w_valid, bool)[:rows]
    groups = [GroupWant() for _ in range(n_groups)]
    for g, c in zip(*np.unique(idv[inr], return_counts=True)):
        groups[int(g)].selected = int(c)
    for g, c in zip(*np.unique(idv[live], return_counts=True)):
        groups[int(g)].count = int(c)
    want = Want(rows, int(sel.sum()), int((sel & ~inr).sum()), groups)
    if not sum_:
        return want
    ww = y if w is None else w
    flt = is_float_mode(y.dtype, ww.dtype)
    at = np.flatnonzero(live)
    gid = idv[at]
    order = np.argsort(gid, kind="stable")
    at, gid = at[order], gid[order]
    starts = np.flatnonzero(np.r_[True, gid[1:] != gid[:-1]]) if at.size else np.array([], np.int64)
    ends = np.r_[starts[1:], at.size] if at.size else starts
    yl, wl = y[at].tolist(), ww[at].tolist()   # Python ints / floats: the original values
    with np.errstate(all="ignore"):
        prod = y[at].astype(np.float64) * ww[at].astype(np.float64) if flt else None
    for s, e in zip(starts.tolist(), ends.tolist()):
        gw = groups[int(gid[s])]
        if not flt:
            gw.kind = "int"
            gw.int_sum = sum(a * b for a, b in zip(yl[s:e], wl[s:e])) & MASK128
            continue
        p = prod[s:e]
        gw.nans = int(np.isnan(p).sum())
        pos, neg = bool(np.any(p == np.inf)), bool(np.any(p == -np.inf))
        if gw.nans or (pos and neg):
            gw.kind = "nan"
        elif pos or neg:
            gw.kind = "+inf" if pos else "-inf"
        else:
            gw.kind = "finite"
            gw.exact, gw.abs_sum = exact_sums(yl[s:e], wl[s:e])
    for gw in groups:
        if gw.kind == "none":
            gw.kind = "finite" if flt else "int"   # an empty group: 0
    return want


def want(ref, w, w_valid, ids, n_groups, mask=None, ops=("count", "sum")):
    """ref: an aggregate_ref.Ref (the oracle's decode of y's pages)"""
    sum_ = "sum" in ops
    if not sum_ or ref.vals is None:
        y = np.zeros(ref.rows, np.int8)
        return reduce(y, ref.valid, None if w is None else np.zeros(ref.rows, np.int8), w_valid, ids, n_groups, mask, False)
    return reduce(ref.vals, ref.valid, w, w_valid, ids, n_groups, mask, True)


def dbl(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def check(got, wanted, what=""):
    """got: a strawboat_amd GroupedAggregate of an aggregate_weighted call, after the synchronize"""
    assert (got.rows, got.selected, got.out_of_range) == (wanted.rows, wanted.selected, wanted.out_of_range), (
        "%s: rows / selected / out_of_range %r, want %r" % (what, (got.rows, got.selected, got.out_of_range),
                                                            (wanted.rows, wanted.selected, wanted.out_of_range)))
    assert len(got.groups) == len(wanted.groups), what
    assert sum(g.selected for g in got.groups) + got.out_of_range == got.selected, what
    worst = 0.0
    for i, (g, w) in enumerate(zip(got.groups, wanted.groups)):
        c = g._c
        assert (int(c.selected), int(c.count), int(c.nans)) == (w.selected, w.count, w.nans), (
            "%s group %d: selected / count / nans %r, want %r" % (what, i, (int(c.selected), int(c.count), int(c.nans)), (w.selected, w.count, w.nans)))
        assert bytes(c.min) == bytes(8) and bytes(c.max) == bytes(8) and int(c.reserved) == 0, "%s group %d: min / max / reserved" % (what, i)
        lo, hi = int(c.sum_lo), int(c.sum_hi)
        if w.kind == "none":
            assert (lo, hi) == (0, 0), "%s group %d: a sum without SUM" % (what, i)
        elif w.kind == "int":
            assert (hi << 64) | lo == w.int_sum, "%s group %d: sum %d, want %d" % (what, i, R.join128(lo, hi), R.join128(*R.split128(w.int_sum)))
        else:
            assert hi == 0, "%s group %d: sum_hi of a float sum" % (what, i)
            v = dbl(lo)
            if w.kind == "nan":
                assert v != v, "%s group %d: sum %r, want NaN" % (what, i, v)
            elif w.kind in ("+inf", "-inf"):
                assert v == float(w.kind), "%s group %d: sum %r, want %s" % (what, i, v, w.kind)
            else:
                assert v == v and abs(v) != float("inf"), "%s group %d: sum %r, want a finite one" % (what, i, v)
                diff = abs(Fraction(v) - w.exact)
                if w.bound:
                    worst = max(worst, float(diff / w.bound))
                assert diff <= w.bound, "%s group %d: sum %r, exact %r, |diff| %.3g > bound %.3g" % (what, i, v, float(w.exact), float(diff), float(w.bound))
    if worst:
        print("%s: largest |diff| / bound of a float sum: %.3g" % (what, worst))
