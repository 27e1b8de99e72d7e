"""The reference of sb_aggregate_columns: the ORACLE's decode of the pages (gen.oracle_read), reduced by numpy and Python.
Sums are Python ints (exact) and math.fsum (correctly rounded); nothing here touches the device or its decoder.

A row is live if its selection bit is set and it is not null.  min / max run over the live rows that are not NaN, in the
order of `order_key`; the float sum runs over all live rows."""
import math
import struct

import numpy as np

from oracle import sbo as S
from tests import gen

NP = gen.NP_OF
FLOATS = (S.T_F32, S.T_F64)
OPS = {"count": 1, "min": 2, "max": 4, "sum": 8}
ALL = ("count", "min", "max", "sum")


def order_keys(ptype, raw):
    """Unsigned integers that order the values of a type as min / max must: integers by signedness, floats in the total
    order -inf < ... < -0.0 < +0.0 < ... < +inf.  `raw`: the values' bytes as an unsigned array of their width.  Not for NaNs."""
    raw = np.asarray(raw)
    top = raw.dtype.type(1 << (8 * raw.dtype.itemsize - 1))
    if ptype in FLOATS:
        return np.where(raw & top != 0, ~raw, raw | top)
    if ptype in (S.T_I8, S.T_I16, S.T_I32, S.T_I64):
        return raw ^ top
    return raw


def order_key(ptype, value):
    """the key of one value of the type (a Python or numpy scalar)"""
    dt = np.dtype(NP[ptype])
    return int(order_keys(ptype, np.array([value], dt).view("<u%d" % dt.itemsize))[0])


def split128(v):
    """(sum_lo, sum_hi) of a Python int as a 128-bit two's-complement number"""
    u = v & ((1 << 128) - 1)
    return u & ((1 << 64) - 1), u >> 64


def join128(lo, hi):
    v = (hi << 64) | lo
    return v - (1 << 128) if hi >> 63 else v


class Want:
    """what one column of a call must give"""

    def __init__(self, rows, selected, count, nans=0, min_bytes=bytes(8), max_bytes=bytes(8), sum_lo=0, sum_hi=0, fsum=None, abs_sum=0.0):
        self.rows, self.selected, self.count, self.nans = rows, selected, count, nans
        self.min_bytes, self.max_bytes, self.sum_lo, self.sum_hi = min_bytes, max_bytes, sum_lo, sum_hi
        self.fsum, self.abs_sum = fsum, abs_sum   # floats: math.fsum of the live rows (None: integers) and of their magnitudes


def reduce_values(ptype, vals, live, selected, ops=ALL):
    """vals: the column's values as a typed array (any bytes in null slots); live: bool per row"""
    mask = sum(OPS[o] for o in ops)
    rows = int(live.size)
    count = int(live.sum())
    if not (mask & 14):
        return Want(rows, selected, count)
    dt = np.dtype(NP[ptype])
    w = dt.itemsize
    v = np.ascontiguousarray(vals[:rows])[live]
    raw = v.view("<u%d" % w)
    nan = np.isnan(v) if ptype in FLOATS else np.zeros(v.size, bool)
    nans = int(nan.sum())
    mn = mx = bytes(8)
    if count - nans:
        good = raw[~nan]
        keys = order_keys(ptype, good)
        if mask & 2:
            mn = int(good[int(np.argmin(keys))]).to_bytes(w, "little") + bytes(8 - w)
        if mask & 4:
            mx = int(good[int(np.argmax(keys))]).to_bytes(w, "little") + bytes(8 - w)
    lo = hi = 0
    fs, abs_sum = None, 0.0
    if ptype in FLOATS:
        xs = v.astype(np.float64).tolist()
        try:
            fs = math.fsum(xs)
        except (OverflowError, ValueError):   # inf - inf, or an intermediate overflow: IEEE says NaN / inf
            with np.errstate(invalid="ignore", over="ignore"):
                fs = float(np.sum(np.array(xs, np.float64)))
        if any(x != x for x in xs):
            fs = float("nan")
        abs_sum = math.fsum(abs(x) for x in xs if x == x and abs(x) != float("inf")) if xs else 0.0
        if mask & 8:
            lo = struct.unpack("<Q", struct.pack("<d", fs))[0]
    elif mask & 8:
        lo, hi = split128(sum(v.tolist()))   # Python ints: exact
    return Want(rows, selected, count, nans, mn, mx, lo, hi, fs if (mask & 8) else None, abs_sum)


class Ref:
    """the oracle's decode of a column's pages, computed once and left unchanged; want(mask) reduces it"""

    def __init__(self, col, pages, metas):
        want = gen.oracle_read(col, pages, metas)
        self.ptype = col["ptype"]
        self.rows = rows = int(want["rows"])
        if self.ptype == S.T_NULL:
            self.valid = np.zeros(rows, bool)
        elif col["nullable"]:
            self.valid = np.unpackbits(np.asarray(want["validity"], np.uint8), bitorder="little")[:rows].astype(bool)
        else:
            self.valid = np.ones(rows, bool)
        self.vals = None
        if self.ptype in NP:
            w = np.dtype(NP[self.ptype]).itemsize
            self.vals = np.ascontiguousarray(want["values"]).view(np.uint8).reshape(-1)[:rows * w].view(NP[self.ptype])

    def want(self, mask=None, ops=ALL):
        """the Want under a selection (a bool per row, or None: every row)"""
        sel = np.ones(self.rows, bool) if mask is None else np.asarray(mask, bool)[:self.rows]
        live = sel & self.valid
        if not (sum(OPS[o] for o in ops) & 14):
            return Want(self.rows, int(sel.sum()), int(live.sum()))
        return reduce_values(self.ptype, self.vals, live, int(sel.sum()), ops)


def reference(col, pages, metas, mask=None, ops=ALL):
    return Ref(col, pages, metas).want(mask, ops)


def float_sum_bound(want):
    """|device sum - fsum| of n finite doubles added in ANY order is at most (n-1) u sum|x| to first order, u = 2^-53;
    n 2^-52 sum|x| (twice that) covers the higher-order terms and the rounding of fsum itself.  Derived, not measured."""
    return want.count * 2.0 ** -52 * want.abs_sum


def check(got, want, what=""):
    """got: a strawboat_amd.aggregate.Aggregate after the synchronize"""
    assert (got.rows, got.selected, got.count, got.nans) == (want.rows, want.selected, want.count, want.nans), (
        "%s: rows / selected / count / nans %r, want %r" % (what, (got.rows, got.selected, got.count, got.nans),
                                                            (want.rows, want.selected, want.count, want.nans)))
    assert got.min_bytes == want.min_bytes, "%s: min bytes %s, want %s" % (what, got.min_bytes.hex(), want.min_bytes.hex())
    assert got.max_bytes == want.max_bytes, "%s: max bytes %s, want %s" % (what, got.max_bytes.hex(), want.max_bytes.hex())
    lo, hi = int(got._c.sum_lo), int(got._c.sum_hi)
    if want.fsum is None:
        assert (lo, hi) == (want.sum_lo, want.sum_hi), "%s: sum %d, want %d" % (what, join128(lo, hi), join128(want.sum_lo, want.sum_hi))
        return
    assert hi == 0, what
    g = struct.unpack("<d", struct.pack("<Q", lo))[0]
    f = want.fsum
    if f != f:
        assert g != g, "%s: sum %r, want NaN" % (what, g)
    elif abs(f) == float("inf"):
        assert g == f, "%s: sum %r, want %r" % (what, g, f)
    else:
        bound = float_sum_bound(want)
        print("%s: float sum %r, fsum %r, |diff| %.3g, bound %.3g" % (what, g, f, abs(g - f), bound))
        assert abs(g - f) <= bound, "%s: sum %r, fsum %r, |diff| %.3g > bound %.3g" % (what, g, f, abs(g - f), bound)
