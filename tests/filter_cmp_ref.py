"""The reference of sb_filter_columns_cmp: the selection words and `selected` from y (the ORACLE's decode of the pages: values
and validity), the operand and its validity, the op, the combine mode and the earlier bitmap.  Nothing here touches the
device or its decoder.

Integer against integer: both sides as Python ints, whatever their dtypes (exact).  A pair with a float: both through
np.float64 (integers round to nearest even) and numpy's IEEE comparisons: a NaN on either side satisfies only "ne",
-0.0 == +0.0.  A row whose y is null or whose operand is invalid satisfies nothing, "ne" included.
tests/test_filter_cmp_host.py checks all of this against a plain Python loop."""
import operator

import numpy as np

from tests.aggregate_ref import Ref  # noqa: F401  (the oracle's decode of a numeric column: .vals, .valid, .rows)

OPS = ("eq", "ne", "lt", "le", "gt", "ge")
OPFN = {"eq": operator.eq, "ne": operator.ne, "lt": operator.lt, "le": operator.le, "gt": operator.gt, "ge": operator.ge}
COMBINES = ("set", "and", "or")


def is_int(a):
    return np.asarray(a).dtype.kind in "iu"


def compare(y, other, op):
    """bool per row: y[row] op other[row], nulls not looked at"""
    y, other = np.asarray(y), np.asarray(other)
    assert y.shape == other.shape and y.ndim == 1
    if is_int(y) and is_int(other):
        a, b = y.astype(object), other.astype(object)   # Python ints: exact at every width and signedness
        return np.array(OPFN[op](a, b), dtype=bool).reshape(y.shape)
    with np.errstate(invalid="ignore"):
        return np.asarray(OPFN[op](y.astype(np.float64), other.astype(np.float64)), dtype=bool)


def result_bits(y, y_valid, other, other_valid, op):
    """bool per row with the nulls of both sides taken out"""
    r = compare(y, other, op)
    if y_valid is not None:
        r = r & np.asarray(y_valid, bool)[:r.size]
    if other_valid is not None:
        r = r & np.asarray(other_valid, bool)[:r.size]
    return r


def words_of(bits):
    """the uint32 words of an LSB-first bitmap of len(bits) rows, the bits behind the last row 0"""
    bits = np.asarray(bits, bool)
    n = (bits.size + 31) // 32
    padded = np.zeros(n * 32, bool)
    padded[:bits.size] = bits
    return np.packbits(padded, bitorder="little").view("<u4").astype(np.uint32)


def combine_words(bits, combine, prev):
    """(words, selected): `bits` combined into the earlier bitmap `prev` (uint32 words, any contents behind the rows).  SET
    ignores prev and writes zeros behind the last row; AND / OR leave the bits behind the last row as prev has them."""
    rows = int(np.asarray(bits).size)
    new = words_of(bits)
    live = words_of(np.ones(rows, bool))   # the positions below `rows`
    if combine == "set":
        out = new
    else:
        prev = np.asarray(prev, np.uint32)
        assert prev.size == new.size
        out = (prev & (new | ~live)) if combine == "and" else (prev | new)
    selected = int(sum(bin(int(w)).count("1") for w in (out & live)))
    return out.astype(np.uint32), selected


def want(y, y_valid, other, other_valid, op, combine="set", prev=None):
    """what one column of a call must give: (selection words, selected)"""
    return combine_words(result_bits(y, y_valid, other, other_valid, op), combine, prev)


def check(sel, words, selected, rows, what=""):
    """sel: a strawboat_amd Selection after the synchronize.  Word for word, and rows / selected."""
    got = sel.bitmap.cpu().numpy()[:((rows + 31) // 32) * 4].view("<u4")
    print("%s: rows %d selected %d (want %d)" % (what, sel.rows, sel.selected, selected))
    assert sel.rows == rows, "%s: rows %d, want %d" % (what, sel.rows, rows)
    bad = np.flatnonzero(got != words)
    assert bad.size == 0, "%s: %d selection words differ, the first at word %d: %#010x, want %#010x" % (
        what, bad.size, bad[0], got[bad[0]], words[bad[0]])
    assert sel.selected == selected, "%s: selected %d, want %d" % (what, sel.selected, selected)
