"""ENDS_WITH / CONTAINS and the NOT_ string predicates without a GPU: the header's constants, the refusals on the host,
like_predicate's table and the reference the GPU tests compare with."""
import os
import re

import numpy as np
import pytest

from strawboat_amd import _native as N
from strawboat_amd.filter import OPS, Predicate, filter_columns, like_predicate, literal_bytes
from strawboat_amd.types import PhysicalType as P
from tests.substring_ref import OPS6, SUB_OPS, selective, sub_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")


def test_header_constants():
    text = open(HEADER).read()
    want = {"SB_PRED_ENDS_WITH": 11, "SB_PRED_CONTAINS": 12, "SB_PRED_NOT_STARTS_WITH": 13, "SB_PRED_NOT_ENDS_WITH": 14,
            "SB_PRED_NOT_CONTAINS": 15, "SB_PRED_STARTS_WITH": 8, "SB_PRED_IN": 9, "SB_PRED_NOT_IN": 10}
    for name, value in want.items():
        m = re.search(r"#define %s (\d+)\b" % name, text)
        assert m and int(m.group(1)) == value == getattr(N, name), name
    assert OPS["ends_with"] == 11 and OPS["contains"] == 12 and OPS["not_starts_with"] == 13
    assert OPS["not_ends_with"] == 14 and OPS["not_contains"] == 15 and OPS["starts_with"] == 8
    assert len(set(OPS.values())) == len(OPS)


def test_literals_and_refusals():
    for ptype in (P.BINARY, P.LARGE_BINARY):
        for op in SUB_OPS:
            assert literal_bytes(ptype, op, "Zürich") == "Zürich".encode("utf-8")
            assert literal_bytes(ptype, op, b"") == b"" and literal_bytes(ptype, op, b"a\0\xff") == b"a\0\xff"
            for bad in (1, 1.5, None, True):
                with pytest.raises(ValueError):
                    literal_bytes(ptype, op, bad)
    for ptype in (P.INT8, P.INT32, P.UINT64, P.FLOAT32, P.FLOAT64, P.BOOLEAN, P.INT128, P.NULL):
        for op in SUB_OPS:
            for lit in (b"a", "a", 1):
                with pytest.raises(ValueError):
                    literal_bytes(ptype, op, lit)
    for op in SUB_OPS:
        assert Predicate(op, b"x").op == op
        with pytest.raises(ValueError):
            Predicate(op)
    with pytest.raises(ValueError):
        Predicate("like", "a%")
    # refused before the context is touched
    from strawboat_amd.read import ColumnPages
    num = ColumnPages(P.INT32, False, None, np.zeros((0, 2), np.uint64))
    col = ColumnPages(P.BINARY, True, None, np.zeros((0, 2), np.uint64))
    for op in SUB_OPS:
        with pytest.raises(ValueError):
            filter_columns(None, [num], [Predicate(op, b"a")])
        with pytest.raises(ValueError):
            filter_columns(None, [col], [Predicate(op, 7)])


def test_like_predicate_table():
    def pl(pattern, **kw):
        p = like_predicate(pattern, **kw)
        return p.op, p.literal

    assert pl("lit") == ("eq", "lit") and pl("lit", negate=True) == ("ne", "lit")
    assert pl("lit%") == ("starts_with", "lit") and pl("lit%", negate=True) == ("not_starts_with", "lit")
    assert pl("%lit") == ("ends_with", "lit") and pl("%lit", negate=True) == ("not_ends_with", "lit")
    assert pl("%lit%") == ("contains", "lit") and pl("%lit%", negate=True) == ("not_contains", "lit")
    assert pl("%") == ("starts_with", "") and pl("%%") == ("starts_with", "")
    assert pl("%", negate=True) == ("not_starts_with", "")
    assert pl("") == ("eq", "")
    assert pl("%.google.%", negate=True) == ("not_contains", ".google.") and pl("%.png") == ("ends_with", ".png")
    # bytes in, bytes out; any byte
    assert pl(b"%a\xff\x00%") == ("contains", b"a\xff\x00") and pl(b"%") == ("starts_with", b"")
    assert pl("%Zürich") == ("ends_with", "Zürich")
    # escapes are literal bytes
    assert pl("100\\%") == ("eq", "100%") and pl("%100\\%") == ("ends_with", "100%")
    assert pl("\\%%") == ("starts_with", "%") and pl("%a\\_b%") == ("contains", "a_b")
    assert pl("a\\\\b%") == ("starts_with", "a\\b") and pl("%\\\\") == ("ends_with", "\\")
    assert pl("%a!%b!_!!%", escape="!") == ("contains", "a%b_!") and pl("a\\b%", escape="!") == ("starts_with", "a\\b")
    for bad in ("a\\", "a\\b", "\\"):
        with pytest.raises(ValueError):
            like_predicate(bad)
    with pytest.raises(ValueError):
        like_predicate("a", escape="ab")
    with pytest.raises(ValueError):
        like_predicate(5)
    for pattern in ("a%b", "%a%b%", "a_", "_", "%a_b%", "a%b%", "%a%b", "_%", b"x%y"):
        with pytest.raises(NotImplementedError) as e:
            like_predicate(pattern)
        assert repr(pattern) in str(e.value)
        with pytest.raises(NotImplementedError):
            like_predicate(pattern, negate=True)
    # what like_predicate gives is a Predicate the filter accepts
    assert all(like_predicate(p).op in OPS for p in ("a", "a%", "%a", "%a%", "%"))


def test_reference_against_hand_written_cases():
    strs = [b"", b"a", b"ab", b"abc", b"xabc", b"abcx", b"xabcx", b"ab", b"c", b"abab", b"\0abc\xff", b"abc"]
    valid = np.array([1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0], bool)
    t, f = True, False
    want = {"contains": [f, f, f, t, t, t, t, f, f, f, t, f], "ends_with": [f, f, f, t, t, f, f, f, f, f, f, f],
            "starts_with": [f, f, f, t, f, t, f, f, f, f, f, f]}
    for op, w in want.items():
        assert sub_expected(strs, valid, op, b"abc").tolist() == w, op
        assert sub_expected(strs, valid, "not_" + op, b"abc").tolist() == [v and not x for v, x in zip(valid.tolist(), w)], op
        assert selective(strs, valid, op, b"abc") and selective(strs, valid, "not_" + op, b"abc")
    # `ab` + `c` in neighbouring rows is no match; the null row satisfies neither form
    assert not sub_expected([b"xab", b"cx"], [True, True], "contains", b"abc").any()
    assert not sub_expected(strs, valid, "contains", b"abc")[11] and not sub_expected(strs, valid, "not_contains", b"abc")[11]
    # the empty literal: the positive forms select every non-null row, the negated ones none
    for op in OPS6:
        got = sub_expected(strs, valid, op, b"")
        assert np.array_equal(got, np.zeros(12, bool) if op.startswith("not_") else valid), op
        assert not selective(strs, valid, op, b"")
    # overlaps, str literals
    assert sub_expected([b"aaaa", b"ababab", b"aa"], [1, 1, 1], "contains", b"aaa").tolist() == [t, f, f]
    assert sub_expected([b"aaaa", b"ababab", b"aa"], [1, 1, 1], "contains", "abab").tolist() == [f, t, f]
    assert sub_expected(["Zürich".encode()], [1], "ends_with", "ürich").tolist() == [t]
