"""sb_filter_columns without a GPU: the symbol is exported, the ctypes struct has the header's layout, and literals are
converted to the column's physical type (or refused) on the host."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from strawboat_amd import _native as N
from strawboat_amd.filter import Predicate, filter_columns, pack_literal
from strawboat_amd.types import PhysicalType as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")


def test_symbol_is_declared_and_exported():
    assert "sb_filter_columns" in N.EXPORTS
    assert re.search(r"\bsb_filter_columns\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_filter_columns$", out, re.M)


def test_ctypes_struct_has_the_headers_layout(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    fields = [name for name, _ in N.ColumnFilterC._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(sb_column_filter));\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_filter, %s));\n' % (f, f) for f in fields) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(N.ColumnFilterC)
    for f in fields:
        assert int(got[f]) == getattr(N.ColumnFilterC, f).offset, f
    # the constants too
    text = open(HEADER).read()
    for name in ("SB_PRED_EQ", "SB_PRED_NE", "SB_PRED_LT", "SB_PRED_LE", "SB_PRED_GT", "SB_PRED_GE", "SB_PRED_IS_NULL",
                 "SB_PRED_IS_NOT_NULL", "SB_SEL_SET", "SB_SEL_AND", "SB_SEL_OR"):
        assert int(re.search(r"#define %s (\d+)" % name, text).group(1)) == getattr(N, name), name


def test_integer_literals():
    assert pack_literal(P.INT8, -1) == b"\xff" + b"\0" * 7
    assert pack_literal(P.UINT8, 255) == b"\xff" + b"\0" * 7
    assert pack_literal(P.INT16, -2) == b"\xfe\xff" + b"\0" * 6
    assert pack_literal(P.UINT32, 1 << 31) == b"\0\0\0\x80" + b"\0" * 4
    assert pack_literal(P.INT64, -(1 << 63)) == b"\0" * 7 + b"\x80"
    assert pack_literal(P.UINT64, (1 << 64) - 1) == b"\xff" * 8
    assert pack_literal(P.INT32, 7.0) == pack_literal(P.INT32, 7) == pack_literal(P.INT32, np.int64(7))
    for ptype, bad in ((P.INT8, 128), (P.INT8, -129), (P.UINT8, 256), (P.UINT8, -1), (P.INT16, 1 << 15), (P.UINT16, 1 << 16),
                       (P.INT32, 1 << 31), (P.UINT32, -1), (P.INT64, 1 << 63), (P.UINT64, 1 << 64), (P.UINT64, -1)):
        with pytest.raises(ValueError):
            pack_literal(ptype, bad)
    for bad in (1.5, float("nan"), float("inf"), "3", None, True):
        with pytest.raises(ValueError):
            pack_literal(P.INT32, bad)


def test_float_literals():
    assert pack_literal(P.FLOAT64, 1.5) == np.float64(1.5).tobytes()
    assert pack_literal(P.FLOAT32, 1.5) == np.float32(1.5).tobytes() + b"\0" * 4
    assert pack_literal(P.FLOAT64, 3) == np.float64(3.0).tobytes()
    assert pack_literal(P.FLOAT64, -0.0) == np.float64(-0.0).tobytes() != pack_literal(P.FLOAT64, 0.0)
    assert math.isnan(np.frombuffer(pack_literal(P.FLOAT64, float("nan")), np.float64)[0])
    assert math.isnan(np.frombuffer(pack_literal(P.FLOAT32, float("nan"))[:4], np.float32)[0])
    assert np.frombuffer(pack_literal(P.FLOAT32, float("-inf"))[:4], np.float32)[0] == -np.inf
    with pytest.raises(ValueError):
        pack_literal(P.FLOAT32, 1e300)
    with pytest.raises(ValueError):
        pack_literal(P.FLOAT64, "1.0")


def test_comparison_literals_of_other_types_are_refused():
    for ptype in (P.BOOLEAN, P.INT128, P.INT256, P.BINARY, P.LARGE_BINARY, P.NULL):
        with pytest.raises(ValueError):
            pack_literal(ptype, 1)


def test_predicates():
    assert Predicate("lt", 5).literal == 5 and Predicate("is_null").literal is None
    for op, lit in (("is_null", 3), ("is_not_null", 0), ("lt", None), ("between", 1)):
        with pytest.raises(ValueError):
            Predicate(op, lit)


def test_bad_arguments_raise_before_anything_is_enqueued():
    """ctx is never touched: the checks come first"""
    from strawboat_amd.read import ColumnPages
    col = ColumnPages(P.INT8, False, None, np.zeros((0, 2), np.uint64))
    with pytest.raises(ValueError):
        filter_columns(None, [col], [Predicate("lt", 1000)])
    with pytest.raises(ValueError):
        filter_columns(None, [col], [Predicate("lt", 1), Predicate("lt", 2)])
    with pytest.raises(ValueError):
        filter_columns(None, [col], [Predicate("lt", 1)], combine="xor")
    with pytest.raises(ValueError):
        filter_columns(None, [col], [Predicate("lt", 1)], combine="and")
