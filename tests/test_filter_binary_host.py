"""sb_filter_columns_var without a GPU: the symbol is exported, the ctypes struct has the header's layout, and literals of
binary and numeric columns are converted (or refused) on the host, before anything is enqueued."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from strawboat_amd import _native as N
from strawboat_amd.filter import Predicate, filter_columns, literal_bytes, pack_literal
from strawboat_amd.types import PhysicalType as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")


def test_symbol_is_declared_and_exported():
    assert "sb_filter_columns_var" in N.EXPORTS
    assert re.search(r"\bsb_filter_columns_var\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_filter_columns_var$", out, re.M)
    assert re.search(r"\bT sb_filter_columns$", out, re.M)


def test_ctypes_struct_has_the_headers_layout(tmp_path):
    assert C.sizeof(N.ColumnFilterVarC) == 112
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    fields = [name for name, _ in N.ColumnFilterVarC._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(sb_column_filter_var));\n'
                   '    printf("old %zu\\n", sizeof(sb_column_filter));\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_filter_var, %s));\n' % (f, f) for f in fields) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(N.ColumnFilterVarC) == 112
    assert int(got["old"]) == C.sizeof(N.ColumnFilterC)     # sb_column_filter keeps its layout
    for f in fields:
        assert int(got[f]) == getattr(N.ColumnFilterVarC, f).offset, f
    assert int(re.search(r"#define SB_PRED_STARTS_WITH (\d+)", open(HEADER).read()).group(1)) == N.SB_PRED_STARTS_WITH == 8


def test_binary_literals():
    for ptype in (P.BINARY, P.LARGE_BINARY, P.UTF8, P.LARGE_UTF8):
        for op in ("eq", "ne", "lt", "le", "gt", "ge", "starts_with"):
            assert literal_bytes(ptype, op, b"Paris") == b"Paris"
            assert literal_bytes(ptype, op, "Paris") == b"Paris"
            assert literal_bytes(ptype, op, b"") == b"" == literal_bytes(ptype, op, "")
            assert literal_bytes(ptype, op, "Zürich") == "Zürich".encode("utf-8") and len(literal_bytes(ptype, op, "Zürich")) == 7
            assert literal_bytes(ptype, op, b"a\0b\xff") == b"a\0b\xff"          # any byte, zero included
            assert literal_bytes(ptype, op, bytearray(b"xy")) == b"xy"
            assert literal_bytes(ptype, op, b"q" * 300) == b"q" * 300              # any length
        assert literal_bytes(ptype, "is_null", None) == b""


def test_numeric_literals_have_the_types_width():
    assert literal_bytes(P.INT8, "lt", -1) == b"\xff"
    assert literal_bytes(P.UINT16, "eq", 513) == b"\x01\x02"
    assert literal_bytes(P.INT32, "ge", 7) == b"\x07\0\0\0"
    assert literal_bytes(P.FLOAT32, "lt", 1.5) == np.float32(1.5).tobytes()
    assert literal_bytes(P.FLOAT64, "lt", 1.5) == np.float64(1.5).tobytes()
    assert literal_bytes(P.UINT64, "ne", (1 << 64) - 1) == b"\xff" * 8
    for ptype in (P.INT8, P.INT16, P.INT32, P.INT64, P.UINT8, P.UINT16, P.UINT32, P.UINT64, P.FLOAT32, P.FLOAT64):
        assert len(literal_bytes(ptype, "eq", 1)) == P.WIDTH[ptype]
        assert literal_bytes(ptype, "eq", 1) == pack_literal(ptype, 1)[:P.WIDTH[ptype]]
    with pytest.raises(ValueError):
        literal_bytes(P.INT8, "lt", 1000)       # pack_literal's rules hold


def test_pack_literal_keeps_its_contract():
    for ptype in (P.BINARY, P.LARGE_BINARY):
        with pytest.raises(ValueError):
            pack_literal(ptype, 1)
        with pytest.raises(ValueError):
            pack_literal(ptype, b"a")


def test_mismatched_literals_are_refused():
    for ptype in (P.INT8, P.INT32, P.UINT64, P.FLOAT32, P.FLOAT64):
        for bad in (b"abc", "abc", b"", bytearray(b"1")):
            with pytest.raises(ValueError):
                literal_bytes(ptype, "eq", bad)
        with pytest.raises(ValueError):
            literal_bytes(ptype, "starts_with", b"a")
        with pytest.raises(ValueError):
            literal_bytes(ptype, "starts_with", 1)
    for ptype in (P.BINARY, P.LARGE_BINARY):
        for bad in (1, 1.5, np.int64(3), None, True, [b"a"]):
            with pytest.raises(ValueError):
                literal_bytes(ptype, "eq", bad)
            with pytest.raises(ValueError):
                literal_bytes(ptype, "starts_with", bad)
    for ptype in (P.BOOLEAN, P.INT128, P.INT256, P.NULL):
        with pytest.raises(ValueError):
            literal_bytes(ptype, "lt", 1)
        with pytest.raises(ValueError):
            literal_bytes(ptype, "starts_with", b"a")


def test_predicates():
    assert Predicate("starts_with", b"https://").literal == b"https://"
    assert Predicate("starts_with", "").literal == ""
    assert Predicate("eq", "Paris").op == "eq"
    with pytest.raises(ValueError):
        Predicate("starts_with")
    with pytest.raises(ValueError):
        Predicate("like", "a%")


def test_bad_arguments_raise_before_anything_is_enqueued():
    """ctx is never touched: the checks come first"""
    from strawboat_amd.read import ColumnPages
    num = ColumnPages(P.INT32, False, None, np.zeros((0, 2), np.uint64))
    for large in (P.BINARY, P.LARGE_BINARY):
        col = ColumnPages(large, True, None, np.zeros((0, 2), np.uint64))
        with pytest.raises(ValueError):
            filter_columns(None, [col], [Predicate("eq", 1)])              # a number on a binary column
        with pytest.raises(ValueError):
            filter_columns(None, [col], [Predicate("starts_with", 7)])
        with pytest.raises(ValueError):
            filter_columns(None, [num, col], [Predicate("lt", 1), Predicate("lt", 2.5)])   # the second column of a mixed call
        with pytest.raises(ValueError):
            filter_columns(None, [col], [Predicate("eq", b"a")], stage_capacity=[1, 2])
    with pytest.raises(ValueError):
        filter_columns(None, [num], [Predicate("eq", b"abc")])                # bytes on a numeric column
    with pytest.raises(ValueError):
        filter_columns(None, [num], [Predicate("eq", "abc")])
    with pytest.raises(ValueError):
        filter_columns(None, [num], [Predicate("starts_with", b"a")])         # starts_with on a numeric column
    with pytest.raises(ValueError):
        filter_columns(None, [num], [Predicate("starts_with", 1)])
