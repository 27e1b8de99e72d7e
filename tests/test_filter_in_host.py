"""sb_filter_columns_in without a GPU: the symbol is exported and declared, sb_column_filter_in has the layout the header
states, and the Python layer packs the lists and refuses bad arguments on the host, before anything is enqueued."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from strawboat_amd import _native as N
from strawboat_amd.types import PhysicalType as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")

OFFSETS = dict(physical_type=0, is_nullable=4, pages=8, pages_len=16, metas=24, n_pages=32, page_offsets=40, op=48, combine=52,
               values=56, value_offsets=64, n_values=72, selection=80, selection_capacity=88, stage_capacity=96, rows=104, selected=112)


def test_symbol_is_declared_and_exported():
    assert "sb_filter_columns_in" in N.EXPORTS
    assert re.search(r"\bsb_filter_columns_in\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_filter_columns_in$", out, re.M)
    assert re.search(r"\bT sb_filter_columns_var$", out, re.M) and re.search(r"\bT sb_filter_columns$", out, re.M)


def test_struct_is_120_bytes_with_the_stated_offsets(tmp_path):
    assert C.sizeof(N.ColumnFilterInC) == 120
    assert [name for name, _ in N.ColumnFilterInC._fields_] == list(OFFSETS)
    for f, off in OFFSETS.items():
        assert getattr(N.ColumnFilterInC, f).offset == off, f
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(sb_column_filter_in));\n'
                   '    printf("var %zu\\n", sizeof(sb_column_filter_var));\n'
                   '    printf("IN %d\\nNOT_IN %d\\nMAX %u\\n", SB_PRED_IN, SB_PRED_NOT_IN, SB_IN_MAX_VALUES);\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_filter_in, %s));\n' % (f, f) for f in OFFSETS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == 120
    assert int(got["var"]) == C.sizeof(N.ColumnFilterVarC) == 112   # sb_column_filter_var keeps its layout
    for f, off in OFFSETS.items():
        assert int(got[f]) == off, f
    assert int(got["IN"]) == N.SB_PRED_IN == 9 and int(got["NOT_IN"]) == N.SB_PRED_NOT_IN == 10
    assert int(got["MAX"]) == N.SB_IN_MAX_VALUES == 1024
    # the header's comment states the offsets
    text = " ".join(open(HEADER).read().split())
    for f, off in OFFSETS.items():
        assert re.search(r"\b%s %d\b" % (f, off), text.replace(" * ", " ")), f


def test_lists_are_packed_as_the_struct_takes_them():
    from strawboat_amd.filter_in import InList, pack_list
    raw, offs = pack_list(P.INT16, [3, -1, 3, 513])
    assert raw == struct.pack("<4h", 3, -1, 3, 513) and offs is None      # any order, duplicates kept: the library sorts
    raw, offs = pack_list(P.UINT64, [2 ** 64 - 1, 2 ** 63])
    assert raw == struct.pack("<2Q", 2 ** 64 - 1, 2 ** 63) and offs is None
    raw, offs = pack_list(P.FLOAT32, [1.5, float("nan"), -0.0])
    assert raw[:4] == struct.pack("<f", 1.5) and raw[8:] == struct.pack("<f", -0.0) and len(raw) == 12
    raw, offs = pack_list(P.FLOAT64, [])
    assert raw == b"" and offs is None
    for ptype in (P.BINARY, P.LARGE_BINARY):
        raw, offs = pack_list(ptype, [b"ab", "", "Zürich", bytearray(b"\0")])
        assert raw == b"ab" + "Zürich".encode("utf-8") + b"\0"
        assert offs.dtype == np.uint64 and offs.tolist() == [0, 2, 2, 9, 10]
        raw, offs = pack_list(ptype, [])
        assert raw == b"" and offs.tolist() == [0]
    assert InList([1, 2]).negate is False and InList([1], negate=True).negate is True
    assert len(InList(range(1024)).values) == 1024


def test_bad_arguments_raise_before_anything_is_enqueued():
    """ctx is never touched: the checks come first"""
    from strawboat_amd.filter import Selection
    from strawboat_amd.filter_in import FilterInBatch, InList, filter_in, pack_list
    from strawboat_amd.read import ColumnPages
    num = ColumnPages(P.INT32, False, None, np.zeros((0, 2), np.uint64))
    txt = ColumnPages(P.BINARY, True, None, np.zeros((0, 2), np.uint64))
    with pytest.raises(ValueError):
        InList(range(1025))                                        # more than 1024 values
    with pytest.raises(ValueError):
        pack_list(P.INT32, list(range(1025)))
    big = InList([1])
    big.values = list(range(1025))                                 # ... also when the list grew after it was made
    with pytest.raises(ValueError):
        filter_in(None, [num], [big])
    for bad in ("abc", b"abc", bytearray(b"1")):
        with pytest.raises(ValueError):
            filter_in(None, [num], [InList([1, bad])])             # a str / bytes literal for a numeric column
    with pytest.raises(ValueError):
        filter_in(None, [txt], [InList(["a", 1])])                 # a number on a binary column
    with pytest.raises(ValueError):
        filter_in(None, [num], [InList([1 << 40])])                # does not fit the type
    with pytest.raises(ValueError):
        filter_in(None, [num], [InList([1.5])])
    with pytest.raises(ValueError):
        filter_in(None, [ColumnPages(P.BOOLEAN, False, None, np.zeros((0, 2), np.uint64))], [InList([1])])
    with pytest.raises(ValueError):
        filter_in(None, [num, num], [InList([1])])                 # one list per column
    with pytest.raises(ValueError):
        filter_in(None, [num], [[1, 2]])                           # not an InList
    with pytest.raises(ValueError):
        filter_in(None, [num], [InList([1])], combine="xor")
    with pytest.raises(ValueError):
        filter_in(None, [num], [InList([1])], combine="and")       # nothing to combine with
    with pytest.raises(ValueError):
        FilterInBatch(None, [num], [InList([1])], out=[])          # a wrong `out` length
    with pytest.raises(ValueError):
        FilterInBatch(None, [num, num], [InList([1]), InList([2])], combine="or", out=[Selection(None, 0, None)])
    with pytest.raises(ValueError):
        filter_in(None, [num], [InList([1])], out=[Selection(None, 7, None)])   # a selection of another column's rows
    with pytest.raises(ValueError):
        filter_in(None, [num], [InList([1])], stage_capacity=[1, 2])
