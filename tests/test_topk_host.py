"""sb_topk_columns without a GPU: the symbol is exported, the ctypes structs have the header's layout, the Python layer
refuses what needs no device before anything is enqueued, and the reference that tests/test_gpu_topk.py compares the
device with (tests/topk_ref.py) is checked against a brute-force Python `sorted` on small arrays."""
import ctypes as C
import functools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import sbo as S
from strawboat_amd import _native as N
from strawboat_amd.topk import check_column, selection_of_rows, topk_columns
from strawboat_amd.types import PhysicalType as P
from tests import topk_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")


def test_symbol_is_declared_and_exported():
    assert "sb_topk_columns" in N.EXPORTS
    assert re.search(r"\bsb_topk_columns\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_topk_columns$", out, re.M)


def test_ctypes_structs_have_the_headers_layout(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    fields = [name for name, _ in N.ColumnTopKC._fields_]
    row_fields = [name for name, _ in N.TopKRowC._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu %zu\\n", sizeof(sb_column_topk), sizeof(sb_topk_row));\n'
                   '    printf("consts %u %u %u\\n", SB_TOPK_MAX_K, SB_TOPK_SMALLEST, SB_TOPK_LARGEST);\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_topk, %s));\n' % (f, f) for f in fields) +
                   "".join('    printf("row.%s %%zu\\n", offsetof(sb_topk_row, %s));\n' % (f, f) for f in row_fields) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    got = dict(line.split(None, 1) for line in lines)
    assert got["sizeof"].split() == [str(C.sizeof(N.ColumnTopKC)), str(C.sizeof(N.TopKRowC))] == ["128", "16"]
    assert got["consts"].split() == [str(c) for c in (N.SB_TOPK_MAX_K, N.SB_TOPK_SMALLEST, N.SB_TOPK_LARGEST)] == ["256", "0", "1"]
    for f in fields:
        assert int(got[f]) == getattr(N.ColumnTopKC, f).offset, f
    for f in row_fields:
        assert int(got["row." + f]) == getattr(N.TopKRowC, f).offset, f
    # ... and the offsets the header's comment pins
    text = open(HEADER).read().split("Layout (pinned by tests/test_topk_host.py)")[1].split("*/")[0]
    row_text, col_text = text.split("sb_column_topk 128 bytes;")
    assert "sb_topk_row 16 bytes;" in row_text
    pinned_row = dict(re.findall(r"(\w+) (\d+)[,.]", row_text.split("sb_topk_row 16 bytes;")[1]))
    pinned = dict(re.findall(r"(\w+) (\d+)[,.]", col_text))
    assert set(pinned) == set(fields) and set(pinned_row) == set(row_fields)
    for f in fields:
        assert int(pinned[f]) == getattr(N.ColumnTopKC, f).offset, f
    for f in row_fields:
        assert int(pinned_row[f]) == getattr(N.TopKRowC, f).offset, f


def test_unsupported_types_bad_k_bad_order_and_short_bitmaps_are_refused_on_the_host():
    every = (P.INT8, P.INT16, P.INT32, P.INT64, P.UINT8, P.UINT16, P.UINT32, P.UINT64, P.FLOAT32, P.FLOAT64,
             P.BOOLEAN, P.INT128, P.INT256, P.BINARY, P.LARGE_BINARY, P.NULL)
    for ptype in every[:10]:
        for k in (1, 7, 256):
            check_column(ptype, 33, 8, k, False)
            check_column(ptype, 33, None, k, True)
    for ptype in every[10:]:
        with pytest.raises(ValueError):
            check_column(ptype, 33, 8, 5, False)
    for k in (0, -1, 257, 1 << 32, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, k, False)
    for order in (0, 1, 2, "desc", None):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, 5, order)
    for rows, nbytes in ((1, 0), (33, 4), (33, 7), (10_000, 1250)):   # (1250 = ceil(rows/8): whole words are asked for)
        with pytest.raises(ValueError):
            check_column(P.INT64, rows, nbytes, 5, False)


def test_bad_arguments_raise_before_anything_is_enqueued():
    """the context is never called: the checks come first"""
    import torch
    from strawboat_amd.read import ColumnPages

    class Ctx:   # (only asked where its tensors live)
        torch_device = torch.device("cpu")

    metas = np.array([[100, 40]], np.uint64)
    col = ColumnPages(P.INT64, False, torch.zeros(100, dtype=torch.uint8), metas)
    with pytest.raises(ValueError):   # a bitmap of 4 bytes for 40 rows
        topk_columns(Ctx(), [col], 5, selection=torch.zeros(4, dtype=torch.uint8))
    for ptype in (P.BOOLEAN, P.BINARY, P.INT128, P.NULL):
        with pytest.raises(ValueError):
            topk_columns(Ctx(), [ColumnPages(ptype, False, col.pages, metas)], 5)
    for k in (0, 257, [5], [5, 5, 5]):   # k out of range; not one k per column
        with pytest.raises(ValueError):
            topk_columns(Ctx(), [col, col], k)
    with pytest.raises(ValueError):   # one order per column
        topk_columns(Ctx(), [col, col], 5, largest=[True])
    with pytest.raises(ValueError):   # one selection per column
        topk_columns(Ctx(), [col, col], 5, selection=[torch.zeros(8, dtype=torch.uint8)])
    with pytest.raises(TypeError):    # not a bitmap
        topk_columns(Ctx(), [col], 5, selection=[np.zeros(8, np.uint8)])
    with pytest.raises(ValueError):   # a bitmap on another device
        topk_columns(Ctx(), [col], 5, selection=torch.zeros(8, dtype=torch.uint8, device="meta"))


def test_selection_of_rows_builds_the_bitmap():
    import torch

    class Ctx:
        torch_device = torch.device("cpu")

    sel = selection_of_rows(Ctx(), 100, np.array([99, 0, 31, 32, 33, 64, 0], np.uint64))
    want = np.zeros(100, bool)
    want[[0, 31, 32, 33, 64, 99]] = True
    assert sel.bitmap.numel() == 16 and sel.rows == 100 and sel.selected == 6
    assert np.array_equal(sel.numpy(), want)
    assert selection_of_rows(Ctx(), 40, []).numpy().sum() == 0
    assert selection_of_rows(Ctx(), 0, []).bitmap.numel() == 0
    with pytest.raises(ValueError):
        selection_of_rows(Ctx(), 100, [100])


# ---- the reference against a brute-force Python sort
def _brute(vals, live, k, largest):
    """Python's `sorted` over (value, row) tuples with a comparison spelled out: by value (-0.0 below +0.0), descending for
    `largest`, and by the lower row for equal values in both orders"""
    def zero_rank(v):
        return (v, 0 if (isinstance(v, float) and v == 0 and math.copysign(1.0, v) < 0) else 1)

    def cmp(a, b):
        ka, kb = zero_rank(a[0]), zero_rank(b[0])
        if ka != kb:
            return (-1 if ka < kb else 1) * (-1 if largest else 1)
        return -1 if a[1] < b[1] else 1

    cands = [(v, r) for r, (v, on) in enumerate(zip(vals.tolist(), live.tolist())) if on and v == v]
    return [r for _, r in sorted(cands, key=functools.cmp_to_key(cmp))[:k]]


def _check_against_brute(ptype, vals, live, ks=(1, 3, 7, 64)):
    for largest in (False, True):
        for k in ks:
            w = T.topk_values(ptype, vals, live, int(live.sum()), k, largest)
            rows = _brute(vals, live, k, largest)
            assert w.row_ids.tolist() == rows, (ptype, k, largest)
            wd = vals.dtype.itemsize
            assert w.value_bytes[:, :wd].tobytes() == vals[rows].tobytes() and not w.value_bytes[:, wd:].any()
            assert w.found == len(rows) == min(k, w.count - w.nans)
            assert len(w.out_bytes) == 16 * k and w.out_bytes[16 * w.found:] == bytes(16 * (k - w.found))


@pytest.mark.parametrize("ptype,dtype", [(S.T_F32, np.float32), (S.T_F64, np.float64)])
def test_the_reference_on_floats_with_ties_zeros_nans_and_infinities(ptype, dtype):
    rng = np.random.default_rng(ptype)
    tiny = np.finfo(dtype).smallest_subnormal
    pool = np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0, tiny, -tiny, 1.5, 1.5, -2.25, 7.0], dtype)
    vals = pool[rng.integers(0, pool.size, 200)]
    live = rng.random(200) < 0.7
    _check_against_brute(ptype, vals, live)
    w = T.topk_values(ptype, vals, live, int(live.sum()), 200, False)
    assert w.nans == int(np.isnan(vals[live]).sum()) > 0 and w.found == w.count - w.nans
    assert not np.isnan(vals[w.row_ids.astype(np.int64)]).any()
    # only the zeros: every -0.0 before every +0.0, rows ascending inside each, in the ascending order
    zeros = np.array([0.0, -0.0, 0.0, -0.0, -0.0], dtype)
    w = T.topk_values(ptype, zeros, np.ones(5, bool), 5, 5, False)
    assert w.row_ids.tolist() == [1, 3, 4, 0, 2]
    w = T.topk_values(ptype, zeros, np.ones(5, bool), 5, 5, True)
    assert w.row_ids.tolist() == [0, 2, 1, 3, 4]
    # only NaNs: nothing is found, and the tail is all of out
    w = T.topk_values(ptype, np.array([np.nan] * 3, dtype), np.ones(3, bool), 3, 4, False)
    assert (w.count, w.nans, w.found) == (3, 3, 0) and w.out_bytes == bytes(64)


@pytest.mark.parametrize("ptype", [S.T_I8, S.T_I16, S.T_I32, S.T_I64, S.T_U8, S.T_U16, S.T_U32, S.T_U64])
def test_the_reference_on_integers_with_ties_and_extremes(ptype):
    dt = np.dtype(T.NP[ptype])
    info = np.iinfo(dt)
    rng = np.random.default_rng(ptype)
    pool = np.array([info.min, info.min, info.max, info.max, 0, 1, info.max - 1, info.min + 1, 5, 5, 5], dt)
    vals = pool[rng.integers(0, pool.size, 150)]
    live = rng.random(150) < 0.6
    _check_against_brute(ptype, vals, live)
    w = T.topk_values(ptype, vals, live, int(live.sum()), 1, False)
    assert vals[int(w.row_ids[0])] == info.min and int(w.row_ids[0]) == int(np.flatnonzero(live & (vals == info.min))[0])
    w = T.topk_values(ptype, vals, live, int(live.sum()), 1, True)
    assert vals[int(w.row_ids[0])] == info.max and int(w.row_ids[0]) == int(np.flatnonzero(live & (vals == info.max))[0])


def test_the_reference_with_fewer_candidates_than_k():
    vals = np.array([3, 1, 2], np.int32)
    w = T.topk_values(S.T_I32, vals, np.array([True, False, True]), 2, 7, False)
    assert (w.found, w.row_ids.tolist()) == (2, [2, 0]) and w.out_bytes[32:] == bytes(16 * 5)
    w = T.topk_values(S.T_I32, vals, np.zeros(3, bool), 0, 7, True)
    assert (w.count, w.found) == (0, 0) and w.out_bytes == bytes(16 * 7)
