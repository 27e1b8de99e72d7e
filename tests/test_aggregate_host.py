"""sb_aggregate_columns without a GPU: the symbol is exported, the ctypes struct has the header's layout, the Python layer
refuses what needs no device before anything is enqueued, and the reference helper that tests/test_gpu_aggregate.py
compares the device with (tests/aggregate_ref.py) is checked on its own."""
import ctypes as C
import math
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import sbo as S
from strawboat_amd import _native as N
from strawboat_amd.aggregate import aggregate_columns, check_column, ops_mask
from strawboat_amd.types import PhysicalType as P
from tests import aggregate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")


def test_symbol_is_declared_and_exported():
    assert "sb_aggregate_columns" in N.EXPORTS
    assert re.search(r"\bsb_aggregate_columns\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_aggregate_columns$", out, re.M)


def test_ctypes_struct_has_the_headers_layout(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    fields = [name for name, _ in N.ColumnAggregateC._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(sb_column_aggregate));\n'
                   '    printf("bits %u %u %u %u\\n", SB_AGG_COUNT, SB_AGG_MIN, SB_AGG_MAX, SB_AGG_SUM);\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_aggregate, %s));\n' % (f, f) for f in fields) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    got = dict(line.split(None, 1) for line in lines)
    assert int(got["sizeof"]) == C.sizeof(N.ColumnAggregateC) == 136
    assert got["bits"].split() == [str(b) for b in (N.SB_AGG_COUNT, N.SB_AGG_MIN, N.SB_AGG_MAX, N.SB_AGG_SUM)] == ["1", "2", "4", "8"]
    for f in fields:
        assert int(got[f]) == getattr(N.ColumnAggregateC, f).offset, f
    # ... and the offsets the header's comment pins
    pinned = dict(re.findall(r"(\w+) (\d+)[,.]", open(HEADER).read().split("Layout (pinned by tests/test_aggregate_host.py)")[1].split("*/")[0]))
    assert set(pinned) == set(fields)
    for f in fields:
        assert int(pinned[f]) == getattr(N.ColumnAggregateC, f).offset, f


def test_unsupported_types_short_bitmaps_and_unknown_ops_are_refused_on_the_host():
    every = (P.INT8, P.INT16, P.INT32, P.INT64, P.UINT8, P.UINT16, P.UINT32, P.UINT64, P.FLOAT32, P.FLOAT64,
             P.BOOLEAN, P.INT128, P.INT256, P.BINARY, P.LARGE_BINARY, P.NULL)
    for ptype in every:   # count works on every type, with or without a bitmap
        check_column(ptype, 33, 8, N.SB_AGG_COUNT)
        check_column(ptype, 33, None, 0)
    for ptype in every[:10]:
        check_column(ptype, 33, 8, 15)
    for ptype in every[10:]:
        for op in (N.SB_AGG_MIN, N.SB_AGG_MAX, N.SB_AGG_SUM, 15):
            with pytest.raises(ValueError):
                check_column(ptype, 33, 8, op)
    for rows, nbytes in ((1, 0), (33, 4), (33, 7), (10_000, 1250)):   # (1250 = ceil(rows/8): whole words are asked for)
        with pytest.raises(ValueError):
            check_column(P.INT64, rows, nbytes, 15)
    assert ops_mask(("count", "min", "max", "sum")) == 15 and ops_mask(()) == 0 and ops_mask(("count",)) == 1 and ops_mask(9) == 9
    for bad in (("avg",), ("count", "median"), 16, 31, -1):
        with pytest.raises(ValueError):
            ops_mask(bad)


def test_bad_arguments_raise_before_anything_is_enqueued():
    """the context is never called: the checks come first"""
    import torch
    from strawboat_amd.read import ColumnPages

    class Ctx:   # (only asked where its tensors live)
        torch_device = torch.device("cpu")

    metas = np.array([[100, 40]], np.uint64)
    col = ColumnPages(P.INT64, False, torch.zeros(100, dtype=torch.uint8), metas)
    with pytest.raises(ValueError):   # a bitmap of 4 bytes for 40 rows
        aggregate_columns(Ctx(), [col], torch.zeros(4, dtype=torch.uint8))
    for ptype in (P.BOOLEAN, P.BINARY, P.INT128, P.NULL):   # an unsupported type with min / max / sum
        for ops in (("min",), ("count", "max"), ("sum",)):
            with pytest.raises(ValueError):
                aggregate_columns(Ctx(), [ColumnPages(ptype, False, col.pages, metas)], torch.zeros(8, dtype=torch.uint8), ops=ops)
    with pytest.raises(ValueError):   # unknown ops
        aggregate_columns(Ctx(), [col], None, ops=("count", "avg"))
    with pytest.raises(ValueError):   # one selection per column
        aggregate_columns(Ctx(), [col, col], [torch.zeros(8, dtype=torch.uint8)])
    with pytest.raises(TypeError):    # not a bitmap
        aggregate_columns(Ctx(), [col], [np.zeros(8, np.uint8)])
    with pytest.raises(ValueError):   # a bitmap on another device
        aggregate_columns(Ctx(), [col], torch.zeros(8, dtype=torch.uint8, device="meta"))


# ---- the reference helper
@pytest.mark.parametrize("ptype,dtype", [(S.T_F32, np.float32), (S.T_F64, np.float64)])
def test_the_order_key_is_the_total_order_of_floats(ptype, dtype):
    tiny = np.finfo(dtype).smallest_subnormal
    ladder = [-np.inf, -1.0, -tiny, -0.0, 0.0, tiny, np.finfo(dtype).tiny, 1.0, np.inf]
    keys = [R.order_key(ptype, dtype(x)) for x in ladder]
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    assert R.order_key(ptype, dtype(-0.0)) < R.order_key(ptype, dtype(0.0))


def test_the_order_key_of_integers_goes_by_signedness():
    assert [R.order_key(S.T_I8, x) for x in (-128, -1, 0, 127)] == [0, 127, 128, 255]
    assert [R.order_key(S.T_U8, x) for x in (0, 127, 128, 255)] == [0, 127, 128, 255]
    k = [R.order_key(S.T_I64, x) for x in (-2 ** 63, -1, 0, 2 ** 63 - 1)]
    assert k == sorted(k) and k[0] == 0 and k[-1] == 2 ** 64 - 1
    assert R.order_key(S.T_U64, 2 ** 64 - 1) > R.order_key(S.T_U64, 2 ** 63)


@pytest.mark.parametrize("ptype,dtype", [(S.T_F32, np.float32), (S.T_F64, np.float64)])
def test_nans_of_either_sign_are_counted_and_kept_out_of_min_and_max(ptype, dtype):
    w = np.dtype(dtype).itemsize
    neg_nan = np.array([1], "<u%d" % w)
    neg_nan[0] = (0xFFC00000 if w == 4 else 0xFFF8000000000000) | 5
    v = np.array([2.5, np.nan, -0.0, 0.0, 0.0, -3.0, 7.0, 0.0], dtype)
    v[4] = neg_nan.view(dtype)[0]
    live = np.array([1, 1, 1, 1, 1, 1, 1, 0], bool)
    want = R.reduce_values(ptype, v, live, 8)
    assert (want.rows, want.selected, want.count, want.nans) == (8, 8, 7, 2)
    assert want.min_bytes[:w] == dtype(-3.0).tobytes() and want.max_bytes[:w] == dtype(7.0).tobytes()
    assert want.min_bytes[w:] == bytes(8 - w)
    assert math.isnan(want.fsum)
    # only the zeros: -0.0 is the minimum, +0.0 the maximum, bit for bit
    want = R.reduce_values(ptype, v, np.array([0, 0, 1, 1, 0, 0, 0, 1], bool), 3)
    assert want.min_bytes[:w] == dtype(-0.0).tobytes() and want.max_bytes[:w] == dtype(0.0).tobytes() and want.nans == 0
    # only NaNs: no row qualifies
    want = R.reduce_values(ptype, v, np.array([0, 1, 0, 0, 1, 0, 0, 0], bool), 2)
    assert want.count == 2 and want.nans == 2 and want.min_bytes == bytes(8) and want.max_bytes == bytes(8)
    # without min / max / sum no value is looked at
    want = R.reduce_values(ptype, v, live, 8, ops=("count",))
    assert (want.count, want.nans, want.fsum) == (7, 0, None)


def test_the_128_bit_split_of_python_sums():
    for v in (2 ** 63 * 10 ** 4, -(2 ** 63 * 10 ** 4), (2 ** 64 - 1) * 10 ** 4, 0, -1, 2 ** 64, -(2 ** 64)):
        lo, hi = R.split128(v)
        assert 0 <= lo < 2 ** 64 and 0 <= hi < 2 ** 64 and R.join128(lo, hi) == v
    assert R.split128(2 ** 63 * 10 ** 4) == ((2 ** 63 * 10 ** 4) % 2 ** 64, 4999 + 1)
    assert R.split128(-(2 ** 63 * 10 ** 4)) == ((-(2 ** 63 * 10 ** 4)) % 2 ** 64, 2 ** 64 - 5000)
    assert R.split128((2 ** 64 - 1) * 10 ** 4) == (2 ** 64 - 10 ** 4, 10 ** 4 - 1)
    assert R.split128(-1) == (2 ** 64 - 1, 2 ** 64 - 1)
    # 10^4 rows of INT64_MIN / of UINT64_MAX through the helper
    want = R.reduce_values(S.T_I64, np.full(10 ** 4, -2 ** 63, np.int64), np.ones(10 ** 4, bool), 10 ** 4)
    assert R.join128(want.sum_lo, want.sum_hi) == -(2 ** 63 * 10 ** 4)
    assert want.min_bytes == want.max_bytes == struct.pack("<q", -2 ** 63)
    want = R.reduce_values(S.T_U64, np.full(10 ** 4, 2 ** 64 - 1, np.uint64), np.ones(10 ** 4, bool), 10 ** 4)
    assert R.join128(want.sum_lo, want.sum_hi) == (2 ** 64 - 1) * 10 ** 4
    want = R.reduce_values(S.T_I8, np.array([-128, 127, -1], np.int8), np.ones(3, bool), 3)
    assert R.join128(want.sum_lo, want.sum_hi) == -2 and want.min_bytes == b"\x80" + bytes(7) and want.max_bytes == b"\x7f" + bytes(7)


def test_the_float_sum_bound():
    rng = np.random.default_rng(1)
    x = rng.normal(size=5000) * 10.0 ** rng.integers(-3, 6, 5000)
    want = R.reduce_values(S.T_F64, x, np.ones(5000, bool), 5000)
    assert want.fsum == math.fsum(x.tolist()) and want.abs_sum == math.fsum(np.abs(x).tolist())
    bound = R.float_sum_bound(want)
    assert bound == 5000 * 2.0 ** -52 * want.abs_sum
    for order in (x, x[::-1], np.sort(x), x[rng.permutation(5000)]):   # any order of double additions stays inside
        s = 0.0
        for v in order.tolist():
            s += v
        assert abs(s - want.fsum) <= bound
