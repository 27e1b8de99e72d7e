"""sb_aggregate_grouped without a GPU: the symbol is exported, the ctypes structs have the header's layout, the Python layer
refuses what needs no device before anything is enqueued, and the reference helper that tests/test_gpu_aggregate_grouped.py
compares the device with (tests/aggregate_grouped_ref.py) is checked on its own."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import sbo as S
from strawboat_amd import _native as N
from strawboat_amd.types import PhysicalType as P
from tests import aggregate_grouped_ref as G
from tests import aggregate_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")
PINNED = "Layout (pinned by tests/test_aggregate_grouped_host.py)"


def test_symbol_is_declared_and_exported():
    assert "sb_aggregate_grouped" in N.EXPORTS
    assert re.search(r"\bsb_aggregate_grouped\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_aggregate_grouped$", out, re.M)
    import strawboat_amd as sb
    assert sb.aggregate_grouped and sb.GroupedAggregateBatch and sb.GroupedAggregate


def test_ctypes_structs_have_the_headers_layout(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    structs = (("sb_column_aggregate_grouped", N.ColumnAggregateGroupedC, 128), ("sb_agg_group", N.AggGroupC, 64))
    body = '    printf("max_groups %u\\n", SB_AGG_MAX_GROUPS);\n'
    for cname, ct, _ in structs:
        body += '    printf("%s.sizeof %%zu\\n", sizeof(%s));\n' % (cname, cname)
        body += "".join('    printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (cname, f, cname, f) for f, _ in ct._fields_)
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n' + body + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    got = dict(line.split(None, 1) for line in lines)
    assert int(got["max_groups"]) == N.SB_AGG_MAX_GROUPS == 256
    # the header's comment: "<struct> <size> bytes; field offset, field offset, ..." per struct
    text = open(HEADER).read().split(PINNED)[1].split("*/")[0]
    for cname, ct, size in structs:
        fields = [f for f, _ in ct._fields_]
        assert int(got[cname + ".sizeof"]) == C.sizeof(ct) == size, cname
        for f in fields:
            assert int(got["%s.%s" % (cname, f)]) == getattr(ct, f).offset, (cname, f)
        part = text.split(cname + " %d bytes;" % size)[1].split(" bytes;")[0]
        pinned = dict(re.findall(r"(\w+) (\d+)[,.]", part))
        assert set(fields) <= set(pinned), (cname, set(fields) - set(pinned))
        for f in fields:
            assert int(pinned[f]) == getattr(ct, f).offset, (cname, f)
    assert N.ColumnAggregateGroupedC.groups.offset == 96 and N.ColumnAggregateGroupedC.out_of_range.offset == 120


def test_check_column_holds_the_refusals_that_need_no_device():
    from strawboat_amd.aggregate_grouped import check_column
    every = (P.INT8, P.INT16, P.INT32, P.INT64, P.UINT8, P.UINT16, P.UINT32, P.UINT64, P.FLOAT32, P.FLOAT64,
             P.BOOLEAN, P.INT128, P.INT256, P.BINARY, P.LARGE_BINARY, P.NULL)
    for ptype in every:   # count works on every type
        check_column(ptype, 33, 8, N.SB_AGG_COUNT, 4, 1, 33)
        check_column(ptype, 33, None, 0, 256, 4, 40)
    for ptype in every[:10]:
        check_column(ptype, 33, 8, 15, 1, 2, 33)
    for ptype in every[10:]:
        for op in (N.SB_AGG_MIN, N.SB_AGG_MAX, N.SB_AGG_SUM, 15):
            with pytest.raises(ValueError):
                check_column(ptype, 33, 8, op, 4, 1, 33)
    with pytest.raises(ValueError):   # a short bitmap
        check_column(P.INT64, 33, 4, 15, 4, 1, 33)
    for bad in (0, 257, -1, 1 << 20, 2.0, None, True):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, 15, bad, 1, 33)
    for width in (None, 0, 3, 8):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, 15, 4, width, 33)
    with pytest.raises(ValueError):   # fewer ids than rows
        check_column(P.INT64, 33, 8, 15, 4, 1, 32)
    check_column(P.INT64, 0, None, 15, 4, 1, 0)


def test_bad_arguments_raise_before_anything_is_enqueued():
    """the context is never called: the checks come first"""
    import torch
    from strawboat_amd import aggregate_grouped
    from strawboat_amd.read import ColumnPages

    class Ctx:   # (only asked where its tensors live)
        torch_device = torch.device("cpu")

    metas = np.array([[100, 40]], np.uint64)
    col = ColumnPages(P.INT64, False, torch.zeros(100, dtype=torch.uint8), metas)
    ids = torch.zeros(40, dtype=torch.uint8)
    bm = torch.zeros(8, dtype=torch.uint8)
    with pytest.raises(ValueError):   # a bitmap of 4 bytes for 40 rows
        aggregate_grouped(Ctx(), [col], ids, 4, torch.zeros(4, dtype=torch.uint8))
    for n_groups in (0, 257, -3):
        with pytest.raises(ValueError):
            aggregate_grouped(Ctx(), [col], ids, n_groups, bm)
    for bad in (torch.zeros(40, dtype=torch.int64), torch.zeros(40, dtype=torch.float32), torch.zeros(40, dtype=torch.int8),
                torch.zeros(39, dtype=torch.uint8), torch.zeros(80, dtype=torch.uint8)[::2], torch.zeros((40, 1), dtype=torch.uint8),
                torch.zeros(40, dtype=torch.uint8, device="meta"), np.zeros(40, np.uint8)):
        with pytest.raises(ValueError):
            aggregate_grouped(Ctx(), [col], bad, 4, bm)
    for ptype in (P.BOOLEAN, P.BINARY, P.INT128, P.NULL):   # an unsupported type with min / max / sum
        for ops in (("min",), ("count", "max"), ("sum",)):
            with pytest.raises(ValueError):
                aggregate_grouped(Ctx(), [ColumnPages(ptype, False, col.pages, metas)], ids, 4, bm, ops=ops)
    with pytest.raises(ValueError):   # unknown ops
        aggregate_grouped(Ctx(), [col], ids, 4, None, ops=("count", "avg"))
    with pytest.raises(ValueError):   # one selection / one ids tensor / one n_groups per column
        aggregate_grouped(Ctx(), [col, col], ids, 4, [bm])
    with pytest.raises(ValueError):
        aggregate_grouped(Ctx(), [col, col], [ids], 4, bm)
    with pytest.raises(ValueError):
        aggregate_grouped(Ctx(), [col, col], ids, [4], bm)
    with pytest.raises(TypeError):    # not a bitmap
        aggregate_grouped(Ctx(), [col], ids, 4, [np.zeros(8, np.uint8)])


# ---- the reference helper
def _column(rows=1000, seed=1):
    rng = np.random.default_rng(seed)
    return rng.integers(-50, 50, rows).astype(np.int64), rng.random(rows) >= 0.2, rng.random(rows) < 0.6


def test_the_reference_keeps_the_invariant_on_selected():
    vals, valid, sel = _column()
    rng = np.random.default_rng(2)
    for n_groups, hi in ((1, 1), (3, 3), (3, 5), (256, 300), (7, 2)):
        ids = rng.integers(0, hi, vals.size)
        w = G.reduce_grouped(S.T_I64, vals, valid, sel, ids, n_groups)
        assert sum(g.selected for g in w.groups) + w.out_of_range == w.selected == int(sel.sum())
        assert sum(g.count for g in w.groups) == int((sel & valid & (ids < n_groups)).sum())
        assert w.out_of_range == int((sel & (ids >= n_groups)).sum())
        whole = R.reduce_values(S.T_I64, vals, sel & valid & (ids < n_groups), 0)
        assert sum(R.join128(g.sum_lo, g.sum_hi) for g in w.groups) == R.join128(whole.sum_lo, whole.sum_hi)
        for g, gw in enumerate(w.groups):
            member = sel & (ids == g)
            live = member & valid
            assert (gw.selected, gw.count) == (int(member.sum()), int(live.sum()))
            if gw.count:
                assert gw.min_bytes == int(vals[live].min()).to_bytes(8, "little", signed=True)
                assert gw.max_bytes == int(vals[live].max()).to_bytes(8, "little", signed=True)
                assert R.join128(gw.sum_lo, gw.sum_hi) == int(vals[live].sum())


def test_the_reference_gives_empty_groups_zeros():
    vals, valid, sel = _column()
    ids = np.where(np.arange(vals.size) % 2 == 0, 0, 5)
    for ptype, v in ((S.T_I64, vals), (S.T_F64, vals.astype(np.float64))):
        w = G.reduce_grouped(ptype, v, valid, sel, ids, 8)
        for g in (1, 2, 3, 4, 6, 7):
            gw = w.groups[g]
            assert (gw.selected, gw.count, gw.nans, gw.sum_lo, gw.sum_hi) == (0, 0, 0, 0, 0)
            assert gw.min_bytes == gw.max_bytes == bytes(8)
        assert w.groups[0].count and w.groups[5].count and w.out_of_range == 0
    # a group whose selected rows are all null: selected counts them, count does not
    w = G.reduce_grouped(S.T_I64, vals, np.zeros(vals.size, bool), sel, ids, 8)
    assert w.groups[0].selected > 0 and w.groups[0].count == 0 and w.groups[0].min_bytes == bytes(8)
    # count only: no value is looked at
    w = G.reduce_grouped(S.T_BIN32, None, valid, sel, ids, 8, ops=("count",))
    assert w.groups[5].selected == int((sel & (ids == 5)).sum()) and w.groups[5].count == int((sel & valid & (ids == 5)).sum())


def test_the_reference_counts_ids_beyond_n_groups_and_ignores_unselected_ones():
    vals, valid, sel = _column()
    ids = np.random.default_rng(3).integers(0, 4, vals.size).astype(np.uint32)
    base = G.reduce_grouped(S.T_I64, vals, valid, sel, ids, 4)
    assert base.out_of_range == 0
    wild = ids.copy()
    wild[~sel] = 0xFFFFFFFF   # unselected rows: any bytes
    same = G.reduce_grouped(S.T_I64, vals, valid, sel, wild, 4)
    assert same.out_of_range == 0
    assert [(g.selected, g.count, g.sum_lo, g.min_bytes) for g in same.groups] == [(g.selected, g.count, g.sum_lo, g.min_bytes) for g in base.groups]
    marked = ids.copy()
    at = np.flatnonzero(sel)[::7]
    marked[at] = np.where(np.arange(at.size) % 2 == 0, 0xFFFFFFFF, 4)
    w = G.reduce_grouped(S.T_I64, vals, valid, sel, marked, 4)
    assert w.out_of_range == at.size and sum(g.selected for g in w.groups) == int(sel.sum()) - at.size
    for width, dtype in ((1, np.uint8), (2, np.uint16)):   # all-ones of a narrower id
        narrow = ids.astype(dtype)
        narrow[at] = np.iinfo(dtype).max
        assert G.reduce_grouped(S.T_I64, vals, valid, sel, narrow, 4).out_of_range == at.size


@pytest.mark.parametrize("n_groups", G.ORDER_TEST_GROUPS)
@pytest.mark.parametrize("ptype,dtype", [(S.T_F32, np.float32), (S.T_F64, np.float64)])
def test_the_float_order_inputs_are_inexact_and_any_order_stays_inside_the_bound(ptype, dtype, n_groups):
    """The inputs of the GPU order test.  Forward, reverse and shuffled numpy sums of a group all lie inside the bound of
    fsum -- and they are not all the same double, so the bound is not what makes the GPU test's bit comparison pass."""
    rows = 10_000
    v, ids = G.inexact_values(rows, n_groups, seed=17)
    v = v.astype(dtype)
    w = G.reduce_grouped(ptype, v, np.ones(rows, bool), np.ones(rows, bool), ids, n_groups)
    rng = np.random.default_rng(4)
    differing = 0
    for g, gw in enumerate(w.groups):
        x = v[ids == g].astype(np.float64)
        assert gw.count == x.size > 50 and gw.fsum == math.fsum(x.tolist())
        bound = R.float_sum_bound(gw)
        assert bound == gw.count * 2.0 ** -52 * math.fsum(np.abs(x).tolist())
        sums = []
        for order in (x, x[::-1], x[rng.permutation(x.size)]):
            s = 0.0
            for t in order.tolist():
                s += t
            assert abs(s - gw.fsum) <= bound, (g, s, gw.fsum, bound)
            sums.append(s)
        differing += len(set(sums)) > 1
        assert any(s != gw.fsum for s in sums), "group %d: the sum is exact in some order" % g
    # (with a hundred rows to a group three orders may agree by chance in a group or two)
    assert differing == n_groups if n_groups < 10 else differing >= 0.9 * n_groups
