"""sb_filter_columns_cmp without a GPU: the symbol is declared, listed and defined, the ctypes struct has the header's layout,
the Python layer refuses what needs no device before a context is touched, the reference that
tests/test_gpu_filter_cmp.py compares the device with (tests/filter_cmp_ref.py) agrees with a plain Python loop over every
op x every one of the 100 type pairs on the edge values, over nulls and over the three combine modes, the comparison the
kernels run (cmp_rel / cmp_pair, csrc/sb_common.h) agrees with that loop in a stand-alone host program, and every column of
tests/filter_cmp_cases.py carries its codec on every page."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from oracle import sbo as S
from strawboat_amd import _native as N
from strawboat_amd.filter_cmp import FilterCmpBatch, check_column, filter_columns_cmp, filter_pair
from strawboat_amd.types import PhysicalType as P
from tests import filter_cmp_cases as Cc
from tests import filter_cmp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")
CSRC = os.path.join(ROOT, "strawboat_amd", "csrc")

OFFSETS = dict(physical_type=0, is_nullable=4, pages=8, pages_len=16, metas=24, n_pages=32, page_offsets=40, op=48, combine=52,
               other=56, other_capacity=64, other_validity=72, other_validity_capacity=80, other_type=88, flags=92, reserved=96,
               selection=104, selection_capacity=112, rows=120, selected=128)


def test_symbol_is_declared_listed_and_defined():
    import strawboat_amd as sb
    assert "sb_filter_columns_cmp" in N.EXPORTS
    assert sb.filter_columns_cmp is filter_columns_cmp and sb.FilterCmpBatch is FilterCmpBatch and sb.filter_pair is filter_pair
    assert {"filter_columns_cmp", "FilterCmpBatch", "filter_pair"} <= set(sb.__all__)
    assert re.search(r"\bsb_filter_columns_cmp\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_filter_columns_cmp$", out, re.M)


def test_ctypes_struct_has_the_headers_layout(tmp_path):
    assert C.sizeof(N.ColumnFilterCmpC) == 136
    assert [name for name, _ in N.ColumnFilterCmpC._fields_] == list(OFFSETS)
    for f, off in OFFSETS.items():
        assert getattr(N.ColumnFilterCmpC, f).offset == off, f
    # the first 56 bytes are sb_column_filter's
    for f in list(OFFSETS)[:9]:
        assert getattr(N.ColumnFilterC, f).offset == OFFSETS[f], f
    assert N.ColumnFilterC.literal.offset == 56
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(sb_column_filter_cmp));\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_filter_cmp, %s));\n' % (f, f) for f in OFFSETS) +
                   "".join('    printf("flt_%s %%zu\\n", offsetof(sb_column_filter, %s));\n' % (f, f) for f in list(OFFSETS)[:9]) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == 136
    for f, off in OFFSETS.items():
        assert int(got[f]) == off, f
    for f in list(OFFSETS)[:9]:
        assert int(got["flt_" + f]) == OFFSETS[f], f
    # ... and the offsets the header's comment pins
    text = open(HEADER).read().split("Layout (pinned by tests/test_filter_cmp_host.py)")[1].split("*/")[0]
    assert "sb_column_filter_cmp 136 bytes;" in text
    pinned = dict(re.findall(r"(\w+) (\d+)[,.]", text.split("sb_column_filter_cmp 136 bytes;")[1]))
    assert {f: int(v) for f, v in pinned.items()} == OFFSETS


# ---- the Python layer
def test_check_column_refuses_what_needs_no_device():
    check_column(P.INT32, 33, "lt", P.INT64, 33 * 8, 8)
    check_column(P.FLOAT64, 0, "ne", P.UINT8, 0, None)
    for op in ("is_null", "is_not_null", "starts_with", "in", "", None, 2):
        with pytest.raises(ValueError):
            check_column(P.INT32, 33, op, P.INT32, 33 * 4, None)
    for t in (P.BOOLEAN, P.INT128, P.INT256, P.BINARY, P.LARGE_BINARY, P.NULL, None, 99):
        with pytest.raises(ValueError):
            check_column(t, 33, "eq", P.INT32, 33 * 4, None)
        with pytest.raises(ValueError):
            check_column(P.INT32, 33, "eq", t, 33 * 4, None)
    with pytest.raises(ValueError):   # a short operand
        check_column(P.INT32, 33, "eq", P.INT64, 33 * 8 - 1, None)
    with pytest.raises(ValueError):   # a short validity: 33 rows need 8 bytes
        check_column(P.INT32, 33, "eq", P.INT64, 33 * 8, 4)


def test_bad_arguments_raise_before_the_context_is_touched():
    import torch
    from strawboat_amd.filter import Selection
    from strawboat_amd.read import ColumnPages, DeviceArray

    class Ctx:   # (only asked where its tensors live: any other attribute is an AttributeError)
        torch_device = torch.device("cpu")

    metas = np.array([[100, 40]], np.uint64)
    col = ColumnPages(P.INT64, False, torch.zeros(100, dtype=torch.uint8), metas)
    o = torch.zeros(40, dtype=torch.int32)
    ov = torch.zeros(8, dtype=torch.uint8)
    sel = Selection(torch.zeros(8, dtype=torch.uint8), 40, None)

    def refused(*a, **k):
        with pytest.raises(ValueError):
            filter_columns_cmp(Ctx(), *a, **k)

    for op in ("is_null", "starts_with", "in", None, 3):
        refused([col], [op], [o])
    refused([col], ["lt", "gt"], [o])                 # one op per column
    refused([col, col], "lt", [o])                    # one operand per column
    refused([col], "lt", o)                           # ... a list
    refused([col], "lt", None)
    for bad in (torch.zeros(39, dtype=torch.int32), torch.zeros(80, dtype=torch.int32)[::2], torch.zeros((40, 1), dtype=torch.int32),
                torch.zeros(40, dtype=torch.bool), torch.zeros(40, dtype=torch.float16), torch.zeros(40, dtype=torch.int32, device="meta"),
                np.zeros(40, np.int32), None, (o,), (o, ov, ov)):
        refused([col], "lt", [bad])
    for bad in (torch.zeros(4, dtype=torch.uint8), torch.zeros(8, dtype=torch.int8), torch.zeros(16, dtype=torch.uint8)[::2],
                torch.zeros(8, dtype=torch.uint8, device="meta"), np.zeros(8, np.uint8)):
        refused([col], "lt", [(o, bad)])
        refused([col], "lt", [o], other_validities=[bad])
    refused([col], "lt", [(o, ov)], other_validities=[ov])       # the validity twice
    refused([col], "lt", [o], other_types=[P.INT64])              # 160 bytes are not 40 values of 8
    refused([col], "lt", [o], other_types=[P.BINARY])
    refused([col], "lt", [o], other_types=[P.INT32, P.INT32])
    refused([col], "lt", [o], combine="xor")
    refused([col], "lt", [o], combine="and")                      # nothing to combine with
    refused([col], "lt", [o], combine="or", selection=[sel, sel])
    refused([col], "lt", [o], combine="and", selection=[Selection(torch.zeros(8, dtype=torch.uint8), 39, None)])
    for ptype in (P.BOOLEAN, P.BINARY, P.INT128, P.INT256, P.LARGE_BINARY, P.NULL):
        refused([ColumnPages(ptype, False, col.pages, metas)], "lt", [o])
    da = DeviceArray(P.BINARY, False, 40, torch.zeros(40, dtype=torch.uint8), None, None, None)
    refused([col], "lt", [da])
    da = DeviceArray(P.INT32, False, 40, torch.zeros(160, dtype=torch.uint8), None, None, None)
    refused([col], "lt", [da], other_types=[P.INT64])            # the DeviceArray says what it is
    refused([col], "lt", [da], other_validities=[ov])
    # filter_pair: the rows of both sides, the types, the combine mode
    right = ColumnPages(P.INT32, True, torch.zeros(100, dtype=torch.uint8), np.array([[100, 39]], np.uint64))
    for a, k in ((("lt", right), {}), (("like", col), {}), (("lt", ColumnPages(P.BINARY, False, col.pages, metas)), {}),
                 (("lt", col), dict(combine="and")), (("lt", col), dict(combine="nand"))):
        with pytest.raises(ValueError):
            filter_pair(Ctx(), col, *a, **k)


# ---- the reference against a plain Python loop
def loop_relation(y, yt, o, ot):
    """0 less, 1 equal, 2 greater, 3 unordered: integers as Python ints, a pair with a float as Python floats (a Python int
    becomes a float by rounding to nearest even, a float32 exactly)"""
    y_int, o_int = np.dtype(Cc.NP[yt]).kind in "iu", np.dtype(Cc.NP[ot]).kind in "iu"
    if y_int and o_int:
        a, b = int(y), int(o)
    else:
        a, b = float(int(y) if y_int else y), float(int(o) if o_int else o)
        if math.isnan(a) or math.isnan(b):
            return 3
    return 0 if a < b else 1 if a == b else 2


MASK = {"eq": {1}, "ne": {0, 2, 3}, "lt": {0}, "le": {0, 1}, "gt": {2}, "ge": {1, 2}}


def loop_bits(y, yt, y_valid, o, ot, o_valid, op):
    out = []
    for i in range(len(y)):
        live = (y_valid is None or bool(y_valid[i])) and (o_valid is None or bool(o_valid[i]))
        out.append(live and loop_relation(y[i], yt, o[i], ot) in MASK[op])
    return np.array(out, bool)


@pytest.mark.parametrize("yt", Cc.TYPES, ids=[Cc.TYPE_NAME[t] for t in Cc.TYPES])
def test_reference_agrees_with_a_python_loop_on_the_edge_values_of_every_pair(yt):
    for ot in Cc.TYPES:
        y, o = Cc.edge_pair_values(yt, ot)
        assert y.size == Cc.edge_values(yt).size * Cc.edge_values(ot).size > 0
        hits = {}
        for op in R.OPS:
            got = R.compare(y, o, op)
            want = loop_bits(y, yt, None, o, ot, None, op)
            assert np.array_equal(got, want), (Cc.TYPE_NAME[yt], Cc.TYPE_NAME[ot], op, int(np.argmax(got != want)))
            hits[op] = int(got.sum())
        assert hits["eq"] and hits["lt"] and hits["gt"], hits   # (no pair whose table decides nothing)


def test_the_edge_tables_hold_what_the_issue_names():
    e = {t: set(Cc.edge_values(t).tolist()) for t in Cc.TYPES if np.dtype(Cc.NP[t]).kind in "iu"}
    for t, vals in e.items():
        info = np.iinfo(Cc.NP[t])
        assert int(info.min) in vals and int(info.max) in vals
    assert -1 in e[S.T_I64] and 2 ** 64 - 1 in e[S.T_U64] and 2 ** 63 in e[S.T_U64] and 2 ** 63 - 1 in e[S.T_I64]
    assert {2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1} <= e[S.T_I64] and {2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1} <= e[S.T_U64]
    for t in (S.T_F32, S.T_F64):
        f = Cc.edge_values(t)
        assert np.isnan(f).sum() >= 2 and np.isposinf(f).any() and np.isneginf(f).any()
        zeros = f[f == 0]
        assert np.signbit(zeros).any() and (~np.signbit(zeros)).any()
    # the rules by hand
    one = lambda y, yt, o, ot, op: bool(R.compare(np.array([y], Cc.NP[yt]), np.array([o], Cc.NP[ot]), op)[0])
    assert one(-1, S.T_I64, 2 ** 64 - 1, S.T_U64, "lt") and not one(-1, S.T_I64, 2 ** 64 - 1, S.T_U64, "eq")
    assert one(-1, S.T_I8, 255, S.T_U8, "lt") and one(255, S.T_U8, -1, S.T_I8, "gt")
    assert one(2 ** 63, S.T_U64, 2 ** 63 - 1, S.T_I64, "gt")
    assert one(2 ** 53 + 1, S.T_I64, 2.0 ** 53, S.T_F64, "eq")          # compared after rounding
    assert one(2 ** 53 + 1, S.T_I64, 2 ** 53, S.T_U64, "gt")             # exactly
    assert one(2 ** 64 - 1, S.T_U64, 2.0 ** 64, S.T_F32, "eq")
    assert one(-0.0, S.T_F32, 0.0, S.T_F64, "eq") and one(-np.inf, S.T_F64, np.inf, S.T_F32, "lt")
    for op in R.OPS:
        assert one(np.nan, S.T_F64, 1, S.T_I32, op) == (op == "ne") and one(1, S.T_I32, np.nan, S.T_F32, op) == (op == "ne")


def test_reference_nulls_and_combine_modes_agree_with_the_loop():
    rng = np.random.default_rng(5)
    for rows in (1, 31, 32, 33, 64, 100):
        y = rng.integers(-3, 3, rows).astype(np.int16)
        o = rng.integers(-3, 3, rows).astype(np.float32)
        o[rng.random(rows) < 0.2] = np.nan
        for y_valid in (None, rng.random(rows) < 0.7):
            for o_valid in (None, rng.random(rows) < 0.7):
                for op in R.OPS:
                    bits = R.result_bits(y, y_valid, o, o_valid, op)
                    want = loop_bits(y, S.T_I16, y_valid, o, S.T_F32, o_valid, op)
                    assert np.array_equal(bits, want)
                    if op == "ne":   # a null row satisfies nothing, NE included
                        for v in (y_valid, o_valid):
                            assert v is None or not bits[~v].any()
                    nwords = (rows + 31) // 32
                    prev = rng.integers(0, 1 << 32, nwords, dtype=np.uint64).astype(np.uint32)
                    for combine in R.COMBINES:
                        words, selected = R.want(y, y_valid, o, o_valid, op, combine, prev)
                        # the loop: bit by bit over all 32 * nwords positions
                        exp = []
                        for pos in range(nwords * 32):
                            old = bool((int(prev[pos // 32]) >> (pos % 32)) & 1)
                            if pos >= rows:
                                exp.append(False if combine == "set" else old)
                            elif combine == "set":
                                exp.append(bool(want[pos]))
                            elif combine == "and":
                                exp.append(old and bool(want[pos]))
                            else:
                                exp.append(old or bool(want[pos]))
                        got = [bool((int(words[pos // 32]) >> (pos % 32)) & 1) for pos in range(nwords * 32)]
                        assert got == exp, (rows, op, combine)
                        assert selected == sum(exp[:rows])


# ---- the kernels' comparison in a host program of its own.  Input: lines "<ykind> <yw> <y hex> <okind> <ow> <o hex>"; output: the
# relation cmp_pair / cmp_rel give, one per line.
PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include "sb_common.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    unsigned yk, yw, ok, ow;
    unsigned long long y, o;
    while (fscanf(f, " %u %u %llx %u %u %llx", &yk, &yw, &y, &ok, &ow, &o) == 6) {
        uint32_t rel = 9;
        sb::cmp_pair(yk, ok, [&](auto a, auto b) { rel = sb::cmp_rel<decltype(a)::value, decltype(b)::value>(yw, (uint64_t)y, ow, (uint64_t)o); });
        printf("%u\n", rel);
    }
    fclose(f);
    return 0;
}
"""
KIND = {"u": 0, "i": 1}   # FK_UNSIGNED, FK_SIGNED; FK_F32 2, FK_F64 3


def _kind(t):
    dt = np.dtype(Cc.NP[t])
    return KIND[dt.kind] if dt.kind in "iu" else (2 if dt.itemsize == 4 else 3)


def test_cmp_rel_agrees_with_the_loop_in_a_host_program(tmp_path):
    """a stand-alone host program (its own main, address and undefined-behaviour sanitizers where the compiler has them)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    src = tmp_path / "cmp_rel.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "cmp_rel"
    base = [hipcc, "--offload-host-only", "-std=c++17", "-O1", "-g", "-I", CSRC, "-o", str(exe), str(src)]
    rt = subprocess.run([hipcc, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if os.path.isabs(rt) and os.path.exists(rt):
        san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        assert san.returncode == 0, "the sanitized build failed though %s exists:\n%s" % (rt, san.stderr)
    else:
        warnings.warn("hipcc has no sanitizer runtime (%r): cmp_rel is compared WITHOUT the sanitizers" % rt)
        subprocess.run(base, check=True)
    lines, want = [], []
    for yt in Cc.TYPES:
        for ot in Cc.TYPES:
            y, o = Cc.edge_pair_values(yt, ot)
            yw, ow = y.dtype.itemsize, o.dtype.itemsize
            yr, orr = y.view("<u%d" % yw), o.view("<u%d" % ow)
            for i in range(y.size):
                # (the words as flt_load gives them: zero-extended)
                lines.append("%u %u %x %u %u %x" % (_kind(yt), yw, int(yr[i]), _kind(ot), ow, int(orr[i])))
                want.append(loop_relation(y[i], yt, o[i], ot))
    inp = tmp_path / "pairs.txt"
    inp.write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    got = [int(x) for x in run.stdout.split()]
    assert len(got) == len(want)
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "%d relations differ, the first: %s -> %d, want %d" % (len(bad), lines[bad[0]], got[bad[0]], want[bad[0]])


# ---- the table of columns
@pytest.mark.parametrize("name", [n for n in Cc.ALL if n != "rle_long"])
def test_every_page_of_a_case_carries_its_codec(name):
    b = Cc.build(name)
    assert b.metas.shape[0] >= 1 and Cc.codecs_seen(b) == {Cc.codec_of(name)}, name
    assert b.ref.vals[:b.rows].size == b.rows == int(b.metas[:, 1].sum())


def test_the_shapes_the_cases_promise():
    from strawboat_amd import stat
    for n in Cc.ROW_COUNTS:
        for c in ("none", "rle", "dict"):
            assert Cc.build("rows_%d_%s" % (n, c)).rows == n
    for c in ("none", "rle", "dict", "lz4"):   # several pages, none a multiple of 32 rows but perhaps the last
        m = Cc.build("seams_" + c).metas
        assert m.shape[0] > 5 and all(int(x) % 32 for x in m[:-1, 1])
    for D in (Cc.FILTER_DICT_BITS, Cc.FILTER_DICT_BITS + 1):
        b = Cc.build("dict_%d" % D)
        assert b.metas.shape[0] == 1 and stat.stat_page(b.pages, b.col["ptype"], b.col["nullable"]).body.unique_num == D
    # RLE pages of more runs than one chunk of the walk (RLE_CHUNK = 1024 run records of 4 + w bytes)
    for name, w in (("rle_hand_u8", 1), ("rle_hand_i16", 2), ("rle_hand_i32", 4), ("rle_hand_i64", 8)):
        b = Cc.build(name)
        assert max(int(x) for x in b.metas[:, 0]) // (4 + w) > 1024, name
    for yt, ot in Cc.PAIRS:
        for codec in (S.NONE, S.RLE, S.DICT):
            b, other = Cc.build_edge_pair(yt, ot, codec)
            assert b.rows == other.size and Cc.codecs_seen(b) == {codec} and b.metas.shape[0] > 1
            # the oracle gives the table back (a codec may not keep what a null row's slot held, nor the sign of a zero in a
            # run or a dictionary: the GPU file compares with the oracle's decode, whatever it is)
            assert np.array_equal(b.ref.vals[:b.rows][b.ref.valid], Cc.edge_pair_values(yt, ot)[0][b.ref.valid], equal_nan=np.dtype(Cc.NP[yt]).kind == "f")
            assert b.ref.valid.sum() == b.rows - (b.rows + 1) // 5
        b, other = Cc.build_random_pair(yt, ot, S.NONE)
        eq = R.compare(b.ref.vals[:b.rows], other, "eq")
        assert 0.4 < eq.mean() < 0.6, (yt, ot, eq.mean())
