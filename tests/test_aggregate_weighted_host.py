"""sb_aggregate_weighted without a GPU: the symbol is exported, the struct has the layout the header documents (through the
host compiler and ctypes), the Python layer refuses what needs no device before the context is touched, the reference
(tests/aggregate_weighted_ref.py) agrees with a dict-based group-by on small inputs, and wgt_mul128 (csrc/sb_common.h) --
the exact low 128 bits of a product of two 64-bit words of either signedness -- is compared with __int128 in a stand-alone
host program."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import warnings
from fractions import Fraction

import numpy as np
import pytest

from strawboat_amd import _native as N
from strawboat_amd.types import PhysicalType as P
from tests import aggregate_weighted_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")
CSRC = os.path.join(ROOT, "strawboat_amd", "csrc")

OFFSETS = dict(physical_type=0, is_nullable=4, pages=8, pages_len=16, metas=24, n_pages=32, page_offsets=40, selection=48,
               selection_capacity=56, group_ids=64, group_ids_capacity=72, group_id_width=80, n_groups=84, ops=88, flags=92,
               weights=96, weights_capacity=104, weights_validity=112, weights_validity_capacity=120, weight_type=128,
               reserved=132, groups=136, rows=144, selected=152, out_of_range=160)


def test_symbol_is_declared_and_exported():
    assert "sb_aggregate_weighted" in N.EXPORTS
    assert re.search(r"\bsb_aggregate_weighted\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_aggregate_weighted$", out, re.M)
    import strawboat_amd as sb
    assert sb.aggregate_weighted and sb.WeightedAggregateBatch and sb.group_by_weighted
    assert all(n in sb.__all__ for n in ("aggregate_weighted", "WeightedAggregateBatch", "group_by_weighted"))
    assert N.SB_WGT_SQUARE == 1


def test_the_structs_layout_through_the_host_compiler(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\ngroup %zu\\ngrouped %zu\\n", sizeof(sb_column_aggregate_weighted), sizeof(sb_agg_group), sizeof(sb_column_aggregate_grouped));\n'
                   '    printf("SQUARE %u\\nLARGE %u\\n", SB_WGT_SQUARE, SB_AGG_LARGE_MAX_GROUPS);\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_aggregate_weighted, %s));\n' % (f, f) for f in OFFSETS) +
                   "".join('    printf("g_%s %%zu\\n", offsetof(sb_column_aggregate_grouped, %s));\n' % (f, f) for f in list(OFFSETS)[:14]) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(N.ColumnAggregateWeightedC) == 168
    assert int(got["group"]) == C.sizeof(N.AggGroupC) == 64 and int(got["grouped"]) == 128   # (the grouped calls' struct is where it was)
    assert int(got["SQUARE"]) == N.SB_WGT_SQUARE == 1 and int(got["LARGE"]) == 1024
    assert [name for name, _ in N.ColumnAggregateWeightedC._fields_] == list(OFFSETS)
    for f, off in OFFSETS.items():
        assert int(got[f]) == off == getattr(N.ColumnAggregateWeightedC, f).offset, f
    for f in list(OFFSETS)[:14]:   # the first 92 bytes are sb_column_aggregate_grouped's
        assert int(got["g_" + f]) == OFFSETS[f] == getattr(N.ColumnAggregateGroupedC, f).offset, f
    assert getattr(N.ColumnAggregateWeightedC, "weight_type").size == 4 and getattr(N.ColumnAggregateWeightedC, "reserved").size == 4


EVERY = (P.INT8, P.INT16, P.INT32, P.INT64, P.UINT8, P.UINT16, P.UINT32, P.UINT64, P.FLOAT32, P.FLOAT64,
         P.BOOLEAN, P.INT128, P.INT256, P.BINARY, P.LARGE_BINARY, P.NULL)


def test_check_column():
    from strawboat_amd.aggregate_weighted import check_column
    CNT, SUM = N.SB_AGG_COUNT, N.SB_AGG_SUM
    for ptype in EVERY:   # count works on every type; the weight's type is checked all the same
        check_column(ptype, 33, 8, CNT, 1024, 2, 33, P.INT64, 33, None, False)
        check_column(ptype, 33, None, 0, 1, None, None, P.FLOAT32, 40, 8, False)
        with pytest.raises(ValueError):
            check_column(ptype, 33, 8, CNT, 4, 1, 33, P.BOOLEAN, 33, None, False)
    for ptype in EVERY[:10]:
        for wtype in EVERY[:10]:
            check_column(ptype, 33, 8, CNT | SUM, 257, 2, 33, wtype, 33, 8, False)
        check_column(ptype, 33, 8, CNT | SUM, 1, None, None, None, 0, None, True)   # square, ungrouped
    for ptype in EVERY[10:]:
        with pytest.raises(ValueError):
            check_column(ptype, 33, 8, SUM, 4, 1, 33, P.INT64, 33, None, False)
        with pytest.raises(ValueError):
            check_column(ptype, 33, 8, SUM, 4, 1, 33, None, 0, None, True)
    for ops in (N.SB_AGG_MIN, N.SB_AGG_MAX, 15, N.SB_AGG_MIN | CNT):   # min / max of a product are not offered
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, ops, 4, 1, 33, P.INT64, 33, None, False)
    for wtype in EVERY[10:] + (None, 99):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, SUM, 4, 1, 33, wtype, 33, None, False)
    with pytest.raises(ValueError):   # a short bitmap
        check_column(P.INT64, 33, 4, SUM, 4, 1, 33, P.INT64, 33, None, False)
    with pytest.raises(ValueError):   # fewer weights than rows
        check_column(P.INT64, 33, 8, SUM, 4, 1, 33, P.INT64, 32, None, False)
    with pytest.raises(ValueError):   # a short weights validity
        check_column(P.INT64, 33, 8, SUM, 4, 1, 33, P.INT64, 33, 4, False)
    with pytest.raises(ValueError):   # fewer ids than rows
        check_column(P.INT64, 33, 8, SUM, 4, 1, 32, P.INT64, 33, None, False)
    for width in (None, 0, 3, 8):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, SUM, 4, width, 33, P.INT64, 33, None, False)
    for bad in (0, 1025, -1, 1 << 20, 2.0, None, True):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, SUM, bad, 2, 33, P.INT64, 33, None, False)
    for ng in (2, 1024):   # without ids every row is in group 0
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, SUM, ng, None, None, P.INT64, 33, None, False)
    check_column(P.INT64, 0, None, SUM, 1024, 1, 0, P.FLOAT64, 0, None, False)


def test_bad_arguments_raise_before_the_context_is_touched():
    import torch
    from strawboat_amd import aggregate_weighted, group_by_weighted
    from strawboat_amd.read import ColumnPages

    class Ctx:   # (only asked where its tensors live: any other attribute is an AttributeError)
        torch_device = torch.device("cpu")

    metas = np.array([[100, 40]], np.uint64)
    col = ColumnPages(P.INT64, False, torch.zeros(100, dtype=torch.uint8), metas)
    ids = torch.zeros(40, dtype=torch.uint16)
    bm = torch.zeros(8, dtype=torch.uint8)
    w = torch.zeros(40, dtype=torch.int64)
    wv = torch.zeros(8, dtype=torch.uint8)

    def refused(*a, **k):
        with pytest.raises(ValueError):
            aggregate_weighted(Ctx(), *a, **k)

    refused([col], [w], ids, 1024, torch.zeros(4, dtype=torch.uint8))            # a bitmap of 4 bytes for 40 rows
    for n_groups in (0, 1025, -3, True, 300.0):
        refused([col], [w], ids, n_groups, bm)
    refused([col], [w], None, 2, bm)                                               # the ungrouped form has one group
    for bad in (torch.zeros(40, dtype=torch.int64), torch.zeros(40, dtype=torch.float32), torch.zeros(39, dtype=torch.uint16),
                torch.zeros(80, dtype=torch.uint16)[::2], torch.zeros(40, dtype=torch.uint16, device="meta"), np.zeros(40, np.uint16)):
        refused([col], [w], bad, 1024, bm)
    for bad in (torch.zeros(39, dtype=torch.int64), torch.zeros(80, dtype=torch.int64)[::2], torch.zeros((40, 1), dtype=torch.int64),
                torch.zeros(40, dtype=torch.bool), torch.zeros(40, dtype=torch.float16), torch.zeros(40, dtype=torch.int64, device="meta"),
                np.zeros(40, np.int64), None, (w,), (w, wv, wv)):
        refused([col], [bad], ids, 1024, bm)
    for bad in (torch.zeros(4, dtype=torch.uint8), torch.zeros(8, dtype=torch.int8), torch.zeros(16, dtype=torch.uint8)[::2],
                torch.zeros(8, dtype=torch.uint8, device="meta"), np.zeros(8, np.uint8)):
        refused([col], [(w, bad)], ids, 1024, bm)
    refused([col], w, ids, 1024, bm)             # one weights entry per column: a list
    refused([col], None, ids, 1024, bm)
    refused([col, col], [w], ids, 1024, bm)
    refused([col], [w], ids, 1024, bm, square=True)   # square takes no weights
    for ops in (("min",), ("count", "max"), ("count", "avg"), 15):
        refused([col], [w], ids, 1024, bm, ops=ops)
    for ptype in (P.BOOLEAN, P.BINARY, P.INT128, P.INT256, P.LARGE_BINARY, P.NULL):   # SUM on a type that has none
        other = ColumnPages(ptype, False, col.pages, metas)
        refused([other], [w], ids, 1024, bm)
        refused([other], None, ids, 1024, bm, square=True)
    refused([col, col], [w, w], ids, 1024, [bm])
    refused([col, col], [w, w], [ids], 1024, bm)
    refused([col, col], [w, w], ids, [1024], bm)
    with pytest.raises(TypeError):    # not a bitmap
        aggregate_weighted(Ctx(), [col], [w], ids, 1024, [np.zeros(8, np.uint8)])
    # group_by_weighted: the key's type, max_keys and the weights, before a key call is made
    for ptype in (P.FLOAT32, P.FLOAT64, P.BOOLEAN, P.INT128, P.NULL):
        with pytest.raises(ValueError):
            group_by_weighted(Ctx(), ColumnPages(ptype, False, col.pages, metas), [col], [w])
    for mk in (0, 1025, -1, True, 2.5, None):
        with pytest.raises(ValueError):
            group_by_weighted(Ctx(), col, [col], [w], max_keys=mk)
    for bad in ([torch.zeros(39, dtype=torch.int64)], [w, w], None, [torch.zeros(40, dtype=torch.bool)]):
        with pytest.raises(ValueError):
            group_by_weighted(Ctx(), col, [col], bad)
    with pytest.raises(ValueError):
        group_by_weighted(Ctx(), col, [col], [w], square=True)
    with pytest.raises(ValueError):
        group_by_weighted(Ctx(), col, [ColumnPages(P.BINARY, False, col.pages, metas)], None, square=True)


# ---- the reference against a dict-based group-by
def _dict_reference(y, yv, w, wv, ids, n_groups, mask):
    groups = {}
    oor = 0
    for i in range(len(y)):
        if not mask[i]:
            continue
        if not 0 <= ids[i] < n_groups:
            oor += 1
            continue
        g = groups.setdefault(int(ids[i]), dict(selected=0, terms=[]))
        g["selected"] += 1
        if yv[i] and wv[i]:
            g["terms"].append((y[i].item(), w[i].item()))
    return groups, oor


@pytest.mark.parametrize("ydt,wdt", [(np.int8, np.int64), (np.uint64, np.uint64), (np.int64, np.uint16), (np.int32, np.float64),
                                     (np.float32, np.float32), (np.float64, np.int16), (np.uint8, np.float32)])
def test_the_reference_against_a_dict_based_group_by(ydt, wdt):
    rng = np.random.default_rng(5)
    rows, n_groups = 300, 7

    def values(dt):
        if np.dtype(dt).kind == "f":
            return (rng.normal(0, 1000, rows) * rng.choice([1e-6, 1.0, 1e6], rows)).astype(dt)
        info = np.iinfo(dt)
        v = rng.integers(info.min, info.max, rows, dtype=dt, endpoint=True)
        v[:4] = [info.min, info.max, info.max, info.min]
        return v

    y, w = values(ydt), values(wdt)
    yv, wv = rng.random(rows) >= 0.2, rng.random(rows) >= 0.2
    ids = rng.integers(0, n_groups + 2, rows)
    ids[:4] = 3
    mask = rng.random(rows) < 0.7
    mask[:4] = yv[:4] = wv[:4] = True
    got = W.reduce(y, yv, w, wv, ids, n_groups, mask)
    groups, oor = _dict_reference(y, yv, w, wv, ids, n_groups, mask)
    assert (got.rows, got.selected, got.out_of_range) == (rows, int(mask.sum()), oor) and oor > 0
    flt = W.is_float_mode(ydt, wdt)
    for g in range(n_groups):
        d = groups.get(g, dict(selected=0, terms=[]))
        gw = got.groups[g]
        assert (gw.selected, gw.count) == (d["selected"], len(d["terms"]))
        if not flt:
            assert gw.kind == "int" and gw.int_sum == sum(a * b for a, b in d["terms"]) % (1 << 128)
        else:
            assert gw.kind == "finite" and gw.nans == 0
            assert gw.exact == sum((Fraction(a) * Fraction(b) for a, b in d["terms"]), Fraction(0))
            f = math.fsum(float(a) * float(b) for a, b in d["terms"])   # a float sum of rounded products lies within the bound
            assert abs(Fraction(f) - gw.exact) <= gw.bound
    # square: w is y; the ungrouped form: one group; no selection: every row
    sq = W.reduce(y, yv, None, None, None, 1, None)
    terms = [(v.item(), v.item()) for v, ok in zip(y, yv) if ok]
    assert (sq.selected, sq.out_of_range, sq.groups[0].selected, sq.groups[0].count) == (rows, 0, rows, len(terms))
    if flt and np.dtype(ydt).kind != "f":
        assert sq.groups[0].kind == "int"   # (an integer y squared is exact whatever w was)
    if sq.groups[0].kind == "int":
        assert sq.groups[0].int_sum == sum(a * b for a, b in terms) % (1 << 128)
    else:
        assert sq.groups[0].exact == sum((Fraction(a) * Fraction(b) for a, b in terms), Fraction(0))
    # count only: no sum whatever the types
    co = W.reduce(y, yv, w, wv, ids, n_groups, mask, sum_=False)
    assert all(g.kind == "none" and g.count == got.groups[i].count for i, g in enumerate(co.groups))


def test_the_reference_classifies_specials():
    y = np.array([np.nan, 0.0, np.inf, np.inf, np.inf, 1.0, -0.0, 2.0], np.float64)
    w = np.array([0.0, 1.0, 0.0, -1.0, 1.0, np.inf, 5.0, 3.0], np.float64)
    ids = np.array([0, 0, 1, 2, 2, 3, 4, 4])
    got = W.reduce(y, None, w, None, ids, 6, None)
    assert [g.kind for g in got.groups] == ["nan", "nan", "nan", "+inf", "finite", "finite"]
    assert [g.nans for g in got.groups] == [1, 1, 0, 0, 0, 0]
    assert got.groups[4].exact == 6 and got.groups[5].count == 0
    got = W.reduce(np.array([1, -1], np.int64), None, np.array([-np.inf, np.inf]), None, None, 1, None)
    assert got.groups[0].kind == "-inf"


# ---- wgt_mul128 in a host program of its own
PROGRAM = r"""
#include <cstdio>
#include <cstdint>
#include <vector>
#include "sb_common.h"

static int fails = 0;
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}
typedef unsigned __int128 u128;
typedef __int128 i128;
// x, y: 64-bit words as the kernels hold them, extended by their own signedness
static void check(uint64_t x, bool xs, uint64_t y, bool ys) {
    uint64_t lo = 1, hi = 1;
    sb::wgt_mul128(x, xs, y, ys, lo, hi);
    const u128 a = xs ? (u128)(i128)(int64_t)x : (u128)x;   // the operand as a 128-bit two's-complement number
    const u128 b = ys ? (u128)(i128)(int64_t)y : (u128)y;
    const u128 want = a * b;                                 // (unsigned: wraps mod 2^128, no overflow to report)
    if ((lo != (uint64_t)want || hi != (uint64_t)(want >> 64)) && fails++ < 10)
        printf("%016llx (%d) * %016llx (%d): %016llx%016llx, want %016llx%016llx\n", (unsigned long long)x, xs, (unsigned long long)y, ys,
               (unsigned long long)hi, (unsigned long long)lo, (unsigned long long)(want >> 64), (unsigned long long)want);
    if (!xs && !ys && sb::wgt_umulhi(x, y) != (uint64_t)(((u128)x * y) >> 64)) fails++, printf("umulhi\n");
}
int main() {
    // the extremes of all eight integer types (as 64-bit words of their own signedness), 0, +-1
    const int64_t sv[] = {INT8_MIN, INT8_MAX, INT16_MIN, INT16_MAX, INT32_MIN, INT32_MAX, INT64_MIN, INT64_MAX, 0, 1, -1};
    const uint64_t uv[] = {0, UINT8_MAX, UINT16_MAX, UINT32_MAX, UINT64_MAX, 1, (uint64_t)INT64_MAX, (uint64_t)INT64_MAX + 1};
    std::vector<std::pair<uint64_t, bool>> ops;
    for (int64_t v : sv) ops.push_back({(uint64_t)v, true});
    for (uint64_t v : uv) ops.push_back({v, false});
    for (auto& a : ops)
        for (auto& b : ops) check(a.first, a.second, b.first, b.second);   // all four signedness pairings among them
    check((uint64_t)INT64_MIN, true, (uint64_t)INT64_MIN, true);
    check(UINT64_MAX, false, UINT64_MAX, false);
    check((uint64_t)INT64_MIN, true, UINT64_MAX, false);
    check(UINT64_MAX, false, (uint64_t)INT64_MIN, true);
    for (int i = 0; i < 10000; i++) {
        uint64_t x = rnd(), y = rnd();
        const uint64_t m = rnd();
        if (m & 1) x >>= (m >> 8) & 63;     // (magnitudes of every size)
        if (m & 2) y >>= (m >> 16) & 63;
        if (m & 4) x = 0 - x;
        if (m & 8) y = 0 - y;
        check(x, (m >> 4) & 1, y, (m >> 5) & 1);
    }
    // four rows of INT64_MIN * INT64_MIN (2^126 each) wrap to 0 mod 2^128
    uint64_t lo, hi, s0 = 0, s1 = 0;
    for (int i = 0; i < 4; i++) {
        sb::wgt_mul128((uint64_t)INT64_MIN, true, (uint64_t)INT64_MIN, true, lo, hi);
        const uint64_t old = s0;
        s0 += lo, s1 += hi + (s0 < old ? 1 : 0);
    }
    if (s0 || s1) fails++, printf("4 * 2^126\n");
    printf("fails %d\n", fails);
    return fails ? 1 : 0;
}
"""


def test_wgt_mul128_against_int128(tmp_path):
    """a stand-alone host program (its own main, address and undefined-behaviour sanitizers where the compiler has them)"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    src = tmp_path / "mul128.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "mul128"
    base = [hipcc, "--offload-host-only", "-std=c++17", "-O1", "-g", "-I", CSRC, "-o", str(exe), str(src)]
    rt = subprocess.run([hipcc, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if os.path.isabs(rt) and os.path.exists(rt):
        san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        assert san.returncode == 0, "the sanitized build failed though %s exists:\n%s" % (rt, san.stderr)
        syms = subprocess.run(["nm", "-D", str(exe)], capture_output=True, text=True).stdout + \
            subprocess.run(["nm", str(exe)], capture_output=True, text=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms, "the program was built without the sanitizers"
    else:
        warnings.warn("hipcc has no sanitizer runtime (%r): wgt_mul128 is compared WITHOUT the sanitizers" % rt)
        subprocess.run(base, check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("fails 0"), run.stdout + run.stderr
