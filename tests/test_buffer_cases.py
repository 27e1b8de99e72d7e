"""The case table of tests/test_gpu_buffers.py without a GPU: every case is written and read back by the oracle (none is
skipped, no exception is caught), forced codecs show on every page, the ladder variants have the string lengths they claim,
scatter / gather / place are inverses, and the span check of a read call's host tables (csrc/sb_span.h) is run by a small
C++ program at the offsets and lengths where a sum would wrap."""
import os
import shutil
import subprocess

import numpy as np

from oracle import sbo as S
from tests import buffer_cases as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "strawboat_amd", "csrc")


def all_cases():
    for g in B.groups():
        yield from B.table(*g)
    for g in B.ladder_groups():
        yield from B.ladder_table(*g)


def test_every_case_is_written_and_read_back_by_the_oracle():
    n = forced = 0
    names = set()
    for case in all_cases():
        pages, metas, want = B.pages_of(case)   # (raises: a case the oracle refuses fails the test)
        col = case.col
        assert want["rows"] == col["rows"] == int(metas[:, 1].sum()), case
        assert int(metas[:, 0].sum()) == pages.size, case
        mps = case.opt["max_page_size"]
        assert metas.shape[0] == (1 if mps is None else -(-col["rows"] // mps)), case
        if case.forced is not None:
            seen = set(S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
            assert seen == {case.forced}, (case, seen)
            forced += 1
        names.add(case.name)
        n += 1
    assert len(names) == n, "case names are unique"
    print("%d cases written and read back, 0 skipped, %d with a forced codec" % (n, forced))
    assert n > 5000 and forced > 2500


def test_the_table_states_the_issues_rule():
    by = {B.group_id(g) for g in B.groups()}
    for t in B.TYPES:
        for o in ("adaptive", "ratio1.5", "lz4", "zstd", "snappy"):
            assert "%s-%s" % (B.TYPE_NAMES[t], o) in by
    assert "bin-rle" not in by and "lbin-rle" not in by and "bool-rle" in by
    for o in ("dict", "dict_rle", "freq"):
        assert "bool-" + o not in by and "bin-" + o in by and "i256-" + o in by
    assert {g for g in by if g.endswith("-onevalue")} == {B.TYPE_NAMES[t] + "-onevalue" for t in B.PRIMS}
    for o in ("bitpack", "deltabp"):
        assert {g for g in by if g.endswith("-" + o)} == {"i32-" + o, "u32-" + o}
        for case in B.table(S.T_I32, B.OPTION_SET[o]):
            assert case.col["rows"] % 128 == 0 and (case.opt["max_page_size"] or 0) % 128 == 0
    assert {g for g in by if g.endswith("-patas")} == {"f64-patas"}
    for case in B.table(S.T_I64, B.OPTION_SET["onevalue"]):
        assert not case.col["values"].any()
    rows = {c.col["rows"] for c in B.table(S.T_I8, B.OPTION_SET["adaptive"])}
    assert rows == set(B.ROWS)
    pages = {(c.col["rows"], c.opt["max_page_size"]) for c in B.table(S.T_I8, B.OPTION_SET["adaptive"])}
    assert (4097, 3000) in pages and (4097, 4096) in pages and (4096, 3000) in pages and (4096, 4096) not in pages
    assert (1000, None) in pages and (16896, None) in pages


def test_ladder_variants_have_the_lengths_they_claim():
    firsts, lasts = {}, {}
    for g in B.ladder_groups():
        for case in B.ladder_table(*g):
            col = case.col
            want = B.pages_of(case)[2]
            rows = col["rows"]
            offs = want["offsets"].view(np.int64 if col["ptype"] == S.T_BIN64 else np.int32).astype(np.int64)
            lens = np.diff(offs)
            valid = np.unpackbits(want["validity"], bitorder="little")[:rows].astype(bool) if col["nullable"] else np.ones(rows, bool)
            nn = np.flatnonzero(valid)
            assert (int(lens[nn[0]]), int(lens[nn[-1]])) == case.claim, case
            if col["nullable"] and rows > len(B.LADDER):
                assert nn[0] > 0 and nn[-1] < rows - 1, case
            if g[1].forced == S.ONEVALUE:
                assert case.claim[0] == case.claim[1]
            if not case.name.endswith("-pone"):
                key = (g[0], g[1].name, rows, col["nullable"])
                firsts.setdefault(key, []).append(case.claim[0])
                lasts.setdefault(key, []).append(case.claim[1])
    for key in firsts:   # the first and the last non-null row have each ladder length once
        assert sorted(firsts[key]) == sorted(B.LADDER), key
        assert sorted(lasts[key]) == sorted(B.LADDER), key


def test_scatter_gather_and_place_are_inverses():
    n = 0
    for case in B.table(S.T_I16, B.OPTION_SET["adaptive"]) + B.table(S.T_BIN32, B.OPTION_SET["dict"]):
        pages, metas, _ = B.pages_of(case)
        for order in ("ascending", "descending"):
            buf, offs = B.scatter(pages, metas, order=order, junk=0xEE)
            assert np.array_equal(B.gather(buf, metas, offs), pages), (case, order)
            lens = metas[:, 0].astype(np.int64)
            o = offs.astype(np.int64)
            if metas.shape[0] > 1:
                d = np.diff(o)
                assert (d > 0).all() if order == "ascending" else (d < 0).all()
            # every page behind 1 to 37 junk bytes, no two pages overlap, the rest of the buffer is junk
            used = np.zeros(buf.size, bool)
            for a, ln in zip(o, lens):
                assert not used[a:a + ln].any()
                used[a:a + ln] = True
            assert (buf[~used] == 0xEE).all()
            ends = np.sort(o + lens)
            starts = np.sort(o)
            gaps = starts - np.concatenate([[0], ends[:-1]])
            assert gaps.min() >= 1 and gaps.max() <= 37
            n += 1
        for shift in (0, 1, 7, 15):
            buf, at = B.place(pages, shift, 0xFF)
            assert at == shift and np.array_equal(buf[at:at + pages.size], pages)
            assert (buf[:at] == 0xFF).all() and (buf[at + pages.size:] == 0xFF).all() and buf.size > at + pages.size
    assert n > 40


SPAN_PROGRAM = r'''
#include <cstdio>
#include "sb_span.h"
int main() {
    const uint64_t M = ~0ull, H = 1ull << 63;
    struct { uint64_t off, len, cap; bool ok; } t[] = {
        {0, 0, 0, true}, {0, 1, 0, false}, {1, 0, 0, false}, {0, 100, 100, true}, {0, 101, 100, false},
        {60, 40, 100, true}, {60, 41, 100, false}, {100, 0, 100, true}, {100, 1, 100, false}, {101, 0, 100, false},
        {M, 1, 100, false}, {M, 2, 100, false}, {1, M, 100, false}, {2, M, 100, false}, {M, M, 100, false},
        {M - 99, 100, 100, false}, {M - 98, 100, 100, false}, {50, M - 49, 100, false}, {50, M - 48, 100, false},
        {H, H, 100, false}, {H, H + 1, 100, false}, {H + 1, H, 100, false}, {H, H, M, false}, {H, H - 1, M, true},
        {H - 1, H, M, true}, {H, H, H, false}, {H, 0, H, true}, {0, H, H, true}, {1, H, H, false}, {H - 1, 1, H, true},
        {H - 1, 2, H, false}, {M, 0, M, true}, {0, M, M, true}, {M, 1, M, false}, {1, M, M, false}, {M - 1, 1, M, true},
    };
    int bad = 0;
    for (auto& c : t)
        if (page_span_ok(c.off, c.len, c.cap) != c.ok) {
            printf("page_span_ok(%llu, %llu, %llu) is not %d\n", (unsigned long long)c.off, (unsigned long long)c.len,
                   (unsigned long long)c.cap, (int)c.ok);
            bad++;
        }
    printf("%zu spans checked\n", sizeof t / sizeof t[0]);
    return bad != 0;
}
'''


def test_span_check_does_not_wrap(tmp_path):
    """offsets and lengths near 2^64 and 2^63, exact fits and one byte over: tested here, never against the GPU"""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "span.cpp"
    src.write_text(SPAN_PROGRAM)
    exe = tmp_path / "span"
    subprocess.run([cxx, "-std=c++17", "-Wall", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout
    assert "36 spans checked" in run.stdout
    # the host tables of the read calls use this check and form no sum of an offset and a length themselves
    api = open(os.path.join(CSRC, "sb_api.hip")).read()
    fill = api[api.index("static int32_t fill_read_tables"):]
    fill = fill[:fill.index("\n}\n")]
    assert fill.count("page_span_ok(") == 2 and "+ len >" not in fill and "in_off > c.pages_len" not in fill
