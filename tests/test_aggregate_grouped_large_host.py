"""sb_aggregate_grouped_large and group_by without a GPU: the symbol is exported, the constants are what the header says
(through the host compiler), the struct it shares with sb_aggregate_grouped keeps its layout, the Python layer refuses
what needs no device before anything is enqueued, and the chunk rule -- column-local tile -> chunk of 16, tile -> page by
PageTask::first_tile (grpl_page_of, csrc/sb_common.h) -- is checked twice: a Python model against hand-written cases,
and the function itself in a stand-alone host program against the same rule stated the slow way."""
import ctypes as C
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from strawboat_amd import _native as N
from strawboat_amd.types import PhysicalType as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")
CSRC = os.path.join(ROOT, "strawboat_amd", "csrc")

OFFSETS = dict(physical_type=0, is_nullable=4, pages=8, pages_len=16, metas=24, n_pages=32, page_offsets=40, selection=48,
               selection_capacity=56, group_ids=64, group_ids_capacity=72, group_id_width=80, n_groups=84, ops=88, reserved=92,
               groups=96, rows=104, selected=112, out_of_range=120)


def test_symbol_is_declared_and_exported():
    assert "sb_aggregate_grouped_large" in N.EXPORTS
    assert re.search(r"\bsb_aggregate_grouped_large\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_aggregate_grouped_large$", out, re.M)
    assert re.search(r"\bT sb_aggregate_grouped$", out, re.M)
    import strawboat_amd as sb
    assert sb.aggregate_grouped_large and sb.GroupedAggregateLargeBatch and sb.group_by
    from strawboat_amd import aggregate_grouped_large as L   # (the name is the function's in the package: the module through sys.modules)
    import sys
    mod = sys.modules["strawboat_amd.aggregate_grouped_large"]
    assert L is mod.aggregate_grouped_large and mod.MAX_GROUPS_LARGE == 1024


def test_the_constants_and_the_shared_structs_layout_through_the_host_compiler(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\ngroup %zu\\n", sizeof(sb_column_aggregate_grouped), sizeof(sb_agg_group));\n'
                   '    printf("LARGE %u\\nMAX %u\\nKEYS %u\\n", SB_AGG_LARGE_MAX_GROUPS, SB_AGG_MAX_GROUPS, SB_KEY_MAX_KEYS);\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_aggregate_grouped, %s));\n' % (f, f) for f in OFFSETS) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["LARGE"]) == N.SB_AGG_LARGE_MAX_GROUPS == 1024 == int(got["KEYS"]) == N.SB_KEY_MAX_KEYS
    assert int(got["MAX"]) == N.SB_AGG_MAX_GROUPS == 256
    assert int(got["sizeof"]) == C.sizeof(N.ColumnAggregateGroupedC) == 128 and int(got["group"]) == C.sizeof(N.AggGroupC) == 64
    assert [name for name, _ in N.ColumnAggregateGroupedC._fields_] == list(OFFSETS)
    for f, off in OFFSETS.items():
        assert int(got[f]) == off == getattr(N.ColumnAggregateGroupedC, f).offset, f


def test_check_column_refuses_what_aggregate_grouped_refuses_with_1024():
    from strawboat_amd.aggregate_grouped import check_column as small
    from strawboat_amd.aggregate_grouped_large import MAX_GROUPS_LARGE, check_column
    assert MAX_GROUPS_LARGE == 1024
    every = (P.INT8, P.INT16, P.INT32, P.INT64, P.UINT8, P.UINT16, P.UINT32, P.UINT64, P.FLOAT32, P.FLOAT64,
             P.BOOLEAN, P.INT128, P.INT256, P.BINARY, P.LARGE_BINARY, P.NULL)
    for ptype in every:   # count works on every type
        check_column(ptype, 33, 8, N.SB_AGG_COUNT, 1024, 2, 33)
        check_column(ptype, 33, None, 0, 257, 4, 40)
    for ptype in every[:10]:
        for ng in (1, 256, 257, 1024):
            check_column(ptype, 33, 8, 15, ng, 2, 33)
    for ptype in every[10:]:
        for op in (N.SB_AGG_MIN, N.SB_AGG_MAX, N.SB_AGG_SUM, 15):
            with pytest.raises(ValueError):
                check_column(ptype, 33, 8, op, 4, 1, 33)
    with pytest.raises(ValueError):   # a short bitmap
        check_column(P.INT64, 33, 4, 15, 4, 1, 33)
    for bad in (0, 1025, -1, 1 << 20, 2.0, 1024.0, None, True, False):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, 15, bad, 2, 33)
    for width in (None, 0, 3, 8):
        with pytest.raises(ValueError):
            check_column(P.INT64, 33, 8, 15, 4, width, 33)
    with pytest.raises(ValueError):   # fewer ids than rows
        check_column(P.INT64, 33, 8, 15, 4, 1, 32)
    check_column(P.INT64, 0, None, 15, 1024, 1, 0)
    # the 256-group call's own limit is where it was
    small(P.INT64, 33, 8, 15, 256, 2, 33)
    for bad in (257, 1024):
        with pytest.raises(ValueError):
            small(P.INT64, 33, 8, 15, bad, 2, 33)


def test_bad_arguments_raise_before_anything_is_enqueued():
    """the context is never called: the checks come first"""
    import torch
    from strawboat_amd import aggregate_grouped, aggregate_grouped_large, group_by
    from strawboat_amd.read import ColumnPages

    class Ctx:   # (only asked where its tensors live)
        torch_device = torch.device("cpu")

    metas = np.array([[100, 40]], np.uint64)
    col = ColumnPages(P.INT64, False, torch.zeros(100, dtype=torch.uint8), metas)
    ids = torch.zeros(40, dtype=torch.uint16)
    bm = torch.zeros(8, dtype=torch.uint8)
    with pytest.raises(ValueError):   # a bitmap of 4 bytes for 40 rows
        aggregate_grouped_large(Ctx(), [col], ids, 1024, torch.zeros(4, dtype=torch.uint8))
    for n_groups in (0, 1025, -3, True, 300.0, 2.5):
        with pytest.raises(ValueError):
            aggregate_grouped_large(Ctx(), [col], ids, n_groups, bm)
    for bad in (torch.zeros(40, dtype=torch.int64), torch.zeros(40, dtype=torch.float32), torch.zeros(40, dtype=torch.int8),
                torch.zeros(40, dtype=torch.int16), torch.zeros(39, dtype=torch.uint16), torch.zeros(80, dtype=torch.uint16)[::2],
                torch.zeros((40, 1), dtype=torch.uint16), torch.zeros(40, dtype=torch.uint16, device="meta"), np.zeros(40, np.uint16)):
        with pytest.raises(ValueError):
            aggregate_grouped_large(Ctx(), [col], bad, 1024, bm)
    for ptype in (P.BOOLEAN, P.BINARY, P.INT128, P.NULL):   # an unsupported type with min / max / sum
        for ops in (("min",), ("count", "max"), ("sum",)):
            with pytest.raises(ValueError):
                aggregate_grouped_large(Ctx(), [ColumnPages(ptype, False, col.pages, metas)], ids, 1024, bm, ops=ops)
    with pytest.raises(ValueError):   # unknown ops
        aggregate_grouped_large(Ctx(), [col], ids, 1024, None, ops=("count", "avg"))
    with pytest.raises(ValueError):   # one selection / one ids tensor / one n_groups per column
        aggregate_grouped_large(Ctx(), [col, col], ids, 1024, [bm])
    with pytest.raises(ValueError):
        aggregate_grouped_large(Ctx(), [col, col], [ids], 1024, bm)
    with pytest.raises(ValueError):
        aggregate_grouped_large(Ctx(), [col, col], ids, [1024], bm)
    with pytest.raises(TypeError):    # not a bitmap
        aggregate_grouped_large(Ctx(), [col], ids, 1024, [np.zeros(8, np.uint8)])
    # the 256-group call still stops at 256
    for n_groups in (257, 1024):
        with pytest.raises(ValueError):
            aggregate_grouped(Ctx(), [col], ids, n_groups, bm)
    # group_by: the key's type and max_keys, before a key call is made
    for ptype in (P.FLOAT32, P.FLOAT64, P.BOOLEAN, P.INT128, P.INT256, P.NULL):
        with pytest.raises(ValueError):
            group_by(Ctx(), ColumnPages(ptype, False, col.pages, metas), [col])
    for mk in (0, 1025, -1, True, 2.5, None, "7"):
        with pytest.raises(ValueError):
            group_by(Ctx(), col, [col], max_keys=mk)
    with pytest.raises(ValueError):   # (a float key, whatever max_keys is)
        group_by(Ctx(), ColumnPages(P.FLOAT64, False, col.pages, metas), [col], max_keys=200)


# ---- the chunk rule: a model, and hand-written cases
TILE_ROWS, CHUNK_TILES = 4096, 16


def model(page_rows):
    """A column of pages of `page_rows` rows each, as the call's host tables describe it.  first_tile[p]: tiles in front of page
    p; then for every column-local tile j: (chunk j // 16, page, tile of the page), found the slow way: by walking the pages."""
    first_tile, tiles = [], []
    for p, n in enumerate(page_rows):
        first_tile.append(len(tiles))
        for t in range(-(-n // TILE_ROWS)):
            tiles.append((len(tiles) // CHUNK_TILES, p, t))
    return first_tile, tiles


def page_of(first_tile, gt):
    """grpl_page_of's rule: the LAST page whose first_tile is <= gt"""
    return max(p for p, f in enumerate(first_tile) if f <= gt)


def test_the_chunk_rule_on_hand_written_cases():
    # tile counts 1, 15, 16, 17, 33 in one page: chunks 1, 1, 1, 2, 3
    for ntiles, chunks in ((1, 1), (15, 1), (16, 1), (17, 2), (33, 3)):
        for rows in ((ntiles - 1) * TILE_ROWS + 1, ntiles * TILE_ROWS):
            first_tile, tiles = model([rows])
            assert len(tiles) == ntiles and first_tile == [0]
            assert -(-len(tiles) // CHUNK_TILES) == chunks == tiles[-1][0] + 1
            assert [c for c, _, _ in tiles] == [j // 16 for j in range(ntiles)]
            assert all(page_of(first_tile, j) == 0 for j in range(ntiles))
    # 33 * 4096 + 5 rows: tile 33 holds the last 5 rows and is alone in chunk 2
    first_tile, tiles = model([33 * 4096 + 5])
    assert len(tiles) == 34 and tiles[15] == (0, 0, 15) and tiles[16] == (1, 0, 16) and tiles[32] == (2, 0, 32) and tiles[33] == (2, 0, 33)
    # pages shorter than a tile: a tile each, 16 pages to a chunk; page 16 opens chunk 1
    first_tile, tiles = model([2050] * 40)
    assert first_tile == list(range(40)) and tiles[15] == (0, 15, 0) and tiles[16] == (1, 16, 0) and tiles[39] == (2, 39, 0)
    assert [page_of(first_tile, j) for j in range(40)] == list(range(40))
    # pages of 1.5 tiles: two tiles each; chunk 0 ends inside no page, chunk boundaries fall on page 8
    first_tile, tiles = model([6000] * 10)
    assert first_tile == [0, 2, 4, 6, 8, 10, 12, 14, 16, 18] and tiles[15] == (0, 7, 1) and tiles[16] == (1, 8, 0)
    # a page of 17 tiles between short ones: the chunk boundary falls inside it
    first_tile, tiles = model([100, 17 * 4096, 100])
    assert first_tile == [0, 1, 18] and tiles[15] == (0, 1, 14) and tiles[16] == (1, 1, 15) and tiles[18] == (1, 2, 0)
    assert [page_of(first_tile, j) for j in (0, 1, 17, 18)] == [0, 1, 1, 2]
    # pages without rows share their first_tile with the page behind them and are never the answer for a tile that exists
    first_tile, tiles = model([0, 5000, 0, 0, 10, 0])
    assert first_tile == [0, 0, 2, 2, 2, 3] and [(p, t) for _, p, t in tiles] == [(1, 0), (1, 1), (4, 0)]
    assert [page_of(first_tile, j) for j in range(3)] == [1, 1, 4]
    # every tile of every layout: the page lookup gives the page the walk gave
    rng = np.random.default_rng(5)
    for _ in range(50):
        page_rows = [int(x) for x in rng.choice([0, 1, 100, 2050, 4096, 4097, 6000, 70_000], int(rng.integers(1, 40)))]
        first_tile, tiles = model(page_rows)
        for j, (chunk, p, t) in enumerate(tiles):
            assert chunk == j // 16 and page_of(first_tile, j) == p and j - first_tile[p] == t


# ---- grpl_page_of and grpl_chunks in a host program of their own
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
// a column of these pages behind `lead` tiles and `p0` pages of other columns: every tile's page by the slow walk
static void check(const std::vector<uint64_t>& page_rows, uint32_t p0, uint32_t lead) {
    std::vector<sb::PageTask> tasks(p0 + page_rows.size());   // (exactly as long as the column's last page: a read behind it is caught)
    for (uint32_t i = 0; i < p0; i++) tasks[i].first_tile = 0xFFFFFFFFu;   // (never looked at)
    std::vector<uint32_t> owner;
    uint32_t tile = lead;
    for (size_t p = 0; p < page_rows.size(); p++) {
        tasks[p0 + p].first_tile = tile;
        tasks[p0 + p].num_values = page_rows[p];
        const uint32_t nt = (uint32_t)((page_rows[p] + sb::TILE_ROWS - 1) / sb::TILE_ROWS);
        for (uint32_t t = 0; t < nt; t++) owner.push_back(p0 + (uint32_t)p);
        tile += nt;
    }
    if (sb::grpl_chunks(owner.size()) != (owner.size() + 15) / 16) fails++, printf("chunks of %zu tiles\n", owner.size());
    for (size_t j = 0; j < owner.size(); j++) {
        const uint32_t got = sb::grpl_page_of(tasks.data(), p0, (uint32_t)page_rows.size(), lead + (uint32_t)j);
        if (got != owner[j] && fails++ < 10) printf("tile %zu of %zu pages: page %u, want %u\n", j, page_rows.size(), got, owner[j]);
        else if (lead + j - tasks[got].first_tile >= (tasks[got].num_values + sb::TILE_ROWS - 1) / sb::TILE_ROWS) fails++, printf("tile %zu outside its page\n", j);
    }
}
int main() {
    if (sb::GRPL_CHUNK_TILES != 16 || sb::GRPL_MAX_GROUPS != 1024 || sb::GRP_MAX_GROUPS != 256 || sb::TILE_ROWS != 4096) fails++, printf("constants\n");
    const uint64_t T = sb::TILE_ROWS;
    const uint32_t counts[] = {1, 15, 16, 17, 33};
    for (uint32_t nt : counts)
        for (uint32_t p0 : {0u, 3u})
            for (uint32_t lead : {0u, 7u, 1000000u}) {
                check({nt * T}, p0, lead);
                check({(nt - 1) * T + 1}, p0, lead);
                check(std::vector<uint64_t>(nt, 2050), p0, lead);           // pages shorter than a tile
                check(std::vector<uint64_t>(nt, T + 1), p0, lead);          // two tiles each
                std::vector<uint64_t> holes;                                // pages without rows among them
                for (uint32_t i = 0; i < nt; i++) holes.push_back(0), holes.push_back(i % 3 ? 5 : 3 * T), holes.push_back(0);
                holes.push_back(1);
                check(holes, p0, lead);
            }
    check({33 * T + 5}, 0, 0);
    check({100, 17 * T, 100}, 2, 5);
    for (int i = 0; i < 300; i++) {
        const uint64_t sizes[] = {0, 1, 100, 2050, T, T + 1, 6000, 70000};
        std::vector<uint64_t> rows(1 + rnd() % 60);
        for (auto& r : rows) r = sizes[rnd() % 8];
        check(rows, (uint32_t)(rnd() % 5), (uint32_t)(rnd() % 100000));
    }
    printf("fails %d\n", fails);
    return fails ? 1 : 0;
}
"""


def test_grpl_page_of_against_the_slow_walk(tmp_path):
    """a stand-alone host program (its own main, address and undefined-behaviour sanitizers where the compiler has them):
    tile counts 1, 15, 16, 17, 33, pages shorter than a tile, pages without rows, columns behind other columns' pages and
    tiles; the PageTask array ends with the column, so a probe behind it is an error the sanitizer reports"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no hipcc"
    src = tmp_path / "page_of.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "page_of"
    base = [hipcc, "--offload-host-only", "-std=c++17", "-O1", "-g", "-I", CSRC, "-o", str(exe), str(src)]
    rt = subprocess.run([hipcc, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
    if os.path.isabs(rt) and os.path.exists(rt):
        san = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
        assert san.returncode == 0, "the sanitized build failed though %s exists:\n%s" % (rt, san.stderr)
        syms = subprocess.run(["nm", "-D", str(exe)], capture_output=True, text=True).stdout + \
            subprocess.run(["nm", str(exe)], capture_output=True, text=True).stdout
        assert "__asan_init" in syms and "__ubsan_handle" in syms, "the program was built without the sanitizers"
    else:
        warnings.warn("hipcc has no sanitizer runtime (%r): grpl_page_of is compared WITHOUT the sanitizers" % rt)
        subprocess.run(base, check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip().endswith("fails 0"), run.stdout + run.stderr
