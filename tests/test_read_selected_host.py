"""sb_read_selected without a GPU: the symbol is exported, the ctypes struct has the header's layout, the Python layer
refuses what needs no device, and the arithmetic of the sink — rank of a selection word + set bits below the row's own =
output row — is checked in numpy on the selection patterns that tests/test_gpu_read_selected.py runs on the device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from strawboat_amd import _native as N
from strawboat_amd.read_selected import check_column, read_selected, selection_bytes
from strawboat_amd.types import PhysicalType as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "strawboat_hip.h")

ROWS = 10_000          # 16 rows in the last selection word
PAGE_ROWS = (2050, 4100)   # the nullable Int64 column of plain pages / the RLE, plain and Dict columns of longer pages, in
                           # whose first page row 4096 is a tile seam (tiles are per page: 2050-row pages have one tile)


def _straddle(rows, at):
    """64 consecutive ones, 32 on each side of row `at`"""
    m = np.zeros(rows, bool)
    m[at - 32:at + 32] = True
    return m


def _random(rows, p, seed):
    return np.random.default_rng(seed).random(rows) < p


def _one(rows, at):
    m = np.zeros(rows, bool)
    m[at] = True
    return m


def _page(rows, page_rows, k):
    m = np.zeros(rows, bool)
    m[k * page_rows:(k + 1) * page_rows] = True
    return m


def patterns(rows, page_rows):
    """[(name, mask, tail)]: tail = every bit behind `rows` of the last word is set in the bitmap (and must be ignored)"""
    assert rows % 32 and page_rows % 32 and rows > 2 * page_rows + 64
    return [
        ("zeros", np.zeros(rows, bool), False),
        ("ones", np.ones(rows, bool), False),
        ("bit 0", _one(rows, 0), False),
        ("last bit", _one(rows, rows - 1), False),
        ("one page", _page(rows, page_rows, 1), False),
        ("alternating", np.arange(rows) % 2 == 0, False),
        ("random 0.001", _random(rows, 0.001, 1), False),
        ("random 0.5", _random(rows, 0.5, 2), False),
        ("random 0.999", _random(rows, 0.999, 3), False),
        ("page seam inside a word", _straddle(rows, page_rows), False),
        ("tile seam", _straddle(rows, 4096), False),
        ("lanes 63 | 64 of a tile", _straddle(rows, 64), False),
        ("lanes 63 | 64 of the second page", _straddle(rows, page_rows + 64), False),
        ("bits behind the rows set", _random(rows, 0.3, 4), True),
        ("zeros, bits behind the rows set", np.zeros(rows, bool), True),
    ]


def bitmap_of(mask, tail=False):
    """the selection bitmap as the filter writes it: LSB-first, whole 32-bit words"""
    rows = mask.size
    bits = np.zeros(selection_bytes(rows) * 8, bool)
    bits[:rows] = mask
    if tail:
        bits[rows:] = True
    return np.packbits(bits, bitorder="little")


def model_output_rows(bitmap, rows):
    """what the kernels compute: (row, output row) of every selected row, and the total"""
    words = bitmap.view("<u4").astype(np.uint64)
    nwords = (rows + 31) // 32
    masked = words[:nwords].copy()
    if rows % 32:
        masked[-1] &= np.uint64((1 << (rows % 32)) - 1)
    popc = np.array([bin(int(w)).count("1") for w in masked], np.uint64)
    rank = np.concatenate([[0], np.cumsum(popc)]).astype(np.uint64)   # nwords + 1 entries: the last is the total
    out = []
    for c in range(rows):
        w = int(words[c >> 5])   # (the sink loads the word as it is: the bits behind `rows` are above every row's own)
        b = c & 31
        if (w >> b) & 1:
            out.append((c, int(rank[c >> 5]) + bin(w & ((1 << b) - 1)).count("1")))
    return out, int(rank[nwords])


def test_symbol_is_declared_and_exported():
    assert "sb_read_selected" in N.EXPORTS
    assert re.search(r"\bsb_read_selected\s*\(", open(HEADER).read())
    if not os.path.exists(N.LIB_PATH):
        pytest.fail("%s is missing: build() first" % N.LIB_PATH)
    out = subprocess.run(["nm", "-D", "--defined-only", N.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT sb_read_selected$", out, re.M)


def test_ctypes_struct_has_the_headers_layout(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    fields = [name for name, _ in N.ColumnReadSelectedC._fields_]
    src = tmp_path / "layout.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "strawboat_hip.h"\nint main() {\n'
                   '    printf("sizeof %zu\\n", sizeof(sb_column_read_selected));\n' +
                   "".join('    printf("%s %%zu\\n", offsetof(sb_column_read_selected, %s));\n' % (f, f) for f in fields) +
                   "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cxx, "-std=c++11", "-I", os.path.dirname(HEADER), "-o", str(exe), str(src)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["sizeof"]) == C.sizeof(N.ColumnReadSelectedC) == 120
    for f in fields:
        assert int(got[f]) == getattr(N.ColumnReadSelectedC, f).offset, f


def test_unsupported_types_and_short_bitmaps_are_refused_on_the_host():
    for ptype in (P.INT8, P.INT16, P.INT32, P.INT64, P.UINT8, P.UINT16, P.UINT32, P.UINT64, P.FLOAT32, P.FLOAT64):
        check_column(ptype, 33, 8)
    for ptype in (P.BOOLEAN, P.INT128, P.INT256, P.BINARY, P.LARGE_BINARY, P.NULL):
        with pytest.raises(ValueError):
            check_column(ptype, 33, 8)
    assert [selection_bytes(r) for r in (0, 1, 32, 33, 10_000)] == [0, 4, 4, 8, 1252]
    for rows, nbytes in ((1, 0), (33, 4), (33, 7), (10_000, 1250)):   # (1250 = ceil(rows/8): whole words are asked for)
        with pytest.raises(ValueError):
            check_column(P.INT64, rows, nbytes)


def test_bad_arguments_raise_before_anything_is_enqueued():
    """the context is never called: the checks come first"""
    import torch
    from strawboat_amd.read import ColumnPages

    class Ctx:   # (only asked where its tensors live)
        torch_device = torch.device("cpu")

    metas = np.array([[100, 40]], np.uint64)
    col = ColumnPages(P.INT64, False, torch.zeros(100, dtype=torch.uint8), metas)
    with pytest.raises(ValueError):   # a bitmap of 4 bytes for 40 rows
        read_selected(Ctx(), [col], torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError):   # an unsupported type
        read_selected(Ctx(), [ColumnPages(P.BOOLEAN, False, col.pages, metas)], torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError):   # one selection per column
        read_selected(Ctx(), [col, col], [torch.zeros(8, dtype=torch.uint8)])
    with pytest.raises(TypeError):    # not a bitmap
        read_selected(Ctx(), [col], [np.zeros(8, np.uint8)])
    with pytest.raises(ValueError):   # a bitmap on another device
        read_selected(Ctx(), [col], torch.zeros(8, dtype=torch.uint8, device="meta"))


@pytest.mark.parametrize("page_rows", PAGE_ROWS)
def test_rank_plus_popcount_below_is_the_output_row(page_rows):
    for name, mask, tail in patterns(ROWS, page_rows):
        bitmap = bitmap_of(mask, tail)
        assert bitmap.size == selection_bytes(ROWS)
        got, total = model_output_rows(bitmap, ROWS)
        want = np.flatnonzero(mask)
        assert total == want.size, name
        assert [c for c, _ in got] == want.tolist(), name
        assert [k for _, k in got] == list(range(want.size)), name


def test_the_seam_patterns_sit_where_they_say():
    for page_rows in PAGE_ROWS:
        p = dict((name, mask) for name, mask, _ in patterns(ROWS, page_rows))
        seam = np.flatnonzero(p["page seam inside a word"])
        assert seam.size == 64 and seam[0] < page_rows <= seam[-1] and page_rows % 32 != 0
        tile = np.flatnonzero(p["tile seam"])
        assert tile[0] == 4096 - 32 and tile[-1] == 4096 + 31
        lanes = np.flatnonzero(p["lanes 63 | 64 of a tile"])
        assert lanes[0] == 32 and lanes[-1] == 95
        assert p["one page"].sum() == page_rows and p["zeros"].sum() == 0 and p["ones"].all()
