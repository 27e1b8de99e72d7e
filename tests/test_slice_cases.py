"""The table of sliced Arrow arrays (tests/slice_cases.py) against the CPU oracle alone: every case sits where it claims.

  * the table is well formed: every family, both fills, the row limits,
  * the oracle's pages for the presented slice reach the codec (and the index codec) the case states: no case left out,
  * primitive and Binary cases: the oracle's bytes do not depend on the poison; primitive cases: they equal the bytes
    of the compacted copy (Binary: `values_len` of the whole buffer enters the selector and the hdr9 by design),
  * Boolean cases: RLE / OneValue pages and pages at an unaligned value offset do not depend on the poison; a Basic page
    whose first value bit is byte aligned holds the bitmap's bytes as they stand (boolean/mod.rs:44-54), so the two fills
    differ in exactly the last byte of the last page's block: asserted, the quirk is pinned on both sides,
  * the row limits the table was built around are the ones in the sources.

tests/test_gpu_write_slices.py sends the same presentations through the device."""
import os
import re

import numpy as np
import pytest

from oracle import sbo as S
from tests import slice_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = T.families()

_written = {}


def written(case, fill):
    """the oracle's (pages, metas) for a presentation (computed once)"""
    key = (case.name, fill)
    if key not in _written:
        _written[key] = T.oracle_write(case, T.present(case, fill)[0])
    return _written[key]


def blocks_decoded(case, pages, metas):
    return S.read_column(case.ptype, case.nullable, pages, metas)


def same_rows(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("values", "validity", "offsets")) and a["rows"] == b["rows"]


def test_the_table_is_well_formed():
    assert list(FAMILIES) == list(T.FAMILIES)
    seen_offsets = set()
    for family, cases in FAMILIES.items():
        assert cases, family
        for c in cases:
            assert c.rows >= 1 and c.start >= 0
            assert c.rows <= T.MAX_ROWS or family == "long_pages", c.name
            assert c.valid is None or len(c.valid) == c.rows, c.name
            for fill in T.FILLS:      # every case exists with both fills, and the buffers end where the contract says
                p, k = T.present(c, fill)
                if c.nullable:
                    assert p["validity"].size == (p["validity_bit_offset"] + c.rows + 7) // 8, c.name
                if c.kind == "bool":
                    assert p["values"].size == (p["values_bit_offset"] + c.rows + 7) // 8, c.name
                if c.kind == "bin":
                    assert p["offsets"][0] != 0 and p["values"].size > int(p["offsets"][-1]), c.name
                if c.kind == "prim" and c.rows > 1 and fill == 0:
                    w = T.WIDTH[c.ptype]
                    buf = p["values_buf"].reshape(-1, w)
                    s = buf[0]
                    inside = buf[c.start:c.start + c.rows]
                    assert not (inside == s).all(axis=1).any(), "%s: the sentinel occurs inside the slice" % c.name
                    assert (buf[-1] == s).all() and p["values_skip"] == c.start * w
            if c.nullable and family not in ("short_bitmaps",):
                seen_offsets.add(c.start)
        if family not in ("bitpack_patas", "long_pages", "short_bitmaps", "host_memory"):
            assert {c.start for c in cases} >= set(T.OFFSETS), family
            assert any(c.advance for c in cases) and any(not c.advance and c.start >= 8 for c in cases), family
    assert seen_offsets >= set(T.OFFSETS)
    for c in FAMILIES["long_pages"]:
        assert c.rows == T.BIG_ROWS + 13 and c.start in (13, 4099)
    for c in FAMILIES["prim_dict_fused"]:
        ps = c.opt["max_page_size"]
        assert T.BP_MIN_ROWS <= ps <= T.BP_MAX_ROWS and c.rows % ps == 0, c.name
    for c in FAMILIES["short_bitmaps"]:
        assert (c.start + c.rows + 7) // 8 <= 8
    assert any((c.start + c.rows + 7) // 8 < 8 for c in FAMILIES["short_bitmaps"])
    assert any((c.start + c.rows) % 8 == 0 for c in FAMILIES["short_bitmaps"])
    bools = FAMILIES["boolean"]
    assert {c.bpos for c in bools} == set(T.BOOL_VALUE_OFFSETS)
    assert {(c.bpos % 8 == 0, c.voff % 8 == 0) for c in bools if c.nullable} == {(a, b) for a in (True, False) for b in (True, False)}
    for family in ("row_level", "binary", "boolean"):     # every edge combination
        assert {(bool(c.valid[0]), bool(c.valid[-1])) for c in FAMILIES[family] if c.nullable} == set(T.EDGES), family


@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_oracle_reaches_the_codec_the_case_states(family):
    wrong = []
    for c in FAMILIES[family]:
        for fill in T.FILLS:
            pages, metas = written(c, fill)
            codecs, inner = S.stat_column(c.ptype, c.nullable, pages, metas)
            want = list(c.codec) if isinstance(c.codec, tuple) else [c.codec] * len(codecs)
            if codecs.tolist() != want:
                wrong.append("%s fill %d: the oracle chose %s, the table states %s" % (c.name, fill, codecs.tolist(), want))
            if c.inner is not None and set(inner.tolist()) != {c.inner}:
                wrong.append("%s fill %d: index codecs %s, the table states %d" % (c.name, fill, inner.tolist(), c.inner))
    assert not wrong, "\n".join(wrong)


def test_forced_dict_cases_sit_on_both_sides_of_the_lds_table():
    seen = set()
    for c in FAMILIES["row_level"]:
        if "keys_" in c.name:
            ps = c.opt["max_page_size"]
            v = np.asarray(c.values)
            for r0 in range(0, c.rows, ps):
                seen.add(len(np.unique(v[r0:r0 + ps][c.valid[r0:r0 + ps]])) + (0 if c.valid[r0] else 1) <= T.DL_CAP)
    assert seen == {True, False}


@pytest.mark.parametrize("family", list(T.FAMILIES))
def test_poison_does_not_reach_primitive_and_binary_pages(family):
    for c in FAMILIES[family]:
        if c.kind == "bool":
            continue
        (p0, m0), (p1, m1) = written(c, 0), written(c, 1)
        assert np.array_equal(m0, m1) and np.array_equal(p0, p1), c.name
        if c.kind == "prim":
            k = T.present(c, 0)[1]
            pk, mk = S.write_column(k["ptype"], k["nullable"], k["rows"], k["values"], validity=k["validity"], options=T.options(c))
            assert np.array_equal(m0, mk) and np.array_equal(p0, pk), "%s: differs from the compacted copy" % c.name


@pytest.mark.parametrize("family", [f for f in T.FAMILIES if any(c.kind == "bool" for c in FAMILIES[f])])
def test_boolean_pages_and_the_spare_bits_of_an_aligned_basic_page(family):
    pinned = 0
    for c in FAMILIES[family]:
        if c.kind != "bool":
            continue
        (p0, m0), (p1, m1) = written(c, 0), written(c, 1)
        codecs = S.stat_column(c.ptype, c.nullable, p0, m0)[0].tolist()
        ps = c.opt.get("max_page_size", c.rows)
        last = len(codecs) - 1
        last_rows = c.rows - last * ps
        # the only bits of the buffer behind a page that are not the slice's own: the spare bits of the last page's last byte
        quirk = codecs[last] in (S.NONE, S.LZ4, S.ZSTD, S.SNAPPY) and T.bool_page_aligned(c, ps, last) and last_rows % 8 != 0
        if not quirk:
            assert np.array_equal(m0, m1) and np.array_equal(p0, p1), c.name
            continue
        pinned += 1
        spans = T.page_spans(m0)
        if c.decode:      # the stream is not pinned: the decoded bitmap differs in the last byte's spare bits only
            d0, d1 = blocks_decoded(c, p0, m0), blocks_decoded(c, p1, m1)
            assert same_rows(d0, d1), c.name
            a0, a1 = spans[last][0], T.page_spans(m1)[last][0]
            assert np.array_equal(p0[:a0], p1[:a1]), c.name
            u0, u1 = raw_block(c, p0[a0:]), raw_block(c, p1[a1:])
        else:
            assert np.array_equal(m0, m1), c.name
            diff = np.flatnonzero(p0 != p1)
            assert diff.tolist() == [spans[last][1] - 1], "%s: the fills differ at %s" % (c.name, diff.tolist())
            u0, u1 = raw_block(c, p0[spans[last][0]:]), raw_block(c, p1[spans[last][0]:])
        assert np.array_equal(u0[:-1], u1[:-1]) and u0[-1] != u1[-1], c.name
        keep, b0, b1 = (1 << (last_rows % 8)) - 1, int(u0[-1]), int(u1[-1])
        assert b0 & ~keep == 0 and b1 | keep == 0xFF and (b0 & keep) == (b1 & keep), c.name
    if family in ("boolean", "basic_blocks"):
        assert pinned >= 2, "no case of %s pins the spare bits" % family


def raw_block(case, page):
    """the uncompressed bytes of a Boolean Basic page's block"""
    cur = T.def_section_len(page, case.nullable)
    codec, csize, usize = int(page[cur]), int.from_bytes(bytes(page[cur + 1:cur + 5]), "little"), int.from_bytes(bytes(page[cur + 5:cur + 9]), "little")
    body = page[cur + 9:cur + 9 + csize]
    nbytes = (usize + 7) // 8       # (a Boolean block's uncompressed_size is its number of rows)
    return body.copy() if codec == S.NONE else S.block_decompress(codec, body, nbytes)


def _source(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.findall(pattern, text)
    assert m, "%s: the pattern %r no longer matches; update tests/slice_cases.py with the source" % (what, pattern)
    assert len(set(m)) == 1, "%s: several different values %s" % (what, m)
    return m[0]


def test_row_limits_of_the_table_are_the_ones_in_the_sources():
    csrc = ("strawboat_amd", "csrc")
    encode, common_h = _source(*csrc, "sb_encode.hip"), _source(*csrc, "sb_common.h")
    lds_h, big_h = _source(*csrc, "sb_dict_lds.h"), _source(*csrc, "sb_select_big.h")
    assert int(_one(r"constexpr\s+int\s+TILE_ROWS\s*=\s*(\d+)\s*;", common_h, "TILE_ROWS")) == T.TILE_ROWS
    assert int(_one(r"constexpr\s+uint64_t\s+BP_MIN_ROWS\s*=\s*(\d+)\s*;", encode, "BP_MIN_ROWS")) == T.BP_MIN_ROWS
    assert int(_one(r"return\s+N\s*>=\s*BP_MIN_ROWS\s*&&\s*N\s*<=\s*(\d+)\s*&&", encode, "bp_fits")) == T.BP_MAX_ROWS
    assert int(_one(r"\bDL_CAP\s*=\s*(\d+)\s*,", lds_h, "DL_CAP")) == T.DL_CAP
    for name, text in (("sb_encode.hip", encode), ("sb_select_big.h", big_h)):
        assert int(_one(r"#define\s+SB_BIN_BIG_ROWS\s+\(1ull\s*<<\s*(\d+)\)", text, "SB_BIN_BIG_ROWS in " + name)) == 18
    assert int(_one(r"constexpr\s+uint64_t\s+SEL_BIG_ROWS\s*=\s*1ull\s*<<\s*(\d+)\s*;", big_h, "SEL_BIG_ROWS")) == 18
    assert T.BIG_ROWS == 1 << 18
