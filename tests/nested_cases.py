"""The edge table of the nested (Dremel) path: long lists, deep paths, chunk and tile borders, stream header lengths.

tests/nested_gen.py draws lists of 0..2 children, at most list -> list -> leaf, 3000-5000 rows.  The columns here are built
for what those shapes never reach in strawboat_amd/csrc/sb_nested.hip: lists that span several windows of k_nested_emit,
child tiles without a parent start in k_nested_gen, pages of more than one tile (and of more than 64), 3-bit rep and 4-bit
def levels, the 1 / 2 / 3-byte stream headers, validity_bit_offset, chunk_row slots of neighbouring pages.

A case is (name, levels, rows, cuts, property): `levels` in nested_gen's format (expected_state and S.nested_write_levels
take them unchanged), `cuts` the max_page_size values to cut at (None: one page), `property` = (text, check) — the condition
the case exists for.  The conditions are asserted by tests/test_nested_cases.py, so another seed cannot silently empty a case.
tests/test_nested_cases.py walks the table on the CPU oracle, tests/test_gpu_nested_edges.py on the device."""
from collections import namedtuple

import numpy as np

from oracle import sbo as S
from tests import gen

# strawboat_amd/csrc/sb_common.h: TILE_ROWS; strawboat_amd/csrc/sb_nested.hip: NE_CHUNK = TILE_ROWS - 32 (entries per window
# of k_nested_emit, without the 32 entries of the group before it)
TILE = 4096
NE_CHUNK = 4064

Case = namedtuple("Case", "name levels rows cuts prop big")   # big: compare with numpy arrays, not Python lists

LIST, LARGE, STRUCT = "list", "large_list", "struct"
_KIND = {LIST: S.K_LIST, LARGE: S.K_LARGE_LIST, STRUCT: S.K_STRUCT}


# ------------------------------------------------------------------------------------------------ builders
def _bitmap(rng, valid, off):
    """packed validity with `off` junk bits in front"""
    if not off:
        return gen.pack_bits(valid)
    return gen.pack_bits(np.concatenate([rng.random(off) < 0.5, valid]))


def build_path(spec, leaf_optional, rows, lens, seed, null_density=0.1, leaf_null=0.2, voff=None):
    """Level dicts for the path `spec` = ((list | large_list | struct, optional?), ...) over a leaf.
    lens(k, n, rng) -> the n list lengths of level k (a null list is made empty afterwards, like nested_gen).
    Structs keep validity=None (nested_gen: the reference drops the leaf slot of a null struct).
    voff = {level index: junk bits in front of that level's bitmap}, passed on as validity_off."""
    rng = np.random.default_rng(seed)
    voff = voff or {}
    lv, n = [], rows
    for k, (kind, optional) in enumerate(spec):
        if kind == STRUCT:
            lv.append(dict(kind=S.K_STRUCT, is_optional=optional, validity=None, length=n))
            continue
        valid = rng.random(n) >= null_density if optional else np.ones(n, bool)
        ln = np.where(valid, np.asarray(lens(k, n, rng), np.int64), 0)
        offs = np.zeros(n + 1, np.int64)
        np.cumsum(ln, out=offs[1:])
        d = dict(kind=_KIND[kind], is_optional=optional, validity=_bitmap(rng, valid, voff.get(k, 0)) if optional else None,
                 offsets=offs.astype(np.int64 if kind == LARGE else np.int32), length=n)
        if optional and voff.get(k, 0):
            d["validity_off"] = voff[k]
        lv.append(d)
        n = int(offs[-1])
    k = len(spec)
    valid = rng.random(n) >= leaf_null
    d = dict(kind=S.K_PRIMITIVE, is_optional=leaf_optional, validity=_bitmap(rng, valid, voff.get(k, 0)) if leaf_optional else None,
             length=n)
    if leaf_optional and voff.get(k, 0):
        d["validity_off"] = voff[k]
    lv.append(d)
    return lv


def lens_for_entries(rng, L, maxlen=3, null_density=0.1):
    """list lengths (null lists already empty) and their validity, of lists that generate exactly L level entries when
    every child is one entry: an empty or null list is one entry, a list of c children is c"""
    ln = rng.integers(0, maxlen + 1, L).astype(np.int64)
    valid = rng.random(L) >= null_density
    ln = np.where(valid, ln, 0)
    cs = np.cumsum(np.maximum(ln, 1))
    k = int(np.searchsorted(cs, L, side="right"))
    rem = L - (int(cs[k - 1]) if k else 0)
    ln, valid = ln[:k], valid[:k]
    if rem:
        ln, valid = np.append(ln, rem), np.append(valid, True)
    return ln, valid


def _list_level(ln, valid, optional=True):
    offs = np.zeros(ln.size + 1, np.int64)
    np.cumsum(ln, out=offs[1:])
    return dict(kind=S.K_LIST, is_optional=optional, validity=gen.pack_bits(valid) if optional else None,
                offsets=offs.astype(np.int32), length=int(ln.size))


def _leaf(n, rng):
    return dict(kind=S.K_PRIMITIVE, is_optional=True, validity=gen.pack_bits(rng.random(n) >= 0.2), length=n)


def exact_entries(L, shape, seed):
    """A column whose ONE page (max_page_size=None) has exactly L level entries.  shape "list": list -> leaf (the fast
    path); "list_list": list -> list -> leaf (the generic path), L // 7 of its entries being empty or null top lists."""
    rng = np.random.default_rng(seed)
    if shape == "list":
        ln, valid = lens_for_entries(rng, L)
        return [_list_level(ln, valid), _leaf(int(ln.sum()), rng)]
    assert shape == "list_list"
    n_empty = L // 7
    iln, ivalid = lens_for_entries(rng, L - n_empty)            # the inner lists: L - n_empty entries
    n_in = iln.size
    steps = rng.integers(1, 4, n_in)                            # non-empty top lists of 1..3 inner lists
    cs = np.cumsum(steps)
    k = int(np.searchsorted(cs, n_in, side="right"))
    rem = n_in - (int(cs[k - 1]) if k else 0)
    top = np.append(steps[:k], rem) if rem else steps[:k]
    tln = np.concatenate([top, np.zeros(n_empty, np.int64)]).astype(np.int64)
    tln = tln[rng.permutation(tln.size)]
    tvalid = np.where(tln > 0, True, rng.random(tln.size) >= 0.5)
    return [_list_level(tln, tvalid), _list_level(iln, ivalid), _leaf(int(iln.sum()), rng)]


def just_over_a_chunk(pages, rows_per_page, seed):
    """list -> leaf, `pages` pages of rows_per_page rows, each with NE_CHUNK + 1 .. NE_CHUNK + 40 entries: one row of a page
    (at a different place in every page) holds what its short neighbours leave"""
    rng = np.random.default_rng(seed)
    lns, valids = [], []
    for p in range(pages):
        target = NE_CHUNK + 1 + (p * 7) % 40
        ln = rng.integers(0, 4, rows_per_page).astype(np.int64)
        valid = rng.random(rows_per_page) >= 0.1
        ln = np.where(valid, ln, 0)
        at = (p * 131 + 17) % rows_per_page
        ln[at], valid[at] = 0, True
        ln[at] = target - (int(np.maximum(ln, 1).sum()) - 1)
        assert ln[at] >= 1
        lns.append(ln)
        valids.append(valid)
    ln, valid = np.concatenate(lns), np.concatenate(valids)
    return [_list_level(ln, valid), _leaf(int(ln.sum()), rng)]


def prefix(levels, rows):
    """the first `rows` top-level rows of a column as a column of its own"""
    out, n = [], rows
    for lv in levels:
        d = dict(lv, length=n)
        if lv["kind"] in (S.K_LIST, S.K_LARGE_LIST):
            d["offsets"] = np.ascontiguousarray(lv["offsets"][:n + 1])
            n = int(d["offsets"][-1])
        out.append(d)
    return out


# ------------------------------------------------------------------------------------------------ expected answers
def _bits(lv, s, e):
    if lv.get("validity") is None:
        return np.ones(e - s, np.uint8)
    off = lv.get("validity_off", 0)
    return np.unpackbits(np.asarray(lv["validity"]), bitorder="little")[off + s:off + e]


def expected_arrays(levels, r0, length):
    """nested_gen.expected_state with numpy arrays instead of Python lists (for pages of hundreds of thousands of entries)"""
    s, e = r0, r0 + length
    lengths, offsets, validity, extra = [], [], [], 0
    none = np.zeros(0, np.uint8)
    for lv in levels:
        lengths.append(e - s)
        if lv["kind"] in (S.K_LIST, S.K_LARGE_LIST):
            offs = np.asarray(lv["offsets"]).astype(np.int64)
            offsets.append(offs[s:e] - offs[s])
            validity.append(_bits(lv, s, e) if lv["is_optional"] else none)
            extra += int(np.count_nonzero(offs[s + 1:e + 1] == offs[s:e]))
            s, e = int(offs[s]), int(offs[e])
        else:
            offsets.append(np.zeros(0, np.int64))
            validity.append(_bits(lv, s, e) if lv["kind"] == S.K_STRUCT and lv["is_optional"] else none)
    leaf = levels[-1]
    return dict(lengths=lengths, offsets=offsets, validity=validity,
                leaf_validity=_bits(leaf, s, e) if leaf["is_optional"] else none,
                leaf_start=s, leaf_count=e - s, num_values=(e - s) + extra)


def page_ranges(rows, cut):
    ps = rows if cut is None else min(cut, rows)
    return [(r0, min(ps, rows - r0)) for r0 in range(0, rows, ps)]


def element_ranges(levels, r0, length):
    """[s, e) of the page's elements at every level (slice_parquet_array)"""
    s, e, out = r0, r0 + length, []
    for lv in levels:
        out.append((s, e))
        if lv["kind"] in (S.K_LIST, S.K_LARGE_LIST):
            s, e = int(lv["offsets"][s]), int(lv["offsets"][e])
    return out


def level_bits(levels):
    """(rep_bits, def_bits) of a path: the widths of parquet's max repetition / definition level"""
    rep = sum(lv["kind"] in (S.K_LIST, S.K_LARGE_LIST) for lv in levels)
    dfn = rep + sum(bool(lv["is_optional"]) for lv in levels)
    return int(rep).bit_length(), int(dfn).bit_length()


def is_fast_path(levels):
    """sb_nested.hip's top_list_only: the only list level is the first one"""
    return len(levels) >= 2 and levels[0]["kind"] in (S.K_LIST, S.K_LARGE_LIST) and all(lv["kind"] == S.K_STRUCT for lv in levels[1:-1])


# ------------------------------------------------------------------------------------------------ conditions
def _list_lengths(lv):
    return np.diff(np.asarray(lv["offsets"]).astype(np.int64))


def _entries(levels, r0, length):
    return expected_arrays(levels, r0, length)["num_values"]


def has_list_longer_than(n, k=0):
    return lambda levels, rows, cuts: int(_list_lengths(levels[k]).max()) > n


def border_after_a_long_row(levels, rows, cuts):
    ln = _list_lengths(levels[0])
    return any(c is not None and c > 1 and c < rows and ln[c - 1] >= 3000 for c in cuts)


def one_row_pages_of_several_chunks(levels, rows, cuts):
    return 1 in cuts and int(_list_lengths(levels[0]).max()) > 2 * NE_CHUNK + 32


def one_row_pages_of_more_than(n):
    return lambda levels, rows, cuts: list(cuts) == [1] and int(_list_lengths(levels[0]).max()) > n


def child_tile_without_parent_start(k):
    """some page has a whole tile of level-k elements in which no element of the list level above starts — what k_nested_gen's
    generic branch sees as an all-zero tile: every child resolves to p_first"""
    def check(levels, rows, cuts):
        par = next(j for j in range(k - 1, -1, -1) if levels[j]["kind"] != S.K_STRUCT)
        if par != k - 1:
            return False
        offs = np.asarray(levels[par]["offsets"]).astype(np.int64)
        for cut in cuts:
            for r0, ln in page_ranges(rows, cut):
                s, e = element_ranges(levels, r0, ln)[k]
                for cb in range(s, e - TILE + 1, TILE):
                    lo, hi = np.searchsorted(offs, cb, side="right"), np.searchsorted(offs, cb + TILE, side="left")
                    if hi <= lo:
                        return True
        return False
    return check


def _empty_runs(ln, at_least):
    """mask of the elements inside a run of >= at_least empty lists"""
    e = ln == 0
    edges = np.flatnonzero(np.diff(np.concatenate([[0], e.astype(np.int8), [0]])))
    m = np.zeros(ln.size, bool)
    for a, b in zip(edges[::2], edges[1::2]):
        if b - a >= at_least:
            m[a:b] = True
    return m


def pages_cut_inside_runs(levels, rows, cuts):
    """runs of >= 300 empties at both levels; a page that starts and ends inside such a run of the top level, and a page
    border inside such a run of the inner level"""
    top, inner = _empty_runs(_list_lengths(levels[0]), 300), _empty_runs(_list_lengths(levels[1]), 300)
    if not top.any() or not inner.any():
        return False
    both_ends = inner_border = False
    offs = np.asarray(levels[0]["offsets"]).astype(np.int64)
    for cut in cuts:
        for r0, ln in page_ranges(rows, cut):
            r1 = r0 + ln
            if 0 < r0 and r1 < rows and top[r0 - 1] and top[r0] and top[r1 - 1] and top[r1]:
                both_ends = True
            s = int(offs[r0])
            if 0 < s < inner.size and inner[s - 1] and inner[s]:
                inner_border = True
    return both_ends and inner_border


def has_level_bits(rep_bits, def_bits):
    return lambda levels, rows, cuts: level_bits(levels) == (rep_bits, def_bits)


def one_page_of(L):
    return lambda levels, rows, cuts: list(cuts) == [None] and _entries(levels, 0, rows) == L


def every_page_just_over_a_chunk(levels, rows, cuts):
    pages = page_ranges(rows, cuts[0])
    return len(cuts) == 1 and len(pages) >= 10 and all(NE_CHUNK + 1 <= _entries(levels, r0, ln) <= NE_CHUNK + 40 for r0, ln in pages)


def has_validity_offset(k, off):
    return lambda levels, rows, cuts: levels[k].get("validity_off", 0) == off and levels[k]["validity"].size * 8 >= off + levels[k]["length"]


def _all(*checks):
    return lambda levels, rows, cuts: all(c(levels, rows, cuts) for c in checks)


# ------------------------------------------------------------------------------------------------ the table
EXACT_L = (1, 31, 32, 33, 504, 505, 4063, 4064, 4065, 4095, 4096, 4097, 8128, 8129, 65528, 65529, 65536)
MORE_THAN_64_TILES = 64 * TILE + 1   # the smallest page at which k_nested_bases takes its second step of 64 tiles


def _long_lens(at_level, every=400, first_long=12000):
    """mostly empty lists, one in `every` with 3000..12000 children (the first of them `first_long`) at level at_level;
    0..2 children at the others"""
    def lens(k, n, rng):
        if k != at_level:
            return rng.integers(0, 3, n)
        ln = np.zeros(n, np.int64)
        at = np.arange(every // 3, n, every)
        ln[at] = rng.integers(3000, 12001, at.size)
        if at.size:
            ln[at[0]] = first_long
        return ln
    return lens


def _short(k, n, rng):
    return rng.integers(0, 4, n)


def _run_lens(k, n, rng):
    """alternating runs of 300..400 empty lists and of as many lists with 1..3 children"""
    ln = np.zeros(n, np.int64)
    i, empty = 0, True
    while i < n:
        run = int(rng.integers(300, 401))
        if not empty:
            ln[i:i + run] = rng.integers(1, 4, min(run, n - i))
        i += run
        empty = not empty
    return ln


def _long_cuts(levels, rows):
    ln = _list_lengths(levels[0])
    long_rows = np.flatnonzero(ln >= 3000)
    return [None, int(long_rows[1]) + 1 if long_rows.size > 1 else None]


def _run_cuts(levels, rows):
    """one cut whose first border lies inside a run of empty top lists (and so does the page's end), one whose first border
    lies inside a run of empty inner lists"""
    top, inner = _empty_runs(_list_lengths(levels[0]), 300), _empty_runs(_list_lengths(levels[1]), 300)
    offs = np.asarray(levels[0]["offsets"]).astype(np.int64)
    cuts = []
    for c in range(320, rows // 2):
        if 2 * c < rows and top[c - 1] and top[c] and top[2 * c - 1] and top[2 * c]:
            cuts.append(c)
            break
    for c in range(320, rows // 2):
        s = int(offs[c])
        if 0 < s < inner.size and inner[s - 1] and inner[s]:
            cuts.append(c)
            break
    return cuts


def build_cases():
    cases = []

    def add(name, levels, cuts, text, check, big=False):
        cases.append(Case(name, levels, levels[0]["length"], list(cuts), (text, check), big))

    two_windows = 2 * NE_CHUNK + 32
    # ---- long lists on the fast path (k_nested_emit): list, list -> struct -> leaf
    for name, spec in (("list", ((LIST, True),)), ("list_struct", ((LIST, True), (STRUCT, True)))):
        lv = build_path(spec, True, 1600, _long_lens(0), seed=101)
        add("long_fast_%s" % name, lv, _long_cuts(lv, 1600),
            "a list longer than 2 windows of k_nested_emit, a page border right behind a long row",
            _all(has_list_longer_than(two_windows), border_after_a_long_row))
        first_long = int(np.flatnonzero(_list_lengths(lv[0]) > two_windows)[0])
        add("long_fast_%s_row_pages" % name, prefix(lv, first_long + 9), [1],
            "one row is one page of several chunks", one_row_pages_of_several_chunks)
    lv = build_path(((LARGE, True),), True, 1600, _long_lens(0), seed=113)
    add("long_fast_large_list", lv, _long_cuts(lv, 1600), "i64 offsets: a list longer than 2 windows of k_nested_emit",
        _all(has_list_longer_than(two_windows), border_after_a_long_row, lambda levels, rows, cuts: levels[0]["offsets"].dtype == np.int64))
    # (the widest levels of the fast path: one list, six optional structs and an optional leaf are def levels 0..9 — case 4 of
    # k_nested_emit's pack switch; its rep levels are always 1 bit)
    lv = build_path(((LIST, True),) + ((STRUCT, True),) * 6, True, 800, _long_lens(0), seed=114)
    add("long_fast_list_6_structs", lv, _long_cuts(lv, 800), "the fast path with rep_bits == 1 and def_bits == 4",
        _all(has_level_bits(1, 4), has_list_longer_than(two_windows), lambda levels, rows, cuts: is_fast_path(levels)))
    # ---- long lists on the generic path (k_nested_gen's parent search)
    lv = build_path(((LIST, True), (LIST, True)), True, 1600, _long_lens(0), seed=102)
    add("long_generic_top", lv, _long_cuts(lv, 1600), "a tile of inner lists with no top list starting in it",
        _all(has_list_longer_than(TILE, 0), child_tile_without_parent_start(1)))
    first_long = int(np.flatnonzero(_list_lengths(lv[0]) > TILE)[0])
    add("long_generic_top_row_pages", prefix(lv, first_long + 9), [1],
        "one top list of more than a tile of inner lists is one page",
        _all(one_row_pages_of_more_than(TILE), child_tile_without_parent_start(1)))
    # (a long list in the first and in the last row of the column: no row in front of the first window, none behind the last)
    for name, spec in (("list", ((LIST, True),)), ("list_list", ((LIST, True), (LIST, True)))):
        lv = build_path(spec, True, 5, lambda k, n, rng: np.array([12000, 0, 1, 0, 9000]) if k == 0 else rng.integers(0, 3, n), seed=120)
        add("long_ends_%s" % name, lv, [None, 2], "the first and the last row hold more than 2 windows of entries each",
            lambda levels, rows, cuts: min(_list_lengths(levels[0])[[0, -1]]) > two_windows)
    lv = build_path(((LIST, True), (LIST, True)), True, 1200, _long_lens(1), seed=103)
    add("long_generic_bottom", lv, [None, 500], "a tile of leaves with no inner list starting in it",
        _all(has_list_longer_than(two_windows, 1), child_tile_without_parent_start(2)))
    lv = build_path(((STRUCT, True), (LIST, True)), True, 1600, _long_lens(1), seed=104)
    add("long_generic_struct_list", lv, [None, 533], "a tile of leaves with no list starting in it (struct -> list)",
        _all(has_list_longer_than(two_windows, 1), child_tile_without_parent_start(2)))
    # ---- runs of empties at both levels of list -> list (required)
    lv = build_path(((LIST, True), (LIST, False)), True, 3000, _run_lens, seed=105, null_density=0.3)
    add("runs_of_empties", lv, [None] + _run_cuts(lv, 3000),
        "runs of >= 300 empty / null lists at both levels, pages that start and end inside one", pages_cut_inside_runs)
    # ---- depth
    mixed = ((LIST, True), (LIST, True), (STRUCT, True), (LARGE, False), (STRUCT, False), (LIST, True), (STRUCT, True))
    add("depth8_mixed", build_path(mixed, True, 400, _short, seed=106), [None, 97],
        "8 levels: list, list, struct, large-list (required), struct (required), list, struct, leaf", has_level_bits(3, 4))
    add("depth8_optional_lists", build_path(((LIST, True),) * 7, True, 400, _short, seed=107), [None, 97],
        "rep_bits == 3 and def_bits == 4", has_level_bits(3, 4))
    add("depth8_required_lists", build_path(((LIST, False),) * 7, False, 400, _short, seed=108), [None, 97],
        "rep_bits == 3 and def_bits == 3 with no optional level", has_level_bits(3, 3))
    add("depth8_required_structs", build_path(((STRUCT, False),) * 7, False, 5000, _short, seed=109), [None, 1234],
        "0 bits at depth 8", has_level_bits(0, 0))
    # ---- exact entry counts: uleb header steps (504 | 505, 65528 | 65529), L % 32, NE_CHUNK, TILE and neighbours
    for shape in ("list", "list_list"):
        for L in EXACT_L:
            add("exact_%s_%d" % (shape, L), exact_entries(L, shape, seed=200 + L % 97), [None], "L == %d" % L, one_page_of(L))
    # ---- many pages of just over one chunk: the chunk_row slots of neighbouring pages
    add("pages_just_over_a_chunk", just_over_a_chunk(12, 800, seed=110), [800],
        "12 pages of NE_CHUNK + 1 .. NE_CHUNK + 40 entries", every_page_just_over_a_chunk)
    # ---- more than 64 tiles in one page (nothing in the table is larger)
    for shape in ("list", "list_list"):
        add("tiles65_%s" % shape, exact_entries(MORE_THAN_64_TILES, shape, seed=111), [None],
            "one page of 64 * 4096 + 1 entries", one_page_of(MORE_THAN_64_TILES), big=True)
    # ---- validity_bit_offset on a list level and on the leaf
    for shape, spec in (("list", ((LIST, True),)), ("list_list", ((LIST, True), (LIST, True)))):
        for off in (3, 13):
            for k in (len(spec) - 1, len(spec)):
                lv = build_path(spec, True, 3000, _short, seed=112 + off, voff={k: off})
                add("voff_%s_level%d_%d" % (shape, k, off), lv, [None, 777],
                    "validity_bit_offset == %d at level %d" % (off, k), has_validity_offset(k, off))
    return cases


_CASES = None


def cases():
    """the table, built once and shared (its columns are never modified)"""
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


def case_names():
    return [c.name for c in cases()]


def by_name(name):
    return next(c for c in cases() if c.name == name)
