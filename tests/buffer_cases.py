"""The case table of tests/test_gpu_buffers.py and its numpy-only helpers (no torch, no device: tests/test_buffer_cases.py
walks the same table on the CPU).

A case is a column (tests/gen.py's dict) and the oracle's write options for it.  Which option set applies to which type and
row count is stated here, by `applies`; nothing is found out by catching what the oracle throws.  pages_of(case) writes
the pages with the oracle and reads them back, once per process."""
import functools

import numpy as np

from oracle import sbo as S
from tests import gen

TILE_ROWS = 4096
PRIMS = (S.T_I8, S.T_I16, S.T_I32, S.T_U32, S.T_I64, S.T_F32, S.T_F64, S.T_I128, S.T_I256)
BINARIES = (S.T_BIN32, S.T_BIN64)
TYPES = PRIMS + (S.T_BOOL,) + BINARIES
TYPE_NAMES = {S.T_I8: "i8", S.T_I16: "i16", S.T_I32: "i32", S.T_U32: "u32", S.T_I64: "i64", S.T_F32: "f32", S.T_F64: "f64",
              S.T_I128: "i128", S.T_I256: "i256", S.T_BOOL: "bool", S.T_BIN32: "bin", S.T_BIN64: "lbin"}
ROWS = (1, 31, 32, 33, 129, 1000, 4095, 4096, 4097, 8193, 16896)   # a bitmap word holds 32 rows, a tile TILE_ROWS
ROWS_128 = (128, 4096, 4224, 16896)                                # Bitpacking / DeltaBitpacking: whole blocks of 128 rows
PAGE_SHARED, PAGE_TILE, PAGE_128 = 3000, 4096, 2944   # 3000: pages share validity words, value bases of 1- / 2- / 4-byte
                                                      # types are not 16-byte aligned


def width_of(ptype):
    """bytes per element of `values` (primitives) or of `offsets` (binary); 0 for Boolean"""
    return {S.T_BIN32: 4, S.T_BIN64: 8, S.T_BOOL: 0}.get(ptype) or S.WIDTH.get(ptype, 0)


class OptionSet:
    def __init__(self, name, opt, forced=None, types=TYPES, rows=None, pages=None, zero_values=False):
        self.name, self.opt, self.forced = name, opt, forced
        self.types, self.rows, self.pages, self.zero_values = types, rows, pages, zero_values

    def applies(self, ptype):
        return ptype in self.types

    def __repr__(self):
        return self.name


NOT_BINARY = PRIMS + (S.T_BOOL,)
NOT_BOOLEAN = PRIMS + BINARIES
OPTION_SETS = [
    OptionSet("adaptive", {}),
    OptionSet("ratio1.5", dict(ratio=1.5)),
    OptionSet("lz4", dict(default_compression=S.LZ4)),
    OptionSet("zstd", dict(default_compression=S.ZSTD)),
    OptionSet("snappy", dict(default_compression=S.SNAPPY)),
    OptionSet("rle", dict(force_codec=S.RLE), S.RLE, NOT_BINARY),
    OptionSet("dict", dict(force_codec=S.DICT), S.DICT, NOT_BOOLEAN),
    OptionSet("dict_rle", dict(force_codec=S.DICT, force_index_codec=S.RLE), S.DICT, NOT_BOOLEAN),
    OptionSet("freq", dict(force_codec=S.FREQ), S.FREQ, NOT_BOOLEAN),
    OptionSet("onevalue", dict(force_codec=S.ONEVALUE), S.ONEVALUE, PRIMS, zero_values=True),
    OptionSet("bitpack", dict(force_codec=S.BITPACK), S.BITPACK, (S.T_I32, S.T_U32), ROWS_128, (None, PAGE_128)),
    OptionSet("deltabp", dict(force_codec=S.DELTABP), S.DELTABP, (S.T_I32, S.T_U32), ROWS_128, (None, PAGE_128)),
    OptionSet("patas", dict(force_codec=S.PATAS), S.PATAS, (S.T_F64,)),
]
OPTION_SET = {o.name: o for o in OPTION_SETS}


def pagings(rows):
    """max_page_size (rows per page) values of a column of `rows` rows: one page; 3000; 4096 for columns of two tiles or more"""
    out = [None]
    if rows > PAGE_SHARED:
        out.append(PAGE_SHARED)
    if rows >= TILE_ROWS + 1:
        out.append(PAGE_TILE)
    return out


class Case:
    """name; col (gen's dict); opt (oracle write options, max_page_size included); forced (the codec every page must show)"""

    def __init__(self, name, col, opt, forced=None, claim=None):
        self.name, self.col, self.opt, self.forced, self.claim = name, col, opt, forced, claim
        self._written = None

    def __repr__(self):
        return self.name


def pages_of(case):
    """(pages, metas, want): the oracle's pages of the case and its own decode of them; computed once, never modified"""
    if case._written is None:
        pages, metas = gen.oracle_write(case.col, **case.opt)
        want = gen.oracle_read(case.col, pages, metas)
        for a in (pages, metas, want["values"], want["validity"], want["offsets"]):
            a.setflags(write=False)
        case._written = (pages, metas, want)
    return case._written


@functools.lru_cache(maxsize=None)
def make_column(ptype, rows, nullable, zero_values=False):
    """the column of every option set of (type, rows, nullable): shared, never modified"""
    nd = 0.2 if nullable else None
    if ptype == S.T_BOOL:
        col = gen.boolean(rows, null_density=nd, runs=5, seed=rows)
    elif ptype in BINARIES:
        col = gen.binary(rows, uniq=200, null_density=nd, large=ptype == S.T_BIN64, seed=rows)
    else:
        col = gen.prim(ptype, rows, uniq=200, runs=5, null_density=nd, seed=rows)
        if zero_values:
            col["values"] = np.zeros_like(col["values"])
    return col


_TABLE = {}


def table(ptype, oset, rows_filter=None):
    """the cases of one (type, option set): rows x nullable x paging"""
    key = (ptype, oset.name)
    if key not in _TABLE:
        out = []
        if oset.applies(ptype):
            for rows in (oset.rows or ROWS):
                for nullable in (False, True):
                    col = make_column(ptype, rows, nullable, oset.zero_values)
                    for mps in (oset.pages or pagings(rows)):
                        name = "%s-%s-r%d-%s-p%s" % (TYPE_NAMES[ptype], oset.name, rows, "null" if nullable else "req", mps or "one")
                        out.append(Case(name, col, dict(oset.opt, max_page_size=mps), oset.forced))
        _TABLE[key] = out
    cases = _TABLE[key]
    if rows_filter is not None:
        cases = [c for c in cases if c.col["rows"] in rows_filter]
    return cases


def groups():
    """[(type, option set)] with at least one case"""
    return [(t, o) for t in TYPES for o in OPTION_SETS if o.applies(t)]


def group_id(g):
    return "%s-%s" % (TYPE_NAMES[g[0]], g[1].name)


# ---------------------------------------------------------------- the string-length ladder
LADDER = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 64, 65)   # both sides of every width a string copy may pick
LADDER_ROWS = (18, 4097, 8193)
LADDER_SETS = [OptionSet("none", dict(force_codec=S.NONE), S.NONE, BINARIES),
               OptionSet("dict", dict(force_codec=S.DICT), S.DICT, BINARIES),
               OptionSet("freq", dict(force_codec=S.FREQ), S.FREQ, BINARIES),
               OptionSet("lz4", dict(force_codec=S.LZ4), S.LZ4, BINARIES),
               OptionSet("onevalue", dict(force_codec=S.ONEVALUE), S.ONEVALUE, BINARIES)]


def ladder_column(rows, variant, nullable, large, majority=False, one_value=False):
    """Non-null row number j (counted over the non-null rows) has LADDER[(j + variant) % 18] bytes, so the first non-null row
    has LADDER[variant] bytes; null rows are empty.  In a nullable column the first and the last row are null (rows > 18)
    and so is every 5th in between.  majority: two of three non-null rows, the first and the last excepted, hold ONE value
    of LADDER[variant] bytes (a Freq page's majority value).  one_value: every row holds it.
    Returns (column, (first length, last length))."""
    valid = None
    if nullable:
        valid = np.arange(rows) % 5 != 2
        if rows > len(LADDER):
            valid[0] = valid[-1] = False
    nn = np.arange(rows) if valid is None else np.flatnonzero(valid)
    j = np.arange(nn.size)
    top = np.ones(nn.size, bool) if one_value else (j % 3 != 0) & (j != nn.size - 1) if majority else np.zeros(nn.size, bool)
    lens = np.zeros(rows, np.int64)
    kind = np.zeros(rows, np.int64)
    lens[nn] = np.where(top, LADDER[variant], np.asarray(LADDER)[(j + variant) % len(LADDER)])
    kind[nn] = np.where(top, 7, j // len(LADDER)) % 5
    offs = np.zeros(rows + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    # byte p of a row is 0x30 + 16 * kind + p % 16: 5 kinds per length (a Dict page has repeats), never 0xA5, the guards' fill
    within = np.arange(offs[-1]) - np.repeat(offs[:-1], lens)
    data = (0x30 + np.repeat(kind, lens) * 16 + within % 16).astype(np.uint8)
    col = dict(ptype=S.T_BIN64 if large else S.T_BIN32, nullable=valid is not None, rows=rows, values=data,
               validity=None if valid is None else gen.pack_bits(valid), offsets=offs.astype(np.int64 if large else np.int32))
    return col, (int(lens[nn[0]]), int(lens[nn[-1]]))


_LADDER = {}


def ladder_table(ptype, oset):
    """the ladder cases of one (binary type, option set): rows x variant x nullable"""
    key = (ptype, oset.name)
    if key not in _LADDER:
        out = []
        for rows in LADDER_ROWS:
            for v in range(len(LADDER)):
                for nullable in (False, True):
                    col, claim = ladder_column(rows, v, nullable, ptype == S.T_BIN64, majority=oset.forced == S.FREQ,
                                               one_value=oset.forced == S.ONEVALUE)
                    name = "%s-ladder-%s-r%d-v%d-%s" % (TYPE_NAMES[ptype], oset.name, rows, LADDER[v], "null" if nullable else "req")
                    mps = None if rows <= PAGE_SHARED or oset.forced == S.ONEVALUE else PAGE_SHARED
                    out.append(Case(name, col, dict(oset.opt, max_page_size=mps), oset.forced, claim))
                    if mps is not None and v % 6 == 0:   # the same column in one page
                        out.append(Case(name + "-pone", col, dict(oset.opt, max_page_size=None), oset.forced, claim))
        _LADDER[key] = out
    return _LADDER[key]


def ladder_groups():
    return [(t, o) for t in BINARIES for o in LADDER_SETS]


def ladder_group_id(g):
    return "%s-ladder-%s" % (TYPE_NAMES[g[0]], g[1].name)


# ---------------------------------------------------------------- placement of the input
def place(pages, shift, junk):
    """(buffer, start): `pages` inside a longer array of `junk` bytes, starting `shift` bytes in (64 junk bytes behind)"""
    pages = np.asarray(pages, np.uint8)
    buf = np.full(shift + pages.size + 64, junk, np.uint8)
    buf[shift:shift + pages.size] = pages
    return buf, shift


def _gaps(n, gaps):
    g = np.resize(np.asarray(gaps, np.int64), n)
    assert n == 0 or (g.min() >= 1 and g.max() <= 37), "gaps are 1 to 37 junk bytes"
    return g


def scatter(pages, metas, gaps=(1, 37, 7, 16, 3, 13, 32, 5, 21), order="ascending", junk=0x5A):
    """(buffer, page_offsets): every page behind a gap of 1 to 37 junk bytes (`gaps`, cycled); ascending: the pages in the
    file's order; descending: the last page first"""
    pages = np.asarray(pages, np.uint8)
    lens = np.asarray(metas, np.uint64).reshape(-1, 2)[:, 0].astype(np.int64)
    n = lens.size
    assert int(lens.sum()) == pages.size and order in ("ascending", "descending")
    src = np.concatenate([[0], np.cumsum(lens)])
    g = _gaps(n, gaps)
    slots = list(range(n)) if order == "ascending" else list(range(n - 1, -1, -1))
    offs = np.zeros(n, np.uint64)
    buf = np.full(int(lens.sum() + g.sum()) + 64, junk, np.uint8)
    at = 0
    for k, p in enumerate(slots):
        at += int(g[k])
        offs[p] = at
        buf[at:at + lens[p]] = pages[src[p]:src[p + 1]]
        at += int(lens[p])
    return buf, offs


def gather(buf, metas, page_offsets):
    """the inverse of scatter: the pages back to back"""
    lens = np.asarray(metas, np.uint64).reshape(-1, 2)[:, 0].astype(np.int64)
    parts = [np.asarray(buf, np.uint8)[int(o):int(o) + int(n)] for o, n in zip(page_offsets, lens)]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


# ---------------------------------------------------------------- expected bytes
def mask_bits(bitmap, rows):
    """the first ceil(rows/8) bytes with the bits at positions >= rows cleared"""
    b = np.array(np.asarray(bitmap, np.uint8)[:(rows + 7) // 8], copy=True)
    if rows % 8:
        b[-1] &= (1 << (rows % 8)) - 1
    return b


def bitmap_bytes(rows):
    return ((rows + 31) // 32) * 4


def capacities(case):
    """(values, offsets, validity) capacities in bytes, exactly as include/strawboat_hip.h documents them (0: no buffer)"""
    col = case.col
    t, rows = col["ptype"], col["rows"]
    want = pages_of(case)[2]
    if t == S.T_BOOL:
        v = bitmap_bytes(rows)
    elif t in BINARIES:
        v = int(want["values"].size)
    else:
        v = rows * S.WIDTH[t]
    o = (rows + 1) * width_of(t) if t in BINARIES else 0
    return v, o, bitmap_bytes(rows) if col["nullable"] else 0
