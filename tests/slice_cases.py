"""The case table of sliced Arrow arrays at the write boundary (a plain module: no fixtures, no tests).

A caller hands the writer slices: `validity_bit_offset`, a Boolean `values_bit_offset`, Binary `offsets` whose first
entry is not 0 (with `values` / `values_len` the whole buffer), a primitive `values` pointer `start * width` bytes into
its buffer.  One case is the rows of a slice, how the slice is presented, the write options, the kernel family it is
aimed at and the page codec its pages must reach.  `present(case, fill)` builds the buffers as the caller holds them:

  * validity: `start` bits in front of the slice; the pointer either stays (validity_bit_offset = start) or is advanced
    by start // 8 bytes (validity_bit_offset = start % 8).  The buffer ends with the byte of the slice's last bit: the
    library may read ceil((validity_bit_offset + rows) / 8) bytes from the pointer and not one more.
  * Boolean values: `bpos` bits in front of the slice, chosen independently of `start`; the same byte rule.
  * Binary: `start` parent rows in front and three behind; `offsets` is entries [start, start + rows] of the parent.
  * primitives: `start` parent rows in front and three behind, the pointer advanced by start * width bytes.

Poison: every validity / Boolean value bit outside the slice's bit range, spare bits of the last byte included, is
`fill`; primitive rows outside the slice hold a sentinel that occurs nowhere inside, Binary rows outside a string of
their own.  With both fills the row in front of a null row 0 is valid once and the row in front of a valid row 0 is
null once (the same at the end), which is what moves OneValue's first valid value, Dict's leading-null entry, RLE's
leading-null run and Freq's vote when an offset is off by one.  Inside the slice a null row never holds a valid row's
value (except in the run-level family, whose kernels look at raw runs), so a misread validity bit changes the page.

Families and the dispatch conditions that lead to their kernels (sb_encode.hip unless stated):

  plain_tiles      force_codec None: k_enc_emit_tiles, def_bits_tile; one tile = TILE_ROWS rows
  row_level        force_codec RLE / OneValue / Dict / Freq: k_enc_emit_pages<kind, codec>; forced Dict of <= 8-byte keys
                   with <= DL_CAP distinct values per page stays in dict_build_lds (sb_dict_lds.h), more of them, floats
                   and wider keys go to dict_build
  run_level        adaptive 4- / 8-byte values: k_enc_select_runs (<= RUNS_CAP raw runs per chunk), else k_enc_select_rle
  prim_dict_fused  adaptive 1- / 2- / 4-byte integers, BP_MIN_ROWS <= rows <= 65536 (bp_fits, pd_page_ok): k_enc_prim_dict
  binary           forced codecs: k_enc_emit_tiles / k_enc_emit_pages<-4|-8, codec>; adaptive pages of BP_MIN_ROWS ...
                   65536 rows: k_enc_bin_page (bp_page_ok), or with SB_BIN_FUSED=0 the k_enc_bin_hash -> k_enc_select ->
                   k_enc_bin_verify -> emit chain, which also takes the pages below BP_MIN_ROWS
  boolean          forced None / RLE / OneValue / LZ4 and adaptive (k_enc_select<0>, choose_bool)
  basic_blocks     default_compression LZ4 / Zstd / Snappy: k_enc_emit_lz4; blocks above 64 KiB of Snappy / Zstd / the
                   parallel LZ4 encoder go through k_enc_lz4_plan (the exact LZ4 parse never does: lz4_page_chunked)
  bitpack_patas    forced Bitpacking / DeltaBitpacking / Patas at a misaligned values pointer (no validity)
  long_pages       adaptive pages of >= SEL_BIG_ROWS (BIN_BIG_ROWS) rows: sb_select_big.h, sb_dict_big.h, sb_freq_big.h
  short_bitmaps    bitmaps shorter than the 8-byte load of bits32 / vword_issue, slices that end on a buffer's last bit
  host_memory      SB_MEM_HOST: the staged sizes are (offset + rows + 7) / 8, values_len and (rows + 1) * width

tests/test_slice_cases.py walks the table with the oracle alone; tests/test_gpu_write_slices.py sends it through the
device."""
from collections import OrderedDict

import numpy as np

from oracle import sbo as S
from tests import gen

TILE_ROWS = 4096            # sb_common.h
BP_MIN_ROWS, BP_MAX_ROWS = 512, 65536   # sb_encode.hip: bp_fits
DL_CAP = 2048               # sb_dict_lds.h
BIG_ROWS = 1 << 18          # sb_select_big.h: SEL_BIG_ROWS, and SB_BIN_BIG_ROWS for binary pages
MAX_ROWS = 70000            # no family but long_pages has more rows

I8, I16, I32, I64, U32 = S.T_I8, S.T_I16, S.T_I32, S.T_I64, S.T_U32
F32, F64, I128, I256, BOOL, BIN32, BIN64 = S.T_F32, S.T_F64, S.T_I128, S.T_I256, S.T_BOOL, S.T_BIN32, S.T_BIN64
NONE, LZ4, ZSTD, SNAPPY = S.NONE, S.LZ4, S.ZSTD, S.SNAPPY
RLE, DICT, ONEVALUE, FREQ, BITPACK, DELTABP, PATAS = S.RLE, S.DICT, S.ONEVALUE, S.FREQ, S.BITPACK, S.DELTABP, S.PATAS
WIDTH = dict(S.WIDTH)
NP_OF = dict(gen.NP_OF)
BINARY = (BIN32, BIN64)

FILLS = (0, 1)
OFFSETS = (1, 7, 8, 13, 63, 64, 65, 4099)    # 63, 64, 65 straddle the 8-byte load of bits32 / vword_issue
# (start, pointer advanced): below 8 the two presentations are the same
PRESENTATIONS = tuple((o, adv) for o in OFFSETS for adv in ((False, True) if o >= 8 else (False,)))
BOOL_VALUE_OFFSETS = (0, 8, 16, 3, 9, 13)    # byte aligned and not
EDGES = ((False, True), (True, False), (False, False), (True, True))   # (row 0 valid, last row valid)
TAIL_ROWS = 3
FAMILIES = ("plain_tiles", "row_level", "run_level", "prim_dict_fused", "binary", "boolean", "basic_blocks",
            "bitpack_patas", "long_pages", "short_bitmaps", "host_memory")


class Case:
    """rows of a slice + presentation + options + what it must reach.

    values: primitives: array of the type (wide integers: int64 limbs, shape (rows, width / 8)); Boolean: bool per row;
    Binary: list of bytes.  valid: bool per row or None.  codec: the codec of every page (a tuple: per page).  inner: the
    codec of the Dict pages' index block where the family names one.  kernels: names that profile_read() must show.
    fused: SB_BIN_FUSED of the context.  host: through SB_MEM_HOST.  decode: the blocks are not byte-pinned (Zstd, Snappy,
    the parallel LZ4 encoder): compared by decoding, def-level sections byte for byte.  readable: False for Patas pages of
    Float32, which neither the reference nor the oracle can read: written bytes only."""

    def __init__(self, family, name, ptype, values, valid, start, advance, opt, codec, kernels, bpos=0, inner=None,
                 fused="1", host=False, decode=False, lz4_exact=True, readable=True):
        self.family, self.name, self.ptype, self.values, self.valid = family, name, ptype, values, valid
        self.start, self.advance, self.bpos, self.opt, self.codec, self.inner = start, advance, bpos, opt, codec, inner
        self.kernels, self.fused, self.host, self.decode, self.lz4_exact = tuple(kernels), fused, host, decode, lz4_exact
        self.readable = readable
        self.rows = len(values)
        self.nullable = valid is not None
        self.kind = "bool" if ptype == BOOL else "bin" if ptype in BINARY else "prim"

    @property
    def voff(self):
        return self.start % 8 if self.advance else self.start

    def group(self):
        """cases of one group can share an encode_columns call"""
        return (self.fused, self.host, self.lz4_exact, opt_key(self.opt))


CASES = OrderedDict()


def opt_key(opt):
    return tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in opt.items()))


def families():
    out = OrderedDict((f, []) for f in FAMILIES)
    for c in CASES.values():
        out[c.family].append(c)
    return out


def add(family, name, *a, **kw):
    name = "%s/%s" % (family, name)
    assert name not in CASES, name
    CASES[name] = Case(family, name, *a, **kw)


# ---------------------------------------------------------------- presenting a case
def sentinel(ptype):
    """a row value that no case holds inside its slice"""
    if ptype in (I128, I256):
        return np.full(WIDTH[ptype] // 8, -0x5A5A5A5A5A5A5A5B, np.int64)
    if ptype in (F32, F64):
        return NP_OF[ptype](-12345.5)
    return np.array(-91 if WIDTH[ptype] == 1 else -23131, np.int64).astype(NP_OF[ptype])   # (unsigned: 2^32 - 23131)


SENTINEL_STRING = b"<outside the slice>"


def bitmap(bits, pos, fill):
    """`bits` at bit `pos` of a buffer of ceil((pos + len) / 8) bytes, every other bit = fill"""
    n = pos + len(bits)
    b = np.full((n + 7) // 8 * 8, bool(fill))
    b[pos:n] = bits
    return gen.pack_bits(b)


def present(case, fill):
    """(presented, compact).  presented: dict(ptype, nullable, rows, values, validity, offsets: what the pointers point to,
    as uint8 / offset arrays; values_bit_offset, validity_bit_offset; values_buf, values_skip, validity_buf,
    validity_skip: the whole buffers and how many bytes the pointers are into them).  compact: the same rows as a column
    with buffers of its own and no offsets (tests/gen.py's dict)."""
    c, rows = case, case.rows
    p = dict(ptype=c.ptype, nullable=c.nullable, rows=rows, offsets=None, values_bit_offset=0, validity_bit_offset=0,
             validity=None, validity_buf=None, validity_skip=0, values_skip=0)
    k = dict(ptype=c.ptype, nullable=c.nullable, rows=rows, validity=None, offsets=None)
    if c.valid is not None:
        p["validity_buf"] = bitmap(c.valid, c.start, fill)
        p["validity_skip"] = c.start // 8 if c.advance else 0
        p["validity_bit_offset"] = c.voff
        p["validity"] = p["validity_buf"][p["validity_skip"]:]
        k["validity"] = gen.pack_bits(c.valid)
    if c.kind == "bool":
        p["values_buf"] = bitmap(c.values, c.bpos, fill)
        p["values_bit_offset"] = c.bpos
        k["values"] = gen.pack_bits(c.values)
    elif c.kind == "bin":
        odt = np.int64 if c.ptype == BIN64 else np.int32
        parent = [SENTINEL_STRING] * c.start + list(c.values) + [SENTINEL_STRING] * TAIL_ROWS
        offs = np.zeros(len(parent) + 1, np.int64)
        np.cumsum([len(s) for s in parent], out=offs[1:])
        p["values_buf"] = np.frombuffer(b"".join(parent), np.uint8).copy()
        p["offsets"] = offs[c.start:c.start + rows + 1].astype(odt)
        own = offs[c.start:c.start + rows + 1] - offs[c.start]
        k["values"] = p["values_buf"][offs[c.start]:offs[c.start + rows]].copy()
        k["offsets"] = own.astype(odt)
    else:
        v = np.asarray(c.values)
        parent = np.empty((c.start + rows + TAIL_ROWS,) + v.shape[1:], v.dtype)
        parent[:] = sentinel(c.ptype)
        parent[c.start:c.start + rows] = v
        p["values_buf"] = parent.reshape(-1).view(np.uint8)
        p["values_skip"] = c.start * WIDTH[c.ptype]
        k["values"] = v.reshape(-1).copy()
    p["values"] = p["values_buf"][p["values_skip"]:]
    return p, k


def options(case):
    return S.make_options(**case.opt)


def oracle_write(case, p):
    """the oracle's pages for a presentation (gen.oracle_write passes no offsets)"""
    return S.write_column(p["ptype"], p["nullable"], p["rows"], p["values"], validity=p["validity"], offsets=p["offsets"],
                          options=options(case), values_bit_offset=p["values_bit_offset"],
                          validity_bit_offset=p["validity_bit_offset"])


def page_spans(metas):
    """(first byte, end) of every page"""
    ends = np.cumsum(np.asarray(metas)[:, 0].astype(np.int64))
    return list(zip((ends - np.asarray(metas)[:, 0].astype(np.int64)).tolist(), ends.tolist()))


def def_section_len(page, nullable):
    return 4 + int.from_bytes(bytes(page[:4]), "little") if nullable else 0


def bool_page_aligned(case, page_rows, k):
    """is page k's first value bit byte aligned?  Then a Basic page holds the bitmap's bytes as they stand
    (boolean/mod.rs:44-54) and the spare bits of its last byte are what follows the page in the buffer"""
    return (case.bpos + k * page_rows) % 8 == 0


# ---------------------------------------------------------------- rows
def validity(rng, rows, edges, density=0.8):
    ok = rng.random(rows) < density
    ok[0], ok[-1] = edges
    if rows > 2:
        ok[1], ok[-2] = not edges[0], not edges[1]   # the slice's own neighbours of its edge rows differ from them
    return ok


def typed(ptype, a):
    """integers `a` as rows of `ptype` (wide integers: sign-extended limbs)"""
    a = np.asarray(a, np.int64)
    if ptype in (I128, I256):
        v = np.empty((a.size, WIDTH[ptype] // 8), np.int64)
        v[:] = (a >> 63)[:, None]
        v[:, 0] = a
        return v
    return a.astype(NP_OF[ptype])


def with_garbage(a, ok, salt):
    """rows that are null get values of their own (1000 + ...: no valid row has them)"""
    if ok is None:
        return a
    a = np.array(a, np.int64)
    null = ~ok
    a[null] = 1000 + (np.arange(a.size)[null] * 7 + salt) % 19
    return a


def small(ptype):
    return 100 if WIDTH.get(ptype, 8) == 1 else 1000


def words(rng, rows, ok, uniq=40, top=None):
    """strings over `uniq` words (`top`: the share of the first word); null rows hold a string of their own"""
    vocab = [b"w%03d" % i * (1 + i % 3) for i in range(uniq)]
    ids = rng.integers(0, uniq, rows)
    if top is not None:
        ids[rng.random(rows) < top] = 0
    out = [vocab[i] for i in ids]
    if ok is not None:
        for r in np.flatnonzero(~ok):
            out[r] = b"~null%d~" % (r % 5)
    return out


def pres(k):
    return PRESENTATIONS[k % len(PRESENTATIONS)]


def tag(start, advance):
    return "at%d%s" % (start, "adv" if advance else "")


TNAME = {I8: "i8", I16: "i16", I32: "i32", I64: "i64", U32: "u32", F32: "f32", F64: "f64", I128: "i128", I256: "i256",
         BOOL: "bool", BIN32: "bin", BIN64: "lbin"}
CNAME = {NONE: "none", LZ4: "lz4", ZSTD: "zstd", SNAPPY: "snappy", RLE: "rle", DICT: "dict", ONEVALUE: "onevalue", FREQ: "freq",
         BITPACK: "bitpack", DELTABP: "deltabp", PATAS: "patas"}
TILES, BASIC = "k_enc_emit_tiles", "k_enc_emit_lz4"


def emit(kd, codec):
    return "k_enc_emit_pages<%d, %d>" % (kd, codec)


def kind_of(ptype):
    return 0 if ptype == BOOL else -4 if ptype == BIN32 else -8 if ptype == BIN64 else WIDTH[ptype]


# ---------------------------------------------------------------- the families
def build_plain_tiles():
    rng = np.random.default_rng(101)
    n = 0
    for ptype in (I8, I32, F64, I256):
        for start, adv in PRESENTATIONS:   # 5 pages of 1001 rows: row0 % 8 != 0 on pages 1 to 4
            ok = validity(rng, 5005, EDGES[n % 4])
            v = typed(ptype, with_garbage(rng.integers(0, small(ptype), 5005), ok, n))
            add("plain_tiles", "%s_%s" % (TNAME[ptype], tag(start, adv)), ptype, v, ok, start, adv,
                dict(max_page_size=1001, force_codec=NONE), NONE, [TILES])
            n += 1
        for start, adv in ((13, False), (4099, True)):   # one page of more than one tile
            rows = TILE_ROWS + 1001
            ok = validity(rng, rows, EDGES[n % 4])
            add("plain_tiles", "%s_two_tiles_%s" % (TNAME[ptype], tag(start, adv)), ptype,
                typed(ptype, rng.integers(0, small(ptype), rows)), ok, start, adv, dict(force_codec=NONE), NONE, [TILES])
            n += 1
    add("plain_tiles", "i32_not_nullable_at13", I32, typed(I32, rng.integers(0, 1000, 5005)), None, 13, False,
        dict(max_page_size=1001, force_codec=NONE), NONE, [TILES])


def build_row_level():
    rng = np.random.default_rng(102)
    n = 0
    for ptype in (I8, I16, I128, I256):
        for codec in (RLE, ONEVALUE, DICT, FREQ):
            for rep in range(2):
                start, adv = pres(n)
                rows = 2002
                ok = validity(rng, rows, EDGES[n % 4])
                if codec == ONEVALUE:
                    a = np.full(rows, 42)
                elif codec == FREQ:
                    a = np.where(rng.random(rows) < 0.93, 7, rng.integers(8, small(ptype), rows))
                elif codec == RLE:
                    a = np.repeat(rng.integers(0, small(ptype), rows // 5 + 1), 5)[:rows]
                else:
                    a = rng.integers(0, small(ptype), rows)
                v = typed(ptype, with_garbage(a, ok, n) if ptype != I8 else np.where(ok, a, 101 + np.arange(rows) % 19))
                add("row_level", "%s_%s_%s" % (CNAME[codec], TNAME[ptype], tag(start, adv)), ptype, v, ok, start, adv,
                    dict(max_page_size=1001, force_codec=codec), codec,
                    ["k_enc_freq_prep/finish"] if codec == FREQ else [emit(WIDTH[ptype], codec)])
                n += 1
    for ptype in (F32, F64):   # a NaN among the keys, float keys: the HBM dict_build
        for start, adv in ((13, False), (64, True), (65, False)):
            rows = 2002
            ok = validity(rng, rows, EDGES[n % 4])
            v = with_garbage(rng.integers(0, 50, rows), ok, n).astype(NP_OF[ptype])
            v[rng.random(rows) < 0.1] = np.nan
            add("row_level", "dict_nan_%s_%s" % (TNAME[ptype], tag(start, adv)), ptype, v, ok, start, adv,
                dict(max_page_size=1001, force_codec=DICT), DICT, [emit(WIDTH[ptype], DICT)])
            n += 1
    for ptype in (I16, I64):   # <= DL_CAP distinct values per page: dict_build_lds; more: dict_build
        for uniq in (DL_CAP, DL_CAP + 900):
            for start, adv in ((7, False), (4099, False)):
                rows = 2 * 4099
                ok = validity(rng, rows, EDGES[n % 4], density=0.95)
                a = 2000 + (np.arange(rows) * 7919) % uniq      # every key on every page (4099 rows > uniq)
                a = np.where(ok, a, 1000 + np.arange(rows) % 19)
                add("row_level", "dict_%dkeys_%s_%s" % (uniq, TNAME[ptype], tag(start, adv)), ptype, typed(ptype, a), ok, start,
                    adv, dict(max_page_size=4099, force_codec=DICT), DICT, [emit(WIDTH[ptype], DICT)])
                n += 1


def run_rows(rows, length, salt):
    return ((np.arange(rows) + salt) // length * 7919 + 13) % 65521


def build_run_level():
    rng = np.random.default_rng(103)
    rows = 65536 + 1001      # one 65536-row page and a short one
    types = (F64, I32, I64)
    for n, (start, adv) in enumerate(PRESENTATIONS):
        ptype = types[n % 3] if start != 13 else (F64 if not adv else I32)   # start 13: the types of the existing test
        ok = validity(rng, rows, EDGES[n % 4], density=0.85)
        # long runs (null rows hold their run's value: the kernel walks raw runs): k_enc_select_runs writes the RLE pages
        add("run_level", "runs37_%s_%s" % (TNAME[ptype], tag(start, adv)), ptype, typed(ptype, run_rows(rows, 37, n)), ok, start, adv,
            dict(max_page_size=65536, ratio=2.0, forbidden=(DICT, FREQ)), RLE,
            ["k_enc_select_runs<%d, %d>" % (WIDTH[ptype], 2 if ptype == F64 else 0)])
        # runs of 3 rows: more than RUNS_CAP raw runs per chunk, the page goes on to k_enc_select_rle
        ptype = types[(n + 1) % 3]
        add("run_level", "runs3_%s_%s" % (TNAME[ptype], tag(start, adv)), ptype, typed(ptype, run_rows(rows, 3, n)), ok, start, adv,
            dict(max_page_size=65536, ratio=1.1, forbidden=(DICT, FREQ, PATAS, BITPACK, DELTABP)), RLE,
            ["k_enc_select_rle<%d, %d>" % (WIDTH[ptype], 2 if ptype == F64 else 0)])
    ok = validity(rng, rows, (True, True), density=0.85)
    add("run_level", "runs37_i64_any_codec_at13", I64, typed(I64, run_rows(rows, 37, 5)), ok, 13, False,
        dict(max_page_size=65536, ratio=2.0), (RLE, DICT), ["k_enc_select_runs<8, 0>"])


def build_prim_dict_fused():
    rng = np.random.default_rng(104)
    n = 0
    for ptype, uniq in ((I8, 60), (I16, 12), (I32, 40)):
        for ps in (1001, 4099):
            for rep in range(5):
                start, adv = pres(n)
                rows = 2 * ps
                ok = validity(rng, rows, EDGES[n % 4])
                a = rng.integers(0, uniq, rows)
                a = np.where(ok, a, uniq + 1 + np.arange(rows) % 19)   # (fits Int8)
                add("prim_dict_fused", "%s_%d_%s" % (TNAME[ptype], ps, tag(start, adv)), ptype, typed(ptype, a), ok, start, adv,
                    dict(max_page_size=ps, ratio=2.0), DICT, ["k_enc_prim_dict"])
                n += 1
    add("prim_dict_fused", "i32_1001_not_nullable_at13", I32, typed(I32, rng.integers(0, 40, 2002)), None, 13, False,
        dict(max_page_size=1001, ratio=2.0), DICT, ["k_enc_prim_dict"])


def build_binary():
    rng = np.random.default_rng(105)
    n = 0
    for ptype in BINARY:
        kd = kind_of(ptype)
        for nullable in (True, False):
            shapes = [("none", dict(max_page_size=1001, force_codec=NONE), NONE, {}, [TILES], "1", 2002),
                      ("dict", dict(max_page_size=1001, force_codec=DICT), DICT, {}, [emit(kd, DICT)], "1", 2002),
                      ("onevalue", dict(max_page_size=1001, force_codec=ONEVALUE), ONEVALUE, dict(uniq=1), [emit(kd, ONEVALUE)], "1", 2002),
                      ("freq", dict(max_page_size=1001, force_codec=FREQ), FREQ, dict(top=0.93), ["k_enc_freq_prep/finish"], "1", 2002),
                      ("fused", dict(max_page_size=1001, ratio=2.0), DICT, {}, ["k_enc_bin_page"], "1", 2002),
                      ("chain", dict(max_page_size=1001, ratio=2.0), DICT, {}, ["k_enc_bin_hash", "k_enc_select<%d>" % kd, "k_enc_bin_verify"], "0", 2002),
                      ("short", dict(max_page_size=300, ratio=2.0), DICT, {}, ["k_enc_bin_hash", "k_enc_select<%d>" % kd], "1", 900)]
            for what, opt, codec, kw, kernels, fused, rows in shapes:
                for rep in range(2):
                    start, adv = pres(n)
                    ok = validity(rng, rows, EDGES[n % 4]) if nullable else None
                    add("binary", "%s_%s%s_%s" % (what, TNAME[ptype], "_nulls" if nullable else "", tag(start, adv)), ptype,
                        words(rng, rows, ok, **kw), ok, start, adv, opt, codec, kernels, fused=fused)
                    n += 1


def build_boolean():
    rng = np.random.default_rng(106)
    shapes = (("none", dict(force_codec=NONE), NONE, [TILES]), ("rle", dict(force_codec=RLE), RLE, [emit(0, RLE)]),
              ("onevalue", dict(force_codec=ONEVALUE), ONEVALUE, [emit(0, ONEVALUE)]),
              ("lz4", dict(default_compression=LZ4), LZ4, [BASIC]), ("adaptive", dict(ratio=1.5), RLE, ["k_enc_select<0>"]))
    n = 0
    for what, opt, codec, kernels in shapes:
        for bpos in BOOL_VALUE_OFFSETS:
            for ps in (1001, 1000):      # 1000: pages 1 and 2 start byte aligned too when bpos is
                start, adv = pres(n)
                rows = 2507              # pages end inside a byte
                ok = validity(rng, rows, EDGES[n % 4])
                if what == "onevalue":
                    b = ok.copy()        # valid rows true, null rows false
                elif what == "rle":
                    b = np.repeat(rng.random(rows // 40 + 1) < 0.5, 40)[:rows] ^ (~ok)    # runs; a null row breaks its run
                elif what == "adaptive":
                    b = np.repeat(rng.random(rows // 100 + 1) < 0.5, 100)[:rows]
                else:
                    b = rng.random(rows) < 0.5
                add("boolean", "%s_v%d_p%d_%s" % (what, bpos, ps, tag(start, adv)), BOOL, b, ok, start, adv,
                    dict(opt, max_page_size=ps), codec, kernels, bpos=bpos)
                n += 1
    for bpos in (8, 13):
        add("boolean", "none_v%d_not_nullable" % bpos, BOOL, rng.random(2507) < 0.5, None, 0, False,
            dict(force_codec=NONE, max_page_size=1000), NONE, [TILES], bpos=bpos)


def build_basic_blocks():
    rng = np.random.default_rng(107)
    n = 0
    for codec in (LZ4, ZSTD, SNAPPY):
        for what in ("i64", "bool", "bin", "lbin"):
            for rep in range(3):
                start, adv = pres(3 * n + rep + 3)
                rows = 2002
                ok = validity(rng, rows, EDGES[(n + rep) % 4])
                opt = dict(max_page_size=1001 if rep else 1000, default_compression=codec)
                name = "%s_%s_%s" % (CNAME[codec], what, tag(start, adv))
                if what == "i64":
                    v = typed(I64, with_garbage(np.repeat(rng.integers(0, 50, rows // 4 + 1), 4)[:rows], ok, n))
                    add("basic_blocks", name, I64, v, ok, start, adv, opt, codec, [BASIC], decode=codec != LZ4)
                elif what == "bool":
                    bpos = BOOL_VALUE_OFFSETS[(0 if rep == 0 else 3) + (n // 4 + rep) % 3]   # 1000-row pages: aligned
                    add("basic_blocks", name + "_v%d" % bpos, BOOL, rng.random(rows) < 0.2, ok, start, adv, opt, codec, [BASIC],
                        bpos=bpos, decode=codec != LZ4)
                else:
                    add("basic_blocks", name, BIN64 if what == "lbin" else BIN32, words(rng, rows, ok), ok, start, adv, opt, codec,
                        [BASIC], decode=codec != LZ4)
            n += 1
    # one page above 64 KiB: the exact LZ4 parse (one wave, u32 table), and the chunked plan of Snappy / Zstd / parallel LZ4
    rows = 9001
    for codec, exact, kernels in ((LZ4, True, [BASIC]), (LZ4, False, ["k_enc_lz4_plan"]), (SNAPPY, True, ["k_enc_lz4_plan"]),
                                  (ZSTD, True, [BASIC])):
        for start, adv in ((13, False), (65, True)):
            ok = validity(rng, rows, EDGES[n % 4])
            v = typed(I64, with_garbage(np.repeat(rng.integers(0, 50, rows // 4 + 1), 4)[:rows], ok, n))
            add("basic_blocks", "%s%s_72k_%s" % (CNAME[codec], "" if exact else "_parallel", tag(start, adv)), I64, v, ok, start, adv,
                dict(default_compression=codec), codec, kernels, decode=not (codec == LZ4 and exact), lz4_exact=exact)
            n += 1


def build_bitpack_patas():
    rng = np.random.default_rng(108)
    for start in (1, 13):
        for ptype in (I32, U32):
            add("bitpack_patas", "bitpack_%s_at%d" % (TNAME[ptype], start), ptype, typed(ptype, rng.integers(0, 5000, 256)), None,
                start, False, dict(max_page_size=128, force_codec=BITPACK), BITPACK, [emit(4, BITPACK)])
            add("bitpack_patas", "deltabp_%s_at%d" % (TNAME[ptype], start), ptype, typed(ptype, np.sort(rng.integers(0, 5000, 256))),
                None, start, False, dict(max_page_size=128, force_codec=DELTABP), DELTABP, [emit(4, DELTABP)])
        for ptype in (F32, F64):
            v = (rng.integers(0, 2000, 301) / 8.0).astype(NP_OF[ptype])
            add("bitpack_patas", "patas_%s_at%d" % (TNAME[ptype], start), ptype, v, None, start, False,
                dict(max_page_size=200, force_codec=PATAS), PATAS, [emit(WIDTH[ptype], PATAS)], readable=ptype != F32)


def build_long_pages():
    rng = np.random.default_rng(109)
    rows = BIG_ROWS + 13
    opt = dict(ratio=2.0)
    for n, (start, adv) in enumerate(((13, False), (4099, False), (4099, True))):
        ok = validity(rng, rows, EDGES[n % 4], density=0.9)
        add("long_pages", "rle_f64_%s" % tag(start, adv), F64, typed(F64, run_rows(rows, 37, n)), ok, start, adv,
            dict(ratio=2.0, forbidden=(DICT, FREQ)), RLE, ["k_sel_big_sec", "k_sel_big_decide", "k_rle_big"])
        a = np.where(ok, rng.integers(0, 3000, rows), 5000 + np.arange(rows) % 19)
        add("long_pages", "dict_i32_%s" % tag(start, adv), I32, typed(I32, a), ok, start, adv, opt, DICT,
            ["k_sel_big_sec", "k_dict_big_insert", "k_dict_big_idx", "k_dict_big_finish"])
        okf = validity(rng, rows, EDGES[n % 4], density=0.99)     # (the majority value has to fill 90 % of ALL rows)
        a = np.where(rng.random(rows) < 0.97, 7, rng.integers(10, 1 << 40, rows))
        a = np.where(okf, a, 1 + np.arange(rows) % 5)
        add("long_pages", "freq_i64_%s" % tag(start, adv), I64, typed(I64, a), okf, start, adv, opt, FREQ,
            ["k_sel_big_sec", "k_freq_big"])
    for n, (ptype, start, adv) in enumerate(((BIN32, 13, False), (BIN64, 4099, True))):
        ok = validity(rng, rows, EDGES[n % 4], density=0.9)
        add("long_pages", "dict_%s_%s" % (TNAME[ptype], tag(start, adv)), ptype, words(rng, rows, ok, uniq=300), ok, start, adv, opt,
            DICT, ["k_sel_big_sec", "k_dict_big_insert", "k_dict_big_finish"])


def build_short_bitmaps():
    rng = np.random.default_rng(110)
    n = 0
    # (rows, offset): fewer than 8 bytes of bitmap (the byte loop of bits32), exactly 8, a slice ending on the last bit
    shapes = [(r, o) for o in (1, 7) for r in (1, 7, 8, 9, 57)] + [(55, 1), (49, 7), (15, 1)]
    for rows, off in shapes:
        for what, ptype, opt, codec, kernels in (("none", I32, dict(force_codec=NONE), NONE, [TILES]),
                                                 ("rle", I64, dict(force_codec=RLE), RLE, [emit(8, RLE)]),
                                                 ("dict", I16, dict(force_codec=DICT), DICT, [emit(2, DICT)]),
                                                 ("bool_rle", BOOL, dict(force_codec=RLE), RLE, [emit(0, RLE)]),
                                                 ("bool_none", BOOL, dict(force_codec=NONE), NONE, [TILES])):
            ok = rng.random(rows) < 0.6
            ok[0], ok[-1] = EDGES[n % 4]
            if ptype == BOOL:
                add("short_bitmaps", "%s_%drows_at%d" % (what, rows, off), BOOL, rng.random(rows) < 0.5, ok, off, False, opt, codec,
                    kernels, bpos=(7, 1, 8)[n % 3])
            else:
                a = np.where(ok, np.arange(rows) // 3, 1000 + np.arange(rows) % 19)
                add("short_bitmaps", "%s_%drows_at%d" % (what, rows, off), ptype, typed(ptype, a), ok, off, False, opt, codec, kernels)
            n += 1


def build_host_memory():
    rng = np.random.default_rng(111)
    rows = 2002
    for n, (start, adv) in enumerate(((13, False), (65, True), (4099, False))):
        ok = validity(rng, rows, EDGES[n % 4])
        add("host_memory", "rle_f64_%s" % tag(start, adv), F64, typed(F64, with_garbage(np.repeat(rng.integers(0, 50, 401), 5)[:rows], ok, n)),
            ok, start, adv, dict(max_page_size=1001, force_codec=RLE), RLE, [emit(8, RLE)], host=True)
        add("host_memory", "none_bool_v%d_%s" % ((13, 8, 3)[n], tag(start, adv)), BOOL, rng.random(rows) < 0.5, ok, start, adv,
            dict(max_page_size=1001, force_codec=NONE), NONE, [TILES], bpos=(13, 8, 3)[n], host=True)
        add("host_memory", "adaptive_bin_%s" % tag(start, adv), BIN32, words(rng, rows, ok), ok, start, adv,
            dict(max_page_size=1001, ratio=2.0), DICT, ["k_enc_bin_page"], host=True)


for _build in (build_plain_tiles, build_row_level, build_run_level, build_prim_dict_fused, build_binary, build_boolean,
               build_basic_blocks, build_bitpack_patas, build_long_pages, build_short_bitmaps, build_host_memory):
    _build()
