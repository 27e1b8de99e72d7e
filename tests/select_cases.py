"""The case table of the adaptive selector's decision boundaries (a plain module: no fixtures, no tests).

Every case is a column built deterministically with numpy, the write options, and the codec the CPU oracle must choose
for each of its pages.  Cases come as neighbours (just below / at / just above a boundary); `neighbour` names the case
on the other side and `flips` says whether the oracle's codec differs between the two.  Where the oracle's choice is
the same on both sides (section B: the mechanics of the run-level kernel), `prop` is a numpy predicate of the column
that states why the case is where it claims to be.

tests/test_select_boundaries.py proves all of that with the oracle alone; tests/test_gpu_select_boundaries.py sends
the same columns through the device selectors.

The table is built around these constants of the device code and of the oracle (the CPU test reads them out of the
sources and compares: move one and the table has to move with it):
"""
from collections import OrderedDict, namedtuple

import numpy as np

from oracle import sbo as S
from tests import gen

RUNS_CAP = 640          # sb_select_runs.h: more raw runs in one chunk hand the page to the row-level kernel
WG, K_ROWS = 256, 16    # sb_common.h / sb_select_runs.h
CHUNK = WG * K_ROWS     # 4096 rows walked per iteration of the run-level kernel
SEL_LDS_SLOTS = 8192    # sb_select.h
KCAP = SEL_LDS_SLOTS // 4   # 2048 keys in the LDS key set (the all-ones key is kept beside it)
PD_CAP = 10240          # sb_encode.hip: distinct values k_enc_prim_dict takes
SAMPLE_COUNT, SAMPLE_SIZE = 10, 64   # sb_select.h and oracle/sbo_codecs.cpp
WHOLE_PAGE_MAX = SAMPLE_COUNT * (SAMPLE_SIZE + 1) - 1   # 649: N / SAMPLE_COUNT <= SAMPLE_SIZE, the trial sees the whole page
SPEC_SLACK = 256        # sb_select_runs.h: speculation stops when nrec * 4 > rows + 256

I8, I16, I32, I64, U8, U32, U64 = S.T_I8, S.T_I16, S.T_I32, S.T_I64, S.T_U8, S.T_U32, S.T_U64
F32, F64, I128, BOOL, BIN32, BIN64 = S.T_F32, S.T_F64, S.T_I128, S.T_BOOL, S.T_BIN32, S.T_BIN64
NONE, RLE, DICT, ONEVALUE, FREQ, BITPACK, DELTABP, PATAS = S.NONE, S.RLE, S.DICT, S.ONEVALUE, S.FREQ, S.BITPACK, S.DELTABP, S.PATAS
CODEC_NAME = {NONE: "None", S.LZ4: "LZ4", RLE: "RLE", DICT: "Dict", ONEVALUE: "OneValue", FREQ: "Freq", BITPACK: "Bitpacking",
              DELTABP: "DeltaBitpacking", PATAS: "Patas"}
TYPE_NAME = {I8: "Int8", I16: "Int16", I32: "Int32", I64: "Int64", U8: "UInt8", U32: "UInt32", U64: "UInt64", F32: "Float32",
             F64: "Float64", I128: "Int128", BOOL: "Boolean", BIN32: "Binary", BIN64: "LargeBinary"}
WIDTH = dict(S.WIDTH)
FLOATS = (F32, F64)
RLE_ONLY = (DICT, FREQ, BITPACK, DELTABP, PATAS)

Case = namedtuple("Case", "family name col opt expect neighbour flips prop")

CASES = OrderedDict()     # name -> Case
FUSED_FAMILIES = ("dict_fused", "binary")   # run with SB_BIN_FUSED=1 and 0, on contexts of their own


def names(codecs):
    return [CODEC_NAME.get(int(c), str(int(c))) for c in np.asarray(codecs).reshape(-1)]


def families():
    out = OrderedDict()
    for c in CASES.values():
        out.setdefault(c.family, []).append(c)
    return out


def opt_key(opt):
    return tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in opt.items()))


# ---------------------------------------------------------------- columns
def prim(ptype, a, valid=None):
    """integers / floats `a` (int64, uint64 or float64) as a column of `ptype`; `valid`: bool per row or None"""
    a = np.asarray(a)
    if ptype == I128:
        lo = a.astype(np.int64)
        v = np.empty((lo.size, 2), np.int64)
        v[:, 0] = lo
        v[:, 1] = lo >> 63      # sign extension
        v = v.reshape(-1)
    else:
        v = a.astype(gen.NP_OF[ptype])
    validity = None if valid is None else gen.pack_bits(valid)
    return dict(ptype=ptype, nullable=validity is not None, rows=int(a.shape[0]), values=v, validity=validity, offsets=None)


def raw(ptype, v, valid=None):
    """a column from values that already have the type's dtype (bit patterns matter: -0.0, NaN payloads, wide integers)"""
    validity = None if valid is None else gen.pack_bits(valid)
    rows = v.size // (WIDTH[ptype] // 8) if ptype == I128 else v.size
    return dict(ptype=ptype, nullable=validity is not None, rows=int(rows), values=v, validity=validity, offsets=None)


def boolean(b, valid=None):
    validity = None if valid is None else gen.pack_bits(valid)
    return dict(ptype=BOOL, nullable=validity is not None, rows=int(len(b)), values=gen.pack_bits(b), validity=validity, offsets=None)


def binary(strings, large, valid=None):
    lens = np.array([len(s) for s in strings], np.int64)
    offs = np.zeros(len(strings) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    data = np.frombuffer(b"".join(strings), np.uint8).copy()
    validity = None if valid is None else gen.pack_bits(valid)
    return dict(ptype=BIN64 if large else BIN32, nullable=validity is not None, rows=len(strings), values=data, validity=validity,
                offsets=offs.astype(np.int64 if large else np.int32))


def scatter(n, salt=0):
    """n different non-negative integers below 2^31 without order or runs (a fixed multiplicative shuffle)"""
    return (np.arange(1, n + 1, dtype=np.int64) * 2654435761 + salt * 40503) % ((1 << 31) - 1)


def cycle(n, uq, base=300, step=3):
    """n rows over exactly uq keys, no two neighbours equal (uq >= 2), unsorted"""
    return base + (np.arange(n, dtype=np.int64) % uq) * step


def add(family, name, col, expect, neighbour=None, flips=False, prop=None, **opt):
    assert name not in CASES, name
    opt.setdefault("ratio", 1.2)
    if col["ptype"] in FLOATS and family != "patas":     # (Patas is a family of its own: keep it out of the others' decisions)
        opt["forbidden"] = tuple(sorted(set(opt.get("forbidden", ())) | {PATAS}))
    opt.setdefault("forbidden", ())
    if isinstance(expect, int):
        expect = [expect]
    CASES[name] = Case(family, name, col, opt, list(expect), neighbour, flips, prop)


def pair(family, stem, sides, **opt):
    """neighbours: sides = [(suffix, column, expected codec), ...]; consecutive sides name each other, and flip
    when their expected codecs differ; a fourth element overrides options for that side"""
    for k, side in enumerate(sides):
        suffix, col, expect = side[:3]
        other = sides[k - 1] if k else sides[1]
        add(family, "%s %s" % (stem, suffix), col, expect, neighbour="%s %s" % (stem, other[0]),
            flips=np.atleast_1d(expect).tolist() != np.atleast_1d(other[2]).tolist(), **dict(opt, **(side[3] if len(side) > 3 else {})))


# ---------------------------------------------------------------- numpy properties (section B)
def row_bits(col):
    w = WIDTH[col["ptype"]]
    return np.ascontiguousarray(col["values"]).view(np.uint8).reshape(col["rows"], w)


def raw_run_starts(col):
    """True where a row's bits differ from the row before (row 0: True)"""
    b = row_bits(col)
    s = np.ones(col["rows"], bool)
    s[1:] = (b[1:] != b[:-1]).any(axis=1)
    return s


def raw_runs_per_chunk(col):
    """what step 1 of the run-level kernel counts: rows whose bits differ from the row before, plus the chunk's first row"""
    s = raw_run_starts(col).copy()
    s[::CHUNK] = True
    return [int(s[c:c + CHUNK].sum()) for c in range(0, col["rows"], CHUNK)]


def valid_rows(col):
    if col["validity"] is None:
        return np.ones(col["rows"], bool)
    return np.unpackbits(col["validity"], bitorder="little")[:col["rows"]].astype(bool)


def runs_without_a_valid_row(col):
    """first rows of the raw runs (as the kernel lists them: split at the chunk seams) that hold no valid row"""
    s = raw_run_starts(col).copy()
    s[::CHUNK] = True
    starts = np.flatnonzero(s)
    ends = np.r_[starts[1:], col["rows"]]
    ok = valid_rows(col)
    return [int(a) for a, b in zip(starts, ends) if not ok[a:b].any()]


def rle_records_at_chunk_ends(col):
    """RLE records closed by the end of every chunk (columns without nulls: one per change of value after row 0)"""
    assert col["validity"] is None
    ch = raw_run_starts(col).copy()
    ch[0] = False
    return [int(ch[:min(c + CHUNK, col["rows"])].sum()) for c in range(0, col["rows"], CHUNK)]


def speculation_stops_at(col):
    """index of the first chunk at whose end nrec * 4 > rows so far + 256, or None"""
    for k, nrec in enumerate(rle_records_at_chunk_ends(col)):
        if nrec * 4 > min((k + 1) * CHUNK, col["rows"]) + SPEC_SLACK:
            return k
    return None


def stays_in_the_run_kernel(col):
    return max(raw_runs_per_chunk(col)) <= RUNS_CAP


def chunk_runs_are(want):
    def prop(col):
        got = raw_runs_per_chunk(col)
        return got == list(want), "raw runs per chunk %s, wanted %s" % (got, list(want))
    return prop


def page_of_runs(chunk_rows, chunk_runs, change_on_first=True, base=100, keys=5):
    """a page whose chunk k has chunk_rows[k] rows in exactly chunk_runs[k] raw runs of near-equal length; with
    change_on_first the value changes on every chunk's first row, without it the chunk's first run continues the last
    run of the chunk before (the kernel counts it for the chunk either way)"""
    out, k = [], 0
    for ci, (n, r) in enumerate(zip(chunk_rows, chunk_runs)):
        edges = (np.arange(r + 1, dtype=np.int64) * n) // r
        ids = np.repeat(np.arange(r), np.diff(edges))
        first = k + 1 if (change_on_first or ci == 0) else k
        out.append(first + ids)
        k = first + r - 1
    ids = np.concatenate(out)
    return base + (ids % keys) * 7 + (ids % 2)      # neighbours always differ (parity), `keys` * 2 values at most


# ================================================================ A. choose_compressor, primitives
A_TYPES = (I32, I64, F64, I16, I128)       # a 4-byte and an 8-byte run-level type, Float64, and two row-level-only widths


def tn(t):
    return TYPE_NAME[t]


def build_onevalue():
    fam = "onevalue"
    for t in A_TYPES:
        n = 1000
        ok = np.ones(n, bool)
        ok[500] = False
        same = np.full(n, 7)
        other = same.copy()
        other[500] = 9
        # unique = 2 with the null slot counted: floats take Freq (999 / 1000); integers cannot (max 9 < 256), and RLE, which
        # does not see the null slot, beats Dict
        pair(fam, "%s all valid rows equal, one null slot" % tn(t),
             [("holding the same value", prim(t, same, ok), ONEVALUE),
              ("holding another value", prim(t, other, ok), FREQ if t in FLOATS else RLE)])
        add(fam, "%s all slots equal" % tn(t), prim(t, same), ONEVALUE)
        # Dict's ratio with one key on a page below 64 rows is N W / W: EQUAL to OneValue's N, and OneValue keeps the page
        add(fam, "%s 32 equal rows, Dict's ratio equals N too" % tn(t), prim(t, np.full(32, 7)), ONEVALUE)
    # r == tuple_count ends the loop: an all-zero 4-byte page of whole 128-row blocks bit-packs to one byte a block, so Bitpacking's
    # ratio (4 * 128 = 512 for any number of blocks) and DeltaBitpacking's (x 1.5) are above OneValue's N.  Only the break keeps
    # the page OneValue; with OneValue forbidden the later ratio shows.
    for t in (I32, U32):
        for n in (128, 256, 640):
            zeros = prim(t, np.zeros(n, np.int64))
            pair(fam, "%s %d zeros, DeltaBitpacking's ratio 768 is above N," % (tn(t), n),
                 [("the loop ends at OneValue", zeros, ONEVALUE), ("OneValue forbidden", zeros, DELTABP, dict(forbidden=(ONEVALUE,)))])
    for t, u in ((F32, np.uint32), (F64, np.uint64)):
        n = 1000
        f = gen.NP_OF[t]
        nan = np.full(n, np.nan, f)
        nan.view(u)[1::3] |= u(0x123)                  # a second payload
        nan.view(u)[2::3] |= u(1) << u(8 * f().itemsize - 1)   # and a sign
        add(fam, "%s all NaN, three bit patterns" % tn(t), raw(t, nan), ONEVALUE)
        z = np.zeros(n, f)
        z[::2] = -0.0
        add(fam, "%s +0.0 and -0.0 only" % tn(t), raw(t, z), ONEVALUE)
        z1 = z.copy()
        z1[999] = 1.0
        add(fam, "%s +0.0 and -0.0 and a single 1.0" % tn(t), raw(t, z1), FREQ, neighbour="%s +0.0 and -0.0 only" % tn(t), flips=True)


def build_freq_nulls():
    fam = "freq_nulls"
    for t in A_TYPES:
        for n in (1000, 10):
            v = 300 + (scatter(n) % 20000 if t == I16 else scatter(n))    # all different; RLE (nulls extend its runs) is next best
            nn = n * 9 // 10
            ok_at = np.ones(n, bool)
            ok_at[:nn] = False
            ok_at = np.roll(ok_at, n // 3)                                # nulls in the middle, valid rows on both ends
            ok_below = ok_at.copy()
            ok_below[np.flatnonzero(~ok_at)[0]] = True
            pair(fam, "%s N=%d nulls" % (tn(t), n),
                 [("%d (one fewer than 0.9 N)" % (nn - 1), prim(t, v, ok_below), RLE),
                  ("%d (0.9 N in double arithmetic)" % nn, prim(t, v, ok_at), FREQ)], ratio=1.5)


def majority_column(t, n, minority_rows, minority_values=None, valid=None, major=1000):
    a = np.full(n, major, np.int64)
    minority_rows = np.asarray(minority_rows)
    a[minority_rows] = 2000 + np.arange(minority_rows.size) if minority_values is None else minority_values
    return prim(t, a, valid)


def build_freq_majority():
    fam = "freq_majority"

    def both(t, stem, n, rows_at, rows_below, values=None, valid=None, below=DICT):
        # at: exactly ceil(0.9 N) rows hold the majority value -> Freq; one more minority row -> Dict takes the page
        assert n - len(rows_at) == -(-9 * n // 10) and len(rows_below) == len(rows_at) + 1
        va = None if values is None else values[:len(rows_at)]
        vb = None if values is None else values[:len(rows_below)]
        pair(fam, "%s majority %s" % (tn(t), stem),
             [("%d/%d" % (n - len(rows_below), n), majority_column(t, n, rows_below, vb, valid), below),
              ("%d/%d" % (n - len(rows_at), n), majority_column(t, n, rows_at, va, valid), FREQ)])

    for t in A_TYPES:
        n = 1000
        both(t, "minority at the front", n, np.arange(100), np.arange(101))
        both(t, "minority at the back", n, np.arange(900, 1000), np.arange(899, 1000))
        both(t, "minority alternating with the majority at the front", n, np.arange(100) * 2, np.arange(101) * 2)
        one = np.full(101, 5000)
        both(t, "minority one value in one run across a wave's rows", n, np.arange(470, 570), np.arange(470, 571), values=one)
        ok = np.ones(n, bool)
        ok[200:500] = False                       # 300 of the majority's rows are null slots: the oracle counts them
        both(t, "partly in null slots, minority at the back", n, np.arange(900, 1000), np.arange(899, 1000), valid=ok)
        n = 1600                                  # one minority row in every 16-row thread segment
        seg = np.arange(100) * 16 + 5
        both(t, "minority one per 16-row segment", n, np.r_[seg, 1599 - np.arange(60) * 16], np.r_[seg, 1599 - np.arange(61) * 16],
             below=RLE if t == I16 else DICT)   # (2-byte values: one index byte a row leaves Dict at 1.6, the sampled RLE trial is above)
        # a minority run LONGER than the majority's runs (the run-length-weighted vote: a lane's / a partial vote's majority count
        # is outweighed and the candidate swaps): ten majority runs of 90 rows, eight single minority rows and one minority run of 92
        n = 1000
        lay, vals, pos = [], [], 0
        for k in range(10):
            pos += 90
            if k == 1:                                     # after the second (short) majority run: the long minority run
                lay.append(pos + np.arange(92))
                vals.append(np.full(92, 5000))
                pos += 92
            elif k < 9:
                lay.append(np.array([pos]))
                vals.append(np.array([6000 + k]))
                pos += 1
        assert pos == n
        rows, vals = np.concatenate(lay), np.concatenate(vals)
        extra = 273 + 5                                    # one more minority row inside the third majority run
        both(t, "in runs of 90, one minority run of 92 rows", n, rows, np.r_[rows, extra], values=np.r_[vals, 7000])
        # the same across two chunks of the run-level kernel: lane 0 holds a majority run of 90 rows from chunk 0 when a minority run
        # of 410 rows is its run in chunk 1
        n = 2 * CHUNK
        head = np.arange(9) * 91 + 90                      # nine single minority rows between majority runs of 90 at the front
        rows = np.r_[head, CHUNK + np.arange(410), CHUNK + 2000 + np.arange(400)]
        vals = np.r_[6000 + np.arange(9), np.full(410, 5000), np.full(400, 5001)]
        both(t, "a minority run of 410 rows first in the second chunk", n, rows, np.r_[rows, 3000], values=np.r_[vals, 7000])
    for t in (I32, I64, F64):                     # one minority block in every 4096-row chunk (the run-level kernel's vote)
        n = 10 * CHUNK
        rows, vals = [], []
        for c in range(10):
            m = 410 if c < 6 else 409
            rows.append(c * CHUNK + 1800 + np.arange(m))
            vals.append(np.full(m, 100000 + c))
        rows, vals = np.concatenate(rows), np.concatenate(vals)
        both(t, "minority one block per 4096-row chunk", n, rows, np.r_[rows, 5], values=np.r_[vals, 77777])


def build_freq_max():
    fam = "freq_max"
    n = 1000

    def col(t, top, valid=None, major=5, at=999):
        a = np.full(n, major, np.int64)
        a[950:] = 10 + np.arange(50)              # 95 % majority, 50 small values, and the page's maximum
        a[at] = top
        return prim(t, a, valid)

    for t in (I32, U32, I64, U64, I16, I128):
        pair(fam, "%s 95 %% majority, maximum" % tn(t), [("255", col(t, 255), DICT), ("256", col(t, 256), FREQ)])
        ok = np.ones(n, bool)
        ok[999] = False
        add(fam, "%s the only value >= 256 sits in a null slot" % tn(t), col(t, 256, ok), FREQ,
            neighbour="%s 95 %% majority, maximum 255" % tn(t), flips=True)
    for t in FLOATS:                               # no maximum condition for floats
        add(fam, "%s 95 %% majority, maximum 60.0" % tn(t), col(t, 60), FREQ)
    for t in (I64, I32, I128):
        a = np.full(n, -5, np.int64)
        a[950:] = -1000 - np.arange(50)
        add(fam, "%s all negative, 95 %% majority" % tn(t), prim(t, a), DICT)
    a = np.full(n, 5, np.uint64)
    a[950:] = 10 + np.arange(50, dtype=np.uint64)
    a[999] = np.uint64(1) << np.uint64(63)         # as_i64(max) is negative
    add(fam, "UInt64 95 % majority, maximum 2^63", prim(U64, a), DICT, neighbour="UInt64 95 % majority, maximum 256", flips=True)
    a[999] = (np.uint64(1) << np.uint64(63)) - np.uint64(1)
    add(fam, "UInt64 95 % majority, maximum 2^63 - 1", prim(U64, a), FREQ, neighbour="UInt64 95 % majority, maximum 2^63", flips=True)
    a = np.full(n, 5, np.int64)
    a[950:] = 10 + np.arange(50)
    a[999] = 1 << 31                               # UInt32's top bit: as_i64 is positive
    add(fam, "UInt32 95 % majority, maximum 2^31", prim(U32, a), FREQ)
    # Int128: max.as_i64() is the low 64 bits of the largest value
    w = prim(I128, col(I64, 255)["values"])
    w["values"][2 * 999 + 1] = 1                   # 2^64 + 255: the maximum, whose low word is 255
    add(fam, "Int128 maximum 2^64 + 255 (low word 255)", w, DICT)
    w = prim(I128, col(I64, 256)["values"])
    w["values"][2 * 999 + 1] = 1
    add(fam, "Int128 maximum 2^64 + 256 (low word 256)", w, FREQ, neighbour="Int128 maximum 2^64 + 255 (low word 255)", flips=True)
    a = np.full(n, 5, np.int64)
    a[950:] = 10 + np.arange(50)
    a[999] = 127
    add(fam, "Int8 95 % majority never takes Freq", prim(I8, a), DICT)
    a[999] = 255
    add(fam, "UInt8 95 % majority never takes Freq", prim(U8, a), DICT)


def build_dict_limit():
    fam = "dict_limit"
    for t in A_TYPES:
        uq = 1000
        pair(fam, "%s unique * 3 =" % tn(t),
             [("N - 1", prim(t, cycle(3001, uq)), DICT), ("N", prim(t, cycle(3000, uq)), NONE),
              ("N + 1", prim(t, cycle(2999, uq)), NONE)], ratio=1.1)
        # null slots with values of their own count as keys
        a = cycle(3001, uq)
        ok = np.ones(3001, bool)
        ok[1500] = False
        b = a.copy()
        b[1500] = 299                              # a 1001st key, in a null slot only
        pair(fam, "%s unique * 3 = N - 1, null slot" % tn(t),
             [("with a key of the page", prim(t, a, ok), DICT), ("with a key of its own", prim(t, b, ok), NONE)], ratio=1.1)
        add(fam, "%s N=1" % tn(t), prim(t, [300]), NONE)      # OneValue's ratio is N = 1: not above the option
        add(fam, "%s N=2, two keys" % tn(t), prim(t, [300, 301]), NONE)
        add(fam, "%s N=3, two keys" % tn(t), prim(t, [300, 301, 300]), NONE)
        add(fam, "%s N=4, two keys" % tn(t), prim(t, [300, 301, 300, 301]), NONE)
        pair(fam, "%s two keys alternating," % tn(t),
             [("N=6", prim(t, cycle(6, 2)), NONE), ("N=7", prim(t, cycle(7, 2)), DICT)])


def build_dict_width():
    fam = "dict_width"
    for t in A_TYPES + (U32, U64):
        # bits_needed(unique) / 8 bytes per index: 0 up to 127 keys, 1 from 128 on, and the ratio falls across 6.0
        pair(fam, "%s N=1024 distinct keys" % tn(t),
             [("127", prim(t, cycle(1024, 127)), DICT), ("128", prim(t, cycle(1024, 128)), NONE)], ratio=6.0)


def build_dict_overflow():
    fam = "dict_overflow"
    n = 8192
    for t in (I64, U64, F64):
        # every row starts a raw run: the row-level kernel's key set
        pair(fam, "%s N=8192 distinct keys" % tn(t), [("2048 (the key set is full)", prim(t, cycle(n, KCAP)), DICT),
                                                     ("2049 (it overflows)", prim(t, cycle(n, KCAP + 1)), DICT)])
        pair(fam, "%s N=8192 distinct keys" % tn(t), [("2730 (unique * 3 = N - 2)", prim(t, cycle(n, 2730)), DICT),
                                                     ("2731 (unique * 3 = N + 1)", prim(t, cycle(n, 2731)), NONE)])
        # runs of 32 rows: the run-level kernel's key set
        ids = np.arange(65536, dtype=np.int64) // 32
        split = ids.copy()
        split[-16:] = 2048
        pair(fam, "%s N=65536 in runs of 32, distinct keys" % tn(t),
             [("2048", prim(t, 300 + (ids * 7919) % 100003), DICT), ("2049", prim(t, 300 + (split * 7919) % 100003), DICT)], forbidden=(RLE,))


def build_dict_allones():
    fam = "dict_allones"
    n = 8192

    def col(t, uq):
        a = cycle(n, uq)
        if t == F64:
            v = a.astype(np.float64)
            v[a == 300] = np.nan                   # (the oracle's key of every NaN is all ones; the device has one quiet NaN)
            return raw(t, v)
        if t == U64:
            v = a.astype(np.uint64)
            v[a == 300] = np.uint64(0xFFFFFFFFFFFFFFFF)
            return raw(t, v)
        a[a == 300] = -1
        return prim(t, a)

    for t in (I64, U64, F64):
        pair(fam, "%s N=8192 distinct keys, the all-ones key among them:" % tn(t),
             [("2730", col(t, 2730), DICT), ("2731", col(t, 2731), NONE)])
        pair(fam, "%s N=8192 the all-ones key and" % tn(t),
             [("2047 others", col(t, KCAP), DICT), ("2048 others (the table is full, the key beside it)", col(t, KCAP + 1), DICT),
              ("2049 others (the table overflows)", col(t, KCAP + 2), DICT)])


def build_dict_fused():
    fam = "dict_fused"
    n = 32768
    for t in (I32, U32, I16):
        base, step = (-5000, 1) if t == I16 else (300, 150000)     # (4-byte values spread over 31 bits: Bitpacking stays out)
        pair(fam, "%s N=32768 distinct keys" % tn(t),
             [("10240 (PD_CAP)", prim(t, cycle(n, PD_CAP, base, step)), DICT), ("10241", prim(t, cycle(n, PD_CAP + 1, base, step)), DICT)], ratio=1.1)
        pair(fam, "%s N=32768 distinct keys" % tn(t),
             [("10922 (unique * 3 = N - 2)", prim(t, cycle(n, 10922, base, step)), DICT),
              ("10923 (unique * 3 = N + 1)", prim(t, cycle(n, 10923, base, step)), NONE)], ratio=1.1)
        pair(fam, "%s N=1024 distinct keys" % tn(t),
             [("127, fused", prim(t, cycle(1024, 127)), DICT), ("128, fused", prim(t, cycle(1024, 128)), NONE)], ratio=6.0)


def build_strict_order():
    fam = "strict_order"
    for t in A_TYPES:
        w = WIDTH[t]
        # whole-page RLE trial on 600 rows: 600 W / (runs (4 + W)) is exactly 4.0
        runs = 600 * w // (4 * (4 + w))
        assert 600.0 * w / (runs * (4 + w)) == 4.0

        def col(r):
            edges = (np.arange(r + 1) * 600) // r
            return prim(t, 300 + (np.repeat(np.arange(r), np.diff(edges)) % 9) * 11)
        pair(fam, "%s 600 rows, RLE ratio against the option 4.0:" % tn(t),
             [("%d runs (above)" % (runs - 1), col(runs - 1), RLE), ("%d runs (equal)" % runs, col(runs), NONE)],
             ratio=4.0, forbidden=(DICT, FREQ))
        # two values in two runs of 256: Dict's ratio 512 W / (2 W + 8) equals RLE's 512 W / (2 (4 + W)); the order decides
        two = prim(t, np.repeat([300, 400], 256))
        pair(fam, "%s 512 rows, two runs, Dict and RLE tie," % tn(t),
             [("Freq forbidden", two, DICT), ("Freq and Dict forbidden", two, RLE, dict(forbidden=(DICT, FREQ)))], forbidden=(FREQ,))
    for t in (I32, U32):
        # RLE against Bitpacking.  An exact tie does not exist: a whole-page trial has at most 5 blocks of 128 rows and a sampled
        # one exactly 5, so Bitpacking's size (blocks + 16 * sum of widths) is a multiple of 8 only with 8 blocks, RLE's always.
        # Nearest neighbours, 512 rows of 0 / 1 (68 bytes bit-packed): 8 runs are 64 bytes of RLE, 9 runs are 72.
        def col01(r):
            edges = (np.arange(r + 1) * 512) // r
            return prim(t, np.repeat(np.arange(r) % 2, np.diff(edges)))
        pair(fam, "%s 512 rows of 0 / 1, RLE against 68 bytes of Bitpacking:" % tn(t),
             [("8 runs (64 bytes)", col01(8), RLE), ("9 runs (72 bytes)", col01(9), BITPACK)], forbidden=(DICT, FREQ, DELTABP))
        # DeltaBitpacking is Bitpacking's ratio x 1.5 on the same sorted page: 512 rows below 2^20, 4 blocks of 1 + 16 * 20 bytes
        srt = prim(t, (1 << 19) + np.arange(512) * 1000)
        bp = 2048.0 / (4 * (1 + 16 * 20))
        pair(fam, "%s 512 sorted rows, DeltaBitpacking's ratio" % tn(t),
             [("equals the option", srt, NONE), ("is above the option", srt, DELTABP, dict(ratio=float(np.nextafter(bp * 1.5, 0.0))))],
             ratio=bp * 1.5)
        add(fam, "%s 512 sorted rows, option between Bitpacking's ratio and x 1.5" % tn(t), srt, DELTABP, ratio=2.0)
        add(fam, "%s 512 sorted rows, option below Bitpacking's ratio" % tn(t), srt, DELTABP, ratio=1.2)


def build_sampling():
    fam = "sampling"
    for t in (I32, I64, F64, I16, I128):              # (Int16 / Int128: the row-level choose_prim stages its own samples)
        w = WIDTH[t]
        at640 = 640.0 * w / (10 * (4 + w))
        at649 = 649.0 * w / (10 * (4 + w))
        opt = (at640 + at649) / 2      # a trial over 640 rows (whole page or sample) stays below, one over 649 rows is above
        for n in (640, 649, 650, 651, 656, 657, 1289):
            sep = n // SAMPLE_COUNT
            # one value per sampling range (the last one takes the remainder): ten runs wherever the sample windows fall
            a = 300 + np.minimum(np.arange(n) // sep, SAMPLE_COUNT - 1) * 3
            want = RLE if (n <= WHOLE_PAGE_MAX and n > 640) else NONE
            for seed in (1, 2, 3):
                add(fam, "%s N=%d one run per sampling range, seed %d" % (tn(t), n, seed), prim(t, a), want,
                    neighbour=None if n not in (649, 650) else "%s N=%d one run per sampling range, seed %d" % (tn(t), 1299 - n, seed),
                    flips=n in (649, 650), ratio=opt, forbidden=(DICT, FREQ), rng_seed=seed)
        # the other direction: a value of its own in the last row of every 65-row range.  The whole-page trial of 649 rows sees
        # 19 runs; the sample of 650 rows (10 windows of 64 rows at offset 0 of their 65 rows) sees one run
        for seed in (1, 2, 3):
            def col(n):
                a = np.full(n, 300)
                a[64::65] = 900 + np.arange(len(a[64::65]))
                return prim(t, a)
            pair(fam, "%s a row of its own every 65 rows, seed %d," % (tn(t), seed),
                 [("N=649", col(649), NONE), ("N=650", col(650), RLE)], ratio=50.0 if w > 2 else 30.0, forbidden=(DICT, FREQ), rng_seed=seed)
        # seeds that decide: every 128-row range starts with 64 equal rows and goes on in runs of 4, so a window's run count grows
        # with its offset.  The windows are placed with the generator the oracle and the device share (sbo_sample_rand), the
        # sample's runs counted here with numpy (page 0's seed is mix64 of the option's); the option lies between the ratios of seed 1 and seed 2.
        n = 1289
        sep, rem = n // SAMPLE_COUNT, n % SAMPLE_COUNT
        i = np.arange(n)
        rng_of = np.minimum(i // sep, SAMPLE_COUNT - 1)
        within = i - rng_of * sep
        a = np.where(within < 64, 300 + rng_of * 3, 1000 + (within // 4) % 2)

        def sampled_ratio(seed):
            offs = [int(S.lib().sbo_sample_rand(S.lib().sbo_mix64(seed), 0, RLE, si, (sep + rem if si == SAMPLE_COUNT - 1 else sep) - SAMPLE_SIZE))
                    for si in range(SAMPLE_COUNT)]
            smp = np.concatenate([a[si * sep + o:si * sep + o + SAMPLE_SIZE] for si, o in enumerate(offs)])
            return 640.0 * w / ((1 + int((smp[1:] != smp[:-1]).sum())) * (4 + w))
        opt = (sampled_ratio(1) + sampled_ratio(2)) / 2
        wants = [RLE if sampled_ratio(seed) > opt else NONE for seed in (1, 2, 6)]
        assert len(set(wants)) == 2, "the seeds were meant to decide"
        for seed, want in zip((1, 2, 6), wants):
            add(fam, "%s N=1289 runs that depend on the window offsets, seed %d" % (tn(t), seed), prim(t, a), want,
                neighbour="%s N=1289 runs that depend on the window offsets, seed %d" % (tn(t), 2 if seed == 1 else 1),
                flips=seed in (1, 2), ratio=opt, forbidden=(DICT, FREQ, BITPACK, DELTABP), rng_seed=seed)


def build_bitpack():
    fam = "bitpack"
    for t in (I32, U32):
        def col(n, neg_at=None, null_at=None):
            a = (np.arange(n, dtype=np.int64) * 7919) % 1000
            ok = None
            if neg_at is not None and t == I32:
                a[neg_at] = -3
            if null_at is not None:
                ok = np.ones(n, bool)
                ok[null_at] = False
            return prim(t, a, ok)
        opt = dict(ratio=2.5)
        pair(fam, "%s values below 1000, N =" % tn(t),
             [("4095 (N % 128 = 127)", col(4095), NONE), ("4096 (N % 128 = 0)", col(4096), BITPACK), ("4097 (N % 128 = 1)", col(4097), NONE)], **opt)
        add(fam, "%s N=4096 with a null (Bitpacking does not mind)" % tn(t), col(4096, null_at=7), BITPACK, **opt)
        if t == I32:
            for where, at in (("row 0", 0), ("the last row", 4095)):
                add(fam, "Int32 N=4096 one negative value at %s" % where, col(4096, neg_at=at), NONE,
                    neighbour="Int32 values below 1000, N = 4096 (N % 128 = 0)", flips=True, **opt)
            add(fam, "Int32 N=4096 one negative value in a null slot", col(4096, neg_at=2000, null_at=2000), NONE,
                neighbour="Int32 values below 1000, N = 4096 (N % 128 = 0)", flips=True, **opt)
    # the same bits: UInt32 with its top bit set is eligible, Int32 is negative.  512 rows (a whole-page trial): three blocks of
    # 8 bits and one of 32
    a = (np.arange(512, dtype=np.int64) * 37) % 200
    a[300] = 1 << 31
    pair(fam, "512 rows below 200 and one value of 2^31 as",
         [("UInt32", prim(U32, a), BITPACK), ("Int32", prim(I32, a.astype(np.uint32).view(np.int32).astype(np.int64)), NONE)], ratio=1.5)
    for t in (I64, I16):                           # Bitpacking is a 4-byte codec
        add(fam, "%s N=4096 values below 1000 never take Bitpacking" % tn(t), prim(t, (np.arange(4096, dtype=np.int64) * 7919) % 1000),
            DICT if t == I64 else NONE, ratio=2.5)


def build_deltabp():
    fam = "deltabp"
    n = 8192
    for t in (I32, U32):
        for shape, base, other in (("distinct", np.arange(n, dtype=np.int64) * 3 + 1, BITPACK),       # row-level kernel
                                   ("runs of 7", np.arange(n, dtype=np.int64) // 7 + 1024, RLE)):     # run-level kernel
            stem = "%s sorted %s," % (tn(t), shape)
            srt = "%s as it is" % stem
            add(fam, srt, prim(t, base), DELTABP, forbidden=(DICT,), ratio=1.5,
                prop=None if shape == "distinct" else lambda c: (stays_in_the_run_kernel(c), "more than RUNS_CAP raw runs in a chunk"))
            for r in (1, 15, 16, 17, 1023, 1024, 4095, 4096, 4097, n - 1):
                a = base.copy()
                a[r] = a[r - 1] - 1                # (positive values: a negative one takes the page out on min < 0 first)
                add(fam, "%s one step down at row %d" % (stem, r), prim(t, a), other, neighbour=srt, flips=True, forbidden=(DICT,), ratio=1.5)
            a = base.copy()
            a[4096] = a[4095]
            a[1] = a[0]
            add(fam, "%s equal neighbours" % stem, prim(t, a), DELTABP, neighbour=srt, forbidden=(DICT,), ratio=1.5)
            for r in (0, 4096, n - 1):
                ok = np.ones(n, bool)
                ok[r] = False
                add(fam, "%s one null at row %d" % (stem, r), prim(t, base, ok), other, neighbour=srt, flips=True, forbidden=(DICT,), ratio=1.5)
        a = np.arange(n, dtype=np.int64) * 3 + 1
        if t == I32:
            a[0] = -1
            add(fam, "Int32 sorted distinct, first value negative", prim(t, a), NONE, neighbour="Int32 sorted distinct, as it is", flips=True,
                forbidden=(DICT,), ratio=1.5)


def build_patas():
    fam = "patas"
    n = 4096
    # Dict's ratio N W / (unique W + N + N / 64) is exactly W / 2 at `at` keys: decide_prim skips the Patas trial from there
    # up.  Patas cannot reach W / 2 (two bytes per value at least), so the oracle keeps Dict on both sides.
    for t, at in ((F64, 504), (F32, 1008)):
        w = WIDTH[t]
        assert float(n * w) / (at * w + n + n * 2 // 128) == w / 2
        for uq, how in ((at - 1, "above W / 2"), (at, "equal to W / 2"), (at + 1, "below W / 2: the Patas trial runs")):
            add(fam, "%s N=4096, %d keys, Dict's ratio %s" % (tn(t), uq, how), prim(t, 1.0 + (np.arange(n) % uq) * 0.25), DICT)
        add(fam, "%s N=4096, %d keys, Dict forbidden" % (tn(t), at), prim(t, 1.0 + (np.arange(n) % at) * 0.25), PATAS, forbidden=(DICT,))
        add(fam, "%s N=4096, scattered mantissas, nothing pays" % tn(t), prim(t, scatter(n).astype(np.float64) * 1.0000001), NONE, ratio=2.5)


# ================================================================ B. mechanics of the run-level kernel
B_TYPES = (I64, F64, I32)
B_OPTS = (("any codec", dict(ratio=1.2)), ("RLE only", dict(ratio=1.1, forbidden=RLE_ONLY)))


def add_b(fam, stem, a_of_type, prop, valid=None, expect=None):
    """a page through the run-level kernel under both option sets; the oracle's codec is whatever it is (section B states
    input properties), except that RLE must stay the choice where it is the only permitted codec"""
    for t in B_TYPES:
        col = a_of_type(t)
        for label, opt in B_OPTS:
            want = expect if expect is not None else (RLE if label == "RLE only" else DICT)
            add(fam, "%s %s, %s" % (tn(t), stem, label), col, want, prop=prop, **opt)


def build_runs_cap():
    fam = "runs_cap"
    rows = (CHUNK, CHUNK, CHUNK, 1000)
    for where, k in (("the first chunk", 0), ("a middle chunk", 2), ("the short last chunk", 3)):
        for first in (True, False):
            if k == 0 and not first:
                continue
            for r in (RUNS_CAP, RUNS_CAP + 1):
                runs = [100, 100, 100, 50]
                runs[k] = r
                a = page_of_runs(rows, runs, change_on_first=first)
                add_b(fam, "%d raw runs in %s, value %s on each chunk's first row" % (r, where, "changing" if first else "continuing"),
                      lambda t, a=a: prim(t, a), chunk_runs_are(runs))


def build_step2():
    fam = "step2"
    for r in (WG, WG + 1, 2 * WG, 2 * WG + 1):
        runs = [100, r, 50]
        a = page_of_runs((CHUNK, CHUNK, 1000), runs)
        add_b(fam, "%d raw runs in the middle chunk (%d passes of step 2)" % (r, -(-r // WG)), lambda t, a=a: prim(t, a), chunk_runs_are(runs))


def build_page_len():
    fam = "page_len"
    for n in (4097, 4111, 4112, 8191):
        a = 100 + ((np.arange(n) // 20) % 9) * 5
        add_b(fam, "N=%d in runs of 20" % n, lambda t, a=a: prim(t, a),
              lambda c: (stays_in_the_run_kernel(c), "more than RUNS_CAP raw runs in a chunk"))


def build_spec_stop():
    fam = "spec_stop"

    def stops(k):
        def prop(col):
            got = speculation_stops_at(col)
            return got == k and stays_in_the_run_kernel(col), "speculation stops at chunk %s, wanted %s; runs per chunk %s" % (
                got, k, raw_runs_per_chunk(col))
        return prop
    # The stop can only fall at the end of a page's LAST chunk: a whole chunk adds at most RUNS_CAP = 640 records and 4096 rows,
    # so after k whole chunks nrec * 4 <= 2560 k < 4096 k + 256 (tests/test_select_boundaries.py asserts 4 * RUNS_CAP <= CHUNK).
    # No page walks on after a stop; chunks walked with the speculation off belong to the pages that forbid RLE (dict_overflow's
    # pages in runs of 32).
    # end of the first chunk: a 2048-row page, nrec * 4 > 2048 + 256 from 577 records (578 runs) on
    # end of a later chunk: 4096 + 700 rows, nrec * 4 > 4796 + 256 from 1264 records on (640 runs, then 624 / 625 more)
    for stem, rows, runs, k in (("2048 rows, 577 runs: 576 records", (2048,), (577,), None),
                                ("2048 rows, 578 runs: 577 records", (2048,), (578,), 0),
                                ("4796 rows, 640 + 624 runs: 1263 records", (CHUNK, 700), (640, 624), None),
                                ("4796 rows, 640 + 625 runs: 1264 records", (CHUNK, 700), (640, 625), 1)):
        a = page_of_runs(rows, runs)
        for t in B_TYPES:
            add(fam, "%s %s, RLE only" % (tn(t), stem), prim(t, a), RLE, prop=stops(k), ratio=1.1, forbidden=RLE_ONLY)


def build_null_runs():
    fam = "null_runs"
    n = 2 * CHUNK + 500

    def base():
        return 100 + ((np.arange(n) // 40) % 9) * 5

    def has_null_run_at(row):
        def prop(col):
            got = runs_without_a_valid_row(col)
            return row in got and stays_in_the_run_kernel(col), "raw runs without a valid row start at %s, wanted one at %d" % (got, row)
        return prop

    for where, lo, hi in (("across a chunk seam", CHUNK - 6, CHUNK + 5), ("across a wave seam (row 1024)", 1020, 1030),
                          ("at the start of the page", 0, 9), ("at the end of the page", n - 7, n),
                          ("on a chunk's last row", CHUNK - 1, CHUNK), ("on a chunk's first row", CHUNK, CHUNK + 1)):
        a = base()
        a[lo:hi] = 9999
        ok = np.ones(n, bool)
        ok[lo:hi] = False
        add_b(fam, "a raw run without a valid row %s" % where, lambda t, a=a, ok=ok: prim(t, a, ok), has_null_run_at(lo))
    # a raw run across a chunk seam whose first valid row lies in the second chunk
    a = base()
    a[CHUNK - 96:CHUNK + 200] = 7777
    ok = np.ones(n, bool)
    ok[CHUNK - 96:CHUNK + 100] = False

    def seam_prop(col):
        s, v = raw_run_starts(col), valid_rows(col)
        return (not s[CHUNK - 95:CHUNK + 200].any() and s[CHUNK - 96] and not v[CHUNK - 96:CHUNK].any() and v[CHUNK + 100]
                and stays_in_the_run_kernel(col)), "the run over the seam is not as described"
    add_b(fam, "a raw run across a chunk seam, first valid row in the second chunk", lambda t, a=a, ok=ok: prim(t, a, ok), seam_prop)
    # equal keys, different bits, on both sides of a chunk seam with nulls between them (floats only)
    for what in ("+0.0 / -0.0", "two NaN payloads"):
        v = (base() * 0.5).astype(np.float64)
        lo, hi = CHUNK - 50, CHUNK + 50
        if what[0] == "+":
            v[lo:CHUNK] = 0.0
            v[CHUNK:hi] = -0.0
        else:
            v[lo:hi] = np.nan
            v.view(np.uint64)[CHUNK:hi] |= np.uint64(0x55)
        v[CHUNK - 4:CHUNK + 4] = 123.0              # null slots between them, a raw run of their own
        ok = np.ones(n, bool)
        ok[CHUNK - 4:CHUNK + 4] = False

        def bits_prop(col):
            b = col["values"].view(np.uint64)
            return (b[CHUNK - 5] != b[CHUNK + 4] and stays_in_the_run_kernel(col)
                    and (col["values"][CHUNK - 5] == col["values"][CHUNK + 4] or np.isnan(col["values"][[CHUNK - 5, CHUNK + 4]]).all())), "keys / bits"
        for label, opt in B_OPTS:
            add(fam, "Float64 %s on both sides of a chunk seam, nulls between, %s" % (what, label), raw(F64, v, ok),
                RLE if label == "RLE only" else DICT, prop=bits_prop, **opt)


# ================================================================ C. boolean and binary selectors
def build_boolean():
    fam = "boolean"
    n = 1000
    b = np.ones(n, bool)
    b[400] = False
    ok = np.ones(n, bool)
    ok[400] = False
    pair(fam, "Boolean all true except one false",
         [("in a null slot", boolean(b, ok), ONEVALUE), ("in a valid row", boolean(b, np.ones(n, bool)), RLE)])
    # whole-page RLE trial on 640 rows: 80 bytes / (5 bytes a run)
    def runs(n, r):
        edges = (np.arange(r + 1) * n) // r
        return boolean(np.repeat(np.arange(r) % 2 == 0, np.diff(edges)))
    pair(fam, "Boolean 640 rows, RLE ratio against the option 4.0:", [("3 runs (above)", runs(640, 3), RLE), ("4 runs (equal)", runs(640, 4), NONE)], ratio=4.0)
    # one run per sampling range: the whole-page trial of 649 rows has 81 bytes, every sample 80, and 10 runs are 50 bytes
    for nn, want in ((640, NONE), (649, RLE), (650, NONE), (5127, NONE), (5200, NONE)):
        sep = nn // SAMPLE_COUNT
        bb = np.minimum(np.arange(nn) // sep, SAMPLE_COUNT - 1) % 2 == 0
        for seed in (1, 2, 3):
            add(fam, "Boolean N=%d one run per sampling range, seed %d" % (nn, seed), boolean(bb), want,
                neighbour=None if nn not in (649, 650) else "Boolean N=%d one run per sampling range, seed %d" % (1299 - nn, seed),
                flips=nn in (649, 650), ratio=1.61, rng_seed=seed)
    # pages that start at bit offsets 1001 and 2002 of the column's bitmap
    bb = np.ones(3003, bool)
    bb[:1001] = np.arange(1001) % 2 == 0            # page 0: no runs
    bb[2002:] = (np.arange(1001) // 250) % 2 == 0   # page 2: five runs; page 1: all true
    okk = np.ones(3003, bool)
    okk[1001:1005] = False
    add(fam, "Boolean pages at bit offsets 0 / 1001 / 2002", boolean(bb, okk), [NONE, ONEVALUE, RLE], max_page_size=1001)


def build_binary():
    fam = "binary"

    def key(i):
        return b"k%07d" % i                        # 8 bytes

    for large in (False, True):
        tnm = TYPE_NAME[BIN64 if large else BIN32]

        def col(ids, valid=None, words=key):
            return binary([words(int(i)) for i in ids], large, valid)
        uq = 1000
        pair(fam, "%s unique * 3 =" % tnm, [("N - 1", col(np.arange(3001) % uq), DICT), ("N", col(np.arange(3000) % uq), NONE)])
        # majority count, no maximum condition
        n = 1000
        ids = np.zeros(n, np.int64)
        ids[900:] = 1 + np.arange(100)
        below = ids.copy()
        below[899] = 500
        pair(fam, "%s majority" % tnm, [("899/1000", col(below), DICT), ("900/1000", col(ids), FREQ)])
        # the empty string as the majority key / as one of Dict's keys
        def with_empty(i):
            return b"" if i == 0 else key(i)
        pair(fam, "%s majority of empty strings" % tnm, [("899/1000", col(below, words=with_empty), DICT), ("900/1000", col(ids, words=with_empty), FREQ)])
        pair(fam, "%s the empty string among the keys, unique * 3 =" % tnm,
             [("N - 1", col(np.arange(3001) % uq, words=with_empty), DICT), ("N", col(np.arange(3000) % uq, words=with_empty), NONE)])
        # null fraction (every slot a string of its own: nothing else compresses the page)
        ok = np.ones(n, bool)
        ok[50:950] = False
        ok1 = ok.copy()
        ok1[50] = True
        pair(fam, "%s N=1000 nulls" % tnm, [("899", col(np.arange(n), ok1), NONE), ("900", col(np.arange(n), ok), FREQ)], ratio=1.5)
        # index width
        pair(fam, "%s N=1024 distinct keys" % tnm, [("127", col(np.arange(1024) % 127), DICT), ("128", col(np.arange(1024) % 128), NONE)], ratio=5.5)
        # null slots with non-empty bytes of their own count as keys
        ids = np.arange(3001) % uq
        okn = np.ones(3001, bool)
        okn[1500] = False
        own = ids.copy()
        own[1500] = 5000
        pair(fam, "%s unique * 3 = N - 1, null slot" % tnm, [("with a key of the page", col(ids, okn), DICT), ("with a key of its own", col(own, okn), NONE)])
        # total_bytes is values().len() of the WHOLE column + the page's offsets: two pages of 1024 rows over 64 keys.  With the
        # option equal to page 0's ratio nothing is taken; one byte more in page 1 lifts page 0 (not page 1: a 65th key) above it
        ids = np.arange(2048) % 64
        osz = 8 if large else 4
        opt = float(8 * 2048 + 1025 * osz) / (64 * 16 + 1024 * 2 // 128)
        longer = [key(int(i)) for i in ids]
        longer[2047] = longer[2047] + b"!"
        pair(fam, "%s Dict ratio against the option, two pages:" % tnm,
             [("equal", col(ids), [NONE, NONE]), ("one byte more in the other page", binary(longer, large), [DICT, NONE])],
             ratio=opt, max_page_size=1024)


for _b in (build_onevalue, build_freq_nulls, build_freq_majority, build_freq_max, build_dict_limit, build_dict_width, build_dict_overflow,
           build_dict_allones, build_dict_fused, build_strict_order, build_sampling, build_bitpack, build_deltabp, build_patas,
           build_runs_cap, build_step2, build_page_len, build_spec_stop, build_null_runs, build_boolean, build_binary):
    _b()
