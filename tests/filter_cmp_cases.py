"""The columns and operands the sb_filter_columns_cmp tests run on.  tests/test_gpu_filter_cmp.py takes its pages from here
alone, and tests/test_filter_cmp_host.py walks the tables on the CPU (every page carries its intended codec), so no GPU
case silently tests another route.

y columns: the codec routes are columns of tests/key_buckets_cases.py (which holds tests/key_lookup_cases.py's), taken as
they are; the row counts, the page seams, the edge tables and the seeded pairs are made here.  build(name) and
build_pair(...) give a Built(col, pages, metas, ref): written by the oracle with the codec forced, the codec of every page
asserted from S.stat_column, the oracle's decode (ref.vals, ref.valid) computed once and left unchanged."""
import functools

import numpy as np

from oracle import sbo as S
from tests import gen
from tests import key_buckets_cases as Bc
from tests import key_lookup_cases as Kc
from tests.filter_cmp_ref import Ref

NP = gen.NP_OF
TYPES = [S.T_I8, S.T_I16, S.T_I32, S.T_I64, S.T_U8, S.T_U16, S.T_U32, S.T_U64, S.T_F32, S.T_F64]
TYPE_NAME = dict(Bc.TYPE_NAME)
CODEC_NAME = dict(Bc.CODEC_NAME)
FILTER_DICT_BITS = Kc.FILTER_DICT_BITS
# one filter_span step is U * WG = 1024 rows, one tile TILE_ROWS = 4096
ROW_COUNTS = (1, 31, 32, 33, 255, 257, 1023, 1025, 4095, 4096, 4097)

# the pairs (y, other) the GPU file covers on the edge tables and with a seeded column: every type with itself, and six mixed
MIXED = [(S.T_I32, S.T_I64), (S.T_I64, S.T_U64), (S.T_U8, S.T_I8), (S.T_I64, S.T_F64), (S.T_F32, S.T_F64), (S.T_U64, S.T_F32)]
PAIRS = [(t, t) for t in TYPES] + MIXED

# the codec routes of y: name in key_buckets_cases -> the codec of its pages
ROUTES = {"route_none": S.NONE, "route_lz4": S.LZ4, "route_zstd": S.ZSTD, "route_snappy": S.SNAPPY, "route_rle": S.RLE,
          "route_onevalue": S.ONEVALUE, "route_dict": S.DICT, "route_bitpack_i32": S.BITPACK, "route_bitpack_u32": S.BITPACK,
          "route_deltabp_i32": S.DELTABP, "route_deltabp_u32": S.DELTABP,
          "dict_%d" % FILTER_DICT_BITS: S.DICT, "dict_%d" % (FILTER_DICT_BITS + 1): S.DICT,
          "f64_none": S.NONE, "f64_rle": S.RLE, "f64_dict": S.DICT, "f64_patas": S.PATAS, "f64_onevalue": S.ONEVALUE,
          "f32_none": S.NONE, "f32_rle": S.RLE, "f32_dict": S.DICT,
          "rle_hand_u8": S.RLE, "rle_hand_i16": S.RLE, "rle_hand_i32": S.RLE, "rle_hand_i64": S.RLE, "rle_long": S.RLE}
FREQ = {"route_freq_i32": S.FREQ, "route_freq_i64": S.FREQ, "route_freq_u8": S.FREQ, "f64_freq": S.FREQ}
FREQ_PLAIN = {"route_freq_i32": "freq_plain_i32", "route_freq_i64": "freq_plain_i64", "route_freq_u8": "freq_plain_u8", "f64_freq": "f64_freq_plain"}


class Built:
    def __init__(self, col, pages, metas):
        self.col, self.pages, self.metas = col, pages, metas
        self.ref = Ref(col, pages, metas)
        self.rows = self.ref.rows


def column(ptype, values, validity=None):
    values = np.ascontiguousarray(values, NP[ptype])
    return dict(ptype=ptype, nullable=validity is not None, rows=values.size, values=values,
                validity=None if validity is None else gen.pack_bits(validity), offsets=None)


def written(col, codec, **opts):
    """the column written by the oracle with `codec` forced; every page must carry it"""
    pages, metas = gen.oracle_write(col, force_codec=codec, **opts)
    metas = np.asarray(metas, np.uint64).reshape(-1, 2)
    seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
    assert seen == {codec}, "the pages carry the codecs %r, not %r alone" % (seen, codec)
    return Built(col, pages, metas)


# ---- the edge values of a type: its extremes, -1 / all ones, 2^63, 2^53 and its neighbours, the zeros, the infinities, NaNs
def edge_values(ptype):
    dt = np.dtype(NP[ptype])
    if dt.kind == "f":
        fi = np.finfo(dt)
        plain = [0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 127.0, 128.0, 255.0, -128.0, 0.5, float(fi.max), -float(fi.max),
                 2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 31, 2.0 ** 32, 2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 63, 2.0 ** 64, -(2.0 ** 63)]
        with np.errstate(over="ignore"):
            return np.concatenate([np.array(plain, dt), Bc.nan_bits(ptype)[:3].view(dt)])
    info = np.iinfo(dt)
    cand = [int(info.min), int(info.min) + 1, -1, 0, 1, 127, 128, 255, int(info.max) - 1, int(info.max),
            2 ** 24, 2 ** 24 + 1, 2 ** 31, 2 ** 32 - 1, 2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1,
            -(2 ** 53) - 1, -(2 ** 31)]
    return np.array(sorted({x for x in cand if info.min <= x <= info.max}), dt)


def edge_pair_values(yt, ot):
    """every edge value of yt against every edge value of ot: (y, other), |E(yt)| * |E(ot)| rows"""
    ey, eo = edge_values(yt), edge_values(ot)
    return np.repeat(ey, eo.size), np.tile(eo, ey.size)


@functools.lru_cache(maxsize=None)
def build_edge_pair(yt, ot, codec):
    """y of the edge pairs of (yt, ot) written with `codec`, every fifth row null, and the operand"""
    y, other = edge_pair_values(yt, ot)
    valid = np.arange(y.size) % 5 != 3
    return written(column(yt, y, valid), codec, max_page_size=29), other


@functools.lru_cache(maxsize=None)
def build_random_pair(yt, ot, codec, rows=6001, seed=0):
    """a seeded column of small values both types hold, in runs, about half of whose rows equal their operand"""
    rng = np.random.default_rng(1000 * yt + 10 * ot + seed)
    signed = all(np.dtype(NP[t]).kind != "u" for t in (yt, ot))
    lo = -60 if signed else 0
    y = np.repeat(rng.integers(lo, 100, rows // 3 + 1), 3)[:rows]
    other = np.where(rng.random(rows) < 0.5, y, rng.integers(lo, 100, rows))
    valid = rng.random(rows) >= 0.15
    return written(column(yt, y.astype(NP[yt]), valid), codec, max_page_size=1500), other.astype(NP[ot])


# ---- row counts and page seams
CASES = {}   # name -> (codec, make() -> col, write options)


def case(name, codec, make, **opts):
    assert name not in CASES and name not in ROUTES and name not in FREQ, name
    CASES[name] = (codec, make, opts)


def _counted(ptype, rows, seed, nulls=0.2):
    rng = np.random.default_rng(seed)
    v = np.repeat(rng.integers(-50, 50, rows // 3 + 1), 3)[:rows]
    return column(ptype, v, None if nulls is None else rng.random(rows) >= nulls)


for _i, _r in enumerate(ROW_COUNTS):
    for _j, _c in enumerate((S.NONE, S.RLE, S.DICT)):
        case("rows_%d_%s" % (_r, CODEC_NAME[_c]), _c, functools.partial(_counted, (S.T_I32, S.T_I64, S.T_I16)[_j], _r, _r + _j),
             max_page_size=1 << 20)
# several pages whose sizes are no multiple of 32: the selection words at the page seams are shared
for _c in (S.NONE, S.RLE, S.DICT, S.LZ4):
    case("seams_" + CODEC_NAME[_c], _c, functools.partial(_counted, S.T_I64, 10_000, 50 + _c), max_page_size=777)
# the four combinations of nulls are the test's (the operand's validity); y without nulls:
for _c in (S.NONE, S.RLE, S.DICT):
    case("nonnull_" + CODEC_NAME[_c], _c, functools.partial(_counted, S.T_I32, 9001, 70 + _c, None), max_page_size=2051)
    case("nullable_" + CODEC_NAME[_c], _c, functools.partial(_counted, S.T_I32, 9001, 80 + _c, 0.3), max_page_size=2051)

ALL = list(ROUTES) + list(FREQ) + list(FREQ_PLAIN.values()) + list(CASES)


def codec_of(name):
    if name in ROUTES:
        return ROUTES[name]
    if name in FREQ:
        return FREQ[name]
    if name in FREQ_PLAIN.values():
        return S.NONE
    return CASES[name][0]


@functools.lru_cache(maxsize=None)
def build(name):
    if name in CASES:
        codec, make, opts = CASES[name]
        return written(make(), codec, **opts)
    b = Bc.build(name)   # (asserts the codec of every page itself)
    assert not b.binary if hasattr(b, "binary") else True
    return b


def codecs_seen(b):
    return set(int(x) for x in S.stat_column(b.col["ptype"], b.col["nullable"], b.pages, b.metas)[0].tolist())


def operand_for(b, ot, seed=0, share=0.5):
    """an operand of type `ot` for a built column: the row's own y (cast to ot, wrapping where it does not fit) in about
    `share` of the rows, another row's y in the rest -- null rows' stored bytes included"""
    rng = np.random.default_rng(seed + b.rows)
    y = b.ref.vals[:b.rows]
    pick = np.where(rng.random(b.rows) < share, np.arange(b.rows), rng.integers(0, max(b.rows, 1), b.rows))
    with np.errstate(invalid="ignore", over="ignore"):
        src = y[pick]
        if np.dtype(NP[ot]).kind in "iu" and src.dtype.kind == "f":
            src = np.nan_to_num(src, nan=0.0, posinf=1e9, neginf=-1e9).clip(-1e9, 1e9)
            if np.dtype(NP[ot]).kind == "u":
                src = np.abs(src)
            src = src.clip(0 if np.dtype(NP[ot]).kind == "u" else np.iinfo(NP[ot]).min, min(1e9, np.iinfo(NP[ot]).max))
        return np.ascontiguousarray(src.astype(NP[ot]))


def garbage_where_invalid(other, other_valid, seed=0):
    """the operand with garbage in the slots of its invalid rows: NaN bit patterns for floats, all kinds of bytes otherwise"""
    rng = np.random.default_rng(seed)
    out = np.array(other, copy=True)
    bad = np.flatnonzero(~np.asarray(other_valid, bool))
    if out.dtype.kind == "f":
        nans = Bc.nan_bits(S.T_F32 if out.dtype.itemsize == 4 else S.T_F64).view(out.dtype)
        out[bad] = nans[rng.integers(0, nans.size, bad.size)]
    else:
        raw = out.view(np.uint8).reshape(-1, out.dtype.itemsize)
        raw[bad] = rng.integers(0, 256, (bad.size, out.dtype.itemsize), dtype=np.uint8)
    return out
