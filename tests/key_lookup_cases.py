"""The columns the sb_key_lookup tests run on, as one table: name -> how the column is made, how the oracle writes it, and
the codec EVERY page of it must carry.  tests/test_gpu_key_lookup.py takes its pages from build() alone, and
tests/test_key_lookup_host.py walks the whole table on the CPU, so no GPU case silently tests another route.

build(name) -> Built(col, pages, metas, ref): written by the oracle (or hand-built and decoded by it), the codec of every
page asserted from S.stat_column, the oracle's decode (key_lookup_ref.Ref / StrRef) computed once and left unchanged."""
import functools

import numpy as np

from oracle import sbo as S
from tests import gen
from tests import key_lookup_ref as L
from tests.key_ids_var_ref import column as str_column

NP = gen.NP_OF
INTS = [S.T_I8, S.T_I16, S.T_I32, S.T_I64, S.T_U8, S.T_U16, S.T_U32, S.T_U64]
TYPE_NAME = {S.T_I8: "i8", S.T_I16: "i16", S.T_I32: "i32", S.T_I64: "i64", S.T_U8: "u8", S.T_U16: "u16", S.T_U32: "u32", S.T_U64: "u64"}
CODEC_NAME = {S.NONE: "none", S.LZ4: "lz4", S.ZSTD: "zstd", S.SNAPPY: "snappy", S.ONEVALUE: "onevalue", S.RLE: "rle", S.DICT: "dict",
              S.BITPACK: "bitpack", S.DELTABP: "deltabp", S.FREQ: "freq"}
FILTER_DICT_BITS = 8192   # csrc/sb_filter.h: the entries of the LDS table of a Dict page
ROW_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193)
BIG_ROWS = 4096 * 4096 + 1   # one tile more than TILE_GRID workgroups take in their first sweep


class Built:
    def __init__(self, col, pages, metas):
        self.col, self.pages, self.metas = col, pages, metas
        self.binary = col["ptype"] in (S.T_BIN32, S.T_BIN64)
        self.ref = (L.StrRef if self.binary else L.Ref)(col, pages, metas)
        self.rows = self.ref.rows


def ints(ptype, values, validity=None):
    values = np.asarray(values, NP[ptype])
    return dict(ptype=ptype, nullable=validity is not None, rows=values.size, values=values,
                validity=None if validity is None else gen.pack_bits(validity), offsets=None)


def spread(ptype, rows, uniq, seed, runs=1, nulls=0.2):
    """`rows` values out of `uniq` distinct ones that leave gaps between, below and above them in the type's range, in runs"""
    rng = np.random.default_rng(seed)
    info = np.iinfo(NP[ptype])
    span = int(info.max) - int(info.min)
    uniq = min(uniq, span // 3)
    step = max(3, span // (uniq + 2))
    pool = (int(info.min) + step + step * np.arange(uniq, dtype=object)).astype(NP[ptype])
    idx = np.repeat(rng.integers(0, uniq, (rows + runs - 1) // runs), runs)[:rows]
    return ints(ptype, pool[idx], None if nulls is None else rng.random(rows) >= nulls)


CASES = {}   # name -> (codecs every page must carry (a set), make() -> (col, pages, metas) or (col, write options))


def case(name, codec, make, **opts):
    assert name not in CASES, name
    CASES[name] = (codec, make, opts)


# ---- numeric codec routes, one per codec
for _c in (S.NONE, S.LZ4, S.ZSTD, S.SNAPPY, S.RLE, S.DICT):
    case("route_" + CODEC_NAME[_c], _c, functools.partial(spread, S.T_I64, 10_000, 60, 100 + _c, runs=7), max_page_size=2050, force_codec=_c)
case("route_onevalue", S.ONEVALUE, functools.partial(spread, S.T_I64, 10_000, 1, 7), max_page_size=2050, force_codec=S.ONEVALUE)
for _t in (S.T_I32, S.T_U32):
    case("route_bitpack_" + TYPE_NAME[_t], S.BITPACK, functools.partial(gen.prim, _t, 128 * 100, uniq=200, seed=3),
         max_page_size=128 * 40, force_codec=S.BITPACK)
    case("route_deltabp_" + TYPE_NAME[_t], S.DELTABP, functools.partial(gen.prim, _t, 128 * 100, uniq=200, seed=4, sorted_=True),
         max_page_size=128 * 40, force_codec=S.DELTABP)


def _freq(ptype, seed):
    from tests.test_gpu_freq import sparse
    return sparse(ptype, 10_000, 0.05, seed, null_density=0.1, exc_uniq=200)


for _t in (S.T_I32, S.T_I64, S.T_U8):
    case("route_freq_" + TYPE_NAME[_t], S.FREQ, functools.partial(_freq, _t, 2), max_page_size=2050, force_codec=S.FREQ)
    case("freq_plain_" + TYPE_NAME[_t], S.NONE, functools.partial(_freq, _t, 2), max_page_size=2050, force_codec=S.NONE)


def _dict_entries(D):
    """one Dict page of exactly D entries: every value at least once, 20 000 rows"""
    rng = np.random.default_rng(D)
    v = np.concatenate([np.arange(D), rng.integers(0, D, 20_000 - D)]) * 5 - 20_000
    valid = rng.random(20_000) >= 0.1
    valid[:D] = True   # (a value that only null rows hold is no entry)
    at = rng.permutation(20_000)
    return ints(S.T_I64, v[at], valid[at])


case("dict_%d" % FILTER_DICT_BITS, S.DICT, functools.partial(_dict_entries, FILTER_DICT_BITS), max_page_size=20_000, force_codec=S.DICT)
case("dict_%d" % (FILTER_DICT_BITS + 1), S.DICT, functools.partial(_dict_entries, FILTER_DICT_BITS + 1), max_page_size=20_000, force_codec=S.DICT)

# ---- every integer type on the three walks
for _t in INTS:
    for _c in (S.NONE, S.RLE, S.DICT):
        case("type_%s_%s" % (TYPE_NAME[_t], CODEC_NAME[_c]), _c, functools.partial(spread, _t, 10_000, 40, _t * 16 + _c, runs=5),
             max_page_size=4100, force_codec=_c)


# ---- more than 256 distinct keys in several pages
case("keys_700_dict", S.DICT, functools.partial(spread, S.T_I64, 10_000, 700, 77, runs=2), max_page_size=2050, force_codec=S.DICT)


# ---- the RLE walk: hand-built pages of more than RLE_CHUNK runs, and the long page that several workgroups share
def _rle_hand(ptype, w, dtype):
    from tests.test_gpu_decode import _rle_hand_built_column
    from tests.test_gpu_filter import hand_built
    col, pages, metas = hand_built(ptype, *_rle_hand_built_column(w, dtype))
    assert col is not None
    return col, pages, metas


def _rle_long():
    from tests.test_gpu_decode import LONG_RLE_ROWS, _rle_long_page
    from tests.test_gpu_filter import hand_built
    col, pages, metas = hand_built(S.T_I64, [_rle_long_page()], [LONG_RLE_ROWS])
    assert col is not None and metas.shape[0] == 1
    return col, pages, metas


for _t, _w, _d in ((S.T_U8, 1, np.uint8), (S.T_I16, 2, np.int16), (S.T_I32, 4, np.int32), (S.T_I64, 8, np.int64)):
    case("rle_hand_" + TYPE_NAME[_t], S.RLE, functools.partial(_rle_hand, _t, _w, _d))
case("rle_long", S.RLE, _rle_long)


# ---- row counts, with two and nine pages, the codec going round
def _counted(ptype, rows, seed):
    return spread(ptype, rows, 30, seed, runs=3)


def pages_size(rows, n_pages):
    return max(1, -(-rows // n_pages))


for _i, _r in enumerate(ROW_COUNTS):
    for _p in (2, 9):
        _c = (S.NONE, S.RLE, S.DICT)[(_i + _p) % 3]
        case("rows_%d_%d" % (_r, _p), _c, functools.partial(_counted, S.T_I32, _r, _r + _p), max_page_size=pages_size(_r, _p), force_codec=_c)


# ---- one column of more than TILE_GRID tiles
def _big():
    rng = np.random.default_rng(1)
    return ints(S.T_U8, rng.integers(0, 200, BIG_ROWS).astype(np.uint8))


case("big_u8", S.NONE, _big, max_page_size=1 << 22, force_codec=S.NONE)


# ---- strings
def edge_strings():
    """0, 7, 8, 9 and 40 bytes; strings that share their first 8 bytes; a proper prefix of another; "a" against "a\\0";
    bytes >= 0x80"""
    return [b"", b"a", b"a\x00", b"a\x00\x00", b"ab", b"abcdefg", b"abcdefgh", b"abcdefghi", b"abcdefgh\x00", b"abcdefgX", b"abcdefghZZ",
            b"abcdefgh" + b"q" * 32, b"abcdefgh" + b"q" * 31 + b"r", b"\x80", b"\xff" * 9, b"\x00", b"zzzzzzz", b"0123456789" * 4]


def strings(voc, rows, seed, runs=1, nulls=0.2, large=False, top=None):
    rng = np.random.default_rng(seed)
    idx = np.repeat(rng.integers(0, len(voc), (rows + runs - 1) // runs), runs)[:rows]
    if top is not None:   # one frequent value, the others its exceptions
        idx = np.where(rng.random(rows) < 0.95, top, idx)
    once = rng.permutation(rows)[:len(voc)]
    idx[once] = np.arange(len(voc))[:rows]
    valid = None if nulls is None else rng.random(rows) >= nulls
    if valid is not None:
        valid[once] = True   # (every string of voc is a live row's at least once)
    return str_column([voc[i] for i in idx], valid, large)


def vocab(n, seed):
    from tests.test_gpu_key_ids_var import vocab as v
    return v(n, seed)


for _large in (False, True):
    _n = "large" if _large else "bin"
    for _c in (S.NONE, S.LZ4, S.DICT):
        case("%s_%s" % (_n, CODEC_NAME[_c]), _c, functools.partial(strings, edge_strings() + vocab(60, 5), 10_000, 20 + _c, 2, 0.2, _large),
             max_page_size=2050, force_codec=_c)
    case("%s_freq" % _n, S.FREQ, functools.partial(strings, edge_strings() + vocab(60, 5), 10_000, 31, 1, 0.1, _large, 6),
         max_page_size=2050, force_codec=S.FREQ)
    case("%s_onevalue" % _n, S.ONEVALUE, functools.partial(strings, [b"abcdefgh"], 10_000, 32, 1, 0.2, _large), max_page_size=2050,
         force_codec=S.ONEVALUE)
for _i, _r in enumerate(ROW_COUNTS):
    _c = (S.NONE, S.DICT)[_i % 2]
    case("bin_rows_%d" % _r, _c, functools.partial(strings, edge_strings(), _r, _r, 2, 0.2, bool(_i % 3 == 0)), max_page_size=pages_size(_r, 2),
         force_codec=_c)


def _bin_dict_entries(D):
    voc = [b"entry-%05d-%s" % (i, b"z" * (i % 7)) for i in range(D)]
    return strings(voc, 20_000, D, 1, 0.1)


case("bin_dict_%d" % FILTER_DICT_BITS, S.DICT, functools.partial(_bin_dict_entries, FILTER_DICT_BITS), max_page_size=20_000, force_codec=S.DICT)
case("bin_dict_%d" % (FILTER_DICT_BITS + 1), S.DICT, functools.partial(_bin_dict_entries, FILTER_DICT_BITS + 1), max_page_size=20_000,
     force_codec=S.DICT)


def dict_entries(b):
    """the entries of the one Dict page of a built column (the page inspector, on the host)"""
    from strawboat_amd import stat
    assert b.metas.shape[0] == 1
    return stat.stat_page(b.pages, b.col["ptype"], b.col["nullable"]).body.unique_num


@functools.lru_cache(maxsize=None)
def build(name):
    codec, make, opts = CASES[name]
    made = make()
    if isinstance(made, tuple):
        col, pages, metas = made
    elif made["rows"] == 0:   # (the oracle writes no empty chunk: a column without pages)
        col, pages, metas = made, np.zeros(0, np.uint8), np.zeros((0, 2), np.uint64)
    else:
        col = made
        pages, metas = gen.oracle_write(col, **opts)
    metas = np.asarray(metas, np.uint64).reshape(-1, 2)
    if metas.shape[0]:
        seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
        assert seen == {codec}, "case %s: the pages carry the codecs %r, not %r alone" % (name, seen, codec)
    else:
        assert col["rows"] == 0, name
    return Built(col, pages, metas)
