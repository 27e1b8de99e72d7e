"""The columns the sb_key_buckets tests run on, as one table: name -> how the column is made, how the oracle writes it, and
the codec EVERY page of it must carry.  The integer columns are the numeric ones of tests/key_lookup_cases.py, taken as
they are; the float columns are made here.  tests/test_gpu_key_buckets.py takes its pages from build() alone, and
tests/test_key_buckets_host.py walks the whole table on the CPU, so no GPU case silently tests another route.

build(name) -> Built(col, pages, metas, ref): written by the oracle, the codec of every page asserted from S.stat_column,
the oracle's decode (key_buckets_ref.Ref) computed once and left unchanged."""
import functools

import numpy as np

from oracle import sbo as S
from tests import gen
from tests import key_lookup_cases as Kc

NP = gen.NP_OF
FLOATS = [S.T_F32, S.T_F64]
TYPE_NAME = dict(Kc.TYPE_NAME)
TYPE_NAME.update({S.T_F32: "f32", S.T_F64: "f64"})
CODEC_NAME = dict(Kc.CODEC_NAME)
CODEC_NAME[S.PATAS] = "patas"
FILTER_DICT_BITS = Kc.FILTER_DICT_BITS
ROW_COUNTS = (0, 1, 4095, 4096, 4097, 8193)
BIG_ROWS = Kc.BIG_ROWS
Built = Kc.Built

# the integer columns: every numeric case of key_lookup_cases but the row counts this file does not ask for
INT_CASES = [n for n in Kc.CASES
             if n.split("_")[0] not in ("bin", "large") and (not n.startswith("rows_") or int(n.split("_")[1]) in ROW_COUNTS)]

CASES = {}   # the float columns: name -> (the codec every page must carry, make() -> col, write options)


def case(name, codec, make, **opts):
    assert name not in CASES and name not in Kc.CASES, name
    CASES[name] = (codec, make, opts)


def nan_bits(ptype):
    """NaNs of both signs and several payloads, as the bits of the type"""
    if ptype == S.T_F32:
        return np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC12345], np.uint32)
    return np.array([0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF,
                     0xFFFFFFFFFFFFFFFF, 0x7FF8000000012345], np.uint64)


def specials(ptype):
    """+-0.0, +-inf, the smallest denormals and normals, the largest finite values, and the NaNs"""
    dt = np.dtype(NP[ptype])
    fi = np.finfo(dt)
    tiny = np.array([1], "<u%d" % dt.itemsize).view(dt)[0]   # the smallest denormal
    plain = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, fi.tiny, -fi.tiny, fi.max, -fi.max], dt)
    return np.concatenate([plain, nan_bits(ptype).view(dt)])


def floats(ptype, values, validity=None):
    values = np.asarray(values, NP[ptype])
    return dict(ptype=ptype, nullable=validity is not None, rows=values.size, values=values,
                validity=None if validity is None else gen.pack_bits(validity), offsets=None)


def fspread(ptype, rows, uniq, seed, runs=1, nulls=0.2, special=True):
    """`rows` values out of `uniq` multiples of 0.25 around zero and (special) the special values, in runs; every value of
    the pool is a live row's at least once"""
    rng = np.random.default_rng(seed)
    pool = ((np.arange(uniq) - uniq // 2) * 0.25).astype(NP[ptype])
    if special:
        pool = np.concatenate([pool, specials(ptype)])
    idx = np.repeat(rng.integers(0, pool.size, (rows + runs - 1) // runs), runs)[:rows]
    once = rng.permutation(rows)[:pool.size]
    idx[once] = np.arange(pool.size)[:rows]
    valid = None if nulls is None else rng.random(rows) >= nulls
    if valid is not None:
        valid[once] = True
    return floats(ptype, pool[idx], valid)


# ---- Float64 on every codec the oracle writes such a page with; Float32 on the three walks
for _c in (S.NONE, S.LZ4, S.ZSTD, S.SNAPPY, S.RLE, S.DICT):
    case("f64_" + CODEC_NAME[_c], _c, functools.partial(fspread, S.T_F64, 10_000, 60, 200 + _c, runs=7), max_page_size=2050, force_codec=_c)
for _c in (S.NONE, S.RLE, S.DICT):
    case("f32_" + CODEC_NAME[_c], _c, functools.partial(fspread, S.T_F32, 10_000, 60, 300 + _c, runs=5), max_page_size=4100, force_codec=_c)


def _patas(seed):
    rng = np.random.default_rng(seed)
    v = np.round(rng.normal(0, 50, 10_000), 2)
    at = rng.permutation(10_000)[:specials(S.T_F64).size]
    v[at] = specials(S.T_F64)
    valid = rng.random(10_000) >= 0.2
    valid[at] = True
    return floats(S.T_F64, v, valid)


case("f64_patas", S.PATAS, functools.partial(_patas, 11), max_page_size=2050, force_codec=S.PATAS)
case("f64_onevalue", S.ONEVALUE, functools.partial(fspread, S.T_F64, 10_000, 1, 12, 1, 0.2, False), max_page_size=2050, force_codec=S.ONEVALUE)


def _one_nan():
    rng = np.random.default_rng(13)
    return floats(S.T_F64, np.full(10_000, np.nan), rng.random(10_000) >= 0.2)


case("f64_onevalue_nan", S.ONEVALUE, _one_nan, max_page_size=2050, force_codec=S.ONEVALUE)


def _freq(seed):
    from tests.test_gpu_freq import sparse
    return sparse(S.T_F64, 10_000, 0.05, seed, null_density=0.1, exc_uniq=200)


case("f64_freq", S.FREQ, functools.partial(_freq, 2), max_page_size=2050, force_codec=S.FREQ)
case("f64_freq_plain", S.NONE, functools.partial(_freq, 2), max_page_size=2050, force_codec=S.NONE)


def _dict_entries(D):
    """one Float64 Dict page of exactly D entries, a NaN among them (one row: the oracle gives every NaN row an entry of
    its own): every value at least once, 20 000 rows"""
    rng = np.random.default_rng(D)
    pool = np.concatenate([(np.arange(D - 1) - D // 2) * 0.5, [np.nan]])
    idx = np.concatenate([np.arange(D), rng.integers(0, D - 1, 20_000 - D)])
    valid = rng.random(20_000) >= 0.1
    valid[:D] = True   # (a value that only null rows hold is no entry)
    at = rng.permutation(20_000)
    return floats(S.T_F64, pool[idx][at], valid[at])


case("f64_dict_%d" % FILTER_DICT_BITS, S.DICT, functools.partial(_dict_entries, FILTER_DICT_BITS), max_page_size=20_000, force_codec=S.DICT)
case("f64_dict_%d" % (FILTER_DICT_BITS + 1), S.DICT, functools.partial(_dict_entries, FILTER_DICT_BITS + 1), max_page_size=20_000,
     force_codec=S.DICT)


def _rle_long():
    from tests.test_gpu_decode import LONG_RLE_ROWS
    return fspread(S.T_F64, LONG_RLE_ROWS, 200, 4, runs=32, nulls=0.1)


case("f64_rle_long", S.RLE, _rle_long, max_page_size=1 << 22, force_codec=S.RLE)

for _i, _r in enumerate(ROW_COUNTS):
    _c = (S.NONE, S.RLE, S.DICT)[_i % 3]
    case("f64_rows_%d" % _r, _c, functools.partial(fspread, S.T_F64, _r, 20, _r + 1, runs=3), max_page_size=Kc.pages_size(_r, 3), force_codec=_c)



# ---- bounds and values at the extremes of each type: every bound as a value, and one step to either side of it
def edge_bounds(ptype):
    dt = np.dtype(NP[ptype])
    if dt.kind == "f":
        fi = np.finfo(dt)
        tiny = np.array([1], "<u%d" % dt.itemsize).view(dt)[0]
        return np.array([-np.inf, -fi.max, -1.0, -tiny, 0.0, tiny, 1.0, fi.max, np.inf], dt)
    info = np.iinfo(dt)
    mid = 0 if info.min < 0 else int(info.max) // 2 + 1
    return np.array(sorted({int(info.min), int(info.min) + 3, mid, int(info.max) - 3, int(info.max)}), dt)


def edge_values(ptype):
    dt = np.dtype(NP[ptype])
    b = edge_bounds(ptype)
    if dt.kind == "f":
        with np.errstate(over="ignore"):   # (one step beyond the largest finite value is inf)
            below, above = np.nextafter(b, dt.type(-np.inf)), np.nextafter(b, dt.type(np.inf))
        return np.concatenate([b, below, above, np.array([-0.0], dt), nan_bits(ptype).view(dt)])
    info = np.iinfo(dt)
    near = [int(x) + d for x in b.tolist() for d in (-1, 0, 1)]
    return np.array(sorted({x for x in near if info.min <= x <= info.max}), dt)


def _edges(ptype, seed):
    rng = np.random.default_rng(seed)
    pool = edge_values(ptype)
    rows = 5000
    idx = np.repeat(rng.integers(0, pool.size, rows // 4), 4)
    once = rng.permutation(rows)[:pool.size]
    idx[once] = np.arange(pool.size)
    valid = rng.random(rows) >= 0.2
    valid[once] = True
    return dict(ptype=ptype, nullable=True, rows=rows, values=pool[idx], validity=gen.pack_bits(valid), offsets=None)


for _t in Kc.INTS + FLOATS:
    for _c in (S.NONE, S.RLE, S.DICT):
        case("edge_%s_%s" % (TYPE_NAME[_t], CODEC_NAME[_c]), _c, functools.partial(_edges, _t, _t * 8 + _c), max_page_size=2050, force_codec=_c)

ALL = INT_CASES + list(CASES)


def _uleb(v):
    out = bytearray()
    while True:
        out.append((v & 0x7F) | (0x80 if v >> 7 else 0))
        v >>= 7
        if not v:
            return bytes(out)


@functools.lru_cache(maxsize=None)
def with_validity_bits_behind_rows(name):
    """The pages of a nullable column with the bits behind the last row of every page's validity bits set: the def-level
    section at the head of a page is u32 length | ULEB128((ceil(N / 8) << 1) | 1) | the bits.  The oracle decodes the
    same rows and the same validity from them."""
    b = build(name)
    assert b.col["nullable"]
    pages = b.pages.copy()
    at, changed = 0, 0
    for length, n in b.metas.tolist():
        nbytes = (n + 7) // 8
        head = _uleb((nbytes << 1) | 1)
        assert int.from_bytes(pages[at:at + 4].tobytes(), "little") == len(head) + nbytes, name
        assert pages[at + 4:at + 4 + len(head)].tobytes() == head, name
        if n % 8:
            pages[at + 4 + len(head) + nbytes - 1] |= (0xFF << (n % 8)) & 0xFF
            changed += 1
        at += length
    assert changed
    out = Built(b.col, pages, b.metas)
    assert np.array_equal(out.ref.valid, b.ref.valid) and out.ref.vals[:out.rows].tobytes() == b.ref.vals[:b.rows].tobytes()
    return out


def dict_entries(b):
    return Kc.dict_entries(b)


@functools.lru_cache(maxsize=None)
def build(name):
    if name in Kc.CASES:
        assert name in INT_CASES, name
        return Kc.build(name)
    codec, make, opts = CASES[name]
    col = make()
    if col["rows"] == 0:   # (the oracle writes no empty chunk: a column without pages)
        pages, metas = np.zeros(0, np.uint8), np.zeros((0, 2), np.uint64)
    else:
        pages, metas = gen.oracle_write(col, **opts)
    metas = np.asarray(metas, np.uint64).reshape(-1, 2)
    if metas.shape[0]:
        seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
        assert seen == {codec}, "case %s: the pages carry the codecs %r, not %r alone" % (name, seen, codec)
    return Built(col, pages, metas)
