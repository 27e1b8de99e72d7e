"""The case table of tests/test_gpu_mixed_columns.py: columns whose pages mix codecs, as the default writer leaves them.

The suites of the sink calls write their columns with one forced codec; a real column is a sequence such as RLE, Dict,
plain, LZ4, OneValue, bit-packed, RLE.  The sinks' code changes exactly where pages of different routes meet: a selection
word that straddles a seam is written by two kernels, the packed outputs of the selected reads place a page behind the
selected rows of every page before it whatever route counted them, an aggregate-like call keeps page slots and tile slots
for one column, and one primitive Freq page sends a column whose other pages already wrote records to the decoded route.

No fixtures, no tests, no device: tests/test_mixed_cases.py walks the same table on the CPU.

stitch(ptype, plan) writes every segment of a plan as ONE page with the oracle's writer (force_codec, no max_page_size) and
concatenates the pages; `adaptive` columns are written with no forced codec at all.  A plan is a list of
(rows, codec, index codec or None, recipe).  The routes of a page, by the kernels that take it:
  R  RLE                      N  None                          I  LZ4 / Zstd / Snappy (Patas on Float64): inflated first
  O  OneValue                 D  Dict (index codec rotating)   P  Bitpacking / DeltaBP (Int32 / UInt32 only)
  F  Freq (a primitive Freq page asks for the replay; a binary one is evaluated on the pages)

Values.  Page p of a numeric column lies in [base_p, base_p + span): the bases ascend by `stride` > span, so a row
credited to the wrong page, or a page's rows placed at the wrong out_row, changes every sink's answer.  A page's shape
follows its codec (OneValue constant, RLE runs, DeltaBP sorted, Freq one dominant value and about 5 % exceptions, Patas
two-decimal floats).  An integer page draws from at most `span` <= 25 values, so a column keeps at most 1024 distinct values
(Int8 has room for a stride of 9 only, the other types take 26).  A float page draws from 24 values base_p + span * u with
u of unit, 1e-3 and 1e-8 size and random mantissas: a sum has digits to lose.  Page p of a binary column carries p in a
prefix of its strings; the empty string is among the values of every third page.  About 10 % nulls everywhere, one all-null
page per plan (OneValue in `pairs`, RLE in `tiles`), and at every seam each side that has two rows or more in the seam's
selection word holds a null and a valid row there (so `ne` and the null tests write both bits on both sides)."""
import functools
import zlib

import numpy as np

from oracle import sbo as S
from tests import gen

NP = gen.NP_OF
TILE_ROWS, CHUNK_TILES = 4096, 16
FLOATS = (S.T_F32, S.T_F64)
BINARY = (S.T_BIN32, S.T_BIN64)
TYPE_NAMES = {S.T_I8: "i8", S.T_I16: "i16", S.T_I32: "i32", S.T_I64: "i64", S.T_U8: "u8", S.T_U16: "u16", S.T_U32: "u32",
              S.T_U64: "u64", S.T_F32: "f32", S.T_F64: "f64", S.T_BIN32: "bin", S.T_BIN64: "lbin"}
CODEC_NAMES = {S.NONE: "None", S.LZ4: "LZ4", S.ZSTD: "Zstd", S.SNAPPY: "Snappy", S.RLE: "RLE", S.DICT: "Dict", S.ONEVALUE: "OneValue",
               S.FREQ: "Freq", S.BITPACK: "Bitpacking", S.DELTABP: "DeltaBP", S.PATAS: "Patas"}
ROUTE_OF = {S.RLE: "R", S.NONE: "N", S.LZ4: "I", S.ZSTD: "I", S.SNAPPY: "I", S.PATAS: "I", S.ONEVALUE: "O", S.DICT: "D", S.BITPACK: "P",
            S.DELTABP: "P", S.FREQ: "F"}
BLOCK = 128                      # Bitpacking / DeltaBP hold whole blocks of 128 values
SHORT_ROWS = (37, 7, 31, 33, 1, 63, 65, 100, 129, 255, 300)
DICT_INDEX_NUM = (S.NONE, S.RLE, S.BITPACK, S.LZ4, S.ONEVALUE)
DICT_INDEX_BIN = (S.NONE, S.RLE, S.BITPACK, S.DELTABP, S.LZ4, S.ZSTD, S.ONEVALUE)
MAX_KEYS = 1024
POOL = 24                        # the values a float or binary page draws from
NULLS = 0.1


def seed_of(*names):
    return zlib.crc32("/".join(str(n) for n in names).encode())


# ---------------------------------------------------------------- plans
class Seg:
    """one page of a plan"""

    def __init__(self, rows, codec, icodec=None, recipe=None):
        self.rows, self.codec, self.icodec = rows, codec, icodec
        self.recipe = recipe or {S.RLE: "runs", S.ONEVALUE: "const", S.DELTABP: "sorted", S.FREQ: "freq", S.PATAS: "patas",
                                 S.DICT: "const" if icodec == S.ONEVALUE else "sorted" if icodec == S.DELTABP else "few"}.get(codec, "noise")

    @property
    def route(self):
        return ROUTE_OF[self.codec]

    @property
    def blocks(self):
        return self.codec in (S.BITPACK, S.DELTABP) or self.icodec in (S.BITPACK, S.DELTABP)

    def __iter__(self):
        return iter((self.rows, self.codec, self.icodec, self.recipe))


def euler(routes):
    """a walk over `routes` in which every ordered pair, a route followed by itself included, is adjacent exactly once:
    len(routes)^2 + 1 stops, from routes[0] back to it (Hierholzer on the complete digraph with loops)"""
    left = {r: list(routes) for r in routes}
    stack, walk = [routes[0]], []
    while stack:
        v = stack[-1]
        if left[v]:
            stack.append(left[v].pop(0))
        else:
            walk.append(stack.pop())
    return walk[::-1]


class Rotor:
    """the codecs of a route, handed out in turn"""

    def __init__(self, ptype):
        binary = ptype in BINARY
        self.of = {"R": [(S.RLE, None)], "N": [(S.NONE, None)], "O": [(S.ONEVALUE, None)], "F": [(S.FREQ, None)],
                   "I": [(S.LZ4, None), (S.ZSTD, None), (S.SNAPPY, None)] + ([(S.PATAS, None)] if ptype == S.T_F64 else []),
                   "D": [(S.DICT, i) for i in (DICT_INDEX_BIN if binary else DICT_INDEX_NUM)],
                   "P": [(S.BITPACK, None), (S.DELTABP, None)]}
        self.at = {r: 0 for r in self.of}

    def take(self, route):
        c = self.of[route][self.at[route] % len(self.of[route])]
        self.at[route] += 1
        return c


def routes_of(ptype):
    if ptype in BINARY:
        return ("D", "N", "O", "I", "F")
    return ("R", "N", "I", "O", "D") + (("P",) if ptype in (S.T_I32, S.T_U32) else ())


def short_rows(segs, start=0):
    """rows for the pages of a plan of short pages: from SHORT_ROWS in turn, from entry `start` on (whole blocks: 128 or
    256), no seam at a multiple of 32"""
    at, k, n_blocks = 0, start, 0
    for s in segs:
        if s.blocks:
            s.rows = BLOCK * (1 + n_blocks % 2)
            n_blocks += 1
        else:
            while (at + SHORT_ROWS[k % len(SHORT_ROWS)]) % 32 == 0:
                k += 1
            s.rows = SHORT_ROWS[k % len(SHORT_ROWS)]
            k += 1
        at += s.rows
        assert at % 32, "a block page may not be the first"
    return segs


# plans whose first shape missed a condition of tests/test_mixed_cases.py (the column's median fell into a constant page,
# where `ne median` selects no row): their pages take their rows from another entry of SHORT_ROWS on
SALT = {("pairs_freq_last", S.T_I32): 2}


def pairs_plan(ptype, freq=None):
    rot = Rotor(ptype)
    walk = euler(routes_of(ptype))
    if ptype in BINARY:
        walk = walk + ["D"]   # (seven index codecs of a binary Dict page: one D more than the walk holds)
    elif freq == "mid":   # X Y becomes X F X Y: the pair the Freq page parts is there again behind it
        i = len(walk) // 2
        walk = walk[:i] + ["F", walk[i - 1]] + walk[i:]
    elif freq == "last":
        walk = walk + ["F"]
    segs = [Seg(0, *rot.take(r)) for r in walk]
    null_route = "O"
    nth = [i for i, s in enumerate(segs) if s.route == null_route][1]
    segs[nth].recipe = "null"
    return short_rows(segs, SALT.get(("pairs_freq_" + freq if freq else "pairs", ptype), 0))


def tiles_plan(ptype, freq=None):
    """19 long pages, 35 tiles: tile 16 lies inside the RLE page 9, tile 32 is the first of the plain page 17 that follows the
    RLE page 16.  Page 1 is an RLE page of more than 1024 runs, page 12 the all-null one."""
    packed = ptype in (S.T_I32, S.T_U32)
    last_i = (S.PATAS, None) if ptype == S.T_F64 else (S.SNAPPY, None)
    segs = [Seg(4095, S.NONE), Seg(4097, S.RLE, None, "short_runs"), Seg(4100, S.DICT, S.RLE), Seg(8197, S.LZ4), Seg(4097, S.ONEVALUE),
            Seg(1, S.ONEVALUE), Seg(2050, S.ZSTD), Seg(BLOCK * 33, S.BITPACK) if packed else Seg(BLOCK * 33, S.NONE), Seg(4096, S.NONE),
            Seg(8197, S.RLE), Seg(4097, S.DICT, S.NONE), Seg(4100, *last_i), Seg(4095, S.RLE, None, "null"),
            Seg(BLOCK * 33, S.DICT, S.BITPACK), Seg(8197, S.NONE), Seg(2050, S.SNAPPY), Seg(8197, S.RLE), Seg(4097, S.NONE), Seg(2050, S.RLE)]
    if freq == "mid":   # (two tiles spliced in behind the RLE page 9; the plain page 14 gives them back, so the borders stay)
        segs[14] = Seg(4096, S.NONE)
        segs.insert(10, Seg(4100, S.FREQ))
    elif freq == "last":
        segs.append(Seg(4100, S.FREQ))
    return segs


def tiles_plan_bin(ptype):
    return [Seg(4097, S.NONE), Seg(8197, S.DICT, S.RLE), Seg(4100, S.ONEVALUE), Seg(9000, S.LZ4), Seg(4097, S.FREQ), Seg(5000, S.DICT, S.NONE),
            Seg(4100, S.ZSTD, None, "null"), Seg(4097, S.NONE)]


def aligned_plan(ptype):
    """every page a multiple of 32 rows: the column keeps the aligned bitmap path"""
    packed = ptype in (S.T_I32, S.T_U32)
    return [Seg(64, S.RLE), Seg(96, S.NONE), Seg(160, S.LZ4), Seg(32, S.ONEVALUE), Seg(128, S.DICT, S.BITPACK),
            Seg(256, S.DELTABP) if packed else Seg(256, S.PATAS if ptype == S.T_F64 else S.SNAPPY), Seg(4096, S.RLE), Seg(32, S.NONE),
            Seg(320, S.DICT, S.RLE), Seg(4128, S.ZSTD), Seg(4096, S.ONEVALUE), Seg(224, S.DICT, S.NONE, "null"), Seg(32, S.RLE),
            Seg(128, S.BITPACK) if packed else Seg(128, S.NONE), Seg(64, S.SNAPPY)]


ADAPTIVE_PAGE = 2048
# what the data of an adaptive column is like, page by page (the writer's selector decides the codec, tests/test_mixed_cases.py
# says what it chose): runs and few values go to Dict pages, a constant to OneValue, `packed` (700 small values) to Bitpacking,
# `plain` (the same with a negative value, doubles with random mantissas, 700 strings) to None, `special` to Patas on
# Float64 (whole numbers) and to Freq on Binary (a dominant string)
ADAPTIVE_RECIPES = ("runs", "plain", "few", "const", "packed", "runs", "special", "plain", "few", "packed", "const", "runs")

NUM_PAIRS = (S.T_I32, S.T_U32, S.T_I64, S.T_F64, S.T_F32, S.T_U16, S.T_I8)
PLANS = {}   # (plan name, ptype) -> a function that gives the plan's segments (None: adaptive)
for _t in NUM_PAIRS + BINARY:
    PLANS[("pairs", _t)] = functools.partial(pairs_plan, _t)
for _t in (S.T_I32, S.T_I64, S.T_F64):
    PLANS[("tiles", _t)] = functools.partial(tiles_plan, _t)
PLANS[("tiles", S.T_BIN32)] = functools.partial(tiles_plan_bin, S.T_BIN32)
for _t in (S.T_I32, S.T_F64):
    PLANS[("aligned", _t)] = functools.partial(aligned_plan, _t)
for _t in (S.T_I32, S.T_I64):
    for _w in ("mid", "last"):
        PLANS[("pairs_freq_" + _w, _t)] = functools.partial(pairs_plan, _t, _w)
        PLANS[("tiles_freq_" + _w, _t)] = functools.partial(tiles_plan, _t, _w)
for _t in (S.T_I32, S.T_F64, S.T_BIN32):
    PLANS[("adaptive", _t)] = None
KEYS = list(PLANS)
FREQ_KEYS = [k for k in KEYS if "freq" in k[0]]
LONG_RLE_ROWS = (1 << 18) + 5   # tests/test_gpu_decode.py: the shortest page that several workgroups share


def key_id(key):
    return "%s-%s" % (key[0], TYPE_NAMES[key[1]])


def is_binary(key):
    return key[1] in BINARY


@functools.lru_cache(maxsize=None)
def plan_of(key):
    return None if PLANS[key] is None else PLANS[key]()


# ---------------------------------------------------------------- values
def spacing(ptype, n_pages):
    """(the first base, stride, span) of the pages' value ranges"""
    if ptype in FLOATS:
        return -float(26 * (n_pages // 2)), 26.0, 25.0
    info = np.iinfo(NP[ptype])
    stride = min(26, (int(info.max) - int(info.min) + 1) // n_pages)
    lo = max(int(info.min) + 1, -(n_pages // 2) * stride) if info.min < 0 else stride   # (a value below all of them exists)
    return lo, stride, stride - 1


def page_pool(ptype, p, n_pages, rng):
    """the values page p draws from, ascending"""
    lo, stride, span = spacing(ptype, n_pages)
    base = lo + p * stride
    if ptype not in FLOATS:
        return (base + np.arange(span)).astype(NP[ptype])
    u = np.minimum((1.0 + rng.random(POOL)) * rng.choice([0.4, 1e-3, 1e-8], POOL), 0.99)
    return np.unique((base + span * u).astype(NP[ptype]))


def draw(recipe, n_pool, rows, rng):
    """the index into the page's pool of every row"""
    if recipe in ("const", "null"):
        return np.full(rows, n_pool // 2)
    if recipe in ("runs", "short_runs", "long_runs"):
        mean = {"runs": 6, "short_runs": 2, "long_runs": 300}[recipe]
        n = rows // mean + 2
        step = rng.integers(1, n_pool, n) if n_pool > 1 else np.zeros(n, np.int64)   # (neighbouring runs differ)
        idx = np.repeat(np.cumsum(step) % n_pool, rng.geometric(1.0 / mean, n) if mean > 2 else rng.integers(1, 4, n))[:rows]
        return np.concatenate([idx, np.full(rows - idx.size, idx[-1])])
    if recipe == "freq":
        return np.where(rng.random(rows) < 0.95, 0, rng.integers(0, n_pool, rows))
    if recipe == "few":
        return rng.integers(0, min(n_pool, 5), rows)
    idx = rng.integers(0, n_pool, rows)
    return np.sort(idx) if recipe == "sorted" else idx


def page_validity(recipe, rows, rng):
    if recipe == "null":
        return np.zeros(rows, bool)
    valid = rng.random(rows) >= NULLS
    if not valid.any():
        valid[0] = True
    return valid


def seam_validity(valid, edges):
    """at every seam, each side that has two rows or more in the seam's selection word holds a null and a valid row there
    (all-null pages stay all null)"""
    for a, s, b in zip(edges[:-2], edges[1:-1], edges[2:]):
        if s % 32 == 0:
            continue
        w0 = s - s % 32
        if s - max(a, w0) >= 2 and valid[a:s].any():
            valid[s - 1], valid[s - 2] = True, False
        if min(b, w0 + 32) - s >= 2 and valid[s:b].any():
            valid[s], valid[s + 1] = True, False
    return valid


def binary_pool(p, rng):
    words = [b"", b"a", b"zz", b"key", b"value-%d" % p, b"\x00\xff", b"long-" * 7, b"mid" * 3]
    words += [bytes(rng.integers(32, 127, int(rng.integers(1, 20)), dtype=np.uint8)) for _ in range(POOL - len(words))]
    pool = sorted(set(b"p%02d:" % p + w for w in words[1:]))
    return ([b""] if p % 3 == 0 else []) + pool


def binary_col(ptype, strs, valid):
    lens = np.fromiter((len(s) for s in strs), np.int64, len(strs))
    offs = np.zeros(len(strs) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    data = np.frombuffer(b"".join(strs), np.uint8).copy()
    return dict(ptype=ptype, nullable=True, rows=len(strs), values=data, validity=gen.pack_bits(valid),
                offsets=offs.astype(np.int64 if ptype == S.T_BIN64 else np.int32))


def page_values(key, p, n_pages, recipe, rows, rng):
    """the values of page p: a typed array, or a list of bytes"""
    ptype = key[1]
    if ptype in BINARY:
        pool = binary_pool(p, rng)
        first = 1 if pool[0] == b"" else 0   # (a constant or dominant value carries the page's prefix)
        idx = draw(recipe, len(pool) - first, rows, rng) + first
        if recipe in ("noise", "few", "sorted") and first:
            idx[rng.random(rows) < 0.1] = 0
        return [pool[i] for i in idx]
    pool = page_pool(ptype, p, n_pages, rng)
    if recipe == "patas":
        pool = np.unique(np.round(pool, 2))
    return pool[draw(recipe, pool.size, rows, rng)]


def adaptive_values(ptype, p, recipe, rows, rng):
    """the values of page p of an adaptive column.  An Int32 column keeps at most 1024 distinct values, so its `packed` and
    `plain` pages share theirs and the pages' ranges are not disjoint"""
    runs = lambda k: np.repeat(rng.integers(0, k, rows // 64 + 1), 64)[:rows]
    wide = recipe in ("plain", "packed") or (recipe == "special" and ptype not in BINARY)
    idx = {"runs": lambda: runs(8), "few": lambda: rng.integers(0, 5, rows), "const": lambda: np.zeros(rows, np.int64),
           "special": lambda: np.where(rng.random(rows) < 0.95, 0, rng.integers(0, 700, rows))}.get(recipe, lambda: rng.integers(0, 700, rows))()
    if ptype in BINARY:
        if recipe == "plain":   # (a string of its own per row: no dictionary pays)
            idx = np.arange(rows) + 50 * rows
        elif recipe != "special":
            idx = np.minimum(idx, 40)
        return [b"a%02d:%d" % (p, i) if i % 50 else b"" for i in idx + 1]
    if ptype in FLOATS:
        if recipe == "special":
            return (1000.0 * p + rng.integers(0, 700, rows)).astype(NP[ptype])
        if recipe == "plain":
            return (26.0 * p + 25.0 * rng.random(rows)).astype(NP[ptype])
        return ((26.0 * p + idx) * 1.000123).astype(NP[ptype])
    if not wide:
        return (2000 + 10 * p + idx).astype(NP[ptype])
    v = rng.integers(0, 700, rows)
    if recipe != "packed":
        v[rng.random(rows) < 0.01] = -1 - p % 3
    return v.astype(NP[ptype])


def build(key, salt=0):
    """(col, edges) of a plan: the concatenated inputs"""
    plan = plan_of(key)
    ptype = key[1]
    rng = np.random.default_rng(seed_of("mixed", key_id(key), salt))
    segs = plan if plan is not None else [Seg(ADAPTIVE_PAGE, S.NONE, None, r) for r in ADAPTIVE_RECIPES]
    n = len(segs)
    parts, valids = [], []
    for p, s in enumerate(segs):
        parts.append(page_values(key, p, n, s.recipe, s.rows, rng) if plan is not None else adaptive_values(ptype, p, s.recipe, s.rows, rng))
        valids.append(page_validity(s.recipe, s.rows, rng))
    edges = np.concatenate([[0], np.cumsum([s.rows for s in segs])]).astype(np.int64)
    valid = seam_validity(np.concatenate(valids), edges.tolist())
    if ptype in BINARY:
        col = binary_col(ptype, [x for part in parts for x in part], valid)
    else:
        col = dict(ptype=ptype, nullable=True, rows=int(edges[-1]), values=np.concatenate(parts).astype(NP[ptype]),
                   validity=gen.pack_bits(valid), offsets=None)
    return col, edges


def slice_col(col, a, b, valid):
    """rows [a, b) of a column as a column of its own"""
    out = dict(ptype=col["ptype"], nullable=True, rows=b - a, validity=gen.pack_bits(valid[a:b]), offsets=None)
    if col["offsets"] is None:
        out["values"] = np.ascontiguousarray(col["values"][a:b])
    else:
        o = col["offsets"].astype(np.int64)
        out["values"] = np.ascontiguousarray(col["values"][o[a]:o[b]])
        out["offsets"] = (o[a:b + 1] - o[a]).astype(col["offsets"].dtype)
    return out


@functools.lru_cache(maxsize=None)
def stitched(key):
    """(col, pages, metas) of a plan: every segment written as one page by the oracle with its codec forced, the pages back
    to back and the metas rows stacked; written once, never modified"""
    col, edges = build(key)
    valid = np.unpackbits(col["validity"], bitorder="little")[:col["rows"]].astype(bool)
    plan = plan_of(key)
    if plan is None:
        pages, metas = gen.oracle_write(col, ratio=2.0, max_page_size=ADAPTIVE_PAGE)
    else:
        page_list, meta_list = [], []
        for s, a, b in zip(plan, edges[:-1], edges[1:]):
            opt = dict(force_codec=s.codec)
            if s.icodec is not None:
                opt["force_index_codec"] = s.icodec
            pg, mt = gen.oracle_write(slice_col(col, int(a), int(b), valid), **opt)
            assert mt.shape[0] == 1 and int(mt[0, 1]) == s.rows, "one segment is one page"
            page_list.append(pg)
            meta_list.append(mt)
        pages, metas = np.concatenate(page_list), np.concatenate(meta_list)
    for a in (pages, metas, col["values"], col["validity"], col["offsets"]):
        if a is not None:
            a.setflags(write=False)
    return col, pages, metas


def stitch(ptype, plan, nullable=True):
    """(col, pages, metas) of the plan registered for (plan name, ptype)"""
    assert nullable
    return stitched((plan, ptype))


def edges_of(key):
    metas = stitched(key)[2]
    return np.concatenate([[0], np.cumsum(np.asarray(metas)[:, 1].astype(np.int64))])


def page_codecs(key):
    """[(codec, index codec)] page by page, as the oracle's stat finds them"""
    col, pages, metas = stitched(key)
    codecs, inner = S.stat_column(col["ptype"], col["nullable"], pages, metas)
    return [(int(c), int(i)) for c, i in zip(codecs.tolist(), inner.tolist())]


def routes(key):
    return [ROUTE_OF[c] for c, _ in page_codecs(key)]


def sequence(key):
    """the stitched codec sequence as text, from S.stat_column"""
    return ", ".join(CODEC_NAMES[c] + ("(%s)" % CODEC_NAMES[i] if c == S.DICT else "") for c, i in page_codecs(key))


# ---------------------------------------------------------------- the oracle's decode
@functools.lru_cache(maxsize=None)
def ref_of(key):
    """the oracle's decode of a stitched column: aggregate_ref.Ref for numbers, key_ids_var_ref.Ref for strings"""
    from tests import aggregate_ref as R
    from tests import key_ids_var_ref as KV
    ref = (KV.Ref if is_binary(key) else R.Ref)(*stitched(key))
    for a in (ref.valid, getattr(ref, "vals", None)):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


# ---------------------------------------------------------------- selections
SELECTIONS = ("random", "sparse", "none", "seams")


@functools.lru_cache(maxsize=None)
def masks(key):
    """the four selections of a column, read-only: a random ~0.35 (with the first and the last valid row of every page, so
    that a valid selected row lies on both sides of every seam), a sparse one that leaves whole pages and tiles out and
    holds the last row (the recipe of test_gpu_read_selected.two_masks), None, and exactly the first and the last row of
    every page"""
    ref, edges = ref_of(key), edges_of(key)
    rows = ref.rows
    rng = np.random.default_rng(seed_of("masks", key_id(key)))
    sparse = np.zeros(rows, bool)
    at = int(rng.integers(0, max(1, rows - 70)))
    sparse[at:at + 70] = rng.random(min(70, rows - at)) < 0.7
    sparse[rows - 1] = True
    rand = rng.random(rows) < 0.35
    seams = np.zeros(rows, bool)
    for a, b in zip(edges[:-1], edges[1:]):
        seams[a] = seams[b - 1] = True
        live = np.flatnonzero(ref.valid[a:b])
        if live.size:
            rand[a + live[0]] = rand[a + live[-1]] = True
    for m in (rand, sparse, seams):
        m.setflags(write=False)
    return (rand, sparse, None, seams)


# ---------------------------------------------------------------- arguments of the calls, from the oracle's decode
def median(key):
    """the median of the valid values (of the valid strings that are not empty)"""
    ref = ref_of(key)
    if is_binary(key):
        v = sorted(x for x in ref.strs[ref.valid].tolist() if x)
        return v[len(v) // 2]
    v = np.sort(ref.vals[ref.valid])
    return v[v.size // 2].item()


def outside(key):
    """(a value below all values, one above all)"""
    ref = ref_of(key)
    v = ref.vals[ref.valid]
    return (v.min() - 1).item(), (v.max() + 1).item()


def in_list(key):
    """one valid value of every third page, and two absent ones"""
    ref, edges = ref_of(key), edges_of(key)
    out = []
    for a, b in list(zip(edges[:-1], edges[1:]))[::3]:
        live = np.flatnonzero(ref.valid[a:b])
        if live.size:
            out.append((ref.strs if is_binary(key) else ref.vals)[a + live[live.size // 2]])
    if is_binary(key):
        return [bytes(x) for x in out] + [b"p00:absent", b"\xff\xffabsent"]
    lo, hi = outside(key)
    return [x.item() for x in out] + [lo, hi]


def lookup_list(key):
    """a shuffled list of the distinct valid values of every second page (None where the type has no key lookup)"""
    ref, edges = ref_of(key), edges_of(key)
    vals = ref.strs if is_binary(key) else ref.vals
    have = set()
    for a, b in list(zip(edges[:-1], edges[1:]))[::2]:
        have |= set(vals[a:b][ref.valid[a:b]].tolist())
    lst = sorted(have)
    order = np.random.default_rng(seed_of("lookup", key_id(key))).permutation(len(lst))
    lst = [lst[i] for i in order]
    return lst if is_binary(key) else np.array(lst, ref.vals.dtype)


def bucket_bounds(key):
    """ascending bounds at the smallest valid value of every page and in the middle of every third page's values: seams
    coincide with bucket changes"""
    ref, edges = ref_of(key), edges_of(key)
    out = set()
    for p, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        v = ref.vals[a:b][ref.valid[a:b]]
        if v.size:
            out.add(v.min().item())
            if p % 3 == 0:
                out.add(np.sort(v)[v.size // 2].item())
    return np.array(sorted(out), ref.vals.dtype)


def group_ids(key, n_groups, seed=0):
    """ids below n_groups at random, and n_groups itself -- out of range -- on about one row in fifty"""
    rng = np.random.default_rng(seed_of("ids", key_id(key), n_groups, seed))
    rows = ref_of(key).rows
    ids = rng.integers(0, n_groups, rows)
    ids[rng.integers(0, rows, rows // 50 + 1)] = n_groups
    return ids


# ---------------------------------------------------------------- can a float column tell the slot orders apart?
def _sequential(xs):
    s = 0.0
    for x in xs:
        s += x
    return s


def sums_by_order(key, mask):
    """(the double sum of the live rows with the RLE pages first, page by page, then the tiles of the other pages, the same
    in row order): each part sequentially, the parts in order.  Not the device's orders -- a lane keeps its own accumulator --
    but a column whose sums differ between them has the digits to show a record that is combined twice or not at all."""
    ref, edges, rts = ref_of(key), edges_of(key), routes(key)
    live = ref.valid if mask is None else (ref.valid & mask)
    v = ref.vals.astype(np.float64)
    part = lambda a, b: _sequential(v[a:b][live[a:b]].tolist())
    spans = list(zip(edges[:-1].tolist(), edges[1:].tolist()))
    page_slots = [part(a, b) for (a, b), r in zip(spans, rts) if r == "R"]
    tile_slots = [part(t, min(t + TILE_ROWS, b)) for (a, b), r in zip(spans, rts) if r != "R" for t in range(a, b, TILE_ROWS)]
    return _sequential(page_slots + tile_slots), part(0, ref.rows)
