"""The case table of tests/test_gpu_replay_routes.py: the decoded route of the six sink kinds that have one, per codec.

When a sink call meets a primitive Freq page the interval is issued again (replay_interval, strawboat_amd/csrc/sb_api.hip)
and, in that replay, sb_filter_columns(_var), sb_filter_columns_in, sb_read_selected, sb_topk_columns and sb_key_ids send
EVERY numeric column through decode_for_replay and their k_*_plain kernels -- also the columns of calls that held no Freq
page.  So each kind has a second implementation for every codec, type and null layout, which runs only when some other
call of the interval holds a Freq page.  (sb_aggregate_columns decodes only the columns that met a Freq page themselves,
like the grouped calls: the order of a float sum's additions belongs to the route.)  Both routes must give the same bytes.

No fixtures, no tests, no device: tests/test_replay_cases.py walks the same table on the CPU.

A case is a victim kind, a victim column (no Freq page in it), a trigger (a sparse Int64 column with Freq pages) and an
order.  The victim is one or more calls of its kind over the victim column; the trigger is
  a   a filter_columns call on the Freq column, a call of its own, enqueued before or after the victim;
  b   an aggregate_columns call on it, likewise;
  c   a further column of the victim's own (first) call, at index 1: the take_if split, the users mapping and the order of
      the results are exercised.
Variants: `chain` takes the selection from a filter_columns call (SET) and a filter_in call (AND) of the same interval, so
a device-written bitmap crosses the stream synchronize inside decode_for_replay; `mixed` puts an IS_NULL column and a Utf8
column -- which the split leaves on the page route -- into the call of a numeric comparison column.

Every page comes from the oracle's writer and every expectation from the oracle's decode, reduced by the references of the
kinds' own suites."""
import functools
import zlib

import numpy as np

from oracle import sbo as S
from tests import aggregate_grouped_ref as G
from tests import aggregate_ref as R
from tests import gen
from tests import key_ids_ref as K
from tests import topk_ref as T

ROWS, PAGE_ROWS, TILE_ROWS = 10_000, 2050, 4096
PACKED, PACKED_ROWS, PACKED_PAGE_ROWS = ("bitpack", "deltabp"), 128 * 78, 128 * 17
LONG_RLE_ROWS = (1 << 18) + 5   # tests/test_gpu_decode.py: the shortest page that several workgroups share
KINDS = ("filter", "filter_in", "read_selected", "aggregate", "topk", "key_ids")
FILTER_KINDS = ("filter", "filter_in")
FLOATS = (S.T_F32, S.T_F64)
NP = gen.NP_OF
TYPE_NAMES = {S.T_I8: "i8", S.T_I16: "i16", S.T_I32: "i32", S.T_I64: "i64", S.T_U8: "u8", S.T_U16: "u16", S.T_U32: "u32",
              S.T_U64: "u64", S.T_F32: "f32", S.T_F64: "f64"}
# name -> (the page codec, the index codec of a Dict page or None)
CODECS = {"none": (S.NONE, None), "rle": (S.RLE, None), "onevalue": (S.ONEVALUE, None), "dict_none": (S.DICT, S.NONE),
          "dict_lz4": (S.DICT, S.LZ4), "bitpack": (S.BITPACK, None), "deltabp": (S.DELTABP, None), "lz4": (S.LZ4, None),
          "zstd": (S.ZSTD, None), "patas": (S.PATAS, None), "long_rle": (S.RLE, None)}
ONEVALUE_FLOAT, ONEVALUE_INT = 0.1, 7
KEY_MAX_KEYS, KEY_FEW_KEYS = 1024, 4
TRIGGERS = (("a", "before"), ("a", "after"), ("b", "before"), ("b", "after"), ("c", "inside"))


def seed_of(*names):
    return zlib.crc32("/".join(str(n) for n in names).encode())


# ---------------------------------------------------------------- columns
class Column:
    """A victim column: `recipe` says how its values are drawn (plain: small integers; inexact: floats whose sums are exact
    in no order; keys: at most 1024 distinct integers; many: more distinct integers than KEY_MAX_KEYS)."""

    def __init__(self, codec, ptype, nullable=True, recipe="plain"):
        self.codec, self.ptype, self.nullable, self.recipe = codec, ptype, nullable, recipe
        # (the bit-packed codecs take pages of whole 128-value blocks only: the nearest shape with five pages, a short last
        # one and the tile borders inside pages)
        self.rows = LONG_RLE_ROWS if codec == "long_rle" else PACKED_ROWS if codec in PACKED else ROWS
        self.page_rows = None if codec == "long_rle" else PACKED_PAGE_ROWS if codec in PACKED else PAGE_ROWS
        self.name = "%s-%s%s%s" % (codec, TYPE_NAMES[ptype], "" if nullable else "-nn", "" if recipe == "plain" else "-" + recipe)
        self.id = "%s/%s" % (recipe, self.name)

    def __repr__(self):
        return self.name


def _values(c, rng):
    dt, rows = NP[c.ptype], c.rows
    if c.codec == "onevalue":
        return np.full(rows, ONEVALUE_FLOAT if c.ptype in FLOATS else ONEVALUE_INT, dt)
    if c.recipe == "inexact":
        return G.inexact_values(rows, 1, int(rng.integers(0, 1 << 30)))[0].astype(dt)
    if c.recipe == "many":
        return rng.integers(0, 5000, rows).astype(dt)
    if c.codec == "patas":
        return np.round(rng.normal(100, 20, rows), 2).astype(dt)
    if c.codec in ("bitpack", "deltabp"):
        v = rng.integers(0, 1000 if c.recipe == "keys" else 1 << 13, rows)
        return (np.sort(v) if c.codec == "deltabp" else v).astype(dt)
    if c.codec in ("rle", "long_rle"):
        mean = 32 if c.codec == "long_rle" else 6
        nrun = rows // mean + 1
        v = np.repeat(rng.integers(0, 100, nrun), rng.geometric(1.0 / mean, nrun))[:rows]
        return np.concatenate([v, np.full(rows - v.size, 3)]).astype(dt)
    return rng.integers(0, 100, rows).astype(dt)


# columns whose first seed gave sums that are the same page by page and tile by tile (tests/test_replay_cases.py): another seed
SALT = {"inexact/dict_lz4-f32-inexact": 1}


def build_column(c):
    """the column as gen's dict, from the seed of its name"""
    rng = np.random.default_rng(seed_of("victim", c.id, SALT.get(c.id, 0)))
    values = _values(c, rng)
    validity = gen.make_validity(rng, c.rows, 0.1) if c.nullable else None
    return dict(ptype=c.ptype, nullable=c.nullable, rows=c.rows, values=values, validity=validity, offsets=None)


def write_options(c):
    codec, icodec = CODECS[c.codec]
    opt = dict(force_codec=codec)
    if c.page_rows:
        opt["max_page_size"] = c.page_rows
    if icodec is not None:
        opt["force_index_codec"] = icodec
    return opt


_INT_SMALL = (S.T_I32, S.T_U16, S.T_I8, S.T_U32, S.T_I16, S.T_U8)
_INT_BIG = (S.T_I64, S.T_U64)
_ANY_SMALL = _INT_SMALL + (S.T_F32,)
_ANY_BIG = (S.T_I64, S.T_F64, S.T_U64)


def columns_of(kind):
    """one type of at most 4 bytes and one of 8 bytes per codec, out of the types the kind's own suite uses; Bitpack and
    DeltaBP hold 32-bit integers only, and Patas Float64 only (the format's Float32 decode is broken, so the oracle writes none)"""
    out = []
    for i, codec in enumerate(("none", "rle", "onevalue", "dict_none", "dict_lz4", "lz4", "zstd")):
        if kind == "aggregate":
            out += [Column(codec, S.T_F32, recipe="inexact"), Column(codec, S.T_F64, recipe="inexact")]
        elif kind == "key_ids":
            out += [Column(codec, _INT_SMALL[i % 6], recipe="keys"), Column(codec, _INT_BIG[i % 2], recipe="keys")]
        else:
            out += [Column(codec, _ANY_SMALL[(i + KINDS.index(kind)) % 7]), Column(codec, _ANY_BIG[(i + KINDS.index(kind)) % 3])]
    recipe = "keys" if kind == "key_ids" else "plain"
    for codec in ("bitpack", "deltabp"):
        out += [Column(codec, S.T_I32, recipe=recipe), Column(codec, S.T_U32, recipe=recipe)]
    if kind == "aggregate":
        out += [Column("patas", S.T_F64, recipe="inexact"), Column("long_rle", S.T_F64, recipe="inexact"), Column("rle", S.T_F64, nullable=False, recipe="inexact"),
                Column("rle", S.T_I64), Column("none", S.T_I16)]   # (integers: 128-bit sums, sign extension)
    elif kind == "key_ids":
        out += [Column("long_rle", S.T_I64, recipe="keys"), Column("rle", S.T_I64, nullable=False, recipe="keys"),
                Column("none", S.T_I64, recipe="many")]   # (overflows KEY_MAX_KEYS)
    else:
        out += [Column("patas", S.T_F64), Column("long_rle", S.T_I64), Column("rle", S.T_F64, nullable=False)]
    return out


def extra_columns():
    """the columns of the variants: the sources of the chained selection, and the Utf8 column of the mixed filter call"""
    return {"chain-x": (gen.prim(S.T_I32, ROWS, uniq=100, null_density=0.2, seed=4), dict(max_page_size=777, force_codec=S.DICT)),
            "chain-y": (gen.prim(S.T_I64, ROWS, uniq=100, null_density=0.1, runs=6, seed=5), dict(max_page_size=PAGE_ROWS, force_codec=S.RLE)),
            "mixed-s": (gen.binary(ROWS, uniq=60, null_density=0.1, seed=3, maxlen=20), dict(max_page_size=PAGE_ROWS, force_codec=S.DICT))}


def trigger_column(rows):
    """a sparse Int64 column of the victim's row count: one value on 95 % of the rows, Freq pages"""
    from tests.test_gpu_freq import sparse
    return sparse(S.T_I64, rows, 0.05, 2, null_density=0.1)


def trigger_id(rows):
    return "trigger-%d" % rows


_VICTIMS = {}


@functools.lru_cache(maxsize=None)
def written(col_id):
    """(col, pages, metas) of a column of the table: written once, never modified"""
    if col_id.startswith("trigger-"):
        col = trigger_column(int(col_id[8:]))
        opt = dict(max_page_size=PAGE_ROWS, force_codec=S.FREQ)
    elif col_id in _VICTIMS:
        col, opt = build_column(_VICTIMS[col_id]), write_options(_VICTIMS[col_id])
    else:
        col, opt = extra_columns()[col_id]
    pages, metas = gen.oracle_write(col, **opt)
    for a in (pages, metas, col["values"], col["validity"]):
        if a is not None:
            a.setflags(write=False)
    return col, pages, metas


def page_codecs(col_id):
    """(the set of page codecs, the set of inner codecs) the oracle's stat finds in a column's pages"""
    col, pages, metas = written(col_id)
    codecs, inner = S.stat_column(col["ptype"], col["nullable"], pages, metas)
    return set(int(x) for x in codecs.tolist()), set(int(x) for x in inner.tolist())


@functools.lru_cache(maxsize=None)
def ref_of(col_id):
    """the oracle's decode of a numeric column (aggregate_ref.Ref): computed once, left unchanged"""
    return R.Ref(*written(col_id))


@functools.lru_cache(maxsize=None)
def strings_of(col_id):
    """(strs, valid) of a binary column from the oracle's decode (key_ids_var_ref.Ref)"""
    from tests import key_ids_var_ref as KV
    ref = KV.Ref(*written(col_id))
    return ref.strs, ref.valid


@functools.lru_cache(maxsize=None)
def masks(rows):
    """the selections of a column of `rows` rows: a random third, a sparse one that leaves whole tiles and pages out (the
    recipe of test_gpu_read_selected.two_masks), and none"""
    rng = np.random.default_rng(11)
    sparse = np.zeros(rows, bool)
    at = int(rng.integers(0, max(1, rows - 70)))
    sparse[at:at + 70] = rng.random(min(70, rows - at)) < 0.7
    sparse[rows - 1] = True
    out = (rng.random(rows) < 0.35, sparse, None)
    for m in out[:2]:
        m.setflags(write=False)
    return out


# ---------------------------------------------------------------- calls
class Entry:
    """one column of a call: the column's id, the argument of its kind, and whether it is the trigger's"""

    def __init__(self, col, arg, trigger=False):
        self.col, self.arg, self.trigger = col, arg, trigger


class Call:
    """kind; entries; for the filter kinds: combine (set / and / or) and the buffer it works on -- `poison` (a buffer of its
    own, 0xA5), `m0` (a buffer of its own that holds masks[0], uploaded) or `chain` (the interval's shared bitmap).  role:
    victim, trigger or prelude (the two calls that write the chained selection)."""

    def __init__(self, kind, entries, role, combine="set", buffer="poison"):
        self.kind, self.entries, self.role, self.combine, self.buffer = kind, list(entries), role, combine, buffer


def _median(col_id):
    ref = ref_of(col_id)
    v = np.sort(ref.vals[ref.valid])
    return v[v.size // 2].item()


def _in_list(col_id):
    """8 literals: six drawn from the column's valid rows, two above all of them"""
    ref = ref_of(col_id)
    v = ref.vals[ref.valid]
    rng = np.random.default_rng(seed_of("in", col_id))
    hi = v.max().item()
    return tuple(v[int(i)].item() for i in rng.integers(0, v.size, 6)) + (hi + 1, hi + 2)


def entries_of(kind, col_id, chain=False):
    """the victim's entries over one column (a chained selection serves one entry of a filter kind: one bitmap)"""
    if kind == "filter":
        med = _median(col_id)
        return [Entry(col_id, ("le", med))] + ([] if chain else [Entry(col_id, ("ne", med))])
    if kind == "filter_in":
        lits = _in_list(col_id)
        return [Entry(col_id, (lits, False))] + ([] if chain else [Entry(col_id, (lits, True))])
    sel = (lambda i: "chain") if chain else (lambda i: i)
    if kind == "read_selected":
        return [Entry(col_id, sel(0)), Entry(col_id, sel(1))]
    if kind == "aggregate":
        return [Entry(col_id, sel(0)), Entry(col_id, sel(1)), Entry(col_id, None)]
    if kind == "topk":
        return [Entry(col_id, (sel(0), 16, False)), Entry(col_id, (None, 64, True)), Entry(col_id, (sel(1), 7, True))]
    return [Entry(col_id, (sel(0), KEY_MAX_KEYS, 2)), Entry(col_id, (None, KEY_MAX_KEYS, 2)), Entry(col_id, (sel(0), KEY_FEW_KEYS, 1))]


def trigger_entry(kind, rows):
    """the Freq column as one more column of a call of `kind`"""
    tid = trigger_id(rows)
    arg = {"filter": ("gt", 7), "filter_in": ((7, 301, 5000, 12345), False), "read_selected": 0, "aggregate": 0, "topk": (0, 16, False),
           "key_ids": (0, KEY_MAX_KEYS, 2)}[kind]
    return Entry(tid, arg, trigger=True)


class Case:
    def __init__(self, kind, column, trigger, order, variant="plain"):
        self.kind, self.column, self.trigger, self.order, self.variant = kind, column, trigger, order, variant
        self.name = "%s/%s/%s-%s%s" % (kind, column.name, trigger, order, "" if variant == "plain" else "/" + variant)

    def __repr__(self):
        return self.name

    def columns(self):
        """the ids of every column the case's intervals hold"""
        ids = [self.column.id, trigger_id(self.column.rows)]
        if self.variant == "chain":
            ids += ["chain-x", "chain-y"]
        if self.variant == "mixed":
            ids += ["mixed-s"]
        return ids

    def victim_calls(self):
        kind, cid = self.kind, self.column.id
        if self.variant == "chain":
            prelude = [Call("filter", [Entry("chain-x", ("le", _median("chain-x")))], "prelude", "set", "chain"),
                       Call("filter_in", [Entry("chain-y", (_in_list("chain-y"), True))], "prelude", "and", "chain")]
            if kind in FILTER_KINDS:
                return prelude + [Call(kind, entries_of(kind, cid, True), "victim", "and", "chain")]
            return prelude + [Call(kind, entries_of(kind, cid, True), "victim")]
        if self.variant == "mixed":
            strs, valid = strings_of("mixed-s")
            lit = sorted(set(strs[valid].tolist()))[30]
            return [Call("filter", [Entry(cid, ("le", _median(cid))), Entry(cid, ("is_null", None)), Entry("mixed-s", ("lt", lit))], "victim")]
        if kind in FILTER_KINDS:
            return [Call(kind, entries_of(kind, cid), "victim", "set", "poison"), Call(kind, entries_of(kind, cid), "victim", "and", "m0"),
                    Call(kind, entries_of(kind, cid), "victim", "or", "m0")]
        return [Call(kind, entries_of(kind, cid), "victim")]

    def calls(self, with_trigger):
        """the calls of one interval, in the order they are enqueued"""
        calls = self.victim_calls()
        if not with_trigger:
            return calls
        rows = self.column.rows
        if self.trigger == "c":
            first = next(c for c in calls if c.role == "victim")
            first.entries.insert(1, trigger_entry(first.kind, rows))
            return calls
        t = Call("filter" if self.trigger == "a" else "aggregate", [trigger_entry("filter" if self.trigger == "a" else "aggregate", rows)], "trigger")
        return [t] + calls if self.order == "before" else calls + [t]


def _table():
    out = []
    for kind in KINDS:
        cols = columns_of(kind)
        for c in cols:
            _VICTIMS[c.id] = c
            for trigger, order in TRIGGERS:
                out.append(Case(kind, c, trigger, order))
        chained = next(c for c in cols if c.codec == "dict_none" and c.rows == ROWS)
        for trigger, order in (("a", "before"), ("c", "inside")):
            out.append(Case(kind, chained, trigger, order, "chain"))
    mixed = next(c for c in columns_of("filter") if c.codec == "rle" and c.nullable)
    for trigger, order in TRIGGERS:
        out.append(Case("filter", mixed, trigger, order, "mixed"))
    return out


CASES = _table()
CASE = {c.name: c for c in CASES}


# ---------------------------------------------------------------- references
def mask_of(sel, rows, chain_mask):
    """the bool mask (or None: every row) of an entry's selection argument"""
    return chain_mask if sel == "chain" else None if sel is None else masks(rows)[sel]


def predicate_mask(kind, entry):
    """the rows the predicate (or the list) of a filter-kind entry matches, from the oracle's decode"""
    from tests.test_gpu_filter import expected as cmp_expected
    from tests.test_gpu_filter_binary import expected as bin_expected
    from tests.test_gpu_filter_in import want_in
    col = written(entry.col)[0]
    if col["ptype"] in (S.T_BIN32, S.T_BIN64):
        return bin_expected(*strings_of(entry.col), *entry.arg)
    ref = ref_of(entry.col)
    if kind == "filter_in":
        return want_in(col, ref.vals, ref.valid, entry.arg[0], entry.arg[1])
    return cmp_expected(col, ref.vals, ref.valid, *entry.arg)


def wants_of(calls):
    """[[want per entry] per call] of one interval: a bool array per entry of a filter kind (the bitmap after the call's
    combine), the Want of the kind's reference otherwise.  The chained bitmap is followed through the calls that write it."""
    out, chain = [], None
    for call in calls:
        wants = []
        for e in call.entries:
            rows = written(e.col)[0]["rows"]
            if call.kind in FILTER_KINDS:
                hit = predicate_mask(call.kind, e)
                shared = call.buffer == "chain" and not e.trigger   # (the trigger's entry of such a call works on masks[0])
                base = chain if shared else masks(rows)[0]
                final = hit if call.combine == "set" else (base & hit) if call.combine == "and" else (base | hit)
                if shared:
                    chain = final
                wants.append(final)
                continue
            sel = e.arg if call.kind in ("read_selected", "aggregate") else e.arg[0]
            if sel == "chain":
                wants.append(_want(call.kind, e.col, e.arg, chain))
            else:
                key = (call.kind, e.col, e.arg)
                if key not in _WANTS:
                    _WANTS[key] = _want(call.kind, e.col, e.arg, None)
                wants.append(_WANTS[key])
        out.append(wants)
    return out


_WANTS = {}   # the references under the uploaded masks: computed once, left unchanged


def _want(kind, col_id, arg, chain):
    ref = ref_of(col_id)
    if kind == "read_selected":
        return mask_of(arg, ref.rows, chain)
    if kind == "aggregate":
        return ref.want(mask_of(arg, ref.rows, chain))
    if kind == "topk":
        return T.want(ref, mask_of(arg[0], ref.rows, chain), arg[1], arg[2])
    return K.want(ref, mask_of(arg[0], ref.rows, chain), arg[1], arg[2])


# ---------------------------------------------------------------- can a float column tell the routes apart?
def _sequential(xs):
    s = 0.0
    for x in xs:
        s += x
    return s


def sums_by_route(col_id, mask):
    """(the double sum of the live rows added page by page, the same tile by tile): each part sequentially, the parts in
    order.  Not the device's orders -- a lane keeps its own accumulator -- but two orders whose parts are the two routes'
    slots; a column whose sums differ between them has the digits to show a change of route."""
    col, pages, metas = written(col_id)
    ref = ref_of(col_id)
    live = ref.valid if mask is None else (ref.valid & mask)
    v = ref.vals.astype(np.float64)
    edges = np.concatenate([[0], np.cumsum(np.asarray(metas)[:, 1].astype(np.int64))])
    by_page = _sequential(_sequential(v[a:b][live[a:b]].tolist()) for a, b in zip(edges[:-1], edges[1:]))
    by_tile = _sequential(_sequential(v[a:a + TILE_ROWS][live[a:a + TILE_ROWS]].tolist()) for a in range(0, ref.rows, TILE_ROWS))
    return by_page, by_tile


def onevalue_sums(col_id, mask):
    """(n * v, n additions of v) for the live rows of a OneValue column's first page"""
    col, pages, metas = written(col_id)
    ref = ref_of(col_id)
    n0 = int(np.asarray(metas)[0, 1])
    live = ref.valid[:n0] if mask is None else (ref.valid & mask)[:n0]
    n, v = int(live.sum()), float(ref.vals[0])
    return v * n, _sequential([v] * n)
