"""The case table of tests/test_gpu_write_hints.py: what an adaptive sb_write_columns call launches depends on what the last
two completed calls with its plan chose (sb_ctx::EncPlan last_counts / prev_counts / counts_valid: apply_enc_hint in
strawboat_amd/csrc/sb_api.hip, EncLaunch::unused in sb_encode.hip), so every kind of page is crossed with every history of
a context.  No fixtures, no tests, no device: tests/test_write_hint_cases.py walks the same table on the CPU.

A variant is the data of one column of a fixed shape; the variants of a table share every field of the plan key
(plan_lookup), so they hit one plan.  A case is a history (intervals on a context of its own), a probe interval, an entry
point, and the replays (sb_ctx_replays) every interval must cost.  The counts are not typed in: `page_slots` derives from
the oracle's pages which slots of codec_counts[32] a call fills (`counts`) and which of the slots the host consults it
cannot do without (`required`); `Model` restates apply_enc_hint and the skipping in Python.

The device's rules as the model restates them (sb_encode.hip unless named):
  * k_enc_select / k_enc_select_runs / k_enc_select_rle / k_enc_bin_page / big_decide count a page under its codec id.  A
    4- / 8-byte RLE page that the fused selector wrote itself (`kept`) counts nowhere and needs no further kernel.
  * slot 31 (HINT_ROW_SELECT): a 4- / 8-byte page with more than RUNS_CAP raw runs in one chunk of 4096 rows
    (sb_select_runs.h, `fallback`), and every page of SEL_BIG_ROWS rows and more (counted, but written by launch_big
    whether k_enc_select_rle runs or not).
  * slot 29 (HINT_RLE_EMIT): RLE pages k_enc_emit_pages<., RLE> wrote.  For 4- / 8-byte pages those are the pages whose
    speculation was stopped (`nrec * 4 > cb + n + 256` after a chunk, sb_select_rle.h / sb_select_runs.h) and which
    chose RLE all the same.  RLE pages of the other kinds go by the codec-id slot and leave this one alone.
  * slot 30 (HINT_BIN_DICT_EMIT): binary Dict pages k_enc_emit_pages<-4, Dict> wrote: with SB_BIN_FUSED on, those whose
    index block is not bit-packed (k_enc_bin_page finishes the others); with it off, all of them, and the launch goes by
    the DICT slot instead.
  * both slots are counted by k_enc_emit_pages for pages of the instance's own kind.  (Found by the mixed-kind cases and
    fixed: counted before the kernel's kind check, an Int16 Dict page made the binary instance count slot 30 -- or not,
    when the binary chain on its side stream ran ahead of the Int16 selector -- so the same history cost one replay or
    none; and every instance counted slot 29.)
  * slot 28 (HINT_FREQ) is freq_count: every Freq page, short or long.  Slot 13 (FREQ) counts the same pages, so the two
    are never apart; launch_freq goes by 28, launch_freq_big and SKIP_FREQ_BIG by 13.
  * LZ4, ZSTD and SNAPPY are consulted jointly (the Basic block chain is left out only when all three are 0).
  * inner codecs (a Dict page's index block, a Freq page's exceptions block) are written by the page's own kernels and
    count nowhere, except for the virtual pages of long pages on the section-parallel path (sb_dict_big.h, sb_freq_big.h:
    the index array of a long Dict page, an exceptions block of VBIG_ROWS rows and more), which big_decide counts under
    their codec id.  Kept as found: that makes the next call with the plan launch, say, k_enc_emit_pages<4, Bitpacking>
    for no page.
  * long RLE pages are written section-parallel (k_rle_big_*, launched by launch_big without a hint): they need no slot.
  * a hit with counts_valid, an adaptive call and no SB_NO_HINTS leaves out the launches whose slot is 0 in last_counts;
    a page that needed one stays unwritten, k_enc_layout raises KIND_REPLAY and the interval is issued once more with
    everything launched.  Only the replay's ENC_HINT records exist when the interval ends (release_interval drops the
    first pass's), and each does last = max(now, prev), prev = now, in call order, if its key is still the context's plan.
  * a plan miss is never hinted (`hit &&` in big_hint), and build_plan clears counts_valid and prev_counts: nothing of the
    plan before it survives, neither as a hint nor in the maximum that the new plan's first call takes.
"""
import zlib

import numpy as np

from oracle import sbo as S
from tests import gen
from tests import hint_cases as H

# ---------------------------------------------------------------- constants (tests/test_write_hint_cases.py reads them out of the sources)
RUNS_CAP = 640
SEL_BIG_ROWS = 1 << 18
VBIG_ROWS = 65536
BP_MIN_ROWS = 512
CHUNK_ROWS = 4096
HINT_FREQ, HINT_RLE_EMIT, HINT_BIN_DICT_EMIT, HINT_ROW_SELECT = 28, 29, 30, 31
SKIP_DICT_BIG, SKIP_FREQ_BIG, SKIP_EMIT = 1, 2, 4
BASIC = "basic"   # the joint slot of LZ4, ZSTD and SNAPPY
BASIC_IDS = (S.LZ4, S.ZSTD, S.SNAPPY)
# every slot the host consults (EncLaunch::unused / unused_peek): a case must cross each
CONSULTED = (S.NONE, BASIC, S.ONEVALUE, S.DICT, S.RLE, S.BITPACK, S.DELTABP, S.PATAS, S.FREQ,
             HINT_FREQ, HINT_RLE_EMIT, HINT_BIN_DICT_EMIT, HINT_ROW_SELECT)
SLOT_NAMES = {S.NONE: "NONE", BASIC: "LZ4|ZSTD|SNAPPY", S.ONEVALUE: "ONEVALUE", S.DICT: "DICT", S.RLE: "RLE", S.BITPACK: "BITPACKING",
              S.DELTABP: "DELTA_BITPACKING", S.PATAS: "PATAS", S.FREQ: "FREQ", HINT_FREQ: "HINT_FREQ", HINT_RLE_EMIT: "HINT_RLE_EMIT",
              HINT_BIN_DICT_EMIT: "HINT_BIN_DICT_EMIT", HINT_ROW_SELECT: "HINT_ROW_SELECT"}

ROWS, PAGE = 32768, 8192
MEM_DEVICE, MEM_HOST = "device", "host"


def seed_of(*names):
    return zlib.crc32("/".join(names).encode())


# ---------------------------------------------------------------- tables and variants
class Table:
    """the shape its variants share: every field of the plan key but the data"""

    def __init__(self, name, ptype, rows, options, values_len=None):
        self.name, self.ptype, self.rows, self.options, self.values_len = name, ptype, rows, dict(options), values_len
        self.variants = {}

    def add(self, name, build, doc):
        self.variants[name] = Variant(self, name, build, doc)

    def page_rows(self):
        ps = self.options.get("max_page_size") or self.rows
        return [min(ps, self.rows - r) for r in range(0, self.rows, ps)]


class Variant:
    def __init__(self, table, name, build, doc):
        self.table, self.name, self.build, self.doc = table, name, build, doc
        self.full = "%s/%s" % (table.name, name)

    def column(self):
        """the column: the same bytes every time"""
        t = self.table
        out = self.build(np.random.default_rng(seed_of(self.full)), t.rows)
        offsets = None
        if isinstance(out, tuple):
            out, offsets = out
        return dict(ptype=t.ptype, nullable=False, rows=t.rows, values=out, validity=None, offsets=offsets)

    def __repr__(self):
        return self.full


SHORT = dict(max_page_size=PAGE, ratio=2.0, forbidden=())


def _runs(rng, rows, length, hi, dtype, lo=0):
    return np.repeat(rng.integers(lo, hi, rows // length + 1), length)[:rows].astype(dtype)


def _mostly(rng, rows, dtype, top, hi, p=0.03, lo=0):
    v = np.full(rows, top, dtype)
    m = rng.random(rows) < p
    v[m] = rng.integers(lo, hi, int(m.sum()))
    return v


def _rle_emit_page(rng, dtype):
    """short runs (3 rows) in the first chunk -- the selector stops speculating -- and runs of 64 behind"""
    head = np.repeat(rng.integers(0, 1 << 30, CHUNK_ROWS // 3 + 1), 3)[:CHUNK_ROWS]
    return np.concatenate([head, np.repeat(rng.integers(0, 1 << 30, (PAGE - CHUNK_ROWS) // 64), 64)]).astype(dtype)


def _one_page_each(rng, rows):
    assert rows == 4 * PAGE
    return np.concatenate([np.full(PAGE, 7), rng.integers(0, 400, PAGE), np.repeat(rng.integers(0, 1 << 30, PAGE // 64), 64),
                           rng.integers(0, 1 << 30, PAGE)]).astype(np.int32)


def _int32_variants(t, lz4):
    i32 = np.int32
    t.add("uniform", lambda rng, n: rng.integers(0, 1 << 30, n).astype(i32), "LZ4 pages" if lz4 else "plain pages (the tiles)")
    t.add("const", lambda rng, n: np.full(n, 7, i32), "OneValue")
    t.add("dict400", lambda rng, n: (rng.integers(0, 400, n) * 100003).astype(i32), "Dict, bit-packed index")
    t.add("small", lambda rng, n: rng.integers(0, 400, n).astype(i32), "Bitpacking, left to the row-level selector")
    t.add("small_runs7", lambda rng, n: _runs(rng, n, 7, 256, i32), "Bitpacking, decided by the run-level selector")
    t.add("freq", lambda rng, n: _mostly(rng, n, i32, 1_000_000, 1 << 30), "Freq, %s exceptions block" % ("an LZ4" if lz4 else "a plain"))
    t.add("freq_small", lambda rng, n: _mostly(rng, n, i32, 1_000_000, 400, p=0.08), "Freq, the exceptions block with a codec of its own")
    if lz4:
        return
    t.add("dict_runs", lambda rng, n: (_runs(rng, n, 64, 50, np.int64) * 100003).astype(i32), "Dict, RLE index")
    t.add("runs64", lambda rng, n: _runs(rng, n, 64, 1 << 30, i32), "RLE, written by the fused selector (kept)")
    t.add("sorted", lambda rng, n: np.sort(rng.integers(0, 1 << 16, n)).astype(i32), "DeltaBitpacking")
    t.add("rle_emit", lambda rng, n: np.tile(_rle_emit_page(rng, i32), n // PAGE), "RLE after the selector stopped speculating")
    t.add("one_page_each", _one_page_each, "[OneValue | Bitpacking | RLE | plain]")


def _words(ids, words):
    vals = np.frombuffer(b"".join(words[i] for i in ids), np.uint8).copy()
    return vals, (np.arange(len(ids) + 1, dtype=np.int32) * len(words[0]))


def _tables():
    out = []
    t = Table("i32", S.T_I32, ROWS, SHORT)
    _int32_variants(t, False)
    out.append(t)
    t = Table("i32lz4", S.T_I32, ROWS, dict(SHORT, default_compression=S.LZ4))
    _int32_variants(t, True)
    out.append(t)

    i64 = np.int64
    t = Table("i64", S.T_I64, ROWS, SHORT)
    t.add("uniform", lambda rng, n: rng.integers(0, 1 << 60, n).astype(i64), "plain pages")
    t.add("runs4", lambda rng, n: _runs(rng, n, 4, 1 << 40, i64), "Dict, DeltaBitpacking index")
    t.add("runs64", lambda rng, n: _runs(rng, n, 64, 1 << 60, i64), "RLE, kept")
    t.add("freq", lambda rng, n: _mostly(rng, n, i64, 1 << 40, 1 << 60), "Freq, plain exceptions block")
    t.add("freq_dict", lambda rng, n: _mostly(rng, n, i64, 1, 5, p=0.05, lo=2) << 40, "Freq, Dict exceptions block")
    out.append(t)

    t = Table("f64", S.T_F64, ROWS, dict(SHORT, ratio=1.2))
    t.add("uniform", lambda rng, n: rng.integers(0, 1 << 62, n).astype(np.uint64).view(np.float64), "plain pages")
    t.add("patas", lambda rng, n: rng.integers(0, 1 << 20, n) / 8.0, "Patas")
    t.add("const", lambda rng, n: np.full(n, 2.5), "OneValue")
    t.add("runs64", lambda rng, n: _runs(rng, n, 64, 1 << 30, np.float64) / 8.0, "RLE, kept")
    out.append(t)

    i16 = np.int16
    t = Table("i16", S.T_I16, ROWS, SHORT)
    t.add("uniform", lambda rng, n: rng.integers(-30000, 30000, n).astype(i16), "plain pages")
    t.add("runs64", lambda rng, n: _runs(rng, n, 64, 30000, i16, lo=-30000), "RLE pages of k_enc_emit_pages<2, RLE>")
    t.add("runs256", lambda rng, n: _runs(rng, n, 256, 30000, i16, lo=-30000), "Dict, RLE index")
    t.add("dict40", lambda rng, n: (rng.integers(0, 40, n) * 701).astype(i16), "Dict")
    t.add("const", lambda rng, n: np.full(n, 5, i16), "OneValue")
    t.add("freq", lambda rng, n: _mostly(rng, n, i16, 1000, 30000, lo=-30000), "Freq")
    out.append(t)

    t = Table("bool", S.T_BOOL, ROWS, SHORT)
    t.add("random", lambda rng, n: gen.pack_bits(rng.random(n) < 0.5), "plain pages")
    t.add("runs100", lambda rng, n: gen.pack_bits(_runs(rng, n, 100, 2, bool)), "RLE and plain pages")
    t.add("runs1000", lambda rng, n: gen.pack_bits(_runs(rng, n, 1000, 2, bool)), "RLE pages")
    t.add("const", lambda rng, n: gen.pack_bits(np.ones(n, bool)), "OneValue")
    out.append(t)

    brows = 2 * PAGE
    words = [b"w%05d" % k for k in range(brows)]
    t = Table("bin", S.T_BIN32, brows, SHORT, values_len=brows * 6)
    t.add("scattered", lambda rng, n: _words(rng.integers(0, 800, n), words), "Dict, bit-packed index: finished by k_enc_bin_page")
    t.add("in_runs", lambda rng, n: _words(np.repeat(rng.integers(0, 800, n // 64), 64), words), "Dict, RLE index: the page kernel's")
    t.add("const", lambda rng, n: _words(np.zeros(n, np.int64), words), "OneValue")
    t.add("unique", lambda rng, n: _words(rng.permutation(n), words), "plain pages")
    out.append(t)

    i32 = np.int32
    t = Table("long", S.T_I32, SEL_BIG_ROWS, dict(ratio=2.0, forbidden=()))
    t.add("uniform", lambda rng, n: rng.integers(0, 1 << 30, n).astype(i32), "a plain page")
    t.add("dict400", lambda rng, n: (rng.integers(0, 400, n) * 100003).astype(i32), "a long Dict page (SKIP_DICT_BIG)")
    t.add("freq", lambda rng, n: _mostly(rng, n, i32, 1_000_000, 1 << 30), "a long Freq page (SKIP_FREQ_BIG, launch_freq_big)")
    t.add("runs64", lambda rng, n: _runs(rng, n, 64, 1 << 30, i32), "a long RLE page (k_rle_big_*)")
    t.add("dict_runs", lambda rng, n: (_runs(rng, n, 64, 50, np.int64) * 100003).astype(i32), "a long Dict page, RLE index")
    out.append(t)

    # another shape: the plan miss between two calls of one shape, and the write that closes a case
    t = Table("other", S.T_I32, PAGE, dict(ratio=2.0, forbidden=()))
    t.add("uniform", lambda rng, n: rng.integers(0, 1 << 30, n).astype(i32), "a plain page")
    out.append(t)
    return out


TABLES = {t.name: t for t in _tables()}
VARIANT = {v.full: v for t in TABLES.values() for v in t.variants.values()}


# ---------------------------------------------------------------- from pages to slots
def kind_of(ptype):
    """the column kind of write_columns_impl: the width, 0 Boolean, -4 / -8 binary"""
    return 0 if ptype == S.T_BOOL else -4 if ptype == S.T_BIN32 else -8 if ptype == S.T_BIN64 else S.WIDTH[ptype]


def raw_runs_fallback(page_values):
    """sb_select_runs.h: a chunk of 4096 rows with more than RUNS_CAP raw runs (every chunk starts one) leaves the page
    to the row-level selector.  page_values: the page's rows as unsigned bit patterns, no nulls"""
    chg = np.ones(page_values.size, bool)
    chg[1:] = page_values[1:] != page_values[:-1]
    for cb in range(0, page_values.size, CHUNK_ROWS):
        c = chg[cb:cb + CHUNK_ROWS].copy()
        c[0] = True
        if int(c.sum()) > RUNS_CAP:
            return True
    return False


def speculation_stopped(page_values, slack=0):
    """`nrec * 4 > cb + n + 256` after a chunk: nrec = the run records written so far (the value changes of a page without
    nulls).  slack: records more or fewer than that -- a claim must not depend on the one record of the first row"""
    chg = np.zeros(page_values.size, bool)
    chg[1:] = page_values[1:] != page_values[:-1]
    nrec = np.cumsum(chg)
    for end in range(CHUNK_ROWS, page_values.size + CHUNK_ROWS, CHUNK_ROWS):
        end = min(end, page_values.size)
        if (int(nrec[end - 1]) + slack) * 4 > end + 256:
            return True
    return False


def page_slots(col, pages, metas, bin_fused=True):
    """(counts, required) of one column's pages as the oracle wrote them: the slots of codec_counts a call with every
    kernel launched leaves non-zero, and the consulted slots without which a page of the column stays unwritten"""
    t = col["ptype"]
    kd = kind_of(t)
    codecs, inner = S.stat_column(t, col["nullable"], pages, metas)
    counts, required = set(), set()
    assert not col["nullable"], "the table's columns have no nulls"
    bits = None
    if kd in (4, 8):
        bits = np.ascontiguousarray(col["values"]).view(np.uint32 if kd == 4 else np.uint64)
    row0 = 0
    for k, (page, rows) in enumerate(H.pages_of(pages, metas)):
        cd, ic = int(codecs[k]), int(inner[k])
        long_page = rows >= SEL_BIG_ROWS
        assert not (long_page and kd != 4), "the table's long pages are Int32"
        kept = False
        if kd in (4, 8):
            pv = bits[row0:row0 + rows]
            if long_page:
                counts.add(HINT_ROW_SELECT)            # counted; launch_big takes the page whatever k_enc_select_rle does
            elif raw_runs_fallback(pv):
                counts.add(HINT_ROW_SELECT)
                required.add(HINT_ROW_SELECT)
            if cd == S.RLE and not long_page:
                stopped = speculation_stopped(pv)
                assert stopped == speculation_stopped(pv, 1) == speculation_stopped(pv, -1), "an RLE page on the edge of the early stop"
                kept = not stopped
        if not kept:
            counts.add(cd)
        if cd in BASIC_IDS:
            required.add(BASIC)
        elif cd == S.FREQ:
            counts.add(HINT_FREQ)
            required.add(HINT_FREQ)
            if long_page:
                required.add(S.FREQ)
                n_ex = H.walk_page(t, False, page)["exceptions"].usize // S.WIDTH[t]
                if n_ex >= VBIG_ROWS:
                    counts.add(ic)
        elif cd == S.RLE:
            if kd in (4, 8):
                if not kept and not long_page:
                    counts.add(HINT_RLE_EMIT)
                    required.add(HINT_RLE_EMIT)
            else:
                required.add(S.RLE)
        elif cd == S.DICT:
            if kd < 0:
                assert BP_MIN_ROWS <= rows <= 65536, "the table's binary pages are k_enc_bin_page's"
                if not bin_fused:
                    counts.add(HINT_BIN_DICT_EMIT)
                    required.add(S.DICT)
                elif ic != S.BITPACK:
                    counts.add(HINT_BIN_DICT_EMIT)
                    required.add(HINT_BIN_DICT_EMIT)
            else:
                required.add(S.DICT)
                if long_page:
                    counts.add(ic)                     # the index array: a virtual page on the section-parallel path
        else:
            required.add(cd)                           # NONE (the tiles), ONEVALUE, BITPACKING, DELTA_BITPACKING, PATAS
        row0 += rows
    return frozenset(counts), frozenset(required)


_written = {}


def written(variant):
    """(col, pages, metas) of a variant: the oracle's pages, written once, shared, never modified"""
    if variant.full not in _written:
        col = variant.column()
        pages, metas = gen.oracle_write(col, **variant.table.options)
        for a in (pages, metas, col["values"], col["offsets"]):
            if a is not None:
                a.setflags(write=False)
        _written[variant.full] = (col, pages, metas)
    return _written[variant.full]


_needs = {}


def needs(variant, bin_fused=True):
    """(counts, required) of a call that writes the variant alone"""
    k = (variant.full, bool(bin_fused))
    if k not in _needs:
        _needs[k] = page_slots(*written(variant), bin_fused=bin_fused)
    return _needs[k]


# ---------------------------------------------------------------- the model
def _satisfied(slot, last):
    return bool(last & set(BASIC_IDS)) if slot == BASIC else slot in last


class Model:
    """The launch-hint state of one context's encode plan.  Only zero / non-zero matters to EncLaunch::unused, so the
    counts are sets of non-zero slots: max() is a union."""

    def __init__(self, no_hints=False):
        self.no_hints = no_hints
        self.key, self.valid, self.prev, self.last = None, False, frozenset(), frozenset()

    def _lookup(self, key):
        if key != self.key:        # build_plan
            self.key, self.valid, self.prev = key, False, frozenset()
            return False
        return True

    def interval(self, calls):
        """calls: [(key, counts, required)] between two synchronizes; returns the replays it costs (0 or 1)"""
        replay = False
        for key, counts, required in calls:
            hit = self._lookup(key)
            if hit and self.valid and not self.no_hints and not all(_satisfied(s, self.last) for s in required):
                replay = True
        if replay:                 # issued again without hints; the first pass's records are gone
            for key, counts, required in calls:
                self._lookup(key)
        for key, counts, required in calls:   # apply_enc_hint, in call order
            if key == self.key:
                self.last, self.prev, self.valid = counts | self.prev, counts, True
        return 1 if replay else 0


# ---------------------------------------------------------------- cases
def call_of(*variant_names, mem=MEM_DEVICE):
    """one sb_write_columns call: its columns, in order"""
    return (tuple(variant_names), mem)


def model_call(call, bin_fused=True, slots=None):
    """(key, counts, required) of a call; slots: {variant: (counts, required)} in place of needs()"""
    names, mem = call
    counts, required = set(), set()
    for n in names:
        c, r = slots[n] if slots is not None else needs(VARIANT[n], bin_fused)
        counts |= c
        required |= r
    return (tuple(VARIANT[n].table.name for n in names), mem), frozenset(counts), frozenset(required)


class Case:
    """name; history: intervals (tuples of calls) on a context of its own; probe: the interval that is judged, issued twice;
    entry: device, two_calls, two_plans, host or mixed"""

    def __init__(self, name, history, probe, entry="device"):
        self.name, self.history, self.probe, self.entry = name, tuple(history), tuple(probe), entry

    def intervals(self):
        return self.history + (self.probe, self.probe)

    def variants(self):
        return sorted({n for iv in self.intervals() for names, _ in iv for n in names})

    def expected(self, no_hints=False, bin_fused=True, slots=None):
        """the replays of every history interval, of the probe and of the probe again"""
        m = Model(no_hints)
        return tuple(m.interval([model_call(c, bin_fused, slots) for c in iv]) for iv in self.intervals())

    def crossed(self, bin_fused=True):
        """the consulted slots the probe needs and the history's last_counts do not hold (with a valid plan hit)"""
        m = Model()
        for iv in self.history:
            m.interval([model_call(c, bin_fused) for c in iv])
        out = set()
        for c in self.probe:
            key, counts, required = model_call(c, bin_fused)
            if key == m.key and m.valid:
                out |= {s for s in required if not _satisfied(s, m.last)}
            break   # (the first call of the probe sees the history's state)
        return out

    def __repr__(self):
        return self.name


def _one(name):
    return (call_of(name),)


def _cases():
    out = []
    # the full cross of every table: history [X, X] x probe Y
    for t in TABLES.values():
        if t.name == "other":
            continue
        for x in t.variants.values():
            for y in t.variants.values():
                out.append(Case("%s-%s-after-2x-%s" % (t.name, y.name, x.name), [_one(x.full)] * 2, _one(y.full)))
    other = _one("other/uniform")
    v = lambda n: "i32/" + n
    for y in ("uniform", "const", "dict400", "rle_emit", "freq"):
        out.append(Case("i32-%s-fresh" % y, [], _one(v(y))))                                      # no hints yet
    for x, y in (("runs64", "uniform"), ("uniform", "rle_emit"), ("small", "dict400"), ("dict400", "dict400")):
        out.append(Case("i32-%s-after-1x-%s" % (y, x), [_one(v(x))], _one(v(y))))
    for x, z, y in (("uniform", "const", "uniform"), ("uniform", "const", "dict400"), ("dict400", "small", "dict400"),
                    ("small", "uniform", "rle_emit"), ("freq", "small_runs7", "freq")):
        out.append(Case("i32-%s-after-%s-%s" % (y, x, z), [_one(v(x)), _one(v(z))], _one(v(y))))   # the maximum of two
        out.append(Case("i32-%s-after-%s-2x-%s" % (y, x, z), [_one(v(x)), _one(v(z)), _one(v(z))], _one(v(y))))   # x has aged out
    for y, y2 in (("const", "uniform"), ("runs64", "dict400"), ("small", "freq")):
        out.append(Case("i32-%s-after-%s-miss" % (y2, y), [_one(v(y)), _one(v(y)), other], _one(v(y2))))   # a plan miss forgets
    for y, y2 in (("const", "uniform"), ("small_runs7", "small")):   # ... and the counts of the plan before it (prev_counts) too
        out.append(Case("i32-%s-after-other-%s" % (y2, y), [other, _one(v(y))], _one(v(y2))))
    for x, y in (("uniform", "const"), ("small", "dict400"), ("small_runs7", "small"), ("uniform", "rle_emit")):
        out.append(Case("i32-%s-%s-alternating" % (x, y), [_one(v(x)), _one(v(x)), _one(v(y)), _one(v(x))], _one(v(y))))
    # two calls of the plan in one interval
    for x, y in (("uniform", "const"), ("const", "uniform"), ("small", "dict400"), ("uniform", "rle_emit"), ("runs64", "freq")):
        out.append(Case("i32-%s-then-%s-one-interval" % (x, y), [_one(v(x))] * 2, (call_of(v(x)), call_of(v(y))), "two_calls"))
    out.append(Case("long-uniform-then-dict400-one-interval", [_one("long/uniform")] * 2, (call_of("long/uniform"), call_of("long/dict400")), "two_calls"))
    # two plans in one interval: the first call's ENC_HINT belongs to a plan that is gone when the interval ends
    for y, z in (("const", "uniform"), ("small_runs7", "small")):
        out.append(Case("i32-%s-after-other-and-%s-one-interval" % (z, y), [(call_of("other/uniform"), call_of(v(y)))], _one(v(z)), "two_plans"))
    # SB_MEM_HOST, single group
    for x, y in (("uniform", "const"), ("uniform", "rle_emit"), ("small", "uniform"), ("dict400", "freq"), ("freq", "freq")):
        out.append(Case("i32-%s-after-2x-%s-host" % (y, x), [(call_of(v(x), mem=MEM_HOST),)] * 2, (call_of(v(y), mem=MEM_HOST),), "host"))
    for x, y in (("uniform", "dict400"), ("uniform", "freq"), ("dict400", "dict_runs")):
        out.append(Case("long-%s-after-2x-%s-host" % (y, x), [(call_of("long/" + x, mem=MEM_HOST),)] * 2, (call_of("long/" + y, mem=MEM_HOST),), "host"))
    # a mixed-kind call (every kind's chain on a stream of its own): one kind's variant changes, the others stay
    base = dict(i16="i16/dict40", i32="i32/small", bin="bin/scattered")
    for kind, y in (("i32", "i32/uniform"), ("i32", "i32/rle_emit"), ("i32", "i32/freq"), ("i32", "i32/small"), ("i16", "i16/runs64"),
                    ("i16", "i16/const"), ("bin", "bin/in_runs"), ("bin", "bin/unique")):
        probe = dict(base)
        probe[kind] = y
        hist = (call_of(base["i16"], base["i32"], base["bin"]),)
        out.append(Case("mixed-%s" % y.replace("/", "-"), [hist] * 2, (call_of(probe["i16"], probe["i32"], probe["bin"]),), "mixed"))
    return out


CASES = _cases()
CASE = {c.name: c for c in CASES}
# slots the oracle cannot be made to cross in isolation at these shapes: none is missing from the table
NOT_CROSSED = ()
