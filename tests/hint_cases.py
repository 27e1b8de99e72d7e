"""The case table of tests/test_gpu_hints.py: what a read call launches depends on what the context's earlier synchronize
intervals met (update_read_hints / read_hints in strawboat_amd/csrc/sb_api.hip), so every probe page is crossed with every
history of a context.  No fixtures, no tests, no device: tests/test_hint_cases.py walks the same table on the CPU.

A case is a history (read intervals applied to a context of its own), a probe (pages that need one particular kernel), an
entry point, and the number of replays (sb_ctx_replays) the probe must cost.  The counts are not typed in: a probe CLAIMS
what its pages queue (`claim`), the CPU test proves the claim with a page walker (`features_of`), and `Model` -- the rules of
update_read_hints / read_hints restated in Python -- turns history and claim into the count.

What the model states beside the two functions:
  * a page that needed a kernel which was left out raises KIND_REPLAY, and the interval is issued once more without hints;
    both passes feed the hint state (each ends in a synchronize).
  * the Freq second pass goes by no hint and changes no hint state, so a Freq page costs what its outer page costs: a
    replay when the tile kernel was left out, none otherwise -- whatever codec and size its exceptions block has.
  * a sink call (filter, IN list, selected read, aggregates, top-k, key ids) consults no hint; a Freq page in one always asks for the decoded route
    (KIND_FILTER_FREQ, sb_filter.h), hints or no hints, first call or second: always one replay.
  * sb_read_columns_sizes is recorded with the calls of the interval it closes and issued again with them.
  * kept as found, and followed: a sink call that meets a Zstd buffer or a giant LZ4 block still teaches the context
    (zstd_recent, lzg_state: update_read_hints guards only the idle counters by read_calls), and the replay of a sink's Freq
    page counts as a read interval that met nothing (its decoded route is a READ whose status word the Freq pass takes).

lz4_giant is the shape of test_gpu_lz4.py's "random" block (one literal run) at the smallest size over LZG_MIN, written by
the oracle like every other probe; only zstd_frames_1mib is written by the device (tests/test_gpu_hints.py builds it).
"""
import zlib

import numpy as np

from oracle import sbo as S
from tests import gen

# ---------------------------------------------------------------- constants (tests/test_hint_cases.py reads them out of the sources)
LZG_MIN = 2 << 20          # compressed bytes of an LZ4 block for the block-parallel chain; page bytes for its pool
ZSTD_LONG_MIN = 1 << 20    # compressed bytes of a Zstd buffer that is left undone without the block pipeline (zb_skipped)
LZ4_BIG_MIN = 64 << 10     # k_inflate_lz4_big takes blocks of a quarter of this and more in calls of few pages
ZSTD_IDLE = 2              # read intervals without a Zstd buffer before zstd_recent is dropped
READ_IDLE = 2              # idle read intervals before queue A's kernels / k_expand are left out
LZG_IDLE = 3               # long-page intervals without a giant block before a chain that has met one is dropped
TILE_ROWS = 4096

BASIC = (S.NONE, S.LZ4, S.ZSTD, S.SNAPPY)
BINARIES = (S.T_BIN32, S.T_BIN64)
CODEC_NAMES = {S.NONE: "none", S.LZ4: "lz4", S.ZSTD: "zstd", S.SNAPPY: "snappy", S.RLE: "rle", S.DICT: "dict",
               S.ONEVALUE: "onevalue", S.FREQ: "freq", S.BITPACK: "bitpack", S.DELTABP: "deltabp", S.PATAS: "patas"}


def size_class(n):
    """which thresholds a compressed size (or a page length) has reached"""
    return "giant" if n >= LZG_MIN else "1mib" if n >= ZSTD_LONG_MIN else "small"


# ---------------------------------------------------------------- the page walker
class Block:
    """a block header: codec u8 | compressed size u32 | uncompressed size u32, at byte `at` of the page"""

    def __init__(self, page, at):
        assert at + 9 <= page.size, "block header outside the page"
        self.at, self.codec = at, int(page[at])
        self.csize = int(page[at + 1:at + 5].view("<u4")[0])
        self.usize = int(page[at + 5:at + 9].view("<u4")[0])
        self.body = at + 9


def walk_page(ptype, nullable, page):
    """The block headers of one page of a primitive or binary column: {"top": Block} and, where the page has one, "values"
    (the second block of a Basic binary page), "index" (the index block of a Dict page), "exceptions" (the nested block of a
    primitive Freq page) with "nested_len" (the bytes from that header to the end of the page: the one-page column the
    second pass reads)."""
    page = np.ascontiguousarray(page, np.uint8)
    at = 0
    if nullable:
        at = 4 + int(page[0:4].view("<u4")[0])
    top = Block(page, at)
    out = {"top": top}
    if top.codec in BASIC and ptype in BINARIES:
        out["values"] = Block(page, top.body + top.csize)
    elif top.codec == S.DICT:
        out["index"] = Block(page, top.body)
    elif top.codec == S.FREQ and ptype not in BINARIES:
        w = S.WIDTH[ptype]
        rb = int(page[top.body + w:top.body + w + 4].view("<u4")[0])
        ex = Block(page, top.body + w + 4 + rb)
        out["exceptions"] = ex
        out["nested_len"] = page.size - ex.at
    return out


def pages_of(pages, metas):
    off = 0
    for length, rows in np.asarray(metas, np.uint64).reshape(-1, 2).tolist():
        yield pages[off:off + length], int(rows)
        off += length


def make_claim(page, tiles, a=(), b=(), z=(), freq=()):
    """What a call queues.  page: size_class of its longest page; tiles: it has tile tasks; a / b / z: the (codec, size_class
    of the compressed bytes) of the inflate jobs of queue A (Basic blocks of primitive pages in a call without binary columns,
    index and offset blocks), B (value blocks of binary columns, and the primitives' of a call that has binary columns) and Z
    (Zstd value blocks of such a call); freq: the claim of the second pass's call, or None"""
    return dict(page=page, tiles=bool(tiles), a=tuple(sorted(set(a))), b=tuple(sorted(set(b))), z=tuple(sorted(set(z))), freq=freq or None)


def features_of(columns, sizes=False):
    """The claim of one call, from its pages: columns = [(col, pages, metas)].  Restates which queue k_parse puts a block on
    (strawboat_amd/csrc/sb_decode.hip: parse_page, push_payload).  sizes: the call is sb_read_columns_sizes."""
    any_binary = any(c["ptype"] in BINARIES for c, _, _ in columns)
    defer = any_binary and not sizes
    a, b, z, nested = [], [], [], []
    tiles, longest = False, 0
    for col, pages, metas in columns:
        t = col["ptype"]
        assert t != S.T_BOOL and t != S.T_NULL, "the table has no Boolean / Null column"
        for page, rows in pages_of(pages, metas):
            longest = max(longest, page.size)
            blk = walk_page(t, col["nullable"], page)
            top = blk["top"]
            job = (CODEC_NAMES[top.codec], size_class(top.csize))
            if t in BINARIES and top.codec in BASIC:
                if top.codec != S.NONE and not sizes:
                    a.append(job)                                                       # the offsets block
                    v = (CODEC_NAMES[top.codec], size_class(blk["values"].csize))
                    (z if top.codec == S.ZSTD else b).append(v)
            elif t not in BINARIES and (top.codec in (S.LZ4, S.ZSTD, S.SNAPPY, S.PATAS)):
                if not sizes:
                    (a if not defer else z if top.codec == S.ZSTD else b).append(job)
            elif top.codec == S.FREQ and t not in BINARIES and not sizes:
                ex = blk["exceptions"]
                ecol = dict(ptype=t, nullable=False)   # (a Freq page of the table has exceptions: the nested page has rows)
                nested.append((ecol, page[ex.at:], np.array([[blk["nested_len"], 1]], np.uint64)))
            if top.codec == S.DICT:
                ix = blk["index"]
                assert ix.codec != S.FREQ, "the table has no Dict page with a Freq index block"
                if ix.codec in (S.LZ4, S.ZSTD, S.SNAPPY):
                    a.append((CODEC_NAMES[ix.codec], size_class(ix.csize)))
            by_page = top.codec == S.RLE and t not in BINARIES and S.WIDTH[t] <= 8
            if rows and not by_page and not (sizes and top.codec == S.FREQ and t not in BINARIES):
                tiles = True
    freq = None
    if nested:   # the second pass: every exceptions block of the interval as a one-page column of one call
        freq = features_of(nested)
    return make_claim(size_class(longest), tiles, a, b, z, freq)


def merge_claims(claims):
    """the claim of an interval's Freq pass: the exceptions blocks of all its calls in one call"""
    claims = [c for c in claims if c]
    if not claims:
        return None
    order = ("small", "1mib", "giant")
    return make_claim(max((c["page"] for c in claims), key=order.index), any(c["tiles"] for c in claims),
                      sum((c["a"] for c in claims), ()), sum((c["b"] for c in claims), ()), sum((c["z"] for c in claims), ()))


# ---------------------------------------------------------------- the model
KIND_ZSTD, KIND_LZ4_GIANT, KIND_REPLAY, KIND_REPLAY_LZG, KIND_QUEUE_A, KIND_TILES, KIND_FILTER_FREQ = 1, 4, 8, 16, 32, 64, 128
READ, SIZES, SINK = "read", "sizes", "sink"


class Model:
    """The launch-hint state of one context.  no_hints: SB_NO_HINTS=1; zb_mode: SB_ZSTD_BLOCKS (0, 1; 2: unset)."""

    def __init__(self, no_hints=False, zb_mode=2):
        self.no_hints, self.zb_mode = no_hints, zb_mode
        self.zstd_recent, self.zstd_idle = False, 0
        self.qa_idle = self.tiles_idle = self.read_calls = 0
        self.lzg_state, self.lzg_idle, self.lzg_long_pages = 0, 0, False

    # update_read_hints
    def update(self, kinds):
        if kinds & KIND_ZSTD:
            self.zstd_recent, self.zstd_idle = True, 0
        elif self.read_calls:
            self.zstd_idle += 1
            if self.zstd_idle >= ZSTD_IDLE:
                self.zstd_recent = False
        if self.read_calls:
            self.qa_idle = 0 if kinds & KIND_QUEUE_A else self.qa_idle + 1
            self.tiles_idle = 0 if kinds & KIND_TILES else self.tiles_idle + 1
        self.read_calls = 0
        if kinds & KIND_LZ4_GIANT:
            self.lzg_state, self.lzg_idle = 1, 0
        elif self.lzg_long_pages and self.lzg_state == 0:
            self.lzg_state = 2
        elif self.lzg_long_pages and self.lzg_state == 1:
            self.lzg_idle += 1
            if self.lzg_idle >= LZG_IDLE:
                self.lzg_state = 2
        self.lzg_long_pages = False

    # read_hints, and what the call's kernels then raise (k_zstd_split, k_inflate_lz4_big, k_plan, the sinks' tile kernels)
    def issue(self, mode, claim, no_hints, freq_pass=False):
        no_hints = no_hints or freq_pass
        sink = mode == SINK
        zb_on = self.zb_mode == 1 or (self.zb_mode == 2 and (self.zstd_recent or no_hints or sink))
        if not freq_pass and not sink:
            self.read_calls += 1
        long_zstd = claim["page"] in ("1mib", "giant")
        zb_skipped = not zb_on and self.zb_mode == 2 and mode != SIZES and long_zstd
        skip_a = skip_t = False
        if not no_hints and mode == READ and not freq_pass:
            skip_a, skip_t = self.qa_idle >= READ_IDLE, self.tiles_idle >= READ_IDLE
        lzg_skipped = lzg_launch = False
        if mode != SIZES and claim["page"] == "giant":
            none_met = self.lzg_state == 2 and not no_hints
            lzg_skipped = none_met and not sink
            lzg_launch = not lzg_skipped and not none_met
            if not sink and not freq_pass:
                self.lzg_long_pages = True
        kinds = 0
        if claim["a"]:
            kinds |= KIND_QUEUE_A
        if claim["tiles"]:
            kinds |= KIND_TILES
        if (skip_a and claim["a"]) or (skip_t and claim["tiles"]):
            kinds |= KIND_REPLAY
        for codec, size in (() if skip_a else claim["a"]) + claim["b"] + claim["z"]:   # the queues k_zstd_split walks
            if codec == "lz4" and size == "giant":
                kinds |= KIND_LZ4_GIANT
            if codec == "zstd":
                kinds |= KIND_ZSTD
                if zb_skipped and size in ("1mib", "giant"):
                    kinds |= KIND_REPLAY
        giant = any(codec == "lz4" and size == "giant" for codec, size in claim["a"] + claim["b"])
        if giant and lzg_skipped:
            kinds |= KIND_REPLAY | KIND_REPLAY_LZG
        if giant and lzg_launch and self.lzg_state == 0:
            self.lzg_state = 1   # (launch_lzg looks for itself on a context that has met no long page yet)
        if sink and claim["freq"]:
            kinds |= KIND_REPLAY | KIND_FILTER_FREQ
        return kinds

    def interval(self, calls):
        """calls: [(mode, claim)] between two synchronizes; returns the replays it costs (0 or 1)"""
        kinds = 0
        for mode, claim in calls:
            kinds |= self.issue(mode, claim, self.no_hints)
        self.update(kinds)
        replays = 0
        if kinds & KIND_REPLAY:
            replays = 1
            if kinds & KIND_REPLAY_LZG:
                self.lzg_state = 1
            kinds = 0
            for mode, claim in calls:
                if mode == SINK and claim["freq"]:
                    # the decoded route: a read into the staging area and its Freq pass at once, which takes the status
                    # word with it -- what the calls of the replay have raised so far is gone (found so, kept so: such a
                    # replay counts as a read interval that met nothing)
                    self.issue(READ, claim, True)
                    self.issue(READ, claim["freq"], True, freq_pass=True)
                    kinds = 0
                else:
                    kinds |= self.issue(mode, claim, True)
            self.update(kinds)
        passes = merge_claims([claim["freq"] for mode, claim in calls if mode != SINK])
        if passes:
            k = self.issue(READ, passes, self.no_hints, freq_pass=True)
            assert not k & KIND_REPLAY, "the Freq pass goes by no hint: nothing of it is left undone"
        return replays


# ---------------------------------------------------------------- data
def seed_of(*names):
    return zlib.crc32("/".join(names).encode())


def _col(ptype, values):
    return dict(ptype=ptype, nullable=False, rows=int(values.size), values=values, validity=None, offsets=None)


def _random_bytes(seed, n):
    return _col(S.T_U8, np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8))


def _freq_i64(seed, rows):
    """one value (0) on 90.5 % of the rows, full-range random exceptions on the others: what the exceptions block compresses
    to is 8 bytes per exception with any codec"""
    rng = np.random.default_rng(seed)
    v = np.zeros(rows, np.int64)
    ex = rng.random(rows) < 0.095
    v[ex] = rng.integers(-(1 << 62), 1 << 62, int(ex.sum()))
    return _col(S.T_I64, v)


def _runs_i32(seed, rows):
    rng = np.random.default_rng(seed)
    return _col(S.T_I32, np.repeat(rng.integers(0, 300, rows // 5 + 1), 5)[:rows].astype(np.int32))


FREQ_ROWS_SMALL = 5000
FREQ_ROWS_ZSTD_1MIB = 1_500_000    # 142 500 exceptions: a Zstd block of 1 141 504 bytes >= 2^20
FREQ_ROWS_LZ4_GIANT = 3_000_000    # 285 000 exceptions: an LZ4 block of 2 290 814 bytes >= 2^21


class Probe:
    """name; build(seed) -> [(col, oracle write options)]: the columns of ONE call; claim: what the call queues"""

    def __init__(self, name, build, claim, needs):
        self.name, self.build, self.claim, self.needs = name, build, claim, needs

    def __repr__(self):
        return self.name


def _freq(rows, nested):
    return lambda seed: [(_freq_i64(seed, rows), dict(force_codec=S.FREQ, force_index_codec=nested))]


_PLAIN = make_claim("small", True)
_FREQ_ZSTD_1MIB = make_claim("1mib", True, freq=make_claim("1mib", True, a=[("zstd", "1mib")]))
PROBES = [
    Probe("plain_i64", lambda seed: [(_col(S.T_I64, np.random.default_rng(seed).integers(-(1 << 62), 1 << 62, 5000)), dict(force_codec=S.NONE))],
          _PLAIN, "k_expand (tiles)"),
    Probe("lz4_i32", lambda seed: [(_runs_i32(seed, 5000), dict(force_codec=S.LZ4))],
          make_claim("small", True, a=[("lz4", "small")]), "queue A"),
    Probe("dict_lz4_index", lambda seed: [(gen.prim(S.T_F64, 128 * 300, uniq=200, null_density=0.1, runs=16, seed=seed),
                                           dict(max_page_size=128 * 100, force_codec=S.DICT, force_index_codec=S.LZ4))],
          make_claim("small", True, a=[("lz4", "small")]), "queue A in front of k_plan"),
    Probe("binary_lz4_values", lambda seed: [(gen.binary(3000, uniq=300, seed=seed), dict(force_codec=S.LZ4))],
          make_claim("small", True, a=[("lz4", "small")], b=[("lz4", "small")]), "queues A and B"),
    Probe("binary_zstd_values", lambda seed: [(gen.binary(3000, uniq=300, seed=seed), dict(force_codec=S.ZSTD))],
          make_claim("small", True, a=[("zstd", "small")], z=[("zstd", "small")]), "queues A and Z"),
    Probe("zstd_small", lambda seed: [(gen.prim(S.T_I64, 5000, uniq=1000, seed=seed), dict(force_codec=S.ZSTD))],
          make_claim("small", True, a=[("zstd", "small")]), "the frame-serial or the block-parallel Zstd decoder"),
    Probe("zstd_1mib", lambda seed: [(_random_bytes(seed, 1_150_000), dict(force_codec=S.ZSTD))],
          make_claim("1mib", True, a=[("zstd", "1mib")]), "the block pipeline (zb_skipped without it)"),
    Probe("lz4_giant", lambda seed: [(_random_bytes(seed, 2_200_000), dict(force_codec=S.LZ4))],
          make_claim("giant", True, a=[("lz4", "giant")]), "the giant-LZ4 chain (lzg_skipped without it)"),
    Probe("freq_plain", _freq(FREQ_ROWS_SMALL, S.NONE), make_claim("small", True, freq=make_claim("small", True)), "the Freq pass"),
    Probe("freq_lz4_small", _freq(FREQ_ROWS_SMALL, S.LZ4),
          make_claim("small", True, freq=make_claim("small", True, a=[("lz4", "small")])), "the Freq pass, queue A"),
    Probe("freq_zstd_small", _freq(FREQ_ROWS_SMALL, S.ZSTD),
          make_claim("small", True, freq=make_claim("small", True, a=[("zstd", "small")])), "the Freq pass, Zstd"),
    Probe("freq_zstd_1mib", _freq(FREQ_ROWS_ZSTD_1MIB, S.ZSTD), _FREQ_ZSTD_1MIB, "the Freq pass, the block pipeline"),
    Probe("freq_lz4_giant", _freq(FREQ_ROWS_LZ4_GIANT, S.LZ4),
          make_claim("giant", True, freq=make_claim("giant", True, a=[("lz4", "giant")])), "the Freq pass, the giant-LZ4 chain"),
    Probe("plain_and_freq_zstd_1mib",
          lambda seed: [(_col(S.T_I64, np.random.default_rng(seed).integers(-(1 << 62), 1 << 62, 5000)), dict(force_codec=S.NONE)),
                        (_freq_i64(seed + 1, FREQ_ROWS_ZSTD_1MIB), dict(force_codec=S.FREQ, force_index_codec=S.ZSTD))],
          _FREQ_ZSTD_1MIB, "the Freq pass of a replayed interval"),
]
PROBE = {p.name: p for p in PROBES}
FREQ_PROBES = ("freq_plain", "freq_lz4_small", "freq_zstd_small", "freq_zstd_1mib", "freq_lz4_giant")
# the device's own Zstd writer: the bytes of zstd_1mib in frames of 16 KiB (the frame scan, zs_on); built on the device
DEVICE_WRITTEN = "zstd_frames_1mib"
DEVICE_WRITTEN_CLAIM = make_claim("1mib", True, a=[("zstd", "1mib")])

# the small binary column of the sizes-then-read sequence, as sb_read_columns_sizes sees it: tile tasks, no job
SIZES_PROBE = Probe("sizes_binary_lz4", lambda seed: [(gen.binary(3000, uniq=300, seed=seed), dict(force_codec=S.LZ4))],
                    make_claim("small", True), "k_parse and k_colscan alone")

# ---------------------------------------------------------------- histories
# the read intervals a history is made of: one call each, small and fixed (only the probes draw from a case's seed)
INTERVALS = {
    # RLE pages of a primitive column: expanded by a page kernel -- no inflate job, no tile
    "rle": Probe("rle", lambda seed: [(gen.prim(S.T_F64, 5000, uniq=50, null_density=0.1, runs=40, seed=5), dict(max_page_size=2048, force_codec=S.RLE))],
                 make_claim("small", False), None),
    "zstd": Probe("zstd", lambda seed: [(gen.prim(S.T_I64, 5000, uniq=1000, seed=6), dict(force_codec=S.ZSTD))],
                  make_claim("small", True, a=[("zstd", "small")]), None),
    # no Zstd buffer, but work for queue A and for the tile kernel: only the Zstd hysteresis moves
    "busy": Probe("busy", lambda seed: [(_runs_i32(7, 5000), dict(force_codec=S.LZ4))],
                  make_claim("small", True, a=[("lz4", "small")]), None),
    # a plain page of LZG_MIN bytes and more beside a small LZ4 page (queue A stays busy: only the giant-LZ4 state moves)
    "long": Probe("long", lambda seed: [(_random_bytes(8, LZG_MIN + 4096), dict(force_codec=S.NONE)), (_runs_i32(9, 5000), dict(force_codec=S.LZ4))],
                  make_claim("giant", True, a=[("lz4", "small")]), None),
    "giant": Probe("giant", lambda seed: [(_random_bytes(10, 2_200_000), dict(force_codec=S.LZ4))],
                   make_claim("giant", True, a=[("lz4", "giant")]), None),
}
HISTORIES = {
    "fresh": (),
    "idle1": ("rle",),
    "idle2": ("rle", "rle"),
    "zstd": ("zstd",),
    "zstd_idle1": ("zstd", "busy"),
    "zstd_idle2": ("zstd", "busy", "busy"),
    "long": ("long",),
    "giant": ("giant",),
    "giant_long2": ("giant", "long", "long"),
    "giant_long3": ("giant", "long", "long", "long"),
}
SINKS = ("filter", "read_selected", "aggregate", "aggregate_grouped", "filter_in", "topk", "key_ids", "aggregate_grouped_large")
SINK_PROBES = ("zstd_1mib", "lz4_giant", "freq_zstd_1mib")
SINK_HISTORIES = ("fresh", "long")
HOST_HISTORIES = ("fresh", "idle2", "zstd_idle2", "long", "giant_long3")
N_GROUPS = 16
N_GROUPS_LARGE = 300       # aggregate_grouped_large: more groups than sb_aggregate_grouped takes, ids of two bytes
IN_LITERALS = 8            # filter_in: literals drawn from the probe's column
TOPK_K = 16
KEY_MAX_KEYS = 256         # key_ids: every value of a U8 probe fits; the exceptions of the Int64 Freq probe overflow it


class Expect:
    def __init__(self, history, probe, again):
        self.history, self.probe, self.again = history, probe, again   # replays of each history interval / the probe / the probe again

    def __eq__(self, o):
        return (self.history, self.probe, self.again) == (o.history, o.probe, o.again)

    def __repr__(self):
        return "Expect(history=%r, probe=%d, again=%d)" % (self.history, self.probe, self.again)


def expect(history, calls, no_hints=False, zb_mode=2, interval_claims=None):
    """history: a key of HISTORIES; calls: the probe interval's [(mode, claim)]; interval_claims: {name: claim} in place of the
    claims INTERVALS states (the CPU test passes what the walker found)"""
    m = Model(no_hints, zb_mode)
    claims = interval_claims or {k: p.claim for k, p in INTERVALS.items()}
    hist = tuple(m.interval([(READ, claims[name])]) for name in HISTORIES[history])
    return Expect(hist, m.interval(calls), m.interval(calls))


class Case:
    """name; history; probe (a Probe, or DEVICE_WRITTEN); entry: device, host, sizes_then_read or one of SINKS; seed"""

    def __init__(self, history, probe, entry):
        pname = probe if isinstance(probe, str) else probe.name
        self.name = "%s-%s-%s" % (pname, history, entry)
        self.history, self.probe, self.entry = history, probe, entry
        self.claim = DEVICE_WRITTEN_CLAIM if isinstance(probe, str) else probe.claim
        self.seed = seed_of(history, pname, entry)

    def calls(self, claim=None, sizes_claim=None):
        """the probe interval's calls, from the probe's claim (or from the ones given)"""
        claim = claim or self.claim
        if self.entry == "sizes_then_read":
            return [(READ, claim), (SIZES, sizes_claim or SIZES_PROBE.claim)]
        return [(SINK if self.entry in SINKS else READ, claim)]

    def expected(self, no_hints=False, zb_mode=2):
        return expect(self.history, self.calls(), no_hints, zb_mode)

    def __repr__(self):
        return self.name


def _table():
    out = []
    for h in HISTORIES:
        for p in PROBES:
            if p.name != "plain_and_freq_zstd_1mib" or h == "idle2":
                out.append(Case(h, p, "device"))
        out.append(Case(h, DEVICE_WRITTEN, "device"))
    for h in HOST_HISTORIES:
        for name in FREQ_PROBES:
            out.append(Case(h, PROBE[name], "host"))
    out.append(Case("idle2", PROBE["plain_i64"], "sizes_then_read"))
    for h in SINK_HISTORIES:
        for name in SINK_PROBES:
            for sink in SINKS:
                out.append(Case(h, PROBE[name], sink))
    return out


CASES = _table()
CASE = {c.name: c for c in CASES}
# the replay counts of the table, with hints: (probe, the same probe again)
REPLAYS = {c.name: (c.expected().probe, c.expected().again) for c in CASES}


def written(probe, seed):
    """[(col, pages, metas, want)] of a probe's columns: the oracle's pages and its own decode of them"""
    out = []
    for col, opt in probe.build(seed):
        pages, metas = gen.oracle_write(col, **opt)
        out.append((col, pages, metas, gen.oracle_read(col, pages, metas)))
    return out
