"""The launch-hint table (tests/hint_cases.py) against the CPU oracle alone: every case is where it claims to be.

  * the constants the table and its model were built around are the ones in the device sources,
  * a page walker finds every probe's block headers -- the exceptions block nested in a Freq page included -- and they
    show the claimed codec on the claimed side of its threshold; the walker agrees with the oracle's stat_column,
  * every probe decodes on the oracle to its input,
  * the table's replay counts are what the model makes of the pages as the walker found them,
  * every (history, probe) pair and entry point the table is meant to hold is there.

tests/test_gpu_hints.py sends the same cases through the device."""
import os
import re

import numpy as np
import pytest

from oracle import sbo as S
from tests import hint_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.findall(pattern, text)
    assert m, "%s: the pattern %r no longer matches; update tests/hint_cases.py with the source" % (what, pattern)
    assert len(set(m)) == 1, "%s: several different values %s" % (what, m)
    return m[0]


def test_constants_of_the_table_are_the_ones_in_the_sources():
    """a change of a threshold or of a hysteresis count must come with a change of the table and its model"""
    csrc = ("strawboat_amd", "csrc")
    common_h, api, decode = _source(*csrc, "sb_common.h"), _source(*csrc, "sb_api.hip"), _source(*csrc, "sb_decode.hip")
    a, b = _one(r"constexpr\s+uint32_t\s+LZG_MIN\s*=\s*(\d+)u\s*<<\s*(\d+)\s*;", common_h, "LZG_MIN")
    assert int(a) << int(b) == H.LZG_MIN
    a, b = _one(r"constexpr\s+uint32_t\s+ZSTD_LONG_MIN\s*=\s*(\d+)u\s*<<\s*(\d+)\s*;", common_h, "ZSTD_LONG_MIN")
    assert int(a) << int(b) == H.ZSTD_LONG_MIN
    a, b = _one(r"constexpr\s+uint32_t\s+LZ4_BIG_MIN\s*=\s*(\d+)u\s*<<\s*(\d+)\s*;", common_h, "LZ4_BIG_MIN")
    assert int(a) << int(b) == H.LZ4_BIG_MIN
    assert int(_one(r"constexpr\s+int\s+TILE_ROWS\s*=\s*(\d+)\s*;", common_h, "TILE_ROWS")) == H.TILE_ROWS
    # the threshold is named once: the host's two uses and the kernel's go by the name
    assert len(re.findall(r"sh\.max_page_len\s*>=\s*ZSTD_LONG_MIN", api)) == 2
    assert re.search(r"a\.zb_skipped\s*&&\s*job\.csize\s*>=\s*ZSTD_LONG_MIN", decode)
    assert re.search(r"lzg_skipped\s*&&\s*j\.csize\s*>=\s*LZG_MIN", decode)
    # the hysteresis counts of update_read_hints and their readers in read_hints
    assert int(_one(r"\+\+ctx->zstd_idle\s*>=\s*(\d+)", api, "the Zstd idle count")) == H.ZSTD_IDLE
    assert int(_one(r"ctx->qa_idle\s*>=\s*(\d+)", api, "queue A's idle count")) == H.READ_IDLE
    assert int(_one(r"ctx->tiles_idle\s*>=\s*(\d+)", api, "the tile kernel's idle count")) == H.READ_IDLE
    assert int(_one(r"\+\+ctx->lzg_idle\s*>=\s*(\d+)", api, "the giant-LZ4 idle count")) == H.LZG_IDLE
    # the KIND_* bits of the model
    for name, bit in (("ZSTD", H.KIND_ZSTD), ("LZ4_GIANT", H.KIND_LZ4_GIANT), ("REPLAY", H.KIND_REPLAY), ("REPLAY_LZG", H.KIND_REPLAY_LZG),
                      ("QUEUE_A", H.KIND_QUEUE_A), ("TILES", H.KIND_TILES), ("FILTER_FREQ", H.KIND_FILTER_FREQ)):
        assert int(_one(r"constexpr\s+uint32_t\s+KIND_%s\s*=\s*(\d+)u\s*;" % name, common_h, "KIND_" + name)) == bit


def test_size_classes_sit_on_the_thresholds():
    assert [H.size_class(n) for n in (0, H.ZSTD_LONG_MIN - 1, H.ZSTD_LONG_MIN, H.LZG_MIN - 1, H.LZG_MIN)] == ["small", "small", "1mib", "1mib", "giant"]


def _check_walker_against_stat(col, pages, metas):
    codecs, inner = S.stat_column(col["ptype"], col["nullable"], pages, metas)
    for k, (page, _) in enumerate(H.pages_of(pages, metas)):
        blk = H.walk_page(col["ptype"], col["nullable"], page)
        assert blk["top"].codec == codecs[k]
        nested = blk.get("index") or blk.get("exceptions")
        assert (nested.codec if nested else 255) == inner[k]
        assert blk["top"].body + blk["top"].csize <= page.size
        if "exceptions" in blk:   # the nested block is the tail of the page
            ex = blk["exceptions"]
            assert ex.body + ex.csize == page.size and blk["nested_len"] == 9 + ex.csize


def _features(probe, seed, sizes=False):
    cols = H.written(probe, seed)
    for col, pages, metas, want in cols:
        _check_walker_against_stat(col, pages, metas)
        assert want["rows"] == col["rows"]
        given = np.ascontiguousarray(col["values"])
        if col["nullable"]:   # (the slot of a null row holds whatever the codec left there)
            assert col["offsets"] is None and np.array_equal(want["validity"], col["validity"])
            valid = np.unpackbits(col["validity"], bitorder="little")[:col["rows"]].astype(bool)
            assert np.array_equal(want["values"].view(given.dtype)[valid], given[valid]), "the oracle does not decode the probe to its input"
        else:
            assert np.array_equal(want["values"], given.view(np.uint8).reshape(-1)), "the oracle does not decode the probe to its input"
        if col["offsets"] is not None:
            assert np.array_equal(want["offsets"], np.ascontiguousarray(col["offsets"]).view(np.uint8).reshape(-1))
    return H.features_of([(c, p, m) for c, p, m, _ in cols], sizes=sizes)


@pytest.fixture(scope="module")
def interval_claims():
    """what the walker finds in the pages of the histories' intervals"""
    return {name: _features(p, 0) for name, p in H.INTERVALS.items()}


def test_history_intervals_are_what_they_claim(interval_claims):
    for name, p in H.INTERVALS.items():
        assert interval_claims[name] == p.claim, name
    # an idle interval queues nothing, a busy one everything but Zstd, a long one no giant block
    assert H.INTERVALS["rle"].claim == H.make_claim("small", False)


def test_every_case_has_a_seed_of_its_own():
    assert len({c.seed for c in H.CASES}) == len(H.CASES)


# (the device-written probe has no pages without a device: tests/test_gpu_hints.py walks them before it reads them)
@pytest.mark.parametrize("case", [c for c in H.CASES if not isinstance(c.probe, str)], ids=repr)
def test_case_is_where_it_claims(case, interval_claims):
    """from the case's own seed: claim, thresholds, oracle round trip, and the model's count from the pages as found"""
    found = _features(case.probe, case.seed)
    assert found == case.claim, "the pages queue %r, the probe claims %r" % (found, case.claim)
    sizes = _features(H.SIZES_PROBE, case.seed, sizes=True) if case.entry == "sizes_then_read" else None
    if sizes is not None:
        assert sizes == H.SIZES_PROBE.claim
    got = H.expect(case.history, case.calls(found, sizes), interval_claims=interval_claims)
    assert (got.probe, got.again) == H.REPLAYS[case.name]


def test_the_measured_sizes_of_the_long_freq_pages():
    """the two shapes the Freq-pass holes need: a nested Zstd block of 2^20 bytes and more, a nested LZ4 block of LZG_MIN and more"""
    for name, codec, floor in (("freq_zstd_1mib", S.ZSTD, H.ZSTD_LONG_MIN), ("freq_lz4_giant", S.LZ4, H.LZG_MIN)):
        (col, pages, metas, _), = H.written(H.PROBE[name], H.CASE["%s-fresh-device" % name].seed)
        assert metas.shape[0] == 1
        blk = H.walk_page(col["ptype"], False, pages)
        assert blk["top"].codec == S.FREQ and blk["exceptions"].codec == codec and blk["exceptions"].csize >= floor, (name, blk["exceptions"].csize)
    assert H.FREQ_ROWS_ZSTD_1MIB * 0.08 * 8 < H.LZG_MIN   # ... and the Zstd block stays below the next threshold


def test_the_table_holds_every_case_it_is_meant_to():
    names = set(H.CASE)
    assert len(names) == len(H.CASES)
    assert list(H.HISTORIES) == ["fresh", "idle1", "idle2", "zstd", "zstd_idle1", "zstd_idle2", "long", "giant", "giant_long2", "giant_long3"]
    probes = ["plain_i64", "lz4_i32", "dict_lz4_index", "binary_lz4_values", "binary_zstd_values", "zstd_small", "zstd_1mib",
              "zstd_frames_1mib", "lz4_giant", "freq_plain", "freq_lz4_small", "freq_zstd_small", "freq_zstd_1mib", "freq_lz4_giant"]
    for h in H.HISTORIES:
        for p in probes:
            assert "%s-%s-device" % (p, h) in names
    assert "plain_and_freq_zstd_1mib-idle2-device" in names and "plain_i64-idle2-sizes_then_read" in names
    for p in H.FREQ_PROBES:
        for h in H.HOST_HISTORIES:
            assert "%s-%s-host" % (p, h) in names
    for p in ("zstd_1mib", "lz4_giant", "freq_zstd_1mib"):
        for h in ("fresh", "long"):
            for sink in ("filter", "read_selected", "aggregate", "aggregate_grouped", "filter_in", "topk", "key_ids", "aggregate_grouped_large"):
                assert "%s-%s-%s" % (p, h, sink) in names
    assert len(H.SINKS) == 8 and len(set(H.SINKS)) == 8


def _replays(name, **kw):
    e = H.CASE[name].expected(**kw)
    return e.probe, e.again


def test_the_model_on_the_documented_sequences():
    """the model against the sequences the feature tests pin on the device (test_gpu_decode.py, test_gpu_lz4.py,
    test_gpu_zstd_blocks.py), and the neighbouring histories from both sides"""
    # queue A and the tile kernel: left out after two idle read intervals, not after one
    for p in ("plain_i64", "lz4_i32", "dict_lz4_index", "binary_lz4_values"):
        assert _replays("%s-idle1-device" % p) == (0, 0) and _replays("%s-idle2-device" % p) == (1, 0), p
    # a long Zstd buffer: replayed on a context that has met no Zstd buffer, or none for two read intervals
    assert _replays("zstd_1mib-fresh-device") == (1, 0) and _replays("zstd_1mib-zstd-device") == (0, 0)
    assert _replays("zstd_1mib-zstd_idle1-device") == (0, 0) and _replays("zstd_1mib-zstd_idle2-device") == (1, 0)
    assert _replays("zstd_small-fresh-device") == (0, 0) and _replays("zstd_frames_1mib-fresh-device") == (1, 0)
    # a giant LZ4 block: the chain is dropped after ONE long-page interval on a new context, after THREE once it met one
    assert _replays("lz4_giant-fresh-device") == (0, 0) and _replays("lz4_giant-long-device") == (1, 0)
    assert _replays("lz4_giant-giant_long2-device") == (0, 0) and _replays("lz4_giant-giant_long3-device") == (1, 0)
    # the Freq pass goes by no hint: a Freq page costs what its outer page costs
    for p in H.FREQ_PROBES:
        for h in H.HISTORIES:
            assert _replays("%s-%s-device" % (p, h)) == ((1, 0) if h == "idle2" else (0, 0)), (p, h)
    assert _replays("plain_and_freq_zstd_1mib-idle2-device") == (1, 0)
    assert _replays("plain_i64-idle2-sizes_then_read") == (1, 0)
    # sinks consult no hint; a Freq page in one takes the decoded route every time
    for h in ("fresh", "long"):
        for sink in H.SINKS:
            assert _replays("zstd_1mib-%s-%s" % (h, sink)) == (0, 0) and _replays("lz4_giant-%s-%s" % (h, sink)) == (0, 0)
            assert _replays("freq_zstd_1mib-%s-%s" % (h, sink)) == (1, 1)
            assert _replays("freq_zstd_1mib-%s-%s" % (h, sink), no_hints=True) == (1, 1)
    # without hints nothing else is ever replayed
    for c in H.CASES:
        if not (c.entry in H.SINKS and c.claim["freq"]):
            e = c.expected(no_hints=True)
            assert (e.history, e.probe, e.again) == ((0,) * len(H.HISTORIES[c.history]), 0, 0), c.name
