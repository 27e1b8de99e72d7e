"""The write-side launch-hint table (tests/write_hint_cases.py) against the CPU oracle alone.

  * the constants and rules the table's model restates are the ones in the device sources,
  * every variant's slots are derived from the oracle's pages, which the page walker of tests/hint_cases.py and the
    oracle's stat_column see alike; every variant decodes on the oracle to its input, and shows the codecs its place
    in the table is for,
  * the variants of a table share every field of the plan key,
  * every slot the host consults is crossed: a case where the history lacks it, the probe needs it and the model expects
    a replay, and a case where the same probe costs none.

tests/test_gpu_write_hints.py sends the same cases through the device."""
import re

import numpy as np
import pytest

from oracle import sbo as S
from tests import hint_cases as H
from tests import write_hint_cases as W
from tests.test_hint_cases import _one, _source

CSRC = ("strawboat_amd", "csrc")


def test_constants_of_the_table_are_the_ones_in_the_sources():
    """a change of a threshold, of a slot or of the rule of apply_enc_hint must come with a change of the table's model"""
    enc, api = _source(*CSRC, "sb_encode.hip"), _source(*CSRC, "sb_api.hip")
    runs, rle = _source(*CSRC, "sb_select_runs.h"), _source(*CSRC, "sb_select_rle.h")
    big, dbig = _source(*CSRC, "sb_select_big.h"), _source(*CSRC, "sb_dict_big.h")
    assert int(_one(r"constexpr\s+uint32_t\s+RUNS_CAP\s*=\s*(\d+)\s*;", runs, "RUNS_CAP")) == W.RUNS_CAP
    assert 1 << int(_one(r"constexpr\s+uint64_t\s+SEL_BIG_ROWS\s*=\s*1ull\s*<<\s*(\d+)\s*;", big, "SEL_BIG_ROWS")) == W.SEL_BIG_ROWS
    assert int(_one(r"constexpr\s+uint32_t\s+VBIG_ROWS\s*=\s*(\d+)\s*;", dbig, "VBIG_ROWS")) == W.VBIG_ROWS
    assert int(_one(r"constexpr\s+uint64_t\s+BP_MIN_ROWS\s*=\s*(\d+)\s*;", enc, "BP_MIN_ROWS")) == W.BP_MIN_ROWS
    for name, slot in (("FREQ", W.HINT_FREQ), ("RLE_EMIT", W.HINT_RLE_EMIT), ("BIN_DICT_EMIT", W.HINT_BIN_DICT_EMIT), ("ROW_SELECT", W.HINT_ROW_SELECT)):
        assert int(_one(r"constexpr\s+int\s+HINT_%s\s*=\s*(\d+)\s*;" % name, enc, "HINT_" + name)) == slot
    m = re.search(r"constexpr\s+uint32_t\s+SKIP_DICT_BIG\s*=\s*(\d+)u,\s*SKIP_FREQ_BIG\s*=\s*(\d+)u,\s*SKIP_EMIT\s*=\s*(\d+)u\s*;", enc)
    assert m and tuple(int(x) for x in m.groups()) == (W.SKIP_DICT_BIG, W.SKIP_FREQ_BIG, W.SKIP_EMIT)
    # the chunk of both fused selectors and their early stop
    for text, what in ((runs, "sb_select_runs.h"), (rle, "sb_select_rle.h")):
        assert int(_one(r"constexpr\s+int\s+K\s*=\s*(\d+)\s*;", text, what + ": K")) * 256 == W.CHUNK_ROWS
        assert re.search(r"constexpr\s+uint32_t\s+CHUNK\s*=\s*WG\s*\*\s*K\s*;", text), what
        assert re.search(r"if\s*\(\(uint64_t\)nrec\s*\*\s*4\s*>\s*cb\s*\+\s*n\s*\+\s*256\)\s*spec\s*=\s*false;", text), what
    assert int(_one(r"constexpr\s+int\s+WG\s*=\s*(\d+)\s*;", _source(*CSRC, "sb_common.h"), "WG")) == 256
    assert re.search(r"if\s*\(total\s*>\s*RUNS_CAP\)\s*\{[^}]*\*fallback\s*=\s*true;", runs)
    # apply_enc_hint: the maximum over two calls, only for the context's own plan; build_plan forgets
    assert re.search(r"if\s*\(!ctx->enc_plan\.valid\s*\|\|\s*ctx->enc_plan\.key\s*!=\s*p\.n\)\s*return;", api)
    assert re.search(r"last_counts\[i\]\s*=\s*std::max\(now\[i\],\s*ctx->enc_plan\.prev_counts\[i\]\);", api)
    assert re.search(r"memcpy\(ctx->enc_plan\.prev_counts,\s*now,\s*128\);\s*ctx->enc_plan\.counts_valid\s*=\s*true;", api)
    assert re.search(r"plan\.counts_valid\s*=\s*false;\s*memset\(plan\.prev_counts,\s*0,\s*sizeof plan\.prev_counts\);", enc)
    assert re.search(r"L\.big_hint\s*=\s*hit\s*&&\s*plan\.counts_valid\s*&&\s*sh\.adaptive\s*&&\s*!ctx->no_hints;", enc)
    assert re.search(r"bool unused_peek\(int slot\) const \{ return big_hint && !plan\.last_counts\[slot\]; \}", enc)
    # the slots the host consults are the model's CONSULTED, no more
    slots = set(re.findall(r"unused(?:_peek)?\((?:SB_CODEC_|HINT_)(\w+)\)", enc))
    assert slots == {"NONE", "LZ4", "ZSTD", "SNAPPY", "DICT", "FREQ", "ROW_SELECT"}, slots   # ... by name; and by expression in launch_emit:
    assert re.search(r"L\.unused\(cd == SB_CODEC_RLE && \(kd == 4 \|\| kd == 8\)\s*\? HINT_RLE_EMIT\s*"
                     r": cd == SB_CODEC_DICT && kd < 0 && L\.wa\.bin_fused && !L\.old_chain \? HINT_BIN_DICT_EMIT\s*: \(int\)cd\)\)", enc)
    cand = re.search(r"static const int32_t CAND\[6\] = \{([^}]*)\};", enc).group(1)
    assert set(re.findall(r"SB_CODEC_(\w+)", cand)) == {"ONEVALUE", "DICT", "RLE", "BITPACKING", "DELTA_BITPACKING", "PATAS"}
    assert re.search(r"L\.unused_peek\(SB_CODEC_LZ4\) && L\.unused_peek\(SB_CODEC_ZSTD\) && L\.unused_peek\(SB_CODEC_SNAPPY\)", enc)
    assert len(W.CONSULTED) == 13
    # slots 29 and 30 are counted behind the page kernel's kind check, for the kinds that consult them
    emit = re.search(r"k_enc_emit_pages\(EncodeArgs a\) \{.*?uint8_t\* slot = page_slot\(a, c, p\);", enc, re.S).group(0)
    kind_check = emit.index("if (is_bool || is_bin || c.width != (uint32_t)KIND) return;")
    m29 = re.search(r"if constexpr \(CODEC == SB_CODEC_RLE && \(KIND == 4 \|\| KIND == 8\)\) \{\s*if \(threadIdx\.x == 0 && a\.use_counts\) "
                    r"atomicAdd\(&a\.codec_counts\[HINT_RLE_EMIT\], 1u\);", emit)
    m30 = re.search(r"if constexpr \(CODEC == SB_CODEC_DICT && KIND < 0\) \{\s*if \(threadIdx\.x == 0 && a\.use_counts\) "
                    r"atomicAdd\(&a\.codec_counts\[HINT_BIN_DICT_EMIT\], 1u\);", emit)
    assert m29 and m30 and m29.start() > kind_check and m30.start() > kind_check
    assert len(re.findall(r"codec_counts\[HINT_(?:RLE_EMIT|BIN_DICT_EMIT)\]", enc)) == 2


def test_the_python_wrapper_derives_out_capacity_from_the_shape():
    """plan_lookup keys on out_capacity: write.WriteBatch takes it from sb_write_bound(type, nullable, rows, values_len,
    options) -- nothing of the data"""
    src = _source("strawboat_amd", "write.py")
    assert re.search(r"sb_write_bound\(col\.physical_type, 1 if col\.is_nullable else 0, col\.rows, vlen, C\.byref\(oc\)", src)
    assert re.search(r"bound, npages = write_bound\(ctx, col, oc\)\s*pages = torch\.empty\(max\(bound, 1\)", src)
    assert re.search(r"c\.out_capacity = pages\.numel\(\)", src)
    enc = _source(*CSRC, "sb_encode.hip")
    key = re.search(r"static bool plan_lookup\(.*?const sb_ctx::EncPlan& plan", enc, re.S).group(0)
    fields = set(re.findall(r"mixk\(\(?(?:\(uint64_t\))?(?:\(int64_t\))?(?:c\.|opts->)(\w+)", key))
    assert fields >= {"physical_type", "is_nullable", "rows", "values_len", "out_capacity", "default_compression", "has_default_compress_ratio",
                      "max_page_size", "forbidden_compressions", "force_codec", "force_index_codec", "flags", "rng_seed"}, fields


@pytest.mark.parametrize("table", [t for t in W.TABLES.values()], ids=lambda t: t.name)
def test_variants_of_a_table_share_the_plan_key(table):
    """type, nullability, rows, options (one dict per table) and, for binary columns, the length of the value bytes"""
    lens = set()
    for v in table.variants.values():
        col = v.column()
        assert (col["ptype"], col["nullable"], col["rows"]) == (table.ptype, False, table.rows)
        assert v.table.options is table.options
        again = v.column()
        assert np.array_equal(np.ascontiguousarray(col["values"]).view(np.uint8), np.ascontiguousarray(again["values"]).view(np.uint8))
        if col["offsets"] is not None:
            lens.add(int(np.ascontiguousarray(col["values"]).view(np.uint8).size))
            assert int(col["offsets"][-1]) == table.values_len
        else:
            nbytes = (table.rows + 7) // 8 if table.ptype == S.T_BOOL else table.rows * S.WIDTH[table.ptype]
            assert np.ascontiguousarray(col["values"]).view(np.uint8).size == nbytes
    assert lens <= {table.values_len}


@pytest.mark.parametrize("variant", list(W.VARIANT.values()), ids=repr)
def test_variant_is_what_it_claims(variant):
    """the walker and stat_column agree on the variant's pages, the oracle decodes them to the input, and the slots are
    a function of the pages alone"""
    col, pages, metas = W.written(variant)
    codecs, inner = S.stat_column(col["ptype"], False, pages, metas)
    assert [r for _, r in H.pages_of(pages, metas)] == variant.table.page_rows()
    for k, (page, rows) in enumerate(H.pages_of(pages, metas)):
        blk = H.walk_page(col["ptype"], False, page)
        assert blk["top"].codec == codecs[k]
        nested = blk.get("index") or blk.get("exceptions")
        if col["ptype"] not in H.BINARIES or blk["top"].codec == S.DICT:
            assert (nested.codec if nested else 255) == inner[k]
    want = S.read_column(col["ptype"], False, pages, metas)
    assert want["rows"] == col["rows"]
    given = np.ascontiguousarray(col["values"]).view(np.uint8).reshape(-1)
    assert np.array_equal(want["values"][:given.size], given), "the oracle does not decode the variant to its input"
    if col["offsets"] is not None:
        assert np.array_equal(want["offsets"], np.ascontiguousarray(col["offsets"]).view(np.uint8).reshape(-1))
    counts, required = W.page_slots(col, pages, metas)
    assert (counts, required) == W.needs(variant)
    assert required <= set(W.CONSULTED)
    for fused in (True, False):
        c, r = W.needs(variant, fused)
        assert all(s in c or (s == W.BASIC and c & set(W.BASIC_IDS)) for s in r), "a needed launch whose slot the call leaves at 0 would be replayed for ever"


def _codecs(name):
    col, pages, metas = W.written(W.VARIANT[name])
    codecs, inner = S.stat_column(col["ptype"], False, pages, metas)
    return codecs.tolist(), inner.tolist()


def test_the_codecs_the_table_is_built_around():
    """what every place of the table is for, proven by the oracle (four pages of 8192 rows; one page of 2^18)"""
    four = lambda c, i=255: ([c] * 4, [i] * 4)
    assert _codecs("i32/uniform") == four(S.NONE) and _codecs("i32lz4/uniform") == four(S.LZ4)
    assert _codecs("i32/const") == four(S.ONEVALUE)
    assert _codecs("i32/dict400") == four(S.DICT, S.BITPACK) and _codecs("i32/dict_runs") == four(S.DICT, S.RLE)
    assert _codecs("i32/small") == four(S.BITPACK) and _codecs("i32/small_runs7") == four(S.BITPACK)
    assert _codecs("i32/runs64") == four(S.RLE) and _codecs("i32/rle_emit") == four(S.RLE)
    assert _codecs("i32/sorted") == four(S.DELTABP)
    assert _codecs("i32/freq") == four(S.FREQ, S.NONE) and _codecs("i32lz4/freq") == four(S.FREQ, S.LZ4)
    assert _codecs("i32/freq_small")[0] == [S.FREQ] * 4 and _codecs("i32lz4/freq_small")[0] == [S.FREQ] * 4
    assert _codecs("i32/one_page_each") == ([S.ONEVALUE, S.BITPACK, S.RLE, S.NONE], [255] * 4)
    assert _codecs("f64/patas") == four(S.PATAS) and _codecs("f64/uniform") == four(S.NONE)
    assert _codecs("i64/runs4") == four(S.DICT, S.DELTABP) and _codecs("i64/freq_dict") == four(S.FREQ, S.DICT)
    assert _codecs("i16/runs64") == four(S.RLE) and _codecs("i16/runs256") == four(S.DICT, S.RLE) and _codecs("i16/freq")[0] == [S.FREQ] * 4
    assert sorted(set(_codecs("bool/runs100")[0])) == [S.NONE, S.RLE] and _codecs("bool/runs1000") == four(S.RLE)
    assert _codecs("bool/const") == four(S.ONEVALUE) and _codecs("bool/random") == four(S.NONE)
    assert _codecs("bin/scattered") == ([S.DICT] * 2, [S.BITPACK] * 2) and _codecs("bin/in_runs") == ([S.DICT] * 2, [S.RLE] * 2)
    assert _codecs("long/uniform") == ([S.NONE], [255]) and _codecs("long/dict400") == ([S.DICT], [S.BITPACK])
    assert _codecs("long/freq") == ([S.FREQ], [S.NONE]) and _codecs("long/runs64") == ([S.RLE], [255])
    assert _codecs("long/dict_runs") == ([S.DICT], [S.RLE])


def test_the_internal_slots_follow_the_restated_rules():
    n = lambda name, fused=True: W.needs(W.VARIANT[name], fused)
    # slot 31: runs of 64 stay with the run-level selector, a uniform page does not; a long page is counted but not in need
    assert W.HINT_ROW_SELECT not in n("i32/runs64")[0] and W.HINT_ROW_SELECT in n("i32/uniform")[1]
    assert n("i32/small_runs7") == ({S.BITPACK}, {S.BITPACK}) and n("i32/small") == ({S.BITPACK, W.HINT_ROW_SELECT},) * 2
    assert W.HINT_ROW_SELECT in n("long/runs64")[0] and n("long/runs64")[1] == frozenset()
    # slot 29: a kept RLE page counts nowhere; one written after the early stop counts RLE and the slot
    assert n("i32/runs64") == (frozenset(), frozenset())
    assert n("i32/rle_emit") == ({S.RLE, W.HINT_RLE_EMIT, W.HINT_ROW_SELECT}, {W.HINT_RLE_EMIT, W.HINT_ROW_SELECT})
    col = W.VARIANT["i32/rle_emit"].column()
    page = col["values"][:W.PAGE].view(np.uint32)
    assert W.speculation_stopped(page[:W.CHUNK_ROWS]) and not W.speculation_stopped(page[W.CHUNK_ROWS:])
    # ... Int16 and Boolean cover the codec-id RLE slot instead
    assert n("i16/runs64")[1] == {S.RLE} and n("bool/runs1000")[1] == {S.RLE}
    # slot 30: only the pages k_enc_bin_page does not finish; without the fused kernel the DICT slot
    assert n("bin/scattered") == ({S.DICT}, frozenset()) and n("bin/in_runs") == ({S.DICT, W.HINT_BIN_DICT_EMIT}, {W.HINT_BIN_DICT_EMIT})
    assert n("bin/scattered", False)[1] == {S.DICT} and n("bin/in_runs", False)[1] == {S.DICT}
    # slot 28 and FREQ: never apart
    for v in W.VARIANT.values():
        c, _ = W.needs(v)
        assert (W.HINT_FREQ in c) == (S.FREQ in c), v
    assert n("i32/freq")[1] == {W.HINT_FREQ} and n("long/freq")[1] == {W.HINT_FREQ, S.FREQ}
    # the virtual pages of long pages: the index array is counted, the short exceptions block is not
    assert n("long/dict400")[0] == {S.DICT, S.BITPACK, W.HINT_ROW_SELECT} and n("long/freq")[0] == {S.FREQ, W.HINT_FREQ, W.HINT_ROW_SELECT}
    assert W.SEL_BIG_ROWS >= W.VBIG_ROWS


def test_every_case_is_well_formed():
    assert len(W.CASE) == len(W.CASES)
    for c in W.CASES:
        for iv in c.intervals():
            for names, mem in iv:
                assert all(nm in W.VARIANT for nm in names), c
                assert mem == (W.MEM_HOST if c.entry == "host" else W.MEM_DEVICE)
        # an interval's calls: three to six short calls of at most 256 KiB each, or long ones of 1 MiB
        calls = [call for iv in c.intervals() for call in iv]
        assert 2 <= len(calls) <= 8, c
        e = c.expected()
        assert len(e) == len(c.history) + 2 and e[-1] == 0, "the probe again is never replayed: %s" % c
        assert c.expected(no_hints=True) == (0,) * len(e), c


def test_the_full_cross_is_there():
    for t in W.TABLES.values():
        if t.name != "other":
            for x in t.variants:
                for y in t.variants:
                    assert "%s-%s-after-2x-%s" % (t.name, y, x) in W.CASE
    entries = {c.entry for c in W.CASES}
    assert entries == {"device", "two_calls", "two_plans", "host", "mixed"}


# FREQ and HINT_FREQ count the same pages (see the table's docstring): a history cannot hold one without the other
NOT_ISOLATED = (S.FREQ,)


@pytest.mark.parametrize("slot", W.CONSULTED, ids=lambda s: W.SLOT_NAMES[s])
def test_every_consulted_slot_is_crossed(slot):
    """a condition, not a measurement: a case where the slot is absent from the history, needed by the probe and the
    model expects the replay -- for that slot ALONE, so that launching it unconditionally changes the count --, and a
    case where the same probe costs none"""
    assert slot not in W.NOT_CROSSED and len(W.NOT_CROSSED) <= 2
    hit = [c for c in W.CASES if slot in c.crossed() and c.expected()[-2] == 1]
    assert hit, "no case crosses %s" % W.SLOT_NAMES[slot]
    alone = [c for c in hit if c.crossed() == {slot}]
    if slot in NOT_ISOLATED:
        assert not alone and all(W.HINT_FREQ in c.crossed() for c in hit)
    else:
        assert alone, "no case crosses %s alone" % W.SLOT_NAMES[slot]
    probes = {c.probe for c in hit}
    free = [c for c in W.CASES if c.probe in probes and c.history and c.expected()[-2] == 0 and not c.crossed()]
    assert free, "no case where a probe that needs %s costs no replay" % W.SLOT_NAMES[slot]


def test_the_model_on_the_documented_sequences():
    e = lambda name, **kw: W.CASE[name].expected(**kw)
    # the existing Dict-emitter test's sequence (tests/test_gpu_select.py), at this table's size
    assert e("bin-in_runs-after-2x-scattered") == (0, 0, 1, 0)
    assert e("bin-in_runs-after-2x-scattered", bin_fused=False) == (0, 0, 0, 0)
    # ... and the long-page one's (tests/test_gpu_big_pages.py): plain, plain, dict / freq
    assert e("long-dict400-after-2x-uniform") == (0, 0, 1, 0) and e("long-freq-after-2x-uniform") == (0, 0, 1, 0)
    assert e("long-runs64-after-2x-uniform") == (0, 0, 0, 0)
    # a fresh context, and a context whose plan has completed one call
    assert e("i32-const-fresh") == (0, 0) and e("i32-uniform-after-1x-runs64") == (0, 1, 0)
    # the maximum of two; x aged out
    assert e("i32-uniform-after-uniform-const") == (0, 1, 0, 0) and e("i32-uniform-after-uniform-2x-const") == (0, 1, 0, 1, 0)
    # a plan miss forgets the counts
    assert e("i32-uniform-after-const-miss") == (0, 0, 0, 0, 0)
    assert e("i32-uniform-after-other-const") == (0, 0, 1, 0) and e("i32-small-after-other-small_runs7") == (0, 0, 1, 0)
    # after a replay both kinds are kept: alternation is not replayed again
    assert e("i32-uniform-const-alternating") == (0, 0, 1, 0, 0, 0)
    # two calls in one interval: one replay for both
    assert e("i32-uniform-then-const-one-interval") == (0, 0, 1, 0)
    # two plans in one interval: only the second call's counts are the plan's (other/uniform's plain pages are forgotten)
    assert e("i32-uniform-after-other-and-const-one-interval") == (0, 1, 0) and e("i32-small-after-other-and-small_runs7-one-interval") == (0, 1, 0)
    # the mixed call: the Int16 RLE pages need their emitter; a binary column that stays Dict with another index codec needs slot 30
    assert e("mixed-i16-runs64") == (0, 0, 1, 0) and e("mixed-bin-in_runs") == (0, 0, 1, 0) and e("mixed-i32-small") == (0, 0, 0, 0)
