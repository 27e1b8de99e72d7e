"""The selector's boundary table (tests/select_cases.py) against the CPU oracle alone: every case sits where it claims.

  * the oracle's page codecs equal what the table states,
  * neighbours that are meant to flip differ,
  * the input properties of the run-level kernel's cases (raw runs per 4096-row chunk, ...) hold,
  * the constants the table was built around are the ones in the device sources and in the oracle.

tests/test_gpu_select_boundaries.py sends the same columns through the device."""
import os
import re

import pytest

from oracle import sbo as S
from tests import gen
from tests import select_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = T.families()

_codecs = {}


def oracle_codecs(case):
    """page codecs the oracle chooses for a case (computed once per case)"""
    if case.name not in _codecs:
        pages, metas = gen.oracle_write(case.col, **case.opt)
        _codecs[case.name] = S.stat_column(case.col["ptype"], case.col["nullable"], pages, metas)[0].tolist()
    return _codecs[case.name]


def test_the_table_is_well_formed():
    assert len(T.CASES) > 500 and len(FAMILIES) == 21
    for c in T.CASES.values():
        assert c.col["rows"] <= 65536, c.name
        assert c.neighbour is None or c.neighbour in T.CASES, "%s names a neighbour that does not exist" % c.name
        assert c.flips is False or c.neighbour is not None, c.name


@pytest.mark.parametrize("family", list(FAMILIES))
def test_oracle_chooses_what_the_table_states(family):
    wrong = []
    for c in FAMILIES[family]:
        got = oracle_codecs(c)
        if got != c.expect:
            wrong.append("%s: the oracle chose %s, the table states %s" % (c.name, T.names(got), T.names(c.expect)))
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_neighbours_flip(family):
    wrong = []
    for c in FAMILIES[family]:
        if c.flips and oracle_codecs(c) == oracle_codecs(T.CASES[c.neighbour]):
            wrong.append("%s and %s: both %s" % (c.name, c.neighbour, T.names(oracle_codecs(c))))
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("family", [f for f in FAMILIES if any(c.prop for c in FAMILIES[f])])
def test_input_properties_hold(family):
    wrong = []
    for c in FAMILIES[family]:
        if c.prop is not None:
            ok, why = c.prop(c.col)
            if not ok:
                wrong.append("%s: %s" % (c.name, why))
    assert not wrong, "\n".join(wrong)


def test_section_b_states_a_property_for_every_case():
    for family in ("runs_cap", "step2", "page_len", "spec_stop", "null_runs"):
        assert all(c.prop is not None for c in FAMILIES[family]), family


def test_the_runs_cap_cases_sit_on_640_and_641():
    seen = set()
    for c in FAMILIES["runs_cap"]:
        per_chunk = T.raw_runs_per_chunk(c.col)
        assert len(per_chunk) == 4 and c.col["rows"] == 3 * T.CHUNK + 1000
        seen.add((per_chunk.index(max(per_chunk)), max(per_chunk)))
    assert seen == {(k, r) for k in (0, 2, 3) for r in (T.RUNS_CAP, T.RUNS_CAP + 1)}


def test_the_speculation_can_only_stop_at_a_pages_last_chunk():
    """why spec_stop has no page that walks on after the stop: k whole chunks hold at most RUNS_CAP * k records"""
    assert 4 * T.RUNS_CAP <= T.CHUNK
    for c in FAMILIES["spec_stop"]:
        k = T.speculation_stops_at(c.col)
        assert k is None or k == len(T.raw_runs_per_chunk(c.col)) - 1, c.name


def _source(*rel):
    with open(os.path.join(ROOT, *rel)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.findall(pattern, text)
    assert m, "%s: the pattern %r no longer matches; update tests/select_cases.py with the source" % (what, pattern)
    assert len(set(m)) == 1, "%s: several different values %s" % (what, m)
    return m[0]


def test_constants_of_the_table_are_the_ones_in_the_sources():
    """A change of RUNS_CAP, the key-set size, PD_CAP or the sample sizes must come with a change of the table: the cases
    would silently move off their boundaries otherwise."""
    csrc = ("strawboat_amd", "csrc")
    runs_h, select_h, encode = _source(*csrc, "sb_select_runs.h"), _source(*csrc, "sb_select.h"), _source(*csrc, "sb_encode.hip")
    common_h, rle_h, oracle = _source(*csrc, "sb_common.h"), _source(*csrc, "sb_select_rle.h"), _source("oracle", "sbo_codecs.cpp")
    assert int(_one(r"constexpr\s+uint32_t\s+RUNS_CAP\s*=\s*(\d+)\s*;", runs_h, "RUNS_CAP")) == T.RUNS_CAP
    assert int(_one(r"constexpr\s+int\s+WG\s*=\s*(\d+)\s*;", common_h, "WG")) == T.WG
    assert int(_one(r"constexpr\s+int\s+K\s*=\s*(\d+)\s*;", runs_h, "rows per thread of the run-level kernel")) == T.K_ROWS
    assert _one(r"constexpr\s+uint32_t\s+CHUNK\s*=\s*([^;]+);", runs_h, "CHUNK").strip() == "WG * K"
    assert T.CHUNK == T.WG * T.K_ROWS
    assert int(_one(r"constexpr\s+uint32_t\s+SEL_LDS_SLOTS\s*=\s*(\d+)\s*;", select_h, "SEL_LDS_SLOTS")) == T.SEL_LDS_SLOTS
    for name, text in (("sb_select_runs.h", runs_h), ("sb_select_rle.h", rle_h), ("sb_encode.hip", encode)):
        ks, kc = _one(r"KSLOTS\s*=\s*SEL_LDS_SLOTS\s*/\s*(\d+)\s*,\s*KCAP\s*=\s*KSLOTS\s*/\s*(\d+)\s*;", text, "KCAP in " + name)
        assert T.SEL_LDS_SLOTS // int(ks) // int(kc) == T.KCAP, name
    assert int(_one(r"\bPD_CAP\s*=\s*(\d+)\s*;", encode, "PD_CAP")) == T.PD_CAP
    for name, text in (("sb_select.h", select_h), ("oracle/sbo_codecs.cpp", oracle)):
        sc, ss = _one(r"SAMPLE_COUNT\s*=\s*(\d+)\s*,\s*SAMPLE_SIZE\s*=\s*(\d+)\s*;", text, "sample sizes in " + name)
        assert (int(sc), int(ss)) == (T.SAMPLE_COUNT, T.SAMPLE_SIZE), name
    assert T.WHOLE_PAGE_MAX == 649
    mul, slack = _one(r"nrec\s*\*\s*(\d+)\s*>\s*cb\s*\+\s*n\s*\+\s*(\d+)", runs_h, "the speculation stop")
    assert (int(mul), int(slack)) == (4, T.SPEC_SLACK)
    assert _one(r"maj_n\s*\+\s*1\.0\s*>=\s*([0-9.]+)\s*\*\s*tuple_count", encode, "the vote shortcut") == "0.8"
