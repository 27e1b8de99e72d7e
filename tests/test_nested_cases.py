"""The nested edge table (tests/nested_cases.py) on the CPU oracle: for every case and every cut of it,
S.nested_write_levels -> S.nested_read_levels rebuilds what nested_gen.expected_state derives from the Arrow buffers
(lengths, offsets, validity, leaf validity, num_values, leaf_start, leaf_count), and the condition the case was built for
holds.  This is what lets tests/test_gpu_nested_edges.py trust the oracle at shapes it was never pinned at before.
No case is skipped; the two pages of more than 64 tiles are compared as numpy arrays (expected_arrays), every other page
with both."""
import numpy as np
import pytest

from oracle import sbo as S
from tests import nested_cases as NC
from tests.nested_gen import expected_state


def _round_trip(levels, r0, ln):
    b, nv, ls, lc = S.nested_write_levels(levels, r0, ln)
    got = S.nested_read_levels(b, nv, [lv["kind"] for lv in levels], [int(lv["is_optional"]) for lv in levels])
    assert got["consumed"] == len(b)
    return got, nv, ls, lc


@pytest.mark.parametrize("name", NC.case_names())
def test_oracle_round_trip_and_condition(name):
    case = NC.by_name(name)
    levels, rows = case.levels, case.rows
    text, check = case.prop
    assert check(levels, rows, case.cuts), "the case no longer has its property: %s" % text
    assert levels[0]["length"] == rows and levels[-1]["kind"] == S.K_PRIMITIVE and len(levels) <= 8
    for cut in case.cuts:
        for r0, ln in NC.page_ranges(rows, cut):
            got, nv, ls, lc = _round_trip(levels, r0, ln)
            want = NC.expected_arrays(levels, r0, ln)
            where = "%s rows %d..%d" % (name, r0, r0 + ln)
            assert (nv, ls, lc) == (want["num_values"], want["leaf_start"], want["leaf_count"]), where
            assert got["lengths"] == want["lengths"], where
            for k in range(len(levels)):
                assert np.array_equal(got["offsets"][k], want["offsets"][k]), "offsets of level %d, %s" % (k, where)
                assert np.array_equal(got["validity"][k], want["validity"][k]), "validity of level %d, %s" % (k, where)
            assert np.array_equal(got["leaf_validity"], want["leaf_validity"]), where
            if case.big:
                continue
            ref = expected_state(levels, r0, ln)   # the same through nested_gen's own (list based) derivation
            assert (nv, ls, lc) == (ref["num_values"], ref["leaf_start"], ref["leaf_count"]), where
            assert got["lengths"] == ref["lengths"], where
            for k in range(len(levels)):
                assert got["offsets"][k].tolist() == ref["offsets"][k], "offsets of level %d, %s" % (k, where)
                assert got["validity"][k].tolist() == ref["validity"][k], "validity of level %d, %s" % (k, where)
            assert got["leaf_validity"].tolist() == ref["leaf_validity"], where


def test_the_table_has_what_the_kernels_branch_on():
    """both encode paths, every header length, both sides of every constant: counted over the table, not per case"""
    cs = NC.cases()
    fast = [c for c in cs if NC.is_fast_path(c.levels)]
    generic = [c for c in cs if not NC.is_fast_path(c.levels)]
    assert len(fast) >= 20 and len(generic) >= 20
    for group in (fast, generic):
        ls = {NC.expected_arrays(c.levels, 0, c.rows)["num_values"] for c in group if c.name.startswith("exact_")}
        assert ls == set(NC.EXACT_L)
        assert any(c.big for c in group)
    assert NC.NE_CHUNK == NC.TILE - 32 and NC.MORE_THAN_64_TILES == 64 * NC.TILE + 1
    assert max(NC.expected_arrays(c.levels, 0, c.rows)["num_values"] for c in cs) == NC.MORE_THAN_64_TILES
    assert len({c.name for c in cs}) == len(cs)


def test_stream_header_lengths_of_the_exact_cases():
    """the rep stream's header is uleb((ceil(L / 8) << 1) | 1): 1 byte up to L = 504, 2 up to 65528, then 3"""
    for L, nbytes in ((504, 1), (505, 2), (65528, 2), (65529, 3)):
        c = NC.by_name("exact_list_%d" % L)
        b, nv, _, _ = S.nested_write_levels(c.levels, 0, c.rows)
        assert nv == L
        h, n = (((L + 7) // 8) << 1) | 1, 0
        want = bytearray()
        while True:
            n += 1
            want.append((h & 0x7F) | (0x80 if h >= 0x80 else 0))
            h >>= 7
            if not h:
                break
        assert n == nbytes and bytes(b[12:12 + n]) == bytes(want)
        rep_len = int.from_bytes(bytes(b[4:8]), "little")
        assert rep_len == n + (L // 32) * 4 + (L % 32 + 7) // 8   # 1 bit per rep level
