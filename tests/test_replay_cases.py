"""The table of the replay routes (tests/replay_cases.py) against the CPU oracle alone: it says what it claims.

  * every victim column has exactly the codec named (the index codec of a Dict page included) and no Freq page, the page
    shape named (five pages with a short last one, or one long RLE page), and the nullability named,
  * every trigger has a Freq page and the victim's row count,
  * case names are unique, and every kind, codec, trigger and variant the table is meant to hold is there,
  * every reference result can be computed, alone and with the trigger,
  * every float column of an aggregate case can tell the routes apart: its live rows added page by page and tile by tile
    give different double bits under at least one of the masks (OneValue: n * v differs from n additions of v).  That is a
    cap on the data, not a measurement: a column that cannot is given another seed here.

tests/test_gpu_replay_routes.py sends the same cases through the device."""
import struct

import numpy as np
import pytest

from oracle import sbo as S
from tests import replay_cases as RC


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def _victims():
    seen = {}
    for c in RC.CASES:
        seen.setdefault(c.column.id, c.column)
    return list(seen.values())


def test_long_rle_rows_is_the_suites_shape():
    from tests.test_gpu_decode import LONG_RLE_ROWS
    assert RC.LONG_RLE_ROWS == LONG_RLE_ROWS and LONG_RLE_ROWS > 64 * RC.TILE_ROWS


@pytest.mark.parametrize("column", _victims(), ids=repr)
def test_victim_column_is_what_it_claims(column):
    col, pages, metas = RC.written(column.id)
    codec, icodec = RC.CODECS[column.codec]
    codecs, inner = RC.page_codecs(column.id)
    assert codecs == {codec}, "%s: page codecs %r, named %r" % (column.name, codecs, codec)
    assert S.FREQ not in codecs and S.FREQ not in inner
    if icodec is not None:
        assert inner == {icodec}, "%s: index codecs %r, named %r" % (column.name, inner, icodec)
    assert col["ptype"] == column.ptype and col["nullable"] == column.nullable and col["rows"] == column.rows
    rows = [int(n) for n in np.asarray(metas)[:, 1]]
    if column.codec == "long_rle":
        assert rows == [RC.LONG_RLE_ROWS]
    else:   # five pages with a short last one, the tile borders at 4096 / 8192 inside pages
        n = column.page_rows
        assert rows == [n] * 4 + [column.rows - 4 * n] and 0 < rows[-1] < n
        assert 4096 % n and 8192 % n
        if column.codec not in RC.PACKED:   # ... and the page seams inside bitmap words
            assert n == 2050 and column.rows == 10_000 and all(e % 32 for e in np.cumsum(rows)[:-1])
    ref = RC.ref_of(column.id)
    assert ref.rows == column.rows
    if column.nullable:
        assert 0.05 < 1 - ref.valid.mean() < 0.15
    else:
        assert ref.valid.all()
    if column.recipe == "keys":
        assert np.unique(ref.vals[ref.valid]).size <= RC.KEY_MAX_KEYS
    if column.recipe == "many":
        assert np.unique(ref.vals[ref.valid & RC.masks(column.rows)[0]]).size > RC.KEY_MAX_KEYS
    if column.codec == "onevalue" and column.ptype in RC.FLOATS:
        assert float(ref.vals[0]) == float(RC.NP[column.ptype](0.1))


@pytest.mark.parametrize("rows", sorted({c.column.rows for c in RC.CASES}))
def test_trigger_has_freq_pages(rows):
    codecs, _ = RC.page_codecs(RC.trigger_id(rows))
    col = RC.written(RC.trigger_id(rows))[0]
    assert S.FREQ in codecs and col["ptype"] == S.T_I64 and col["rows"] == rows and col["nullable"]


def test_extra_columns_hold_no_freq_page():
    for cid in RC.extra_columns():
        codecs, inner = RC.page_codecs(cid)
        assert S.FREQ not in codecs and S.FREQ not in inner, cid


def test_the_table_holds_every_case_it_is_meant_to():
    assert len(RC.CASE) == len(RC.CASES), "case names are unique"
    for kind in RC.KINDS:
        mine = [c for c in RC.CASES if c.kind == kind]
        cols = {c.column.id: c.column for c in mine}.values()
        named = {c.codec for c in cols}
        want = set(RC.CODECS) - ({"patas"} if kind == "key_ids" else set())
        assert named == want, (kind, named ^ want)
        for codec in named - {"bitpack", "deltabp", "long_rle", "patas"}:   # a type of at most 4 bytes and one of 8
            widths = {S.WIDTH[c.ptype] for c in cols if c.codec == codec}
            assert 8 in widths and min(widths) <= 4, (kind, codec, widths)
        assert any(not c.nullable for c in cols), kind
        for col in cols:   # every column under every trigger and order
            assert {(c.trigger, c.order) for c in mine if c.column.id == col.id and c.variant == "plain"} == set(RC.TRIGGERS)
        assert any(c.variant == "chain" for c in mine), kind
        if kind == "aggregate":   # every codec that can hold floats, with both float types
            for codec in want - {"bitpack", "deltabp", "long_rle", "patas"}:
                assert {c.ptype for c in cols if c.codec == codec and c.recipe == "inexact"} == set(RC.FLOATS), codec
        if kind == "key_ids":
            assert any(c.recipe == "many" for c in cols)
    assert sum(c.variant == "mixed" for c in RC.CASES) == len(RC.TRIGGERS)


@pytest.mark.parametrize("case", RC.CASES, ids=repr)
def test_case_has_references(case):
    """the references of the interval alone and with the trigger; the victim's are the same in both"""
    alone, with_t = case.calls(False), case.calls(True)
    wa, wt = RC.wants_of(alone), RC.wants_of(with_t)
    assert sum(len(c.entries) for c in with_t) == sum(len(c.entries) for c in alone) + 1
    assert sum(e.trigger for c in with_t for e in c.entries) == 1 and not any(e.trigger for c in alone for e in c.entries)
    roles = [c.role for c in with_t]
    if case.trigger == "c":
        assert "trigger" not in roles and with_t[roles.index("victim")].entries[1].trigger
    else:
        assert roles[0 if case.order == "before" else -1] == "trigger" and roles.count("trigger") == 1
    # the victim's wants do not depend on the trigger
    flat_a = [w for c, ws in zip(alone, wa) for e, w in zip(c.entries, ws)]
    flat_t = [w for c, ws in zip(with_t, wt) for e, w in zip(c.entries, ws) if not e.trigger]
    assert len(flat_a) == len(flat_t)
    for a, t in zip(flat_a, flat_t):
        if isinstance(a, np.ndarray):
            assert np.array_equal(a, t)
    # a filter victim selects something and not everything; a selection is neither empty nor full
    for c, ws in zip(alone, wa):
        if c.kind in RC.FILTER_KINDS and c.role == "victim" and case.column.codec != "onevalue":
            assert any(0 < w.sum() < w.size for w in ws), case.name
    if case.variant == "chain":
        chain = wa[1][0]
        assert 0 < chain.sum() < chain.size


def _float_victims():
    return [c for c in _victims() if c.recipe == "inexact"]


@pytest.mark.parametrize("column", _float_victims(), ids=repr)
def test_float_column_can_tell_the_routes_apart(column):
    masks = RC.masks(column.rows)
    if column.codec == "onevalue":
        pairs = [RC.onevalue_sums(column.id, m) for m in masks]
        if column.ptype == S.T_F32:
            # float(0.1f) has 24 significant bits: the product and up to 2^29 additions of it are exact in double, so no
            # route can give other bits.  The case stays (its bytes are compared like every other's); it cannot tell.
            assert all(_bits(a) == _bits(b) for a, b in pairs)
            return
    else:
        pairs = [RC.sums_by_route(column.id, m) for m in masks]
    assert any(_bits(a) != _bits(b) for a, b in pairs), "%s: the same sum on both routes under every mask: choose another seed" % column.name
