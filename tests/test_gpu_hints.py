"""Reads on contexts of every launch-hint history (tests/hint_cases.py), against the oracle.

Every case gets a context of its own: the history's read intervals first, then the probe into buffers filled with a poison
byte, compared with the oracle's decode (sinks: with the references of their own suites); then the same probe once more, and
a small plain read at the end.  The replays each step costs (sb_ctx_replays) are the table's, which come from its model of
update_read_hints / read_hints; with SB_NO_HINTS=1 (or SB_ZSTD_BLOCKS set) the model is asked for that switch's counts and
nothing else changes -- every value assertion runs under every switch.

The selection of a selected read or an aggregate is the reference result of the case's filter predicate, uploaded: a filter
call on the same context would put an interval of its own between the history and the probe.  A Freq page holds one value
on 90 % of its rows, so no comparison matches half of them: the predicate (<= 0, the top value) takes the top rows and half
of the exceptions.

Measured on an MI355X: a context costs 3.6 ms to create and destroy, so every case affords one; the module's 192 tests take
8.5 s (9.9 s with SB_NO_HINTS=1), the slowest 0.2 s apart from the first, which loads the library (1.6 s).  The 24 cases
of the later sinks (filter_in, topk, key_ids, aggregate_grouped_large) add 6.2 s: their references run over the probes'
millions of rows once per case (300 groups: 0.3 - 0.7 s a case)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from oracle import sbo as S
from tests import aggregate_grouped_ref as G
from tests import aggregate_ref as R
from tests import hint_cases as H
from tests import key_ids_ref as K
from tests import topk_ref as T

pytestmark = pytest.mark.gpu
POISON = 0xA5
AGG_OPS = ("count", "sum")


def _switches():
    """(no_hints, zb_mode) as sb_ctx_create reads them"""
    nh, zb = os.environ.get("SB_NO_HINTS"), os.environ.get("SB_ZSTD_BLOCKS")
    return nh is not None and nh[:1] != "0", 2 if zb is None else 0 if zb[:1] == "0" else 1 if zb[:1] == "1" else 2


_written = {}


def fixed(probe):
    """the pages of a history interval or of the closing read: written once, shared, never modified"""
    if probe.name not in _written:
        cols = H.written(probe, 1)
        for col, pages, metas, want in cols:
            for a in (pages, metas, want["values"], want["validity"], want["offsets"]):
                a.setflags(write=False)
        _written[probe.name] = cols
    return _written[probe.name]


def up(ctx, a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(ctx.torch_device)


def column_pages(ctx, cols):
    from strawboat_amd import read
    return [read.ColumnPages(col["ptype"], col["nullable"], up(ctx, pages), metas) for col, pages, metas, _ in cols]


def poisoned(ctx, cols):
    """output buffers of exactly the documented capacities, every byte POISON"""
    import torch
    from strawboat_amd import read
    full = lambda n: torch.full((int(n),), POISON, dtype=torch.uint8, device=ctx.torch_device)
    outs = []
    for col, _, _, want in cols:
        t, rows = col["ptype"], col["rows"]
        if t in H.BINARIES:
            values, offsets = full(max(want["values"].size, 1)), full((rows + 1) * (4 if t == S.T_BIN32 else 8))
        else:
            values, offsets = full(rows * S.WIDTH[t]), None
        validity = full((rows + 31) // 32 * 4) if col["nullable"] else None
        outs.append(read.DeviceArray(t, col["nullable"], rows, values, validity, offsets, None))
    return outs


def check_arrays(cols, got):
    for (col, _, _, want), g in zip(cols, got):
        assert g.rows == want["rows"] and g.values_len == want["values"].size
        assert np.array_equal(g.values_numpy(), want["values"]), "values differ from the oracle's decode"
        if col["nullable"]:
            assert np.array_equal(g.validity_numpy(), want["validity"]), "validity differs"
        if col["offsets"] is not None:
            assert np.array_equal(g.offsets_numpy(), want["offsets"]), "offsets differ"


def read_device(ctx, cols):
    from strawboat_amd import read
    got = read.batch_read_columns(ctx, column_pages(ctx, cols), out=poisoned(ctx, cols))
    ctx.synchronize()
    check_arrays(cols, got)


def read_host(ctx, cols):
    """SB_MEM_HOST: host page bytes in, host Arrow buffers out (primitive columns without nulls)"""
    from strawboat_amd import _native as N
    n = len(cols)
    cr = (N.ColumnReadC * n)()
    keep = []
    for i, (col, pages, metas, want) in enumerate(cols):
        assert not col["nullable"] and col["offsets"] is None
        p, m = np.array(pages, copy=True), np.ascontiguousarray(metas, np.uint64)
        out = np.full(col["rows"] * S.WIDTH[col["ptype"]], POISON, np.uint8)
        keep.append((p, m, out))
        cr[i].physical_type, cr[i].is_nullable = col["ptype"], 0
        cr[i].pages, cr[i].pages_len = p.ctypes.data, p.size
        cr[i].metas, cr[i].n_pages = m.ctypes.data_as(C.POINTER(N.PageMetaC)), m.shape[0]
        cr[i].values, cr[i].values_capacity = out.ctypes.data, out.size
    ctx._check(ctx._lib.sb_read_columns(ctx._h, cr, n, N.SB_MEM_HOST))
    ctx.synchronize()
    for i, (col, _, _, want) in enumerate(cols):
        assert cr[i].rows == want["rows"] and cr[i].values_len == want["values"].size
        assert np.array_equal(keep[i][2], want["values"]), "values differ from the oracle's decode"


def sizes_then_read(ctx, cols, bin_cols):
    """a read is enqueued, and the synchronize that a sizes call brings closes its interval"""
    from strawboat_amd import read
    batch = read.ReadBatch(ctx, column_pages(ctx, cols), out=poisoned(ctx, cols))
    got = batch.enqueue()
    sizes = read.batch_read_sizes(ctx, column_pages(ctx, bin_cols))
    assert sizes == [(want["rows"], want["values"].size) for _, _, _, want in bin_cols], "rows / values_len of the sizes call"
    check_arrays(cols, got)
    ctx.synchronize()


def _typed(col, want):
    return want["values"].view(np.dtype(R.NP[col["ptype"]]))[:col["rows"]]


def predicate_of(col):
    """(Predicate, the rows it matches): half of the rows of a U8 column, the top value and half of the exceptions of a Freq one"""
    from strawboat_amd.filter import Predicate
    return Predicate("lt", 128) if col["ptype"] == S.T_U8 else Predicate("le", 0)


def matching(col, want):
    v = _typed(col, want)
    mask = v < 128 if col["ptype"] == S.T_U8 else v <= 0
    assert 0.4 < mask.mean() < 0.97
    return mask


def selection_tensor(ctx, mask):
    bits = np.zeros((mask.size + 31) // 32 * 4, np.uint8)
    packed = np.packbits(mask, bitorder="little")
    bits[:packed.size] = packed
    return up(ctx, bits)


_wants = {}


def _once(sink, seed, compute):
    """the reference of a case's probe, computed for the first of its two runs and left unchanged (a case has a seed of its own)"""
    if (sink, seed) not in _wants:
        _wants[(sink, seed)] = compute()
    return _wants[(sink, seed)]


def run_sink(ctx, sink, cols, seed):
    import torch
    from strawboat_amd import filter as flt
    from strawboat_amd.aggregate import aggregate_columns
    from strawboat_amd.aggregate_grouped import aggregate_grouped
    from strawboat_amd.aggregate_grouped_large import aggregate_grouped_large
    from strawboat_amd.filter_in import InList, filter_in
    from strawboat_amd.key_ids import key_ids
    from strawboat_amd.read_selected import read_selected
    from strawboat_amd.topk import topk_columns
    from tests.test_gpu_filter_in import want_in
    (col, pages, metas, want), = cols
    cp, = column_pages(ctx, cols)
    mask = matching(col, want)
    rows = col["rows"]
    if sink == "filter":
        out = flt.Selection(torch.full(((rows + 31) // 32 * 4,), POISON, dtype=torch.uint8, device=ctx.torch_device), rows, None)
        sel, = flt.filter_columns(ctx, [cp], [predicate_of(col)], out=[out])
        ctx.synchronize()
        assert sel.selected == int(mask.sum())
        assert np.array_equal(sel.numpy(), mask), "the selection bitmap differs"
        return
    if sink == "filter_in":
        v = _typed(col, want)
        lits = [v[int(i)].item() for i in np.random.default_rng(seed).integers(0, rows, H.IN_LITERALS)]
        out = flt.Selection(torch.full(((rows + 31) // 32 * 4,), POISON, dtype=torch.uint8, device=ctx.torch_device), rows, None)
        sel, = filter_in(ctx, [cp], [InList(lits)], out=[out])
        ctx.synchronize()
        hit = _once(sink, seed, lambda: want_in(col, v, np.ones(rows, bool), lits, False))
        assert sel.selected == int(hit.sum()) > 0
        assert np.array_equal(sel.numpy(), hit), "the selection bitmap differs"
        assert not np.unpackbits(sel.bitmap.cpu().numpy(), bitorder="little")[rows:].any(), "bits behind the last row must be 0 after set"
        return
    sel = selection_tensor(ctx, mask)
    if sink == "read_selected":
        values = torch.full((rows * S.WIDTH[col["ptype"]],), POISON, dtype=torch.uint8, device=ctx.torch_device)
        got, = read_selected(ctx, [cp], sel, out=[(values, None)])
        ctx.synchronize()
        assert got.selected == int(mask.sum())
        assert np.array_equal(got.numpy()[0], _typed(col, want)[mask]), "the selected rows differ"
        return
    ref = R.Ref(col, pages, metas)
    if sink == "aggregate":
        got, = aggregate_columns(ctx, [cp], sel, ops=AGG_OPS)
        ctx.synchronize()
        R.check(got, ref.want(mask, AGG_OPS), sink)
        return
    if sink == "topk":
        got, = topk_columns(ctx, [cp], H.TOPK_K, False, sel)
        ctx.synchronize()
        T.check(got, _once(sink, seed, lambda: T.want(ref, mask, H.TOPK_K, False)), sink)
        return
    if sink == "key_ids":
        ids_out = torch.full((rows * 2,), POISON, dtype=torch.uint8, device=ctx.torch_device).view(torch.uint16)   # (exactly rows ids)
        got, = key_ids(ctx, [cp], sel, max_keys=H.KEY_MAX_KEYS, id_width=2, out=[ids_out])
        ctx.synchronize()
        want_keys = _once(sink, seed, lambda: K.want(ref, mask, H.KEY_MAX_KEYS, 2))
        assert want_keys.overflow == (col["ptype"] != S.T_U8), "the Int64 Freq probe overflows max_keys, a U8 probe cannot"
        K.check(got, want_keys, sink)   # (rows, selected, count, overflow; keys and ids where nothing overflowed)
        return
    if sink == "aggregate_grouped_large":
        ids = np.random.default_rng(seed).integers(0, H.N_GROUPS_LARGE, rows).astype(np.uint16)
        got, = aggregate_grouped_large(ctx, [cp], up(ctx, ids), H.N_GROUPS_LARGE, sel, ops=AGG_OPS)
        ctx.synchronize()
        G.check(got, _once(sink, seed, lambda: G.want(ref, ids, H.N_GROUPS_LARGE, mask, AGG_OPS)), sink)
        return
    ids = np.random.default_rng(seed).integers(0, H.N_GROUPS, rows).astype(np.uint8)
    got, = aggregate_grouped(ctx, [cp], up(ctx, ids), H.N_GROUPS, sel, ops=AGG_OPS)
    ctx.synchronize()
    G.check(got, G.want(ref, ids, H.N_GROUPS, mask, AGG_OPS), sink)


ZSTD_MAGIC = np.frombuffer((0xFD2FB528).to_bytes(4, "little"), np.uint8)


def device_written(seed):
    """the bytes of zstd_1mib as ONE Basic(Zstd) page of the device's writer: a frame per piece of the input, so the
    buffer is LONG (>= ZSTD_LONG_MIN) and made of many frames -- what the frame scan (zs_on) is for.  Written on a
    context of its own; the oracle reads what the device wrote."""
    import strawboat_amd as sb
    from strawboat_amd import write, WriteOptions
    from tests.test_gpu_encode import to_device_column
    col = H._random_bytes(seed, 1_150_000)
    ctx = sb.Context(0)
    try:
        enc = write.write(ctx, to_device_column(ctx, col), WriteOptions(default_compression=S.ZSTD))
        pages, metas = enc.pages_numpy(), enc.metas_array()
    finally:
        ctx.close()
    want = S.read_column(col["ptype"], False, pages, metas)
    assert np.array_equal(want["values"], col["values"])
    assert H.features_of([(col, pages, metas)]) == H.DEVICE_WRITTEN_CLAIM
    body = pages[9:]
    magics = int(np.count_nonzero((body[:-3] == ZSTD_MAGIC[0]) & (body[1:-2] == ZSTD_MAGIC[1]) & (body[2:-1] == ZSTD_MAGIC[2]) & (body[3:] == ZSTD_MAGIC[3])))
    assert magics >= 16, "the device wrote %d frames" % magics
    return [(col, pages, metas, want)]


def run_probe(ctx, case, cols, extra):
    if case.entry == "device":
        read_device(ctx, cols)
    elif case.entry == "host":
        read_host(ctx, cols)
    elif case.entry == "sizes_then_read":
        sizes_then_read(ctx, cols, extra)
    else:
        run_sink(ctx, case.entry, cols, case.seed)


@pytest.mark.parametrize("case", H.CASES, ids=repr)
def test_case(case):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but torch.cuda.is_available() is False")
    import strawboat_amd as sb
    no_hints, zb_mode = _switches()
    exp = case.expected(no_hints, zb_mode)
    cols = device_written(case.seed) if isinstance(case.probe, str) else H.written(case.probe, case.seed)
    extra = H.written(H.SIZES_PROBE, case.seed) if case.entry == "sizes_then_read" else None
    ctx = sb.Context(0)
    try:
        for name, replays in zip(H.HISTORIES[case.history], exp.history):
            r0 = ctx.replays()
            read_device(ctx, fixed(H.INTERVALS[name]))
            assert ctx.replays() - r0 == replays, "history interval %r: %d replays, the model says %d" % (name, ctx.replays() - r0, replays)
        for what, replays in (("the probe", exp.probe), ("the probe again", exp.again)):
            r0 = ctx.replays()
            run_probe(ctx, case, cols, extra)
            assert ctx.replays() - r0 == replays, "%s: %d replays, the table says %d" % (what, ctx.replays() - r0, replays)
        read_device(ctx, fixed(H.PROBE["plain_i64"]))   # the context still works
    finally:
        ctx.close()


def test_context_creation_is_cheap():
    """a context per case is affordable: creating and destroying one is a stream, two small allocations and a few
    memsets -- 3.6 ms on an MI355X.  Printed, and asserted only loosely (a context must not cost a second): the table
    creates one per case."""
    import strawboat_amd as sb
    sb.Context(0).close()
    t0 = time.perf_counter()
    for _ in range(5):
        sb.Context(0).close()
    dt = (time.perf_counter() - t0) / 5
    print("context create + destroy: %.2f ms" % (dt * 1e3))
    assert dt < 1.0
