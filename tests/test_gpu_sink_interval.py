"""One interval that holds one call of every sink entry point, in this order: sb_filter_columns, sb_filter_columns_var,
sb_read_selected, sb_read_selected_var, sb_aggregate_columns, sb_aggregate_grouped.  The suites of the six drive one or two
kinds of call per interval; what the kinds share on the host -- the staging area and its shares, the staging slots, the
pending results, the temporaries of a replayed interval -- is shared exactly where they meet, so here they all meet.

Every call has two columns of two pages, 1000 and 37 rows: bitmap word 31 straddles the page seam.  The numeric columns
are nullable Int32, the binary ones nullable Utf8.  The selection of the reads and aggregates is the reference result of
the first filter predicate, uploaded (as tests/test_gpu_hints.py does), so no call depends on another.  Device outputs
are 0xA5-filled buffers of exactly the documented capacities; everything is compared with the oracle's decode through the
references of the six suites.  With freq=True the first numeric column of every call holds Freq pages and the interval is
issued again once: the decoded route of every kind that has one, the page route of the others, in one replay."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import sbo as S
from tests import aggregate_grouped_ref as G
from tests import aggregate_ref as R
from tests import gen
from tests.test_gpu_aggregate import bitmap
from tests.test_gpu_aggregate_grouped import ids_dev
from tests.test_gpu_filter import expected as num_expected, oracle_column as num_oracle, upload
from tests.test_gpu_filter_binary import expected as bin_expected, oracle_strings, strings_of
from tests.test_gpu_read_selected import Case as NumCase
from tests.test_gpu_read_selected_var import Case as BinCase

pytestmark = pytest.mark.gpu

ROWS, PAGE_ROWS = 1037, 1000
POISON = 0xA5
N_GROUPS = 3


@functools.lru_cache(maxsize=None)
def written(freq):
    """{name: (col, pages, metas)}: written once per parametrisation, never modified"""
    from tests.test_gpu_freq import sparse
    a = sparse(S.T_I32, ROWS, 0.05, 2, null_density=0.1) if freq else gen.prim(S.T_I32, ROWS, uniq=100, null_density=0.2, runs=4, seed=1)
    cols = dict(a=(a, S.FREQ if freq else S.RLE),
                b=(gen.prim(S.T_I32, ROWS, uniq=100, null_density=0.2, seed=4), S.DICT),
                s=(gen.binary(ROWS, uniq=60, null_density=0.1, seed=3, maxlen=20), S.DICT),
                t=(gen.binary(ROWS, uniq=80, null_density=0.2, seed=9, maxlen=16), S.NONE))
    out = {}
    for name, (col, codec) in cols.items():
        pages, metas = gen.oracle_write(col, max_page_size=PAGE_ROWS, force_codec=codec)
        assert [int(n) for n in metas[:, 1]] == [PAGE_ROWS, ROWS - PAGE_ROWS]
        assert col["nullable"]
        out[name] = (col, pages, metas)
    if freq:
        a, pages, metas = out["a"]
        assert S.FREQ in set(int(x) for x in S.stat_column(a["ptype"], a["nullable"], pages, metas)[0].tolist())
    return out


def median(col):
    return int(np.sort(col["values"])[col["values"].size // 2])


def poisoned_selection(ctx):
    import torch
    from strawboat_amd.filter import Selection
    with torch.cuda.stream(ctx.torch_stream):   # (the fill is ordered before the call's kernels)
        buf = torch.full(((ROWS + 31) // 32 * 4,), POISON, dtype=torch.uint8, device=ctx.torch_device)
    return Selection(buf, ROWS, None)


def fixed_filter_array(batch, cols, preds):
    """the descriptors of a FilterBatch as sb_column_filter, the layout with the 8 inline literal bytes"""
    from strawboat_amd import _native as N, filter as F
    arr = (N.ColumnFilterC * len(cols))()
    for i, (col, (op, lit)) in enumerate(zip(cols, preds)):
        v, c = batch._arr[i], arr[i]
        for f in ("physical_type", "is_nullable", "pages", "pages_len", "metas", "n_pages", "page_offsets", "op", "combine",
                  "selection", "selection_capacity"):
            setattr(c, f, getattr(v, f))
        C.memmove(c.literal, F.pack_literal(col["ptype"], lit), 8)
    return arr


def check_selection(bitmap_tensor, cstruct, want, what):
    got = np.unpackbits(bitmap_tensor.cpu().numpy(), bitorder="little").astype(bool)
    assert int(cstruct.rows) == ROWS and int(cstruct.selected) == int(want.sum()), (what, int(cstruct.rows), int(cstruct.selected), int(want.sum()))
    assert np.array_equal(got[:ROWS], want), "%s: %d rows differ, first at %d" % (what, int((got[:ROWS] != want).sum()), int(np.argmax(got[:ROWS] != want)))
    assert not got[ROWS:].any(), "%s: bits behind the last row must be 0 after set" % what


@pytest.mark.parametrize("freq", [False, True])
def test_one_call_of_every_sink_in_one_interval(gpu_ctx, freq):
    import strawboat_amd as sb
    from strawboat_amd import _native as N
    from strawboat_amd.filter import FilterBatch
    ctx = gpu_ctx
    w = written(freq)
    (a, ap, am), (b, bp, bm), (s, sp, sm), (t, tp, tm) = w["a"], w["b"], w["s"], w["t"]
    a_or, b_or = num_oracle(a, ap, am), num_oracle(b, bp, bm)
    s_or, t_or = oracle_strings(s, sp, sm), oracle_strings(t, tp, tm)
    a_pred, b_pred = ("le", median(a)), ("gt", median(b))
    s_pred = ("lt", sorted(set(strings_of(s)))[30])
    a_want, b_want = num_expected(a, *a_or, *a_pred), num_expected(b, *b_or, *b_pred)
    s_want = bin_expected(*s_or, *s_pred)
    mask = a_want   # what the reads and aggregates consume: the reference result of the first filter predicate
    for m in (a_want, b_want, s_want):
        assert 0 < m.sum() < ROWS
    assert mask[PAGE_ROWS - 8:PAGE_ROWS].any() and mask[PAGE_ROWS:PAGE_ROWS + 24].any()   # (both sides of the seam, in one word)
    acp, bcp, scp = upload(ctx, a, ap, am), upload(ctx, b, bp, bm), upload(ctx, s, sp, sm)
    a_ref, b_ref = R.Ref(a, ap, am), R.Ref(b, bp, bm)
    ids = np.random.default_rng(5).integers(0, N_GROUPS + 1, ROWS)   # (id 3 is out of range)

    # everything is built before the first call, so that the six enqueues follow each other
    f_sels = [poisoned_selection(ctx), poisoned_selection(ctx)]
    f_batch = FilterBatch(ctx, [acp, bcp], [sb.Predicate(*a_pred), sb.Predicate(*b_pred)], out=f_sels)
    f_arr = fixed_filter_array(f_batch, [a, b], [a_pred, b_pred])
    v_sels = [poisoned_selection(ctx), poisoned_selection(ctx)]
    v_batch = FilterBatch(ctx, [acp, scp], [sb.Predicate(*a_pred), sb.Predicate(*s_pred)], out=v_sels)
    nums = [NumCase(ctx, a, ap, am, mask, oracle=(a_or[0].view(np.uint8).reshape(ROWS, 4), a_or[1])),
            NumCase(ctx, b, bp, bm, mask, oracle=(b_or[0].view(np.uint8).reshape(ROWS, 4), b_or[1]))]
    strs = [BinCase(ctx, s, sp, sm, mask, oracle=s_or), BinCase(ctx, t, tp, tm, mask, oracle=t_or)]
    r_batch = sb.ReadSelectedBatch(ctx, [c.cp for c in nums], [c.bitmap for c in nums], out=[c.out() for c in nums])
    rv_batch = sb.ReadSelectedVarBatch(ctx, [c.cp for c in strs], [c.bitmap for c in strs], out=[c.out() for c in strs])
    sel = bitmap(ctx, mask)
    agg_ops = [("min", "max", "sum"), ("count",)]
    g_batch = sb.AggregateBatch(ctx, [acp, bcp], sel)
    for i, ops in enumerate(agg_ops):
        g_batch._arr[i].ops = g_batch.results[i].ops = sum(R.OPS[o] for o in ops)
    gg_batch = sb.GroupedAggregateBatch(ctx, [acp, bcp], ids_dev(ctx, ids, 1), N_GROUPS, sel)
    for r in gg_batch.results:
        C.memset(r._groups, POISON, C.sizeof(r._groups))

    r0 = ctx.replays()
    ctx._keep.append((f_batch, f_arr))
    ctx._check(ctx._lib.sb_filter_columns(ctx._h, f_arr, 2, N.SB_MEM_DEVICE))
    v_batch.enqueue()
    r_arrs = r_batch.enqueue()
    rv_arrs = rv_batch.enqueue()
    g_res = g_batch.enqueue()
    gg_res = gg_batch.enqueue()
    ctx.synchronize()
    assert ctx.replays() == r0 + (1 if freq else 0)

    check_selection(f_sels[0].bitmap, f_arr[0], a_want, "sb_filter_columns column 0")
    check_selection(f_sels[1].bitmap, f_arr[1], b_want, "sb_filter_columns column 1")
    check_selection(v_sels[0].bitmap, v_batch._arr[0], a_want, "sb_filter_columns_var column 0")
    check_selection(v_sels[1].bitmap, v_batch._arr[1], s_want, "sb_filter_columns_var column 1 (Utf8)")
    for i, (c, arr) in enumerate(zip(nums, r_arrs)):
        c.check(arr, "sb_read_selected column %d" % i)
    for i, (c, arr) in enumerate(zip(strs, rv_arrs)):
        c.check(arr, "sb_read_selected_var column %d" % i)
    R.check(g_res[0], a_ref.want(mask, agg_ops[0]), "sb_aggregate_columns column 0 (min / max / sum)")
    R.check(g_res[1], b_ref.want(mask, agg_ops[1]), "sb_aggregate_columns column 1 (count only)")
    G.check(gg_res[0], G.want(a_ref, ids, N_GROUPS, mask), "sb_aggregate_grouped column 0")
    G.check(gg_res[1], G.want(b_ref, ids, N_GROUPS, mask), "sb_aggregate_grouped column 1")
    assert gg_res[0].out_of_range > 0
