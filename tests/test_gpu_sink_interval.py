"""Intervals in which the kinds of sink call meet.

test_one_call_of_all_twelve_sinks_in_one_interval adds the six later entry points (sb_filter_columns_in, sb_topk_columns,
sb_key_ids, sb_key_ids_var, sb_key_combine, sb_aggregate_grouped_large) to the six of the first test, again without a call
that depends on another; test_a_query_chain_in_one_interval is one query in which every step consumes what the step before
left on the device, with its one Freq column at every place a replay can start from.

The first test: one interval that holds one call of every sink entry point of its time, in this order: sb_filter_columns, sb_filter_columns_var,
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
from tests import key_combine_ref as KC
from tests import key_ids_ref as K
from tests import key_ids_var_ref as KV
from tests import topk_ref as T
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


# ---------------------------------------------------------------- all twelve kinds
N_GROUPS_LARGE = 300   # more than sb_aggregate_grouped takes
KEYS_CAPACITY = 4096


def poisoned(ctx, nbytes):
    import torch
    with torch.cuda.stream(ctx.torch_stream):   # (the fill is ordered before the call's kernels)
        return torch.full((int(nbytes),), POISON, dtype=torch.uint8, device=ctx.torch_device)


def poisoned_ids(ctx, rows, width=2):
    """exactly `rows` ids of `width` bytes, every byte POISON"""
    import torch
    return poisoned(ctx, rows * width).view({1: torch.uint8, 2: torch.uint16, 4: torch.int32}[width])


def poison_key_var_results(batch):
    """the host buffers of a KeyIdsVarBatch: the offsets and the keys' bytes"""
    for r in batch.results:
        r._offsets.view(np.uint8)[:] = POISON
        C.memset(r._keys, POISON, C.sizeof(r._keys))


def drawn_literals(vals, valid, n, seed):
    v = vals[valid]
    return [v[int(i)].item() for i in np.random.default_rng(seed).integers(0, v.size, n)]


@pytest.mark.parametrize("freq", [False, True])
def test_one_call_of_all_twelve_sinks_in_one_interval(gpu_ctx, freq):
    import strawboat_amd as sb
    from strawboat_amd import _native as N
    from strawboat_amd.filter import FilterBatch
    from strawboat_amd.filter_in import FilterInBatch
    from strawboat_amd.key_combine import KeyCombineBatch
    from strawboat_amd.key_ids import KeyIdsBatch
    from strawboat_amd.key_ids_var import KeyIdsVarBatch
    from strawboat_amd.aggregate_grouped_large import GroupedAggregateLargeBatch
    from strawboat_amd.topk import TopKBatch
    from tests.test_gpu_filter_in import want_in
    from tests.test_gpu_key_combine import part_dev
    ctx = gpu_ctx
    w = written(freq)
    (a, ap, am), (b, bp, bm), (s, sp, sm), (t, tp, tm) = w["a"], w["b"], w["s"], w["t"]
    a_or, b_or = num_oracle(a, ap, am), num_oracle(b, bp, bm)
    s_or, t_or = oracle_strings(s, sp, sm), oracle_strings(t, tp, tm)
    a_pred, b_pred = ("le", median(a)), ("gt", median(b))
    s_pred = ("lt", sorted(set(strings_of(s)))[30])
    a_want, b_want = num_expected(a, *a_or, *a_pred), num_expected(b, *b_or, *b_pred)
    s_want = bin_expected(*s_or, *s_pred)
    mask = a_want
    acp, bcp, scp, tcp = upload(ctx, a, ap, am), upload(ctx, b, bp, bm), upload(ctx, s, sp, sm), upload(ctx, t, tp, tm)
    a_ref, b_ref = R.Ref(a, ap, am), R.Ref(b, bp, bm)
    s_ref, t_ref = KV.Ref(s, sp, sm), KV.Ref(t, tp, tm)
    rng = np.random.default_rng(5)
    ids = rng.integers(0, N_GROUPS + 1, ROWS)                 # (id 3 is out of range)
    ids_large = rng.integers(0, N_GROUPS_LARGE + 1, ROWS)     # (id 300 is out of range)
    a_lits, b_lits = drawn_literals(*a_or, 8, 6), drawn_literals(*b_or, 8, 7)
    in_wants = [want_in(a, *a_or, a_lits, False), want_in(b, *b_or, b_lits, True)]
    key_wants = [K.want(a_ref, mask, 256, 2), K.want(b_ref, mask, 256, 2)]
    keyv_wants = [KV.want(s_ref, mask, 256, 2, KEYS_CAPACITY), KV.want(t_ref, mask, 256, 2, KEYS_CAPACITY)]
    assert not any(k.overflow for k in key_wants + keyv_wants)
    # sb_key_combine runs over id arrays uploaded from the reference: it depends on no other call of the interval
    comb_parts = [([key_wants[0].ids, keyv_wants[0].ids], [key_wants[0].n_keys, keyv_wants[0].n_keys]),
                  ([key_wants[1].ids, keyv_wants[1].ids], [key_wants[1].n_keys, keyv_wants[1].n_keys])]
    comb_wants = [KC.combine(parts, bounds, 1024, 2) for parts, bounds in comb_parts]
    assert not any(c.overflow for c in comb_wants) and all(0 < c.live < ROWS for c in comb_wants)

    # everything is built before the first call, so that the twelve enqueues follow each other
    f_sels = [poisoned_selection(ctx), poisoned_selection(ctx)]
    f_batch = FilterBatch(ctx, [acp, bcp], [sb.Predicate(*a_pred), sb.Predicate(*b_pred)], out=f_sels)
    f_arr = fixed_filter_array(f_batch, [a, b], [a_pred, b_pred])
    v_sels = [poisoned_selection(ctx), poisoned_selection(ctx)]
    v_batch = FilterBatch(ctx, [acp, scp], [sb.Predicate(*a_pred), sb.Predicate(*s_pred)], out=v_sels)
    i_sels = [poisoned_selection(ctx), poisoned_selection(ctx)]
    i_batch = FilterInBatch(ctx, [acp, bcp], [sb.InList(a_lits), sb.InList(b_lits, negate=True)], out=i_sels)
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
    gl_batch = GroupedAggregateLargeBatch(ctx, [acp, bcp], ids_dev(ctx, ids_large, 2), N_GROUPS_LARGE, sel)
    for r in gg_batch.results + gl_batch.results:
        C.memset(r._groups, POISON, C.sizeof(r._groups))
    t_batch = TopKBatch(ctx, [acp, bcp], [16, 7], [False, True], sel)
    for r in t_batch.results:
        C.memset(r._out, POISON, C.sizeof(r._out))
    k_ids = [poisoned_ids(ctx, ROWS), poisoned_ids(ctx, ROWS)]
    k_batch = KeyIdsBatch(ctx, [acp, bcp], sel, 256, 2, out=k_ids)
    for r in k_batch.results:
        C.memset(r._keys, POISON, C.sizeof(r._keys))
    kv_ids = [poisoned_ids(ctx, ROWS), poisoned_ids(ctx, ROWS)]
    kv_batch = KeyIdsVarBatch(ctx, [scp, tcp], sel, 256, 2, KEYS_CAPACITY, out=kv_ids)
    poison_key_var_results(kv_batch)
    c_ids = [poisoned_ids(ctx, ROWS), poisoned_ids(ctx, ROWS)]
    c_batch = KeyCombineBatch(ctx, [[(part_dev(ctx, p), n) for p, n in zip(parts, bounds)] for parts, bounds in comb_parts], 1024, 2, out=c_ids)
    for r in c_batch.results:
        r._tuples.view(np.uint8)[:] = POISON

    r0 = ctx.replays()
    ctx._keep.append((f_batch, f_arr))
    ctx._check(ctx._lib.sb_filter_columns(ctx._h, f_arr, 2, N.SB_MEM_DEVICE))
    v_batch.enqueue()
    i_batch.enqueue()
    r_arrs = r_batch.enqueue()
    rv_arrs = rv_batch.enqueue()
    g_res = g_batch.enqueue()
    gg_res = gg_batch.enqueue()
    gl_res = gl_batch.enqueue()
    t_res = t_batch.enqueue()
    k_res = k_batch.enqueue()
    kv_res = kv_batch.enqueue()
    c_res = c_batch.enqueue()
    ctx.synchronize()
    assert ctx.replays() == r0 + (1 if freq else 0)

    check_selection(f_sels[0].bitmap, f_arr[0], a_want, "sb_filter_columns column 0")
    check_selection(f_sels[1].bitmap, f_arr[1], b_want, "sb_filter_columns column 1")
    check_selection(v_sels[0].bitmap, v_batch._arr[0], a_want, "sb_filter_columns_var column 0")
    check_selection(v_sels[1].bitmap, v_batch._arr[1], s_want, "sb_filter_columns_var column 1 (Utf8)")
    check_selection(i_sels[0].bitmap, i_batch._arr[0], in_wants[0], "sb_filter_columns_in column 0 (IN)")
    check_selection(i_sels[1].bitmap, i_batch._arr[1], in_wants[1], "sb_filter_columns_in column 1 (NOT IN)")
    for i, (c, arr) in enumerate(zip(nums, r_arrs)):
        c.check(arr, "sb_read_selected column %d" % i)
    for i, (c, arr) in enumerate(zip(strs, rv_arrs)):
        c.check(arr, "sb_read_selected_var column %d" % i)
    R.check(g_res[0], a_ref.want(mask, agg_ops[0]), "sb_aggregate_columns column 0 (min / max / sum)")
    R.check(g_res[1], b_ref.want(mask, agg_ops[1]), "sb_aggregate_columns column 1 (count only)")
    G.check(gg_res[0], G.want(a_ref, ids, N_GROUPS, mask), "sb_aggregate_grouped column 0")
    G.check(gg_res[1], G.want(b_ref, ids, N_GROUPS, mask), "sb_aggregate_grouped column 1")
    assert gg_res[0].out_of_range > 0
    G.check(gl_res[0], G.want(a_ref, ids_large, N_GROUPS_LARGE, mask), "sb_aggregate_grouped_large column 0")
    G.check(gl_res[1], G.want(b_ref, ids_large, N_GROUPS_LARGE, mask), "sb_aggregate_grouped_large column 1")
    assert gl_res[0].out_of_range > 0 and len(gl_res[0].groups) == N_GROUPS_LARGE > 256
    T.check(t_res[0], T.want(a_ref, mask, 16, False), "sb_topk_columns column 0 (smallest 16)")
    T.check(t_res[1], T.want(b_ref, mask, 7, True), "sb_topk_columns column 1 (largest 7)")
    for i in range(2):
        K.check(k_res[i], key_wants[i], "sb_key_ids column %d" % i)
        KV.check(kv_res[i], keyv_wants[i], "sb_key_ids_var column %d" % i)
        KC.check(c_res[i], comb_wants[i], "sb_key_combine item %d" % i)


# ---------------------------------------------------------------- a query chain
# SELECT k, u, count / min / max / sum of v and y ... WHERE f <= 800 AND g IN (...) GROUP BY k, u -- and the top 16 of p and
# the rows of r and u under the same WHERE -- in one interval: every step consumes what the step before left on the device.
FREQ_AT = ("nowhere", "f", "k", "v", "p")   # the column written as Freq pages: none, the first filter's, the integer key, the Int32 value, the top-k


@functools.lru_cache(maxsize=None)
def chain_columns():
    """{name: col}: f, k, v and p hold sparse values, which Freq and Dict pages both take"""
    from tests.test_gpu_freq import sparse
    half = (ROWS + 1) // 2
    y = np.repeat(G.inexact_values(half, 1, 3)[0][:half], 2)[:ROWS]   # (runs of two, so that Dict pages can hold it)
    rng = np.random.default_rng(17)
    return dict(f=sparse(S.T_I32, ROWS, 0.08, 21, null_density=0.1, exc_uniq=1 << 10),
                g=gen.prim(S.T_I32, ROWS, uniq=100, null_density=0.1, seed=22),
                k=sparse(S.T_I32, ROWS, 0.3, 23, null_density=0.1, exc_uniq=12),
                u=gen.binary(ROWS, uniq=9, null_density=0.1, seed=24, maxlen=20),
                v=sparse(S.T_I32, ROWS, 0.08, 25, null_density=0.1, exc_uniq=1 << 16),
                y=dict(ptype=S.T_F64, nullable=True, rows=ROWS, values=y, validity=gen.make_validity(rng, ROWS, 0.1), offsets=None),
                p=sparse(S.T_I32, ROWS, 0.08, 26, null_density=0.1, exc_uniq=1 << 16),
                r=gen.prim(S.T_I32, ROWS, uniq=100, null_density=0.2, seed=27))


@functools.lru_cache(maxsize=None)
def chain_written(name, freq):
    col = chain_columns()[name]
    codec = S.FREQ if freq else S.DICT
    pages, metas = gen.oracle_write(col, max_page_size=PAGE_ROWS, force_codec=codec)
    assert [int(n) for n in metas[:, 1]] == [PAGE_ROWS, ROWS - PAGE_ROWS]
    seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
    assert (S.FREQ in seen) if freq else (seen == {S.DICT}), (name, seen)
    return col, pages, metas


F_PRED = ("le", 800)
G_LIST = list(range(60))
CHAIN_KEYS, CHAIN_GROUPS, CHAIN_K = 256, 1024, 16


@functools.lru_cache(maxsize=None)
def chain_reference():
    """the same numpy chain for every place of the Freq column: the Dict pages' decode (the Freq pages hold the same values)"""
    from tests.test_gpu_filter_in import want_in
    w = {name: chain_written(name, False) for name in chain_columns()}
    f_or, g_or = num_oracle(*w["f"]), num_oracle(*w["g"])
    m1 = num_expected(w["f"][0], *f_or, *F_PRED)
    mask = m1 & want_in(w["g"][0], *g_or, G_LIST, False)
    assert 0 < mask.sum() < m1.sum() < ROWS
    refs = {name: R.Ref(*w[name]) for name in ("k", "v", "y", "p", "r")}
    u_ref = KV.Ref(*w["u"])
    kid = K.want(refs["k"], mask, CHAIN_KEYS, 2)
    uid = KV.want(u_ref, mask, CHAIN_KEYS, 2, KEYS_CAPACITY)
    comb = KC.combine([kid.ids, uid.ids], [CHAIN_KEYS, CHAIN_KEYS], CHAIN_GROUPS, 2)
    assert not (kid.overflow or uid.overflow or comb.overflow) and comb.n_keys > 20
    ids = comb.ids   # (all ones where a key is null or the row is not selected: out of range)
    return dict(m1=m1, mask=mask, kid=kid, uid=uid, comb=comb, v=G.want(refs["v"], ids, CHAIN_GROUPS, mask),
                y=G.want(refs["y"], ids, CHAIN_GROUPS, mask), p=T.want(refs["p"], mask, CHAIN_K, True), refs=refs,
                r_oracle=num_oracle(*w["r"]), u_oracle=oracle_strings(*w["u"]))


def run_chain(ctx, freq_at):
    """the interval with the Freq column at `freq_at`; returns the snapshot of every result"""
    import strawboat_amd as sb
    want = chain_reference()
    mask = want["mask"]
    w = {name: chain_written(name, name == freq_at) for name in chain_columns()}
    cp = {name: upload(ctx, *w[name]) for name in w}
    r_case = NumCase(ctx, *w["r"], mask, oracle=(want["r_oracle"][0].view(np.uint8).reshape(ROWS, 4), want["r_oracle"][1]))
    u_case = BinCase(ctx, *w["u"], mask, oracle=want["u_oracle"], cp=cp["u"])
    r0 = ctx.replays()
    # 1, 2: the WHERE clause
    sel = sb.filter_columns(ctx, [cp["f"]], [sb.Predicate(*F_PRED)], out=[poisoned_selection(ctx)])
    sel2 = sb.filter_in(ctx, [cp["g"]], [sb.InList(G_LIST)], combine="and", out=sel)
    # 3, 4: the keys' ids, and the ids of their pairs
    kid, = sb.key_ids(ctx, [cp["k"]], sel[0], max_keys=CHAIN_KEYS, id_width=2, out=[poisoned_ids(ctx, ROWS)])
    uid, = sb.key_ids_var(ctx, [cp["u"]], sel[0], max_keys=CHAIN_KEYS, id_width=2, key_bytes=KEYS_CAPACITY, out=[poisoned_ids(ctx, ROWS)])
    comb = sb.key_combine(ctx, [kid, uid], max_keys=CHAIN_GROUPS, id_width=2, out=poisoned_ids(ctx, ROWS))
    # 5: GROUP BY the pairs
    v_res, y_res = sb.aggregate_grouped_large(ctx, [cp["v"], cp["y"]], comb.ids, CHAIN_GROUPS, sel[0])
    # 6, 7: ORDER BY p DESC LIMIT 16, and the rows of r and u
    top, = sb.topk_columns(ctx, [cp["p"]], CHAIN_K, True, sel[0])
    r_arr, = sb.read_selected(ctx, [cp["r"]], sel[0], out=[r_case.out()])
    u_arr, = sb.read_selected_var(ctx, [cp["u"]], sel[0], out=[u_case.out()])
    ctx.synchronize()
    assert ctx.replays() == r0 + (0 if freq_at == "nowhere" else 1), "Freq column at %s: %d replays" % (freq_at, ctx.replays() - r0)

    got = np.unpackbits(sel[0].bitmap.cpu().numpy(), bitorder="little").astype(bool)
    assert np.array_equal(got[:ROWS], mask) and not got[ROWS:].any(), "the bitmap behind the two filter calls"
    assert sel[0].selected == int(want["m1"].sum()) and sel2[0].selected == int(mask.sum())
    K.check(kid, want["kid"], "key_ids")
    KV.check(uid, want["uid"], "key_ids_var")
    KC.check(comb, want["comb"], "key_combine")
    G.check(v_res, want["v"], "aggregate_grouped_large, Int32")
    G.check(y_res, want["y"], "aggregate_grouped_large, Float64")
    T.check(top, want["p"], "topk")
    # (an interval that is issued again ran the reads twice, the first time under the bitmap its first pass left: only the
    # capacity bounds what that wrote behind the result)
    replayed = freq_at != "nowhere"
    nsel = int(mask.sum())
    if replayed:
        assert (r_arr.rows, r_arr.selected, r_arr.values_len) == (ROWS, nsel, 4 * nsel)
    else:
        r_case.check(r_arr, "read_selected")
    u_case.check(u_arr, "read_selected_var", replayed=replayed)
    r_vals, r_valid = r_arr.numpy()
    assert np.array_equal(r_valid, want["refs"]["r"].valid[mask]) and np.array_equal(r_vals.view(np.uint8), want["r_oracle"][0][mask].view(np.uint8))
    u_offs, u_vals, u_bits = u_arr.numpy()
    groups = lambda res: (res.rows, res.selected, res.out_of_range, bytes(res._groups))
    return dict(bitmap=sel[0].bitmap.cpu().numpy().tobytes(), selected=(sel[0].selected, sel2[0].selected),
                key_ids=(kid.rows, kid.selected, kid.count, kid.n_keys, kid.overflow, kid.key_bytes, kid.ids.cpu().numpy().tobytes()),
                key_ids_var=(uid.rows, uid.selected, uid.count, uid.n_keys, uid.keys_len, uid.overflow, uid.key_offsets.tobytes(), uid.key_bytes,
                             uid.ids.cpu().numpy().tobytes()),
                key_combine=(comb.rows, comb.live, comb.n_keys, comb.overflow, comb.tuple_words.tobytes(), comb.ids.cpu().numpy().tobytes()),
                grouped_v=groups(v_res), grouped_y=groups(y_res),
                topk=(top.rows, top.selected, top.count, top.nans, top.found, top.out_bytes),
                read_selected=(r_arr.rows, r_arr.selected, r_arr.values_len, r_vals.tobytes(), np.packbits(r_valid, bitorder="little").tobytes(),
                               r_arr.validity_buf[:(nsel + 31) // 32 * 4].cpu().numpy().tobytes()),
                read_selected_var=(u_arr.rows, u_arr.selected, u_arr.values_len, u_offs.tobytes(), u_vals.tobytes(), u_bits.tobytes()))


_chain_snapshots = {}


def chain_snapshot(ctx, freq_at):
    if freq_at not in _chain_snapshots:
        _chain_snapshots[freq_at] = run_chain(ctx, freq_at)
    return _chain_snapshots[freq_at]


@pytest.mark.parametrize("freq_at", FREQ_AT)
def test_a_query_chain_in_one_interval(gpu_ctx, freq_at):
    """the chain matches the numpy chain, and its complete result -- the float sums of the groups included -- is the same
    byte for byte wherever the Freq column sits (each place is compared with the interval that holds none)"""
    base = chain_snapshot(gpu_ctx, "nowhere")
    snap = chain_snapshot(gpu_ctx, freq_at)
    assert list(snap) == list(base)
    for field in base:
        assert snap[field] == base[field], "Freq column at %s: %s differs from the interval without a Freq column" % (freq_at, field)
