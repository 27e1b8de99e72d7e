"""sb_filter_columns_cmp on the GPU: the selection bitmap of `y op other`, compared WORD FOR WORD, with rows / selected,
against tests/filter_cmp_ref.py over the ORACLE's decode of the pages (the reference is checked on its own against a plain
Python loop in tests/test_filter_cmp_host.py).  Nothing here is compared with what the device's own decoder gives.

Every column comes from tests/filter_cmp_cases.py (the codec of every page is asserted there; the host test walks the
table).  Unless a test says otherwise a call has one column per op, all six over the same pages; SET is written onto a
bitmap of all ones, so the zero bits behind `rows` are part of every comparison, and AND / OR onto seeded words, whose bits
behind `rows` must stay.  Null rows keep their stored bytes in the pages, and the slots of invalid operands hold garbage
(NaN bit patterns for floats)."""
import numpy as np
import pytest

from oracle import sbo as S
from tests import filter_cmp_cases as Cc
from tests import filter_cmp_ref as R
from tests.test_gpu_read_selected import oracle_code, read_code, to_dev, upload

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_BYTES = 4096
WORD = 0x5A5A5A5A5A5A5A5A
NP = Cc.NP


def y_of(b):
    return b.ref.vals[:b.rows], (b.ref.valid if b.col["nullable"] else None)


def sel_bytes(rows):
    return (rows + 31) // 32 * 4


def seeded_words(rows, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, (rows + 31) // 32, dtype=np.uint64).astype(np.uint32)


def selection_of(ctx, rows, words):
    from strawboat_amd.filter import Selection
    return Selection(to_dev(ctx, np.ascontiguousarray(words, np.uint32).view(np.uint8)), rows, None)


def run(ctx, b, ops, others, valids=None, combine="set", prev=None, cp=None, what=""):
    """ONE call of len(ops) columns over the pages of `b`: column i is `y ops[i] others[i]` under valids[i] (a bool per
    row or None).  prev: the words the bitmaps hold before the call (None: all ones)."""
    import strawboat_amd as sb
    n = len(ops)
    others = [others] * n if isinstance(others, np.ndarray) else list(others)
    valids = [valids] * n if valids is None or isinstance(valids, np.ndarray) else list(valids)
    cp = upload(ctx, b.col, b.pages, b.metas) if cp is None else cp
    nwords = (b.rows + 31) // 32
    prevs = [np.full(nwords, 0xFFFFFFFF, np.uint32) if prev is None else prev for _ in range(n)]
    outs = [selection_of(ctx, b.rows, p) for p in prevs]
    devs = [(to_dev(ctx, o), None if v is None else to_dev(ctx, Cc.gen.pack_bits(np.concatenate([v, np.ones((-v.size) % 32, bool)]))))
            for o, v in zip(others, valids)]
    sels = sb.filter_columns_cmp(ctx, [cp] * n, list(ops), [d if d[1] is not None else d[0] for d in devs], combine=combine, selection=outs)
    ctx.synchronize()
    y, y_valid = y_of(b)
    for i, s in enumerate(sels):
        words, selected = R.want(y, y_valid, others[i], valids[i], ops[i], combine, prevs[i])
        R.check(s, words, selected, b.rows, "%s, %s %s, column %d" % (what, ops[i], combine, i))
        # the operand and its validity are inputs: unchanged
        assert devs[i][0].cpu().numpy().tobytes() == np.ascontiguousarray(others[i]).tobytes(), what
    return sels


def operands(b, ot, seed=1):
    """(other, other_valid) of type ot for a built column: about half the rows equal, a fifth of the operands invalid with
    garbage in their slots"""
    other = Cc.operand_for(b, ot, seed)
    valid = np.random.default_rng(seed).random(b.rows) >= 0.2
    return Cc.garbage_where_invalid(other, valid, seed), valid


def mixed_type(ptype):
    return S.T_F64 if np.dtype(NP[ptype]).kind in "iu" else S.T_I64


def six_ops_both_operands(ctx, name, b=None):
    b = Cc.build(name) if b is None else b
    cp = upload(ctx, b.col, b.pages, b.metas)
    o, v = operands(b, b.col["ptype"])
    run(ctx, b, R.OPS, o, v, cp=cp, what=name + ", same type")
    o, v = operands(b, mixed_type(b.col["ptype"]), 2)
    run(ctx, b, R.OPS, o, None, cp=cp, what=name + ", mixed types")


# ---- 1: the codec routes of y
@pytest.mark.parametrize("name", list(Cc.ROUTES))
def test_codec_routes(gpu_ctx, name):
    six_ops_both_operands(gpu_ctx, name)


@pytest.mark.parametrize("name", list(Cc.FREQ))
def test_freq_pages_take_the_replay_and_give_the_same_bits_twice(gpu_ctx, name):
    import strawboat_amd as sb
    b, plain = Cc.build(name), Cc.build(Cc.FREQ_PLAIN[name])
    # (the same column written twice: the live rows hold the same values, the slots of null rows what each codec leaves there)
    assert b.rows == plain.rows and np.array_equal(b.ref.valid, plain.ref.valid)
    assert b.ref.vals[:b.rows][b.ref.valid].tobytes() == plain.ref.vals[:b.rows][b.ref.valid].tobytes()
    cp = upload(gpu_ctx, b.col, b.pages, b.metas)
    o, v = operands(b, b.col["ptype"])
    before = gpu_ctx.replays()
    first = run(gpu_ctx, b, R.OPS, o, v, cp=cp, what=name)
    assert gpu_ctx.replays() == before + 1, "a primitive Freq page asks for the replay"
    again = run(gpu_ctx, b, R.OPS, o, v, cp=cp, what=name + ", again")
    for s, t in zip(first, again):
        assert s.bitmap.cpu().numpy().tobytes() == t.bitmap.cpu().numpy().tobytes() and s.selected == t.selected
    # the same bits as the plain pages of the same values, in the three modes
    prev = seeded_words(b.rows, 3)
    for combine in R.COMBINES:
        f = run(gpu_ctx, b, R.OPS, o, v, combine, prev, cp=cp, what=name)
        p = run(gpu_ctx, plain, R.OPS, o, v, combine, prev, what=name + " as plain pages")
        for s, t in zip(f, p):
            assert s.bitmap.cpu().numpy().tobytes() == t.bitmap.cpu().numpy().tobytes() and s.selected == t.selected
    # a Freq column and a column without one in ONE call: both through the replay
    other = Cc.build("route_rle")
    oo, ov = operands(other, S.T_I32, 4)
    sels = sb.filter_columns_cmp(gpu_ctx, [cp, upload(gpu_ctx, other.col, other.pages, other.metas)], ["le", "gt"],
                                 [(to_dev(gpu_ctx, o), to_dev(gpu_ctx, bits_of(v))), (to_dev(gpu_ctx, oo), to_dev(gpu_ctx, bits_of(ov)))])
    gpu_ctx.synchronize()
    for s, bb, op, x, xv in ((sels[0], b, "le", o, v), (sels[1], other, "gt", oo, ov)):
        yy, yv = y_of(bb)
        R.check(s, *R.want(yy, yv, x, xv, op), bb.rows, name + " beside route_rle")


def bits_of(valid):
    return Cc.gen.pack_bits(np.concatenate([valid, np.ones((-valid.size) % 32, bool)]))


# ---- 2: row counts, page seams, chunk seams
@pytest.mark.parametrize("rows", Cc.ROW_COUNTS)
def test_row_counts(gpu_ctx, rows):
    for c in ("none", "rle", "dict"):
        six_ops_both_operands(gpu_ctx, "rows_%d_%s" % (rows, c))


@pytest.mark.parametrize("codec", ["none", "rle", "dict", "lz4"])
def test_pages_that_share_selection_words_at_their_seams(gpu_ctx, codec):
    b = Cc.build("seams_" + codec)
    o, v = operands(b, S.T_I16)
    prev = seeded_words(b.rows, 11)
    for combine in R.COMBINES:
        run(gpu_ctx, b, R.OPS, o, v, combine, prev, what="seams_" + codec)


def test_a_column_without_pages_beside_one_with_pages(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    b = Cc.build("rows_33_rle")
    o, v = operands(b, S.T_I64, 21)
    empty = read.ColumnPages(S.T_I32, True, torch.zeros(0, dtype=torch.uint8, device=gpu_ctx.torch_device), np.zeros((0, 2), np.uint64))
    none = torch.zeros(0, dtype=torch.float32, device=gpu_ctx.torch_device)
    sels = sb.filter_columns_cmp(gpu_ctx, [empty, upload(gpu_ctx, b.col, b.pages, b.metas), empty], ["ne", "ge", "eq"],
                                 [none, (to_dev(gpu_ctx, o), to_dev(gpu_ctx, bits_of(v))), none])
    gpu_ctx.synchronize()
    assert (sels[0].rows, sels[0].selected, sels[2].rows, sels[2].selected) == (0, 0, 0, 0)
    R.check(sels[1], *R.want(*y_of(b), o, v, "ge"), b.rows, "between two columns without pages")
    only = sb.filter_columns_cmp(gpu_ctx, [empty], ["lt"], [none])
    gpu_ctx.synchronize()
    assert (only[0].rows, only[0].selected) == (0, 0)


# ---- 3: type pairs on the edge values, all six ops, and a seeded column per pair
@pytest.mark.parametrize("yt,ot", Cc.PAIRS, ids=["%s_%s" % (Cc.TYPE_NAME[a], Cc.TYPE_NAME[b]) for a, b in Cc.PAIRS])
def test_type_pairs_on_the_edge_values(gpu_ctx, yt, ot):
    for codec in (S.NONE, S.RLE, S.DICT):
        b, other = Cc.build_edge_pair(yt, ot, codec)
        what = "edges %s vs %s, %s" % (Cc.TYPE_NAME[yt], Cc.TYPE_NAME[ot], Cc.CODEC_NAME[codec])
        run(gpu_ctx, b, R.OPS, other, None, what=what)
        valid = np.arange(b.rows) % 3 != 1
        run(gpu_ctx, b, R.OPS, Cc.garbage_where_invalid(other, valid, yt + ot), valid, what=what + ", operand validity")


@pytest.mark.parametrize("yt,ot", Cc.PAIRS, ids=["%s_%s" % (Cc.TYPE_NAME[a], Cc.TYPE_NAME[b]) for a, b in Cc.PAIRS])
def test_type_pairs_on_a_seeded_column_half_of_whose_rows_are_equal(gpu_ctx, yt, ot):
    for codec in (S.NONE, S.RLE, S.DICT, S.ZSTD):
        b, other = Cc.build_random_pair(yt, ot, codec)
        sels = run(gpu_ctx, b, R.OPS, other, None, what="seeded %s vs %s, %s" % (Cc.TYPE_NAME[yt], Cc.TYPE_NAME[ot], Cc.CODEC_NAME[codec]))
        live = int(b.ref.valid.sum())
        assert 0.4 * live < sels[0].selected < 0.6 * live   # "eq"


# ---- 4: nulls
@pytest.mark.parametrize("codec", ["none", "rle", "dict"])
def test_the_four_combinations_of_nulls(gpu_ctx, codec):
    for name in ("nonnull_" + codec, "nullable_" + codec):
        b = Cc.build(name)
        y, y_valid = y_of(b)
        assert (y_valid is None) == name.startswith("nonnull")
        for ot in (S.T_I32, S.T_F32):
            other = Cc.operand_for(b, ot, 5)
            for with_validity in (False, True):
                valid = np.random.default_rng(6).random(b.rows) >= 0.3 if with_validity else None
                o = Cc.garbage_where_invalid(other, valid, 7) if with_validity else other
                sels = run(gpu_ctx, b, R.OPS, o, valid, what="%s, operand validity %r" % (name, with_validity))
                ne = sels[1].numpy()
                dead = np.zeros(b.rows, bool)
                if y_valid is not None:
                    dead |= ~y_valid
                if valid is not None:
                    dead |= ~valid
                assert not ne[dead].any(), "NE selected a null row"
                assert ne[~dead].any()


def test_operand_validity_bits_behind_rows_are_ignored(gpu_ctx):
    import strawboat_amd as sb
    b = Cc.build("rows_33_none")
    other = Cc.operand_for(b, S.T_I32, 1)
    valid = np.arange(33) % 2 == 0
    y, y_valid = y_of(b)
    for tail in (False, True):
        bits = Cc.gen.pack_bits(np.concatenate([valid, np.full(31, tail)]))
        sels = sb.filter_columns_cmp(gpu_ctx, [upload(gpu_ctx, b.col, b.pages, b.metas)], ["ge"], [(to_dev(gpu_ctx, other), to_dev(gpu_ctx, bits))])
        gpu_ctx.synchronize()
        R.check(sels[0], *R.want(y, y_valid, other, valid, "ge"), 33, "tail bits %r" % tail)


# ---- 5: combine modes
@pytest.mark.parametrize("name", ["rows_1_none", "rows_33_rle", "rows_4097_dict", "route_lz4", "route_bitpack_i32", "f64_patas"])
def test_combine_modes(gpu_ctx, name):
    b = Cc.build(name)
    o, v = operands(b, b.col["ptype"], 8)
    nwords = (b.rows + 31) // 32
    sels = run(gpu_ctx, b, R.OPS, o, v, "set", None, what=name)   # onto all ones
    if b.rows % 32:
        for s in sels:
            last = int(s.bitmap.cpu().numpy().view("<u4")[nwords - 1])
            assert last >> (b.rows % 32) == 0, "bits behind rows after SET"
    prev = seeded_words(b.rows, 9)
    for combine in ("and", "or"):
        sels = run(gpu_ctx, b, R.OPS, o, v, combine, prev, what=name)
        if b.rows % 32:
            for s in sels:
                last = int(s.bitmap.cpu().numpy().view("<u4")[nwords - 1])
                assert last >> (b.rows % 32) == int(prev[-1]) >> (b.rows % 32), "bits behind rows changed by %s" % combine


# ---- 6: where the bytes land
def test_buffers_of_exactly_their_size_between_guards(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd.filter import Selection
    for name in ("route_none", "route_rle", "route_dict", "route_lz4", "rows_4097_rle", "rows_1025_none", "seams_dict", "route_freq_i32"):
        b = Cc.build(name)
        y, y_valid = y_of(b)
        cp = upload(gpu_ctx, b.col, b.pages, b.metas)
        for ot in (S.T_I8, S.T_I64):
            o, v = operands(b, ot, 10)
            w = o.dtype.itemsize
            nsel, nother = sel_bytes(b.rows), b.rows * w
            # selection: guard | bitmap | guard.  other and other_validity: their bytes end where a guard begins
            host = np.full(2 * GUARD_BYTES + nsel, GUARD, np.uint8)
            host[GUARD_BYTES:GUARD_BYTES + nsel] = 0xFF
            sel_whole = to_dev(gpu_ctx, host)
            pad = (-nother) % 8
            host_o = np.full(pad + nother + GUARD_BYTES, GUARD, np.uint8)
            host_o[pad:pad + nother] = o.view(np.uint8)
            o_whole = to_dev(gpu_ctx, host_o)
            host_v = np.full(nsel + GUARD_BYTES, GUARD, np.uint8)
            host_v[:nsel] = bits_of(v)
            v_whole = to_dev(gpu_ctx, host_v)
            o_t = o_whole[pad:pad + nother].view(getattr(torch, np.dtype(o.dtype).name))
            for combine in R.COMBINES:
                prev = np.full((b.rows + 31) // 32, 0xFFFFFFFF, np.uint32)
                sel_whole[GUARD_BYTES:GUARD_BYTES + nsel] = 0xFF
                torch.cuda.synchronize()
                out = Selection(sel_whole[GUARD_BYTES:GUARD_BYTES + nsel], b.rows, None)
                batch = sb.FilterCmpBatch(gpu_ctx, [cp], ["lt"], [(o_t, v_whole[:nsel])], combine=combine, out=[out])
                c = batch._arr[0]
                assert (c.selection_capacity, c.other_capacity, c.other_validity_capacity) == (nsel, nother, nsel)
                res = batch.enqueue()
                gpu_ctx.synchronize()
                R.check(res[0], *R.want(y, y_valid, o, v, "lt", combine, prev), b.rows, "%s between guards, %s" % (name, combine))
                h = sel_whole.cpu().numpy()
                assert (h[:GUARD_BYTES] == GUARD).all() and (h[GUARD_BYTES + nsel:] == GUARD).all(), "a byte outside selection was written"
                assert o_whole.cpu().numpy().tobytes() == host_o.tobytes() and v_whole.cpu().numpy().tobytes() == host_v.tobytes()


def test_pages_at_odd_byte_offsets_and_scattered_page_offsets(gpu_ctx):
    import torch
    from strawboat_amd import read
    for name in ("route_none", "route_rle", "route_dict", "route_lz4", "f64_patas", "seams_rle"):
        b = Cc.build(name)
        col, pages, metas = b.col, b.pages, b.metas
        o, v = operands(b, col["ptype"], 12)
        for off in (1, 3, 7):
            buf = torch.zeros(off + pages.size, dtype=torch.uint8, device=gpu_ctx.torch_device)
            buf[off:] = torch.from_numpy(np.ascontiguousarray(pages)).to(gpu_ctx.torch_device)
            torch.cuda.synchronize()
            run(gpu_ctx, b, R.OPS, o, v, cp=read.ColumnPages(col["ptype"], col["nullable"], buf[off:], metas), what="%s at offset %d" % (name, off))
        # the pages in descending order in the buffer, with gaps of odd lengths between them
        lens = [int(x) for x in metas[:, 0]]
        starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
        offs, at = [0] * len(lens), 5
        for p in range(len(lens) - 1, -1, -1):
            offs[p] = at
            at += lens[p] + 3 + 2 * p
        buf = np.full(at, 0xEE, np.uint8)
        for p in range(len(lens)):
            buf[offs[p]:offs[p] + lens[p]] = pages[starts[p]:starts[p] + lens[p]]
        cp = read.ColumnPages(col["ptype"], col["nullable"], to_dev(gpu_ctx, buf), metas, page_offsets=np.array(offs, np.uint64))
        run(gpu_ctx, b, R.OPS, o, v, cp=cp, what=name + ", page_offsets")


# ---- 7: the interval
@pytest.mark.parametrize("left,right", [("nullable_none", "nonnull_rle"), ("nullable_dict", "nullable_rle"), ("nonnull_rle", "nullable_none"),
                                        ("route_rle", "route_zstd"), ("route_dict", "f64_patas"), ("f64_rle", "route_lz4")])
def test_filter_pair_decodes_right_and_compares_left_in_one_interval(gpu_ctx, left, right):
    import strawboat_amd as sb
    lb, rb = Cc.build(left), Cc.build(right)
    assert lb.rows == rb.rows
    lcp, rcp = upload(gpu_ctx, lb.col, lb.pages, lb.metas), upload(gpu_ctx, rb.col, rb.pages, rb.metas)
    y, y_valid = y_of(lb)
    o, o_valid = y_of(rb)
    for op in R.OPS:
        sel = sb.filter_pair(gpu_ctx, lcp, op, rcp)
        gpu_ctx.synchronize()
        R.check(sel, *R.want(y, y_valid, o, o_valid, op), lb.rows, "%s %s %s" % (left, op, right))
    prev = seeded_words(lb.rows, 13)
    for combine in ("and", "or"):
        sel = sb.filter_pair(gpu_ctx, lcp, "le", rcp, combine=combine, selection=selection_of(gpu_ctx, lb.rows, prev))
        gpu_ctx.synchronize()
        R.check(sel, *R.want(y, y_valid, o, o_valid, "le", combine, prev), lb.rows, "%s le %s, %s" % (left, right, combine))


def test_filter_pair_whose_left_column_has_freq_pages(gpu_ctx):
    """the replay issues the read of `right` and the comparison again, in their places"""
    import strawboat_amd as sb
    lb, rb = Cc.build("route_freq_i64"), Cc.build("route_lz4")
    assert lb.rows == rb.rows
    lcp, rcp = upload(gpu_ctx, lb.col, lb.pages, lb.metas), upload(gpu_ctx, rb.col, rb.pages, rb.metas)
    y, y_valid = y_of(lb)
    o, o_valid = y_of(rb)
    before = gpu_ctx.replays()
    for op in ("lt", "ne"):
        sel = sb.filter_pair(gpu_ctx, lcp, op, rcp)
        gpu_ctx.synchronize()
        R.check(sel, *R.want(y, y_valid, o, o_valid, op), lb.rows, "freq %s lz4" % op)
    assert gpu_ctx.replays() == before + 2


@pytest.mark.parametrize("name", ["route_none", "route_rle", "dict_8193", "route_snappy", "route_freq_i32"])
def test_literal_filter_then_cmp_with_and_then_read_selected(gpu_ctx, name):
    import strawboat_amd as sb
    b = Cc.build(name)
    y, y_valid = y_of(b)
    cp = upload(gpu_ctx, b.col, b.pages, b.metas)
    o, v = operands(b, mixed_type(b.col["ptype"]), 14)
    lit = np.sort(y)[b.rows // 3].item()
    sels = sb.filter_columns(gpu_ctx, [cp], [sb.Predicate("ge", lit)])
    od, vd = to_dev(gpu_ctx, o), to_dev(gpu_ctx, bits_of(v))
    out = sb.filter_columns_cmp(gpu_ctx, [cp], ["le"], [(od, vd)], combine="and", selection=sels)
    got = sb.read_selected(gpu_ctx, [cp], out[0])
    gpu_ctx.synchronize()
    live = np.ones(b.rows, bool) if y_valid is None else y_valid
    first = (y >= lit) & live
    words, selected = R.want(y, y_valid, o, v, "le", "and", R.words_of(first))
    R.check(out[0], words, selected, b.rows, name + ", chained")
    want_rows = first & R.result_bits(y, y_valid, o, v, "le")
    assert 0 < selected == int(want_rows.sum()) < b.rows
    vals, bits = got[0].numpy()
    assert got[0].selected == selected and vals.tobytes() == y[want_rows].tobytes()
    assert bits is None or bits.all()


def test_two_columns_of_different_types_in_one_call(gpu_ctx):
    import strawboat_amd as sb
    a, b = Cc.build("route_rle"), Cc.build("f32_dict")
    ao, av = operands(a, S.T_U16, 15)
    bo, bv = operands(b, S.T_F64, 16)
    sels = sb.filter_columns_cmp(gpu_ctx, [upload(gpu_ctx, a.col, a.pages, a.metas), upload(gpu_ctx, b.col, b.pages, b.metas)], ["gt", "ne"],
                                 [(to_dev(gpu_ctx, ao), to_dev(gpu_ctx, bits_of(av))), to_dev(gpu_ctx, bo)])
    gpu_ctx.synchronize()
    R.check(sels[0], *R.want(*y_of(a), ao, av, "gt"), a.rows, "column 0")
    R.check(sels[1], *R.want(*y_of(b), bo, None, "ne"), b.rows, "column 1")


def test_inside_an_interval_that_another_call_causes_to_be_replayed(gpu_ctx):
    """a column without a Freq page, replayed on the account of a literal filter over Freq pages in the same interval"""
    import strawboat_amd as sb
    b, f = Cc.build("seams_rle"), Cc.build("route_freq_i32")
    o, v = operands(b, S.T_I64, 17)
    prev = seeded_words(b.rows, 18)
    for combine in R.COMBINES:
        before = gpu_ctx.replays()
        out = selection_of(gpu_ctx, b.rows, prev)
        sels = sb.filter_columns_cmp(gpu_ctx, [upload(gpu_ctx, b.col, b.pages, b.metas)], ["ge"], [(to_dev(gpu_ctx, o), to_dev(gpu_ctx, bits_of(v)))],
                                     combine=combine, selection=[out])
        sb.filter_columns(gpu_ctx, [upload(gpu_ctx, f.col, f.pages, f.metas)], [sb.Predicate("lt", 5)])
        gpu_ctx.synchronize()
        assert gpu_ctx.replays() == before + 1
        R.check(sels[0], *R.want(*y_of(b), o, v, "ge", combine, prev), b.rows, "replayed for another call, " + combine)


# ---- 8: refusals through the raw C call
def _raw(ctx, cps, others, valids, rows, combine="set"):
    import torch
    import strawboat_amd as sb
    n = len(cps)
    outs = [selection_of(ctx, rows, np.full((rows + 31) // 32 + 2, 0xA5A5A5A5, np.uint32)) for _ in range(n)]
    batch = sb.FilterCmpBatch(ctx, cps, ["lt"] * n, [(to_dev(ctx, o), to_dev(ctx, np.concatenate([bits_of(v), np.zeros(8, np.uint8)])))
                                                    for o, v in zip(others, valids)], combine=combine, out=outs)
    batch._outs = outs
    for i in range(n):
        batch._arr[i].selection_capacity = sel_bytes(rows)
        batch._arr[i].other_validity_capacity = sel_bytes(rows)
        batch._arr[i].rows = batch._arr[i].selected = WORD
    torch.cuda.synchronize()
    return batch


def _canaries_kept(batch):
    for c, out in zip(batch._arr, batch._outs):
        assert c.rows == WORD and c.selected == WORD
        assert bool((out.bitmap == GUARD).all())


def test_refusals_at_the_call(gpu_ctx):
    from strawboat_amd import _native as N
    a, b = Cc.build("nullable_none"), Cc.build("nonnull_rle")
    rows = a.rows
    assert b.rows == rows
    acp, bcp = upload(gpu_ctx, a.col, a.pages, a.metas), upload(gpu_ctx, b.col, b.pages, b.metas)
    (ao, av), (bo, bv) = operands(a, S.T_I64, 19), operands(b, S.T_F32, 20)

    def fresh(**kw):
        return _raw(gpu_ctx, [acp, bcp], [ao, bo], [av, bv], rows, **kw)

    def refused(batch, code, what, mem=N.SB_MEM_DEVICE, sticky=False):
        assert gpu_ctx._lib.sb_filter_columns_cmp(gpu_ctx._h, batch._arr, 2, mem) == code, what
        if sticky:   # (like its siblings', the refusal of a page outside pages_len is the interval's result as well)
            with pytest.raises(N.NativeError) as e:
                gpu_ctx.synchronize()
            assert e.value.code == code, what
        else:
            gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        _canaries_kept(batch)

    def each(change, code, what, sticky=False):
        for i in (0, 1):
            batch = fresh()
            change(batch._arr[i])
            refused(batch, code, "%s (column %d)" % (what, i), sticky=sticky)

    for op in (-1, N.SB_PRED_IS_NULL, N.SB_PRED_IS_NOT_NULL, N.SB_PRED_STARTS_WITH, N.SB_PRED_IN, N.SB_PRED_NOT_IN, N.SB_PRED_CONTAINS, 16, 99):
        each(lambda c, op=op: setattr(c, "op", op), N.SB_ERR_INVALID, "op %d" % op)
    for combine in (-1, 3, 99):
        each(lambda c, combine=combine: setattr(c, "combine", combine), N.SB_ERR_INVALID, "combine %d" % combine)
    each(lambda c: setattr(c, "other", None), N.SB_ERR_INVALID, "other null")
    each(lambda c: setattr(c, "other", c.other + 1), N.SB_ERR_INVALID, "other misaligned")
    each(lambda c: setattr(c, "other_capacity", c.other_capacity - 1), N.SB_ERR_INVALID, "other short")
    each(lambda c: setattr(c, "other_validity", c.other_validity + 2), N.SB_ERR_INVALID, "other_validity misaligned")
    each(lambda c: setattr(c, "other_validity_capacity", sel_bytes(rows) - 4), N.SB_ERR_INVALID, "other_validity short")
    each(lambda c: setattr(c, "other_validity", None), N.SB_ERR_INVALID, "a validity capacity without a pointer")
    for flags in (1, 2, 0x80000000):
        each(lambda c, flags=flags: setattr(c, "flags", flags), N.SB_ERR_INVALID, "flags %#x" % flags)
    each(lambda c: setattr(c, "reserved", 1), N.SB_ERR_INVALID, "reserved != 0")

    def onto_other(c):   # the last word of the selection is the first of the operand
        c.selection = c.other - sel_bytes(rows) + 4

    def onto_validity(c):
        c.selection = c.other_validity + sel_bytes(rows) - 4

    each(onto_other, N.SB_ERR_INVALID, "selection overlaps other")
    each(onto_validity, N.SB_ERR_INVALID, "selection overlaps other_validity")
    batch = fresh()
    batch._arr[1].selection = batch._arr[0].selection + sel_bytes(rows) - 4
    refused(batch, N.SB_ERR_INVALID, "the selections of two columns overlap")
    # every argument refusal of sb_filter_columns
    for bad in (-1, S.T_NULL + 1, 99):
        each(lambda c, bad=bad: setattr(c, "physical_type", bad), N.SB_ERR_INVALID, "bad physical_type %d" % bad)
        each(lambda c, bad=bad: setattr(c, "other_type", bad), N.SB_ERR_INVALID, "bad other_type %d" % bad)
    each(lambda c: setattr(c, "selection", None), N.SB_ERR_INVALID, "selection null")
    each(lambda c: setattr(c, "selection", c.selection + 1), N.SB_ERR_INVALID, "misaligned selection")
    each(lambda c: setattr(c, "selection_capacity", sel_bytes(rows) - 4), N.SB_ERR_INVALID, "short selection_capacity")
    each(lambda c: setattr(c, "metas", None), N.SB_ERR_INVALID, "metas null with n_pages > 0")
    for ptype in (S.T_BIN32, S.T_BIN64, S.T_BOOL, S.T_I128, S.T_I256, S.T_NULL):
        each(lambda c, ptype=ptype: setattr(c, "physical_type", ptype), N.SB_ERR_NYI, "y of type %d" % ptype)
        each(lambda c, ptype=ptype: setattr(c, "other_type", ptype), N.SB_ERR_NYI, "other of type %d" % ptype)
    refused(fresh(), N.SB_ERR_NYI, "SB_MEM_HOST", mem=N.SB_MEM_HOST)
    each(lambda c: setattr(c, "pages_len", c.pages_len - 1), N.SB_ERR_IO, "a page outside [0, pages_len)", sticky=True)
    keep = np.array([1 << 40], np.uint64)
    batch = fresh()
    batch._arr[0].page_offsets = np.concatenate([np.zeros(a.metas.shape[0] - 1, np.uint64), keep]).ctypes.data
    refused(batch, N.SB_ERR_IO, "a page offset outside pages_len", sticky=True)
    # the same batch, as it was built, then succeeds, in each mode
    for combine in R.COMBINES:
        batch = fresh(combine=combine)
        res = batch.enqueue()
        gpu_ctx.synchronize()
        prev = np.full((rows + 31) // 32, 0xA5A5A5A5, np.uint32)
        for r, bb, o, v in zip(res, (a, b), (ao, bo), (av, bv)):
            R.check(r, *R.want(*y_of(bb), o, v, "lt", combine, prev), rows, "after the refusals, " + combine)
            assert bool((r.bitmap[sel_bytes(rows):] == GUARD).all())


# ---- 9: errors at the synchronize
def cmp_code(ctx, cp, other):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    try:
        sb.filter_columns_cmp(ctx, [cp], ["lt"], [other])
        ctx.synchronize()
    except NativeError as e:
        try:
            ctx.synchronize()
        except NativeError:
            pass
        return e.code
    return 0


def test_corrupt_pages_raise_what_the_decoder_raises(gpu_ctx):
    from tests import gen
    # a truncated last page
    for name in ("route_none", "route_rle", "route_dict", "route_lz4", "f64_patas"):
        b = Cc.build(name)
        m = np.array(b.metas, np.uint64).copy()
        cut = int(m[-1, 0]) // 2
        m[-1, 0] -= cut
        bad = b.pages[:b.pages.size - cut].copy()
        cp = upload(gpu_ctx, b.col, bad, m)
        want = read_code(gpu_ctx, cp)
        oc = oracle_code(b.col, bad, m)
        assert want != 0 and oc != 0 and (oc is None or oc == want), (name, want, oc)
        assert cmp_code(gpu_ctx, cp, to_dev(gpu_ctx, Cc.operand_for(b, S.T_I32))) == want, name
    # a Dict page with an index >= D: plain u32 indices behind hdr9 Dict | hdr9 None
    for uniq in (50, 20_000):   # at or below FILTER_DICT_BITS entries, and above: one route here
        col = gen.prim(S.T_I64, 40_000, uniq=uniq, seed=uniq)
        pages, metas = gen.oracle_write(col, max_page_size=40_000, force_codec=S.DICT, force_index_codec=S.NONE)
        bad = pages.copy()
        pos = 9 + 9 + 25_000 * 4
        bad[pos:pos + 4] = np.frombuffer(np.uint32(1 << 30).tobytes(), np.uint8)
        cp = upload(gpu_ctx, col, bad, metas)
        want = read_code(gpu_ctx, cp)
        assert want == -1 and oracle_code(col, bad, metas) != 0
        assert cmp_code(gpu_ctx, cp, to_dev(gpu_ctx, np.zeros(40_000, np.int64))) == want
    # the context still works
    six_ops_both_operands(gpu_ctx, "route_dict")
