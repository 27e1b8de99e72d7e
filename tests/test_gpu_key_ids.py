"""sb_key_ids on the GPU: pages written by the CPU oracle, the distinct keys and the dense ids found on the device, compared
with the ORACLE's decode of the pages under np.unique / np.searchsorted (tests/key_ids_ref.py, checked on its own against
a dict-based group-by in tests/test_key_ids_host.py).  Nothing here is compared with what the device's own decoder gives.

Every comparison is exact: the bytes of `keys`, every id, and rows / selected / count / n_keys / overflow.  Unless a test
says otherwise a column has about 10 000 rows and runs with no selection, under a random selection of about 30 % and under
a selection that leaves no row; the forced codec is asserted from S.stat_column."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import sbo as S
from tests import gen
from tests import key_ids_ref as K
from tests.test_gpu_aggregate import bitmap
from tests.test_gpu_decode import LONG_RLE_ROWS, _rle_hand_built_column, _rle_long_page
from tests.test_gpu_filter import hand_built
from tests.test_gpu_read_selected import oracle_code, read_code, to_dev, upload

pytestmark = pytest.mark.gpu

NP = gen.NP_OF
INTS = [S.T_I8, S.T_I16, S.T_I32, S.T_I64, S.T_U8, S.T_U16, S.T_U32, S.T_U64]
GUARD = 0xA5
GUARD_BYTES = 4096
WORD = 0x5A5A5A5A5A5A5A5A
RESULTS = ("rows", "selected", "count", "n_keys", "overflow")


def three_masks(rows, seed):
    """no selection, a random one of about 30 %, and one that leaves no row"""
    return [None, np.random.default_rng(seed).random(rows) < 0.3, np.zeros(rows, bool)]


def run(ctx, cps, masks, refs, max_keys, id_widths, what=""):
    """the columns of ONE call, each under its own selection (None: no selection), max_keys and id_width"""
    import strawboat_amd as sb
    res = sb.key_ids(ctx, cps, [bitmap(ctx, m) for m in masks], list(max_keys), list(id_widths))
    ctx.synchronize()
    for i, (r, ref, m, mk, w) in enumerate(zip(res, refs, masks, max_keys, id_widths)):
        K.check(r, K.want(ref, m, mk, w), "%s column %d (max_keys %d, id_width %d)" % (what, i, mk, w))
    return res


def check_pages(ctx, col, pages, metas, masks=None, max_keys=256, id_widths=(1, 2, 4), what=""):
    ref = K.Ref(col, pages, metas)
    if masks is None:
        masks = three_masks(ref.rows, 11)
    cp = upload(ctx, col, pages, metas)
    combos = [(m, w) for m in masks for w in id_widths]
    n = len(combos)
    # (ids of one byte name at most 255 keys: all ones is no id)
    return run(ctx, [cp] * n, [c[0] for c in combos], [ref] * n, [min(max_keys, 255 if c[1] == 1 else 1024) for c in combos],
               [c[1] for c in combos], what)


def check(ctx, col, codec=None, masks=None, max_keys=256, id_widths=(1, 2, 4), **opt):
    pages, metas = gen.oracle_write(col, **opt)
    if codec is not None:
        seen = set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())
        assert seen == {codec}, (seen, codec)
    return check_pages(ctx, col, pages, metas, masks, max_keys, id_widths, what="codec %r %r" % (codec, opt))


def _column(ptype, values, validity=None):
    values = np.asarray(values, NP[ptype])
    return dict(ptype=ptype, nullable=validity is not None, rows=values.size, values=values,
                validity=None if validity is None else gen.pack_bits(validity), offsets=None)


# ---- 1: codecs x types
@pytest.mark.parametrize("ptype", INTS)
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT, S.ONEVALUE])
def test_prim_codecs(gpu_ctx, ptype, codec):
    uniq = 1 if codec == S.ONEVALUE else 100
    for nd, page in ((0.2, 2050), (None, 4100), (0.2, 777), (None, 2048)):
        col = gen.prim(ptype, 10_000, uniq=uniq, null_density=nd, runs=8 if nd else 3, seed=page)
        res = check(gpu_ctx, col, codec=codec, max_page_size=page, force_codec=codec)
        assert not res[0].overflow and 1 <= res[0].n_keys <= uniq and res[-1].n_keys == 0


# ---- 2: bit-packed pages
@pytest.mark.parametrize("ptype", [S.T_I32, S.T_U32])
@pytest.mark.parametrize("codec", [S.BITPACK, S.DELTABP])
def test_bitpacking(gpu_ctx, ptype, codec):
    col = gen.prim(ptype, 128 * 100, uniq=200, sorted_=(codec == S.DELTABP))
    check(gpu_ctx, col, codec=codec, id_widths=(1, 4), max_page_size=128 * 40, force_codec=codec)


# ---- 3: the index codecs of Dict pages
@pytest.mark.parametrize("icodec", [S.NONE, S.RLE, S.BITPACK, S.DELTABP, S.ONEVALUE, S.LZ4])
def test_dict_index_codecs(gpu_ctx, icodec):
    uniq = 1 if icodec == S.ONEVALUE else 200
    col = gen.prim(S.T_I64, 128 * 100, uniq=uniq, null_density=0.1, runs=16, sorted_=(icodec == S.DELTABP))
    check(gpu_ctx, col, codec=S.DICT, id_widths=(1, 2), max_page_size=128 * 40, force_codec=S.DICT, force_index_codec=icodec)


# ---- 4: only the entries that live rows point at are keys; both sides of the LDS table
def test_dict_referenced_entries_only_on_both_sides_of_the_table(gpu_ctx):
    for uniq, rows in ((8000, 60_000), (8192 * 4, 70_000)):
        col = gen.prim(S.T_I64, rows, uniq=uniq, null_density=0.2, seed=uniq)
        pages, metas = gen.oracle_write(col, max_page_size=rows, force_codec=S.DICT)
        assert metas.shape[0] == 1
        assert set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist()) == {S.DICT}
        d = np.unique(col["values"]).size
        assert (d <= 8192) == (uniq == 8000), d
        ref = K.Ref(col, pages, metas)
        live = np.unique(ref.vals[ref.valid])
        assert live.size > 1024
        chosen = live[[0, 1, live.size // 3, live.size // 2, -1]]
        only = np.isin(ref.vals, chosen)   # (null rows of these values are selected too: they give no key)
        cp = upload(gpu_ctx, col, pages, metas)
        res = run(gpu_ctx, [cp] * 3, [only, None, only], [ref] * 3, [16, 1024, 5], [1, 2, 4], what="dict %d" % uniq)
        assert (res[0].n_keys, res[0].overflow) == (5, False) and res[0].keys.tolist() == chosen.tolist()
        assert res[1].overflow and not res[2].overflow


# ---- 5: compressed pages are inflated into the staging area once, and walked twice
@pytest.mark.parametrize("ptype", [S.T_I16, S.T_I64])
@pytest.mark.parametrize("codec", [S.LZ4, S.ZSTD, S.SNAPPY])
def test_basic_pages_are_staged(gpu_ctx, ptype, codec):
    col = gen.prim(ptype, 10_000, uniq=300, null_density=0.2, runs=5, seed=codec)
    check(gpu_ctx, col, codec=codec, max_keys=512, id_widths=(2, 4), max_page_size=7001, force_codec=codec)


# ---- 6: the RLE walk
@pytest.mark.parametrize("ptype,w,dtype", [(S.T_U8, 1, np.uint8), (S.T_I16, 2, np.int16), (S.T_I32, 4, np.int32), (S.T_I64, 8, np.int64)])
def test_rle_hand_built_pages(gpu_ctx, ptype, w, dtype):
    col, pages, metas = hand_built(ptype, *_rle_hand_built_column(w, dtype))
    assert col is not None
    check_pages(gpu_ctx, col, pages, metas, what="hand-built RLE")


def test_rle_long_page_in_parts(gpu_ctx):
    col, pages, metas = hand_built(S.T_I64, [_rle_long_page()], [LONG_RLE_ROWS])
    assert col is not None and metas.shape[0] == 1
    n = np.unique(col["values"]).size
    masks = [None, np.random.default_rng(6).random(LONG_RLE_ROWS) < 0.3, np.zeros(LONG_RLE_ROWS, bool)]
    check_pages(gpu_ctx, col, pages, metas, masks, max_keys=min(1024, n), id_widths=(2,), what="long RLE page")


def test_rle_runs_without_a_live_row_give_no_key(gpu_ctx):
    rng = np.random.default_rng(61)
    v = np.repeat(rng.integers(0, 50, 400), 25).astype(np.int32)   # 400 runs of 25 rows
    v[1000:1025] = 7777    # a run that is unselected as a whole
    v[5000:5025] = 8888    # a run that is null as a whole
    v[9000:9025] = 9999    # a run with one live row
    valid = rng.random(10_000) >= 0.1
    valid[5000:5025] = False
    valid[9010] = True
    mask = rng.random(10_000) < 0.5
    mask[1000:1025] = False
    mask[9000:9025] = False
    mask[9010] = True
    col = _column(S.T_I32, v, valid)
    res = check(gpu_ctx, col, codec=S.RLE, masks=[mask] + three_masks(10_000, 62), id_widths=(1,), max_page_size=4100, force_codec=S.RLE)
    keys = res[0].keys.tolist()
    assert 7777 not in keys and 8888 not in keys and 9999 in keys


# ---- 7: Freq pages: the interval is issued again, the call's columns decoded
@pytest.mark.parametrize("ptype", [S.T_I32, S.T_I64, S.T_U8])
def test_freq_pages(gpu_ctx, ptype):
    from tests.test_gpu_freq import sparse
    rows = 10_000
    f = sparse(ptype, rows, 0.05, 2, null_density=0.1, exc_uniq=200)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    assert S.FREQ in set(int(x) for x in S.stat_column(f["ptype"], f["nullable"], fp, fm)[0].tolist())
    fref = K.Ref(f, fp, fm)
    fcp = upload(gpu_ctx, f, fp, fm)
    masks = three_masks(rows, ptype)
    for _ in range(2):   # ... and the same column again in the next interval
        r0 = gpu_ctx.replays()
        run(gpu_ctx, [fcp] * 3, masks, [fref] * 3, [255, 256, 1024], [1, 2, 4], what="freq")
        assert gpu_ctx.replays() == r0 + 1


# ---- 8: the overflow boundary
def _boundary_column(max_keys, where, rng):
    """10 000 rows of exactly max_keys distinct values in runs of two, and one extra value at `where`: 'first', 'last',
    'dead' (a row that is null, under a selection that leaves it out as well) or None (no extra value)"""
    rows = 10_000
    base = (np.arange(max_keys, dtype=np.int64) * 7919 - 3_000_000)
    v = np.repeat(base[rng.integers(0, max_keys, rows // 2)], 2)
    v[2:2 + 2 * max_keys:2] = base[:min(max_keys, (rows - 2) // 2)]   # every value is there
    valid = rng.random(rows) >= 0.1
    valid[2:2 + 2 * max_keys:2] = True
    valid[0] = valid[rows - 1] = True
    mask = np.ones(rows, bool)
    extra = 123_456_789
    if where == "first":
        v[0] = extra
    elif where == "last":
        v[rows - 1] = extra
    elif where == "dead":
        v[rows // 2 + 1] = extra
        valid[rows // 2 + 1] = False
        v[rows // 2 + 3] = extra
        mask[rows // 2 + 3] = False
    return _column(S.T_I64, v, valid), mask


@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
@pytest.mark.parametrize("max_keys,id_width", [(1, 1), (255, 1), (256, 2), (1024, 2), (1024, 4)])
def test_the_overflow_boundary(gpu_ctx, codec, max_keys, id_width):
    rng = np.random.default_rng(max_keys + id_width)
    cps, masks, refs, wants = [], [], [], []
    for where in (None, "first", "last", "dead"):
        col, mask = _boundary_column(max_keys, where, rng)
        pages, metas = gen.oracle_write(col, max_page_size=4100, force_codec=codec)
        assert set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist()) == {codec}
        cps.append(upload(gpu_ctx, col, pages, metas))
        refs.append(K.Ref(col, pages, metas))
        masks.append(mask)
        wants.append(where in ("first", "last"))
    res = run(gpu_ctx, cps, masks, refs, [max_keys] * 4, [id_width] * 4, what="boundary")   # (the synchronize returned)
    assert [r.overflow for r in res] == wants
    for r in (res[0], res[3]):
        assert r.n_keys == max_keys
        ids = K.ids_numpy(r)
        assert int(ids[ids != (1 << (8 * id_width)) - 1].max()) == max_keys - 1


# ---- 9: extremes
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_extremes_are_keys_in_the_order_of_the_signedness(gpu_ctx, codec):
    rng = np.random.default_rng(codec + 9)
    runs = np.repeat(np.arange(10_000 // 5 + 1), 5)[:10_000]
    for ptype in INTS:
        dt = np.dtype(NP[ptype])
        info = np.iinfo(dt)
        pool = [info.min, info.max, 0] + ([-1, info.min + 1] if info.min < 0 else [1, info.max - 1])
        v = np.array(pool, dt)[rng.integers(0, len(pool), 10_000)[runs]]
        valid = rng.random(10_000) >= 0.2
        v[:5 * len(pool)] = np.repeat(np.array(pool, dt), 5)
        valid[:5 * len(pool)] = True
        res = check(gpu_ctx, _column(ptype, v, valid), codec=codec, id_widths=(1,), max_page_size=4100, force_codec=codec)
        r = res[0]   # (no selection; the random and the empty one are checked against the reference like it)
        assert r.keys.tolist() == sorted(set(pool)) and r.keys[0] == info.min and r.keys[-1] == info.max
        kb = np.frombuffer(r.key_bytes, np.uint8).reshape(r.max_keys, 8)
        assert not kb[:, dt.itemsize:].any(), "zeros behind the value's width"


# ---- 10: buffers
def _guarded(ctx, nbytes, align=1):
    """(the `nbytes` handed to the call, the whole buffer): between two guards of GUARD_BYTES bytes of GUARD"""
    import torch
    whole = torch.full((2 * GUARD_BYTES + nbytes,), GUARD, dtype=torch.uint8, device=ctx.torch_device)
    assert whole.data_ptr() % 4 == 0 and GUARD_BYTES % align == 0
    return whole[GUARD_BYTES:GUARD_BYTES + nbytes], whole


def _guards_intact(whole, nbytes):
    h = whole.cpu().numpy()
    return bool((h[:GUARD_BYTES] == GUARD).all() and (h[GUARD_BYTES + nbytes:] == GUARD).all())


@pytest.mark.parametrize("id_width", [1, 2, 4])
def test_ids_and_keys_of_exactly_their_size_between_guards(gpu_ctx, id_width):
    import torch
    import strawboat_amd as sb
    from strawboat_amd.key_ids import ID_DTYPES
    rows, max_keys = 10_001, 64
    shapes = ((40, S.NONE), (40, S.RLE), (40, S.DICT), (500, S.NONE), (500, S.DICT))   # (500: the overflow)
    for (uniq, codec), mask in [(sh, m) for sh in shapes for m in three_masks(rows, id_width)]:
        col = gen.prim(S.T_I32, rows, uniq=uniq, null_density=0.2, runs=4, seed=uniq + codec)
        pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
        ref = K.Ref(col, pages, metas)
        cp = upload(gpu_ctx, col, pages, metas)
        ids_bytes, ids_whole = _guarded(gpu_ctx, rows * id_width, id_width)
        ids = ids_bytes.view(getattr(torch, ID_DTYPES[id_width]))
        batch = sb.KeyIdsBatch(gpu_ctx, [cp], bitmap(gpu_ctx, mask), max_keys, id_width, out=[ids])
        keys = (C.c_uint8 * (8 * max_keys + 2 * GUARD_BYTES))()
        C.memset(keys, GUARD, C.sizeof(keys))
        batch._arr[0].keys = C.addressof(keys) + GUARD_BYTES
        assert batch._arr[0].ids_capacity == rows * id_width
        res = batch.enqueue()
        gpu_ctx.synchronize()
        w = K.want(ref, mask, max_keys, id_width)
        assert res[0].overflow == w.overflow == (uniq == 500 and (mask is None or bool(mask.any())))
        assert _guards_intact(ids_whole, rows * id_width), "a byte outside ids was written"
        kb = bytes(keys)
        assert kb[:GUARD_BYTES] == bytes([GUARD]) * GUARD_BYTES and kb[GUARD_BYTES + 8 * max_keys:] == bytes([GUARD]) * GUARD_BYTES
        if not w.overflow:
            assert kb[GUARD_BYTES:GUARD_BYTES + 8 * max_keys] == w.key_bytes
            assert kb[GUARD_BYTES + 8 * w.n_keys:GUARD_BYTES + 8 * max_keys] == bytes(8 * (max_keys - w.n_keys))
            assert np.array_equal(ids.cpu().numpy().view(K.ID_NP[id_width]), w.ids)
            assert (res[0].rows, res[0].selected, res[0].count, res[0].n_keys) == (w.rows, w.selected, w.count, w.n_keys)


def test_pages_at_odd_byte_offsets_and_scattered_page_offsets(gpu_ctx):
    import torch
    from strawboat_amd import read
    for codec in (S.NONE, S.RLE, S.DICT, S.LZ4):
        col = gen.prim(S.T_I64, 10_000, uniq=90, null_density=0.2, runs=5, seed=codec)
        pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
        ref = K.Ref(col, pages, metas)
        cps = []
        for off in (1, 3, 7):
            buf = torch.zeros(off + pages.size, dtype=torch.uint8, device=gpu_ctx.torch_device)
            buf[off:] = torch.from_numpy(np.ascontiguousarray(pages)).to(gpu_ctx.torch_device)
            cps.append(read.ColumnPages(col["ptype"], col["nullable"], buf[off:], metas))
        # the pages in descending order in the buffer, with gaps of odd lengths between them
        lens = [int(x) for x in metas[:, 0]]
        starts = np.concatenate([[0], np.cumsum(lens)])[:-1]
        scattered, offs, at = [], [0] * len(lens), 5
        for p in range(len(lens) - 1, -1, -1):
            offs[p] = at
            at += lens[p] + 3 + 2 * p
        buf = np.full(at, 0xEE, np.uint8)
        for p in range(len(lens)):
            buf[offs[p]:offs[p] + lens[p]] = pages[starts[p]:starts[p] + lens[p]]
        cps.append(read.ColumnPages(col["ptype"], col["nullable"], to_dev(gpu_ctx, buf), metas, page_offsets=np.array(offs, np.uint64)))
        for mask in three_masks(10_000, codec):
            run(gpu_ctx, cps, [mask] * 4, [ref] * 4, [128] * 4, [1, 2, 4, 1], what="offsets, codec %d" % codec)


def test_columns_without_rows_or_pages(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    dev = gpu_ctx.torch_device
    empty = read.ColumnPages(S.T_I64, True, torch.zeros(0, dtype=torch.uint8, device=dev), np.zeros((0, 2), np.uint64))
    for sel in (None, torch.zeros(0, dtype=torch.uint8, device=dev)):
        r = sb.key_ids(gpu_ctx, [empty], sel, 7)[0]
        gpu_ctx.synchronize()
        assert (r.rows, r.selected, r.count, r.n_keys, r.overflow) == (0, 0, 0, 0, False) and r.key_bytes == bytes(56)
        assert r.ids.numel() == 0
    col = gen.prim(S.T_I32, 3000, uniq=50, null_density=0.3, seed=4)
    pages, metas = gen.oracle_write(col, max_page_size=777, force_codec=S.NONE)
    ref = K.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(1).random(3000) < 0.5
    res = sb.key_ids(gpu_ctx, [empty, cp, empty], [None, bitmap(gpu_ctx, mask), None], [3, 64, 1024], [1, 1, 4])
    gpu_ctx.synchronize()
    assert (res[0].rows, res[0].n_keys, res[2].selected) == (0, 0, 0) and res[2].key_bytes == bytes(8 * 1024)
    K.check(res[1], K.want(ref, mask, 64, 1), "next to empty columns")


# ---- 11: the same bytes every time
def test_the_same_bytes_every_time(gpu_ctx):
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows = 10_000
    rng = np.random.default_rng(7)
    shapes = [(S.T_I64, S.NONE, 40), (S.T_I16, S.DICT, 3), (S.T_I64, S.RLE, 20), (S.T_U32, S.LZ4, 200),
              (S.T_U8, S.NONE, 250), (S.T_I32, S.DICT, 900), (S.T_U64, S.RLE, 500), (S.T_I8, S.ONEVALUE, 1)]
    cps, refs = [], []
    for i, (ptype, codec, uniq) in enumerate(shapes * 2):   # 16 columns
        col = gen.prim(ptype, rows, uniq=uniq, null_density=0.2 if i % 2 else None, runs=6 if codec == S.RLE else None, seed=i)
        pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=codec)
        cps.append(upload(gpu_ctx, col, pages, metas))
        refs.append(K.Ref(col, pages, metas))
    mask = rng.random(rows) < 0.35
    mks = [1024 if i % 3 else 256 for i in range(16)]
    ws = [2 if i % 4 else 4 for i in range(16)]
    batch = sb.KeyIdsBatch(gpu_ctx, cps, bitmap(gpu_ctx, mask), mks, ws)
    seen = []
    for _ in range(5):   # fresh intervals
        res = batch.enqueue()
        gpu_ctx.synchronize()
        seen.append([(r.key_bytes, r.ids.cpu().numpy().tobytes(), r.n_keys, r.count) for r in res])
    # ... and in an interval that a filter call's Freq column causes to be issued again
    x = sparse(S.T_I32, rows, 0.05, 2, null_density=0.1)
    xp, xm = gen.oracle_write(x, max_page_size=2050, force_codec=S.FREQ)
    r0 = gpu_ctx.replays()
    sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("ne", 7)])
    res = batch.enqueue()
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    seen.append([(r.key_bytes, r.ids.cpu().numpy().tobytes(), r.n_keys, r.count) for r in res])
    assert all(s == seen[0] for s in seen[1:])
    for i, (r, ref) in enumerate(zip(res, refs)):
        K.check(r, K.want(ref, mask, mks[i], ws[i]), "in the replayed interval, column %d" % i)


# ---- 12: the chain the call exists for
def test_filter_then_key_ids_then_grouped_aggregate_in_one_interval(gpu_ctx):
    import strawboat_amd as sb
    from tests.aggregate_ref import reduce_values
    rows = 10_007
    rng = np.random.default_rng(12)
    x = gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    keys40 = (rng.integers(-2 ** 62, 2 ** 62, 40)).astype(np.int64)   # sparse keys
    k = _column(S.T_I64, keys40[rng.integers(0, 40, rows)], rng.random(rows) >= 0.15)
    y = gen.prim(S.T_I64, rows, uniq=5000, null_density=0.1, seed=2)
    xp, xm = gen.oracle_write(x, max_page_size=2050, force_codec=S.RLE)
    kp, km = gen.oracle_write(k, max_page_size=4100, force_codec=S.DICT)
    yp, ym = gen.oracle_write(y, max_page_size=4100, force_codec=S.NONE)
    xr, kr, yr = K.Ref(x, xp, xm), K.Ref(k, kp, km), K.Ref(y, yp, ym)
    mask = (xr.vals < 60) & xr.valid
    assert 0 < mask.sum() < rows
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("lt", 60)])
    kid = sb.key_ids(gpu_ctx, [upload(gpu_ctx, k, kp, km)], sel[0], max_keys=64)[0]
    assert kid.id_width == 1
    agg = sb.aggregate_grouped(gpu_ctx, [upload(gpu_ctx, y, yp, ym)], kid.ids, 64, sel[0])[0]
    gpu_ctx.synchronize()   # (the only one)
    assert np.array_equal(sel[0].numpy(), mask)
    K.check(kid, K.want(kr, mask, 64, 1), "behind the filter")
    # a numpy group-by of the oracle's decode
    want_keys = np.unique(kr.vals[mask & kr.valid])
    assert kid.n_keys == want_keys.size == 40
    assert agg.out_of_range == int((mask & ~kr.valid).sum())
    for g, key in enumerate(want_keys.tolist()):
        in_group = mask & kr.valid & (kr.vals == key)
        w = reduce_values(S.T_I64, yr.vals, in_group & yr.valid, int(in_group.sum()))
        got = agg[g]
        assert (got.selected, got.count) == (int(in_group.sum()), w.count), g
        live = yr.vals[in_group & yr.valid]
        if w.count:
            assert (got.min, got.max, got.sum) == (int(live.min()), int(live.max()), int(live.astype(object).sum())), g
    for g in range(40, 64):
        assert (agg[g].selected, agg[g].count) == (0, 0)


def test_keys_as_the_list_of_a_semi_join(gpu_ctx):
    import strawboat_amd as sb
    rows = 10_000
    rng = np.random.default_rng(13)
    dim = _column(S.T_I32, rng.integers(0, 5000, rows) * 3 - 700, rng.random(rows) >= 0.1)   # the dimension's key column
    flag = gen.prim(S.T_U8, rows, uniq=10, seed=3)                                           # ... and its filter column
    fact = _column(S.T_I32, rng.integers(0, 5000, rows) * 3 - 700, rng.random(rows) >= 0.1)
    dp, dm = gen.oracle_write(dim, max_page_size=2050, force_codec=S.NONE)
    gp, gm = gen.oracle_write(flag, max_page_size=2050, force_codec=S.RLE)
    fp, fm = gen.oracle_write(fact, max_page_size=4100, force_codec=S.DICT)
    dr, gr, fr = K.Ref(dim, dp, dm), K.Ref(flag, gp, gm), K.Ref(fact, fp, fm)
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, flag, gp, gm)], [sb.Predicate("eq", 3)])
    kid = sb.key_ids(gpu_ctx, [upload(gpu_ctx, dim, dp, dm)], sel[0], max_keys=1024)[0]
    gpu_ctx.synchronize()
    mask = (gr.vals == 3) & gr.valid
    K.check(kid, K.want(dr, mask, 1024, 2), "the build side")
    assert not kid.overflow and 100 < kid.n_keys <= 1024
    hit = sb.filter_in(gpu_ctx, [upload(gpu_ctx, fact, fp, fm)], [sb.InList(kid.keys.tolist())])
    gpu_ctx.synchronize()
    assert np.array_equal(hit[0].numpy(), np.isin(fr.vals, dr.vals[mask & dr.valid]) & fr.valid)


# ---- 13: several columns of different types, max_keys and id_width in one call
def test_columns_with_different_types_max_keys_and_widths_in_one_call(gpu_ctx):
    rng = np.random.default_rng(8)
    cps, refs = [], []
    for ptype, codec, page, uniq in ((S.T_I64, S.NONE, 4100, 300), (S.T_U8, S.DICT, 2050, 200), (S.T_U16, S.RLE, 2050, 700),
                                     (S.T_I32, S.LZ4, 2050, 30), (S.T_I8, S.ONEVALUE, 777, 1)):
        col = gen.prim(ptype, 10_000, uniq=uniq, null_density=0.2, runs=5, seed=page + ptype)
        pages, metas = gen.oracle_write(col, max_page_size=page, force_codec=codec)
        cps.append(upload(gpu_ctx, col, pages, metas))
        refs.append(K.Ref(col, pages, metas))
    masks = [rng.random(10_000) < 0.35, None, rng.random(10_000) < 0.9, np.zeros(10_000, bool), None]
    for mks, ws in (([512, 255, 1024, 64, 1], [2, 1, 4, 1, 1]), ([100, 100, 100, 10, 3], [4, 2, 2, 4, 2]), ([1024] * 5, [2] * 5)):
        res = run(gpu_ctx, cps, masks, refs, mks, ws, what="max_keys %r" % (mks,))
        run(gpu_ctx, cps[::-1], masks[::-1], refs[::-1], mks, ws, what="max_keys %r, the columns turned round" % (mks,))
        assert any(r.overflow for r in res) == (mks[0] == 100)


# ---- 14: refusals through the raw C call
def _raw(ctx, cps, bitmaps, rows, max_keys=7, id_width=2):
    import torch
    import strawboat_amd as sb
    batch = sb.KeyIdsBatch(ctx, cps, bitmaps, max_keys, id_width)
    batch._keys, batch._ids = [], []
    for i in range(len(cps)):
        keys = (C.c_uint8 * (8 * max_keys))()
        C.memset(keys, GUARD, C.sizeof(keys))
        batch._arr[i].keys = C.addressof(keys)
        ids = torch.full((rows * id_width + 8,), GUARD, dtype=torch.uint8, device=ctx.torch_device)
        batch._arr[i].ids = ids.data_ptr()
        batch._arr[i].ids_capacity = rows * id_width + 8
        batch._keys.append(keys)
        batch._ids.append(ids)
        for f in RESULTS:
            setattr(batch._arr[i], f, WORD)
    return batch


def _canaries_kept(batch):
    for c, keys, ids in zip(batch._arr, batch._keys, batch._ids):
        assert all(getattr(c, f) == WORD for f in RESULTS)
        assert bytes(keys) == bytes([GUARD]) * C.sizeof(keys)
        assert bool((ids == GUARD).all())


def test_refusals_at_the_call(gpu_ctx):
    from strawboat_amd import _native as N
    rows = 5000
    col = gen.prim(S.T_I64, rows, uniq=5, null_density=0.2)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.NONE)
    ref = K.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(9).random(rows) < 0.5
    bm = bitmap(gpu_ctx, mask)

    def fresh(**kw):
        return _raw(gpu_ctx, [cp, cp], [bm, bm], rows, **kw)

    def refused(batch, code, what, mem=N.SB_MEM_DEVICE):
        assert gpu_ctx._lib.sb_key_ids(gpu_ctx._h, batch._arr, 2, mem) == code, what
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        _canaries_kept(batch)

    for w in (0, 3, 8, 0xFFFFFFFF):
        batch = fresh()
        batch._arr[1].id_width = w
        refused(batch, N.SB_ERR_INVALID, "id_width %d" % w)
    for mk, w in ((0, 2), (1025, 2), (1025, 4), (1 << 31, 4), (256, 1), (1024, 1)):
        batch = fresh()
        batch._arr[1].max_keys, batch._arr[1].id_width = mk, w
        refused(batch, N.SB_ERR_INVALID, "max_keys %d at id_width %d" % (mk, w))
    batch = fresh()
    batch._arr[0].ids = None
    refused(batch, N.SB_ERR_INVALID, "ids null")
    batch = fresh()
    batch._arr[1].ids += 1
    refused(batch, N.SB_ERR_INVALID, "ids misaligned")
    batch = fresh()
    batch._arr[1].ids_capacity = rows * 2 - 1
    refused(batch, N.SB_ERR_INVALID, "ids too small")
    batch = fresh()
    batch._arr[0].keys = None
    refused(batch, N.SB_ERR_INVALID, "keys null")
    batch = fresh()
    batch._arr[1].reserved = 1
    refused(batch, N.SB_ERR_INVALID, "reserved != 0")
    batch = fresh()
    batch._arr[1].ids = batch._arr[0].ids + rows * 2 - 2   # the last id of column 0 is the first of column 1
    refused(batch, N.SB_ERR_INVALID, "ids of two columns overlap")
    for bad in (-1, S.T_NULL + 1, 99):
        batch = fresh()
        batch._arr[0].physical_type = bad
        refused(batch, N.SB_ERR_INVALID, "bad physical_type %d" % bad)
    batch = fresh()
    batch._arr[1].selection += 1
    refused(batch, N.SB_ERR_INVALID, "misaligned selection")
    batch = fresh()
    batch._arr[1].selection_capacity = (rows + 31) // 32 * 4 - 4
    refused(batch, N.SB_ERR_INVALID, "short selection_capacity")
    batch = fresh()
    batch._arr[0].metas = None
    refused(batch, N.SB_ERR_INVALID, "metas null with n_pages > 0")
    for ptype in (S.T_F32, S.T_F64, S.T_BOOL, S.T_I128, S.T_I256, S.T_BIN32, S.T_BIN64, S.T_NULL):
        batch = fresh()
        batch._arr[1].physical_type = ptype
        refused(batch, N.SB_ERR_NYI, "type %d" % ptype)
    batch = fresh()
    refused(batch, N.SB_ERR_NYI, "SB_MEM_HOST", mem=N.SB_MEM_HOST)
    # the same batch, as it was built, then succeeds
    batch = fresh()
    res = batch.enqueue()
    gpu_ctx.synchronize()
    w = K.want(ref, mask, 7, 2)
    for r, keys, ids in zip(res, batch._keys, batch._ids):
        assert bytes(keys) == w.key_bytes and (r.n_keys, r.count, r.overflow) == (w.n_keys, w.count, False)
        h = ids.cpu().numpy()
        assert np.array_equal(h[:rows * 2].view(np.uint16), w.ids) and (h[rows * 2:] == GUARD).all()


# ---- 15: errors at the synchronize
def test_a_truncated_page_raises_what_the_decoder_raises(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    for codec in (S.NONE, S.RLE, S.DICT, S.LZ4):
        col = gen.prim(S.T_I64, 9000, uniq=60, null_density=0.1, runs=6)
        pages, metas = gen.oracle_write(col, max_page_size=3000, force_codec=codec)
        m = np.array(metas, np.uint64).copy()
        cut = int(m[-1, 0]) // 2
        m[-1, 0] -= cut
        bad = pages[:pages.size - cut].copy()
        cp = upload(gpu_ctx, col, bad, m)
        want = read_code(gpu_ctx, cp)
        oc = oracle_code(col, bad, m)
        assert want != 0 and oc != 0 and (oc is None or oc == want), (codec, want, oc)
        sel = np.random.default_rng(12).random(9000) < 0.5
        for mask in (sel, None):
            res = sb.key_ids(gpu_ctx, [cp], bitmap(gpu_ctx, mask), 128)
            with pytest.raises(NativeError) as e:
                gpu_ctx.synchronize()
            assert e.value.code == want, codec
            # rows and selected are delivered even when the interval failed
            assert res[0].rows == 9000 and res[0].selected == (9000 if mask is None else int(sel.sum()))
    # the context still works
    check(gpu_ctx, gen.prim(S.T_I64, 9000, uniq=60), max_page_size=3000, force_codec=S.DICT)


# ---- 16: a context whose read path holds launch hints
def test_on_a_context_that_holds_launch_hints(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd import read
    ctx = sb.Context(0)
    try:
        col = gen.prim(S.T_I64, 200_000, uniq=50, null_density=0.1, runs=40, seed=5)
        pages, metas = gen.oracle_write(col, max_page_size=65536, force_codec=S.RLE)
        plain = gen.prim(S.T_I64, 50_000, uniq=700, seed=6)
        pp, pm = gen.oracle_write(plain, max_page_size=65536, force_codec=S.NONE)
        ref, pref = K.Ref(col, pages, metas), K.Ref(plain, pp, pm)
        cp, pcp = upload(ctx, col, pages, metas), upload(ctx, plain, pp, pm)
        mask = np.random.default_rng(13).random(200_000) < 0.35
        for _ in range(3):   # the hints now say: RLE pages alone, no tiles
            read.read_simple(ctx, cp)
        r0 = ctx.replays()
        # a column of tiles: a read call would be issued again for it; this call goes by no hint
        run(ctx, [cp, pcp], [mask, None], [ref, pref], [64, 1024], [1, 2], what="behind reads")
        assert ctx.replays() == r0
        # ... and feeds none: the read path still holds "RLE pages alone", so the same RLE read is right without a replay,
        # and the first read of the column of tiles is the one that is issued again
        want, pwant = gen.oracle_read(col, pages, metas), gen.oracle_read(plain, pp, pm)
        got = read.read_simple(ctx, cp)
        assert np.array_equal(got.values_numpy(), want["values"]) and ctx.replays() == r0
        if os.environ.get("SB_NO_HINTS", "0") == "0":
            got = read.read_simple(ctx, pcp)
            assert np.array_equal(got.values_numpy(), pwant["values"]) and ctx.replays() == r0 + 1
    finally:
        ctx.close()
