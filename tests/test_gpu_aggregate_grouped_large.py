"""sb_aggregate_grouped_large and group_by on the GPU: pages written by the CPU oracle, count / min / max / sum of the selected
rows per group, up to 1024 groups, computed on the device and compared with the ORACLE's decode of the pages reduced per
group by numpy and Python (tests/aggregate_grouped_ref.py on tests/aggregate_ref.py, both unchanged).  Nothing here is
compared with what the device's own decoder or sb_aggregate_grouped give.

Integers, the counts and the bytes of min / max are compared exactly; a group's float sum over finite data must lie within
count_g * 2^-52 * sum_g|x| of math.fsum (aggregate_ref.float_sum_bound: derived, not measured).  Unless a test says otherwise
every column runs under a random ~0.35 selection, a sparse one that leaves whole tiles, chunks and pages out, and no
selection at all, as three columns of one call.  A chunk is 16 tiles of 4096 rows of a column: the rows that share one
table of the kernels (csrc/sb_aggregate_grouped_large.h)."""
import ctypes as C

import numpy as np
import pytest

from oracle import sbo as S
from tests import aggregate_grouped_ref as G
from tests import aggregate_ref as R
from tests import gen
from tests.test_gpu_aggregate import _column, _every_type_columns, _specials, bitmap
from tests.test_gpu_decode import LONG_RLE_ROWS, RLE_OVERSHOOT, _rle_page
from tests.test_gpu_read_selected import TYPES, oracle_code, read_code, to_dev, two_masks, upload

pytestmark = pytest.mark.gpu

NP = gen.NP_OF
SENTINEL = 0x5A
WORD = 0x5A5A5A5A5A5A5A5A
ID_DTYPE = {1: np.uint8, 2: np.uint16, 4: np.uint32}
TILE, CHUNK = 4096, 16 * 4096
EDGE_ROWS = (CHUNK - 1, CHUNK, CHUNK + 1, 33 * TILE + 5)


def ids_dev(ctx, ids, width=4):
    return to_dev(ctx, np.asarray(ids).astype(ID_DTYPE[width]))


def bits(res):
    """what must be the same every time: the sums' bits and the bytes of min / max of every group of every column"""
    return [[(g._c.sum_lo, g._c.sum_hi, g.min_bytes, g.max_bytes) for g in r.groups] for r in res]


def run(ctx, cps, masks, refs, ids, n_groups, ops=R.ALL, what="", width=4):
    """the columns of ONE call, each under its own selection (None: none), its own ids (or one array for all) and its own
    n_groups (or one for all), checked against their references"""
    import strawboat_amd as sb
    n = len(cps)
    ids_list = list(ids) if isinstance(ids, (list, tuple)) else [ids] * n
    ng_list = list(n_groups) if isinstance(n_groups, (list, tuple)) else [n_groups] * n
    shared = {}
    devs = [shared.setdefault(id(a), ids_dev(ctx, a, width)) for a in ids_list]
    res = sb.aggregate_grouped_large(ctx, cps, devs if isinstance(ids, (list, tuple)) else devs[0], ng_list,
                                     [bitmap(ctx, m) for m in masks], ops=ops)
    ctx.synchronize()
    wants = {}
    for i, (r, ref, m) in enumerate(zip(res, refs, masks)):
        key = (id(ref), id(ids_list[i]), ng_list[i], id(m))
        if key not in wants:   # (computed once per distinct column of the call)
            wants[key] = G.want(ref, ids_list[i], ng_list[i], m, ops)
        G.check(r, wants[key], "%s column %d" % (what, i))
    return res


def some_ids(rows, top, seed=0):
    return np.random.default_rng(2000 + seed).integers(0, top, rows)


def check_pages(ctx, col, pages, metas, ids=None, n_groups=1000, masks=None, ops=R.ALL, what="", width=4):
    ref = R.Ref(col, pages, metas)
    if masks is None:
        masks = two_masks(ref.rows, 11) + [None]
    if ids is None:
        ids = some_ids(ref.rows, n_groups + 3)
    cp = upload(ctx, col, pages, metas)
    return run(ctx, [cp] * len(masks), masks, [ref] * len(masks), ids, n_groups, ops, what, width)


def codecs_of(col, pages, metas):
    return set(int(x) for x in S.stat_column(col["ptype"], col["nullable"], pages, metas)[0].tolist())


def check(ctx, col, codec=None, ids=None, n_groups=1000, masks=None, ops=R.ALL, width=4, **opt):
    pages, metas = gen.oracle_write(col, **opt)
    if codec is not None:
        assert codecs_of(col, pages, metas) == {codec}, (codecs_of(col, pages, metas), codec)
    return check_pages(ctx, col, pages, metas, ids, n_groups, masks, ops, "codec %r %r" % (codec, opt), width)


# ---- 1: codecs x types
@pytest.mark.parametrize("ptype", TYPES)
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT, S.ONEVALUE])
def test_prim_codecs(gpu_ctx, ptype, codec):
    uniq = 1 if codec == S.ONEVALUE else 100
    for nd, page in ((0.2, 777), (None, 4100)):
        col = gen.prim(ptype, 10_000, uniq=uniq, null_density=nd, runs=8 if nd else 3, seed=page)
        check(gpu_ctx, col, codec=codec, n_groups=1000, max_page_size=page, force_codec=codec)


# ---- 2: the other codecs, 1024 groups
@pytest.mark.parametrize("ptype", [S.T_I32, S.T_U32])
@pytest.mark.parametrize("codec", [S.BITPACK, S.DELTABP])
def test_bitpacking(gpu_ctx, ptype, codec):
    col = gen.prim(ptype, 128 * 100, uniq=1 << 13, sorted_=(codec == S.DELTABP))
    check(gpu_ctx, col, codec=codec, n_groups=1024, max_page_size=128 * 40, force_codec=codec)


@pytest.mark.parametrize("icodec", [S.NONE, S.RLE, S.BITPACK, S.DELTABP, S.ONEVALUE, S.LZ4])
def test_dict_index_codecs(gpu_ctx, icodec):
    uniq = 1 if icodec == S.ONEVALUE else 200
    col = gen.prim(S.T_F64, 128 * 100, uniq=uniq, null_density=0.1, runs=16, sorted_=(icodec == S.DELTABP))
    check(gpu_ctx, col, codec=S.DICT, n_groups=1024, max_page_size=128 * 40, force_codec=S.DICT, force_index_codec=icodec)


@pytest.mark.parametrize("codec,ptype", [(S.LZ4, S.T_I16), (S.ZSTD, S.T_I64), (S.SNAPPY, S.T_F64)])
def test_basic_pages_are_staged(gpu_ctx, codec, ptype):
    col = gen.prim(ptype, 10_000, uniq=300, null_density=0.2, runs=5, seed=codec)
    check(gpu_ctx, col, codec=codec, n_groups=1024, max_page_size=2050, force_codec=codec)


def test_patas_pages(gpu_ctx):
    rng = np.random.default_rng(3)
    v = np.round(rng.normal(100, 20, 10_000), 2)
    col = dict(ptype=S.T_F64, nullable=True, rows=v.size, values=v, validity=gen.make_validity(rng, v.size, 0.2), offsets=None)
    check(gpu_ctx, col, codec=S.PATAS, n_groups=1024, max_page_size=2050, force_codec=S.PATAS)


# ---- 3: group-count edges
GROUP_COUNTS = (1, 255, 256, 257, 511, 512, 513, 1023, 1024)


@pytest.fixture(scope="module")
def shape_columns():
    out = []
    for ptype, codec, page in ((S.T_F64, S.NONE, 4100), (S.T_I64, S.RLE, 2050), (S.T_F32, S.DICT, 2048)):
        col = gen.prim(ptype, 10_000, uniq=100, null_density=0.2, runs=4, seed=page)
        pages, metas = gen.oracle_write(col, max_page_size=page, force_codec=codec)
        out.append((col, pages, metas, R.Ref(col, pages, metas)))
    return out


@pytest.mark.parametrize("n_groups", GROUP_COUNTS)
def test_group_count_edges(gpu_ctx, shape_columns, n_groups):
    """ids cover [0, n_groups + 3): every group has rows, the last one included, and three ids are out of range"""
    rows = 10_000
    rng = np.random.default_rng(n_groups)
    masks = two_masks(rows, 11) + [None]
    for k, (col, pages, metas, ref) in enumerate(shape_columns):
        ids = rng.integers(0, n_groups + 3, rows)
        ids[rng.permutation(rows)[:n_groups + 3]] = np.arange(n_groups + 3)
        cp = upload(gpu_ctx, col, pages, metas)
        res = run(gpu_ctx, [cp] * 3, masks, [ref] * 3, ids, n_groups, what="%d groups" % n_groups, width=2 if k % 2 else 4)
        assert res[2].out_of_range > 0 and all(g.selected > 0 for g in res[2].groups)


def test_one_byte_ids_with_1024_groups_and_n_groups_per_column(gpu_ctx, shape_columns):
    rows = 10_000
    rng = np.random.default_rng(7)
    masks = two_masks(rows, 11) + [None]
    col, pages, metas, ref = shape_columns[0]
    cp = upload(gpu_ctx, col, pages, metas)
    res = run(gpu_ctx, [cp] * 3, masks, [ref] * 3, rng.integers(0, 256, rows), 1024, what="one-byte ids", width=1)
    assert res[2].out_of_range == 0 and all(g.selected == 0 for g in res[2].groups[256:])
    # per-column n_groups and ids in one call: the records of a slot are gmax = 1024 apart, a column reads its own alone
    a, b, c = rng.integers(0, 5, rows), rng.integers(0, 260, rows), rng.integers(0, 1030, rows)
    cps = [upload(gpu_ctx, cl, p, m) for cl, p, m, _ in shape_columns]
    refs = [r for _, _, _, r in shape_columns]
    run(gpu_ctx, cps, [masks[0], None, masks[1]], refs, [a, b, c], [3, 257, 1024], what="n_groups per column")
    run(gpu_ctx, cps, [None, masks[0], masks[0]], refs, [c, a, b], [1024, 3, 257], what="n_groups per column, turned")


# ---- 4 .. 6: chunk edges
@pytest.fixture(scope="module")
def edge_columns():
    """rows -> [(col, pages, metas, ref)]: one Dict page and one plain page of each length, and for the longest the same rows
    in pages of 2050"""
    out = {}
    for rows in EDGE_ROWS:
        cases = []
        for ptype, codec in ((S.T_F64, S.DICT), (S.T_I64, S.NONE)):
            col = gen.prim(ptype, rows, uniq=500, null_density=0.1, runs=3, seed=rows % 1000)
            pages, metas = gen.oracle_write(col, max_page_size=1 << 20, force_codec=codec)
            assert metas.shape[0] == 1 and codecs_of(col, pages, metas) == {codec}
            cases.append((col, pages, metas, R.Ref(col, pages, metas)))
        out[rows] = cases
    col = out[EDGE_ROWS[-1]][0][0]
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.DICT)
    assert metas.shape[0] > 60 and int(metas[:, 1].max()) <= TILE
    out["short"] = [(col, pages, metas, R.Ref(col, pages, metas))]
    return out


@pytest.mark.parametrize("rows", EDGE_ROWS)
def test_chunk_edges_one_page(gpu_ctx, edge_columns, rows):
    ids = some_ids(rows, 303, rows)
    ids[rows - 1] = 299   # (the last row of the column has a group of its own)
    ids[:rows - 1][ids[:rows - 1] == 299] = 0
    for col, pages, metas, ref in edge_columns[rows]:
        cp = upload(gpu_ctx, col, pages, metas)
        res = run(gpu_ctx, [cp] * 3, two_masks(rows, 11) + [None], [ref] * 3, ids, 300, what="%d rows in one page" % rows, width=2)
        assert all(r.groups[299].selected == 1 for r in res[1:])   # (the sparse selection has the last row, like no selection)


def test_chunk_edges_short_pages(gpu_ctx, edge_columns):
    """one-tile pages, 16 to a chunk: the page of a tile is found from first_tile"""
    col, pages, metas, ref = edge_columns["short"][0]
    rows = ref.rows
    cp = upload(gpu_ctx, col, pages, metas)
    run(gpu_ctx, [cp] * 3, two_masks(rows, 11) + [None], [ref] * 3, some_ids(rows, 303, 5), 300, what="short pages", width=2)


def test_chunk_edges_selections(gpu_ctx, edge_columns):
    rows = EDGE_ROWS[-1]
    r = np.arange(rows)
    last = r == rows - 1                       # the only set bit is the last row: chunk 2 alone has a record
    every_second = (r // CHUNK) % 2 == 1       # chunks 0 and 2 are skipped entirely
    one_per_chunk = (r % CHUNK) == 4097        # exactly one row per chunk (none in the 5-row chunk's tile: chunk 2 has tile 32)
    assert one_per_chunk.sum() == 3 and every_second.sum() == CHUNK
    ids = some_ids(rows, 303, 6)
    for col, pages, metas, ref in edge_columns[rows] + edge_columns["short"]:
        cp = upload(gpu_ctx, col, pages, metas)
        res = run(gpu_ctx, [cp] * 3, [last, every_second, one_per_chunk], [ref] * 3, ids, 300, what="chunk selections")
        assert [x.selected for x in res] == [1, CHUNK, 3]


# ---- 7: RLE and non-RLE pages of one column within one chunk
def test_mixed_routes_in_a_chunk(gpu_ctx):
    """the adaptive writer gives a column of long runs and of noise, page by page, RLE pages and others: the tiles of the RLE
    pages are passed over by the chunk's walk and reduced by the page walk"""
    rng = np.random.default_rng(12)
    page, n_pages = 4096, 12
    parts = []
    for p in range(n_pages):
        if p % 3 == 1:
            parts.append(rng.integers(-10 ** 12, 10 ** 12, page))
        else:
            parts.append(np.repeat(rng.integers(-1000, 1000, page // 512), 512))
    v = np.concatenate(parts).astype(np.int64)
    rows = v.size
    col = _column(S.T_I64, v, rng.random(rows) >= 0.1)
    pages, metas = gen.oracle_write(col, max_page_size=page, ratio=2.0, forbidden=(S.DICT,))   # (no forced codec: chosen page by page)
    seen = codecs_of(col, pages, metas)
    assert len(seen) >= 2 and S.RLE in seen, seen
    assert rows < CHUNK   # (one chunk)
    check_pages(gpu_ctx, col, pages, metas, n_groups=700, what="mixed routes")


# ---- 8: a long RLE page: several workgroups share it
@pytest.mark.parametrize("ptype", [S.T_F64, S.T_I64])
def test_long_rle_page(gpu_ctx, ptype):
    rng = np.random.default_rng(ptype)
    ids = np.repeat(rng.integers(0, 1024, LONG_RLE_ROWS // 100 + 1), 100)[:LONG_RLE_ROWS]
    ids[::4099] = 1027   # (out of range)
    col = gen.prim(ptype, LONG_RLE_ROWS, uniq=256, null_density=0.1, runs=32, seed=4 + ptype)
    pages, metas = gen.oracle_write(col, force_codec=S.RLE)
    assert metas.shape[0] == 1 and codecs_of(col, pages, metas) == {S.RLE}
    res = check_pages(gpu_ctx, col, pages, metas, ids, 1024, [rng.random(LONG_RLE_ROWS) < 0.01, None], what="long RLE page", width=2)
    assert res[1].out_of_range == len(range(0, LONG_RLE_ROWS, 4099))


# ---- 9: count alone works on every type
def test_count_only_on_every_type(gpu_ctx):
    rng = np.random.default_rng(8)
    ids = rng.integers(0, 603, 3000)
    for col in _every_type_columns():
        pages, metas = gen.oracle_write(col, max_page_size=777)
        ref = R.Ref(col, pages, metas)
        cp = upload(gpu_ctx, col, pages, metas)
        masks = [rng.random(3000) < 0.35, two_masks(3000, 3)[1], None]
        for ops in (("count",), ()):
            res = run(gpu_ctx, [cp] * 3, masks, [ref] * 3, ids, 600, ops=ops, what="count only, type %d" % col["ptype"], width=2)
            assert all(g.min is None and g.max is None and g.sum is None for r in res for g in r.groups)
        if col["ptype"] == S.T_NULL:
            assert sum(g.count for g in res[2].groups) == 0 and sum(g.selected for g in res[2].groups) + res[2].out_of_range == 3000


# ---- 10: 128-bit sums and float specials
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_extremes(gpu_ctx, codec):
    rng = np.random.default_rng(codec + 7)
    rows = 10_000
    opt = dict(max_page_size=4100, force_codec=codec)
    runs = np.repeat(np.arange(rows // 5 + 1), 5)[:rows]
    # all in group 1023: INT64 min repeated, the 64-bit sum wraps, the 128-bit sum does not
    ids = np.full(rows, 1023)
    res = check(gpu_ctx, _column(S.T_I64, np.full(rows, -2 ** 63), rng.random(rows) >= 0.2), codec=codec, ids=ids, n_groups=1024, **opt)
    g = res[2].groups[1023]
    assert g.sum == -2 ** 63 * g.count < -2 ** 64 * 3000 and g.min == g.max == -2 ** 63
    res = check(gpu_ctx, _column(S.T_U64, np.full(rows, 2 ** 64 - 1, np.uint64), rng.random(rows) >= 0.1), codec=codec, ids=ids, n_groups=1024, **opt)
    g = res[2].groups[1023]
    assert g.sum == (2 ** 64 - 1) * g.count > 2 ** 64 * 8000 and g.min == g.max == 2 ** 64 - 1
    # spread over 1024 groups: min, max and small values by the id's remainder
    ids = rng.integers(0, 1024, rows)[runs]
    v = np.where(ids % 3 == 0, -2 ** 63, np.where(ids % 3 == 1, 2 ** 63 - 1, rng.integers(-5, 5, rows)[runs])).astype(np.int64)
    res = check(gpu_ctx, _column(S.T_I64, v, rng.random(rows) >= 0.2), codec=codec, ids=ids, n_groups=1024, **opt)
    assert any(g.sum < -2 ** 64 for g in res[2].groups) and any(g.sum > 2 ** 64 for g in res[2].groups)
    v = np.where(ids % 2 == 0, np.uint64(2 ** 64 - 1), rng.integers(0, 50, rows)[runs].astype(np.uint64))
    res = check(gpu_ctx, _column(S.T_U64, v, rng.random(rows) >= 0.1), codec=codec, ids=ids, n_groups=1024, **opt)
    assert any(g.sum > 2 ** 66 for g in res[2].groups)


@pytest.mark.parametrize("ptype", [S.T_F32, S.T_F64])
@pytest.mark.parametrize("codec", [S.NONE, S.RLE, S.DICT])
def test_float_specials(gpu_ctx, ptype, codec):
    """group 1000: NaNs of both signs among finite rows; 1001: +inf; 1002: -inf; 1003: the zeros alone; 1004: NaNs alone;
    the rest: finite rows"""
    dtype = NP[ptype]
    rng = np.random.default_rng(ptype)
    rows = 10_000
    v = np.repeat(rng.normal(0, 50, rows // 4 + 1), 4)[:rows].astype(dtype)
    nan, nan_neg, inf, ninf, zero, nzero, tiny, ntiny = _specials(dtype)
    ids = rng.integers(0, 1000, rows)
    ids[rng.random(rows) < 0.2] = 1000
    ids[rng.random(rows) < 0.1] = 1001
    ids[rng.random(rows) < 0.1] = 1002
    special = np.zeros(rows, bool)
    for at, value, group in (([10, 4097, 9000], nan, 1000), ([11, 8300], nan_neg, 1000), ([500, 4095], inf, 1001), ([4096], ninf, 1002),
                             ([20, 21, 22], zero, 1003), ([23, 24], nzero, 1003), ([30, 31, 5000], nan, 1004), ([32], nan_neg, 1004),
                             ([40], tiny, 1005), ([41], ntiny, 1005)):
        v[at] = value
        ids[at] = group
        special[at] = True
    valid = rng.random(rows) >= 0.1
    valid[special] = True
    col = _column(ptype, v, valid)
    pages, metas = gen.oracle_write(col, max_page_size=4100, force_codec=codec)
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    masks = [special | (rng.random(rows) < 0.3), None]
    res = run(gpu_ctx, [cp] * 2, masks, [ref] * 2, ids, 1024, what="float specials")
    w = np.dtype(dtype).itemsize
    for r in res:
        g = r.groups
        assert g[1000].nans == 5 and g[1000].sum != g[1000].sum and g[1000].min is not None
        assert g[1001].sum == np.inf and g[1001].max == np.inf and g[1002].sum == -np.inf and g[1002].min == -np.inf
        assert g[1003].count == 5 and g[1003].sum == 0.0
        if np.signbit(ref.vals[23]) and not np.signbit(ref.vals[20]):   # (the pages kept the zeros' signs)
            assert g[1003].min_bytes[:w] == dtype(-0.0).tobytes() and g[1003].max_bytes[:w] == dtype(0.0).tobytes()
        assert g[1004].count == 4 and g[1004].nans == 4 and g[1004].min is None and g[1004].sum != g[1004].sum
        assert g[1004].min_bytes == g[1004].max_bytes == bytes(8)
        assert g[1005].nans == 0 and np.isfinite(g[1005].sum)


# ---- 11: Freq pages: the interval is issued again, the column that met one is decoded
def _freq_case(ctx, ptype, rows=10_000):
    from tests.test_gpu_freq import sparse
    f = sparse(ptype, rows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    assert S.FREQ in codecs_of(f, fp, fm)
    b = gen.prim(S.T_F64, rows, uniq=100, null_density=0.2, runs=6, seed=2)
    bp, bm = gen.oracle_write(b, max_page_size=4100, force_codec=S.RLE)
    assert codecs_of(b, bp, bm) == {S.RLE}
    return (R.Ref(f, fp, fm), upload(ctx, f, fp, fm)), (R.Ref(b, bp, bm), upload(ctx, b, bp, bm))


@pytest.mark.parametrize("ptype", [S.T_I32, S.T_I64])
def test_freq_pages(gpu_ctx, ptype):
    import strawboat_amd as sb
    rows = 10_000
    (fref, fcp), (bref, bcp) = _freq_case(gpu_ctx, ptype)
    mask = np.random.default_rng(ptype).random(rows) < 0.3
    ids = some_ids(rows, 703)
    r0 = gpu_ctx.replays()
    res = run(gpu_ctx, [fcp, bcp, fcp], [mask, mask, None], [fref, bref, fref], ids, 700, what="freq")
    assert gpu_ctx.replays() == r0 + 1
    # the column without a Freq page stays on the page route in the replay: the bits of a call of its own
    r0 = gpu_ctx.replays()
    alone = run(gpu_ctx, [bcp], [mask], [bref], ids, 700, what="the RLE column alone")
    assert gpu_ctx.replays() == r0
    assert bits(alone) == bits(res[1:2])
    # a Freq column without a selected row: the replay all the same
    r0 = gpu_ctx.replays()
    run(gpu_ctx, [fcp, bcp], [np.zeros(rows, bool), mask], [fref, bref], ids, [700, 1024], what="freq, nothing selected")
    assert gpu_ctx.replays() == r0 + 1
    # count alone looks at no page body: no replay
    r0 = gpu_ctx.replays()
    run(gpu_ctx, [fcp], [mask], [fref], ids, 700, ops=("count",), what="freq, count only")
    assert gpu_ctx.replays() == r0
    # an interval that holds both kinds of call, each with a Freq column and a column without: the marks are kept apart
    dev = ids_dev(gpu_ctx, ids)
    bmp = bitmap(gpu_ctx, mask)
    r0 = gpu_ctx.replays()
    small = sb.aggregate_grouped(gpu_ctx, [fcp, bcp], dev, 256, bmp)
    large = sb.aggregate_grouped_large(gpu_ctx, [bcp, fcp], dev, 700, bmp)
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    G.check(small[0], G.want(fref, ids, 256, mask), "the 256-group call's Freq column")
    G.check(small[1], G.want(bref, ids, 256, mask), "the 256-group call's RLE column")
    G.check(large[1], G.want(fref, ids, 700, mask), "the large call's Freq column")
    G.check(large[0], G.want(bref, ids, 700, mask), "the large call's RLE column")
    assert bits(large[:1]) == bits(alone)


def test_the_256_group_calls_freq_test_next_to_a_large_call(gpu_ctx):
    """tests/test_gpu_aggregate_grouped.py::test_freq_pages, issued in intervals that hold a large call as well"""
    import strawboat_amd as sb
    from tests import test_gpu_aggregate_grouped as T
    rows = 10_000
    _, (bref, bcp) = _freq_case(gpu_ctx, S.T_I64)
    ids = some_ids(rows, 703)
    dev = ids_dev(gpu_ctx, ids)
    pending = []

    class Both:   # the context T.run sees: every synchronize of the 256-group test ends an interval that holds a large call too
        def __getattr__(self, name):
            return getattr(gpu_ctx, name)

        def synchronize(self):
            # (a column without a Freq page: the large call asks for no replay of its own, so the test's replay counts hold)
            pending.append(sb.aggregate_grouped_large(gpu_ctx, [bcp], dev, 700, None))
            gpu_ctx.synchronize()

    T.test_freq_pages(Both(), S.T_I64)
    assert len(pending) == 4
    G.check(pending[0][0], G.want(bref, ids, 700, None), "the large call's RLE column")
    # replayed on the 256-group call's account or not: the column stayed on the page route, the same bits
    assert all(bits(res) == bits(pending[0]) for res in pending)


# ---- 12: the order of the float additions: the same bits every time, a replayed interval included
@pytest.mark.parametrize("n_groups", [300, 1024])
@pytest.mark.parametrize("ptype,codec", [(S.T_F64, S.NONE), (S.T_F32, S.DICT), (S.T_F64, S.RLE)])
def test_float_sums_that_are_exact_in_no_order(gpu_ctx, ptype, codec, n_groups):
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows = 3 * CHUNK // 2 + 77   # (two chunks on the tile route)
    v, ids = G.inexact_values(rows, n_groups, seed=17)
    rng = np.random.default_rng(codec * 10 + ptype)
    col = _column(ptype, v.astype(NP[ptype]), rng.random(rows) >= 0.1)
    pages, metas = gen.oracle_write(col, max_page_size=2050 * 9, force_codec=codec)
    assert codecs_of(col, pages, metas) == {codec}
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    masks = two_masks(rows, 11) + [None]
    res = run(gpu_ctx, [cp] * 3, masks, [ref] * 3, ids, n_groups, what="inexact float sums")
    first = bits(res)
    # the same call three times in fresh intervals
    dev = ids_dev(gpu_ctx, ids)
    bitmaps = [bitmap(gpu_ctx, m) for m in masks]
    batch = sb.GroupedAggregateLargeBatch(gpu_ctx, [cp] * 3, dev, n_groups, bitmaps)
    for _ in range(3):
        again = batch.enqueue()
        gpu_ctx.synchronize()
        assert bits(again) == first
    # ... and the unchanged call in intervals that are issued again on another call's account: a filter on a Freq column, a
    # 256-group call on a Freq column, a large call on one
    frows = 10_000
    f = sparse(S.T_I64, frows, 0.05, 2, null_density=0.1)
    fp, fm = gen.oracle_write(f, max_page_size=2050, force_codec=S.FREQ)
    fcp = upload(gpu_ctx, f, fp, fm)
    fref = R.Ref(f, fp, fm)
    fids = some_ids(frows, 200)
    fdev = ids_dev(gpu_ctx, fids)
    fwant = {}
    for others in ("filter", "grouped", "large"):
        r0 = gpu_ctx.replays()
        if others == "filter":
            sb.filter_columns(gpu_ctx, [fcp], [sb.Predicate("ne", 7)])
        elif others == "grouped":
            fres = sb.aggregate_grouped(gpu_ctx, [fcp], fdev, 200, None)
        else:
            fres = sb.aggregate_grouped_large(gpu_ctx, [fcp], fdev, 200, None)
        again = batch.enqueue()
        gpu_ctx.synchronize()
        assert gpu_ctx.replays() == r0 + 1, others
        assert bits(again) == first, others
        if others != "filter":
            fwant.setdefault(0, G.want(fref, fids, 200, None))
            G.check(fres[0], fwant[0], "the Freq column next to it (%s)" % others)
    # ... and as columns of one call with a Freq column: the Freq column is decoded, the others stay where they were
    r0 = gpu_ctx.replays()
    both = sb.GroupedAggregateLargeBatch(gpu_ctx, [cp] * 3 + [fcp], [dev] * 3 + [fdev], [n_groups] * 3 + [200], bitmaps + [None]).enqueue()
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    assert bits(both[:3]) == first
    G.check(both[3], fwant[0], "the Freq column of the call")


# ---- 13: errors
def _raw_array(ctx, cps, bitmaps, dev_ids, n_groups, ops, extra=0):
    """a batch whose result fields and `groups` records (n_groups + extra of them) hold a sentinel"""
    from strawboat_amd import _native as N
    from strawboat_amd.aggregate_grouped_large import GroupedAggregateLargeBatch
    batch = GroupedAggregateLargeBatch(ctx, cps, dev_ids, n_groups, bitmaps, ops=("count",))
    batch._garrs = []
    for i in range(len(cps)):
        batch._arr[i].ops = ops
        batch.results[i].ops = ops
        for f in ("rows", "selected", "out_of_range"):
            setattr(batch._arr[i], f, WORD)
        garr = (N.AggGroupC * (n_groups + extra))()
        C.memset(garr, SENTINEL, 64 * (n_groups + extra))
        batch._garrs.append(garr)
        batch._arr[i].groups = garr
    return batch


def _sentinels_kept(batch):
    for c, garr in zip(batch._arr, batch._garrs):
        assert all(getattr(c, f) == WORD for f in ("rows", "selected", "out_of_range"))
        assert bytes(garr) == bytes([SENTINEL]) * C.sizeof(garr)


def test_refusals_at_the_call(gpu_ctx):
    from strawboat_amd import _native as N
    rows = 5000
    col = gen.prim(S.T_I64, rows, uniq=10, null_density=0.2)
    pages, metas = gen.oracle_write(col, max_page_size=2050, force_codec=S.NONE)
    ref = R.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(9).random(rows) < 0.5
    bm = bitmap(gpu_ctx, mask)
    ids = some_ids(rows, 600)
    dev = ids_dev(gpu_ctx, ids, 4)
    boolean = gen.boolean(rows)
    bpages, bmetas = gen.oracle_write(boolean)
    bcp = upload(gpu_ctx, boolean, bpages, bmetas)
    binary = gen.binary(rows, uniq=20)
    npages, nmetas = gen.oracle_write(binary)
    ncp = upload(gpu_ctx, binary, npages, nmetas)

    def fresh(cps=None):
        return _raw_array(gpu_ctx, cps or [cp, cp], [bm, bm], dev, 600, 15)

    def refused(batch, code, what, mem=N.SB_MEM_DEVICE):
        assert gpu_ctx._lib.sb_aggregate_grouped_large(gpu_ctx._h, batch._arr, 2, mem) == code, what
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        _sentinels_kept(batch)

    def tweak(what, code=N.SB_ERR_INVALID, col=1, **fields):
        batch = fresh()
        for f, v in fields.items():
            setattr(batch._arr[col], f, v)
        refused(batch, code, what)

    for n_groups in (0, 1025, 1 << 16):
        tweak("n_groups %d" % n_groups, n_groups=n_groups)
    for width in (0, 3, 8):
        tweak("group_id_width %d" % width, group_id_width=width)
    tweak("group_ids null with rows > 0", group_ids=None)
    tweak("group_ids misaligned", group_ids=dev.data_ptr() + 2)
    tweak("group_ids misaligned, width 2", group_ids=dev.data_ptr() + 1, group_id_width=2)
    tweak("group_ids too short", group_ids_capacity=rows * 4 - 1)
    tweak("groups null", groups=None)
    tweak("unknown ops bits", ops=16 | 1)
    tweak("reserved != 0", reserved=1)
    tweak("misaligned selection", selection=bm.data_ptr() + 1)
    for other in (bcp, ncp):
        for ops in (N.SB_AGG_MIN, N.SB_AGG_MAX, N.SB_AGG_SUM, 15):
            batch = fresh([cp, other])
            batch._arr[1].ops = ops
            refused(batch, N.SB_ERR_NYI, "min / max / sum on Boolean / Binary")
    refused(fresh(), N.SB_ERR_NYI, "SB_MEM_HOST", mem=N.SB_MEM_HOST)
    # the 256-group call still refuses 257 groups, and what it refuses this call takes
    batch = fresh()
    batch._arr[0].n_groups = batch._arr[1].n_groups = 257
    assert gpu_ctx._lib.sb_aggregate_grouped(gpu_ctx._h, batch._arr, 2, N.SB_MEM_DEVICE) == N.SB_ERR_INVALID
    gpu_ctx.synchronize()
    _sentinels_kept(batch)
    # the batch as it was built then succeeds; a `groups` array longer than n_groups keeps its sentinel behind record n_groups
    batch = _raw_array(gpu_ctx, [cp, cp], [bm, None], dev, 600, 15, extra=3)
    assert gpu_ctx._lib.sb_aggregate_grouped_large(gpu_ctx._h, batch._arr, 2, N.SB_MEM_DEVICE) == 0
    gpu_ctx.synchronize()
    from strawboat_amd.aggregate_grouped import GroupedAggregate
    for c, garr, m in zip(batch._arr, batch._garrs, (mask, None)):
        assert bytes(garr)[64 * 600:] == bytes([SENTINEL]) * (64 * 3)
        got = GroupedAggregate(col["ptype"], 15, c, [garr[i] for i in range(600)])
        G.check(got, G.want(ref, ids, 600, m), "after the refusals")


def test_corrupt_pages_raise_what_the_decoder_raises(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError

    def code_of(cp, rows, sel):
        try:
            sb.aggregate_grouped_large(gpu_ctx, [cp], ids_dev(gpu_ctx, np.arange(rows) % 1000, 2), 1000,
                                       bitmap(gpu_ctx, np.ones(rows, bool)) if sel else None)
            gpu_ctx.synchronize()
        except NativeError as e:
            try:
                gpu_ctx.synchronize()
            except NativeError:
                pass
            return e.code
        return 0

    for codec in (S.NONE, S.RLE, S.DICT, S.LZ4):   # a truncated last page
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
        assert code_of(cp, 9000, True) == want, codec
        assert code_of(cp, 9000, False) == want, codec
    # a Dict page with an index >= D on a live row: plain u32 indices behind hdr9 Dict | hdr9 None
    col = gen.prim(S.T_I64, 40_000, uniq=50, seed=50)
    pages, metas = gen.oracle_write(col, max_page_size=40_000, force_codec=S.DICT, force_index_codec=S.NONE)
    bad = pages.copy()
    pos = 9 + 9 + 25_000 * 4
    bad[pos:pos + 4] = np.frombuffer(np.uint32(1 << 30).tobytes(), np.uint8)
    cp = upload(gpu_ctx, col, bad, metas)
    assert read_code(gpu_ctx, cp) == -1 and oracle_code(col, bad, metas) != 0
    assert code_of(cp, 40_000, True) == -1
    # a hand-built RLE page whose run overshoots the page; rows and selected are delivered even when the interval failed
    ptype, dtype, w, runs, rows = RLE_OVERSHOOT
    page = _rle_page(runs, w, dtype).copy()
    cp = upload(gpu_ctx, dict(ptype=ptype, nullable=False), page, np.array([[page.size, rows]], np.uint64))
    assert read_code(gpu_ctx, cp) == -1 and code_of(cp, rows, True) == -1
    sel = np.random.default_rng(12).random(rows) < 0.5
    res = sb.aggregate_grouped_large(gpu_ctx, [cp], ids_dev(gpu_ctx, np.arange(rows) % 3, 1), 1024, bitmap(gpu_ctx, sel))
    with pytest.raises(NativeError):
        gpu_ctx.synchronize()
    assert res[0].rows == rows and res[0].selected == int(sel.sum())
    # the context still works
    check(gpu_ctx, gen.prim(S.T_I64, 9000, uniq=60), n_groups=1024, max_page_size=3000, force_codec=S.DICT)


# ---- 14: group_by: filter, key ids and the aggregates in one interval
def _dict_group_by(keys, key_valid, mask, refs):
    """{key: (selected rows, [live values per value column])} by a Python dict over the oracle's decodes"""
    groups = {}
    for i in np.flatnonzero(mask & key_valid):
        g = groups.setdefault(keys[i], [0, [[] for _ in refs]])
        g[0] += 1
        for j, r in enumerate(refs):
            if r.valid[i]:
                g[1][j].append(r.vals[i].item())
    return groups


def _check_group_by(kres, aggs, groups, mask, key_valid, refs, max_keys):
    import math
    from strawboat_amd.group_by import trim
    order = sorted(groups)
    assert not kres.overflow and kres.n_keys == len(order)
    assert list(kres.keys.tolist() if hasattr(kres.keys, "tolist") else kres.keys) == order
    trimmed = trim(kres, aggs)
    for j, (a, r) in enumerate(zip(aggs, refs)):
        assert len(a.groups) == max_keys and len(trimmed[j]) == len(order)
        assert a.selected == int(mask.sum()) and a.out_of_range == int((mask & ~key_valid).sum())
        for g, key in enumerate(order):
            n_sel, live = groups[key]
            got = trimmed[j][g]
            assert (got.selected, got.count) == (n_sel, len(live[j])), (j, g)
            if live[j] and r.ptype == S.T_F64:
                f = math.fsum(live[j])
                assert (got.min, got.max) == (min(live[j]), max(live[j])), (j, g)
                assert abs(got.sum - f) <= len(live[j]) * 2.0 ** -52 * math.fsum(abs(x) for x in live[j]), (j, g)
            elif live[j]:
                assert (got.min, got.max, got.sum) == (min(live[j]), max(live[j]), sum(live[j])), (j, g)
        for g in range(len(order), max_keys):
            assert bytes(a.groups[g]._c) == bytes(64), (j, g)


@pytest.fixture(scope="module")
def group_by_columns():
    rows = 20_011
    x = gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    y = gen.prim(S.T_I64, rows, uniq=5000, null_density=0.1, seed=2)
    z = gen.prim(S.T_F64, rows, uniq=3000, null_density=0.2, runs=3, seed=3)
    out = {"rows": rows}
    for name, col, codec, page in (("x", x, S.RLE, 2050), ("y", y, S.NONE, 4100), ("z", z, S.DICT, 2050)):
        pages, metas = gen.oracle_write(col, max_page_size=page, force_codec=codec)
        out[name] = (col, pages, metas, R.Ref(col, pages, metas))
    return out


@pytest.mark.parametrize("distinct,max_keys", [(700, 1024), (150, 200)])
def test_group_by_an_integer_key(gpu_ctx, group_by_columns, distinct, max_keys):
    """700 sparse keys: the large call; 150 keys under max_keys 200: the 256-group call"""
    import strawboat_amd as sb
    from tests.key_ids_ref import Ref as KeyRef
    rows = group_by_columns["rows"]
    rng = np.random.default_rng(distinct)
    pool = rng.choice(np.arange(-10 ** 15, 10 ** 15, 10 ** 9 + 7), distinct, replace=False)
    kv = pool[rng.integers(0, distinct, rows)]
    kv[rng.permutation(rows)[:distinct]] = pool
    k = _column(S.T_I64, kv, rng.random(rows) >= 0.1)
    kp, km = gen.oracle_write(k, max_page_size=4100)
    kr = KeyRef(k, kp, km)
    (x, xp, xm, xr), (y, yp, ym, yr), (z, zp, zm, zr) = (group_by_columns[n] for n in "xyz")
    mask = (xr.vals < 60) & xr.valid
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("lt", 60)])
    kres, aggs = sb.group_by(gpu_ctx, upload(gpu_ctx, k, kp, km), [upload(gpu_ctx, y, yp, ym), upload(gpu_ctx, z, zp, zm)], sel[0],
                             max_keys=max_keys)
    gpu_ctx.synchronize()   # (the only one)
    assert np.array_equal(sel[0].numpy(), mask)
    groups = _dict_group_by(kr.vals.tolist(), kr.valid, mask, [yr, zr])
    assert len(groups) > 0.9 * distinct
    _check_group_by(kres, aggs, groups, mask, kr.valid, [yr, zr], max_keys)


def test_group_by_a_utf8_key_and_an_overflow(gpu_ctx, group_by_columns):
    import strawboat_amd as sb
    from strawboat_amd.group_by import trim
    from tests import key_ids_var_ref as K
    from tests.test_gpu_key_ids_var import pick, vocab
    rows = group_by_columns["rows"]
    rng = np.random.default_rng(4)
    voc = vocab(400, 10, maxlen=20)
    k = K.column(pick(voc, rows, 10), rng.random(rows) >= 0.15)
    kp, km = gen.oracle_write(k, max_page_size=4100)
    kr = K.Ref(k, kp, km)
    (x, xp, xm, xr), (y, yp, ym, yr), (z, zp, zm, zr) = (group_by_columns[n] for n in "xyz")
    mask = (xr.vals < 60) & xr.valid
    kcp = upload(gpu_ctx, k, kp, km)
    vcps = [upload(gpu_ctx, y, yp, ym), upload(gpu_ctx, z, zp, zm)]
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("lt", 60)])
    kres, aggs = sb.group_by(gpu_ctx, kcp, vcps, sel[0], max_keys=1024)
    gpu_ctx.synchronize()
    assert np.array_equal(sel[0].numpy(), mask)
    groups = _dict_group_by(kr.strs, kr.valid, mask, [yr, zr])
    assert len(groups) == 400
    _check_group_by(kres, aggs, groups, mask, kr.valid, [yr, zr], 1024)
    # more keys than max_keys: the overflow is passed through, not raised; trim refuses
    kres, aggs = sb.group_by(gpu_ctx, kcp, vcps, None, max_keys=300)
    gpu_ctx.synchronize()
    assert kres.overflow and aggs[0].rows == rows and len(aggs[0].groups) == 300
    with pytest.raises(ValueError):
        trim(kres, aggs)
