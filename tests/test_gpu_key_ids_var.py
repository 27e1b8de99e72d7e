"""sb_key_ids_var on the GPU: pages of Binary / LargeBinary columns written by the CPU oracle, the distinct keys and the dense
ids found on the device, compared with the ORACLE's decode of the pages under np.unique(..., return_inverse=True) on an
object array of bytes (tests/key_ids_var_ref.py, checked on its own against a dict-based group-by in
tests/test_key_ids_var_host.py).  Nothing here is compared with what the device's own decoder gives.

Every comparison is exact: the keys, key_offsets, the bytes of `keys`, every id, and rows / selected / count / n_keys /
keys_len / overflow.  Unless a test says otherwise a column has about 10 000 rows and runs with no selection, under a random
selection of about 30 % and under a selection that leaves no row; the forced codec is asserted from S.stat_column.  The
vocabularies are built here so that the strings are distinct; null rows keep their bytes."""
import ctypes as C

import numpy as np
import pytest

from oracle import sbo as S
from tests import gen
from tests import key_ids_var_ref as K
from tests.test_gpu_aggregate import bitmap
from tests.test_gpu_read_selected import oracle_code, read_code, to_dev, upload

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_BYTES = 4096
WORD = 0x5A5A5A5A5A5A5A5A
RESULTS = ("rows", "selected", "count", "n_keys", "keys_len", "overflow")


def three_masks(rows, seed):
    """no selection, a random one of about 30 %, and one that leaves no row"""
    return [None, np.random.default_rng(seed).random(rows) < 0.3, np.zeros(rows, bool)]


def vocab(n, seed=0, minlen=0, maxlen=40):
    """n distinct strings of minlen .. maxlen bytes, bytes >= 0x80 and zero bytes among them; the empty string when minlen == 0"""
    rng = np.random.default_rng(seed)
    out = {}
    if minlen == 0:
        out[b""] = True
    while len(out) < n:
        L = int(rng.integers(max(minlen, 1), maxlen + 1))
        body = ("w%d:" % len(out)).encode()[:L]   # (the counter makes long strings distinct; short ones are drawn again)
        tail = bytes(rng.integers(0, 256, L - len(body), dtype=np.uint8)) if L > len(body) and len(out) % 3 == 0 else b"x" * (L - len(body))
        out[body + tail] = True
    return list(out)[:n]


def pick(voc, rows, seed, runs=1, each=True):
    """`rows` strings drawn from voc, in runs of `runs`; each: every string of voc is there at least once"""
    rng = np.random.default_rng(seed)
    idx = np.repeat(rng.integers(0, len(voc), (rows + runs - 1) // runs), runs)[:rows]
    if each:
        idx[rng.permutation(rows)[:len(voc)]] = np.arange(len(voc))
    return [voc[i] for i in idx]


def validity(rows, nd, seed):
    return None if nd is None else np.random.default_rng(seed).random(rows) >= nd


def write(col, codec, icodec=None, **opt):
    pages, metas = gen.oracle_write(col, **opt)
    st = S.stat_column(col["ptype"], col["nullable"], pages, metas)
    seen = set(int(x) for x in st[0].tolist())
    assert seen == {codec}, (seen, codec)
    if icodec is not None:
        inner = set(int(x) for x in st[1].tolist())
        assert inner == {icodec}, (inner, icodec)
    return pages, metas


def run(ctx, cps, masks, refs, max_keys, id_widths, key_bytes=None, what=""):
    """the columns of ONE call, each under its own selection (None: no selection), max_keys, id_width and keys_capacity"""
    import strawboat_amd as sb
    kbs = [65536] * len(cps) if key_bytes is None else list(key_bytes)
    res = sb.key_ids_var(ctx, cps, [bitmap(ctx, m) for m in masks], list(max_keys), list(id_widths), kbs)
    ctx.synchronize()
    for i, (r, ref, m, mk, w, kb) in enumerate(zip(res, refs, masks, max_keys, id_widths, kbs)):
        K.check(r, K.want(ref, m, mk, w, kb), "%s column %d (max_keys %d, id_width %d, keys_capacity %d)" % (what, i, mk, w, kb))
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
               [c[1] for c in combos], what=what)


# ---- 1: codecs x {Binary, LargeBinary}
CODECS = [("none", S.NONE), ("lz4", S.LZ4), ("zstd", S.ZSTD), ("snappy", S.SNAPPY), ("dict", S.DICT), ("freq", S.FREQ), ("onevalue", S.ONEVALUE)]


def codec_strings(codec, rows, seed):
    voc = vocab(100, seed)
    if codec == S.ONEVALUE:
        return [voc[7]] * rows
    if codec == S.FREQ:   # one frequent value, the others its exceptions
        rng = np.random.default_rng(seed)
        idx = np.where(rng.random(rows) < 0.95, 5, rng.integers(0, 100, rows))
        idx[rng.permutation(rows)[:100]] = np.arange(100)
        return [voc[i] for i in idx]
    return pick(voc, rows, seed, runs=3)


@pytest.mark.parametrize("large", [False, True], ids=["binary", "large"])
@pytest.mark.parametrize("name,codec", CODECS, ids=[c[0] for c in CODECS])
def test_codecs(gpu_ctx, name, codec, large):
    for nd, page in ((0.2, 2050), (None, 4100), (0.2, 777), (None, 2048)):
        col = K.column(codec_strings(codec, 10_000, page), validity(10_000, nd, page), large)
        pages, metas = write(col, codec, max_page_size=page, force_codec=codec)
        res = check_pages(gpu_ctx, col, pages, metas, what="%s %d" % (name, page))
        assert not res[0].overflow and res[0].n_keys == (1 if codec == S.ONEVALUE else 100) and res[-1].n_keys == 0


# ---- 2: the index codecs of Dict pages
@pytest.mark.parametrize("icodec", [S.NONE, S.RLE, S.BITPACK, S.DELTABP, S.ONEVALUE, S.LZ4])
def test_dict_index_codecs(gpu_ctx, icodec):
    rows = 128 * 100
    voc = vocab(200, 2, maxlen=24)
    if icodec == S.ONEVALUE:
        strs = [voc[3]] * rows
    elif icodec == S.DELTABP:   # the entries in the order of their first row: ascending indices
        strs = [voc[i * 200 // rows] for i in range(rows)]
    else:
        strs = pick(voc, rows, 3, runs=16 if icodec == S.RLE else 1)
    col = K.column(strs, validity(rows, 0.1, 4))
    pages, metas = write(col, S.DICT, icodec, max_page_size=128 * 40, force_codec=S.DICT, force_index_codec=icodec)
    check_pages(gpu_ctx, col, pages, metas, id_widths=(1, 2), what="index codec %d" % icodec)


# ---- 3: only the entries that live rows point at are keys; both sides of FILTER_DICT_BITS (8192 entries)
def test_dict_referenced_entries_only_on_both_sides_of_the_table(gpu_ctx):
    for uniq, rows in ((8000, 60_000), (9000, 70_000)):
        voc = [b"entry-%05d-%s" % (i, b"z" * (i % 7)) for i in range(uniq)]
        col = K.column(pick(voc, rows, uniq), validity(rows, 0.2, uniq))
        pages, metas = write(col, S.DICT, max_page_size=rows, force_codec=S.DICT)
        assert metas.shape[0] == 1 and (uniq <= 8192) == (uniq == 8000)
        ref = K.Ref(col, pages, metas)
        live = sorted(set(ref.strs[ref.valid]))
        assert len(live) > 1024
        chosen = [live[0], live[1], live[len(live) // 3], live[len(live) // 2], live[-1]]
        only = np.isin(ref.strs, np.array(chosen, object))   # (null rows of these strings are selected too: they give no key)
        cp = upload(gpu_ctx, col, pages, metas)
        res = run(gpu_ctx, [cp] * 3, [only, None, only], [ref] * 3, [16, 1024, 5], [1, 2, 4], what="dict %d" % uniq)
        assert (res[0].n_keys, res[0].overflow) == (5, 0) and res[0].keys == chosen
        assert res[1].overflow & 1 and res[1].overflow_keys and not res[2].overflow


# ---- 4: the compare's edges
def edge_strings():
    pat = (b"abcdefghijklmnopqrstuvwxyz" * 8)
    out = {}
    for L in (0, 1, 3, 4, 7, 8, 9, 15, 16, 17, 24, 25, 32, 33, 200):
        p = pat[:L]
        out[p] = True                                         # each a proper prefix of the longer ones
        if L:
            out[p[:-1] + b"\xff"] = True                      # differs in the last byte only
            out[p[:-1] + b"\x00"] = True
        if L > 8:
            out[p[:8] + b"\x80" + p[9:]] = True               # differs at byte 8 only
    for s in (b"a\x00", b"a\x00\x00", b"\x80", b"\xfe\xff", b"\xff" * 9, b"\x00", b"\x00" * 8, b"\x00" * 9):
        out[s] = True
    return list(out)


@pytest.mark.parametrize("codec", [S.NONE, S.DICT], ids=["none", "dict"])
def test_the_edges_of_the_compare(gpu_ctx, codec):
    voc = edge_strings()
    assert b"" in voc and b"a" in voc and b"a\x00" in voc
    rows = 10_000
    for large in (False, True):
        col = K.column(pick(voc, rows, 41, runs=2), validity(rows, 0.2, 42), large)
        pages, metas = write(col, codec, max_page_size=2050, force_codec=codec)
        res = check_pages(gpu_ctx, col, pages, metas, id_widths=(1, 4), what="edges")
        keys = res[0].keys
        assert keys == sorted(voc) and keys[0] == b"" and keys.index(b"a") + 1 == keys.index(b"a\x00")
        assert keys[-1] == b"\xff" * 9 and keys.index(b"abcdefgh") < keys.index(b"abcdefghi") < keys.index(b"abcdefgh\x80")
    # the empty string only in null rows is no key; live, it is the first
    strs = pick([s for s in voc if s], rows, 43)
    valid = np.random.default_rng(44).random(rows) >= 0.2
    for i in np.flatnonzero(~valid)[::2]:
        strs[i] = b""
    col = K.column(strs, valid)
    pages, metas = write(col, codec, max_page_size=2050, force_codec=codec)
    res = check_pages(gpu_ctx, col, pages, metas, id_widths=(2,), what="empty string in null rows")
    assert b"" not in res[0].keys and res[0].n_keys == len(voc) - 1


# ---- 5: 1024 keys with 2-byte ids.  The tag of a slot has 8 bits (KEYV_TAG_BITS, csrc/sb_common.h; pinned by
# tests/test_key_ids_var_host.py), so among 1024 strings equal tags on different strings are certain (4 strings per tag on
# average): every probe sequence that meets one goes through the exact compare behind a tag hit.
@pytest.mark.parametrize("codec", [S.NONE, S.DICT, S.LZ4], ids=["none", "dict", "lz4"])
def test_1024_keys_with_two_byte_ids(gpu_ctx, codec):
    voc = vocab(1024, 5, maxlen=48)
    col = K.column(pick(voc, 10_000, 51), validity(10_000, 0.1, 52))
    pages, metas = write(col, codec, max_page_size=4100, force_codec=codec)
    res = check_pages(gpu_ctx, col, pages, metas, max_keys=1024, id_widths=(2,), what="1024 keys")
    assert res[0].n_keys > 1000 and not res[0].overflow


# ---- 6: the overflow boundaries
@pytest.mark.parametrize("codec", [S.NONE, S.DICT], ids=["none", "dict"])
@pytest.mark.parametrize("max_keys,id_width", [(1, 1), (255, 1), (256, 2), (1024, 2)])
def test_the_overflow_boundary_of_max_keys(gpu_ctx, codec, max_keys, id_width):
    rows = 10_000
    voc = vocab(max_keys + 1, max_keys, minlen=1, maxlen=20)
    cps, refs, masks = [], [], []
    for n, where in ((max_keys, None), (max_keys + 1, 0), (max_keys + 1, rows - 1), (max_keys, "dead")):
        strs = pick(voc[:max_keys], rows, n, runs=2)
        valid = np.random.default_rng(n + 1).random(rows) >= 0.1
        mask = np.ones(rows, bool)
        for i, s in enumerate(voc[:max_keys]):   # every string is there, live
            strs[2 + 2 * i if 2 + 2 * i < rows - 2 else i] = s
            valid[2 + 2 * i if 2 + 2 * i < rows - 2 else i] = True
        if where == "dead":   # the extra string in a null row and in a row the selection leaves out
            strs[rows // 2 + 1], valid[rows // 2 + 1] = voc[max_keys], False
            strs[rows // 2 + 3], mask[rows // 2 + 3] = voc[max_keys], False
        elif where is not None:
            strs[where], valid[where] = voc[max_keys], True
        col = K.column(strs, valid)
        pages, metas = write(col, codec, max_page_size=4100, force_codec=codec)
        cps.append(upload(gpu_ctx, col, pages, metas))
        refs.append(K.Ref(col, pages, metas))
        masks.append(mask)
    res = run(gpu_ctx, cps, masks, refs, [max_keys] * 4, [id_width] * 4, what="boundary")   # (the synchronize returned)
    assert [r.overflow for r in res] == [0, 1, 1, 0]
    for r in (res[0], res[3]):
        assert r.n_keys == max_keys
        ids = K.ids_numpy(r)
        assert int(ids[ids != (1 << (8 * id_width)) - 1].max()) == max_keys - 1


@pytest.mark.parametrize("codec", [S.NONE, S.DICT], ids=["none", "dict"])
def test_the_overflow_boundary_of_keys_capacity(gpu_ctx, codec):
    voc = vocab(300, 6, maxlen=30)
    col = K.column(pick(voc, 10_000, 61), validity(10_000, 0.1, 62))
    pages, metas = write(col, codec, max_page_size=4100, force_codec=codec)
    ref = K.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    for mask in three_masks(10_000, 63)[:2]:
        total = K.want(ref, mask, 512, 2).keys_len
        assert total > 1000
        res = run(gpu_ctx, [cp] * 4, [mask] * 4, [ref] * 4, [512] * 4, [2] * 4, [total, total - 1, 0, total + 5], what="keys_capacity")
        assert [r.overflow for r in res] == [0, 2, 2, 0] and res[1].overflow_bytes and not res[1].overflow_keys
        # one byte short: ids, key_offsets, n_keys and keys_len are still exact (K.check), only the bytes are not delivered
        assert res[1].keys_len == total and res[1].n_keys == res[0].n_keys and res[1].key_bytes == bytes(total - 1)
        assert np.array_equal(K.ids_numpy(res[1]), K.ids_numpy(res[0])) and np.array_equal(res[1].key_offsets, res[0].key_offsets)


@pytest.mark.parametrize("codec", [S.NONE, S.DICT, S.ZSTD], ids=["none", "dict", "zstd"])
def test_a_column_whose_rows_are_all_distinct(gpu_ctx, codec):
    col = K.column([b"row-%06d" % i for i in range(10_000)], validity(10_000, 0.05, 7))
    pages, metas = write(col, codec, max_page_size=4100, force_codec=codec)
    res = check_pages(gpu_ctx, col, pages, metas, max_keys=1024, id_widths=(2, 4), what="all distinct")
    assert res[0].overflow == 1 and res[-1].overflow == 0 and res[-1].n_keys == 0


# ---- 7: guards
def _guarded(ctx, nbytes, align=1):
    """(the `nbytes` handed to the call, the whole buffer): between two guards of GUARD_BYTES bytes of GUARD"""
    import torch
    with torch.cuda.stream(ctx.torch_stream):   # (the fill is ordered before the call's kernels)
        whole = torch.full((2 * GUARD_BYTES + nbytes,), GUARD, dtype=torch.uint8, device=ctx.torch_device)
    assert whole.data_ptr() % 4 == 0 and GUARD_BYTES % align == 0
    return whole[GUARD_BYTES:GUARD_BYTES + nbytes], whole


def _guards_intact(whole, nbytes):
    h = whole.cpu().numpy()
    return bool((h[:GUARD_BYTES] == GUARD).all() and (h[GUARD_BYTES + nbytes:] == GUARD).all())


@pytest.mark.parametrize("id_width", [1, 2, 4])
def test_ids_keys_and_offsets_of_exactly_their_size_between_guards(gpu_ctx, id_width):
    import torch
    import strawboat_amd as sb
    from strawboat_amd.key_ids import ID_DTYPES
    rows, max_keys = 10_001, 64
    shapes = ((40, S.NONE), (40, S.DICT), (40, S.LZ4), (500, S.NONE), (500, S.DICT))   # (500: the overflow)
    for uniq, codec in shapes:
        col = K.column(pick(vocab(uniq, uniq, maxlen=30), rows, uniq + codec, runs=2), validity(rows, 0.2, codec))
        pages, metas = write(col, codec, max_page_size=2050, force_codec=codec)
        ref = K.Ref(col, pages, metas)
        cp = upload(gpu_ctx, col, pages, metas)
        full = K.want(ref, None, 1024, 2).keys_len
        for mask, kcap in [(m, kc) for m in three_masks(rows, id_width) for kc in (full, 100)]:
            ids_bytes, ids_whole = _guarded(gpu_ctx, rows * id_width, id_width)
            ids = ids_bytes.view(getattr(torch, ID_DTYPES[id_width]))
            batch = sb.KeyIdsVarBatch(gpu_ctx, [cp], bitmap(gpu_ctx, mask), max_keys, id_width, kcap, out=[ids])
            keys = (C.c_uint8 * (kcap + 2 * GUARD_BYTES))()
            offs = (C.c_uint8 * (8 * (max_keys + 1) + 2 * GUARD_BYTES))()
            C.memset(keys, GUARD, C.sizeof(keys))
            C.memset(offs, GUARD, C.sizeof(offs))
            batch._arr[0].keys = C.addressof(keys) + GUARD_BYTES
            batch._arr[0].key_offsets = C.addressof(offs) + GUARD_BYTES
            assert batch._arr[0].ids_capacity == rows * id_width and batch._arr[0].keys_capacity == kcap
            res = batch.enqueue()
            gpu_ctx.synchronize()
            w = K.want(ref, mask, max_keys, id_width, kcap)
            assert res[0].overflow == w.overflow
            assert (w.overflow & 1) == (uniq == 500 and (mask is None or bool(mask.any())))
            assert _guards_intact(ids_whole, rows * id_width), "a byte outside ids was written"
            kb, ob = bytes(keys), bytes(offs)
            guard = bytes([GUARD]) * GUARD_BYTES
            assert kb[:GUARD_BYTES] == guard and kb[GUARD_BYTES + kcap:] == guard, "a byte outside keys was written"
            assert ob[:GUARD_BYTES] == guard and ob[GUARD_BYTES + 8 * (max_keys + 1):] == guard, "a byte outside key_offsets was written"
            if not w.overflow & 1:
                assert np.array_equal(np.frombuffer(ob[GUARD_BYTES:GUARD_BYTES + 8 * (max_keys + 1)], np.uint64), w.key_offsets)
                assert np.array_equal(ids.cpu().numpy().view(K.ID_NP[id_width]), w.ids)
                assert (res[0].rows, res[0].selected, res[0].count, res[0].n_keys, res[0].keys_len) == (w.rows, w.selected, w.count, w.n_keys, w.keys_len)
            if not w.overflow:
                assert kb[GUARD_BYTES:GUARD_BYTES + kcap] == w.key_bytes


def test_pages_at_odd_byte_offsets_and_scattered_page_offsets(gpu_ctx):
    import torch
    from strawboat_amd import read
    for codec in (S.NONE, S.DICT, S.LZ4, S.FREQ):
        col = K.column(codec_strings(codec, 10_000, codec), validity(10_000, 0.2, codec), large=codec == S.DICT)
        pages, metas = write(col, codec, max_page_size=2050, force_codec=codec)
        ref = K.Ref(col, pages, metas)
        cps = []
        for off in (1, 3, 7):
            buf = torch.zeros(off + pages.size, dtype=torch.uint8, device=gpu_ctx.torch_device)
            buf[off:] = torch.from_numpy(np.ascontiguousarray(pages)).to(gpu_ctx.torch_device)
            cps.append(read.ColumnPages(col["ptype"], col["nullable"], buf[off:], metas))
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
        cps.append(read.ColumnPages(col["ptype"], col["nullable"], to_dev(gpu_ctx, buf), metas, page_offsets=np.array(offs, np.uint64)))
        for mask in three_masks(10_000, codec):
            run(gpu_ctx, cps, [mask] * 4, [ref] * 4, [128] * 4, [1, 2, 4, 1], what="offsets, codec %d" % codec)


# ---- 8: mixed calls
def test_binary_and_large_binary_with_different_max_keys_and_widths_share_a_selection(gpu_ctx):
    rng = np.random.default_rng(8)
    cps, refs = [], []
    for large, codec, page, uniq in ((False, S.NONE, 4100, 300), (True, S.DICT, 2050, 200), (False, S.ZSTD, 2050, 700),
                                     (True, S.LZ4, 2050, 30), (False, S.ONEVALUE, 777, 1), (True, S.FREQ, 2050, 100)):
        strs = codec_strings(codec, 10_000, page) if codec in (S.FREQ, S.ONEVALUE) else pick(vocab(uniq, uniq), 10_000, page)
        col = K.column(strs, validity(10_000, 0.2, uniq), large)
        pages, metas = write(col, codec, max_page_size=page, force_codec=codec)
        cps.append(upload(gpu_ctx, col, pages, metas))
        refs.append(K.Ref(col, pages, metas))
    shared = rng.random(10_000) < 0.35
    for masks in ([shared] * 6, [shared, None, rng.random(10_000) < 0.9, np.zeros(10_000, bool), None, shared]):
        for mks, ws, kbs in (([512, 255, 1024, 64, 1, 128], [2, 1, 4, 1, 1, 2], [65536, 4096, 1 << 20, 64, 40, 8192]),
                             ([100, 100, 100, 10, 3, 100], [4, 2, 2, 4, 2, 1], [65536] * 6), ([1024] * 6, [2] * 6, [20000] * 6)):
            res = run(gpu_ctx, cps, masks, refs, mks, ws, kbs, what="max_keys %r" % (mks,))
            run(gpu_ctx, cps[::-1], masks[::-1], refs[::-1], mks, ws, kbs, what="max_keys %r, the columns turned round" % (mks,))
            assert any(r.overflow_keys for r in res) == (mks[0] == 100)


def test_columns_without_rows_or_pages(gpu_ctx):
    import torch
    import strawboat_amd as sb
    from strawboat_amd import read
    dev = gpu_ctx.torch_device
    empty = read.ColumnPages(S.T_BIN32, True, torch.zeros(0, dtype=torch.uint8, device=dev), np.zeros((0, 2), np.uint64))
    for sel in (None, torch.zeros(0, dtype=torch.uint8, device=dev)):
        r = sb.key_ids_var(gpu_ctx, [empty], sel, 7, key_bytes=24)[0]
        gpu_ctx.synchronize()
        assert (r.rows, r.selected, r.count, r.n_keys, r.keys_len, r.overflow) == (0, 0, 0, 0, 0, 0)
        assert r.key_bytes == bytes(24) and not r.key_offsets.any() and r.keys == [] and r.ids.numel() == 0
    col = K.column(pick(vocab(50, 9), 3000, 9), validity(3000, 0.3, 9), True)
    pages, metas = write(col, S.NONE, max_page_size=777, force_codec=S.NONE)
    ref = K.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(1).random(3000) < 0.5
    res = sb.key_ids_var(gpu_ctx, [empty, cp, empty], [None, bitmap(gpu_ctx, mask), None], [3, 64, 1024], [1, 1, 4], [0, 4096, 1 << 20])
    gpu_ctx.synchronize()
    assert (res[0].rows, res[0].n_keys, res[2].selected) == (0, 0, 0) and res[2].key_bytes == bytes(1 << 20) and not res[2].key_offsets.any()
    K.check(res[1], K.want(ref, mask, 64, 1, 4096), "next to empty columns")


# ---- 9: the same bytes every time
def _same_bytes(ctx):
    import strawboat_amd as sb
    from tests.test_gpu_freq import sparse
    rows = 10_000
    rng = np.random.default_rng(7)
    shapes = [(False, S.NONE, 40), (True, S.DICT, 3), (False, S.FREQ, 100), (True, S.LZ4, 200), (False, S.NONE, 250), (False, S.DICT, 900),
              (True, S.ZSTD, 500), (False, S.ONEVALUE, 1)]
    cps, refs = [], []
    for i, (large, codec, uniq) in enumerate(shapes * 2):   # 16 columns
        strs = codec_strings(codec, rows, i) if codec in (S.FREQ, S.ONEVALUE) else pick(vocab(uniq, i), rows, i)
        col = K.column(strs, validity(rows, 0.2 if i % 2 else None, i), large)
        pages, metas = write(col, codec, max_page_size=2050, force_codec=codec)
        cps.append(upload(ctx, col, pages, metas))
        refs.append(K.Ref(col, pages, metas))
    mask = rng.random(rows) < 0.35
    mks = [1024 if i % 3 else 256 for i in range(16)]
    ws = [2 if i % 4 else 4 for i in range(16)]
    batch = sb.KeyIdsVarBatch(ctx, cps, bitmap(ctx, mask), mks, ws)

    def state(res):
        return [(r.key_bytes, r.key_offsets.tobytes(), r.ids.cpu().numpy().tobytes(), r.n_keys, r.keys_len, r.count, r.overflow) for r in res]

    seen = []
    for _ in range(2):   # fresh intervals
        res = batch.enqueue()
        ctx.synchronize()
        seen.append(state(res))
    # ... and in an interval that a filter call's primitive Freq column causes to be issued again
    x = sparse(S.T_I32, rows, 0.05, 2, null_density=0.1)
    xp, xm = gen.oracle_write(x, max_page_size=2050, force_codec=S.FREQ)
    r0 = ctx.replays()
    sb.filter_columns(ctx, [upload(ctx, x, xp, xm)], [sb.Predicate("ne", 7)])
    res = batch.enqueue()
    ctx.synchronize()
    assert ctx.replays() == r0 + 1
    seen.append(state(res))
    assert all(s == seen[0] for s in seen[1:])
    for i, (r, ref) in enumerate(zip(res, refs)):
        K.check(r, K.want(ref, mask, mks[i], ws[i]), "in the replayed interval, column %d" % i)
    return cps[0], refs[0]


def test_the_same_bytes_every_time_and_in_a_replayed_interval(gpu_ctx):
    _same_bytes(gpu_ctx)


def test_on_a_context_that_holds_launch_hints(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd import read
    ctx = sb.Context(0)
    try:
        col = gen.prim(S.T_I64, 200_000, uniq=50, null_density=0.1, runs=40, seed=5)
        pages, metas = gen.oracle_write(col, max_page_size=65536, force_codec=S.RLE)
        cp = upload(ctx, col, pages, metas)
        for _ in range(3):   # the hints now say: RLE pages alone, no tiles, nothing in queue A
            read.read_simple(ctx, cp)
        r0 = ctx.replays()
        _same_bytes(ctx)     # (its own replay: the primitive Freq filter's)
        assert ctx.replays() == r0 + 1
        # ... and the read path still reads right behind it
        got = read.read_simple(ctx, cp)
        assert np.array_equal(got.values_numpy(), gen.oracle_read(col, pages, metas)["values"])
    finally:
        ctx.close()


# ---- 10: the chains the call exists for
def test_filter_then_key_ids_var_then_grouped_aggregate_in_one_interval(gpu_ctx):
    import strawboat_amd as sb
    from tests.aggregate_ref import Ref as NumRef
    rows = 10_007
    x = gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1)
    voc = vocab(40, 10, maxlen=20)
    k = K.column(pick(voc, rows, 10), validity(rows, 0.15, 10))
    y = gen.prim(S.T_I64, rows, uniq=5000, null_density=0.1, seed=2)
    xp, xm = gen.oracle_write(x, max_page_size=2050, force_codec=S.RLE)
    kp, km = write(k, S.DICT, max_page_size=4100, force_codec=S.DICT)
    yp, ym = gen.oracle_write(y, max_page_size=4100, force_codec=S.NONE)
    xr, kr, yr = NumRef(x, xp, xm), K.Ref(k, kp, km), NumRef(y, yp, ym)
    mask = (xr.vals < 60) & xr.valid
    assert 0 < mask.sum() < rows
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, x, xp, xm)], [sb.Predicate("lt", 60)])
    kid = sb.key_ids_var(gpu_ctx, [upload(gpu_ctx, k, kp, km)], sel[0], max_keys=64)[0]
    assert kid.id_width == 1
    agg = sb.aggregate_grouped(gpu_ctx, [upload(gpu_ctx, y, yp, ym)], kid.ids, 64, sel[0])[0]
    gpu_ctx.synchronize()   # (the only one)
    assert np.array_equal(sel[0].numpy(), mask)
    K.check(kid, K.want(kr, mask, 64, 1), "behind the filter")
    # a Python dict group-by of the oracle's decodes
    groups = {}
    for i in np.flatnonzero(mask & kr.valid):
        g = groups.setdefault(kr.strs[i], [0, []])
        g[0] += 1
        if yr.valid[i]:
            g[1].append(int(yr.vals[i]))
    assert kid.keys == sorted(groups) and kid.n_keys == 40
    assert agg.out_of_range == int((mask & ~kr.valid).sum())
    for g, key in enumerate(sorted(groups)):
        n_sel, live = groups[key]
        got = agg[g]
        assert (got.selected, got.count) == (n_sel, len(live)), g
        if live:
            assert (got.min, got.max, got.sum) == (min(live), max(live), sum(live)), g
    for g in range(40, 64):
        assert (agg[g].selected, agg[g].count) == (0, 0)


def test_keys_as_the_list_of_a_semi_join(gpu_ctx):
    import strawboat_amd as sb
    from tests.aggregate_ref import Ref as NumRef
    rows = 10_000
    voc = vocab(900, 13, maxlen=24)
    dim = K.column(pick(voc[:600], rows, 13, each=False), validity(rows, 0.1, 13))          # the dimension's key column
    flag = gen.prim(S.T_U8, rows, uniq=10, seed=3)                                           # ... and its filter column
    fact = K.column(pick(voc, rows, 14), validity(rows, 0.1, 14), True)
    dp, dm = write(dim, S.NONE, max_page_size=2050, force_codec=S.NONE)
    gp, gm = gen.oracle_write(flag, max_page_size=2050, force_codec=S.RLE)
    fp, fm = write(fact, S.DICT, max_page_size=4100, force_codec=S.DICT)
    dr, gr, fr = K.Ref(dim, dp, dm), NumRef(flag, gp, gm), K.Ref(fact, fp, fm)
    sel = sb.filter_columns(gpu_ctx, [upload(gpu_ctx, flag, gp, gm)], [sb.Predicate("eq", 3)])
    kid = sb.key_ids_var(gpu_ctx, [upload(gpu_ctx, dim, dp, dm)], sel[0], max_keys=1024)[0]
    gpu_ctx.synchronize()
    mask = (gr.vals == 3) & gr.valid
    K.check(kid, K.want(dr, mask, 1024, 2), "the build side")
    assert not kid.overflow and 100 < kid.n_keys <= 1024
    hit = sb.filter_in(gpu_ctx, [upload(gpu_ctx, fact, fp, fm)], [kid.as_in_list()])
    gpu_ctx.synchronize()
    assert np.array_equal(hit[0].numpy(), np.isin(fr.strs, dr.strs[mask & dr.valid]) & fr.valid)


# ---- 11: refusals through the raw C call
def _raw(ctx, cps, bitmaps, rows, max_keys=7, id_width=2, kcap=256):
    import torch
    import strawboat_amd as sb
    batch = sb.KeyIdsVarBatch(ctx, cps, bitmaps, max_keys, id_width, kcap)
    batch._keys, batch._offs, batch._ids = [], [], []
    for i in range(len(cps)):
        keys = (C.c_uint8 * kcap)()
        offs = (C.c_uint8 * (8 * (max_keys + 1)))()
        C.memset(keys, GUARD, C.sizeof(keys))
        C.memset(offs, GUARD, C.sizeof(offs))
        batch._arr[i].keys = C.addressof(keys)
        batch._arr[i].key_offsets = C.addressof(offs)
        ids = torch.full((rows * id_width + 8,), GUARD, dtype=torch.uint8, device=ctx.torch_device)
        batch._arr[i].ids = ids.data_ptr()
        batch._arr[i].ids_capacity = rows * id_width + 8
        batch._keys.append(keys)
        batch._offs.append(offs)
        batch._ids.append(ids)
        for f in RESULTS:
            setattr(batch._arr[i], f, WORD)
    return batch


def _canaries_kept(batch):
    for c, keys, offs, ids in zip(batch._arr, batch._keys, batch._offs, batch._ids):
        assert all(getattr(c, f) == WORD for f in RESULTS)
        assert bytes(keys) == bytes([GUARD]) * C.sizeof(keys) and bytes(offs) == bytes([GUARD]) * C.sizeof(offs)
        assert bool((ids == GUARD).all())


def test_refusals_at_the_call(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd import _native as N
    rows = 5000
    col = K.column(pick(vocab(5, 11, minlen=1), rows, 11), validity(rows, 0.2, 11))
    pages, metas = write(col, S.NONE, max_page_size=2050, force_codec=S.NONE)
    ref = K.Ref(col, pages, metas)
    cp = upload(gpu_ctx, col, pages, metas)
    mask = np.random.default_rng(9).random(rows) < 0.5
    bm = bitmap(gpu_ctx, mask)

    def fresh(**kw):
        return _raw(gpu_ctx, [cp, cp], [bm, bm], rows, **kw)

    def refused(batch, code, what, mem=N.SB_MEM_DEVICE):
        assert gpu_ctx._lib.sb_key_ids_var(gpu_ctx._h, batch._arr, 2, mem) == code, what
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
    batch._arr[0].key_offsets = None
    refused(batch, N.SB_ERR_INVALID, "key_offsets null")
    batch = fresh()
    batch._arr[0].keys = None
    refused(batch, N.SB_ERR_INVALID, "keys null with keys_capacity > 0")
    batch = fresh()
    batch._arr[1].keys_capacity = (1 << 20) + 1
    refused(batch, N.SB_ERR_INVALID, "keys_capacity above the limit")
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
    for ptype in (S.T_I8, S.T_I32, S.T_I64, S.T_U64, S.T_F32, S.T_F64, S.T_BOOL, S.T_I128, S.T_I256, S.T_NULL):
        batch = fresh()
        batch._arr[1].physical_type = ptype
        refused(batch, N.SB_ERR_NYI, "type %d" % ptype)
    batch = fresh()
    refused(batch, N.SB_ERR_NYI, "SB_MEM_HOST", mem=N.SB_MEM_HOST)
    # a page of more rows, or of more bytes, than the reference word of a slot has bits for (checked before a byte is read)
    for field, value in ((1, (1 << 26) + 1), (0, 1 << 32)):
        batch = fresh()
        m = np.array(metas, np.uint64).copy()
        m[0, field] = value
        keep = (N.PageMetaC * m.shape[0]).from_buffer_copy(m.tobytes())
        batch._arr[1].metas = keep
        batch._arr[1].ids_capacity = 1 << 40
        batch._arr[1].selection = None
        refused(batch, N.SB_ERR_NYI, "a page beyond the reference word's fields")
    # keys null is no refusal with keys_capacity 0; the same batch, as it was built, succeeds
    batch = fresh()
    batch._arr[0].keys, batch._arr[0].keys_capacity = None, 0
    res = batch.enqueue()
    gpu_ctx.synchronize()
    w = K.want(ref, mask, 7, 2, 256)
    assert res[0].overflow == 2 and res[0].n_keys == w.n_keys and res[0].keys_len == w.keys_len and bytes(batch._keys[0]) == bytes([GUARD]) * 256
    for i, (r, keys, offs, ids) in enumerate(zip(res, batch._keys, batch._offs, batch._ids)):
        assert np.array_equal(np.frombuffer(bytes(offs), np.uint64), w.key_offsets) and (r.n_keys, r.count) == (w.n_keys, w.count)
        if i:
            assert bytes(keys) == w.key_bytes and r.overflow == 0
        h = ids.cpu().numpy()
        assert np.array_equal(h[:rows * 2].view(np.uint16), w.ids) and (h[rows * 2:] == GUARD).all()
    # sb_key_ids still refuses Binary / LargeBinary
    for large in (False, True):
        b = sb.KeyIdsBatch(gpu_ctx, [upload(gpu_ctx, gen.prim(S.T_I64, 100, uniq=5), *gen.oracle_write(gen.prim(S.T_I64, 100, uniq=5)))], None, 7, 2)
        b._arr[0].physical_type = S.T_BIN64 if large else S.T_BIN32
        assert gpu_ctx._lib.sb_key_ids(gpu_ctx._h, b._arr, 1, N.SB_MEM_DEVICE) == N.SB_ERR_NYI
        gpu_ctx.synchronize()


# ---- 12: errors at the synchronize
def test_a_truncated_page_raises_what_the_decoder_raises(gpu_ctx):
    import strawboat_amd as sb
    from strawboat_amd._native import NativeError
    for codec in (S.NONE, S.DICT, S.LZ4, S.FREQ):
        col = K.column(codec_strings(codec, 9000, codec), validity(9000, 0.1, codec))
        pages, metas = write(col, codec, max_page_size=3000, force_codec=codec)
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
            res = sb.key_ids_var(gpu_ctx, [cp], bitmap(gpu_ctx, mask), 128)
            with pytest.raises(NativeError) as e:
                gpu_ctx.synchronize()
            assert e.value.code == want, codec
            # rows and selected are delivered even when the interval failed
            assert res[0].rows == 9000 and res[0].selected == (9000 if mask is None else int(sel.sum()))
    # the context still works
    col = K.column(pick(vocab(60, 12), 9000, 12))
    pages, metas = write(col, S.DICT, max_page_size=3000, force_codec=S.DICT)
    check_pages(gpu_ctx, col, pages, metas, what="after the errors")
