"""sb_key_combine and group_by over several key columns on the GPU.  The device's tuples and ids are compared with the numpy
reference (tests/key_combine_ref.py) fed with the same id arrays; the chains that start from pages are compared with a
Python dict group-by over the ORACLE's decodes of the pages.  Every comparison is exact.

The kernels take one row per lane and 256 rows per workgroup step, and at most 2048 workgroups stride over an item's rows
(csrc/sb_key_combine.h): the row edges below cover a wave, a workgroup step and, once, the first row of the second sweep."""
import ctypes as C

import numpy as np
import pytest

from oracle import sbo as S
from tests import aggregate_ref as R
from tests import gen
from tests import key_combine_ref as K
from tests import key_ids_var_ref as KV
from tests.test_gpu_aggregate import _column, bitmap
from tests.test_gpu_read_selected import to_dev, upload

pytestmark = pytest.mark.gpu

GUARD = 0xA5
GUARD_BYTES = 4096
SWEEP = 2048 * 256   # rows the grid covers in one sweep
NP_OF_WIDTH = {1: np.uint8, 2: np.uint16, 4: np.uint32}
WORD = 0x5A5A5A5A5A5A5A5A


def part_dev(ctx, a):
    """a part array on the device, at the very end of its allocation's tensor: capacity exactly rows * width"""
    import torch
    a = np.ascontiguousarray(a)
    raw = a.view(np.uint8)
    whole = torch.empty(64 + raw.size, dtype=torch.uint8, device=ctx.torch_device)
    tail = whole[64:]
    tail.copy_(torch.from_numpy(raw.copy()))
    dt = {1: torch.uint8, 2: torch.uint16, 4: torch.int32}[a.dtype.itemsize]
    return tail.view(dt)


def guarded_ids(ctx, rows, id_width):
    """(the ids tensor handed to the call, the whole buffer): exactly rows * id_width bytes between two guards"""
    import torch
    with torch.cuda.stream(ctx.torch_stream):   # (the fill is ordered before the call's kernels)
        whole = torch.full((2 * GUARD_BYTES + rows * id_width,), GUARD, dtype=torch.uint8, device=ctx.torch_device)
    dt = {1: torch.uint8, 2: torch.uint16, 4: torch.int32}[id_width]
    return whole[GUARD_BYTES:GUARD_BYTES + rows * id_width].view(dt), whole


def guards_intact(whole, nbytes):
    h = whole.cpu().numpy()
    return bool((h[:GUARD_BYTES] == GUARD).all() and (h[GUARD_BYTES + nbytes:] == GUARD).all())


class Guarded:
    """one item of a call with every output between guards: ids on the device, tuples on the host"""

    def __init__(self, ctx, parts, bounds, max_keys, id_width, devs=None):
        from strawboat_amd.key_combine import KeyCombineBatch
        self.parts, self.bounds, self.max_keys, self.id_width = parts, bounds, max_keys, id_width
        self.rows = int(parts[0].size)
        self.devs = devs or [part_dev(ctx, p) for p in parts]
        self.ids, self.whole = guarded_ids(ctx, self.rows, id_width)
        self.batch = KeyCombineBatch(ctx, [[(d, b) for d, b in zip(self.devs, bounds)]], max_keys, id_width, out=[self.ids])
        self.tup = (C.c_uint8 * (16 * max_keys + 2 * GUARD_BYTES))()
        C.memset(self.tup, GUARD, C.sizeof(self.tup))
        self.batch._arr[0].tuples = C.addressof(self.tup) + GUARD_BYTES
        self.res = self.batch.results[0]

    def enqueue(self):
        self.batch.enqueue()

    def tuple_bytes(self):
        return bytes(self.tup)[GUARD_BYTES:GUARD_BYTES + 16 * self.max_keys]

    def check(self, what=""):
        """after the synchronize"""
        w = K.combine(self.parts, self.bounds, self.max_keys, self.id_width)
        tb = bytes(self.tup)
        assert tb[:GUARD_BYTES] == bytes([GUARD]) * GUARD_BYTES and tb[GUARD_BYTES + 16 * self.max_keys:] == bytes([GUARD]) * GUARD_BYTES, \
            "%s: a byte outside tuples was written" % what
        assert guards_intact(self.whole, self.rows * self.id_width), "%s: a byte outside ids was written" % what
        r = self.res
        assert (r.rows, r.live, r.overflow) == (w.rows, w.live, w.overflow), (what, r, (w.rows, w.live, w.overflow))
        if w.overflow:
            return w
        assert r.n_keys == w.n_keys, (what, r.n_keys, w.n_keys)
        assert self.tuple_bytes() == w.tuple_words.tobytes(), "%s: the words of tuples differ" % what
        ids = self.ids.cpu().numpy().view(NP_OF_WIDTH[self.id_width])
        bad = np.flatnonzero(ids != w.ids)
        assert bad.size == 0, "%s: %d ids differ, the first at row %d" % (what, bad.size, bad[0] if bad.size else -1)
        return w


def run_one(ctx, parts, bounds, max_keys, id_width, what=""):
    g = Guarded(ctx, parts, bounds, max_keys, id_width)
    g.enqueue()
    ctx.synchronize()
    return g, g.check(what)


def some_parts(rows, tops, widths, seed, dead=0.1, beyond=5, bounds=None):
    """ids below tops[p]; about `dead` of each part all ones; `beyond` ids at or above the bound that are not all ones"""
    rng = np.random.default_rng(seed)
    out = []
    for p, (top, w) in enumerate(zip(tops, widths)):
        dt = NP_OF_WIDTH[w]
        a = rng.integers(0, top, rows).astype(dt)
        a[rng.random(rows) < dead] = np.iinfo(dt).max
        if rows and beyond and bounds is not None:
            hi = np.iinfo(dt).max
            if bounds[p] < hi:
                at = rng.integers(0, rows, beyond)
                a[at] = rng.integers(bounds[p], hi, beyond).astype(dt)
        out.append(a)
    return out


# ---- 1: the width matrix
@pytest.mark.parametrize("id_width", [1, 2, 4])
@pytest.mark.parametrize("w0", [1, 2, 4])
@pytest.mark.parametrize("w1", [1, 2, 4])
def test_width_matrix(gpu_ctx, w0, w1, id_width):
    """bounds (7, 300), of which 7 x 30 are used so that one-byte ids hold the tuples.  A one-byte part cannot reach a bound
    of 300: its all-ones id, 255, is below the bound and so a valid id like any other, which makes 31 values of part 1"""
    bounds = (7, 300)
    parts = some_parts(10_000, (7, 30), (w0, w1), 10 * w0 + w1, bounds=bounds)
    g, w = run_one(gpu_ctx, parts, bounds, 255 if id_width == 1 else 1024, id_width, "widths %d %d -> %d" % (w0, w1, id_width))
    assert not w.overflow and w.n_keys == 7 * (31 if w1 == 1 else 30) and 0 < w.live < 10_000


# ---- 2: row edges
@pytest.mark.parametrize("rows", [0, 1, 63, 64, 65, 255, 256, 257, 1023, 1025, SWEEP + 1])
def test_row_edges(gpu_ctx, rows):
    for id_width, widths in ((1, (1, 2)), (2, (2, 1)), (4, (4, 4))):
        if rows > 70_000 and id_width != 1:
            continue   # (the second sweep of the grid: once)
        bounds = (5, 40)
        parts = some_parts(rows, (5, 40), widths, rows + id_width, bounds=bounds)
        if rows:   # the last row is live and has a tuple of its own
            parts[0][rows - 1], parts[1][rows - 1] = 4, 39
            parts[1][:rows - 1][parts[1][:rows - 1] == 39] = 0
        g, w = run_one(gpu_ctx, parts, bounds, 200, id_width, "%d rows" % rows)
        assert not w.overflow
        if rows:
            assert w.ids[rows - 1] == w.n_keys - 1 and tuple(w.tuples[-1]) == (4, 39)
        else:
            assert (g.res.n_keys, g.res.live) == (0, 0)


# ---- 3: the whole code word
@pytest.mark.parametrize("n_parts", [3, 4])
def test_the_whole_code_word(gpu_ctx, n_parts):
    rng = np.random.default_rng(n_parts)
    rows = 5000
    widths = (2, 4, 2, 4)[:n_parts]
    t = rng.integers(0, 1024, (rows, n_parts))
    t[0] = 0                      # the zero code
    t[1] = 1023                   # the top bit of every field
    t[2] = 1023, *([0] * (n_parts - 1))
    t[3] = *([0] * (n_parts - 1)), 1023
    base = rng.integers(1, 1023, n_parts)
    for k in range(20):           # tuples that differ only in the last part, and only in the first
        t[10 + k] = base
        t[10 + k, n_parts - 1] = 500 + k
        t[40 + k] = base
        t[40 + k, 0] = 500 + k
    for p in range(n_parts):      # every bit of every field alone
        for bit in range(10):
            t[100 + 10 * p + bit] = 0
            t[100 + 10 * p + bit, p] = 1 << bit
    t[200:] = t[rng.integers(0, 200, rows - 200)]     # (about 190 distinct tuples, many rows each)
    parts = [t[:, p].astype(NP_OF_WIDTH[w]) for p, w in enumerate(widths)]
    for p in range(n_parts):
        parts[p][300 + p::37] = np.iinfo(parts[p].dtype).max
    g, w = run_one(gpu_ctx, parts, (1024,) * n_parts, 1024, 2, "%d parts" % n_parts)
    assert not w.overflow and tuple(w.tuples[0]) == (0,) * n_parts and tuple(w.tuples[-1]) == (1023,) * n_parts
    assert w.ids[0] == 0 and w.ids[1] == w.n_keys - 1


# ---- 4: limits
def _cross(na, nb, rows, seed):
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, na * nb, rows)
    pick[rng.permutation(rows)[:na * nb]] = np.arange(na * nb)
    return pick // nb, pick % nb


def test_limits(gpu_ctx):
    rows = 20_000
    # 1024 tuples from a full 32 x 32 cross
    a, b = _cross(32, 32, rows, 1)
    g, w = run_one(gpu_ctx, [a.astype(np.uint8), b.astype(np.uint16)], (32, 32), 1024, 2, "32 x 32")
    assert not w.overflow and w.n_keys == 1024
    # 1024 sparse tuples in 1024 x 1024
    rng = np.random.default_rng(2)
    pool = np.unique(rng.integers(0, 1 << 20, 4000))[:1024]
    rng.shuffle(pool)
    pick = pool[rng.integers(0, 1024, rows)]
    pick[rng.permutation(rows)[:1024]] = pool
    sparse = [(pick >> 10).astype(np.uint16), (pick & 1023).astype(np.uint32)]
    g, w = run_one(gpu_ctx, sparse, (1024, 1024), 1024, 4, "1024 sparse tuples")
    assert not w.overflow and w.n_keys == 1024
    # exactly max_keys tuples: no overflow; max_keys + 1: an overflow, SB_OK at the synchronize, the guards intact
    for n, max_keys, id_width in ((300, 300, 2), (301, 300, 2), (255, 255, 1), (256, 255, 1), (1024, 1023, 2)):
        keep = pool[:n]
        pick = keep[rng.integers(0, n, rows)]
        pick[rng.permutation(rows)[:n]] = keep
        parts = [(pick >> 10).astype(np.uint16), (pick & 1023).astype(np.uint16)]
        g, w = run_one(gpu_ctx, parts, (1024, 1024), max_keys, id_width, "%d tuples, max_keys %d" % (n, max_keys))
        assert w.overflow == (n > max_keys) and g.res.overflow == (n > max_keys)
        assert g.res.live == rows
        if not w.overflow:
            assert g.res.n_keys == n


# ---- 5: arbitrary part bits
@pytest.mark.parametrize("id_width", [1, 2])
def test_arbitrary_part_bits(gpu_ctx, id_width):
    """what a part whose own key call overflowed may hold: random 32-bit words, most at or above the bound"""
    rng = np.random.default_rng(id_width)
    rows = 30_000
    parts = [rng.integers(0, 1 << 32, rows, dtype=np.uint64).astype(np.uint32) for _ in range(3)]
    for p in parts:   # a fifth of the rows below the bound, in all three parts at once for half of them
        low = rng.random(rows) < 0.2
        p[low] = rng.integers(0, 6, int(low.sum()))
    both = rng.random(rows) < 0.1
    for p in parts:
        p[both] = rng.integers(0, 6, int(both.sum()))
    g, w = run_one(gpu_ctx, parts, (6, 5, 6), 200, id_width, "random words")
    assert not w.overflow and 0 < w.live < rows and w.n_keys == 6 * 5 * 6
    # ... and 11-bit words against bounds of 1024: a quarter of the rows live, nearly each with a tuple of its own: far more
    # than max_keys tuples, nothing outside the buffers
    parts = [rng.integers(0, 1 << 11, rows).astype(np.uint16) for _ in range(2)]
    g, w = run_one(gpu_ctx, parts, (1024, 1024), 100, id_width, "random words, overflow")
    assert w.overflow


# ---- 6: several items in one call
def test_several_items_in_one_call(gpu_ctx):
    from strawboat_amd.key_combine import KeyCombineBatch
    a = some_parts(9000, (9, 20, 4), (1, 2, 4), 1, bounds=(9, 20, 4))
    b = some_parts(777, (9, 3), (1, 2), 2, bounds=(9, 3))
    devs = [part_dev(gpu_ctx, x) for x in a] + [part_dev(gpu_ctx, x) for x in b]
    items = [
        ([0, 1], (9, 20), 1024, 2),
        ([0, 1, 2], (9, 20, 4), 1024, 4),
        ([3, 4], (9, 3), 27, 1),
        ([2, 0], (4, 9), 36, 1),          # shares part arrays with the first two items
        ([1, 0, 1, 0], (20, 9, 20, 9), 255, 1),
    ]
    arrays = a + b
    batch = KeyCombineBatch(gpu_ctx, [[(devs[i], bd) for i, bd in zip(idx, bounds)] for idx, bounds, _, _ in items],
                            [mk for _, _, mk, _ in items], [w for _, _, _, w in items])
    first = None
    for turn in range(2):   # a call issued twice gives the same bytes
        res = batch.enqueue()
        gpu_ctx.synchronize()
        for r, (idx, bounds, mk, w) in zip(res, items):
            K.check(r, K.combine([arrays[i] for i in idx], bounds, mk, w), "item %r" % (idx,))
        now = [(r.ids.cpu().numpy().tobytes(), r.tuple_words.tobytes()) for r in res]
        first = first or now
        assert now == first
    assert res[0].rows == 9000 and res[2].rows == 777


# ---- 7: refusals through ctypes
def test_refusals_at_the_call(gpu_ctx):
    import torch
    from strawboat_amd import _native as N
    from strawboat_amd.key_combine import KeyCombineBatch
    rows = 3000
    arrays = some_parts(rows, (5, 6, 7), (2, 4, 1), 3, bounds=(5, 6, 7))
    devs = [part_dev(gpu_ctx, x) for x in arrays]

    def fresh():
        batch = KeyCombineBatch(gpu_ctx, [[(devs[0], 5), (devs[1], 6)], [(devs[1], 6), (devs[2], 7), (devs[0], 5)]], 250, 2)
        batch._ids = []
        batch._tups = []
        for i in range(2):
            ids = torch.full((rows * 2 + 8,), GUARD, dtype=torch.uint8, device=gpu_ctx.torch_device)
            tup = (C.c_uint8 * (16 * 250))()
            C.memset(tup, GUARD, C.sizeof(tup))
            batch._ids.append(ids)
            batch._tups.append(tup)
            c = batch._arr[i]
            c.ids, c.ids_capacity, c.tuples = ids.data_ptr(), rows * 2, C.addressof(tup)
            c.live = c.n_keys = c.overflow = WORD
        torch.cuda.synchronize()
        return batch

    def kept(batch):
        for c, ids, tup in zip(batch._arr, batch._ids, batch._tups):
            assert (c.live, c.n_keys, c.overflow) == (WORD, WORD, WORD)
            assert bytes(tup) == bytes([GUARD]) * C.sizeof(tup) and bool((ids == GUARD).all())

    def refused(batch, code, what, mem=N.SB_MEM_DEVICE):
        assert gpu_ctx._lib.sb_key_combine(gpu_ctx._h, batch._arr, 2, mem) == code, what
        gpu_ctx.synchronize()   # (nothing was enqueued, nothing is raised here)
        kept(batch)

    def tweak(what, item=1, code=N.SB_ERR_INVALID, **fields):
        batch = fresh()
        for f, v in fields.items():
            setattr(batch._arr[item], f, v)
        refused(batch, code, what)

    def tweak_part(what, field, p, value, item=1):
        batch = fresh()
        getattr(batch._arr[item], field)[p] = value
        refused(batch, N.SB_ERR_INVALID, what)

    refused(fresh(), N.SB_ERR_NYI, "SB_MEM_HOST", mem=N.SB_MEM_HOST)
    for n_parts in (0, 1, 5, 1 << 31):
        tweak("n_parts %d" % n_parts, n_parts=n_parts)
    for w in (0, 3, 8, 0xFFFFFFFF):
        tweak("id_width %d" % w, id_width=w)
        tweak_part("part_width %d" % w, "part_width", 1, w)
    for b in (0, 1025, 0xFFFFFFFF):
        tweak_part("part_keys %d" % b, "part_keys", 2, b)
    tweak_part("a part null with rows > 0", "part_ids", 0, None)
    tweak_part("a part misaligned", "part_ids", 0, devs[1].data_ptr() + 2)
    tweak_part("a part too short", "part_capacity", 0, rows * 4 - 1)
    tweak("ids null", ids=None)
    tweak("ids misaligned", ids=fresh()._ids[1].data_ptr() + 1)
    tweak("ids too short", ids_capacity=rows * 2 - 1)
    for mk, w in ((0, 2), (1025, 2), (1025, 4), (256, 1), (1 << 31, 4)):
        tweak("max_keys %d at id_width %d" % (mk, w), max_keys=mk, id_width=w)
    tweak("tuples null", tuples=None)
    tweak("reserved != 0", reserved=1)
    tweak("ids overlaps a part of its own item", ids=devs[1].data_ptr() + 4, ids_capacity=rows * 2)
    tweak("ids overlaps a part of another item", item=0, ids=devs[2].data_ptr() + rows - 2, ids_capacity=rows * 2)
    batch = fresh()
    batch._arr[1].ids = batch._arr[0].ids + rows * 2 - 2   # the last id of item 0 is the first of item 1
    refused(batch, N.SB_ERR_INVALID, "ids of two items overlap")
    # the fields of the parts at and behind n_parts are ignored
    batch = fresh()
    batch._arr[0].part_width[2], batch._arr[0].part_keys[3], batch._arr[0].part_ids[2], batch._arr[0].part_capacity[3] = 3, 5000, 7, 1
    assert gpu_ctx._lib.sb_key_combine(gpu_ctx._h, batch._arr, 2, N.SB_MEM_DEVICE) == 0
    gpu_ctx.synchronize()
    for c, ids, tup, (idx, bounds) in zip(batch._arr, batch._ids, batch._tups, (((0, 1), (5, 6)), ((1, 2, 0), (6, 7, 5)))):
        w = K.combine([arrays[i] for i in idx], bounds, 250, 2)
        assert (c.live, c.n_keys, c.overflow) == (w.live, w.n_keys, 0)
        assert bytes(tup) == w.tuple_words.tobytes()
        h = ids.cpu().numpy()
        assert np.array_equal(h[:rows * 2].view(np.uint16), w.ids) and (h[rows * 2:] == GUARD).all()


# ---- 8 .. 10: from pages
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


def _check_groups(keys, n_keys, aggs, groups, mask, key_valid, refs, max_keys):
    order = sorted(groups)
    assert n_keys == len(order) and list(keys) == order
    for j, (a, r) in enumerate(zip(aggs, refs)):
        assert len(a.groups) == max_keys
        assert a.selected == int(mask.sum()) and a.out_of_range == int((mask & ~key_valid).sum())
        for g, key in enumerate(order):
            n_sel, live = groups[key]
            got = a.groups[g]
            assert (got.selected, got.count) == (n_sel, len(live[j])), (j, g)
            if live[j]:
                assert (got.min, got.max, got.sum) == (min(live[j]), max(live[j]), sum(live[j])), (j, g)
        for g in range(len(order), max_keys):
            assert bytes(a.groups[g]._c) == bytes(64), (j, g)


class Pages:
    """the columns of the chains, written once by the oracle: an integer key (plain and as Freq pages), a Utf8 key, a
    filter column and two integer value columns, 20 011 rows; 30 x 20 key pairs, and 3 x 2 in the columns `a3`, `s2`"""

    def __init__(self):
        from tests.test_gpu_freq import sparse
        from tests.test_gpu_key_ids_var import pick, vocab
        rows = self.rows = 20_011
        rng = np.random.default_rng(77)

        def put(name, col, ref_cls=R.Ref, **opt):
            pages, metas = gen.oracle_write(col, **opt)
            setattr(self, name, (col, pages, metas, ref_cls(col, pages, metas)))

        pool = np.arange(30, dtype=np.int64) * (10 ** 12 + 7) - 10 ** 13
        put("a", _column(S.T_I64, pool[rng.integers(0, 30, rows)], rng.random(rows) >= 0.1), max_page_size=4100)
        put("s", KV.column(pick(vocab(20, 3, maxlen=12), rows, 5), rng.random(rows) >= 0.15), KV.Ref, max_page_size=4100)
        put("a3", _column(S.T_I32, np.array([-5, 0, 9], np.int32)[rng.integers(0, 3, rows)], rng.random(rows) >= 0.1), max_page_size=2050)
        put("s2", KV.column(pick([b"no", b"yes"], rows, 6), rng.random(rows) >= 0.1), KV.Ref, max_page_size=4100)
        # the Freq case: one frequent value and a few exceptions, the same values once as Freq pages and once plain
        f = sparse(S.T_I64, rows, 0.05, 2, null_density=0.1, exc_uniq=25)
        put("f", f, max_page_size=2050, force_codec=S.FREQ)
        assert S.FREQ in set(int(x) for x in S.stat_column(f["ptype"], f["nullable"], self.f[1], self.f[2])[0].tolist())
        put("f_plain", f, max_page_size=2050, force_codec=S.NONE)
        put("x", gen.prim(S.T_I32, rows, uniq=100, null_density=0.2, runs=4, seed=1), max_page_size=2050, force_codec=S.RLE)
        put("y", gen.prim(S.T_I64, rows, uniq=5000, null_density=0.1, seed=2), max_page_size=4100, force_codec=S.NONE)
        put("z", gen.prim(S.T_I32, rows, uniq=3000, null_density=0.2, runs=3, seed=3), max_page_size=2050, force_codec=S.DICT)
        xr = self.x[3]
        self.mask = (xr.vals < 60) & xr.valid

    def up(self, ctx, name):
        col, pages, metas, _ = getattr(self, name)
        return upload(ctx, col, pages, metas)

    def pairs(self, a, s):
        """(key tuples per row, key validity) of an integer and a Utf8 key column"""
        ar, sr = getattr(self, a)[3], getattr(self, s)[3]
        return list(zip(ar.vals.tolist(), sr.strs.tolist())), ar.valid & sr.valid


@pytest.fixture(scope="module")
def pg():
    return Pages()


def _chain(ctx, pg, int_name, max_keys=1024):
    """filter, key_ids, key_ids_var, key_combine, aggregate_grouped_large: everything enqueued, nothing synchronized"""
    import strawboat_amd as sb
    sel = sb.filter_columns(ctx, [pg.up(ctx, "x")], [sb.Predicate("lt", 60)])
    ka = sb.key_ids(ctx, [pg.up(ctx, int_name)], sel[0], max_keys=max_keys)[0]
    ks = sb.key_ids_var(ctx, [pg.up(ctx, "s")], sel[0], max_keys=max_keys)[0]
    comb = sb.key_combine(ctx, [ka, ks], max_keys=max_keys)
    aggs = sb.aggregate_grouped_large(ctx, [pg.up(ctx, "y"), pg.up(ctx, "z")], comb.ids, max_keys, sel[0])
    return sel, ka, ks, comb, aggs


def test_one_interval_end_to_end(gpu_ctx, pg):
    r0 = gpu_ctx.replays()
    sel, ka, ks, comb, aggs = _chain(gpu_ctx, pg, "a")
    gpu_ctx.synchronize()   # (the only one)
    assert gpu_ctx.replays() == r0
    assert np.array_equal(sel[0].numpy(), pg.mask)
    keys, valid = pg.pairs("a", "s")
    assert int((pg.mask & ~pg.a[3].valid).sum()) > 0 and int((pg.mask & ~pg.s[3].valid).sum()) > 0
    groups = _dict_group_by(keys, valid, pg.mask, [pg.y[3], pg.z[3]])
    assert len(groups) > 500 and not comb.overflow and comb.live == int((pg.mask & valid).sum())
    _check_groups(comb.keys(), comb.n_keys, aggs, groups, pg.mask, valid, [pg.y[3], pg.z[3]], 1024)
    # the device's tuples are the reference's over the parts' own ids
    K.check(comb, K.combine([ka.ids.cpu().numpy().view(np.uint16), ks.ids.cpu().numpy().view(np.uint16)], (1024, 1024), 1024, 2))


def _snapshot(comb, aggs):
    return (comb.ids.cpu().numpy().tobytes(), comb.tuple_words.tobytes(), comb.live, comb.n_keys, comb.overflow,
            [(a.selected, a.out_of_range, [bytes(g._c) for g in a.groups]) for a in aggs])


def test_replay(gpu_ctx, pg):
    """the integer key as Freq pages: sb_key_ids asks for the replay, and the combine is issued again in its place"""
    r0 = gpu_ctx.replays()
    sel, ka, ks, comb, aggs = _chain(gpu_ctx, pg, "f")
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0 + 1
    replayed = _snapshot(comb, aggs)
    keys, valid = pg.pairs("f", "s")
    groups = _dict_group_by(keys, valid, pg.mask, [pg.y[3], pg.z[3]])
    _check_groups(comb.keys(), comb.n_keys, aggs, groups, pg.mask, valid, [pg.y[3], pg.z[3]], 1024)
    # the same values in plain pages: no replay, and every result identical
    r0 = gpu_ctx.replays()
    sel, ka, ks, comb, aggs = _chain(gpu_ctx, pg, "f_plain")
    gpu_ctx.synchronize()
    assert gpu_ctx.replays() == r0
    assert _snapshot(comb, aggs) == replayed
    # ... and the replayed chain once more: the same bytes
    sel, ka, ks, comb, aggs = _chain(gpu_ctx, pg, "f")
    gpu_ctx.synchronize()
    assert _snapshot(comb, aggs) == replayed


def test_group_by_two_keys(gpu_ctx, pg):
    import strawboat_amd as sb
    from strawboat_amd.group_by import trim
    values = [pg.up(gpu_ctx, "y"), pg.up(gpu_ctx, "z")]
    refs = [pg.y[3], pg.z[3]]
    # about 600 tuples under a filter's selection: the large call
    sel = sb.filter_columns(gpu_ctx, [pg.up(gpu_ctx, "x")], [sb.Predicate("lt", 60)])
    gk, aggs = sb.group_by(gpu_ctx, [pg.up(gpu_ctx, "a"), pg.up(gpu_ctx, "s")], values, sel[0], max_keys=1024)
    gpu_ctx.synchronize()   # (the only one)
    assert isinstance(gk, sb.GroupKeys) and isinstance(gk.parts[0], sb.KeyIds) and isinstance(gk.parts[1], sb.KeyIdsVar)
    keys, valid = pg.pairs("a", "s")
    groups = _dict_group_by(keys, valid, pg.mask, refs)
    assert len(groups) > 500 and not gk.overflow and gk.combined.id_width == 2
    _check_groups(gk.keys, gk.n_keys, aggs, groups, pg.mask, valid, refs, 1024)
    assert [len(t) for t in trim(gk, aggs)] == [len(groups)] * 2
    # 3 x 2 keys under max_keys 16: one-byte ids and the 256-group call; the Utf8 key first
    gk, aggs = sb.group_by(gpu_ctx, (pg.up(gpu_ctx, "s2"), pg.up(gpu_ctx, "a3")), values, sel[0], max_keys=16)
    gpu_ctx.synchronize()
    keys, valid = pg.pairs("a3", "s2")
    keys = [(s, a) for a, s in keys]
    groups = _dict_group_by(keys, valid, pg.mask, refs)
    assert len(groups) == 6 and gk.combined.id_width == 1 and gk.ids.dtype == gk.parts[0].ids.dtype
    _check_groups(gk.keys, gk.n_keys, aggs, groups, pg.mask, valid, refs, 16)
    assert trim(gk, aggs)[0][0].selected == groups[sorted(groups)[0]][0]
    # no selection at all, and no value column
    gk, aggs = sb.group_by(gpu_ctx, [pg.up(gpu_ctx, "a3"), pg.up(gpu_ctx, "s2")], [], None, max_keys=16)
    gpu_ctx.synchronize()
    keys, valid = pg.pairs("a3", "s2")
    assert aggs == [] and gk.keys == sorted(set(k for k, v in zip(keys, valid) if v))
    # an overflow of the combine alone is passed through, not raised; trim refuses
    gk, aggs = sb.group_by(gpu_ctx, [pg.up(gpu_ctx, "a"), pg.up(gpu_ctx, "s")], values, None, max_keys=300)
    gpu_ctx.synchronize()
    assert gk.overflow and gk.combined.overflow and not gk.parts[0].overflow and not gk.parts[1].overflow
    assert aggs[0].rows == pg.rows and len(aggs[0].groups) == 300 and gk.keys == []
    with pytest.raises(ValueError):
        trim(gk, aggs)
    # ... and of a part: 30 integer keys under max_keys 25
    gk, aggs = sb.group_by(gpu_ctx, [pg.up(gpu_ctx, "a"), pg.up(gpu_ctx, "s2")], values, None, max_keys=25)
    gpu_ctx.synchronize()
    assert gk.overflow and gk.parts[0].overflow and aggs[0].rows == pg.rows
    with pytest.raises(ValueError):
        trim(gk, aggs)
    # a single ColumnPages key behaves as before
    kres, aggs = sb.group_by(gpu_ctx, pg.up(gpu_ctx, "a"), values, sel[0], max_keys=1024)
    gpu_ctx.synchronize()
    assert isinstance(kres, sb.KeyIds) and kres.n_keys == 30 and len(aggs) == 2
