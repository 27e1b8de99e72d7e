"""The reference of sb_key_ids_var: the ORACLE's decode of the pages (gen.oracle_read: offsets, values, validity) turned
into a list of `bytes`, np.unique on an object array for the keys and its return_inverse for the ids.  Nothing here touches
the device or its decoder.

A row is live if its selection bit is set and it is not null.  The keys are the distinct byte strings of the live rows;
np.unique orders `bytes` objects as Python does: bytes unsigned, a proper prefix first — the order of SB_PRED_LT of
sb_filter_columns_var, e.g. [b'', b'a', b'a\\x00', b'ab', b'a\\xff', b'b', b'\\x80'] (tests/test_key_ids_var_host.py).  A row's id
is the position of its string among the keys, all ones in id_width bytes where the row is not live.  More keys than max_keys:
SB_KEY_OVERFLOW_KEYS, and n_keys, keys_len, the key buffers and ids are unspecified (check() looks at none of them).  Keys
that fit max_keys but not keys_capacity: SB_KEY_OVERFLOW_BYTES, and everything but the bytes of `keys` is checked."""
import numpy as np

from oracle import sbo as S
from tests import gen

ID_NP = {1: np.uint8, 2: np.uint16, 4: np.uint32}
OVER_KEYS, OVER_BYTES = 1, 2


def column(strs, validity=None, large=False):
    """a binary column of these strings (null rows keep their bytes)"""
    lens = np.array([len(s) for s in strs], np.int64)
    offs = np.zeros(len(strs) + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    data = np.frombuffer(b"".join(strs), np.uint8).copy() if len(strs) else np.zeros(0, np.uint8)
    return dict(ptype=S.T_BIN64 if large else S.T_BIN32, nullable=validity is not None, rows=len(strs), values=data,
                validity=None if validity is None else gen.pack_bits(validity), offsets=offs.astype(np.int64 if large else np.int32))


class Ref:
    """the oracle's decode of a binary column, computed once: `strs` (an object array of bytes, one per row) and `valid`"""

    def __init__(self, col, pages, metas):
        want = gen.oracle_read(col, pages, metas)
        rows = self.rows = int(want["rows"])
        self.valid = (np.unpackbits(np.asarray(want["validity"], np.uint8), bitorder="little")[:rows].astype(bool)
                      if col["nullable"] else np.ones(rows, bool))
        odt = np.int64 if col["ptype"] == S.T_BIN64 else np.int32
        offs = np.ascontiguousarray(want["offsets"]).view(np.uint8).reshape(-1).view(odt)[:rows + 1].astype(np.int64)
        data = np.asarray(want["values"], np.uint8).tobytes()
        self.strs = np.empty(rows, object)
        for i in range(rows):
            self.strs[i] = data[offs[i]:offs[i + 1]]


class Want:
    """what one column of a call must give"""

    def __init__(self, rows, selected, count, max_keys, id_width, keys_capacity, keys, ids):
        self.rows, self.selected, self.count = rows, selected, count
        self.max_keys, self.id_width, self.keys_capacity = max_keys, id_width, keys_capacity
        self.overflow = 0
        self.keys = self.ids = self.n_keys = self.keys_len = self.key_offsets = None
        if len(keys) > max_keys:
            self.overflow = OVER_KEYS
            return
        self.keys, self.ids, self.n_keys = keys, ids, len(keys)
        self.keys_len = sum(len(k) for k in keys)
        self.key_offsets = np.full(max_keys + 1, self.keys_len, np.uint64)
        self.key_offsets[:self.n_keys + 1] = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.uint64)
        if self.keys_len > keys_capacity:
            self.overflow = OVER_BYTES

    @property
    def key_bytes(self):
        """the keys_capacity bytes of `keys`: the keys back to back, zeros behind keys_len (no overflow)"""
        return b"".join(self.keys) + bytes(self.keys_capacity - self.keys_len)


def key_ids_values(strs, live, selected, max_keys, id_width, keys_capacity=65536):
    """strs: an object array of bytes (any bytes in null rows); live: bool per row"""
    rows = int(live.size)
    none = (1 << (8 * id_width)) - 1
    ids = np.full(rows, none, ID_NP[id_width])
    keys = []
    if live.any():
        u, inv = np.unique(strs[live], return_inverse=True)
        keys = list(u)
        if len(keys) <= max_keys:
            ids[live] = inv.astype(ID_NP[id_width])
    return Want(rows, selected, int(live.sum()), max_keys, id_width, keys_capacity, keys, ids)


def want(ref, mask, max_keys, id_width, keys_capacity=65536):
    """the Want of a column (a Ref) under a selection (a bool per row, or None: every row)"""
    sel = np.ones(ref.rows, bool) if mask is None else np.asarray(mask, bool)[:ref.rows]
    return key_ids_values(ref.strs, sel & ref.valid, int(sel.sum()), max_keys, id_width, keys_capacity)


def ids_numpy(got):
    """the ids of a strawboat_amd.key_ids_var.KeyIdsVar as unsigned integers of their width"""
    return got.ids.cpu().numpy().view(ID_NP[got.id_width])


def check(got, w, what=""):
    """got: a strawboat_amd.key_ids_var.KeyIdsVar after the synchronize.  Every comparison is exact."""
    head = (got.rows, got.selected, got.count, got.overflow)
    assert head == (w.rows, w.selected, w.count, w.overflow), (
        "%s: rows / selected / count / overflow %r, want %r" % (what, head, (w.rows, w.selected, w.count, w.overflow)))
    if w.overflow & OVER_KEYS:
        return
    assert (got.n_keys, got.keys_len) == (w.n_keys, w.keys_len), "%s: n_keys / keys_len %r, want %r" % (
        what, (got.n_keys, got.keys_len), (w.n_keys, w.keys_len))
    assert np.array_equal(got.key_offsets, w.key_offsets), "%s: key_offsets differ" % what
    if not w.overflow:
        assert got.keys == w.keys, "%s: the keys differ" % what
        assert got.key_bytes == w.key_bytes, "%s: the bytes of keys differ (zeros behind keys_len)" % what
    ids = ids_numpy(got)
    assert ids.size == w.rows
    bad = np.flatnonzero(ids != w.ids)
    assert bad.size == 0, "%s: %d ids differ, the first at row %d: %d, want %d" % (
        what, bad.size, bad[0] if bad.size else -1, ids[bad[0]] if bad.size else 0, w.ids[bad[0]] if bad.size else 0)
