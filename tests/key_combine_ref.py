"""The reference of sb_key_combine, in numpy: the live mask from the bounds, the code of a live row (one 10-bit field per
part, part 0 highest), np.unique of the codes for the tuples and np.searchsorted for the ids.  Nothing here touches the
device.

A row is live if every part id is below its part's bound.  The tuples are the distinct tuples of the live rows, ascending
lexicographically with part 0 most significant; a row's id is the position of its tuple among them, all ones in id_width
bytes where the row is not live.  More distinct tuples than max_keys: overflow, and then n_keys, tuples and ids are
unspecified (check() looks at none of them)."""
import numpy as np

ID_NP = {1: np.uint8, 2: np.uint16, 4: np.uint32}
FIELD_BITS = 10


def pack(ids):
    """the code of a tuple of part ids (Python ints), part 0 highest"""
    code = 0
    for v in ids:
        code = (code << FIELD_BITS) | int(v)
    return code


def unpack(code, n_parts):
    return tuple((code >> (FIELD_BITS * (n_parts - 1 - p))) & 1023 for p in range(n_parts))


class Want:
    """what one item of a call must give"""

    def __init__(self, rows, n_parts, live, max_keys, id_width, overflow, tuples, ids):
        self.rows, self.n_parts, self.live = rows, n_parts, live
        self.max_keys, self.id_width, self.overflow = max_keys, id_width, overflow
        self.tuples = tuples   # np.uint32[n_keys, n_parts], ascending (None on overflow)
        self.ids = ids         # np.uint8 / uint16 / uint32 per row (None on overflow)
        self.n_keys = None if overflow else int(tuples.shape[0])

    @property
    def tuple_words(self):
        """the (max_keys, 4) words of `tuples`: zeros in the unused parts and behind n_keys"""
        out = np.zeros((self.max_keys, 4), np.uint32)
        out[:self.n_keys, :self.n_parts] = self.tuples
        return out


def combine(parts, bounds, max_keys, id_width):
    """parts: one unsigned integer array per part, as the device arrays hold them; bounds: the exclusive bound per part"""
    n_parts = len(parts)
    rows = int(parts[0].size)
    live = np.ones(rows, bool)
    code = np.zeros(rows, np.uint64)
    for a, b in zip(parts, bounds):
        a = np.asarray(a).astype(np.uint64)
        live &= a < np.uint64(b)
        code = (code << np.uint64(FIELD_BITS)) | (a & np.uint64(1023))
    codes = np.unique(code[live])
    n_live = int(live.sum())
    if codes.size > max_keys:
        return Want(rows, n_parts, n_live, max_keys, id_width, True, None, None)
    none = (1 << (8 * id_width)) - 1
    ids = np.full(rows, none, ID_NP[id_width])
    ids[live] = np.searchsorted(codes, code[live]).astype(ID_NP[id_width])
    tuples = np.zeros((codes.size, n_parts), np.uint32)
    for p in range(n_parts):
        tuples[:, p] = (codes >> np.uint64(FIELD_BITS * (n_parts - 1 - p))) & np.uint64(1023)
    return Want(rows, n_parts, n_live, max_keys, id_width, False, tuples, ids)


def ids_numpy(got):
    """the ids of a strawboat_amd.key_combine.KeyCombine as unsigned integers of their width"""
    return got.ids.cpu().numpy().view(ID_NP[got.id_width])


def check(got, w, what=""):
    """got: a strawboat_amd.key_combine.KeyCombine after the synchronize.  Every comparison is exact."""
    head = (got.rows, got.live, got.overflow)
    assert head == (w.rows, w.live, w.overflow), "%s: rows / live / overflow %r, want %r" % (what, head, (w.rows, w.live, w.overflow))
    if w.overflow:
        return
    assert got.n_keys == w.n_keys, "%s: n_keys %d, want %d" % (what, got.n_keys, w.n_keys)
    assert got.tuple_words.tobytes() == w.tuple_words.tobytes(), "%s: the words of tuples differ" % what
    assert np.array_equal(got.tuples, w.tuples), what
    ids = ids_numpy(got)
    assert ids.size == w.rows
    bad = np.flatnonzero(ids != w.ids)
    assert bad.size == 0, "%s: %d ids differ, the first at row %d: %d, want %d" % (
        what, bad.size, bad[0] if bad.size else -1, ids[bad[0]] if bad.size else 0, w.ids[bad[0]] if bad.size else 0)
