"""key_combine:: — dense ids of composite keys, on the GPU: GROUP BY a, b and SELECT DISTINCT a, b.

Every key column goes through `key_ids` / `key_ids_var` first; the 2 to 4 id tensors they wrote go in here, and
one call (sb_key_combine in include/strawboat_hip.h) turns them into the sorted distinct tuples of part ids
(`KeyCombine.tuples`, on the host) and a dense tuple id per row (`KeyCombine.ids`, a device tensor), which
`aggregate_grouped` / `aggregate_grouped_large` take as `group_ids`, unchanged.  A row is live when every part id
is below that part's bound; a row that is unselected or null in any key column (all ones there) has no tuple and
gets all ones here too.  The tuples are sorted by part id with part 0 most significant, which is the order of the
key values themselves, since the part ids preserve it.  More than `max_keys` distinct tuples set `overflow`,
which is no error.
"""
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N
from .key_ids import ID_DTYPES, KeyIds, max_keys_limit, narrowest_id_width
from .key_ids_var import KeyIdsVar
from .read import _dev_ptr

MAX_KEYS = N.SB_KEY_MAX_KEYS
MAX_PARTS = N.SB_KEY_COMBINE_MAX_PARTS
_WIDTH_OF = {"torch." + name: w for w, name in ID_DTYPES.items()}


def _is_int(v):
    return not isinstance(v, bool) and isinstance(v, (int, np.integer))


def check_parts(widths: Sequence[int], bounds: Sequence[int], max_keys, id_width):
    """The refusals that need no device and no tensor: the number of parts, their widths and bounds, the ids' width,
    max_keys against it."""
    if not 2 <= len(widths) <= MAX_PARTS or len(bounds) != len(widths):
        raise ValueError("a composite key has 2 .. %d parts, not %d" % (MAX_PARTS, len(widths)))
    for w in widths:
        if isinstance(w, bool) or w not in (1, 2, 4):
            raise ValueError("a part's id width is %r, not 1, 2 or 4" % (w,))
    for b in bounds:
        if not _is_int(b) or not 1 <= b <= MAX_KEYS:
            raise ValueError("a part's bound is %r, not an int in 1 .. %d" % (b, MAX_KEYS))
    if isinstance(id_width, bool) or id_width not in (1, 2, 4):
        raise ValueError("id_width is %r, not 1, 2 or 4" % (id_width,))
    if not _is_int(max_keys) or not 1 <= max_keys <= max_keys_limit(id_width):
        raise ValueError("max_keys is %r, not an int in 1 .. %d (id_width %d)" % (max_keys, max_keys_limit(id_width), id_width))


def _part_of(part):
    """(ids tensor, width, bound, key result or None) of a part: a KeyIds / KeyIdsVar, or a pair (ids tensor, n_ids)"""
    import torch
    if isinstance(part, (KeyIds, KeyIdsVar)):
        return part.ids, part.id_width, part.max_keys, part
    if isinstance(part, (tuple, list)) and len(part) == 2 and isinstance(part[0], torch.Tensor):
        ids, bound = part
        w = _WIDTH_OF.get(str(ids.dtype))
        if w is None:
            raise ValueError("a part's ids are a torch.uint8, uint16 or int32 tensor, not %s" % ids.dtype)
        return ids, w, bound, None
    raise ValueError("a part is a KeyIds, a KeyIdsVar or a pair (ids tensor, n_ids), not %r" % type(part).__name__)


def _check_tensors(ctx, tensors, out, id_width):
    import torch
    rows = tensors[0].numel()
    for t in tensors:
        if t.dim() != 1 or not t.is_contiguous() or t.numel() != rows:
            raise ValueError("the parts' ids are contiguous 1-d tensors of one length")
        if t.device != ctx.torch_device:
            raise ValueError("a part's ids are on %s, the context on %s" % (t.device, ctx.torch_device))
    if out is not None:
        if not isinstance(out, torch.Tensor) or str(out.dtype) != "torch." + ID_DTYPES[id_width]:
            raise ValueError("out is a torch.%s tensor for id_width %d" % (ID_DTYPES[id_width], id_width))
        if out.device != ctx.torch_device:
            raise ValueError("out is on %s, the context on %s" % (out.device, ctx.torch_device))
        if out.dim() != 1 or not out.is_contiguous() or out.numel() < rows:
            raise ValueError("out is a contiguous 1-d tensor of at least %d ids" % rows)
    return rows


class KeyCombine:
    """The tuples and ids of one item; the scalars and `tuples` are valid after Context.synchronize()."""

    def __init__(self, n_parts, max_keys, id_width, cstruct, ids, tuples_buf, sources):
        self.n_parts = n_parts
        self.max_keys = max_keys
        self.id_width = id_width
        self._c = cstruct
        #: torch tensor on the context's device, one id per row, of the dtype KeyIds.ids has for the width
        self.ids = ids
        self._tuples = tuples_buf   # np.uint32[max_keys, 4]
        self._sources = sources     # per part: the KeyIds / KeyIdsVar it came from, or None

    rows = property(lambda self: int(self._c.rows))
    live = property(lambda self: int(self._c.live))
    n_keys = property(lambda self: int(self._c.n_keys))
    overflow = property(lambda self: bool(self._c.overflow))

    @property
    def none(self):
        """the id of a row that is not live: all ones in id_width bytes, as the ids' dtype shows it"""
        return -1 if self.id_width == 4 else (1 << (8 * self.id_width)) - 1

    @property
    def tuple_words(self):
        """all 4 * max_keys words of `tuples` as the library wrote them: zeros in unused parts and behind n_keys"""
        return self._tuples.copy()

    @property
    def tuples(self):
        """the distinct tuples of the live rows, ascending: a (n_keys, n_parts) uint32 array of part ids"""
        n = 0 if self.overflow else self.n_keys
        return self._tuples[:n, :self.n_parts].copy()

    def keys(self):
        """the tuples as the parts' own key values: a list of n_keys tuples (the parts must be key results)"""
        if any(s is None for s in self._sources):
            raise ValueError("keys() needs parts that are KeyIds / KeyIdsVar results")
        if self.overflow or any(s.overflow for s in self._sources):
            raise ValueError("the keys were not delivered: a part or the combine overflowed")
        cols = []
        for s in self._sources:
            k = s.keys
            cols.append(k.tolist() if hasattr(k, "tolist") else list(k))
        return [tuple(cols[p][int(t[p])] for p in range(self.n_parts)) for t in self.tuples]

    def __repr__(self):
        return "KeyCombine(rows=%d, live=%d, n_keys=%d, overflow=%r, n_parts=%d, max_keys=%d, id_width=%d)" % (
            self.rows, self.live, self.n_keys, self.overflow, self.n_parts, self.max_keys, self.id_width)


class KeyCombineBatch:
    """A prepared sb_key_combine call of one or more items: the C descriptors, the ids tensors and the tuples'
    buffers are built once; enqueue() then costs one C call.

    items: a list of items, each a list of 2 .. 4 parts (a KeyIds, a KeyIdsVar, or a pair (ids tensor, n_ids): the
    exclusive bound of a valid id).  max_keys, id_width: one value for all items or one per item; id_width None
    picks the narrowest width that holds max_keys.  out: None, or one ids tensor per item (None entries are
    allocated)."""

    def __init__(self, ctx, items, max_keys=MAX_KEYS, id_width=None, out=None):
        import torch
        n = len(items)
        mks = list(max_keys) if isinstance(max_keys, (list, tuple)) else [max_keys] * n
        ws = list(id_width) if isinstance(id_width, (list, tuple)) else [id_width] * n
        outs = [None] * n if out is None else list(out)
        if len(mks) != n or len(ws) != n:
            raise ValueError("one max_keys and one id_width per item (or one for all)")
        if len(outs) != n:
            raise ValueError("one out tensor per item (or None)")
        parsed, all_rows = [], []
        for i, parts in enumerate(items):   # every refusal that needs no device, before anything is enqueued
            if not isinstance(parts, (list, tuple)):
                raise ValueError("an item is a list of parts")
            if not 2 <= len(parts) <= MAX_PARTS:
                raise ValueError("a composite key has 2 .. %d parts, not %d" % (MAX_PARTS, len(parts)))
            ps = [_part_of(p) for p in parts]
            if ws[i] is None and _is_int(mks[i]):
                ws[i] = narrowest_id_width(mks[i])
            check_parts([p[1] for p in ps], [p[2] for p in ps], mks[i], ws[i])
            all_rows.append(_check_tensors(ctx, [p[0] for p in ps], outs[i], ws[i]))
            parsed.append(ps)
        arr = (N.KeyCombineItemC * n)()
        keep, res = [], []
        for i, ps in enumerate(parsed):
            c = arr[i]
            rows, w, mk = all_rows[i], int(ws[i]), int(mks[i])
            c.rows, c.n_parts, c.id_width = rows, len(ps), w
            for p, (t, pw, bound, _) in enumerate(ps):
                keep.append(t)
                c.part_ids[p] = _dev_ptr(t).value
                c.part_capacity[p] = t.numel() * pw
                c.part_width[p] = pw
                c.part_keys[p] = int(bound)
            ids = outs[i]
            if ids is None:
                ids = torch.empty(rows, dtype=getattr(torch, ID_DTYPES[w]), device=ctx.torch_device)
            keep.append(ids)
            c.ids = _dev_ptr(ids)
            c.ids_capacity = ids.numel() * w
            c.max_keys, c.reserved = mk, 0
            tbuf = np.zeros((mk, 4), np.uint32)
            keep.append(tbuf)
            c.tuples = tbuf.ctypes.data
            res.append(KeyCombine(len(ps), mk, w, c, ids[:rows], tbuf, [p[3] for p in ps]))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.results = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_key_combine(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.results


def key_combine(ctx, parts: List[object], max_keys: int = MAX_KEYS, id_width: Optional[int] = None, out=None) -> KeyCombine:
    """Enqueue the tuples and ids of one composite key on ctx's stream, behind the key_ids / key_ids_var calls
    that write the parts; `ids` are ordered on that stream, the scalars and `tuples` come with ctx.synchronize()."""
    return KeyCombineBatch(ctx, [parts], max_keys, id_width, None if out is None else [out]).enqueue()[0]
