"""key_ids_var:: — the distinct keys of a Binary / Utf8 key column and a dense group id per row, on the GPU.

`key_ids` for string keys: SELECT country, ... WHERE x < 5 GROUP BY country, SELECT DISTINCT status WHERE ...
The pages of the key column and the selection bitmap go in; the distinct byte strings of the live rows come
back on the host in byte order (`KeyIdsVar.keys`: bytes unsigned, a proper prefix first), and every row gets
the position of its string among them in a device tensor (`KeyIdsVar.ids`), all ones for a row that is not
selected or null (sb_key_ids_var in include/strawboat_hip.h).  The ids are what `aggregate_grouped` takes as
`group_ids`; `as_in_list()` is what `filter_in` takes as the list of a semi-join.  More than `max_keys`
distinct strings set `overflow_keys`, keys that need more than `key_bytes` bytes set `overflow_bytes` (the ids,
the offsets and `keys_len` are valid then: `keys_len` says what to ask for); neither is an error.
"""
from typing import List, Optional

import numpy as np

from . import _native as N
from .filter import Selection
from .filter_in import InList
from .key_ids import ID_DTYPES, _check_out, max_keys_limit, narrowest_id_width
from .read import ColumnPages, _dev_ptr
from .read_selected import _bitmap_of, selection_bytes
from .types import PhysicalType as _P

MAX_KEYS = N.SB_KEY_MAX_KEYS
MAX_KEY_BYTES = N.SB_KEY_VAR_MAX_BYTES
BINARY_TYPES = (_P.BINARY, _P.LARGE_BINARY)


def check_column(physical_type, rows: int, bitmap_bytes: Optional[int], max_keys, id_width, key_bytes):
    """The refusals that need no device: the type, the width, max_keys, key_bytes, the bitmap's length."""
    if physical_type not in BINARY_TYPES:
        raise ValueError("key_ids_var takes Binary / LargeBinary columns, not physical type %d (integers: key_ids)" % physical_type)
    if isinstance(id_width, bool) or id_width not in (1, 2, 4):
        raise ValueError("id_width is %r, not 1, 2 or 4" % (id_width,))
    if isinstance(max_keys, bool) or not isinstance(max_keys, (int, np.integer)) or not 1 <= max_keys <= max_keys_limit(id_width):
        raise ValueError("max_keys is %r, not an int in 1 .. %d (id_width %d)" % (max_keys, max_keys_limit(id_width), id_width))
    if isinstance(key_bytes, bool) or not isinstance(key_bytes, (int, np.integer)) or not 0 <= key_bytes <= MAX_KEY_BYTES:
        raise ValueError("key_bytes is %r, not an int in 0 .. %d" % (key_bytes, MAX_KEY_BYTES))
    if bitmap_bytes is not None and bitmap_bytes < selection_bytes(rows):
        raise ValueError("the selection bitmap has %d bytes, %d rows need %d (4*ceil(rows/32))"
                         % (bitmap_bytes, rows, selection_bytes(rows)))


class KeyIdsVar:
    """The keys and ids of one column; the scalars, `keys` and `key_offsets` are valid after Context.synchronize()."""

    def __init__(self, physical_type, max_keys, id_width, cstruct, ids, offsets_buf, keys_buf, keys_capacity):
        self.physical_type = physical_type
        self.max_keys = max_keys
        self.id_width = id_width
        self._c = cstruct
        #: torch tensor on the context's device, one id per row, as KeyIds.ids
        self.ids = ids
        self._offsets = offsets_buf   # np.uint64[max_keys + 1]
        self._keys = keys_buf         # (c_uint8 * max(1, key_bytes))
        self.keys_capacity = keys_capacity

    rows = property(lambda self: int(self._c.rows))
    selected = property(lambda self: int(self._c.selected))
    count = property(lambda self: int(self._c.count))
    n_keys = property(lambda self: int(self._c.n_keys))
    keys_len = property(lambda self: int(self._c.keys_len))
    overflow = property(lambda self: int(self._c.overflow))
    overflow_keys = property(lambda self: bool(self._c.overflow & N.SB_KEY_OVERFLOW_KEYS))
    overflow_bytes = property(lambda self: bool(self._c.overflow & N.SB_KEY_OVERFLOW_BYTES))

    @property
    def none(self):
        """the id of a row that is not live: all ones in id_width bytes, as the ids' dtype shows it"""
        return -1 if self.id_width == 4 else (1 << (8 * self.id_width)) - 1

    @property
    def key_offsets(self):
        """all max_keys + 1 offsets as the library wrote them: [0] == 0, keys_len behind n_keys"""
        return self._offsets.copy()

    @property
    def key_bytes(self):
        """all bytes of the keys' buffer as the library wrote them: zeros behind keys_len"""
        return bytes(self._keys)[:self.keys_capacity]

    @property
    def keys(self):
        """the distinct strings of the live rows in byte order, a list of `bytes` (empty on either overflow)"""
        if self.overflow:
            return []
        raw, o = self.key_bytes, self._offsets
        return [raw[int(o[i]):int(o[i + 1])] for i in range(self.n_keys)]

    def as_in_list(self, negate=False):
        """the keys as the list `filter_in` takes: the semi-join of another column against this one's keys"""
        if self.overflow:
            raise ValueError("the keys were not delivered (overflow %d)" % self.overflow)
        return InList(self.keys, negate)

    def __repr__(self):
        return "KeyIdsVar(rows=%d, selected=%d, count=%d, n_keys=%d, keys_len=%d, overflow=%d, max_keys=%d, id_width=%d)" % (
            self.rows, self.selected, self.count, self.n_keys, self.keys_len, self.overflow, self.max_keys, self.id_width)


class KeyIdsVarBatch:
    """A prepared sb_key_ids_var call: the C descriptors, the ids tensors and the keys' buffers are built
    once; enqueue() then costs one C call.

    max_keys, id_width, key_bytes: one value for all columns or one per column; id_width None picks the
    narrowest width that holds max_keys; key_bytes is the capacity of the keys' bytes (at most 1 MiB).
    selection, out: as in KeyIdsBatch.  stage_capacity: as in filter_columns."""

    def __init__(self, ctx, columns: List[ColumnPages], selection=None, max_keys=256, id_width=None, key_bytes=65536, out=None,
                 stage_capacity=None):
        import torch
        from .read import _prepare
        n = len(columns)
        mks = list(max_keys) if isinstance(max_keys, (list, tuple)) else [max_keys] * n
        ws = list(id_width) if isinstance(id_width, (list, tuple)) else [id_width] * n
        kbs = list(key_bytes) if isinstance(key_bytes, (list, tuple)) else [key_bytes] * n
        outs = [None] * n if out is None else list(out)
        if selection is None or isinstance(selection, (Selection, torch.Tensor)):
            selections = [selection] * n
        else:
            selections = list(selection)
        if len(mks) != n or len(ws) != n or len(kbs) != n:
            raise ValueError("one max_keys, one id_width and one key_bytes per column (or one for all)")
        if len(selections) != n:
            raise ValueError("one selection per column (or one for all, or None)")
        if len(outs) != n:
            raise ValueError("one out tensor per column (or None)")
        if stage_capacity is not None and len(stage_capacity) != n:
            raise ValueError("one stage_capacity per column")
        bitmaps, all_rows = [], []
        for i, (col, sel) in enumerate(zip(columns, selections)):   # every refusal that needs no device, before anything is enqueued
            bitmap = None if sel is None else _bitmap_of(ctx, sel)
            m = col.metas_array()
            rows = int(m[:, 1].sum()) if m.shape[0] else 0
            if ws[i] is None and not isinstance(mks[i], bool) and isinstance(mks[i], (int, np.integer)):
                ws[i] = narrowest_id_width(mks[i])
            check_column(col.physical_type, rows, None if bitmap is None else bitmap.numel(), mks[i], ws[i], kbs[i])
            if outs[i] is not None:
                _check_out(ctx, outs[i], rows, ws[i])
            bitmaps.append(bitmap)
            all_rows.append(rows)
        rarr, keep = _prepare(ctx, columns)
        arr = (N.ColumnKeyIdsVarC * n)()
        res = []
        for i, col in enumerate(columns):
            c, r = arr[i], rarr[i]
            c.physical_type, c.is_nullable = r.physical_type, r.is_nullable
            c.pages, c.pages_len, c.metas, c.n_pages = r.pages, r.pages_len, r.metas, r.n_pages
            c.page_offsets = r.page_offsets
            keep.append(bitmaps[i])
            # (a bitmap of no bytes — a column without rows — has no address: the same as no selection)
            c.selection = _dev_ptr(bitmaps[i])
            c.selection_capacity = bitmaps[i].numel() if bitmaps[i] is not None else 0
            w, mk, kb = int(ws[i]), int(mks[i]), int(kbs[i])
            ids = outs[i]
            if ids is None:
                ids = torch.empty(all_rows[i], dtype=getattr(torch, ID_DTYPES[w]), device=ctx.torch_device)
            keep.append(ids)
            c.ids = _dev_ptr(ids)
            c.ids_capacity = ids.numel() * w
            c.id_width, c.max_keys, c.reserved = w, mk, 0
            obuf = np.zeros(mk + 1, dtype=np.uint64)
            kbuf = (N.C.c_uint8 * max(1, kb))()
            keep += [obuf, kbuf]
            c.key_offsets = obuf.ctypes.data
            c.keys = N.C.addressof(kbuf)
            c.keys_capacity = kb
            c.stage_capacity = int(stage_capacity[i]) if stage_capacity is not None else 0
            res.append(KeyIdsVar(col.physical_type, mk, w, c, ids[:all_rows[i]], obuf, kbuf, kb))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.results = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_key_ids_var(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.results


def key_ids_var(ctx, columns: List[ColumnPages], selection=None, max_keys=256, id_width=None, key_bytes=65536, out=None) -> List[KeyIdsVar]:
    """Enqueue the keys and ids of the Binary / Utf8 columns[i] under selection[i] (or one selection for
    all, or None: every row) on ctx's stream, behind the filter calls that write the bitmaps; `ids` are
    ordered on that stream, the scalars, `keys` and `key_offsets` come with ctx.synchronize()."""
    return KeyIdsVarBatch(ctx, columns, selection, max_keys, id_width, key_bytes, out).enqueue()
