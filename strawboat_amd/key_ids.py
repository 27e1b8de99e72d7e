"""key_ids:: — the distinct keys of an integer key column and a dense group id per row, on the GPU.

The link between `filter_columns` and `aggregate_grouped`: SELECT k, ... WHERE x < 5 GROUP BY k for a key
column whose values are no dense small integers (sparse keys, dates, status codes), and SELECT DISTINCT k
WHERE ...  The pages of k and the selection bitmap go in; the sorted distinct values of the live rows come
back on the host (`KeyIds.keys`), and every row gets the position of its value among them in a device
tensor (`KeyIds.ids`), all ones for a row that is not selected or null (sb_key_ids in
include/strawboat_hip.h).  The ids are what `aggregate_grouped` takes as `group_ids`, unchanged; its
`out_of_range` then counts the selected rows whose key is null.  More than `max_keys` distinct values set
`overflow`, which is no error: an engine probes a column's cardinality this way and falls back.
"""
from typing import List, Optional

import numpy as np

from . import _native as N
from .filter import Selection
from .read import ColumnPages, _dev_ptr
from .read_selected import NUMPY_DTYPES, _bitmap_of, selection_bytes
from .types import PhysicalType as _P

MAX_KEYS = N.SB_KEY_MAX_KEYS
INTEGER_TYPES = (_P.INT8, _P.INT16, _P.INT32, _P.INT64, _P.UINT8, _P.UINT16, _P.UINT32, _P.UINT64)
# the ids' tensor dtype per width: the dtypes aggregate_grouped takes as group ids.  int32 holds the unsigned bits (torch
# computes little on uint32): the all-ones id reads as -1 there, as 255 / 65535 in the narrower two.
ID_DTYPES = {1: "uint8", 2: "uint16", 4: "int32"}


def narrowest_id_width(max_keys: int) -> int:
    """the narrowest id width whose all-ones value is no id: 1 up to 255 keys, 2 beyond"""
    return 1 if max_keys <= 255 else 2


def max_keys_limit(id_width: int) -> int:
    return min(MAX_KEYS, (1 << (8 * id_width)) - 1)


def check_column(physical_type, rows: int, bitmap_bytes: Optional[int], max_keys, id_width):
    """The refusals that need no device: the type, the width, max_keys, the bitmap's length."""
    if physical_type not in INTEGER_TYPES:
        raise ValueError("key ids are implemented for 8- to 64-bit integers, not physical type %d" % physical_type)
    if isinstance(id_width, bool) or id_width not in (1, 2, 4):
        raise ValueError("id_width is %r, not 1, 2 or 4" % (id_width,))
    if isinstance(max_keys, bool) or not isinstance(max_keys, (int, np.integer)) or not 1 <= max_keys <= max_keys_limit(id_width):
        raise ValueError("max_keys is %r, not an int in 1 .. %d (id_width %d)" % (max_keys, max_keys_limit(id_width), id_width))
    if bitmap_bytes is not None and bitmap_bytes < selection_bytes(rows):
        raise ValueError("the selection bitmap has %d bytes, %d rows need %d (4*ceil(rows/32))"
                         % (bitmap_bytes, rows, selection_bytes(rows)))


def _check_out(ctx, out, rows: int, id_width: int):
    import torch
    if not isinstance(out, torch.Tensor) or str(out.dtype) != "torch." + ID_DTYPES[id_width]:
        raise ValueError("out is a torch.%s tensor for id_width %d" % (ID_DTYPES[id_width], id_width))
    if out.device != ctx.torch_device:
        raise ValueError("out is on %s, the context on %s" % (out.device, ctx.torch_device))
    if out.dim() != 1 or not out.is_contiguous() or out.numel() < rows:
        raise ValueError("out is a contiguous 1-d tensor of at least %d ids" % rows)


class KeyIds:
    """The keys and ids of one column; the scalars and `keys` are valid after Context.synchronize()."""

    def __init__(self, physical_type, max_keys, id_width, cstruct, ids, keys_buf):
        self.physical_type = physical_type
        self.max_keys = max_keys
        self.id_width = id_width
        self._c = cstruct
        #: torch tensor on the context's device, one id per row: uint8 (id_width 1), uint16 (2) or int32 (4, the
        #: unsigned bits).  Written by the call's kernels: ordered behind them on the context's stream.
        self.ids = ids
        self._keys = keys_buf   # (c_uint8 * (8 * max_keys))

    rows = property(lambda self: int(self._c.rows))
    selected = property(lambda self: int(self._c.selected))
    count = property(lambda self: int(self._c.count))
    n_keys = property(lambda self: int(self._c.n_keys))
    overflow = property(lambda self: bool(self._c.overflow))

    @property
    def none(self):
        """the id of a row that is not live: all ones in id_width bytes, as the ids' dtype shows it"""
        return -1 if self.id_width == 4 else (1 << (8 * self.id_width)) - 1

    @property
    def key_bytes(self):
        """all 8 * max_keys bytes of `keys` as the library wrote them: zeros behind n_keys"""
        return bytes(self._keys)

    @property
    def keys(self):
        """the distinct values of the live rows, ascending, as an array of the column's dtype (length n_keys)"""
        dt = np.dtype(NUMPY_DTYPES[self.physical_type])
        n = 0 if self.overflow else self.n_keys
        slots = np.frombuffer(self.key_bytes, dtype=np.uint8).reshape(self.max_keys, 8)[:n]
        return slots[:, :dt.itemsize].copy().view(dt).reshape(n)

    def __repr__(self):
        return "KeyIds(rows=%d, selected=%d, count=%d, n_keys=%d, overflow=%r, max_keys=%d, id_width=%d)" % (
            self.rows, self.selected, self.count, self.n_keys, self.overflow, self.max_keys, self.id_width)


class KeyIdsBatch:
    """A prepared key-id call: the C descriptors, the ids tensors and the keys' buffers are built once;
    enqueue() then costs one C call.

    max_keys, id_width: one value for all columns or one per column; id_width None picks the narrowest
    width that holds max_keys.  selection: one per column, a single one for all columns, or None (every
    row); each a filter.Selection or a contiguous uint8 tensor on the context's device.  out: None, or
    one ids tensor per column to write into (None entries are allocated)."""

    def __init__(self, ctx, columns: List[ColumnPages], selection=None, max_keys=256, id_width=None, out=None):
        import torch
        from .read import _prepare
        n = len(columns)
        mks = list(max_keys) if isinstance(max_keys, (list, tuple)) else [max_keys] * n
        ws = list(id_width) if isinstance(id_width, (list, tuple)) else [id_width] * n
        outs = [None] * n if out is None else list(out)
        if selection is None or isinstance(selection, (Selection, torch.Tensor)):
            selections = [selection] * n
        else:
            selections = list(selection)
        if len(mks) != n or len(ws) != n:
            raise ValueError("one max_keys and one id_width per column (or one for all)")
        if len(selections) != n:
            raise ValueError("one selection per column (or one for all, or None)")
        if len(outs) != n:
            raise ValueError("one out tensor per column (or None)")
        bitmaps, all_rows = [], []
        for i, (col, sel) in enumerate(zip(columns, selections)):   # every refusal that needs no device, before anything is enqueued
            bitmap = None if sel is None else _bitmap_of(ctx, sel)
            m = col.metas_array()
            rows = int(m[:, 1].sum()) if m.shape[0] else 0
            if ws[i] is None and not isinstance(mks[i], bool) and isinstance(mks[i], (int, np.integer)):
                ws[i] = narrowest_id_width(mks[i])
            check_column(col.physical_type, rows, None if bitmap is None else bitmap.numel(), mks[i], ws[i])
            if outs[i] is not None:
                _check_out(ctx, outs[i], rows, ws[i])
            bitmaps.append(bitmap)
            all_rows.append(rows)
        rarr, keep = _prepare(ctx, columns)
        arr = (N.ColumnKeyIdsC * n)()
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
            w, mk = int(ws[i]), int(mks[i])
            ids = outs[i]
            if ids is None:
                ids = torch.empty(all_rows[i], dtype=getattr(torch, ID_DTYPES[w]), device=ctx.torch_device)
            keep.append(ids)
            c.ids = _dev_ptr(ids)
            c.ids_capacity = ids.numel() * w
            c.id_width, c.max_keys, c.reserved = w, mk, 0
            kbuf = (N.C.c_uint8 * (8 * mk))()
            keep.append(kbuf)
            c.keys = N.C.addressof(kbuf)
            res.append(KeyIds(col.physical_type, mk, w, c, ids[:all_rows[i]], kbuf))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.results = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_key_ids(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.results


def key_ids(ctx, columns: List[ColumnPages], selection=None, max_keys=256, id_width=None, out=None) -> List[KeyIds]:
    """Enqueue the keys and ids of columns[i] under selection[i] (or one selection for all, or None: every
    row) on ctx's stream, behind the filter calls that write the bitmaps; `ids` are ordered on that stream,
    the scalars and `keys` come with ctx.synchronize()."""
    return KeyIdsBatch(ctx, columns, selection, max_keys, id_width, out).enqueue()
