"""key_lookup:: — the ids a given list assigns to the rows of a key column, on the GPU.

`key_ids` / `key_ids_var` discover the distinct keys of one call's rows and number them by rank, so their ids mean
something within that call only.  Here the caller hands in the list: up to 1024 values per column, and (optionally)
the id of each.  Every row gets the id of its value, all ones for a row that is not selected, is null, or whose value
is not in the list (sb_key_lookup in include/strawboat_hip.h).  That is

  * a join against a small dimension: `fact.fk = dim.pk`, and with `value_ids` many-to-one (`nation -> region`) the
    ids are the group ids of `GROUP BY dim.attr` directly;
  * ids that are comparable between calls: two row groups, two files or the page ranges of two ranks looked up against
    one list give index-aligned grouped results, which add;
  * GROUP BY over a key set that is known, without the discovery walk, table and sort of `key_ids`.

The ids are what `aggregate_grouped` / `aggregate_grouped_large` take as `group_ids`, unchanged; rows without an id
arrive in their `out_of_range` (inner-join semantics).
"""
import ctypes as C
from typing import List, Optional

import numpy as np

from . import _native as N
from .filter import Selection
from .filter_in import InList, pack_list
from .key_ids import ID_DTYPES, INTEGER_TYPES, KeyIds, _check_out
from .key_ids_var import BINARY_TYPES, KeyIdsVar
from .read import ColumnPages, _dev_ptr
from .read_selected import NUMPY_DTYPES, _bitmap_of, selection_bytes

MAX_VALUES = N.SB_KEY_MAX_KEYS


def id_none(id_width: int) -> int:
    """all ones in id_width bytes: the id no list may hand out"""
    return (1 << (8 * id_width)) - 1


def narrowest_id_width(largest_id: int) -> int:
    """the narrowest width whose all-ones value is above the largest id"""
    return 1 if largest_id < 0xFF else 2 if largest_id < 0xFFFF else 4


def list_values(physical_type, values):
    """The list of one column as Python values: a numpy array of the column's dtype, a sequence of bytes / str, an
    InList, or a finished KeyIds / KeyIdsVar (its keys)."""
    if isinstance(values, KeyIds):
        if values.overflow:
            raise ValueError("the keys were not delivered (overflow)")
        values = values.keys
    elif isinstance(values, KeyIdsVar):
        values = values.as_in_list().values
    elif isinstance(values, InList):
        if values.negate:
            raise ValueError("a negated list assigns no ids")
        values = values.values
    if physical_type in INTEGER_TYPES:
        dt = np.dtype(NUMPY_DTYPES[physical_type])
        if isinstance(values, np.ndarray):
            if values.dtype != dt or values.ndim != 1:
                raise ValueError("values is a 1-d %s array for this column, not %s%r" % (dt, values.dtype, values.shape))
            return values
        vals = list(values)
        for v in vals:
            if isinstance(v, (str, bytes, bytearray, memoryview, bool)) or not isinstance(v, (int, np.integer)):
                raise ValueError("value %r is not an integer" % (v,))
            if not np.iinfo(dt).min <= int(v) <= np.iinfo(dt).max:
                raise ValueError("value %r does not fit %s" % (v, dt))
        return np.array(vals, dtype=dt)
    if physical_type in BINARY_TYPES:
        if isinstance(values, np.ndarray):
            raise ValueError("values of a binary column are bytes / str, not an array")
        return list(values)
    raise ValueError("key lookup is implemented for 8- to 64-bit integers and Binary / LargeBinary, not physical type %d" % physical_type)


def check_column(physical_type, rows: int, bitmap_bytes: Optional[int], n_values: int, value_ids, id_width):
    """The refusals that need no device: the type, the list's length, the ids, the width, the bitmap's length.
    Returns (value_ids as a uint32 array or None, id_width)."""
    if physical_type not in INTEGER_TYPES and physical_type not in BINARY_TYPES:
        raise ValueError("key lookup is implemented for 8- to 64-bit integers and Binary / LargeBinary, not physical type %d" % physical_type)
    if n_values > MAX_VALUES:
        raise ValueError("a lookup list has at most %d values, not %d" % (MAX_VALUES, n_values))
    ids = None
    if value_ids is not None:
        raw = list(value_ids.tolist() if isinstance(value_ids, np.ndarray) else value_ids)
        if len(raw) != n_values:
            raise ValueError("%d value_ids for %d values" % (len(raw), n_values))
        for v in raw:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) < 0xFFFFFFFF:
                raise ValueError("value id %r is not an int in 0 .. 2^32 - 2" % (v,))
        ids = np.array(raw, dtype=np.uint32)
    largest = (int(ids.max()) if ids is not None and n_values else n_values - 1 if n_values else 0)
    if id_width is None:
        id_width = narrowest_id_width(largest)
    if isinstance(id_width, bool) or not isinstance(id_width, (int, np.integer)) or id_width not in (1, 2, 4):
        raise ValueError("id_width is %r, not 1, 2 or 4" % (id_width,))
    if largest >= id_none(id_width):
        raise ValueError("the id %d is all ones of id_width %d or does not fit it" % (largest, id_width))
    if bitmap_bytes is not None and bitmap_bytes < selection_bytes(rows):
        raise ValueError("the selection bitmap has %d bytes, %d rows need %d (4*ceil(rows/32))"
                         % (bitmap_bytes, rows, selection_bytes(rows)))
    return ids, int(id_width)


class KeyLookup:
    """The ids of one column; the scalars are valid after Context.synchronize()."""

    def __init__(self, physical_type, id_width, cstruct, ids):
        self.physical_type = physical_type
        self.id_width = id_width
        self._c = cstruct
        #: torch tensor on the context's device, one id per row: uint8 (id_width 1), uint16 (2) or int32 (4, the
        #: unsigned bits).  Written by the call's kernels: ordered behind them on the context's stream.
        self.ids = ids

    rows = property(lambda self: int(self._c.rows))
    selected = property(lambda self: int(self._c.selected))
    count = property(lambda self: int(self._c.count))
    matched = property(lambda self: int(self._c.matched))

    @property
    def none(self):
        """the id of a row without one: all ones in id_width bytes, as the ids' dtype shows it"""
        return -1 if self.id_width == 4 else id_none(self.id_width)

    def __repr__(self):
        return "KeyLookup(rows=%d, selected=%d, count=%d, matched=%d, id_width=%d)" % (
            self.rows, self.selected, self.count, self.matched, self.id_width)


class KeyLookupBatch:
    """A prepared key-lookup call: the C descriptors, the packed lists and the ids tensors are built once; enqueue()
    then costs one C call.

    values: one list per column (list_values says what a list may be).  value_ids: None (a value's id is its
    position in the list), or per column None or one id per value; several values may share an id.  id_width: one
    value for all columns or one per column; None picks the narrowest width that holds the column's largest id.
    selection: one per column, a single one for all columns, or None (every row).  out: None, or one ids tensor per
    column to write into (None entries are allocated).  Numeric and binary columns may share a call."""

    def __init__(self, ctx, columns: List[ColumnPages], values, value_ids=None, selection=None, id_width=None, out=None,
                 stage_capacity=None):
        import torch
        from .read import _prepare
        n = len(columns)
        lists = list(values)
        vids = [None] * n if value_ids is None else list(value_ids)
        ws = list(id_width) if isinstance(id_width, (list, tuple)) else [id_width] * n
        outs = [None] * n if out is None else list(out)
        if selection is None or isinstance(selection, (Selection, torch.Tensor)):
            selections = [selection] * n
        else:
            selections = list(selection)
        if len(lists) != n:
            raise ValueError("one list of values per column")
        if len(vids) != n:
            raise ValueError("one value_ids per column (or None)")
        if len(ws) != n:
            raise ValueError("one id_width per column (or one for all)")
        if len(selections) != n:
            raise ValueError("one selection per column (or one for all, or None)")
        if len(outs) != n:
            raise ValueError("one out tensor per column (or None)")
        if stage_capacity is not None and len(stage_capacity) != n:
            raise ValueError("one stage_capacity per column")
        bitmaps, all_rows, packed, id_arrays = [], [], [], []
        for i, (col, sel) in enumerate(zip(columns, selections)):   # every refusal that needs no device, before anything is enqueued
            if not isinstance(col, ColumnPages):
                raise ValueError("a column is a ColumnPages, not %r" % type(col).__name__)
            if col.physical_type not in INTEGER_TYPES and col.physical_type not in BINARY_TYPES:
                raise ValueError("key lookup is implemented for 8- to 64-bit integers and Binary / LargeBinary, not physical type %d"
                                 % col.physical_type)
            vals = list_values(col.physical_type, lists[i])
            if len(vals) > MAX_VALUES:
                raise ValueError("a lookup list has at most %d values, not %d" % (MAX_VALUES, len(vals)))
            bitmap = None if sel is None else _bitmap_of(ctx, sel)
            m = col.metas_array()
            rows = int(m[:, 1].sum()) if m.shape[0] else 0
            ids, ws[i] = check_column(col.physical_type, rows, None if bitmap is None else bitmap.numel(), len(vals), vids[i], ws[i])
            if outs[i] is not None:
                _check_out(ctx, outs[i], rows, ws[i])
            if col.physical_type in INTEGER_TYPES:
                packed.append((np.ascontiguousarray(vals).tobytes(), None, len(vals)))
            else:
                raw, offsets = pack_list(col.physical_type, vals)
                packed.append((raw, offsets, len(vals)))
            bitmaps.append(bitmap)
            all_rows.append(rows)
            id_arrays.append(ids)
        rarr, keep = _prepare(ctx, columns)
        arr = (N.ColumnKeyLookupC * n)()
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
            w = ws[i]
            ids = outs[i]
            if ids is None:
                ids = torch.empty(all_rows[i], dtype=getattr(torch, ID_DTYPES[w]), device=ctx.torch_device)
            keep.append(ids)
            c.ids = _dev_ptr(ids)
            c.ids_capacity = ids.numel() * w
            c.id_width, c.reserved0, c.reserved = w, 0, 0
            raw, offsets, nv = packed[i]
            buf = C.create_string_buffer(raw, max(1, len(raw)))   # (read again by a replay: kept with the batch)
            keep.append(buf)
            c.values = C.addressof(buf)
            if offsets is not None:
                keep.append(offsets)
                c.value_offsets = offsets.ctypes.data
            if id_arrays[i] is not None:
                keep.append(id_arrays[i])
                c.value_ids = id_arrays[i].ctypes.data if nv else None
            c.n_values = nv
            c.stage_capacity = int(stage_capacity[i]) if stage_capacity is not None else 0
            res.append(KeyLookup(col.physical_type, w, c, ids[:all_rows[i]]))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.results = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_key_lookup(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.results


def key_lookup(ctx, columns: List[ColumnPages], values, value_ids=None, selection=None, id_width=None, out=None) -> List[KeyLookup]:
    """Enqueue the ids of columns[i] against values[i] under selection[i] (or one selection for all, or None: every
    row) on ctx's stream, behind the filter calls that write the bitmaps; `ids` are ordered on that stream, the
    scalars come with ctx.synchronize()."""
    return KeyLookupBatch(ctx, columns, values, value_ids, selection, id_width, out).enqueue()
