"""key_buckets:: — the range bucket of every row of a numeric key column, on the GPU.

`key_ids`, `key_ids_var`, `key_combine` and `key_lookup` give a row a group id by equality.  Here the id says where
the row's value falls among up to 1023 strictly increasing bounds (sb_key_buckets in include/strawboat_hip.h):

  * `GROUP BY date_trunc('month', d)` over a Date32 or timestamp column, the month starts being the bounds;
  * price, age or latency bands (`CASE WHEN x < 10 ... WHEN x < 100 ...`, `width_bucket`);
  * histograms and approximate quantiles;
  * any `GROUP BY` over a Float32 / Float64 column.

Bucket 0 is below the first bound, bucket i is [bounds[i - 1], bounds[i]) -- or (bounds[i - 1], bounds[i]] with
`right_closed` -- and bucket n_bounds is open-ended.  `bucket_ids` renames, merges or drops buckets (None / NONE: no
id).  A live NaN gets `nan_id` (None: no id) and is counted in `nans`.  The ids are what `aggregate_grouped` /
`aggregate_grouped_large` / `aggregate_weighted` take as `group_ids`, unchanged; rows without an id arrive in their
`out_of_range`.
"""
import ctypes as C
from typing import List, Optional

import numpy as np

from . import _native as N
from .filter import Selection
from .key_ids import ID_DTYPES, INTEGER_TYPES, _check_out
from .key_lookup import id_none, narrowest_id_width
from .read import ColumnPages, _dev_ptr
from .read_selected import NUMPY_DTYPES, _bitmap_of, selection_bytes
from .types import PhysicalType as _P

MAX_BOUNDS = N.SB_BUCKET_MAX_BOUNDS
NONE = N.SB_KEY_ID_NONE
FLOAT_TYPES = (_P.FLOAT32, _P.FLOAT64)
_REFUSED = "key buckets are implemented for 8- to 64-bit integers, Float32 and Float64, not physical type %d"


def bounds_values(physical_type, bounds):
    """The bounds of one column as a 1-d numpy array of the column's dtype: at most 1023 values, strictly increasing
    under the column's comparison (-0.0 == +0.0), none of them a NaN; +-inf are bounds like any other."""
    if physical_type not in INTEGER_TYPES and physical_type not in FLOAT_TYPES:
        raise ValueError(_REFUSED % physical_type)
    dt = np.dtype(NUMPY_DTYPES[physical_type])
    if isinstance(bounds, np.ndarray):
        if bounds.dtype != dt or bounds.ndim != 1:
            raise ValueError("bounds is a 1-d %s array for this column, not %s%r" % (dt, bounds.dtype, bounds.shape))
        arr = np.ascontiguousarray(bounds)
    else:
        vals = list(bounds)
        for v in vals:
            if isinstance(v, (str, bytes, bytearray, memoryview, bool)):
                raise ValueError("bound %r is not a number" % (v,))
            if dt.kind == "f":
                if not isinstance(v, (int, float, np.integer, np.floating)):
                    raise ValueError("bound %r is not a number" % (v,))
            else:
                if not isinstance(v, (int, np.integer)):
                    raise ValueError("bound %r is not an integer" % (v,))
                if not np.iinfo(dt).min <= int(v) <= np.iinfo(dt).max:
                    raise ValueError("bound %r does not fit %s" % (v, dt))
        arr = np.array(vals, dtype=dt)
    if arr.size > MAX_BOUNDS:
        raise ValueError("a call takes at most %d bounds, not %d" % (MAX_BOUNDS, arr.size))
    if dt.kind == "f" and np.isnan(arr).any():
        raise ValueError("a bound is NaN")
    if arr.size > 1 and not (arr[1:] > arr[:-1]).all():
        raise ValueError("bounds are not strictly increasing")
    return arr


def check_column(physical_type, rows: int, bitmap_bytes: Optional[int], n_bounds: int, bucket_ids, nan_id, id_width):
    """The refusals that need no device: the type, the number of bounds, the ids, nan_id, the width, the bitmap's
    length.  Returns (bucket_ids as a uint32 array or None, nan_id as the C field, id_width)."""
    if physical_type not in INTEGER_TYPES and physical_type not in FLOAT_TYPES:
        raise ValueError(_REFUSED % physical_type)
    if n_bounds > MAX_BOUNDS:
        raise ValueError("a call takes at most %d bounds, not %d" % (MAX_BOUNDS, n_bounds))
    ids = None
    handed = [n_bounds]
    if bucket_ids is not None:
        raw = list(bucket_ids.tolist() if isinstance(bucket_ids, np.ndarray) else bucket_ids)
        if len(raw) != n_bounds + 1:
            raise ValueError("%d bucket_ids for %d bounds: a call has n_bounds + 1 buckets" % (len(raw), n_bounds))
        raw = [NONE if v is None else v for v in raw]
        for v in raw:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= NONE:
                raise ValueError("bucket id %r is not None or an int in 0 .. 2^32 - 2" % (v,))
        ids = np.array(raw, dtype=np.uint32)
        handed = [int(v) for v in raw if int(v) != NONE]
    if nan_id is None or (not isinstance(nan_id, bool) and isinstance(nan_id, (int, np.integer)) and int(nan_id) == NONE):
        nan_c = NONE
    else:
        if isinstance(nan_id, bool) or not isinstance(nan_id, (int, np.integer)) or not 0 <= int(nan_id) < NONE:
            raise ValueError("nan_id is %r, not None or an int in 0 .. 2^32 - 2" % (nan_id,))
        if physical_type not in FLOAT_TYPES:
            raise ValueError("nan_id on an integer column")
        nan_c = int(nan_id)
        handed.append(nan_c)
    largest = max(handed) if handed else 0
    if id_width is None:
        id_width = narrowest_id_width(largest)
    if isinstance(id_width, bool) or not isinstance(id_width, (int, np.integer)) or id_width not in (1, 2, 4):
        raise ValueError("id_width is %r, not 1, 2 or 4" % (id_width,))
    if largest >= id_none(id_width):
        raise ValueError("the id %d is all ones of id_width %d or does not fit it" % (largest, id_width))
    if bitmap_bytes is not None and bitmap_bytes < selection_bytes(rows):
        raise ValueError("the selection bitmap has %d bytes, %d rows need %d (4*ceil(rows/32))"
                         % (bitmap_bytes, rows, selection_bytes(rows)))
    return ids, nan_c, int(id_width)


class KeyBuckets:
    """The bucket ids of one column; the scalars are valid after Context.synchronize()."""

    def __init__(self, physical_type, id_width, n_bounds, cstruct, ids):
        self.physical_type = physical_type
        self.id_width = id_width
        self.n_bounds = n_bounds
        self._c = cstruct
        #: torch tensor on the context's device, one id per row: uint8 (id_width 1), uint16 (2) or int32 (4, the
        #: unsigned bits).  Written by the call's kernels: ordered behind them on the context's stream.
        self.ids = ids

    rows = property(lambda self: int(self._c.rows))
    selected = property(lambda self: int(self._c.selected))
    count = property(lambda self: int(self._c.count))
    matched = property(lambda self: int(self._c.matched))
    nans = property(lambda self: int(self._c.nans))

    @property
    def none(self):
        """the id of a row without one: all ones in id_width bytes, as the ids' dtype shows it"""
        return -1 if self.id_width == 4 else id_none(self.id_width)

    def __repr__(self):
        return "KeyBuckets(rows=%d, selected=%d, count=%d, matched=%d, nans=%d, id_width=%d)" % (
            self.rows, self.selected, self.count, self.matched, self.nans, self.id_width)


def _per_column(value, n, what):
    """one value for all columns, or one per column"""
    if isinstance(value, (list, tuple)):
        if len(value) != n:
            raise ValueError("one %s per column (or one for all)" % what)
        return list(value)
    return [value] * n


class KeyBucketsBatch:
    """A prepared key-buckets call: the C descriptors, the bounds and the ids tensors are built once; enqueue() then
    costs one C call.

    bounds: one list per column (bounds_values says what a list may be).  bucket_ids: None (a bucket's id is its
    number), or per column None or n_bounds + 1 ids, None / NONE among them for a bucket without an id; several
    buckets may share an id.  right_closed, nan_id, id_width: one value for all columns or one per column; id_width
    None picks the narrowest width that holds the column's largest id.  selection: one per column, a single one for
    all columns, or None (every row).  out: None, or one ids tensor per column to write into (None entries are
    allocated).  Columns of different types may share a call."""

    def __init__(self, ctx, columns: List[ColumnPages], bounds, bucket_ids=None, selection=None, right_closed=False,
                 nan_id=None, id_width=None, out=None):
        import torch
        from .read import _prepare
        n = len(columns)
        lists = list(bounds)
        bids = [None] * n if bucket_ids is None else list(bucket_ids)
        ws = _per_column(id_width, n, "id_width")
        nans = _per_column(nan_id, n, "nan_id")
        closed = _per_column(right_closed, n, "right_closed")
        outs = [None] * n if out is None else list(out)
        if selection is None or isinstance(selection, (Selection, torch.Tensor)):
            selections = [selection] * n
        else:
            selections = list(selection)
        if len(lists) != n:
            raise ValueError("one list of bounds per column")
        if len(bids) != n:
            raise ValueError("one bucket_ids per column (or None)")
        if len(selections) != n:
            raise ValueError("one selection per column (or one for all, or None)")
        if len(outs) != n:
            raise ValueError("one out tensor per column (or None)")
        bitmaps, all_rows, arrays, id_arrays = [], [], [], []
        for i, (col, sel) in enumerate(zip(columns, selections)):   # every refusal that needs no device, before anything is enqueued
            if not isinstance(col, ColumnPages):
                raise ValueError("a column is a ColumnPages, not %r" % type(col).__name__)
            arr = bounds_values(col.physical_type, lists[i])
            if not isinstance(closed[i], (bool, np.bool_)):
                raise ValueError("right_closed is %r, not a bool" % (closed[i],))
            bitmap = None if sel is None else _bitmap_of(ctx, sel)
            m = col.metas_array()
            rows = int(m[:, 1].sum()) if m.shape[0] else 0
            ids, nans[i], ws[i] = check_column(col.physical_type, rows, None if bitmap is None else bitmap.numel(), arr.size,
                                               bids[i], nans[i], ws[i])
            if outs[i] is not None:
                _check_out(ctx, outs[i], rows, ws[i])
            bitmaps.append(bitmap)
            all_rows.append(rows)
            arrays.append(arr)
            id_arrays.append(ids)
        rarr, keep = _prepare(ctx, columns)
        carr = (N.ColumnKeyBucketsC * n)()
        res = []
        for i, col in enumerate(columns):
            c, r = carr[i], rarr[i]
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
            c.flags = N.SB_BUCKET_RIGHT_CLOSED if closed[i] else 0
            raw = arrays[i].tobytes()
            buf = C.create_string_buffer(raw, max(1, len(raw)))   # (read again by a replay: kept with the batch)
            keep.append(buf)
            c.bounds = C.addressof(buf)
            if id_arrays[i] is not None:
                keep.append(id_arrays[i])
                c.bucket_ids = id_arrays[i].ctypes.data
            c.n_bounds = arrays[i].size
            c.nan_id = nans[i]
            res.append(KeyBuckets(col.physical_type, w, int(arrays[i].size), c, ids[:all_rows[i]]))
        self.ctx, self._arr, self._keep, self._n = ctx, carr, keep, n
        self.results = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_key_buckets(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.results


def key_buckets(ctx, cols: List[ColumnPages], bounds, bucket_ids=None, selection=None, right_closed=False, nan_id=None,
                id_width=None, out=None) -> List[KeyBuckets]:
    """Enqueue the bucket ids of cols[i] among bounds[i] under selection[i] (or one selection for all, or None: every
    row) on ctx's stream, behind the filter calls that write the bitmaps; `ids` are ordered on that stream, the
    scalars come with ctx.synchronize()."""
    return KeyBucketsBatch(ctx, cols, bounds, bucket_ids, selection, right_closed, nan_id, id_width, out).enqueue()
