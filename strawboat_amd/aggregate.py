"""aggregate:: — count / min / max / sum of the selected rows of columns, on the GPU.

The third thing a scan does with a block: `filter_columns` turns the WHERE columns into a selection
bitmap, `read_selected` materialises payload columns behind it, and `aggregate_columns` answers
SELECT count(y), min(y), max(y), sum(y) without materialising anything: the pages and the bitmap go
in, a few scalars per column come back (sb_aggregate_columns in include/strawboat_hip.h).  A row
counts if its selection bit is set and it is not null.
"""
import struct
from typing import List, Optional, Sequence

from . import _native as N
from .filter import Selection
from .read import ColumnPages, _dev_ptr
from .read_selected import NUMPY_DTYPES, _bitmap_of, selection_bytes
from .types import PhysicalType

_P = PhysicalType
OPS = {"count": N.SB_AGG_COUNT, "min": N.SB_AGG_MIN, "max": N.SB_AGG_MAX, "sum": N.SB_AGG_SUM}
VALUE_OPS = N.SB_AGG_MIN | N.SB_AGG_MAX | N.SB_AGG_SUM
_FORMATS = {_P.INT8: "<b", _P.INT16: "<h", _P.INT32: "<i", _P.INT64: "<q", _P.UINT8: "<B", _P.UINT16: "<H",
            _P.UINT32: "<I", _P.UINT64: "<Q", _P.FLOAT32: "<f", _P.FLOAT64: "<d"}
_FLOATS = (_P.FLOAT32, _P.FLOAT64)


def ops_mask(ops) -> int:
    """the SB_AGG_* bits of ("count", "min", ...) or of an int"""
    if isinstance(ops, int):
        mask = ops
    else:
        mask = 0
        for op in ops:
            if op not in OPS:
                raise ValueError("unknown aggregate %r (one of %s)" % (op, ", ".join(sorted(OPS))))
            mask |= OPS[op]
    if mask & ~(N.SB_AGG_COUNT | VALUE_OPS) or mask < 0:
        raise ValueError("unknown ops bits in %#x" % mask)
    return mask


def check_column(physical_type, rows: int, bitmap_bytes: Optional[int], ops: int):
    """The refusals that need no device: min / max / sum on a type that has none, the bitmap's length."""
    if (ops & VALUE_OPS) and physical_type not in NUMPY_DTYPES:
        raise ValueError("min / max / sum are implemented for 8- to 64-bit integers and floats, not physical type %d "
                         "(count works on every type)" % physical_type)
    if bitmap_bytes is not None and bitmap_bytes < selection_bytes(rows):
        raise ValueError("the selection bitmap has %d bytes, %d rows need %d (4*ceil(rows/32))"
                         % (bitmap_bytes, rows, selection_bytes(rows)))


class Aggregate:
    """The aggregates of one column; every property is valid after Context.synchronize()."""

    def __init__(self, physical_type, ops, cstruct):
        self.physical_type = physical_type
        self.ops = ops
        self._c = cstruct

    rows = property(lambda self: int(self._c.rows))
    selected = property(lambda self: int(self._c.selected))
    count = property(lambda self: int(self._c.count))
    nans = property(lambda self: int(self._c.nans))

    def _scalar(self, field, bit):
        if not (self.ops & bit) or self.count - self.nans == 0 or self.physical_type not in _FORMATS:
            return None
        fmt = _FORMATS[self.physical_type]
        return struct.unpack_from(fmt, bytes(field))[0]

    @property
    def min(self):
        """a Python scalar of the column's type; None when no row qualifies (or min was not asked for)"""
        return self._scalar(self._c.min, N.SB_AGG_MIN)

    @property
    def max(self):
        return self._scalar(self._c.max, N.SB_AGG_MAX)

    @property
    def min_bytes(self):
        return bytes(self._c.min)

    @property
    def max_bytes(self):
        return bytes(self._c.max)

    @property
    def sum(self):
        """integers: the exact sum as a Python int (128-bit two's complement on the device); floats: the double
        sum of the live rows; None when sum was not asked for"""
        if not (self.ops & N.SB_AGG_SUM):
            return None
        lo, hi = int(self._c.sum_lo), int(self._c.sum_hi)
        if self.physical_type in _FLOATS:
            return struct.unpack("<d", struct.pack("<Q", lo))[0]
        v = (hi << 64) | lo
        return v - (1 << 128) if hi >> 63 else v

    def __repr__(self):
        return "Aggregate(rows=%d, selected=%d, count=%d, nans=%d, min=%r, max=%r, sum=%r)" % (
            self.rows, self.selected, self.count, self.nans, self.min, self.max, self.sum)


class AggregateBatch:
    """A prepared aggregate call: the C descriptors are built once; enqueue() then costs one C call.

    selection: one per column, a single one for all columns, or None (every row); each a
    filter.Selection or a contiguous uint8 tensor on the context's device."""

    def __init__(self, ctx, columns: List[ColumnPages], selection=None, ops=("count", "min", "max", "sum")):
        import torch
        from .read import _prepare
        n = len(columns)
        mask = ops_mask(ops)
        if selection is None or isinstance(selection, (Selection, torch.Tensor)):
            selections = [selection] * n
        else:
            selections = list(selection)
        if len(selections) != n:
            raise ValueError("one selection per column (or one for all, or None)")
        bitmaps = []
        for col, sel in zip(columns, selections):   # every refusal that needs no device, before anything is enqueued
            bitmap = None if sel is None else _bitmap_of(ctx, sel)
            m = col.metas_array()
            rows = int(m[:, 1].sum()) if m.shape[0] else 0
            check_column(col.physical_type, rows, None if bitmap is None else bitmap.numel(), mask)
            bitmaps.append(bitmap)
        rarr, keep = _prepare(ctx, columns)
        arr = (N.ColumnAggregateC * n)()
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
            c.ops, c.reserved = mask, 0
            res.append(Aggregate(col.physical_type, mask, c))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.results = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_aggregate_columns(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.results


def aggregate_columns(ctx, columns: List[ColumnPages], selection=None,
                      ops: Sequence[str] = ("count", "min", "max", "sum")) -> List[Aggregate]:
    """Enqueue the aggregates of columns[i] under selection[i] (or one selection for all, or None: every
    row) on ctx's stream, behind the filter calls that write the bitmaps; results after ctx.synchronize()."""
    return AggregateBatch(ctx, columns, selection, ops).enqueue()
