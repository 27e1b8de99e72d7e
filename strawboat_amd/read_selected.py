"""read_selected:: — read only the selected rows of primitive columns, on the GPU.

The second half of a filter: `filter_columns` turns the pages of the WHERE columns into a selection
bitmap; `read_selected` takes the pages of the other columns and that bitmap and writes the rows
whose bit is set, packed (sb_read_selected in include/strawboat_hip.h).  Output row k is the
column's row at the k-th set bit: its value bytes are what a full read writes for that row (the
slot of a null row included), its validity is bit k of the packed validity bitmap.
"""
import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N
from .filter import Selection
from .read import ColumnPages, _dev_ptr
from .types import PhysicalType

_P = PhysicalType
NUMPY_DTYPES = {_P.INT8: np.int8, _P.INT16: np.int16, _P.INT32: np.int32, _P.INT64: np.int64,
                _P.UINT8: np.uint8, _P.UINT16: np.uint16, _P.UINT32: np.uint32, _P.UINT64: np.uint64,
                _P.FLOAT32: np.float32, _P.FLOAT64: np.float64}
_TORCH_NAMES = {_P.INT8: "int8", _P.INT16: "int16", _P.INT32: "int32", _P.INT64: "int64",
                _P.UINT8: "uint8", _P.UINT16: "uint16", _P.UINT32: "uint32", _P.UINT64: "uint64",
                _P.FLOAT32: "float32", _P.FLOAT64: "float64"}


def selection_bytes(rows: int) -> int:
    """bytes of a selection bitmap of `rows` rows: whole 32-bit words"""
    return ((rows + 31) // 32) * 4


def check_column(physical_type, rows: int, bitmap_bytes: int):
    """The refusals that need no device: the type and the bitmap's length."""
    if physical_type not in NUMPY_DTYPES:
        raise ValueError("read_selected is implemented for 8- to 64-bit integers and floats, not physical type %d"
                         % physical_type)
    if bitmap_bytes < selection_bytes(rows):
        raise ValueError("the selection bitmap has %d bytes, %d rows need %d (4*ceil(rows/32))"
                         % (bitmap_bytes, rows, selection_bytes(rows)))


class SelectedArray:
    """The selected rows of one column in HBM; `selected` is valid after Context.synchronize()."""

    def __init__(self, physical_type, is_nullable, rows, values_buf, validity_buf, cstruct):
        self.physical_type = physical_type
        self.is_nullable = is_nullable
        self.rows = rows
        self.values_buf = values_buf       # torch.uint8: the whole buffers, as given or allocated
        self.validity_buf = validity_buf
        self._c = cstruct

    @property
    def selected(self):
        return int(self._c.selected)

    @property
    def values_len(self):
        return int(self._c.values_len)

    @property
    def values(self):
        """the selected values as a typed tensor of `selected` entries"""
        import torch
        return self.values_buf[:self.values_len].view(getattr(torch, _TORCH_NAMES[self.physical_type]))

    @property
    def validity(self):
        """the packed validity bitmap of the selected rows (uint8, ceil(selected/8) bytes) or None"""
        if self.validity_buf is None:
            return None
        return self.validity_buf[:(self.selected + 7) // 8]

    def numpy(self):
        """(values, validity): a typed array of `selected` entries and a bool array (None: not nullable)"""
        vals = self.values_buf[:self.values_len].cpu().numpy().view(NUMPY_DTYPES[self.physical_type])
        if self.validity_buf is None:
            return vals, None
        bits = np.unpackbits(self.validity.cpu().numpy(), bitorder="little")[:self.selected].astype(bool)
        return vals, bits


def _bitmap_of(ctx, sel):
    import torch
    bitmap = sel.bitmap if isinstance(sel, Selection) else sel
    if not isinstance(bitmap, torch.Tensor) or bitmap.dtype != torch.uint8 or not bitmap.is_contiguous():
        raise TypeError("a selection is a filter.Selection or a contiguous torch.uint8 tensor")
    if bitmap.device != ctx.torch_device:
        raise ValueError("the selection bitmap is on %s, the context on %s" % (bitmap.device, ctx.torch_device))
    return bitmap


class ReadSelectedBatch:
    """A prepared selected read: the C descriptors and the output buffers are built once;
    enqueue() then costs one C call (steady-state callers, scripts/read_selected_probe.py).

    selections: one per column, or a single one for all columns (the usual case).  out[i]: a
    SelectedArray whose buffers are used again, or a (values, validity) pair of uint8 tensors;
    default: the capacities that are always enough (rows * width, 4*ceil(rows/32))."""

    def __init__(self, ctx, columns: List[ColumnPages], selections, out: Optional[Sequence] = None):
        import torch
        from .read import _prepare
        n = len(columns)
        if isinstance(selections, (Selection, torch.Tensor)):
            selections = [selections] * n
        if len(selections) != n:
            raise ValueError("one selection per column (or one for all)")
        if out is not None and len(out) != n:
            raise ValueError("one output per column")
        bitmaps, rows_of = [], []
        for col, sel in zip(columns, selections):   # every refusal that needs no device, before anything is enqueued
            bitmap = _bitmap_of(ctx, sel)
            m = col.metas_array()
            rows = int(m[:, 1].sum()) if m.shape[0] else 0
            check_column(col.physical_type, rows, bitmap.numel())
            bitmaps.append(bitmap)
            rows_of.append(rows)
        rarr, keep = _prepare(ctx, columns)
        arr = (N.ColumnReadSelectedC * n)()
        res = []
        dev = ctx.torch_device
        with torch.cuda.stream(ctx.torch_stream):
            for i, col in enumerate(columns):
                c, r = arr[i], rarr[i]
                c.physical_type, c.is_nullable = r.physical_type, r.is_nullable
                c.pages, c.pages_len, c.metas, c.n_pages = r.pages, r.pages_len, r.metas, r.n_pages
                c.page_offsets = r.page_offsets
                rows = rows_of[i]
                if out is not None:
                    o = out[i]
                    values, validity = (o.values_buf, o.validity_buf) if isinstance(o, SelectedArray) else o
                else:
                    values = torch.empty(rows * _P.WIDTH[col.physical_type], dtype=torch.uint8, device=dev)
                    validity = torch.empty(selection_bytes(rows), dtype=torch.uint8, device=dev) if col.is_nullable else None
                keep.extend([bitmaps[i], values, validity])
                c.selection = _dev_ptr(bitmaps[i])
                c.selection_capacity = bitmaps[i].numel()
                c.values = _dev_ptr(values)
                c.values_capacity = values.numel() if values is not None else 0
                c.validity = _dev_ptr(validity)
                c.validity_capacity = validity.numel() if validity is not None else 0
                res.append(SelectedArray(col.physical_type, col.is_nullable, rows, values, validity, c))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.arrays = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_read_selected(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.arrays


def read_selected(ctx, columns: List[ColumnPages], selections, out: Optional[Sequence] = None) -> List[SelectedArray]:
    """Enqueue the selected read of columns[i] with selections[i] (or one selection for all) on
    ctx's stream, behind the filter calls that write the bitmaps; results after ctx.synchronize()."""
    return ReadSelectedBatch(ctx, columns, selections, out).enqueue()
