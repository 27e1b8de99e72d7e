"""read_selected_var:: — read only the selected rows of Binary / Utf8 columns, on the GPU.

The string half of `read_selected`: the pages of a Binary / LargeBinary payload column and a
selection bitmap go in, the selected rows come out packed as Arrow buffers
(sb_read_selected_var in include/strawboat_hip.h).  Output row k is the column's row at the k-th
set bit: `offsets[k + 1] - offsets[k]` is its byte length as a full read gives it (a null row's
included), `values[offsets[k]:offsets[k + 1]]` are its bytes, its validity is bit k of the
packed validity bitmap.
"""
import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N
from .filter import Selection
from .read import ColumnPages, _dev_ptr
from .read_selected import _bitmap_of, selection_bytes
from .types import PhysicalType

_P = PhysicalType
OFFSET_DTYPES = {_P.BINARY: np.int32, _P.LARGE_BINARY: np.int64}
_TORCH_NAMES = {_P.BINARY: "int32", _P.LARGE_BINARY: "int64"}


def check_column(physical_type, rows: int, bitmap_bytes: int):
    """The refusals that need no device: the type and the bitmap's length."""
    if physical_type not in OFFSET_DTYPES:
        raise ValueError("read_selected_var is implemented for Binary and LargeBinary, not physical type %d "
                         "(numbers: read_selected)" % physical_type)
    if bitmap_bytes < selection_bytes(rows):
        raise ValueError("the selection bitmap has %d bytes, %d rows need %d (4*ceil(rows/32))"
                         % (bitmap_bytes, rows, selection_bytes(rows)))


class SelectedBinaryArray:
    """The selected rows of one binary column in HBM; `selected` and `values_len` are valid
    after Context.synchronize() — also when it raised because a buffer was too small: they say
    what the buffers have to hold."""

    def __init__(self, physical_type, is_nullable, rows, offsets_buf, values_buf, validity_buf, cstruct):
        self.physical_type = physical_type
        self.is_nullable = is_nullable
        self.rows = rows
        self.offsets_buf = offsets_buf     # torch.uint8: the whole buffers, as given or allocated
        self.values_buf = values_buf
        self.validity_buf = validity_buf
        self._c = cstruct

    @property
    def selected(self):
        return int(self._c.selected)

    @property
    def values_len(self):
        return int(self._c.values_len)

    @property
    def offsets(self):
        """the selected + 1 offsets as an int32 / int64 tensor"""
        import torch
        w = _P.WIDTH[self.physical_type]
        return self.offsets_buf[:(self.selected + 1) * w].view(getattr(torch, _TORCH_NAMES[self.physical_type]))

    @property
    def values(self):
        """the bytes of the selected rows, back to back (uint8, values_len bytes)"""
        if self.values_buf is None:
            import torch
            return torch.empty(0, dtype=torch.uint8, device=self.offsets_buf.device)
        return self.values_buf[:self.values_len]

    @property
    def validity(self):
        """the packed validity bitmap of the selected rows (uint8, ceil(selected/8) bytes) or None"""
        if self.validity_buf is None:
            return None
        return self.validity_buf[:(self.selected + 7) // 8]

    def numpy(self):
        """(offsets, values, validity): int32 / int64 offsets, the bytes, a bool array (None: not nullable)"""
        offs = self.offsets.cpu().numpy()
        vals = self.values.cpu().numpy()
        if self.validity_buf is None:
            return offs, vals, None
        bits = np.unpackbits(self.validity.cpu().numpy(), bitorder="little")[:self.selected].astype(bool)
        return offs, vals, bits

    def to_pylist(self):
        """the selected rows as bytes objects, None for a null row"""
        offs, vals, bits = self.numpy()
        raw = vals.tobytes()
        return [raw[int(offs[k]):int(offs[k + 1])] if bits is None or bits[k] else None for k in range(self.selected)]


class ReadSelectedVarBatch:
    """A prepared selected read of binary columns: the C descriptors and the output buffers are
    built once; enqueue() then costs one C call (scripts/read_selected_var_probe.py).

    selections: one per column, or a single one for all columns (the usual case).  out[i]: a
    SelectedBinaryArray whose buffers are used again, or an (offsets, values, validity) triple of
    uint8 tensors.  Default: offsets and validity at the capacities that are always enough
    ((rows + 1) * sizeof(offset), 4*ceil(rows/32)); values at 4 * pages_len, the reference's own
    guess for a binary read — a column that needs more raises at the synchronize with
    `values_len` filled in.  stage_capacity: per column or one for all (None / 0: 4 * pages_len)."""

    def __init__(self, ctx, columns: List[ColumnPages], selections, out: Optional[Sequence] = None, stage_capacity=None):
        import torch
        from .read import _prepare
        n = len(columns)
        if isinstance(selections, (Selection, torch.Tensor)):
            selections = [selections] * n
        if len(selections) != n:
            raise ValueError("one selection per column (or one for all)")
        if out is not None and len(out) != n:
            raise ValueError("one output per column")
        if stage_capacity is None or isinstance(stage_capacity, int):
            stage_capacity = [stage_capacity or 0] * n
        if len(stage_capacity) != n:
            raise ValueError("one stage_capacity per column (or one for all)")
        bitmaps, rows_of = [], []
        for col, sel in zip(columns, selections):   # every refusal that needs no device, before anything is enqueued
            bitmap = _bitmap_of(ctx, sel)
            m = col.metas_array()
            rows = int(m[:, 1].sum()) if m.shape[0] else 0
            check_column(col.physical_type, rows, bitmap.numel())
            bitmaps.append(bitmap)
            rows_of.append(rows)
        rarr, keep = _prepare(ctx, columns)
        arr = (N.ColumnReadSelectedVarC * n)()
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
                    offsets, values, validity = ((o.offsets_buf, o.values_buf, o.validity_buf)
                                                 if isinstance(o, SelectedBinaryArray) else o)
                else:
                    offsets = torch.empty((rows + 1) * _P.WIDTH[col.physical_type], dtype=torch.uint8, device=dev)
                    values = torch.empty(4 * int(r.pages_len), dtype=torch.uint8, device=dev)
                    validity = torch.empty(selection_bytes(rows), dtype=torch.uint8, device=dev) if col.is_nullable else None
                keep.extend([bitmaps[i], offsets, values, validity])
                c.selection = _dev_ptr(bitmaps[i])
                c.selection_capacity = bitmaps[i].numel()
                c.values = _dev_ptr(values)
                c.values_capacity = values.numel() if values is not None else 0
                c.validity = _dev_ptr(validity)
                c.validity_capacity = validity.numel() if validity is not None else 0
                c.offsets = _dev_ptr(offsets)
                c.offsets_capacity = offsets.numel() if offsets is not None else 0
                c.stage_capacity = int(stage_capacity[i] or 0)
                res.append(SelectedBinaryArray(col.physical_type, col.is_nullable, rows, offsets, values, validity, c))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.arrays = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_read_selected_var(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.arrays


def read_selected_var(ctx, columns: List[ColumnPages], selections, out: Optional[Sequence] = None,
                      stage_capacity=None) -> List[SelectedBinaryArray]:
    """Enqueue the selected read of the binary columns[i] with selections[i] (or one selection for
    all) on ctx's stream, behind the filter calls that write the bitmaps; results after
    ctx.synchronize()."""
    return ReadSelectedVarBatch(ctx, columns, selections, out, stage_capacity).enqueue()
