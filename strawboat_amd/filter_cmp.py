"""filter_cmp:: — `WHERE a < b`: the pages of a column compared row by row with a second column, on the GPU.

Every other filter call compares a column with constants.  This one takes the pages of a primitive column y and a
dense per-row operand on the device -- a column `read_columns` decoded earlier in the interval, or anything the
engine computed -- and gives the `Selection` of filter:: (sb_filter_columns_cmp in include/strawboat_hip.h), so it
chains with filter_columns, filter_in, read_selected and the aggregates.  y is never written: `rows / 8` bytes
come out.  Two integers compare exactly whatever their widths and signedness; a pair with a float compares as
doubles (IEEE 754: NaN satisfies only "ne", -0.0 == 0.0).  A row whose y is null or whose operand is invalid
satisfies nothing, "ne" included.
"""
from typing import List, Optional, Sequence

from . import _native as N
from .filter import COMBINE, Selection
from .read import ColumnPages, DeviceArray, _dev_ptr
from .read_selected import NUMPY_DTYPES, selection_bytes
from .types import PhysicalType as _P

OPS = {"eq": N.SB_PRED_EQ, "ne": N.SB_PRED_NE, "lt": N.SB_PRED_LT, "le": N.SB_PRED_LE, "gt": N.SB_PRED_GT, "ge": N.SB_PRED_GE}

#: the other_type of an operand tensor, by its dtype
OTHER_TYPES = {"torch.int8": _P.INT8, "torch.int16": _P.INT16, "torch.int32": _P.INT32, "torch.int64": _P.INT64,
               "torch.uint8": _P.UINT8, "torch.uint16": _P.UINT16, "torch.uint32": _P.UINT32, "torch.uint64": _P.UINT64,
               "torch.float32": _P.FLOAT32, "torch.float64": _P.FLOAT64}


def check_column(physical_type, rows: int, op, other_type, other_bytes: int, validity_bytes: Optional[int]):
    """The refusals that need no device.  other_type None: a dtype that is no operand type."""
    if op not in OPS:
        raise ValueError("unknown comparison %r: one of %s" % (op, ", ".join(OPS)))
    if physical_type not in NUMPY_DTYPES:
        raise ValueError("column comparisons are implemented for 8- to 64-bit integers and floats, not physical type %r"
                         % (physical_type,))
    if other_type not in NUMPY_DTYPES:
        raise ValueError("operands are 8- to 64-bit integers, float32 or float64, not %r" % (other_type,))
    need = rows * _P.WIDTH[other_type]
    if other_bytes < need:
        raise ValueError("the operand has %d bytes, %d rows of physical type %d need %d" % (other_bytes, rows, other_type, need))
    if validity_bytes is not None and validity_bytes < selection_bytes(rows):
        raise ValueError("the operand's validity has %d bytes, %d rows need %d (4*ceil(rows/32))"
                         % (validity_bytes, rows, selection_bytes(rows)))


def _other_of(ctx, other, other_type, validity):
    """(tensor, validity or None, other_type or None) of an operand: a typed tensor, a (tensor, validity) pair, or a
    DeviceArray of a numeric column as read_columns gave it.  A stated other_type says what the tensor's bytes are."""
    import torch
    if isinstance(other, DeviceArray):
        if validity is not None:
            raise ValueError("a DeviceArray brings its own validity")
        if other_type is not None and other_type != other.physical_type:
            raise ValueError("other_type %r, the DeviceArray is of physical type %d" % (other_type, other.physical_type))
        other_type, validity, other = other.physical_type, other.validity, other.values
    elif isinstance(other, (tuple, list)):
        if len(other) != 2 or validity is not None:
            raise ValueError("an operand is a tensor, a (tensor, validity) pair or a DeviceArray")
        other, validity = other
    if not isinstance(other, torch.Tensor):
        raise ValueError("operands are torch tensors on the context's device")
    if other.device != ctx.torch_device:
        raise ValueError("the operand is on %s, the context on %s" % (other.device, ctx.torch_device))
    if other.dim() != 1 or not other.is_contiguous():
        raise ValueError("operands are contiguous 1-d tensors")
    if validity is not None:
        if not isinstance(validity, torch.Tensor) or validity.dtype != torch.uint8 or not validity.is_contiguous():
            raise ValueError("the operand's validity is a contiguous torch.uint8 tensor (an LSB-first bitmap)")
        if validity.device != ctx.torch_device:
            raise ValueError("the operand's validity is on %s, the context on %s" % (validity.device, ctx.torch_device))
    if other_type is None:
        other_type = OTHER_TYPES.get(str(other.dtype))
    return other, validity, other_type


def _per_column(n: int, what, name: str):
    if what is None:
        return [None] * n
    what = list(what)
    if len(what) != n:
        raise ValueError("one %s per column" % name)
    return what


class FilterCmpBatch:
    """A prepared sb_filter_columns_cmp call: the C descriptors are built once and keep the operand tensors alive
    until the synchronize; enqueue() then costs one C call.  What needs no device is refused here, before a context
    is touched.

    ops: one of "eq" "ne" "lt" "le" "gt" "ge" per column, or one for all; others: one operand per column (a typed
    tensor, a (tensor, validity) pair or a DeviceArray); other_types / other_validities: optional, per column."""

    def __init__(self, ctx, columns: List[ColumnPages], ops, others, other_types=None, other_validities=None,
                 combine="set", out: Optional[List[Selection]] = None):
        import torch
        from .read import _prepare
        n = len(columns)
        ops = [ops] * n if isinstance(ops, str) else list(ops)
        if len(ops) != n:
            raise ValueError("one op per column (or one for all)")
        if others is None or isinstance(others, (torch.Tensor, DeviceArray)):
            raise ValueError("one operand per column: a list of tensors, (tensor, validity) pairs or DeviceArrays")
        others = _per_column(n, others, "operand")
        types = _per_column(n, other_types, "other_type")
        valids = _per_column(n, other_validities, "operand validity")
        if combine not in COMBINE:
            raise ValueError("unknown combine mode %r" % (combine,))
        if combine != "set" and out is None:
            raise ValueError("combine=%r needs the selections to combine with (selection=)" % combine)
        if out is not None and len(out) != n:
            raise ValueError("one selection per column")
        prepared = []
        for i, col in enumerate(columns):   # before anything is enqueued
            m = col.metas_array()
            rows = int(m[:, 1].sum()) if m.shape[0] else 0
            t, v, tt = _other_of(ctx, others[i], types[i], valids[i])
            check_column(col.physical_type, rows, ops[i], tt, t.numel() * t.element_size(), None if v is None else v.numel())
            if out is not None and out[i].rows != rows:
                raise ValueError("selection %d has %d rows, the column %d" % (i, out[i].rows, rows))
            prepared.append((rows, t, v, tt))
        rarr, keep = _prepare(ctx, columns)
        arr = (N.ColumnFilterCmpC * n)()
        res = []
        with torch.cuda.stream(ctx.torch_stream):
            for i in range(n):
                c, r = arr[i], rarr[i]
                rows, t, v, tt = prepared[i]
                c.physical_type, c.is_nullable = r.physical_type, r.is_nullable
                c.pages, c.pages_len, c.metas, c.n_pages = r.pages, r.pages_len, r.metas, r.n_pages
                c.page_offsets = r.page_offsets
                c.op, c.combine = OPS[ops[i]], COMBINE[combine]
                keep.extend([t, v])
                c.other = _dev_ptr(t)
                c.other_capacity = t.numel() * t.element_size()
                c.other_validity = _dev_ptr(v)
                c.other_validity_capacity = v.numel() if v is not None and v.numel() else 0
                c.other_type, c.flags, c.reserved = tt, 0, 0
                if out is not None:
                    bitmap = out[i].bitmap
                else:
                    bitmap = torch.empty(selection_bytes(rows), dtype=torch.uint8, device=ctx.torch_device)
                keep.append(bitmap)
                c.selection = _dev_ptr(bitmap)
                c.selection_capacity = bitmap.numel()
                res.append(Selection(bitmap, rows, c))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.selections = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_filter_columns_cmp(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.selections


def filter_columns_cmp(ctx, columns: List[ColumnPages], ops, others, other_types: Optional[Sequence[int]] = None,
                       other_validities=None, combine="set", selection: Optional[List[Selection]] = None) -> List[Selection]:
    """Enqueue `columns[i] ops[i] others[i]` on ctx's stream, behind the calls that write the operands; the
    Selections of filter_columns come back (`selected` after ctx.synchronize()).  others[i]: a typed device tensor
    (its dtype gives other_type when none is stated), a (tensor, validity) pair or a DeviceArray.  combine: "set"
    writes the result, "and" / "or" combine it with what selection[i].bitmap holds; `selection` re-uses earlier
    selections' buffers and is required for "and" / "or"."""
    return FilterCmpBatch(ctx, columns, ops, others, other_types, other_validities, combine, selection).enqueue()


def filter_pair(ctx, left: ColumnPages, op, right: ColumnPages, combine="set", selection: Optional[Selection] = None) -> Selection:
    """`left op right` between two columns of one block, in one interval: sb_read_columns of `right` into device
    buffers (values and validity) is enqueued, then the comparison of left's pages against them.  Only `right` is
    decoded into memory.  Both columns have the same number of rows."""
    from .read import batch_read_columns
    lm, rm = left.metas_array(), right.metas_array()
    lrows = int(lm[:, 1].sum()) if lm.shape[0] else 0
    rrows = int(rm[:, 1].sum()) if rm.shape[0] else 0
    if lrows != rrows:
        raise ValueError("left has %d rows, right %d" % (lrows, rrows))
    check_column(left.physical_type, lrows, op, right.physical_type,
                 rrows * _P.WIDTH.get(right.physical_type, 0) if right.physical_type in NUMPY_DTYPES else 0, None)
    if combine not in COMBINE:
        raise ValueError("unknown combine mode %r" % (combine,))
    if combine != "set" and selection is None:
        raise ValueError("combine=%r needs the selection to combine with (selection=)" % combine)
    operand = batch_read_columns(ctx, [right])[0]
    return filter_columns_cmp(ctx, [left], [op], [operand], combine=combine,
                              selection=None if selection is None else [selection])[0]
