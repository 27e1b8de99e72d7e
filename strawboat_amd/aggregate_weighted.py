"""aggregate_weighted:: — count and sum(y * w) of the selected rows of columns, per group, on the GPU.

The aggregates analytic queries ask for are aggregates of an expression: sum(price * discount), weighted means,
var(y) through sum(y * y).  `aggregate_grouped_large` with a second dense per-row input beside the ids: a weight
per row, on the device -- a column `read_columns` decoded earlier in the interval, or anything the engine computed
from other columns.  The pages of y, the selection bitmap, the ids and the weights go in; a record per group
comes back (sb_aggregate_weighted in include/strawboat_hip.h): `sum` is the sum of the products, exact modulo
2^128 when y and w are both integers, a double otherwise.  `square=True`: the weight of a row is its own y.
Without `group_ids` every selected row is in group 0 (n_groups 1).
"""
from typing import List, Optional, Sequence

from . import _native as N
from .aggregate import check_column as _check_ungrouped, ops_mask
from .aggregate_grouped import GroupedAggregate, _ids_of
from .aggregate_grouped_large import MAX_GROUPS_LARGE
from .filter import Selection
from .read import ColumnPages, DeviceArray, _dev_ptr
from .read_selected import NUMPY_DTYPES, _bitmap_of, selection_bytes
from .types import PhysicalType as _P

#: the weight_type of a weights tensor, by its dtype
WEIGHT_TYPES = {"torch.int8": _P.INT8, "torch.int16": _P.INT16, "torch.int32": _P.INT32, "torch.int64": _P.INT64,
                "torch.uint8": _P.UINT8, "torch.uint16": _P.UINT16, "torch.uint32": _P.UINT32, "torch.uint64": _P.UINT64,
                "torch.float32": _P.FLOAT32, "torch.float64": _P.FLOAT64}
_FLOATS = (_P.FLOAT32, _P.FLOAT64)


def check_column(physical_type, rows: int, bitmap_bytes: Optional[int], ops: int, n_groups, id_width, id_count: Optional[int],
                 weight_type, weight_count: int, validity_bytes: Optional[int], square: bool):
    """The refusals that need no device.  id_count None: the ungrouped form (no group_ids); weight_type None: a
    dtype that is no weight type."""
    if ops & (N.SB_AGG_MIN | N.SB_AGG_MAX):
        raise ValueError("aggregate_weighted offers count and sum, not min / max of a product")
    _check_ungrouped(physical_type, rows, bitmap_bytes, ops)
    if isinstance(n_groups, bool) or not isinstance(n_groups, int) or not 1 <= n_groups <= MAX_GROUPS_LARGE:
        raise ValueError("n_groups is %r, not an int in 1 .. %d" % (n_groups, MAX_GROUPS_LARGE))
    if id_count is None:
        if n_groups != 1:
            raise ValueError("without group_ids every row is in group 0: n_groups is 1, not %d" % n_groups)
    else:
        if id_width not in (1, 2, 4):
            raise ValueError("group ids are uint8, uint16, uint32 or int32")
        if id_count < rows:
            raise ValueError("%d group ids for a column of %d rows" % (id_count, rows))
    if square:
        return
    if weight_type not in NUMPY_DTYPES:
        raise ValueError("weights are 8- to 64-bit integers, float32 or float64")
    if weight_count < rows:
        raise ValueError("%d weights for a column of %d rows" % (weight_count, rows))
    if validity_bytes is not None and validity_bytes < selection_bytes(rows):
        raise ValueError("the weights' validity has %d bytes, %d rows need %d (4*ceil(rows/32))"
                         % (validity_bytes, rows, selection_bytes(rows)))


def _weights_of(ctx, w):
    """(tensor, validity or None, weight_type or None) of a weights argument: a typed tensor, a (tensor, validity)
    pair, or a DeviceArray of a numeric column as read_columns gave it"""
    import torch
    validity = None
    if isinstance(w, DeviceArray):
        if w.physical_type not in NUMPY_DTYPES:
            raise ValueError("weights are 8- to 64-bit integers, float32 or float64, not physical type %d" % w.physical_type)
        dtype = getattr(torch, NUMPY_DTYPES[w.physical_type].__name__)
        w, validity = w.values[:w.rows * _P.WIDTH[w.physical_type]].view(dtype), w.validity
    elif isinstance(w, (tuple, list)):
        if len(w) != 2:
            raise ValueError("weights are a tensor or a (tensor, validity) pair")
        w, validity = w
    if not isinstance(w, torch.Tensor):
        raise ValueError("weights are a torch tensor on the context's device")
    if w.device != ctx.torch_device:
        raise ValueError("weights are on %s, the context on %s" % (w.device, ctx.torch_device))
    if w.dim() != 1 or not w.is_contiguous():
        raise ValueError("weights are a contiguous 1-d tensor")
    if validity is not None:
        if not isinstance(validity, torch.Tensor) or validity.dtype != torch.uint8 or not validity.is_contiguous():
            raise ValueError("the weights' validity is a contiguous torch.uint8 tensor (an LSB-first bitmap)")
        if validity.device != ctx.torch_device:
            raise ValueError("the weights' validity is on %s, the context on %s" % (validity.device, ctx.torch_device))
    return w, validity, WEIGHT_TYPES.get(str(w.dtype))


def _weights_list(n: int, weights, square: bool):
    """one weights entry per column (None each with square)"""
    import torch
    if square:
        if weights is not None and any(w is not None for w in (weights if isinstance(weights, (list, tuple)) else [weights])):
            raise ValueError("square=True takes the column's own values as weights: weights is None")
        return [None] * n
    if weights is None or isinstance(weights, (torch.Tensor, DeviceArray)):
        raise ValueError("one weights entry per column: a list of tensors, (tensor, validity) pairs or DeviceArrays")
    weights = list(weights)
    if len(weights) != n:
        raise ValueError("one weights entry per column")
    return weights


def check_weights(ctx, columns: List[ColumnPages], weights, square: bool):
    """What WeightedAggregateBatch refuses of the value columns and their weights alone (group_by_weighted: before a
    key call is made)."""
    for col, w in zip(columns, _weights_list(len(columns), weights, bool(square))):
        m = col.metas_array()
        rows = int(m[:, 1].sum()) if m.shape[0] else 0
        wt = wv = wtype = None
        if not square:
            wt, wv, wtype = _weights_of(ctx, w)
        check_column(col.physical_type, rows, None, N.SB_AGG_COUNT | N.SB_AGG_SUM, 1, None, None, wtype,
                     0 if wt is None else wt.numel(), None if wv is None else wv.numel(), bool(square))


class WeightedAggregateBatch:
    """A prepared sb_aggregate_weighted call: the C descriptors and the groups' records are built once; enqueue()
    then costs one C call.

    weights: one per column (a tensor, a (tensor, validity) pair or a DeviceArray), or None with square=True;
    group_ids: one tensor per column, one for all, or None (the ungrouped form, n_groups 1); n_groups an int per
    column or one for all; selection as in AggregateBatch."""

    def __init__(self, ctx, columns: List[ColumnPages], weights, group_ids=None, n_groups=1, selection=None,
                 ops=("count", "sum"), square=False):
        import torch
        from .read import _prepare
        n = len(columns)
        mask = ops_mask(ops)
        square = bool(square)
        if selection is None or isinstance(selection, (Selection, torch.Tensor)):
            selections = [selection] * n
        else:
            selections = list(selection)
        ids_list = [group_ids] * n if group_ids is None or isinstance(group_ids, torch.Tensor) else list(group_ids)
        groups_list = list(n_groups) if isinstance(n_groups, (list, tuple)) else [n_groups] * n
        weights_list = _weights_list(n, weights, square)
        if len(selections) != n:
            raise ValueError("one selection per column (or one for all, or None)")
        if len(ids_list) != n or len(groups_list) != n:
            raise ValueError("one group_ids tensor and one n_groups per column (or one for all)")
        prepared = []
        for col, sel, ids, ng, w in zip(columns, selections, ids_list, groups_list, weights_list):   # before anything is enqueued
            bitmap = None if sel is None else _bitmap_of(ctx, sel)
            width = None
            if ids is not None:
                ids, width = _ids_of(ctx, ids)
            wt = wv = wtype = None
            if not square:
                wt, wv, wtype = _weights_of(ctx, w)
            m = col.metas_array()
            rows = int(m[:, 1].sum()) if m.shape[0] else 0
            check_column(col.physical_type, rows, None if bitmap is None else bitmap.numel(), mask, ng, width,
                         None if ids is None else ids.numel(), wtype, 0 if wt is None else wt.numel(),
                         None if wv is None else wv.numel(), square)
            prepared.append((bitmap, ids, width, wt, wv, wtype))
        rarr, keep = _prepare(ctx, columns)
        arr = (N.ColumnAggregateWeightedC * n)()
        res = []
        for i, col in enumerate(columns):
            c, r = arr[i], rarr[i]
            bitmap, ids, width, wt, wv, wtype = prepared[i]
            c.physical_type, c.is_nullable = r.physical_type, r.is_nullable
            c.pages, c.pages_len, c.metas, c.n_pages = r.pages, r.pages_len, r.metas, r.n_pages
            c.page_offsets = r.page_offsets
            keep.extend([bitmap, ids, wt, wv])
            c.selection = _dev_ptr(bitmap)
            c.selection_capacity = bitmap.numel() if bitmap is not None else 0
            if ids is not None:
                # (a tensor without elements has no pointer: the column has no rows then, and one id of padding keeps
                # the grouped form)
                if not ids.numel():
                    ids = torch.zeros(1, dtype=ids.dtype, device=ids.device)
                    keep.append(ids)
                c.group_ids = _dev_ptr(ids)
                c.group_ids_capacity = ids.numel() * width
                c.group_id_width = width
            c.n_groups = groups_list[i]
            c.ops, c.flags, c.reserved = mask, (N.SB_WGT_SQUARE if square else 0), 0
            result_type = col.physical_type
            if not square:
                if not wt.numel():
                    wt = torch.zeros(1, dtype=wt.dtype, device=wt.device)
                    keep.append(wt)
                c.weights = _dev_ptr(wt)
                c.weights_capacity = wt.numel() * wt.element_size()
                c.weights_validity = _dev_ptr(wv)
                c.weights_validity_capacity = wv.numel() if wv is not None and wv.numel() else 0
                c.weight_type = wtype
                if wtype in _FLOATS and col.physical_type in NUMPY_DTYPES:
                    result_type = _P.FLOAT64   # (Group.sum: a double if either operand is a float)
            garr = (N.AggGroupC * groups_list[i])()
            keep.append(garr)
            c.groups = garr
            res.append(GroupedAggregate(result_type, mask, c, garr))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.results = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_aggregate_weighted(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.results


def aggregate_weighted(ctx, columns: List[ColumnPages], weights, group_ids=None, n_groups=1, selection=None,
                       ops: Sequence[str] = ("count", "sum"), square: bool = False) -> List[GroupedAggregate]:
    """Enqueue count and sum(y * w) per group of columns[i] under selection[i], group_ids[i] and weights[i] on
    ctx's stream, behind the calls that write the bitmaps, the ids and the weights; results after
    ctx.synchronize().  Group.sum is an exact Python int when y and w are integers, a float otherwise."""
    return WeightedAggregateBatch(ctx, columns, weights, group_ids, n_groups, selection, ops, square).enqueue()
