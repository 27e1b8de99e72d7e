"""aggregate_grouped:: — count / min / max / sum of the selected rows of columns, per group, on the GPU.

`aggregate_columns` with a GROUP BY: SELECT k, count(*), count(y), min(y), max(y), sum(y) ... WHERE x < 5
GROUP BY k.  The pages of y, the selection bitmap of a `filter_columns` call and one unsigned id per row
— the key column k as `read_columns` decoded it, or ids the engine computed — go in; a record per group
comes back (sb_aggregate_grouped in include/strawboat_hip.h).  A selected row whose id is >= n_groups is
aggregated nowhere and counted in `out_of_range`.
"""
import struct
from typing import List, Optional, Sequence

from . import _native as N
from .aggregate import _FLOATS, _FORMATS, VALUE_OPS, check_column as _check_ungrouped, ops_mask
from .filter import Selection
from .read import ColumnPages, _dev_ptr
from .read_selected import _bitmap_of

MAX_GROUPS = N.SB_AGG_MAX_GROUPS
ID_WIDTHS = {"torch.uint8": 1, "torch.uint16": 2, "torch.uint32": 4, "torch.int32": 4}


def check_column(physical_type, rows: int, bitmap_bytes: Optional[int], ops: int, n_groups: int,
                 id_width: Optional[int], id_count: int):
    """The refusals that need no device: those of aggregate.check_column, the number of groups, the ids' width
    (None: a dtype that is none of uint8 / uint16 / uint32 / int32) and their number."""
    _check_ungrouped(physical_type, rows, bitmap_bytes, ops)
    if isinstance(n_groups, bool) or not isinstance(n_groups, int) or not 1 <= n_groups <= MAX_GROUPS:
        raise ValueError("n_groups is %r, not an int in 1 .. %d" % (n_groups, MAX_GROUPS))
    if id_width not in (1, 2, 4):
        raise ValueError("group ids are uint8, uint16, uint32 or int32")
    if id_count < rows:
        raise ValueError("%d group ids for a column of %d rows" % (id_count, rows))


def _ids_of(ctx, ids):
    """the ids as a contiguous tensor on the context's device, and their width (None: a dtype that has none)"""
    import torch
    if not isinstance(ids, torch.Tensor):
        raise ValueError("group_ids is a torch tensor (uint8 / uint16 / uint32 / int32) on the context's device")
    if ids.device != ctx.torch_device:
        raise ValueError("group_ids is on %s, the context on %s" % (ids.device, ctx.torch_device))
    if ids.dim() != 1 or not ids.is_contiguous():
        raise ValueError("group_ids is a contiguous 1-d tensor")
    return ids, ID_WIDTHS.get(str(ids.dtype))


class Group:
    """The aggregates of one group of one column."""

    def __init__(self, physical_type, ops, cgroup):
        self.physical_type = physical_type
        self.ops = ops
        self._c = cgroup

    selected = property(lambda self: int(self._c.selected))
    count = property(lambda self: int(self._c.count))
    nans = property(lambda self: int(self._c.nans))

    def _scalar(self, field, bit):
        if not (self.ops & bit) or self.count - self.nans == 0 or self.physical_type not in _FORMATS:
            return None
        return struct.unpack_from(_FORMATS[self.physical_type], bytes(field))[0]

    @property
    def min(self):
        """a Python scalar of the column's type; None for a group without a qualifying row (or min not asked for)"""
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
        """integers: the exact sum as a Python int; floats: the double sum of the group's live rows; None when sum
        was not asked for"""
        if not (self.ops & N.SB_AGG_SUM):
            return None
        lo, hi = int(self._c.sum_lo), int(self._c.sum_hi)
        if self.physical_type in _FLOATS:
            return struct.unpack("<d", struct.pack("<Q", lo))[0]
        v = (hi << 64) | lo
        return v - (1 << 128) if hi >> 63 else v

    def __repr__(self):
        return "Group(selected=%d, count=%d, nans=%d, min=%r, max=%r, sum=%r)" % (
            self.selected, self.count, self.nans, self.min, self.max, self.sum)


class GroupedAggregate:
    """The aggregates of one column, per group; every property is valid after Context.synchronize()."""

    def __init__(self, physical_type, ops, cstruct, cgroups):
        self.physical_type = physical_type
        self.ops = ops
        self._c = cstruct
        self._groups = cgroups
        self.groups = [Group(physical_type, ops, g) for g in cgroups]

    rows = property(lambda self: int(self._c.rows))
    selected = property(lambda self: int(self._c.selected))
    out_of_range = property(lambda self: int(self._c.out_of_range))
    n_groups = property(lambda self: len(self.groups))

    def __len__(self):
        return len(self.groups)

    def __getitem__(self, g):
        return self.groups[g]

    def __repr__(self):
        return "GroupedAggregate(rows=%d, selected=%d, out_of_range=%d, n_groups=%d)" % (
            self.rows, self.selected, self.out_of_range, len(self.groups))


class GroupedAggregateBatch:
    """A prepared grouped aggregate call: the C descriptors and the groups' records are built once; enqueue()
    then costs one C call.

    group_ids: one tensor per column or one for all; n_groups likewise an int per column or one for all;
    selection as in AggregateBatch."""

    def __init__(self, ctx, columns: List[ColumnPages], group_ids, n_groups, selection=None,
                 ops=("count", "min", "max", "sum")):
        import torch
        from .read import _prepare
        n = len(columns)
        mask = ops_mask(ops)
        if selection is None or isinstance(selection, (Selection, torch.Tensor)):
            selections = [selection] * n
        else:
            selections = list(selection)
        ids_list = [group_ids] * n if isinstance(group_ids, torch.Tensor) else list(group_ids)
        groups_list = list(n_groups) if isinstance(n_groups, (list, tuple)) else [n_groups] * n
        if len(selections) != n:
            raise ValueError("one selection per column (or one for all, or None)")
        if len(ids_list) != n or len(groups_list) != n:
            raise ValueError("one group_ids tensor and one n_groups per column (or one for all)")
        bitmaps, ids_dev = [], []
        for col, sel, ids, ng in zip(columns, selections, ids_list, groups_list):   # before anything is enqueued
            bitmap = None if sel is None else _bitmap_of(ctx, sel)
            ids, width = _ids_of(ctx, ids)
            m = col.metas_array()
            rows = int(m[:, 1].sum()) if m.shape[0] else 0
            check_column(col.physical_type, rows, None if bitmap is None else bitmap.numel(), mask, ng, width, ids.numel())
            bitmaps.append(bitmap)
            ids_dev.append((ids, width))
        rarr, keep = _prepare(ctx, columns)
        arr = (N.ColumnAggregateGroupedC * n)()
        res = []
        for i, col in enumerate(columns):
            c, r = arr[i], rarr[i]
            c.physical_type, c.is_nullable = r.physical_type, r.is_nullable
            c.pages, c.pages_len, c.metas, c.n_pages = r.pages, r.pages_len, r.metas, r.n_pages
            c.page_offsets = r.page_offsets
            keep.append(bitmaps[i])
            c.selection = _dev_ptr(bitmaps[i])
            c.selection_capacity = bitmaps[i].numel() if bitmaps[i] is not None else 0
            ids, width = ids_dev[i]
            keep.append(ids)
            c.group_ids = _dev_ptr(ids)
            c.group_ids_capacity = ids.numel() * width
            c.group_id_width, c.n_groups = width, groups_list[i]
            c.ops, c.reserved = mask, 0
            garr = (N.AggGroupC * groups_list[i])()
            keep.append(garr)
            c.groups = garr
            res.append(GroupedAggregate(col.physical_type, mask, c, garr))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.results = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_aggregate_grouped(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.results


def aggregate_grouped(ctx, columns: List[ColumnPages], group_ids, n_groups, selection=None,
                      ops: Sequence[str] = ("count", "min", "max", "sum")) -> List[GroupedAggregate]:
    """Enqueue the per-group aggregates of columns[i] under selection[i] and group_ids[i] on ctx's stream, behind
    the filter calls that write the bitmaps and the read calls that write the ids; results after
    ctx.synchronize()."""
    return GroupedAggregateBatch(ctx, columns, group_ids, n_groups, selection, ops).enqueue()
