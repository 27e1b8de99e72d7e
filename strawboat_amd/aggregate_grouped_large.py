"""aggregate_grouped_large:: — `aggregate_grouped` for up to 1024 groups.

`key_ids` / `key_ids_var` hand out up to 1024 ids; `aggregate_grouped` stops at 256 groups.  This call takes
the same inputs and gives the same `GroupedAggregate` / `Group` results for n_groups 1 .. 1024
(sb_aggregate_grouped_large in include/strawboat_hip.h).  One thing differs: the bits of a float sum are this
call's own -- the same every time it is issued, but not necessarily those `aggregate_grouped` gives for the same
input.
"""
from typing import List, Optional, Sequence

from . import _native as N
from .aggregate import check_column as _check_ungrouped, ops_mask
from .aggregate_grouped import GroupedAggregate, _ids_of
from .filter import Selection
from .read import ColumnPages, _dev_ptr
from .read_selected import _bitmap_of

MAX_GROUPS_LARGE = N.SB_AGG_LARGE_MAX_GROUPS


def check_column(physical_type, rows: int, bitmap_bytes: Optional[int], ops: int, n_groups: int,
                 id_width: Optional[int], id_count: int):
    """The refusals of aggregate_grouped.check_column, with MAX_GROUPS_LARGE as the limit of n_groups."""
    _check_ungrouped(physical_type, rows, bitmap_bytes, ops)
    if isinstance(n_groups, bool) or not isinstance(n_groups, int) or not 1 <= n_groups <= MAX_GROUPS_LARGE:
        raise ValueError("n_groups is %r, not an int in 1 .. %d" % (n_groups, MAX_GROUPS_LARGE))
    if id_width not in (1, 2, 4):
        raise ValueError("group ids are uint8, uint16, uint32 or int32")
    if id_count < rows:
        raise ValueError("%d group ids for a column of %d rows" % (id_count, rows))


class GroupedAggregateLargeBatch:
    """A prepared sb_aggregate_grouped_large call: GroupedAggregateBatch with n_groups up to 1024.

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
        ctx._check(ctx._lib.sb_aggregate_grouped_large(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.results


def aggregate_grouped_large(ctx, columns: List[ColumnPages], group_ids, n_groups, selection=None,
                            ops: Sequence[str] = ("count", "min", "max", "sum")) -> List[GroupedAggregate]:
    """Enqueue the per-group aggregates of columns[i] under selection[i] and group_ids[i], n_groups up to 1024, on
    ctx's stream, behind the filter calls that write the bitmaps and the calls that write the ids; results after
    ctx.synchronize()."""
    return GroupedAggregateLargeBatch(ctx, columns, group_ids, n_groups, selection, ops).enqueue()
