"""filter_in:: — `WHERE c IN (...)` / `NOT IN` over the pages of primitive and binary columns, on the GPU.

One call searches a list of up to 1024 literals per column in one walk of the column's pages
(sb_filter_columns_in in include/strawboat_hip.h): once per run of an RLE page, per entry of a
Dict page, per OneValue page and per row of the others.  The result is the `Selection` of
filter::, so the calls chain with filter_columns, read_selected and aggregate_columns.
A null row is neither in a list nor outside it; numbers compare as "eq" does (-0.0 == 0.0, a NaN
row is in no list, a NaN literal matches nothing); binary values compare as byte strings.
"""
import ctypes as C
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N
from .filter import COMBINE, Selection, _BINARY, _WIDTH, pack_literal
from .read import ColumnPages, _dev_ptr

MAX_VALUES = N.SB_IN_MAX_VALUES


class InList:
    """The literals of one column, in any order, duplicates allowed; negate=True: NOT IN."""

    def __init__(self, values, negate=False):
        self.values = list(values)
        self.negate = bool(negate)
        if len(self.values) > MAX_VALUES:
            raise ValueError("an IN list has at most %d values, not %d" % (MAX_VALUES, len(self.values)))

    def __repr__(self):
        return "InList(%r, negate=%r)" % (self.values, self.negate)


def pack_list(physical_type, values):
    """(values bytes, offsets or None) as sb_column_filter_in takes them: numbers of the column's
    own type back to back (pack_literal's rules for each), binary literals back to back with
    their n + 1 offsets (`str` is encoded as UTF-8).  A bytes / str literal on a numeric column
    and a number on a binary column raise ValueError."""
    values = list(values)
    if len(values) > MAX_VALUES:
        raise ValueError("an IN list has at most %d values, not %d" % (MAX_VALUES, len(values)))
    if physical_type in _BINARY:
        parts = []
        for v in values:
            if isinstance(v, str):
                parts.append(v.encode("utf-8"))
            elif isinstance(v, (bytes, bytearray, memoryview)):
                parts.append(bytes(v))
            else:
                raise ValueError("literal %r is not bytes or str, the column is a binary column" % (v,))
        offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
        if parts:
            offsets[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        return b"".join(parts), offsets
    if physical_type not in _WIDTH:
        raise ValueError("IN lists are implemented for 8- to 64-bit integers, floats and binary types, "
                         "not physical type %d" % physical_type)
    w = _WIDTH[physical_type]
    out = []
    for v in values:
        if isinstance(v, (str, bytes, bytearray, memoryview)):
            raise ValueError("literal %r is not a number" % (v,))
        out.append(pack_literal(physical_type, v)[:w])
    return b"".join(out), None


class FilterInBatch:
    """A prepared sb_filter_columns_in call: descriptors, packed lists and selection buffers are
    built once; enqueue() then costs one C call.  Everything is validated before anything is
    enqueued."""

    def __init__(self, ctx, columns: List[ColumnPages], lists: Sequence[InList], combine="set",
                 out: Optional[List[Selection]] = None, stage_capacity: Optional[Sequence[int]] = None):
        if len(columns) != len(lists):
            raise ValueError("one list per column")
        if combine not in COMBINE:
            raise ValueError("unknown combine mode %r" % (combine,))
        if combine != "set" and out is None:
            raise ValueError("combine=%r needs the selections to combine with (out=)" % combine)
        if out is not None and len(out) != len(columns):
            raise ValueError("one selection per column")
        if stage_capacity is not None and len(stage_capacity) != len(columns):
            raise ValueError("one stage_capacity per column")
        n = len(columns)
        packed = []
        for col, lst in zip(columns, lists):
            if not isinstance(lst, InList):
                raise ValueError("%r is not an InList" % (lst,))
            packed.append(pack_list(col.physical_type, lst.values))
        rows = [int(col.metas_array()[:, 1].sum()) if len(col.metas_array()) else 0 for col in columns]
        if out is not None:
            for i in range(n):
                if out[i].rows != rows[i]:
                    raise ValueError("selection %d has %d rows, the column %d" % (i, out[i].rows, rows[i]))
        import torch
        from .read import _prepare
        rarr, keep = _prepare(ctx, columns)   # (validates the page tensors; the descriptors' common head)
        arr = (N.ColumnFilterInC * n)()
        res = []
        with torch.cuda.stream(ctx.torch_stream):
            for i, (col, lst) in enumerate(zip(columns, lists)):
                c, r = arr[i], rarr[i]
                c.physical_type, c.is_nullable = r.physical_type, r.is_nullable
                c.pages, c.pages_len, c.metas, c.n_pages = r.pages, r.pages_len, r.metas, r.n_pages
                c.page_offsets = r.page_offsets
                c.op = N.SB_PRED_NOT_IN if lst.negate else N.SB_PRED_IN
                c.combine = COMBINE[combine]
                raw, offsets = packed[i]
                buf = C.create_string_buffer(raw, max(1, len(raw)))   # (read again by a replay: kept with the batch)
                keep.append(buf)
                c.values = C.addressof(buf)
                if offsets is not None:
                    keep.append(offsets)
                    c.value_offsets = offsets.ctypes.data
                c.n_values = len(lst.values)
                c.stage_capacity = int(stage_capacity[i]) if stage_capacity is not None else 0
                if out is not None:
                    bitmap = out[i].bitmap
                else:
                    bitmap = torch.empty(((rows[i] + 31) // 32) * 4, dtype=torch.uint8, device=ctx.torch_device)
                keep.append(bitmap)
                c.selection = _dev_ptr(bitmap)
                c.selection_capacity = bitmap.numel()
                res.append(Selection(bitmap, rows[i], c))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.selections = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_filter_columns_in(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.selections


def filter_in(ctx, columns: List[ColumnPages], lists: Sequence[InList], combine="set",
              out: Optional[List[Selection]] = None, stage_capacity: Optional[Sequence[int]] = None) -> List[Selection]:
    """Enqueue lists[i] over columns[i] on ctx's stream; numeric and binary columns may share a
    call.  combine, out and stage_capacity are those of filter.filter_columns."""
    return FilterInBatch(ctx, columns, lists, combine, out, stage_capacity).enqueue()
