"""topk:: — ORDER BY y [DESC] LIMIT k of the selected rows of columns, on the GPU.

The fourth thing a scan does with a block: `filter_columns` turns the WHERE columns into a selection
bitmap, and `topk_columns` answers SELECT ... ORDER BY y LIMIT k without materialising the selected
values: the pages and the bitmap go in, the k best rows come back with their row numbers
(sb_topk_columns in include/strawboat_hip.h).  A row takes part if its selection bit is set, it is not
null and it is not NaN; ties are broken by the lower row number, in both orders, so the result is unique.
`selection_of_rows` turns the winners' row numbers into a bitmap with which `read_selected` fetches
their other columns.
"""
from typing import List, Optional

import numpy as np

from . import _native as N
from .filter import Selection
from .read import ColumnPages, _dev_ptr
from .read_selected import NUMPY_DTYPES, _bitmap_of, selection_bytes

MAX_K = N.SB_TOPK_MAX_K


def check_column(physical_type, rows: int, bitmap_bytes: Optional[int], k, largest):
    """The refusals that need no device: the type, k, the order, the bitmap's length."""
    if physical_type not in NUMPY_DTYPES:
        raise ValueError("top-k is implemented for 8- to 64-bit integers and floats, not physical type %d" % physical_type)
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K:
        raise ValueError("k is %r, not an int in 1 .. %d" % (k, MAX_K))
    if not isinstance(largest, (bool, np.bool_)):
        raise ValueError("largest is %r, not a bool" % (largest,))
    if bitmap_bytes is not None and bitmap_bytes < selection_bytes(rows):
        raise ValueError("the selection bitmap has %d bytes, %d rows need %d (4*ceil(rows/32))"
                         % (bitmap_bytes, rows, selection_bytes(rows)))


class TopK:
    """The k best rows of one column; every property is valid after Context.synchronize()."""

    def __init__(self, physical_type, k, largest, cstruct, out):
        self.physical_type = physical_type
        self.k = k
        self.largest = largest
        self._c = cstruct
        self._out = out   # (TopKRowC * k)

    rows = property(lambda self: int(self._c.rows))
    selected = property(lambda self: int(self._c.selected))
    count = property(lambda self: int(self._c.count))
    nans = property(lambda self: int(self._c.nans))
    found = property(lambda self: int(self._c.found))

    @property
    def out_bytes(self):
        """all k entries of `out` as the library wrote them: 16 bytes each, zeros behind `found`"""
        return bytes(self._out)

    def _table(self):
        return np.frombuffer(self.out_bytes, dtype=np.dtype([("row", "<u8"), ("value", "V8")]))[:self.found]

    @property
    def row_ids(self):
        """np.uint64[found]: the winners' row numbers in the column, best first"""
        return self._table()["row"].copy()

    @property
    def value_bytes(self):
        """np.uint8[found, 8]: the winners' values, little endian in the first `width` bytes, 0 behind them"""
        return np.frombuffer(self._table()["value"].tobytes(), dtype=np.uint8).reshape(self.found, 8).copy()

    @property
    def values(self):
        """the winners' values as an array of the column's dtype, best first"""
        dt = np.dtype(NUMPY_DTYPES[self.physical_type])
        return self.value_bytes[:, :dt.itemsize].copy().view(dt).reshape(self.found)

    def __repr__(self):
        return "TopK(rows=%d, selected=%d, count=%d, nans=%d, found=%d, k=%d, largest=%r)" % (
            self.rows, self.selected, self.count, self.nans, self.found, self.k, self.largest)


class TopKBatch:
    """A prepared top-k call: the C descriptors are built once; enqueue() then costs one C call.

    k, largest: one value for all columns or one per column.  selection: one per column, a single one
    for all columns, or None (every row); each a filter.Selection or a contiguous uint8 tensor on the
    context's device."""

    def __init__(self, ctx, columns: List[ColumnPages], k, largest=False, selection=None):
        import torch
        from .read import _prepare
        n = len(columns)
        ks = list(k) if isinstance(k, (list, tuple)) else [k] * n
        orders = list(largest) if isinstance(largest, (list, tuple)) else [largest] * n
        if selection is None or isinstance(selection, (Selection, torch.Tensor)):
            selections = [selection] * n
        else:
            selections = list(selection)
        if len(ks) != n or len(orders) != n:
            raise ValueError("one k and one order per column (or one for all)")
        if len(selections) != n:
            raise ValueError("one selection per column (or one for all, or None)")
        bitmaps = []
        for col, sel, kk, lg in zip(columns, selections, ks, orders):   # every refusal that needs no device, before anything is enqueued
            bitmap = None if sel is None else _bitmap_of(ctx, sel)
            m = col.metas_array()
            rows = int(m[:, 1].sum()) if m.shape[0] else 0
            check_column(col.physical_type, rows, None if bitmap is None else bitmap.numel(), kk, lg)
            bitmaps.append(bitmap)
        rarr, keep = _prepare(ctx, columns)
        arr = (N.ColumnTopKC * n)()
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
            out = (N.TopKRowC * int(ks[i]))()
            keep.append(out)
            c.k, c.order, c.reserved = int(ks[i]), N.SB_TOPK_LARGEST if orders[i] else N.SB_TOPK_SMALLEST, 0
            c.out = out
            res.append(TopK(col.physical_type, int(ks[i]), bool(orders[i]), c, out))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.results = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_topk_columns(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.results


def topk_columns(ctx, columns: List[ColumnPages], k, largest=False, selection=None) -> List[TopK]:
    """Enqueue the top-k of columns[i] under selection[i] (or one selection for all, or None: every row)
    on ctx's stream, behind the filter calls that write the bitmaps; results after ctx.synchronize()."""
    return TopKBatch(ctx, columns, k, largest, selection).enqueue()


class _Selected:
    """what a Selection keeps of a C struct: the number of bits set"""

    def __init__(self, selected):
        self.selected = selected


def selection_of_rows(ctx, n_rows: int, row_ids) -> Selection:
    """The selection bitmap of a column of `n_rows` rows in which exactly the rows `row_ids` are set, on
    the context's device: with it `read_selected` fetches the other columns of a top-k's winners.

    `read_selected` returns its rows in ROW order, not in rank order.  To get rank order, permute them:
    with ids = topk.row_ids, the selected read's j-th value belongs to row np.sort(ids)[j], so
    values_in_rank_order = values[np.argsort(np.argsort(ids))]  (ids holds no row twice).

    The bitmap is built on the host and uploaded with one copy that has finished when this returns (the
    rows are on the host anyway, and 4*ceil(n_rows/32) bytes are few): no kernel of any stream writes it,
    so a call enqueued on the context's stream afterwards reads it whole."""
    import torch
    ids = np.asarray(row_ids, dtype=np.uint64).reshape(-1)
    if ids.size and int(ids.max()) >= n_rows:
        raise ValueError("row %d is not below n_rows = %d" % (int(ids.max()), n_rows))
    words = np.zeros(selection_bytes(n_rows) // 4, dtype=np.uint32)
    np.bitwise_or.at(words, (ids >> np.uint64(5)).astype(np.int64), np.uint32(1) << (ids & np.uint64(31)).astype(np.uint32))
    bitmap = torch.from_numpy(words.view(np.uint8)).to(ctx.torch_device)   # (pageable memory: the copy is synchronous)
    return Selection(bitmap, n_rows, _Selected(int(np.unique(ids).size)))
