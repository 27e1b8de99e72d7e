"""filter:: — evaluate a predicate on the pages of primitive and binary columns, on the GPU.

What a query engine does first with the filter columns of a block: `WHERE x < 5 AND s = 'a'` over
the pages of `x` and `s` gives one bit per row (LSB-first, like an Arrow validity bitmap) and the
number of bits set, without the decoded values ever being written to memory
(sb_filter_columns_var in include/strawboat_hip.h).  Null rows satisfy no comparison; floats
compare as IEEE 754; Binary / Utf8 values compare as byte strings (bytes unsigned, a proper
prefix is less), and have "starts_with", "ends_with", "contains" and their "not_" forms beside
the six orderings (like_predicate maps the LIKE patterns these serve onto them).
"""
import ctypes as C
import math
import struct
from typing import List, Optional, Sequence

import numpy as np

from . import _native as N
from .read import ColumnPages, _dev_ptr
from .types import PhysicalType

OPS = {"eq": N.SB_PRED_EQ, "ne": N.SB_PRED_NE, "lt": N.SB_PRED_LT, "le": N.SB_PRED_LE, "gt": N.SB_PRED_GT,
       "ge": N.SB_PRED_GE, "is_null": N.SB_PRED_IS_NULL, "is_not_null": N.SB_PRED_IS_NOT_NULL,
       "starts_with": N.SB_PRED_STARTS_WITH, "ends_with": N.SB_PRED_ENDS_WITH, "contains": N.SB_PRED_CONTAINS,
       "not_starts_with": N.SB_PRED_NOT_STARTS_WITH, "not_ends_with": N.SB_PRED_NOT_ENDS_WITH,
       "not_contains": N.SB_PRED_NOT_CONTAINS}
STRING_OPS = ("starts_with", "ends_with", "contains", "not_starts_with", "not_ends_with", "not_contains")
COMBINE = {"set": N.SB_SEL_SET, "and": N.SB_SEL_AND, "or": N.SB_SEL_OR}

_P = PhysicalType
_INT_FORMATS = {_P.INT8: "<b", _P.INT16: "<h", _P.INT32: "<i", _P.INT64: "<q",
                _P.UINT8: "<B", _P.UINT16: "<H", _P.UINT32: "<I", _P.UINT64: "<Q"}


def pack_literal(physical_type, value) -> bytes:
    """The 8 literal bytes of sb_column_filter for a value of the column's own physical type.
    No implicit widening: an integer that does not fit the type, or a float that is not integral
    for an integer column, raises ValueError (the engine above folds `int8_col < 1000` itself)."""
    if isinstance(value, (bool, np.bool_)):
        raise ValueError("a boolean is not a literal of a numeric column")
    if physical_type in _INT_FORMATS:
        if isinstance(value, (float, np.floating)):
            if not math.isfinite(value) or value != math.floor(value):
                raise ValueError("literal %r is not integral, the column is an integer column" % (value,))
            value = int(value)
        elif isinstance(value, (int, np.integer)):
            value = int(value)
        else:
            raise ValueError("literal %r is not a number" % (value,))
        try:
            raw = struct.pack(_INT_FORMATS[physical_type], value)
        except struct.error:
            raise ValueError("literal %d does not fit physical type %d" % (value, physical_type))
    elif physical_type in (_P.FLOAT32, _P.FLOAT64):
        if not isinstance(value, (int, float, np.integer, np.floating)):
            raise ValueError("literal %r is not a number" % (value,))
        value = float(value)
        if physical_type == _P.FLOAT32:
            with np.errstate(over="ignore"):
                f = np.float32(value)
            if math.isfinite(value) and not np.isfinite(f):
                raise ValueError("literal %r does not fit a 32-bit float" % (value,))
            raw = f.tobytes()
        else:
            raw = struct.pack("<d", value)
    else:
        raise ValueError("comparison predicates are implemented for 8- to 64-bit integers and floats, "
                         "not physical type %d" % physical_type)
    return raw + b"\0" * (8 - len(raw))


_BINARY = (_P.BINARY, _P.LARGE_BINARY)
_WIDTH = {_P.INT8: 1, _P.UINT8: 1, _P.INT16: 2, _P.UINT16: 2, _P.INT32: 4, _P.UINT32: 4, _P.FLOAT32: 4,
          _P.INT64: 8, _P.UINT64: 8, _P.FLOAT64: 8}


def literal_bytes(physical_type, op, value) -> bytes:
    """The literal of sb_column_filter_var: exactly the type's width for a number (pack_literal's
    rules), the bytes themselves for a Binary / LargeBinary column (`str` is encoded as UTF-8).
    A bytes / str literal on a numeric column, a number on a binary column and a string op
    ("starts_with", "ends_with", "contains" and their "not_" forms) on a numeric column raise
    ValueError."""
    if op in ("is_null", "is_not_null"):
        return b""
    if physical_type in _BINARY:
        if isinstance(value, str):
            return value.encode("utf-8")
        if isinstance(value, (bytes, bytearray, memoryview)):
            return bytes(value)
        raise ValueError("literal %r is not bytes or str, the column is a binary column" % (value,))
    if op in STRING_OPS:
        raise ValueError("%s needs a Binary / LargeBinary column, not physical type %d" % (op, physical_type))
    if isinstance(value, (str, bytes, bytearray, memoryview)):
        raise ValueError("literal %r is not a number" % (value,))
    return pack_literal(physical_type, value)[:_WIDTH[physical_type]]


class Predicate:
    """op: "eq" "ne" "lt" "le" "gt" "ge" (with a literal), "starts_with" "ends_with" "contains"
    "not_starts_with" "not_ends_with" "not_contains" (binary columns, with a bytes / str literal;
    a "not_" op selects the non-null rows whose positive form is false) or "is_null"
    "is_not_null" (without)."""

    def __init__(self, op, literal=None):
        if op not in OPS:
            raise ValueError("unknown predicate %r" % (op,))
        if op in ("is_null", "is_not_null"):
            if literal is not None:
                raise ValueError("%s takes no literal" % op)
        elif literal is None:
            raise ValueError("%s needs a literal" % op)
        self.op = op
        self.literal = literal

    def __repr__(self):
        return "Predicate(%r, %r)" % (self.op, self.literal)


def like_predicate(pattern, negate=False, escape="\\") -> Predicate:
    """The Predicate of SQL's `col LIKE pattern` (`NOT LIKE` with negate) for the patterns the
    device serves: 'lit' -> eq (ne), 'lit%' -> starts_with, '%lit' -> ends_with, '%lit%' ->
    contains (the "not_" ops when negated), '%' / '%%' -> starts_with b"" (every non-null row).
    `escape` + '%', '_' or the escape character itself is that character, literally.  Every other
    pattern, which means a '%' inside the literal or an unescaped '_', raises NotImplementedError.
    Runs on the host only; `pattern` is str or bytes, and so is the literal."""
    is_str = isinstance(pattern, str)
    if not is_str and not isinstance(pattern, (bytes, bytearray, memoryview)):
        raise ValueError("pattern %r is not str or bytes" % (pattern,))
    text = pattern if is_str else bytes(pattern).decode("latin-1")   # (one character per byte, mapped back below)
    esc = escape if isinstance(escape, str) else bytes(escape).decode("latin-1")
    if len(esc) != 1:
        raise ValueError("escape must be one character")
    lit, wild = [], []   # the literal's characters; positions in `lit` where a '%' stands in front
    i = 0
    while i < len(text):
        ch = text[i]
        if ch == esc:
            if i + 1 >= len(text) or text[i + 1] not in ("%", "_", esc):
                raise ValueError("pattern %r: the escape character must be followed by %%, _ or itself" % (pattern,))
            lit.append(text[i + 1])
            i += 2
            continue
        if ch == "_":
            raise NotImplementedError("LIKE pattern %r: '_' is not served on the device" % (pattern,))
        if ch == "%":
            wild.append(len(lit))
        else:
            lit.append(ch)
        i += 1
    if any(0 < w < len(lit) for w in wild):
        raise NotImplementedError("LIKE pattern %r: a '%%' inside the literal is not served on the device" % (pattern,))
    literal = "".join(lit)
    literal = literal if is_str else literal.encode("latin-1")
    head = bool(wild) and wild[0] == 0
    tail = bool(wild) and wild[-1] == len(lit)
    if not lit and wild:
        op = "starts_with"   # matches every non-null row
    elif head and tail:
        op = "contains"
    elif head:
        op = "ends_with"
    elif tail:
        op = "starts_with"
    else:
        return Predicate("ne" if negate else "eq", literal)
    return Predicate("not_" + op if negate else op, literal)


class Selection:
    """The selection bitmap of one column in HBM; `selected` is valid after Context.synchronize()."""

    def __init__(self, bitmap, rows, cstruct):
        self.bitmap = bitmap   # torch.uint8, 4*ceil(rows/32) bytes
        self.rows = rows
        self._c = cstruct

    @property
    def selected(self):
        return int(self._c.selected)

    def numpy(self):
        """bool array of `rows` entries"""
        b = self.bitmap[:(self.rows + 7) // 8].cpu().numpy()
        return np.unpackbits(b, bitorder="little")[:self.rows].astype(bool)


class FilterBatch:
    """A prepared filter call: the C descriptors and the selection buffers are built once;
    enqueue() then costs one C call (steady-state callers, scripts/filter_probe.py)."""

    def __init__(self, ctx, columns: List[ColumnPages], predicates: Sequence[Predicate], combine="set",
                 out: Optional[List[Selection]] = None, stage_capacity: Optional[Sequence[int]] = None):
        import torch
        from .read import _prepare
        if len(columns) != len(predicates):
            raise ValueError("one predicate per column")
        if combine not in COMBINE:
            raise ValueError("unknown combine mode %r" % (combine,))
        if combine != "set" and out is None:
            raise ValueError("combine=%r needs the selections to combine with (out=)" % combine)
        if out is not None and len(out) != len(columns):
            raise ValueError("one selection per column")
        if stage_capacity is not None and len(stage_capacity) != len(columns):
            raise ValueError("one stage_capacity per column")
        n = len(columns)
        literals = []
        for col, pr in zip(columns, predicates):   # every literal is checked before anything is enqueued
            literals.append(literal_bytes(col.physical_type, pr.op, pr.literal))
        rarr, keep = _prepare(ctx, columns)   # (validates the page tensors; the descriptors' common head)
        arr = (N.ColumnFilterVarC * n)()
        res = []
        with torch.cuda.stream(ctx.torch_stream):
            for i, (col, pr) in enumerate(zip(columns, predicates)):
                c, r = arr[i], rarr[i]
                c.physical_type, c.is_nullable = r.physical_type, r.is_nullable
                c.pages, c.pages_len, c.metas, c.n_pages = r.pages, r.pages_len, r.metas, r.n_pages
                c.page_offsets = r.page_offsets
                c.op = OPS[pr.op]
                c.combine = COMBINE[combine]
                buf = C.create_string_buffer(literals[i], max(1, len(literals[i])))   # (read again by a replay: kept with the batch)
                keep.append(buf)
                c.literal = C.addressof(buf)
                c.literal_len = len(literals[i])
                c.stage_capacity = int(stage_capacity[i]) if stage_capacity is not None else 0
                rows = int(col.metas_array()[:, 1].sum()) if c.n_pages else 0
                if out is not None:
                    if out[i].rows != rows:
                        raise ValueError("selection %d has %d rows, the column %d" % (i, out[i].rows, rows))
                    bitmap = out[i].bitmap
                else:
                    bitmap = torch.empty(((rows + 31) // 32) * 4, dtype=torch.uint8, device=ctx.torch_device)
                keep.append(bitmap)
                c.selection = _dev_ptr(bitmap)
                c.selection_capacity = bitmap.numel()
                res.append(Selection(bitmap, rows, c))
        self.ctx, self._arr, self._keep, self._n = ctx, arr, keep, n
        self.selections = res

    def enqueue(self):
        ctx = self.ctx
        ctx._keep.append(self)
        ctx._check(ctx._lib.sb_filter_columns_var(ctx._h, self._arr, self._n, N.SB_MEM_DEVICE))
        return self.selections


def filter_columns(ctx, columns: List[ColumnPages], predicates: Sequence[Predicate], combine="set",
                   out: Optional[List[Selection]] = None, stage_capacity: Optional[Sequence[int]] = None) -> List[Selection]:
    """Enqueue predicates[i] over columns[i] on ctx's stream; numeric and binary columns may share
    a call.  combine: "set" writes the result, "and" / "or" combine it with what `out[i].bitmap`
    holds (chain predicates with one call after the other).  `out` re-uses earlier selections'
    buffers; required for "and" / "or".  stage_capacity[i]: the bytes the value blocks of a binary
    column's LZ4 / Zstd / Snappy pages may inflate to (0 / None: 4 x the column's page bytes)."""
    return FilterBatch(ctx, columns, predicates, combine, out, stage_capacity).enqueue()
