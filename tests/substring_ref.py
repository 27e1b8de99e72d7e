"""The reference of the string predicates of sb_filter_columns_var: Python's own `lit in s`, `s.endswith(lit)` and
`s.startswith(lit)` over a list of `bytes` (the oracle's decode of the pages, test_gpu_filter_binary.oracle_strings),
ANDed with the validity; a "not_" op is `valid & ~positive`."""
import numpy as np

POSITIVE = {"starts_with": lambda s, lit: s.startswith(lit), "ends_with": lambda s, lit: s.endswith(lit),
            "contains": lambda s, lit: lit in s}
SUB_OPS = ["ends_with", "contains", "not_starts_with", "not_ends_with", "not_contains"]
OPS6 = ["starts_with"] + SUB_OPS   # the five new ops and starts_with for comparison


def sub_expected(strs, valid, op, lit):
    """bool per row"""
    lit = lit.encode("utf-8") if isinstance(lit, str) else bytes(lit)
    neg = op.startswith("not_")
    f = POSITIVE[op[4:] if neg else op]
    memo = {}
    pos = np.zeros(len(strs), bool)
    for i, s in enumerate(strs):
        r = memo.get(s)
        if r is None:
            r = memo[s] = bool(f(s, lit))
        pos[i] = r
    valid = np.asarray(valid, bool)
    return valid & ~pos if neg else valid & pos


def selective(strs, valid, op, lit):
    """the predicate selects some but not all of the valid rows: a constant answer cannot pass"""
    w = sub_expected(strs, valid, op, lit)
    return 0 < int(w.sum()) < int(np.asarray(valid, bool).sum())
