"""group_by:: — SELECT k, count(*), count(y), min(y), max(y), sum(y) ... WHERE ... GROUP BY k in one call.

The whole chain on the device, in one synchronize interval: `key_ids` (integer keys) or `key_ids_var` (Binary /
Utf8 keys) turns the key column into dense ids, `aggregate_grouped` (max_keys <= 256) or
`aggregate_grouped_large` (up to 1024) reduces the value columns per id.  The number of distinct keys is not
known before the synchronize, so every value column gets `max_keys` groups; the groups behind `n_keys` are
empty, and `trim` cuts them off afterwards.  The selected rows whose key is null arrive in `out_of_range`.  More
than `max_keys` distinct keys set the keys result's `overflow`, which is passed through, not raised: the groups
mean nothing then.

GROUP BY a, b: a list of 2 to 4 key columns.  Each goes through its key call with `max_keys`, `key_combine` turns
the parts' ids into the ids of the distinct tuples, and the aggregate call takes those: still one interval.  A row
with a null in any key column has no tuple and arrives in `out_of_range`.
"""
from typing import List, Sequence, Tuple

import numpy as np

from . import _native as N
from .aggregate_grouped import MAX_GROUPS, Group, GroupedAggregate, aggregate_grouped
from .aggregate_grouped_large import MAX_GROUPS_LARGE, aggregate_grouped_large
from .key_combine import MAX_PARTS, key_combine
from .key_ids import INTEGER_TYPES, key_ids
from .key_ids_var import BINARY_TYPES, key_ids_var
from .read import ColumnPages


def check_group_by(key_type, max_keys):
    """The refusals that need no device: the key's type and max_keys."""
    if key_type not in INTEGER_TYPES and key_type not in BINARY_TYPES:
        raise ValueError("group_by keys are 8- to 64-bit integers or Binary / LargeBinary, not physical type %d" % key_type)
    if isinstance(max_keys, bool) or not isinstance(max_keys, (int, np.integer)) or not 1 <= max_keys <= MAX_GROUPS_LARGE:
        raise ValueError("max_keys is %r, not an int in 1 .. %d" % (max_keys, MAX_GROUPS_LARGE))


class GroupKeys:
    """The keys of a GROUP BY over several columns: the parts' own key results and the combined tuples; the scalars
    and `keys` are valid after Context.synchronize()."""

    def __init__(self, parts, combined):
        #: one KeyIds / KeyIdsVar per key column, in the order of the key list
        self.parts = parts
        #: the KeyCombine over their ids
        self.combined = combined

    ids = property(lambda self: self.combined.ids)
    n_keys = property(lambda self: self.combined.n_keys)
    max_keys = property(lambda self: self.combined.max_keys)

    @property
    def overflow(self):
        """true if any part or the combine overflowed: the ids, and with them the groups, mean nothing then"""
        return bool(self.combined.overflow) or any(bool(p.overflow) for p in self.parts)

    @property
    def keys(self):
        """the distinct key tuples in ascending order, as tuples of the key columns' values (empty on an overflow)"""
        return [] if self.overflow else self.combined.keys()

    def __repr__(self):
        return "GroupKeys(n_keys=%d, overflow=%r, parts=%r)" % (self.n_keys, self.overflow, self.parts)


def _composite_keys(ctx, keys, selection, max_keys):
    """the keys of a list of 2 .. 4 key columns: the integer parts in one key_ids call, the Binary / Utf8 parts in one
    key_ids_var call, then key_combine, all in the open interval"""
    keys = list(keys)
    if not 2 <= len(keys) <= MAX_PARTS:
        raise ValueError("group_by takes one key column or a list of 2 .. %d, not %d" % (MAX_PARTS, len(keys)))
    for k in keys:
        if not isinstance(k, ColumnPages):
            raise ValueError("a key is a ColumnPages, not %r" % type(k).__name__)
        check_group_by(k.physical_type, max_keys)
    max_keys = int(max_keys)
    ints = [i for i, k in enumerate(keys) if k.physical_type in INTEGER_TYPES]
    strs = [i for i, k in enumerate(keys) if k.physical_type not in INTEGER_TYPES]
    parts = [None] * len(keys)
    # (every part gets max_keys: a part with more distinct values than that cannot have fewer tuples)
    if ints:
        for i, r in zip(ints, key_ids(ctx, [keys[i] for i in ints], selection, max_keys=max_keys)):
            parts[i] = r
    if strs:
        for i, r in zip(strs, key_ids_var(ctx, [keys[i] for i in strs], selection, max_keys=max_keys)):
            parts[i] = r
    return GroupKeys(parts, key_combine(ctx, parts, max_keys=max_keys))


def _keys_of(ctx, key, selection, max_keys):
    """the key call(s) of group_by / group_by_weighted, enqueued: a KeyIds, a KeyIdsVar or (a key list) a GroupKeys"""
    if isinstance(key, (list, tuple)):
        return _composite_keys(ctx, key, selection, max_keys)
    check_group_by(key.physical_type, max_keys)
    if key.physical_type in INTEGER_TYPES:
        return key_ids(ctx, [key], selection, max_keys=int(max_keys))[0]
    return key_ids_var(ctx, [key], selection, max_keys=int(max_keys))[0]


def group_by(ctx, key, values: List[ColumnPages], selection=None,
             ops: Sequence[str] = ("count", "min", "max", "sum"), max_keys: int = N.SB_KEY_MAX_KEYS) -> Tuple[object, List[GroupedAggregate]]:
    """Enqueue the keys and ids of `key` and the per-key aggregates of every column of `values` under `selection`
    (one for all, or None: every row) on ctx's stream.  Returns (keys_result, [GroupedAggregate per value column]):
    a KeyIds or KeyIdsVar, and results of max_keys groups each; all valid after ctx.synchronize().

    `key` may also be a list or tuple of 2 .. 4 ColumnPages, integer and Binary / Utf8 mixed (GROUP BY a, b): the
    keys result is then a GroupKeys, whose `keys` are tuples of the columns' values in ascending order."""
    kres = _keys_of(ctx, key, selection, max_keys)
    max_keys = int(max_keys)
    if not values:
        return kres, []
    call = aggregate_grouped if max_keys <= MAX_GROUPS else aggregate_grouped_large
    return kres, call(ctx, list(values), kres.ids, max_keys, selection, ops)


def group_by_weighted(ctx, key, values: List[ColumnPages], weights, selection=None, max_keys: int = N.SB_KEY_MAX_KEYS,
                      square: bool = False) -> Tuple[object, List[GroupedAggregate]]:
    """SELECT k, count(y), sum(y * w) ... WHERE ... GROUP BY k: group_by's key chain (`key` one column or a list of
    2 .. 4), then `aggregate_weighted` of every column of `values` with its entry of `weights` (None with
    square=True: sum(y * y)), in the open interval.  Returns what group_by returns; `trim` cuts the groups behind
    n_keys off."""
    from .aggregate_weighted import WeightedAggregateBatch, check_weights
    values = list(values)
    check_weights(ctx, values, weights, square)   # (before a key call is made)
    kres = _keys_of(ctx, key, selection, max_keys)
    if not values:
        return kres, []
    return kres, WeightedAggregateBatch(ctx, values, weights, kres.ids, int(max_keys), selection, ("count", "sum"), square).enqueue()


def group_by_keys(ctx, key: ColumnPages, key_values, values: List[ColumnPages], selection=None,
                  ops: Sequence[str] = ("count", "min", "max", "sum"), value_ids=None, n_groups=None):
    """GROUP BY over a key set that is given: `key_lookup` of `key` against `key_values` (with `value_ids`, several
    values may share a group), then the per-group aggregates of every column of `values`, in the open interval.
    Returns (KeyLookup, [GroupedAggregate per value column]); group g belongs to key_values[g], or to the values whose
    value id is g.  n_groups: None = the largest id + 1.  The ids are the list's own, so the groups of two calls with one
    list are index-aligned: the count and sum records of two row groups, files or ranks add, group by group.  Selected
    rows whose key is null or not in the list arrive in `out_of_range`."""
    from .key_lookup import key_lookup, list_values
    n_values = len(list_values(key.physical_type, key_values))
    if value_ids is None:
        largest = n_values - 1
    else:
        ids = [int(v) for v in (value_ids.tolist() if isinstance(value_ids, np.ndarray) else value_ids)]
        largest = max(ids) if ids else -1
    if n_groups is None:
        n_groups = max(1, largest + 1)
    if isinstance(n_groups, bool) or not isinstance(n_groups, (int, np.integer)) or not 1 <= n_groups <= MAX_GROUPS_LARGE:
        raise ValueError("n_groups is %r, not an int in 1 .. %d" % (n_groups, MAX_GROUPS_LARGE))
    if largest >= n_groups:
        raise ValueError("the list hands out the id %d, n_groups is %d" % (largest, n_groups))
    n_groups = int(n_groups)
    kres = key_lookup(ctx, [key], [key_values], None if value_ids is None else [value_ids], selection)[0]
    if not values:
        return kres, []
    call = aggregate_grouped if n_groups <= MAX_GROUPS else aggregate_grouped_large
    return kres, call(ctx, list(values), kres.ids, n_groups, selection, ops)


def _bucket_groups(key, bounds, bucket_ids, n_groups, nan_id):
    """What group_by_buckets checks before anything is enqueued: the bounds, and that every id has a group.
    Returns (the bounds as an array, n_groups)."""
    from .key_buckets import NONE, bounds_values
    if not isinstance(key, ColumnPages):
        raise ValueError("a column is a ColumnPages, not %r" % type(key).__name__)
    arr = bounds_values(key.physical_type, bounds)
    if bucket_ids is None:
        handed = [int(arr.size)]
    else:
        raw = bucket_ids.tolist() if isinstance(bucket_ids, np.ndarray) else list(bucket_ids)
        handed = [int(v) for v in raw if isinstance(v, (int, np.integer)) and not isinstance(v, bool) and int(v) != NONE]
    if isinstance(nan_id, (int, np.integer)) and not isinstance(nan_id, bool) and int(nan_id) != NONE:
        handed.append(int(nan_id))
    largest = max(handed) if handed else -1
    if n_groups is None:
        n_groups = max(1, largest + 1)
    if isinstance(n_groups, bool) or not isinstance(n_groups, (int, np.integer)) or not 1 <= n_groups <= MAX_GROUPS_LARGE:
        raise ValueError("n_groups is %r, not an int in 1 .. %d" % (n_groups, MAX_GROUPS_LARGE))
    if largest >= n_groups:
        raise ValueError("the buckets hand out the id %d, n_groups is %d" % (largest, n_groups))
    return arr, int(n_groups)


def group_by_buckets(ctx, key: ColumnPages, bounds, values: List[ColumnPages], selection=None,
                     ops: Sequence[str] = ("count", "min", "max", "sum"), bucket_ids=None, n_groups=None,
                     right_closed=False, nan_id=None):
    """GROUP BY where the key falls: `key_buckets` of `key` among `bounds`, then the per-group aggregates of every
    column of `values` (`aggregate_grouped` up to 256 groups, `aggregate_grouped_large` beyond), in the open interval.
    Returns (KeyBuckets, [GroupedAggregate per value column]); group g is bucket g, or the buckets whose bucket id is
    g.  n_groups: None = the largest id + 1.  The ids are the bounds' own, so the groups of two calls with one list of
    bounds are index-aligned: the count and sum records of two row groups, files or ranks add, group by group.
    Selected rows whose key is null, a NaN without a `nan_id`, or in a bucket without an id arrive in `out_of_range`."""
    from .key_buckets import KeyBucketsBatch
    arr, n_groups = _bucket_groups(key, bounds, bucket_ids, n_groups, nan_id)
    batch = KeyBucketsBatch(ctx, [key], [arr], None if bucket_ids is None else [bucket_ids], selection, right_closed, nan_id)
    agg = None
    if values:   # (both calls are prepared, and with that checked, before either is enqueued)
        from .aggregate_grouped import GroupedAggregateBatch
        from .aggregate_grouped_large import GroupedAggregateLargeBatch
        prepared = GroupedAggregateBatch if n_groups <= MAX_GROUPS else GroupedAggregateLargeBatch
        agg = prepared(ctx, list(values), batch.results[0].ids, n_groups, selection, ops)
    kres = batch.enqueue()[0]
    return kres, agg.enqueue() if agg is not None else []


class Histogram:
    """The count-only chain of `histogram`; every property is valid after Context.synchronize()."""

    def __init__(self, buckets, aggregate):
        #: the KeyBuckets of the column
        self.buckets = buckets
        #: the GroupedAggregate ("count") of the column under its own bucket ids
        self.aggregate = aggregate

    @property
    def counts(self):
        """the n_bounds + 1 counts of the selected, non-null rows that are not NaN, as an int64 array"""
        return np.array([g.count for g in self.aggregate.groups], dtype=np.int64)

    nans = property(lambda self: self.buckets.nans)

    def __repr__(self):
        return "Histogram(buckets=%d, %r)" % (self.buckets.n_bounds + 1, self.buckets)


def histogram(ctx, column: ColumnPages, bounds, selection=None, right_closed=False) -> Histogram:
    """The histogram of a numeric column over `bounds`: `key_buckets` of the column, then the count of the column
    itself per bucket, in the open interval.  After the synchronize `counts` has the n_bounds + 1 counts; nulls and
    NaNs are in none of them (`nans` counts the latter)."""
    kres, aggs = group_by_buckets(ctx, column, bounds, [column], selection, ("count",), None, None, right_closed, None)
    return Histogram(kres, aggs[0])


def trim(keys_result, aggregates: List[GroupedAggregate]) -> List[List[Group]]:
    """After the synchronize: the groups of every value column that have a key, groups[i][g] belonging to key g of
    keys_result.  Raises on an overflow of the keys: the ids, and with them the groups, mean nothing then."""
    if keys_result.overflow:
        raise ValueError("the key column has more distinct keys than max_keys (overflow %d)" % int(keys_result.overflow))
    n = keys_result.n_keys
    return [list(a.groups[:n]) for a in aggregates]
