"""strawboat_amd — MI355X-native page encode/decode path of strawboat (sundy-li/strawboat).

Host-side mirror of the reference's `read::` / `write::` page-level API over the C ABI of
libstrawboat_hip.so (hand-written gfx950 kernels).  PyTorch is used for device memory and
streams only.  There is no CPU fallback: without the built library and a GPU, calls raise.
"""
from .types import (ColumnMeta, CommonCompression, Compression, PageMeta, PhysicalType,  # noqa: F401
                    WriteOptions)
from .context import Context  # noqa: F401
from . import filter, read, shard, write  # noqa: F401
from .filter import Predicate, Selection, filter_columns, like_predicate  # noqa: F401
from .filter_in import FilterInBatch, InList, filter_in  # noqa: F401
from .filter_cmp import FilterCmpBatch, filter_columns_cmp, filter_pair  # noqa: F401
from .read_selected import ReadSelectedBatch, SelectedArray, read_selected  # noqa: F401
from .read_selected_var import ReadSelectedVarBatch, SelectedBinaryArray, read_selected_var  # noqa: F401
from .aggregate import Aggregate, AggregateBatch, aggregate_columns  # noqa: F401
from .aggregate_grouped import GroupedAggregate, GroupedAggregateBatch, aggregate_grouped  # noqa: F401
from .aggregate_grouped_large import GroupedAggregateLargeBatch, aggregate_grouped_large  # noqa: F401
from .aggregate_weighted import WeightedAggregateBatch, aggregate_weighted  # noqa: F401
from .topk import TopK, TopKBatch, selection_of_rows, topk_columns  # noqa: F401
from .key_ids import KeyIds, KeyIdsBatch, key_ids  # noqa: F401
from .key_ids_var import KeyIdsVar, KeyIdsVarBatch, key_ids_var  # noqa: F401
from .key_lookup import KeyLookup, KeyLookupBatch, key_lookup  # noqa: F401
from .key_buckets import KeyBuckets, KeyBucketsBatch, key_buckets  # noqa: F401
from .key_combine import KeyCombine, KeyCombineBatch, key_combine  # noqa: F401
from .group_by import GroupKeys, Histogram, group_by, group_by_buckets, group_by_keys, histogram, group_by_weighted  # noqa: F401

__all__ = ["Context", "read", "write", "filter", "Predicate", "Selection", "filter_columns", "like_predicate", "InList", "FilterInBatch", "filter_in", "FilterCmpBatch", "filter_columns_cmp", "filter_pair", "read_selected", "ReadSelectedBatch", "SelectedArray",
           "read_selected_var", "ReadSelectedVarBatch", "SelectedBinaryArray", "aggregate_columns", "AggregateBatch", "Aggregate",
           "aggregate_grouped", "GroupedAggregateBatch", "GroupedAggregate", "aggregate_grouped_large", "GroupedAggregateLargeBatch", "aggregate_weighted", "WeightedAggregateBatch", "group_by", "group_by_weighted", "topk_columns", "TopKBatch", "TopK", "selection_of_rows", "key_ids", "KeyIdsBatch", "KeyIds", "key_ids_var", "KeyIdsVarBatch", "KeyIdsVar", "key_combine", "KeyCombineBatch", "KeyCombine", "GroupKeys", "key_lookup", "KeyLookupBatch", "KeyLookup", "group_by_keys", "key_buckets", "KeyBucketsBatch", "KeyBuckets", "group_by_buckets", "histogram", "Histogram", "WriteOptions", "PageMeta", "ColumnMeta", "Compression",
           "CommonCompression", "PhysicalType"]
