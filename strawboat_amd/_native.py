"""ctypes binding of include/strawboat_hip.h (the C ABI of libstrawboat_hip.so).

The library is the product: if it is missing, or there is no GPU, every entry point fails
loudly — there is no CPU fallback in this package.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libstrawboat_hip.so")

SB_OK = 0
SB_ERR_OUT_OF_SPEC, SB_ERR_EXTERNAL, SB_ERR_IO, SB_ERR_NYI, SB_ERR_INVALID = -1, -2, -3, -4, -5
SB_MEM_DEVICE, SB_MEM_HOST = 0, 1
SB_WRITE_LZ4_EXACT = 1

# every symbol include/strawboat_hip.h declares
EXPORTS = ("sb_version", "sb_ctx_create", "sb_ctx_destroy", "sb_ctx_synchronize", "sb_ctx_last_error",
           "sb_ctx_stream", "sb_read_columns", "sb_read_columns_sizes", "sb_write_bound", "sb_write_columns",
           "sb_ctx_profile", "sb_ctx_profile_read", "sb_ctx_zstd_block_stats", "sb_ctx_side_forks", "sb_ctx_replays", "sb_nested_levels_bound", "sb_nested_write_levels", "sb_nested_write_levels_enqueue", "sb_nested_read_levels_enqueue",
           "sb_nested_read_levels", "sb_nested_write_levels_batch", "sb_nested_read_levels_batch", "sb_file_last_error", "sb_file_writer_open", "sb_file_writer_start",
           "sb_file_writer_write_column", "sb_file_writer_finish", "sb_file_writer_close", "sb_file_reader_open",
           "sb_file_reader_n_columns", "sb_file_reader_column", "sb_file_reader_schema", "sb_file_reader_read_pages",
           "sb_file_reader_close", "sb_stat_page", "sb_schema_last_error", "sb_schema_to_bytes", "sb_schema_from_bytes",
           "sb_schema_metadata_from_bytes", "sb_filter_columns", "sb_filter_columns_var", "sb_read_selected",
           "sb_read_selected_var", "sb_aggregate_columns", "sb_aggregate_grouped", "sb_filter_columns_in",
           "sb_topk_columns", "sb_key_ids", "sb_key_ids_var", "sb_aggregate_grouped_large",
           "sb_key_combine", "sb_key_lookup", "sb_aggregate_weighted", "sb_key_buckets",
           "sb_filter_columns_cmp")

SB_PRED_EQ, SB_PRED_NE, SB_PRED_LT, SB_PRED_LE, SB_PRED_GT, SB_PRED_GE, SB_PRED_IS_NULL, SB_PRED_IS_NOT_NULL = range(8)
SB_PRED_STARTS_WITH = 8   # binary types only (sb_filter_columns_var)
SB_PRED_IN, SB_PRED_NOT_IN = 9, 10   # sb_filter_columns_in
# binary types only (sb_filter_columns_var)
SB_PRED_ENDS_WITH, SB_PRED_CONTAINS, SB_PRED_NOT_STARTS_WITH, SB_PRED_NOT_ENDS_WITH, SB_PRED_NOT_CONTAINS = range(11, 16)
SB_IN_MAX_VALUES = 1024
SB_SEL_SET, SB_SEL_AND, SB_SEL_OR = range(3)
SB_AGG_COUNT, SB_AGG_MIN, SB_AGG_MAX, SB_AGG_SUM = 1, 2, 4, 8
SB_AGG_MAX_GROUPS = 256
SB_AGG_LARGE_MAX_GROUPS = 1024   # == SB_KEY_MAX_KEYS
SB_WGT_SQUARE = 1                # sb_aggregate_weighted: flags bit 0, the weight of a row is its own y
SB_TOPK_MAX_K = 256
SB_TOPK_SMALLEST, SB_TOPK_LARGEST = 0, 1
SB_KEY_MAX_KEYS = 1024
SB_KEY_ID_NONE = 0xFFFFFFFF
SB_BUCKET_MAX_BOUNDS = 1023       # sb_key_buckets: 1024 buckets == SB_AGG_LARGE_MAX_GROUPS
SB_BUCKET_RIGHT_CLOSED = 1        # ... flags bit 0: bucket i is (bounds[i - 1], bounds[i]]
SB_KEY_VAR_MAX_BYTES = 1 << 20
SB_KEY_OVERFLOW_KEYS, SB_KEY_OVERFLOW_BYTES = 1, 2
SB_KEY_COMBINE_MAX_PARTS = 4


class PageMetaC(C.Structure):
    _fields_ = [("length", C.c_uint64), ("num_values", C.c_uint64)]


class WriteOptionsC(C.Structure):
    _fields_ = [("default_compression", C.c_int32), ("has_default_compress_ratio", C.c_int32),
                ("default_compress_ratio", C.c_double), ("max_page_size", C.c_uint64),
                ("forbidden_compressions", C.c_uint32), ("force_codec", C.c_int32),
                ("force_index_codec", C.c_int32), ("flags", C.c_uint32), ("rng_seed", C.c_uint64)]


class ColumnReadC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("values", C.c_void_p), ("values_capacity", C.c_uint64), ("validity", C.c_void_p),
                ("validity_capacity", C.c_uint64), ("offsets", C.c_void_p), ("offsets_capacity", C.c_uint64),
                ("rows", C.c_uint64), ("values_len", C.c_uint64), ("page_offsets", C.c_void_p)]


class ColumnFilterC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("op", C.c_int32), ("combine", C.c_int32),
                ("literal", C.c_uint8 * 8), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("rows", C.c_uint64), ("selected", C.c_uint64)]


class ColumnFilterVarC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("op", C.c_int32), ("combine", C.c_int32),
                ("literal", C.c_void_p), ("literal_len", C.c_uint64), ("selection", C.c_void_p),
                ("selection_capacity", C.c_uint64), ("stage_capacity", C.c_uint64),
                ("rows", C.c_uint64), ("selected", C.c_uint64)]


class ColumnFilterInC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("op", C.c_int32), ("combine", C.c_int32),
                ("values", C.c_void_p), ("value_offsets", C.c_void_p), ("n_values", C.c_uint64),
                ("selection", C.c_void_p), ("selection_capacity", C.c_uint64), ("stage_capacity", C.c_uint64),
                ("rows", C.c_uint64), ("selected", C.c_uint64)]


class ColumnReadSelectedC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("values", C.c_void_p), ("values_capacity", C.c_uint64), ("validity", C.c_void_p),
                ("validity_capacity", C.c_uint64), ("rows", C.c_uint64), ("selected", C.c_uint64),
                ("values_len", C.c_uint64)]


class ColumnReadSelectedVarC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("values", C.c_void_p), ("values_capacity", C.c_uint64), ("validity", C.c_void_p),
                ("validity_capacity", C.c_uint64), ("offsets", C.c_void_p), ("offsets_capacity", C.c_uint64),
                ("stage_capacity", C.c_uint64), ("rows", C.c_uint64), ("selected", C.c_uint64),
                ("values_len", C.c_uint64)]


class ColumnAggregateC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("ops", C.c_uint32), ("reserved", C.c_uint32), ("rows", C.c_uint64), ("selected", C.c_uint64),
                ("count", C.c_uint64), ("nans", C.c_uint64), ("min", C.c_uint8 * 8), ("max", C.c_uint8 * 8),
                ("sum_lo", C.c_uint64), ("sum_hi", C.c_uint64)]


class AggGroupC(C.Structure):
    _fields_ = [("selected", C.c_uint64), ("count", C.c_uint64), ("nans", C.c_uint64), ("min", C.c_uint8 * 8),
                ("max", C.c_uint8 * 8), ("sum_lo", C.c_uint64), ("sum_hi", C.c_uint64), ("reserved", C.c_uint64)]


class ColumnAggregateGroupedC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("group_ids", C.c_void_p), ("group_ids_capacity", C.c_uint64), ("group_id_width", C.c_uint32),
                ("n_groups", C.c_uint32), ("ops", C.c_uint32), ("reserved", C.c_uint32),
                ("groups", C.POINTER(AggGroupC)), ("rows", C.c_uint64), ("selected", C.c_uint64),
                ("out_of_range", C.c_uint64)]


class ColumnAggregateWeightedC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("group_ids", C.c_void_p), ("group_ids_capacity", C.c_uint64), ("group_id_width", C.c_uint32),
                ("n_groups", C.c_uint32), ("ops", C.c_uint32), ("flags", C.c_uint32),
                ("weights", C.c_void_p), ("weights_capacity", C.c_uint64), ("weights_validity", C.c_void_p),
                ("weights_validity_capacity", C.c_uint64), ("weight_type", C.c_int32), ("reserved", C.c_uint32),
                ("groups", C.POINTER(AggGroupC)), ("rows", C.c_uint64), ("selected", C.c_uint64),
                ("out_of_range", C.c_uint64)]


class TopKRowC(C.Structure):
    _fields_ = [("row", C.c_uint64), ("value", C.c_uint8 * 8)]


class ColumnTopKC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("k", C.c_uint32), ("order", C.c_uint32), ("out", C.POINTER(TopKRowC)), ("reserved", C.c_uint64),
                ("rows", C.c_uint64), ("selected", C.c_uint64), ("count", C.c_uint64), ("nans", C.c_uint64),
                ("found", C.c_uint64)]


class ColumnKeyIdsC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("ids", C.c_void_p), ("ids_capacity", C.c_uint64), ("id_width", C.c_uint32), ("max_keys", C.c_uint32),
                ("keys", C.c_void_p), ("reserved", C.c_uint64),
                ("rows", C.c_uint64), ("selected", C.c_uint64), ("count", C.c_uint64), ("n_keys", C.c_uint64),
                ("overflow", C.c_uint64)]


class ColumnKeyIdsVarC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("ids", C.c_void_p), ("ids_capacity", C.c_uint64), ("id_width", C.c_uint32), ("max_keys", C.c_uint32),
                ("key_offsets", C.c_void_p), ("keys", C.c_void_p), ("keys_capacity", C.c_uint64),
                ("stage_capacity", C.c_uint64), ("reserved", C.c_uint64),
                ("rows", C.c_uint64), ("selected", C.c_uint64), ("count", C.c_uint64), ("n_keys", C.c_uint64),
                ("keys_len", C.c_uint64), ("overflow", C.c_uint64)]


class KeyCombineItemC(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("n_parts", C.c_uint32), ("id_width", C.c_uint32),
                ("part_ids", C.c_void_p * 4), ("part_capacity", C.c_uint64 * 4), ("part_width", C.c_uint32 * 4),
                ("part_keys", C.c_uint32 * 4), ("ids", C.c_void_p), ("ids_capacity", C.c_uint64),
                ("max_keys", C.c_uint32), ("reserved", C.c_uint32), ("tuples", C.c_void_p),
                ("live", C.c_uint64), ("n_keys", C.c_uint64), ("overflow", C.c_uint64)]


class ColumnKeyLookupC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("ids", C.c_void_p), ("ids_capacity", C.c_uint64), ("id_width", C.c_uint32), ("reserved0", C.c_uint32),
                ("values", C.c_void_p), ("value_offsets", C.c_void_p), ("value_ids", C.c_void_p),
                ("n_values", C.c_uint64), ("stage_capacity", C.c_uint64), ("reserved", C.c_uint64),
                ("rows", C.c_uint64), ("selected", C.c_uint64), ("count", C.c_uint64), ("matched", C.c_uint64)]


class ColumnKeyBucketsC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("ids", C.c_void_p), ("ids_capacity", C.c_uint64), ("id_width", C.c_uint32), ("flags", C.c_uint32),
                ("bounds", C.c_void_p), ("bucket_ids", C.c_void_p), ("n_bounds", C.c_uint64),
                ("nan_id", C.c_uint32), ("reserved0", C.c_uint32), ("reserved", C.c_uint64),
                ("rows", C.c_uint64), ("selected", C.c_uint64), ("count", C.c_uint64), ("matched", C.c_uint64),
                ("nans", C.c_uint64)]


class ColumnFilterCmpC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("pages", C.c_void_p),
                ("pages_len", C.c_uint64), ("metas", C.POINTER(PageMetaC)), ("n_pages", C.c_uint64),
                ("page_offsets", C.c_void_p), ("op", C.c_int32), ("combine", C.c_int32),
                ("other", C.c_void_p), ("other_capacity", C.c_uint64), ("other_validity", C.c_void_p),
                ("other_validity_capacity", C.c_uint64), ("other_type", C.c_int32), ("flags", C.c_uint32),
                ("reserved", C.c_uint64), ("selection", C.c_void_p), ("selection_capacity", C.c_uint64),
                ("rows", C.c_uint64), ("selected", C.c_uint64)]


class ColumnWriteC(C.Structure):
    _fields_ = [("physical_type", C.c_int32), ("is_nullable", C.c_int32), ("rows", C.c_uint64),
                ("values", C.c_void_p), ("values_bit_offset", C.c_uint64), ("values_len", C.c_uint64),
                ("validity", C.c_void_p), ("validity_bit_offset", C.c_uint64), ("offsets", C.c_void_p),
                ("out_pages", C.c_void_p), ("out_capacity", C.c_uint64), ("out_metas", C.POINTER(PageMetaC)),
                ("n_pages_capacity", C.c_uint64), ("n_pages", C.c_uint64), ("out_len", C.c_uint64),
                ("page_rows", C.c_void_p), ("page_head_bytes", C.c_void_p), ("page_heads", C.c_void_p),
                ("n_pages_in", C.c_uint64), ("first_page_index", C.c_uint64), ("column_values_len", C.c_uint64)]


class NestedLevelC(C.Structure):
    _fields_ = [("validity", C.c_void_p), ("offsets", C.c_void_p), ("validity_bit_offset", C.c_uint64),
                ("length", C.c_uint64), ("kind", C.c_int32), ("is_optional", C.c_int32)]


class NestedPageC(C.Structure):
    _fields_ = [("level_bytes", C.c_uint64), ("num_values", C.c_uint64), ("leaf_start", C.c_uint64),
                ("leaf_count", C.c_uint64)]


class NestedLevelOutC(C.Structure):
    _fields_ = [("offsets", C.c_void_p), ("validity", C.c_void_p), ("offsets_capacity", C.c_uint64),
                ("validity_capacity", C.c_uint64), ("length", C.c_uint64), ("kind", C.c_int32),
                ("is_nullable", C.c_int32)]


class NestedLevelsWriteC(C.Structure):
    _fields_ = [("levels", C.POINTER(NestedLevelC)), ("n_levels", C.c_uint32), ("reserved", C.c_uint32), ("rows", C.c_uint64),
                ("out_levels", C.c_void_p), ("out_capacity", C.c_uint64), ("pages", C.POINTER(NestedPageC)),
                ("n_pages_capacity", C.c_uint64), ("n_pages", C.c_uint64)]


class NestedLevelsReadC(C.Structure):
    _fields_ = [("pages", C.c_void_p), ("pages_len", C.c_uint64), ("metas", C.c_void_p), ("n_pages", C.c_uint64),
                ("levels", C.POINTER(NestedLevelOutC)), ("n_levels", C.c_uint32), ("reserved", C.c_uint32),
                ("leaf_validity", C.c_void_p), ("leaf_validity_capacity", C.c_uint64),
                ("page_leaf_counts", C.c_void_p), ("page_block_offsets", C.c_void_p)]


class PageInfoC(C.Structure):
    _fields_ = [("codec", C.c_int32), ("has_validity_size", C.c_int32), ("validity_size", C.c_uint32),
                ("compressed_size", C.c_uint32), ("uncompressed_size", C.c_uint32), ("unique_num", C.c_uint32),
                ("exceptions_bitmap_size", C.c_uint32), ("has_nested", C.c_int32)]


class SchemaFieldC(C.Structure):
    _fields_ = [("name", C.c_char_p), ("timezone", C.c_char_p), ("type_id", C.c_int32), ("nullable", C.c_int32),
                ("n_children", C.c_int32), ("bit_width", C.c_int32), ("is_signed", C.c_int32), ("precision", C.c_int32),
                ("scale", C.c_int32), ("unit", C.c_int32), ("metadata", C.c_void_p), ("n_metadata", C.c_uint64)]


class KernelStatC(C.Structure):
    _fields_ = [("name", C.c_char_p), ("launches", C.c_uint64), ("total_ms", C.c_double)]


class NativeError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("strawboat-hip error %d: %s" % (code, message))
        self.code = code


_lib = None


def load():
    """Load libstrawboat_hip.so.  torch must be imported first so that one HIP runtime
    (SONAME libamdhip64.so.7) is shared by torch and this library."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(or `make -C strawboat_amd/csrc`)" % LIB_PATH)
    import torch  # noqa: F401  (loads the HIP runtime)
    L = C.CDLL(LIB_PATH)
    L.sb_version.restype = C.c_char_p
    L.sb_ctx_create.restype = C.c_int32
    L.sb_ctx_create.argtypes = [C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    L.sb_ctx_destroy.argtypes = [C.c_void_p]
    L.sb_ctx_synchronize.restype = C.c_int32
    L.sb_ctx_synchronize.argtypes = [C.c_void_p]
    L.sb_ctx_last_error.restype = C.c_char_p
    L.sb_ctx_last_error.argtypes = [C.c_void_p]
    L.sb_ctx_stream.restype = C.c_void_p
    L.sb_ctx_stream.argtypes = [C.c_void_p]
    L.sb_read_columns.restype = C.c_int32
    L.sb_read_columns.argtypes = [C.c_void_p, C.POINTER(ColumnReadC), C.c_uint64, C.c_int32]
    L.sb_filter_columns.restype = C.c_int32
    L.sb_filter_columns.argtypes = [C.c_void_p, C.POINTER(ColumnFilterC), C.c_uint64, C.c_int32]
    L.sb_filter_columns_var.restype = C.c_int32
    L.sb_filter_columns_var.argtypes = [C.c_void_p, C.POINTER(ColumnFilterVarC), C.c_uint64, C.c_int32]
    L.sb_filter_columns_in.restype = C.c_int32
    L.sb_filter_columns_in.argtypes = [C.c_void_p, C.POINTER(ColumnFilterInC), C.c_uint64, C.c_int32]
    L.sb_read_selected.restype = C.c_int32
    L.sb_read_selected.argtypes = [C.c_void_p, C.POINTER(ColumnReadSelectedC), C.c_uint64, C.c_int32]
    L.sb_read_selected_var.restype = C.c_int32
    L.sb_read_selected_var.argtypes = [C.c_void_p, C.POINTER(ColumnReadSelectedVarC), C.c_uint64, C.c_int32]
    L.sb_aggregate_columns.restype = C.c_int32
    L.sb_aggregate_columns.argtypes = [C.c_void_p, C.POINTER(ColumnAggregateC), C.c_uint64, C.c_int32]
    L.sb_aggregate_grouped.restype = C.c_int32
    L.sb_aggregate_grouped.argtypes = [C.c_void_p, C.POINTER(ColumnAggregateGroupedC), C.c_uint64, C.c_int32]
    L.sb_aggregate_grouped_large.restype = C.c_int32
    L.sb_aggregate_grouped_large.argtypes = [C.c_void_p, C.POINTER(ColumnAggregateGroupedC), C.c_uint64, C.c_int32]
    L.sb_key_buckets.restype = C.c_int32
    L.sb_key_buckets.argtypes = [C.c_void_p, C.POINTER(ColumnKeyBucketsC), C.c_uint64, C.c_int32]
    L.sb_filter_columns_cmp.restype = C.c_int32
    L.sb_filter_columns_cmp.argtypes = [C.c_void_p, C.POINTER(ColumnFilterCmpC), C.c_uint64, C.c_int32]
    L.sb_aggregate_weighted.restype = C.c_int32
    L.sb_aggregate_weighted.argtypes = [C.c_void_p, C.POINTER(ColumnAggregateWeightedC), C.c_uint64, C.c_int32]
    L.sb_topk_columns.restype = C.c_int32
    L.sb_topk_columns.argtypes = [C.c_void_p, C.POINTER(ColumnTopKC), C.c_uint64, C.c_int32]
    L.sb_key_ids.restype = C.c_int32
    L.sb_key_ids.argtypes = [C.c_void_p, C.POINTER(ColumnKeyIdsC), C.c_uint64, C.c_int32]
    L.sb_key_ids_var.restype = C.c_int32
    L.sb_key_ids_var.argtypes = [C.c_void_p, C.POINTER(ColumnKeyIdsVarC), C.c_uint64, C.c_int32]
    L.sb_key_combine.restype = C.c_int32
    L.sb_key_combine.argtypes = [C.c_void_p, C.POINTER(KeyCombineItemC), C.c_uint64, C.c_int32]
    L.sb_key_lookup.restype = C.c_int32
    L.sb_key_lookup.argtypes = [C.c_void_p, C.POINTER(ColumnKeyLookupC), C.c_uint64, C.c_int32]
    L.sb_read_columns_sizes.restype = C.c_int32
    L.sb_read_columns_sizes.argtypes = [C.c_void_p, C.POINTER(ColumnReadC), C.c_uint64, C.c_int32]
    L.sb_write_bound.restype = C.c_uint64
    L.sb_write_bound.argtypes = [C.c_int32, C.c_int32, C.c_uint64, C.c_uint64, C.POINTER(WriteOptionsC),
                                 C.POINTER(C.c_uint64)]
    L.sb_write_columns.restype = C.c_int32
    L.sb_write_columns.argtypes = [C.c_void_p, C.POINTER(ColumnWriteC), C.c_uint64, C.POINTER(WriteOptionsC),
                                   C.c_int32]
    L.sb_ctx_profile.restype = C.c_int32
    L.sb_ctx_profile.argtypes = [C.c_void_p, C.c_int32]
    L.sb_ctx_side_forks.restype = C.c_uint64
    L.sb_ctx_side_forks.argtypes = [C.c_void_p]
    L.sb_ctx_replays.restype = C.c_uint64
    L.sb_ctx_replays.argtypes = [C.c_void_p]
    L.sb_ctx_zstd_block_stats.restype = C.c_int32
    L.sb_ctx_zstd_block_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.sb_ctx_profile_read.restype = C.c_uint32
    L.sb_ctx_profile_read.argtypes = [C.c_void_p, C.POINTER(KernelStatC), C.c_uint32]
    L.sb_nested_levels_bound.restype = C.c_uint64
    L.sb_nested_levels_bound.argtypes = [C.POINTER(NestedLevelC), C.c_uint32, C.c_uint64, C.c_uint64]
    L.sb_nested_write_levels.restype = C.c_int32
    L.sb_nested_write_levels.argtypes = [C.c_void_p, C.POINTER(NestedLevelC), C.c_uint32, C.c_uint64, C.c_uint64,
                                         C.c_void_p, C.c_uint64, C.POINTER(NestedPageC), C.c_uint64,
                                         C.POINTER(C.c_uint64)]
    L.sb_nested_read_levels.restype = C.c_int32
    L.sb_nested_read_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(PageMetaC), C.c_uint64,
                                        C.POINTER(NestedLevelOutC), C.c_uint32, C.c_void_p, C.c_uint64,
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.sb_nested_write_levels_batch.restype = C.c_int32
    L.sb_nested_write_levels_batch.argtypes = [C.c_void_p, C.POINTER(NestedLevelsWriteC), C.c_uint64, C.c_uint64]
    L.sb_nested_read_levels_batch.restype = C.c_int32
    L.sb_nested_read_levels_batch.argtypes = [C.c_void_p, C.POINTER(NestedLevelsReadC), C.c_uint64]
    L.sb_nested_write_levels_enqueue.restype = C.c_int32
    L.sb_nested_write_levels_enqueue.argtypes = [C.c_void_p, C.POINTER(NestedLevelsWriteC), C.c_uint64, C.c_uint64]
    L.sb_nested_read_levels_enqueue.restype = C.c_int32
    L.sb_nested_read_levels_enqueue.argtypes = [C.c_void_p, C.POINTER(NestedLevelsReadC), C.c_uint64]
    L.sb_file_last_error.restype = C.c_char_p
    L.sb_file_writer_open.restype = C.c_int32
    L.sb_file_writer_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.sb_file_writer_start.restype = C.c_int32
    L.sb_file_writer_start.argtypes = [C.c_void_p]
    L.sb_file_writer_write_column.restype = C.c_int32
    L.sb_file_writer_write_column.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(PageMetaC), C.c_uint64]
    L.sb_file_writer_finish.restype = C.c_int32
    L.sb_file_writer_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sb_file_writer_close.argtypes = [C.c_void_p]
    L.sb_file_reader_open.restype = C.c_int32
    L.sb_file_reader_open.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
    L.sb_file_reader_n_columns.restype = C.c_uint64
    L.sb_file_reader_n_columns.argtypes = [C.c_void_p]
    L.sb_file_reader_column.restype = C.c_int32
    L.sb_file_reader_column.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                        C.POINTER(C.POINTER(PageMetaC))]
    L.sb_file_reader_schema.restype = C.c_int32
    L.sb_file_reader_schema.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    L.sb_file_reader_read_pages.restype = C.c_int32
    L.sb_file_reader_read_pages.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64,
                                            C.POINTER(C.c_uint64)]
    L.sb_file_reader_close.argtypes = [C.c_void_p]
    L.sb_stat_page.restype = C.c_int32
    L.sb_stat_page.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_int32, C.POINTER(PageInfoC), C.c_uint32,
                               C.POINTER(C.c_uint32)]
    L.sb_schema_last_error.restype = C.c_char_p
    L.sb_schema_to_bytes.restype = C.c_int32
    L.sb_schema_to_bytes.argtypes = [C.POINTER(SchemaFieldC), C.c_uint64, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64,
                                     C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sb_schema_from_bytes.restype = C.c_int32
    L.sb_schema_from_bytes.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(SchemaFieldC), C.c_uint64, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.sb_schema_metadata_from_bytes.restype = C.c_int32
    L.sb_schema_metadata_from_bytes.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                                C.POINTER(C.c_uint64)]
    _lib = L
    return L
