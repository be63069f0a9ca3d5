"""s3imph — Python binding of libs3imph.so, the MI355X-native MPHF builder.

Mirrors the reference's MPHF stage interface, ``format.StreamingMPHFBuilder``
(/root/reference/pkg/format/mphf_streaming.go:29-232):

    b = StreamingMPHFBuilder(temp_dir)       # NewStreamingMPHFBuilder (:48)
    b.add(prefix, pos)                       # Add (:68)
    b.count()                                # Count (:100)
    b.build(out_dir)                         # Build (:122) -> mph.bin, mph_fp.u64, mph_pos.u64,
                                             #                  prefix_blob.bin, prefix_offsets.u64
    b.close()                                # Close (:105)

plus the device-resident API that bench.py times (``DeviceBuilder``), the
multi-GPU rank API (``DistBuilder``), the batched lookup (``MPHF``), the reader,
``Index`` (indexread.Index: Open / Lookup / Stats / Descendants* over a batch), and the front
of the pipeline: ``aggregate`` (extsort.Aggregator + SortPrefixRows: object listing -> prefix
rows) and ``build_index_from_objects`` (object listing -> index directory), both for a
byte-sorted listing; ``sort_objects`` and ``build_index_from_unsorted_objects`` take one in any
order (the stable byte-order sort and the gather run on the GPU too); ``parse_inventory_csv`` and
``build_index_from_inventory_csv`` start from the inventory's CSV text, ``gunzip`` and
``build_index_from_inventory_csv_gz`` from the ``.csv.gz`` files (inflated on the GPU).  With one tier id
per object (``TIERS``, ``tier_from_s3``) both also carry the per-storage-class statistics that
``Index.tier_breakdown*`` answer from, and ``PriceTable`` / ``Index.monthly_cost*`` price them
(pricing.ComputeMonthlyCost per position, on the GPU); ``Index.descendants_top`` keeps the k
largest positions of every descendants row by cost, bytes or object count.

Every compute call goes through the HIP library; there is no CPU fallback.
If libs3imph.so is missing, importing this module raises.
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from dataclasses import dataclass

import numpy as np

try:  # One HIP runtime per process: let torch load its libamdhip64 first.
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is part of the image
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "libs3imph.so")

OK = 0
ERR_INVALID = 1
ERR_DUP_KEY_HASH = 2
ERR_TOO_MANY_LEVELS = 3
ERR_KEY_HASH_ZERO = 4
ERR_HIP = 5
ERR_RCCL = 6
ERR_IO = 7
ERR_NOMEM = 8
ERR_FORMAT = 9
ERR_INTERNAL = 10
ERR_STATE = 11

MULTI_FORCE_SHARDED = 1   # the sharded (multi-GPU) build even for one GPU
MULTI_HOST_TRANSPORT = 2  # in-process host-copy collectives instead of RCCL
MULTI_BITMAP = 4          # the bitmap decomposition of the sharded levels
DIST_ROUTE = 0            # sharded levels: records routed to their position-range owner
DIST_BITMAP = 1           # sharded levels: count-lane reduction of the collision bitmap
DIST_STRICT = 0x100       # or-ed into DIST_BITMAP: no fallback to routing (the build fails instead)

# Every entry point include/s3imph.h declares (checked by tests/test_capi.py).
EXPORTS = (
    "s3imph_abi_version", "s3imph_status_string",
    "s3imph_builder_new", "s3imph_builder_add", "s3imph_builder_add_batch", "s3imph_builder_count",
    "s3imph_builder_build", "s3imph_builder_close", "s3imph_builder_reserve",
    "s3imph_build_host", "s3imph_build_host_multi", "s3imph_builder_set_gpus", "s3imph_free",
    "s3imph_write_index_files",
    "s3imph_ctx_create", "s3imph_ctx_destroy", "s3imph_ctx_reserve", "s3imph_build_device",
    "s3imph_ctx_mph_bin", "s3imph_ctx_set_profiling", "s3imph_ctx_stage_times",
    "s3imph_dist_unique_id", "s3imph_ctx_create_dist", "s3imph_ctx_create_dist_host", "s3imph_build_device_dist",
    "s3imph_dist_segments", "s3imph_dist_out_cap", "s3imph_ctx_last_error", "s3imph_ctx_set_dist_mode",
    "s3imph_ctx_load_mph_bin", "s3imph_lookup_device", "s3imph_gen_keys",
    "s3imph_finalize_index_host", "s3imph_finalize_index_device",
    "s3imph_write_manifest", "s3imph_verify_manifest", "s3imph_sha256_file",
    "s3imph_dev_knobs", "s3imph_build_host_into", "s3imph_mph_bin_bound", "s3imph_release_workspaces",
    "s3imph_index_open", "s3imph_index_attach", "s3imph_index_close", "s3imph_index_count",
    "s3imph_index_max_depth", "s3imph_index_last_error", "s3imph_index_lookup_device",
    "s3imph_index_nodes_device", "s3imph_index_descendants_plan", "s3imph_index_descendants_fill",
    "s3imph_aggregate_plan_device", "s3imph_aggregate_fill_device", "s3imph_aggregate_host",
    "s3imph_index_from_objects_host",
    "s3imph_tier_from_s3", "s3imph_tier_name", "s3imph_tier_file",
    "s3imph_aggregate_plan_tiers_device", "s3imph_aggregate_fill_tiers_device", "s3imph_aggregate_tiers_host",
    "s3imph_index_from_objects_tiers_host", "s3imph_write_tier_files",
    "s3imph_index_attach_tiers", "s3imph_index_tier_count", "s3imph_index_tier_ids", "s3imph_index_tiers_device",
    "s3imph_sort_objects_device", "s3imph_gather_objects_device", "s3imph_sort_objects_host",
    "s3imph_index_from_unsorted_objects_host",
    "s3imph_csv_header_schema", "s3imph_csv_plan_device", "s3imph_csv_fill_device", "s3imph_csv_parse_host",
    "s3imph_index_from_csv_host", "s3imph_csv_geometry",
    "s3imph_price_table_default", "s3imph_price_table_load", "s3imph_price_table_save",
    "s3imph_compute_monthly_cost", "s3imph_index_cost_device", "s3imph_index_descendants_top",
    "s3imph_merge_rows_plan_device", "s3imph_merge_rows_fill_device", "s3imph_merge_geometry",
    "s3imph_merge_rows_host", "s3imph_index_from_rows_host",
    "s3imph_rowset_new", "s3imph_rowset_add_objects", "s3imph_rowset_add_csv", "s3imph_rowset_add_rows",
    "s3imph_rowset_runs", "s3imph_rowset_rows", "s3imph_rowset_build", "s3imph_rowset_close",
    "s3imph_index_open_flags", "s3imph_index_attach_prefixes", "s3imph_index_has_prefixes",
    "s3imph_index_prefixes_plan", "s3imph_index_prefixes_fill", "s3imph_index_lookup_verify_device",
    "s3imph_index_verify_device",
    "s3imph_gunzip_geometry", "s3imph_gunzip_room_hint", "s3imph_gunzip_device", "s3imph_gunzip_host",
    "s3imph_index_from_csv_gz_host", "s3imph_rowset_add_csv_gz",
)
GZ_OK, GZ_MORE, GZ_EOF, GZ_HEADER, GZ_DATA, GZ_CHECKSUM = range(6)  # S3IMPH_GZ_*
OPEN_PREFIXES = 1  # S3IMPH_OPEN_PREFIXES
MERGE_MAX_RUNS = 64  # S3IMPH_MERGE_MAX_RUNS
NUM_TIERS = 12  # S3IMPH_NUM_TIERS


class MPHFError(RuntimeError):
    """A non-OK s3imph_status; ``.status`` holds the code."""

    def __init__(self, status: int, msg: str):
        super().__init__(msg)
        self.status = status


ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64)
ALLTOALLV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                ctypes.POINTER(ctypes.c_uint64))


class HostComm(ctypes.Structure):
    """s3imph_host_comm: host-callback collectives (include/s3imph.h, section 4)."""
    _fields_ = [("user", ctypes.c_void_p), ("allgather", ALLGATHER_FN), ("alltoallv", ALLTOALLV_FN)]


class BuildInfo(ctypes.Structure):
    _fields_ = [
        ("status", ctypes.c_int32),
        ("num_levels", ctypes.c_uint32),
        ("total_words", ctypes.c_uint64),
        ("mph_bin_len", ctypes.c_uint64),
        ("big_levels", ctypes.c_uint64),
        ("n_keys", ctypes.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}


class IndexArrays(ctypes.Structure):
    """s3imph_index_arrays: an index's arrays in HBM (include/s3imph.h, section 5c)."""
    _fields_ = [
        ("mph_bin", ctypes.c_void_p), ("mph_len", ctypes.c_uint64), ("n", ctypes.c_uint64),
        ("d_fp", ctypes.c_void_p), ("d_pos", ctypes.c_void_p),
        ("d_depth", ctypes.c_void_p), ("d_max_depth_in_subtree", ctypes.c_void_p),
        ("d_subtree_end", ctypes.c_void_p), ("d_depth_offsets", ctypes.c_void_p),
        ("d_depth_positions", ctypes.c_void_p), ("max_depth", ctypes.c_uint32),
        ("d_object_count", ctypes.c_void_p), ("d_total_bytes", ctypes.c_void_p),
    ]


class AggInfo(ctypes.Structure):
    """s3imph_agg_info: what an aggregation plan found (include/s3imph.h, section 5d)."""
    _fields_ = [
        ("n_prefixes", ctypes.c_uint64), ("blob_bytes", ctypes.c_uint64), ("n_objects", ctypes.c_uint64),
        ("total_bytes", ctypes.c_uint64), ("first_unsorted", ctypes.c_uint64),
        ("max_depth_seen", ctypes.c_uint32), ("pad", ctypes.c_uint32),
    ]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "pad"}


class AggTierInfo(ctypes.Structure):
    """s3imph_agg_tier_info: what a plan with tiers found (include/s3imph.h, section 5e)."""
    _fields_ = [("present_mask", ctypes.c_uint64), ("first_bad_tier", ctypes.c_uint64)]


class SortInfo(ctypes.Structure):
    """s3imph_sort_info: what a listing sort found (include/s3imph.h, section 5f)."""
    _fields_ = [
        ("n_objects", ctypes.c_uint64), ("key_bytes", ctypes.c_uint64), ("first_unsorted", ctypes.c_uint64),
        ("n_equal", ctypes.c_uint64), ("rounds", ctypes.c_uint32), ("pad", ctypes.c_uint32),
    ]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_ if f != "pad"}


class CsvSchema(ctypes.Structure):
    """s3imph_csv_schema: the columns of an inventory CSV (include/s3imph.h, section 5g)."""
    _fields_ = [("key_col", ctypes.c_int32), ("size_col", ctypes.c_int32), ("storage_col", ctypes.c_int32),
                ("access_tier_col", ctypes.c_int32)]


class CsvInfo(ctypes.Structure):
    """s3imph_csv_info: what a CSV parse found (include/s3imph.h, section 5g)."""
    _fields_ = [
        ("n_records", ctypes.c_uint64), ("n_objects", ctypes.c_uint64), ("key_bytes", ctypes.c_uint64),
        ("n_short", ctypes.c_uint64), ("n_empty_key", ctypes.c_uint64), ("n_bad_size", ctypes.c_uint64),
    ]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}


class GunzipInfo(ctypes.Structure):
    """s3imph_gunzip_info: how one gzip file ended (include/s3imph.h, section 5j)."""
    _fields_ = [
        ("out_bytes", ctypes.c_uint64), ("in_used", ctypes.c_uint64), ("members", ctypes.c_uint32),
        ("status", ctypes.c_uint32), ("crc32", ctypes.c_uint32), ("reserved", ctypes.c_uint32),
    ]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}


class MergeInfo(ctypes.Structure):
    """s3imph_merge_info: what a row merge plan found (include/s3imph.h, section 5i)."""
    _fields_ = [
        ("n_in", ctypes.c_uint64), ("n_out", ctypes.c_uint64), ("blob_bytes", ctypes.c_uint64),
        ("first_unsorted", ctypes.c_uint64), ("present_mask", ctypes.c_uint64),
        ("max_depth_seen", ctypes.c_uint32), ("n_runs", ctypes.c_uint32),
    ]

    def as_dict(self) -> dict:
        return {f: getattr(self, f) for f, _ in self._fields_}


class RowRun(ctypes.Structure):
    """s3imph_row_run: one sorted run of prefix rows in host memory (include/s3imph.h, section 5i)."""
    _fields_ = [
        ("blob", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("depth", ctypes.c_void_p),
        ("count", ctypes.c_void_p), ("bytes", ctypes.c_void_p), ("tier_count", ctypes.c_void_p),
        ("tier_bytes", ctypes.c_void_p), ("n", ctypes.c_uint64), ("tier_stride", ctypes.c_uint64),
    ]


class _PriceTable(ctypes.Structure):
    """s3imph_price_table (include/s3imph.h, section 5h)."""
    _fields_ = [("per_gb_month", ctypes.c_double * 12), ("priced_mask", ctypes.c_uint32), ("pad", ctypes.c_uint32),
                ("monitoring_per_1000_objects", ctypes.c_double), ("standard_price_per_gb", ctypes.c_double)]


# s3imph_cost: what Index.cost_device returns, one record per queried position
COST_DTYPE = np.dtype([("total", "<u8"), ("monitoring", "<u8"), ("min_object_size", "<u8"),
                       ("glacier_overhead", "<u8"), ("per_tier", "<u8", (12,)), ("tier_mask", "<u4"), ("found", "<u4")])
RANK_OBJECT_COUNT = 0
RANK_TOTAL_BYTES = 1
RANK_MONTHLY_COST = 2
_RANK_KEYS = {"count": RANK_OBJECT_COUNT, "object_count": RANK_OBJECT_COUNT, "bytes": RANK_TOTAL_BYTES,
              "total_bytes": RANK_TOTAL_BYTES, "cost": RANK_MONTHLY_COST}

# s3imph_node: what Index.nodes returns, one record per queried position
NODE_DTYPE = np.dtype([("pos", "<u8"), ("subtree_end", "<u8"), ("object_count", "<u8"), ("total_bytes", "<u8"),
                       ("depth", "<u4"), ("max_depth_in_subtree", "<u4"), ("found", "<u4"), ("pad", "<u4")])
DESC_AT = 0    # DescendantsAtDepth[Filtered]: one result row per query
DESC_UPTO = 1  # DescendantsUpToDepth: min(max_rel, maxDepth) result rows per query


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libs3imph.so not built at {LIB_PATH}: run `make -C s3-inv-db_amd` "
                          "(or __graft_entry__.build()); there is no CPU fallback")
    lib = ctypes.CDLL(LIB_PATH)
    u64, i32, vp, cp, sz = ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t
    P = ctypes.POINTER
    sig = {
        "s3imph_abi_version": (i32, []),
        "s3imph_status_string": (cp, [i32]),
        "s3imph_builder_new": (i32, [cp, i32, P(vp), cp, sz]),
        "s3imph_builder_add": (i32, [vp, cp, u64, u64, cp, sz]),
        "s3imph_builder_add_batch": (i32, [vp, vp, vp, vp, u64, cp, sz]),
        "s3imph_builder_count": (u64, [vp]),
        "s3imph_builder_reserve": (i32, [vp, u64, u64, cp, sz]),
        "s3imph_builder_build": (i32, [vp, cp, cp, sz]),
        "s3imph_builder_close": (i32, [vp]),
        "s3imph_build_host": (i32, [i32, vp, vp, vp, u64, vp, vp, P(vp), P(u64), cp, sz]),
        "s3imph_build_host_multi": (i32, [i32, vp, ctypes.c_uint, vp, vp, vp, u64, vp, vp, P(vp), P(u64), cp, sz]),
        "s3imph_builder_set_gpus": (i32, [vp, i32, vp, ctypes.c_uint]),
        "s3imph_free": (None, [vp]),
        "s3imph_write_index_files": (i32, [cp, vp, u64, vp, vp, u64, vp, vp, cp, sz]),
        "s3imph_ctx_create": (i32, [i32, P(vp), cp, sz]),
        "s3imph_ctx_destroy": (i32, [vp]),
        "s3imph_ctx_reserve": (i32, [vp, u64, u64]),
        "s3imph_build_device": (i32, [vp, vp, vp, vp, u64, vp, vp, vp, P(BuildInfo)]),
        "s3imph_ctx_mph_bin": (i32, [vp, vp, u64, P(u64)]),
        "s3imph_ctx_set_profiling": (i32, [vp, i32]),
        "s3imph_ctx_stage_times": (i32, [vp, P(ctypes.c_float), i32, P(i32), cp, sz]),
        "s3imph_dist_unique_id": (i32, [vp]),
        "s3imph_ctx_create_dist": (i32, [i32, vp, i32, i32, P(vp), cp, sz]),
        "s3imph_ctx_create_dist_host": (i32, [i32, P(HostComm), i32, i32, P(vp), cp, sz]),
        "s3imph_build_device_dist": (i32, [vp, vp, vp, vp, u64, u64, vp, vp, u64, P(u64), vp, P(BuildInfo)]),
        "s3imph_dist_segments": (i32, [vp, P(u64), u64, P(u64)]),
        "s3imph_dist_out_cap": (u64, [vp, u64]),
        "s3imph_ctx_set_dist_mode": (i32, [vp, i32]),
        "s3imph_ctx_last_error": (cp, [vp]),
        "s3imph_ctx_load_mph_bin": (i32, [vp, vp, u64]),
        "s3imph_lookup_device": (i32, [vp, vp, vp, u64, vp, vp, u64, vp, vp]),
        "s3imph_finalize_index_host": (i32, [i32, vp, vp, vp, u64, cp, cp, sz]),
        "s3imph_finalize_index_device": (i32, [vp, vp, vp, vp, u64, vp, vp, vp, vp, vp, u64,
                                               P(ctypes.c_uint32), vp]),
        "s3imph_gen_keys": (i32, [i32, u64, ctypes.c_uint32, u64, u64, vp, vp, P(u64)]),
        "s3imph_write_manifest": (i32, [cp, u64, ctypes.c_uint32, cp, sz]),
        "s3imph_verify_manifest": (i32, [cp, cp, sz]),
        "s3imph_sha256_file": (i32, [cp, i32, cp, cp, sz]),
        "s3imph_dev_knobs": (i32, [i32]),
        "s3imph_build_host_into": (i32, [i32, vp, vp, vp, u64, vp, vp, vp, u64, P(u64), cp, sz]),
        "s3imph_mph_bin_bound": (u64, [u64]),
        "s3imph_release_workspaces": (i32, []),
        "s3imph_index_open": (i32, [i32, cp, P(vp), cp, sz]),
        "s3imph_index_attach": (i32, [i32, P(IndexArrays), P(vp), cp, sz]),
        "s3imph_index_close": (i32, [vp]),
        "s3imph_index_count": (u64, [vp]),
        "s3imph_index_max_depth": (u64, [vp]),
        "s3imph_index_last_error": (cp, [vp]),
        "s3imph_index_lookup_device": (i32, [vp, vp, vp, u64, vp, vp]),
        "s3imph_index_nodes_device": (i32, [vp, vp, u64, vp, vp]),
        "s3imph_index_descendants_plan": (i32, [vp, vp, vp, u64, i32, ctypes.c_int32, u64, u64, vp, vp, u64,
                                                P(u64), P(u64), vp]),
        "s3imph_index_descendants_fill": (i32, [vp, vp, u64, vp]),
        "s3imph_aggregate_plan_device": (i32, [vp, vp, vp, vp, u64, ctypes.c_uint32, P(AggInfo), vp]),
        "s3imph_aggregate_fill_device": (i32, [vp, vp, u64, vp, vp, vp, vp, u64, vp]),
        "s3imph_aggregate_host": (i32, [i32, vp, vp, vp, u64, ctypes.c_uint32, P(vp), P(vp), P(vp), P(vp), P(vp),
                                        P(u64), cp, sz]),
        "s3imph_index_from_objects_host": (i32, [i32, vp, vp, vp, u64, ctypes.c_uint32, cp, cp, sz]),
        "s3imph_tier_from_s3": (i32, [cp, cp]),
        "s3imph_tier_name": (cp, [i32]),
        "s3imph_tier_file": (cp, [i32]),
        "s3imph_aggregate_plan_tiers_device": (i32, [vp, vp, vp, vp, vp, u64, ctypes.c_uint32, P(AggInfo),
                                                     P(AggTierInfo), vp]),
        "s3imph_aggregate_fill_tiers_device": (i32, [vp, vp, vp, u64, vp]),
        "s3imph_aggregate_tiers_host": (i32, [i32, vp, vp, vp, vp, u64, ctypes.c_uint32, P(vp), P(vp), P(vp), P(vp),
                                              P(vp), P(vp), P(vp), P(u64), P(u64), cp, sz]),
        "s3imph_index_from_objects_tiers_host": (i32, [i32, vp, vp, vp, vp, u64, ctypes.c_uint32, cp, cp, sz]),
        "s3imph_write_tier_files": (i32, [cp, u64, vp, vp, u64, u64, cp, sz]),
        "s3imph_index_attach_tiers": (i32, [vp, vp, u64, vp, vp, u64]),
        "s3imph_index_tier_count": (u64, [vp]),
        "s3imph_index_tier_ids": (u64, [vp, vp, u64]),
        "s3imph_index_tiers_device": (i32, [vp, vp, u64, vp, vp, vp]),
        "s3imph_sort_objects_device": (i32, [vp, vp, vp, u64, vp, P(SortInfo), vp]),
        "s3imph_gather_objects_device": (i32, [vp, vp, vp, vp, vp, u64, vp, vp, u64, vp, vp, vp, vp]),
        "s3imph_sort_objects_host": (i32, [i32, vp, vp, u64, P(vp), P(SortInfo), cp, sz]),
        "s3imph_index_from_unsorted_objects_host": (i32, [i32, vp, vp, vp, vp, u64, ctypes.c_uint32, cp, cp, sz]),
        "s3imph_csv_header_schema": (i32, [vp, u64, P(CsvSchema), P(u64), cp, sz]),
        "s3imph_csv_plan_device": (i32, [vp, vp, u64, P(CsvSchema), P(CsvInfo), vp]),
        "s3imph_csv_fill_device": (i32, [vp, vp, u64, u64, vp, vp, vp, vp]),
        "s3imph_csv_parse_host": (i32, [i32, vp, u64, P(CsvSchema), P(vp), P(vp), P(vp), P(vp), P(CsvInfo), cp, sz]),
        "s3imph_index_from_csv_host": (i32, [i32, P(vp), P(u64), u64, P(CsvSchema), i32, ctypes.c_uint32, cp,
                                             P(CsvInfo), cp, sz]),
        "s3imph_csv_geometry": (None, [P(ctypes.c_uint32), P(ctypes.c_uint32)]),
        "s3imph_price_table_default": (i32, [P(_PriceTable)]),
        "s3imph_price_table_load": (i32, [cp, P(_PriceTable), cp, sz]),
        "s3imph_price_table_save": (i32, [cp, P(_PriceTable), cp, sz]),
        "s3imph_compute_monthly_cost": (i32, [vp, vp, vp, u64, P(_PriceTable), vp]),
        "s3imph_index_cost_device": (i32, [vp, vp, u64, P(_PriceTable), vp, vp]),
        "s3imph_index_descendants_top": (i32, [vp, i32, P(_PriceTable), ctypes.c_uint32, vp, vp, vp, vp]),
        "s3imph_merge_rows_plan_device": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, u64, vp, ctypes.c_uint32,
                                                P(MergeInfo), vp]),
        "s3imph_merge_rows_fill_device": (i32, [vp, vp, u64, vp, vp, vp, vp, vp, vp, u64, vp]),
        "s3imph_merge_geometry": (None, [P(ctypes.c_uint32)]),
        "s3imph_merge_rows_host": (i32, [i32, P(RowRun), u64, P(vp), P(vp), P(vp), P(vp), P(vp), P(vp), P(vp),
                                         P(u64), P(u64), P(MergeInfo), cp, sz]),
        "s3imph_index_from_rows_host": (i32, [i32, P(RowRun), u64, cp, cp, sz]),
        "s3imph_rowset_new": (i32, [i32, ctypes.c_uint32, i32, P(vp), cp, sz]),
        "s3imph_rowset_add_objects": (i32, [vp, vp, vp, vp, vp, u64, cp, sz]),
        "s3imph_rowset_add_csv": (i32, [vp, P(vp), P(u64), u64, P(CsvSchema), cp, sz]),
        "s3imph_rowset_add_rows": (i32, [vp, P(RowRun), cp, sz]),
        "s3imph_rowset_add_csv_gz": (i32, [vp, P(vp), P(u64), u64, P(CsvSchema), u64, cp, sz]),
        "s3imph_gunzip_geometry": (None, [P(ctypes.c_uint32), P(ctypes.c_uint32), P(ctypes.c_uint32)]),
        "s3imph_gunzip_room_hint": (u64, [vp, u64]),
        "s3imph_gunzip_device": (i32, [vp, vp, P(u64), u64, vp, P(u64), P(GunzipInfo), vp]),
        "s3imph_gunzip_host": (i32, [i32, P(vp), P(u64), u64, P(vp), P(u64), P(GunzipInfo), cp, sz]),
        "s3imph_index_from_csv_gz_host": (i32, [i32, P(vp), P(u64), u64, P(CsvSchema), i32, ctypes.c_uint32, u64, cp,
                                                P(CsvInfo), cp, sz]),
        "s3imph_rowset_runs": (u64, [vp]),
        "s3imph_rowset_rows": (u64, [vp]),
        "s3imph_rowset_build": (i32, [vp, cp, cp, sz]),
        "s3imph_rowset_close": (i32, [vp]),
        "s3imph_index_open_flags": (i32, [i32, cp, ctypes.c_uint, P(vp), cp, sz]),
        "s3imph_index_attach_prefixes": (i32, [vp, vp, vp]),
        "s3imph_index_has_prefixes": (i32, [vp]),
        "s3imph_index_prefixes_plan": (i32, [vp, vp, u64, vp, vp, P(u64), vp]),
        "s3imph_index_prefixes_fill": (i32, [vp, vp, u64, vp]),
        "s3imph_index_lookup_verify_device": (i32, [vp, vp, vp, u64, vp, vp]),
        "s3imph_index_verify_device": (i32, [vp, P(u64), P(u64), P(u64), vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(lib, name)
        f.restype = res
        f.argtypes = args
    return lib


LIB = _load()
# Developer knobs (A/B geometry, test fallbacks, fault hooks: include/s3imph.h section 7) are
# read by the library only after this opt-in; the tests and tools/gpu.sh set S3IMPH_DEV=1.
if os.environ.get("S3IMPH_DEV") == "1":
    LIB.s3imph_dev_knobs(1)


# tiers.AllTiers (pkg/tiers/tiers.go:39-53): (id, name, file prefix), from the library's table
TIERS = tuple((t, LIB.s3imph_tier_name(t).decode(), LIB.s3imph_tier_file(t).decode()) for t in range(NUM_TIERS))


def tier_from_s3(storage_class: str, access_tier: str = "") -> int:
    """Mapping.FromS3 (tiers.go:85-115): an inventory row's StorageClass and
    IntelligentTieringAccessTier -> tier id."""
    return int(LIB.s3imph_tier_from_s3((storage_class or "").encode(), (access_tier or "").encode()))


def _tier_ids(tiers, m: int) -> np.ndarray:
    t = np.ascontiguousarray(tiers, np.uint8)
    if t.shape != (m,):
        raise ValueError("tiers must hold one id per key")
    return t


def write_tier_files(out_dir: str, present_mask: int, tier_count: np.ndarray, tier_bytes: np.ndarray) -> None:
    """s3imph_write_tier_files: tier_stats/ and tiers.json for the tiers of present_mask from
    (NUM_TIERS, n) u64 arrays; nothing for an empty mask."""
    tc = np.ascontiguousarray(tier_count, np.uint64).reshape(NUM_TIERS, -1)
    tb = np.ascontiguousarray(tier_bytes, np.uint64).reshape(NUM_TIERS, -1)
    n = tc.shape[1]
    if tb.shape != tc.shape:
        raise ValueError("tier_count and tier_bytes must have the same shape")
    err = ctypes.create_string_buffer(1024)
    _check(LIB.s3imph_write_tier_files(os.fsencode(out_dir), present_mask, ctypes.c_void_p(tc.ctypes.data),
                                       ctypes.c_void_p(tb.ctypes.data), n, n, err, 1024), err)


def dev_knobs(on: bool = True) -> None:
    """Let the library read its S3IMPH_* developer knobs (tests, A/B runs); not for builds
    that produce an index."""
    LIB.s3imph_dev_knobs(1 if on else 0)


def status_string(code: int) -> str:
    return LIB.s3imph_status_string(code).decode()


def _check(rc: int, err: ctypes.Array | None = None, what: str = ""):
    if rc != OK:
        msg = err.value.decode(errors="replace") if err is not None and err.value else status_string(rc)
        raise MPHFError(rc, f"{what}{': ' if what else ''}{msg}")


def _np_ptr(a: np.ndarray | None):
    if a is None:
        return None
    return ctypes.c_void_p(a.ctypes.data) if a.size else ctypes.c_void_p(0)


def _dev_ptr(t) -> ctypes.c_void_p | None:
    """Device pointer of a torch tensor, an int address, or None."""
    if t is None:
        return None
    if isinstance(t, int):
        return ctypes.c_void_p(t)
    return ctypes.c_void_p(t.data_ptr())


_GO_ESCAPES = {0x07: "\\a", 0x08: "\\b", 0x0c: "\\f", 0x0a: "\\n", 0x0d: "\\r", 0x09: "\\t", 0x0b: "\\v",
               0x22: '\\"', 0x5c: "\\\\"}


def _go_quote(b: bytes) -> str:
    """fmt's %q of a string (strconv.Quote): printable runes as they are, the C escapes, \\x for
    other control characters and for bytes that are not UTF-8, \\u / \\U for the rest."""
    out = []
    for ch in b.decode("utf-8", errors="surrogateescape"):
        c = ord(ch)
        if 0xdc80 <= c <= 0xdcff:  # a byte that was not UTF-8
            out.append("\\x%02x" % (c - 0xdc00))
        elif c in _GO_ESCAPES:
            out.append(_GO_ESCAPES[c])
        elif ch.isprintable():
            out.append(ch)
        elif c < 0x20 or c == 0x7f:
            out.append("\\x%02x" % c)
        else:
            out.append("\\u%04x" % c if c < 0x10000 else "\\U%08x" % c)
    return '"' + "".join(out) + '"'


def keys_to_blob(keys) -> tuple[np.ndarray, np.ndarray]:
    """Keys (bytes/str) -> (blob u8, offsets u64[N+1]): the prefix_blob.bin / prefix_offsets.u64 layout."""
    bs = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
    offs = np.zeros(len(bs) + 1, np.uint64)
    if bs:
        offs[1:] = np.cumsum([len(k) for k in bs], dtype=np.uint64)
    blob = np.frombuffer(b"".join(bs), np.uint8).copy() if bs else np.zeros(0, np.uint8)
    return blob, offs


# ------------------------------------------------------------------------- pricing --
class PriceTable:
    """pricing.PriceTable (pkg/pricing/pricing.go:25-35) keyed by tier id underneath:
    ``per_gb_month`` is a dict by tier name holding the priced tiers, the two scalars are
    ``monitoring_per_1000_objects`` and ``standard_price_per_gb``."""

    def __init__(self, per_gb_month: dict | None = None, monitoring_per_1000_objects: float = 0.0,
                 standard_price_per_gb: float = 0.0):
        self.per_gb_month = dict(per_gb_month or {})
        self.monitoring_per_1000_objects = float(monitoring_per_1000_objects)
        self.standard_price_per_gb = float(standard_price_per_gb)

    @classmethod
    def _from_c(cls, c: "_PriceTable") -> "PriceTable":
        return cls({TIERS[t][1]: c.per_gb_month[t] for t in range(NUM_TIERS) if (c.priced_mask >> t) & 1},
                   c.monitoring_per_1000_objects, c.standard_price_per_gb)

    def _c(self) -> "_PriceTable":
        """The C struct; a name that is none of the twelve tiers is left out, as the loader does."""
        c = _PriceTable()
        ids = {name: t for t, name, _ in TIERS}
        for name, price in self.per_gb_month.items():
            if name in ids:
                c.per_gb_month[ids[name]] = float(price)
                c.priced_mask |= 1 << ids[name]
        c.monitoring_per_1000_objects = self.monitoring_per_1000_objects
        c.standard_price_per_gb = self.standard_price_per_gb
        return c

    @classmethod
    def default_us_east_1(cls) -> "PriceTable":
        """DefaultUSEast1Prices (pricing.go:67-93)."""
        c = _PriceTable()
        _check(LIB.s3imph_price_table_default(ctypes.byref(c)))
        return cls._from_c(c)

    @classmethod
    def load(cls, path: str) -> "PriceTable":
        """LoadPriceTable (pricing.go:96-108)."""
        c = _PriceTable()
        err = ctypes.create_string_buffer(1024)
        _check(LIB.s3imph_price_table_load(os.fsencode(path), ctypes.byref(c), err, 1024), err)
        return cls._from_c(c)

    def save(self, path: str) -> None:
        """SavePriceTable (pricing.go:111-122)."""
        err = ctypes.create_string_buffer(1024)
        _check(LIB.s3imph_price_table_save(os.fsencode(path), ctypes.byref(self._c()), err, 1024), err)

    def __eq__(self, other):
        return isinstance(other, PriceTable) and (self.per_gb_month, self.monitoring_per_1000_objects,
                                                  self.standard_price_per_gb) == (
            other.per_gb_month, other.monitoring_per_1000_objects, other.standard_price_per_gb)

    def __repr__(self):
        return (f"PriceTable({self.per_gb_month!r}, {self.monitoring_per_1000_objects!r}, "
                f"{self.standard_price_per_gb!r})")


def _pt_c(pt) -> "_PriceTable":
    if pt is None:
        pt = PriceTable.default_us_east_1()
    return pt if isinstance(pt, _PriceTable) else pt._c()


def _cost_dict(r) -> dict:
    """One COST_DTYPE record as a dict shaped like pricing.CostResult (per-tier by name, only the
    tier_mask tiers) plus ``found``."""
    return {"found": bool(r["found"]), "total": int(r["total"]), "monitoring": int(r["monitoring"]),
            "min_object_size": int(r["min_object_size"]), "glacier_overhead": int(r["glacier_overhead"]),
            "per_tier": {TIERS[t][1]: int(r["per_tier"][t]) for t in range(NUM_TIERS) if (int(r["tier_mask"]) >> t) & 1}}


def compute_monthly_cost_record(breakdown, pt=None) -> np.ndarray:
    """s3imph_compute_monthly_cost over a breakdown [(tier id, name, bytes, count)] (what
    Index.tier_breakdown[_all] returns per position): one COST_DTYPE record, host only."""
    ids = np.array([e[0] for e in breakdown], np.uint8)
    tb = np.array([e[2] for e in breakdown], np.uint64)
    tc = np.array([e[3] for e in breakdown], np.uint64)
    out = np.zeros(1, COST_DTYPE)
    rc = LIB.s3imph_compute_monthly_cost(_np_ptr(ids), _np_ptr(tc), _np_ptr(tb), len(ids), ctypes.byref(_pt_c(pt)),
                                         ctypes.c_void_p(out.ctypes.data))
    _check(rc, None, "pricing")
    return out[0]


def compute_monthly_cost(breakdown, pt=None) -> dict:
    """pricing.ComputeMonthlyCost (pricing.go:159-240) as a dict; see compute_monthly_cost_record."""
    return _cost_dict(compute_monthly_cost_record(breakdown, pt))


_MIN_SIZE_TIERS = frozenset((1, 2, 3))
_MONITORING_TIERS = frozenset((7, 8, 9, 10, 11))
_GLACIER_TIERS = frozenset((4, 5, 10, 11))


def compute_detailed_breakdown(breakdown, pt=None) -> list:
    """pricing.ComputeDetailedBreakdown (pricing.go:256-312): one dict of dollars per priced tier
    of the breakdown.  A display helper, in Python floats."""
    pt = PriceTable.default_us_east_1() if pt is None else pt
    ids = {name: t for t, name, _ in TIERS}
    out = []
    for tier, name, nbytes, count in breakdown:
        if name not in pt.per_gb_month or name not in ids:
            continue
        price = float(pt.per_gb_month[name])
        avg = nbytes // count if count else 0
        cb = {"tier_name": name, "object_count": count, "bytes": nbytes, "avg_object_size_bytes": avg,
              "storage_cost": nbytes / 1073741824.0 * price, "min_size_penalty": 0.0, "monitoring_cost": 0.0,
              "glacier_overhead": 0.0}
        if tier in _MIN_SIZE_TIERS and 0 < avg < 131072:
            cb["min_size_penalty"] = (((131072 - avg) * count) & ((1 << 64) - 1)) / 1073741824.0 * price
        if tier in _MONITORING_TIERS and pt.monitoring_per_1000_objects > 0:
            mon = count if avg >= 131072 else (count // 2 if avg > 0 else 0)
            cb["monitoring_cost"] = mon / 1000.0 * pt.monitoring_per_1000_objects
        if tier in _GLACIER_TIERS and count > 0:
            cb["glacier_overhead"] = ((count * 32768) & ((1 << 64) - 1)) / 1073741824.0 * price
            cb["glacier_overhead"] += ((count * 8192) & ((1 << 64) - 1)) / 1073741824.0 * pt.standard_price_per_gb
        cb["total_cost"] = cb["storage_cost"] + cb["min_size_penalty"] + cb["monitoring_cost"] + cb["glacier_overhead"]
        out.append(cb)
    return out


def format_cost_dollars(dollars: float) -> str:
    """pricing.FormatCostDollars (pricing.go:320-331)."""
    if dollars < 0.01:
        return "$%.6f" % dollars
    if dollars < 1:
        return "$%.4f" % dollars
    if dollars < 100:
        return "$%.2f" % dollars
    return "$%.0f" % dollars


def format_cost(microdollars: int) -> str:
    """pricing.FormatCost (pricing.go:315-317)."""
    return format_cost_dollars(float(microdollars) / 1_000_000)


# ------------------------------------------------------------------- builder mirror --
class StreamingMPHFBuilder:
    """format.StreamingMPHFBuilder (mphf_streaming.go:29-232) backed by the GPU build."""

    def __init__(self, temp_dir: str | None = None, device: int = 0):
        err = ctypes.create_string_buffer(512)
        h = ctypes.c_void_p()
        rc = LIB.s3imph_builder_new((temp_dir or "").encode(), device, ctypes.byref(h), err, 512)
        _check(rc, err, "create temp file" if rc == ERR_IO else "")
        self._h = h

    def add(self, prefix, pos: int) -> None:
        b = prefix.encode() if isinstance(prefix, str) else bytes(prefix)
        err = ctypes.create_string_buffer(256)
        _check(LIB.s3imph_builder_add(self._h, b, len(b), pos, err, 256), err)

    def add_batch(self, blob: np.ndarray, offsets: np.ndarray, pos: np.ndarray | None = None) -> None:
        blob = np.ascontiguousarray(blob, np.uint8)
        offsets = np.ascontiguousarray(offsets, np.uint64)
        if pos is not None:
            pos = np.ascontiguousarray(pos, np.uint64)
        err = ctypes.create_string_buffer(256)
        _check(LIB.s3imph_builder_add_batch(self._h, _np_ptr(blob), _np_ptr(offsets), _np_ptr(pos),
                                            len(offsets) - 1, err, 256), err)

    def count(self) -> int:
        return LIB.s3imph_builder_count(self._h)

    def reserve(self, n_keys: int, n_bytes: int) -> None:
        """Capacity hint: the device copy of the keys is allocated once (s3imph_builder_reserve)."""
        err = ctypes.create_string_buffer(256)
        _check(LIB.s3imph_builder_reserve(self._h, n_keys, n_bytes, err, 256), err)

    def set_gpus(self, num_gpus: int, devices=None, flags: int = 0) -> None:
        """Build on `num_gpus` GPUs (s3imph_builder_set_gpus; see build_host)."""
        devs = None if devices is None else (ctypes.c_int * num_gpus)(*devices)
        _check(LIB.s3imph_builder_set_gpus(self._h, num_gpus, devs, flags), None, "set_gpus")

    def build(self, out_dir: str) -> None:
        err = ctypes.create_string_buffer(1024)
        _check(LIB.s3imph_builder_build(self._h, out_dir.encode(), err, 1024), err)

    def close(self) -> None:
        if self._h:
            LIB.s3imph_builder_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def release_workspaces() -> None:
    """Free the device workspaces cached by the host-memory builds (s3imph_release_workspaces)."""
    _check(LIB.s3imph_release_workspaces(), None, "release_workspaces")


def mph_bin_bound(n: int) -> int:
    """An upper bound on mph.bin's size for n keys (the buffer of build_host_into)."""
    return int(LIB.s3imph_mph_bin_bound(n))


def build_host_into(blob: np.ndarray, offsets: np.ndarray, out: tuple[np.ndarray, np.ndarray],
                    mph_buf: np.ndarray, pos: np.ndarray | None = None, device: int = 0) -> int:
    """s3imph_build_host_into: the one-shot host build into caller-owned, reusable outputs —
    fp / pos arrays (u64, N each) and mph_buf (u8, >= mph_bin_bound(N)); returns mph.bin's
    length (mph_buf[:len] holds it)."""
    blob = np.ascontiguousarray(blob, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    if pos is not None:
        pos = np.ascontiguousarray(pos, np.uint64)
    fp_out, pos_out = out
    for a in (fp_out, pos_out):
        if a.dtype != np.uint64 or len(a) < n or not a.flags.c_contiguous:
            raise ValueError("out arrays must be contiguous uint64 with at least N entries")
    if mph_buf.dtype != np.uint8 or not mph_buf.flags.c_contiguous:
        raise ValueError("mph_buf must be a contiguous uint8 array")
    ml = ctypes.c_uint64()
    err = ctypes.create_string_buffer(1024)
    rc = LIB.s3imph_build_host_into(device, _np_ptr(blob), _np_ptr(offsets), _np_ptr(pos), n, _np_ptr(fp_out),
                                    _np_ptr(pos_out), _np_ptr(mph_buf), len(mph_buf), ctypes.byref(ml), err, 1024)
    _check(rc, err)
    return int(ml.value)


def build_host(blob: np.ndarray, offsets: np.ndarray, pos: np.ndarray | None = None, device: int = 0,
               out: tuple[np.ndarray, np.ndarray] | None = None, num_gpus: int = 1, devices=None, flags: int = 0):
    """One-shot build from host memory: (fp_out u64[N], pos_out u64[N], mph_bin bytes).
    `out` may supply the two output arrays (u64, N each) to be filled in place.
    num_gpus > 1 (or `devices`, or `flags`) runs s3imph_build_host_multi: one host thread
    per GPU, RCCL between them (or in-process host copies when devices repeat or flags
    has MULTI_HOST_TRANSPORT)."""
    blob = np.ascontiguousarray(blob, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    n = len(offsets) - 1
    if pos is not None:
        pos = np.ascontiguousarray(pos, np.uint64)
    if out is not None:
        fp_out, pos_out = out
        if fp_out.dtype != np.uint64 or pos_out.dtype != np.uint64 or len(fp_out) < n or len(pos_out) < n \
                or not fp_out.flags.c_contiguous or not pos_out.flags.c_contiguous:
            raise ValueError("out arrays must be contiguous uint64 with at least N entries")
    else:
        fp_out = np.zeros(n, np.uint64)
        pos_out = np.zeros(n, np.uint64)
    mp = ctypes.c_void_p()
    ml = ctypes.c_uint64()
    err = ctypes.create_string_buffer(1024)
    if num_gpus == 1 and devices is None and not flags:
        rc = LIB.s3imph_build_host(device, _np_ptr(blob), _np_ptr(offsets), _np_ptr(pos), n, _np_ptr(fp_out),
                                   _np_ptr(pos_out), ctypes.byref(mp), ctypes.byref(ml), err, 1024)
    else:
        if devices is not None:
            num_gpus = len(devices)
        devs = None if devices is None else (ctypes.c_int * num_gpus)(*devices)
        rc = LIB.s3imph_build_host_multi(num_gpus, devs, flags, _np_ptr(blob), _np_ptr(offsets), _np_ptr(pos), n,
                                         _np_ptr(fp_out), _np_ptr(pos_out), ctypes.byref(mp), ctypes.byref(ml), err,
                                         1024)
    _check(rc, err)
    mph = ctypes.string_at(mp.value, ml.value) if ml.value else b""
    if mp.value:
        LIB.s3imph_free(mp)
    return fp_out, pos_out, mph


def write_index_files(out_dir: str, mph_bin: bytes, fp: np.ndarray, pos: np.ndarray, blob: np.ndarray,
                      offsets: np.ndarray) -> None:
    """Emit mph.bin, mph_fp.u64, mph_pos.u64, prefix_blob.bin, prefix_offsets.u64 (reference framing)."""
    fp = np.ascontiguousarray(fp, np.uint64)
    pos = np.ascontiguousarray(pos, np.uint64)
    blob = np.ascontiguousarray(blob, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    err = ctypes.create_string_buffer(1024)
    rc = LIB.s3imph_write_index_files(out_dir.encode(), mph_bin, len(mph_bin), _np_ptr(fp), _np_ptr(pos),
                                      len(fp), _np_ptr(blob), _np_ptr(offsets), err, 1024)
    _check(rc, err)


def gen_keys(kind: int, seed: int, avg_len: int, lo: int, n: int) -> tuple[np.ndarray, np.ndarray]:
    """Deterministic synthetic prefixes [lo, lo+n) (see include/s3imph.h §6). Blob is padded to 8 bytes."""
    total = ctypes.c_uint64()
    _check(LIB.s3imph_gen_keys(kind, seed, avg_len, lo, n, None, None, ctypes.byref(total)))
    blob = np.zeros(((total.value + 7) // 8) * 8 + 8, np.uint8)
    offsets = np.zeros(n + 1, np.uint64)
    _check(LIB.s3imph_gen_keys(kind, seed, avg_len, lo, n, _np_ptr(blob), _np_ptr(offsets), ctypes.byref(total)))
    return blob, offsets


# ----------------------------------------------------------------- device builders --
class DeviceBuilder:
    """A device context: device-resident builds, mph.bin marshalling, batched lookup."""

    def __init__(self, device: int = 0):
        err = ctypes.create_string_buffer(512)
        h = ctypes.c_void_p()
        _check(LIB.s3imph_ctx_create(device, ctypes.byref(h), err, 512), err)
        self._h = h
        self.device = device
        self.last_info: dict | None = None

    def reserve(self, max_keys: int, max_global_keys: int = 0) -> None:
        _check(LIB.s3imph_ctx_reserve(self._h, max_keys, max_global_keys), None, "reserve")

    def set_profiling(self, on) -> None:
        """False/0 off, True/1 every stage, 2 the level-0 hash (or route) stage only."""
        LIB.s3imph_ctx_set_profiling(self._h, int(on))

    def stage_times(self) -> dict:
        ms = (ctypes.c_float * 64)()
        cnt = ctypes.c_int()
        names = ctypes.create_string_buffer(2048)
        LIB.s3imph_ctx_stage_times(self._h, ms, 64, ctypes.byref(cnt), names, 2048)
        keys = names.value.decode().split(",") if cnt.value else []
        return {k: ms[i] for i, k in enumerate(keys)}

    def last_error(self) -> str:
        return LIB.s3imph_ctx_last_error(self._h).decode(errors="replace")

    def build(self, d_blob, d_offsets, n: int, d_fp_out, d_pos_out, d_pos=None, stream=None) -> dict:
        info = BuildInfo()
        rc = LIB.s3imph_build_device(self._h, _dev_ptr(d_blob), _dev_ptr(d_offsets), _dev_ptr(d_pos), n,
                                     _dev_ptr(d_fp_out), _dev_ptr(d_pos_out), _stream_ptr(stream),
                                     ctypes.byref(info))
        if rc != OK:
            raise MPHFError(rc, f"build MPHF: {self.last_error() or status_string(rc)}")
        self.last_info = info.as_dict()
        return self.last_info

    def mph_bin(self) -> bytes:
        ln = ctypes.c_uint64()
        LIB.s3imph_ctx_mph_bin(self._h, None, 0, ctypes.byref(ln))
        buf = ctypes.create_string_buffer(max(ln.value, 1))
        _check(LIB.s3imph_ctx_mph_bin(self._h, buf, ln.value, ctypes.byref(ln)), None, "marshal MPHF")
        return buf.raw[: ln.value]

    def load_mph_bin(self, mph: bytes) -> None:
        """OpenMPHF (mphf.go:186-247): this context's lookups now answer against `mph`."""
        rc = LIB.s3imph_ctx_load_mph_bin(self._h, mph if mph else None, len(mph))
        if rc != OK:
            raise MPHFError(rc, f"open MPHF: {self.last_error() or status_string(rc)}")

    def lookup(self, d_blob, d_offsets, n: int, d_fp, d_pos, count: int, d_result, stream=None) -> None:
        _check(LIB.s3imph_lookup_device(self._h, _dev_ptr(d_blob), _dev_ptr(d_offsets), n, _dev_ptr(d_fp),
                                        _dev_ptr(d_pos), count, _dev_ptr(d_result), _stream_ptr(stream)),
               None, "lookup")

    def finalize_index(self, d_blob, d_offsets, n: int, d_depths=None, stream=None) -> dict:
        """IndexBuilder.Finalize's arrays on the device (indexbuild.go:393-415,474-503,
        depthindex.go:32-96): torch tensors depth (int32), subtree_end (int64),
        max_depth_in_subtree (int32), depth_positions (int64), depth_offsets (int64), max_depth."""
        import torch
        dev = d_offsets.device
        depth = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        send = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        mds = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        dpos = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        md = ctypes.c_uint32()
        cap = 64
        for _ in range(2):
            doff = torch.empty(cap, dtype=torch.int64, device=dev)
            rc = LIB.s3imph_finalize_index_device(self._h, _dev_ptr(d_blob), _dev_ptr(d_offsets), _dev_ptr(d_depths),
                                                  n, _dev_ptr(depth), _dev_ptr(send), _dev_ptr(mds), _dev_ptr(dpos),
                                                  _dev_ptr(doff), cap, ctypes.byref(md), _stream_ptr(stream))
            if rc == OK:
                break
            if rc != ERR_INVALID or cap >= md.value + 2:
                raise MPHFError(rc, f"finalize index: {self.last_error() or status_string(rc)}")
            cap = md.value + 2
        return {"depth": depth[:n], "subtree_end": send[:n], "max_depth_in_subtree": mds[:n],
                "depth_positions": dpos[:n], "depth_offsets": doff[: md.value + 2], "max_depth": md.value}

    def aggregate_plan(self, d_keys, d_key_offsets, m: int, d_sizes=None, max_depth: int = 0, stream=None,
                       tiers=None) -> dict:
        """s3imph_aggregate_plan_device: size the prefix rows of a byte-sorted object listing in
        HBM (AddObject over every key, aggregator.go:44-61).  Returns s3imph_agg_info as a dict
        (n_prefixes, blob_bytes, n_objects, total_bytes, first_unsorted, max_depth_seen); a
        refusal raises MPHFError with that dict as ``.info``.  The key tensors must stay valid
        and unchanged until aggregate_fill.  With ``tiers`` (a uint8 device tensor, one tier id per
        key) it is s3imph_aggregate_plan_tiers_device: the dict gains present_mask and
        first_bad_tier, and tiers / d_sizes must stay valid until aggregate_fill_tiers."""
        info = AggInfo()
        if tiers is None:
            rc = LIB.s3imph_aggregate_plan_device(self._h, _dev_ptr(d_keys), _dev_ptr(d_key_offsets),
                                                  _dev_ptr(d_sizes), m, max_depth, ctypes.byref(info),
                                                  _stream_ptr(stream))
            self.last_agg = info.as_dict()
        else:
            tinfo = AggTierInfo()
            rc = LIB.s3imph_aggregate_plan_tiers_device(self._h, _dev_ptr(d_keys), _dev_ptr(d_key_offsets),
                                                        _dev_ptr(d_sizes), _dev_ptr(tiers), m, max_depth,
                                                        ctypes.byref(info), ctypes.byref(tinfo), _stream_ptr(stream))
            self.last_agg = info.as_dict()
            self.last_agg["present_mask"] = int(tinfo.present_mask)
            self.last_agg["first_bad_tier"] = int(tinfo.first_bad_tier)
        if rc != OK:
            e = MPHFError(rc, self.last_error() or f"aggregate: {status_string(rc)}")
            e.info = self.last_agg
            raise e
        return self.last_agg

    def aggregate_fill(self, n_cap: int | None = None, blob_cap: int | None = None, device=None, stream=None) -> dict:
        """s3imph_aggregate_fill_device: the rows of the last plan (Drain + SortPrefixRows) as
        torch tensors: blob (uint8, padded with zeros to 8 bytes), offsets (int64, n + 1), depth
        (int32), object_count / total_bytes (int64 holding the u64 bits), n, blob_bytes.  The
        capacities default to what the plan asked for."""
        import torch
        info = getattr(self, "last_agg", None) or {"n_prefixes": 0, "blob_bytes": 0}
        n, nbytes = info["n_prefixes"], info["blob_bytes"]
        n_cap = n if n_cap is None else n_cap
        blob_cap = (nbytes + 7) // 8 * 8 if blob_cap is None else blob_cap
        dev = f"cuda:{self.device}" if device is None else device
        blob = torch.empty(max(blob_cap, 8), dtype=torch.uint8, device=dev)
        offs = torch.empty(max(n_cap, n) + 1, dtype=torch.int64, device=dev)
        depth = torch.empty(max(n_cap, 1), dtype=torch.int32, device=dev)
        ocnt = torch.empty(max(n_cap, 1), dtype=torch.int64, device=dev)
        tbytes = torch.empty(max(n_cap, 1), dtype=torch.int64, device=dev)
        rc = LIB.s3imph_aggregate_fill_device(self._h, _dev_ptr(blob), blob_cap, _dev_ptr(offs), _dev_ptr(depth),
                                              _dev_ptr(ocnt), _dev_ptr(tbytes), n_cap, _stream_ptr(stream))
        if rc != OK:
            raise MPHFError(rc, self.last_error() or f"aggregate: {status_string(rc)}")
        return {"blob": blob[: (nbytes + 7) // 8 * 8], "offsets": offs[: n + 1], "depth": depth[:n],
                "object_count": ocnt[:n], "total_bytes": tbytes[:n], "n": n, "blob_bytes": nbytes}

    def aggregate_fill_tiers(self, n_cap: int | None = None, device=None, stream=None) -> dict:
        """s3imph_aggregate_fill_tiers_device: the tier columns of the last plan's rows, after
        aggregate_fill: tier_count / tier_bytes as (NUM_TIERS, n_cap) int64 tensors holding the
        u64 bits (row t = TierCounts[t] / TierBytes[t] of every prefix row; [:, :n] is valid),
        n, present_mask."""
        import torch
        info = getattr(self, "last_agg", None) or {"n_prefixes": 0}
        n = info["n_prefixes"]
        n_cap = n if n_cap is None else n_cap
        dev = f"cuda:{self.device}" if device is None else device
        tc = torch.empty((NUM_TIERS, max(n_cap, 1)), dtype=torch.int64, device=dev)
        tb = torch.empty((NUM_TIERS, max(n_cap, 1)), dtype=torch.int64, device=dev)
        # the column stride is the tensors' row length (n_cap, or 1 for an empty result)
        rc = LIB.s3imph_aggregate_fill_tiers_device(self._h, _dev_ptr(tc), _dev_ptr(tb), n_cap if n_cap else 0,
                                                    _stream_ptr(stream))
        if rc != OK:
            raise MPHFError(rc, self.last_error() or f"aggregate: {status_string(rc)}")
        return {"tier_count": tc, "tier_bytes": tb, "n": n, "present_mask": info.get("present_mask", 0)}

    def sort_objects(self, d_keys, d_key_offsets, m: int, stream=None):
        """s3imph_sort_objects_device: the byte order of an object listing in HBM, in any order
        (what SortPrefixRows' comparison gives, types.go:160-164; stable).  Returns (order, info):
        order an int32 tensor holding the u32 bits, order[j] = the input index of the j-th key in
        sorted order; info s3imph_sort_info as a dict (n_objects, key_bytes, first_unsorted,
        n_equal, rounds).  A refusal raises MPHFError with that dict as ``.info``."""
        import torch
        dev = f"cuda:{self.device}" if d_key_offsets is None else d_key_offsets.device
        order = torch.empty(max(m, 1), dtype=torch.int32, device=dev)
        info = SortInfo()
        rc = LIB.s3imph_sort_objects_device(self._h, _dev_ptr(d_keys), _dev_ptr(d_key_offsets), m, _dev_ptr(order),
                                            ctypes.byref(info), _stream_ptr(stream))
        self.last_sort = info.as_dict()
        if rc != OK:
            e = MPHFError(rc, self.last_error() or f"sort: {status_string(rc)}")
            e.info = self.last_sort
            raise e
        return order[:m], self.last_sort

    def gather_objects(self, d_keys, d_key_offsets, m: int, d_order, d_sizes=None, d_tiers=None,
                       keys_cap: int | None = None, stream=None) -> dict:
        """s3imph_gather_objects_device: the listing put into the order d_order, out of place, as
        torch tensors: keys (uint8, padded with zeros to 8 bytes), offsets (int64, m + 1, starting
        at 0), sizes (int64 holding the u64 bits, or None without d_sizes), tiers (uint8, or None
        without d_tiers), key_bytes.  keys_cap defaults to what the listing needs."""
        import torch
        dev = f"cuda:{self.device}" if d_key_offsets is None else d_key_offsets.device
        with _torch_on(stream, dev):  # the read-back waits for the stream that produces the offsets
            nbytes = int(d_key_offsets[m] - d_key_offsets[0]) if m else 0
        keys_cap = (nbytes + 7) // 8 * 8 if keys_cap is None else keys_cap
        keys = torch.empty(max(keys_cap, 8), dtype=torch.uint8, device=dev)
        offs = torch.empty(m + 1, dtype=torch.int64, device=dev)
        sizes = None if d_sizes is None else torch.empty(max(m, 1), dtype=torch.int64, device=dev)
        tiers = None if d_tiers is None else torch.empty(max(m, 1), dtype=torch.uint8, device=dev)
        rc = LIB.s3imph_gather_objects_device(self._h, _dev_ptr(d_keys), _dev_ptr(d_key_offsets), _dev_ptr(d_sizes),
                                              _dev_ptr(d_tiers), m, _dev_ptr(d_order), _dev_ptr(keys), keys_cap,
                                              _dev_ptr(offs), _dev_ptr(sizes), _dev_ptr(tiers), _stream_ptr(stream))
        if rc != OK:
            raise MPHFError(rc, self.last_error() or f"sort: {status_string(rc)}")
        return {"keys": keys[: (nbytes + 7) // 8 * 8], "offsets": offs, "sizes": None if sizes is None else sizes[:m],
                "tiers": None if tiers is None else tiers[:m], "key_bytes": nbytes}

    def csv_plan(self, d_csv, length: int, schema, stream=None) -> dict:
        """s3imph_csv_plan_device: every pass that sizes the listing of one inventory CSV buffer in
        HBM (d_csv: a uint8 tensor or an address, any alignment, readable to round_up(length, 8)).
        schema = (key_col, size_col, storage_col, access_tier_col).  Returns s3imph_csv_info as a
        dict and keeps the plan for csv_fill."""
        info = CsvInfo()
        rc = LIB.s3imph_csv_plan_device(self._h, _dev_ptr(d_csv), length, ctypes.byref(_csv_schema(schema)),
                                        ctypes.byref(info), _stream_ptr(stream))
        self.last_csv = info.as_dict()
        if rc != OK:
            e = MPHFError(rc, self.last_error() or f"csv: {status_string(rc)}")
            e.info = self.last_csv
            raise e
        return self.last_csv

    def csv_fill(self, d_keys=None, d_key_offsets=None, d_sizes=None, d_tiers=None, key_base: int = 0,
                 keys_cap: int | None = None, with_tiers: bool = True, stream=None) -> dict:
        """s3imph_csv_fill_device: the last csv_plan's listing as torch tensors: keys (uint8),
        offsets (int64, n_objects + 1, starting at key_base), sizes (int64 holding the u64 bits),
        tiers (uint8, or None without with_tiers).  Without arguments the arrays are made here, the
        keys padded to 8 bytes; given arrays are written in place (key_base: where the keys start in
        d_keys; keys_cap defaults to its length), so file after file appends into one listing."""
        import torch
        info = getattr(self, "last_csv", None) or {"n_objects": 0, "key_bytes": 0}
        n, end = info["n_objects"], key_base + info["key_bytes"]
        dev = f"cuda:{self.device}"
        keys = torch.empty(max((end + 7) // 8 * 8, 8), dtype=torch.uint8, device=dev) if d_keys is None else d_keys
        if keys_cap is None:
            keys_cap = (end + 7) // 8 * 8 if d_keys is None else int(d_keys.numel())
        offs = torch.empty(n + 1, dtype=torch.int64, device=dev) if d_key_offsets is None else d_key_offsets
        sizes = torch.empty(max(n, 1), dtype=torch.int64, device=dev) if d_sizes is None else d_sizes
        tiers = d_tiers
        if tiers is None and with_tiers:
            tiers = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        rc = LIB.s3imph_csv_fill_device(self._h, _dev_ptr(keys), keys_cap, key_base, _dev_ptr(offs), _dev_ptr(sizes),
                                        _dev_ptr(tiers), _stream_ptr(stream))
        if rc != OK:
            raise MPHFError(rc, self.last_error() or f"csv: {status_string(rc)}")
        return {"keys": keys[: (end + 7) // 8 * 8] if d_keys is None else keys, "offsets": offs[: n + 1],
                "sizes": sizes[:n], "tiers": None if tiers is None else tiers[:n], "key_bytes": info["key_bytes"]}

    def gunzip(self, d_gz, gz_offsets, d_out, out_offsets, stream=None) -> list:
        """s3imph_gunzip_device: gzip files in HBM inflated in one launch.  File i is
        d_gz[gz_offsets[i]:gz_offsets[i + 1]] (a uint8 tensor or an address, any alignment) and
        may write only d_out[out_offsets[i]:out_offsets[i + 1]]; the offsets are host sequences of
        n + 1 entries.  Returns one s3imph_gunzip_info dict per file; "status" is a GZ_* value."""
        n = len(gz_offsets) - 1
        if n != len(out_offsets) - 1 or n < 0:
            raise MPHFError(ERR_INVALID, "gzip: gz_offsets and out_offsets need n + 1 entries each")
        go = (ctypes.c_uint64 * (n + 1))(*[int(v) for v in gz_offsets])
        oo = (ctypes.c_uint64 * (n + 1))(*[int(v) for v in out_offsets])
        info = (GunzipInfo * max(n, 1))()
        rc = LIB.s3imph_gunzip_device(self._h, _dev_ptr(d_gz), go, n, _dev_ptr(d_out), oo, info, _stream_ptr(stream))
        if rc != OK:
            raise MPHFError(rc, self.last_error() or f"gzip: {status_string(rc)}")
        return [info[i].as_dict() for i in range(n)]

    def merge_rows_plan(self, d_blob, d_offsets, d_depth, d_count, d_bytes, run_starts, d_tier_count=None,
                        d_tier_bytes=None, tier_stride: int = 0, stream=None) -> dict:
        """s3imph_merge_rows_plan_device: MergeIterator (merger.go:104-140) over one row set in HBM
        sorted in K stretches; run_starts is a HOST sequence of K + 1 row indices.  Returns
        s3imph_merge_info as a dict (n_in, n_out, blob_bytes, first_unsorted, present_mask,
        max_depth_seen, n_runs); a refusal raises MPHFError with that dict as ``.info``.  The input
        tensors must stay valid and unchanged until merge_rows_fill."""
        rs = np.ascontiguousarray(run_starts, np.uint64)
        info = MergeInfo()
        rc = LIB.s3imph_merge_rows_plan_device(self._h, _dev_ptr(d_blob), _dev_ptr(d_offsets), _dev_ptr(d_depth),
                                               _dev_ptr(d_count), _dev_ptr(d_bytes), _dev_ptr(d_tier_count),
                                               _dev_ptr(d_tier_bytes), tier_stride,
                                               ctypes.c_void_p(rs.ctypes.data) if rs.size else None,
                                               max(len(rs) - 1, 0), ctypes.byref(info), _stream_ptr(stream))
        self.last_merge = info.as_dict()
        self.last_merge["tiered"] = d_tier_count is not None
        if rc != OK:
            e = MPHFError(rc, self.last_error() or f"merge: {status_string(rc)}")
            e.info = self.last_merge
            raise e
        return self.last_merge

    def merge_rows_fill(self, n_cap: int | None = None, blob_cap: int | None = None, device=None, stream=None) -> dict:
        """s3imph_merge_rows_fill_device: the merged rows of the last plan as torch tensors: blob
        (uint8, padded with zeros to 8 bytes), offsets (int64, n + 1), depth (int32), object_count /
        total_bytes (int64 holding the u64 bits), and after a plan with tier columns tier_count /
        tier_bytes as (NUM_TIERS, n_cap) int64 tensors (else None), n, blob_bytes, present_mask."""
        import torch
        info = getattr(self, "last_merge", None) or {"n_out": 0, "blob_bytes": 0, "tiered": False, "present_mask": 0}
        n, nbytes = info["n_out"], info["blob_bytes"]
        n_cap = n if n_cap is None else n_cap
        blob_cap = (nbytes + 7) // 8 * 8 if blob_cap is None else blob_cap
        dev = f"cuda:{self.device}" if device is None else device
        blob = torch.empty(max(blob_cap, 8), dtype=torch.uint8, device=dev)
        offs = torch.empty(max(n_cap, n) + 1, dtype=torch.int64, device=dev)
        depth = torch.empty(max(n_cap, 1), dtype=torch.int32, device=dev)
        ocnt = torch.empty(max(n_cap, 1), dtype=torch.int64, device=dev)
        tbytes = torch.empty(max(n_cap, 1), dtype=torch.int64, device=dev)
        tc = tb = None
        if info.get("tiered"):
            tc = torch.empty((NUM_TIERS, max(n_cap, 1)), dtype=torch.int64, device=dev)
            tb = torch.empty((NUM_TIERS, max(n_cap, 1)), dtype=torch.int64, device=dev)
        rc = LIB.s3imph_merge_rows_fill_device(self._h, _dev_ptr(blob), blob_cap, _dev_ptr(offs), _dev_ptr(depth),
                                               _dev_ptr(ocnt), _dev_ptr(tbytes), _dev_ptr(tc), _dev_ptr(tb), n_cap,
                                               _stream_ptr(stream))
        if rc != OK:
            raise MPHFError(rc, self.last_error() or f"merge: {status_string(rc)}")
        return {"blob": blob[: (nbytes + 7) // 8 * 8], "offsets": offs[: n + 1], "depth": depth[:n],
                "object_count": ocnt[:n], "total_bytes": tbytes[:n], "tier_count": tc, "tier_bytes": tb, "n": n,
                "blob_bytes": nbytes, "present_mask": info.get("present_mask", 0)}

    def close(self) -> None:
        if getattr(self, "_h", None):
            LIB.s3imph_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def finalize_index_host(blob: np.ndarray, offsets: np.ndarray, out_dir: str, depths: np.ndarray | None = None,
                        device: int = 0) -> None:
    """IndexBuilder.Finalize's depth / subtree / depth-index files (indexbuild.go:393-415,
    474-503; depthindex.go:32-96), computed on the GPU, written into out_dir."""
    blob = np.ascontiguousarray(blob, np.uint8)
    offsets = np.ascontiguousarray(offsets, np.uint64)
    dp = None if depths is None else np.ascontiguousarray(depths, np.uint32)
    err = ctypes.create_string_buffer(1024)
    rc = LIB.s3imph_finalize_index_host(device, _np_ptr(blob), _np_ptr(offsets), _np_ptr(dp) if dp is not None else None,
                                        len(offsets) - 1, out_dir.encode(), err, 1024)
    _check(rc, err)


def _listing(keys_blob, key_offsets, sizes):
    blob = np.ascontiguousarray(keys_blob, np.uint8)
    offs = np.ascontiguousarray(key_offsets, np.uint64)
    m = len(offs) - 1
    sz = None if sizes is None else np.ascontiguousarray(sizes, np.uint64)
    if sz is not None and len(sz) != m:
        raise ValueError("sizes must hold one entry per key")
    return blob, offs, sz, m


def aggregate(keys_blob: np.ndarray, key_offsets: np.ndarray, sizes: np.ndarray | None, max_depth: int = 0,
              device: int = 0, tiers=None):
    """extsort.Aggregator + SortPrefixRows (aggregator.go:44-76, :138-) on the GPU
    (s3imph_aggregate_host): the byte-sorted object listing (keys in the blob / offsets layout,
    one size per key; max_depth 0 = unlimited) -> (prefix_blob u8, prefix_offsets u64[n + 1],
    depth u32[n], object_count u64[n], total_bytes u64[n]) in the reference's row order.  With
    ``tiers`` (one tier id per key; s3imph_aggregate_tiers_host) the tuple gains tier_count and
    tier_bytes, (NUM_TIERS, n) u64 each, and present_mask."""
    blob, offs, sz, m = _listing(keys_blob, key_offsets, sizes)
    out = [ctypes.c_void_p() for _ in range(5 if tiers is None else 7)]
    n = ctypes.c_uint64()
    mask = ctypes.c_uint64()
    err = ctypes.create_string_buffer(1024)
    if tiers is None:
        rc = LIB.s3imph_aggregate_host(device, _np_ptr(blob), _np_ptr(offs), _np_ptr(sz), m, max_depth,
                                       *[ctypes.byref(p) for p in out], ctypes.byref(n), err, 1024)
    else:
        tr = _tier_ids(tiers, m)
        rc = LIB.s3imph_aggregate_tiers_host(device, _np_ptr(blob), _np_ptr(offs), _np_ptr(sz), _np_ptr(tr), m,
                                             max_depth, *[ctypes.byref(p) for p in out], ctypes.byref(mask),
                                             ctypes.byref(n), err, 1024)
    try:
        _check(rc, err)
        nn = n.value

        def take(p, dtype, count):
            a = np.zeros(count, dtype)
            if count and p.value:
                ctypes.memmove(a.ctypes.data, p.value, a.nbytes)
            return a

        offsets = take(out[1], np.uint64, nn + 1)
        rows = (take(out[0], np.uint8, int(offsets[-1])), offsets, take(out[2], np.uint32, nn),
                take(out[3], np.uint64, nn), take(out[4], np.uint64, nn))
        if tiers is None:
            return rows
        return rows + (take(out[5], np.uint64, NUM_TIERS * nn).reshape(NUM_TIERS, nn),
                       take(out[6], np.uint64, NUM_TIERS * nn).reshape(NUM_TIERS, nn), int(mask.value))
    finally:
        for p in out:
            if p.value:
                LIB.s3imph_free(p)


def build_index_from_objects(keys_blob: np.ndarray, key_offsets: np.ndarray, sizes: np.ndarray | None, out_dir: str,
                             max_depth: int = 0, device: int = 0, tiers=None) -> None:
    """Object listing in, index directory out (s3imph_index_from_objects_host): aggregation,
    MPHF build and finalize in one device residency; writes the MPHF-stage files, the finalize
    files, object_count.u64 / total_bytes.u64 and manifest.json into out_dir.  With ``tiers`` (one
    tier id per key; s3imph_index_from_objects_tiers_host) also tier_stats/ and tiers.json."""
    blob, offs, sz, m = _listing(keys_blob, key_offsets, sizes)
    err = ctypes.create_string_buffer(1024)
    if tiers is None:
        _check(LIB.s3imph_index_from_objects_host(device, _np_ptr(blob), _np_ptr(offs), _np_ptr(sz), m, max_depth,
                                                  os.fsencode(out_dir), err, 1024), err)
    else:
        tr = _tier_ids(tiers, m)
        _check(LIB.s3imph_index_from_objects_tiers_host(device, _np_ptr(blob), _np_ptr(offs), _np_ptr(sz), _np_ptr(tr),
                                                        m, max_depth, os.fsencode(out_dir), err, 1024), err)


def sort_objects(keys_blob: np.ndarray, key_offsets: np.ndarray, device: int = 0):
    """s3imph_sort_objects_host: the byte order of an object listing in any order (unsigned bytes,
    a proper prefix first, equal keys in input order: SortPrefixRows' comparison, types.go:160-164)
    -> (order u32[m], info dict); order[j] is the input index of the j-th key in sorted order."""
    blob, offs, _, m = _listing(keys_blob, key_offsets, None)
    p = ctypes.c_void_p()
    info = SortInfo()
    err = ctypes.create_string_buffer(1024)
    rc = LIB.s3imph_sort_objects_host(device, _np_ptr(blob), _np_ptr(offs), m, ctypes.byref(p), ctypes.byref(info),
                                      err, 1024)
    try:
        _check(rc, err)
        order = np.zeros(m, np.uint32)
        if m and p.value:
            ctypes.memmove(order.ctypes.data, p.value, order.nbytes)
        return order, info.as_dict()
    finally:
        if p.value:
            LIB.s3imph_free(p)


def build_index_from_unsorted_objects(keys_blob: np.ndarray, key_offsets: np.ndarray, sizes: np.ndarray | None,
                                      out_dir: str, tiers=None, max_depth: int = 0, device: int = 0) -> None:
    """build_index_from_objects for a listing in any order (s3imph_index_from_unsorted_objects_host):
    the listing is sorted (stably) and gathered on the GPU, then takes the same path; the directory
    is the one build_index_from_objects writes for the listing sorted beforehand."""
    blob, offs, sz, m = _listing(keys_blob, key_offsets, sizes)
    tr = None if tiers is None else _tier_ids(tiers, m)
    err = ctypes.create_string_buffer(1024)
    _check(LIB.s3imph_index_from_unsorted_objects_host(device, _np_ptr(blob), _np_ptr(offs), _np_ptr(sz), _np_ptr(tr),
                                                       m, max_depth, os.fsencode(out_dir), err, 1024), err)


def _csv_schema(schema) -> CsvSchema:
    if isinstance(schema, CsvSchema):
        return schema
    cols = tuple(int(c) for c in schema) + (-1, -1)
    return CsvSchema(*cols[:4])


def csv_geometry() -> tuple[int, int]:
    """(run bytes, tile bytes) of the CSV automaton passes: a lane walks a run, a workgroup a tile
    (s3imph_csv_geometry; for tests that place events on the edges)."""
    run, tile = ctypes.c_uint32(), ctypes.c_uint32()
    LIB.s3imph_csv_geometry(ctypes.byref(run), ctypes.byref(tile))
    return int(run.value), int(tile.value)


def csv_header_schema(data) -> tuple[tuple[int, int, int, int], int]:
    """s3imph_csv_header_schema (OpenFileWithOptions, reader.go:96-135; host only): the columns
    named key / size / storageclass / intelligenttieringaccesstier in the CSV's first record
    (-1: absent) and the byte offset where the data rows begin."""
    buf = np.frombuffer(bytes(data), np.uint8)
    sch, start = CsvSchema(), ctypes.c_uint64()
    err = ctypes.create_string_buffer(1024)
    _check(LIB.s3imph_csv_header_schema(_np_ptr(buf), len(buf), ctypes.byref(sch), ctypes.byref(start), err, 1024), err)
    return (sch.key_col, sch.size_col, sch.storage_col, sch.access_tier_col), int(start.value)


def parse_inventory_csv(data, schema, device: int = 0):
    """s3imph_csv_parse_host: decompressed inventory CSV bytes -> the object listing CSVReader.Read
    (reader.go:250-297) returns record by record, parsed on the GPU: (keys_blob u8, key_offsets
    u64[m + 1], sizes u64[m], tiers u8[m], info dict).  schema = (key_col, size_col, storage_col,
    access_tier_col), the last two -1 when absent."""
    buf = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else np.ascontiguousarray(data, np.uint8)
    out = [ctypes.c_void_p() for _ in range(4)]
    info = CsvInfo()
    err = ctypes.create_string_buffer(1024)
    rc = LIB.s3imph_csv_parse_host(device, _np_ptr(buf), len(buf), ctypes.byref(_csv_schema(schema)),
                                   *[ctypes.byref(p) for p in out], ctypes.byref(info), err, 1024)
    try:
        _check(rc, err)

        def take(p, dtype, count):
            a = np.zeros(count, dtype)
            if count and p.value:
                ctypes.memmove(a.ctypes.data, p.value, a.nbytes)
            return a

        m = info.n_objects
        return (take(out[0], np.uint8, info.key_bytes), take(out[1], np.uint64, m + 1), take(out[2], np.uint64, m),
                take(out[3], np.uint8, m), info.as_dict())
    finally:
        for p in out:
            if p.value:
                LIB.s3imph_free(p)


def build_index_from_inventory_csv(files, schema, out_dir: str, with_tiers: bool = False, max_depth: int = 0,
                                   device: int = 0) -> dict:
    """s3imph_index_from_csv_host: decompressed inventory CSV buffers (a list of bytes-likes, each
    parsed on its own and appended in order) -> index directory, everything after the H2D on the
    GPU: parse, sort, aggregation, MPHF build, finalize.  Returns the summed s3imph_csv_info."""
    bufs = [np.frombuffer(bytes(f), np.uint8) if not isinstance(f, np.ndarray) else np.ascontiguousarray(f, np.uint8)
            for f in files]
    k = len(bufs)
    ptrs = (ctypes.c_void_p * max(k, 1))(*[b.ctypes.data if b.size else None for b in bufs])
    lens = (ctypes.c_uint64 * max(k, 1))(*[b.size for b in bufs])
    info = CsvInfo()
    err = ctypes.create_string_buffer(1024)
    _check(LIB.s3imph_index_from_csv_host(device, ptrs, lens, k, ctypes.byref(_csv_schema(schema)), int(with_tiers),
                                          max_depth, os.fsencode(out_dir), ctypes.byref(info), err, 1024), err)
    return info.as_dict()


def _host_files(files):
    bufs = [np.frombuffer(bytes(f), np.uint8) if not isinstance(f, np.ndarray) else np.ascontiguousarray(f, np.uint8)
            for f in files]
    k = len(bufs)
    ptrs = (ctypes.c_void_p * max(k, 1))(*[b.ctypes.data if b.size else None for b in bufs])
    lens = (ctypes.c_uint64 * max(k, 1))(*[b.size for b in bufs])
    return bufs, ptrs, lens, k


def gunzip_geometry() -> tuple[int, int, int]:
    """(in_chunk_bytes, batch_symbols, waves_per_cu) of the GPU inflate (s3imph_gunzip_geometry;
    for tests that place events on the edges)."""
    a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    LIB.s3imph_gunzip_geometry(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


def gunzip_room_hint(data) -> int:
    """s3imph_gunzip_room_hint (host only): min(ISIZE of the file's last four bytes,
    1032 * len + 64), 0 for a file shorter than 18 bytes."""
    buf = np.frombuffer(bytes(data), np.uint8)
    return int(LIB.s3imph_gunzip_room_hint(_np_ptr(buf), len(buf)))


def gunzip(files, device: int = 0, with_info: bool = False):
    """s3imph_gunzip_host: gzip files (a list of bytes-likes) inflated on the GPU, one wave per
    file -> a list of bytes; with_info also the s3imph_gunzip_info dicts.  A bad file raises
    MPHFError(ERR_FORMAT, "gzip: file <i>: ...")."""
    bufs, ptrs, lens, k = _host_files(files)
    outs = (ctypes.c_void_p * max(k, 1))()
    out_len = (ctypes.c_uint64 * max(k, 1))()
    info = (GunzipInfo * max(k, 1))()
    err = ctypes.create_string_buffer(1024)
    rc = LIB.s3imph_gunzip_host(device, ptrs, lens, k, outs, out_len, info, err, 1024)
    try:
        _check(rc, err)
        texts = [ctypes.string_at(outs[i], out_len[i]) if out_len[i] else b"" for i in range(k)]
    finally:
        for i in range(k):
            if outs[i]:
                LIB.s3imph_free(outs[i])
    return (texts, [info[i].as_dict() for i in range(k)]) if with_info else texts


def build_index_from_inventory_csv_gz(files, schema, out_dir: str, with_tiers: bool = False, max_depth: int = 0,
                                      group_bytes: int = 0, device: int = 0) -> dict:
    """s3imph_index_from_csv_gz_host: .csv.gz inventory files (a list of bytes-likes) -> index
    directory.  The compressed bytes go to the GPU, which inflates them in groups of about
    group_bytes (0: the library's default) and parses the texts where they lie; from there as
    build_index_from_inventory_csv.  Returns the summed s3imph_csv_info."""
    bufs, ptrs, lens, k = _host_files(files)
    info = CsvInfo()
    err = ctypes.create_string_buffer(1024)
    _check(LIB.s3imph_index_from_csv_gz_host(device, ptrs, lens, k, ctypes.byref(_csv_schema(schema)),
                                             int(with_tiers), max_depth, group_bytes, os.fsencode(out_dir),
                                             ctypes.byref(info), err, 1024), err)
    return info.as_dict()


def merge_geometry() -> int:
    """The row merge's sample step (s3imph_merge_geometry): every step-th row of a run is a
    splitter; for tests that place run lengths on its edges."""
    step = ctypes.c_uint32()
    LIB.s3imph_merge_geometry(ctypes.byref(step))
    return int(step.value)


def _row_runs(runs):
    """Runs as (blob, offsets, depth, count, bytes[, tier_count, tier_bytes[, mask]]) tuples — the
    tuples aggregate() returns — -> (RowRun array, k, the arrays kept alive).  A run may also be a
    RowRun the caller has filled (any offsets[0], any tier_stride, NULL pointers): it is passed as
    it is, and the caller keeps its arrays alive."""
    keep, out = [], []
    for run in runs:
        if isinstance(run, RowRun):
            keep.append(run)
            out.append(run)
            continue
        run = tuple(run)
        if len(run) not in (5, 7, 8):
            raise ValueError("a run is (blob, offsets, depth, count, bytes[, tier_count, tier_bytes])")
        blob = np.ascontiguousarray(run[0], np.uint8)
        offs = np.ascontiguousarray(run[1], np.uint64)
        n = len(offs) - 1
        depth = np.ascontiguousarray(run[2], np.uint32)
        cnt = np.ascontiguousarray(run[3], np.uint64)
        tot = np.ascontiguousarray(run[4], np.uint64)
        if n < 0 or len(depth) != n or len(cnt) != n or len(tot) != n:
            raise ValueError("a run's depth, count and bytes must hold one entry per row")
        tc = tb = None
        if len(run) >= 7 and run[5] is not None:
            tc = np.ascontiguousarray(run[5], np.uint64).reshape(NUM_TIERS, -1)
            tb = np.ascontiguousarray(run[6], np.uint64).reshape(NUM_TIERS, -1)
            if tc.shape != (NUM_TIERS, n) or tb.shape != (NUM_TIERS, n):
                raise ValueError("a run's tier columns must be (NUM_TIERS, n)")
        keep.append((blob, offs, depth, cnt, tot, tc, tb))
        p = lambda a: a.ctypes.data if a is not None and a.size else None  # noqa: E731
        out.append(RowRun(p(blob), offs.ctypes.data if n else None, p(depth), p(cnt), p(tot),
                          tc.ctypes.data if tc is not None and n else None,
                          tb.ctypes.data if tb is not None and n else None, n, n))
    k = len(out)
    return (RowRun * max(k, 1))(*out), k, keep


def merge_rows(runs, device: int = 0, with_info: bool = False):
    """MergeIterator + PrefixRow.Merge (merger.go:104-140, types.go:82-91) on the GPU
    (s3imph_merge_rows_host): sorted runs of prefix rows — tuples (blob, offsets, depth, count,
    bytes[, tier_count, tier_bytes]) as aggregate() returns them — merged into one: the same
    tuple, with present_mask appended when the runs carry tier columns.  Equal prefixes are summed;
    the depth comes from the lowest run.  More than MERGE_MAX_RUNS runs merge in rounds.  With
    ``with_info`` the s3imph_merge_info dict is appended."""
    arr, k, keep = _row_runs(runs)
    out = [ctypes.c_void_p() for _ in range(7)]
    n, mask, info = ctypes.c_uint64(), ctypes.c_uint64(), MergeInfo()
    err = ctypes.create_string_buffer(1024)
    rc = LIB.s3imph_merge_rows_host(device, arr, k, *[ctypes.byref(p) for p in out], ctypes.byref(mask),
                                    ctypes.byref(n), ctypes.byref(info), err, 1024)
    try:
        if rc != OK:
            e = MPHFError(rc, err.value.decode(errors="replace") or status_string(rc))
            e.info = info.as_dict()
            raise e
        nn = n.value

        def take(p, dtype, count):
            a = np.zeros(count, dtype)
            if count and p.value:
                ctypes.memmove(a.ctypes.data, p.value, a.nbytes)
            return a

        offsets = take(out[1], np.uint64, nn + 1)
        rows = (take(out[0], np.uint8, int(offsets[-1])), offsets, take(out[2], np.uint32, nn),
                take(out[3], np.uint64, nn), take(out[4], np.uint64, nn))
        if any(arr[r].tier_count and arr[r].n for r in range(k)):  # an empty run counts with neither
            rows += (take(out[5], np.uint64, NUM_TIERS * nn).reshape(NUM_TIERS, nn),
                     take(out[6], np.uint64, NUM_TIERS * nn).reshape(NUM_TIERS, nn), int(mask.value))
        return rows + (info.as_dict(),) if with_info else rows
    finally:
        for p in out:
            if p.value:
                LIB.s3imph_free(p)


def build_index_from_rows(runs, out_dir: str, device: int = 0) -> None:
    """runMergeBuildPhase (pipeline.go:786-914; s3imph_index_from_rows_host): sorted runs of prefix
    rows in, index directory out — merge, MPHF build and finalize in one device residency; the
    tier files are written when the runs carry tier columns.  No rows: the empty index."""
    arr, k, keep = _row_runs(runs)
    err = ctypes.create_string_buffer(1024)
    _check(LIB.s3imph_index_from_rows_host(device, arr, k, os.fsencode(out_dir), err, 1024), err)
    del keep


class RowSet:
    """The chunked build (s3imph_rowset_*; Pipeline's ingest loop, pipeline.go:370-517, :703-783):
    chunks of a listing that does not fit one GPU are each sorted and aggregated on the GPU into a
    run held in host memory; build() merges the runs on the GPU and writes the directory
    build_index_from_unsorted_objects writes for the concatenation of the chunks."""

    def __init__(self, max_depth: int = 0, with_tiers: bool = False, device: int = 0):
        self._h = ctypes.c_void_p()
        self.with_tiers = bool(with_tiers)
        err = ctypes.create_string_buffer(1024)
        _check(LIB.s3imph_rowset_new(device, max_depth, int(self.with_tiers), ctypes.byref(self._h), err, 1024), err)

    def add_objects(self, keys_blob, key_offsets, sizes, tiers=None) -> None:
        """One chunk of the listing, in any order: one run (none for a chunk without an object)."""
        blob, offs, sz, m = _listing(keys_blob, key_offsets, sizes)
        tr = None if tiers is None else _tier_ids(tiers, m)
        err = ctypes.create_string_buffer(1024)
        _check(LIB.s3imph_rowset_add_objects(self._h, _np_ptr(blob), _np_ptr(offs), _np_ptr(sz), _np_ptr(tr), m,
                                             err, 1024), err)

    def add_csv(self, files, schema) -> None:
        """Decompressed inventory CSV buffers (a list of bytes-likes), parsed on the GPU: one run."""
        bufs = [np.frombuffer(bytes(f), np.uint8) if not isinstance(f, np.ndarray)
                else np.ascontiguousarray(f, np.uint8) for f in files]
        k = len(bufs)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[b.ctypes.data if b.size else None for b in bufs])
        lens = (ctypes.c_uint64 * max(k, 1))(*[b.size for b in bufs])
        err = ctypes.create_string_buffer(1024)
        _check(LIB.s3imph_rowset_add_csv(self._h, ptrs, lens, k, ctypes.byref(_csv_schema(schema)), err, 1024), err)

    def add_csv_gz(self, files, schema, group_bytes: int = 0) -> None:
        """.csv.gz inventory files (a list of bytes-likes), inflated and parsed on the GPU: one run."""
        bufs, ptrs, lens, k = _host_files(files)
        err = ctypes.create_string_buffer(1024)
        _check(LIB.s3imph_rowset_add_csv_gz(self._h, ptrs, lens, k, ctypes.byref(_csv_schema(schema)), group_bytes,
                                            err, 1024), err)

    def add_rows(self, run) -> None:
        """A caller's sorted run (a tuple as merge_rows takes them), copied."""
        arr, _, keep = _row_runs([run])
        err = ctypes.create_string_buffer(1024)
        _check(LIB.s3imph_rowset_add_rows(self._h, arr, err, 1024), err)
        del keep

    @property
    def runs(self) -> int:
        return int(LIB.s3imph_rowset_runs(self._h))

    @property
    def rows(self) -> int:
        return int(LIB.s3imph_rowset_rows(self._h))

    def build(self, out_dir: str) -> None:
        err = ctypes.create_string_buffer(1024)
        _check(LIB.s3imph_rowset_build(self._h, os.fsencode(out_dir), err, 1024), err)

    def close(self) -> None:
        if getattr(self, "_h", None):
            LIB.s3imph_rowset_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def write_manifest(out_dir: str, node_count: int, max_depth: int) -> None:
    """format.WriteManifest (pkg/format/manifest.go:33-95): manifest.json with the size and
    SHA-256 of every index file present in out_dir."""
    err = ctypes.create_string_buffer(1024)
    _check(LIB.s3imph_write_manifest(out_dir.encode(), node_count, max_depth, err, 1024), err)


def read_manifest(dir_: str) -> dict:
    """format.ReadManifest (manifest.go:97-111)."""
    import json
    with open(os.path.join(dir_, "manifest.json"), "rb") as f:
        return json.loads(f.read())


def verify_manifest(dir_: str) -> None:
    """format.VerifyManifest (manifest.go:113-138): every listed file's size and checksum;
    raises MPHFError (ERR_FORMAT on a mismatch, ERR_IO on a missing file)."""
    err = ctypes.create_string_buffer(1024)
    _check(LIB.s3imph_verify_manifest(dir_.encode(), err, 1024), err)


def sha256_file(path: str, portable: bool = False) -> str:
    """checksumFile (manifest.go:140-155): hex SHA-256 of a file."""
    err = ctypes.create_string_buffer(1024)
    out = ctypes.create_string_buffer(65)
    _check(LIB.s3imph_sha256_file(path.encode(), int(portable), out, err, 1024), err)
    return out.value.decode()


S3ID_MAGIC = 0x53334944  # pkg/format/format.go:6-45
S3ID_VERSION = 1
S3ID_HEADER = 20


def read_array(path: str, width: int = 8) -> np.ndarray:
    """OpenArray (pkg/format/reader.go:81-119): S3ID header checked (magic, version, the
    expected width, payload size), payload returned as little-endian u64 / u32
    (memory-mapped)."""
    raw = np.memmap(path, dtype=np.uint8, mode="r")
    if len(raw) < S3ID_HEADER:
        raise MPHFError(ERR_FORMAT, f"open array {path}: file too small")
    hdr = bytes(raw[:S3ID_HEADER])
    magic, version = int.from_bytes(hdr[0:4], "little"), int.from_bytes(hdr[4:8], "little")
    count, w = int.from_bytes(hdr[8:16], "little"), int.from_bytes(hdr[16:20], "little")
    if magic != S3ID_MAGIC or version != S3ID_VERSION or w != width or len(raw) != S3ID_HEADER + width * count:
        raise MPHFError(ERR_FORMAT, f"open array {path}: bad header")
    return raw[S3ID_HEADER:].view("<u8" if width == 8 else "<u4")


def read_u64_array(path: str) -> np.ndarray:
    """OpenArray for width-8 arrays (mph_fp.u64, mph_pos.u64, prefix_offsets.u64, ...)."""
    return read_array(path, 8)


class MPHF:
    """format.MPHF on the GPU (OpenMPHF / Lookup / VerifyMPHF, pkg/format/mphf.go:186-302,
    :372-393): mph.bin loaded into a device context, mph_fp / mph_pos in HBM, batched
    Lookup; prefix_blob.bin / prefix_offsets.u64 (when present) for VerifyMPHF."""

    def __init__(self, out_dir: str, device: int = 0):
        import torch
        mph = open(os.path.join(out_dir, "mph.bin"), "rb").read()
        self.ctx = DeviceBuilder(device)
        self.count = 0
        self.dev = f"cuda:{device}"
        self.blob = self.offsets = None
        if mph:
            fp = read_u64_array(os.path.join(out_dir, "mph_fp.u64"))
            pos = read_u64_array(os.path.join(out_dir, "mph_pos.u64"))
            if len(fp) != len(pos):
                raise MPHFError(ERR_FORMAT, "open MPHF: fingerprint and position arrays differ in length")
            self.count = len(fp)
            # read_u64_array may hand back a read-only view of the file: copy before torch takes it
            self.d_fp = torch.from_numpy(np.array(fp, dtype=np.uint64).view(np.int64)).to(self.dev)
            self.d_pos = torch.from_numpy(np.array(pos, dtype=np.uint64).view(np.int64)).to(self.dev)
        else:
            self.d_fp = self.d_pos = torch.zeros(1, dtype=torch.int64, device=self.dev)
        self.ctx.load_mph_bin(mph)
        bp, op = os.path.join(out_dir, "prefix_blob.bin"), os.path.join(out_dir, "prefix_offsets.u64")
        if os.path.exists(bp):
            self.offsets = np.ascontiguousarray(read_u64_array(op))
            self.blob = np.fromfile(bp, dtype=np.uint8)

    def lookup(self, keys) -> np.ndarray:
        """Lookup (mphf.go:275-302) of a batch: pos per key, or 2^64-1 when not found."""
        blob, offs = keys_to_blob(keys)
        return self.lookup_blob(blob, offs)

    def lookup_blob(self, blob: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        import torch
        n = len(offsets) - 1
        pad = np.zeros(((len(blob) + 7) // 8) * 8 + 8, np.uint8)
        pad[:len(blob)] = blob
        d_blob = torch.from_numpy(pad).to(self.dev)
        # offsets may be a read-only view of prefix_offsets.u64: copy before torch takes it
        d_offs = torch.from_numpy(np.array(offsets, dtype=np.uint64).view(np.int64)).to(self.dev)
        res = torch.empty(max(n, 1), dtype=torch.int64, device=self.dev)
        self.ctx.lookup(d_blob, d_offs, n, self.d_fp, self.d_pos, self.count, res)
        return res[:n].cpu().numpy().view(np.uint64)

    def verify(self) -> None:
        """VerifyMPHF (mphf.go:372-393): every prefix i of the blob looks up to i."""
        if self.offsets is None:
            raise MPHFError(ERR_STATE, "prefix blob not loaded")
        got = self.lookup_blob(self.blob, self.offsets)
        bad = np.nonzero(got != np.arange(len(got), dtype=np.uint64))[0]
        if len(bad):
            i = int(bad[0])
            raise MPHFError(ERR_INTERNAL, f"lookup returned wrong pos for prefix {i}: got {int(got[i])}, want {i}")

    def close(self) -> None:
        self.ctx.close()


class Index:
    """indexread.Index on the GPU (pkg/indexread/index.go; include/s3imph.h section 5c): the
    index's arrays in HBM and the reader's queries answered for a whole batch per call.

        idx = Index(dir)                          # Open (:31)
        idx.count, idx.max_depth                  # Count (:188), MaxDepth (:193)
        idx.lookup(keys)                          # Lookup (:128), 2^64-1 when not found
        idx.nodes(pos)                            # Stats / Depth / SubtreeEnd / MaxDepthInSubtree (:135-176)
        idx.stats_for_prefix(keys)                # StatsForPrefix (:146)
        idx.descendants_at_depth(pos, rel)        # DescendantsAtDepth[Filtered] (:206, :277)
        idx.descendants_up_to_depth(pos, max_rel) # DescendantsUpToDepth (:239)
        idx.prefix_string(pos)                    # PrefixString (:179), one position from the host files
        idx = Index(dir, prefixes=True)           # ... with the prefix blob in HBM (OpenMPHF, mphf.go:226-238)
        idx.prefix_strings(pos)                   # PrefixString for a batch, None where out of bounds
        idx.lookup_verify(keys)                   # MPHF.LookupWithVerify (mphf.go:306)
        idx.verify()                              # VerifyMPHF (mphf.go:372)
        idx.has_tier_data(), idx.present_tiers()  # HasTierData (:360), the manifest's tiers
        idx.tier_breakdown_all(pos)               # TierBreakdownAll (:380)
        idx.tier_breakdown(pos)                   # TierBreakdown (:368)
        idx.tier_breakdown_for_prefix(keys)       # TierBreakdownForPrefix (:394)
        idx.close()                               # Close (:108)

    Positions are given as a sequence, a numpy array or a device tensor (int64 holding the
    u64 bits).  object_count.u64 / total_bytes.u64 are optional (zeros without them)."""

    def __init__(self, dir_: str, device: int = 0, prefixes: bool = False):
        err = ctypes.create_string_buffer(1024)
        h = ctypes.c_void_p()
        if prefixes:  # s3imph_index_open_flags: the prefix blob in HBM too, when the directory has one
            _check(LIB.s3imph_index_open_flags(device, os.fsencode(dir_), OPEN_PREFIXES, ctypes.byref(h), err, 1024),
                   err)
        else:
            _check(LIB.s3imph_index_open(device, os.fsencode(dir_), ctypes.byref(h), err, 1024), err)
        self._h = h
        self._init(device, dir_, None)

    def _init(self, device: int, dir_: str | None, keep) -> None:
        self.device = device
        self.dev = f"cuda:{device}"
        self.dir = dir_
        self._keep = keep  # borrowed device tensors stay alive with the handle
        self._prefixes = None
        self._keep_prefixes = None
        self.count = int(LIB.s3imph_index_count(self._h))
        self.max_depth = int(LIB.s3imph_index_max_depth(self._h))

    @classmethod
    def from_arrays(cls, mph_bin: bytes, fp, pos, depth, subtree_end, max_depth_in_subtree, depth_offsets,
                    depth_positions, max_depth: int | None = None, object_count=None, total_bytes=None,
                    device: int | None = None) -> "Index":
        """s3imph_index_attach: an index over device tensors (e.g. DeviceBuilder.build's outputs,
        mph_bin() and finalize_index()'s arrays), borrowed for the life of the handle."""
        if device is None:
            device = fp.device.index or 0
        n = int(fp.shape[0])
        a = IndexArrays()
        buf = ctypes.create_string_buffer(mph_bin, max(len(mph_bin), 1))
        a.mph_bin, a.mph_len, a.n = ctypes.cast(buf, ctypes.c_void_p).value, len(mph_bin), n
        a.d_fp, a.d_pos = fp.data_ptr(), pos.data_ptr()
        a.d_depth, a.d_max_depth_in_subtree = depth.data_ptr(), max_depth_in_subtree.data_ptr()
        a.d_subtree_end, a.d_depth_offsets = subtree_end.data_ptr(), depth_offsets.data_ptr()
        a.d_depth_positions = depth_positions.data_ptr()
        a.max_depth = int(depth_offsets.shape[0]) - 2 if max_depth is None else max_depth
        a.d_object_count = None if object_count is None else object_count.data_ptr()
        a.d_total_bytes = None if total_bytes is None else total_bytes.data_ptr()
        err = ctypes.create_string_buffer(1024)
        h = ctypes.c_void_p()
        _check(LIB.s3imph_index_attach(device, ctypes.byref(a), ctypes.byref(h), err, 1024), err)
        self = cls.__new__(cls)
        self._h = h
        self._init(device, None, (fp, pos, depth, subtree_end, max_depth_in_subtree, depth_offsets, depth_positions,
                                  object_count, total_bytes))
        return self

    attach = from_arrays  # s3imph_index_attach under its own name

    def attach_tiers(self, ids, tier_count, tier_bytes) -> None:
        """s3imph_index_attach_tiers: tier data for a handle of from_arrays, from the
        (NUM_TIERS, stride) device tensors DeviceBuilder.aggregate_fill_tiers returned; ``ids``
        are the tiers to answer for, in result order (a present_mask's set bits, usually).  The
        handle copies what it needs."""
        ids = np.ascontiguousarray(ids, np.uint8).reshape(-1)
        stride = int(tier_count.stride(0)) if tier_count.dim() == 2 else int(tier_count.numel()) // NUM_TIERS
        self._fail(LIB.s3imph_index_attach_tiers(self._h, _np_ptr(ids), len(ids), _dev_ptr(tier_count),
                                                 _dev_ptr(tier_bytes), stride), "attach tiers")

    # -- tier statistics ------------------------------------------------------------------
    def has_tier_data(self) -> bool:
        """HasTierData (index.go:360)."""
        return int(LIB.s3imph_index_tier_count(self._h)) > 0

    def present_tiers(self) -> list:
        """The tier ids the index holds, in manifest order (TierStatsReader.PresentTiers)."""
        ids = np.zeros(NUM_TIERS, np.uint8)
        t = int(LIB.s3imph_index_tier_ids(self._h, _np_ptr(ids), NUM_TIERS))
        return [int(v) for v in ids[:t]]

    def tiers_device(self, pos, stream=None):
        """s3imph_index_tiers_device: (out int64 (nq, T, 2) holding count, bytes as u64 bits; mask
        int32 (nq,)) on the device; T == 0 gives empty tensors."""
        import torch
        with _torch_on(stream, self.dev):  # the fills are ordered before the library's writes
            d_pos = self._pos_dev(pos)
            nq, t = int(d_pos.shape[0]), int(LIB.s3imph_index_tier_count(self._h))
            out = torch.zeros((max(nq, 1), max(t, 1), 2), dtype=torch.int64, device=self.dev)
            mask = torch.zeros(max(nq, 1), dtype=torch.int32, device=self.dev)
        self._fail(LIB.s3imph_index_tiers_device(self._h, _dev_ptr(d_pos), nq, _dev_ptr(out), _dev_ptr(mask),
                                                 _stream_ptr(stream)), "tier breakdown")
        return out[:nq, :t], mask[:nq]

    def tier_breakdown_all(self, pos) -> list:
        """TierBreakdownAll (index.go:380; GetBreakdownAll, tierstats.go:189) per position: a list
        of (tier id, tier name, bytes, object count) for every tier of the index, in manifest
        order (zeros past the end of the index); [] without tier data."""
        ids = self.present_tiers()
        out, _ = self.tiers_device(pos)
        v = out.cpu().numpy().view(np.uint64)
        return [[(t, TIERS[t][1], int(v[q, s, 1]), int(v[q, s, 0])) for s, t in enumerate(ids)]
                for q in range(v.shape[0])]

    def tier_breakdown(self, pos) -> list:
        """TierBreakdown (index.go:368; GetBreakdown, tierstats.go:157): as tier_breakdown_all,
        keeping only the tiers with a non-zero count or bytes at the position."""
        ids = self.present_tiers()
        out, mask = self.tiers_device(pos)
        v, mk = out.cpu().numpy().view(np.uint64), mask.cpu().numpy().view(np.uint32)
        return [[(t, TIERS[t][1], int(v[q, s, 1]), int(v[q, s, 0])) for s, t in enumerate(ids) if (mk[q] >> s) & 1]
                for q in range(v.shape[0])]

    def tier_breakdown_for_prefix(self, keys) -> list:
        """TierBreakdownForPrefix (index.go:394) per key: tier_breakdown at the key's position,
        [] for a key the index does not hold."""
        return self.tier_breakdown(self.lookup_device(*self._keys_dev(*keys_to_blob(keys))))

    # -- monthly cost (section 5h) ------------------------------------------------------
    def cost_device(self, pos, pt=None, stream=None):
        """s3imph_index_cost_device: an (nq, 17) int64 tensor holding one s3imph_cost per row
        (COST_DTYPE on the host).  pt None: the default us-east-1 table."""
        import torch
        with _torch_on(stream, self.dev):
            d_pos = self._pos_dev(pos)
        nq = int(d_pos.shape[0])
        out = torch.empty((max(nq, 1), COST_DTYPE.itemsize // 8), dtype=torch.int64, device=self.dev)
        self._fail(LIB.s3imph_index_cost_device(self._h, _dev_ptr(d_pos), nq, ctypes.byref(_pt_c(pt)), _dev_ptr(out),
                                                _stream_ptr(stream)), "monthly cost")
        return out[:nq]

    def cost_records(self, pos, pt=None) -> np.ndarray:
        """One COST_DTYPE record per position."""
        t = self.cost_device(pos, pt)
        if t.shape[0] == 0:
            return np.zeros(0, COST_DTYPE)
        return t.cpu().numpy().reshape(-1).view(COST_DTYPE)

    def monthly_cost(self, pos, pt=None) -> list:
        """query --estimate-cost per position: TierBreakdown(pos) -> ComputeMonthlyCost as dicts
        shaped like CostResult (per-tier by name, only the tier_mask tiers), plus ``found``."""
        return [_cost_dict(r) for r in self.cost_records(pos, pt)]

    def monthly_cost_for_prefix(self, keys, pt=None) -> list:
        """monthly_cost at each key's position; found False for a key the index does not hold."""
        return self.monthly_cost(self.lookup_device(*self._keys_dev(*keys_to_blob(keys))), pt)

    def descendants_top(self, pos, rel=None, max_rel: int = 0, key="cost", k: int = 10, pt=None, min_count: int = 0,
                        min_bytes: int = 0, stream=None):
        """descendants_plan followed by s3imph_index_descendants_top: (top_n int32 (n_rows,),
        top_pos int64 (n_rows, k), top_key int64 (n_rows, k)) on the device, u64 bits; key is
        "cost", "bytes" or "count" (or a RANK_* value)."""
        _, _, n_rows, _ = self.descendants_plan(pos, rel, max_rel, min_count, min_bytes, stream=stream)
        return self.top_of_plan(n_rows, key, k, pt, stream)

    def top_of_plan(self, n_rows: int, key="cost", k: int = 10, pt=None, stream=None):
        """s3imph_index_descendants_top on the rows of the last descendants_plan."""
        import torch
        kid = _RANK_KEYS.get(key, key) if isinstance(key, str) else int(key)
        if isinstance(kid, str):
            raise ValueError(f"unknown ranking key {key!r}")
        cells = max(n_rows * max(k, 0), 1) if n_rows * max(k, 0) < (1 << 31) else 1
        top_pos = torch.empty(cells, dtype=torch.int64, device=self.dev)
        top_key = torch.empty(cells, dtype=torch.int64, device=self.dev)
        top_n = torch.empty(max(n_rows, 1), dtype=torch.int32, device=self.dev)
        c_pt = ctypes.byref(_pt_c(pt)) if kid == RANK_MONTHLY_COST else None
        self._fail(LIB.s3imph_index_descendants_top(self._h, kid, c_pt, k, _dev_ptr(top_pos), _dev_ptr(top_key),
                                                    _dev_ptr(top_n), _stream_ptr(stream)), "descendants top")
        return (top_n[:n_rows], top_pos[: n_rows * k].reshape(n_rows, k), top_key[: n_rows * k].reshape(n_rows, k))

    def last_error(self) -> str:
        return LIB.s3imph_index_last_error(self._h).decode(errors="replace")

    def _fail(self, rc: int, what: str):
        if rc != OK:
            raise MPHFError(rc, f"{what}: {self.last_error() or status_string(rc)}")

    def _pos_dev(self, pos):
        """Query positions as a contiguous int64 device tensor (u64 bits)."""
        import torch
        if torch.is_tensor(pos):
            return pos.to(device=self.dev, dtype=torch.int64).contiguous()
        a = np.ascontiguousarray(np.asarray(pos, dtype=np.uint64).reshape(-1))
        return torch.from_numpy(a.view(np.int64).copy()).to(self.dev)

    # -- Lookup ------------------------------------------------------------------------
    def lookup_device(self, d_blob, d_offsets, nq: int, stream=None):
        """s3imph_index_lookup_device over a query blob in HBM: an int64 tensor of u64 positions."""
        import torch
        res = torch.empty(max(nq, 1), dtype=torch.int64, device=self.dev)
        self._fail(LIB.s3imph_index_lookup_device(self._h, _dev_ptr(d_blob), _dev_ptr(d_offsets), nq, _dev_ptr(res),
                                                  _stream_ptr(stream)), "lookup")
        return res[:nq]

    def _keys_dev(self, blob: np.ndarray, offsets: np.ndarray):
        """A query blob (padded to whole words) and its offsets on the device, and the key count."""
        import torch
        pad = np.zeros(((len(blob) + 7) // 8) * 8 + 8, np.uint8)
        pad[:len(blob)] = blob
        d_offs = torch.from_numpy(np.array(offsets, dtype=np.uint64).view(np.int64)).to(self.dev)
        return torch.from_numpy(pad).to(self.dev), d_offs, len(offsets) - 1

    def lookup_blob(self, blob: np.ndarray, offsets: np.ndarray) -> np.ndarray:
        return self.lookup_device(*self._keys_dev(blob, offsets)).cpu().numpy().view(np.uint64)

    def lookup(self, keys) -> np.ndarray:
        """Lookup (index.go:128) of a batch: pos per key, or 2^64-1 when not found."""
        return self.lookup_blob(*keys_to_blob(keys))

    # -- Stats / Depth / SubtreeEnd / MaxDepthInSubtree --------------------------------
    def nodes_device(self, pos, stream=None):
        """s3imph_index_nodes_device: an (nq, 6) int64 tensor holding one s3imph_node per row."""
        import torch
        with _torch_on(stream, self.dev):
            d_pos = self._pos_dev(pos)
        nq = int(d_pos.shape[0])
        out = torch.empty((max(nq, 1), NODE_DTYPE.itemsize // 8), dtype=torch.int64, device=self.dev)
        self._fail(LIB.s3imph_index_nodes_device(self._h, _dev_ptr(d_pos), nq, _dev_ptr(out), _stream_ptr(stream)),
                   "nodes")
        return out[:nq]

    def nodes(self, pos) -> np.ndarray:
        """One NODE_DTYPE record per position; all zero with found = 0 when pos >= count."""
        t = self.nodes_device(pos)
        if t.shape[0] == 0:
            return np.zeros(0, NODE_DTYPE)
        return t.cpu().numpy().reshape(-1).view(NODE_DTYPE)

    def stats_for_prefix(self, keys):
        """StatsForPrefix (index.go:146): (found bool, object_count u64, total_bytes u64) arrays."""
        blob, offs = keys_to_blob(keys)
        return self.stats_for_prefix_blob(blob, offs)

    def stats_for_prefix_blob(self, blob: np.ndarray, offsets: np.ndarray):
        r = self.nodes(self.lookup_device(*self._keys_dev(blob, offsets)))
        return r["found"] != 0, r["object_count"].copy(), r["total_bytes"].copy()

    # -- Descendants -------------------------------------------------------------------
    def descendants_plan(self, pos, rel=None, max_rel: int = 0, min_count: int = 0, min_bytes: int = 0,
                         row_ptr_cap: int | None = None, stream=None):
        """s3imph_index_descendants_plan.  rel given (an int for the batch or one per query):
        DESC_AT; rel None: DESC_UPTO with max_rel.  Returns (levels int32[nq], row_ptr
        int64[n_rows + 1], n_rows, total), tensors on the device."""
        import torch
        with _torch_on(stream, self.dev):  # conversions and the zero fill ahead of the library's work
            d_pos = self._pos_dev(pos)
            nq = int(d_pos.shape[0])
            if rel is not None:
                mode, rows = DESC_AT, nq
                if torch.is_tensor(rel):
                    d_rel = rel.to(device=self.dev, dtype=torch.int32).contiguous()
                else:
                    d_rel = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(rel, np.int32), (nq,)))
                                             .copy()).to(self.dev)
            else:
                mode, rows, d_rel = DESC_UPTO, nq * min(max(max_rel, 0), self.max_depth), None
            cap = rows + 1 if row_ptr_cap is None else row_ptr_cap
            levels = torch.empty(max(nq, 1), dtype=torch.int32, device=self.dev)
            row_ptr = torch.zeros(max(cap, 1), dtype=torch.int64, device=self.dev)
        n_rows, total = ctypes.c_uint64(), ctypes.c_uint64()
        self._fail(LIB.s3imph_index_descendants_plan(self._h, _dev_ptr(d_pos), _dev_ptr(d_rel), nq, mode, max_rel,
                                                     min_count, min_bytes, _dev_ptr(levels), _dev_ptr(row_ptr), cap,
                                                     ctypes.byref(n_rows), ctypes.byref(total), _stream_ptr(stream)),
                   "descendants plan")
        return levels[:nq], row_ptr[: n_rows.value + 1], int(n_rows.value), int(total.value)

    def descendants_fill(self, total: int, cap: int | None = None, stream=None):
        """s3imph_index_descendants_fill of the last plan: an int64 tensor of `total` u64 positions."""
        import torch
        cap = total if cap is None else cap
        out = torch.empty(max(cap, 1), dtype=torch.int64, device=self.dev)
        self._fail(LIB.s3imph_index_descendants_fill(self._h, _dev_ptr(out), cap, _stream_ptr(stream)),
                   "descendants fill")
        return out[:total]

    def descendants_csr(self, pos, rel=None, max_rel: int = 0, min_count: int = 0, min_bytes: int = 0, stream=None):
        """The raw form: (levels, row_ptr, out) tensors on the device.  Row r of the batch is
        out[row_ptr[r] : row_ptr[r + 1]]; DESC_AT has one row per query, DESC_UPTO
        min(max(max_rel, 0), max_depth) rows per query of which the first levels[q] count."""
        levels, row_ptr, _, total = self.descendants_plan(pos, rel, max_rel, min_count, min_bytes, stream=stream)
        return levels, row_ptr, self.descendants_fill(total, stream=stream)

    def descendants_at_depth(self, pos, rel, min_count: int = 0, min_bytes: int = 0) -> list:
        """DescendantsAtDepth / DescendantsAtDepthFiltered (index.go:206, :277) per query: None
        where the reference returns nil, else the u64 positions (possibly none)."""
        levels, row_ptr, out = self.descendants_csr(pos, rel, 0, min_count, min_bytes)
        lv, rp = levels.cpu().numpy(), row_ptr.cpu().numpy()
        o = out.cpu().numpy().view(np.uint64)
        return [o[rp[q]:rp[q + 1]] if lv[q] else None for q in range(len(lv))]

    def descendants_up_to_depth(self, pos, max_rel: int) -> list:
        """DescendantsUpToDepth (index.go:239) per query: None where the reference returns nil,
        else one u64 array per depth level."""
        levels, row_ptr, out = self.descendants_csr(pos, None, max_rel)
        lv, rp = levels.cpu().numpy(), row_ptr.cpu().numpy()
        o = out.cpu().numpy().view(np.uint64)
        R = (len(rp) - 1) // len(lv) if len(lv) else 0
        return [[o[rp[q * R + j]:rp[q * R + j + 1]] for j in range(lv[q])] if lv[q] else None
                for q in range(len(lv))]

    # -- PrefixString ------------------------------------------------------------------
    def prefix_string(self, pos: int) -> str:
        """PrefixString (index.go:179) from prefix_blob.bin / prefix_offsets.u64."""
        if self._prefixes is None:
            bp = None if self.dir is None else os.path.join(self.dir, "prefix_blob.bin")
            if bp is None or not os.path.exists(bp):
                raise MPHFError(ERR_STATE, f"get prefix for pos {pos}: prefix blob not loaded")
            offs = read_u64_array(os.path.join(self.dir, "prefix_offsets.u64"))
            self._prefixes = (np.memmap(bp, dtype=np.uint8, mode="r") if os.path.getsize(bp) else
                              np.zeros(0, np.uint8), offs)
        blob, offs = self._prefixes
        if pos < 0 or pos + 1 >= len(offs):
            raise MPHFError(ERR_INVALID, f"get prefix for pos {pos}: position out of bounds")
        return bytes(blob[int(offs[pos]):int(offs[pos + 1])]).decode(errors="surrogateescape")

    # -- the prefix blob in HBM: PrefixString for a batch, LookupWithVerify, VerifyMPHF --------
    def attach_prefixes(self, blob, offsets) -> None:
        """s3imph_index_attach_prefixes: the stored prefixes of a from_arrays handle, as device
        tensors (count + 1 offsets; the blob readable up to its last offset rounded up to 8),
        borrowed for the life of the handle.  A second call replaces the first."""
        self._fail(LIB.s3imph_index_attach_prefixes(self._h, _dev_ptr(blob), _dev_ptr(offsets)), "attach prefixes")
        self._keep_prefixes = (blob, offsets)

    def has_prefixes(self) -> bool:
        return bool(LIB.s3imph_index_has_prefixes(self._h))

    def prefixes_plan(self, pos, stream=None):
        """s3imph_index_prefixes_plan: (out_offsets int64[nq + 1], found int32[nq], total), the
        tensors on the device."""
        import torch
        with _torch_on(stream, self.dev):
            d_pos = self._pos_dev(pos)
            nq = int(d_pos.shape[0])
            offs = torch.zeros(nq + 1, dtype=torch.int64, device=self.dev)
            found = torch.zeros(max(nq, 1), dtype=torch.int32, device=self.dev)
        total = ctypes.c_uint64()
        self._fail(LIB.s3imph_index_prefixes_plan(self._h, _dev_ptr(d_pos), nq, _dev_ptr(offs), _dev_ptr(found),
                                                  ctypes.byref(total), _stream_ptr(stream)), "prefixes plan")
        return offs, found[:nq], int(total.value)

    def prefixes_fill(self, total: int, out=None, stream=None):
        """s3imph_index_prefixes_fill of the last prefixes plan: a uint8 tensor of round_up(total,
        8) bytes, one word when total is 0 (`out`, when given: a uint8 device tensor of any
        alignment and at least round_up(total, 8) bytes)."""
        import torch
        if out is None:
            out = torch.empty(max((total + 7) // 8 * 8, 8), dtype=torch.uint8, device=self.dev)
        self._fail(LIB.s3imph_index_prefixes_fill(self._h, _dev_ptr(out), int(out.numel()), _stream_ptr(stream)),
                   "prefixes fill")
        return out

    def prefixes_device(self, pos, stream=None):
        """PrefixString (index.go:179) for a batch of positions (a sequence, or a device tensor such as
        descendants_fill's output): (out_offsets int64[nq + 1], found int32[nq], out_bytes uint8),
        all on the device; row q is out_bytes[out_offsets[q]:out_offsets[q + 1]], and (out_bytes,
        out_offsets) goes straight back into lookup_device."""
        offs, found, total = self.prefixes_plan(pos, stream)
        return offs, found, self.prefixes_fill(total, stream=stream)

    def prefix_strings(self, pos) -> list:
        """PrefixString per position as bytes; None where the reference returns ErrBoundsCheck."""
        offs, found, out = self.prefixes_device(pos)
        o, f, b = offs.cpu().numpy(), found.cpu().numpy(), out.cpu().numpy().tobytes()
        return [b[o[q]:o[q + 1]] if f[q] else None for q in range(len(f))]

    def lookup_verify_device(self, d_blob, d_offsets, nq: int, stream=None):
        """s3imph_index_lookup_verify_device over a query blob in HBM: as lookup_device, 2^64-1
        unless the stored prefix at the position equals the query."""
        import torch
        res = torch.empty(max(nq, 1), dtype=torch.int64, device=self.dev)
        self._fail(LIB.s3imph_index_lookup_verify_device(self._h, _dev_ptr(d_blob), _dev_ptr(d_offsets), nq,
                                                         _dev_ptr(res), _stream_ptr(stream)), "lookup verify")
        return res[:nq]

    def lookup_verify(self, keys) -> np.ndarray:
        """LookupWithVerify (mphf.go:306-320) of a batch: pos per key, or 2^64-1."""
        return self.lookup_verify_device(*self._keys_dev(*keys_to_blob(keys))).cpu().numpy().view(np.uint64)

    def verify_device(self, stream=None) -> tuple:
        """s3imph_index_verify_device: (n_bad, first_bad, first_got)."""
        r = [ctypes.c_uint64() for _ in range(3)]
        self._fail(LIB.s3imph_index_verify_device(self._h, ctypes.byref(r[0]), ctypes.byref(r[1]), ctypes.byref(r[2]),
                                                  _stream_ptr(stream)), "verify")
        return tuple(int(v.value) for v in r)

    def verify(self) -> None:
        """VerifyMPHF (mphf.go:372-393): raises MPHFError(ERR_INTERNAL) with the reference's text for
        the first stored prefix that does not look up to its own index."""
        n_bad, i, got = self.verify_device()
        if n_bad == 0:
            return
        q = _go_quote(self.prefix_strings([i])[0])
        if got == (1 << 64) - 1:
            raise MPHFError(ERR_INTERNAL, f"lookup failed for prefix {q} at pos {i}")
        raise MPHFError(ERR_INTERNAL, f"lookup returned wrong pos for {q}: got {got}, want {i}")

    def close(self) -> None:
        if getattr(self, "_h", None):
            LIB.s3imph_index_close(self._h)
            self._h = None
            self._keep = None
            self._keep_prefixes = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dist_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(128)
    _check(LIB.s3imph_dist_unique_id(buf), None, "ncclGetUniqueId")
    return buf.raw


class DistBuilder(DeviceBuilder):
    """One rank of a multi-GPU build.  Collectives: RCCL (the library owns the
    communicator; `unique_id` from rank 0's dist_unique_id()), or, with `host_comm`,
    the given torch.distributed process group on host copies (test transport:
    several ranks may share one GPU)."""

    def __init__(self, device: int, unique_id: bytes | None, rank: int, nranks: int, host_comm=None):
        err = ctypes.create_string_buffer(512)
        h = ctypes.c_void_p()
        if host_comm is None:
            idbuf = ctypes.create_string_buffer(unique_id, 128)
            _check(LIB.s3imph_ctx_create_dist(device, idbuf, rank, nranks, ctypes.byref(h), err, 512), err)
        else:
            self._comm = _TorchHostComm(None if host_comm is True else host_comm, nranks)
            _check(LIB.s3imph_ctx_create_dist_host(device, ctypes.byref(self._comm.cstruct), rank, nranks,
                                                   ctypes.byref(h), err, 512), err)
        self._h = h
        self.device = device
        self.rank, self.nranks = rank, nranks
        self.last_info = None

    def out_cap(self, n_global: int) -> int:
        return LIB.s3imph_dist_out_cap(self._h, n_global)

    def set_mode(self, mode: int) -> None:
        """DIST_ROUTE or DIST_BITMAP (every rank of a build must choose the same)."""
        _check(LIB.s3imph_ctx_set_dist_mode(self._h, mode), None, "set_dist_mode")

    def segments(self) -> list[tuple[int, int, int]]:
        """(global p, count, local offset) of this rank's outputs in the last build."""
        cnt = ctypes.c_uint64()
        LIB.s3imph_dist_segments(self._h, None, 0, ctypes.byref(cnt))
        buf = (ctypes.c_uint64 * max(3 * cnt.value, 1))()
        _check(LIB.s3imph_dist_segments(self._h, buf, cnt.value, ctypes.byref(cnt)), None, "segments")
        return [(buf[3 * i], buf[3 * i + 1], buf[3 * i + 2]) for i in range(cnt.value)]

    def build_shard(self, d_blob, d_offsets, n_local: int, key_base: int, d_fp_out, d_pos_out, out_cap: int,
                    d_pos=None, stream=None) -> tuple[int, list, dict]:
        """Build this rank's share; returns (local outputs, segments, info)."""
        info = BuildInfo()
        cnt = ctypes.c_uint64()
        rc = LIB.s3imph_build_device_dist(self._h, _dev_ptr(d_blob), _dev_ptr(d_offsets), _dev_ptr(d_pos),
                                          n_local, key_base, _dev_ptr(d_fp_out), _dev_ptr(d_pos_out), out_cap,
                                          ctypes.byref(cnt), _stream_ptr(stream), ctypes.byref(info))
        if rc != OK:
            raise MPHFError(rc, f"build MPHF (dist): {self.last_error() or status_string(rc)}")
        self.last_info = info.as_dict()
        return cnt.value, self.segments(), self.last_info


class _TorchHostComm:
    """s3imph_host_comm over a torch.distributed process group (gloo), CPU tensors."""

    def __init__(self, group, nranks: int):
        import torch.distributed as tdist
        self.group, self.nranks, self.dist = group, nranks, tdist
        self.cstruct = HostComm(None, ALLGATHER_FN(self._allgather), ALLTOALLV_FN(self._alltoallv))

    def _allgather(self, _user, send, recv, nbytes):
        try:
            src = torch.frombuffer((ctypes.c_uint8 * max(nbytes, 1)).from_address(send), dtype=torch.uint8)[:nbytes]
            out = torch.empty(nbytes * self.nranks, dtype=torch.uint8)
            self.dist.all_gather_into_tensor(out, src.clone(), group=self.group)
            if nbytes:
                ctypes.memmove(recv, out.data_ptr(), nbytes * self.nranks)
            return 0
        except Exception:  # noqa: BLE001 - reported to the library as a failed collective
            import traceback
            traceback.print_exc()
            return 1

    def _alltoallv(self, _user, send, soff, sbytes, recv, roff, rbytes):
        try:
            P = self.nranks
            sb = [sbytes[q] for q in range(P)]
            rb = [rbytes[q] for q in range(P)]
            st, rt = sum(sb), sum(rb)
            src = torch.empty(st, dtype=torch.uint8)
            for q in range(P):
                if sb[q]:
                    ctypes.memmove(src.data_ptr() + sum(sb[:q]), send + soff[q], sb[q])
            out = torch.empty(rt, dtype=torch.uint8)
            self.dist.all_to_all_single(out, src, rb, sb, group=self.group)
            for q in range(P):
                if rb[q]:
                    ctypes.memmove(recv + roff[q], out.data_ptr() + sum(rb[:q]), rb[q])
            return 0
        except Exception:  # noqa: BLE001
            import traceback
            traceback.print_exc()
            return 1


def assemble_dist(parts: list, n_global: int) -> tuple[np.ndarray, np.ndarray]:
    """Global (mph_fp, mph_pos) from every rank's (local fp, local pos, segments)."""
    fp = np.zeros(n_global, np.uint64)
    po = np.zeros(n_global, np.uint64)
    seen = np.zeros(n_global, bool)
    for lfp, lpo, segs in parts:
        for p0, cnt, off in segs:
            if seen[p0:p0 + cnt].any():
                raise ValueError("overlapping output segments")
            seen[p0:p0 + cnt] = True
            fp[p0:p0 + cnt] = lfp[off:off + cnt]
            po[p0:p0 + cnt] = lpo[off:off + cnt]
    if not seen.all():
        raise ValueError("output segments do not cover [0, N)")
    return fp, po


def _stream_ptr(stream):
    """hipStream_t for a call: an explicit stream, else torch's current stream when it is
    not the legacy default (the library's own stream is blocking, hence already ordered
    after work on the default stream)."""
    if stream is None:
        if torch is not None and torch.cuda.is_initialized():
            cur = torch.cuda.current_stream().cuda_stream
            return ctypes.c_void_p(cur) if cur else None
        return None
    if isinstance(stream, int):
        return ctypes.c_void_p(stream)
    return ctypes.c_void_p(stream.cuda_stream)


@contextlib.contextmanager
def _torch_on(stream, device):
    """The wrappers' own torch work (zero fills, conversions of host arguments, sizes read back)
    goes to the stream the library call is given: queued on torch's current stream it would be
    unordered with the library's work whenever ``stream=`` names another, non-blocking one."""
    if stream is None or torch is None:
        yield
        return
    if not isinstance(stream, torch.cuda.Stream):
        stream = torch.cuda.ExternalStream(int(stream), device=device)
    with torch.cuda.stream(stream):
        yield


@dataclass
class ShardPlan:
    """Contiguous key-index shard of a global prefix set, balanced by key count."""
    rank: int
    nranks: int
    n_global: int

    @property
    def lo(self) -> int:
        return self.n_global * self.rank // self.nranks

    @property
    def hi(self) -> int:
        return self.n_global * (self.rank + 1) // self.nranks

    @property
    def n_local(self) -> int:
        return self.hi - self.lo
