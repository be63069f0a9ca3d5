"""Section 5d of the C ABI (prefix aggregation, index from objects) without a GPU: the symbols
are exported and declared, and null or short arguments are refused before any device is
touched."""
import ctypes

import numpy as np

import s3imph

NEW = ("s3imph_aggregate_plan_device", "s3imph_aggregate_fill_device", "s3imph_aggregate_host",
       "s3imph_index_from_objects_host")


def test_symbols_exported_and_bound():
    lib = ctypes.CDLL(s3imph.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in s3imph.EXPORTS
        assert getattr(s3imph.LIB, name).argtypes is not None
    for name in ("aggregate", "build_index_from_objects"):
        assert callable(getattr(s3imph, name))
    for name in ("aggregate_plan", "aggregate_fill"):
        assert callable(getattr(s3imph.DeviceBuilder, name))


def test_agg_info_layout():
    """s3imph_agg_info: five u64, then max_depth_seen and a pad — 48 bytes."""
    assert ctypes.sizeof(s3imph.AggInfo) == 48
    assert s3imph.AggInfo.first_unsorted.offset == 32 and s3imph.AggInfo.max_depth_seen.offset == 40


def test_device_calls_refuse_null_arguments():
    info = s3imph.AggInfo()
    L = s3imph.LIB
    assert L.s3imph_aggregate_plan_device(None, None, None, None, 0, 0, ctypes.byref(info), None) == s3imph.ERR_INVALID
    assert L.s3imph_aggregate_fill_device(None, None, 0, None, None, None, None, 0, None) == s3imph.ERR_INVALID


def test_host_calls_refuse_null_and_short_arguments(tmp_path):
    L = s3imph.LIB
    err = ctypes.create_string_buffer(256)
    keys = np.frombuffer(b"a/b", np.uint8).copy()
    offs = np.array([0, 3], np.uint64)
    kp, op = ctypes.c_void_p(keys.ctypes.data), ctypes.c_void_p(offs.ctypes.data)
    out = [ctypes.c_void_p() for _ in range(5)]
    n = ctypes.c_uint64()
    refs = [ctypes.byref(p) for p in out]
    # a missing output pointer, whichever one
    for hole in range(5):
        args = list(refs)
        args[hole] = None
        assert L.s3imph_aggregate_host(0, kp, op, None, 1, 0, *args, ctypes.byref(n), err, 256) == s3imph.ERR_INVALID
    assert L.s3imph_aggregate_host(0, kp, op, None, 1, 0, *refs, None, err, 256) == s3imph.ERR_INVALID
    # keys announced but not given
    assert L.s3imph_aggregate_host(0, None, op, None, 1, 0, *refs, ctypes.byref(n), err, 256) == s3imph.ERR_INVALID
    assert L.s3imph_aggregate_host(0, kp, None, None, 1, 0, *refs, ctypes.byref(n), err, 256) == s3imph.ERR_INVALID
    d = str(tmp_path).encode()
    assert L.s3imph_index_from_objects_host(0, kp, op, None, 1, 0, None, err, 256) == s3imph.ERR_INVALID
    assert L.s3imph_index_from_objects_host(0, None, op, None, 1, 0, d, err, 256) == s3imph.ERR_INVALID
    assert L.s3imph_index_from_objects_host(0, kp, None, None, 1, 0, d, err, 256) == s3imph.ERR_INVALID
    assert all(p.value is None for p in out)
    # a missing directory is an I/O error, found before the device is selected
    rc = L.s3imph_index_from_objects_host(0, kp, op, None, 1, 0, str(tmp_path / "nope").encode(), err, 256)
    assert rc == s3imph.ERR_IO and b"no such directory" in err.value


def test_sizes_must_match_the_keys():
    import pytest
    with pytest.raises(ValueError):
        s3imph.aggregate(np.zeros(3, np.uint8), np.array([0, 3], np.uint64), np.zeros(2, np.uint64))


def test_empty_listing_needs_no_gpu(tmp_path):
    """m == 0: Drain returns nil — no rows, offsets = [0]; the directory is the empty index."""
    blob, offs, depth, cnt, tot = s3imph.aggregate(np.zeros(0, np.uint8), np.zeros(1, np.uint64), None)
    assert len(blob) == 0 and list(offs) == [0] and len(depth) == len(cnt) == len(tot) == 0
    s3imph.build_index_from_objects(np.zeros(0, np.uint8), np.zeros(1, np.uint64), None, str(tmp_path))
    assert (tmp_path / "mph.bin").read_bytes() == b""
    for name in ("object_count.u64", "total_bytes.u64", "mph_fp.u64", "subtree_end.u64"):
        assert len(s3imph.read_u64_array(str(tmp_path / name))) == 0
    assert list(s3imph.read_u64_array(str(tmp_path / "depth_offsets.u64"))) == [0, 0]
    s3imph.verify_manifest(str(tmp_path))
    assert s3imph.read_manifest(str(tmp_path))["node_count"] == 0
