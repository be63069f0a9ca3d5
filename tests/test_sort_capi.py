"""Section 5f of the C ABI (listing sort, gather, index from an unsorted listing) without a GPU:
the symbols are exported, declared and bound, and null, short or mismatched arguments are refused
before any device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

import s3imph
from conftest import ROOT

NEW = ("s3imph_sort_objects_device", "s3imph_gather_objects_device", "s3imph_sort_objects_host",
       "s3imph_index_from_unsorted_objects_host")


def _declared():
    src = open(os.path.join(ROOT, "include", "s3imph.h")).read()
    return set(re.findall(r"^int (s3imph_[a-z0-9_]+)\(", src, re.M))


def test_symbols_exported_declared_and_bound():
    lib = ctypes.CDLL(s3imph.LIB_PATH)
    declared = _declared()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in s3imph.EXPORTS and name in declared
        f = getattr(s3imph.LIB, name)
        assert f.argtypes is not None and f.restype is ctypes.c_int
    for name in ("sort_objects", "build_index_from_unsorted_objects"):
        assert callable(getattr(s3imph, name))
    for name in ("sort_objects", "gather_objects"):
        assert callable(getattr(s3imph.DeviceBuilder, name))
    assert s3imph.LIB.s3imph_abi_version() == 1


def test_sort_info_layout():
    """s3imph_sort_info: four u64, then rounds and a pad — 40 bytes."""
    S = s3imph.SortInfo
    assert ctypes.sizeof(S) == 40
    assert [getattr(S, f).offset for f in ("n_objects", "key_bytes", "first_unsorted", "n_equal", "rounds", "pad")] \
        == [0, 8, 16, 24, 32, 36]
    assert set(S().as_dict()) == {"n_objects", "key_bytes", "first_unsorted", "n_equal", "rounds"}


def _one_key():
    keys = np.frombuffer(b"a/b", np.uint8).copy()
    offs = np.array([0, 3], np.uint64)
    return keys, offs, ctypes.c_void_p(keys.ctypes.data), ctypes.c_void_p(offs.ctypes.data)


def test_device_calls_refuse_null_arguments():
    L = s3imph.LIB
    info = s3imph.SortInfo()
    keys, offs, kp, op = _one_key()
    assert L.s3imph_sort_objects_device(None, kp, op, 1, kp, ctypes.byref(info), None) == s3imph.ERR_INVALID
    assert L.s3imph_sort_objects_device(None, None, None, 0, None, ctypes.byref(info), None) == s3imph.ERR_INVALID
    assert L.s3imph_sort_objects_device(None, None, None, 0, None, None, None) == s3imph.ERR_INVALID
    assert L.s3imph_gather_objects_device(None, kp, op, None, None, 1, kp, kp, 8, op, None, None, None) \
        == s3imph.ERR_INVALID
    assert L.s3imph_gather_objects_device(None, None, None, None, None, 0, None, None, 0, None, None, None, None) \
        == s3imph.ERR_INVALID
    # one of a pair without the other, whichever one
    for args in ((op, None, None, None), (None, None, op, None), (None, kp, None, None), (None, None, None, kp)):
        d_sizes, d_tiers, d_sizes_out, d_tiers_out = args
        assert L.s3imph_gather_objects_device(None, kp, op, d_sizes, d_tiers, 1, kp, kp, 8, op, d_sizes_out,
                                              d_tiers_out, None) == s3imph.ERR_INVALID


def test_host_calls_refuse_null_and_short_arguments(tmp_path):
    L = s3imph.LIB
    err = ctypes.create_string_buffer(256)
    info = s3imph.SortInfo()
    keys, offs, kp, op = _one_key()
    order = ctypes.c_void_p()
    assert L.s3imph_sort_objects_host(0, kp, op, 1, None, ctypes.byref(info), err, 256) == s3imph.ERR_INVALID
    assert L.s3imph_sort_objects_host(0, kp, op, 1, ctypes.byref(order), None, err, 256) == s3imph.ERR_INVALID
    # keys announced but not given
    assert L.s3imph_sort_objects_host(0, None, op, 1, ctypes.byref(order), ctypes.byref(info), err, 256) \
        == s3imph.ERR_INVALID
    assert L.s3imph_sort_objects_host(0, kp, None, 1, ctypes.byref(order), ctypes.byref(info), err, 256) \
        == s3imph.ERR_INVALID
    assert order.value is None
    d = str(tmp_path).encode()
    f = L.s3imph_index_from_unsorted_objects_host
    assert f(0, kp, op, None, None, 1, 0, None, err, 256) == s3imph.ERR_INVALID
    assert f(0, None, op, None, None, 1, 0, d, err, 256) == s3imph.ERR_INVALID
    assert f(0, kp, None, None, None, 1, 0, d, err, 256) == s3imph.ERR_INVALID
    # a missing directory is an I/O error, found before the device is selected
    rc = f(0, kp, op, None, None, 1, 0, str(tmp_path / "nope").encode(), err, 256)
    assert rc == s3imph.ERR_IO and b"no such directory" in err.value


def test_2_to_the_32_objects_are_refused_before_any_device_work(tmp_path):
    """The order is a uint32_t: m >= 2^32 is ERR_INVALID, whatever else is passed."""
    L = s3imph.LIB
    err = ctypes.create_string_buffer(256)
    info = s3imph.SortInfo()
    keys, offs, kp, op = _one_key()
    order = ctypes.c_void_p()
    m = 1 << 32
    assert L.s3imph_sort_objects_host(0, kp, op, m, ctypes.byref(order), ctypes.byref(info), err, 256) \
        == s3imph.ERR_INVALID
    assert L.s3imph_sort_objects_device(None, kp, op, m, kp, ctypes.byref(info), None) == s3imph.ERR_INVALID
    assert L.s3imph_gather_objects_device(None, kp, op, None, None, m, kp, kp, 8, op, None, None, None) \
        == s3imph.ERR_INVALID
    rc = L.s3imph_index_from_unsorted_objects_host(0, kp, op, None, None, m, 0, str(tmp_path).encode(), err, 256)
    assert rc == s3imph.ERR_INVALID and err.value.startswith(b"sort: ")


def test_sizes_and_tiers_must_match_the_keys(tmp_path):
    with pytest.raises(ValueError):
        s3imph.build_index_from_unsorted_objects(np.zeros(3, np.uint8), np.array([0, 3], np.uint64),
                                                 np.zeros(2, np.uint64), str(tmp_path))
    with pytest.raises(ValueError):
        s3imph.build_index_from_unsorted_objects(np.zeros(3, np.uint8), np.array([0, 3], np.uint64), None,
                                                 str(tmp_path), tiers=np.zeros(2, np.uint8))


def test_empty_listing_needs_no_gpu(tmp_path):
    """m == 0: no order; the directory is the empty index verify_manifest accepts."""
    order, info = s3imph.sort_objects(np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert order.dtype == np.uint32 and len(order) == 0
    assert info == {"n_objects": 0, "key_bytes": 0, "first_unsorted": 2**64 - 1, "n_equal": 0, "rounds": 0}
    for sub, tiers in (("plain", None), ("tiers", np.zeros(0, np.uint8))):
        d = tmp_path / sub
        d.mkdir()
        s3imph.build_index_from_unsorted_objects(np.zeros(0, np.uint8), np.zeros(1, np.uint64), None, str(d),
                                                 tiers=tiers)
        assert (d / "mph.bin").read_bytes() == b""
        for name in ("object_count.u64", "total_bytes.u64", "mph_fp.u64", "subtree_end.u64"):
            assert len(s3imph.read_u64_array(str(d / name))) == 0
        assert list(s3imph.read_u64_array(str(d / "depth_offsets.u64"))) == [0, 0]
        s3imph.verify_manifest(str(d))
        assert s3imph.read_manifest(str(d))["node_count"] == 0
        assert not (d / "tiers.json").exists()
