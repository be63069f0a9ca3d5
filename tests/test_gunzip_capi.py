"""Section 5j of the C ABI (gzip files inflated on the GPU, the index from .csv.gz files) without a
GPU: the symbols are exported, declared and bound, the info struct has its declared layout, the
room hint follows its rule, and null, non-monotonic or missing-directory arguments are refused
before any device is touched."""
import ctypes
import gzip
import os
import re
import struct

import numpy as np

import s3imph
from conftest import ROOT

NEW = ("s3imph_gunzip_geometry", "s3imph_gunzip_room_hint", "s3imph_gunzip_device", "s3imph_gunzip_host",
       "s3imph_index_from_csv_gz_host", "s3imph_rowset_add_csv_gz")


def test_symbols_exported_declared_and_bound():
    lib = ctypes.CDLL(s3imph.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "s3imph.h")).read()
    declared = set(re.findall(r"^(?:int|void|uint64_t) (s3imph_[a-z0-9_]+)\(", src, re.M))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in s3imph.EXPORTS and name in declared
        assert getattr(s3imph.LIB, name).argtypes is not None
    for name in ("GunzipInfo", "gunzip_geometry", "gunzip_room_hint", "gunzip", "build_index_from_inventory_csv_gz"):
        assert hasattr(s3imph, name)
    assert callable(s3imph.DeviceBuilder.gunzip) and callable(s3imph.RowSet.add_csv_gz)
    assert s3imph.LIB.s3imph_abi_version() == 1 and "S3IMPH_ABI_VERSION 1" in src
    assert "the caller inflates" not in src
    for k, name in enumerate(("OK", "MORE", "EOF", "HEADER", "DATA", "CHECKSUM")):
        assert getattr(s3imph, "GZ_" + name) == k and re.search(r"S3IMPH_GZ_%s = %d\b" % (name, k), src)


def test_info_layout():
    I = s3imph.GunzipInfo
    assert ctypes.sizeof(I) == 32
    assert [getattr(I, f).offset for f in ("out_bytes", "in_used", "members", "status", "crc32", "reserved")] == \
        [0, 8, 16, 20, 24, 28]


def test_geometry_is_positive():
    chunk, batch, waves = s3imph.gunzip_geometry()
    assert chunk > 0 and batch > 0 and waves > 0
    s3imph.LIB.s3imph_gunzip_geometry(None, None, None)  # each pointer may be null


def test_room_hint():
    text = b"k/%d,1\n" * 100 % tuple(range(100))
    data = gzip.compress(text)
    assert s3imph.gunzip_room_hint(data) == len(text)
    lying = data[:-4] + struct.pack("<I", 0xFFFFFFF0)
    assert s3imph.gunzip_room_hint(lying) == 1032 * len(lying) + 64
    assert s3imph.gunzip_room_hint(data[:-4] + struct.pack("<I", 7)) == 7
    assert s3imph.gunzip_room_hint(b"\x1f\x8b" + b"\xff" * 15) == 0  # 17 bytes
    assert s3imph.gunzip_room_hint(b"\x1f\x8b" + b"\0" * 12 + struct.pack("<I", 9)) == 9  # 18 bytes
    assert s3imph.gunzip_room_hint(b"") == 0
    assert s3imph.LIB.s3imph_gunzip_room_hint(None, 100) == 0


def _args():
    gz = np.frombuffer(gzip.compress(b"a,1\n"), np.uint8).copy()
    return gz, ctypes.c_void_p(gz.ctypes.data), s3imph.CsvSchema(0, 1, -1, -1)


def test_device_call_refuses_bad_arguments_before_any_device_work():
    L = s3imph.LIB
    gz, gp, _ = _args()
    offs = (ctypes.c_uint64 * 3)(0, 10, 20)
    back = (ctypes.c_uint64 * 3)(0, 10, 9)
    info = (s3imph.GunzipInfo * 2)()
    assert L.s3imph_gunzip_device(None, gp, offs, 2, gp, offs, info, None) == s3imph.ERR_INVALID
    # the ctx is checked first and never touched: a made-up non-null one does
    fake = ctypes.c_void_p(8)
    assert L.s3imph_gunzip_device(fake, None, offs, 2, gp, offs, info, None) == s3imph.ERR_INVALID
    assert L.s3imph_gunzip_device(fake, gp, None, 2, gp, offs, info, None) == s3imph.ERR_INVALID
    assert L.s3imph_gunzip_device(fake, gp, offs, 2, None, offs, info, None) == s3imph.ERR_INVALID
    assert L.s3imph_gunzip_device(fake, gp, offs, 2, gp, None, info, None) == s3imph.ERR_INVALID
    assert L.s3imph_gunzip_device(fake, gp, offs, 2, gp, offs, None, None) == s3imph.ERR_INVALID
    assert L.s3imph_gunzip_device(fake, gp, back, 2, gp, offs, info, None) == s3imph.ERR_INVALID
    assert L.s3imph_gunzip_device(fake, gp, offs, 2, gp, back, info, None) == s3imph.ERR_INVALID
    assert L.s3imph_gunzip_device(fake, gp, offs, 1 << 31, gp, offs, info, None) == s3imph.ERR_INVALID
    # no file: nothing to do, and nothing is read
    assert L.s3imph_gunzip_device(fake, None, None, 0, None, None, None, None) == s3imph.OK


def test_host_calls_refuse_bad_arguments_before_any_device_work(tmp_path):
    L = s3imph.LIB
    gz, gp, sch = _args()
    err = ctypes.create_string_buffer(256)
    ptrs = (ctypes.c_void_p * 1)(gz.ctypes.data)
    nulls = (ctypes.c_void_p * 1)(None)
    lens = (ctypes.c_uint64 * 1)(len(gz))
    outs = (ctypes.c_void_p * 1)()
    out_len = (ctypes.c_uint64 * 1)()
    f = L.s3imph_gunzip_host
    assert f(0, None, lens, 1, outs, out_len, None, err, 256) == s3imph.ERR_INVALID
    assert f(0, ptrs, None, 1, outs, out_len, None, err, 256) == s3imph.ERR_INVALID
    assert f(0, ptrs, lens, 1, None, out_len, None, err, 256) == s3imph.ERR_INVALID
    assert f(0, ptrs, lens, 1, outs, None, None, err, 256) == s3imph.ERR_INVALID
    assert f(0, nulls, lens, 1, outs, out_len, None, err, 256) == s3imph.ERR_INVALID
    assert outs[0] is None
    assert f(0, None, None, 0, None, None, None, err, 256) == s3imph.OK
    assert s3imph.gunzip([]) == []

    g = L.s3imph_index_from_csv_gz_host
    d = str(tmp_path).encode()
    s = ctypes.byref(sch)
    assert g(0, ptrs, lens, 1, None, 0, 0, 0, d, None, err, 256) == s3imph.ERR_INVALID
    assert g(0, ptrs, lens, 1, s, 0, 0, 0, None, None, err, 256) == s3imph.ERR_INVALID
    assert g(0, None, lens, 1, s, 0, 0, 0, d, None, err, 256) == s3imph.ERR_INVALID
    assert g(0, ptrs, None, 1, s, 0, 0, 0, d, None, err, 256) == s3imph.ERR_INVALID
    assert g(0, nulls, lens, 1, s, 0, 0, 0, d, None, err, 256) == s3imph.ERR_INVALID
    for bad in (s3imph.CsvSchema(-1, 1, -1, -1), s3imph.CsvSchema(0, -1, -1, -1)):
        assert g(0, ptrs, lens, 1, ctypes.byref(bad), 0, 0, 0, d, None, err, 256) == s3imph.ERR_INVALID
    # a missing directory is an I/O error, found before the device is selected
    rc = g(0, ptrs, lens, 1, s, 0, 0, 0, str(tmp_path / "nope").encode(), None, err, 256)
    assert rc == s3imph.ERR_IO and b"no such directory" in err.value
    assert os.listdir(tmp_path) == []

    h = L.s3imph_rowset_add_csv_gz
    assert h(None, ptrs, lens, 1, s, 0, err, 256) == s3imph.ERR_INVALID
    with s3imph.RowSet() as rs:
        assert h(rs._h, ptrs, lens, 1, None, 0, err, 256) == s3imph.ERR_INVALID
        assert h(rs._h, None, lens, 1, s, 0, err, 256) == s3imph.ERR_INVALID
        assert h(rs._h, ptrs, None, 1, s, 0, err, 256) == s3imph.ERR_INVALID
        assert h(rs._h, nulls, lens, 1, s, 0, err, 256) == s3imph.ERR_INVALID
        assert h(rs._h, ptrs, lens, 1, ctypes.byref(s3imph.CsvSchema(0, -1, -1, -1)), 0, err, 256) == s3imph.ERR_INVALID
        rs.add_csv_gz([], (0, 1, -1, -1))  # no file: no run, no device
        assert rs.runs == 0


def test_no_file_builds_the_empty_index_without_a_gpu(tmp_path):
    """n_files == 0: the empty index, as the CSV call writes it for no buffer."""
    for with_tiers in (False, True):
        d = tmp_path / str(with_tiers)
        d.mkdir()
        total = s3imph.build_index_from_inventory_csv_gz([], (0, 1, 2, 3), str(d), with_tiers=with_tiers)
        assert total["n_objects"] == 0 and total["n_records"] == 0
        assert (d / "mph.bin").read_bytes() == b""
        assert list(s3imph.read_u64_array(str(d / "depth_offsets.u64"))) == [0, 0]
        s3imph.verify_manifest(str(d))
        assert s3imph.read_manifest(str(d))["node_count"] == 0
        assert not (d / "tiers.json").exists()
