"""s3imph_index_open refuses a malformed index directory on the host, before any device call
(include/s3imph.h section 5c): this file runs without a GPU, so a case that got as far as
selecting a device would come back as a HIP error instead of the status asserted here.
Error texts follow indexread.Open (pkg/indexread/index.go:31-86)."""
import os
import shutil
import struct

import numpy as np
import pytest

import oracle as O
import s3imph
from index_dirs import write_index_dir

KEYS = [b"", b"a/", b"a/b/", b"b/", b"c/"]
N = len(KEYS)


@pytest.fixture(scope="module")
def valid_dir(tmp_path_factory, oracle_lib):
    d = tmp_path_factory.mktemp("index")
    arr = write_index_dir(d, oracle_lib, KEYS)
    assert arr["max_depth"] == 2
    return d


def _u64(path):
    return np.array(s3imph.read_array(str(path), 8), dtype=np.uint64)


def _u32(path):
    return np.array(s3imph.read_array(str(path), 4), dtype=np.uint32)


def _put(path, data):
    with open(path, "wb") as f:
        f.write(data)


def _remove(name):
    return lambda d: os.remove(d / name)


def _wrong_magic(d):
    raw = bytearray((d / "subtree_end.u64").read_bytes())
    raw[0:4] = struct.pack("<I", 0x12345678)
    _put(d / "subtree_end.u64", bytes(raw))


def _width4(d):
    # a well-formed width-4 array where the reader expects width 8
    _put(d / "subtree_end.u64", O.s3id_u32_array(_u64(d / "subtree_end.u64")))


def _depth_short(d):
    _put(d / "depth.u32", O.s3id_u32_array(_u32(d / "depth.u32")[:-1]))


def _fp_pos_differ(d):
    _put(d / "mph_pos.u64", O.s3id_u64_array(_u64(d / "mph_pos.u64")[:-1]))


def _offsets_decrease(d):
    o = _u64(d / "depth_offsets.u64")  # [0, 1, 4, 5]
    o[1], o[2] = o[2], o[1]
    _put(d / "depth_offsets.u64", O.s3id_u64_array(o))


def _offsets_end(d):
    o = _u64(d / "depth_offsets.u64")
    o[-1] -= 1
    _put(d / "depth_offsets.u64", O.s3id_u64_array(o))


def _depth_too_deep(d):
    v = _u32(d / "depth.u32")
    v[2] = 3  # maxDepth + 1
    _put(d / "depth.u32", O.s3id_u32_array(v))


def _dpos_is_n(d):
    v = _u64(d / "depth_positions.u64")
    v[-1] = N
    _put(d / "depth_positions.u64", O.s3id_u64_array(v))


def _mph_pos_is_n(d):
    v = _u64(d / "mph_pos.u64")
    v[1] = N
    _put(d / "mph_pos.u64", O.s3id_u64_array(v))


def _stats_short(d):
    _put(d / "object_count.u64", O.s3id_u64_array(np.arange(N - 1, dtype=np.uint64)))
    _put(d / "total_bytes.u64", O.s3id_u64_array(np.arange(N, dtype=np.uint64)))


def _mph_truncated(d):
    _put(d / "mph.bin", (d / "mph.bin").read_bytes()[:-3])


CASES = [
    ("missing_subtree_end", _remove("subtree_end.u64"), s3imph.ERR_IO, "open subtree_end"),
    ("missing_depth_positions", _remove("depth_positions.u64"), s3imph.ERR_IO, "open depth index"),
    ("wrong_magic", _wrong_magic, s3imph.ERR_FORMAT, "open subtree_end"),
    ("width_4_for_8", _width4, s3imph.ERR_FORMAT, "open subtree_end"),
    ("depth_one_short", _depth_short, s3imph.ERR_FORMAT, "open depth"),
    ("fp_pos_counts_differ", _fp_pos_differ, s3imph.ERR_FORMAT, "open MPHF"),
    ("depth_offsets_decreasing", _offsets_decrease, s3imph.ERR_FORMAT, "open depth index"),
    ("depth_offsets_end", _offsets_end, s3imph.ERR_FORMAT, "open depth index"),
    ("depth_above_max_depth", _depth_too_deep, s3imph.ERR_FORMAT, "open depth"),
    ("depth_position_is_n", _dpos_is_n, s3imph.ERR_FORMAT, "open depth index"),
    ("mph_pos_is_n", _mph_pos_is_n, s3imph.ERR_FORMAT, "open MPHF"),
    ("object_count_one_short", _stats_short, s3imph.ERR_FORMAT, "open object_count"),
    ("mph_bin_truncated", _mph_truncated, s3imph.ERR_FORMAT, "open MPHF"),
]


@pytest.mark.parametrize("name,damage,status,prefix", CASES, ids=[c[0] for c in CASES])
def test_open_refuses_on_the_host(valid_dir, tmp_path, name, damage, status, prefix):
    d = tmp_path / "idx"
    shutil.copytree(valid_dir, d)
    damage(d)
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.Index(str(d))
    assert e.value.status == status, str(e.value)
    assert str(e.value).startswith(prefix + ": "), str(e.value)


def test_valid_directory_passes_host_validation(valid_dir):
    """The undamaged directory gets past every host check: what stops it here, if anything,
    is the device (this file runs on machines without one)."""
    try:
        idx = s3imph.Index(str(valid_dir))
    except s3imph.MPHFError as e:
        assert e.status == s3imph.ERR_HIP, str(e)
    else:
        assert idx.count == N and idx.max_depth == 2
        idx.close()


def test_null_arguments():
    import ctypes
    h = ctypes.c_void_p()
    assert s3imph.LIB.s3imph_index_open(0, None, ctypes.byref(h), None, 0) == s3imph.ERR_INVALID
    assert s3imph.LIB.s3imph_index_attach(0, None, ctypes.byref(h), None, 0) == s3imph.ERR_INVALID
    assert s3imph.LIB.s3imph_index_close(None) == s3imph.OK
    assert s3imph.LIB.s3imph_index_count(None) == 0
    assert s3imph.LIB.s3imph_index_descendants_fill(None, None, 0, None) == s3imph.ERR_INVALID
