"""s3imph_index_open_flags(S3IMPH_OPEN_PREFIXES) refuses malformed prefix files on the host, before
any device call (include/s3imph.h section 5c): this file runs without a GPU, so a case that got as
far as selecting a device would come back as a HIP error instead of the status asserted here.
Error texts follow OpenMPHF / OpenBlob (pkg/format/mphf.go:226-238, reader.go:213-229); what the
reference checks per Get (reader.go:250-270) is checked once at open."""
import ctypes
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
BLOB_SIZE = sum(len(k) for k in KEYS)
PREFIX = "open MPHF: open prefix blob: "


@pytest.fixture(scope="module")
def valid_dir(tmp_path_factory, oracle_lib):
    d = tmp_path_factory.mktemp("index")
    write_index_dir(d, oracle_lib, KEYS)
    assert os.path.getsize(d / "prefix_blob.bin") == BLOB_SIZE
    return d


def _offsets(d):
    return np.array(s3imph.read_array(str(d / "prefix_offsets.u64"), 8), dtype=np.uint64)


def _put(path, data):
    with open(path, "wb") as f:
        f.write(data)


def _missing(d):
    os.remove(d / "prefix_offsets.u64")


def _wrong_magic(d):
    raw = bytearray((d / "prefix_offsets.u64").read_bytes())
    raw[0:4] = struct.pack("<I", 0x12345678)
    _put(d / "prefix_offsets.u64", bytes(raw))


def _width4(d):
    _put(d / "prefix_offsets.u64", O.s3id_u32_array(_offsets(d)))


def _one_short(d):
    _put(d / "prefix_offsets.u64", O.s3id_u64_array(_offsets(d)[:-1]))


def _one_more(d):
    o = _offsets(d)
    _put(d / "prefix_offsets.u64", O.s3id_u64_array(np.append(o, o[-1])))


def _decreasing(d):
    o = _offsets(d)  # [0, 0, 2, 6, 8, 10]
    o[2], o[3] = o[3], o[2]
    _put(d / "prefix_offsets.u64", O.s3id_u64_array(o))


def _past_the_blob(d):
    o = _offsets(d)
    o[-1] = BLOB_SIZE + 1
    _put(d / "prefix_offsets.u64", O.s3id_u64_array(o))


CASES = [
    ("offsets_missing", _missing, s3imph.ERR_IO),
    ("wrong_magic", _wrong_magic, s3imph.ERR_FORMAT),
    ("width_4", _width4, s3imph.ERR_FORMAT),
    ("n_entries", _one_short, s3imph.ERR_FORMAT),
    ("n_plus_2_entries", _one_more, s3imph.ERR_FORMAT),
    ("one_decreasing_pair", _decreasing, s3imph.ERR_FORMAT),
    ("last_offset_past_the_blob", _past_the_blob, s3imph.ERR_FORMAT),
]


def _opens_or_stops_at_the_device(d, prefixes):
    """Past every host check: what stops the open here, if anything, is the device."""
    try:
        idx = s3imph.Index(str(d), prefixes=prefixes)
    except s3imph.MPHFError as e:
        assert e.status == s3imph.ERR_HIP, str(e)
        return None
    assert idx.count == N
    return idx


@pytest.mark.parametrize("name,damage,status", CASES, ids=[c[0] for c in CASES])
def test_open_flags_refuses_on_the_host(valid_dir, tmp_path, name, damage, status):
    d = tmp_path / "idx"
    shutil.copytree(valid_dir, d)
    damage(d)
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.Index(str(d), prefixes=True)
    assert e.value.status == status, str(e.value)
    text = str(e.value)
    assert text.startswith(PREFIX), text
    if name in ("offsets_missing", "wrong_magic", "width_4"):
        assert text.startswith(PREFIX + "open offsets: "), text


@pytest.mark.parametrize("damage", [_wrong_magic, _one_short, _decreasing], ids=["magic", "short", "decreasing"])
def test_offsets_are_not_examined_without_the_blob(valid_dir, tmp_path, damage):
    """OpenMPHF stats the blob first (mphf.go:231): no blob, no prefixes, whatever the offsets hold."""
    d = tmp_path / "idx"
    shutil.copytree(valid_dir, d)
    damage(d)
    os.remove(d / "prefix_blob.bin")
    idx = _opens_or_stops_at_the_device(d, True)
    if idx is not None:
        assert not idx.has_prefixes()
        idx.close()


@pytest.mark.parametrize("damage", [_missing, _wrong_magic, _past_the_blob], ids=["missing", "magic", "past"])
def test_flags_0_does_not_read_the_prefix_files(valid_dir, tmp_path, damage):
    d = tmp_path / "idx"
    shutil.copytree(valid_dir, d)
    damage(d)
    h = ctypes.c_void_p()
    err = ctypes.create_string_buffer(1024)
    rc = s3imph.LIB.s3imph_index_open_flags(0, os.fsencode(str(d)), 0, ctypes.byref(h), err, 1024)
    assert rc in (s3imph.OK, s3imph.ERR_HIP), err.value
    if rc == s3imph.OK:
        assert s3imph.LIB.s3imph_index_has_prefixes(h) == 0
        s3imph.LIB.s3imph_index_close(h)
    idx = _opens_or_stops_at_the_device(d, False)
    if idx is not None:
        idx.close()


def test_valid_directory_and_allowed_slack_pass_host_validation(valid_dir, tmp_path):
    """offsets[0] != 0 and bytes after the last offset are allowed, as in the reference."""
    idx = _opens_or_stops_at_the_device(valid_dir, True)
    if idx is not None:
        assert idx.has_prefixes()
        idx.close()
    d = tmp_path / "idx"
    shutil.copytree(valid_dir, d)
    _put(d / "prefix_blob.bin", b"##" + (d / "prefix_blob.bin").read_bytes() + b"slack")
    _put(d / "prefix_offsets.u64", O.s3id_u64_array(_offsets(d) + np.uint64(2)))
    idx = _opens_or_stops_at_the_device(d, True)
    if idx is not None:
        idx.close()


def test_empty_index_opens_with_prefixes(tmp_path, oracle_lib):
    write_index_dir(tmp_path, oracle_lib, [])
    assert (tmp_path / "prefix_blob.bin").read_bytes() == b""
    try:
        idx = s3imph.Index(str(tmp_path), prefixes=True)
    except s3imph.MPHFError as e:
        assert e.status == s3imph.ERR_HIP, str(e)
    else:
        assert idx.count == 0 and idx.has_prefixes()
        idx.close()
