"""Section 5g of the C ABI (inventory CSV -> object listing -> index) without a GPU: the symbols
are exported, declared and bound, the structs have their declared layout, the header row is read
as the reference reads it, and null, negative-column or missing-directory arguments are refused
before any device is touched."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import csv_ref as C
import s3imph
from conftest import GOLDEN, ROOT

NEW = ("s3imph_csv_header_schema", "s3imph_csv_plan_device", "s3imph_csv_fill_device", "s3imph_csv_parse_host",
       "s3imph_index_from_csv_host", "s3imph_csv_geometry")
CASES = json.load(open(os.path.join(GOLDEN, "csv", "cases.json")))


def test_symbols_exported_declared_and_bound():
    lib = ctypes.CDLL(s3imph.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "s3imph.h")).read()
    declared = set(re.findall(r"^(?:int|void) (s3imph_[a-z0-9_]+)\(", src, re.M))
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in s3imph.EXPORTS and name in declared
        assert getattr(s3imph.LIB, name).argtypes is not None
    for name in ("CsvInfo", "csv_header_schema", "parse_inventory_csv", "build_index_from_inventory_csv"):
        assert hasattr(s3imph, name)
    for name in ("csv_plan", "csv_fill"):
        assert callable(getattr(s3imph.DeviceBuilder, name))
    assert s3imph.LIB.s3imph_abi_version() == 1
    assert "S3IMPH_ABI_VERSION 1" in src
    assert "Host-only, no device call" not in src


def test_struct_layouts():
    I = s3imph.CsvInfo
    assert ctypes.sizeof(I) == 48
    assert [getattr(I, f).offset for f in ("n_records", "n_objects", "key_bytes", "n_short", "n_empty_key",
                                           "n_bad_size")] == [0, 8, 16, 24, 32, 40]
    S = s3imph.CsvSchema
    assert ctypes.sizeof(S) == 16
    assert [getattr(S, f).offset for f in ("key_col", "size_col", "storage_col", "access_tier_col")] == [0, 4, 8, 12]


def test_geometry_is_exported_for_the_boundary_tests():
    run, tile = s3imph.csv_geometry()
    assert run > 0 and tile % run == 0 and tile // run > 1 and tile % 16 == 0


def header_inputs():
    out = [(c["name"], c["csv"].encode()) for c in CASES["header"] + [t for t in CASES["tiers"] if t.get("header")]]
    out += [
        ("empty", b""), ("only_empty_lines", b"\n\r\n\n"), ("no_newline", b"Key,Size"),
        ("crlf", b"Key,Size\r\na,1\r\n"), ("duplicate_last_wins", b'key,"Si""ze",SIZE , storageclass,KEY\nx'),
        ("case_and_space", b" IntelligentTieringAccessTier\t,sIzE,\vkEy\f\r\nx"),
        ("quoted_names", b'"Key","Size","StorageClass"\n'), ("lazy_quote_in_name", b'Ke"y,Key,Size\n'),
        ("leading_empty_lines", b"\n\nkey,size\nz"), ("name_with_high_bytes", b"k\xc3\xa9y,key,size\n"),
    ]
    return out


HEADERS = header_inputs()


@pytest.mark.parametrize("name,data", HEADERS, ids=[h[0] for h in HEADERS])
def test_header_schema_follows_the_reference(name, data):
    want = C.header_schema(data)
    if isinstance(want, str):
        with pytest.raises(s3imph.MPHFError) as e:
            s3imph.csv_header_schema(data)
        assert str(e.value) == want and e.value.status == s3imph.ERR_FORMAT
    else:
        assert s3imph.csv_header_schema(data) == want


def test_header_error_texts_are_the_declared_ones():
    for data, text in ((b"Bucket,Size\nb,1\n", "CSV header missing 'Key' column"),
                       (b"Bucket,Key\nb,k\n", "CSV header missing 'Size' column"), (b"", "read CSV header: EOF")):
        with pytest.raises(s3imph.MPHFError) as e:
            s3imph.csv_header_schema(data)
        assert str(e.value) == text


def _args():
    csv = np.frombuffer(b"a,1\n", np.uint8).copy()
    return csv, ctypes.c_void_p(csv.ctypes.data), s3imph.CsvSchema(0, 1, -1, -1), s3imph.CsvInfo()


def test_header_schema_refuses_null_arguments():
    L = s3imph.LIB
    csv, cp, sch, _ = _args()
    start = ctypes.c_uint64()
    err = ctypes.create_string_buffer(256)
    assert L.s3imph_csv_header_schema(cp, 4, None, ctypes.byref(start), err, 256) == s3imph.ERR_INVALID
    assert L.s3imph_csv_header_schema(cp, 4, ctypes.byref(sch), None, err, 256) == s3imph.ERR_INVALID
    assert L.s3imph_csv_header_schema(None, 4, ctypes.byref(sch), ctypes.byref(start), err, 256) == s3imph.ERR_INVALID


def test_device_calls_refuse_bad_arguments_before_any_device_work():
    L = s3imph.LIB
    csv, cp, sch, info = _args()
    bi = ctypes.byref(info)
    assert L.s3imph_csv_plan_device(None, cp, 4, ctypes.byref(sch), bi, None) == s3imph.ERR_INVALID
    # the ctx is checked first, so a made-up non-null one is never touched either
    fake = ctypes.c_void_p(8)
    assert L.s3imph_csv_plan_device(fake, cp, 4, None, bi, None) == s3imph.ERR_INVALID
    assert L.s3imph_csv_plan_device(fake, cp, 4, ctypes.byref(sch), None, None) == s3imph.ERR_INVALID
    assert L.s3imph_csv_plan_device(fake, None, 4, ctypes.byref(sch), bi, None) == s3imph.ERR_INVALID
    for bad in (s3imph.CsvSchema(-1, 1, -1, -1), s3imph.CsvSchema(0, -1, -1, -1), s3imph.CsvSchema(-5, -5, 0, 0)):
        assert L.s3imph_csv_plan_device(fake, cp, 4, ctypes.byref(bad), bi, None) == s3imph.ERR_INVALID
    assert L.s3imph_csv_fill_device(None, cp, 8, 0, cp, cp, cp, None) == s3imph.ERR_INVALID


def test_host_calls_refuse_bad_arguments_before_any_device_work(tmp_path):
    L = s3imph.LIB
    csv, cp, sch, info = _args()
    err = ctypes.create_string_buffer(256)
    out = [ctypes.c_void_p() for _ in range(4)]
    refs = [ctypes.byref(p) for p in out]
    f = L.s3imph_csv_parse_host
    assert f(0, cp, 4, None, *refs, ctypes.byref(info), err, 256) == s3imph.ERR_INVALID
    assert f(0, None, 4, ctypes.byref(sch), *refs, ctypes.byref(info), err, 256) == s3imph.ERR_INVALID
    assert f(0, cp, 4, ctypes.byref(sch), *refs, None, err, 256) == s3imph.ERR_INVALID
    for k in range(4):
        some = list(refs)
        some[k] = None
        assert f(0, cp, 4, ctypes.byref(sch), *some, ctypes.byref(info), err, 256) == s3imph.ERR_INVALID
    for bad in (s3imph.CsvSchema(-1, 1, -1, -1), s3imph.CsvSchema(0, -1, -1, -1)):
        assert f(0, cp, 4, ctypes.byref(bad), *refs, ctypes.byref(info), err, 256) == s3imph.ERR_INVALID
    assert all(p.value is None for p in out)

    g = L.s3imph_index_from_csv_host
    ptrs = (ctypes.c_void_p * 1)(csv.ctypes.data)
    lens = (ctypes.c_uint64 * 1)(4)
    d = str(tmp_path).encode()
    assert g(0, ptrs, lens, 1, None, 0, 0, d, None, err, 256) == s3imph.ERR_INVALID
    assert g(0, ptrs, lens, 1, ctypes.byref(sch), 0, 0, None, None, err, 256) == s3imph.ERR_INVALID
    assert g(0, None, lens, 1, ctypes.byref(sch), 0, 0, d, None, err, 256) == s3imph.ERR_INVALID
    assert g(0, ptrs, None, 1, ctypes.byref(sch), 0, 0, d, None, err, 256) == s3imph.ERR_INVALID
    assert g(0, (ctypes.c_void_p * 1)(None), lens, 1, ctypes.byref(sch), 0, 0, d, None, err, 256) == s3imph.ERR_INVALID
    bad = s3imph.CsvSchema(0, -1, -1, -1)
    assert g(0, ptrs, lens, 1, ctypes.byref(bad), 0, 0, d, None, err, 256) == s3imph.ERR_INVALID
    # a missing directory is an I/O error, found before the device is selected
    rc = g(0, ptrs, lens, 1, ctypes.byref(sch), 0, 0, str(tmp_path / "nope").encode(), None, err, 256)
    assert rc == s3imph.ERR_IO and b"no such directory" in err.value


def test_empty_input_needs_no_gpu(tmp_path):
    """len == 0: the empty listing; no buffers, or only empty ones: the empty index."""
    keys, offs, sizes, tiers, info = s3imph.parse_inventory_csv(b"", (0, 1, -1, -1))
    assert len(keys) == 0 and offs.tolist() == [0] and len(sizes) == 0 and len(tiers) == 0
    assert info == dict(n_records=0, n_objects=0, key_bytes=0, n_short=0, n_empty_key=0, n_bad_size=0)
    for sub, files, with_tiers in (("none", [], False), ("empties", [b"", b""], True)):
        d = tmp_path / sub
        d.mkdir()
        total = s3imph.build_index_from_inventory_csv(files, (0, 1, 2, 3), str(d), with_tiers=with_tiers)
        assert total["n_objects"] == 0 and total["n_records"] == 0
        assert (d / "mph.bin").read_bytes() == b""
        assert list(s3imph.read_u64_array(str(d / "depth_offsets.u64"))) == [0, 0]
        s3imph.verify_manifest(str(d))
        assert s3imph.read_manifest(str(d))["node_count"] == 0
        assert not (d / "tiers.json").exists()


def test_tier_from_s3_keeps_its_rule_after_the_move():
    """The table and the trim now live where host and device share them: the host answers as
    before, and as the test reference does."""
    names = [n for _, n, _ in s3imph.TIERS] + ["INTELLIGENT_TIERING", "", "nonsense", "x" * 100, "GLACIER\xa0"]
    access = ["", "FREQUENT_ACCESS", "FREQUENT", "INFREQUENT_ACCESS", "INFREQUENT", "ARCHIVE_INSTANT_ACCESS",
              "ARCHIVE_ACCESS", "ARCHIVE", "DEEP_ARCHIVE_ACCESS", "DEEP_ARCHIVE", "nope", "y" * 64]
    for n in names:
        for a in access:
            for f in (str, str.lower, lambda t: " \t" + t + "\r\n", lambda t: t[:3] + " " + t[3:]):
                sc, at = f(n), f(a)
                assert s3imph.tier_from_s3(sc, at) == C.tier_of(sc.encode("latin-1"), at.encode("latin-1")), (sc, at)
    for t, name, _ in s3imph.TIERS:
        assert s3imph.tier_from_s3(name) == t
