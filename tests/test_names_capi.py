"""The reader's prefix-blob entry points (include/s3imph.h section 5c: open_flags, attach_prefixes,
has_prefixes, prefixes_plan / fill, lookup_verify_device, verify_device) are declared, bound and
exported, the ABI version stays 1 (the change is additive), and their argument checks that need no
device answer without one."""
import ctypes
import os
import re

import s3imph
from conftest import ROOT

NAMES = ("s3imph_index_open_flags", "s3imph_index_attach_prefixes", "s3imph_index_has_prefixes",
         "s3imph_index_prefixes_plan", "s3imph_index_prefixes_fill", "s3imph_index_lookup_verify_device",
         "s3imph_index_verify_device")


def test_declared_bound_and_exported():
    src = open(os.path.join(ROOT, "include", "s3imph.h")).read()
    declared = set(re.findall(r"^int\s+(s3imph_[a-z0-9_]+)\(", src, re.M))
    lib = ctypes.CDLL(s3imph.LIB_PATH)
    for name in NAMES:
        assert name in declared, name
        assert name in s3imph.EXPORTS, name
        assert hasattr(lib, name), name
        f = getattr(s3imph.LIB, name)
        assert f.restype is ctypes.c_int and f.argtypes, name
    assert re.search(r"^#define S3IMPH_OPEN_PREFIXES 1$", src, re.M)
    assert s3imph.OPEN_PREFIXES == 1


def test_abi_version_stays_1():
    assert s3imph.LIB.s3imph_abi_version() == 1


def test_verify_quotes_names_like_percent_q():
    """Index.verify words its errors with fmt's %q (mphf.go:384,387), i.e. strconv.Quote."""
    q = s3imph._go_quote
    assert q(b"") == '""'
    assert q(b"foo/bar/") == '"foo/bar/"'
    assert q('日本語/'.encode()) == '"日本語/"'
    assert q(b'a"b\\c') == '"a\\"b\\\\c"'
    assert q(b"a\nb\tc\x00d\x7f") == '"a\\nb\\tc\\x00d\\x7f"'
    assert q(b"bad\xff/") == '"bad\\xff/"'
    assert q("a\u200bb".encode()) == '"a\\u200bb"'


def test_null_arguments():
    L = s3imph.LIB
    h = ctypes.c_void_p()
    v = ctypes.c_uint64()
    assert L.s3imph_index_open_flags(0, None, 1, ctypes.byref(h), None, 0) == s3imph.ERR_INVALID
    assert L.s3imph_index_open_flags(0, b"/nonexistent", 2, ctypes.byref(h), None, 0) == s3imph.ERR_INVALID
    assert L.s3imph_index_attach_prefixes(None, None, None) == s3imph.ERR_INVALID
    assert L.s3imph_index_has_prefixes(None) == 0
    assert L.s3imph_index_prefixes_plan(None, None, 0, None, None, ctypes.byref(v), None) == s3imph.ERR_INVALID
    assert L.s3imph_index_prefixes_fill(None, None, 0, None) == s3imph.ERR_INVALID
    assert L.s3imph_index_lookup_verify_device(None, None, None, 0, None, None) == s3imph.ERR_INVALID
    assert L.s3imph_index_verify_device(None, ctypes.byref(v), ctypes.byref(v), ctypes.byref(v),
                                        None) == s3imph.ERR_INVALID
