"""Section 5i of the C ABI (row merge, index from rows, the chunked build) without a GPU: the
symbols are exported, declared and bound, and every refusal that comes before device work returns
ERR_INVALID without a device being touched (these tests run where there is none)."""
import ctypes
import os
import re

import numpy as np
import pytest

import merge_ref as M
import s3imph
from conftest import ROOT

NEW_INT = ("s3imph_merge_rows_plan_device", "s3imph_merge_rows_fill_device", "s3imph_merge_rows_host",
           "s3imph_index_from_rows_host", "s3imph_rowset_new", "s3imph_rowset_add_objects", "s3imph_rowset_add_csv",
           "s3imph_rowset_add_rows", "s3imph_rowset_build", "s3imph_rowset_close")
NEW_OTHER = ("s3imph_merge_geometry", "s3imph_rowset_runs", "s3imph_rowset_rows")


def _declared():
    src = open(os.path.join(ROOT, "include", "s3imph.h")).read()
    return set(re.findall(r"^(?:int|void|uint64_t)\s+(s3imph_[a-z0-9_]+)\(", src, re.M))


def test_symbols_exported_declared_and_bound():
    lib = ctypes.CDLL(s3imph.LIB_PATH)
    declared = _declared()
    for name in NEW_INT + NEW_OTHER:
        assert hasattr(lib, name), name
        assert name in s3imph.EXPORTS and name in declared, name
        assert getattr(s3imph.LIB, name).argtypes is not None
    for name in NEW_INT:
        assert getattr(s3imph.LIB, name).restype is ctypes.c_int
    for name in ("merge_rows", "build_index_from_rows", "merge_geometry", "RowSet", "MergeInfo"):
        assert hasattr(s3imph, name), name
    for name in ("merge_rows_plan", "merge_rows_fill"):
        assert callable(getattr(s3imph.DeviceBuilder, name))
    for name in ("add_objects", "add_csv", "add_rows", "build", "close", "__enter__", "__exit__"):
        assert callable(getattr(s3imph.RowSet, name))
    assert s3imph.LIB.s3imph_abi_version() == 1
    assert s3imph.MERGE_MAX_RUNS == 64
    src = open(os.path.join(ROOT, "include", "s3imph.h")).read()
    assert re.search(r"#define S3IMPH_MERGE_MAX_RUNS 64\b", src)


def test_struct_layouts():
    I = s3imph.MergeInfo
    assert ctypes.sizeof(I) == 48
    assert [getattr(I, f).offset for f in ("n_in", "n_out", "blob_bytes", "first_unsorted", "present_mask",
                                           "max_depth_seen", "n_runs")] == [0, 8, 16, 24, 32, 40, 44]
    R = s3imph.RowRun
    assert ctypes.sizeof(R) == 72
    assert [getattr(R, f).offset for f in ("blob", "offsets", "depth", "count", "bytes", "tier_count", "tier_bytes",
                                           "n", "tier_stride")] == list(range(0, 72, 8))


def test_geometry():
    step = s3imph.merge_geometry()
    assert step >= 2
    s3imph.LIB.s3imph_merge_geometry(None)  # a null argument is ignored


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def test_device_calls_refuse_before_any_device_work():
    """Without a GPU no context can be made, so the calls get none: every shape below is refused."""
    L = s3imph.LIB
    info = s3imph.MergeInfo()
    x = np.zeros(16, np.uint64)
    p = _ptr(x)

    def plan(blob=p, offs=p, depth=p, cnt=p, nbytes=p, tc=None, tb=None, stride=0, starts=(0, 1), k=None, inf=info):
        rs = np.array(starts, np.uint64)
        return L.s3imph_merge_rows_plan_device(None, blob, offs, depth, cnt, nbytes, tc, tb, stride, _ptr(rs),
                                               len(rs) - 1 if k is None else k, ctypes.byref(inf) if inf else None,
                                               None)

    assert plan() == s3imph.ERR_INVALID                          # no context
    assert plan(inf=None) == s3imph.ERR_INVALID
    for name in ("blob", "offs", "depth", "cnt", "nbytes"):
        assert plan(**{name: None}) == s3imph.ERR_INVALID
    assert plan(tc=p) == s3imph.ERR_INVALID                      # one tier array without the other
    assert plan(tb=p) == s3imph.ERR_INVALID
    assert plan(tc=p, tb=p, stride=0) == s3imph.ERR_INVALID      # tier_stride below N
    assert plan(starts=(1, 2)) == s3imph.ERR_INVALID             # does not start at 0
    assert plan(starts=(0, 3, 2, 4)) == s3imph.ERR_INVALID       # decreases
    assert plan(starts=[0] * 66, k=65) == s3imph.ERR_INVALID     # k > S3IMPH_MERGE_MAX_RUNS
    assert plan(starts=(0, 1 << 32)) == s3imph.ERR_INVALID       # N >= 2^32 claimed through run_starts
    assert L.s3imph_merge_rows_plan_device(None, p, p, p, p, p, None, None, 0, None, 1, ctypes.byref(info), None) \
        == s3imph.ERR_INVALID                                    # no run_starts
    assert L.s3imph_merge_rows_fill_device(None, p, 8, p, p, p, p, None, None, 1, None) == s3imph.ERR_INVALID


def _run(rows, tiers):
    a = M.to_arrays(rows)
    return a if tiers else a[:5]


def test_host_calls_refuse_mixed_and_malformed_runs(tmp_path):
    with_t = _run([M.row("a/", 1, 1, 1, {0: (1, 1)})], True)
    without = _run([M.row("b/", 1, 1, 1)], False)
    for call in (lambda: s3imph.merge_rows([with_t, without]),
                 lambda: s3imph.merge_rows([with_t, _run([], False), without]),
                 lambda: s3imph.build_index_from_rows([without, with_t], str(tmp_path))):
        with pytest.raises(s3imph.MPHFError) as e:
            call()
        assert e.value.status == s3imph.ERR_INVALID and str(e.value).startswith("merge: ")
        assert "mixed" in str(e.value)
    assert not os.listdir(tmp_path)
    L = s3imph.LIB
    err = ctypes.create_string_buffer(256)
    out = [ctypes.c_void_p() for _ in range(7)]
    n, mask = ctypes.c_uint64(), ctypes.c_uint64()
    refs = [ctypes.byref(q) for q in out]
    # runs announced but not given; a run whose arrays are missing; one tier array without the other
    assert L.s3imph_merge_rows_host(0, None, 2, *refs, ctypes.byref(mask), ctypes.byref(n), None, err, 256) \
        == s3imph.ERR_INVALID
    x = np.zeros(4, np.uint64)
    bad = (s3imph.RowRun * 1)(s3imph.RowRun(None, x.ctypes.data, None, None, None, None, None, 1, 1))
    assert L.s3imph_merge_rows_host(0, bad, 1, *refs, ctypes.byref(mask), ctypes.byref(n), None, err, 256) \
        == s3imph.ERR_INVALID and err.value.startswith(b"merge: ")
    p = x.ctypes.data
    half = (s3imph.RowRun * 1)(s3imph.RowRun(p, p, p, p, p, p, None, 1, 1))
    assert L.s3imph_merge_rows_host(0, half, 1, *refs, ctypes.byref(mask), ctypes.byref(n), None, err, 256) \
        == s3imph.ERR_INVALID and b"one tier array" in err.value
    assert L.s3imph_index_from_rows_host(0, half, 1, str(tmp_path).encode(), err, 256) == s3imph.ERR_INVALID
    # outputs missing
    good = (s3imph.RowRun * 1)(s3imph.RowRun(p, p, p, p, p, None, None, 1, 1))
    assert L.s3imph_merge_rows_host(0, good, 1, None, *refs[1:], ctypes.byref(mask), ctypes.byref(n), None, err, 256) \
        == s3imph.ERR_INVALID
    assert L.s3imph_index_from_rows_host(0, good, 1, None, err, 256) == s3imph.ERR_INVALID
    rc = L.s3imph_index_from_rows_host(0, good, 1, str(tmp_path / "nope").encode(), err, 256)
    assert rc == s3imph.ERR_IO and b"no such directory" in err.value
    assert all(q.value is None for q in out)


def test_no_rows_need_no_gpu(tmp_path):
    """k == 0 or only empty runs: zero rows, and the empty index s3imph_index_open accepts."""
    empty = _run([], False)
    for runs in ([], [empty], [empty, _run([], True)]):
        got = s3imph.merge_rows(runs, with_info=True)
        assert len(got[1]) == 1 and got[1][0] == 0 and all(len(a) == 0 for a in got[2:5])
        assert got[-1]["n_in"] == 0 and got[-1]["n_out"] == 0 and got[-1]["first_unsorted"] == 2**64 - 1
    for sub, runs in (("none", []), ("empties", [empty, empty])):
        d = tmp_path / sub
        d.mkdir()
        s3imph.build_index_from_rows(runs, str(d))
        assert (d / "mph.bin").read_bytes() == b""
        assert list(s3imph.read_u64_array(str(d / "depth_offsets.u64"))) == [0, 0]
        s3imph.verify_manifest(str(d))
        assert s3imph.read_manifest(str(d))["node_count"] == 0 and not (d / "tiers.json").exists()


def test_rowset_bookkeeping_without_gpu(tmp_path):
    with s3imph.RowSet(max_depth=0, with_tiers=True) as rs:
        assert (rs.runs, rs.rows) == (0, 0)
        rs.add_objects(np.zeros(0, np.uint8), np.zeros(1, np.uint64), None, np.zeros(0, np.uint8))  # no object: no run
        rs.add_csv([b"", b""], (0, 1))
        rs.add_rows(_run([], True))
        assert (rs.runs, rs.rows) == (0, 0)
        rows = [M.row("", 0, 2, 9, {1: (2, 9)}), M.row("a/", 1, 2, 9, {1: (2, 9)})]
        rs.add_rows(_run(rows, True))
        assert (rs.runs, rs.rows) == (1, 2)
        with pytest.raises(s3imph.MPHFError) as e:
            rs.add_rows(_run(rows, False))  # a run without tier columns in a set with them
        assert e.value.status == s3imph.ERR_INVALID and "mixed" in str(e.value)
        with pytest.raises(s3imph.MPHFError) as e:
            rs.add_objects(np.frombuffer(b"a/b", np.uint8), np.array([0, 3], np.uint64), None)  # tiers missing
        assert e.value.status == s3imph.ERR_INVALID
        with pytest.raises(s3imph.MPHFError) as e:
            rs.build(str(tmp_path / "nope"))
        assert e.value.status == s3imph.ERR_IO
    with s3imph.RowSet() as rs:
        rs.build(str(tmp_path))  # no runs: the empty index
        s3imph.verify_manifest(str(tmp_path))
        assert s3imph.read_manifest(str(tmp_path))["node_count"] == 0
    err = ctypes.create_string_buffer(64)
    assert s3imph.LIB.s3imph_rowset_new(0, 0, 0, None, err, 64) == s3imph.ERR_INVALID
    assert s3imph.LIB.s3imph_rowset_add_rows(None, None, err, 64) == s3imph.ERR_INVALID
    assert s3imph.LIB.s3imph_rowset_runs(None) == 0 and s3imph.LIB.s3imph_rowset_rows(None) == 0
