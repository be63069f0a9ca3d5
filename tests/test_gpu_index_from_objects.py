"""Object listing in, queryable index out (s3imph.build_index_from_objects, include/s3imph.h
section 5d): the directory equals, file for file, the one the oracle writes for the reference
rows of tests/aggregate_ref.py, and the reader answers from it — filtered descendants
included, which need the object_count / total_bytes columns no other build writes."""
import os

import numpy as np
import pytest

import aggregate_ref as R
import finalize_queries as FQ
import oracle as O
import s3imph
from index_dirs import write_index_dir

pytestmark = pytest.mark.gpu


def listing(m=20_000, seed=5):
    """About m distinct sorted object keys, 0 to 5 directories deep, a few objects per directory."""
    rng = np.random.default_rng(seed)
    keys = set()
    while len(keys) < m:
        depth = int(rng.integers(0, 6))
        dirs = [b"d%02d" % int(rng.integers(0, 40))] + [b"s%d" % int(rng.integers(0, 4)) for _ in range(depth)]
        keys.add(b"/".join(dirs[:depth]) + (b"/" if depth else b"") + b"obj-%04d.bin" % int(rng.integers(0, 3000)))
    keys = sorted(keys)
    sizes = rng.integers(0, 1 << 44, len(keys), dtype=np.uint64)
    sizes[::97] = 0
    return keys, sizes


def _build_both(keys, sizes, got, want, oracle_lib):
    """The GPU-built directory `got`, the oracle-written one `want` for the reference rows, the rows."""
    rows = R.aggregate_dict(keys, sizes)
    blob, offs = O.keys_to_blob(keys)
    s3imph.build_index_from_objects(blob, offs, sizes, str(got))
    prefixes = [r[0] for r in rows]
    count = np.array([r[2] for r in rows], np.uint64)
    total = np.array([r[3] for r in rows], np.uint64)
    arr = write_index_dir(str(want), oracle_lib, prefixes, stats=(count, total), depths=[r[1] for r in rows])
    s3imph.write_manifest(str(want), len(rows), int(arr["max_depth"]))
    return {"got": got, "want": want, "rows": rows, "keys": keys, "arr": arr, "count": count, "total": total}


@pytest.fixture(scope="module")
def built(tmp_path_factory, oracle_lib):
    keys, sizes = listing()
    return _build_both(keys, sizes, tmp_path_factory.mktemp("from_objects"), tmp_path_factory.mktemp("from_oracle"),
                       oracle_lib)


def test_directory_equals_the_oracle_written_one(built):
    _directories_equal(built)


def test_one_object_100_directories_deep(tmp_path_factory, oracle_lib):
    """One object key with 100 '/': maxDepth 100 is beyond the 64 depth_offsets entries the
    finalize of the rows is offered first, so the listing-to-directory path takes its retry."""
    keys, sizes = listing(m=2000, seed=6)
    deep = b"d20/" + b"x/" * 99 + b"obj"
    assert deep.count(b"/") == 100 and deep not in keys
    keys = sorted(keys + [deep])
    sizes = np.concatenate([sizes, np.array([12345], np.uint64)])
    b = _build_both(keys, sizes, tmp_path_factory.mktemp("deep_objects"), tmp_path_factory.mktemp("deep_oracle"),
                    oracle_lib)
    assert b["arr"]["max_depth"] == 100 and len(b["arr"]["depth_offsets"]) == 102
    _directories_equal(b)
    with s3imph.Index(str(b["got"])) as idx:
        assert idx.count == len(b["rows"]) and idx.max_depth == 100


def _directories_equal(built):
    names = sorted(os.listdir(built["want"]))
    assert sorted(os.listdir(built["got"])) == names and "object_count.u64" in names and len(names) == 13
    for name in names:
        if name != "manifest.json":
            assert (built["got"] / name).read_bytes() == (built["want"] / name).read_bytes(), name
    a, b = s3imph.read_manifest(str(built["got"])), s3imph.read_manifest(str(built["want"]))
    a.pop("created_at")
    b.pop("created_at")
    assert a == b and a["node_count"] == len(built["rows"])
    s3imph.verify_manifest(str(built["got"]))


def test_index_opens_and_answers(built):
    rows, arr = built["rows"], built["arr"]
    with s3imph.Index(str(built["got"])) as idx:
        assert idx.count == len(rows) and idx.max_depth == arr["max_depth"]
        found, cnt, tot = idx.stats_for_prefix([r[0] for r in rows])
        assert found.all()
        assert np.array_equal(cnt, built["count"]) and np.array_equal(tot, built["total"])
        # full object keys are not prefixes (none of them ends in '/')
        objs = [k for k in built["keys"][::50]]
        assert (idx.lookup(objs) == np.uint64(2**64 - 1)).all()
        # filtered descendants of the root: ERR_STATE on every index written without the columns
        for k in (1, 30, 400, 10**6):
            ref = [p for p in FQ.descendants_at_depth(arr, 0, 1) if built["count"][p] >= k]
            got = idx.descendants_at_depth([0], 1, min_count=k)[0]
            assert [int(p) for p in got] == ref, k
        big = int(np.median(built["total"]))
        ref = [p for p in FQ.descendants_at_depth(arr, 0, 2)
               if built["count"][p] >= 5 and built["total"][p] >= big]
        assert [int(p) for p in idx.descendants_at_depth([0], 2, min_count=5, min_bytes=big)[0]] == ref
        assert len(ref) > 0


def test_empty_listing_gives_an_index_that_opens(tmp_path):
    s3imph.build_index_from_objects(np.zeros(0, np.uint8), np.zeros(1, np.uint64), None, str(tmp_path))
    with s3imph.Index(str(tmp_path)) as idx:
        assert idx.count == 0
    s3imph.verify_manifest(str(tmp_path))


def test_refusals_are_worded(tmp_path):
    blob, offs = O.keys_to_blob([b"b/x", b"a/x"])
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.build_index_from_objects(blob, offs, None, str(tmp_path))
    assert e.value.status == s3imph.ERR_INVALID and str(e.value).startswith("aggregate: ")
    assert not os.listdir(tmp_path)
