"""The chunked build (s3imph.RowSet, include/s3imph.h section 5i): a listing fed in chunks gives,
file for file, the directory the oracle writes for the reference rows of the whole listing — the
one s3imph.build_index_from_unsorted_objects writes for it in one piece — whatever the chunking,
through add_objects, add_csv and add_rows; and the reader answers the merged sums from it."""
import os

import numpy as np
import pytest

import merge_ref as M
import oracle as O
import s3imph
import tiers_ref as T
from index_dirs import write_index_dir
from test_gpu_index_from_objects import listing

pytestmark = pytest.mark.gpu

# storage classes whose tier id needs no access-tier column (tiers.go:85-115)
CLASSES = ["STANDARD", "STANDARD_IA", "ONEZONE_IA", "GLACIER_IR", "GLACIER", "DEEP_ARCHIVE", "REDUCED_REDUNDANCY"]


@pytest.fixture(scope="module")
def ref(tmp_path_factory, oracle_lib):
    """The 20k-object listing, shuffled; its reference rows; the oracle-written directory."""
    keys, sizes = listing(20_000, seed=23)
    rng = np.random.default_rng(24)
    tiers = rng.integers(0, len(CLASSES), len(keys)).astype(np.uint8)
    tiers[:50] = 6  # one tier only at the front of the sorted listing
    rows = T.aggregate_dict_tiers(keys, sizes, tiers)
    order = rng.permutation(len(keys))
    want = tmp_path_factory.mktemp("rowset_oracle")
    count = np.array([r[2] for r in rows], np.uint64)
    total = np.array([r[3] for r in rows], np.uint64)
    arr = write_index_dir(str(want), oracle_lib, [r[0] for r in rows], stats=(count, total),
                          depths=[r[1] for r in rows])
    s3imph.write_manifest(str(want), len(rows), int(arr["max_depth"]))
    return {"keys": [keys[i] for i in order], "sizes": sizes[order], "tiers": tiers[order], "rows": rows,
            "want": want, "count": count, "total": total, "tc_tb": T.tier_arrays(rows), "mask": T.present_mask(tiers)}


def same_directory(got, ref, tiers=True):
    want = ref["want"]
    names = sorted(os.listdir(want))
    extra = ["tier_stats", "tiers.json"] if tiers else []
    assert sorted(os.listdir(got)) == sorted(names + extra) and len(names) == 13
    for name in names:
        if name != "manifest.json":
            assert (got / name).read_bytes() == (want / name).read_bytes(), name
    a, b = s3imph.read_manifest(str(got)), s3imph.read_manifest(str(want))
    a.pop("created_at")
    b.pop("created_at")
    assert a == b and a["node_count"] == len(ref["rows"])
    s3imph.verify_manifest(str(got))
    if tiers:
        tc, tb = ref["tc_tb"]
        ids = T.mask_ids(ref["mask"])
        assert (got / "tiers.json").read_bytes() == T.tiers_json(ids)
        files = {}
        for t in ids:
            files[T.TIER_TABLE[t][1] + "_count.u64"] = O.s3id_u64_array(tc[t])
            files[T.TIER_TABLE[t][1] + "_bytes.u64"] = O.s3id_u64_array(tb[t])
        assert sorted(os.listdir(got / "tier_stats")) == sorted(files)
        for name, data in files.items():
            assert (got / "tier_stats" / name).read_bytes() == data, name


def chunks_of(ref, cuts):
    """The shuffled listing cut at `cuts` (ascending indices): (blob, offsets, sizes, tiers) each."""
    out = []
    for lo, hi in zip([0] + cuts, cuts + [len(ref["keys"])]):
        blob, offs = O.keys_to_blob(ref["keys"][lo:hi])
        out.append((blob, offs, ref["sizes"][lo:hi], ref["tiers"][lo:hi]))
    return out


@pytest.mark.parametrize("cuts", [[], [7000], [3000, 3000, 9000, 19_990]], ids=["1", "2", "5 with an empty one"])
def test_add_objects_in_chunks(ref, tmp_path, cuts):
    with s3imph.RowSet(with_tiers=True) as rs:
        for blob, offs, sizes, tiers in chunks_of(ref, cuts):
            rs.add_objects(blob, offs, sizes, tiers)
        assert rs.runs == len(cuts) + 1 - (1 if len(cuts) == 4 else 0)  # a chunk without an object adds no run
        assert rs.rows >= len(ref["rows"])
        rs.build(str(tmp_path))
    same_directory(tmp_path, ref)


def test_equals_the_build_from_the_whole_listing(ref, tmp_path):
    """The contract as the header states it, against the library's own one-piece build."""
    blob, offs = O.keys_to_blob(ref["keys"])
    s3imph.build_index_from_unsorted_objects(blob, offs, ref["sizes"], str(tmp_path), tiers=ref["tiers"])
    same_directory(tmp_path, ref)


def test_add_csv_in_three_buffers(ref, tmp_path):
    for t, name in enumerate(CLASSES):
        assert s3imph.tier_from_s3(name) == t
    lines = [b"bucket,%s,%d,%s\n" % (k, int(z), CLASSES[t].encode())
             for k, z, t in zip(ref["keys"], ref["sizes"], ref["tiers"])]
    bufs = [b"".join(lines[:5000]), b"".join(lines[5000:5001]), b"".join(lines[5001:])]
    with s3imph.RowSet(with_tiers=True) as rs:
        for buf in bufs:
            rs.add_csv([buf], (1, 2, 3, -1))
        assert rs.runs == 3
        rs.build(str(tmp_path))
    same_directory(tmp_path, ref)


def test_add_rows_mixed_with_add_objects(ref, tmp_path):
    """The first part as hand-made rows (the reference aggregation of that part), the rest as objects."""
    cut = 4000
    part = T.aggregate_dict_tiers(ref["keys"][:cut], ref["sizes"][:cut], ref["tiers"][:cut])
    rest = chunks_of(ref, [cut])[1]
    with s3imph.RowSet(with_tiers=True) as rs:
        rs.add_objects(*rest)
        rs.add_rows(M.to_arrays(part))
        assert rs.runs == 2
        rs.build(str(tmp_path))
        same_directory(tmp_path, ref)


def test_index_answers_the_merged_sums(ref, tmp_path):
    with s3imph.RowSet(with_tiers=True) as rs:
        for blob, offs, sizes, tiers in chunks_of(ref, [100, 12_000]):
            rs.add_objects(blob, offs, sizes, tiers)
        rs.build(str(tmp_path))
    rows = ref["rows"]
    tc, tb = ref["tc_tb"]
    ids = T.mask_ids(ref["mask"])
    with s3imph.Index(str(tmp_path)) as idx:
        assert idx.count == len(rows) and idx.has_tier_data() and idx.present_tiers() == ids
        pick = list(range(0, len(rows), 37)) + [len(rows) - 1]
        found, cnt, tot = idx.stats_for_prefix([rows[p][0] for p in pick])
        assert found.all()
        assert np.array_equal(cnt, ref["count"][pick]) and np.array_equal(tot, ref["total"][pick])
        assert int(cnt[0]) == len(ref["keys"])  # the root holds every object of every chunk
        got = idx.tier_breakdown_for_prefix([rows[p][0] for p in pick])
        assert got == [T.get_breakdown(ids, tc, tb, p) for p in pick]


def test_no_runs_build_the_empty_index(tmp_path):
    with s3imph.RowSet(with_tiers=True) as rs:
        rs.build(str(tmp_path))
    with s3imph.Index(str(tmp_path)) as idx:
        assert idx.count == 0
    s3imph.verify_manifest(str(tmp_path))
    assert not (tmp_path / "tiers.json").exists() and not (tmp_path / "tier_stats").exists()


def test_rows_without_tier_columns_write_no_tier_files(ref, tmp_path):
    cut = 9000
    runs = [M.to_arrays(T.aggregate_dict_tiers(ref["keys"][lo:hi], ref["sizes"][lo:hi], ref["tiers"][lo:hi]))[:5]
            for lo, hi in ((0, cut), (cut, len(ref["keys"])))]
    s3imph.build_index_from_rows(runs, str(tmp_path))
    same_directory(tmp_path, ref, tiers=False)


def test_failures_are_worded(ref, tmp_path):
    rows = ref["rows"][:10]
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.build_index_from_rows([M.to_arrays(rows[::-1])], str(tmp_path))
    assert e.value.status == s3imph.ERR_INVALID and str(e.value).startswith("merge: ")
    assert not os.listdir(tmp_path)
