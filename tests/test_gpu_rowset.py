"""The chunked build (s3imph.RowSet, include/s3imph.h section 5i): a listing fed in chunks gives,
file for file, the directory the oracle writes for the reference rows of the whole listing — the
one s3imph.build_index_from_unsorted_objects writes for it in one piece — whatever the chunking,
through add_objects, add_csv and add_rows; and the reader answers the merged sums from it.  The
second half checks that contract over the axes the code branches on (tests/rowset_cases.py, whose
closure under chunking tests/test_rowset_cases.py proves on the CPU): depth cut, tier switch,
repeated keys, chunk shapes, more than 64 runs, depth past 62, repeated builds, refusals, and
host runs in every layout s3imph_row_run allows."""
import os

import numpy as np
import pytest

import merge_ref as M
import oracle as O
import rowset_cases as RC
import s3imph
import tiers_ref as T
from index_dirs import write_index_dir
from test_gpu_index_from_objects import listing

pytestmark = pytest.mark.gpu

CLASSES = RC.CLASSES


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


def same_directory(got, ref, tiers=True, max_depth=None):
    """got equals the oracle-written ref["want"] file for file; with `tiers` the tier files are
    those of the reference rows, without it there are none; max_depth: what the manifest holds."""
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
    if max_depth is not None:
        assert a["max_depth"] == max_depth
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


# ---- the contract across the axes the code branches on (tests/rowset_cases.py) ------------------
def reference(path, oracle_lib, rows):
    """The oracle-written directory for reference rows, shaped like the `ref` fixture."""
    count = np.array([r[2] for r in rows], np.uint64)
    total = np.array([r[3] for r in rows], np.uint64)
    arr = write_index_dir(str(path), oracle_lib, [r[0] for r in rows], stats=(count, total),
                          depths=[r[1] for r in rows])
    s3imph.write_manifest(str(path), len(rows), int(arr["max_depth"]))
    return {"rows": rows, "want": path, "count": count, "total": total, "tc_tb": T.tier_arrays(rows),
            "mask": M.present_mask(rows), "arr": arr}


@pytest.fixture(scope="module")
def refs(tmp_path_factory, oracle_lib):
    """name -> the reference of that case's whole listing; cases with the same listing and depth
    cut share one directory."""
    made = {}

    def get(name):
        key = RC.case(name).ref_key()
        if key not in made:
            made[key] = reference(tmp_path_factory.mktemp("rowset_case"), oracle_lib, RC.whole_rows(name))
        return made[key]
    return get


def feed(rs, chunks, with_tiers, max_depth=0):
    """Every chunk through the call it names; add_objects is always handed the tier ids.  Returns
    the runs held."""
    held = rs.runs
    for ch in chunks:
        if ch.how == "objects":
            rs.add_objects(*O.keys_to_blob(ch.keys), ch.sizes, ch.tiers)
        elif ch.how == "csv":
            rs.add_csv([ch.csv()], RC.SCHEMA)
        else:
            rows = T.aggregate_dict_tiers(ch.keys, ch.sizes, ch.tiers, max_depth) if ch.keys else []
            rs.add_rows(M.to_arrays(rows)[:7 if with_tiers else 5])
        held += bool(ch.keys)
        assert rs.runs == held, "a chunk without an object adds no run, every other chunk one"
    return held


@pytest.mark.parametrize("name", [n for n in RC.NAMES if n != "extended"])
def test_chunked_build_equals_the_whole_listing_reference(refs, tmp_path, name):
    c = RC.case(name)
    ref = refs(name)
    with s3imph.RowSet(max_depth=c.max_depth, with_tiers=c.with_tiers) as rs:
        held = feed(rs, c.chunks, c.with_tiers, c.max_depth)
        assert held == sum(bool(ch.keys) for ch in c.chunks) and rs.rows == sum(len(r) for r in c.chunk_rows())
        rs.build(str(tmp_path))
    deepest = max(r[1] for r in ref["rows"])
    assert deepest == (c.max_depth or deepest)
    same_directory(tmp_path, ref, tiers=c.with_tiers, max_depth=deepest)


def test_depth_past_62_after_the_merge(refs, tmp_path):
    """No chunk's own finalize sees the depth the merged rows have: the retry of the rows' finalize."""
    ref = refs("deep")
    assert ref["arr"]["max_depth"] == 100 and len(ref["arr"]["depth_offsets"]) == 102
    with s3imph.RowSet(with_tiers=True) as rs:
        feed(rs, RC.case("deep").chunks[::-1], True)  # the deep chunk first: its ancestors' sums come second
        rs.build(str(tmp_path))
    same_directory(tmp_path, ref, max_depth=100)
    assert len((tmp_path / "depth_offsets.u64").read_bytes()) == len(O.s3id_u64_array(np.zeros(102, np.uint64)))
    with s3imph.Index(str(tmp_path)) as idx:
        assert idx.count == len(ref["rows"]) and idx.max_depth == 100


def test_the_one_piece_build_agrees_on_the_small_listing(refs, tmp_path):
    """The second witness: the library's own build of the concatenation, keys repeated and empty."""
    keys, sizes, tiers = RC.case("shapes").objects()
    s3imph.build_index_from_unsorted_objects(*O.keys_to_blob(keys), sizes, str(tmp_path), tiers=tiers)
    same_directory(tmp_path, refs("shapes"))


def test_build_may_be_repeated_and_the_set_extended(refs, tmp_path):
    first, second, third = tmp_path / "a", tmp_path / "b", tmp_path / "c"
    for d in (first, second, third):
        d.mkdir()
    base, more = RC.case("extended").chunks[:-1], RC.case("extended").chunks[-1:]
    with s3imph.RowSet(with_tiers=True) as rs:
        held = feed(rs, base, True)
        rs.build(str(first))
        rs.build(str(second))
        assert rs.runs == held
        same_directory(first, refs("shapes"))
        same_directory(second, refs("shapes"))
        rs.add_objects(*O.keys_to_blob(more[0].keys), more[0].sizes, more[0].tiers)
        assert rs.runs == held + 1
        rs.build(str(third))
    same_directory(third, refs("extended"))
    same_directory(first, refs("shapes"))  # the earlier directories are not touched


def _refused(call, word):
    with pytest.raises(s3imph.MPHFError) as e:
        call()
    assert e.value.status == s3imph.ERR_INVALID and word in str(e.value) and len(str(e.value)) > 10
    return str(e.value)


@pytest.mark.parametrize("with_tiers", [True, False])
def test_a_refused_add_leaves_the_set_as_it_was(refs, tmp_path, with_tiers):
    name = "shapes" if with_tiers else "no tiers"
    chunks = RC.case(name).chunks
    part = RC.part_rows(5)[0]
    with s3imph.RowSet(with_tiers=with_tiers) as rs:
        feed(rs, chunks[:2], with_tiers)
        before = (rs.runs, rs.rows)
        if with_tiers:
            ch = chunks[2]
            _refused(lambda: rs.add_objects(*O.keys_to_blob(ch.keys), ch.sizes), "rowset: ")
            assert (rs.runs, rs.rows) == before
            _refused(lambda: rs.add_rows(M.to_arrays(part)[:5]), "merge: ")
        else:
            _refused(lambda: rs.add_rows(M.to_arrays(part)), "merge: ")
        assert (rs.runs, rs.rows) == before
        # an empty run counts with neither: accepted either way, and adds nothing
        rs.add_rows(M.to_arrays([]))
        rs.add_rows(M.to_arrays([])[:5])
        assert (rs.runs, rs.rows) == before
        feed(rs, chunks[2:], with_tiers)
        rs.build(str(tmp_path))
    same_directory(tmp_path, refs(name), tiers=with_tiers)


def test_an_unsorted_run_is_accepted_at_add_and_refused_at_build(tmp_path):
    rows = RC.part_rows(5)[0]
    bad = rows[:40] + [rows[41], rows[40]] + rows[42:]
    with s3imph.RowSet(with_tiers=True) as rs:
        rs.add_rows(M.to_arrays(RC.part_rows(5)[1]))
        rs.add_rows(M.to_arrays(bad))
        assert rs.runs == 2 and rs.rows == len(rows) + len(RC.part_rows(5)[1])
        msg = _refused(lambda: rs.build(str(tmp_path)), "merge: ")
        assert msg.startswith("merge: ") and "not byte-sorted" in msg
        assert not os.listdir(tmp_path)
        assert rs.runs == 2


# ---- host run layouts through build_index_from_rows and RowSet.add_rows -------------------------
@pytest.fixture(scope="module")
def laid(tmp_path_factory, oracle_lib):
    """5 parts of the small listing and a root-only run, in the layouts of RC.layouts; the
    reference of their merge by merge_heap."""
    runs = RC.part_rows(5) + [RC.ROOT_ONLY]
    merged = M.merge_heap(runs)
    assert [r[0] for r in merged] == [r[0] for r in RC.whole_rows("shapes")]
    return {"runs": runs, "ref": reference(tmp_path_factory.mktemp("rowset_layouts"), oracle_lib, merged)}


@pytest.mark.parametrize("tiers", [True, False], ids=["tiers", "no tiers"])
def test_build_index_from_rows_in_every_layout(laid, tmp_path, tiers):
    logical, runs = RC.layouts(laid["runs"], tiers)
    packed, other = tmp_path / "packed", tmp_path / "laid"
    packed.mkdir()
    other.mkdir()
    s3imph.build_index_from_rows([M.to_arrays(r)[:7 if tiers else 5] for r in logical], str(packed))
    s3imph.build_index_from_rows(runs, str(other))
    same_directory(packed, laid["ref"], tiers=tiers)
    same_directory(other, laid["ref"], tiers=tiers)


@pytest.mark.parametrize("tiers", [True, False], ids=["tiers", "no tiers"])
def test_add_rows_repacks_every_layout(laid, tmp_path, tiers):
    logical, runs = RC.layouts(laid["runs"], tiers)
    with s3imph.RowSet(with_tiers=tiers) as rs:
        held = rows = 0
        for want, run in zip(logical, runs):
            rs.add_rows(run)
            held += bool(want)
            rows += len(want)
            assert (rs.runs, rs.rows) == (held, rows)  # empty runs, NULL or not, with tier pointers or not, add none
        assert held == len(laid["runs"])
        rs.build(str(tmp_path))
    same_directory(tmp_path, laid["ref"], tiers=tiers)


def test_build_index_from_rows_with_an_empty_group_of_64(refs, tmp_path):
    """130 runs of which runs 64..127 have no rows: the first round's second group is empty."""
    c = RC.case("130 runs with 64 empty")
    runs = [M.to_arrays(r) if r else RC.layout_run([], null=True) for r in c.chunk_rows()]
    assert sum(isinstance(r, s3imph.RowRun) for r in runs[64:128]) == 64
    s3imph.build_index_from_rows(runs, str(tmp_path))
    same_directory(tmp_path, refs(c.name))
