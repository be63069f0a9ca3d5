"""tests/rowset_cases.py on its own (no GPU): the reference model is closed under every chunking
the generator makes — each chunk's reference rows, merged by merge_ref.merge_heap in chunk order,
are the reference rows of the whole listing, in rows, depths, counts, bytes, the 24 tier columns
and present_mask — without which tests/test_gpu_rowset.py could not compare a chunked build with
the whole-listing reference; every listing has the property it was built for; and the run layouts
decode to the rows they were made from."""
import numpy as np
import pytest

import aggregate_ref as R
import csv_ref as C
import merge_ref as M
import rowset_cases as RC
import tiers_ref as T


@pytest.mark.parametrize("name", RC.NAMES)
def test_the_model_is_closed_under_the_chunking(name):
    c = RC.case(name)
    keys, sizes, tiers = c.objects()
    runs = c.chunk_rows()
    whole = RC.whole_rows(name)
    merged = M.merge_heap(runs)
    assert merged == whole == M.merge_dict(runs)
    assert M.to_arrays(merged)[5].tobytes() == T.tier_arrays(whole)[0].tobytes()
    assert M.present_mask(merged) == T.present_mask(tiers)
    # the tier-less reference agrees on everything but the tier columns
    plain = R.aggregate_dict(keys, sizes, c.max_depth)
    assert [tuple(r[:4]) for r in plain] == [r[:4] for r in whole]
    assert max(r[1] for r in whole) == (c.max_depth or max(k.count(b"/") for k in keys))
    assert sum(len(r) for r in runs) > len(whole)  # the merge has something to fold
    for ch in c.chunks:  # a CSV chunk reads back as its objects
        if ch.how == "csv":
            rec = C.records(ch.csv(), RC.SCHEMA)
            assert rec["keys"] == ch.keys and np.array_equal(rec["sizes"], ch.sizes)
            assert np.array_equal(rec["tiers"], ch.tiers)


def test_names_cover_the_cases():
    assert sorted(RC.NAMES) == sorted(RC._cases())
    assert {(RC.case(n).max_depth, RC.case(n).with_tiers) for n in RC.NAMES} >= {(0, True), (1, True), (3, False),
                                                                               (0, False)}


def test_each_segment_has_the_shape_it_is_named_for():
    s = RC.small()
    assert 2900 <= sum(len(s[n][0]) for n in RC.SEGMENTS) <= 3100
    bulk = s["bulk"][0]
    assert len(set(bulk)) == len(bulk) == 2400 and sorted(bulk) != bulk
    again = s["again"][0]
    assert len(set(again)) == 100 and all(again.count(k) == 2 and k in bulk for k in set(again))
    srt, rev = s["sorted"][0], s["reverse"][0]
    assert len(srt) > 100 and srt == sorted(srt) and len(set(srt)) == len(srt)  # the sort's identity path
    assert len(rev) > 100 and rev == sorted(rev, reverse=True) and rev != sorted(rev)
    assert len(s["one"][0]) == 1
    flat = s["flat"][0]
    assert len(flat) > 1 and not any(b"/" in k for k in flat)
    assert [r[0] for r in T.aggregate_dict_tiers(*s["flat"])] == [b""]           # a root row only
    assert s["empty"][0] == [b""] * 10
    assert [r[:3] for r in T.aggregate_dict_tiers(*s["empty"])] == [(b"", 0, 10)]
    # prefix x/ occurs in three chunks of the shaped chunking (sorted, reverse, one), x/y/ in two
    shaped = RC.case("shapes")
    has = [any(r[0] == b"x/" for r in rows) for rows in shaped.chunk_rows()]
    assert sum(has) == 3 and sum(any(r[0] == b"x/y/" for r in rows) for rows in shaped.chunk_rows()) == 2
    # the root is in every chunk that has an object
    assert all(rows[0][0] == b"" for rows in shaped.chunk_rows() if rows)


def test_the_dropped_csv_chunk_holds_records_and_no_object():
    rec = C.records(RC.CSV_ALL_DROPPED, RC.SCHEMA)
    info = rec["info"]
    assert rec["keys"] == [] and info["n_records"] == 5 and info["n_short"] == 3 and info["n_empty_key"] == 2
    for name, at in (("shapes", 3), ("csv no tiers", 2), ("csv depth 1", 0)):
        ch = RC.case(name).chunks[at]
        assert ch.how == "csv" and ch.raw == RC.CSV_ALL_DROPPED and ch.keys == []


def test_chunk_counts_reach_the_rounds():
    assert len(RC.case("65 chunks").chunks) == 65 and len(RC.case("130 chunks").chunks) == 130
    assert all(ch.keys for ch in RC.case("130 chunks").chunks)
    c = RC.case("130 runs with 64 empty")
    rows = c.chunk_rows()
    assert len(rows) == 130 and [r for r in range(130) if not rows[r]] == list(range(64, 128))
    assert all(ch.how == "rows" for ch in c.chunks)
    assert M.merge_heap(RC.part_rows(65)) == RC.whole_rows("shapes") == RC.whole_rows("130 chunks")


def test_the_deep_key_and_its_ancestors_are_in_different_chunks():
    first, second = RC.case("deep").chunks
    assert second.keys == [RC.DEEP_KEY] and RC.DEEP_KEY.count(b"/") == 100
    a, b = RC.case("deep").chunk_rows()
    assert max(r[1] for r in a) < 62 and max(r[1] for r in b) == 100 and len(b) == 101
    shared = {r[0] for r in a} & {r[0] for r in b}
    assert shared == {b"", b"deep/", b"deep/x/", b"deep/x/x/"}
    assert max(r[1] for r in RC.whole_rows("deep")) == 100


def test_the_extension_adds_new_and_known_prefixes():
    old, new = RC.whole_rows("shapes"), RC.whole_rows("extended")
    assert RC.case("extended").chunks[:-1][0].keys == RC.case("shapes").chunks[0].keys
    assert len(new) == len(old) and new != old  # no new prefix, other sums
    assert dict((r[0], r[2]) for r in new)[b""] == dict((r[0], r[2]) for r in old)[b""] + 4


@pytest.mark.parametrize("tiers", [True, False])
def test_layouts_decode_to_their_rows(tiers):
    runs = RC.part_rows(5)[:4] + [RC.ROOT_ONLY]
    logical, laid = RC.layouts(runs, tiers)
    assert [r for r in logical if r] == runs
    empties = [i for i, r in enumerate(logical) if not r]
    assert empties[0] == 0 and empties[-1] == len(logical) - 1 and any(0 < i - 2 < len(logical) - 4 for i in empties)
    want = logical if tiers else [RC.strip_tiers(r) for r in logical]
    bases, strides = set(), set()
    for rows, w, run in zip(logical, want, laid):
        assert RC.decode_run(run) == w
        if run.n:
            offs = run.arrays[1]
            bases.add(int(offs[0]))
            assert bool(run.tier_count) == bool(run.tier_bytes) == tiers
            strides.add(int(run.tier_stride) - int(run.n) if tiers else 0)
            blob = run.arrays[0]
            assert (blob[:int(offs[0])] == RC.JUNK).all() and (blob[int(offs[-1]):] == RC.JUNK).all()
            if tiers:
                assert (run.arrays[5][:, int(run.n):] == RC.SLACK).all()
    assert bases == {1, 5, 8, 13, 7} and strides == ({0, 3} if tiers else {0})
    nulls = [run for run in laid if not run.n and not run.offsets]
    real = [run for run in laid if not run.n and run.offsets]
    assert len(nulls) == 3 and len(real) == 3 and all(not (r.blob or r.depth or r.tier_count) for r in nulls)
    assert sum(bool(r.tier_count) != tiers for r in real) == 1  # one empty run disagrees about tier columns
    root = laid[[i for i, r in enumerate(logical) if r == RC.ROOT_ONLY][0]]
    assert not root.blob and root.arrays[1].tolist() == [7, 7]
    # the merge reference sees the same rows in both layouts
    assert M.merge_heap(logical) == M.merge_heap(runs)
