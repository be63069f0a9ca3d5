"""tests/merge_ref.py against the reference's own test tables (tests/golden/merge/cases.json) and
against the aggregation it has to commute with: merging the rows of the parts of a listing gives
the rows of the whole listing.  No GPU."""
import numpy as np
import pytest

import merge_ref as M
import tiers_ref as T


@pytest.mark.parametrize("case", M.golden_cases(), ids=lambda c: c[0])
def test_reference_tables(case):
    _, tiers, runs, want = case
    assert M.merge_heap(runs) == want
    assert M.merge_dict(runs) == want
    assert M.first_unsorted(runs) is None
    if not tiers:
        assert M.present_mask(want) == 0


def test_named_expectations_of_the_reference():
    cases = {c[0]: c for c in M.golden_cases()}
    got = M.merge_heap(cases["TestMerger"][2])
    assert [(r[0], r[2], r[3]) for r in got] == [(b"", 12, 1200), (b"alpha/", 2, 200), (b"beta/", 4, 400),
                                                 (b"gamma/", 8, 800)]
    got = {r[0]: r for r in M.merge_heap(cases["TestParallelMerger_DuplicatePrefixes"][2])}
    assert len(got) == 4 and got[b"b/"][2] == 13 and got[b"c/"][2] == 15
    (r,) = M.merge_heap(cases["TestParallelMerger_TierDataPreserved"][2])
    assert (r[2], r[3]) == (30, 3000)
    assert (r[4][0], r[4][4], r[4][3], r[5][0]) == (20, 5, 5, 2000)
    assert M.present_mask([r]) == (1 << 0) | (1 << 3) | (1 << 4)
    assert M.merge_heap([]) == [] and M.merge_heap([[], []]) == []


def test_fold_inside_a_run_lowest_run_wins_and_wrap():
    a = [M.row("k/", 7, 1, 2), M.row("k/", 8, (1 << 64) - 1, 5), M.row("z/", 1, 1, 1)]
    b = [M.row("k/", 9, 3, (1 << 64) - 6)]
    for merge in (M.merge_heap, M.merge_dict):
        got = merge([a, b])
        assert [(r[0], r[1], r[2], r[3]) for r in got] == [(b"k/", 7, 3, 1), (b"z/", 1, 1, 1)]
        assert merge([b, a])[0][1] == 9
    assert M.first_unsorted([a, [M.row("b/"), M.row("a/")]]) == 4
    assert M.first_unsorted([[M.row("b/")], [M.row("a/")]]) is None  # a descent at a run boundary


def listing(m, seed):
    rng = np.random.default_rng(seed)
    keys = []
    for _ in range(m):
        depth = int(rng.integers(0, 5))
        dirs = [b"d%d" % int(rng.integers(0, 6)) for _ in range(depth)]
        keys.append(b"/".join(dirs) + (b"/" if depth else b"") + b"o%d" % int(rng.integers(0, 50)))
    sizes = rng.integers(0, 1 << 62, m, dtype=np.uint64)
    tiers = rng.integers(0, 12, m, dtype=np.uint8)
    return keys, sizes, tiers


@pytest.mark.parametrize("max_depth", [0, 2])
def test_merge_of_the_parts_is_the_aggregate_of_the_whole(max_depth):
    keys, sizes, tiers = listing(1500, 3 + max_depth)
    whole = T.aggregate_dict_tiers(keys, sizes, tiers, max_depth)
    rng = np.random.default_rng(11)
    for trial in range(6):
        parts = int(rng.integers(1, 9))
        owner = rng.integers(0, parts, len(keys))
        if trial % 2:
            owner[owner == parts - 1] = 0  # an empty part
        runs = []
        for p in range(parts):
            sel = np.flatnonzero(owner == p)
            runs.append(T.aggregate_dict_tiers([keys[i] for i in sel], sizes[sel], tiers[sel], max_depth))
        assert M.merge_heap(runs) == whole
        assert M.merge_dict(runs) == whole
        assert M.present_mask(whole) == T.present_mask(tiers)


def test_arrays_round_trip():
    keys, sizes, tiers = listing(200, 9)
    rows = T.aggregate_dict_tiers(keys, sizes, tiers)
    assert M.from_arrays(*M.to_arrays(rows)) == rows
    assert M.from_arrays(*M.to_arrays([])) == []
