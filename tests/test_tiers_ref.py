"""tests/tiers_ref.py reproduces the reference's own tier tests (fixtures in
tests/golden/tiers/cases.json) and agrees with itself: dict form against numpy form."""
import json
import os

import numpy as np
import pytest

import aggregate_ref as R
import oracle as O
import tiers_ref as T
from conftest import GOLDEN

CASES = json.load(open(os.path.join(GOLDEN, "tiers", "cases.json")))


def test_tier_table_matches_the_fixture():
    assert [(i, *row) for i, row in enumerate(T.TIER_TABLE)] == [tuple(r) for r in CASES["tier_table"]]
    assert len(T.TIER_TABLE) == T.NUM_TIERS


@pytest.mark.parametrize("case", CASES["index_cases"], ids=[c["name"] for c in CASES["index_cases"]])
def test_index_cases(case):
    keys = [k.encode() for k, _, _ in case["objects"]]
    assert keys == sorted(keys)
    sizes = [z for _, z, _ in case["objects"]]
    tiers = [t for _, _, t in case["objects"]]
    rows = T.aggregate_dict_tiers(keys, sizes, tiers)
    tc, tb = T.tier_arrays(rows)
    ids = T.mask_ids(T.present_mask(tiers))
    assert ids == case["present"]
    pos = {r[0].decode(): i for i, r in enumerate(rows)}
    for e in case["expect"]:
        got = {t: (b, c) for t, _, b, c in T.get_breakdown(ids, tc, tb, pos[e["prefix"]])}
        assert got[e["tier"]] == (e["bytes"], e["count"]), e
    for p, k in case.get("min_entries", {}).items():
        assert len(T.get_breakdown(ids, tc, tb, pos[p])) >= k
    for p, k in case.get("entries", {}).items():
        assert len(T.get_breakdown(ids, tc, tb, pos[p])) == k
    # the plain columns are the sums of the tier columns, and equal the plain restatement
    plain = R.aggregate_dict(keys, sizes)
    assert [r[:4] for r in rows] == plain
    assert list(tc.sum(axis=0)) == [r[2] for r in plain] and list(tb.sum(axis=0)) == [r[3] for r in plain]


@pytest.mark.parametrize("case", CASES["reader_cases"], ids=[c["name"] for c in CASES["reader_cases"]])
def test_reader_cases(case):
    n = len(case["nodes"])
    tc, tb = np.zeros((T.NUM_TIERS, n), np.uint64), np.zeros((T.NUM_TIERS, n), np.uint64)
    for i, node in enumerate(case["nodes"]):
        for t, v in node["tier_counts"].items():
            tc[int(t), i] = v
        for t, v in node["tier_bytes"].items():
            tb[int(t), i] = v
    ids = case["present"]
    if "files" in case:
        assert sorted(case["files"]) == sorted(T.TIER_TABLE[t][1] + s for t in ids for s in ("_bytes.u64", "_count.u64"))
    for pos, want in case.get("breakdown", {}).items():
        got = T.get_breakdown(ids, tc, tb, int(pos))
        assert sorted((name, b, c) for _, name, b, c in got) == sorted(tuple(w) for w in want)
    for pos, k in case.get("breakdown_len", {}).items():
        assert len(T.get_breakdown(ids, tc, tb, int(pos))) == k
    for pos, k in case.get("breakdown_all_len", {}).items():
        assert len(T.get_breakdown_all(ids, tc, tb, int(pos))) == k
    if "present_len" in case:
        assert len(json.loads(T.tiers_json(ids))["tiers"]) == case["present_len"]
    assert T.get_breakdown_all(ids, tc, tb, n) == [(t, T.TIER_TABLE[t][0], 0, 0) for t in ids]  # past the end
    assert T.get_breakdown(ids, tc, tb, n + 7) == []


def test_tiers_json_is_marshal_indent():
    m = CASES["manifest_case"]
    text = T.tiers_json(m["present"])
    assert text == (b'{\n  "tiers": [\n    {\n      "id": 0,\n      "name": "STANDARD",\n      "file": "standard"\n    },\n'
                    b'    {\n      "id": 4,\n      "name": "GLACIER",\n      "file": "glacier_fr"\n    },\n'
                    b'    {\n      "id": 7,\n      "name": "INTELLIGENT_TIERING_FREQUENT",\n      "file": "it_frequent"\n'
                    b'    }\n  ]\n}')
    doc = json.loads(text)
    assert len(doc["tiers"]) == m["n_tiers"] and [t["id"] for t in doc["tiers"]] == m["present"]
    assert all(list(t) == ["id", "name", "file"] for t in doc["tiers"])
    assert T.tiers_json([5, 0]).index(b'"id": 5') < T.tiers_json([5, 0]).index(b'"id": 0')  # the given order


def test_dict_and_numpy_forms_agree():
    rng = np.random.default_rng(77)
    alpha = np.frombuffer(b"ab/", np.uint8)
    keys = sorted(bytes(alpha[rng.integers(0, 3, rng.integers(0, 12))]) for _ in range(700))
    sizes = rng.integers(0, 1 << 62, len(keys), dtype=np.uint64)
    sizes[::9] = (1 << 64) - 1
    tiers = rng.integers(0, T.NUM_TIERS, len(keys)).astype(np.uint8)
    tiers[tiers == 6] = 3  # one tier absent
    blob, offs = O.keys_to_blob(keys)
    for md in (0, 2):
        rows = T.aggregate_dict_tiers(keys, sizes, tiers, md)
        tc, tb = T.tier_arrays(rows)
        nrows, ntc, ntb = T.tier_columns_numpy(blob, offs, sizes, tiers, md)
        assert np.array_equal(nrows[3], np.array([r[2] for r in rows], np.uint64))
        assert np.array_equal(tc, ntc) and np.array_equal(tb, ntb)
        assert not tc[6].any() and T.present_mask(tiers) == 0xfff & ~(1 << 6)
        with np.errstate(over="ignore"):
            assert np.array_equal(tc.sum(axis=0, dtype=np.uint64), nrows[3])
            assert np.array_equal(tb.sum(axis=0, dtype=np.uint64), nrows[4])


def test_bad_tier_id_is_out_of_range():
    with pytest.raises(IndexError):
        T.aggregate_dict_tiers([b"a/b"], [1], [12])
