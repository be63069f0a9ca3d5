"""The aggregation restatements (tests/aggregate_ref.py) against the reference's own test
values (tests/golden/aggregate/cases.json) and against each other — no GPU."""
import json
import os

import numpy as np
import pytest

import aggregate_ref as R
import oracle as O
from conftest import GOLDEN

CASES = json.load(open(os.path.join(GOLDEN, "aggregate", "cases.json")))["cases"]


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_dict_form_reproduces_the_reference_tests(case):
    keys = [k.encode() for k, _ in case["objects"]]
    sizes = [z for _, z in case["objects"]]
    assert keys == sorted(keys)
    rows = R.aggregate_dict(keys, sizes, case["max_depth"])
    if "n_rows" in case:
        assert len(rows) == case["n_rows"]
    if "prefixes" in case:
        assert [r[0].decode() for r in rows] == case["prefixes"]
    if "depths" in case:
        assert [r[1] for r in rows] == case["depths"]
    if "object_count" in case:
        assert rows[0][2] == case["object_count"] and rows[0][3] == case["bytes_processed"]
    by = {r[0].decode(): r for r in rows}
    for p, want in case.get("stats", {}).items():
        assert by[p][2] == want["object_count"], p
        if "total_bytes" in want:
            assert by[p][3] == want["total_bytes"], p


def random_listing(rng, m):
    """Sorted keys over an alphabet with bytes below '/', above it and at or above 0x80."""
    alpha = np.frombuffer(b"ab/!~\xc3", np.uint8)
    keys = sorted(bytes(alpha[rng.integers(0, len(alpha), rng.integers(0, 9))]) for _ in range(m))
    big = np.array([0, 1, 7, 1 << 63, (1 << 64) - 1, 12345], np.uint64)
    return keys, big[rng.integers(0, len(big), m)]


@pytest.mark.parametrize("max_depth", [0, 1, 2])
def test_numpy_form_equals_dict_form(max_depth):
    rng = np.random.default_rng(100 + max_depth)
    for _ in range(300):
        keys, sizes = random_listing(rng, int(rng.integers(0, 40)))
        want = R.rows_to_arrays(R.aggregate_dict(keys, sizes, max_depth))
        blob, offs = O.keys_to_blob(keys)
        got = R.aggregate_numpy(blob, offs, sizes, max_depth)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (keys, list(sizes))


def test_rows_are_byte_sorted_and_distinct():
    rng = np.random.default_rng(7)
    keys, sizes = random_listing(rng, 500)
    blob, offs = O.keys_to_blob(keys)
    out = R.aggregate_numpy(blob, offs, sizes)
    prefixes = R.keys_of(out[0], out[1])
    assert prefixes == sorted(set(prefixes)) and prefixes[0] == b""
