"""The staging-window regimes of k_fin_keys_lds, decided on the CPU from the offsets alone
(finalize_regimes.walk):

  - the key sets tests/test_gpu_finalize.py has used so far reach neither a cut round nor a
    key that misses the window: the gap tests/test_gpu_finalize_keys.py closes;
  - each key set of finalize_keysets meets the coverage condition it was built for;
  - on those sets the two independent restatements of the reference's finalize, the C
    oracle and oracle.py_finalize, agree: the expected values are pinned before a GPU runs.
"""
import numpy as np
import pytest

import finalize_keysets as K
import finalize_regimes as W
import oracle as O
from test_gpu_finalize import _prefix_set

ARRAYS = ("depth", "subtree_end", "max_depth_in_subtree", "depth_offsets", "depth_positions", "max_depth")


def _as_lists(arr):
    return {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in arr.items()}


def _offsets(keys):
    offs = np.zeros(len(keys) + 1, np.uint64)
    offs[1:] = np.cumsum([len(k) for k in keys], dtype=np.uint64)
    return offs


# ------------------------------------------------------------- the walker itself ----
def test_walker_on_hand_made_rounds():
    # 3 keys of 16 KiB: two fill the window exactly, the third waits for the next round
    w = W.walk(np.arange(4, dtype=np.uint64) * 16384)
    assert w == {"rounds": 2, "cut": 1, "oversize": 0, "exact": 1, "fit": 3}
    # one key of 32 KiB + 1: it does not fit, alone or not
    w = W.walk(np.array([0, 32769, 32770], np.uint64))
    assert w == {"rounds": 2, "cut": 0, "oversize": 1, "exact": 0, "fit": 1}
    # a round starting at byte 24 has its window from byte 16: the 32 760-byte key fills it to
    # its last byte (16 + 32 KiB) after the first round was cut before it; the third key waits
    w = W.walk(np.array([0, 24, 24 + 32760, 24 + 32761], np.uint64) + 5)  # offsets[0] is rebased
    assert w == {"rounds": 3, "cut": 2, "oversize": 0, "exact": 1, "fit": 3}
    # 1025 one-byte keys: two workgroups of 513 and 512 keys, the first needs two rounds
    w = W.walk(np.arange(1026, dtype=np.uint64))
    assert w == {"rounds": 3, "cut": 0, "oversize": 0, "exact": 0, "fit": 1025}
    assert W.walk(np.zeros(1, np.uint64))["rounds"] == 0
    assert (W.kFinT, W.kFinBB, W.kFinGrid) == (256, 32768, 4096)


# ------------------------------------------------------------- the gap, recorded ----
# test_random_trees' parameters, closed and not, and test_unaligned_caller_depths' (closed only)
EXISTING = [(s, n, f, d, c) for (s, n, f, d) in [(1, 2000, 4, 5), (2, 200_000, 16, 9), (3, 400_000, 64, 4)]
            for c in (True, False)] + [(7, 3000, 8, 7, True), (7, 300_000, 8, 7, True)]


@pytest.mark.parametrize("seed,n_obj,fan,depth,closed", EXISTING)
def test_existing_random_trees_reach_neither_regime(seed, n_obj, fan, depth, closed):
    w = W.walk(_offsets(_prefix_set(seed, n_obj, fan, depth, closed)))
    assert w["rounds"] > 0 and w["cut"] == 0 and w["oversize"] == 0, w


def test_existing_wide_subtrees_reach_neither_regime():
    """test_wide_subtrees_cross_superblocks: b"", then per top b"t%d/" and its 11-byte children."""
    lens = [0]
    for top in range(3):
        lens += [3] + [11] * (700_000 + 123_457 * top)
    offs = np.zeros(len(lens) + 1, np.uint64)
    offs[1:] = np.cumsum(lens, dtype=np.uint64)
    w = W.walk(offs)
    assert w["rounds"] > 0 and w["cut"] == 0 and w["oversize"] == 0, w


# ------------------------------------------------------- the new sets' conditions ----
@pytest.mark.parametrize("name", [n for n, (_, cond) in K.SETS.items() if cond is not None])
def test_key_set_meets_its_coverage_condition(name):
    keys = K.keyset(name)
    w = W.walk(_offsets(keys))
    print(name, len(keys), "keys", sum(map(len, keys)), "bytes", w)
    assert K.SETS[name][1](w), (name, w)


@pytest.mark.parametrize("name", list(K.SETS))
def test_key_sets_are_sorted_distinct_and_small(name):
    keys = K.keyset(name)
    assert all(a < b for a, b in zip(keys, keys[1:]))
    assert sum(map(len, keys)) <= 1_200_000 and len(keys) <= 6000


def test_key_set_shapes():
    comb = K.keyset("comb")
    assert len(comb) == 1201 and sum(map(len, comb)) == 360_600
    assert K.keyset("oversize_first")[0] == K._big()[:40_000]
    assert K.keyset("oversize_last")[-1] == K._big()[:40_000]
    nested = K.keyset("oversize_nested")
    assert [len(k) - 2 for k in nested[300:305]] == list(K.NESTED_LENGTHS)
    fit = K.keyset("exact_fit")
    assert sum(map(len, fit[:32])) == W.kFinBB
    assert sum(map(len, K.keyset("exact_fit_plus1")[:33])) == W.kFinBB + 1
    for n in K.BLOCK_EDGE_N:
        assert len(K.comb_cut(n)) == n
    # the block-edge combs hold keys that leave the spine, not its prefixes only
    assert len({len(k) for k in K.comb_cut(5)}) < 5


# -------------------------------------------------- the expected values, pinned ----
def test_comb_has_one_subtree_end_per_prefix(oracle_lib):
    for name in ("comb", "comb_flip"):
        arr = oracle_lib.finalize(*K.blob_of(K.keyset(name)))
        assert len(set(arr["subtree_end"].tolist())) == 601, name


def test_mask_leak_depth_is_length_or_zero(oracle_lib):
    keys = K.keyset("mask_leak")
    arr = oracle_lib.finalize(*K.blob_of(keys))
    assert arr["depth"].tolist() == [len(k) if k[0] == 0x2F else 0 for k in keys]
    assert set(oracle_lib.finalize(*K.blob_of(K.keyset("slash_sweep")))["depth"].tolist()) == {1}


def test_ragged_needs_the_depth_offsets_retry(oracle_lib):
    arr = oracle_lib.finalize(*K.blob_of(K.keyset("ragged")))
    assert arr["max_depth"] >= 63  # beyond the 64 depth_offsets entries of the first offer
    assert int((arr["subtree_end"] > np.arange(len(arr["subtree_end"]), dtype=np.uint64)).sum()) >= 100


def test_nested_oversize_has_four_internal_nodes(oracle_lib):
    arr = oracle_lib.finalize(*K.blob_of(K.keyset("oversize_nested")))
    assert arr["subtree_end"][300:305].tolist() == [304] * 5
    assert int((arr["subtree_end"] != np.arange(605, dtype=np.uint64)).sum()) == 4


@pytest.mark.parametrize("depths", ["slashes", "hashed"])
@pytest.mark.parametrize("name", list(K.SETS))
def test_two_oracle_restatements_agree(oracle_lib, name, depths):
    keys = list(K.keyset(name))
    d = None if depths == "slashes" else K.hashed_depths(len(keys))
    got = _as_lists(oracle_lib.finalize(*K.blob_of(keys), d))
    want = O.py_finalize(keys, None if d is None else d.tolist())
    for k in ARRAYS:
        assert got[k] == want[k], k


@pytest.mark.parametrize("n", K.BLOCK_EDGE_N)
def test_two_oracle_restatements_agree_on_block_edge_combs(oracle_lib, n):
    keys = K.comb_cut(n)
    d = K.hashed_depths(n)
    got = _as_lists(oracle_lib.finalize(*K.blob_of(keys), d))
    want = O.py_finalize(keys, d.tolist())
    for k in ARRAYS:
        assert got[k] == want[k], k


@pytest.mark.parametrize("d", [v for v in K.EDGE_DEPTHS if v <= 256])
def test_two_oracle_restatements_agree_on_depth_edges(oracle_lib, d):
    """py_finalize walks every depth over every key: the 16- and 17-bit depths are left to
    the C oracle alone."""
    keys = K.short_tree()
    depths = K.edge_depths(len(keys), [(1234, d)])
    got = _as_lists(oracle_lib.finalize(*K.blob_of(keys), depths))
    want = O.py_finalize(keys, depths.tolist())
    for k in ARRAYS:
        assert got[k] == want[k], k
    assert got["depth_offsets"][1:d + 1] == [len(keys) - 1] * d
