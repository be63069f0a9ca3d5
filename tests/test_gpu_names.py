"""PrefixString for a batch on the GPU (s3imph_index_open_flags / prefixes_plan / prefixes_fill;
include/s3imph.h section 5c), against the numpy slice of (blob, offsets) in names_cases.want_names,
offset for offset and byte for byte (run on an MI355X, -m gpu).

The reference's own key sets come first (TestPrefixStringRetrieval, TestMPHFLookupWithVerify,
VerifyMPHF in pkg/format/mphf_test.go:63,133,167,244), then the emit's edges: the output is cut into
chunks of 8 * 256 = 2048 bytes and the row scan into blocks of 8 * 256 = 2048 rows."""
import numpy as np
import pytest

import names_cases as NC
import oracle as O
from index_dirs import write_index_dir, write_stats

pytestmark = pytest.mark.gpu

NOT_FOUND = NC.NOT_FOUND
CHUNK = 2048
GOLDEN_SETS = ("mphf_simple", "mphf_verify_lookup", "mphf_verify", "mphf_unicode", "mphf_large_1000")


@pytest.fixture(scope="module")
def s3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import s3imph
    return s3imph


class Edge:
    pass


@pytest.fixture(scope="module")
def edge(s3, oracle_lib, tmp_path_factory):
    """~5000 keys with every edge length, opened from a directory with S3IMPH_OPEN_PREFIXES."""
    e = Edge()
    e.keys = NC.edge_keys()
    e.n = len(e.keys)
    e.blob, e.offs = O.keys_to_blob(e.keys)
    e.dir = str(tmp_path_factory.mktemp("names"))
    write_index_dir(e.dir, oracle_lib, e.keys)
    e.idx = s3.Index(e.dir, prefixes=True)
    assert e.idx.count == e.n and e.idx.has_prefixes()
    e.at = NC.by_length(e.keys)
    yield e
    e.idx.close()


# --------------------------------------------------------------- the reference's own sets ----
@pytest.mark.parametrize("name", GOLDEN_SETS)
def test_reference_sets_round_trip(s3, name):
    keys, idx = NC.golden_index(s3, name)
    n = len(keys)
    pos = idx.lookup(keys)
    assert np.array_equal(pos, np.arange(n, dtype=np.uint64))
    assert idx.prefix_strings(pos) == keys                                   # TestPrefixStringRetrieval
    got = idx.lookup_verify(keys + [b"missing/"])                           # TestMPHFLookupWithVerify
    assert np.array_equal(got[:n], np.arange(n, dtype=np.uint64)) and got[n] == NOT_FOUND
    idx.verify()                                                             # VerifyMPHF
    assert idx.verify_device() == (0, NOT_FOUND, NOT_FOUND)
    idx.close()


# ------------------------------------------------------------------------- the emit's edges ----
def _rows_to(e, rng, lo, hi):
    """Random short rows whose lengths sum to something in [lo, hi]."""
    rows, total = [], 0
    while total < lo:
        p = int(rng.integers(0, e.n))
        ln = len(e.keys[p])
        if ln <= 64 and total + ln <= hi:
            rows.append(p)
            total += ln
    return rows, total


def _batches(e):
    rng = np.random.default_rng(17)
    n, at = e.n, e.at
    mixed = rng.integers(0, n + 40, 4099).astype(np.uint64)  # some >= n: not found
    mixed[::97] = NOT_FOUND
    mixed[5], mixed[2050], mixed[4098] = at[2500], at[1024], at[0]
    head, got = _rows_to(e, rng, 1800, 2040)
    spans = np.array(head + [at[2500]] + _rows_to(e, rng, 100, 300)[0], np.uint64)
    assert got // CHUNK == 0 and (got + 2500 - 1) // CHUNK == 2  # starts in chunk 0, ends in chunk 2
    zero = [at[0], n, NOT_FOUND, at[0]]
    k = at[1024]
    zero_runs = np.array(zero + [k, k] + zero + [k, k] + zero + [at[7]] + zero, np.uint64)
    return [
        ("nq_0", np.zeros(0, np.uint64)),
        ("nq_1", np.array([at[17]], np.uint64)),
        ("nq_1_root", np.array([at[0]], np.uint64)),
        ("nq_1_not_found", np.array([n], np.uint64)),
        ("two_scan_blocks", mixed),
        ("long_key_over_three_chunks", spans),
        ("zero_byte_runs", zero_runs),  # at the batch's start, at bytes 2048 and 4096, at the end
        ("one_position_300_times", np.full(300, at[9], np.uint64)),
        ("long_key_300_times", np.full(300, at[2500], np.uint64)),
        ("none_found", np.array([n, NOT_FOUND, n + 1] * 100, np.uint64)),
        ("descending", np.arange(n - 1, -1, -1, dtype=np.uint64)),
        ("every_edge_length", np.array([at[ln] for ln in NC.EDGE_LENGTHS] * 3, np.uint64)),
    ]


def test_zero_runs_sit_on_chunk_bounds(edge):
    """The zero_byte_runs batch puts its 0-byte rows where it says."""
    pos = dict(_batches(edge))["zero_byte_runs"]
    offs, _, _ = NC.want_names(edge.blob, edge.offs, pos)
    empty_at = {int(offs[q]) for q in range(len(pos)) if offs[q] == offs[q + 1]}
    assert empty_at == {0, CHUNK, 2 * CHUNK, 2 * CHUNK + 7}


BATCHES = ("nq_0", "nq_1", "nq_1_root", "nq_1_not_found", "two_scan_blocks", "long_key_over_three_chunks",
           "zero_byte_runs", "one_position_300_times", "long_key_300_times", "none_found", "descending",
           "every_edge_length")


@pytest.mark.parametrize("name", BATCHES)
def test_batches_match_the_numpy_slice(edge, name):
    batches = dict(_batches(edge))
    assert set(batches) == set(BATCHES)
    pos = batches[name]
    offs, found, out, total = NC.check_names(edge.idx, edge.blob, edge.offs, pos, name)
    if name == "none_found":
        assert total == 0
    if len(pos):  # the output is a key blob: straight back into the lookup
        back = edge.idx.lookup_device(out, offs, len(pos)).cpu().numpy().view(np.uint64)
        ok = pos < np.uint64(edge.n)
        assert np.array_equal(back[ok], pos[ok]), name
        # a 0-byte row that was not found reads as "" and finds the root
        assert np.all(back[~ok] == np.uint64(edge.at[0])), name


def test_output_at_odd_alignment(edge):
    import torch
    pos = dict(_batches(edge))["two_scan_blocks"]
    total = int(NC.want_names(edge.blob, edge.offs, pos)[0][-1])
    need = (total + 7) // 8 * 8
    buf = torch.full((need + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    NC.check_names(edge.idx, edge.blob, edge.offs, pos, "odd alignment", out=buf[3:3 + need])
    b = buf.cpu().numpy()
    assert np.all(b[:3] == 0xAA) and np.all(b[3 + need:] == 0xAA)  # nothing outside the slice


def test_short_cap_and_missing_plan(s3, edge):
    import torch
    idx = edge.idx
    _, _, total = idx.prefixes_plan(np.arange(100, dtype=np.uint64))
    need = (total + 7) // 8 * 8
    assert need >= 16
    with pytest.raises(s3.MPHFError) as e:
        idx.prefixes_fill(total, out=torch.empty(need - 8, dtype=torch.uint8, device="cuda"))
    assert e.value.status == s3.ERR_INVALID
    idx.prefixes_fill(total, out=torch.empty(need, dtype=torch.uint8, device="cuda"))  # the plan is still there
    fresh = s3.Index(edge.dir, prefixes=True)
    with pytest.raises(s3.MPHFError) as e:
        fresh.prefixes_fill(0)
    assert e.value.status == s3.ERR_STATE and "no plan" in str(e.value)
    fresh.close()


def test_handle_without_prefixes_answers_state(s3, edge):
    idx = s3.Index(edge.dir)  # flags == 0
    assert not idx.has_prefixes()
    calls = (lambda: idx.prefixes_plan([0]), lambda: idx.prefixes_fill(0), lambda: idx.lookup_verify([b"x"]),
             lambda: idx.verify_device(), lambda: idx.prefix_strings([0]), lambda: idx.verify())
    for call in calls:
        with pytest.raises(s3.MPHFError) as e:
            call()
        assert e.value.status == s3.ERR_STATE and "prefix blob not loaded" in str(e.value)
    assert idx.prefix_string(3) == edge.keys[3].decode()  # the host path stays as it was
    idx.close()


def test_empty_index(s3, oracle_lib, tmp_path):
    write_index_dir(str(tmp_path), oracle_lib, [])
    idx = s3.Index(str(tmp_path), prefixes=True)
    assert idx.count == 0 and idx.has_prefixes()
    blob, offs = np.zeros(0, np.uint8), np.zeros(1, np.uint64)
    NC.check_names(idx, blob, offs, np.array([0, NOT_FOUND], np.uint64), "empty index")
    assert idx.prefix_strings([0]) == [None]
    assert list(idx.lookup_verify([b"", b"a/"])) == [NOT_FOUND, NOT_FOUND]
    assert idx.verify_device() == (0, NOT_FOUND, NOT_FOUND)
    idx.verify()
    idx.close()


# ----------------------------------------------------------- beside the descendants plan ----
def _tree_keys():
    keys = {b""}
    for a in range(12):
        keys.add(b"d%02d/" % a)
        for b in range(a + 3):
            keys.add(b"d%02d/s%d/" % (a, b))
            for c in range(b % 4):
                keys.add(b"d%02d/s%d/leaf-%d/" % (a, b, c))
    return sorted(keys)


@pytest.fixture(scope="module")
def tree(s3, oracle_lib, tmp_path_factory):
    e = Edge()
    e.keys = _tree_keys()
    e.n = len(e.keys)
    e.blob, e.offs = O.keys_to_blob(e.keys)
    e.dir = str(tmp_path_factory.mktemp("names_tree"))
    e.arr = write_index_dir(e.dir, oracle_lib, e.keys)
    rng = np.random.default_rng(3)
    e.stats = (rng.integers(1, 1000, e.n).astype(np.uint64), rng.integers(1, 1 << 30, e.n).astype(np.uint64))
    write_stats(e.dir, *e.stats)
    e.idx = s3.Index(e.dir, prefixes=True)
    yield e
    e.idx.close()


def _children(e, pos, rel):
    """DescendantsAtDepth restated: the positions at depth[pos] + rel inside pos's subtree."""
    d, send = e.arr["depth"], e.arr["subtree_end"]
    return [np.array([p for p in range(q, int(send[q]) + 1) if d[p] == d[q] + rel], np.uint64) for q in pos]


def test_names_of_a_descendants_result(tree):
    e = tree
    q = np.array([0, 1, e.n - 1, 5], np.uint64)
    rows = _children(e, [int(v) for v in q], 1)
    want_pos = np.concatenate(rows)
    _, row_ptr, _, total = e.idx.descendants_plan(q, 1)
    out = e.idx.descendants_fill(total)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want_pos)
    offs, found, names = e.idx.prefixes_device(out)  # a device tensor goes straight in
    o, b = offs.cpu().numpy(), names.cpu().numpy().tobytes()
    assert [b[o[i]:o[i + 1]] for i in range(len(want_pos))] == [e.keys[int(p)] for p in want_pos]
    assert bool(found.cpu().numpy().all())
    assert e.idx.prefix_strings(want_pos) == [e.keys[int(p)] for p in want_pos]


def test_plans_do_not_disturb_each_other(tree):
    e = tree
    q = np.array([0, 2, 7], np.uint64)
    want_pos = np.concatenate(_children(e, [0, 2, 7], 1))
    names_pos = np.array([3, e.n, 0, 11, 4], np.uint64)
    w_offs, _, w_bytes = NC.want_names(e.blob, e.offs, names_pos)

    # descendants plan -> prefixes plan -> descendants fill
    _, _, n_rows, total = e.idx.descendants_plan(q, 1)
    _, _, ntotal = e.idx.prefixes_plan(names_pos)
    assert np.array_equal(e.idx.descendants_fill(total).cpu().numpy().view(np.uint64), want_pos)
    assert e.idx.prefixes_fill(ntotal).cpu().numpy().tobytes() == w_bytes.tobytes()
    # ... and the ranked rows of the still-valid descendants plan
    top_n, top_pos, _ = e.idx.top_of_plan(n_rows, "count", k=2)
    tp, tn = top_pos.cpu().numpy().view(np.uint64), top_n.cpu().numpy()
    for r, row in enumerate(_children(e, [0, 2, 7], 1)):
        order = sorted(row, key=lambda p: (-int(e.stats[0][int(p)]), int(p)))[:2]
        assert tn[r] == len(order) and [int(v) for v in tp[r][:tn[r]]] == [int(v) for v in order]

    # prefixes plan -> descendants plan -> prefixes fill
    g_offs, _, ntotal = e.idx.prefixes_plan(names_pos)
    _, _, _, total = e.idx.descendants_plan(np.array([1], np.uint64), 2)
    assert np.array_equal(g_offs.cpu().numpy().view(np.uint64), w_offs)
    assert e.idx.prefixes_fill(ntotal).cpu().numpy().tobytes() == w_bytes.tobytes()
    assert np.array_equal(e.idx.descendants_fill(total).cpu().numpy().view(np.uint64), _children(e, [1], 2)[0])
