"""indexread.Index on the GPU (s3imph.Index; include/s3imph.h section 5c): Open, Lookup,
Stats / Depth / SubtreeEnd / MaxDepthInSubtree, DescendantsAtDepth[Filtered] and
DescendantsUpToDepth for whole batches, against the reference's reader restated in
tests/finalize_queries.py (run on an MI355X, -m gpu).

The index under test never comes from the GPU build: the MPHF is oracle_lib.build's, the
finalize arrays oracle_lib.finalize's (index_dirs.write_index_dir), so the queries are
checked on their own.  Only the last test builds and finalizes on the GPU, end to end.

Expected answers.  finalize_queries.py turns a whole depth slice into a Python list per
call, which is fine for the exhaustive small trees and too slow for batches of thousands of
queries over 10^5-entry slices.  Those use `_at` / `_upto` below, the same two binary searches
through numpy.searchsorted; every test that uses them first checks them equal to
finalize_queries on a sample of its own batch (and the exhaustive tests check them on every
query), so finalize_queries stays the reference throughout.  Everything is integer: all
comparisons are exact.
"""
import json
import os

import numpy as np
import pytest

import finalize_queries as Q
import oracle as O
from conftest import GOLDEN
from index_dirs import write_index_dir, write_stats

pytestmark = pytest.mark.gpu

CASES = json.load(open(os.path.join(GOLDEN, "finalize", "cases.json")))
NOT_FOUND = 2**64 - 1
CHUNK_KS = [255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 65535, 65536, 65537]


@pytest.fixture(scope="module")
def s3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import s3imph
    return s3imph


# ------------------------------------------------------------------------ restatements ----
def _at(arr, pos, rel):
    """finalize_queries.descendants_at_depth through numpy (None = the reference's nil)."""
    if pos >= len(arr["depth"]):
        return None
    t = int(arr["depth"][pos]) + rel
    if rel < 0 or t > arr["max_depth"]:
        return None
    o = arr["depth_offsets"]
    sl = arr["depth_positions"][int(o[t]):int(o[t + 1])]
    lo = np.searchsorted(sl, np.uint64(pos), "left")
    hi = np.searchsorted(sl, arr["subtree_end"][pos], "right")
    return sl[lo:max(lo, hi)]


def _upto(arr, pos, max_rel):
    """finalize_queries.descendants_up_to_depth through numpy."""
    if pos >= len(arr["depth"]):
        return None
    base, msd = int(arr["depth"][pos]), int(arr["max_depth_in_subtree"][pos])
    if max_rel < 0 or min(msd - base, max_rel) <= 0:
        return None
    return [_at(arr, pos, j) for j in range(1, min(msd - base, max_rel) + 1)]


def _filtered(positions, stats, min_count, min_bytes):
    """DescendantsAtDepthFiltered, index.go:283-295."""
    if positions is None or (min_count == 0 and min_bytes == 0):
        return positions
    at = positions.astype(np.int64)
    keep = (stats[0][at] >= np.uint64(min_count)) & (stats[1][at] >= np.uint64(min_bytes))
    return positions[keep]


def _q_at(arr, pos, rel):
    return None if pos >= len(arr["depth"]) else Q.descendants_at_depth(arr, pos, rel)


def _q_upto(arr, pos, max_rel):
    return None if pos >= len(arr["depth"]) else Q.descendants_up_to_depth(arr, pos, max_rel)


def _same_row(got, want):
    if want is None or got is None:
        return want is None and got is None
    return len(got) == len(want) and np.array_equal(np.asarray(got, np.uint64), np.asarray(want, np.uint64))


def _check_at(got, want, what):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        assert _same_row(g, w), (what, q)


def _check_upto(got, want, what):
    assert len(got) == len(want)
    for q, (g, w) in enumerate(zip(got, want)):
        if w is None or g is None:
            assert w is None and g is None, (what, q)
            continue
        assert len(g) == len(w), (what, q)
        for j, (gr, wr) in enumerate(zip(g, w)):
            assert _same_row(gr, wr), (what, q, j)


def _exhaustive(idx, arr, what):
    """Every pos in [0, n] and rel in [-1, maxDepth + 2] (AT), every max_rel in
    [-1, maxDepth + 1] (UPTO) against finalize_queries; the numpy forms on the way."""
    n, md = len(arr["depth"]), arr["max_depth"]
    assert idx.count == n and idx.max_depth == md
    pos = np.repeat(np.arange(n + 1, dtype=np.uint64), md + 4)
    rel = np.tile(np.arange(-1, md + 3, dtype=np.int32), n + 1)
    want = [_q_at(arr, int(p), int(r)) for p, r in zip(pos, rel)]
    _check_at([_at(arr, int(p), int(r)) for p, r in zip(pos, rel)], want, what + " numpy AT")
    _check_at(idx.descendants_at_depth(pos, rel), want, what + " AT")
    allpos = np.arange(n + 1, dtype=np.uint64)
    for max_rel in range(-1, md + 2):
        want = [_q_upto(arr, int(p), max_rel) for p in allpos]
        _check_upto([_upto(arr, int(p), max_rel) for p in allpos], want, what + " numpy UPTO %d" % max_rel)
        _check_upto(idx.descendants_up_to_depth(allpos, max_rel), want, what + " UPTO %d" % max_rel)


def _prefix_set(seed, n_objects, fanout, max_depth, closed):
    rng = np.random.default_rng(seed)
    s = {""} if closed else set()
    for _ in range(n_objects):
        d = int(rng.integers(1, max_depth + 1))
        parts = ["%x" % int(rng.integers(0, fanout)) for _ in range(d)]
        if closed:
            for j in range(1, d + 1):
                s.add("/".join(parts[:j]) + "/")
        else:
            s.add("/".join(parts) + "/")
    return sorted(k.encode() for k in s)


def _random_stats(seed, n):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 2**64, n, dtype=np.uint64), rng.integers(0, 2**64, n, dtype=np.uint64))


# ---------------------------------------------------------------------------- fixtures ----
class Tree:
    def __init__(self, s3, oracle_lib, path, keys, stats=None, depths=None):
        self.keys, self.stats, self.dir = keys, stats, str(path)
        self.arr = write_index_dir(self.dir, oracle_lib, keys, stats, depths)
        self.n = len(keys)
        self.idx = s3.Index(self.dir)


@pytest.fixture(scope="module")
def big(s3, oracle_lib, tmp_path_factory):
    """(seed 2, 200 000 objects, fan-out 16, depth 9), ancestor-closed, with random stats, and
    its sampled batch of 4096 (pos, rel) pairs."""
    keys = _prefix_set(2, 200_000, 16, 9, True)
    t = Tree(s3, oracle_lib, tmp_path_factory.mktemp("big"), keys, _random_stats(22, len(keys)))
    rng = np.random.default_rng(5)
    t.qpos = rng.integers(0, t.n + 1, 4096).astype(np.uint64)  # n itself: out of range
    t.qpos[:64] = rng.integers(0, 40, 64)                       # shallow nodes: long rows
    t.qrel = rng.integers(-1, t.arr["max_depth"] + 3, 4096).astype(np.int32)
    t.want = [_at(t.arr, int(p), int(r)) for p, r in zip(t.qpos, t.qrel)]
    for q in range(0, 4096, 64):  # the numpy form against finalize_queries on a sample
        assert _same_row(t.want[q], _q_at(t.arr, int(t.qpos[q]), int(t.qrel[q]))), q
    yield t
    t.idx.close()


def _chunk_keys():
    keys = [b""]
    for K in CHUNK_KS:
        keys.append(b"n%d/" % K)
        keys.extend(b"n%d/%05x/" % (K, i) for i in range(K))
    keys.append(b"z/")
    return sorted(keys)


@pytest.fixture(scope="module")
def chunky(s3, oracle_lib, tmp_path_factory):
    """Row lengths on both sides of the fill's 2048-position chunk (and of every other power
    of two up to 65536) next to empty rows; random stats with values on both sides of 2^63."""
    keys = _chunk_keys()
    t = Tree(s3, oracle_lib, tmp_path_factory.mktemp("chunky"), keys, _random_stats(33, len(keys)))
    at = {k: i for i, k in enumerate(keys)}
    z, root = at[b"z/"], at[b""]
    skew = []
    for K in CHUNK_KS:
        skew += [z, at[b"n%d/" % K], z]
    skew += [root, z]
    t.batches = [("skew", np.array(skew, np.uint64), 1), ("grandchildren", np.array([root], np.uint64), 2),
                 ("equal", np.full(70_000, at[b"n257/"], np.uint64), 1)]
    t.at = at
    yield t
    t.idx.close()


# ------------------------------------------------------------------------------- tests ----
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_cases(s3, oracle_lib, tmp_path, case):
    keys = [k.encode() for k in case["keys"]]
    t = Tree(s3, oracle_lib, tmp_path, keys, depths=case.get("depths"))
    idx, at = t.idx, {k: i for i, k in enumerate(case["keys"])}
    for key, rel, names, count in case.get("descendants_at_depth", []):
        got = idx.descendants_at_depth([at[key]], rel)[0]
        assert len(got) == count, (key, rel)
        if names is not None:
            assert [case["keys"][int(p)] for p in got] == names, (key, rel)
    for key, max_rel, sizes in case.get("descendants_up_to_depth", []):
        got = idx.descendants_up_to_depth([at[key]], max_rel)[0]
        assert [len(g) for g in got] == sizes, (key, max_rel)
    _exhaustive(idx, t.arr, case["name"])
    idx.close()


@pytest.mark.parametrize("closed", [True, False])
def test_random_tree_exhaustive(s3, oracle_lib, tmp_path, closed):
    t = Tree(s3, oracle_lib, tmp_path, _prefix_set(1, 2000, 4, 5, closed))
    _exhaustive(t.idx, t.arr, "seed 1")
    t.idx.close()


def test_random_tree_sampled_batch(big):
    """4096 (pos, rel) pairs in one batch; then the root at every rel and UPTO of the root at
    max_rel = 9: rows of 10^5 entries next to empty ones."""
    _check_at(big.idx.descendants_at_depth(big.qpos, big.qrel), big.want, "sampled")
    md = big.arr["max_depth"]
    rels = np.arange(-1, md + 3, dtype=np.int32)
    want = [_at(big.arr, 0, int(r)) for r in rels]
    assert _same_row(want[3], _q_at(big.arr, 0, 2)) and max(len(w) for w in want if w is not None) > 100_000
    _check_at(big.idx.descendants_at_depth(np.zeros(len(rels), np.uint64), rels), want, "root")
    pos = np.array([big.n - 1, 0, big.n, 1], np.uint64)
    want = [_upto(big.arr, int(p), 9) for p in pos]
    assert want[0] is None and want[2] is None and len(want[1]) == 9
    got = big.idx.descendants_up_to_depth(pos, 9)
    _check_upto(got, want, "root UPTO")
    _check_upto(got[3:], [_q_upto(big.arr, 1, 9)], "UPTO against finalize_queries")


def test_chunk_edges_and_skew(chunky):
    for name, pos, rel in chunky.batches:
        want = [_at(chunky.arr, int(p), rel) for p in (pos if name != "equal" else pos[:1])]
        if name == "equal":
            want = want * len(pos)
        for q in ((1, 4, len(pos) - 2) if name == "skew" else (0,)):  # n255, n256, the root
            assert _same_row(want[q], _q_at(chunky.arr, int(pos[q]), rel)), (name, q)
        if name == "skew":
            assert [len(w) for w in want[1::3]][:len(CHUNK_KS)] == CHUNK_KS and len(want[-2]) == 16
        if name == "grandchildren":
            assert len(want[0]) == sum(CHUNK_KS)
        levels, row_ptr, out = chunky.idx.descendants_csr(pos, rel)
        rp = row_ptr.cpu().numpy()
        assert levels.cpu().numpy().tolist() == [1] * len(pos), name
        assert np.array_equal(rp, np.concatenate([[0], np.cumsum([len(w) for w in want])])), name
        assert np.array_equal(out.cpu().numpy().view(np.uint64), np.concatenate(want)), name


FILTERS = [(0, 0), (2**63, 0), (0, 2**63), (2**62, 2**62), (2**64 - 1, 2**64 - 1)]


@pytest.mark.parametrize("min_count,min_bytes", FILTERS)
def test_filter(chunky, min_count, min_bytes):
    """Stats drawn from the whole u64 range: a signed compare gets the values >= 2^63 wrong."""
    for name, pos, rel in chunky.batches[:2]:
        plain = [_at(chunky.arr, int(p), rel) for p in pos]
        want = [_filtered(w, chunky.stats, min_count, min_bytes) for w in plain]
        for w, p in zip(want, plain):  # index.go:283-295, position by position, on the short rows
            if len(p) <= 4097:
                assert [int(x) for x in w] == [
                    int(x) for x in p if (min_count == 0 and min_bytes == 0) or
                    (int(chunky.stats[0][x]) >= min_count and int(chunky.stats[1][x]) >= min_bytes)]
        kept, total = sum(len(w) for w in want), sum(len(p) for p in plain)
        if (min_count, min_bytes) == (0, 0):
            assert kept == total
        elif min_count == 2**64 - 1:
            assert kept < 4
        else:
            assert total // 8 < kept < total * 3 // 4
        _check_at(chunky.idx.descendants_at_depth(pos, rel, min_count, min_bytes), want, name)


def test_filter_needs_stats_and_at_mode(s3, oracle_lib, tmp_path, chunky):
    t = Tree(s3, oracle_lib, tmp_path, [b"", b"a/", b"a/b/", b"b/", b"c/"])
    r = t.idx.nodes(np.arange(5, dtype=np.uint64))
    assert r["found"].tolist() == [1] * 5
    assert r["object_count"].tolist() == [0] * 5 and r["total_bytes"].tolist() == [0] * 5
    for f in ((1, 0), (0, 1)):
        with pytest.raises(s3.MPHFError) as e:
            t.idx.descendants_at_depth([0], 1, *f)
        assert e.value.status == s3.ERR_STATE
    _check_at(t.idx.descendants_at_depth([0, 1], 1, 0, 0), [_q_at(t.arr, 0, 1), _q_at(t.arr, 1, 1)], "no stats")
    for idx in (t.idx, chunky.idx):  # a filter with UPTO: invalid with or without stats
        with pytest.raises(s3.MPHFError) as e:
            idx.descendants_plan([0], None, 2, 1, 0)
        assert e.value.status == s3.ERR_INVALID
    t.idx.close()


def test_lookup_and_nodes(s3, big):
    """StatsForPrefix on every member, on the same keys with one byte appended and on the
    empty key; nodes past the end; the query blob at a misaligned device address."""
    import torch
    arr, n, idx = big.arr, big.n, big.idx
    blob, offs = O.keys_to_blob(big.keys)
    pos = idx.lookup_blob(blob, offs)
    assert np.array_equal(pos, np.arange(n, dtype=np.uint64))
    r = idx.nodes(pos)
    assert r["found"].all() and np.array_equal(r["pos"], pos)
    assert np.array_equal(r["object_count"], big.stats[0]) and np.array_equal(r["total_bytes"], big.stats[1])
    for f in ("depth", "subtree_end", "max_depth_in_subtree"):
        assert np.array_equal(r[f], arr[f]), f
    found, oc, tb = idx.stats_for_prefix_blob(blob, offs)
    assert found.all() and np.array_equal(oc, big.stats[0]) and np.array_equal(tb, big.stats[1])
    # non-members: every key with one byte appended (no member ends in 'x')
    lens = np.diff(offs.astype(np.int64))
    offs2 = offs + np.arange(n + 1, dtype=np.uint64)
    blob2 = np.full(int(offs2[-1]), ord("x"), np.uint8)
    keep = np.ones(len(blob2), bool)
    keep[(offs2[1:] - np.uint64(1)).astype(np.int64)] = False
    blob2[keep] = blob
    assert bytes(blob2[int(offs2[1]):int(offs2[2])]) == big.keys[1] + b"x" and lens[0] == 0
    assert (idx.lookup_blob(blob2, offs2) == np.uint64(NOT_FOUND)).all()
    found, oc, tb = idx.stats_for_prefix_blob(blob2, offs2)
    assert not found.any() and not oc.any() and not tb.any()
    found, oc, tb = idx.stats_for_prefix([b"", b"nope/"])
    assert found.tolist() == [True, False] and int(oc[0]) == int(big.stats[0][0]) and int(oc[1]) == 0
    r = idx.nodes(np.array([n, NOT_FOUND, n - 1], np.uint64))
    assert r["found"].tolist() == [0, 0, 1]
    assert r[:2].tobytes() == bytes(2 * s3.NODE_DTYPE.itemsize)
    # the same member lookup from a view 3 bytes into a 16-byte aligned allocation
    m = 50_000
    nb = int(offs[m])
    buf = torch.zeros(3 + (nb + 7) // 8 * 8 + 16, dtype=torch.uint8, device="cuda")
    buf[3:3 + nb] = torch.from_numpy(blob[:nb].copy()).cuda()
    view = buf[3:]
    assert buf.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 3
    d_offs = torch.from_numpy(offs[:m + 1].view(np.int64).copy()).cuda()
    got = idx.lookup_device(view, d_offs, m).cpu().numpy().view(np.uint64)
    assert np.array_equal(got, np.arange(m, dtype=np.uint64))


def test_empty_and_single(s3, oracle_lib, tmp_path, big):
    t = Tree(s3, oracle_lib, tmp_path / "empty", [])
    assert (tmp_path / "empty" / "mph.bin").read_bytes() == b"" and t.arr["depth_offsets"].tolist() == [0, 0]
    assert t.idx.count == 0 and t.idx.max_depth == 0
    assert t.idx.lookup([b"", b"a/"]).tolist() == [NOT_FOUND, NOT_FOUND]
    assert t.idx.stats_for_prefix([b"a/"])[0].tolist() == [False]
    assert t.idx.nodes([0])["found"].tolist() == [0]
    assert t.idx.descendants_at_depth([0, 0, 1, NOT_FOUND], [0, 1, 0, -1]) == [None] * 4
    for max_rel in (-1, 0, 1, 5):
        assert t.idx.descendants_up_to_depth([0, 1], max_rel) == [None, None]
    t.idx.close()
    # nq = 0 on a non-empty index
    none = np.zeros(0, np.uint64)
    assert big.idx.descendants_at_depth(none, 1) == [] and big.idx.descendants_up_to_depth(none, 3) == []
    assert len(big.idx.nodes(none)) == 0 and len(big.idx.lookup([])) == 0
    levels, row_ptr, out = big.idx.descendants_csr(none, 1)
    assert len(levels) == 0 and row_ptr.cpu().tolist() == [0] and len(out) == 0
    # one key
    t = Tree(s3, oracle_lib, tmp_path / "single", [b"only/"])
    assert t.idx.count == 1 and t.idx.max_depth == 1
    assert t.idx.lookup([b"only/", b"only", b""]).tolist() == [0, NOT_FOUND, NOT_FOUND]
    assert t.idx.prefix_string(0) == "only/"
    _exhaustive(t.idx, t.arr, "single")
    t.idx.close()


def test_api_edges(s3, chunky):
    idx = s3.Index(chunky.dir)  # a fresh handle: no plan yet
    with pytest.raises(s3.MPHFError) as e:
        idx.descendants_fill(0)
    assert e.value.status == s3.ERR_STATE
    pos = np.array([chunky.at[b"n255/"], chunky.at[b"z/"], chunky.at[b"n256/"]], np.uint64)
    with pytest.raises(s3.MPHFError) as e:
        idx.descendants_plan(pos, 1, row_ptr_cap=3)  # n_rows = 3 needs 4 entries
    assert e.value.status == s3.ERR_INVALID
    with pytest.raises(s3.MPHFError) as e:  # the refused plan left none behind
        idx.descendants_fill(0)
    assert e.value.status == s3.ERR_STATE
    # 2^31 result rows are refused from the arguments alone (nothing is read or launched)
    import ctypes
    import torch
    d = torch.zeros(4, dtype=torch.int64, device="cuda")
    n_rows, total = ctypes.c_uint64(), ctypes.c_uint64()
    for nq, mode, max_rel in ((2**31, s3.DESC_AT, 0), (2**30, s3.DESC_UPTO, 2)):
        rc = s3.LIB.s3imph_index_descendants_plan(idx._h, d.data_ptr(), d.data_ptr(), nq, mode, max_rel, 0, 0,
                                                  d.data_ptr(), d.data_ptr(), 2**33, ctypes.byref(n_rows),
                                                  ctypes.byref(total), None)
        assert rc == s3.ERR_INVALID, (nq, mode)
    levels, row_ptr, n_rows, total = idx.descendants_plan(pos, 1)
    assert (n_rows, total) == (3, 511) and row_ptr.cpu().tolist() == [0, 255, 255, 511]
    with pytest.raises(s3.MPHFError) as e:
        idx.descendants_fill(total, cap=total - 1)
    assert e.value.status == s3.ERR_INVALID
    first = idx.descendants_fill(total).cpu().numpy().view(np.uint64)
    assert np.array_equal(first, np.concatenate([_at(chunky.arr, int(p), 1) for p in pos]))
    # a second plan replaces the first
    idx.descendants_plan(pos, 1)
    levels, row_ptr, n_rows, total = idx.descendants_plan(pos[::-1].copy(), [1, 0, 1])
    assert (n_rows, total) == (3, 256 + 1 + 255)
    second = idx.descendants_fill(total).cpu().numpy().view(np.uint64)
    assert np.array_equal(second, np.concatenate([_at(chunky.arr, int(p), r) for p, r in zip(pos[::-1], (1, 0, 1))]))
    idx.close()


# ---- the row scan past 1024 scan blocks ------------------------------------------------------
SCAN_BLOCK = 2048                    # rows per scan block (k_rows_reduce / k_rows_down)
SCAN_PASS = 1024 * SCAN_BLOCK        # rows one pass of k_rows_top covers: 2^21
TINY_KEYS = [b"a/", b"a/x/", b"a/x/1/", b"a/y/", b"a/z/", b"b/", b"b/p/", b"b/q/", b"c/", b"c/r/", b"d/", b"e/"]


@pytest.fixture(scope="module")
def tiny(s3, oracle_lib, tmp_path_factory):
    """Twelve nodes without a root, rows of 0 to 3 positions, depths 1 to 3; stats that a filter
    of min_count = 1 splits (every third node has none)."""
    n = len(TINY_KEYS)
    stats = (np.arange(n, dtype=np.uint64) % np.uint64(3), np.full(n, 7, np.uint64))
    t = Tree(s3, oracle_lib, tmp_path_factory.mktemp("tiny"), TINY_KEYS, stats)
    assert t.arr["max_depth"] == 3
    yield t
    t.idx.close()


def _expand(per_node, qi, rows_per_query):
    """row_ptr and the flat positions of a batch whose query q has the rows per_node[qi[q]] (a list
    of rows_per_query arrays each): np.cumsum over the row lengths, np.repeat over the rows."""
    lens = np.array([[len(r) for r in rows] for rows in per_node], np.int64)           # (nodes, R)
    flat = np.concatenate([np.asarray(r, np.uint64) for rows in per_node for r in rows] + [np.zeros(0, np.uint64)])
    start = np.concatenate([[0], np.cumsum(lens.reshape(-1))])[:-1].reshape(lens.shape)  # of each row in flat
    row_len, row_start = lens[qi].reshape(-1), start[qi].reshape(-1)
    assert row_len.shape == (len(qi) * rows_per_query,)
    row_ptr = np.concatenate([[0], np.cumsum(row_len)])
    src = np.repeat(row_start - row_ptr[:-1], row_len) + np.arange(row_ptr[-1])
    return row_ptr, flat[src]


def _cycle(n, nq):
    """nq queries cycling over positions 0 .. n (n itself out of range: empty rows at the block
    edges, 2048 and n + 1 being coprime), the last 3000 all out of range."""
    qi = np.arange(nq) % (n + 1)
    qi[-3000:] = n
    return qi


@pytest.mark.parametrize("min_count", [0, 1], ids=["plain", "filtered"])
def test_at_batch_past_one_pass_of_the_block_sum_scan(tiny, min_count):
    """2^21 + 2049 + 5 DESC_AT rows: k_rows_top carries its running sum into a second pass of 1024
    block sums; with the filter k_desc_filter<kRows> writes as many row_ptr entries, thousands
    of them for rows that start at `total`."""
    arr, n = tiny.arr, tiny.n
    per = [_at(arr, p, 1) for p in range(n + 1)]
    for p in range(n + 1):
        assert _same_row(per[p], _q_at(arr, p, 1)), p
    assert sorted({len(r) for r in per if r is not None}) == [0, 1, 2, 3] and per[n] is None
    kept = [_filtered(r, tiny.stats, min_count, 0) for r in per]
    assert min_count == 0 or 0 < sum(len(r) for r in kept if r is not None) < sum(len(r) for r in per if r is not None)
    nq = SCAN_PASS + SCAN_BLOCK + 1 + 5
    qi = _cycle(n, nq)
    row_ptr, out = _expand([[r if r is not None else []] for r in kept], qi, 1)
    levels, got_rp, got = tiny.idx.descendants_csr(qi.astype(np.uint64), 1, 0, min_count, 0)
    assert np.array_equal(levels.cpu().numpy(), np.array([r is not None for r in per], np.int32)[qi])
    assert np.array_equal(got_rp.cpu().numpy(), row_ptr)
    assert row_ptr[-1] == row_ptr[-3000] and np.array_equal(got.cpu().numpy().view(np.uint64), out)


def test_upto_batch_past_one_pass_of_the_block_sum_scan(tiny):
    """DESC_UPTO with three rows per query crosses the same bound with a third of the queries."""
    arr, n, R = tiny.arr, tiny.n, 3
    per = [_upto(arr, p, R) for p in range(n + 1)]
    for p in range(n + 1):
        _check_upto([per[p]], [_q_upto(arr, p, R)], "tiny UPTO %d" % p)
    nq = SCAN_PASS // R + 700
    assert nq * R > SCAN_PASS + SCAN_BLOCK
    qi = _cycle(n, nq)
    rows = [list(r or []) + [[]] * (R - len(r or [])) for r in per]
    row_ptr, out = _expand(rows, qi, R)
    levels, got_rp, got = tiny.idx.descendants_csr(qi.astype(np.uint64), None, R)
    assert np.array_equal(levels.cpu().numpy(), np.array([len(r or []) for r in per], np.int32)[qi])
    assert max(len(r or []) for r in per) == 2 and np.array_equal(got_rp.cpu().numpy(), row_ptr)
    assert np.array_equal(got.cpu().numpy().view(np.uint64), out)


def test_attach_and_end_to_end(s3, big, tmp_path):
    """Index.from_arrays over the device build's and the device finalize's tensors, then the
    whole pipeline through files: builder, finalize, stats, manifest, Open."""
    import torch
    blob, offs = O.keys_to_blob(big.keys)
    n = big.n
    pad = np.zeros((len(blob) + 7) // 8 * 8 + 8, np.uint8)
    pad[:len(blob)] = blob
    d_blob = torch.from_numpy(pad).cuda()
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).cuda()
    d_fp = torch.empty(n, dtype=torch.int64, device="cuda")
    d_po = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx = s3.DeviceBuilder(0)
    ctx.build(d_blob, d_offs, n, d_fp, d_po)
    f = ctx.finalize_index(d_blob, d_offs, n)
    torch.cuda.synchronize()
    d_oc = torch.from_numpy(big.stats[0].view(np.int64).copy()).cuda()
    d_tb = torch.from_numpy(big.stats[1].view(np.int64).copy()).cuda()
    idx = s3.Index.from_arrays(ctx.mph_bin(), d_fp, d_po, f["depth"], f["subtree_end"], f["max_depth_in_subtree"],
                               f["depth_offsets"], f["depth_positions"], f["max_depth"], d_oc, d_tb)
    assert idx.count == n and idx.max_depth == big.arr["max_depth"]
    _check_at(idx.descendants_at_depth(big.qpos, big.qrel), big.want, "attached")
    want = [_filtered(w, big.stats, 2**62, 2**62) for w in big.want]
    _check_at(idx.descendants_at_depth(big.qpos, big.qrel, 2**62, 2**62), want, "attached, filtered")
    assert np.array_equal(idx.lookup(big.keys[:1000]), np.arange(1000, dtype=np.uint64))
    idx.close()
    ctx.close()

    b = s3.StreamingMPHFBuilder(str(tmp_path))
    b.add_batch(blob, offs)
    b.build(str(tmp_path))
    b.close()
    s3.finalize_index_host(blob, offs, str(tmp_path))
    write_stats(str(tmp_path), *big.stats)
    s3.write_manifest(str(tmp_path), n, big.arr["max_depth"])
    s3.verify_manifest(str(tmp_path))
    with s3.Index(str(tmp_path)) as idx:
        assert idx.count == n and idx.max_depth == big.arr["max_depth"]
        _check_at(idx.descendants_at_depth(big.qpos, big.qrel), big.want, "end to end")
        _check_at(idx.descendants_at_depth(big.qpos, big.qrel, 2**62, 2**62), want, "end to end, filtered")
        assert idx.prefix_string(1) == big.keys[1].decode()
        found, oc, tb = idx.stats_for_prefix(big.keys[:100])
        assert found.all() and np.array_equal(oc, big.stats[0][:100])
