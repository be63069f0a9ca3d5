"""The cost estimate and the ranked descendant rows on the GPU (include/s3imph.h section 5h) against
tests/pricing_ref.py: s3imph_index_cost_device record for record over the fixture's random
breakdowns, its batch edges, its composition with lookup and descendants_fill, and
s3imph_index_descendants_top against the plan's own rows sorted on the host."""
import ctypes
import shutil

import numpy as np
import pytest

import oracle as O
import pricing_cases as C
import pricing_ref as P
import s3imph
import tiers_ref as T
from index_dirs import write_index_dir, write_stats
from test_gpu_tiers import INDEX_KEYS, INDEX_SIZES, INDEX_TIERS

pytestmark = pytest.mark.gpu

U64 = (1 << 64) - 1
N = C.N  # nodes of the test tree = breakdowns of the fixture
K = 10
BIG = 2100  # children of big/ at one depth: crosses the 2048-position chunk


def tree_prefixes():
    """N byte-sorted prefixes: big/ with BIG children (30 of them with a grandchild), parents with
    0, 1, K - 1, K and K + 1 children, fillers below the root."""
    p = [b"", b"big/"] + [b"big/c%04d/" % j for j in range(BIG)] + [b"big/c%04d/g/" % j for j in range(30)]
    p += [b"p00/", b"p01/", b"p09/", b"p10/", b"p11/"]
    for name, kids in ((b"p01/", 1), (b"p09/", K - 1), (b"p10/", K), (b"p11/", K + 1)):
        p += [name + b"k%02d/" % j for j in range(kids)]
    p += [b"z%04d/" % j for j in range(N - len(p))]
    p = sorted(p)
    assert len(p) == N == len(set(p))
    return p


def key_columns():
    """object_count with many ties, values >= 2^63 and values that differ only in their high or only
    in their low 32 bits; total_bytes with two values only."""
    rng = np.random.default_rng(5)
    vals = np.array([0, 5, 5, 1 << 63, (1 << 63) + 1, 1 << 32, (1 << 32) + 1, 7 << 32, (7 << 32) + 1, U64], np.uint64)
    return vals[rng.integers(0, len(vals), N)], np.array([3, 9], np.uint64)[rng.integers(0, 2, N)]


@pytest.fixture(scope="module")
def tree(tmp_path_factory, oracle_lib):
    d = tmp_path_factory.mktemp("pricing_tree")
    prefixes = tree_prefixes()
    write_index_dir(str(d), oracle_lib, prefixes, stats=key_columns())
    return d, prefixes


def with_tiers(tree, tmp_path, ids, zero_rows=None, name="idx"):
    """A copy of the tree's directory carrying the fixture's columns for the tiers `ids`, listed in
    that order in tiers.json; zero_rows: nodes whose columns are all zero."""
    d, _ = tree
    e = tmp_path / name
    shutil.copytree(d, e)
    tc, tb = np.zeros((12, N), np.uint64), np.zeros((12, N), np.uint64)
    for t in ids:
        tc[t], tb[t] = C.COUNT[:, t], C.BYTES[:, t]
    if zero_rows is not None:
        tc[:, zero_rows] = 0
        tb[:, zero_rows] = 0
    s3imph.write_tier_files(str(e), sum(1 << t for t in ids), tc, tb)
    (e / "tiers.json").write_bytes(T.tiers_json(list(ids)))
    return s3imph.Index(str(e))


def lib_table(name):
    t = C.CASES["tables"][name]
    return s3imph.PriceTable(t["per_gb_month"], t["monitoring_per_1000_objects"], t["standard_price_per_gb"])


def same_records(got, want, what):
    assert len(got) == len(want), what
    for f in ("total", "monitoring", "min_object_size", "glacier_overhead", "tier_mask", "found"):
        w = np.array([r[f] for r in want], np.uint64)
        if not np.array_equal(got[f].astype(np.uint64), w):
            i = int(np.nonzero(got[f].astype(np.uint64) != w)[0][0])
            raise AssertionError(f"{what}: {f}[{i}] = {int(got[f][i])}, want {int(w[i])}")
    assert np.array_equal(got["per_tier"], np.array([r["per_tier"] for r in want], np.uint64)), (what, "per_tier")


SLOTS = {1: (6,), 5: (5, 0, 11, 4, 7), 12: (3, 0, 1, 2, 11, 4, 5, 6, 7, 8, 9, 10)}  # manifest orders, not ascending


# ---- s3imph_index_cost_device ---------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 5, 12])
def test_parity_over_every_position(tree, tmp_path, nt):
    ids = SLOTS[nt]
    with with_tiers(tree, tmp_path, ids) as idx:
        assert idx.present_tiers() == list(ids)
        for table in ("default", "no_monitoring", "partial", "high", "clamp") if nt == 12 else ("default",):
            got = idx.cost_records(np.arange(N, dtype=np.uint64), lib_table(table))
            same_records(got, C.ref_records(table, ids), f"T={nt} {table}")
        if nt == 12:
            assert (got["per_tier"][:, 0] == U64).any()  # the clamp was reached on the device too
            assert idx.cost_records(np.arange(N, dtype=np.uint64)).tobytes() == \
                idx.cost_records(np.arange(N, dtype=np.uint64), lib_table("default")).tobytes()


@pytest.mark.parametrize("nt", [5, 12])
def test_batch_edges(tree, tmp_path, nt):
    import torch
    ids = SLOTS[nt]
    qb = 256 // nt  # the kernel's queries per workgroup
    ref = C.ref_records("default", ids)
    pt = lib_table("default")
    rng = np.random.default_rng(nt)
    with with_tiers(tree, tmp_path, ids) as idx:
        for nq in (1, qb - 1, qb, qb + 1, 3 * qb + 7):
            pos = rng.integers(0, N, nq).astype(np.uint64)
            pos[nq // 2] = pos[0]  # a duplicate
            if nq > 3:
                pos[1], pos[nq - 1] = N, U64
            want = [ref[int(p)] if p < N else P.ZERO_COST for p in pos]
            same_records(idx.cost_records(pos, pt), want, f"T={nt} nq={nq}")
            # d_qpos 8 bytes into a 16-byte aligned allocation
            buf = torch.from_numpy(np.concatenate([np.zeros(1, np.uint64), pos]).view(np.int64)).to("cuda")
            assert buf.data_ptr() % 16 == 0
            got = idx.cost_device(buf[1:], pt).cpu().numpy().reshape(-1).view(s3imph.COST_DTYPE)
            same_records(got, want, f"T={nt} nq={nq} misaligned")
        out = torch.full((4, 17), -7, dtype=torch.int64, device="cuda")
        rc = s3imph.LIB.s3imph_index_cost_device(idx._h, None, 0, ctypes.byref(pt._c()), out.data_ptr(), None)
        assert rc == s3imph.OK and bool((out == -7).all())


def test_index_without_tier_data(tree):
    d, _ = tree
    with s3imph.Index(str(d)) as idx:
        assert not idx.has_tier_data()
        got = idx.cost_records(np.array([0, 5, N - 1, N, U64, 5], np.uint64))
        same_records(got, [dict(P.ZERO_COST, found=f) for f in (1, 1, 1, 0, 0, 1)], "no tiers")
        assert idx.monthly_cost([0, N]) == [
            {"found": True, "total": 0, "monitoring": 0, "min_object_size": 0, "glacier_overhead": 0, "per_tier": {}},
            {"found": False, "total": 0, "monitoring": 0, "min_object_size": 0, "glacier_overhead": 0, "per_tier": {}}]


def test_refused_tables(tree, tmp_path):
    with with_tiers(tree, tmp_path, SLOTS[5]) as idx:
        for bad in (s3imph.PriceTable({"STANDARD": -0.01}), s3imph.PriceTable({}, float("nan"), 0.0),
                    s3imph.PriceTable({}, 0.0, float("inf"))):
            with pytest.raises(s3imph.MPHFError) as e:
                idx.cost_device([0, 1], bad)
            assert e.value.status == s3imph.ERR_INVALID and "pricing: " in str(e.value)
            assert idx.last_error().startswith("pricing: ")
            with pytest.raises(s3imph.MPHFError) as e:
                idx.descendants_top([0], rel=1, key="cost", pt=bad)
            assert e.value.status == s3imph.ERR_INVALID and idx.last_error().startswith("pricing: ")


# ---- composition ---------------------------------------------------------------------------------
def test_monthly_cost_for_prefix_on_a_built_listing_index(tmp_path):
    blob, offs = O.keys_to_blob(INDEX_KEYS)
    s3imph.build_index_from_objects(blob, offs, INDEX_SIZES, str(tmp_path), tiers=INDEX_TIERS)
    rows = T.aggregate_dict_tiers(INDEX_KEYS, INDEX_SIZES, INDEX_TIERS)
    keys = [r[0] for r in rows] + [b"nope/", b"mixed/su"]
    for table in ("default", "partial"):
        pt, rt = lib_table(table), C.TABLES[table]
        with s3imph.Index(str(tmp_path)) as idx:
            got = idx.monthly_cost_for_prefix(keys, pt)
            breakdowns = idx.tier_breakdown_for_prefix(keys)
        for q, (g, bd) in enumerate(zip(got, breakdowns)):
            w = P.compute_monthly_cost([(t, c, b) for t, _, b, c in bd], rt, found=int(q < len(rows)))
            assert g == {"found": bool(w["found"]), "total": w["total"], "monitoring": w["monitoring"],
                         "min_object_size": w["min_object_size"], "glacier_overhead": w["glacier_overhead"],
                         "per_tier": {P.TIER_NAMES[t]: w["per_tier"][t] for t in range(12) if (w["tier_mask"] >> t) & 1}}
            assert g == dict(s3imph.compute_monthly_cost(bd, pt), found=g["found"])
        # the listing's sizes are a few hundred bytes: every cost truncates to 0, the keys are there
        assert not got[-1]["found"] and not got[-2]["found"] and "STANDARD" in got[0]["per_tier"]


def test_cost_device_straight_from_descendants_fill(tree, tmp_path):
    d, prefixes = tree
    ids = SLOTS[12]
    ref = C.ref_records("default", ids)
    q = np.array([prefixes.index(b"big/"), 0, prefixes.index(b"p11/")], np.uint64)
    with with_tiers(tree, tmp_path, ids) as idx:
        _, _, out = idx.descendants_csr(q, rel=1)
        assert out.shape[0] > 2048
        got = idx.cost_device(out).cpu().numpy().reshape(-1).view(s3imph.COST_DTYPE)
        same_records(got, [ref[int(p)] for p in out.cpu().numpy().view(np.uint64)], "from fill")


# ---- s3imph_index_descendants_top ----------------------------------------------------------------
def rank_queries(prefixes):
    at = [prefixes.index(p) for p in (b"big/", b"p00/", b"p01/", b"p09/", b"p10/", b"p11/", b"")]
    return np.array(at + [at[0], N], np.uint64)  # one query repeated, one past the end


def check_top(idx, q, key_of, key, k, pt=None, **plan):
    """descendants_top against the plan's own rows (descendants_csr) ordered by tests/pricing_ref.py."""
    _, row_ptr, out = idx.descendants_csr(q, **plan)
    rp, o = row_ptr.cpu().numpy(), out.cpu().numpy().view(np.uint64)
    n_rows = len(rp) - 1
    top_n, top_pos, top_key = idx.descendants_top(q, key=key, k=k, pt=pt, **plan)
    tn = top_n.cpu().numpy()
    tp, tk = top_pos.cpu().numpy().view(np.uint64), top_key.cpu().numpy().view(np.uint64)
    assert tn.shape == (n_rows,) and tp.shape == tk.shape == (n_rows, k)
    for r in range(n_rows):
        row = [int(p) for p in o[rp[r]:rp[r + 1]]]
        want = P.top_of_row(row, key_of, k)
        assert tn[r] == min(k, len(row)), (key, k, r)
        assert [int(p) for p in tp[r, :tn[r]]] == want, (key, k, r)
        assert [int(v) for v in tk[r, :tn[r]]] == [key_of[p] for p in want], (key, k, r)
        assert (tp[r, tn[r]:] == U64).all() and not tk[r, tn[r]:].any(), (key, k, r, "padding")
    # the plan stays: a fill after top still returns the plan's rows
    assert np.array_equal(idx.descendants_fill(len(o)).cpu().numpy().view(np.uint64), o)
    return rp


@pytest.mark.parametrize("key", ["count", "bytes", "cost", "cost_high", "cost_ties"])
def test_ranking(tree, tmp_path, key):
    d, prefixes = tree
    ocnt, tbytes = key_columns()
    q = rank_queries(prefixes)
    ids = SLOTS[12]
    zero_rows = np.arange(N) % 3 != 0 if key == "cost_ties" else None  # two thirds of the costs are 0
    table = "high" if key == "cost_high" else "default"
    if key.startswith("cost"):
        ref = C.ref_records(table, ids)
        key_of = [0 if zero_rows is not None and zero_rows[p] else ref[p]["total"] for p in range(N)]
        assert key != "cost_high" or sum(v >= 1 << 63 for v in key_of) >= 8
    else:
        key_of = [int(v) for v in (ocnt if key == "count" else tbytes)]
    pt = lib_table(table)
    name = "cost" if key.startswith("cost") else key
    with with_tiers(tree, tmp_path, ids, zero_rows) as idx:
        for k in (1, K, BIG + 500):
            rp = check_top(idx, q, key_of, name, k, pt, rel=1)
            assert list(np.diff(rp)) == [BIG, 0, 1, K - 1, K, K + 1, N - BIG - 30 - 31 - 1, BIG, 0]
        check_top(idx, q, key_of, name, K, pt, rel=1, min_count=5)
        check_top(idx, q, key_of, name, K, pt, rel=1, min_bytes=9)
        check_top(idx, q, key_of, name, K, pt, rel=1, min_count=U64, min_bytes=10)  # nothing passes: total 0
        check_top(idx, q, key_of, name, K, pt, rel=None, max_rel=2)
        check_top(idx, q[1:2], key_of, name, 3, pt, rel=1)  # one empty row
        check_top(idx, q[0:1], key_of, name, K, pt, rel=1)  # one row alone (sorted device-wide), over a chunk
        check_top(idx, q[0:1], key_of, name, K, pt, rel=1, min_count=5)


def test_top_state_and_argument_errors(tree, tmp_path):
    import torch
    d, prefixes = tree
    pt = lib_table("default")._c()
    top = s3imph.LIB.s3imph_index_descendants_top
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    args = (buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), None)
    with with_tiers(tree, tmp_path, SLOTS[5]) as idx:
        assert top(idx._h, 2, ctypes.byref(pt), 3, *args) == s3imph.ERR_STATE and "no plan" in idx.last_error()
        _, _, n_rows, _ = idx.descendants_plan([0, 1, 2, 3], rel=1)
        assert n_rows == 4
        assert top(idx._h, 2, ctypes.byref(pt), 0, *args) == s3imph.ERR_INVALID      # k == 0
        assert top(idx._h, 3, ctypes.byref(pt), 3, *args) == s3imph.ERR_INVALID      # an unknown key
        assert top(idx._h, -1, ctypes.byref(pt), 3, *args) == s3imph.ERR_INVALID
        assert top(idx._h, 2, None, 3, *args) == s3imph.ERR_INVALID                  # COST without a table
        assert top(idx._h, 0, None, 1 << 29, *args) == s3imph.ERR_INVALID            # n_rows * k == 2^31
        assert "2^31" in idx.last_error()
        assert top(idx._h, 0, None, 3, *args) == s3imph.OK                           # COUNT needs no table
        # an empty batch is a plan with no rows: OK, nothing written
        idx.descendants_plan(np.zeros(0, np.uint64), rel=1)
        buf.fill_(-3)
        assert top(idx._h, 2, ctypes.byref(pt), 3, *args) == s3imph.OK and bool((buf == -3).all())
    with s3imph.Index(str(d)) as idx:  # stats, no tier data
        idx.descendants_plan([0], rel=1)
        assert top(idx._h, 2, ctypes.byref(pt), 3, *args) == s3imph.ERR_STATE and "tier data" in idx.last_error()
        assert top(idx._h, 1, None, 3, *args) == s3imph.OK
    e = tmp_path / "nostats"
    shutil.copytree(d, e)
    (e / "object_count.u64").unlink()
    (e / "total_bytes.u64").unlink()
    with s3imph.Index(str(e)) as idx:
        idx.descendants_plan([0], rel=1)
        for key in (0, 1):
            assert top(idx._h, key, None, 3, *args) == s3imph.ERR_STATE and "object_count" in idx.last_error()
