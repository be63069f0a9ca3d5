"""Per-tier statistics on the GPU (include/s3imph.h section 5e) against tests/tiers_ref.py: the
aggregation's 24 columns, the files of the index directory and the reader's batched breakdown."""
import json
import os

import numpy as np
import pytest

import aggregate_ref as R
import oracle as O
import s3imph
import tiers_ref as T
from conftest import GOLDEN
from test_gpu_aggregate import listing_to_dev, same

pytestmark = pytest.mark.gpu

CASES = json.load(open(os.path.join(GOLDEN, "tiers", "cases.json")))
U64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def ctx():
    c = s3imph.DeviceBuilder(0)
    yield c
    c.close()


def tiers_to_dev(tiers):
    import torch
    return torch.from_numpy(np.ascontiguousarray(tiers, np.uint8).copy()).to("cuda")


def device_tier_rows(ctx, blob, offs, sizes, tiers, max_depth=0, align=0):
    """plan (with tiers) + fill + fill_tiers: the plan's info, the five arrays, the (12, n) columns."""
    d_keys, d_offs, d_sizes = listing_to_dev(blob, offs, sizes, align)
    d_tiers = tiers_to_dev(tiers)
    info = ctx.aggregate_plan(d_keys, d_offs, len(offs) - 1, d_sizes, max_depth, tiers=d_tiers)
    out = ctx.aggregate_fill()
    tout = ctx.aggregate_fill_tiers()
    n, nb = info["n_prefixes"], info["blob_bytes"]
    rows = (out["blob"].cpu().numpy()[:nb], out["offsets"].cpu().numpy().view(np.uint64),
            out["depth"].cpu().numpy().view(np.uint32), out["object_count"].cpu().numpy().view(np.uint64),
            out["total_bytes"].cpu().numpy().view(np.uint64))
    tc = tout["tier_count"].cpu().numpy().view(np.uint64)[:, :n]
    tb = tout["tier_bytes"].cpu().numpy().view(np.uint64)[:, :n]
    assert tout["n"] == n and tout["present_mask"] == info["present_mask"]
    return info, rows, tc, tb


def same_columns(tc, tb, wtc, wtb, what=""):
    for name, g, w in (("tier_count", tc, wtc), ("tier_bytes", tb, wtb)):
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            t, r = (int(v[0]) for v in np.nonzero(g != w))
            raise AssertionError(f"{what}: {name}[tier {t}][row {r}] = {g[t, r]}, want {w[t, r]}")


def check(ctx, keys, sizes, tiers, max_depth=0, align=0, what=""):
    """Device against the dict restatement; returns (rows, tc, tb) of the restatement."""
    keys = [bytes(k) for k in keys]
    assert keys == sorted(keys)
    sizes = None if sizes is None else np.asarray(sizes, np.uint64)
    zs = np.zeros(len(keys), np.uint64) if sizes is None else sizes
    rows = T.aggregate_dict_tiers(keys, zs, tiers, max_depth)
    wtc, wtb = T.tier_arrays(rows)
    blob, offs = O.keys_to_blob(keys)
    info, got, tc, tb = device_tier_rows(ctx, blob, offs, sizes, tiers, max_depth, align)
    same(got, R.rows_to_arrays([r[:4] for r in rows]), what)
    same_columns(tc, tb, wtc, wtb, what)
    assert info["present_mask"] == T.present_mask(tiers), what
    assert info["first_bad_tier"] == U64
    return rows, wtc, wtb


# ---- the aggregation -------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES["index_cases"], ids=[c["name"] for c in CASES["index_cases"]])
def test_reference_fixtures(ctx, case):
    keys = [k.encode() for k, _, _ in case["objects"]]
    sizes = [z for _, z, _ in case["objects"]]
    tiers = [t for _, _, t in case["objects"]]
    rows, tc, tb = check(ctx, keys, sizes, tiers, what=case["name"])
    pos = {r[0].decode(): i for i, r in enumerate(rows)}
    for e in case["expect"]:
        assert (int(tc[e["tier"], pos[e["prefix"]]]), int(tb[e["tier"], pos[e["prefix"]]])) == (e["count"], e["bytes"])
    blob, offs = O.keys_to_blob(keys)
    got = s3imph.aggregate(blob, offs, np.asarray(sizes, np.uint64), tiers=tiers)  # the host form
    same(got[:5], R.rows_to_arrays([r[:4] for r in rows]), case["name"] + " (host)")
    same_columns(got[5], got[6], tc, tb, case["name"] + " (host)")
    assert got[7] == T.present_mask(tiers) == sum(1 << t for t in case["present"])


DIR_SIZES = (63, 64, 65, 256, 1024)


def edge_listing(m):
    """m keys in directories of exactly 63 / 64 / 65 / 256 / 1024 keys (the last one cut at m), so
    the rows' key ranges start and end on, one before and one after the tile and block edges."""
    keys, d = [], 0
    while len(keys) < m:
        k = min(DIR_SIZES[d % len(DIR_SIZES)], m - len(keys))
        keys += [b"d%03d/f%04d" % (d, j) for j in range(k)]
        d += 1
    return keys


@pytest.mark.parametrize("m", [1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_tile_and_block_edges(ctx, m):
    keys = edge_listing(m)
    sizes = (np.arange(m, dtype=np.uint64) * 7919 + 1) % 100003
    check(ctx, keys, sizes, np.arange(m) % 12, what=f"m={m} j%12")
    rng = np.random.default_rng(1000 + m)
    check(ctx, keys, sizes, rng.integers(0, 12, m), align=3, what=f"m={m} random")


def test_directory_over_tiles_inside_a_parent_over_blocks(ctx):
    """p/ holds 3000 keys (three 1024-key blocks); p/q/ inside it holds 200 (four tiles) and starts
    at key 1037, neither end on a tile edge; p/q/r/ is a tile-sized run inside that."""
    keys = [b"a/%03d" % j for j in range(37)]
    keys += [b"p/%04d" % j for j in range(1000)]
    keys += [b"p/q/%03d" % j for j in range(70)] + [b"p/q/r/%02d" % j for j in range(64)]
    keys += [b"p/q/s%02d" % j for j in range(66)]
    keys += [b"p/z%04d" % j for j in range(1800)] + [b"z/%d" % j for j in range(5)]
    assert keys == sorted(keys) and sum(k.startswith(b"p/") for k in keys) == 3000
    assert sum(k.startswith(b"p/q/") for k in keys) == 200
    rng = np.random.default_rng(5)
    sizes = rng.integers(0, 1 << 40, len(keys), dtype=np.uint64)
    rows, tc, _ = check(ctx, keys, sizes, rng.integers(0, 12, len(keys)), what="nested")
    pos = {r[0]: i for i, r in enumerate(rows)}
    assert int(tc[:, pos[b"p/"]].sum()) == 3000 and int(tc[:, pos[b"p/q/r/"]].sum()) == 64


def test_per_tier_wrap(ctx):
    keys = [b"a/b/%02d" % i for i in range(40)] + [b"c/%02d" % i for i in range(9)]
    sizes = np.array([1 << 63, U64] * 24 + [1 << 63], np.uint64)
    tiers = np.array([3, 3, 3, 9] * 12 + [3], np.uint8)
    rows, _, tb = check(ctx, keys, sizes, tiers, what="wrap")
    want3 = sum(int(z) for z, t in zip(sizes, tiers) if t == 3) & U64
    assert int(tb[3, 0]) == want3 and want3 != sum(int(z) for z, t in zip(sizes, tiers) if t == 3)


@pytest.mark.parametrize("tier", [0, 11])
def test_all_objects_in_one_tier(ctx, tier):
    keys = edge_listing(300)
    rows, tc, _ = check(ctx, keys, np.arange(300, dtype=np.uint64), np.full(300, tier), what=f"all {tier}")
    assert np.array_equal(tc[tier], np.array([r[2] for r in rows], np.uint64))


def test_tier_present_only_through_size_zero_objects(ctx):
    keys = [b"a/1", b"a/2", b"b/1", b"b/2"]
    rows, tc, tb = check(ctx, keys, [5, 0, 0, 7], [0, 6, 6, 0], what="size 0")
    assert int(tc[6, 0]) == 2 and not tb[6].any()


def test_no_sizes_means_zero_bytes(ctx):
    keys = edge_listing(200)
    tiers = np.arange(200) % 5
    _, tc, tb = check(ctx, keys, None, tiers, what="no sizes")
    assert not tb.any() and int(tc[:, 0].sum()) == 200
    blob, offs = O.keys_to_blob(keys)
    got = s3imph.aggregate(blob, offs, None, tiers=tiers)
    same_columns(got[5], got[6], tc, tb, "no sizes (host)")


@pytest.mark.parametrize("max_depth", [1, 2])
def test_max_depth_cut(ctx, max_depth):
    rng = np.random.default_rng(13)
    alpha = np.frombuffer(b"ab/", np.uint8)
    keys = sorted(bytes(alpha[rng.integers(0, 3, rng.integers(0, 14))]) for _ in range(400))
    rows, _, _ = check(ctx, keys, rng.integers(0, 1 << 30, 400, dtype=np.uint64), rng.integers(0, 12, 400), max_depth,
                       what=f"max_depth {max_depth}")
    assert max(r[1] for r in rows) == max_depth


def test_keys_without_a_slash(ctx):
    rows, tc, _ = check(ctx, [b"a", b"b", b"c"], [1, 2, 3], [2, 2, 8], what="no slash")
    assert len(rows) == 1 and list(tc[:, 0]) == [0, 0, 2, 0, 0, 0, 0, 0, 1, 0, 0, 0]


def test_no_objects(ctx):
    info, rows, tc, tb = device_tier_rows(ctx, np.zeros(0, np.uint8), np.zeros(1, np.uint64), None,
                                          np.zeros(0, np.uint8))
    assert info["n_prefixes"] == 0 and info["present_mask"] == 0 and tc.shape == (12, 0) and tb.shape == (12, 0)
    got = s3imph.aggregate(np.zeros(0, np.uint8), np.zeros(1, np.uint64), None, tiers=np.zeros(0, np.uint8))
    assert got[5].shape == (12, 0) and got[7] == 0


BAD_IDS = {"12_at_index_0": ({0: 12}, 0), "255_in_the_middle": ({700: 255}, 700),
           "two_bad_ids": ({1100: 40, 333: 12}, 333)}


@pytest.mark.parametrize("name", BAD_IDS, ids=list(BAD_IDS))
def test_bad_tier_ids_are_refused(ctx, name):
    import torch
    put, first = BAD_IDS[name]
    keys = edge_listing(1500)
    tiers = np.arange(1500) % 12
    for i, t in put.items():
        tiers[i] = t
    blob, offs = O.keys_to_blob(keys)
    d_keys, d_offs, d_sizes = listing_to_dev(blob, offs, np.ones(1500, np.uint64))
    with pytest.raises(s3imph.MPHFError) as e:
        ctx.aggregate_plan(d_keys, d_offs, 1500, d_sizes, tiers=tiers_to_dev(tiers))
    assert e.value.status == s3imph.ERR_INVALID and e.value.info["first_bad_tier"] == first
    assert f"object {first} " in str(e.value) and str(e.value).startswith("aggregate: ")
    # nothing is written: the refused plan left nothing to fill
    with pytest.raises(s3imph.MPHFError) as e:
        ctx.aggregate_fill(n_cap=2000, blob_cap=1 << 16)
    assert e.value.status == s3imph.ERR_STATE
    tc = torch.full((12, 2000), -1, dtype=torch.int64, device="cuda")
    tb = torch.full((12, 2000), -1, dtype=torch.int64, device="cuda")
    rc = s3imph.LIB.s3imph_aggregate_fill_tiers_device(ctx._h, tc.data_ptr(), tb.data_ptr(), 2000, None)
    assert rc == s3imph.ERR_STATE and bool((tc == -1).all()) and bool((tb == -1).all())
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.aggregate(blob, offs, None, tiers=tiers)
    assert e.value.status == s3imph.ERR_INVALID and f"object {first} " in str(e.value)


def test_state_errors(ctx):
    keys = edge_listing(500)
    sizes = np.arange(500, dtype=np.uint64)
    tiers = np.arange(500) % 12
    blob, offs = O.keys_to_blob(keys)
    d_keys, d_offs, d_sizes = listing_to_dev(blob, offs, sizes)
    d_tiers = tiers_to_dev(tiers)
    ctx.aggregate_plan(d_keys, d_offs, 500, d_sizes)  # a plain plan
    ctx.aggregate_fill()
    with pytest.raises(s3imph.MPHFError) as e:
        ctx.aggregate_fill_tiers()
    assert e.value.status == s3imph.ERR_STATE
    info = ctx.aggregate_plan(d_keys, d_offs, 500, d_sizes, tiers=d_tiers)
    with pytest.raises(s3imph.MPHFError) as e:  # before the fill of the rows
        ctx.aggregate_fill_tiers()
    assert e.value.status == s3imph.ERR_STATE
    ctx.aggregate_fill()
    with pytest.raises(s3imph.MPHFError) as e:
        ctx.aggregate_fill_tiers(n_cap=info["n_prefixes"] - 1)
    assert e.value.status == s3imph.ERR_INVALID
    wide = ctx.aggregate_fill_tiers(n_cap=info["n_prefixes"] + 5)  # the plan survives; a wider stride
    rows = T.aggregate_dict_tiers(keys, sizes, tiers)
    wtc, wtb = T.tier_arrays(rows)
    n = info["n_prefixes"]
    same_columns(wide["tier_count"].cpu().numpy().view(np.uint64)[:, :n],
                 wide["tier_bytes"].cpu().numpy().view(np.uint64)[:, :n], wtc, wtb, "wide stride")


def test_plain_plan_after_a_tiers_plan_equals_a_fresh_context(ctx):
    rng = np.random.default_rng(21)
    keys = edge_listing(2049)
    sizes = rng.integers(0, 1 << 50, 2049, dtype=np.uint64)
    blob, offs = O.keys_to_blob(keys)
    device_tier_rows(ctx, blob, offs, sizes, rng.integers(0, 12, 2049))

    def plain(c):
        d_keys, d_offs, d_sizes = listing_to_dev(blob, offs, sizes)
        info = c.aggregate_plan(d_keys, d_offs, 2049, d_sizes)
        out = c.aggregate_fill()
        return info, [out[k].cpu().numpy() for k in ("blob", "offsets", "depth", "object_count", "total_bytes")]

    info_a, a = plain(ctx)
    fresh = s3imph.DeviceBuilder(0)
    try:
        info_b, b = plain(fresh)
    finally:
        fresh.close()
    assert info_a == info_b and "present_mask" not in info_a
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def big_listing(m=200_000, seed=31):
    """About 4 objects per directory, depth up to 6, byte-sorted."""
    rng = np.random.default_rng(seed)
    ndirs = m // 4
    depth = rng.integers(1, 7, ndirs)
    comp = rng.integers(0, 12, (ndirs, 6))
    dirs = sorted({b"".join(b"d%02d/" % comp[i, k] for k in range(depth[i])) + b"x%05d/" % i for i in range(ndirs)})
    pick = np.sort(rng.integers(0, len(dirs), m))
    keys = [dirs[d] + b"o%06d" % j for j, d in enumerate(pick)]
    assert keys == sorted(keys)
    return keys, rng.integers(0, 1 << 62, m, dtype=np.uint64), rng.integers(0, 12, m).astype(np.uint8)


def test_invariant_at_200k_objects(ctx):
    keys, sizes, tiers = big_listing()
    sizes[::1000] = U64
    blob, offs = O.keys_to_blob(keys)
    wrows, wtc, wtb = T.tier_columns_numpy(blob, offs, sizes, tiers)
    info, rows, tc, tb = device_tier_rows(ctx, blob, offs, sizes, tiers, align=3)
    same(rows, wrows, "200k rows")
    assert int(rows[2].max()) >= 6
    with np.errstate(over="ignore"):
        assert np.array_equal(tc.sum(axis=0, dtype=np.uint64), rows[3])
        assert np.array_equal(tb.sum(axis=0, dtype=np.uint64), rows[4])
    same_columns(tc, tb, wtc, wtb, "200k")
    assert info["present_mask"] == 0xfff


# ---- the index directory and the reader -------------------------------------------------------
INDEX_KEYS = [b"glacier/file1.txt", b"glacier/file2.txt", b"mixed/deep.txt", b"mixed/glacier.txt", b"mixed/sub/a",
              b"mixed/sub/b", b"standard/file1.txt", b"standard/file2.txt", b"zero/empty"]
INDEX_SIZES = np.array([500, 500, 200, 400, U64, 2, 100, 200, 0], np.uint64)
INDEX_TIERS = np.array([4, 4, 5, 4, 0, 0, 0, 0, 9], np.uint8)


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    d = tmp_path_factory.mktemp("tier_index")
    blob, offs = O.keys_to_blob(INDEX_KEYS)
    s3imph.build_index_from_objects(blob, offs, INDEX_SIZES, str(d), tiers=INDEX_TIERS)
    rows = T.aggregate_dict_tiers(INDEX_KEYS, INDEX_SIZES, INDEX_TIERS)
    return d, rows, T.tier_arrays(rows)


def test_index_directory_files(built):
    d, rows, (tc, tb) = built
    n = len(rows)
    ids = [0, 4, 5, 9]
    assert (d / "tiers.json").read_bytes() == T.tiers_json(ids)
    want = {}
    for t in ids:
        want[T.TIER_TABLE[t][1] + "_count.u64"] = O.s3id_u64_array(tc[t])
        want[T.TIER_TABLE[t][1] + "_bytes.u64"] = O.s3id_u64_array(tb[t])
    assert sorted(os.listdir(d / "tier_stats")) == sorted(want)
    for name, data in want.items():
        assert (d / "tier_stats" / name).read_bytes() == data, name
        assert len(s3imph.read_u64_array(str(d / "tier_stats" / name))) == n
    s3imph.verify_manifest(str(d))
    assert "tiers.json" not in s3imph.read_manifest(str(d))["files"]
    assert np.array_equal(s3imph.read_u64_array(str(d / "object_count.u64")), np.array([r[2] for r in rows], np.uint64))


def breakdowns(ids, tc, tb, positions):
    return ([T.get_breakdown_all(ids, tc, tb, int(p)) for p in positions],
            [T.get_breakdown(ids, tc, tb, int(p)) for p in positions])


def test_open_and_batched_breakdown(built):
    d, rows, (tc, tb) = built
    n = len(rows)
    with s3imph.Index(str(d)) as idx:
        assert idx.has_tier_data() and idx.present_tiers() == [0, 4, 5, 9] and idx.count == n
        positions = np.array(list(range(n)) + [n, n + 5, U64] + list(range(n - 1, -1, -1)), np.uint64)
        want_all, want = breakdowns([0, 4, 5, 9], tc, tb, [p if p < n else n for p in positions])
        assert idx.tier_breakdown_all(positions) == want_all
        assert idx.tier_breakdown(positions) == want
        assert want[n] == want[n + 1] == want[n + 2] == []
        assert idx.tier_breakdown_all(np.zeros(0, np.uint64)) == []
        keys = [r[0] for r in rows] + [b"nope/", b"mixed/su", b"mixed/sub/a"]
        got = idx.tier_breakdown_for_prefix(keys)
        assert got[:n] == want[:n] and got[n:] == [[], [], []]
        by_name = {name: (b, c) for _, name, b, c in got[[r[0] for r in rows].index(b"mixed/")]}
        assert by_name == {"STANDARD": ((U64 + 2) & U64, 2), "GLACIER": (400, 1), "DEEP_ARCHIVE": (200, 1)}
        zero = got[[r[0] for r in rows].index(b"zero/")]
        assert zero == [(9, "INTELLIGENT_TIERING_ARCHIVE_INSTANT", 0, 1)]  # count alone keeps the tier


def test_many_queries_cross_workgroups(built):
    d, rows, (tc, tb) = built
    n = len(rows)
    rng = np.random.default_rng(8)
    positions = rng.integers(0, n + 3, 5000).astype(np.uint64)
    with s3imph.Index(str(d)) as idx:
        out, mask = idx.tiers_device(positions)
        v, mk = out.cpu().numpy().view(np.uint64), mask.cpu().numpy().view(np.uint32)
    ids = [0, 4, 5, 9]
    ok = positions < n
    p = np.where(ok, positions, 0).astype(np.int64)
    for s, t in enumerate(ids):
        assert np.array_equal(v[:, s, 0], np.where(ok, tc[t][p], 0)) and np.array_equal(v[:, s, 1], np.where(ok, tb[t][p], 0))
    assert np.array_equal(mk, sum((((v[:, s, 0] | v[:, s, 1]) != 0).astype(np.uint32) << s) for s in range(4)))


def test_manifest_order_is_kept(built, tmp_path):
    import shutil
    d, rows, (tc, tb) = built
    e = tmp_path / "idx"
    shutil.copytree(d, e)
    order = [5, 0, 4]  # as Go's map iteration may list them; tier 9's files stay unlisted
    (e / "tiers.json").write_bytes(T.tiers_json(order))
    with s3imph.Index(str(e)) as idx:
        assert idx.present_tiers() == order
        positions = np.arange(len(rows) + 1, dtype=np.uint64)
        want_all, want = breakdowns(order, tc, tb, positions)
        assert idx.tier_breakdown_all(positions) == want_all and idx.tier_breakdown(positions) == want
        assert [t for t, _, _, _ in want_all[0]] == order


def test_directory_without_tier_data(tmp_path):
    blob, offs = O.keys_to_blob(INDEX_KEYS)
    s3imph.build_index_from_objects(blob, offs, INDEX_SIZES, str(tmp_path))
    assert not (tmp_path / "tiers.json").exists() and not (tmp_path / "tier_stats").exists()
    with s3imph.Index(str(tmp_path)) as idx:
        assert not idx.has_tier_data() and idx.present_tiers() == []
        assert idx.tier_breakdown_all([0, 1]) == [[], []] and idx.tier_breakdown([0, 1]) == [[], []]
        assert idx.tier_breakdown_for_prefix([b"mixed/"]) == [[]]
        assert idx.nodes([0])["object_count"][0] == len(INDEX_KEYS)


def test_no_objects_write_no_tier_files(tmp_path):
    s3imph.build_index_from_objects(np.zeros(0, np.uint8), np.zeros(1, np.uint64), None, str(tmp_path),
                                    tiers=np.zeros(0, np.uint8))
    assert not (tmp_path / "tiers.json").exists() and not (tmp_path / "tier_stats").exists()
    with s3imph.Index(str(tmp_path)) as idx:
        assert idx.count == 0 and not idx.has_tier_data()


def test_attach_path_equals_the_opened_directory(ctx, built):
    d, rows, _ = built
    blob, offs = O.keys_to_blob(INDEX_KEYS)
    d_keys, d_offs, d_sizes = listing_to_dev(blob, offs, INDEX_SIZES)
    d_tiers = tiers_to_dev(INDEX_TIERS)  # stays valid until aggregate_fill_tiers
    info = ctx.aggregate_plan(d_keys, d_offs, len(INDEX_KEYS), d_sizes, tiers=d_tiers)
    out = ctx.aggregate_fill()
    tout = ctx.aggregate_fill_tiers()
    import torch
    n = info["n_prefixes"]
    fp = torch.empty(n, dtype=torch.int64, device="cuda")
    po = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.build(out["blob"], out["offsets"], n, fp, po)
    fin = ctx.finalize_index(out["blob"], out["offsets"], n, out["depth"])
    att = s3imph.Index.attach(ctx.mph_bin(), fp, po, fin["depth"], fin["subtree_end"], fin["max_depth_in_subtree"],
                              fin["depth_offsets"], fin["depth_positions"], fin["max_depth"],
                              out["object_count"], out["total_bytes"])
    try:
        assert not att.has_tier_data()
        att.attach_tiers(T.mask_ids(info["present_mask"]), tout["tier_count"], tout["tier_bytes"])
        del tout  # the handle copied what it needs
        positions = np.array(list(range(n)) + [n, U64], np.uint64)
        keys = [r[0] for r in rows] + [b"absent/"]
        with s3imph.Index(str(d)) as opened:
            assert att.present_tiers() == opened.present_tiers() == [0, 4, 5, 9]
            assert att.tier_breakdown_all(positions) == opened.tier_breakdown_all(positions)
            assert att.tier_breakdown(positions) == opened.tier_breakdown(positions)
            assert att.tier_breakdown_for_prefix(keys) == opened.tier_breakdown_for_prefix(keys)
        with pytest.raises(s3imph.MPHFError) as e:
            att.attach_tiers([0, 0], out["object_count"], out["total_bytes"])
        assert e.value.status == s3imph.ERR_INVALID
    finally:
        att.close()
