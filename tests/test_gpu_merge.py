"""The row merge on the GPU (include/s3imph.h section 5i) against tests/merge_ref.py: all seven
outputs — blob, offsets, depth, count, bytes, tier counts, tier bytes — compared exactly, through
the device plan / fill and through merge_rows (the host call, with its rounds past 64 runs, up to
three levels of them, and with runs in every memory layout s3imph_row_run allows); the byte emit
on its 2048-byte chunk edges."""
import time

import numpy as np
import pytest

import merge_ref as M
import rowset_cases as RC
import s3imph
import tiers_ref as T

pytestmark = pytest.mark.gpu

NAMES = ("blob", "offsets", "depth", "count", "bytes", "tier_count", "tier_bytes")
NONE = (1 << 64) - 1
S = s3imph.merge_geometry()


@pytest.fixture(scope="module")
def ctx():
    c = s3imph.DeviceBuilder(0)
    yield c
    c.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to("cuda")


def device_merge(ctx, runs, tiers=True, align=0, off0=0, stride_extra=0):
    """The runs concatenated into one row set in HBM, plan + fill: (info, the output arrays).  The
    blob starts `align` bytes into its allocation and the offsets at off0; the tier columns have a
    stride of N + stride_extra."""
    import torch
    flat = [r for run in runs for r in run]
    blob, offs, depth, cnt, nbytes, tc, tb = M.to_arrays(flat)
    n = len(flat)
    starts = np.concatenate([[0], np.cumsum([len(run) for run in runs])]).astype(np.uint64)
    end = off0 + len(blob)
    pad = np.full(align + (end + 7) // 8 * 8 + 8, 0xAA, np.uint8)  # bytes before offsets[0] are not keys
    pad[align + off0:align + end] = blob
    d_blob = torch.from_numpy(pad).to("cuda")[align:]
    d_offs = _dev(offs + np.uint64(off0))
    d_tc = d_tb = None
    stride = 0
    if tiers:
        stride = n + stride_extra
        wide = np.full((2, M.NUM_TIERS, max(stride, 1)), 0x5555, np.uint64)  # the slack is not read
        wide[0, :, :n], wide[1, :, :n] = tc, tb
        d_tc, d_tb = _dev(wide[0]), _dev(wide[1])
    keep = (d_blob, d_offs, _dev(depth), _dev(cnt), _dev(nbytes), d_tc, d_tb)
    info = ctx.merge_rows_plan(*keep[:5], starts, d_tier_count=d_tc, d_tier_bytes=d_tb, tier_stride=stride)
    out = ctx.merge_rows_fill()
    nb = info["blob_bytes"]
    raw = out["blob"].cpu().numpy()
    assert not raw[nb:].any(), "the padding up to 8 bytes must be zeros"
    u64 = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
    got = [raw[:nb], u64(out["offsets"]), out["depth"].cpu().numpy().view(np.uint32), u64(out["object_count"]),
           u64(out["total_bytes"])]
    if tiers:
        got += [u64(out["tier_count"])[:, :info["n_out"]], u64(out["tier_bytes"])[:, :info["n_out"]]]
    return info, got


def same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            i = np.argwhere(g != w)[0]
            raise AssertionError(f"{what}: {name}{list(i)} = {g[tuple(i)]}, want {w[tuple(i)]}")


def check(ctx, runs, tiers=True, host=True, what="", **layout):
    want_rows = M.merge_heap(runs)
    assert want_rows == M.merge_dict(runs)
    want = M.to_arrays(want_rows)
    if not tiers:
        want = want[:5]
    n_in = sum(len(run) for run in runs)
    info, got = device_merge(ctx, runs, tiers, **layout)
    same(got, want, what + " (device)")
    assert info["n_in"] == n_in and info["n_out"] == len(want_rows) and info["n_runs"] == len(runs)
    assert info["blob_bytes"] == len(want[0]) and info["first_unsorted"] == NONE
    assert info["max_depth_seen"] == max([r[1] for r in want_rows], default=0)
    assert info["present_mask"] == (M.present_mask(want_rows) if tiers else 0)
    if host:
        arrays = [M.to_arrays(run) if tiers else M.to_arrays(run)[:5] for run in runs]
        out = s3imph.merge_rows(arrays, with_info=True)
        hinfo = out[-1]
        if tiers and n_in:
            assert out[7] == M.present_mask(want_rows)
        same(out[:7 if tiers and n_in else 5], want, what + " (host)")
        assert hinfo["n_in"] == n_in and hinfo["n_out"] == len(want_rows) and hinfo["first_unsorted"] == NONE
    return want_rows


def rows_of(keys, base=1, depth=None):
    """Rows for sorted keys with distinguishable counts, bytes and two tiers each."""
    out = []
    for i, k in enumerate(keys):
        c, b = base + i, (base + i) * 1000 + 7
        k = k.encode("latin-1") if isinstance(k, str) else k
        out.append(M.row(k, k.count(b"/") if depth is None else depth, c, b, {i % 12: (c, b), (i + 5) % 12: (1, 0)}))
    return out


def numbered(lo, n, step=1, fmt=b"k/%06d/"):
    return [fmt % (lo + i * step) for i in range(n)]


@pytest.mark.parametrize("case", M.golden_cases(), ids=lambda c: c[0])
def test_reference_cases(ctx, case):
    name, tiers, runs, want = case
    assert check(ctx, runs, tiers, what=name) == want


LENGTHS = (0, 1, S - 1, S, S + 1, 2 * S + 1)


@pytest.mark.parametrize("a", LENGTHS)
def test_two_runs_with_lengths_at_the_sample_step(ctx, a):
    for b in LENGTHS:
        # overlapping ranges with shared keys: every third key of B is also in A
        runs = [rows_of(numbered(0, a, 3)), rows_of(numbered(1, b, 2), base=500)]
        check(ctx, runs, host=(b in (0, S + 1)), what=f"{a}+{b}")


@pytest.mark.parametrize("lens", [(0, S, S + 1), (S - 1, 0, 2 * S + 1), (S + 1, 1, 0), (2 * S + 1, S, S - 1),
                                  (1, 1, 1), (0, 0, 0), (0, 0, S)])
def test_three_runs_with_an_empty_run_first_middle_last(ctx, lens):
    runs = [rows_of(numbered(r, n, r + 2), base=100 * r + 1) for r, n in enumerate(lens)]
    check(ctx, runs, what=str(lens))


@pytest.mark.parametrize("n", LENGTHS)
def test_one_run_is_the_identity_except_that_equal_neighbours_fold(ctx, n):
    run = rows_of(numbered(0, n))
    got = check(ctx, [run], what=f"k=1 n={n}")
    assert got == run
    if n >= 2:
        dup = sorted(run + rows_of(numbered(0, n)[::2], base=9000), key=lambda r: r[0])
        assert len(check(ctx, [dup], what=f"k=1 dup n={n}")) == n


def test_placement(ctx):
    lo, hi = rows_of(numbered(0, 3 * S + 5)), rows_of(numbered(10**5, 2 * S + 3), base=77)
    check(ctx, [lo, hi], what="A before B")          # every window is empty
    check(ctx, [hi, lo], what="B before A")
    check(ctx, [rows_of(numbered(0, 2 * S + 1, 2)), rows_of(numbered(1, 2 * S + 1, 2), base=50)], what="interleaved")
    same_keys = numbered(0, S + 3)
    got = check(ctx, [rows_of(same_keys, base=1 + 10 * r) for r in range(5)], what="identical runs")
    assert len(got) == len(same_keys)


def test_ties(ctx):
    k = b"dup/"
    run0 = [M.row(b"a/", 1, 1, 1), M.row(k, 7, 1, 10, {0: (1, 10)}), M.row(k, 8, 2, 20, {1: (2, 20)}),
            M.row(k, 9, 3, 30, {0: (3, 30)}), M.row(b"z/", 1, 1, 1)]
    run1 = [M.row(k, 5, 4, 40, {2: (4, 40)})]
    run2 = [M.row(b"b/", 1, 1, 1), M.row(k, 6, 5, 50, {0: (5, 50)})]
    got = check(ctx, [run0, run1, run2], what="ties")
    (row,) = [r for r in got if r[0] == k]
    assert row[1:4] == (7, 15, 150) and row[4][:3] == [9, 2, 4]   # the lowest run's first row gives the depth
    got = check(ctx, [run1, run2, run0], what="ties, other order")
    assert [r for r in got if r[0] == k][0][1] == 5
    got = check(ctx, [run2, run0], what="ties, two runs")
    assert [r for r in got if r[0] == k][0][1] == 6


def test_byte_order(ctx):
    keys = [b"", b"a", b"a/", b"a/b", b"a/b/", b"a\x00/", b"a0/", b"\xff/"]
    assert sorted(keys) != keys  # Go's string <: 0x00 sorts low, 0xff high, a prefix first
    srt = sorted(keys)
    check(ctx, [rows_of(srt[0::2]), rows_of(srt[1::2], base=40), rows_of(srt[::3], base=80)], what="bytes")
    for n in (7, 8, 9, 15, 16, 17):  # keys that differ only in their last byte, around the 8-byte words
        stem = bytes(range(65, 65 + n - 1))
        ks = [stem + bytes([c]) for c in (0, 1, 0x2F, 0x7F, 0x80, 0xFF)] + [stem]
        ks.sort()
        check(ctx, [rows_of(ks[0::2]), rows_of(ks[1::2], base=9), rows_of(ks[2:5], base=33)], what=f"len {n}")
    long = [b"p" * 200 + b"/%03d/" % i for i in range(300)]
    # spread over 3 runs, a few keys repeated inside a run and across runs
    check(ctx, [rows_of(sorted(long[r::3] + long[r * 7:r * 7 + 9]), base=1000 * r + 1) for r in range(3)],
          what="shared 200-byte prefix")


def test_layout(ctx):
    runs = [rows_of(numbered(0, S + 7, 2)), rows_of(numbered(3, 2 * S, 3), base=200), rows_of([b"", b"a/"], base=3)]
    for align in range(1, 8):
        check(ctx, runs, host=False, align=align, off0=5, what=f"align {align}")
    check(ctx, runs, host=False, stride_extra=3, what="tier_stride = N + 3")
    check(ctx, runs, tiers=False, align=3, off0=5, what="no tier columns")


def test_arithmetic(ctx):
    big = (1 << 64) - 1
    run0 = [M.row(b"w/", 1, big, big - 3, {4: (big, 1 << 63)}), M.row(b"x/", 1, 1, 1, {7: (0, 9)})]
    run1 = [M.row(b"w/", 1, 5, 10, {4: (1, 1 << 63), 2: (0, 0)}), M.row(b"x/", 1, 1, 1, {7: (0, 1)})]
    got = check(ctx, [run0, run1], what="wrap")
    w, x = got
    assert w[2:4] == (4, 6) and (w[4][4], w[5][4]) == (0, 0)  # tier 4 wraps to zero in its only row
    assert (x[4][7], x[5][7]) == (0, 10)
    # a tier with count 0 but bytes is present; tier 2 is zero everywhere, tier 4 sums to zero: absent
    assert M.present_mask(got) == 1 << 7


@pytest.mark.parametrize("k", [16, 17, 64])
def test_fan_in_on_the_device(ctx, k):
    rng = np.random.default_rng(k)
    runs = []
    for r in range(k):
        n = int(rng.integers(0, 3 * S))
        picks = np.sort(rng.choice(6 * S, n, replace=False))
        runs.append(rows_of([b"f/%05d/" % int(p) for p in picks], base=1 + 1000 * r, depth=r + 1))
    check(ctx, runs, host=(k == 64), what=f"K={k}")


@pytest.mark.parametrize("k", [65, 130])
def test_fan_in_through_the_rounds(ctx, k):
    """merge_rows past 64 runs; one key in the first and the last run with different depths."""
    runs = [rows_of([b"r/%04d/" % (3 * r), b"r/%04d/" % (3 * r + 4)], base=10 * r + 1) for r in range(k)]
    runs[0] = [M.row(b"both/", 3, 1, 2, {0: (1, 2)})] + runs[0]
    runs[-1] = [M.row(b"both/", 9, 10, 20, {11: (10, 20)})] + runs[-1]
    want_rows = M.merge_heap(runs)
    assert [r for r in want_rows if r[0] == b"both/"][0][1:4] == (3, 11, 22)
    out = s3imph.merge_rows([M.to_arrays(run) for run in runs], with_info=True)
    same(out[:7], M.to_arrays(want_rows), f"K={k}")
    assert out[7] == M.present_mask(want_rows)
    assert out[8]["n_in"] == sum(len(r) for r in runs) and out[8]["n_out"] == len(want_rows)
    # an unsorted run in the second group: first_unsorted indexes the concatenation of all runs
    runs[k - 1] = runs[k - 1][::-1]
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.merge_rows([M.to_arrays(run) for run in runs])
    assert e.value.status == s3imph.ERR_INVALID and str(e.value).startswith("merge: ")
    assert e.value.info["first_unsorted"] == M.first_unsorted(runs)


def test_refusals(ctx):
    good = rows_of(numbered(0, S + 2))
    bad = rows_of(numbered(0, S + 2))
    bad[S], bad[S + 1] = bad[S + 1], bad[S]
    runs = [good, bad, good]
    with pytest.raises(s3imph.MPHFError) as e:
        device_merge(ctx, runs)
    assert e.value.status == s3imph.ERR_INVALID and str(e.value).startswith("merge: ")
    assert e.value.info["first_unsorted"] == M.first_unsorted(runs) == len(good) + S + 1
    with pytest.raises(s3imph.MPHFError) as e:  # the refused plan left no plan
        ctx.merge_rows_fill()
    assert e.value.status == s3imph.ERR_STATE
    # a descent exactly at a run boundary is no error
    check(ctx, [rows_of([b"m/", b"z/"]), rows_of([b"a/", b"m/"], base=8)], what="descent at a boundary")
    # the shape refusals, with their messages
    import torch
    z = torch.zeros(16, dtype=torch.int64, device="cuda")
    for starts, word in (((1, 2), "run_starts[0]"), ((0, 3, 2, 4), "decreases"), ((0, 1 << 32), "2^32"),
                         ([0] * 66, "S3IMPH_MERGE_MAX_RUNS")):
        with pytest.raises(s3imph.MPHFError) as e:
            ctx.merge_rows_plan(z, z, z, z, z, starts)
        assert e.value.status == s3imph.ERR_INVALID and str(e.value).startswith("merge: ") and word in str(e.value)
    with pytest.raises(s3imph.MPHFError) as e:
        ctx.merge_rows_plan(z, z, z, z, z, (0, 1), d_tier_count=z)
    assert e.value.status == s3imph.ERR_INVALID and "one tier array" in str(e.value)


def test_fill_state_and_capacities():
    c = s3imph.DeviceBuilder(0)
    try:
        with pytest.raises(s3imph.MPHFError) as e:
            c.merge_rows_fill()
        assert e.value.status == s3imph.ERR_STATE and str(e.value).startswith("merge: ")
        runs = [rows_of(numbered(0, 10)), rows_of(numbered(5, 10), base=30)]
        info, _ = device_merge(c, runs)
        assert info["n_out"] == 15
        for kw in ({"n_cap": 14}, {"blob_cap": (info["blob_bytes"] + 7) // 8 * 8 - 8}):
            with pytest.raises(s3imph.MPHFError) as e:
                c.merge_rows_fill(**kw)
            assert e.value.status == s3imph.ERR_INVALID and str(e.value).startswith("merge: ")
        # N == 0 with any K is OK with zero rows
        for starts in ((0,), (0, 0, 0)):
            import torch
            info = c.merge_rows_plan(None, None, None, None, None, starts)
            assert info["n_out"] == 0 and info["n_runs"] == len(starts) - 1
            assert int(c.merge_rows_fill()["offsets"][0]) == 0
    finally:
        c.close()


def _listing(m, seed):
    """About m distinct object keys shaped like test_gpu_index_from_objects.listing, with tiers."""
    rng = np.random.default_rng(seed)
    keys = set()
    while len(keys) < m:
        depth = int(rng.integers(0, 6))
        dirs = [b"d%02d" % int(rng.integers(0, 40))] + [b"s%d" % int(rng.integers(0, 4)) for _ in range(depth)]
        keys.add(b"/".join(dirs[:depth]) + (b"/" if depth else b"") + b"obj-%04d.bin" % int(rng.integers(0, 3000)))
    keys = sorted(keys)
    sizes = rng.integers(0, 1 << 44, len(keys), dtype=np.uint64)
    tiers = rng.integers(0, 9, len(keys), dtype=np.uint8)
    return keys, sizes, tiers


def test_random_runs_of_unequal_size(ctx):
    """7 runs from a partition of a 60k-object listing, from a handful of objects to half of them.
    That listing has 10,377 distinct prefixes, so the runs hold 23,180 rows in all; the test below
    brings the input to 200k rows."""
    keys, sizes, tiers = _listing(60_000, 17)
    rng = np.random.default_rng(18)
    owner = rng.choice(7, len(keys), p=[0.5, 0.25, 0.12, 0.08, 0.04, 0.009, 0.001])
    runs = []
    for p in range(7):
        sel = np.flatnonzero(owner == p)
        runs.append(T.aggregate_dict_tiers([keys[i] for i in sel], sizes[sel], tiers[sel]))
    want = check(ctx, runs, what="random")
    assert want == T.aggregate_dict_tiers(keys, sizes, tiers)
    assert sum(len(r) for r in runs) > len(want) and len({len(r) for r in runs}) == 7


def test_200k_rows_in_7_runs_of_unequal_size(ctx):
    """200k input rows with tiers: 7 sorted draws, from 300 to 80,000 rows, out of 120k keys."""
    rng = np.random.default_rng(29)
    pool = sorted({b"p%02d/q%03d/r%05d/" % (int(a), int(b), int(c))
                   for a, b, c in zip(rng.integers(0, 50, 130_000), rng.integers(0, 400, 130_000),
                                      rng.integers(0, 10**5, 130_000))})[:120_000]
    assert len(pool) == 120_000
    runs = []
    for r, n in enumerate((80_000, 60_000, 35_000, 15_000, 7_000, 2_700, 300)):
        picks = np.sort(rng.choice(len(pool), n, replace=False))
        cnt = rng.integers(0, 1 << 63, n, dtype=np.uint64)
        run = [M.row(pool[p], 3, int(c), int(c) * 3 & M.M64, {r: (int(c), 1), (r + 3) % 12: (0, int(c) >> 7)})
               for p, c in zip(picks, cnt)]
        runs.append(run)
    assert sum(len(r) for r in runs) == 200_000
    want = check(ctx, runs, what="200k")
    assert len(want) < 120_000


# ---- the host merge in the run layouts the header allows (tests/rowset_cases.py) ----------------
def host_merge(runs, tiers, what):
    """merge_rows over RowRuns or tuples: (the 7 or 5 arrays, the mask or None, info)."""
    out = s3imph.merge_rows(runs, with_info=True)
    assert len(out) == (9 if tiers else 6), what
    return list(out[:7 if tiers else 5]), (out[7] if tiers else None), out[-1]


@pytest.mark.parametrize("tiers", [True, False], ids=["tiers", "no tiers"])
@pytest.mark.parametrize("k", [5, 65])
def test_merge_rows_in_every_layout(k, tiers):
    """Bases 1, 5, 8, 13 with junk around the keys, tier_stride n + 3 with junk in the slack, a
    root-only run with a NULL blob, empty runs (NULL and not) first, in the middle and last; with
    k = 65 the laid-out runs also pass through the first round's download and come back as the
    second round's runs."""
    parts = RC.part_rows(k)
    runs = parts[:k // 2] + [RC.ROOT_ONLY] + parts[k // 2:]
    logical, laid = RC.layouts(runs, tiers)
    assert len(laid) == k + 7 and (k < 64 or len(laid) > 64)
    want_rows = M.merge_heap(logical)
    assert want_rows == M.merge_heap(runs) and len(want_rows) == len(RC.whole_rows("shapes"))
    want = M.to_arrays(want_rows)[:7 if tiers else 5]
    got, mask, info = host_merge(laid, tiers, "laid out")
    same(got, want, f"k={k} laid out")
    packed, pmask, pinfo = host_merge([M.to_arrays(r)[:7 if tiers else 5] for r in logical], tiers, "packed")
    same(packed, want, f"k={k} packed")
    assert mask == pmask == (M.present_mask(want_rows) if tiers else None)
    assert info == pinfo and info["n_in"] == sum(len(r) for r in runs) and info["n_out"] == len(want_rows)
    assert info["first_unsorted"] == NONE and info["max_depth_seen"] == max(r[1] for r in want_rows)


@pytest.mark.parametrize("base", [1, 5, 8, 13])
def test_one_run_with_a_base_is_the_identity(base):
    """A single run whose offsets start at `base`: the rebasing alone, no second run to hide behind."""
    rows = RC.part_rows(5)[base % 5]
    got, mask, info = host_merge([RC.layout_run(rows, base=base, stride_extra=base % 2)], True, f"base {base}")
    same(got, M.to_arrays(rows), f"base {base}")
    assert mask == M.present_mask(rows) and info["n_in"] == info["n_out"] == len(rows)


def test_only_empty_runs_in_every_layout():
    _, laid = RC.layouts([], True)
    out = s3imph.merge_rows(laid, with_info=True)
    assert len(out) == 6 and out[1].tolist() == [0] and len(out[0]) == 0 and out[-1]["n_out"] == 0


def test_an_unsorted_run_in_a_layout_is_reported_at_its_row():
    parts = RC.part_rows(5)
    bad = parts[2][:10] + [parts[2][11], parts[2][10]] + parts[2][12:]
    runs = parts[:2] + [bad] + parts[3:]
    _, laid = RC.layouts(runs, True)
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.merge_rows(laid)
    assert e.value.status == s3imph.ERR_INVALID and str(e.value).startswith("merge: ")
    assert e.value.info["first_unsorted"] == M.first_unsorted(runs) == len(parts[0]) + len(parts[1]) + 11


# ---- rounds --------------------------------------------------------------------------------------
def test_an_empty_group_of_64_runs():
    """130 runs, runs 64..127 without a row (NULL pointers and real empty arrays alternating): the
    first round's second group yields an empty run for the second round."""
    parts = RC.part_rows(66)
    hole = [RC.layout_run([], null=True) if r % 2 else RC.layout_run([], base=5) for r in range(64)]
    runs = [M.to_arrays(r) for r in parts[:64]] + hole + [M.to_arrays(r) for r in parts[64:]]
    got, mask, info = host_merge(runs, True, "hole")
    want_rows = RC.whole_rows("shapes")
    same(got, M.to_arrays(want_rows), "130 runs, 64 of them empty")
    assert mask == M.present_mask(want_rows)
    assert info["n_in"] == sum(len(r) for r in parts) and info["n_out"] == len(want_rows) and info["n_runs"] == 130


def test_the_smallest_unsorted_row_over_two_groups():
    """130 runs, an unsorted run in group 0 and another in group 1: the smallest index is reported,
    as an index into the concatenation of all runs."""
    runs = [rows_of([b"r/%04d/" % (3 * r), b"r/%04d/" % (3 * r + 4)], base=10 * r + 1) for r in range(130)]
    runs[5], runs[100] = runs[5][::-1], runs[100][::-1]
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.merge_rows([M.to_arrays(run) for run in runs])
    assert e.value.status == s3imph.ERR_INVALID and str(e.value).startswith("merge: ")
    assert e.value.info["first_unsorted"] == M.first_unsorted(runs) == 11
    assert e.value.info["n_in"] == 260
    runs[5] = runs[5][::-1]  # only group 1 is left unsorted
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.merge_rows([M.to_arrays(run) for run in runs])
    assert e.value.info["first_unsorted"] == M.first_unsorted(runs) == 201


def test_4097_runs_take_three_rounds():
    """64 * 64 + 1 runs of one or two rows, no tier columns: 65 groups, then 2, then the last merge.
    One key sits in run 0, run 2048 and run 4096 with three depths; run 0's wins.  The call takes
    about 0.4 s on an MI355X (printed)."""
    k = 64 * 64 + 1
    runs = []
    for r in range(k):
        keys = [b"t/%05d/" % (2 * r)] + ([b"t/%05d/" % (2 * r + 4)] if r % 3 else [])
        runs.append([M.row(key, 2, r + 1, 10 * r + i) for i, key in enumerate(keys)])
    for r, d in ((0, 4), (2048, 7), (4096, 9)):
        runs[r] = [M.row(b"same/", d, 100 + r, r)] + runs[r]
    want_rows = M.merge_heap(runs)
    (row,) = [r for r in want_rows if r[0] == b"same/"]
    assert row[1:4] == (4, 300 + 2048 + 4096, 2048 + 4096)
    assert len(want_rows) < sum(len(r) for r in runs)  # t/%05d/ keys of neighbouring runs coincide
    arrays = [M.to_arrays(run)[:5] for run in runs]
    t0 = time.perf_counter()
    out = s3imph.merge_rows(arrays, with_info=True)
    took = time.perf_counter() - t0
    print(f"4097 runs through merge_rows: {took:.2f} s")
    assert len(out) == 6
    same(out[:5], M.to_arrays(want_rows)[:5], "K=4097")
    info = out[-1]
    assert info["n_in"] == sum(len(r) for r in runs) and info["n_out"] == len(want_rows)
    assert info["first_unsorted"] == NONE and info["max_depth_seen"] == 4 and info["present_mask"] == 0


# ---- the byte emit at its 2048-byte chunk edges --------------------------------------------------
EMIT_CHUNK = 8 * 256  # k_merge_bytes: one 8-byte word per lane, 256 lanes per workgroup


def emit_runs(lengths):
    """Rows with the given key lengths in output order (distinct, byte-sorted by their first byte),
    dealt over three runs so that neighbouring output rows come from different runs.  Two rows are
    duplicated: the longest (it sits in run 1) also into run 0, so the head and its bytes come from
    the copy; and row 3 (of run 0) also into run 1, so they come from the original."""
    assert len(lengths) < 90
    keys = [bytes([0x21 + i]) + bytes([0x61 + (i + j) % 26 for j in range(ln - 1)]) for i, ln in enumerate(lengths)]
    assert keys == sorted(keys) and [len(k) for k in keys] == list(lengths)
    rows = rows_of(keys)
    runs = [rows[0::3], rows[1::3], rows[2::3]]
    big = max(range(len(keys)), key=lambda i: lengths[i])
    assert big % 3 == 1 and big != 3
    for i, r in ((big, 0), (3, 1)):
        runs[r] = sorted(runs[r] + [M.row(keys[i], 50, 7, 7, {3: (7, 7)})], key=lambda x: x[0])
    return runs, keys


EMIT_LAYOUTS = {
    # 1, 2, 3: three rows inside the first word; 1..9 bytes; a row ending at byte 2048; a key of 4200
    # bytes owning chunk [4096, 6144) and the start of the next; a total of 6253 = 5 mod 8
    "edges": [1, 2, 3, 4, 5, 6, 7, 8, 9, 2003, 4200, 3, 2],
    "2048": [1, 2, 3, 9, 2033],
    "2049": [1, 2, 3, 9, 2033, 1],
}


@pytest.mark.parametrize("name", EMIT_LAYOUTS)
def test_merged_bytes_at_the_emit_chunk_edges(ctx, name):
    lengths = EMIT_LAYOUTS[name]
    runs, keys = emit_runs(lengths)
    want_rows = M.merge_heap(runs)
    assert [r[0] for r in want_rows] == keys and sum(len(r) for r in runs) == len(keys) + 2
    offs = M.to_arrays(want_rows)[1].tolist()
    # neighbouring output rows come from different runs, but for the one head moved into run 0
    owner = [min(r for r in range(3) if any(x[0] == key for x in runs[r])) for key in keys]
    assert sum(a == b for a, b in zip(owner, owner[1:])) <= 1 and set(owner) == {0, 1, 2}
    heads = {r[0]: r[1] for r in want_rows}
    assert sorted(d for d in heads.values() if d == 50) == [50]  # one head is the copy, the other the original
    if name == "edges":
        assert offs[:4] == [0, 1, 3, 6] and offs[10] == EMIT_CHUNK and offs[11] == EMIT_CHUNK + 4200
        assert offs[11] > 3 * EMIT_CHUNK and offs[11] % EMIT_CHUNK != 0 and offs[-1] == 6253 and offs[-1] % 8 == 5
        assert [b - a for a, b in zip(offs, offs[1:])][:9] == list(range(1, 10))
    else:
        assert offs[-1] == int(name) and offs[5] == EMIT_CHUNK
    for align in range(1, 8):
        check(ctx, runs, host=False, align=align, off0=5, what=f"{name} align {align}")
    check(ctx, runs, tiers=False, host=True, align=3, off0=5, what=f"{name} no tiers")
