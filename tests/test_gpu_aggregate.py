"""Prefix aggregation on the GPU (include/s3imph.h section 5d) against tests/aggregate_ref.py,
row for row and byte for byte."""
import json
import os

import numpy as np
import pytest

import aggregate_ref as R
import oracle as O
import s3imph
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = json.load(open(os.path.join(GOLDEN, "aggregate", "cases.json")))["cases"]
NAMES = ("prefix_blob", "prefix_offsets", "depth", "object_count", "total_bytes")
BIG = np.array([0, 1, 7, 1 << 63, (1 << 64) - 1, 12345], np.uint64)


@pytest.fixture(scope="module")
def ctx():
    c = s3imph.DeviceBuilder(0)
    yield c
    c.close()


def listing_to_dev(blob, offs, sizes, align=0):
    """The listing as torch tensors; the key blob starts `align` bytes into its allocation."""
    import torch
    nbytes = int(offs[-1])
    pad = np.zeros(align + (nbytes + 7) // 8 * 8 + 8, np.uint8)
    pad[align:align + nbytes] = blob[:nbytes]
    d_keys = torch.from_numpy(pad).to("cuda")[align:]
    d_offs = torch.from_numpy(np.ascontiguousarray(offs, np.uint64).view(np.int64).copy()).to("cuda")
    d_sizes = None if sizes is None else \
        torch.from_numpy(np.ascontiguousarray(sizes, np.uint64).view(np.int64).copy()).to("cuda")
    return d_keys, d_offs, d_sizes


def device_rows(ctx, blob, offs, sizes, max_depth=0, align=0):
    """plan + fill over torch tensors: the plan's info and the five arrays on the host."""
    d_keys, d_offs, d_sizes = listing_to_dev(blob, offs, sizes, align)
    info = ctx.aggregate_plan(d_keys, d_offs, len(offs) - 1, d_sizes, max_depth)
    out = ctx.aggregate_fill()
    n, nb = info["n_prefixes"], info["blob_bytes"]
    raw = out["blob"].cpu().numpy()
    assert not raw[nb:].any(), "the padding up to 8 bytes must be zeros"
    return info, (raw[:nb], out["offsets"].cpu().numpy().view(np.uint64),
                  out["depth"].cpu().numpy().view(np.uint32), out["object_count"].cpu().numpy().view(np.uint64),
                  out["total_bytes"].cpu().numpy().view(np.uint64))


def same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and len(g) == len(w), (what, name, len(g), len(w))
        if not np.array_equal(g, w):
            i = int(np.flatnonzero(g != w)[0])
            raise AssertionError(f"{what}: {name}[{i}] = {g[i]}, want {w[i]}")


def check(ctx, keys, sizes=None, max_depth=0, align=0, host=False, what=""):
    keys = [bytes(k) for k in keys]
    assert keys == sorted(keys)
    if sizes is None:
        sizes = np.arange(1, len(keys) + 1, dtype=np.uint64) * 3
    sizes = np.asarray(sizes, np.uint64)
    want = R.rows_to_arrays(R.aggregate_dict(keys, sizes, max_depth))
    blob, offs = O.keys_to_blob(keys)
    info, got = device_rows(ctx, blob, offs, sizes, max_depth, align)
    same(got, want, what)
    assert info["n_objects"] == len(keys) and info["first_unsorted"] == (1 << 64) - 1
    assert info["total_bytes"] == int(np.sum(sizes, dtype=np.uint64)) if len(keys) else info["total_bytes"] == 0
    assert info["max_depth_seen"] == (int(want[2].max()) if len(want[2]) else 0)
    if host:
        same(s3imph.aggregate(blob, offs, sizes, max_depth), want, what + " (host)")
    return want


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_fixtures(ctx, case):
    keys = [k.encode() for k, _ in case["objects"]]
    want = check(ctx, keys, [z for _, z in case["objects"]], case["max_depth"], host=True, what=case["name"])
    prefixes = [p.decode() for p in R.keys_of(want[0], want[1])]
    if "prefixes" in case:
        assert prefixes == case["prefixes"]
    for p, st in case.get("stats", {}).items():
        assert int(want[3][prefixes.index(p)]) == st["object_count"]


DEGENERATE = {
    "no_objects": [],
    "one_key_no_slash": [b"abc"],
    "only_slashes": [b"////"],
    "only_slashes_long": [b"/" * 29],
    "empty_key": [b""],
    "empty_keys": [b"", b"", b"a/"],
    "identical_neighbours": [b"a/b", b"a/b", b"a/b/c", b"a/b/c", b"a/b/c"],
    "begin_and_end_with_slash": [b"/a/", b"/a/b/", b"/b/", b"c/"],
    "double_slash": [b"a//b", b"a//c", b"a/b//", b"a/b///x"],
    "slash_at_word_edges": [b"1234567/", b"1234567/8", b"12345678/", b"12345678/9abcdef/", b"12345678/9abcdef/0"],
}


@pytest.mark.parametrize("name", DEGENERATE, ids=list(DEGENERATE))
def test_degenerate_inputs(ctx, name):
    check(ctx, DEGENERATE[name], host=True, what=name)
    check(ctx, DEGENERATE[name], max_depth=1, what=name + " depth 1")


def test_no_sizes_means_zero(ctx):
    keys = [b"a/b", b"a/c/d", b"b"]
    blob, offs = O.keys_to_blob(keys)
    _, got = device_rows(ctx, blob, offs, None)
    same(got, R.rows_to_arrays(R.aggregate_dict(keys, [0, 0, 0])))
    same(s3imph.aggregate(blob, offs, None), R.rows_to_arrays(R.aggregate_dict(keys, [0, 0, 0])))


LCP_EDGES = {
    "lcp_ends_inside_a_segment": [b"ab/c", b"abc/d"],
    "shorter_key_is_a_whole_prefix": [b"a/b", b"a/b/c"],
    "slash_exactly_at_lcp_word_edge": [b"a/bcdefg", b"a/bcdefg/h", b"a/bcdefg/h/i"],
    "differ_below_slash": [b"a!/x", b"a/x"],
    "differ_at_0x80_and_above": [b"a/\x7f/x", b"a/\x80/x", b"a/\xc3\xa9/x", b"a/\xc3\xa9/y", b"a/\xff/"],
    "differ_just_above_slash": [b"a/x", b"a0/x", b"a0/y"],
}


@pytest.mark.parametrize("name", LCP_EDGES, ids=list(LCP_EDGES))
def test_lcp_edges(ctx, name):
    for align in (0, 3):
        check(ctx, LCP_EDGES[name], align=align, what=name)


def test_keys_longer_than_32k(ctx):
    """Keys of 40 000 bytes (longer than any on-chip window a key pass may stage) that part
    only near their end, next to short ones."""
    seg = (b"d" * 99 + b"/") * 400
    keys = sorted([seg + b"x/1", seg + b"x/2", seg + b"y", seg[:-1], b"d", seg[:20000] + b"!"])
    check(ctx, keys, what="long keys")
    check(ctx, keys, max_depth=2, align=5, what="long keys, depth 2")


def test_rows_at_the_byte_emit_chunk_edges(ctx):
    """The byte emit writes the prefix blob in chunks of 256 words (2048 bytes), one workgroup each:
    rows of 1 to 9 bytes (up to three inside one word), a row that ends exactly on the chunk edge at
    byte 2048, a row that owns a whole chunk, a blob length that is no multiple of 8."""
    keys = [b"/////////x", b"a" * 2002 + b"/x", b"b/c/d/e/f/g/h/i/x", b"c" * 4200 + b"/y/z"]
    want = check(ctx, keys, [5, 1 << 40, 7, (1 << 64) - 3], what="chunk edges")
    assert want[1].tolist() == [0, 0, 1, 3, 6, 10, 15, 21, 28, 36, 45, 2048, 2050, 2054, 2060, 2068, 2078, 2090,
                                2104, 2120, 6321, 10524]
    check(ctx, keys, align=3, what="chunk edges, misaligned keys")


def random_keys(rng, m, max_len=9, alphabet=b"ab/!~\xc3"):
    alpha = np.frombuffer(alphabet, np.uint8)
    return sorted(bytes(alpha[rng.integers(0, len(alpha), rng.integers(0, max_len))]) for _ in range(m))


@pytest.mark.parametrize("max_depth", [0, 1, 2])
def test_random_small_sets(ctx, max_depth):
    rng = np.random.default_rng(500 + max_depth)
    for t in range(40):
        keys = random_keys(rng, int(rng.integers(1, 60)))
        check(ctx, keys, BIG[rng.integers(0, len(BIG), len(keys))], max_depth, align=t % 16, what=f"set {t}")


def test_every_blob_alignment(ctx):
    rng = np.random.default_rng(11)
    keys = random_keys(rng, 3000, max_len=40, alphabet=b"abcdefgh/")
    sizes = rng.integers(0, 1 << 40, len(keys), dtype=np.uint64)
    want = R.rows_to_arrays(R.aggregate_dict(keys, sizes))
    blob, offs = O.keys_to_blob(keys)
    for align in range(16):
        _, got = device_rows(ctx, blob, offs, sizes, align=align)
        same(got, want, f"alignment {align}")


def test_one_key_with_5000_slashes_among_10000(ctx):
    rng = np.random.default_rng(12)
    keys = [b"k%05d/" % i + (b"x/" if i % 3 == 0 else b"") + b"f" for i in range(10000)]
    keys.append(b"k05000/" + b"ab/" * 4999 + b"tail")
    keys.sort()
    sizes = rng.integers(0, 1 << 30, len(keys), dtype=np.uint64)
    want = check(ctx, keys, sizes, what="skew")
    assert int(want[2].max()) == 5000


def test_wrapping_sums(ctx):
    keys = [b"a/b/%02d" % i for i in range(40)] + [b"c/%02d" % i for i in range(9)]
    sizes = np.array([1 << 63, (1 << 64) - 1] * 24 + [1 << 63], np.uint64)
    want = check(ctx, keys, sizes, host=True, what="wrap")
    assert int(want[4][0]) == sum(int(z) for z in sizes) % (1 << 64)


def test_max_depth_cut(ctx):
    rng = np.random.default_rng(13)
    keys = random_keys(rng, 400, max_len=14, alphabet=b"ab/")
    assert max(k.count(b"/") for k in keys) >= 6
    for md in (1, 2):
        want = check(ctx, keys, max_depth=md, host=True, what=f"max_depth {md}")
        assert int(want[2].max()) == md


# ---- range ends: 2^21 + 5 keys -----------------------------------------------------------
DIGITS = np.frombuffer(b"0123456789ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz", np.uint8)


def range_listing():
    """3 keys, then 2^21 - 1 keys under a/ in nested directories that end inside the first
    1024-key block (a/p/), in a later block (a/q/), in a later superblock (a/r/, past key
    2^20) and together three keys before the end (a/, a/s/, a/s/~t/, a/s/~t/~u/), then z/y/x/
    whose directories end at m.  Sub-directories start with '~', so they sort after the files."""
    groups = [(b"a/p/", 700), (b"a/q/", 4300), (b"a/r/", 300_000), (b"a/r/~0/", 400_000), (b"a/r/~1/", 500_000),
              (b"a/s/", 100_000), (b"a/s/~t/", 300_000)]
    groups.append((b"a/s/~t/~u/", (1 << 21) - 1 - sum(c for _, c in groups)))
    parts, lens = [np.frombuffer(b"!0!1!2", np.uint8)], [np.full(3, 2, np.int64)]
    for prefix, cnt in groups:
        j = np.arange(cnt)
        mat = np.empty((cnt, len(prefix) + 4), np.uint8)
        mat[:, :len(prefix)] = np.frombuffer(prefix, np.uint8)
        for k in range(4):
            mat[:, len(prefix) + k] = DIGITS[(j // 62 ** (3 - k)) % 62]
        parts.append(mat.reshape(-1))
        lens.append(np.full(cnt, mat.shape[1], np.int64))
    parts.append(np.frombuffer(b"z/y/x/0z/y/x/1z/y/x/2", np.uint8))
    lens.append(np.full(3, 7, np.int64))
    blob = np.concatenate(parts)
    offs = np.concatenate(([0], np.cumsum(np.concatenate(lens)))).astype(np.uint64)
    rng = np.random.default_rng(14)
    sizes = rng.integers(0, 1 << 50, len(offs) - 1, dtype=np.uint64)
    sizes[::1000] = BIG[rng.integers(0, len(BIG), len(sizes[::1000]))]
    return blob, offs, sizes


def test_range_ends_over_blocks_and_superblocks(ctx):
    blob, offs, sizes = range_listing()
    m = len(offs) - 1
    assert m == (1 << 21) + 5
    # the numpy form against the dict form on a slice of the same listing (both ends of it)
    part = R.keys_of(blob, offs[:25_001]) + R.keys_of(blob, offs[-25_001:])
    assert part == sorted(part)
    psz = np.concatenate((sizes[:25_000], sizes[-25_000:]))
    pblob, poffs = O.keys_to_blob(part)
    same(R.aggregate_numpy(pblob, poffs, psz), R.rows_to_arrays(R.aggregate_dict(part, psz)), "numpy vs dict")
    want = R.aggregate_numpy(blob, offs, sizes)
    prefixes = {p: i for i, p in enumerate(R.keys_of(want[0], want[1]))}
    assert int(want[3][prefixes[b"a/"]]) == m - 6 and int(want[3][prefixes[b"z/y/x/"]]) == 3
    assert int(want[3][prefixes[b"a/p/"]]) == 700 and int(want[3][prefixes[b"a/r/"]]) == 1_200_000
    info, got = device_rows(ctx, blob, offs, sizes)
    same(got, want, "range ends")
    assert info["n_prefixes"] == len(prefixes)


# ---- refusals ------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["start", "middle", "end"])
def test_unsorted_input_is_refused(ctx, where):
    keys = [b"d/%05d" % i for i in range(5000)]
    bad = {"start": 1, "middle": 2600, "end": 4999}[where]
    keys[bad] = b"a" if where != "start" else b"c"  # smaller than its predecessor
    if where == "middle":
        keys[4000] = b"a"  # a later offender: the smallest index is the one reported
    blob, offs = O.keys_to_blob(keys)
    with pytest.raises(s3imph.MPHFError) as e:
        device_rows(ctx, blob, offs, None)
    assert e.value.status == s3imph.ERR_INVALID
    assert e.value.info["first_unsorted"] == bad
    assert f"key {bad} " in str(e.value) and str(e.value).startswith("aggregate: ")
    with pytest.raises(s3imph.MPHFError) as e:  # the failed plan left nothing to fill
        ctx.aggregate_fill(n_cap=10, blob_cap=80)
    assert e.value.status == s3imph.ERR_STATE
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.aggregate(blob, offs, None)
    assert e.value.status == s3imph.ERR_INVALID and f"key {bad} " in str(e.value)


def test_a_proper_prefix_after_its_extension_is_unsorted(ctx):
    blob, offs = O.keys_to_blob([b"a/b/c", b"a/b"])
    with pytest.raises(s3imph.MPHFError) as e:
        device_rows(ctx, blob, offs, None)
    assert e.value.status == s3imph.ERR_INVALID and e.value.info["first_unsorted"] == 1


def test_depth_past_uint16_is_refused_not_wrapped(ctx):
    keys = [b"a", b"b/" + b"/" * 65535, b"c"]
    blob, offs = O.keys_to_blob(keys)
    with pytest.raises(s3imph.MPHFError) as e:
        device_rows(ctx, blob, offs, None)
    assert e.value.status == s3imph.ERR_INVALID and "65535" in str(e.value)
    info, got = device_rows(ctx, blob, offs, None, max_depth=3)  # cut before it matters
    assert info["n_prefixes"] == 4 and list(got[2]) == [0, 1, 2, 3]
    keys[1] = b"b/" + b"/" * 65534  # exactly 65535, the deepest depth a uint16 holds: planned
    blob, offs = O.keys_to_blob(keys)  # (not filled: its rows are 2 GB of prefix bytes)
    d_keys, d_offs, _ = listing_to_dev(blob, offs, None)
    info = ctx.aggregate_plan(d_keys, d_offs, 3)
    assert info["max_depth_seen"] == 65535 and info["n_prefixes"] == 65536
    assert info["blob_bytes"] == sum(range(2, 65537))


def test_fill_without_a_plan():
    c = s3imph.DeviceBuilder(0)
    try:
        with pytest.raises(s3imph.MPHFError) as e:
            c.aggregate_fill(n_cap=4, blob_cap=64)
        assert e.value.status == s3imph.ERR_STATE
    finally:
        c.close()


def test_short_capacities(ctx):
    import torch
    keys = [b"a/b/c", b"a/b/d", b"e/f"]
    blob, offs = O.keys_to_blob(keys)
    pad = np.zeros(24, np.uint8)
    pad[:len(blob)] = blob
    d_keys = torch.from_numpy(pad).to("cuda")
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).to("cuda")
    info = ctx.aggregate_plan(d_keys, d_offs, 3)
    assert (info["n_prefixes"], info["blob_bytes"]) == (4, 8)
    for kw in ({"n_cap": 3}, {"blob_cap": 7}, {"blob_cap": 0}):
        with pytest.raises(s3imph.MPHFError) as e:
            ctx.aggregate_fill(**kw)
        assert e.value.status == s3imph.ERR_INVALID
    out = ctx.aggregate_fill()  # the plan survives a refused fill
    assert bytes(out["blob"].cpu().numpy()[:8]) == b"a/a/b/e/"
