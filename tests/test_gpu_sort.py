"""The listing sort on the GPU (include/s3imph.h section 5f) against tests/sort_ref.py: the order
and the info, the gather, and the directory built from an unsorted listing — which must equal,
file for file, the one the existing sorted-only build writes for the listing sorted beforehand."""
import json
import os

import numpy as np
import pytest

import aggregate_ref as R
import oracle as O
import s3imph
import sort_ref as S
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NONE = S.NONE
AGG_CASES = json.load(open(os.path.join(GOLDEN, "aggregate", "cases.json")))["cases"]
TIER_CASES = json.load(open(os.path.join(GOLDEN, "tiers", "cases.json")))["index_cases"]
UNICODE = [k.encode() for k in json.load(open(os.path.join(GOLDEN, "mphf_unicode.json")))["keys"]]


@pytest.fixture(scope="module")
def ctx():
    c = s3imph.DeviceBuilder(0)
    yield c
    c.close()


def to_dev(keys, sizes=None, tiers=None, align=0, base=0):
    """The listing as torch tensors: the key blob starts `align` bytes into its allocation and its
    first key `base` bytes into the blob (offsets[0] = base); readable up to round_up(offsets[m], 8)."""
    import torch
    blob, offs = O.keys_to_blob(keys)
    offs = offs + np.uint64(base)
    end8 = (int(offs[-1]) + 7) // 8 * 8
    raw = np.full(align + end8 + 8, 0xA5, np.uint8)  # bytes outside the keys must not matter
    raw[align + base:align + base + len(blob)] = blob
    d_keys = torch.from_numpy(raw).to("cuda")[align:]
    d_offs = torch.from_numpy(offs.view(np.int64).copy()).to("cuda")
    d_sizes = None if sizes is None else torch.from_numpy(np.asarray(sizes, np.uint64).view(np.int64).copy()).to("cuda")
    d_tiers = None if tiers is None else torch.from_numpy(np.asarray(tiers, np.uint8).copy()).to("cuda")
    return d_keys, d_offs, d_sizes, d_tiers


def check_sort(ctx, keys, align=0, base=0, what=""):
    """Sorts on the device; the order and the info must be sort_ref's.  Returns the info."""
    keys = [bytes(k) for k in keys]
    d_keys, d_offs, _, _ = to_dev(keys, align=align, base=base)
    order, info = ctx.sort_objects(d_keys, d_offs, len(keys))
    got = order.cpu().numpy().view(np.uint32)
    want = S.sort_order(keys)
    if not np.array_equal(got, want):
        j = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: order[{j}] = {got[j]}, want {want[j]}")
    rounds = info.pop("rounds")
    assert info == S.info(keys), what
    max_len = max(map(len, keys))
    assert rounds <= (max_len + 1 + 6) // 7
    assert (rounds == 0) == (info["first_unsorted"] == NONE)
    return dict(info, rounds=rounds)


def distinct(m, seed=3, lo=0, hi=24):
    """m distinct keys of lo..hi bytes over a small alphabet (many shared chunks), in random order."""
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"\x00/aab\x7f\x80\xff", np.uint8)
    keys = set()
    while len(keys) < m:
        keys.add(alphabet[rng.integers(0, len(alphabet), int(rng.integers(lo, hi + 1)))].tobytes())
    keys = sorted(keys)
    return [keys[i] for i in rng.permutation(m)]


# ---------------------------------------------------------------- order and info ------------
@pytest.mark.parametrize("m", [63, 64, 65, 1023, 1024, 1025])
def test_sizes_around_the_wave_and_the_workgroup(ctx, m):
    info = check_sort(ctx, distinct(m, seed=m), what=f"m={m}")
    assert info["first_unsorted"] != NONE and info["n_equal"] == 0


def test_one_key_and_two_keys_in_both_orders(ctx):
    assert check_sort(ctx, [b"only/key"])["rounds"] == 0
    assert check_sort(ctx, [b""])["rounds"] == 0
    assert check_sort(ctx, [b"a/x", b"b/x"])["first_unsorted"] == NONE
    info = check_sort(ctx, [b"b/x", b"a/x"])
    assert info["first_unsorted"] == 1 and info["rounds"] >= 1


def test_sorted_input_is_the_identity_without_rounds(ctx):
    keys = sorted(distinct(1500, seed=11))
    d_keys, d_offs, _, _ = to_dev(keys)
    order, info = ctx.sort_objects(d_keys, d_offs, len(keys))
    assert np.array_equal(order.cpu().numpy().view(np.uint32), np.arange(len(keys), dtype=np.uint32))
    assert info["first_unsorted"] == 2**64 - 1 and info["rounds"] == 0 and info["n_equal"] == 0
    check_sort(ctx, keys + keys[-1:], what="sorted with an equal pair")  # n_equal == 1 from the first pass


def test_reverse_sorted_input(ctx):
    keys = sorted(distinct(1500, seed=12), reverse=True)
    assert check_sort(ctx, keys, what="reverse")["first_unsorted"] == 1


@pytest.mark.parametrize("align", [1, 2, 3, 4, 5, 6, 7])
def test_blob_at_every_alignment_and_offsets_not_from_zero(ctx, align):
    keys = distinct(300, seed=20 + align, hi=40)
    check_sort(ctx, keys, align=align, what=f"align {align}")
    check_sort(ctx, keys, align=align, base=8 - align + 3, what=f"align {align}, offsets[0] != 0")
    check_sort(ctx, keys, base=align, what=f"offsets[0] = {align}")


# ---------------------------------------------------------------- byte semantics ------------
BYTES = {
    "empty_among_others": [b"b", b"", b"a", b"\x00"],
    "several_empty": [b"a", b"", b"", b"\x00", b""],
    "prefixes_and_nul": [b"a0", b"a/", b"a\x00\x00", b"a\x00", b"a", b"a\x00\x01", b"a\x01"],
    "high_bytes": [b"\xff", b"\x80", b"\x7f", b"\x7f\xff", b"\x80\x00", b"a\xffb", b"a\x7fb", b"a\x80b", b"\xff\xff"],
    "unicode": UNICODE[::-1] + [k + b"/" for k in UNICODE] + [k[:-1] for k in UNICODE],
    "chunk_edges": [b"12345678", b"1234567\x00", b"1234567", b"123456", b"12345678\x00",
                    b"12345678901234", b"1234567890123\x00", b"1234567890123", b"12345678901234\x00",
                    b"123456789012345", b"12345678901234\x00\x00", b"1234567890123456"],
}


@pytest.mark.parametrize("name", BYTES, ids=list(BYTES))
def test_byte_semantics(ctx, name):
    keys = BYTES[name]
    check_sort(ctx, keys, what=name)
    check_sort(ctx, keys[::-1], what=name + " reversed")
    check_sort(ctx, keys + keys, what=name + " doubled")


@pytest.mark.parametrize("at", [6, 7, 8, 13, 14, 15])
def test_first_difference_at_a_chunk_edge(ctx, at):
    """Keys that agree on `at` bytes and differ in the next, with tails that would order them
    the other way if the differing byte were missed."""
    stem = b"abcdefghijklmnopqrstuvwx"[:at]
    keys = [stem + bytes([c]) + tail for c, tail in ((0xff, b"a"), (0x80, b"z"), (0x7f, b""), (0x00, b"zz"),
                                                    (0x2f, b"\xff"), (0x01, b"\x00"))]
    keys += [stem, stem[:-1]]
    check_sort(ctx, keys, what=f"differ at {at}")
    check_sort(ctx, keys[::-1], what=f"differ at {at}, reversed")


# ---------------------------------------------------------------- stability -----------------
def test_identical_keys_keep_their_input_order(ctx):
    info = check_sort(ctx, [b"same/key"] * 65, what="65 identical")  # found sorted by the first pass
    assert info["n_equal"] == 64 and info["rounds"] == 0
    info = check_sort(ctx, [b"z"] + [b"same/key/longer-than-a-chunk"] * 65, what="65 identical after a larger key")
    assert info["n_equal"] == 64 and info["rounds"] >= 1


def test_duplicates_come_out_of_the_gather_in_input_order(ctx):
    rng = np.random.default_rng(4)
    pool = [b"dup/a", b"dup/b", b"dup/a/", b"dup", b"other/key/with/more/than/seven/bytes"]
    keys = [pool[i] for i in rng.integers(0, len(pool), 700)]
    sizes = np.arange(len(keys), dtype=np.uint64)  # the size names the input position
    d_keys, d_offs, d_sizes, _ = to_dev(keys, sizes)
    order, info = ctx.sort_objects(d_keys, d_offs, len(keys))
    out = ctx.gather_objects(d_keys, d_offs, len(keys), order, d_sizes=d_sizes)
    got = out["sizes"].cpu().numpy().view(np.uint64)
    assert np.array_equal(got, S.sort_order(keys).astype(np.uint64))
    assert info["n_equal"] == len(keys) - len(pool)


# ---------------------------------------------------------------- depth and segment size ----
def test_300_keys_sharing_200_bytes(ctx):
    rng = np.random.default_rng(5)
    stem = bytes(rng.integers(0, 256, 200, dtype=np.uint8))
    keys = [stem + bytes([int(c)]) for c in rng.permutation(256)] + [stem + b"\x00" + bytes([c]) for c in range(44)]
    info = check_sort(ctx, keys, what="long shared prefix")  # rounds <= ceil(203 / 7) = 29 checked there
    assert info["rounds"] >= 1 and info["n_equal"] == 0


def test_5000_keys_sharing_their_first_chunk(ctx):
    rng = np.random.default_rng(6)
    keys = [b"shared/" + b"%05d" % int(i) + bytes(rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8))
            for i in rng.permutation(5000)]
    check_sort(ctx, keys, what="one wide segment")


def test_lengths_1_to_1024_in_one_listing(ctx):
    rng = np.random.default_rng(8)
    keys = [bytes(rng.integers(0x61, 0x64, n, dtype=np.uint8)) for n in rng.permutation(np.arange(1, 1025))]
    assert max(map(len, keys)) == 1024
    check_sort(ctx, keys, what="lengths 1..1024")


# ---------------------------------------------------------------- one medium listing --------
@pytest.mark.parametrize("kind,avg,n", [(0, 32, 200_000), (1, 0, 20_000)], ids=["s3_like_200k", "skewed_20k"])
def test_medium_listing_twice(ctx, kind, avg, n):
    blob, offs = s3imph.gen_keys(kind, 42, avg, 0, n)
    keys = R.keys_of(blob, offs)
    keys = [keys[i] for i in np.random.default_rng(7).permutation(n)]
    want = S.sort_order(keys)
    d_keys, d_offs, _, _ = to_dev(keys)
    runs = []
    for _ in range(2):
        order, info = ctx.sort_objects(d_keys, d_offs, n)
        runs.append((order.cpu().numpy().view(np.uint32), info))
    assert np.array_equal(runs[0][0], want)
    assert np.array_equal(runs[1][0], runs[0][0]) and runs[1][1] == runs[0][1]
    assert runs[0][1]["n_equal"] == 0 and runs[0][1]["key_bytes"] == int(offs[-1])


# ---------------------------------------------------------------- gather --------------------
@pytest.fixture(scope="module")
def gathered(ctx):
    keys = distinct(3000, seed=9, hi=70) + [b"", b"", b"x" * 1024]
    rng = np.random.default_rng(10)
    sizes = rng.integers(0, 1 << 63, len(keys), dtype=np.uint64)
    tiers = rng.integers(0, s3imph.NUM_TIERS, len(keys), dtype=np.uint8)
    dev = to_dev(keys, sizes, tiers, align=3, base=5)
    order, info = ctx.sort_objects(dev[0], dev[1], len(keys))
    return {"keys": keys, "sizes": sizes, "tiers": tiers, "dev": dev, "order": order, "info": info,
            "want": S.sort_order(keys)}


def test_gather_matches_numpy_indexing(ctx, gathered):
    g = gathered
    d_keys, d_offs, d_sizes, d_tiers = g["dev"]
    m = len(g["keys"])
    out = ctx.gather_objects(d_keys, d_offs, m, g["order"], d_sizes=d_sizes, d_tiers=d_tiers)
    want_keys = [g["keys"][i] for i in g["want"]]
    blob, offs = O.keys_to_blob(want_keys)
    got_offs = out["offsets"].cpu().numpy().view(np.uint64)
    assert got_offs[0] == 0 and np.array_equal(got_offs, offs)
    raw = out["keys"].cpu().numpy()
    assert len(raw) == (len(blob) + 7) // 8 * 8 and out["key_bytes"] == len(blob) == g["info"]["key_bytes"]
    assert np.array_equal(raw[:len(blob)], blob)
    assert not raw[len(blob):].any(), "the padding up to 8 bytes must be zeros"
    assert np.array_equal(out["sizes"].cpu().numpy().view(np.uint64), g["sizes"][g["want"]])
    assert np.array_equal(out["tiers"].cpu().numpy(), g["tiers"][g["want"]])
    # the gathered listing is what the existing aggregation wants
    agg = ctx.aggregate_plan(out["keys"], out["offsets"], m, out["sizes"], tiers=out["tiers"])
    assert agg["first_unsorted"] == 2**64 - 1 and agg["n_objects"] == m


CHUNK = 2048  # bytes of output one workgroup of the byte emit writes: 256 words

# output key lengths, in output order: a key that ends exactly on the chunk edge at byte 2048, two
# empty keys on that edge, nine keys inside two words, a key that owns all of chunk 2 and chunk 3's
# start (a workgroup whose first and last owner are the same key), an empty last key, 6164 bytes in
# all (no multiple of 8); then exactly one chunk, and one chunk plus one byte
CHUNK_EDGE_LAYOUTS = {
    "edges": [2040, 3, 0, 5, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 4100, 0, 7, 0],
    "one_chunk": [0, 2047, 1, 0],
    "one_chunk_and_a_byte": [0, 2047, 1, 1, 0],
}


@pytest.mark.parametrize("name", CHUNK_EDGE_LAYOUTS, ids=list(CHUNK_EDGE_LAYOUTS))
def test_gather_at_chunk_edges(ctx, name):
    """The output layout is chosen here, not left to the sort: the order is a seeded permutation
    and the input listing is the wanted output scattered by it."""
    import torch
    lens = CHUNK_EDGE_LAYOUTS[name]
    m = len(lens)
    rng = np.random.default_rng(21)
    want_keys = [rng.integers(1, 256, n, dtype=np.uint8).tobytes() for n in lens]
    order = rng.permutation(m).astype(np.uint32)  # order[j] = input index of the j-th output key
    keys = [b""] * m
    for j, i in enumerate(order):
        keys[i] = want_keys[j]
    sizes = rng.integers(0, 1 << 63, m, dtype=np.uint64)
    tiers = rng.integers(0, s3imph.NUM_TIERS, m, dtype=np.uint8)
    blob, offs = O.keys_to_blob(want_keys)
    assert offs.tolist() == [0] + np.cumsum(lens).tolist()
    if name == "edges":
        assert len(blob) == 6164 and offs[4] == CHUNK
        owners = np.searchsorted(offs, np.arange(4) * CHUNK, side="right") - 1
        assert owners.tolist() == [0, 6, 16, 16]
    else:
        assert len(blob) == CHUNK + (name != "one_chunk")
    d_keys, d_offs, d_sizes, d_tiers = to_dev(keys, sizes, tiers)
    d_order = torch.from_numpy(order.view(np.int32).copy()).to("cuda")
    out = ctx.gather_objects(d_keys, d_offs, m, d_order, d_sizes=d_sizes, d_tiers=d_tiers)
    assert np.array_equal(out["offsets"].cpu().numpy().view(np.uint64), offs)
    raw = out["keys"].cpu().numpy()
    assert len(raw) == (len(blob) + 7) // 8 * 8 and out["key_bytes"] == len(blob)
    assert np.array_equal(raw[:len(blob)], blob)
    assert not raw[len(blob):].any(), "the padding up to 8 bytes must be zeros"
    assert np.array_equal(out["sizes"].cpu().numpy().view(np.uint64), sizes[order])
    assert np.array_equal(out["tiers"].cpu().numpy(), tiers[order])


def test_gather_without_sizes_and_tiers_and_into_a_misaligned_blob(ctx, gathered):
    import torch
    g = gathered
    d_keys, d_offs, _, _ = g["dev"]
    m = len(g["keys"])
    out = ctx.gather_objects(d_keys, d_offs, m, g["order"])
    assert out["sizes"] is None and out["tiers"] is None
    blob, offs = O.keys_to_blob([g["keys"][i] for i in g["want"]])
    assert np.array_equal(out["keys"].cpu().numpy()[:len(blob)], blob)
    # the output blob at an odd address: the byte-store form
    cap = (len(blob) + 7) // 8 * 8
    buf = torch.full((cap + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    d_off_out = torch.empty(m + 1, dtype=torch.int64, device="cuda")
    rc = s3imph.LIB.s3imph_gather_objects_device(ctx._h, d_keys.data_ptr(), d_offs.data_ptr(), None, None, m,
                                                 g["order"].data_ptr(), buf.data_ptr() + 1, cap,
                                                 d_off_out.data_ptr(), None, None, None)
    assert rc == s3imph.OK
    raw = buf.cpu().numpy()
    assert raw[0] == 0x5A and np.array_equal(raw[1:1 + len(blob)], blob)
    assert not raw[1 + len(blob):1 + cap].any() and (raw[1 + cap:] == 0x5A).all()


def test_gather_refuses_a_short_blob_and_a_bad_order(ctx, gathered):
    g = gathered
    d_keys, d_offs, _, _ = g["dev"]
    m = len(g["keys"])
    need = (g["info"]["key_bytes"] + 7) // 8 * 8
    with pytest.raises(s3imph.MPHFError) as e:
        ctx.gather_objects(d_keys, d_offs, m, g["order"], keys_cap=need - 8)
    assert e.value.status == s3imph.ERR_INVALID and str(e.value).startswith("sort: ")
    bad = g["order"].clone()
    bad[17] = m  # not an index
    with pytest.raises(s3imph.MPHFError) as e:
        ctx.gather_objects(d_keys, d_offs, m, bad)
    assert e.value.status == s3imph.ERR_INVALID and "order[17]" in str(e.value)


def test_empty_listing_on_the_device(ctx):
    import torch
    d_offs = torch.zeros(1, dtype=torch.int64, device="cuda")
    order, info = ctx.sort_objects(None, d_offs, 0)
    assert len(order) == 0 and info["n_objects"] == 0 and info["first_unsorted"] == 2**64 - 1
    out = ctx.gather_objects(None, d_offs, 0, None)
    assert out["offsets"].cpu().tolist() == [0] and out["key_bytes"] == 0


def test_host_sort(ctx):
    keys = distinct(2000, seed=13)
    blob, offs = O.keys_to_blob(keys)
    order, info = s3imph.sort_objects(blob, offs)
    assert order.dtype == np.uint32 and np.array_equal(order, S.sort_order(keys))
    info.pop("rounds")
    assert info == S.info(keys)
    # offsets that do not start at 0
    order2, _ = s3imph.sort_objects(np.concatenate([np.zeros(5, np.uint8), blob]), offs + np.uint64(5))
    assert np.array_equal(order2, order)


# ---------------------------------------------------------------- listing to directory ------
def big_listing(m=20_000, seed=5):
    """The listing() shape of test_gpu_index_from_objects.py: about m distinct object keys, 0 to 5
    directories deep, a few objects per directory (sorted)."""
    rng = np.random.default_rng(seed)
    keys = set()
    while len(keys) < m:
        depth = int(rng.integers(0, 6))
        dirs = [b"d%02d" % int(rng.integers(0, 40))] + [b"s%d" % int(rng.integers(0, 4)) for _ in range(depth)]
        keys.add(b"/".join(dirs[:depth]) + (b"/" if depth else b"") + b"obj-%04d.bin" % int(rng.integers(0, 3000)))
    keys = sorted(keys)
    sizes = rng.integers(0, 1 << 44, len(keys), dtype=np.uint64)
    sizes[::97] = 0
    tiers = rng.integers(0, s3imph.NUM_TIERS, len(keys), dtype=np.uint8)
    return keys, sizes, tiers


def listings():
    out = []
    for c in AGG_CASES:
        out.append(("agg_" + c["name"], [k.encode() for k, _ in c["objects"]], [z for _, z in c["objects"]], None,
                    c["max_depth"]))
    for c in TIER_CASES:
        out.append(("tiers_" + c["name"], [k.encode() for k, _, _ in c["objects"]], [z for _, z, _ in c["objects"]],
                    [t for _, _, t in c["objects"]], 0))
    keys, sizes, tiers = big_listing()
    out.append(("listing_20k", keys, sizes, None, 0))
    out.append(("listing_20k_tiers", keys, sizes, tiers, 0))
    out.append(("listing_20k_depth_2", keys, sizes, None, 2))
    return out


LISTINGS = listings()


def files_of(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)


@pytest.mark.parametrize("case", LISTINGS, ids=[c[0] for c in LISTINGS])
def test_directory_equals_the_sorted_build(tmp_path, case):
    name, keys, sizes, tiers, max_depth = case
    m = len(keys)
    perm = np.random.default_rng(7).permutation(m)
    keys = [keys[i] for i in perm]
    sizes = np.asarray(sizes, np.uint64)[perm]
    tiers = None if tiers is None else np.asarray(tiers, np.uint8)[perm]
    blob, offs = O.keys_to_blob(keys)
    got, want = tmp_path / "got", tmp_path / "want"
    got.mkdir()
    want.mkdir()
    s3imph.build_index_from_unsorted_objects(blob, offs, sizes, str(got), tiers=tiers, max_depth=max_depth)
    # the reference: the code as it stands, on the listing sorted (stably) beforehand
    order = S.sort_order(keys)
    skeys = [keys[i] for i in order]
    sblob, soffs = O.keys_to_blob(skeys)
    s3imph.build_index_from_objects(sblob, soffs, sizes[order], str(want), max_depth=max_depth,
                                    tiers=None if tiers is None else tiers[order])
    names = files_of(want)
    assert files_of(got) == names and "object_count.u64" in names
    assert any(n.startswith("tier_stats") for n in names) == (tiers is not None)
    for n in names:
        if n != "manifest.json":
            assert (got / n).read_bytes() == (want / n).read_bytes(), n
    a, b = s3imph.read_manifest(str(got)), s3imph.read_manifest(str(want))
    a.pop("created_at")
    b.pop("created_at")
    assert a == b
    s3imph.verify_manifest(str(got))
    # the reader answers from it
    rows = R.aggregate_dict(skeys, sizes[order], max_depth)
    at = list(range(0, len(rows), max(1, len(rows) // 200)))
    sample = [rows[i] for i in at]
    with s3imph.Index(str(got)) as idx:
        assert idx.count == len(rows)
        pos = idx.lookup([r[0] for r in sample])
        assert np.array_equal(pos, np.array(at, np.uint64))
        found, cnt, tot = idx.stats_for_prefix([r[0] for r in sample])
        assert found.all()
        assert np.array_equal(cnt, np.array([r[2] for r in sample], np.uint64))
        assert np.array_equal(tot, np.array([r[3] for r in sample], np.uint64))
    # nothing existing changed: the sorted-only call still refuses the shuffled listing
    other = tmp_path / "other"
    other.mkdir()
    if S.first_unsorted(keys) == NONE:
        s3imph.build_index_from_objects(blob, offs, sizes, str(other), max_depth=max_depth, tiers=tiers)
    else:
        with pytest.raises(s3imph.MPHFError) as e:
            s3imph.build_index_from_objects(blob, offs, sizes, str(other), max_depth=max_depth, tiers=tiers)
        assert e.value.status == s3imph.ERR_INVALID and str(e.value).startswith("aggregate: ")
        assert not os.listdir(other)
