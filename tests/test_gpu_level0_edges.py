"""Level 0 at the edges the big random parity sets only wander over (run on an MI355X, -m gpu).

Everything is integer, so every comparison is exact: mph.bin bytes, mph_fp, mph_pos, lookup
results and finalize arrays against the CPU oracle.  Four groups:

A. device blob pointers that really are misaligned (a view `shift` bytes into a 16-byte
   aligned allocation): the build's per-lane level-0 hash k_hash_count0 on the reservation
   path (its plain loop and its length-sorted groups), k_lookup, and finalize without the
   LDS-staged key pass;
B. a key whose FNV-1a-64 is 0 (S3IMPH_ERR_KEY_HASH_ZERO) through each level-0 hash kernel
   and each entry point, and its precedence below duplicates;
C. the round / window edges of the aligned hashes (k_hash0_pair's 32 KiB window and its
   256 length classes, k_hash_skew's 64-key batches and 64-byte chunk steps) on crafted
   length layouts, and the blob's last bytes at every residue mod 16;
D. P0 (level 0 through super-tiles) at 33-130 tiles instead of 2051 and up, fused and
   unfused, in a child process that sets the geometry knobs.

Which kernel hashes a set is decided by the host from the pointer (s3imph_binned.hip
launch_binned_count: 16-byte aligned or not), by the device from 1024 sampled key lengths
(k_init_state, restated in `_skewed`), and by the level-0 path: only the reservation path
(no "hscan0" stage) runs the hash without a histogram, which a context reserved for 2^20
keys takes for every set here (res_fits: 4 n <= bucket_cap).  Each case asserts all three.
"""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from conftest import GOLDEN, from_dev, to_dev

pytestmark = pytest.mark.gpu

NOT_FOUND = np.uint64(2**64 - 1)
# FNV-1a-64 preimages of 0 (pinned on the CPU in test_oracle.py::test_zero_hash_preimages)
ZERO_KEY = b"!0IC=VloaY"
ZERO_KEYS = [ZERO_KEY, b"77kepQFQ8Kl", bytes.fromhex("d56bb95342870836")]
SHIFTS = [1, 4, 8, 15]


@pytest.fixture(scope="module")
def s3():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import s3imph
    return s3imph


@pytest.fixture(scope="module")
def ctx(s3):
    c = s3.DeviceBuilder(0)
    c.reserve(1 << 20)  # bucket_cap 1.25 x 2^20: every set here (n <= 2^18) takes the reservation path
    c.set_profiling(1)
    yield c
    c.close()


# ------------------------------------------------------------------------ helpers ----
def _dev_view(a, shift):
    """`a` (u8) at `shift` bytes into a zeroed, 16-byte aligned device allocation: a view
    whose data pointer is `shift` mod 16, readable to round_up(len(a), 8) and 16 bytes on."""
    import torch
    a = np.ascontiguousarray(a, np.uint8)
    n = len(a)
    buf = torch.zeros(shift + (n + 7) // 8 * 8 + 16, dtype=torch.uint8, device="cuda")
    if n:
        buf[shift:shift + n] = torch.from_numpy(a.copy()).to("cuda")
    view = buf[shift:]
    assert buf.data_ptr() % 16 == 0
    assert view.data_ptr() % 16 == shift
    return view


def _skewed(offs):
    """k_init_state's rule (s3imph_kernels.hip): 1024 key lengths sampled at t * n // 1024;
    skewed iff the longest exceeds twice their mean + 16 B."""
    n = len(offs) - 1
    if n == 0:
        return False
    i = np.arange(1024, dtype=np.uint64) * np.uint64(n) // np.uint64(1024)
    ln = (offs[i + np.uint64(1)] - offs[i]).astype(np.int64)
    return int(ln.max()) * 1024 > 2 * int(ln.sum()) + 16 * 1024


def _sample_indices(n):
    return set(int(t) * n // 1024 for t in range(1024))


def _make(ln, o0=0, fixed=None):
    """(blob, offs) for key lengths `ln` behind `o0` leading bytes.  Contents are a fixed
    byte pattern with the key's index stamped into its first 4 bytes (a per-length counter
    for keys of 1-3 bytes), so keys are distinct; `fixed` {index: bytes} sets whole keys."""
    ln = np.array(ln, np.int64)
    fixed = fixed or {}
    for i, k in fixed.items():
        ln[i] = len(k)
    n = len(ln)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(ln, dtype=np.uint64)
    offs += np.uint64(o0)
    total = int(offs[-1])
    blob = ((np.arange(total, dtype=np.int64) * 131 + 17) % 251).astype(np.uint8)
    st = offs[:-1].astype(np.int64)
    idx = np.arange(n, dtype=np.int64)
    big = ln >= 4
    for b in range(4):
        blob[st[big] + b] = (idx[big] >> (8 * b)) & 255
    assert int((ln == 0).sum()) <= 1
    for L in (1, 2, 3):
        sel = np.nonzero(ln == L)[0]
        assert len(sel) <= 256
        for c, i in enumerate(sel):
            blob[st[i]] = c
    for i, k in fixed.items():
        blob[st[i]:st[i] + len(k)] = np.frombuffer(k, np.uint8)
    return blob, offs


def _layout(n, runs, skew, o0=0, fixed=None):
    """n keys of 8-40 B with `runs` [(first index, [lengths], blob offset mod 16 of the run's
    first key, or None)] laid over them; the key before a run is lengthened by 0-15 B to
    reach the residue.  skew: one 6000 B key on a sampled index makes the set skewed."""
    ln = 8 + (np.arange(n, dtype=np.int64) * 7) % 33
    taken = set()
    for i0, ls, _ in runs:
        assert not taken & set(range(i0, i0 + len(ls))) and i0 + len(ls) <= n
        taken |= set(range(i0, i0 + len(ls)))
        ln[i0:i0 + len(ls)] = ls
    if skew:
        j = 512 * n // 1024
        assert j not in taken and j in _sample_indices(n)
        ln[j] = 6000
        taken.add(j)
    for i, k in (fixed or {}).items():
        assert i not in taken
        ln[i] = len(k)
        taken.add(i)
    for i0, ls, res in sorted(runs, key=lambda r: r[0]):
        if res is not None:
            assert i0 > 0 and i0 - 1 not in taken
            ln[i0 - 1] += (res - (o0 + int(ln[:i0].sum()))) % 16
            taken.add(i0 - 1)
    blob, offs = _make(ln, o0, fixed)
    for i0, ls, res in runs:
        assert res is None or int(offs[i0]) % 16 == res
    assert _skewed(offs) == skew
    return blob, offs


def _build(ctx, blob, offs, pos=None, shift=0):
    import torch
    n = len(offs) - 1
    d_blob = _dev_view(blob[: int(offs[-1])], shift)
    assert (d_blob.data_ptr() % 16 != 0) == (shift != 0)
    d_offs = to_dev(offs)
    d_pos = to_dev(pos) if pos is not None else None
    d_fp = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
    d_po = torch.zeros(max(n, 1), dtype=torch.int64, device="cuda")
    ctx.build(d_blob, d_offs, n, d_fp, d_po, d_pos=d_pos)
    torch.cuda.synchronize()
    return from_dev(d_fp)[:n], from_dev(d_po)[:n], ctx.mph_bin(), (d_blob, d_offs, d_fp, d_po)


def _on_reservation_path(ctx):
    """The last build's level 0 ran hash -> reservation scatter -> tiles: its hash had no
    histogram (k_hash0_pair / k_hash_skew, or k_hash_count0 with hist == nullptr)."""
    st = ctx.stage_times()
    assert "hash_count0" in st and "scatter0" in st and "hscan0" not in st, st


def _same(got, want):
    gfp, gpo, gmph = got[:3]
    st, fp, po, mph = want
    assert st == 0
    assert gmph == mph
    assert np.array_equal(gfp, fp)
    assert np.array_equal(gpo, po)


def _check(ctx, want, blob, offs, pos=None, shift=0):
    got = _build(ctx, blob, offs, pos, shift)
    _same(got, want)
    _on_reservation_path(ctx)
    return got


# ------------------------------------------------- A. truly misaligned device pointers ----
GEN_SETS = [("uniform", 1), ("uniform", 65), ("uniform", 5000), ("uniform", 70000),
            ("skewed", 5000), ("skewed", 70000), ("offset11_pos", 5000)]


@functools.lru_cache(maxsize=None)
def _gen_set(kind, n):
    """(blob, offs, pos, oracle build) of a gen_keys set, computed once for all shifts."""
    import s3imph
    if kind == "skewed":
        blob, offs = s3imph.gen_keys(1, 23, 0, 0, n)
    else:
        blob, offs = s3imph.gen_keys(0, 7, 24, 0, n)
    blob = blob[: int(offs[-1])]
    pos = None
    if kind == "offset11_pos":
        blob = np.concatenate([np.frombuffer(b"0123456789a", np.uint8), blob])
        offs = offs + np.uint64(11)
        pos = np.random.default_rng(n).permutation(n).astype(np.uint64) * np.uint64(3) + np.uint64(7)
    assert _skewed(offs) == (kind == "skewed")
    want = O.lib().build(blob, offs, pos)
    for a in (blob, offs) + want[1:3]:
        a.setflags(write=False)
    return blob, offs, pos, want


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kind,n", GEN_SETS, ids=["%s-%d" % s for s in GEN_SETS])
def test_misaligned_blob_build(s3, ctx, oracle_lib, kind, n, shift):
    """k_hash_count0 as the reservation path's level-0 hash at a device pointer that is
    `shift` mod 16: near-uniform lengths (its fnv_both_pf loop, n = 1 to more than one
    1024-key group per block), skewed lengths (its length-sorted 1024-key groups and their
    per-group "not skewed" branch), and a non-zero offsets[0] with caller positions."""
    blob, offs, pos, want = _gen_set(kind, n)
    _check(ctx, want, blob, offs, pos, shift)


@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("kind,n", [("uniform", 5000), ("skewed", 70000)])
def test_misaligned_blob_lookup(s3, ctx, oracle_lib, kind, n, shift):
    """k_lookup at misaligned key blobs: every member maps to its pos and 2000 keys of
    another seed to NOT_FOUND, at query counts around its i1 = i0 + 256 pairing."""
    import torch
    blob, offs, pos, want = _gen_set(kind, n)
    _, _, _, (d_blob, d_offs, d_fp, d_po) = _check(ctx, want, blob, offs, pos, shift)
    for q in (1, 255, 256, 257, 511, 512, 513, n):
        res = torch.full((q,), -2, dtype=torch.int64, device="cuda")
        ctx.lookup(d_blob, d_offs, q, d_fp, d_po, n, res)
        assert np.array_equal(from_dev(res), np.arange(q, dtype=np.uint64)), q
    qb, qo = s3.gen_keys(0, 8, 24, 10 ** 7, 2000)
    d_q = _dev_view(qb[: int(qo[-1])], shift)
    assert d_q.data_ptr() % 16 != 0
    res = torch.zeros(2000, dtype=torch.int64, device="cuda")
    ctx.lookup(d_q, to_dev(qo), 2000, d_fp, d_po, n, res)
    assert (from_dev(res) == NOT_FOUND).all()


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


@functools.lru_cache(maxsize=None)
def _finalize_set(n_obj):
    blob, offs = O.keys_to_blob(_prefix_set(7, n_obj, 8, 7, True))
    return blob, offs, O.lib().finalize(blob, offs)


@pytest.mark.parametrize("shift", [1, 8])
@pytest.mark.parametrize("n_obj", [3000, 300_000])
def test_misaligned_blob_finalize(s3, ctx, oracle_lib, n_obj, shift):
    """Finalize without the LDS-staged key pass (staged == false, k_fin_keys): depth, subtree
    and depth-index arrays of a sorted, ancestor-closed prefix set equal the oracle's."""
    import torch
    blob, offs, want = _finalize_set(n_obj)
    d_blob = _dev_view(blob, shift)
    assert d_blob.data_ptr() % 16 != 0
    r = ctx.finalize_index(d_blob, to_dev(offs), len(offs) - 1)
    torch.cuda.synchronize()
    for k in ("depth", "max_depth_in_subtree"):
        assert np.array_equal(r[k].cpu().numpy().view(np.uint32), want[k]), k
    for k in ("subtree_end", "depth_positions", "depth_offsets"):
        assert np.array_equal(r[k].cpu().numpy().view(np.uint64), want[k]), k
    assert r["max_depth"] == want["max_depth"]


# ------------------------------------------------------------------ B. key hash zero ----
def _zero_set(n, where, skew, zero=True, fixed_extra=None):
    i = {"first": 0, "middle": n // 2 + 1, "last": n - 1}[where]
    fixed = {i: ZERO_KEY} if zero else {}
    fixed.update(fixed_extra or {})
    return _layout(n, [], skew, fixed=fixed)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("kernel", ["k_hash0_pair", "k_hash_skew", "k_hash_count0", "k_hash_count0_sorted"])
def test_zero_key_hash_each_level0_kernel(s3, ctx, oracle_lib, kernel, where):
    """One zero-hash key among 5000: each kernel that sets kStKeyZero (the aligned pair hash,
    the aligned skewed hash, the per-lane hash's plain loop and its sorted groups at a
    misaligned pointer) reports it; the oracle does; the context then builds the set with
    that key replaced."""
    skew = kernel in ("k_hash_skew", "k_hash_count0_sorted")
    shift = 1 if kernel.startswith("k_hash_count0") else 0
    blob, offs = _zero_set(5000, where, skew)
    assert oracle_lib.build(blob, offs)[0] == O.ORC_ERR_KEY_ZERO
    with pytest.raises(s3.MPHFError) as e:
        _build(ctx, blob, offs, shift=shift)
    assert e.value.status == s3.ERR_KEY_HASH_ZERO
    _on_reservation_path(ctx)
    blob, offs = _zero_set(5000, where, skew, zero=False)
    _check(ctx, oracle_lib.build(blob, offs), blob, offs, shift=shift)


@pytest.mark.parametrize("shift", [0, 1])
def test_zero_key_hash_single_key(s3, ctx, oracle_lib, shift):
    blob, offs = O.keys_to_blob([ZERO_KEY])
    assert not _skewed(offs)
    assert oracle_lib.build(blob, offs)[0] == O.ORC_ERR_KEY_ZERO
    with pytest.raises(s3.MPHFError) as e:
        _build(ctx, blob, offs, shift=shift)
    assert e.value.status == s3.ERR_KEY_HASH_ZERO
    _on_reservation_path(ctx)
    blob, offs = O.keys_to_blob([b"only/"])
    _check(ctx, oracle_lib.build(blob, offs), blob, offs, shift=shift)


def test_zero_key_hash_build_host(s3, oracle_lib):
    blob, offs = _zero_set(5000, "middle", False)
    with pytest.raises(s3.MPHFError) as e:
        s3.build_host(blob, offs)
    assert e.value.status == s3.ERR_KEY_HASH_ZERO
    blob, offs = _zero_set(5000, "middle", False, zero=False)
    _same(s3.build_host(blob, offs), oracle_lib.build(blob, offs))


def test_zero_key_hash_builder(s3, tmp_path):
    """StreamingMPHFBuilder.build fails with the zero-hash status and writes no file."""
    blob, offs = _zero_set(5000, "last", False)
    b = s3.StreamingMPHFBuilder(str(tmp_path))
    for i in range(len(offs) - 1):
        b.add(bytes(blob[int(offs[i]):int(offs[i + 1])]), i)
    out = tmp_path / "idx"
    out.mkdir()
    with pytest.raises(s3.MPHFError) as e:
        b.build(str(out))
    assert e.value.status == s3.ERR_KEY_HASH_ZERO
    assert list(out.iterdir()) == []
    b.close()


@pytest.mark.parametrize("flags", ["route", "bitmap"])
def test_zero_key_hash_two_ranks(s3, oracle_lib, flags):
    """Two ranks on one GPU, both decompositions: the zero-hash key lies on rank 1's shard
    (shards are cut by key bytes; it is the last key), the status flags are all-gathered,
    and the build fails with the zero-hash status; the cached rank contexts then build the
    clean set."""
    fl = s3.MULTI_BITMAP if flags == "bitmap" else 0
    blob, offs = _zero_set(5000, "last", False)
    with pytest.raises(s3.MPHFError) as e:
        s3.build_host(blob, offs, devices=[0, 0], flags=fl)
    assert e.value.status == s3.ERR_KEY_HASH_ZERO
    blob, offs = _zero_set(5000, "last", False, zero=False)
    _same(s3.build_host(blob, offs, devices=[0, 0], flags=fl), oracle_lib.build(blob, offs))


def test_zero_hash_keys_as_queries(s3, oracle_lib, tmp_path):
    """The three zero-hash keys as queries against an index that does not hold them:
    MPHF.lookup on the GPU answers what the oracle's Lookup answers (a key hash of 0 still
    probes the levels; the fingerprint rejects it)."""
    keys = [b"q/%05d/" % i for i in range(5000)]
    blob, offs = O.keys_to_blob(keys)
    fp, po, mph = s3.build_host(blob, offs)
    s3.write_index_files(str(tmp_path), mph, fp, po, blob, offs)
    st, m = oracle_lib.unmarshal(mph)
    assert st == 0
    queries = ZERO_KEYS + keys[:300] + [b"absent/%d" % i for i in range(300)]
    want = [oracle_lib.lookup(m, fp, po, k) for k in queries]
    assert want[:3] == [None] * 3
    want = np.array([NOT_FOUND if w is None else w for w in want], np.uint64)
    h = s3.MPHF(str(tmp_path))
    try:
        assert np.array_equal(h.lookup(queries), want)
    finally:
        h.close()


@pytest.mark.parametrize("case", ["aligned", "misaligned", "skewed", "zero_twice"])
def test_duplicates_take_precedence_over_zero_key_hash(s3, ctx, oracle_lib, case):
    """A set with a zero-hash key AND a duplicate pair is DUP_KEY_HASH on the GPU, as the
    reference fails in bbhash.New (mphf_streaming.go:141-144) before its Key() == 0 loop
    (:248-252); the oracle reports its duplicate status too.  zero_twice: the duplicate is
    the zero-hash key itself."""
    extra = {4000: ZERO_KEY} if case == "zero_twice" else {4000: b"dup/key/", 77: b"dup/key/"}
    blob, offs = _zero_set(5000, "middle", case == "skewed", fixed_extra=extra)
    assert oracle_lib.build(blob, offs)[0] == O.ORC_ERR_TOO_MANY_LEVELS
    assert oracle_lib.build_mt(blob, offs, threads=4)[0] == O.ORC_ERR_TOO_MANY_LEVELS
    with pytest.raises(s3.MPHFError) as e:
        _build(ctx, blob, offs, shift=1 if case == "misaligned" else 0)
    assert e.value.status == s3.ERR_DUP_KEY_HASH
    with pytest.raises(s3.MPHFError) as e:
        s3.build_host(blob, offs)
    assert e.value.status == s3.ERR_DUP_KEY_HASH


# ------------------------------------ C. window and round edges of the aligned hashes ----
# k_hash0_pair: 4096 blocks of ceil(n / 4096) consecutive keys, rounds of up to 512 keys whose
# bytes lie in the 32 KiB window that starts at the round's first key rounded down to 16 B.
# n = 65536: 16 keys per block, samples at multiples of 64, so a run at i = 16 (mod 64) starts
# a block and stays off the sampled indices.
W = 32768
N_PAIR = 65536
# k_hash_skew: 256 blocks; 65 keys each at n = 256 x 65 (batches of 64 + 1).
N_SKEW = 256 * 65


def _runs(n, step):
    """The edge runs, each at the start of its own hash block, spread over the set: index
    64 k + 16 at n = 65536 (step 16), 65 k at n = 256 x 65 (step 65)."""
    starts = iter([64 * (3 + 50 * j) + 16 for j in range(20)] if step == 16 else
                  [65 * (2 + 12 * j) for j in range(20)])

    def block():
        i0 = next(starts)
        assert i0 % step == 0 and i0 + 16 <= n - 16
        return i0

    runs = {
        # a key of exactly the window: fits when 16-byte aligned (len << 16 = 2^31), else alone
        "w32768_res0": [(block(), [W], 0), (block() + 5, [W], 0)],
        "w32768_res1_res15": [(block(), [W], 1), (block(), [W], 15)],
        "w32767": [(block(), [W - 1], 0), (block(), [W - 1], 1), (block(), [W - 1], 2)],
        "w32769": [(block(), [W + 1], 0), (block(), [W + 1], 15)],
        # 16 x 2300 B cross the window once: the keys past it wait for the next round;
        # the second run ends the blob
        "cross_2300": [(block(), [2300] * 16, 3), (n - 16, [2300] * 16, None)],
        # 5 + 7 x 4096 + 4091 = 32768: a key ending exactly at wlo + 32768, the next past it
        "end_at_window": [(block(), [4096] * 7 + [4091] + [100] * 8, 5)],
        # the 256 length classes clamp at 255; k_hash_skew's 4-byte classes clamp at 1020
        "classes": [(block(), [0, 1, 254, 255, 256, 257, 1019, 1020, 4096, 2, 3, 4, 1021, 1023, 1024, 5], 7)],
        # a partial round (one key), an alone round (40000 B from global memory), the rest
        "second_key_40000": [(block(), [24, 40000] + [30] * 14, 9)],
        # k_hash_skew's 64-byte chunk steps
        "chunk_steps": [(block(), [63, 64, 65, 127, 128, 129], 0), (block(), [63, 64, 65, 127, 128, 129], 15),
                        (block(), [129, 128, 127, 65, 64, 63], 8)],
    }
    return runs


@functools.lru_cache(maxsize=None)
def _edge_set(n, name, skew):
    step = 16 if n == N_PAIR else 65
    runs = _runs(n, step)[name]
    if n == N_PAIR and not skew:
        for i0, ls, _ in runs:
            assert i0 % 16 == 0 or name == "w32768_res0"
            assert not _sample_indices(n) & set(range(i0 - 1, i0 + len(ls)))
    blob, offs = _layout(n, runs, skew)
    return blob, offs, O.lib().build(blob, offs)


EDGE_NAMES = list(_runs(N_PAIR, 16))


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_pair_hash_window_edges(s3, ctx, oracle_lib, name):
    """k_hash0_pair (aligned pointer, near-uniform samples) over each crafted run."""
    blob, offs, want = _edge_set(N_PAIR, name, False)
    _check(ctx, want, blob, offs)


@pytest.mark.parametrize("n", [N_PAIR, N_SKEW])
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_skew_hash_window_edges(s3, ctx, oracle_lib, name, n):
    """The same runs in a set made skewed (one 6000 B key on a sampled index): k_hash_skew's
    sorted groups, 64-key batches (256 or 64 + 1 keys per block) and 64-byte chunk steps."""
    blob, offs, want = _edge_set(n, name, True)
    _check(ctx, want, blob, offs)


@pytest.mark.parametrize("shift", [1, 15])
@pytest.mark.parametrize("skew", [False, True], ids=["plain", "sorted"])
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_per_lane_hash_edge_layouts(s3, ctx, oracle_lib, name, skew, shift):
    """The same layouts at a misaligned pointer: k_hash_count0's plain loop (fnv_both_pf over
    keys of up to 40000 B), and, in the skewed set, its 1024-key groups — sorted where a
    group holds a long key (4-byte length classes, clamped at 1020), unsorted ("not skewed")
    everywhere else."""
    blob, offs, want = _edge_set(N_PAIR, name, skew)
    _check(ctx, want, blob, offs, shift=shift)


def test_blob_end_sweep(s3, ctx, oracle_lib):
    """tail8 / end8 in both aligned hashes: sets of 1-40 keys whose blob ends at every
    residue mod 16, behind offsets[0] in {0, 1, 8, 15}; once near-uniform (k_hash0_pair),
    once with one ~200 B key among 4 B keys (k_hash_skew), 128 builds."""
    for r in range(16):
        for k, o0 in enumerate((0, 1, 8, 15)):
            n = 1 + (4 * r + 7 * k) % 40
            ln = 4 + np.arange(n) % 5
            ln[-1] += (r - (o0 + int(ln.sum()))) % 16
            blob, offs = _make(ln, o0)
            assert int(offs[-1]) % 16 == r and not _skewed(offs)
            _check(ctx, oracle_lib.build(blob, offs), blob, offs)
            n = 3 + (4 * r + 7 * k) % 38
            ln = np.full(n, 4)
            ln[(r + k) % n] = 200
            ln[(r + k) % n] += (r - (o0 + int(ln.sum()))) % 16
            blob, offs = _make(ln, o0)
            assert int(offs[-1]) % 16 == r and _skewed(offs)
            _check(ctx, oracle_lib.build(blob, offs), blob, offs)


# ------------------------------------------------------------ D. P0 at small shapes ----
# (n, gen_keys kind, avg): 33 full 2^14-position tiles; a 34th of 64 positions; 130 tiles in
# 9 super-tiles of 15 (the last one ragged); a skewed set (k_hash_skew's regions).
P0_CASES = [(8192 * 33, 0, 20), (8192 * 33 + 32, 0, 20), (1056801, 0, 20), (400000, 1, 0)]
P0_ENV = {"S3IMPH_DEV": "1", "S3IMPH_P0_MIN_TILES": "16", "S3IMPH_P0_TPS": "16"}

_P0_CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r]
import numpy as np, torch, s3imph, oracle as O
out = []
ctx = s3imph.DeviceBuilder(0)
ctx.set_profiling(1)
for n, kind, avg in %r:
    blob, offs = s3imph.gen_keys(kind, 19, avg, 0, n)
    blob = blob[: int(offs[-1])]
    st, fp, po, mph = O.lib().build_mt(blob, offs, None, threads=16)
    assert st == 0
    d_offs = torch.from_numpy(offs.view(np.int64)).to('cuda')
    for shift in (0, 1):
        buf = torch.zeros(shift + (len(blob) + 7) // 8 * 8 + 16, dtype=torch.uint8, device='cuda')
        buf[shift:shift + len(blob)] = torch.from_numpy(blob).to('cuda')
        view = buf[shift:]
        assert buf.data_ptr() %% 16 == 0 and view.data_ptr() %% 16 == shift
        for b in range(2):
            d_fp = torch.zeros(n, dtype=torch.int64, device='cuda')
            d_po = torch.zeros(n, dtype=torch.int64, device='cuda')
            ctx.build(view, d_offs, n, d_fp, d_po)
            out.append({'n': n, 'shift': shift, 'build': b, 'ptr16': view.data_ptr() %% 16,
                        'stages': sorted(ctx.stage_times()), 'mph': ctx.mph_bin() == mph,
                        'fp': bool(np.array_equal(d_fp.cpu().numpy().view(np.uint64), fp)),
                        'po': bool(np.array_equal(d_po.cpu().numpy().view(np.uint64), po))})
ctx.close()
print('RESULT ' + json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def _p0_child():
    """Every P0 case in ONE fresh process (the library reads its knobs once per process):
    each set at an aligned pointer and at shift 1, two builds each; a record per build."""
    root = os.path.join(os.path.dirname(GOLDEN), "..")
    code = _P0_CHILD % (os.path.join(root, "s3-inv-db_amd"), os.path.join(root, "oracle"), P0_CASES)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=280,
                       env={**os.environ, **P0_ENV})
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    assert r.returncode == 0 and lines, r.stderr[-2000:]
    return json.loads(lines[-1][7:])


@pytest.mark.parametrize("shift", [0, 1], ids=["fused", "unfused"])
@pytest.mark.parametrize("n,kind,avg", P0_CASES)
def test_p0_small_shapes(s3, oracle_lib, n, kind, avg, shift):
    """P0 at 33 / 34 / 130 tiles (S3IMPH_P0_MIN_TILES=16, S3IMPH_P0_TPS=16: 3 / 3 / 9
    super-tiles of 11 / 12 / 15 tiles) and on a skewed 400000-key set (49 tiles): the fused
    hash (k_hash0_pair<.., PT> or k_hash_skew's partition form) at an aligned pointer, and at
    shift 1 k_hash_count0 then the partition pass (launch_p0_partition, only_skew = false).
    Both builds bit-exact vs the oracle, and the last attempt is P0's (no conservative rerun)."""
    recs = [r for r in _p0_child() if r["n"] == n and r["shift"] == shift]
    assert [r["build"] for r in recs] == [0, 1]
    for r in recs:
        assert r["ptr16"] == shift
        assert r["mph"] and r["fp"] and r["po"], r
        assert "scatter0_p0" in r["stages"], r
