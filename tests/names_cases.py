"""Key sets, handles and the numpy restatements for the prefix-blob queries of the GPU reader
(tests/test_gpu_names.py, test_gpu_lookup_verify.py, test_gpu_verify.py, test_gpu_names_streams.py).

The restatements are slices of (blob, offsets): PrefixString is blob[offsets[p]:offsets[p + 1]]
(BlobReader.Get, reader.go:250-270), LookupWithVerify is Lookup masked by byte equality with that
slice (mphf.go:312-317), VerifyMPHF compares Lookup(prefix i) with i (mphf.go:372-393)."""
import json
import os

import numpy as np

import oracle as O
from conftest import GOLDEN

NOT_FOUND = 2**64 - 1
EDGE_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 1024, 2500)


def edge_keys(n_fill=5000, seed=7):
    """~n_fill byte-sorted distinct keys, among them one of every EDGE_LENGTHS length: the
    lengths around the emit's 8-byte word, one key of half an output chunk (1024) and one longer
    than a chunk (2500 > 2048)."""
    rng = np.random.default_rng(seed)
    keys = {b""}
    for c, ln in zip(b"ABCDEFGHI", EDGE_LENGTHS[1:]):
        body = bytes(rng.integers(97, 123, ln - 1, dtype=np.uint8)) if ln > 1 else b""
        keys.add(bytes([c]) + body)
    for i in range(n_fill):
        tail = bytes(rng.integers(97, 123, int(rng.integers(0, 30)), dtype=np.uint8))
        keys.add(b"k%04d/" % i + tail + b"/")
    keys = sorted(keys)
    assert {len(k) for k in keys} >= set(EDGE_LENGTHS)
    return keys


def by_length(keys):
    """Index of the one key of each edge length."""
    at = {}
    for ln in EDGE_LENGTHS:
        hits = [i for i, k in enumerate(keys) if len(k) == ln and (ln == 0 or k[0:1].isupper())]
        assert len(hits) == 1, ln
        at[ln] = hits[0]
    return at


def want_names(blob, offs, pos):
    """(out_offsets u64[nq + 1], found u32[nq], out bytes padded with zeros to a whole word)."""
    pos = np.asarray(pos, np.uint64).reshape(-1)
    n = len(offs) - 1
    ok = pos < np.uint64(n)
    p = np.where(ok, pos, 0).astype(np.int64)
    lens = np.where(ok, offs[p + 1] - offs[p], 0).astype(np.uint64) if n else np.zeros(len(pos), np.uint64)
    out_offs = np.concatenate([np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64)])
    raw = b"".join(blob[int(offs[q]):int(offs[q + 1])].tobytes() for q, k in zip(p, ok) if k)
    assert len(raw) == int(out_offs[-1])
    return out_offs, ok.astype(np.uint32), np.frombuffer(raw + b"\0" * (-len(raw) % 8), np.uint8)


def check_names(idx, blob, offs, pos, what, out=None):
    """prefixes_plan + prefixes_fill against want_names, offset for offset and byte for byte."""
    w_offs, w_found, w_bytes = want_names(blob, offs, pos)
    g_offs, g_found, total = idx.prefixes_plan(pos)
    assert total == int(w_offs[-1]), what
    assert np.array_equal(g_offs.cpu().numpy().view(np.uint64), w_offs), what
    assert np.array_equal(g_found.cpu().numpy().view(np.uint32), w_found), what
    got = idx.prefixes_fill(total, out=out)
    assert int(got.numel()) >= len(w_bytes), what
    g = got.cpu().numpy()[:len(w_bytes)]
    if g.tobytes() != w_bytes.tobytes():
        at = int(np.flatnonzero(g != w_bytes)[0])
        raise AssertionError(f"{what}: byte {at} of {len(w_bytes)} is {g[at]}, want {w_bytes[at]}")
    return g_offs, g_found, got, total


def dev(a):
    """numpy -> cuda tensor (u64 / u32 as their signed bits)."""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to("cuda")


def padded(blob):
    """A blob readable up to its length rounded up to 8 bytes, and a word beyond."""
    out = np.zeros((len(blob) + 7) // 8 * 8 + 8, np.uint8)
    out[:len(blob)] = blob
    return out


def flat_arrays(n):
    """Finalize arrays of n nodes that are all roots at depth 0: enough for s3imph_index_attach,
    which the prefix-blob queries never read."""
    return dict(depth=np.zeros(max(n, 1), np.uint32), subtree_end=np.arange(max(n, 1), dtype=np.uint64),
                max_depth_in_subtree=np.zeros(max(n, 1), np.uint32), depth_offsets=np.array([0, n], np.uint64),
                depth_positions=np.arange(max(n, 1), dtype=np.uint64))


def attached(s3, mph, fp, pos, blob=None, offs=None):
    """An attached handle (Index.from_arrays) over an MPHF's arrays, with (blob, offs) as its
    stored prefixes when given."""
    n = len(fp)
    a = flat_arrays(n)
    pad = lambda v: v if len(v) else np.zeros(1, v.dtype)
    idx = s3.Index.from_arrays(mph, dev(pad(np.asarray(fp, np.uint64)))[:n], dev(pad(np.asarray(pos, np.uint64)))[:n],
                               dev(a["depth"]), dev(a["subtree_end"]), dev(a["max_depth_in_subtree"]),
                               dev(a["depth_offsets"]), dev(a["depth_positions"]), max_depth=0)
    if blob is not None:
        idx.attach_prefixes(dev(padded(blob)), dev(offs))
    return idx


def golden_set(name):
    """A key set of the reference's own tests with its MPHF (tests/golden/<name>.json): keys in
    Add order (key i was added with pos i), mph.bin, mph_fp, mph_pos."""
    fx = json.load(open(os.path.join(GOLDEN, name + ".json")))
    keys = [k.encode() for k in fx["keys"]]
    return keys, bytes.fromhex(fx["mph_bin_hex"]), np.array(fx["fp_out"], np.uint64), np.array(fx["pos_out"], np.uint64)


def golden_index(s3, name):
    keys, mph, fp, pos = golden_set(name)
    blob, offs = O.keys_to_blob(keys)
    return keys, attached(s3, mph, fp, pos, blob, offs)
