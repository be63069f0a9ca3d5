"""Key sets that cut, fill or exceed the 32 KiB staging window of k_fin_keys_lds
(s3imph_finalize.hip), and whose expected values move when an lcp is off by a byte or a
'/' count leaks past a key's end.  Generated, byte-sorted, distinct; no GPU, no library.

tests/test_finalize_regimes.py states on the CPU which window regime each set reaches
(finalize_regimes.walk); tests/test_gpu_finalize_keys.py runs the same bytes on the GPU.
"""
import functools

import numpy as np

ALPHABET = np.frombuffer(b"./01", np.uint8)


def _sorted_distinct(keys):
    out = sorted(keys)
    assert all(a != b for a, b in zip(out, out[1:])), "keys must be distinct"
    return out


def _comb_spine(J, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(0x30, 0x7A, J, dtype=np.uint8)
    s[rng.random(J) < 0.1] = 0x2F
    return s.tobytes()


def comb(J=600, flip=False, seed=11):
    """Every prefix S[:j], j = 0..J, of one random J-byte string (a tenth of it '/'), and per
    j < J one key that leaves S at byte j: S[:j] + (S[j] + 1), or S[:j] + (S[j] ^ 0x80) with
    `flip`.  S[:j+1]'s subtree ends just before the key that diverges at j, so each of the
    J + 1 prefixes has its own subtree_end and an lcp wrong by one byte, at any byte phase,
    changes an answer."""
    s = _comb_spine(J, seed)
    keys = [s[:j] for j in range(J + 1)]
    keys += [s[:j] + bytes([s[j] ^ 0x80 if flip else s[j] + 1]) for j in range(J)]
    return _sorted_distinct(keys)


def comb_cut(n, seed=11):
    """A comb of exactly n keys: J = n // 2, without its last key when n is even."""
    return comb(n // 2, seed=seed)[:n]


def mask_leak():
    """"/" * k and "!" * k for k = 1..300: every key end of the '/' keys lies among '/' bytes,
    and the longest '!' key is followed by them, so depth == len (or 0) fails on a count that
    leaks past a key's end or stops a byte short."""
    return _sorted_distinct([b"/" * k for k in range(1, 301)] + [b"!" * k for k in range(1, 301)])


def slash_sweep():
    """Every length 1..64 with a single '/' at every position of it."""
    return _sorted_distinct([b"a" * p + b"/" + b"a" * (L - p - 1) for L in range(1, 65) for p in range(L)])


def ragged(n=6000, seed=23):
    """n distinct keys, lengths log-uniform in 1..1024, over the alphabet . / 0 1."""
    rng = np.random.default_rng(seed)
    keys = set()
    while len(keys) < n:
        L = min(1024, int(np.exp(rng.uniform(0.0, np.log(1025.0)))))
        keys.add(ALPHABET[rng.integers(0, 4, L)].tobytes())
    return _sorted_distinct(keys)


def exact_fit(extra=False, slash_last=False):
    """40 keys of exactly 1024 bytes sharing 1000: the 32nd ends at byte 32768, the window's
    last byte; behind one extra key b"c" it ends at 32769 and no longer fits.  With
    `slash_last` each key's last byte is a '/', so a key taken from the window with its last
    byte outside it loses one from its depth."""
    tail = b"x" * 20 + b"/" if slash_last else b"x" * 21
    keys = [b"d/" * 500 + b"%02d/" % i + tail for i in range(40)]
    assert all(len(k) == 1024 for k in keys)
    return _sorted_distinct(([b"c"] if extra else []) + keys)


def _big():
    return ALPHABET[np.random.default_rng(31).integers(0, 4, 70_000)].tobytes()


def oversize_first():
    """A 40 000-byte key, then 300 short ones."""
    return _sorted_distinct([_big()[:40_000]] + [b"s%03d/" % i for i in range(300)])


def oversize_last():
    """300 short keys, then the 40 000-byte key as the last of the set (lcp = -1)."""
    return _sorted_distinct([b"!%03d/" % i for i in range(300)] + [_big()[:40_000]])


NESTED_LENGTHS = (5, 32768, 32769, 40_000, 70_000)


def oversize_nested():
    """b"n/" + big[:L] for L in NESTED_LENGTHS between two runs of 300 short keys: each long
    key is the parent of the next, with lcps far longer than the window."""
    big = _big()
    return _sorted_distinct([b"a%03d/" % i for i in range(300)] + [b"n/" + big[:L] for L in NESTED_LENGTHS]
                            + [b"z%03d/" % i for i in range(300)])


def short_tree(n=3000):
    """n short keys, a third of them parents of the next two."""
    assert n % 3 == 0
    keys = []
    for i in range(n // 3):
        keys += [b"p%03d/" % i, b"p%03d/a/" % i, b"p%03d/b/" % i]
    return _sorted_distinct(keys)


def hashed_depths(n):
    """The caller depths test_gpu_finalize.py uses: i * 2654435761 % 23."""
    return (np.arange(n, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(23)).astype(np.uint32)


def true_depths(keys):
    return np.array([k.count(b"/") for k in keys], np.uint32)


def edge_depths(n, placed):
    """0 everywhere but depth d at position p for (p, d) in `placed`."""
    d = np.zeros(n, np.uint32)
    for p, v in placed:
        d[p] = v
    return d


# depth-index edges: one depth on one key of short_tree(); the position is neither first nor
# last unless stated, so k_fin_doff meets the gap in the middle of the sorted order's tail
EDGE_DEPTHS = (62, 63, 64, 255, 256, 65535, 70_000)
BLOCK_EDGE_N = (1, 2, 3, 4, 5, 1023, 1024, 1025, 2047, 2049)

# name -> (generator, coverage condition on finalize_regimes.walk's counts, or None)
SETS = {
    "comb": (comb, lambda w: w["cut"] >= 5),
    "comb_flip": (functools.partial(comb, flip=True), lambda w: w["cut"] >= 5),
    "mask_leak": (mask_leak, None),
    "slash_sweep": (slash_sweep, None),
    "ragged": (ragged, lambda w: w["cut"] >= 10),
    "exact_fit": (exact_fit, lambda w: w["exact"] == 1),
    "exact_fit_plus1": (functools.partial(exact_fit, extra=True), lambda w: w["exact"] == 0 and w["cut"] >= 1),
    "exact_fit_slash": (functools.partial(exact_fit, slash_last=True), lambda w: w["exact"] == 1),
    "exact_fit_slash_plus1": (functools.partial(exact_fit, extra=True, slash_last=True),
                              lambda w: w["exact"] == 0 and w["cut"] >= 1),
    "oversize_first": (oversize_first, lambda w: w["oversize"] >= 1),
    "oversize_last": (oversize_last, lambda w: w["oversize"] >= 1),
    "oversize_nested": (oversize_nested, lambda w: w["oversize"] == 4),
}


@functools.lru_cache(maxsize=None)
def keyset(name):
    """The sorted keys of SETS[name] (generated once per process; treat as read-only)."""
    return tuple(SETS[name][0]())


def blob_of(keys):
    """(blob u8, offsets u64[n + 1]) of the keys, prefix_blob.bin / prefix_offsets.u64 layout."""
    offs = np.zeros(len(keys) + 1, np.uint64)
    if keys:
        offs[1:] = np.cumsum([len(k) for k in keys], dtype=np.uint64)
    return np.frombuffer(b"".join(keys), np.uint8).copy(), offs
