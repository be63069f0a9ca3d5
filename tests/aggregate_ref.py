"""The prefix aggregation restated for the tests (no GPU):

  aggregate_dict   AddObject / Drain / SortPrefixRows of pkg/extsort/aggregator.go:44-76, :138-,
                   as a dict keyed by prefix bytes — the reference's own data structure;
  aggregate_numpy  the sorted-input formulation of DESIGN.md §4.5b in numpy, for inputs too
                   large for the dict.

Both take byte-sorted keys with one u64 size each and return the rows in byte order:
(prefix_blob u8, prefix_offsets u64[n + 1], depth u32[n], object_count u64[n],
total_bytes u64[n]).  Sums wrap mod 2^64 like Go's uint64 +=."""
import numpy as np

M64 = (1 << 64) - 1


def aggregate_dict(keys, sizes, max_depth=0):
    """Rows [(prefix bytes, depth, count, bytes)] in byte order; [] for no objects."""
    rows = {}

    def accumulate(prefix, depth, size):
        st = rows.get(prefix)
        if st is None:
            st = rows[prefix] = [depth, 0, 0]
        st[1] += 1
        st[2] = (st[2] + size) & M64

    for key, size in zip(keys, sizes):
        key, size = bytes(key), int(size)
        accumulate(b"", 0, size)
        depth = 1
        for i, ch in enumerate(key):
            if ch == 0x2F:
                if max_depth > 0 and depth > max_depth:
                    break
                accumulate(key[:i + 1], depth, size)
                depth += 1
    return [(p, st[0], st[1], st[2]) for p, st in sorted(rows.items())]


def rows_to_arrays(rows):
    """aggregate_dict's rows in the arrays' form."""
    n = len(rows)
    offs = np.zeros(n + 1, np.uint64)
    if n:
        offs[1:] = np.cumsum([len(r[0]) for r in rows], dtype=np.uint64)
    blob = np.frombuffer(b"".join(r[0] for r in rows), np.uint8).copy()
    return (blob, offs, np.array([r[1] for r in rows], np.uint32), np.array([r[2] for r in rows], np.uint64),
            np.array([r[3] for r in rows], np.uint64))


def keys_of(blob, offs):
    raw = np.asarray(blob, np.uint8).tobytes()
    return [raw[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]


def aggregate_numpy(blob, offs, sizes, max_depth=0):
    """The formulation: s = '/' per key, c = '/' inside the common prefix with the predecessor;
    key i opens depths c'+1 .. s'; row (i, d) ends at e = first index > i with c[e] < d."""
    blob = np.asarray(blob, np.uint8)
    offs = np.asarray(offs, np.uint64).astype(np.int64)
    m = len(offs) - 1
    if m == 0:
        return (np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64),
                np.zeros(0, np.uint64))
    sizes = np.zeros(m, np.uint64) if sizes is None else np.asarray(sizes, np.uint64)
    lens = np.diff(offs)
    width = int(lens.max()) if m else 0
    # keys as rows of a matrix, padded with 256 (equal past both ends: the lcp is cut at the lengths)
    mat = np.full((m, width + 1), 256, np.int16)
    col = np.arange(offs[0], offs[m]) - np.repeat(offs[:-1], lens)
    mat[np.repeat(np.arange(m), lens), col] = blob[offs[0]:offs[m]]
    slash = np.zeros((m, width + 2), np.int32)
    np.cumsum(mat == 0x2F, axis=1, out=slash[:, 1:])  # slash[i, j] = '/' in key i before byte j
    s = slash[:, -1].astype(np.int64)
    c = np.zeros(m, np.int64)
    if m > 1:
        ne = mat[1:] != mat[:-1]
        first = np.where(ne.any(axis=1), ne.argmax(axis=1), width + 1)
        lcp = np.minimum(first, np.minimum(lens[1:], lens[:-1]))
        c[1:] = slash[np.arange(1, m), lcp]
    if max_depth > 0:
        sc, cc = np.minimum(s, max_depth), np.minimum(c, max_depth)
    else:
        sc, cc = s, c
    per = sc - cc
    n = 1 + int(per.sum())
    key = np.repeat(np.arange(m), per)                       # the key of each non-root row
    first_row = np.concatenate(([0], np.cumsum(per)))[:-1]   # ... its rows start here (root excluded)
    d = cc[key] + 1 + (np.arange(n - 1) - first_row[key])
    # the d-th '/' of the key: all '/' positions in key order
    spos = np.flatnonzero(blob[offs[0]:offs[m]] == 0x2F) + offs[0]
    s0 = np.concatenate(([0], np.cumsum(s)))[:-1]
    plen = spos[s0[key] + d - 1] - offs[key] + 1
    e = np.full(n - 1, m, np.int64)
    for dv in np.unique(d):
        below = np.flatnonzero(c < dv)
        sel = np.flatnonzero(d == dv)
        j = np.searchsorted(below, key[sel], side="right")
        ok = j < len(below)
        e[sel[ok]] = below[j[ok]]
    z = np.concatenate((np.zeros(1, np.uint64), np.cumsum(sizes, dtype=np.uint64)))
    depth = np.concatenate(([0], d)).astype(np.uint32)
    count = np.concatenate(([m], e - key)).astype(np.uint64)
    total = np.concatenate((z[m:m + 1], z[e] - z[key]))
    out_offs = np.zeros(n + 1, np.uint64)
    out_offs[2:] = np.cumsum(plen, dtype=np.uint64)
    src = np.repeat(offs[key] - out_offs[1:-1].astype(np.int64), plen) + np.arange(int(out_offs[-1]))
    return blob[src], out_offs, depth, count, total
