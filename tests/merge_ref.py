"""The run merge restated for the tests (no GPU): pkg/extsort's MergeIterator.Next
(merger.go:104-140) with PrefixRow.Merge (types.go:82-91), and a dict fold as a second opinion.

A row is (prefix bytes, depth, count, bytes, tier_counts[12], tier_bytes[12]) — the rows of
tiers_ref.aggregate_dict_tiers; a run is a list of rows in non-decreasing byte order.  Sums wrap
mod 2^64.  Among rows with equal prefixes the reference keeps the depth of whichever its heap pops
first, which is unspecified; here, as in the library, the heap is ordered by (prefix, run, row), so
the lowest run wins, and in a tie the lowest row."""
import heapq
import json
import os

import numpy as np

M64 = (1 << 64) - 1
NUM_TIERS = 12


def row(prefix, depth=0, count=0, nbytes=0, tiers=None):
    """A row from a prefix and {tier id: (count, bytes)}."""
    tc, tb = [0] * NUM_TIERS, [0] * NUM_TIERS
    for t, (c, b) in (tiers or {}).items():
        tc[int(t)], tb[int(t)] = int(c), int(b)
    p = prefix.encode("latin-1") if isinstance(prefix, str) else bytes(prefix)
    return (p, int(depth), int(count), int(nbytes), tc, tb)


def _merge_into(acc, r):
    """PrefixRow.Merge (types.go:82-91): Count, TotalBytes and both tier arrays are summed."""
    acc[2] = (acc[2] + r[2]) & M64
    acc[3] = (acc[3] + r[3]) & M64
    for t in range(NUM_TIERS):
        acc[4][t] = (acc[4][t] + r[4][t]) & M64
        acc[5][t] = (acc[5][t] + r[5][t]) & M64


def merge_heap(runs):
    """MergeIterator.Next until EOF (merger.go:104-140): pop the smallest, then fold every row
    with an equal prefix into it (:125-137) — equal neighbours inside one run included."""
    heap = [(run[0][0], r, 0) for r, run in enumerate(runs) if run]
    heapq.heapify(heap)
    out = []

    def pop():
        prefix, r, i = heapq.heappop(heap)
        if i + 1 < len(runs[r]):
            heapq.heappush(heap, (runs[r][i + 1][0], r, i + 1))
        return runs[r][i]

    while heap:
        first = pop()
        acc = [first[0], first[1], first[2] & M64, first[3] & M64, list(first[4]), list(first[5])]
        while heap and heap[0][0] == acc[0]:
            _merge_into(acc, pop())
        out.append(tuple(acc))
    return out


def merge_dict(runs):
    """The second opinion: every row folded into a dict in (run, row) order, then sorted."""
    rows = {}
    for run in runs:
        for r in run:
            acc = rows.get(r[0])
            if acc is None:
                rows[r[0]] = [r[0], r[1], r[2] & M64, r[3] & M64, list(r[4]), list(r[5])]
            else:
                _merge_into(acc, r)
    return [tuple(rows[p]) for p in sorted(rows)]


def first_unsorted(runs):
    """The global index (into the runs' concatenation) of the first row smaller than its
    predecessor in the same run; None when every run is sorted."""
    base = 0
    for run in runs:
        for i in range(1, len(run)):
            if run[i][0] < run[i - 1][0]:
                return base + i
        base += len(run)
    return None


def present_mask(rows):
    """Bit t set iff some row has tier_count[t] | tier_bytes[t] != 0 (indexbuild.go:192-196)."""
    mask = 0
    for r in rows:
        for t in range(NUM_TIERS):
            if r[4][t] | r[5][t]:
                mask |= 1 << t
    return mask


def to_arrays(rows):
    """Rows -> (blob u8, offsets u64[n + 1], depth u32, count u64, bytes u64, tier_count (12, n),
    tier_bytes (12, n))."""
    n = len(rows)
    offs = np.zeros(n + 1, np.uint64)
    if n:
        offs[1:] = np.cumsum([len(r[0]) for r in rows], dtype=np.uint64)
    blob = np.frombuffer(b"".join(r[0] for r in rows), np.uint8).copy()
    tc, tb = np.zeros((NUM_TIERS, n), np.uint64), np.zeros((NUM_TIERS, n), np.uint64)
    for i, r in enumerate(rows):
        tc[:, i] = r[4]
        tb[:, i] = r[5]
    return (blob, offs, np.array([r[1] for r in rows], np.uint32), np.array([r[2] for r in rows], np.uint64),
            np.array([r[3] for r in rows], np.uint64), tc, tb)


def from_arrays(blob, offs, depth, count, nbytes, tc=None, tb=None):
    n = len(offs) - 1
    raw = bytes(np.asarray(blob, np.uint8))
    zero = [0] * NUM_TIERS
    return [(raw[int(offs[i]):int(offs[i + 1])], int(depth[i]), int(count[i]), int(nbytes[i]),
             zero[:] if tc is None else [int(v) for v in tc[:, i]],
             zero[:] if tb is None else [int(v) for v in tb[:, i]]) for i in range(n)]


def golden_cases():
    """tests/golden/merge/cases.json as [(name, with tiers, runs, expected rows)]."""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge", "cases.json")
    out = []
    for c in json.load(open(path))["cases"]:
        runs = [[row(*r) for r in run] for run in c["runs"]]
        out.append((c["name"], bool(c["tiers"]), runs, [row(*r) for r in c["expected"]]))
    return out
