"""The per-tier statistics restated for the tests (no GPU), on top of tests/aggregate_ref.py:

  aggregate_dict_tiers   AddObject(key, size, tierID) / PrefixStats.Add (pkg/extsort/aggregator.go:44-76,
                         types.go:200-205) as a dict keyed by prefix bytes, with the two 12-wide arrays;
  tier_columns_numpy     the same columns for inputs too large for the dict, from aggregate_numpy with
                         sizes = (tier == t) for the counts and sizes * (tier == t) for the bytes;
  tiers_json             tiers.json as json.MarshalIndent(TierManifest, "", "  ") writes it (tiers.go:126-150);
  get_breakdown[_all]    TierStatsReader.GetBreakdown / GetBreakdownAll (pkg/format/tierstats.go:157-215).

Tier columns are (12, n) u64 arrays, row t = the tier's value for every prefix row; sums wrap mod 2^64."""
import numpy as np

import aggregate_ref as R

M64 = R.M64
NUM_TIERS = 12
# tiers.AllTiers (pkg/tiers/tiers.go:39-53): id -> (name, file prefix)
TIER_TABLE = [
    ("STANDARD", "standard"), ("STANDARD_IA", "standard_ia"), ("ONEZONE_IA", "onezone_ia"),
    ("GLACIER_IR", "glacier_ir"), ("GLACIER", "glacier_fr"), ("DEEP_ARCHIVE", "deep_archive"),
    ("REDUCED_REDUNDANCY", "reduced_redundancy"), ("INTELLIGENT_TIERING_FREQUENT", "it_frequent"),
    ("INTELLIGENT_TIERING_INFREQUENT", "it_infrequent"),
    ("INTELLIGENT_TIERING_ARCHIVE_INSTANT", "it_archive_instant"),
    ("INTELLIGENT_TIERING_ARCHIVE", "it_archive"), ("INTELLIGENT_TIERING_DEEP_ARCHIVE", "it_deep_archive"),
]


def aggregate_dict_tiers(keys, sizes, tiers, max_depth=0):
    """Rows [(prefix bytes, depth, count, bytes, tier_counts[12], tier_bytes[12])] in byte order."""
    rows = {}

    def accumulate(prefix, depth, size, tier):
        st = rows.get(prefix)
        if st is None:
            st = rows[prefix] = [depth, 0, 0, [0] * NUM_TIERS, [0] * NUM_TIERS]
        st[1] += 1
        st[2] = (st[2] + size) & M64
        st[3][tier] += 1                          # a tier id >= 12 raises, as Go's index panics
        st[4][tier] = (st[4][tier] + size) & M64

    for key, size, tier in zip(keys, sizes, tiers):
        key, size, tier = bytes(key), int(size), int(tier)
        accumulate(b"", 0, size, tier)
        depth = 1
        for i, ch in enumerate(key):
            if ch == 0x2F:
                if max_depth > 0 and depth > max_depth:
                    break
                accumulate(key[:i + 1], depth, size, tier)
                depth += 1
    return [(p, st[0], st[1], st[2], st[3], st[4]) for p, st in sorted(rows.items())]


def tier_arrays(rows):
    """(tier_count, tier_bytes) as (12, n) u64 arrays from aggregate_dict_tiers' rows."""
    n = len(rows)
    tc, tb = np.zeros((NUM_TIERS, n), np.uint64), np.zeros((NUM_TIERS, n), np.uint64)
    for r, row in enumerate(rows):
        tc[:, r] = row[4]
        tb[:, r] = row[5]
    return tc, tb


def present_mask(tiers):
    """Bit t set iff some object has tier t (IndexBuilder.presentTiers: a size-0 object counts)."""
    mask = 0
    for t in np.unique(np.asarray(tiers, np.uint8)):
        mask |= 1 << int(t)
    return mask


def mask_ids(mask):
    return [t for t in range(NUM_TIERS) if (mask >> t) & 1]


def tier_columns_numpy(blob, offs, sizes, tiers, max_depth=0):
    """The rows of R.aggregate_numpy and the (12, n) tier columns, tier by tier."""
    tiers = np.asarray(tiers, np.uint8)
    m = len(tiers)
    sizes = np.zeros(m, np.uint64) if sizes is None else np.asarray(sizes, np.uint64)
    rows = R.aggregate_numpy(blob, offs, sizes, max_depth)
    n = len(rows[2])
    tc, tb = np.zeros((NUM_TIERS, n), np.uint64), np.zeros((NUM_TIERS, n), np.uint64)
    for t in np.unique(tiers):
        sel = tiers == t
        tc[t] = R.aggregate_numpy(blob, offs, sel.astype(np.uint64), max_depth)[4]
        tb[t] = R.aggregate_numpy(blob, offs, sizes * sel.astype(np.uint64), max_depth)[4]
    return rows, tc, tb


def tiers_json(ids):
    """tiers.json's bytes for the tier ids in the given order."""
    if not ids:
        return b'{\n  "tiers": []\n}'
    items = ['    {\n      "id": %d,\n      "name": "%s",\n      "file": "%s"\n    }' % (t, *TIER_TABLE[t]) for t in ids]
    return ('{\n  "tiers": [\n' + ",\n".join(items) + "\n  ]\n}").encode()


def get_breakdown_all(ids, tc, tb, pos):
    """[(tier id, name, bytes, count)] for every manifest tier, in manifest order; zeros when pos
    is past the arrays (tierstats.go:189-215)."""
    n = tc.shape[1]
    return [(t, TIER_TABLE[t][0], int(tb[t, pos]) if pos < n else 0, int(tc[t, pos]) if pos < n else 0) for t in ids]


def get_breakdown(ids, tc, tb, pos):
    """Only the tiers with bytes or count at pos (tierstats.go:157-186)."""
    return [e for e in get_breakdown_all(ids, tc, tb, pos) if e[2] or e[3]]
