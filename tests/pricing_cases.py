"""tests/golden/pricing/cases.json decoded once for the pricing tests: the tables in the form
tests/pricing_ref.py prices with, the random breakdowns (random.npz) as (n, 12) u64 arrays, and the reference
record of every (table, node), computed once and shared."""
import json
import os

import numpy as np

import pricing_ref as P

_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pricing")
CASES = json.load(open(os.path.join(_DIR, "cases.json")))
TIER_ID = {name: t for t, name in enumerate(P.TIER_NAMES)}


def ref_table(by_name):
    """A fixture table (tier names) as pricing_ref wants it (tier ids; other names dropped)."""
    return {"per_gb_month": {TIER_ID[n]: p for n, p in by_name["per_gb_month"].items() if n in TIER_ID},
            "monitoring": by_name["monitoring_per_1000_objects"], "standard": by_name["standard_price_per_gb"]}


TABLES = {name: ref_table(t) for name, t in CASES["tables"].items()}


with np.load(os.path.join(_DIR, CASES["random"]["file"])) as _z:
    COUNT, BYTES = _z["count"].astype(np.uint64), _z["bytes"].astype(np.uint64)
assert COUNT.shape == BYTES.shape == (CASES["random"]["n"], CASES["random"]["tiers"])
N = COUNT.shape[0]

_REF = {}


def ref_records(table, ids=tuple(range(12))):
    """The reference record of every node for the manifest slots `ids` (tier ids, in order) under the
    named table: a list of N dicts, kept."""
    key = (table, tuple(ids))
    if key not in _REF:
        pt = TABLES[table]
        _REF[key] = [P.compute_monthly_cost([(t, int(COUNT[i, t]), int(BYTES[i, t])) for t in ids], pt)
                     for i in range(N)]
    return _REF[key]


def same_record(got, want, what=""):
    """A COST_DTYPE record against a pricing_ref dict, field for field."""
    for f in ("total", "monitoring", "min_object_size", "glacier_overhead", "tier_mask", "found"):
        assert int(got[f]) == want[f], (what, f, int(got[f]), want[f])
    assert [int(v) for v in got["per_tier"]] == want["per_tier"], (what, "per_tier")
