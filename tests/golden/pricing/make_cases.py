"""Writes cases.json and random.npz beside this file: python tests/golden/pricing/make_cases.py

  reference_cases     the cases of the reference's own tests (pkg/pricing/pricing_test.go) as data:
                      a breakdown by tier name under the default table and the values they pin;
  format_cost[_dollars]   the FormatCost / FormatCostDollars tables of the same file;
  default_table[_json]    DefaultUSEast1Prices and the text SavePriceTable writes for it;
  tables              the price tables the tests run the random set under;
  random              N breakdowns of all twelve tiers, each value log-uniform over [1, 2^64) (a uniform
                      octave, uniform inside it), with the edge cases of `edges` planted over some of
                      them.  The values themselves are binary, in random.npz: `count` and `bytes`,
                      [N][12] u64 each; cases.json names the file, the seed and the shape.
"""
import json
import os

import numpy as np

# The seed is chosen so that the set holds at least 8 storage terms whose truncated value depends on
# the order of the two multiplications (about 2 in 10 000 do; tests/test_pricing_ref.py counts them).
SEED, N, T = 20266, 4096, 12
M64 = (1 << 64) - 1
NAMES = ["STANDARD", "STANDARD_IA", "ONEZONE_IA", "GLACIER_IR", "GLACIER", "DEEP_ARCHIVE", "REDUCED_REDUNDANCY",
         "INTELLIGENT_TIERING_FREQUENT", "INTELLIGENT_TIERING_INFREQUENT", "INTELLIGENT_TIERING_ARCHIVE_INSTANT",
         "INTELLIGENT_TIERING_ARCHIVE", "INTELLIGENT_TIERING_DEEP_ARCHIVE"]
PRICES = [0.023, 0.0125, 0.01, 0.004, 0.0036, 0.00099, 0.024, 0.023, 0.0125, 0.004, 0.0036, 0.00099]
DEFAULT = {"per_gb_month": dict(zip(NAMES, PRICES)), "monitoring_per_1000_objects": 0.0025,
           "standard_price_per_gb": 0.023}
DEFAULT_JSON = """{
  "per_gb_month": {
    "DEEP_ARCHIVE": 0.00099,
    "GLACIER": 0.0036,
    "GLACIER_IR": 0.004,
    "INTELLIGENT_TIERING_ARCHIVE": 0.0036,
    "INTELLIGENT_TIERING_ARCHIVE_INSTANT": 0.004,
    "INTELLIGENT_TIERING_DEEP_ARCHIVE": 0.00099,
    "INTELLIGENT_TIERING_FREQUENT": 0.023,
    "INTELLIGENT_TIERING_INFREQUENT": 0.0125,
    "ONEZONE_IA": 0.01,
    "REDUCED_REDUNDANCY": 0.024,
    "STANDARD": 0.023,
    "STANDARD_IA": 0.0125
  },
  "monitoring_per_1000_objects": 0.0025,
  "standard_price_per_gb": 0.023
}"""

KB, MB, GB = 1024, 1024 * 1024, 1024 * 1024 * 1024
# [tier name, bytes, object count] as pricing_test.go gives them; `expect` holds what the test pins
# (a value), `nonzero` the fields it only asks to be non-zero
REFERENCE_CASES = [
    {"name": "StandardStorage", "breakdown": [["STANDARD", GB, 1]],
     "expect": {"total": 23000, "monitoring": 0, "min_object_size": 0}, "nonzero": []},
    {"name": "StandardIA_MinObjectSize", "breakdown": [["STANDARD_IA", 10 * KB * 1000, 1000]],
     "expect": {}, "nonzero": ["min_object_size"]},
    {"name": "IntelligentTiering_Monitoring", "breakdown": [["INTELLIGENT_TIERING_FREQUENT", MB * 1000, 1000]],
     "expect": {"monitoring": 2500}, "nonzero": []},
    {"name": "IntelligentTiering_SmallObjects", "breakdown": [["INTELLIGENT_TIERING_FREQUENT", 50 * KB * 1000, 1000]],
     "expect": {"monitoring": 1250}, "nonzero": []},
    {"name": "Glacier_Overhead", "breakdown": [["GLACIER", GB, 1000]], "expect": {}, "nonzero": ["glacier_overhead"]},
    {"name": "DeepArchive_Overhead", "breakdown": [["DEEP_ARCHIVE", 10 * GB, 10000]], "expect": {},
     "nonzero": ["glacier_overhead"]},
    {"name": "UnknownTier", "breakdown": [["UNKNOWN_TIER", GB, 100]], "expect": {"total": 0}, "nonzero": []},
    {"name": "ZeroBytes", "breakdown": [["STANDARD", 0, 0]], "expect": {"total": 0}, "nonzero": []},
]
FORMAT_COST = [[0, "$0.000000"], [100, "$0.000100"], [10_000, "$0.0100"], [100_000, "$0.1000"], [1_000_000, "$1.00"],
               [50_000_000, "$50.00"], [100_000_000, "$100"]]
FORMAT_COST_DOLLARS = [[0.0001, "$0.000100"], [0.05, "$0.0500"], [5.50, "$5.50"], [150.0, "$150"]]

TABLES = {
    "default": DEFAULT,
    "no_monitoring": dict(DEFAULT, monitoring_per_1000_objects=0.0),
    "partial": {"per_gb_month": {n: DEFAULT["per_gb_month"][n] for n in
                                 ("STANDARD", "GLACIER_IR", "INTELLIGENT_TIERING_ARCHIVE", "DEEP_ARCHIVE")},
                "monitoring_per_1000_objects": 0.0025, "standard_price_per_gb": 0.023},
    # a custom price large enough that u64() of a cost reaches the UINT64_MAX clamp
    "clamp": dict(DEFAULT, per_gb_month=dict(DEFAULT["per_gb_month"], STANDARD=1e30, GLACIER=3e25),
                  monitoring_per_1000_objects=1e22, standard_price_per_gb=7e24),
    # a price that puts an octave of the byte counts into [2^63, 2^64) microdollars, below the clamp
    "high": dict(DEFAULT, per_gb_month=dict(DEFAULT["per_gb_month"], STANDARD=1e6)),
}

# name -> (node, tier id, count, bytes), planted over the random values
EDGES = {
    "avg_131071": (3, 1, 1000, 131071 * 1000 + 999),
    "avg_131072": (5, 2, 1000, 131072 * 1000),
    "avg_131072_monitored": (5, 7, 4097, 131072 * 4097),
    "avg_131071_monitored": (6, 8, 4097, 131072 * 4097 - 1),
    "avg_0_bytes_gt_0": (7, 3, 5000, 4999),
    "avg_0_monitored": (7, 9, 5000, 4999),
    "count_0_bytes_gt_0": (9, 1, 0, 123456789),
    "count_0_glacier": (9, 4, 0, 1 << 40),
    "bytes_2_53_plus_1": (11, 0, 3, (1 << 53) + 1),
    "bytes_max": (12, 6, M64, M64),
    "count_2_49": (13, 5, 1 << 49, 1 << 60),
    "count_2_63_overhead_wraps": (14, 10, (1 << 63) + 12345, M64),
    "penalty_product_wraps": (15, 1, 1 << 50, (1 << 50) * 100),
    "penalty_product_wraps_to_small": (16, 3, 1 << 48, 1 << 48),
    "all_zero_node": None,  # node 20: every slot 0
}


def main():
    rng = np.random.default_rng(SEED)

    def log_uniform():  # the octave [2^e, 2^(e+1)) uniform over e, the value uniform inside it
        e = rng.integers(0, 64, (N, T)).astype(np.uint64)
        top = np.uint64(1) << e
        return top | (rng.integers(0, 1 << 64, (N, T), dtype=np.uint64) & (top - np.uint64(1)))

    count, nbytes = log_uniform(), log_uniform()
    edges = {}
    for name, e in EDGES.items():
        if e is None:
            count[20] = 0
            nbytes[20] = 0
            edges[name] = [20, -1]
            continue
        node, tier, c, b = e
        count[node, tier], nbytes[node, tier] = c, b
        edges[name] = [node, tier]
    out = {
        "reference_cases": REFERENCE_CASES, "format_cost": FORMAT_COST, "format_cost_dollars": FORMAT_COST_DOLLARS,
        "default_table": DEFAULT, "default_table_json": DEFAULT_JSON, "tables": TABLES, "edges": edges,
        "random": {"seed": SEED, "n": N, "tiers": T, "file": "random.npz"},
    }
    here = os.path.dirname(os.path.abspath(__file__))
    np.savez_compressed(os.path.join(here, "random.npz"), count=count.astype("<u8"), bytes=nbytes.astype("<u8"))
    path = os.path.join(here, "cases.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
