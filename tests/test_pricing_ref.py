"""tests/pricing_ref.py against the values the reference's own tests pin, and the fixture's random set
against what it must contain to be worth running the library over (no GPU, no library)."""
import numpy as np

import pricing_cases as C
import pricing_ref as P

CASES = C.CASES
DEFAULT = C.TABLES["default"]


def by_id(breakdown):
    """[tier name, bytes, count] -> [(tier id, count, bytes)]; a name that is no tier has no id and
    cannot be in a breakdown of ours (the reference skips it as unpriced)."""
    return [(C.TIER_ID[n], c, b) for n, b, c in breakdown if n in C.TIER_ID]


def test_reference_cases():
    for case in CASES["reference_cases"]:
        r = P.compute_monthly_cost(by_id(case["breakdown"]), DEFAULT)
        for field, want in case["expect"].items():
            assert r[field] == want, (case["name"], field)
        for field in case["nonzero"]:
            assert r[field] > 0, (case["name"], field)
        assert r["total"] == (sum(r["per_tier"]) + r["monitoring"]) & P.M64  # TestComputeMonthlyCost_MultipleTiers


def test_min_object_size_case_in_full():
    # 10 KB x 1000 in STANDARD_IA: storage 10240000 / 2^30 * 12500 = 119.21 -> 119; the penalty is on
    # 118 KB x 1000: 120832000 / 2^30 * 12500 = 1406.67 -> 1406 (both far from an integer: no rounding doubt)
    r = P.compute_monthly_cost([(1, 1000, 10 * 1024 * 1000)], DEFAULT)
    assert r["min_object_size"] == 120832000 * 12500 // (1 << 30) == 1406
    assert r["per_tier"][1] == 10240000 * 12500 // (1 << 30) + 1406 == 119 + 1406 == r["total"] and r["tier_mask"] == 2


def test_detailed_breakdown():
    d = P.compute_detailed_breakdown([(1, 1000, 10 * 1024 * 1000), (7, 100, 100 << 20), (4, 500, 1 << 30)], DEFAULT)
    assert [e["tier_name"] for e in d] == ["STANDARD_IA", "INTELLIGENT_TIERING_FREQUENT", "GLACIER"]
    assert d[0]["min_size_penalty"] > 0 and d[0]["avg_object_size_bytes"] == 10 * 1024
    assert d[1]["monitoring_cost"] == 100 / 1000.0 * 0.0025 and d[2]["glacier_overhead"] > 0
    for e in d:
        assert e["total_cost"] == e["storage_cost"] + e["min_size_penalty"] + e["monitoring_cost"] + e["glacier_overhead"]
    assert P.compute_detailed_breakdown([(0, 1, 1)], C.TABLES["partial"])[0]["tier_name"] == "STANDARD"
    assert P.compute_detailed_breakdown([(1, 1, 1)], C.TABLES["partial"]) == []


def test_formatters():
    for micro, want in CASES["format_cost"]:
        assert P.format_cost(micro) == want
    for dollars, want in CASES["format_cost_dollars"]:
        assert P.format_cost_dollars(dollars) == want


def test_price_table_json():
    assert P.price_table_json(DEFAULT) == CASES["default_table_json"].encode()
    assert DEFAULT == P.default_table()
    for v, want in ((0.0, "0"), (5.0, "5"), (1e-6, "0.000001"), (9.9e-7, "9.9e-7"), (1.5e-10, "1.5e-10"),
                    (1e20, "100000000000000000000"), (1e21, "1e+21"), (1.25e30, "1.25e+30"), (0.1 + 0.2, "0.30000000000000004")):
        assert P.json_number(v) == want, v
    empty = {"per_gb_month": {}, "monitoring": 0.0, "standard": 0.0}
    assert P.price_table_json(empty) == (b'{\n  "per_gb_month": {},\n  "monitoring_per_1000_objects": 0,\n'
                                         b'  "standard_price_per_gb": 0\n}')


def test_random_set_is_sensitive_to_order_and_precision():
    prices = np.array([DEFAULT["per_gb_month"][t] for t in range(12)])
    g = C.BYTES.astype(np.float64) / P.GB
    exact = np.floor(g * prices * 1e6)
    reordered = np.floor(g * (prices * 1e6))
    g32 = C.BYTES.astype(np.float32) / np.float32(P.GB)
    single = np.floor((g32 * prices.astype(np.float32) * np.float32(1e6)).astype(np.float64))
    assert C.BYTES.size >= 49152
    assert int((exact != reordered).sum()) >= 8
    assert int((exact != single).sum()) >= 8
    # the numpy form above is the ref's own arithmetic: spot-check it on the terms that differ
    for i, t in zip(*np.nonzero(exact != reordered)):
        assert P.micro(int(C.BYTES[i, t]), float(prices[t])) == int(exact[i, t])


def test_random_set_holds_the_edge_cases():
    e = CASES["edges"]

    def slot(name):
        i, t = e[name]
        return t, int(C.COUNT[i, t]), int(C.BYTES[i, t])

    def avg(name):
        _, c, b = slot(name)
        return b // c

    assert avg("avg_131071") == 131071 and avg("avg_131072") == 131072
    assert avg("avg_131071_monitored") == 131071 and avg("avg_131072_monitored") == 131072
    t, c, b = slot("avg_0_bytes_gt_0")
    assert b > 0 and c > b and t in P.MIN_SIZE
    t, c, b = slot("avg_0_monitored")
    assert b > 0 and c > b and t in P.MONITORING
    for name in ("count_0_bytes_gt_0", "count_0_glacier"):
        t, c, b = slot(name)
        assert c == 0 and b > 0
    assert slot("count_0_glacier")[0] in P.GLACIER
    t, c, b = slot("bytes_2_53_plus_1")
    assert b >= 1 << 53 and int(float(b)) != b
    t, c, b = slot("count_2_49")
    assert t in P.GLACIER and c >= 1 << 49 and c * 32768 > P.M64
    t, c, b = slot("count_2_63_overhead_wraps")
    assert t in P.GLACIER and t in P.MONITORING and c * 8192 > P.M64
    for name in ("penalty_product_wraps", "penalty_product_wraps_to_small"):
        t, c, b = slot(name)
        assert t in P.MIN_SIZE and 0 < b // c < 131072 and (131072 - b // c) * c > P.M64
    assert not C.COUNT[e["all_zero_node"][0]].any() and not C.BYTES[e["all_zero_node"][0]].any()
    # the random part itself reaches these without planting
    assert int((C.BYTES >= np.uint64(1 << 53)).sum()) > 100 and int((C.COUNT >= np.uint64(1 << 49)).sum()) > 100
    assert int((C.COUNT > C.BYTES).sum()) > 1000
    # the tables
    assert C.TABLES["no_monitoring"]["monitoring"] == 0
    assert 0 < len(C.TABLES["partial"]["per_gb_month"]) < 12
    clamped = C.ref_records("clamp")
    assert any(r["per_tier"][0] == P.M64 for r in clamped) and any(r["monitoring"] != 0 for r in clamped)
    assert P.u64(float("nan")) == P.M64 and P.u64(2.0 ** 64) == P.M64 and P.u64(2.0 ** 64 - 2048) == (1 << 64) - 2048


def test_edge_values_by_hand():
    r = P.compute_monthly_cost([(3, 5000, 4999), (9, 5000, 4999)], DEFAULT)  # avg 0: no penalty, nothing monitored
    assert r["min_object_size"] == 0 and r["monitoring"] == 0 and r["tier_mask"] == (1 << 3 | 1 << 9)
    r = P.compute_monthly_cost([(7, 4097, 131072 * 4097), (8, 4097, 131072 * 4097 - 1)], DEFAULT)
    assert r["monitoring"] == int(4097 / 1000.0 * 0.0025 * 1e6) + int(2048 / 1000.0 * 0.0025 * 1e6)
    r = P.compute_monthly_cost([(4, 0, 1 << 40)], DEFAULT)  # count 0: storage only
    assert r["glacier_overhead"] == 0 and r["total"] == int(1024 * 0.0036 * 1e6)
    r = P.compute_monthly_cost([(1, 1 << 50, (1 << 50) * 100)], DEFAULT)
    add = ((131072 - 100) << 50) & P.M64
    assert r["min_object_size"] == int(float(add) / P.GB * 0.0125 * 1e6) and add < (131072 - 100) << 50
    assert P.compute_monthly_cost([(0, 7, 1 << 30)], C.TABLES["partial"])["total"] == 23000
    assert P.compute_monthly_cost([(1, 7, 1 << 30)], C.TABLES["partial"]) == dict(P.ZERO_COST, found=1)


def test_top_of_row():
    key = {0: 5, 1: 1 << 63, 2: 5, 3: 0, 4: (1 << 63) + 1, 9: 5}
    assert P.top_of_row([0, 1, 2, 3, 4, 9], key, 4) == [4, 1, 0, 2]
    assert P.top_of_row([9, 2, 0], key, 10) == [0, 2, 9] and P.top_of_row([], key, 3) == []
