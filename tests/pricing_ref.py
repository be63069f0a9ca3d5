"""The cost estimate restated for the tests (no GPU; include/s3imph.h section 5h):

  compute_monthly_cost        pricing.ComputeMonthlyCost (pkg/pricing/pricing.go:159-240) over a
                              breakdown [(tier id, count, bytes)], as a dict shaped like s3imph_cost;
  compute_detailed_breakdown  ComputeDetailedBreakdown (:256-312);
  format_cost[_dollars]       FormatCost / FormatCostDollars (:315-331);
  price_table_json            json.MarshalIndent(PriceTable, "", "  ") (SavePriceTable, :111-122);
  top_of_row                  descendants_top's ordering of one row.

Python floats are IEEE binary64 and int() truncates toward zero, so the arithmetic below is the
reference's, operation for operation; u64 sums and products wrap through M64.  A price table here is
a dict {"per_gb_month": {tier id: price}, "monitoring": fee, "standard": price}."""
from decimal import Decimal

M64 = (1 << 64) - 1
NUM_TIERS = 12
TIER_NAMES = ["STANDARD", "STANDARD_IA", "ONEZONE_IA", "GLACIER_IR", "GLACIER", "DEEP_ARCHIVE", "REDUCED_REDUNDANCY",
              "INTELLIGENT_TIERING_FREQUENT", "INTELLIGENT_TIERING_INFREQUENT", "INTELLIGENT_TIERING_ARCHIVE_INSTANT",
              "INTELLIGENT_TIERING_ARCHIVE", "INTELLIGENT_TIERING_DEEP_ARCHIVE"]
MIN_SIZE = frozenset((1, 2, 3))           # TiersWithMinObjectSize, pricing.go:39-43
MONITORING = frozenset((7, 8, 9, 10, 11))  # TiersWithMonitoringCost, :46-52
GLACIER = frozenset((4, 5, 10, 11))       # TiersWithGlacierOverhead, :56-61
GB = 1073741824.0
MIN_OBJECT = 131072


def default_table():
    """DefaultUSEast1Prices (pricing.go:67-93) by tier id."""
    p = [0.023, 0.0125, 0.01, 0.004, 0.0036, 0.00099, 0.024, 0.023, 0.0125, 0.004, 0.0036, 0.00099]
    return {"per_gb_month": dict(enumerate(p)), "monitoring": 0.0025, "standard": 0.023}


def u64(x: float) -> int:
    """uint64(x) for x >= 0; NaN and x >= 2^64 are pinned to 2^64 - 1 (section 5h)."""
    if x != x or x >= 18446744073709551616.0:
        return M64
    return int(x)


def micro(nbytes: int, price: float) -> int:
    return u64(float(nbytes) / GB * price * 1e6)


def price_slot(tier, count, nbytes, pt):
    """(storage, penalty, monitoring, overhead) of a priced slot, None for an unpriced tier."""
    if tier not in pt["per_gb_month"]:
        return None
    price = pt["per_gb_month"][tier]
    storage = micro(nbytes, price)
    avg = nbytes // count if count else 0
    penalty = monitoring = overhead = 0
    if tier in MIN_SIZE and 0 < avg < MIN_OBJECT:
        penalty = micro(((MIN_OBJECT - avg) * count) & M64, price)
    if tier in MONITORING and pt["monitoring"] > 0:
        mon = count if avg >= MIN_OBJECT else (count // 2 if avg > 0 else 0)
        if mon > 0:
            monitoring = u64(float(mon) / 1000.0 * pt["monitoring"] * 1e6)
    if tier in GLACIER and count > 0:
        overhead = (micro((count * 32768) & M64, price) + micro((count * 8192) & M64, pt["standard"])) & M64
    return storage, penalty, monitoring, overhead


def compute_monthly_cost(breakdown, pt, found=1):
    """s3imph_cost as a dict for a breakdown [(tier id, count, bytes)] (distinct ids)."""
    r = {"total": 0, "monitoring": 0, "min_object_size": 0, "glacier_overhead": 0, "per_tier": [0] * NUM_TIERS,
         "tier_mask": 0, "found": found}
    for tier, count, nbytes in breakdown:
        c = price_slot(tier, count, nbytes, pt)
        if c is None:
            continue
        storage, penalty, monitoring, overhead = c
        tier_total = (storage + penalty + overhead) & M64
        r["per_tier"][tier] = tier_total
        r["total"] = (r["total"] + tier_total) & M64
        r["monitoring"] = (r["monitoring"] + monitoring) & M64
        r["min_object_size"] = (r["min_object_size"] + penalty) & M64
        r["glacier_overhead"] = (r["glacier_overhead"] + overhead) & M64
        if count | nbytes:
            r["tier_mask"] |= 1 << tier
    r["total"] = (r["total"] + r["monitoring"]) & M64
    return r


ZERO_COST = {"total": 0, "monitoring": 0, "min_object_size": 0, "glacier_overhead": 0, "per_tier": [0] * NUM_TIERS,
             "tier_mask": 0, "found": 0}


def compute_detailed_breakdown(breakdown, pt):
    """ComputeDetailedBreakdown over [(tier id, count, bytes)]: dicts of dollars per priced tier."""
    out = []
    for tier, count, nbytes in breakdown:
        if tier not in pt["per_gb_month"]:
            continue
        price = pt["per_gb_month"][tier]
        avg = nbytes // count if count else 0
        cb = {"tier_name": TIER_NAMES[tier], "object_count": count, "bytes": nbytes, "avg_object_size_bytes": avg,
              "storage_cost": float(nbytes) / GB * price, "min_size_penalty": 0.0, "monitoring_cost": 0.0,
              "glacier_overhead": 0.0}
        if tier in MIN_SIZE and 0 < avg < MIN_OBJECT:
            cb["min_size_penalty"] = float(((MIN_OBJECT - avg) * count) & M64) / GB * price
        if tier in MONITORING and pt["monitoring"] > 0:
            mon = count if avg >= MIN_OBJECT else (count // 2 if avg > 0 else 0)
            cb["monitoring_cost"] = float(mon) / 1000.0 * pt["monitoring"]
        if tier in GLACIER and count > 0:
            cb["glacier_overhead"] = float((count * 32768) & M64) / GB * price
            cb["glacier_overhead"] += float((count * 8192) & M64) / GB * pt["standard"]
        cb["total_cost"] = cb["storage_cost"] + cb["min_size_penalty"] + cb["monitoring_cost"] + cb["glacier_overhead"]
        out.append(cb)
    return out


def format_cost_dollars(dollars: float) -> str:
    if dollars < 0.01:
        return "$%.6f" % dollars
    if dollars < 1:
        return "$%.4f" % dollars
    if dollars < 100:
        return "$%.2f" % dollars
    return "$%.0f" % dollars


def format_cost(microdollars: int) -> str:
    return format_cost_dollars(float(microdollars) / 1_000_000)


def json_number(v: float) -> str:
    """encoding/json's float64: shortest round trip; 'f' for 1e-6 <= |v| < 1e21 and 0, else 'e' with a
    two-digit negative exponent's leading zero dropped."""
    a = abs(v)
    if a != 0 and (a < 1e-6 or a >= 1e21):
        mant, exp = repr(v).split("e")  # repr uses the exponent form throughout this range
        if mant.endswith(".0"):
            mant = mant[:-2]
        sign, digits = exp[0], exp[1:].lstrip("0")
        if sign == "+" or len(digits) >= 2:
            digits = digits.rjust(2, "0")
        return f"{mant}e{sign}{digits}"
    s = format(Decimal(repr(v)), "f")
    if "." in s:
        s = s.rstrip("0").rstrip(".")
    return s


def price_table_json(pt) -> bytes:
    """SavePriceTable's bytes: the priced tiers by name in byte order, then the two scalars."""
    items = sorted((TIER_NAMES[t], p) for t, p in pt["per_gb_month"].items())
    body = ",\n".join('    "%s": %s' % (n, json_number(p)) for n, p in items)
    m = "{\n" + body + "\n  }" if items else "{}"
    return ('{\n  "per_gb_month": %s,\n  "monitoring_per_1000_objects": %s,\n  "standard_price_per_gb": %s\n}'
            % (m, json_number(pt["monitoring"]), json_number(pt["standard"]))).encode()


def top_of_row(row, key, k):
    """The k positions of `row` with the largest key[p] (unsigned), ties by ascending position."""
    return sorted(row, key=lambda p: (-key[p], p))[:k]
