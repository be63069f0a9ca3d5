"""The host side of the cost estimate (include/s3imph.h section 5h) against tests/pricing_ref.py:
s3imph_compute_monthly_cost, the default table, the price-table files, the argument checks.  No
device call here."""
import ctypes
import os
import re

import numpy as np
import pytest

import pricing_cases as C
import pricing_ref as P
import s3imph
from conftest import ROOT

CASES = C.CASES
NEW = ("s3imph_price_table_default", "s3imph_price_table_load", "s3imph_price_table_save",
       "s3imph_compute_monthly_cost", "s3imph_index_cost_device", "s3imph_index_descendants_top")


def lib_table(name):
    t = CASES["tables"][name]
    return s3imph.PriceTable(t["per_gb_month"], t["monitoring_per_1000_objects"], t["standard_price_per_gb"])


def record(ids, count, nbytes, pt):
    ids = np.asarray(ids, np.uint8)
    out = np.zeros(1, s3imph.COST_DTYPE)
    c, b = np.ascontiguousarray(count, np.uint64), np.ascontiguousarray(nbytes, np.uint64)
    rc = s3imph.LIB.s3imph_compute_monthly_cost(ids.ctypes.data, c.ctypes.data, b.ctypes.data, len(ids),
                                                ctypes.byref(pt._c()), out.ctypes.data)
    return rc, out[0]


@pytest.mark.parametrize("table", list(CASES["tables"]))
def test_host_cost_equals_the_ref_on_every_fixture_case(table):
    pt = lib_table(table)._c()
    want = C.ref_records(table)
    ids = np.arange(12, dtype=np.uint8)
    out = np.zeros(C.N, s3imph.COST_DTYPE)
    f = s3imph.LIB.s3imph_compute_monthly_cost
    for i in range(C.N):
        assert f(ids.ctypes.data, C.COUNT[i].ctypes.data, C.BYTES[i].ctypes.data, 12, ctypes.byref(pt),
                 out[i:].ctypes.data) == s3imph.OK
    for i in range(C.N):
        C.same_record(out[i], want[i], f"{table} node {i}")


def test_host_cost_subset_and_manifest_order():
    order = [5, 0, 11, 4, 7]
    want = C.ref_records("default", order)
    pt = lib_table("default")
    for i in (0, 3, 5, 7, 9, 13, 14, 20, 4095):
        rc, got = record(order, C.COUNT[i, order], C.BYTES[i, order], pt)
        assert rc == s3imph.OK
        C.same_record(got, want[i], f"node {i}")
    rc, got = record([], [], [], pt)
    assert rc == s3imph.OK
    C.same_record(got, dict(P.ZERO_COST, found=1))


def test_reference_cases_through_the_binding():
    for case in CASES["reference_cases"]:
        bd = [(C.TIER_ID[n], n, b, c) for n, b, c in case["breakdown"] if n in C.TIER_ID]
        r = s3imph.compute_monthly_cost(bd)
        for field, want in case["expect"].items():
            assert r[field] == want, (case["name"], field)
        for field in case["nonzero"]:
            assert r[field] > 0, (case["name"], field)
        assert set(r["per_tier"]) == {n for _, n, b, c in bd if b or c}
    d = s3imph.compute_detailed_breakdown([(1, "STANDARD_IA", 10 * 1024 * 1000, 1000), (4, "GLACIER", 1 << 30, 500),
                                           (0, "NOPE", 1, 1)])
    assert d == P.compute_detailed_breakdown([(1, 1000, 10 * 1024 * 1000), (4, 500, 1 << 30)], C.TABLES["default"])
    for micro, want in CASES["format_cost"]:
        assert s3imph.format_cost(micro) == want
    for dollars, want in CASES["format_cost_dollars"]:
        assert s3imph.format_cost_dollars(dollars) == want


def test_default_table_and_its_file(tmp_path):
    pt = s3imph.PriceTable.default_us_east_1()
    d = CASES["default_table"]
    assert pt.per_gb_month == d["per_gb_month"]
    assert pt.monitoring_per_1000_objects == d["monitoring_per_1000_objects"]
    assert pt.standard_price_per_gb == d["standard_price_per_gb"]
    p = tmp_path / "prices.json"
    pt.save(str(p))
    assert p.read_bytes() == CASES["default_table_json"].encode()
    assert (os.stat(p).st_mode & 0o777) == 0o644 & ~_umask()
    assert s3imph.PriceTable.load(str(p)) == pt


def _umask():
    m = os.umask(0)
    os.umask(m)
    return m


def test_load_save_round_trips_random_tables_bit_for_bit(tmp_path):
    rng = np.random.default_rng(77)
    names = [n for _, n, _ in s3imph.TIERS]
    p = tmp_path / "t.json"
    for k in range(40):
        # doubles of every magnitude: random bit patterns with the sign cleared, finite
        vals = rng.integers(0, 0x7FF0 << 48, 14, dtype=np.uint64).view(np.float64)
        if k == 0:
            vals[:6] = [0.0, 5e-324, 1e-6, 9.999999e-7, 1e21, 1.7976931348623157e308]
        priced = [n for n in names if rng.integers(0, 2)] if k else names
        pt = s3imph.PriceTable({n: float(vals[i]) for i, n in enumerate(priced)}, float(vals[12]), float(vals[13]))
        pt.save(str(p))
        ref = {"per_gb_month": {C.TIER_ID[n]: v for n, v in pt.per_gb_month.items()},
               "monitoring": pt.monitoring_per_1000_objects, "standard": pt.standard_price_per_gb}
        assert p.read_bytes() == P.price_table_json(ref), k
        got = s3imph.PriceTable.load(str(p))
        assert got == pt, k  # float == float: the same bits (no NaN, no negative zero here)


def test_load_is_lenient_as_encoding_json(tmp_path):
    p = tmp_path / "t.json"
    p.write_text('{"Per_GB_Month": {"STANDARD": 0.5, "standard": 9, "MOON_BASE": 3, "GLACIER": null},'
                 ' "MONITORING_PER_1000_OBJECTS": 2e-3, "comment": ["x", {"y": [1, 2]}], "standard_price_per_gb": 1}')
    pt = s3imph.PriceTable.load(str(p))
    assert pt.per_gb_month == {"STANDARD": 0.5, "GLACIER": 0.0}
    assert pt.monitoring_per_1000_objects == 0.002 and pt.standard_price_per_gb == 1.0
    p.write_text("{}")
    assert s3imph.PriceTable.load(str(p)) == s3imph.PriceTable()
    p.write_text('{"per_gb_month": {"STANDARD": 1e-999}}')
    assert s3imph.PriceTable.load(str(p)).per_gb_month == {"STANDARD": 0.0}


MALFORMED = {
    "truncated": '{"per_gb_month": {"STANDARD": 0.02',
    "not_json": "not valid json",
    "string_for_number": '{"per_gb_month": {"STANDARD": "0.023"}}',
    "string_for_fee": '{"monitoring_per_1000_objects": "x"}',
    "array_for_map": '{"per_gb_month": [1, 2]}',
    "array_at_top": "[]",
    "out_of_range": '{"per_gb_month": {"STANDARD": 1e999}}',
    "negative_price": '{"per_gb_month": {"GLACIER": -0.004}}',
    "negative_fee": '{"monitoring_per_1000_objects": -1}',
    "trailing": '{} {}',
    "empty": "",
}


@pytest.mark.parametrize("name", MALFORMED, ids=list(MALFORMED))
def test_load_refuses_malformed_tables(tmp_path, name):
    p = tmp_path / "t.json"
    p.write_text(MALFORMED[name])
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.PriceTable.load(str(p))
    assert e.value.status == s3imph.ERR_FORMAT and str(e.value).startswith("parse price table: ")


def test_load_missing_file_and_save_into_missing_dir(tmp_path):
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.PriceTable.load(str(tmp_path / "nope.json"))
    assert e.value.status == s3imph.ERR_IO and str(e.value).startswith("read price table: ")
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.PriceTable.default_us_east_1().save(str(tmp_path / "nope" / "t.json"))
    assert e.value.status == s3imph.ERR_IO and str(e.value).startswith("write price table: ")


def test_invalid_arguments_of_the_host_cost():
    pt = lib_table("default")
    one = np.ones(13, np.uint64)
    assert record(list(range(12)) + [0], one, one, pt)[0] == s3imph.ERR_INVALID     # T > 12
    assert record([0, 12], one[:2], one[:2], pt)[0] == s3imph.ERR_INVALID           # id >= 12
    assert record([3, 5, 3], one[:3], one[:3], pt)[0] == s3imph.ERR_INVALID         # duplicate id
    for bad in (-0.5, float("nan"), float("inf")):
        assert record([0], one[:1], one[:1], s3imph.PriceTable({"STANDARD": bad}))[0] == s3imph.ERR_INVALID
        assert record([0], one[:1], one[:1], s3imph.PriceTable({}, bad, 0.0))[0] == s3imph.ERR_INVALID
        assert record([0], one[:1], one[:1], s3imph.PriceTable({}, 0.0, bad))[0] == s3imph.ERR_INVALID
    f = s3imph.LIB.s3imph_compute_monthly_cost
    out = np.zeros(1, s3imph.COST_DTYPE)
    assert f(None, None, None, 1, ctypes.byref(pt._c()), out.ctypes.data) == s3imph.ERR_INVALID
    assert f(None, None, None, 0, None, out.ctypes.data) == s3imph.ERR_INVALID
    assert f(None, None, None, 0, ctypes.byref(pt._c()), None) == s3imph.ERR_INVALID
    assert s3imph.LIB.s3imph_price_table_default(None) == s3imph.ERR_INVALID


def test_header_binding_and_exports_agree_on_the_new_names():
    src = open(os.path.join(ROOT, "include", "s3imph.h")).read()
    declared = set(re.findall(r"^int\s+(s3imph_[a-z0-9_]+)\(", src, re.M))
    lib = ctypes.CDLL(s3imph.LIB_PATH)
    for name in NEW:
        assert name in declared and name in s3imph.EXPORTS and hasattr(lib, name), name
    assert s3imph.LIB.s3imph_abi_version() == 1
    assert ctypes.sizeof(s3imph._PriceTable) == 120 and s3imph.COST_DTYPE.itemsize == 136
    assert "/* 120 bytes */" in src and "/* 136 bytes */" in src
    for name, v in (("S3IMPH_RANK_OBJECT_COUNT", 0), ("S3IMPH_RANK_TOTAL_BYTES", 1), ("S3IMPH_RANK_MONTHLY_COST", 2)):
        assert re.search(r"^#define %s\s+%d\b" % (name, v), src, re.M)
    assert (s3imph.RANK_OBJECT_COUNT, s3imph.RANK_TOTAL_BYTES, s3imph.RANK_MONTHLY_COST) == (0, 1, 2)


def test_device_entry_points_refuse_null_arguments_on_the_host():
    pt = lib_table("default")._c()
    cost, top = s3imph.LIB.s3imph_index_cost_device, s3imph.LIB.s3imph_index_descendants_top
    assert cost(None, None, 0, ctypes.byref(pt), None, None) == s3imph.ERR_INVALID
    assert cost(None, None, 5, None, None, None) == s3imph.ERR_INVALID
    assert top(None, 2, ctypes.byref(pt), 10, None, None, None, None) == s3imph.ERR_INVALID
    assert top(None, 0, None, 0, None, None, None, None) == s3imph.ERR_INVALID
