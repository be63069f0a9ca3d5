"""The host side of the per-tier statistics (include/s3imph.h section 5e) without a GPU: the tier
table and s3imph_tier_from_s3 against the reference's vectors, tiers.json and tier_stats/ byte
for byte, and s3imph_index_open refusing a malformed tier set on the host — a case that got as
far as selecting a device would come back as a HIP error instead of the status asserted here."""
import ctypes
import json
import os
import re
import shutil
import stat

import numpy as np
import pytest

import oracle as O
import s3imph
import tiers_ref as T
from conftest import GOLDEN, ROOT
from index_dirs import write_index_dir

CASES = json.load(open(os.path.join(GOLDEN, "tiers", "cases.json")))
NEW = {"s3imph_tier_from_s3", "s3imph_tier_name", "s3imph_tier_file", "s3imph_aggregate_plan_tiers_device",
       "s3imph_aggregate_fill_tiers_device", "s3imph_aggregate_tiers_host", "s3imph_index_from_objects_tiers_host",
       "s3imph_write_tier_files", "s3imph_index_attach_tiers", "s3imph_index_tier_count", "s3imph_index_tier_ids",
       "s3imph_index_tiers_device"}

KEYS = [b"", b"a/", b"a/b/", b"b/", b"c/"]
N = len(KEYS)
IDS = [0, 4, 7]
TC = np.zeros((12, N), np.uint64)
TB = np.zeros((12, N), np.uint64)
TC[0], TB[0] = [3, 2, 1, 1, 0], [400, 300, 100, 100, 0]
TC[4], TB[4] = [1, 0, 0, 0, 1], [(1 << 64) - 1, 0, 0, 0, (1 << 64) - 1]
TC[7], TB[7] = [2, 2, 2, 0, 0], [0, 0, 0, 0, 0]  # present through size-0 objects only
MASK = sum(1 << t for t in IDS)


# ---- the table and FromS3 ----------------------------------------------------------------
def test_tier_table():
    assert s3imph.NUM_TIERS == 12
    assert [list(t) for t in s3imph.TIERS] == CASES["tier_table"]
    for bad in (12, 13, 255, -1):
        assert s3imph.LIB.s3imph_tier_name(bad) is None and s3imph.LIB.s3imph_tier_file(bad) is None


@pytest.mark.parametrize("sc,at,want", CASES["from_s3"], ids=[f"{v[0].strip()}-{v[1]}" for v in CASES["from_s3"]])
def test_tier_from_s3(sc, at, want):
    assert s3imph.tier_from_s3(sc, at) == want


def test_tier_from_s3_edges():
    assert s3imph.LIB.s3imph_tier_from_s3(None, None) == 0
    assert s3imph.tier_from_s3("\tintelligent_tiering\n", " archive_access ") == 10
    assert s3imph.tier_from_s3("INTELLIGENT_TIERING_ARCHIVE", "") == 10  # the tiers' own names map to themselves
    assert s3imph.tier_from_s3("GLACIER", "DEEP_ARCHIVE") == 4           # access tier ignored outside IT


def test_header_and_binding_agree_on_the_new_exports():
    src = open(os.path.join(ROOT, "include", "s3imph.h")).read()
    declared = set(re.findall(r"^(?:int|void|uint64_t|const char)\s*\*?\s*(s3imph_[a-z0-9_]+)\(", src, re.M))
    assert NEW <= declared and NEW <= set(s3imph.EXPORTS)
    lib = ctypes.CDLL(s3imph.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
    assert s3imph.LIB.s3imph_abi_version() == 1
    assert "#define S3IMPH_NUM_TIERS 12" in src


# ---- the files -----------------------------------------------------------------------------
def test_tier_files_byte_for_byte(tmp_path):
    s3imph.write_tier_files(str(tmp_path), MASK, TC, TB)
    text = (tmp_path / "tiers.json").read_bytes()
    assert text == T.tiers_json(IDS)
    assert text == (b'{\n  "tiers": [\n    {\n      "id": 0,\n      "name": "STANDARD",\n      "file": "standard"\n    },\n'
                    b'    {\n      "id": 4,\n      "name": "GLACIER",\n      "file": "glacier_fr"\n    },\n'
                    b'    {\n      "id": 7,\n      "name": "INTELLIGENT_TIERING_FREQUENT",\n      "file": "it_frequent"\n'
                    b'    }\n  ]\n}')
    assert stat.S_IMODE(os.stat(tmp_path / "tiers.json").st_mode) & ~0o644 == 0
    want = {}
    for t in IDS:
        want[T.TIER_TABLE[t][1] + "_count.u64"] = O.s3id_u64_array(TC[t])
        want[T.TIER_TABLE[t][1] + "_bytes.u64"] = O.s3id_u64_array(TB[t])
    assert sorted(os.listdir(tmp_path / "tier_stats")) == sorted(want)
    for name, data in want.items():
        assert (tmp_path / "tier_stats" / name).read_bytes() == data, name


def test_no_present_tier_writes_nothing(tmp_path):
    s3imph.write_tier_files(str(tmp_path), 0, np.zeros((12, 0), np.uint64), np.zeros((12, 0), np.uint64))
    s3imph.write_tier_files(str(tmp_path), 1 << 12, TC, TB)  # bits past the 12 tiers are no tiers
    assert os.listdir(tmp_path) == []


def test_tier_files_missing_dir_is_io_error(tmp_path):
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.write_tier_files(str(tmp_path / "nope"), MASK, TC, TB)
    assert e.value.status == s3imph.ERR_IO and str(e.value).startswith("create tier_stats dir: ")


# ---- Open ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def valid_dir(tmp_path_factory, oracle_lib):
    d = tmp_path_factory.mktemp("tier_index")
    write_index_dir(d, oracle_lib, KEYS)
    s3imph.write_tier_files(str(d), MASK, TC, TB)
    return d


def _json(d, doc):
    (d / "tiers.json").write_text(doc if isinstance(doc, str) else json.dumps(doc))


def _entries(*ids, **over):
    out = []
    for t in ids:
        e = {"id": t, "name": T.TIER_TABLE[t % 12][0], "file": T.TIER_TABLE[t % 12][1]}
        e.update(over)
        out.append(e)
    return {"tiers": out}


def _short(name):
    def damage(d):
        (d / "tier_stats" / name).write_bytes(O.s3id_u64_array(np.arange(N - 1, dtype=np.uint64)))
    return damage


def _width4(d):
    (d / "tier_stats" / "standard_bytes.u64").write_bytes(O.s3id_u32_array(np.arange(N, dtype=np.uint32)))


BAD = [
    ("missing_bytes_file", lambda d: os.remove(d / "tier_stats" / "glacier_fr_bytes.u64"), s3imph.ERR_IO,
     "open tier stats: open GLACIER bytes: "),
    ("missing_counts_file", lambda d: os.remove(d / "tier_stats" / "it_frequent_count.u64"), s3imph.ERR_IO,
     "open tier stats: open INTELLIGENT_TIERING_FREQUENT counts: "),
    ("missing_tier_stats_dir", lambda d: shutil.rmtree(d / "tier_stats"), s3imph.ERR_IO,
     "open tier stats: open STANDARD bytes: "),
    ("bytes_one_short", _short("standard_bytes.u64"), s3imph.ERR_FORMAT, "open tier stats: open STANDARD bytes: "),
    ("counts_one_short", _short("glacier_fr_count.u64"), s3imph.ERR_FORMAT, "open tier stats: open GLACIER counts: "),
    ("width_4_for_8", _width4, s3imph.ERR_FORMAT, "open tier stats: open STANDARD bytes: "),
    ("json_truncated", lambda d: _json(d, '{"tiers": [{"id": 0, "name": "STANDARD"'), s3imph.ERR_FORMAT,
     "open tier stats: read tier manifest: parse tier manifest: "),
    ("json_not_json", lambda d: _json(d, "tiers: standard"), s3imph.ERR_FORMAT,
     "open tier stats: read tier manifest: parse tier manifest: "),
    ("json_trailing_text", lambda d: _json(d, T.tiers_json(IDS).decode() + "}"), s3imph.ERR_FORMAT,
     "open tier stats: read tier manifest: parse tier manifest: "),
    ("json_tiers_is_a_string", lambda d: _json(d, {"tiers": "standard"}), s3imph.ERR_FORMAT,
     "open tier stats: read tier manifest: parse tier manifest: "),
    ("json_id_is_a_string", lambda d: _json(d, _entries(0, id="0")), s3imph.ERR_FORMAT,
     "open tier stats: read tier manifest: parse tier manifest: "),
    ("json_id_negative", lambda d: _json(d, _entries(0, id=-1)), s3imph.ERR_FORMAT,
     "open tier stats: read tier manifest: parse tier manifest: "),
    ("duplicate_id", lambda d: _json(d, _entries(0, 4, 0)), s3imph.ERR_FORMAT, "open tier stats: read tier manifest: "),
    ("id_12", lambda d: _json(d, _entries(0, 12)), s3imph.ERR_FORMAT, "open tier stats: read tier manifest: "),
    ("id_255", lambda d: _json(d, _entries(255)), s3imph.ERR_FORMAT, "open tier stats: read tier manifest: "),
    ("file_with_separator", lambda d: _json(d, _entries(0, file="../tier_stats/standard")), s3imph.ERR_FORMAT,
     "open tier stats: read tier manifest: "),
    ("file_with_dotdot", lambda d: _json(d, _entries(0, file="..standard")), s3imph.ERR_FORMAT,
     "open tier stats: read tier manifest: "),
    ("file_with_slash", lambda d: _json(d, _entries(0, file="x/standard")), s3imph.ERR_FORMAT,
     "open tier stats: read tier manifest: "),
]


@pytest.mark.parametrize("name,damage,status,prefix", BAD, ids=[c[0] for c in BAD])
def test_open_refuses_bad_tier_data_on_the_host(valid_dir, tmp_path, name, damage, status, prefix):
    d = tmp_path / "idx"
    shutil.copytree(valid_dir, d)
    damage(d)
    with pytest.raises(s3imph.MPHFError) as e:
        s3imph.Index(str(d))
    assert e.value.status == status, str(e.value)
    assert str(e.value).startswith(prefix), str(e.value)


def _passes_host_validation(d, tiers):
    """What stops an undamaged directory here, if anything, is the device (no GPU on this machine)."""
    try:
        idx = s3imph.Index(str(d))
    except s3imph.MPHFError as e:
        assert e.status == s3imph.ERR_HIP, str(e)
    else:
        assert idx.count == N and idx.present_tiers() == tiers and idx.has_tier_data() == bool(tiers)
        idx.close()


def test_valid_tier_directory_passes_host_validation(valid_dir):
    _passes_host_validation(valid_dir, IDS)


def test_manifest_order_and_extra_fields_pass(valid_dir, tmp_path):
    d = tmp_path / "idx"
    shutil.copytree(valid_dir, d)
    doc = _entries(7, 0, 4)
    doc["tiers"][0]["note"] = {"nested": [1, 2.5e3, "x\\u0041", None, True]}
    doc["version"] = 3
    _json(d, doc)
    _passes_host_validation(d, [7, 0, 4])


@pytest.mark.parametrize("doc", [None, '{"tiers": []}', "{}", '{"tiers": null}'], ids=["absent", "empty", "none", "null"])
def test_directory_without_tier_data_opens_as_before(valid_dir, tmp_path, doc):
    d = tmp_path / "idx"
    shutil.copytree(valid_dir, d)
    os.remove(d / "tiers.json")
    shutil.rmtree(d / "tier_stats")  # not looked at without a manifest
    if doc is not None:
        _json(d, doc)
    _passes_host_validation(d, [])


def test_null_arguments():
    assert s3imph.LIB.s3imph_index_tier_count(None) == 0
    assert s3imph.LIB.s3imph_index_tier_ids(None, None, 0) == 0
    assert s3imph.LIB.s3imph_index_tiers_device(None, None, 0, None, None, None) == s3imph.ERR_INVALID
    assert s3imph.LIB.s3imph_index_attach_tiers(None, None, 0, None, None, 0) == s3imph.ERR_INVALID
    assert s3imph.LIB.s3imph_aggregate_fill_tiers_device(None, None, None, 0, None) == s3imph.ERR_INVALID
    assert s3imph.LIB.s3imph_write_tier_files(None, 0, None, None, 0, 0, None, 0) == s3imph.ERR_INVALID
