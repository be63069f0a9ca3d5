"""Section 5g on the GPU: inventory CSV text -> object listing -> index directory.  Every result is
compared bit for bit with tests/csv_ref.py's line-based restatement of encoding/csv (a different
formulation from the kernels' automaton): the info, the offsets, the key blob with its zero
padding, the sizes and the tiers."""
import json
import os
import random

import numpy as np
import pytest

import csv_cases as K
import csv_ref as C
import oracle as O
import s3imph
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CASES = json.load(open(os.path.join(GOLDEN, "csv", "cases.json")))
AGG_CASES = json.load(open(os.path.join(GOLDEN, "aggregate", "cases.json")))["cases"]
TIER_CASES = json.load(open(os.path.join(GOLDEN, "tiers", "cases.json")))["index_cases"]
RUN, TILE = s3imph.csv_geometry()
KS = (0, 1, -1, -1)


@pytest.fixture(scope="module")
def ctx():
    c = s3imph.DeviceBuilder(0)
    yield c
    c.close()


def to_dev(data: bytes, align: int = 0):
    """The text `align` bytes into its allocation, readable up to round_up(len, 8) from its start;
    every byte around it is poison."""
    import torch
    n = len(data)
    raw = np.full(align + (n + 7) // 8 * 8 + 8, 0xA5, np.uint8)
    raw[align:align + n] = np.frombuffer(data, np.uint8)
    return torch.from_numpy(raw).to("cuda")[align:]


def check(ctx, data: bytes, schema=KS, align: int = 0):
    """plan + fill of one buffer against the reference; returns the reference's records."""
    import torch
    want = C.records(data, schema)
    d_csv = to_dev(data, align)
    info = ctx.csv_plan(d_csv, len(data), schema)
    assert info == want["info"]
    blob, offs = C.listing(want)
    n = len(want["keys"])
    d_keys = torch.full((len(blob) + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    d_offs = torch.full((n + 2,), -1, dtype=torch.int64, device="cuda")
    d_sizes = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    d_tiers = torch.full((n + 1,), 0xEE, dtype=torch.uint8, device="cuda")
    ctx.csv_fill(d_keys, d_offs, d_sizes, d_tiers, keys_cap=len(blob))
    keys = d_keys.cpu().numpy().tobytes()
    assert keys[:len(blob)] == blob and keys[len(blob):] == b"\x5a" * 16
    assert d_offs.cpu().numpy().view(np.uint64).tolist() == offs.tolist() + [2**64 - 1]
    assert d_sizes.cpu().numpy().view(np.uint64).tolist() == want["sizes"].tolist() + [2**64 - 1]
    assert d_tiers.cpu().numpy().tolist() == want["tiers"].tolist() + [0xEE]
    return want


def golden():
    out = []
    for group in ("reader", "tiers", "unified", "header"):
        for c in CASES[group]:
            if "records" in c:
                out.append((group + "_" + c["name"], c))
    return out


GOLDEN_CASES = golden()


@pytest.mark.parametrize("name,case", GOLDEN_CASES, ids=[g[0] for g in GOLDEN_CASES])
def test_golden_cases(ctx, name, case):
    data = case["csv"].encode()
    schema = tuple(case["schema"])
    if name.startswith("header_") or case.get("header"):
        found, start = s3imph.csv_header_schema(data)
        assert found[:2] == schema[:2]
        data = data[start:]
    got = check(ctx, data, schema)
    assert [k.decode() for k in got["keys"]] == [r["key"] for r in case["records"]]
    assert got["sizes"].tolist() == [r["size"] for r in case["records"]]
    assert got["tiers"].tolist() == [r["tier"] for r in case["records"]]


# ---------------------------------------------------------------------------------------------
# boundaries of runs and tiles
# ---------------------------------------------------------------------------------------------
def filler(nbytes: int, seed: int = 0) -> bytes:
    """Inventory-like rows, cut to exactly nbytes (the cut may fall anywhere in a row)."""
    rng = random.Random(seed)
    rows = []
    size = 0
    i = 0
    while size < nbytes:
        key = "d%d/s%d/obj-%05d.bin" % (rng.randrange(9), rng.randrange(4), i)
        if i % 7 == 3:
            key = '"%s, ""q"" %d"' % (key, i)
        row = ("%s,%d,%s,\r\n" if i % 5 == 0 else "%s,%d,%s,\n") % (key, rng.randrange(1 << 40), "GLACIER" if i % 3 else "STANDARD")
        rows.append(row.encode())
        size += len(rows[-1])
        i += 1
    return b"".join(rows)[:nbytes]


LENGTHS = [RUN - 1, RUN, RUN + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]


@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_around_a_run_and_a_tile(ctx, n):
    check(ctx, filler(n, seed=n), (0, 1, 2, 3))
    # and ending in each way a buffer can end: inside a quote, after a quote, on '\r', on ','
    for tail in (b'"ab', b'"ab"', b"a,1\r", b"a,", b"a,1\n", b"\n"):
        check(ctx, filler(n - len(tail), seed=n + 1).rsplit(b"\n", 1)[0][:n - len(tail) - 1] + b"\n" + tail, (0, 1, 2, 3))


# (head, tail) of the text just before the event — pad bytes go between them —, the two-byte
# event, and the text after it
EVENTS = {
    "crlf": ((b"", b"abc,12"), b"\r\n", b"next,3\n"),
    "crlf_in_quotes": ((b'"', b"ab"), b"\r\n", b'cd",5\n'),
    "escaped_quote": ((b'"', b"ab"), b'""', b'cd",5\nn,1\n'),
    "quote_comma": ((b'"', b"abc"), b'",', b"7\nn,1\n"),
    "lazy_quote": ((b'"', b"abc"), b'"x', b'yz",3\nn,1\n'),
    "lazy_quote_unquoted": ((b"", b"abc"), b'"x', b"yz,3\nn,1\n"),
    "comma_newline": ((b"", b"abc"), b",\n", b"n,1\n"),
    "cr_not_deleted": ((b"", b"abc"), b"\rx", b",4\nn,1\n"),
    "cr_at_the_end": ((b"", b"abc,1"), b"\r", b""),
}


def place(event: str, at: int) -> bytes:
    """A text whose event's first byte stands at offset `at`."""
    (head, tail), ev, rest = EVENTS[event]
    row = b"key/0001,1\n"
    nrows = (at - len(head) - len(tail)) // len(row)
    pad = at - len(head) - len(tail) - nrows * len(row)
    text = row * nrows + head + b"x" * pad + tail
    assert len(text) == at
    return text + ev + rest


@pytest.mark.parametrize("event", sorted(EVENTS))
@pytest.mark.parametrize("where", ["run", "tile", "second_tile"])
def test_two_byte_events_across_an_edge(ctx, event, where):
    at = {"run": RUN - 1, "tile": TILE - 1, "second_tile": 2 * TILE - 1}[where]
    data = place(event, at)
    want = check(ctx, data)
    assert want["info"]["n_objects"] >= 1
    # the same with the event wholly before and wholly after the edge
    check(ctx, place(event, at - 1))
    check(ctx, place(event, at + 1))


def test_a_quoted_field_open_across_three_tiles(ctx):
    body = (b'line, with "" and ,commas\r\nand more\n' * (2 * TILE // 30))[:2 * TILE + 100]
    body = body.rstrip(b'"').rstrip(b"\r")
    data = filler(TILE - 50, 3).rsplit(b"\n", 1)[0] + b'\n"' + body + b'",77\nlast,1\n'
    want = check(ctx, data)
    assert max(len(k) for k in want["keys"]) > TILE  # and its raw text spans 2 * TILE + 100 bytes
    assert want["keys"][-1] == b"last" and want["sizes"].tolist()[-2:] == [77, 1]


@pytest.mark.parametrize("edge", [RUN, TILE, 2 * TILE], ids=["run", "tile", "second_tile"])
def test_every_state_before_every_kind_of_byte_at_an_edge(ctx, edge):
    """csv_cases.matrix: each of the five states just before the edge, each of the eight things
    that can stand there (test_csv_ref.py proves the texts are what they claim)."""
    objects = 0
    for name, state, at, text in K.matrix(edge):
        try:
            objects += check(ctx, text)["info"]["n_objects"]
        except AssertionError as e:
            raise AssertionError("%s at %d: %s" % (name, at, e)) from e
    assert objects > 55 * (edge // len(K.ROW) - 2)


# ---------------------------------------------------------------------------------------------
# more tiles than k_csv_tile_scan has lanes: a lane composes and walks a share of several tiles
# ---------------------------------------------------------------------------------------------
def test_scan_edges_the_matrix_at_lane_boundaries_of_the_tile_scan(ctx):
    text, placed = K.scan_edges()
    assert len(text) == 1024 * TILE + 1 and len(placed) == 80
    want = check(ctx, text)
    assert want["info"]["n_objects"] > 80000


def test_short_rows_in_1024_and_1025_tiles(ctx):
    """Every lane of the tile scan busy with one tile; then shares of two, the last busy lane with
    one tile and the lanes behind it idle.  About 1.9e5 records and 3.9 MB of keys through the
    record scans, k_csv_meta and the key fill."""
    text = filler(1024 * TILE + 1)
    want = check(ctx, text[:1024 * TILE], (0, 1, 2, 3))
    assert want["info"]["n_objects"] > 150000 and want["info"]["key_bytes"] > 3 * 10**6
    check(ctx, text, (0, 1, 2, 3))


def test_long_rows_three_tiles_per_lane_then_small_plans_on_the_same_scratch(ctx):
    text = K.long_rows()
    assert len(text) == 2048 * TILE + 1
    want = check(ctx, text, (0, 1, 2, 3))
    assert want["info"]["n_objects"] > 20000 and want["info"]["key_bytes"] > 14 * 10**6
    # the scratch of 2049 tiles and its record arrays stay in the context: a plan of one tile and
    # one of three must not read what the large one left past their own tiles and records
    check(ctx, b"k,5\n")
    check(ctx, filler(2 * TILE + 100, seed=21), (0, 1, 2, 3))


# ---------------------------------------------------------------------------------------------
# size fields
# ---------------------------------------------------------------------------------------------
def test_size_fields_on_the_device(ctx):
    text, want = K.sizes_text()
    ref = check(ctx, text)
    assert ref["sizes"].tolist() == [v for _, v, _ in want]
    assert ref["info"]["n_bad_size"] == sum(not ok for _, _, ok in want) > 40


def test_size_literals_on_the_device(ctx):
    """Literals straight from the device's arrays, so that the reference and the device cannot be
    wrong together."""
    rows = [(b"18446744073709551615", 2**64 - 1), (b"18446744073709551616", 0), (b"18446744073709551621", 0),
            (b"+1", 0), (b"0" * 30 + b"5", 5), (b"18446744073709551609", 2**64 - 7), (b"1844674407370955162", 1844674407370955162),
            (b'"\v\f\r\n7 "', 7), (b"99999999999999999999", 0), (b"9223372036854775808", 2**63)]
    text = b"".join(b"k%d,%s\n" % (i, t) for i, (t, _) in enumerate(rows))
    d_csv = to_dev(text)  # the plan keeps its address until the fill
    info = ctx.csv_plan(d_csv, len(text), KS)
    assert info["n_objects"] == info["n_records"] == len(rows) and info["n_bad_size"] == 4
    out = ctx.csv_fill(with_tiers=False)
    assert out["sizes"].cpu().numpy().view(np.uint64).tolist() == [v for _, v in rows]


# ---------------------------------------------------------------------------------------------
# degenerate inputs
# ---------------------------------------------------------------------------------------------
def test_empty_buffer(ctx):
    import torch
    info = ctx.csv_plan(None, 0, KS)
    assert info == dict(n_records=0, n_objects=0, key_bytes=0, n_short=0, n_empty_key=0, n_bad_size=0)
    offs = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    ctx.csv_fill(None, offs, None, None, keys_cap=0)
    assert offs.cpu().tolist() == [0, -1]


@pytest.mark.parametrize("data", [
    b"\n", b"\n\r\n\n\r\n" * 700, b"\r", b"\r\n",                       # only empty lines
    b"only\nshort\nrows\n", b",1\n,2\n", b"a\n,1\nb\n" * 3000,            # every record dropped
    b"a,1\nb,2", b"a,1\nb,2\r", b'a,1\n"b', b'a,1\n"b"', b"a,1\nb,",      # no trailing newline
    b"a,1\r\nb,2\r\n\r", b"a,1\r\r\n", b"\ra,1\n", b"a\r,1\n",            # '\r' kept and deleted
    b'"', b'""', b'"""', b",", b"a", b'a"b,1',
], ids=lambda d: repr(d[:12]))
def test_degenerate_inputs(ctx, data):
    check(ctx, data)


def test_every_record_dropped_fill_writes_the_single_offset(ctx):
    import torch
    data = b"x\ny\n,3\n"
    info = ctx.csv_plan(to_dev(data), len(data), KS)
    assert info["n_objects"] == 0 and info["n_records"] == 3 and info["n_short"] == 2 and info["n_empty_key"] == 1
    offs = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    keys = torch.full((16,), 0x5A, dtype=torch.uint8, device="cuda")
    ctx.csv_fill(keys, offs, None, None, key_base=3, keys_cap=8)
    assert offs.cpu().tolist() == [3, -1]
    assert keys.cpu().numpy().tobytes() == b"\x5a" * 3 + b"\0" * 5 + b"\x5a" * 8


def test_one_record_longer_than_two_tiles(ctx):
    key = (b"part, of\nthe key / " * (2 * TILE // 18 + 8))
    data = b'"' + key + b'",123,GLACIER\n'
    want = check(ctx, data, (0, 1, 2, -1))
    assert want["keys"] == [key] and len(key) > 2 * TILE and want["tiers"].tolist() == [4]


# ---------------------------------------------------------------------------------------------
# fuzz
# ---------------------------------------------------------------------------------------------
def fuzz_inputs(count=300, seed=9157):
    rng = random.Random(seed)
    out = []
    for i in range(count):
        n = rng.randrange(0, 4097) if i % 10 else rng.choice([0, 1, 2, 4095, 4096])
        out.append(K.fuzz_text(rng, n, i % 2 == 1))
    return out


def fuzz_inputs_over_a_tile_edge(count=60, seed=8192):
    """The same two generators at lengths of one to two tiles: whatever they make stands at the
    tile edge, and the text ends anywhere from just before the first edge to just past the second."""
    rng = random.Random(seed)
    ends = [TILE - 64, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 2 * TILE + 64]
    return [K.fuzz_text(rng, rng.randrange(TILE - 64, 2 * TILE + 65) if i % 5 else rng.choice(ends), i % 2 == 1)
            for i in range(count)]


FUZZ_SCHEMAS = [(0, 1, 2, 3), (1, 0, 5, 2)]  # key_col > size_col; storage_col beyond most records


def test_fuzz(ctx):
    kept = 0
    for i, d in enumerate(fuzz_inputs()):
        kept += check(ctx, d, FUZZ_SCHEMAS[i % 2])["info"]["n_objects"]
    assert kept > 1000


def test_fuzz_over_a_tile_edge(ctx):
    inputs = fuzz_inputs_over_a_tile_edge()
    assert len(inputs) == 60 and all(TILE - 64 <= len(d) <= 2 * TILE + 64 for d in inputs)
    kept = 0
    for i, d in enumerate(inputs):
        # both generators under both schemas: the generator alternates with i, the schema with i // 2
        kept += check(ctx, d, FUZZ_SCHEMAS[i // 2 % 2])["info"]["n_objects"]
    assert kept > 1000


# ---------------------------------------------------------------------------------------------
# alignment, append, tiers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", range(1, 8))
def test_misaligned_input(ctx, align):
    check(ctx, filler(TILE + 3 * RUN + align, seed=align), (0, 1, 2, 3), align=align)
    check(ctx, b'"a""b",1\r\n' * 5 + b"z", KS, align=align)


@pytest.mark.parametrize("out_align", [0, 3])
def test_append_two_buffers_into_one_listing(ctx, out_align):
    import torch
    first = filler(TILE + 77, seed=5).rsplit(b"\n", 1)[0] + b'\nk/open,"7 never closed\nb,2\n'
    second = b'c",3\n' + filler(700, seed=6)
    schema = (0, 1, 2, 3)
    a, b = C.records(first, schema), C.records(second, schema)
    # the first buffer ends inside the open quote of its last size field; the second starts anew
    assert a["keys"][-1] == b"k/open" and a["info"]["n_bad_size"] == 1 and b["keys"][0] == b'c"'
    n1, n2 = len(a["keys"]), len(b["keys"])
    blob1, offs1 = C.listing(a)
    kb = int(offs1[-1])
    blob2, offs2 = C.listing(b, key_base=kb)
    total = (kb + b["info"]["key_bytes"] + 7) // 8 * 8
    raw = torch.full((out_align + total + 16,), 0x5A, dtype=torch.uint8, device="cuda")
    d_keys = raw[out_align:]
    d_offs = torch.full((n1 + n2 + 2,), -1, dtype=torch.int64, device="cuda")
    d_sizes = torch.full((n1 + n2,), -1, dtype=torch.int64, device="cuda")
    d_tiers = torch.full((n1 + n2,), 0xEE, dtype=torch.uint8, device="cuda")
    assert ctx.csv_plan(to_dev(first), len(first), schema) == a["info"]
    ctx.csv_fill(d_keys, d_offs, d_sizes, d_tiers, keys_cap=total)
    assert ctx.csv_plan(to_dev(second), len(second), schema) == b["info"]
    ctx.csv_fill(d_keys, d_offs[n1:], d_sizes[n1:], d_tiers[n1:], key_base=kb, keys_cap=total)
    want_blob = blob1[:kb] + blob2
    got = raw.cpu().numpy().tobytes()
    assert got[:out_align] == b"\x5a" * out_align and got[out_align + total:] == b"\x5a" * 16
    assert got[out_align:out_align + total] == want_blob
    assert d_offs.cpu().numpy().view(np.uint64).tolist() == offs1.tolist() + offs2.tolist()[1:] + [2**64 - 1]
    assert d_sizes.cpu().numpy().view(np.uint64).tolist() == a["sizes"].tolist() + b["sizes"].tolist()
    assert d_tiers.cpu().numpy().tolist() == a["tiers"].tolist() + b["tiers"].tolist()


@pytest.mark.parametrize("residue", range(8))
def test_append_at_every_residue_of_key_base(ctx, residue):
    """The second buffer's keys start `residue` bytes into an 8-byte word of the blob: the bytes
    of that word below key_base survive the second fill, zeros pad the end, the poison stays."""
    import torch
    schema = (0, 1, 2, 3)
    first = b"first/" + b"f" * ((residue - 16) % 8) + b",1,GLACIER\nsecond/one,2\n"
    # a key that is written by the re-walk first, then one straight from the text, then many
    second = b'"re""walk",3\nplain,4\n' + filler(RUN * 9 + residue, seed=30 + residue)
    a, b = C.records(first, schema), C.records(second, schema)
    n1, n2 = len(a["keys"]), len(b["keys"])
    blob1, offs1 = C.listing(a)
    kb = int(offs1[-1])
    assert kb % 8 == residue and n1 == 2 and b["keys"][:2] == [b're"walk', b"plain"] and n2 > 5
    blob2, offs2 = C.listing(b, key_base=kb)
    total = (kb + b["info"]["key_bytes"] + 7) // 8 * 8
    for out_align in (0, 5):
        raw = torch.full((out_align + total + 16,), 0x5A, dtype=torch.uint8, device="cuda")
        d_keys = raw[out_align:]
        d_offs = torch.full((n1 + n2 + 2,), -1, dtype=torch.int64, device="cuda")
        d_sizes = torch.full((n1 + n2 + 1,), -1, dtype=torch.int64, device="cuda")
        d_tiers = torch.full((n1 + n2 + 1,), 0xEE, dtype=torch.uint8, device="cuda")
        d_first, d_second = to_dev(first), to_dev(second)
        assert ctx.csv_plan(d_first, len(first), schema) == a["info"]
        ctx.csv_fill(d_keys, d_offs, d_sizes, d_tiers, keys_cap=total)
        got = raw.cpu().numpy().tobytes()
        assert got[out_align:out_align + len(blob1)] == blob1 and set(got[out_align + len(blob1):]) == {0x5A}
        assert ctx.csv_plan(d_second, len(second), schema) == b["info"]
        ctx.csv_fill(d_keys, d_offs[n1:], d_sizes[n1:], d_tiers[n1:], key_base=kb, keys_cap=total)
        got = raw.cpu().numpy().tobytes()
        assert got[:out_align] == b"\x5a" * out_align and got[out_align + total:] == b"\x5a" * 16
        assert got[out_align:out_align + kb] == blob1[:kb]  # the first buffer's keys, those of the shared word too
        assert got[out_align + kb:out_align + total] == blob2 and blob2.endswith(b"\0" * (-(kb + b["info"]["key_bytes"]) % 8))
        assert d_offs.cpu().numpy().view(np.uint64).tolist() == offs1.tolist() + offs2.tolist()[1:] + [2**64 - 1]
        assert d_sizes.cpu().numpy().view(np.uint64).tolist() == a["sizes"].tolist() + b["sizes"].tolist() + [2**64 - 1]
        assert d_tiers.cpu().numpy().tolist() == a["tiers"].tolist() + b["tiers"].tolist() + [0xEE]


def test_every_tier_name_on_the_device(ctx):
    names = [n for _, n, _ in s3imph.TIERS] + ["INTELLIGENT_TIERING", "", "nonsense", "GLACIER_", "x" * 50,
                                                "INTELLIGENT_TIERING_ARCHIVE_INSTANT" + "X" * 10,
                                                "INTELLIGENT_TIERING_ARCHIVE_INSTANTXYZ"]
    access = ["", "FREQUENT_ACCESS", "FREQUENT", "INFREQUENT_ACCESS", "INFREQUENT", "ARCHIVE_INSTANT_ACCESS",
              "ARCHIVE_ACCESS", "ARCHIVE", "DEEP_ARCHIVE_ACCESS", "DEEP_ARCHIVE", "nope", "y" * 70]
    forms = (str, str.lower, lambda t: " \t" + t + " \v", lambda t: t[:3] + " " + t[3:], lambda t: '"%s"' % t)
    rows, want = [], []
    for n in names:
        for a in access:
            for f in forms:
                rows.append("k%d,1,%s,%s\n" % (len(rows), f(n), f(a)))
                want.append(s3imph.tier_from_s3(f(n).strip('"'), f(a).strip('"')))
    rows += ["short%d,1\n" % i for i in range(3)] + ["nocol%d,1,GLACIER\n" % i for i in range(3)]
    want += [0, 0, 0, 4, 4, 4]
    # names whose bytes do not stand contiguous in the text: a CRLF that is trimmed away, one that is
    # not, a "" inside the name, a lazy quote after it; a name of 35 bytes and one byte more
    rows += ['q0,1,"GLACIER\r\n",\n', 'q1,1,"GLA\r\nCIER",\n', 'q2,1,"GLAC""IER",\n', 'q3,1,"GLACIER"x",\n',
             'q4,1,"INTELLIGENT_TIERING\r\n"," \r\nARCHIVE_ACCESS\r\n"\n', 'q5,1,INTELLIGENT_TIERING,"DEEP_""ARCHIVE"\n',
             "q6,1, \tINTELLIGENT_TIERING_ARCHIVE_INSTANT\v ,\n", "q7,1,INTELLIGENT_TIERING_ARCHIVE_INSTANT_,\n"]
    want += [4, 0, 0, 0, 10, 7, 9, 0]
    got = check(ctx, "".join(rows).encode(), (0, 1, 2, 3))
    assert got["tiers"].tolist() == want
    assert set(want) == set(range(s3imph.NUM_TIERS))
    # without the columns every object is STANDARD
    assert set(check(ctx, "".join(rows).encode(), KS)["tiers"].tolist()) == {0}


# ---------------------------------------------------------------------------------------------
# statuses
# ---------------------------------------------------------------------------------------------
def test_fill_without_plan_short_cap_and_plan_without_fill():
    import torch
    c = s3imph.DeviceBuilder(0)
    try:
        keys = torch.empty(64, dtype=torch.uint8, device="cuda")
        offs = torch.empty(8, dtype=torch.int64, device="cuda")
        sizes = torch.empty(8, dtype=torch.int64, device="cuda")
        with pytest.raises(s3imph.MPHFError) as e:
            c.csv_fill(keys, offs, sizes, None, with_tiers=False)
        assert e.value.status == s3imph.ERR_STATE
        data = b"abcdefgh,1\nij,2\n"  # 10 key bytes: 16 with the padding
        d_csv = to_dev(data)
        assert c.csv_plan(d_csv, len(data), KS)["key_bytes"] == 10
        with pytest.raises(s3imph.MPHFError) as e:
            c.csv_fill(keys, offs, sizes, None, keys_cap=15, with_tiers=False)
        assert e.value.status == s3imph.ERR_INVALID and "16" in str(e.value)
        # the plan is still there, and a plan that is never filled is simply replaced
        out = c.csv_fill(keys, offs, sizes, None, keys_cap=16, with_tiers=False)
        assert keys.cpu().numpy().tobytes()[:16] == b"abcdefghij" + b"\0" * 6 and out["tiers"] is None
        c.csv_plan(d_csv, len(data), KS)
        check(c, b"k,5\n")
        s3imph.release_workspaces()
        check(c, b"k,6\nm,7\n")
    finally:
        c.close()


def test_parse_host(ctx):
    data = filler(3 * TILE + 11, seed=12)
    want = C.records(data, (0, 1, 2, 3))
    keys, offs, sizes, tiers, info = s3imph.parse_inventory_csv(data, (0, 1, 2, 3))
    blob, woffs = C.listing(want)
    assert info == want["info"] and keys.tobytes() == blob[:want["info"]["key_bytes"]]
    assert offs.tolist() == woffs.tolist() and sizes.tolist() == want["sizes"].tolist()
    assert tiers.tolist() == want["tiers"].tolist()
    # text without an object
    keys, offs, sizes, tiers, info = s3imph.parse_inventory_csv(b"x\n,1\n", KS)
    assert offs.tolist() == [0] and len(keys) == 0 and info["n_records"] == 2


# ---------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------
STORAGE = {0: ("STANDARD", ""), 1: ("STANDARD_IA", ""), 2: ("ONEZONE_IA", ""), 3: ("GLACIER_IR", ""), 4: ("GLACIER", ""),
           5: ("DEEP_ARCHIVE", ""), 6: ("REDUCED_REDUNDANCY", ""), 7: ("INTELLIGENT_TIERING", "FREQUENT_ACCESS"),
           8: ("INTELLIGENT_TIERING", "INFREQUENT_ACCESS"), 9: ("INTELLIGENT_TIERING", "ARCHIVE_INSTANT_ACCESS"),
           10: ("INTELLIGENT_TIERING", "ARCHIVE_ACCESS"), 11: ("INTELLIGENT_TIERING", "DEEP_ARCHIVE_ACCESS")}


def render(keys, sizes, tiers, eol: bytes) -> list:
    """Headerless inventory rows: bucket, key, size, storage class, access tier."""
    rows = []
    for i, (k, z) in enumerate(zip(keys, sizes)):
        if any(ch in k for ch in b'",\n\r') or i % 11 == 5:
            k = b'"' + k.replace(b'"', b'""') + b'"'
        sc, at = STORAGE[int(tiers[i])] if tiers is not None else ("STANDARD", "")
        rows.append(b"bucket," + k + b",%d,%s,%s" % (int(z), sc.encode(), at.encode()) + eol)
    return rows


def listings():
    out = []
    for c in AGG_CASES:
        out.append(("agg_" + c["name"], [k.encode() for k, _ in c["objects"]], [z for _, z in c["objects"]], None,
                    c["max_depth"]))
    for c in TIER_CASES:
        out.append(("tiers_" + c["name"], [k.encode() for k, _, _ in c["objects"]], [z for _, z, _ in c["objects"]],
                    [t for _, _, t in c["objects"]], 0))
    return out


LISTINGS = listings()


def files_of(d):
    return sorted(os.path.relpath(os.path.join(r, f), d) for r, _, fs in os.walk(d) for f in fs)


@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
@pytest.mark.parametrize("case", LISTINGS, ids=[c[0] for c in LISTINGS])
def test_directory_from_csv_equals_the_one_from_the_listing(tmp_path, case, eol):
    name, keys, sizes, tiers, max_depth = case
    # what CSV cannot carry: an empty key is dropped by the reader, "\r\n" inside a key is normalised
    sel = [i for i, k in enumerate(keys) if k and b"\r\n" not in k and not k.endswith(b"\r")]
    perm = np.random.default_rng(11).permutation(len(sel))
    keys = [keys[sel[i]] for i in perm]
    sizes = [sizes[sel[i]] for i in perm]
    tiers = None if tiers is None else [tiers[sel[i]] for i in perm]
    rows = render(keys, sizes, tiers, eol)
    cut = len(rows) // 2
    files = [b"".join(rows[:cut]), b"".join(rows[cut:])]
    schema = (1, 2, 3, 4)
    ref = C.records(files[0] + files[1], schema)
    assert ref["keys"] == keys and ref["sizes"].tolist() == [int(z) for z in sizes]
    if tiers is not None:
        assert ref["tiers"].tolist() == [int(t) for t in tiers]
    got, want = tmp_path / "got", tmp_path / "want"
    got.mkdir()
    want.mkdir()
    total = s3imph.build_index_from_inventory_csv(files, schema, str(got), with_tiers=tiers is not None,
                                                  max_depth=max_depth)
    assert total == ref["info"]
    blob, offs = O.keys_to_blob(ref["keys"])
    s3imph.build_index_from_unsorted_objects(blob, offs, ref["sizes"], str(want), max_depth=max_depth,
                                             tiers=None if tiers is None else ref["tiers"])
    names = files_of(want)
    assert files_of(got) == names and "manifest.json" in names
    assert any(n.startswith("tier_stats") for n in names) == (tiers is not None and len(keys) > 0)
    for n in names:
        if n != "manifest.json":
            assert (got / n).read_bytes() == (want / n).read_bytes(), n
    a, b = s3imph.read_manifest(str(got)), s3imph.read_manifest(str(want))
    a.pop("created_at")
    b.pop("created_at")
    assert a == b
    s3imph.verify_manifest(str(got))


@pytest.mark.parametrize("with_tiers", [False, True], ids=["plain", "tiers"])
@pytest.mark.parametrize("kind", ["objects", "key_bytes"])
def test_the_appended_listing_grows(tmp_path, kind, with_tiers):
    """csv_listing sizes its arrays from the first file that yields an object; here later files
    yield far more objects (kind "objects": after an empty file, one without an object and a sparse
    one) or far more key bytes at fewer objects than estimated (kind "key_bytes"), so the arrays
    are made anew and copied more than once with files already in them."""
    files = K.growth_files(kind)
    schema = (0, 1, 2, 3)
    g = K.growth_estimate(files, schema)  # the preconditions, as test_csv_ref.py holds them
    if kind == "objects":
        assert g["objects"] > 2.25 * g["est_objects"]
    else:
        assert g["key_bytes"] > 2.25 * g["est_key_bytes"] and g["objects"] <= int(g["est_objects"])
    ref = C.records(b"".join(files), schema)
    each = [C.records(f, schema) for f in files]  # every file is parsed on its own: here that is the same
    assert ref["keys"] == [k for r in each for k in r["keys"]] and len(set(ref["keys"])) == len(ref["keys"])
    assert set(ref["tiers"].tolist()) >= ({0, 4, 5} if kind == "objects" else {2, 3})
    got, want = tmp_path / "got", tmp_path / "want"
    got.mkdir()
    want.mkdir()
    total = s3imph.build_index_from_inventory_csv(files, schema, str(got), with_tiers=with_tiers)
    assert total == {k: sum(r["info"][k] for r in each) for k in ref["info"]}
    blob, offs = O.keys_to_blob(ref["keys"])
    s3imph.build_index_from_unsorted_objects(blob, offs, ref["sizes"], str(want), tiers=ref["tiers"] if with_tiers else None)
    names = files_of(want)
    assert files_of(got) == names and "manifest.json" in names
    assert any(n.startswith("tier_stats") for n in names) == with_tiers
    for n in names:
        if n != "manifest.json":
            assert (got / n).read_bytes() == (want / n).read_bytes(), n
    a, b = s3imph.read_manifest(str(got)), s3imph.read_manifest(str(want))
    a.pop("created_at")
    b.pop("created_at")
    assert a == b
    s3imph.verify_manifest(str(got))


def test_a_lone_quote_in_one_file_does_not_swallow_the_next(tmp_path):
    files = [b'a/x,1\nb/q,"2 never closed\n', b"c/y,3\nd/z,4\n", b"", b"\n"]
    total = s3imph.build_index_from_inventory_csv(files, KS, str(tmp_path))
    assert total["n_objects"] == 4 and total["n_records"] == 4
    with s3imph.Index(str(tmp_path)) as idx:
        assert idx.count == 5  # "", a/, b/, c/, d/
