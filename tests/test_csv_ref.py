"""tests/csv_ref.py against the reference's own reader tests (tests/golden/csv/cases.json) and
against itself: the line-based restatement of encoding/csv and the byte automaton agree on a
seeded fuzz corpus that provably holds every construct the grammar has.  And the preconditions of
the generated inputs in tests/csv_cases.py, which tests/test_gpu_csv.py gives to the device."""
import json
import os
import random

import pytest

import csv_cases as K
import csv_ref as C
from conftest import GOLDEN
from csv_cases import SIZES, TILE

CASES = json.load(open(os.path.join(GOLDEN, "csv", "cases.json")))
ALPHABET = b'",\n\ra 1'


def record_cases():
    out = []
    for group in ("reader", "tiers", "unified", "header"):
        for c in CASES[group]:
            if "records" in c:
                out.append((group, c))
    return out


RECORD_CASES = record_cases()


@pytest.mark.parametrize("group,case", RECORD_CASES, ids=[g + "_" + c["name"] for g, c in RECORD_CASES])
@pytest.mark.parametrize("parse", [C.parse_lines, C.parse_automaton], ids=["lines", "automaton"])
def test_golden_records(group, case, parse):
    data = case["csv"].encode()
    schema = tuple(case["schema"])
    if group == "header" or case.get("header"):
        found, start = C.header_schema(data)
        if case.get("track_tiers", True):
            assert found == schema
        else:
            assert found[:2] == schema[:2]  # the columns are there; the reader was told not to use them
        data = data[start:]
    got = C.records(data, schema, parse)
    want = case["records"]
    assert [k.decode() for k in got["keys"]] == [r["key"] for r in want]
    assert got["sizes"].tolist() == [r["size"] for r in want]
    assert got["tiers"].tolist() == [r["tier"] for r in want]
    assert got["info"]["n_objects"] == len(want)


@pytest.mark.parametrize("case", CASES["header"], ids=[c["name"] for c in CASES["header"]])
def test_golden_headers(case):
    got = C.header_schema(case["csv"].encode())
    if "error" in case:
        assert got == case["error"]
    else:
        assert got[0] == tuple(case["schema"])
        assert case["csv"].encode()[:got[1]].count(b"\n") == 1


def test_header_rules():
    assert C.header_schema(b"") == "read CSV header: EOF"
    assert C.header_schema(b"\n\r\n") == "read CSV header: EOF"
    assert C.header_schema(b"\n\nkey,size") == ((0, 1, -1, -1), 10)
    # the last match wins; quoted names; white space and case
    assert C.header_schema(b'key,"Si""ze",SIZE , storageclass,KEY\n')[0] == (4, 2, 3, -1)
    assert C.header_schema(b" IntelligentTieringAccessTier\t,size,key\r\nx")[0] == (2, 1, -1, 0)


def corpus(n=20000, seed=20240):
    rng = random.Random(seed)
    return [bytes(rng.choice(ALPHABET) for _ in range(rng.randrange(0, 17))) for _ in range(n)]


def features(data: bytes) -> set:
    """Which constructs an input holds, from the line-based reference parser alone: the branches
    of readRecord it took (csv_ref's trace) and what the reader rules dropped."""
    f = set()
    C.parse_lines(data, f)
    info = C.records(data, (0, 1, -1, -1))["info"]
    if info["n_short"]:
        f.add("short_record")
    if info["n_empty_key"]:
        f.add("empty_key")
    return f


def test_the_two_parsers_agree_on_a_corpus_that_holds_every_construct():
    seen = set()
    inputs = corpus()
    assert len(inputs) >= 20000 and all(len(d) <= 16 for d in inputs)
    for d in inputs:
        a, b = C.parse_lines(d), C.parse_automaton(d)
        assert a == b, d
        seen |= features(d)
    assert seen == {"escaped_quote", "lazy_in_unquoted", "lazy_in_quoted", "crlf_in_quotes", "unterminated_quote",
                    "short_record", "empty_key"}


def test_record_ends_of_the_automaton():
    recs, ends = C.parse_automaton(b'a,1\n\n"x\ny",2\r\nz', with_ends=True)
    assert recs == [[b"a", b"1"], [b"x\ny", b"2"], [b"z"]] and ends == [4, 14, 15]


@pytest.mark.parametrize("text,value,ok", SIZES, ids=[repr(s[0])[:24] for s in SIZES])
def test_size_edges(text, value, ok):
    assert C.parse_size(text) == (value, ok)
    got = C.records(b"k," + text.replace(b"\n", b" ") + b"\n", (0, 1, -1, -1))
    want = C.parse_size(text.replace(b"\n", b" "))
    assert got["sizes"].tolist() == [want[0]] and got["info"]["n_bad_size"] == (not want[1])


def test_size_literals():
    """Written out, not computed: the table above and parse_size cannot be wrong together."""
    for text, value, ok in [(b"18446744073709551615", 2**64 - 1, True), (b"18446744073709551616", 0, False),
                            (b"18446744073709551621", 0, False), (b"+1", 0, False), (b"0" * 30 + b"5", 5, True),
                            (b"9223372036854775808", 2**63, True), (b"99999999999999999999", 0, False)]:
        assert (text, value, ok) in SIZES and C.parse_size(text) == (value, ok)
    assert len({s[0] for s in SIZES}) == len(SIZES)
    assert {s[0][-1:] for s in SIZES if len(s[0]) == 20 and s[0].startswith(b"1844674407370955161")} \
        == {b"%d" % d for d in range(10)}


def test_sizes_text_holds_every_entry_three_times():
    text, want = K.sizes_text()
    got = C.records(text, (0, 1, -1, -1))
    assert got["keys"] == [k for k, _, _ in want]
    assert got["sizes"].tolist() == [v for _, v, _ in want]
    assert got["info"]["n_bad_size"] == sum(not ok for _, _, ok in want)
    assert got["info"]["n_records"] == len(want) == 3 * len(SIZES) - 1  # one entry holds a '\n': not bare
    by_key = {k: (v, ok) for k, v, ok in want}
    for i, (entry, value, ok) in enumerate(SIZES):
        for k in [b"bare%02d" % i] * (b"\n" not in entry) + [b"quoted%02d" % i] + [k for k in by_key if k.startswith(b"pad%02d/" % i)]:
            assert by_key[k] == (value, ok), k


# ----------------------------------------------------------------------------------------------
# the generated inputs of tests/csv_cases.py put what they claim where they claim
# ----------------------------------------------------------------------------------------------
def test_state_at():
    # a , " b " " , \n: the '""' is an escape, so the comma and the newline stay inside the quotes
    assert C.state_at(b'a,"b"",\n', range(9)) == [C.R, C.U, C.F, C.Q, C.Q, C.E, C.Q, C.Q, C.Q]
    # a deleted '\r' leaves the state alone; offsets in any order, and twice
    assert C.state_at(b"a\r\nb\r", [5, 3, 2, 1, 0, 4, 3]) == [C.U, C.R, C.U, C.U, C.R, C.U, C.R]
    assert C.state_at(b'"a"x', [3, 4]) == [C.E, C.Q] and C.state_at(b"a\rb,", [2, 4]) == [C.U, C.F]
    assert C.state_at(b"", [0]) == [C.R] and C.state_at(b"abc", []) == []
    # every record of the automaton ends where the state is R again, or at the end of the buffer
    for d in corpus(2000, seed=5):
        recs, ends = C.parse_automaton(d, with_ends=True)
        states = C.state_at(d, ends)
        assert all(s == C.R or e == len(d) for s, e in zip(states, ends)), d
        assert len(recs) == len(ends) and (C.state_at(d, [len(d)]) == [C.R] or ends[-1] == len(d)), d


@pytest.mark.parametrize("edge", [K.RUN, K.TILE, 2 * K.TILE], ids=["run", "tile", "second_tile"])
def test_matrix_puts_each_state_before_each_kind(edge):
    seen, combos = set(), set()
    for name, state, at, text in K.matrix(edge):
        kind = name.split("_", 1)[1].replace("_split", "")
        assert C.state_at(text, [at]) == [state], name
        assert text[at:at + len(K.KINDS[kind])] == K.KINDS[kind], name
        assert (len(text) == at + len(K.KINDS[kind])) == (kind in K.EOF_KINDS), name
        assert text.endswith(K.TAIL) or kind in K.EOF_KINDS
        assert at in (edge, edge - 1)
        assert C.parse_lines(text, seen) == C.parse_automaton(text), name
        combos.add((state, kind, edge - at))
    assert {(s, k) for s, k, shift in combos if shift == 0} == {(s, k) for s in K.STATES for k in K.KINDS}
    assert {(s, k) for s, k, shift in combos if shift == 1} == {(s, k) for s in K.STATES for k in K.SPLIT_KINDS}
    assert len(K.STATES) * len(K.KINDS) == 40
    assert seen == {"escaped_quote", "lazy_in_unquoted", "lazy_in_quoted", "crlf_in_quotes", "unterminated_quote"}


def test_scan_edges_puts_the_matrix_on_lane_boundaries_and_inside_lanes():
    text, placed = K.scan_edges()
    nt = -(-len(text) // TILE)
    assert len(text) == K.SCAN_LANES * TILE + 1 and nt == 1025 and -(-nt // K.SCAN_LANES) == 2
    assert C.state_at(text, [at for at, _, _, _ in placed]) == [state for _, state, _, _ in placed]
    combos = set()
    for at, state, k, kind in placed:
        assert text[at:at + len(K.KINDS[kind])] == K.KINDS[kind] and k * TILE - at in (0, 1) and 0 < k < nt
        combos.add((state, kind, k % 2, k * TILE - at))
    plain = {(s, k) for s in K.STATES for k in K.KINDS if k not in K.EOF_KINDS}
    two = {(s, k) for s, k in plain if len(K.KINDS[k]) == 2}
    assert len(plain) == 30 and len(two) == 10
    assert combos == {(s, k, par, 0) for s, k in plain for par in (0, 1)} | {(s, k, par, 1) for s, k in two for par in (0, 1)}


def test_long_rows_enter_tiles_in_every_state_at_and_off_a_lane_boundary():
    text = K.long_rows()
    nt = -(-len(text) // TILE)
    assert nt == 2049 and -(-nt // K.SCAN_LANES) == 3
    entry = C.state_at(text, [k * TILE for k in range(nt)])
    for s in K.STATES:
        ks = [k for k in range(1, nt) if entry[k] == s]
        assert any(k % 3 == 0 for k in ks) and any(k % 3 for k in ks), (K.STATE_NAMES[s], ks[:10])
    keys = C.records(text[:200000], (0, 1, 2, 3))["keys"]
    assert sum(len(k) > 800 and b'"' in k and b"," in k and b"\n" in k for k in keys) > 100


@pytest.mark.parametrize("kind", ["objects", "key_bytes"])
def test_growth_files_outgrow_the_first_estimate(kind):
    files = K.growth_files(kind)
    g = K.growth_estimate(files, (0, 1, 2, 3))
    # more than 1.5 x twice over: an array that grows by half has to grow more than once
    if kind == "objects":
        infos = [C.records(f, (0, 1, 2, 3))["info"] for f in files]
        assert [i["n_objects"] for i in infos[:3]] == [0, 0, 2] and infos[1]["n_records"] == 80 and len(files[0]) == 0
        assert [len(f) for f in files[2:]] == [4096] * 4 and infos[2]["n_short"] > 4
        assert g["objects"] > 2.25 * g["est_objects"]
    else:
        assert g["key_bytes"] > 2.25 * g["est_key_bytes"] and g["objects"] <= int(g["est_objects"])
    allkeys = C.records(b"".join(files), (0, 1, 2, 3))["keys"]
    assert len(set(allkeys)) == len(allkeys) == g["objects"]


def test_tier_rule():
    assert C.tier_of(b" glacier\t", b"") == 4
    assert C.tier_of(b"INTELLIGENT_TIERING", b"") == 7
    assert C.tier_of(b"intelligent_tiering", b" Deep_Archive_Access ") == 11
    assert C.tier_of(b"INTELLIGENT_TIERING_FREQUENT", b"") == 7
    assert C.tier_of(b"nonsense", b"ARCHIVE") == 0


def test_listing_layout():
    rec = C.records(b"ab,1\ncde,2\n", (0, 1, -1, -1))
    blob, offs = C.listing(rec)
    assert blob == b"abcde\0\0\0" and offs.tolist() == [0, 2, 5]
    blob, offs = C.listing(rec, key_base=6)
    assert blob == b"abcde" + b"\0" * 5 and offs.tolist() == [6, 8, 11]
