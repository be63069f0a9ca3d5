"""tests/csv_ref.py against the reference's own reader tests (tests/golden/csv/cases.json) and
against itself: the line-based restatement of encoding/csv and the byte automaton agree on a
seeded fuzz corpus that provably holds every construct the grammar has."""
import json
import os
import random

import pytest

import csv_ref as C
from conftest import GOLDEN

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


SIZES = [
    (b"18446744073709551615", 18446744073709551615, True),
    (b"18446744073709551616", 0, False),
    (b"+1", 0, False), (b"-0", 0, False), (b"1_0", 0, False),
    (b" 12\t", 12, True), (b"\v\f\r\n7 ", 7, True),
    (b"0" * 30 + b"5", 5, True), (b"", 0, False), (b"  ", 0, False), (b"1 2", 0, False),
    (b"\xc2\xa012", 0, False),  # U+00A0: the reference would trim it; the library's ASCII rule does not
]


@pytest.mark.parametrize("text,value,ok", SIZES, ids=[repr(s[0])[:24] for s in SIZES])
def test_size_edges(text, value, ok):
    assert C.parse_size(text) == (value, ok)
    got = C.records(b"k," + text.replace(b"\n", b" ") + b"\n", (0, 1, -1, -1))
    want = C.parse_size(text.replace(b"\n", b" "))
    assert got["sizes"].tolist() == [want[0]] and got["info"]["n_bad_size"] == (not want[1])


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
