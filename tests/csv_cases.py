"""Generated inventory CSV inputs that both tests/test_csv_ref.py (on the CPU: does the input put
what it claims where it claims?) and tests/test_gpu_csv.py (the device against csv_ref) import.
A plain module: no fixtures, no test collection."""
import random

import csv_ref as C
import s3imph

RUN, TILE = s3imph.csv_geometry()
STATE_NAMES = {C.R: "R", C.F: "F", C.U: "U", C.Q: "Q", C.E: "E"}
STATES = sorted(STATE_NAMES)

# ----------------------------------------------------------------------------------------------
# size fields: (text, value, ok) of strconv.ParseUint(strings.TrimSpace(text), 10, 64)
# ----------------------------------------------------------------------------------------------
SIZES = [
    (b"18446744073709551615", 18446744073709551615, True),
    (b"18446744073709551616", 0, False),
    (b"+1", 0, False), (b"-0", 0, False), (b"1_0", 0, False),
    (b" 12\t", 12, True), (b"\v\f\r\n7 ", 7, True),
    (b"0" * 30 + b"5", 5, True), (b"", 0, False), (b"  ", 0, False), (b"1 2", 0, False),
    (b"\xc2\xa012", 0, False),  # U+00A0: the reference would trim it; the library's ASCII rule does not
]
# one value per last digit on either side of the limit (…615 and …616 stand above)
SIZES += [(b"%d" % v, v if v < 2**64 else 0, v < 2**64) for v in range(2**64 - 6, 2**64 + 4) if v not in (2**64 - 1, 2**64)]
SIZES += [
    (b"9223372036854775808", 2**63, True),
    (b"9" * 19, 10**19 - 1, True), (b"9" * 20, 0, False),
    (b"18446744073709551621", 0, False),  # 2^64 + 5: a wrapped sum would read 5
    (b"123456789012345678901234567890123456789", 0, False),
    (b"00", 0, True), (b"1\t\t", 1, True),
    ("٣".encode(), 0, False),  # ARABIC-INDIC DIGIT THREE: ParseUint takes ASCII digits only
    (b"1e3", 0, False), (b"0x10", 0, False), (b"1.0", 0, False),
]


def sizes_text():
    """(text, want): every SIZES entry as the size of an object in three renderings — bare (not
    the entry that holds a '\\n'), quoted, and behind a key padded so that the field straddles a
    multiple of RUN — and what the reader makes of each: (key, value, ok) per object."""
    out, want = bytearray(), []

    def row(key: bytes, field: bytes, text: bytes):
        out.extend(key + b"," + field + b"\n")
        v, ok = C.parse_size(text)  # '\r\n' inside quotes reaches the field as '\n': white space either way
        want.append((key, v, ok))

    for i, (text, _, _) in enumerate(SIZES):
        if b"\n" not in text:
            row(b"bare%02d" % i, text, text)
        row(b"quoted%02d" % i, b'"' + text + b'"', text)
        # the field's middle byte on a multiple of RUN
        key = b"pad%02d/" % i
        start = len(out) + len(key) + 2  # behind the key, the comma and the opening quote
        key += b"p" * (-(start + len(text) // 2) % RUN)
        assert (len(out) + len(key) + 2 + len(text) // 2) % RUN == 0
        row(key, b'"' + text + b'"', text)
    return bytes(out), want


# ----------------------------------------------------------------------------------------------
# a state, then a kind of byte, at a chosen offset
# ----------------------------------------------------------------------------------------------
ROW = b"key/0001,1\n"
# (head, tail) of the text that leaves the automaton in each state: pad bytes go between them
REACH = {C.R: (b"", b"\n"), C.F: (b"", b","), C.U: (b"", b"abc"), C.Q: (b'"', b"ab"), C.E: (b'"', b'ab"')}
KINDS = {"quote": b'"', "comma": b",", "nl": b"\n", "other": b"x", "crlf": b"\r\n", "cr_other": b"\rx",
         "cr_eof": b"\r", "eof": b""}
EOF_KINDS = ("cr_eof", "eof")
SPLIT_KINDS = ("crlf", "cr_other", "cr_eof")  # two bytes (the end of the buffer counting as one): also placed one byte early
# closes a quote if one is open and ends the record from any state; then two plain rows, so that a
# wrong state shifts later records too
TAIL = b'q",9\nn,1\nm,2\n'


def reach(state: int, nbytes: int, row: bytes = ROW) -> bytes:
    """nbytes of text from a record start: whole rows, then the way into `state` with 'x' padding."""
    head, tail = REACH[state]
    nrows = (nbytes - len(head) - len(tail)) // len(row)
    pad = nbytes - len(head) - len(tail) - nrows * len(row)
    assert nrows >= 0
    return row * nrows + head + b"x" * pad + tail


def at_edge(state: int, kind: str, at: int) -> bytes:
    """A text that is in `state` just before offset `at`, where the first byte of `kind` stands."""
    text = reach(state, at) + KINDS[kind]
    return text if kind in EOF_KINDS else text + TAIL


def matrix(edge: int):
    """(id, state, offset of the kind's first byte, text) for the 5 states x 8 kinds at `edge`,
    the kinds of SPLIT_KINDS once more one byte early so that the edge splits them."""
    for state in STATES:
        for kind in KINDS:
            for shift in (0, 1) if kind in SPLIT_KINDS else (0,):
                yield "%s_%s%s" % (STATE_NAMES[state], kind, "_split" if shift else ""), state, edge - shift, \
                    at_edge(state, kind, edge - shift)


# ----------------------------------------------------------------------------------------------
# more tiles than the tile scan has lanes
# ----------------------------------------------------------------------------------------------
SCAN_LANES = 1024  # k_csv_tile_scan's workgroup: lane t takes tiles [t * share, (t + 1) * share), share = ceil(nt / 1024)
PAD_ROW = b"pad/" + b"p" * 89 + b",1\n"


def scan_edges():
    """(text, placed): 1025 tiles (share 2: every even tile edge is a lane boundary of the tile
    scan, every odd one lies inside a lane's share).  The 30 state x kind combinations that do not
    end the buffer, the first byte of each on a tile edge — once an even, once an odd one —, the
    two-byte kinds once more one byte before such edges.  placed: (offset of the kind's first
    byte, state there, tile edge, kind)."""
    events = [(state, kind, parity, shift) for parity in (0, 1) for shift in (0, 1) for state in STATES
              for kind in KINDS if kind not in EOF_KINDS and (not shift or len(KINDS[kind]) == 2)]
    assert len(events) == 2 * 30 + 2 * 10
    parts, pos, placed = [], 0, []
    for j, (state, kind, parity, shift) in enumerate(events):
        k = 2 + 12 * j + parity
        at = k * TILE - shift
        parts.append(reach(state, at - pos, PAD_ROW) + KINDS[kind] + TAIL)
        pos += len(parts[-1])
        placed.append((at, state, k, kind))
    total = SCAN_LANES * TILE + 1
    assert pos < total
    parts.append((PAD_ROW * ((total - pos) // len(PAD_ROW) + 1))[:total - pos])
    return b"".join(parts), placed


def long_rows(nbytes: int = 2 * SCAN_LANES * TILE + 1, seed: int = 4104) -> bytes:
    """2049 tiles (share 3) of rows whose quoted keys of about 1 KiB hold commas, newlines, '""'
    and CRLF; every row an odd number of bytes, so tile edges fall at every phase of a row; every
    other one followed by short rows and empty lines."""
    rng = random.Random(seed)
    tokens = [b"part/of the key ", b"d%d/" % 7, b"obj-000123.bin", b", ", b",", b"\n", b'""', b'""', b'""', b"\r\n",
              b"long run of plain key bytes without anything in them at all / "]
    rows, size, i = [], 0, 0
    while size < nbytes:
        body = bytearray()
        target = rng.randrange(900, 1100)
        while len(body) < target:
            body += rng.choice(tokens)
        row = b'"' + bytes(body) + b'",%d,%s,%s,,,,,,,,' % (rng.randrange(1 << 40), b"GLACIER" if i % 3 else b"intelligent_tiering",
                                                        b"ARCHIVE_ACCESS" if i % 2 else b"")
        row += b"\n" if (len(row) + 1) % 2 else b"\r\n"
        assert len(row) % 2 == 1
        if i % 2 == 1:
            row += b"s/%d,%d\n\n\n\r\n\n\n\n\n,,,\nplain/key/%d,7,STANDARD_IA\n" % (i, i, i)
        rows.append(row)
        size += len(row)
        i += 1
    return b"".join(rows)[:nbytes]


# ----------------------------------------------------------------------------------------------
# files that make the appended listing grow
# ----------------------------------------------------------------------------------------------
def _fill_to(rows: bytes, nbytes: int, drop: bytes) -> bytes:
    """rows, then dropped rows (one field each) up to exactly nbytes."""
    out = rows
    while len(out) + len(drop) + 1 <= nbytes:
        out += drop + b"\n"
    rest = nbytes - len(out)
    return out + (b"d" * (rest - 1) + b"\n" if rest else b"")


def growth_files(kind: str) -> list:
    """The files of the two growth tests, in order (schema 0, 1, 2, 3)."""
    if kind == "objects":
        long_drop = b"dropped row of one field " * 16
        sparse = b"a/first,10,GLACIER\n" + (long_drop + b"\n") * 3 + b"," + long_drop + b",5\n" + b"a/second,20,DEEP_ARCHIVE\n"
        dense = [_fill_to(b"".join(b"k%05d,1\n" % (500 * f + i) for i in range(4096 // 9)), 4096, b"") for f in range(3)]
        return [b"", b"short\n,1\nonly\r\n,2,STANDARD\n" * 20, _fill_to(sparse, 4096, long_drop)] + dense
    assert kind == "key_bytes"
    one = [bytes([c]) for c in range(0x21, 0x7F) if chr(c) not in '",/']
    first = b"".join(k + b",1,ONEZONE_IA\n" for k in one)
    rest = [b"".join(b"big/%d/%d/" % (f, j) + b"%d" % (f + j) * 2040 + b",%d,GLACIER_IR\n" % (2048 + j) for j in range(2))
            for f in range(4)]
    return [first] + rest


def growth_estimate(files, schema) -> dict:
    """What csv_listing's sizing rule makes of the files, from the reference alone.  The rule, as
    s3imph_csv.hip writes it: the first file that yields an object sizes the arrays, with
    1.05 x its objects (its key bytes) x the bytes from that file on / its own length; after that
    an array grows to what it needs or by half, whichever is more.  A change of the rule changes
    this function with it."""
    infos = [C.records(f, schema)["info"] for f in files]
    first = next(i for i, x in enumerate(infos) if x["n_objects"])
    scale = 1.05 * sum(len(f) for f in files[first:]) / len(files[first])
    return dict(est_objects=infos[first]["n_objects"] * scale, est_key_bytes=infos[first]["key_bytes"] * scale,
                objects=sum(x["n_objects"] for x in infos), key_bytes=sum(x["key_bytes"] for x in infos))


# ----------------------------------------------------------------------------------------------
# fuzz
# ----------------------------------------------------------------------------------------------
FUZZ_ALPHABET = b'",\n\ra 1/\x80'
FUZZ_TOKENS = [b",", b",", b"\n", b"\r\n", b'"', b'""', b"a/b", b"17", b" 5 ", b"GLACIER", b"x\x80y", b"\r", b' "q" ',
               b"STANDARD_IA", b"intelligent_tiering", b"ARCHIVE"]


def fuzz_text(rng, n: int, by_bytes: bool) -> bytes:
    """The two generators of the fuzz sets: n bytes drawn one by one, or tokens cut at n."""
    if by_bytes:
        return bytes(rng.choice(FUZZ_ALPHABET) for _ in range(n))
    d = bytearray()
    while len(d) < n:
        d += rng.choice(FUZZ_TOKENS)
    return bytes(d[:n])
