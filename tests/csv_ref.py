"""CPU reference of the inventory CSV parse (include/s3imph.h section 5g).

Two statements of Go's csv.Reader.readRecord with Comma = ',', LazyQuotes, FieldsPerRecord = -1,
no comment character and TrimLeadingSpace = false, and the reader's rules on top of them:

  parse_lines(data)      the line-based form, readLine + readRecord as encoding/csv writes them:
                         what the GPU is compared with (a different formulation from its kernels);
  parse_automaton(data)  the five-state byte automaton of the header, a second statement;
  state_at(data, offs)   that automaton's state just before given offsets (for generated inputs);
  records(data, schema)  CSVReader.Read's rules (pkg/inventory/reader.go:250-297) over parse_lines.

Go is not on the build machine: both rest on a reading of encoding/csv, and agree with each other
(tests/test_csv_ref.py).
"""
from __future__ import annotations

import numpy as np

from tiers_ref import TIER_TABLE

SPACE = b"\t\n\v\f\r "  # strings.TrimSpace's ASCII set: the library's one trim rule
U64_MAX = (1 << 64) - 1


# ----------------------------------------------------------------------------------------------
# line-based: readLine / readRecord
# ----------------------------------------------------------------------------------------------
class _Lines:
    def __init__(self, data: bytes):
        self.data = data
        self.at = 0
        self.crlf = False  # the last line read ended in '\r\n'

    def read_line(self):
        """(line, eof): readLine — through the next '\\n' or to the end; a '\\r' before the end
        of input is dropped, '\\r\\n' becomes '\\n'."""
        d = self.data
        if self.at >= len(d):
            return b"", True
        nl = d.find(b"\n", self.at)
        end = len(d) if nl < 0 else nl + 1
        line = d[self.at:end]
        self.at = end
        if nl < 0 and line.endswith(b"\r"):
            line = line[:-1]
        self.crlf = len(line) >= 2 and line[-2:] == b"\r\n"
        if self.crlf:
            line = line[:-2] + b"\n"
        return line, False


def _length_nl(line: bytes) -> int:
    return 1 if line.endswith(b"\n") else 0


def _read_record(src: _Lines, trace=None):
    """One record as a list of fields, or None at io.EOF.  trace (a set) collects the constructs
    met on the way, named where readRecord takes the branch that handles them."""
    trace = set() if trace is None else trace
    while True:
        line, eof = src.read_line()
        if eof:
            return None
        if len(line) == _length_nl(line):
            continue  # empty line
        break
    fields = []
    while True:
        if not line.startswith(b'"'):
            i = line.find(b",")
            fields.append(line[:i] if i >= 0 else line[:len(line) - _length_nl(line)])
            if b'"' in fields[-1]:
                trace.add("lazy_in_unquoted")  # a bare quote, kept because of LazyQuotes
            if i >= 0:
                line = line[i + 1:]
                continue
            return fields
        line = line[1:]
        buf = bytearray()
        while True:
            i = line.find(b'"')
            if i >= 0:
                buf += line[:i]
                line = line[i + 1:]
                if line.startswith(b'"'):
                    trace.add("escaped_quote")
                    buf += b'"'
                    line = line[1:]
                elif line.startswith(b","):
                    line = line[1:]
                    fields.append(bytes(buf))
                    break  # next field
                elif _length_nl(line) == len(line):
                    fields.append(bytes(buf))
                    return fields
                else:
                    trace.add("lazy_in_quoted")
                    buf += b'"'  # LazyQuotes: the quote is data
            elif len(line) > 0:
                if src.crlf:
                    trace.add("crlf_in_quotes")
                buf += line
                line, _ = src.read_line()  # at EOF: the empty line, handled below
            else:
                trace.add("unterminated_quote")
                fields.append(bytes(buf))  # abrupt end of input
                return fields


def parse_lines(data: bytes, trace=None) -> list:
    src = _Lines(bytes(data))
    out = []
    while True:
        rec = _read_record(src, trace)
        if rec is None:
            return out
        out.append(rec)


# ----------------------------------------------------------------------------------------------
# the byte automaton
# ----------------------------------------------------------------------------------------------
R, F, U, Q, E = range(5)


def _automaton(data: bytes, probes=()):
    """The one loop behind parse_automaton and state_at: (records, record ends, the state just
    before each offset of `probes`, which must ascend; an offset of len(data) is the final state)."""
    data = bytes(data)
    n = len(data)
    out, ends, fields, cur = [], [], [], bytearray()
    st = R
    seen = []
    probes = list(probes)
    assert probes == sorted(probes) and all(0 <= p <= n for p in probes)
    nxt = probes[0] if probes else -1

    def end_field():
        fields.append(bytes(cur))
        cur.clear()

    for i, c in enumerate(data):
        while i == nxt:
            seen.append(st)
            nxt = probes[len(seen)] if len(seen) < len(probes) else -1
        if c == 0x0D and (i + 1 == n or data[i + 1] == 0x0A):
            continue
        quote, comma, nl = c == 0x22, c == 0x2C, c == 0x0A
        if st == Q:
            if quote:
                st = E
            else:
                cur.append(c)
            continue
        if st == E and (quote or not (comma or nl)):
            cur.append(0x22)
            if not quote:
                cur.append(c)
            st = Q
            continue
        if quote:
            if st == U:
                cur.append(c)
            else:
                st = Q
        elif comma:
            end_field()
            st = F
        elif nl:
            if st != R:
                end_field()
                out.append(fields)
                ends.append(i + 1)
                fields = []
            st = R
        else:
            cur.append(c)
            st = U
    seen += [st] * (len(probes) - len(seen))  # probes at len(data)
    if st != R:
        end_field()
        out.append(fields)
        ends.append(n)
    return out, ends, seen


def parse_automaton(data: bytes, with_ends: bool = False):
    out, ends, _ = _automaton(data)
    return (out, ends) if with_ends else out


def state_at(data: bytes, offsets) -> list:
    """The automaton's state just before each byte offset (a deleted '\\r' leaves it as it is; at
    len(data): the state in which the buffer ends), in the order given.  For tests that must prove
    that a generated input puts what it claims where it claims."""
    offsets = list(offsets)
    order = sorted(range(len(offsets)), key=offsets.__getitem__)
    seen = _automaton(data, [offsets[j] for j in order])[2]
    got = [None] * len(offsets)
    for j, s in zip(order, seen):
        got[j] = s
    return got


# ----------------------------------------------------------------------------------------------
# the reader's rules
# ----------------------------------------------------------------------------------------------
def parse_size(field: bytes):
    """(value, ok): strconv.ParseUint(strings.TrimSpace(field), 10, 64)."""
    t = field.strip(SPACE)
    if not t or any(not (0x30 <= b <= 0x39) for b in t):
        return 0, False
    v = int(t)
    return (v, True) if v <= U64_MAX else (0, False)


_IT_ACCESS = {
    b"FREQUENT_ACCESS": 7, b"FREQUENT": 7, b"INFREQUENT_ACCESS": 8, b"INFREQUENT": 8,
    b"ARCHIVE_INSTANT_ACCESS": 9, b"ARCHIVE_ACCESS": 10, b"ARCHIVE": 10,
    b"DEEP_ARCHIVE_ACCESS": 11, b"DEEP_ARCHIVE": 11,
}
_CLASS = {name.encode(): t for t, (name, _) in enumerate(TIER_TABLE)}


def _trim_upper(b: bytes) -> bytes:
    return bytes(c - 32 if 0x61 <= c <= 0x7A else c for c in b.strip(SPACE))


def tier_of(storage: bytes, access: bytes) -> int:
    """Mapping.FromS3 (pkg/tiers/tiers.go:85-115) on field bytes, with the ASCII trim."""
    sc, at = _trim_upper(storage), _trim_upper(access)
    if sc == b"INTELLIGENT_TIERING":
        return _IT_ACCESS.get(at, 7)
    return _CLASS.get(sc, 0)


def records(data: bytes, schema, parse=parse_lines) -> dict:
    """CSVReader.Read over the whole buffer.  schema = (key_col, size_col, storage_col,
    access_tier_col).  Returns keys (list of bytes), sizes (uint64), tiers (uint8), info (dict of
    s3imph_csv_info's fields)."""
    kc, sc, stc, atc = schema
    keys, sizes, tiers = [], [], []
    info = dict(n_records=0, n_objects=0, key_bytes=0, n_short=0, n_empty_key=0, n_bad_size=0)
    for f in parse(data):
        info["n_records"] += 1
        if len(f) <= kc or len(f) <= sc:
            info["n_short"] += 1
            continue
        if f[kc] == b"":
            info["n_empty_key"] += 1
            continue
        v, ok = parse_size(f[sc])
        info["n_bad_size"] += not ok
        keys.append(f[kc])
        sizes.append(v)
        tiers.append(tier_of(f[stc] if 0 <= stc < len(f) else b"", f[atc] if 0 <= atc < len(f) else b""))
    info["n_objects"] = len(keys)
    info["key_bytes"] = sum(len(k) for k in keys)
    return dict(keys=keys, sizes=np.array(sizes, dtype=np.uint64), tiers=np.array(tiers, dtype=np.uint8), info=info)


def listing(rec: dict, key_base: int = 0):
    """The listing arrays of a records() result: the key blob padded with zeros to a multiple of 8
    (counted from the blob's start, the keys standing from key_base on) and the n + 1 offsets."""
    offs = np.zeros(len(rec["keys"]) + 1, dtype=np.uint64)
    offs[0] = key_base
    if rec["keys"]:
        offs[1:] = key_base + np.cumsum([len(k) for k in rec["keys"]], dtype=np.uint64)
    end = int(offs[-1])
    body = b"".join(rec["keys"])
    return body + b"\0" * (-end % 8), offs


def header_schema(data: bytes):
    """OpenFileWithOptions' column search (reader.go:96-135): (schema, data_start) or the error
    text."""
    recs, ends = parse_automaton(data, with_ends=True)
    if not recs:
        return "read CSV header: EOF"
    cols = {"key": -1, "size": -1, "storageclass": -1, "intelligenttieringaccesstier": -1}
    for i, col in enumerate(recs[0]):
        name = bytes(b + 32 if 0x41 <= b <= 0x5A else b for b in col.strip(SPACE))
        try:
            name = name.decode("ascii")
        except UnicodeDecodeError:
            continue
        if name in cols:
            cols[name] = i
    if cols["key"] < 0:
        return "CSV header missing 'Key' column"
    if cols["size"] < 0:
        return "CSV header missing 'Size' column"
    return (cols["key"], cols["size"], cols["storageclass"], cols["intelligenttieringaccesstier"]), ends[0]
