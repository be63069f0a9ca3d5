"""Listings, chunkings and host run layouts for the chunked build and the host row merge (no GPU;
include/s3imph.h section 5i).  tests/test_rowset_cases.py proves on the CPU that the reference
model is closed under every chunking made here — the chunks' reference rows, merged by
merge_ref.merge_heap in chunk order, are the reference rows of the whole listing — which is what
entitles tests/test_gpu_rowset.py to compare a chunked build with the whole-listing reference.

  small()        about 3 000 objects in named segments, each built for one chunk shape;
  deep()         one key 100 directories deep, its shallow ancestors in another chunk;
  case(name)     a Case: chunks (how they are fed, their objects), max_depth, the tier switch;
  layout_run()   one run of rows as an s3imph.RowRun in a chosen memory layout;
  decode_run()   the rows such a RowRun describes, read the way the header defines the layout."""
import ctypes
from functools import lru_cache

import numpy as np

import merge_ref as M
import s3imph
import tiers_ref as T

# storage classes whose tier id needs no access-tier column (tiers.go:85-115)
CLASSES = ["STANDARD", "STANDARD_IA", "ONEZONE_IA", "GLACIER_IR", "GLACIER", "DEEP_ARCHIVE", "REDUCED_REDUNDANCY"]
SCHEMA = (1, 2, 3, -1)  # bucket,key,size,storage class
SEGMENTS = ("bulk", "again", "sorted", "reverse", "one", "flat", "empty")
# every record of this buffer is dropped by the reader's rules (reader.go:250-297): too few fields
# for the key or the size column, or an empty key
CSV_ALL_DROPPED = b"bucket\nbucket,\nbucket,,5,STANDARD\n\nbucket,\"\",7,GLACIER\nx\n"


class Chunk:
    """One add_* call: how = "objects" | "csv" | "rows"; its objects (none for `raw` CSV)."""

    def __init__(self, how, keys, sizes, tiers, raw=None):
        self.how, self.keys, self.raw = how, list(keys), raw
        self.sizes, self.tiers = np.asarray(sizes, np.uint64), np.asarray(tiers, np.uint8)

    def csv(self):
        if self.raw is not None:
            return self.raw
        return b"".join(b"bucket,%s,%d,%s\n" % (k, int(z), CLASSES[t].encode())
                        for k, z, t in zip(self.keys, self.sizes, self.tiers))


class Case:
    def __init__(self, name, chunks, max_depth=0, with_tiers=True):
        self.name, self.chunks, self.max_depth, self.with_tiers = name, chunks, max_depth, with_tiers

    def objects(self):
        """The concatenation of the chunks: (keys, sizes, tiers)."""
        keys = [k for c in self.chunks for k in c.keys]
        return (keys, np.concatenate([c.sizes for c in self.chunks] + [np.zeros(0, np.uint64)]),
                np.concatenate([c.tiers for c in self.chunks] + [np.zeros(0, np.uint8)]))

    def chunk_rows(self):
        """Each chunk's reference rows, in chunk order (a chunk without an object: no rows)."""
        return [T.aggregate_dict_tiers(c.keys, c.sizes, c.tiers, self.max_depth) if c.keys else []
                for c in self.chunks]

    def ref_key(self):
        """Cases with equal keys here share their whole-listing reference."""
        keys, sizes, tiers = self.objects()
        return (hash((tuple(keys), sizes.tobytes(), tiers.tobytes())), self.max_depth)


def _random_keys(rng, m, top=12):
    keys = set()
    while len(keys) < m:
        depth = int(rng.integers(0, 6))
        dirs = [b"d%02d" % int(rng.integers(0, top))] + [b"s%d" % int(rng.integers(0, 3)) for _ in range(depth)]
        keys.add(b"/".join(dirs[:depth]) + (b"/" if depth else b"") + b"obj-%04d.bin" % int(rng.integers(0, 3000)))
    return sorted(keys)


@lru_cache(maxsize=None)
def small():
    """{segment: (keys, sizes, tiers)}.  bulk: 2 400 distinct keys, shuffled.  again: 100 of
    bulk's keys, each twice.  sorted / reverse: keys in ascending / descending byte order.  one: a
    single object.  flat: keys without '/'.  empty: empty keys."""
    rng = np.random.default_rng(61)
    pool = _random_keys(rng, 2650)
    pool = [pool[i] for i in rng.permutation(len(pool))]
    bulk, rest = pool[:2400], pool[2400:]
    again = [bulk[i] for i in rng.choice(len(bulk), 100, replace=False)] * 2
    again = [again[i] for i in rng.permutation(len(again))]
    seg = {"bulk": bulk, "again": again, "sorted": sorted(rest[:150] + [b"x/%03d" % i for i in range(20)]),
           "reverse": sorted(rest[150:] + [b"x/y/%03d" % i for i in range(20)], reverse=True),
           "one": [b"x/y/z/only"], "flat": [b"top-%02d" % i for i in range(20)], "empty": [b""] * 10}
    out = {}
    for name in SEGMENTS:
        n = len(seg[name])
        sizes = rng.integers(0, 1 << 44, n, dtype=np.uint64)
        sizes[::7] = 0
        out[name] = (seg[name], sizes, rng.integers(0, len(CLASSES), n).astype(np.uint8))
    return out


def _take(seg, lo=None, hi=None):
    keys, sizes, tiers = seg
    return keys[lo:hi], sizes[lo:hi], tiers[lo:hi]


def _concat(parts):
    return ([k for p in parts for k in p[0]], np.concatenate([p[1] for p in parts]),
            np.concatenate([p[2] for p in parts]))


def _even(objects, k, how="objects"):
    """k chunks of (nearly) equal size, none empty."""
    keys, sizes, tiers = objects
    cuts = [len(keys) * i // k for i in range(k + 1)]
    return [Chunk(how, keys[lo:hi], sizes[lo:hi], tiers[lo:hi]) for lo, hi in zip(cuts, cuts[1:])]


def shaped(how="objects", segments=SEGMENTS, dropped_at=None):
    """One chunk per segment (bulk in two), optionally the all-dropped CSV buffer as chunk `dropped_at`."""
    s = small()
    chunks = []
    for name in segments:
        if name == "bulk":
            chunks += [Chunk(how, *_take(s[name], 0, 1100)), Chunk(how, *_take(s[name], 1100))]
        else:
            chunks.append(Chunk(how, *s[name]))
    if dropped_at is not None:
        chunks.insert(dropped_at, Chunk("csv", [], [], [], raw=CSV_ALL_DROPPED))
    return chunks


def whole_small():
    return _concat([small()[name] for name in SEGMENTS])


DEEP_KEY = b"deep/" + b"x/" * 99 + b"obj"


@lru_cache(maxsize=None)
def deep():
    """Two chunks: 300 ordinary objects and the ancestors deep/, deep/x/ as objects' directories;
    then the one key with 100 '/'."""
    rng = np.random.default_rng(67)
    keys = _random_keys(rng, 300, top=4) + [b"deep/a", b"deep/x/b", b"deep/x/x/c"]
    keys = [keys[i] for i in rng.permutation(len(keys))]
    sizes = rng.integers(0, 1 << 40, len(keys) + 1, dtype=np.uint64)
    tiers = rng.integers(0, len(CLASSES), len(keys) + 1).astype(np.uint8)
    return [Chunk("objects", keys, sizes[:-1], tiers[:-1]), Chunk("objects", [DEEP_KEY], sizes[-1:], tiers[-1:])]


EXTRA = ([b"x/late", b"d00/s0/late", b"late", b"x/y/z/only"], np.array([5, 0, 1 << 40, 9], np.uint64),
         np.array([6, 0, 3, 3], np.uint8))


@lru_cache(maxsize=None)
def _cases():
    no_empty = tuple(s for s in SEGMENTS if s != "empty")  # the CSV reader drops records with an empty key
    rows130 = _even(whole_small(), 66, "rows")
    hole = [Chunk("rows", [], [], []) for _ in range(64)]
    cases = [
        Case("shapes", shaped(dropped_at=3)),
        Case("depth 1", shaped(), max_depth=1),
        Case("depth 3 no tiers", shaped(), max_depth=3, with_tiers=False),
        Case("no tiers", _even(whole_small(), 3), with_tiers=False),
        Case("csv no tiers", shaped("csv", no_empty, dropped_at=2), with_tiers=False),
        Case("csv depth 1", shaped("csv", no_empty, dropped_at=0), max_depth=1),
        Case("65 chunks", _even(whole_small(), 65)),
        Case("130 chunks", _even(whole_small(), 130)),
        Case("130 runs with 64 empty", rows130[:64] + hole + rows130[64:]),
        Case("deep", list(deep())),
        Case("extended", shaped() + [Chunk("objects", *EXTRA)]),
    ]
    return {c.name: c for c in cases}


NAMES = ("shapes", "depth 1", "depth 3 no tiers", "no tiers", "csv no tiers", "csv depth 1", "65 chunks",
         "130 chunks", "130 runs with 64 empty", "deep", "extended")


def case(name):
    return _cases()[name]


@lru_cache(maxsize=None)
def whole_rows(name):
    """The reference rows of the case's whole listing."""
    c = case(name)
    return T.aggregate_dict_tiers(*c.objects(), c.max_depth)


@lru_cache(maxsize=None)
def part_rows(k):
    """The small listing cut into k even parts, each part's reference rows: k runs whose merge is
    whole_rows("shapes")."""
    return [T.aggregate_dict_tiers(c.keys, c.sizes, c.tiers) for c in _even(whole_small(), k)]


# ---- host run layouts ---------------------------------------------------------------------------
JUNK, SLACK = 0xAA, 0x5555555555555555


def layout_run(rows, base=0, tail=3, stride_extra=0, tiers=True, null=False, null_blob=False):
    """rows as an s3imph.RowRun: the key bytes start `base` bytes into a blob filled with 0xAA
    before and (`tail` bytes) after them, the tier columns have a stride of n + stride_extra with
    0x55 in the slack.  null (only for no rows): every pointer NULL.  null_blob (only when every
    key is empty): blob NULL, the offsets all equal to base.  The arrays live as long as the run."""
    blob, offs, depth, cnt, nbytes, tc, tb = M.to_arrays(rows)
    n = len(rows)
    if null:
        assert n == 0
        return s3imph.RowRun(None, None, None, None, None, None, None, 0, 0)
    wide = np.full(base + len(blob) + tail, JUNK, np.uint8)
    wide[base:base + len(blob)] = blob
    offs = offs + np.uint64(base)
    stride = n + stride_extra
    wtc, wtb = np.full((2, M.NUM_TIERS, max(stride, 1)), SLACK, np.uint64)
    wtc[:, :n], wtb[:, :n] = tc, tb
    if null_blob:
        assert len(blob) == 0
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    run = s3imph.RowRun(None if null_blob else ptr(wide), ptr(offs), ptr(depth), ptr(cnt), ptr(nbytes),
                        ptr(wtc) if tiers else None, ptr(wtb) if tiers else None, n, stride if tiers else 0)
    run.arrays = (wide, offs, depth, cnt, nbytes, wtc, wtb)
    return run


def decode_run(run):
    """The rows of a RowRun, read as the header defines it: key i is blob[offsets[i]:offsets[i + 1]],
    tier column t starts at t * tier_stride."""
    n = int(run.n)
    if n == 0:
        return []
    arr = lambda p, ct, count: np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ct)), (count,))  # noqa: E731
    offs = arr(run.offsets, ctypes.c_uint64, n + 1)
    end = int(offs[n])
    blob = bytes(arr(run.blob, ctypes.c_uint8, end)) if run.blob else b""
    depth, cnt = arr(run.depth, ctypes.c_uint32, n), arr(run.count, ctypes.c_uint64, n)
    nb = arr(run.bytes, ctypes.c_uint64, n)
    stride = int(run.tier_stride)
    out = []
    for i in range(n):
        tc, tb = [0] * M.NUM_TIERS, [0] * M.NUM_TIERS
        if run.tier_count:
            tc = [int(v) for v in arr(run.tier_count, ctypes.c_uint64, M.NUM_TIERS * stride)[i::stride][:M.NUM_TIERS]]
            tb = [int(v) for v in arr(run.tier_bytes, ctypes.c_uint64, M.NUM_TIERS * stride)[i::stride][:M.NUM_TIERS]]
        out.append((blob[int(offs[i]):int(offs[i + 1])], int(depth[i]), int(cnt[i]), int(nb[i]), tc, tb))
    return out


def strip_tiers(rows):
    zero = [0] * M.NUM_TIERS
    return [(r[0], r[1], r[2], r[3], zero[:], zero[:]) for r in rows]


ROOT_ONLY = [M.row(b"", 0, 4, 400, {2: (4, 400)})]


def layouts(runs, tiers=True):
    """The logical runs (lists of rows; one whose every key is empty gets a NULL blob) in the
    layouts the header allows, with empty runs first, in the middle and last: (logical runs in
    the order given to the library, the RowRuns).  Bases cycle through 1, 5, 8, 13; every other
    run has tier_stride n + 3; empty runs come once with NULL pointers and once with real empty
    arrays, and one of them disagrees with the others about tier columns."""
    bases = (1, 5, 8, 13)
    logical, out = [], []

    def put(rows, **kw):
        logical.append(rows)
        out.append(layout_run(rows, tiers=kw.pop("tiers", tiers), **kw))

    put([], null=True)
    put([], base=5)
    for i, rows in enumerate(runs):
        if all(len(r[0]) == 0 for r in rows) and rows:
            put(rows, base=7, tail=0, null_blob=True, stride_extra=(i % 2) * 3)
        else:
            put(rows, base=bases[i % 4], stride_extra=(i % 2) * 3)
        if i == len(runs) // 2:
            put([], null=True)
            put([], base=8, tiers=not tiers)  # an empty run counts with neither
    put([], base=13)
    put([], null=True)
    return logical, out
