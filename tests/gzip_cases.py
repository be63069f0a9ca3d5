"""The gzip files the inflate tests share (section 5j of include/s3imph.h): every case names the
status it must end with and carries the edge it is meant to hit as a predicate on gzip_ref's trace,
which test_gzip_ref.py checks on the CPU, so that the GPU tests know their inputs reach the paths
they are there for.  Shapes follow the decoder's geometry (s3imph.gunzip_geometry)."""
import functools
import gzip
import io
import random
import struct
import zlib
from collections import namedtuple

import gzip_ref as G
import s3imph

IN_CHUNK, BATCH, WAVES_PER_CU = s3imph.gunzip_geometry()

# status: what the file ends with; edge(trace, text): the property the case exists for;
# cpython_rejects: False where Python's gzip module reads the file although Go does not.
Case = namedtuple("Case", "name data status edge cpython_rejects")


def filler(nbytes: int, seed: int = 0) -> bytes:
    """Inventory-like rows, cut to exactly nbytes (the shape of test_gpu_csv.py's filler)."""
    rng = random.Random(seed)
    rows, size, i = [], 0, 0
    while size < nbytes:
        key = "d%d/s%d/obj-%05d.bin" % (rng.randrange(9), rng.randrange(4), i)
        if i % 7 == 3:
            key = '"%s, ""q"" %d"' % (key, i)
        row = ("%s,%d,%s,\r\n" if i % 5 == 0 else "%s,%d,%s,\n") % (key, rng.randrange(1 << 40),
                                                                    "GLACIER" if i % 3 else "STANDARD")
        rows.append(row.encode())
        size += len(rows[-1])
        i += 1
    return b"".join(rows)[:nbytes]


def gz(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, **kw):
    return G.member(G.raw_deflate(text, level, strategy), text, **kw)


def fib_text():
    """24 symbols with Fibonacci frequencies, 121 392 bytes: zlib's Huffman code for them has a
    15-bit code."""
    f = [1, 1]
    while len(f) < 24:
        f.append(f[-1] + f[-2])
    data = bytearray()
    for s, n in enumerate(f):
        data += bytes([97 + s]) * n
    random.Random(5).shuffle(data)
    assert len(data) == 121392
    return bytes(data)


def with_size(target, seed):
    """Filler text whose level-6 gzip file has exactly `target` bytes: the text is grown until the
    file is a few bytes short, and an FEXTRA field makes up the rest when no length fits."""
    n = max(target * 3, 64)
    while len(gz(filler(n, seed))) < target - 40:
        n += max((target - len(gz(filler(n, seed)))) * 2, 1)
    best = None
    for m in range(n, n + 4000):
        size = len(gz(filler(m, seed)))
        if size == target:
            return gz(filler(m, seed))
        if size <= target - 2:
            best = m
        if size > target:
            break
    text = filler(best, seed)
    pad = target - len(gz(text)) - 2
    out = gz(text, flg=4, extra=b"x" * pad)
    assert len(out) == target
    return out


def fixed_member(symbols, before=b"", **kw):
    w = G.BitWriter()
    w.fixed(symbols, final=True)
    return G.member(w.done(), G.expand(symbols, before), **kw)


def stored_straddle(shift):
    """Two stored blocks, the second one's LEN word starting `shift` bytes before byte IN_CHUNK of
    the file."""
    first = IN_CHUNK - shift - 10 - 5 - 1  # header, the first block's five bytes, the second's first
    a, b = filler(first, 41), filler(100, 42)
    w = G.BitWriter()
    w.stored(a)
    w.stored(b, final=True)
    data = G.member(w.done(), a + b)
    assert data[IN_CHUNK - shift:IN_CHUNK - shift + 4] == struct.pack("<HH", 100, 100 ^ 0xFFFF)
    return data


def repeat_over_the_boundary():
    """A hand-made dynamic block (zlib never writes one like it): code lengths 97: 2, 98: 3, 99: 3,
    255: 2, 256: 2 and four distance codes of length 2, where one repeat symbol 16 copies the
    length of 255 into 256 and on into all four distance lengths."""
    w = G.BitWriter()
    w.raw_bits(1, 1)
    w.raw_bits(2, 2)
    w.raw_bits(0, 5)   # HLIT: 257 literal/length codes
    w.raw_bits(3, 5)   # HDIST: 4 distance codes
    w.raw_bits(12, 4)  # HCLEN: 16 code-length code lengths
    cl = {16: 2, 18: 2, 3: 2, 2: 2}  # canonical: 2 -> 00, 3 -> 01, 16 -> 10, 18 -> 11
    for sym in G.CL_ORDER[:16]:
        w.raw_bits(cl.get(sym, 0), 3)
    code = {2: 0, 3: 1, 16: 2, 18: 3}
    for sym, extra, nbits in ((18, 97 - 11, 7), (2, 0, 0), (3, 0, 0), (3, 0, 0), (18, 138 - 11, 7), (18, 17 - 11, 7),
                              (2, 0, 0), (16, 5 - 3, 2)):
        w.put_code(code[sym], 2)
        w.raw_bits(extra, nbits)
    lit = {97: (0, 2), 255: (1, 2), 256: (2, 2), 98: (6, 3), 99: (7, 3)}
    text = b"abcab\xffcc"
    for ch in list(text) + [256]:
        w.put_code(*lit[ch])
    return G.member(w.done(), text)


def any_status(tr, text):
    return True


def valid_cases():
    out = []

    def add(name, data, edge=any_status):
        out.append(Case(name, data, G.OK, edge, True))

    add("empty_member", gzip.compress(b""), lambda tr, t: t == b"" and tr.members == 1)
    for n in (0, 1, 65535):
        w = G.BitWriter()
        text = filler(n, 50 + n % 7)
        w.stored(text, final=True)
        add("stored_%d" % n, G.member(w.done(), text), lambda tr, t, n=n: tr.stored_lens == [n])
    add("stored_zlib_70000", gz(filler(70000, 3), 0), lambda tr, t: len(tr.stored_lens) >= 2 and set(tr.block_types) == {0})
    for shift in (1, 2, 3):
        add("stored_straddle_%d" % shift, stored_straddle(shift), lambda tr, t: tr.stored_lens[1] == 100)
    add("fixed", gz(filler(3000, 4), 6, zlib.Z_FIXED), lambda tr, t: set(tr.block_types) == {1} and tr.matches > 10)
    for level in (1, 6, 9):
        add("dynamic_level_%d" % level, gz(filler(20000, 5), level), lambda tr, t: 2 in tr.block_types and tr.matches > 100)
    add("dynamic_repeat_over_the_boundary", repeat_over_the_boundary(),
        lambda tr, t: tr.cross_boundary_repeat and t == b"abcab\xffcc" and tr.block_types == [2])
    add("huffman_only_15_bits", gz(fib_text(), 6, zlib.Z_HUFFMAN_ONLY), lambda tr, t: tr.max_code_len == 15 and tr.matches == 0)
    rle = b"".join(bytes([65 + i % 26]) * (1 + (i * 37) % 700) for i in range(60))
    add("rle", gz(rle, 6, zlib.Z_RLE), lambda tr, t: tr.min_dist == 1 and tr.max_dist == 1 and tr.max_len == 258 and tr.overlaps > 10)
    far = list(filler(32768, 6))
    add("fixed_258_at_32768", fixed_member(far + [(258, 32768)]), lambda tr, t: tr.max_dist == 32768 and tr.max_len == 258)
    add("fixed_3_at_1", fixed_member([65, (3, 1)]), lambda tr, t: t == b"AAAA" and tr.overlaps == 1)
    w = G.BitWriter()
    w.fixed(list(b"abcdef"))
    w.fixed([(6, 6), 33, (5, 9)], final=True)
    two = b"abcdef" + G.expand([(6, 6), 33, (5, 9)], b"abcdef")
    add("match_into_previous_block", G.member(w.done(), two),
        lambda tr, t: tr.cross_block_match and t == b"abcdefabcdef!efabc")
    w = G.BitWriter()
    w.stored(b"hello world")
    w.fixed([(11, 11), (4, 1)], final=True)
    add("match_into_previous_stored_block", G.member(w.done(), b"hello worldhello worlddddd"),
        lambda tr, t: tr.cross_block_match and tr.block_types == [0, 1])
    chain = [97, 98, 99] + [(3, 3)] * (BATCH + 50) + [(7, 3), (258, 5)] * 20
    add("dependent_matches_over_a_batch_edge", fixed_member(chain), lambda tr, t: tr.matches > BATCH + 80 and tr.overlaps >= 40)
    for n in range(0, 301):
        add("filler_%d" % n, gz(filler(n, n)))
    for k in (1, 2, 3):
        for d in (-1, 1):
            target = k * IN_CHUNK + d
            add("compressed_%d" % target, with_size(target, 60 + k), lambda tr, t, target=target: tr.in_used == target)
    text = filler(700, 7)
    add("fextra", gz(text, flg=4, extra=b"\x01\x02\x03\0payload"), lambda tr, t: tr.flags == [4])
    buf = io.BytesIO()
    with gzip.GzipFile(filename="inventory.csv", mode="wb", fileobj=buf, mtime=0) as f:
        f.write(text)
    add("fname_from_python", buf.getvalue(), lambda tr, t: tr.flags == [8])
    add("fcomment", gz(text, flg=16, comment=b"a comment"), lambda tr, t: tr.flags == [16])
    add("fhcrc", gz(text, flg=2), lambda tr, t: tr.flags == [2])
    add("all_flags", gz(text, flg=2 | 4 | 8 | 16, extra=b"e" * 300, name=b"n.csv", comment=b"c" * 40),
        lambda tr, t: tr.flags == [0x1E])
    add("all_flags_and_reserved_bits", gz(text, flg=0xFE, extra=b"e" * 30, name=b"n.csv", comment=b"c" * 4),
        lambda tr, t: tr.flags == [0xFE])
    add("fextra_over_a_chunk", gz(text, flg=4 | 2, extra=bytes(range(256)) * 20), lambda tr, t: tr.flags == [6])
    a, b, c = filler(900, 8), filler(40, 9), filler(1300, 10)
    add("two_members", gz(a) + gz(c, 9), lambda tr, t: tr.members == 2)
    add("three_members", gz(a) + gz(b, 0) + gz(c, 1), lambda tr, t: tr.members == 3)
    add("empty_member_in_the_middle", gz(a) + gzip.compress(b"") + gz(c), lambda tr, t: tr.members == 3)
    rows = filler(2000, 11)
    cut = rows.index(b"\n", 1000) - 7
    add("record_cut_by_the_member_boundary", gz(rows[:cut]) + gz(rows[cut:]),
        lambda tr, t: tr.members == 2 and t == rows and rows[cut - 1] != 10)
    return out


def sixty():
    """A gzip file of exactly 60 bytes."""
    for n in range(20, 200):
        data = gz(filler(n, 12))
        if len(data) == 60:
            return data
    raise AssertionError("no 60-byte file")


def invalid_cases():
    out = []

    def add(name, data, status, cpython_rejects=True):
        out.append(Case(name, data, status, lambda tr, t: True, cpython_rejects))

    whole = sixty()
    for cut in range(60):  # (Python's gzip module reads no byte at all as no text)
        add("cut_at_%d" % cut, whole[:cut], G.EOF, cut > 0)
    good = gz(filler(500, 13))
    add("bad_magic_0", b"\x1e" + good[1:], G.HEADER)
    add("bad_magic_1", good[:1] + b"\x8c" + good[2:], G.HEADER)
    add("cm_7", good[:2] + b"\x07" + good[3:], G.HEADER)
    # CPython's gzip module skips the header CRC without checking it
    add("wrong_fhcrc", gz(filler(500, 13), flg=2, hcrc=0x1234), G.HEADER, False)
    # CPython's gzip module skips zero padding after the last member; Go's does not
    add("trailing_zeros", good + b"\0" * 12, G.HEADER, False)
    add("trailing_zero", good + b"\0", G.HEADER, False)
    add("zero_length", b"", G.EOF, False)
    w = G.BitWriter()
    w.fixed(list(b"abc"))
    w.raw_bits(1, 1)
    w.raw_bits(3, 2)
    add("block_type_3", G.member(w.done() + b"\0" * 8, b"abc"), G.DATA)
    w = G.BitWriter()
    w.stored(b"payload", final=True, nlen=7)
    add("len_nlen_mismatch", G.member(w.done(), b"payload"), G.DATA)
    add("distance_past_the_member_start", fixed_member([65, (3, 2)], before=b"?"), G.DATA)
    add("second_member_reaches_into_the_first", gz(b"abcdef") + fixed_member([(3, 3)], before=b"abcdef"), G.DATA)
    w = G.BitWriter()
    w.raw_bits(1, 1)
    w.raw_bits(2, 2)
    w.raw_bits(0, 5)
    w.raw_bits(0, 5)
    w.raw_bits(15, 4)
    for _ in range(19):
        w.raw_bits(1, 3)  # nineteen code-length codes of one bit each
    add("over_subscribed_code_lengths", G.member(w.done() + b"\0" * 16, b""), G.DATA)
    add("crc_bit", good[:-8] + bytes([good[-8] ^ 4]) + good[-7:], G.CHECKSUM)
    add("isize_bit", good[:-4] + bytes([good[-4] ^ 1]) + good[-3:], G.CHECKSUM)
    w = G.BitWriter()
    text = filler(400, 14)
    w.stored(text, final=True)
    st = bytearray(G.member(w.done(), text))
    st[10 + 5 + 200] ^= 0x10
    add("stored_payload_bit", bytes(st), G.CHECKSUM)
    return out


VALID = valid_cases()
INVALID = invalid_cases()


@functools.lru_cache(maxsize=None)
def refs():
    """{name: (text, trace)} of every case by gzip_ref, computed once for all tests."""
    return {c.name: G.gunzip(c.data) for c in VALID + INVALID}


def lying_isize(text, isize=5):
    """A good file whose last four bytes say `isize` although it holds far more: two members, and
    the trailer at the end tells only the last one's size, so the room hint is too small."""
    return gz(text) + gz(b"x" * isize)
