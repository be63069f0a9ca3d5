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


def symbol_pairs(base_count, ext):
    """(symbol index, extra value) with the extra bits all zero and all one, for every symbol."""
    return sorted({(k, v) for k in range(base_count) for v in (0, (1 << ext[k]) - 1)})


LEN_PAIRS = [(257 + k, v) for k, v in symbol_pairs(29, G.LEXT)]  # (284, 31) is length 258 the long way
DIST_PAIRS = symbol_pairs(30, G.DEXT)


def every_pair():
    """Matches that use every pair of LEN_PAIRS and of DIST_PAIRS at least once."""
    n = max(len(LEN_PAIRS), len(DIST_PAIRS))
    out = []
    for i in range(n):
        out += [("ll",) + LEN_PAIRS[i % len(LEN_PAIRS)], ("dd",) + DIST_PAIRS[i % len(DIST_PAIRS)]]
    return out


def has_every_pair(tr):
    return tr.len_syms >= set(LEN_PAIRS) and (284, 31) in tr.len_syms and tr.dist_syms >= set(DIST_PAIRS)


def dynamic_member(symbols, ll_lens, dd_lens, **kw):
    w = G.BitWriter()
    w.dynamic(symbols, ll_lens, dd_lens, final=True, **kw)
    return G.member(w.done(), G.expand(symbols))


def flushed(text, mode, piece=50):
    """A member whose writer flushed with `mode` after every `piece` bytes, as pgzip's and Go's do."""
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = b"".join(c.compress(text[i:i + piece]) + c.flush(mode) for i in range(0, len(text), piece))
    return G.member(raw + c.flush(), text)


# 0..12 and the three repeat symbols, four bits each: a complete code-length code for the hand-made
# headers below
CL_WITH_REPEATS = [4] * 13 + [0] * 3 + [4] * 3


def hand_made_valid(add):
    """Streams that zlib never writes and RFC 1951 allows (Go's compress/flate, pgzip and Java
    write some of them), from BitWriter.dynamic and the raw items of BitWriter.fixed."""
    far = list(filler(32768, 6))
    w = G.BitWriter()
    w.fixed(far)
    w.fixed(every_pair(), final=True)
    add("every_length_and_distance_symbol", G.member(w.done(), G.expand(far + every_pair())),
        lambda tr, t: has_every_pair(tr) and tr.block_types == [1, 1])
    # 226 codes of 8 bits and 60 of 9, 2 distance codes of 4 bits and 28 of 5: both sets complete
    add("every_symbol_of_a_dynamic_block_286_30",
        dynamic_member(far + every_pair(), [8] * 226 + [9] * 60, [4] * 2 + [5] * 28),
        lambda tr, t: has_every_pair(tr) and tr.dyn_blocks == [(286, 30, 30)] and tr.block_types == [2])
    add("dynamic_smallest", dynamic_member(list(b"abbaab"), {97: 1, 98: 2, 256: 2}, [0]),
        lambda tr, t: tr.dyn_blocks == [(257, 1, 0)] and tr.matches == 0 and t == b"abbaab")
    add("single_distance_code",
        dynamic_member([97, (3, 1), 98, (258, 1), (4, 1), 97], {97: 2, 98: 2, 256: 3, 257: 3, 258: 3, 285: 3}, [1]),
        lambda tr, t: tr.dyn_blocks == [(286, 1, 1)] and tr.matches == 3 and tr.max_dist == 1 and tr.decoded_lens["dd"] == {1})
    # the sixteen codes 0, 10, 110, ..., thirteen ones and a zero, and two of 15 bits; each used once
    ladder = list(range(1, 16)) + [15]
    text = list(filler(300, 15))
    for name, lens in (("distance_codes_to_15_bits", ladder), ("distance_codes_from_15_bits", ladder[::-1])):
        add(name, dynamic_member(text + [(3 + k, G.DBASE[k]) for k in range(16)], [8] * 226 + [9] * 60, lens),
            lambda tr, t: all(l in tr.decoded_lens["dd"] for l in (7, 8, 9, 10, 11, 12, 13, 14, 15))
            and {d for d, _ in tr.dist_syms} == set(range(16)) and tr.max_code_len == 15)
    # a..n with 1..14 bits, end-of-block and length 3 with 15
    lens = {97 + k: 1 + k for k in range(14)}
    lens.update({256: 15, 257: 15})
    add("literal_codes_at_every_length", dynamic_member(list(b"abcdefghijklmn") * 2 + [(3, 1)] + list(b"nmlkjihg"), lens, [1]),
        lambda tr, t: all(l in tr.decoded_lens["ll"] for l in (10, 11, 12, 13, 14, 15)) and tr.decoded_lens["ll"] == set(range(1, 16)))
    for name, mode in (("sync_flush_every_50_bytes", zlib.Z_SYNC_FLUSH), ("full_flush_every_50_bytes", zlib.Z_FULL_FLUSH)):
        add(name, flushed(filler(1100, 16), mode), lambda tr, t: len(tr.block_types) >= 20 and tr.empty_stored_not_final >= 10)
    for n in (BATCH - 1, BATCH, BATCH + 1):
        first = list(filler(n - 2, 17)) + [(5, 9), (258, 1)]
        second = list(b"abab") + [(4, 2)]
        w = G.BitWriter()
        w.fixed(first)
        w.dynamic(second, {97: 2, 98: 2, 256: 2, 258: 2}, [0, 1])
        w.dynamic(second, {97: 2, 98: 2, 256: 2, 258: 2}, [0, 1], final=True)
        add("block_of_%d_symbols_then_a_dynamic_block" % n, G.member(w.done(), G.expand(first + second + second)),
            lambda tr, t, n=n: tr.block_syms == [n, 5, 5] and tr.block_types == [1, 2, 2])
    a, b = filler(5000, 18), filler(700, 19)
    mid = [(258, 4000), (100, 4358), 33, (3, 4000), (258, 5000)]
    w = G.BitWriter()
    w.stored(a)
    w.fixed(mid)
    w.stored(b, final=True)
    add("stored_then_matches_then_stored", G.member(w.done(), a + G.expand(mid, a) + b),
        lambda tr, t: tr.block_types == [0, 1, 0] and tr.stored_lens == [5000, 700] and tr.max_dist == 5000
        and tr.cross_block_match and IN_CHUNK * 2 < 5000)
    for n in (8191, 8192, 8193, 16384):  # the CRC kernels cut a text every 8192 bytes
        add("text_of_%d_bytes" % n, gz(filler(n, 20)), lambda tr, t, n=n: len(t) == n)


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
    hand_made_valid(add)
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
    corrupt_blocks(add)
    cuts(add)
    return out


def corrupt_blocks(add):
    """The ways a Huffman block can be corrupt, each a whole member with its trailer behind it,
    and four of them once more with the file ending right behind the bad symbol: a reader that
    looks ahead must still call them corrupt, not cut.  zlib refuses them all."""
    ok_ll, ok_dd = {97: 1, 256: 2, 257: 2}, [1]

    def dyn(name, symbols, ll_lens, dd_lens, **kw):
        w = G.BitWriter()
        w.dynamic(symbols, ll_lens, dd_lens, final=True, **kw)
        add(name, G.member(w.done(), b""), G.DATA)

    def lens(name, items, tail=True):
        w = G.BitWriter()
        w.dynamic_header(257, 1, CL_WITH_REPEATS, items, final=True)
        add(name, G.member(w.done(), b"") if tail else G.member(w.done(), b"")[:-8], G.DATA)

    def fixed(name, symbols, tail=True):
        w = G.BitWriter()
        w.fixed(symbols, final=True, end=tail)
        add(name, G.member(w.done(), b"") if tail else G.member(w.done(), b"")[:-8], G.DATA)

    for n in (287, 288):
        dyn("hlit_%d" % n, [97], ok_ll, ok_dd, hlit=n)
    for n in (31, 32):
        dyn("hdist_%d" % n, [97], ok_ll, ok_dd, hdist=n)
    for sym in (286, 287):
        fixed("fixed_symbol_%d" % sym, [65, ("ll", sym, 0)])
    for sym in (30, 31):
        fixed("fixed_distance_code_%d" % sym, [65, ("ll", 257, 0), ("dd", sym, 0)])
    lens("repeat_16_first", [(16, 0)] + [(0, 0)] * 255)
    # 258 lengths in all: 138 + 111 zeros, then a run that ends at 259
    lens("repeat_16_one_past_the_total", [(18, 127), (18, 100), (2, 0), (2, 0), (2, 0), (2, 0), (16, 3)])
    lens("repeat_17_one_past_the_total", [(18, 127), (18, 100), (17, 7)])
    lens("repeat_18_one_past_the_total", [(18, 127), (18, 99), (18, 0)])
    dyn("no_end_of_block_code", [97], {97: 1, 98: 1}, ok_dd)
    dyn("two_literal_codes_of_length_2", [97], {97: 2, 256: 2}, ok_dd)
    dyn("over_subscribed_literal_set", [97], {97: 1, 98: 1, 256: 1}, ok_dd)
    dyn("over_subscribed_distance_set", [97], ok_ll, [1, 1, 1])
    dyn("two_distance_codes_of_length_2", [97], ok_ll, [2, 2])
    dyn("single_distance_code_of_length_2", [97], ok_ll, [2])
    dyn("unused_bit_of_the_single_distance_code", [97, ("ll", 257, 0), ("bits", 1, 1)], ok_ll, [1])
    dyn("match_with_an_empty_distance_set", [97, ("ll", 257, 0)], ok_ll, [0])
    w = G.BitWriter()
    w.dynamic_header(257, 1, [0] * 19, [], final=True)
    add("all_zero_code_length_set", G.member(w.done(), b""), G.DATA)
    fixed("fixed_symbol_286_then_the_end", [65, ("ll", 286, 0)], tail=False)
    fixed("distance_past_the_member_start_then_the_end", [65, ("ll", 257, 0), ("dd", 1, 0)], tail=False)
    fixed("fixed_distance_code_30_then_the_end", [65, ("ll", 257, 0), ("dd", 30, 0)], tail=False)
    lens("repeat_16_first_then_the_end", [(16, 0)], tail=False)


def cuts(add):
    """Files cut where the input stage, a dynamic header, a trailer, a stored payload or a second
    member's header is under the reader: all unexpected EOF, and a mistake is a hang."""
    def cut(name, data, at):
        for n in at:
            assert n < len(data)
            add("%s_cut_at_%d" % (name, n), data[:n], G.EOF)

    one = with_size(IN_CHUNK + 60, 81)
    cut("one_stage", one, range(IN_CHUNK - 24, IN_CHUNK + 60))
    two = with_size(2 * IN_CHUNK + 30, 82)
    cut("two_stages", two, range(2 * IN_CHUNK - 24, 2 * IN_CHUNK + 30))
    text = filler(2000, 21)
    whole = gz(text)
    tr = G.gunzip(whole)[1]
    assert tr.block_types == [2]
    bit0, bit1 = tr.dyn_headers[0]
    cut("dynamic_header", whole, range(bit0 // 8, (bit1 + 7) // 8 + 1))
    cut("trailer", whole, range(len(whole) - 8, len(whole)))
    w = G.BitWriter()
    payload = filler(IN_CHUNK + 500, 22)
    w.stored(payload, final=True)
    cut("stored_payload", G.member(w.done(), payload), (IN_CHUNK - 1, IN_CHUNK, IN_CHUNK + 1))
    first = gz(filler(900, 8))
    second = gz(filler(1300, 10), flg=2 | 4 | 8 | 16, extra=b"extra", name=b"n.csv", comment=b"c c")
    hdr = 10 + 2 + 5 + 6 + 4 + 2
    assert G.gunzip(first + second)[1].status == G.OK and second[hdr - 2:hdr] != second[hdr:hdr + 2]
    cut("second_header", first + second, range(len(first) + 1, len(first) + hdr + 1))


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
