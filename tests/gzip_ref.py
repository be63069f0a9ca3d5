"""A pure-Python gzip reader written from RFC 1951 and RFC 1952, as section 5j of include/s3imph.h
states the contract: the reference the GPU inflate is compared with, itself checked against zlib
and gzip (test_gzip_ref.py).  It returns the text and a trace of what the stream held, so that a
test case can prove that it reaches the edge it is meant for.  Beside it a tiny writer of stored,
fixed-Huffman and dynamic-Huffman blocks for hand-made streams, the ones no compressor writes."""
import struct
import zlib

OK, MORE, EOF, HEADER, DATA, CHECKSUM = range(6)
STATUS_TEXT = {EOF: "unexpected EOF", HEADER: "invalid header", DATA: "corrupt input", CHECKSUM: "invalid checksum"}

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
         258]
LEXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
         6145, 8193, 12289, 16385, 24577]
DEXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DD = [5] * 32


class Stop(Exception):
    def __init__(self, status):
        self.status = status


class Trace:
    def __init__(self):
        self.block_types = []      # of every block, in order
        self.max_code_len = 0      # longest code length of any dynamic table
        self.max_dist = 0
        self.max_len = 0
        self.min_dist = 1 << 20
        self.matches = 0
        self.overlaps = 0          # copies with distance < length
        self.stored_lens = []
        self.members = 0
        self.status = OK
        self.flags = []            # FLG of every member
        self.in_used = 0
        self.crc32 = 0
        self.cross_boundary_repeat = False  # a 16/17/18 run over the literal/length - distance boundary
        self.cross_block_match = False      # a match whose source lies in an earlier block
        self.len_syms = set()      # (length symbol, value of its extra bits) of every match
        self.dist_syms = set()     # (distance symbol, value of its extra bits) of every match
        self.decoded_lens = {"cl": set(), "ll": set(), "dd": set()}  # the code lengths met while decoding, per table
        self.dyn_blocks = []       # (nlen, ndist, non-zero distance lengths) of every dynamic block
        self.dyn_headers = []      # (first bit, bit behind the last code length) of every dynamic block, in the file
        self.block_syms = []       # literals and matches of every block (0 for a stored one)
        self.empty_stored_not_final = 0  # stored blocks with LEN = 0 that were not final: sync and full flushes


class Bits:
    def __init__(self, data, pos):
        self.d, self.pos, self.bb, self.bn = data, pos, 0, 0

    def take(self, n):
        while self.bn < n:
            if self.pos >= len(self.d):
                raise Stop(EOF)
            self.bb |= self.d[self.pos] << self.bn
            self.pos += 1
            self.bn += 8
        v = self.bb & ((1 << n) - 1)
        self.bb >>= n
        self.bn -= n
        return v

    def align(self):
        self.take(self.bn & 7)

    def byte_pos(self):
        return self.pos - self.bn // 8

    def bit_pos(self):
        return 8 * self.pos - self.bn


def make_code(lens):
    """{(length, code): symbol} of a canonical code; Stop(DATA) for a set that is over-subscribed,
    or incomplete and neither empty nor a single code of length 1."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    left = 1
    for l in range(1, 16):
        left = 2 * left - count[l]
        if left < 0:
            raise Stop(DATA)
    n = sum(count)
    if left > 0 and n != 0 and not (n == 1 and count[1] == 1):
        raise Stop(DATA)
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        nxt[l] = code
        code = (code + count[l]) << 1
    table = {}
    for s, l in enumerate(lens):
        if l:
            table[(l, nxt[l])] = s
            nxt[l] += 1
    return table


def decode(bits, table, seen):
    code = 0
    for l in range(1, 16):
        code = code << 1 | bits.take(1)
        if (l, code) in table:
            seen.add(l)
            return table[(l, code)]
    raise Stop(DATA)


def inflate_member(bits, out, tr):
    start = len(out)
    while True:
        bit0 = bits.bit_pos()
        bfinal, btype = bits.take(1), bits.take(2)
        tr.block_types.append(btype)
        tr.block_syms.append(0)
        block_start = len(out)
        if btype == 0:
            bits.align()
            ln, nln = bits.take(16), bits.take(16)
            if ln ^ 0xFFFF != nln:
                raise Stop(DATA)
            p = bits.byte_pos()
            if p + ln > len(bits.d):
                raise Stop(EOF)
            out += bits.d[p:p + ln]
            bits.pos, bits.bb, bits.bn = p + ln, 0, 0
            tr.stored_lens.append(ln)
            tr.empty_stored_not_final += ln == 0 and not bfinal
        elif btype == 3:
            raise Stop(DATA)
        else:
            if btype == 1:
                ll, dd = make_code(FIXED_LL), make_code(FIXED_DD)
            else:
                nlen, ndist, ncl = bits.take(5) + 257, bits.take(5) + 1, bits.take(4) + 4
                if nlen > 286 or ndist > 30:
                    raise Stop(DATA)
                cl = [0] * 19
                for i in range(ncl):
                    cl[CL_ORDER[i]] = bits.take(3)
                clt = make_code(cl)
                lens = []
                while len(lens) < nlen + ndist:
                    s = decode(bits, clt, tr.decoded_lens["cl"])
                    if s < 16:
                        lens.append(s)
                        continue
                    if s == 16:
                        if not lens:
                            raise Stop(DATA)
                        v, rep = lens[-1], 3 + bits.take(2)
                    elif s == 17:
                        v, rep = 0, 3 + bits.take(3)
                    else:
                        v, rep = 0, 11 + bits.take(7)
                    if len(lens) + rep > nlen + ndist:
                        raise Stop(DATA)
                    if len(lens) < nlen < len(lens) + rep:
                        tr.cross_boundary_repeat = True
                    lens += [v] * rep
                if lens[256] == 0:
                    raise Stop(DATA)
                tr.max_code_len = max(tr.max_code_len, max(lens))
                tr.dyn_blocks.append((nlen, ndist, sum(l != 0 for l in lens[nlen:])))
                tr.dyn_headers.append((bit0, bits.bit_pos()))
                ll, dd = make_code(lens[:nlen]), make_code(lens[nlen:])
            while True:
                s = decode(bits, ll, tr.decoded_lens["ll"])
                if s < 256:
                    out.append(s)
                    tr.block_syms[-1] += 1
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise Stop(DATA)
                    lx = bits.take(LEXT[s - 257])
                    ln = LBASE[s - 257] + lx
                    ds = decode(bits, dd, tr.decoded_lens["dd"])
                    if ds > 29:
                        raise Stop(DATA)
                    dx = bits.take(DEXT[ds])
                    dist = DBASE[ds] + dx
                    if dist > len(out) - start:
                        raise Stop(DATA)
                    tr.matches += 1
                    tr.block_syms[-1] += 1
                    tr.len_syms.add((s, lx))
                    tr.dist_syms.add((ds, dx))
                    tr.max_dist, tr.min_dist, tr.max_len = max(tr.max_dist, dist), min(tr.min_dist, dist), max(tr.max_len, ln)
                    tr.overlaps += dist < ln
                    if len(out) - dist < block_start:
                        tr.cross_block_match = True
                    for _ in range(ln):
                        out.append(out[-dist])
        if bfinal:
            return


def gunzip(data):
    """(text, trace) of a gzip file; trace.status says how it ended, and on an error the text is
    what had been decoded until then."""
    data = bytes(data)
    out, tr, pos, crc = bytearray(), Trace(), 0, 0
    try:
        while True:
            if pos == len(data):
                if tr.members == 0:
                    raise Stop(EOF)
                break
            # the header, byte by byte: a wrong byte is an invalid header where it stands
            want = {0: 0x1f, 1: 0x8b, 2: 8}
            h0 = pos
            for k in range(10):
                if pos >= len(data):
                    raise Stop(EOF)
                if k in want and data[pos] != want[k]:
                    raise Stop(HEADER)
                pos += 1
            flg = data[h0 + 3]
            tr.flags.append(flg)
            if flg & 4:
                if pos + 2 > len(data):
                    raise Stop(EOF)
                xlen = data[pos] | data[pos + 1] << 8
                pos += 2 + xlen
                if pos > len(data):
                    raise Stop(EOF)
            for bit in (8, 16):
                if flg & bit:
                    end = data.find(b"\0", pos)
                    if end < 0:
                        raise Stop(EOF)
                    pos = end + 1
            if flg & 2:
                if pos + 2 > len(data):
                    raise Stop(EOF)
                if data[pos] | data[pos + 1] << 8 != zlib.crc32(data[h0:pos]) & 0xFFFF:
                    raise Stop(HEADER)
                pos += 2
            bits = Bits(data, pos)
            m0 = len(out)
            try:
                inflate_member(bits, out, tr)
                bits.align()
                mcrc, isize = bits.take(32), bits.take(32)
            finally:
                pos = bits.byte_pos()
            if isize != (len(out) - m0) & 0xFFFFFFFF:
                raise Stop(CHECKSUM)
            if mcrc != zlib.crc32(bytes(out[m0:])):
                raise Stop(CHECKSUM)
            crc = zlib.crc32(bytes(out[m0:]), crc)
            tr.members += 1
    except Stop as s:
        tr.status = s.status
    tr.in_used = pos
    tr.crc32 = crc
    return bytes(out), tr


# ---------------------------------------------------------------- a writer for hand-made streams
class BitWriter:
    def __init__(self):
        self.out, self.bb, self.bn = bytearray(), 0, 0

    def put(self, v, n):
        self.bb |= v << self.bn
        self.bn += n
        while self.bn >= 8:
            self.out.append(self.bb & 255)
            self.bb >>= 8
            self.bn -= 8

    def put_code(self, code, n):  # Huffman codes go most significant bit first
        for k in range(n - 1, -1, -1):
            self.put(code >> k & 1, 1)

    def align(self):
        if self.bn:
            self.put(0, 8 - self.bn)

    def stored(self, payload, final=False, nlen=None):
        self.put(int(final), 1)
        self.put(0, 2)
        self.align()
        self.out += struct.pack("<HH", len(payload), (len(payload) ^ 0xFFFF) if nlen is None else nlen)
        self.out += payload

    def fixed(self, symbols, final=False, end=True):
        """One fixed-Huffman block of `symbols` (see _symbols); end=False leaves the end-of-block
        code out, for a stream that is cut behind a symbol."""
        self.put(int(final), 1)
        self.put(1, 2)
        self._symbols(symbols, canonical(FIXED_LL), canonical(FIXED_DD), end)

    def dynamic(self, symbols, ll_lens, dd_lens, final=False, hlit=None, hdist=None, end=True):
        """One dynamic-Huffman block of `symbols` (see _symbols) with the canonical codes of the
        code lengths ll_lens and dd_lens (lists, or {symbol: length}), whatever they are: an
        incomplete or over-subscribed set is written as it stands.  The lengths are sent with the
        plainest code-length code, 0..15 at four bits each and HCLEN = 19, without repeats.  hlit
        and hdist are the counts the header states when they are not the lists' lengths (the
        refused 287, 288, 31 and 32 among them).  The end-of-block code follows where it has a
        length and `end` is true."""
        ll_lens, dd_lens = as_lens(ll_lens, 257), as_lens(dd_lens, 1)
        self.dynamic_header(len(ll_lens) if hlit is None else hlit, len(dd_lens) if hdist is None else hdist,
                            [4] * 16 + [0] * 3, [(l, 0) for l in ll_lens + dd_lens], final)
        self._symbols(symbols, canonical(ll_lens), canonical(dd_lens), end and ll_lens[256] != 0)

    def dynamic_header(self, nlen, ndist, cl_lens, cl_items, final=False):
        """A dynamic block up to its code lengths: the counts as stated, the nineteen lengths of
        the code-length code, then cl_items, (symbol 0..18, value of its extra bits) each."""
        self.put(int(final), 1)
        self.put(2, 2)
        self.put(nlen - 257, 5)
        self.put(ndist - 1, 5)
        self.put(15, 4)
        for s in CL_ORDER:
            self.put(cl_lens[s], 3)
        code = canonical(cl_lens)
        for s, extra in cl_items:
            self.put_code(*code[s])
            self.put(extra, {16: 2, 17: 3, 18: 7}.get(s, 0))

    def _symbols(self, symbols, ll, dd, end):
        """ints are literals; (length, distance) is a match with the usual symbols; ("ll", symbol,
        extra) and ("dd", symbol, extra) write that very symbol of the literal/length or the
        distance code and the given value of its extra bits, so that a test picks the symbol and
        not the value (258 as symbol 284 + 31, the refused 286, 287, 30 and 31, which have no
        extra bits); ("bits", value, n) writes n raw bits."""
        for s in symbols:
            if isinstance(s, int):
                self.put_code(*ll[s])
            elif s[0] == "ll":
                self.put_code(*ll[s[1]])
                self.put(s[2], LEXT[s[1] - 257] if 257 <= s[1] <= 285 else 0)
            elif s[0] == "dd":
                self.put_code(*dd[s[1]])
                self.put(s[2], DEXT[s[1]] if s[1] <= 29 else 0)
            elif s[0] == "bits":
                self.put(s[1], s[2])
            else:
                ln, dist = s
                i = max(k for k in range(29) if LBASE[k] <= ln and (k == 28 or ln != 258))
                self.put_code(*ll[257 + i])
                self.put(ln - LBASE[i], LEXT[i])
                j = max(k for k in range(30) if DBASE[k] <= dist)
                self.put_code(*dd[j])
                self.put(dist - DBASE[j], DEXT[j])
        if end:
            self.put_code(*ll[256])

    def raw_bits(self, v, n):
        self.put(v, n)

    def done(self):
        self.align()
        return bytes(self.out)


def as_lens(lens, least):
    """A list of code lengths from a list or from {symbol: length}, no shorter than `least`."""
    if isinstance(lens, dict):
        lens = [lens.get(s, 0) for s in range(max(lens) + 1)]
    return list(lens) + [0] * (least - len(lens))


def canonical(lens):
    """{symbol: (code, length)} by RFC 1951 3.2.2, for any set of lengths: where it is
    over-subscribed the codes run over their length, which no reader gets to see."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def expand(symbols, before=b""):
    """What a run of BitWriter._symbols items decodes to after `before`."""
    out, ln = bytearray(before), 0
    for s in symbols:
        if isinstance(s, int) or (s[0] == "ll" and s[1] < 256):
            out.append(s if isinstance(s, int) else s[1])
        elif s[0] == "ll":
            ln = LBASE[s[1] - 257] + s[2] if s[1] > 256 else 0
        elif s[0] == "dd":
            for _ in range(ln):
                out.append(out[-(DBASE[s[1]] + s[2])])
        elif s[0] != "bits":
            for _ in range(s[0]):
                out.append(out[-s[1]])
    return bytes(out[len(before):])


def member(deflate, text, flg=0, extra=b"", name=b"", comment=b"", crc=None, isize=None, hcrc=None):
    """A gzip member around a raw DEFLATE stream."""
    h = bytearray(b"\x1f\x8b\x08" + bytes([flg]) + b"\0\0\0\0\0\xff")
    if flg & 4:
        h += struct.pack("<H", len(extra)) + extra
    if flg & 8:
        h += name + b"\0"
    if flg & 16:
        h += comment + b"\0"
    if flg & 2:
        h += struct.pack("<H", (zlib.crc32(bytes(h)) & 0xFFFF) if hcrc is None else hcrc)
    return bytes(h) + deflate + struct.pack("<II", zlib.crc32(text) if crc is None else crc,
                                            (len(text) & 0xFFFFFFFF) if isize is None else isize)


def raw_deflate(text, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem=8):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    return c.compress(text) + c.flush()
