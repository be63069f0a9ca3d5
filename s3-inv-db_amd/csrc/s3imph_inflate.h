// s3imph_inflate.h — the serial parts of the gzip reader (include/s3imph.h, section 5j), written
// once for the device and the host: the CRC-32 operators, the bit reader, the Huffman table
// builder, the gzip header walk and the decode step of RFC 1951 / RFC 1952.  s3imph_inflate.hip
// runs them on one lane of a wave (the builder on sixteen); tools/inflate_host.cpp drives the same
// functions on the host, for tests/test_inflate_host.py and when a stream decodes wrongly.  Not
// part of the ABI.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define S3I_HD __host__ __device__ inline
#else
#define S3I_HD inline
#endif

namespace s3imph {
namespace inflate {

// ---------------------------------------------------------------- CRC-32 (reflected, 0xEDB88320)
// A CRC value is a polynomial over GF(2) modulo P, bit 31 the coefficient of x^0.
constexpr uint32_t kCrcPoly = 0xEDB88320u;

// One byte into the raw (unconditioned) register.
S3I_HD uint32_t crc_byte(uint32_t c, uint32_t b) {
  c ^= b;
  for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ kCrcPoly : c >> 1;
  return c;
}

// a * b mod P.
S3I_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1) ? (b >> 1) ^ kCrcPoly : b >> 1;  // b * x
  }
  return p;
}

// x^(8 n) mod P by square-and-multiply over the bits of n.
S3I_HD uint32_t crc_xpow8(uint64_t n) {
  uint32_t p = 1u << 31, sq = 1u << 23;  // x^0, x^8
  for (; n; n >>= 1) {
    if (n & 1) p = crc_mul(sq, p);
    sq = crc_mul(sq, sq);
  }
  return p;
}

// crc(A || B) from crc(A), crc(B) and x^(8 |B|): the zero-extension operator.  The conditioning
// (all-ones preset, final complement) of the two values cancels, so it holds for CRC-32 as zlib
// and the gzip trailer define it; crc of the empty string is 0.
S3I_HD uint32_t crc_concat(uint32_t crc_a, uint32_t crc_b, uint32_t xpow_b) { return crc_mul(xpow_b, crc_a) ^ crc_b; }

// ---------------------------------------------------------------- bit reader
// Reads a file through a window of its bytes: win[0] is file byte `base`, the window ends at file
// byte `lim` (<= len).  No byte outside [base, lim) is ever read; bits wanted past the window come
// as zeros and are counted in `zn`.  Callers keep br_ready() true before every step, so such bits
// lie past the file's end.  They are the last ones buffered, and looking ahead at them is free:
// only a step that has used one, which leaves fewer bits buffered than zeros supplied, has run
// over the end (br_over).  A corrupt symbol just before the end is therefore corrupt input, as for
// a reader that takes bits only as it needs them, and not an unexpected EOF.
struct BitReader {
  const uint8_t* win;
  int64_t base;
  uint64_t lim, len;
  uint64_t pos;  // next file byte to take
  uint64_t bb;   // bits taken and not yet used, the next one lowest
  uint32_t bn;
  uint32_t zn;   // zero bits supplied past the end since the reader was last emptied
};

// 16 bytes lie in the window beyond the buffered bits, or the window reaches the file's end: no
// decode step takes more than 71 bits (a dynamic block's counts and its 19 code-length lengths).
constexpr uint32_t kStepBytes = 16;
S3I_HD bool br_ready(const BitReader& r) { return r.lim == r.len || r.pos + kStepBytes <= r.lim; }

S3I_HD void br_need(BitReader& r, uint32_t n) {  // n <= 57
  while (r.bn < n) {
    uint64_t b = 0;
    if (r.pos < r.lim && (int64_t)r.pos >= r.base) {
      b = r.win[(int64_t)r.pos - r.base];
      ++r.pos;
    } else {
      r.zn += 8;
    }
    r.bb |= b << r.bn;
    r.bn += 8;
  }
}

S3I_HD void br_drop(BitReader& r, uint32_t n) {
  r.bb >>= n;
  r.bn -= n;
}

// A bit that the file does not hold has been used; stays true once it is.
S3I_HD bool br_over(const BitReader& r) { return r.zn > r.bn; }

S3I_HD uint32_t br_bits(BitReader& r, uint32_t n) {  // n <= 32
  br_need(r, n);
  const uint32_t v = (uint32_t)(r.bb & ((1ull << n) - 1));
  br_drop(r, n);
  return v;
}

S3I_HD void br_align(BitReader& r) { br_drop(r, r.bn & 7); }

// The file byte the next bit comes from (the reader is byte-aligned where this is asked); the
// file's length once the reader has run over its end.
S3I_HD uint64_t br_byte_pos(const BitReader& r) { return r.pos - (r.bn > r.zn ? (r.bn - r.zn) / 8 : 0); }

// ---------------------------------------------------------------- Huffman tables
// Canonical decoding: a primary table over the next PBITS bits answers the short codes, the
// counts and first codes per length answer the long ones bit by bit.  An entry of the primary
// table is (symbol << 4) | length, 0 where the bits begin a longer code or none.
template <int NSYM, int PBITS>
struct Huff {
  static constexpr int kSyms = NSYM, kPBits = PBITS;
  uint16_t count[16];  // codes of each length
  uint16_t first[16];  // the first code of each length
  uint16_t start[16];  // where the length's symbols begin in sym[]
  uint16_t sym[NSYM];  // symbols by (length, symbol)
  uint16_t prim[1 << PBITS];
};

// Step 1, for lanes `lane` of `nl`: the count of every length, and an empty primary table.
template <class H>
S3I_HD void huff_count(H& h, const uint8_t* lens, uint32_t n, uint32_t lane, uint32_t nl) {
  for (uint32_t l = lane; l < 16; l += nl) {
    uint32_t c = 0;
    for (uint32_t s = 0; s < n; ++s) c += lens[s] == l;
    h.count[l] = (uint16_t)c;
  }
  for (uint32_t i = lane; i < (1u << H::kPBits); i += nl) h.prim[i] = 0;
}

// Step 2, one lane: first codes and starts; false for a set that is over-subscribed, or
// incomplete and neither empty nor a single code of length 1.
template <class H>
S3I_HD bool huff_plan(H& h, uint32_t n) {
  int32_t left = 1;
  uint32_t code = 0, idx = 0;
  h.first[0] = h.start[0] = 0;
  for (uint32_t l = 1; l < 16; ++l) {
    left = 2 * left - (int32_t)h.count[l];
    if (left < 0) return false;
    h.first[l] = (uint16_t)code;
    h.start[l] = (uint16_t)idx;
    idx += h.count[l];
    code = (code + h.count[l]) << 1;
  }
  if (left > 0 && idx != 0 && !(idx == 1 && h.count[1] == 1)) return false;
  (void)n;
  return true;
}

S3I_HD uint32_t bit_reverse(uint32_t v, uint32_t n) {
  uint32_t r = 0;
  for (uint32_t k = 0; k < n; ++k) r |= ((v >> k) & 1) << (n - 1 - k);
  return r;
}

// Step 3, for lanes `lane` of `nl`, a length each: its symbols in order, its primary entries.
template <class H>
S3I_HD void huff_place(H& h, const uint8_t* lens, uint32_t n, uint32_t lane, uint32_t nl) {
  for (uint32_t l = 1 + lane; l < 16; l += nl) {
    if (!h.count[l]) continue;
    uint32_t code = h.first[l], idx = h.start[l];
    for (uint32_t s = 0; s < n; ++s) {
      if (lens[s] != l) continue;
      if (idx < (uint32_t)H::kSyms) h.sym[idx] = (uint16_t)s;
      ++idx;
      if (l <= (uint32_t)H::kPBits)
        for (uint32_t i = bit_reverse(code, l); i < (1u << H::kPBits); i += 1u << l)
          h.prim[i] = (uint16_t)((s << 4) | l);
      ++code;
    }
  }
}

// The next symbol, or -1 when the next 15 bits begin no code of the set; those 15 bits are then
// taken, so that br_over() tells whether the file held them all.  Takes up to 15 bits.
template <class H>
S3I_HD int32_t huff_decode(const H& h, BitReader& r) {
  br_need(r, 15);
  const uint32_t e = h.prim[r.bb & ((1u << H::kPBits) - 1)];
  if (e) {
    br_drop(r, e & 15);
    return (int32_t)(e >> 4);
  }
  uint32_t code = 0;
  uint64_t bits = r.bb;
  for (uint32_t l = 1; l < 16; ++l) {
    code |= (uint32_t)(bits & 1);
    bits >>= 1;
    const uint32_t k = code - h.first[l];
    if (k < h.count[l]) {  // code >= first[l]: an unsigned difference below the count
      const uint32_t at = h.start[l] + k;
      if (at >= (uint32_t)H::kSyms) return -1;
      br_drop(r, l);
      return h.sym[at];
    }
    code <<= 1;
  }
  br_drop(r, 15);
  return -1;
}

// ---------------------------------------------------------------- the decoder
enum Status : uint32_t { kOk = 0, kMore = 1, kEof = 2, kHeader = 3, kData = 4, kChecksum = 5 };

// What a step asks of its caller.
enum Event : uint32_t {
  kCont = 0,    // step again
  kFlush,       // the symbol queue is full
  kStored,      // copy Dec::slen bytes from file byte Dec::ssrc to the output
  kBuildCl,     // build Tabs::cl from Tabs::cllens
  kBuildFixed,  // build Tabs::ll and Tabs::dd for a fixed block
  kBuildDyn,    // build them from Tabs::lens (nlen literal/length, then ndist distance lengths)
  kEnd          // the file has ended with Dec::status
};

// A queued symbol: a literal byte, or kMatch | distance << 9 | length.
constexpr uint32_t kMatch = 1u << 31;

enum State : uint32_t { kStHeader, kStBlock, kStDyn, kStLens, kStSyms, kStTrailer0, kStTrailer1 };
enum HdrState : uint32_t {  // 0..9: the fixed bytes
  kHXlen0 = 10, kHXlen1, kHExtra, kHName, kHComment, kHCrc0, kHCrc1, kHDone
};

using HuffLL = Huff<288, 9>;
using HuffDD = Huff<32, 6>;
using HuffCL = Huff<19, 7>;

struct Tabs {
  HuffLL ll;
  HuffDD dd;
  HuffCL cl;
  uint8_t lens[320];  // 286 + 30 code lengths of a dynamic block, 288 + 32 of a fixed one
  uint8_t cllens[20];
};

struct Dec {
  uint32_t st = kStHeader, status = kOk;
  uint32_t hs = 0, flg = 0, hcrc = 0xFFFFFFFFu, xlen = 0, hcrc_want = 0;  // the header walk
  uint32_t bfinal = 0, nlen = 0, ndist = 0, li = 0;
  uint32_t mcrc = 0, members = 0, crc_file = 0;
  uint64_t mout = 0;  // bytes of this member so far
  uint64_t fout = 0;  // bytes of the file so far
  uint64_t ssrc = 0;
  uint32_t slen = 0;
};

S3I_HD uint32_t end_with(Dec& d, uint32_t status) {
  d.status = status;
  return kEnd;
}

S3I_HD uint32_t hdr_next(uint32_t flg, uint32_t after) {  // after: 0 fixed, 1 extra, 2 name, 3 comment
  if (after < 1 && (flg & 4)) return kHXlen0;
  if (after < 2 && (flg & 8)) return kHName;
  if (after < 3 && (flg & 16)) return kHComment;
  if (flg & 2) return kHCrc0;
  return kHDone;
}

// One header byte (RFC 1952 2.3).  0: more, 1: the header is over, 2: invalid header.
S3I_HD int hdr_byte(Dec& d, uint32_t b) {
  const uint32_t hs = d.hs;
  if (hs == 0) d.hcrc = 0xFFFFFFFFu;
  if (hs != kHCrc0 && hs != kHCrc1) d.hcrc = crc_byte(d.hcrc, b);
  if (hs < 10) {
    if ((hs == 0 && b != 0x1f) || (hs == 1 && b != 0x8b) || (hs == 2 && b != 8)) return 2;
    if (hs == 3) d.flg = b;
    d.hs = hs < 9 ? hs + 1 : hdr_next(d.flg, 0);
  } else if (hs == kHXlen0) {
    d.xlen = b;
    d.hs = kHXlen1;
  } else if (hs == kHXlen1) {
    d.xlen |= b << 8;
    d.hs = d.xlen ? (uint32_t)kHExtra : hdr_next(d.flg, 1);
  } else if (hs == kHExtra) {
    if (--d.xlen == 0) d.hs = hdr_next(d.flg, 1);
  } else if (hs == kHName) {
    if (b == 0) d.hs = hdr_next(d.flg, 2);
  } else if (hs == kHComment) {
    if (b == 0) d.hs = hdr_next(d.flg, 3);
  } else if (hs == kHCrc0) {
    d.hcrc_want = b;
    d.hs = kHCrc1;
  } else {
    if ((d.hcrc_want | b << 8) != (~d.hcrc & 0xFFFFu)) return 2;
    d.hs = kHDone;
  }
  return d.hs == kHDone ? 1 : 0;
}

// Base and extra bits of length symbol s (0..28) and distance symbol s (0..29), RFC 1951 3.2.5.
S3I_HD void length_code(uint32_t s, uint32_t* base, uint32_t* extra) {
  if (s < 8) {
    *base = 3 + s, *extra = 0;
  } else if (s == 28) {
    *base = 258, *extra = 0;
  } else {
    *extra = (s - 4) >> 2;
    *base = 3 + ((4 + (s & 3)) << *extra);
  }
}
S3I_HD void dist_code(uint32_t s, uint32_t* base, uint32_t* extra) {
  if (s < 4) {
    *base = 1 + s, *extra = 0;
  } else {
    *extra = (s >> 1) - 1;
    *base = 1 + ((2 + (s & 1)) << *extra);
  }
}

// One step of the file.  Termination: every step that returns kCont has taken at least one bit
// from the reader (a header byte, a block header, a code, a trailer word), except the one step per
// dynamic block that finds its code lengths complete, and the bits are finite: a step that takes
// a bit past the file's end finds br_over() true behind it and ends the file.  kFlush, kStored
// and the kBuild events take no bit, and each is followed by a step that does or by kEnd: the
// caller empties the queue, a stored block's header is behind the reader, a build moves on to
// kStSyms.
S3I_HD uint32_t step(Dec& d, BitReader& r, Tabs& t, uint32_t* q, uint32_t* nq, uint32_t qcap) {
  switch (d.st) {
    case kStHeader: {
      if (d.hs == 0 && r.bn <= r.zn && r.pos >= r.len) return end_with(d, d.members ? kOk : kEof);
      const uint32_t b = br_bits(r, 8);
      if (br_over(r)) return end_with(d, kEof);
      const int h = hdr_byte(d, b);
      if (h == 2) return end_with(d, kHeader);
      if (h == 1) {
        d.st = kStBlock;
        d.mout = 0;
        d.hs = 0;
      }
      return kCont;
    }
    case kStBlock: {
      d.bfinal = br_bits(r, 1);
      const uint32_t type = br_bits(r, 2);
      if (br_over(r)) return end_with(d, kEof);
      if (type == 0) {
        br_align(r);
        const uint32_t len = br_bits(r, 16), nlen = br_bits(r, 16);
        if (br_over(r)) return end_with(d, kEof);
        if ((len ^ 0xFFFFu) != nlen) return end_with(d, kData);
        const uint64_t src = br_byte_pos(r);
        if (src + len > r.len) return end_with(d, kEof);
        d.ssrc = src;
        d.slen = len;
        r.bb = 0, r.bn = 0, r.zn = 0, r.pos = src + len;  // the caller moves the window
        d.mout += len;
        d.fout += len;
        d.st = d.bfinal ? kStTrailer0 : kStBlock;
        return len ? (uint32_t)kStored : (uint32_t)kCont;
      }
      if (type == 1) {
        d.st = kStSyms;
        return kBuildFixed;
      }
      if (type == 2) {
        d.st = kStDyn;
        return kCont;
      }
      return end_with(d, kData);
    }
    case kStDyn: {
      d.nlen = br_bits(r, 5) + 257;
      d.ndist = br_bits(r, 5) + 1;
      const uint32_t ncl = br_bits(r, 4) + 4;
      if (br_over(r)) return end_with(d, kEof);
      if (d.nlen > 286 || d.ndist > 30) return end_with(d, kData);
      br_need(r, 3 * ncl);  // <= 57
      const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
      for (uint32_t i = 0; i < 19; ++i) t.cllens[order[i]] = i < ncl ? (uint8_t)br_bits(r, 3) : 0;
      if (br_over(r)) return end_with(d, kEof);
      d.li = 0;
      d.st = kStLens;
      return kBuildCl;
    }
    case kStLens: {
      const uint32_t total = d.nlen + d.ndist;
      if (d.li == total) {
        if (t.lens[256] == 0) return end_with(d, kData);  // no end-of-block code: the block could not end
        d.st = kStSyms;
        return kBuildDyn;
      }
      const int32_t s = huff_decode(t.cl, r);
      if (br_over(r)) return end_with(d, kEof);
      if (s < 0) return end_with(d, kData);
      if (s < 16) {
        t.lens[d.li++] = (uint8_t)s;
        return kCont;
      }
      uint32_t prev = 0, rep;
      if (s == 16) {
        if (d.li == 0) return end_with(d, kData);
        prev = t.lens[d.li - 1];
        rep = 3 + br_bits(r, 2);
      } else if (s == 17) {
        rep = 3 + br_bits(r, 3);
      } else {
        rep = 11 + br_bits(r, 7);
      }
      if (br_over(r)) return end_with(d, kEof);
      if (d.li + rep > total) return end_with(d, kData);
      for (uint32_t k = 0; k < rep; ++k) t.lens[d.li++] = (uint8_t)prev;
      return kCont;
    }
    case kStSyms: {
      if (*nq >= qcap) return kFlush;
      const int32_t s = huff_decode(t.ll, r);
      if (br_over(r)) return end_with(d, kEof);
      if (s < 0) return end_with(d, kData);
      if (s < 256) {
        q[(*nq)++] = (uint32_t)s;
        ++d.mout;
        ++d.fout;
        return kCont;
      }
      if (s == 256) {
        d.st = d.bfinal ? kStTrailer0 : kStBlock;
        return kCont;
      }
      if (s > 285) return end_with(d, kData);
      uint32_t base, extra;
      length_code((uint32_t)s - 257, &base, &extra);
      const uint32_t len = base + br_bits(r, extra);
      const int32_t ds = huff_decode(t.dd, r);
      if (br_over(r)) return end_with(d, kEof);
      if (ds < 0 || ds > 29) return end_with(d, kData);
      dist_code((uint32_t)ds, &base, &extra);
      const uint32_t dist = base + br_bits(r, extra);
      if (br_over(r)) return end_with(d, kEof);
      if (len > 258 || dist > d.mout) return end_with(d, kData);  // before the member's first byte
      q[(*nq)++] = kMatch | dist << 9 | len;
      d.mout += len;
      d.fout += len;
      return kCont;
    }
    case kStTrailer0: {
      br_align(r);
      d.mcrc = br_bits(r, 32);
      if (br_over(r)) return end_with(d, kEof);
      d.st = kStTrailer1;
      return kCont;
    }
    default: {  // kStTrailer1
      const uint32_t isize = br_bits(r, 32);
      if (br_over(r)) return end_with(d, kEof);
      if (isize != (uint32_t)d.mout) return end_with(d, kChecksum);
      d.crc_file = crc_concat(d.crc_file, d.mcrc, crc_xpow8(d.mout));
      ++d.members;
      d.st = kStHeader;
      d.hs = 0;
      return kCont;
    }
  }
}

// The code lengths of a fixed block (RFC 1951 3.2.6): 288 literal/length, then 32 distance codes
// (symbols 286, 287, 30 and 31 take part in the code and are refused when they are met).
S3I_HD uint8_t fixed_len(uint32_t i) { return i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5; }

}  // namespace inflate
}  // namespace s3imph
