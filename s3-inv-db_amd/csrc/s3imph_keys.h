// s3imph_keys.h — device pieces shared by the kernels that read or write byte strings packed
// in HBM as (blob, offsets): the finalize pass, the reader, the aggregation and the listing
// sort (s3imph_finalize.hip, s3imph_index.hip, s3imph_aggregate.hip, s3imph_sort.hip).  Nothing
// here knows its caller: what differs between two users comes in as an argument or a callable.
#pragma once

#include "s3imph_device.h"

namespace s3imph {

// 8 key bytes from blob address a (any alignment): two aligned words and a byte funnel.
// The blob is readable up to end8 = round_up(offsets[n], 8).
__device__ __forceinline__ uint64_t load8(const uint8_t* blob, uint64_t a, uint64_t end8) {
  const uint64_t al = a & ~7ull;
  const uint64_t* w = reinterpret_cast<const uint64_t*>(blob + al);
  const uint64_t lo = w[0];
  const uint64_t hi = (a & 7) && al + 8 < end8 ? w[1] : 0;
  return (a & 7) ? funnel_bytes(lo, hi, (unsigned)(a & 7)) : lo;
}

// exact per-byte zero test: high bit of each byte of the result set iff that byte of x is 0
__device__ __forceinline__ uint64_t zero_bytes(uint64_t x) {
  constexpr uint64_t k7f = 0x7f7f7f7f7f7f7f7full;
  const uint64_t t = (x & k7f) + k7f;
  return ~(t | x | k7f);
}

// bit 8j+7 set iff byte j of the first `valid` (1..8) bytes of x is '/'
__device__ __forceinline__ uint64_t slash_bits(uint64_t x, uint64_t valid) {
  uint64_t z = zero_bytes(x ^ 0x2f2f2f2f2f2f2f2full);
  if (valid < 8) z &= (1ull << (8 * valid)) - 1;
  return z;
}

// Three-way byte order of two keys of one blob (Go's string <: unsigned bytes, a proper prefix
// first): negative, zero or positive as key a (blob address a0, alen bytes) sorts before, equals
// or sorts after key b.  Word by word, the comparison k_sort_check and k_agg_keys make inline.
__device__ __forceinline__ int compare_keys(const uint8_t* blob, uint64_t a0, uint64_t alen, uint64_t b0,
                                            uint64_t blen, uint64_t end8) {
  const uint64_t mm = min(alen, blen);  // bytes both keys have
  for (uint64_t k = 0; k < mm; k += 8) {
    const uint64_t wa = load8(blob, a0 + k, end8), wb = load8(blob, b0 + k, end8);
    const uint64_t x = wa ^ wb;
    if (x) {
      const unsigned fd = (unsigned)(__builtin_ctzll(x) >> 3);
      if (fd < mm - k) return ((wa >> (8 * fd)) & 0xff) < ((wb >> (8 * fd)) & 0xff) ? -1 : 1;
      break;  // they differ only past the shorter key's end, in this last word
    }
  }
  return alen < blen ? -1 : (alen > blen ? 1 : 0);
}

// First index in [lo, hi) with U[index] > u, or hi.
__device__ __forceinline__ uint64_t first_above(const uint64_t* __restrict__ U, uint64_t lo, uint64_t hi,
                                                uint64_t u) {
  uint64_t len = hi - lo;
  while (len) {
    const uint64_t h = len >> 1;
    const bool right = U[lo + h] <= u;
    lo = right ? lo + h + 1 : lo;
    len = right ? len - h - 1 : h;
  }
  return lo;
}
// First index in [lo, hi) with U[index] >= u, or hi.
__device__ __forceinline__ uint64_t first_at_least(const uint64_t* __restrict__ U, uint64_t lo, uint64_t hi,
                                                   uint64_t u) {
  uint64_t len = hi - lo;
  while (len) {
    const uint64_t h = len >> 1;
    const bool right = U[lo + h] < u;
    lo = right ? lo + h + 1 : lo;
    len = right ? len - h - 1 : h;
  }
  return lo;
}

// A kernel that cuts its output into chunks of `step` units (rows, or bytes of a blob) needs the
// owner (key, or row) of each chunk's first unit: an upper-bound search in a scan U of `entries`
// entries.  The owner of chunk t = the last index with U[index] <= max(t * step, first_min).
// Run with one lane per chunk (k_agg_bounds, k_gather_bounds), so the searches' dependent loads
// overlap across chunks instead of standing at the head of every workgroup.
__device__ __forceinline__ uint64_t chunk_owner(const uint64_t* __restrict__ U, uint64_t entries, uint64_t step,
                                                uint64_t first_min, uint64_t t) {
  return first_above(U, 0, entries, max(t * step, first_min)) - 1;
}

// The byte emit: rows r = 0..n-1 are to stand back to back in `out`, row r at offsets[r]
// (n + 1 entries, offsets[0] = 0, offsets[n] = total), its bytes taken from blob address src(r)
// on.  One workgroup of kT lanes per chunk of kT output words; each lane assembles one 8-byte
// word.  The row of a byte is the last one that starts at or before it (upper-bound search in
// the offsets inside the workgroup's rows, bounds[] from chunk_owner with step 8 kT); a word
// takes one unaligned 8-byte read of the blob per row it overlaps, which may run past the row's
// source, never past the blob's readable end end8.  Bytes past `total` in the last word are zeros.
template <int kT, class Src>
__device__ __forceinline__ void emit_word(const uint8_t* __restrict__ blob, uint64_t end8,
                                          const uint64_t* __restrict__ offsets,
                                          const uint64_t* __restrict__ bounds, uint64_t n, uint64_t total,
                                          uint8_t* __restrict__ out, Src src) {
  const uint64_t wbase = (uint64_t)blockIdx.x * kT;
  const uint64_t nw = (total + 7) / 8;
  if (wbase >= nw) return;
  const uint64_t r_lo = bounds[blockIdx.x];
  const uint64_t r_hi = blockIdx.x + 1 < gridDim.x ? bounds[blockIdx.x + 1] : n - 1;
  const uint64_t wi = wbase + threadIdx.x;
  if (wi >= nw) return;
  const uint64_t a = 8 * wi, aend = min(a + 8, total);
  uint64_t r = first_above(offsets, r_lo + 1, r_hi + 1, a) - 1;
  uint64_t o0 = offsets[r], o1 = offsets[r + 1];
  uint64_t v = 0;
  for (uint64_t p = a; p < aend;) {
    while (o1 <= p) {  // offsets[n] = total > p ends it
      ++r;
      o0 = o1;
      o1 = offsets[r + 1];
    }
    const uint64_t cnt = min(o1, aend) - p;  // bytes of row r in this word, 1..8
    const uint64_t x = load8(blob, src(r) + (p - o0), end8);
    v |= (cnt >= 8 ? x : x & ((1ull << (8 * cnt)) - 1)) << (8 * (p - a));
    p += cnt;
  }
  if (((uintptr_t)out & 7) == 0) {
    *reinterpret_cast<uint64_t*>(out + a) = v;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) out[a + j] = (uint8_t)(v >> (8 * j));
  }
}

}  // namespace s3imph
