// s3imph_sort.hip — the step in front of the aggregation: an object listing in ANY order in HBM
// is put into byte order (include/s3imph.h section 5f), so that "listing in, index out" needs no
// host sort.
//
// Reference (pkg/extsort):
//   aggregator.go:44-76  AddObject accumulates into a map in whatever order objects arrive;
//   types.go:160-164     SortPrefixRows makes the order afterwards: sort.Slice by Go's string <,
//                        i.e. unsigned bytes, a proper prefix before its extensions.
// Here the OBJECT keys are sorted (stably: equal keys keep their input order) and the sorted
// listing goes through the aggregation of s3imph_aggregate.hip unchanged.
//
// GPU formulation: MSD refinement by 7-byte chunks.  In round r key i
// contributes one u64,
//     word = (bytes[7r .. 7r+7) big-endian, zero-padded) << 8 | min(len - 7r, 8),
// the low byte being the chunk's valid bytes, 8 = "more follow".  Comparing the words round by
// round is the byte order: equal padded bytes with different counts means one key is a prefix of
// the other, and the shorter has the smaller count.  A key whose low byte is <= 7 is finished;
// finished keys with equal words in every round are identical.
//
// The active elements are kept as packed = segment << 32 | input index, ordered by segment; a
// segment is a run of keys equal in every earlier chunk, and delta[segment] + (array index) is
// an element's position in the final order.  Per round: words of the active keys (k_sort_words),
// a stable rocPRIM radix sort by word and one by the segment bits, then k_sort_mark cuts every
// segment where the word changes, writes singletons and finished runs to their final position,
// and k_sort_compact (after one scan) keeps the rest as the next round's segments.  The active
// set shrinks to what is still unresolved; the rounds end at ceil((max_len + 1) / 7) at the latest.
// A first pass (k_sort_check, the comparison k_agg_keys makes) finds sorted input and returns
// the identity without any of this.
//
// Gather: lengths in sorted order, one scan into the output offsets, and the key bytes copied by
// OUTPUT 8-byte word (emit_word, s3imph_keys.h), so writes are coalesced and a long key is spread
// over lanes; sizes and tier ids follow the same order.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "s3imph_entry.h"
#include "s3imph_keys.h"
#include "s3imph_prim.h"

namespace s3imph {

namespace {

constexpr int kST = 256;  // lanes per workgroup: one element / one output word each

// What the check pass reports: the smallest unsorted index, the equal neighbours (of sorted
// input), the longest key.
struct SortTop {
  unsigned long long first_unsorted, n_equal, max_len;
};

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor((unsigned long long)v, o);
  return v;
}

// The first pass: key i against key i - 1, word by word (the comparison of k_agg_keys).
__global__ __launch_bounds__(kST) void k_sort_check(const uint8_t* __restrict__ blob,
                                                    const uint64_t* __restrict__ offsets, uint64_t m,
                                                    SortTop* __restrict__ top) {
  const uint64_t i = (uint64_t)blockIdx.x * kST + threadIdx.x;
  const uint64_t end8 = (offsets[m] + 7) & ~7ull;
  uint64_t len = 0;
  bool equal = false, unsorted = false;
  if (i < m) {
    const uint64_t b0 = offsets[i];
    len = offsets[i + 1] - b0;
    if (i > 0) {
      const uint64_t p0 = offsets[i - 1], plen = b0 - p0;
      const uint64_t mm = min(len, plen);  // bytes both keys have
      bool differ = false, less = false;
      for (uint64_t k = 0; k < mm; k += 8) {
        const uint64_t x = load8(blob, b0 + k, end8) ^ load8(blob, p0 + k, end8);
        const unsigned avail = (unsigned)min((uint64_t)8, mm - k);
        const unsigned fd = x ? (unsigned)(__builtin_ctzll(x) >> 3) : 8u;
        if (fd < avail) {
          const uint64_t w = load8(blob, b0 + k, end8), pw = w ^ x;
          less = ((w >> (8 * fd)) & 0xff) < ((pw >> (8 * fd)) & 0xff);
          differ = true;
          break;
        }
      }
      if (!differ) {
        less = len < plen;  // a proper prefix of its predecessor
        equal = len == plen;
      }
      unsorted = less;
    }
  }
  // In a shuffled listing half of all keys are smaller than their predecessor: one atomic per
  // wave, and only while it can still lower the minimum (the read may be stale; the atomic decides)
  const uint64_t bad = __ballot(unsorted);
  const uint64_t eq = wave_sum(equal ? 1 : 0);
  uint64_t mx = len;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = max(mx, (uint64_t)__shfl_xor((unsigned long long)mx, o));
  if (lane_id() == 0) {
    const unsigned long long first = i + (bad ? (unsigned)__builtin_ctzll(bad) : 0u);
    if (bad && first < *reinterpret_cast<volatile unsigned long long*>(&top->first_unsorted))
      atomicMin(&top->first_unsorted, first);
    if (eq) atomicAdd(&top->n_equal, (unsigned long long)eq);
    if (mx > *reinterpret_cast<volatile unsigned long long*>(&top->max_len))
      atomicMax(&top->max_len, (unsigned long long)mx);
  }
}

__global__ __launch_bounds__(kST) void k_sort_iota(uint32_t* __restrict__ out, uint64_t m) {
  const uint64_t i = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (i < m) out[i] = (uint32_t)i;
}

// Round 0's active set: every key, one segment that starts at position 0.
__global__ __launch_bounds__(kST) void k_sort_init(uint64_t* __restrict__ packed, uint32_t* __restrict__ delta,
                                                   uint64_t m) {
  const uint64_t i = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (i < m) packed[i] = i;
  if (i == 0) delta[0] = 0;
}

// (a) The round's word of every active key.  A key active in round r > 0 had "more follow" in
// round r - 1, so it has at least 7r + 1 bytes; in round 0 an empty key reads nothing.
__global__ __launch_bounds__(kST) void k_sort_words(const uint8_t* __restrict__ blob,
                                                    const uint64_t* __restrict__ offsets, uint64_t m,
                                                    const uint64_t* __restrict__ packed, uint64_t active,
                                                    uint64_t skip, uint64_t* __restrict__ word) {
  const uint64_t j = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (j >= active) return;
  const uint64_t end8 = (offsets[m] + 7) & ~7ull;
  const uint64_t i = packed[j] & 0xffffffffull;
  const uint64_t b0 = offsets[i], len = offsets[i + 1] - b0;
  const uint64_t rem = len > skip ? len - skip : 0;
  uint64_t w = 0;
  if (rem) {
    const unsigned valid = (unsigned)min(rem, (uint64_t)7);
    const uint64_t be = __builtin_bswap64(load8(blob, b0 + skip, end8));  // byte 0 on top
    w = be & (~0ull << (8 * (8 - valid)));                                // valid <= 7: the low byte goes
  }
  word[j] = w | min(rem, (uint64_t)8);
}

// (c) Re-segmentation over the active set sorted by (segment, word).  A run is a stretch of equal
// (segment, word); its elements are in input order (every sort and the compaction are stable).
// The element at array index j belongs at position delta[segment] + j of the final order.  A
// singleton run and a finished run (low byte <= 7: identical keys) are written there and leave;
// the other runs stay as the next round's segments.  v[j] = stays | (stays and heads its run)
// << 32, for one scan that yields both the compacted index and the new segment id.
__global__ __launch_bounds__(kST) void k_sort_mark(const uint64_t* __restrict__ packed,
                                                   const uint64_t* __restrict__ word,
                                                   const uint32_t* __restrict__ delta, uint64_t active,
                                                   uint32_t* __restrict__ order, uint32_t* __restrict__ fpos,
                                                   uint64_t* __restrict__ v, SortTop* __restrict__ top) {
  const uint64_t j = (uint64_t)blockIdx.x * kST + threadIdx.x;
  bool dup = false;
  if (j < active) {
    const uint64_t p = packed[j], w = word[j];
    const uint64_t sg = p >> 32;
    const bool head = j == 0 || (packed[j - 1] >> 32) != sg || word[j - 1] != w;
    const bool next_head = j + 1 == active || (packed[j + 1] >> 32) != sg || word[j + 1] != w;
    const bool finished = (w & 0xff) <= 7;
    const uint32_t pos = delta[sg] + (uint32_t)j;
    const bool stays = !finished && !(head && next_head);
    if (!stays) order[pos] = (uint32_t)p;
    dup = finished && !head;  // the same key as its sorted predecessor
    fpos[j] = pos;
    v[j] = stays ? 1ull | ((uint64_t)head << 32) : 0ull;
  } else if (j == active) {
    v[j] = 0;  // the scan's last entry: the totals
  }
  const uint64_t eq = wave_sum(dup ? 1 : 0);
  if (lane_id() == 0 && eq) atomicAdd(&top->n_equal, (unsigned long long)eq);
}

// (d) The next round's active set: E is the exclusive scan of v (low half: elements kept before
// j, high half: run heads kept before j).
__global__ __launch_bounds__(kST) void k_sort_compact(const uint64_t* __restrict__ packed,
                                                      const uint32_t* __restrict__ fpos,
                                                      const uint64_t* __restrict__ E, uint64_t active,
                                                      uint64_t* __restrict__ packed_out,
                                                      uint32_t* __restrict__ delta_out) {
  const uint64_t j = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (j >= active) return;
  const uint64_t e = E[j], d = E[j + 1] - e;  // d = v[j]
  if (!(d & 1)) return;
  const uint64_t dest = e & 0xffffffffull;
  const bool head = (d >> 32) != 0;
  const uint64_t sg = (e >> 32) - (head ? 0 : 1);  // a kept non-head has its head before it
  packed_out[dest] = (sg << 32) | (packed[j] & 0xffffffffull);
  if (head) delta_out[sg] = fpos[j] - (uint32_t)dest;
}

// Gather, first half: the length of the j-th key in sorted order (scanned into the output
// offsets afterwards), its size and its tier id.  An order entry >= m is reported, not followed.
__global__ __launch_bounds__(kST) void k_gather_meta(const uint64_t* __restrict__ offsets,
                                                     const uint64_t* __restrict__ sizes,
                                                     const uint8_t* __restrict__ tiers, uint64_t m,
                                                     const uint32_t* __restrict__ order,
                                                     uint64_t* __restrict__ off_out, uint64_t* __restrict__ sizes_out,
                                                     uint8_t* __restrict__ tiers_out,
                                                     unsigned long long* __restrict__ first_bad) {
  const uint64_t j = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (j > m) return;
  if (j == m) {
    off_out[m] = 0;
    return;
  }
  const uint64_t i = order[j];
  if (i >= m) {
    atomicMin(first_bad, (unsigned long long)j);
    off_out[j] = 0;
    return;
  }
  off_out[j] = offsets[i + 1] - offsets[i];
  if (sizes) sizes_out[j] = sizes[i];
  if (tiers) tiers_out[j] = tiers[i];
}

// The owner (sorted key) of each output chunk's first word: one lane per chunk (chunk_owner).
__global__ __launch_bounds__(kST) void k_gather_bounds(const uint64_t* __restrict__ U, uint64_t entries,
                                                       uint64_t step, uint64_t nchunks,
                                                       uint64_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kST + threadIdx.x;
  if (t < nchunks) out[t] = chunk_owner(U, entries, step, 0, t);
}

// Gather, second half, by output bytes (emit_word): each lane assembles one 8-byte word of the
// sorted blob; the source of output key r is input key order[r].
__global__ __launch_bounds__(kST) void k_gather_bytes(const uint8_t* __restrict__ blob, uint64_t key_end8,
                                                      const uint64_t* __restrict__ offsets,
                                                      const uint32_t* __restrict__ order,
                                                      const uint64_t* __restrict__ off_out,
                                                      const uint64_t* __restrict__ bounds, uint64_t m,
                                                      uint64_t total, uint8_t* __restrict__ out) {
  emit_word<kST>(blob, key_end8, off_out, bounds, m, total, out, [&](uint64_t r) { return offsets[order[r]]; });
}

}  // namespace

// Scratch of the sort and the gather, kept in the context and grown as needed.  Per object:
// two packed and two word buffers (4 x 8 B), the scan (8 B), the positions (4 B) and two
// segment tables of at most m / 2 + 1 entries (4 B together): 48 B, plus rocPRIM's temporary.
struct SortScratch {
  uint64_t *packed[2] = {nullptr, nullptr}, *word[2] = {nullptr, nullptr}, *v = nullptr;
  uint32_t *fpos = nullptr, *delta[2] = {nullptr, nullptr};
  uint64_t cap = 0;  // keys
  SortTop* top = nullptr;
  unsigned long long* bad = nullptr;  // the gather's first order entry out of range
  uint64_t* bounds = nullptr;         // the gather chunks' first keys
  uint64_t bounds_cap = 0;
  PrimTmp tmp;
  void release() {
    for (int b = 0; b < 2; ++b) {
      dfree(packed[b]);
      dfree(word[b]);
      dfree(delta[b]);
    }
    dfree(v);
    dfree(fpos);
    dfree(top);
    dfree(bad);
    dfree(bounds);
    tmp.release();
    cap = bounds_cap = 0;
  }
};

void sort_scratch_free(s3imph_ctx* c) {
  if (c->srt) {
    c->srt->release();
    delete c->srt;
    c->srt = nullptr;
  }
}

namespace {

unsigned blocks(uint64_t count) { return (unsigned)((count + kST - 1) / kST); }

}  // namespace

// The order of m keys in HBM: order[j] = input index of the j-th key in byte order.  Waits for
// the stream.
int sort_objects(s3imph_ctx* c, const uint8_t* keys, const uint64_t* koff, uint64_t m, uint32_t* order,
                 s3imph_sort_info* info, hipStream_t s, std::string* msg) {
  std::memset(info, 0, sizeof *info);
  info->first_unsorted = UINT64_MAX;
  info->n_objects = m;
  if (m >> 32) {
    *msg = "sort: 2^32 objects or more (the order is a uint32)";
    return S3IMPH_ERR_INVALID;
  }
  if (m == 0) return S3IMPH_OK;
  if (!c->srt) c->srt = new SortScratch();
  SortScratch& a = *c->srt;
  if (!a.top) dalloc(a.top, 1);
  const SortTop top0{~0ull, 0, 0};
  SortTop top = top0;
  uint64_t ends[2] = {0, 0};
  HIPCHECK(hipMemcpyAsync(a.top, &top0, sizeof top0, hipMemcpyHostToDevice, s));
  k_sort_check<<<blocks(m), kST, 0, s>>>(keys, koff, m, a.top);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(&top, a.top, sizeof top, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&ends[0], koff, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&ends[1], koff + m, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  info->key_bytes = ends[1] - ends[0];
  info->first_unsorted = top.first_unsorted;
  if (top.first_unsorted == ~0ull) {  // (f) already in order: the identity
    info->n_equal = top.n_equal;
    k_sort_iota<<<blocks(m), kST, 0, s>>>(order, m);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    return S3IMPH_OK;
  }
  if (m > a.cap) {
    a.cap = 0;
    for (int b = 0; b < 2; ++b) {
      dalloc(a.packed[b], m);
      dalloc(a.word[b], m);
      dalloc(a.delta[b], m / 2 + 1);
    }
    dalloc(a.v, m + 1);
    dalloc(a.fpos, m);
    a.cap = m;
  }
  // the check counted the equal neighbours of the INPUT order; the rounds count the sorted one's
  HIPCHECK(hipMemsetAsync(&a.top->n_equal, 0, 8, s));
  k_sort_init<<<blocks(m), kST, 0, s>>>(a.packed[0], a.delta[0], m);
  HIPCHECK(hipGetLastError());
  const uint64_t max_rounds = (top.max_len + 1 + 6) / 7;
  uint64_t active = m, segs = 1;
  uint32_t round = 0;
  uint64_t *act = a.packed[0], *oth = a.packed[1];  // the active set, the other packed buffer
  int cur = 0;                                      // delta[cur] is the active set's segment table
  while (active) {
    if (round >= max_rounds) {
      *msg = "sort: keys unresolved after " + std::to_string(round) + " rounds";
      return S3IMPH_ERR_INTERNAL;
    }
    if (c->debug)
      std::fprintf(stderr, "[s3imph] sort round %u: %llu active in %llu segments\n", round,
                   (unsigned long long)active, (unsigned long long)segs);
    k_sort_words<<<blocks(active), kST, 0, s>>>(keys, koff, m, act, active, 7ull * round, a.word[0]);
    HIPCHECK(hipGetLastError());
    // stable by word, then stable by segment: ordered by (segment, word, input index)
    sort_pairs(a.tmp, a.word[0], a.word[1], act, oth, active, 0, 64, s);
    uint64_t *pk = oth, *wd = a.word[1], *next = act;  // the sorted set, and the buffer now free
    if (segs > 1) {
      unsigned bits = 1;
      while (bits < 32 && ((segs - 1) >> bits)) ++bits;
      sort_pairs(a.tmp, oth, act, a.word[1], a.word[0], active, 32, 32 + bits, s);
      pk = act;
      wd = a.word[0];
      next = oth;
    }
    k_sort_mark<<<blocks(active + 1), kST, 0, s>>>(pk, wd, a.delta[cur], active, order, a.fpos, a.v, a.top);
    HIPCHECK(hipGetLastError());
    scan_u64(a.tmp, a.v, active + 1, 0, s);
    k_sort_compact<<<blocks(active), kST, 0, s>>>(pk, a.fpos, a.v, active, next, a.delta[cur ^ 1]);
    HIPCHECK(hipGetLastError());
    uint64_t tot = 0;
    HIPCHECK(hipMemcpyAsync(&tot, a.v + active, 8, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    act = next;
    oth = pk;
    cur ^= 1;
    active = tot & 0xffffffffull;
    segs = tot >> 32;
    ++round;
  }
  HIPCHECK(hipMemcpyAsync(&top, a.top, sizeof top, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  info->n_equal = top.n_equal;
  info->rounds = round;
  return S3IMPH_OK;
}

// The listing in the order `order`, out of place.  Waits for the stream.
int gather_objects(s3imph_ctx* c, const uint8_t* keys, const uint64_t* koff, const uint64_t* sizes,
                   const uint8_t* tiers, uint64_t m, const uint32_t* order, uint8_t* keys_out, uint64_t keys_cap,
                   uint64_t* off_out, uint64_t* sizes_out, uint8_t* tiers_out, hipStream_t s, std::string* msg) {
  if (m >> 32) {
    *msg = "sort: 2^32 objects or more (the order is a uint32)";
    return S3IMPH_ERR_INVALID;
  }
  if (m == 0) {
    HIPCHECK(hipMemsetAsync(off_out, 0, 8, s));
    HIPCHECK(hipStreamSynchronize(s));
    return S3IMPH_OK;
  }
  if (!c->srt) c->srt = new SortScratch();
  SortScratch& a = *c->srt;
  if (!a.bad) dalloc(a.bad, 1);
  HIPCHECK(hipMemsetAsync(a.bad, 0xff, 8, s));
  k_gather_meta<<<blocks(m + 1), kST, 0, s>>>(koff, sizes, tiers, m, order, off_out, sizes_out, tiers_out, a.bad);
  HIPCHECK(hipGetLastError());
  scan_u64(a.tmp, off_out, m + 1, 0, s);
  unsigned long long bad = 0;
  uint64_t total = 0, key_end = 0;
  HIPCHECK(hipMemcpyAsync(&bad, a.bad, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&total, off_out + m, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&key_end, koff + m, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  if (bad != ~0ull) {
    *msg = "sort: order[" + std::to_string(bad) + "] is not an index below " + std::to_string(m);
    return S3IMPH_ERR_INVALID;
  }
  if (keys_cap < ((total + 7) & ~7ull)) {
    *msg = "sort: the gathered keys need " + std::to_string((total + 7) & ~7ull) + " blob bytes";
    return S3IMPH_ERR_INVALID;
  }
  const uint64_t nw = (total + 7) / 8;
  if (nw) {
    if (!keys_out) {
      *msg = "sort: null output array";
      return S3IMPH_ERR_INVALID;
    }
    const uint64_t chunks = (nw + kST - 1) / kST;
    grow(a.bounds, a.bounds_cap, chunks);
    k_gather_bounds<<<blocks(chunks), kST, 0, s>>>(off_out, m + 1, 8ull * kST, chunks, a.bounds);
    k_gather_bytes<<<(unsigned)chunks, kST, 0, s>>>(keys, (key_end + 7) & ~7ull, koff, order, off_out, a.bounds, m,
                                                    total, keys_out);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
  }
  return S3IMPH_OK;
}

}  // namespace s3imph

using namespace s3imph;

extern "C" {

int s3imph_sort_objects_device(s3imph_ctx* c, const uint8_t* d_keys, const uint64_t* d_key_offsets, uint64_t m,
                               uint32_t* d_order, s3imph_sort_info* info, void* stream) {
  if (!c || !info || (m >> 32) || (m && (!d_keys || !d_key_offsets || !d_order))) return S3IMPH_ERR_INVALID;
  return device_entry(c, "sort: ", [&](std::string& msg) {
    hipStream_t s = use_device(c->device, stream, c->own_stream);
    return retry_on_nomem(c, s, &msg, [&] {
      return sort_objects(c, d_keys, d_key_offsets, m, d_order, info, s, &msg);
    });
  });
}

int s3imph_gather_objects_device(s3imph_ctx* c, const uint8_t* d_keys, const uint64_t* d_key_offsets,
                                 const uint64_t* d_sizes, const uint8_t* d_tiers, uint64_t m, const uint32_t* d_order,
                                 uint8_t* d_keys_out, uint64_t keys_cap, uint64_t* d_offsets_out,
                                 uint64_t* d_sizes_out, uint8_t* d_tiers_out, void* stream) {
  if (!c || !d_offsets_out || (m >> 32) || (m && (!d_keys || !d_key_offsets || !d_order))) return S3IMPH_ERR_INVALID;
  if (!d_sizes != !d_sizes_out || !d_tiers != !d_tiers_out) return S3IMPH_ERR_INVALID;
  return device_entry(c, "sort: ", [&](std::string& msg) {
    hipStream_t s = use_device(c->device, stream, c->own_stream);
    return retry_on_nomem(c, s, &msg, [&] {
      return gather_objects(c, d_keys, d_key_offsets, d_sizes, d_tiers, m, d_order, d_keys_out, keys_cap,
                            d_offsets_out, d_sizes_out, d_tiers_out, s, &msg);
    });
  });
}

int s3imph_sort_objects_host(int device, const uint8_t* keys, const uint64_t* key_offsets, uint64_t m,
                             uint32_t** order, s3imph_sort_info* info, char* err, size_t errlen) {
  if (!order || !info || (m >> 32) || !listing_given(keys, key_offsets, m)) return S3IMPH_ERR_INVALID;
  *order = nullptr;
  std::memset(info, 0, sizeof *info);
  info->first_unsorted = UINT64_MAX;
  if (m == 0) return S3IMPH_OK;
  uint32_t* out = static_cast<uint32_t*>(std::malloc(m * sizeof(uint32_t)));
  if (!out) {
    set_err(err, errlen, "sort: out of host memory");
    return S3IMPH_ERR_NOMEM;
  }
  const int rc = host_entry(device, "sort: ", err, errlen, [&](s3imph_ctx* c, hipStream_t s, std::string& msg) {
    DevGuard g;
    uint8_t* d_keys = nullptr;
    uint64_t* d_koff = nullptr;
    uint32_t* d_order = nullptr;
    upload_keys(c, g, keys, key_offsets, m, d_keys, d_koff);
    g.make(d_order, m);
    const int rc2 = sort_objects(c, d_keys, d_koff, m, d_order, info, s, &msg);
    if (rc2 == S3IMPH_OK) staged_copy(c, false, out, d_order, m * 4);
    return rc2;
  });
  if (rc == S3IMPH_OK)
    *order = out;
  else
    std::free(out);
  return rc;
}

int s3imph_index_from_unsorted_objects_host(int device, const uint8_t* keys, const uint64_t* key_offsets,
                                            const uint64_t* sizes, const uint8_t* tiers, uint64_t m,
                                            uint32_t max_depth, const char* out_dir, char* err, size_t errlen) {
  if (m >> 32) {
    set_err(err, errlen, "sort: 2^32 objects or more (the order is a uint32)");
    return S3IMPH_ERR_INVALID;
  }
  return index_from_objects(device, keys, key_offsets, sizes, tiers, m, max_depth, out_dir, true, err, errlen);
}

}  // extern "C"
