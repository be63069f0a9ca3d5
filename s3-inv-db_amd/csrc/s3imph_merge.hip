// s3imph_merge.hip — the back of the external-sort pipeline on the GPU: sorted runs of prefix
// rows are merged in HBM into the rows IndexBuilder consumes, and an index is built in chunks
// from a listing that does not fit one GPU (include/s3imph.h section 5i).
//
// Reference (pkg/extsort):
//   pipeline.go:703-783        flushAggregator: the aggregator drained into a sorted run;
//   pipeline.go:786-914        runMergeBuildPhase: the runs k-way merged into IndexBuilder;
//   merger.go:104-140          MergeIterator.Next: the smallest prefix of all runs, every row
//                              with an equal prefix folded into it (:125-137);
//   types.go:82-91             PrefixRow.Merge: Count, TotalBytes, TierCounts, TierBytes summed;
//   parallel_merge.go:122-190  ParallelMerger.MergeAll: rounds over groups of runs.
//
// GPU formulation.  The input is ONE row set sorted in K stretches.  The order is
// total on (key, run, row), so the place of row i of run r in the merged, not yet folded, sequence is
//     dest = i + sum_{s<r} #{j : key_s[j] <= key} + sum_{s>r} #{j : key_s[j] < key}:
// no heap, one independent search per (row, other run).  Every kMS-th row of a run is a splitter
// that does the full binary searches (k_merge_splitters); both bounds are monotone in the key, so
// a row between two splitters searches only between their answers (k_merge_rank): short windows,
// local in memory.  The fold: merged row j is a head iff its key differs from merged row j - 1's
// (k_merge_heads); one scan numbers the heads, one sums their byte lengths; an output row sums its
// members, which are contiguous in the merged order (k_merge_rows); the bytes are copied by output
// word from the head's place in the input blob (emit_word, s3imph_keys.h).
#include <cstring>

#include "s3imph_entry.h"
#include "s3imph_keys.h"
#include "s3imph_prim.h"
#include "s3imph_tiers.h"

namespace s3imph {

namespace {

constexpr int kMT = 256;       // lanes per workgroup: one row / one search / one output word each
constexpr uint32_t kMS = 64;   // sample step: every kMS-th row of a run is a splitter
constexpr uint32_t kMaxRuns = S3IMPH_MERGE_MAX_RUNS;
constexpr uint64_t kMaxRows = 1ull << 30;  // what the MPHF build takes on one GPU
constexpr int kNT = S3IMPH_NUM_TIERS;

// What the passes report: the smallest row below its predecessor in its run, the deepest head,
// the tiers of the merged rows.
struct MergeTop {
  unsigned long long first_unsorted;
  unsigned maxd, mask;
};

// The run of global row i (or of global tile i): the last r with starts[r] <= i.  starts has
// k + 1 non-decreasing entries and starts[k] > i, so an empty run is never the answer.
__device__ __forceinline__ uint32_t run_of(const uint64_t* __restrict__ starts, uint32_t k, uint64_t i) {
  return (uint32_t)(first_above(starts, 0, (uint64_t)k + 1, i) - 1);
}

// First j in [lo, hi) whose key sorts after the key (a0, alen) (kUpper) or not before it (!kUpper),
// or hi: lo + the number of rows of [lo, hi) that are <= (kUpper) or < (!kUpper) the key.
template <bool kUpper>
__device__ __forceinline__ uint64_t key_bound(const uint8_t* __restrict__ blob, const uint64_t* __restrict__ offsets,
                                              uint64_t end8, uint64_t lo, uint64_t hi, uint64_t a0, uint64_t alen) {
  uint64_t len = hi - lo;
  while (len) {
    const uint64_t h = len >> 1;
    const uint64_t b0 = offsets[lo + h];
    const int c = compare_keys(blob, b0, offsets[lo + h + 1] - b0, a0, alen, end8);
    const bool right = kUpper ? c <= 0 : c < 0;
    lo = right ? lo + h + 1 : lo;
    len = right ? len - h - 1 : h;
  }
  return lo;
}

// Row against its predecessor WITHIN its run (never across a run boundary), word by word: the
// comparison k_sort_check / k_agg_keys make.  One atomic per wave, and only while it can still
// lower the minimum.
__global__ __launch_bounds__(kMT) void k_merge_check(const uint8_t* __restrict__ blob,
                                                     const uint64_t* __restrict__ offsets, uint64_t n,
                                                     const uint64_t* __restrict__ starts, uint32_t k,
                                                     MergeTop* __restrict__ top) {
  const uint64_t i = (uint64_t)blockIdx.x * kMT + threadIdx.x;
  const uint64_t end8 = (offsets[n] + 7) & ~7ull;
  bool unsorted = false;
  if (i > 0 && i < n && i > starts[run_of(starts, k, i)]) {
    const uint64_t b0 = offsets[i], p0 = offsets[i - 1];
    unsorted = compare_keys(blob, b0, offsets[i + 1] - b0, p0, b0 - p0, end8) < 0;
  }
  const uint64_t bad = __ballot(unsorted);
  if (lane_id() == 0 && bad) {
    const unsigned long long first = i + (unsigned)__builtin_ctzll(bad);
    if (first < *reinterpret_cast<volatile unsigned long long*>(&top->first_unsorted))
      atomicMin(&top->first_unsorted, first);
  }
}

// The splitter table: one lane per (tile T, other run s), so the binary searches' dependent loads
// overlap.  Tile T is tile t = T - tbase[r] of run r; its splitter is row t * kMS of that run.
// W[T * k + s] = the rows of run s that sort before the splitter in the (key, run, row) order:
// those <= it for s < r, those < it for s > r (W[T * k + r] is not read).
__global__ __launch_bounds__(kMT) void k_merge_splitters(const uint8_t* __restrict__ blob,
                                                         const uint64_t* __restrict__ offsets, uint64_t n,
                                                         const uint64_t* __restrict__ starts,
                                                         const uint64_t* __restrict__ tbase, uint32_t k,
                                                         uint64_t tiles, uint32_t* __restrict__ W) {
  const uint64_t idx = (uint64_t)blockIdx.x * kMT + threadIdx.x;
  if (idx >= tiles * k) return;
  const uint64_t T = idx / k;
  const uint32_t s = (uint32_t)(idx % k);
  const uint32_t r = run_of(tbase, k, T);
  uint32_t w = 0;
  if (s != r) {
    const uint64_t end8 = (offsets[n] + 7) & ~7ull;
    const uint64_t row = starts[r] + (T - tbase[r]) * kMS;
    const uint64_t a0 = offsets[row], alen = offsets[row + 1] - a0;
    const uint64_t lo = starts[s], hi = starts[s + 1];
    const uint64_t p = s < r ? key_bound<true>(blob, offsets, end8, lo, hi, a0, alen)
                             : key_bound<false>(blob, offsets, end8, lo, hi, a0, alen);
    w = (uint32_t)(p - lo);
  }
  W[idx] = w;
}

// One lane per row: its place in the merged order.  In every other run it searches only between
// its tile's splitter answer and the next tile's (up to the run's end for the last tile), and
// writes src[dest] = its global row.
__global__ __launch_bounds__(kMT) void k_merge_rank(const uint8_t* __restrict__ blob,
                                                    const uint64_t* __restrict__ offsets, uint64_t n,
                                                    const uint64_t* __restrict__ starts,
                                                    const uint64_t* __restrict__ tbase, uint32_t k,
                                                    const uint32_t* __restrict__ W, uint32_t* __restrict__ src) {
  const uint64_t i = (uint64_t)blockIdx.x * kMT + threadIdx.x;
  if (i >= n) return;
  const uint64_t end8 = (offsets[n] + 7) & ~7ull;
  const uint32_t r = run_of(starts, k, i);
  const uint64_t li = i - starts[r];
  const uint64_t T = tbase[r] + li / kMS;
  const bool last = T + 1 == tbase[r + 1];
  const uint64_t a0 = offsets[i], alen = offsets[i + 1] - a0;
  uint64_t dest = li;
  for (uint32_t s = 0; s < k; ++s) {
    const uint64_t s0 = starts[s], ns = starts[s + 1] - s0;
    if (s == r || ns == 0) continue;
    const uint64_t lo = s0 + W[T * k + s];
    const uint64_t hi = s0 + (last ? ns : (uint64_t)W[(T + 1) * k + s]);
    const uint64_t p = s < r ? key_bound<true>(blob, offsets, end8, lo, hi, a0, alen)
                             : key_bound<false>(blob, offsets, end8, lo, hi, a0, alen);
    dest += p - s0;
  }
  if (dest < n) src[dest] = (uint32_t)i;  // always, for runs the check pass found sorted
}

// Merged row j is a head iff its key differs from merged row j - 1's.  flag[j] = 1 for a head,
// hlen[j] = its byte length; entry n of both is the zero their exclusive scans turn into the
// totals.  The deepest head goes to top->maxd (one atomic per wave).
__global__ __launch_bounds__(kMT) void k_merge_heads(const uint8_t* __restrict__ blob,
                                                     const uint64_t* __restrict__ offsets, uint64_t n,
                                                     const uint32_t* __restrict__ src,
                                                     const uint32_t* __restrict__ depth, uint64_t* __restrict__ flag,
                                                     uint64_t* __restrict__ hlen, MergeTop* __restrict__ top) {
  const uint64_t j = (uint64_t)blockIdx.x * kMT + threadIdx.x;
  uint32_t d = 0;
  if (j < n) {
    const uint64_t end8 = (offsets[n] + 7) & ~7ull;
    const uint64_t a = src[j];
    const uint64_t a0 = offsets[a], alen = offsets[a + 1] - a0;
    bool head = j == 0;
    if (!head) {
      const uint64_t p = src[j - 1];
      const uint64_t p0 = offsets[p], plen = offsets[p + 1] - p0;
      head = plen != alen || compare_keys(blob, a0, alen, p0, plen, end8) != 0;
    }
    flag[j] = head ? 1 : 0;
    hlen[j] = head ? alen : 0;
    if (head) d = depth[a];
  } else if (j == n) {
    flag[n] = 0;
    hlen[n] = 0;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) d = max(d, __shfl_xor(d, o));
  if (lane_id() == 0 && d) atomicMax(&top->maxd, d);
}

// After the scan of the flags (flag[j] = heads before j): output row flag[j] starts at merged row j.
__global__ __launch_bounds__(kMT) void k_merge_place(const uint64_t* __restrict__ flag, uint64_t n,
                                                     uint32_t* __restrict__ headpos) {
  const uint64_t j = (uint64_t)blockIdx.x * kMT + threadIdx.x;
  if (j < n && flag[j + 1] != flag[j]) headpos[flag[j]] = (uint32_t)j;
}

// One lane per output row: its members are merged rows [headpos[o], headpos[o + 1]).  The depth
// comes from the first member (the lowest run, then the lowest row), the columns are summed
// (wrapping).  Tier columns are column-major in (stride) and out (n_cap).  !kEmit is the plan's
// pass: only the tiers of the merged rows, by wave OR and one atomicOr per wave.
template <bool kTiers, bool kEmit>
__global__ __launch_bounds__(kMT) void k_merge_rows(
    const uint32_t* __restrict__ src, const uint32_t* __restrict__ headpos, uint64_t n, uint64_t n_out,
    const uint64_t* __restrict__ in_off, const uint32_t* __restrict__ in_depth, const uint64_t* __restrict__ in_cnt,
    const uint64_t* __restrict__ in_bytes, const uint64_t* __restrict__ in_tc, const uint64_t* __restrict__ in_tb,
    uint64_t stride, const uint64_t* __restrict__ hoff, uint64_t blob_bytes, uint64_t* __restrict__ offsets,
    uint32_t* __restrict__ depth, uint64_t* __restrict__ cnt, uint64_t* __restrict__ bytes,
    uint64_t* __restrict__ tc, uint64_t* __restrict__ tb, uint64_t n_cap, uint64_t* __restrict__ rowsrc,
    MergeTop* __restrict__ top) {
  const uint64_t o = (uint64_t)blockIdx.x * kMT + threadIdx.x;
  unsigned mask = 0;
  if (o < n_out) {
    const uint64_t j0 = headpos[o], j1 = o + 1 < n_out ? headpos[o + 1] : n;
    if (kEmit) {
      const uint64_t first = src[j0];
      uint64_t c = 0, b = 0;
      for (uint64_t j = j0; j < j1; ++j) {
        const uint64_t a = src[j];
        c += in_cnt[a];
        b += in_bytes[a];
      }
      offsets[o] = hoff[j0];
      if (o == 0) offsets[n_out] = blob_bytes;
      rowsrc[o] = in_off[first];
      depth[o] = in_depth[first];
      cnt[o] = c;
      bytes[o] = b;
    }
    if (kTiers) {
      uint64_t c[kNT], b[kNT];
#pragma unroll
      for (int t = 0; t < kNT; ++t) {
        c[t] = 0;
        b[t] = 0;
      }
      for (uint64_t j = j0; j < j1; ++j) {
        const uint64_t a = src[j];
#pragma unroll
        for (int t = 0; t < kNT; ++t) {
          c[t] += in_tc[(uint64_t)t * stride + a];
          b[t] += in_tb[(uint64_t)t * stride + a];
        }
      }
#pragma unroll
      for (int t = 0; t < kNT; ++t) {
        if (c[t] | b[t]) mask |= 1u << t;
        if (kEmit) {
          tc[(uint64_t)t * n_cap + o] = c[t];
          tb[(uint64_t)t * n_cap + o] = b[t];
        }
      }
    }
  }
  if (kTiers && !kEmit) {
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) mask |= __shfl_xor(mask, w);
    if (lane_id() == 0 && mask) atomicOr(&top->mask, mask);
  }
}

// The byte emit's chunks: the output row of each chunk's first word (chunk_owner), one lane per chunk.
__global__ __launch_bounds__(kMT) void k_merge_bounds(const uint64_t* __restrict__ U, uint64_t entries,
                                                      uint64_t step, uint64_t nchunks, uint64_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kMT + threadIdx.x;
  if (t < nchunks) out[t] = chunk_owner(U, entries, step, 0, t);
}

// The output blob by 8-byte word (emit_word): the source of output row o is its head's key in the
// input blob, rowsrc[o] — the point of the single-blob input layout.
__global__ __launch_bounds__(kMT) void k_merge_bytes(const uint8_t* __restrict__ blob, uint64_t end8,
                                                     const uint64_t* __restrict__ offsets,
                                                     const uint64_t* __restrict__ rowsrc,
                                                     const uint64_t* __restrict__ bounds, uint64_t n_out,
                                                     uint64_t blob_bytes, uint8_t* __restrict__ out) {
  emit_word<kMT>(blob, end8, offsets, bounds, n_out, blob_bytes, out, [&](uint64_t r) { return rowsrc[r]; });
}

unsigned blocks(uint64_t lanes) { return (unsigned)((lanes + kMT - 1) / kMT); }

}  // namespace

// Scratch of the merge and the last plan, kept in the context and grown as needed.
struct MergeScratch {
  uint32_t *src = nullptr, *headpos = nullptr;
  uint64_t *flag = nullptr, *hlen = nullptr, *rowsrc = nullptr;
  uint64_t cap = 0;  // input rows
  uint32_t* W = nullptr;
  uint64_t w_cap = 0;
  uint64_t* meta = nullptr;  // run starts (kMaxRuns + 1), tiles before each run (kMaxRuns + 1)
  MergeTop* top = nullptr;
  uint64_t* bounds = nullptr;
  uint64_t bounds_cap = 0;
  PrimTmp tmp;
  // the last plan
  bool have_plan = false, tiered = false;
  const uint8_t* blob = nullptr;
  const uint64_t *offsets = nullptr, *cnt = nullptr, *bytes = nullptr, *tc = nullptr, *tb = nullptr;
  const uint32_t* depth = nullptr;
  uint64_t stride = 0, n = 0, n_out = 0, blob_bytes = 0, end8 = 0;
  void release() {
    dfree(src);
    dfree(headpos);
    dfree(flag);
    dfree(hlen);
    dfree(rowsrc);
    dfree(W);
    dfree(meta);
    dfree(top);
    dfree(bounds);
    tmp.release();
    cap = w_cap = bounds_cap = 0;
    have_plan = false;
  }
};

void merge_scratch_free(s3imph_ctx* c) {
  if (c->mrg) {
    c->mrg->release();
    delete c->mrg;
    c->mrg = nullptr;
  }
}

namespace {

// Every check of the plan's arguments that needs no device: "" when they are good.
std::string merge_args_bad(const uint8_t* blob, const uint64_t* offsets, const uint32_t* depth, const uint64_t* cnt,
                           const uint64_t* bytes, const uint64_t* tc, const uint64_t* tb, uint64_t stride,
                           const uint64_t* run_starts, uint32_t k) {
  if ((tc == nullptr) != (tb == nullptr)) return "merge: one tier array without the other";
  if (k > kMaxRuns)
    return "merge: " + std::to_string(k) + " runs, more than S3IMPH_MERGE_MAX_RUNS (" + std::to_string(kMaxRuns) + ")";
  if (!run_starts) return k ? "merge: null run_starts" : "";
  if (run_starts[0] != 0) return "merge: run_starts[0] is not 0";
  for (uint32_t r = 0; r < k; ++r)
    if (run_starts[r + 1] < run_starts[r]) return "merge: run_starts decreases at run " + std::to_string(r + 1);
  const uint64_t n = run_starts[k];
  if (n >= (1ull << 32)) return "merge: 2^32 input rows or more (the merged order is a uint32_t)";
  if (n && (!blob || !offsets || !depth || !cnt || !bytes)) return "merge: null input array";
  if (n && tc && stride < n) return "merge: tier_stride below the row count";
  return "";
}

// Plan: the order, the fold and the scans for n rows in k runs in HBM; fills *info, keeps the plan
// in the context.  The arguments have passed merge_args_bad.  Waits for the stream.
int merge_plan(s3imph_ctx* c, const uint8_t* blob, const uint64_t* offsets, const uint32_t* depth, const uint64_t* cnt,
               const uint64_t* bytes, const uint64_t* tc, const uint64_t* tb, uint64_t stride,
               const uint64_t* run_starts, uint32_t k, s3imph_merge_info* info, hipStream_t s, std::string* msg) {
  std::memset(info, 0, sizeof *info);
  info->first_unsorted = UINT64_MAX;
  info->n_runs = k;
  const uint64_t n = run_starts ? run_starts[k] : 0;
  info->n_in = n;
  if (!c->mrg) c->mrg = new MergeScratch();
  MergeScratch& a = *c->mrg;
  a.have_plan = false;
  a.tiered = tc != nullptr;
  if (n == 0) {
    a.n = a.n_out = a.blob_bytes = 0;
    a.have_plan = true;
    return S3IMPH_OK;
  }
  if (n > a.cap) {
    a.cap = 0;
    dalloc(a.src, n);
    dalloc(a.headpos, n);
    dalloc(a.flag, n + 1);
    dalloc(a.hlen, n + 1);
    dalloc(a.rowsrc, n);
    a.cap = n;
  }
  if (!a.meta) dalloc(a.meta, 2 * (kMaxRuns + 1));
  if (!a.top) dalloc(a.top, 1);
  // the runs' rows and tiles: tile t of run r is rows [t kMS, (t + 1) kMS) of it
  uint64_t meta[2 * (kMaxRuns + 1)];
  uint64_t tiles = 0;
  for (uint32_t r = 0; r <= k; ++r) {
    meta[r] = run_starts[r];
    meta[k + 1 + r] = tiles;
    if (r < k) tiles += (run_starts[r + 1] - run_starts[r] + kMS - 1) / kMS;
  }
  const uint64_t *d_starts = a.meta, *d_tbase = a.meta + k + 1;
  grow(a.W, a.w_cap, tiles * k);
  const MergeTop top0{~0ull, 0, 0};
  MergeTop top = top0;
  uint64_t end = 0;
  HIPCHECK(hipMemcpyAsync(a.meta, meta, 2 * (k + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(a.top, &top0, sizeof top0, hipMemcpyHostToDevice, s));
  k_merge_check<<<blocks(n), kMT, 0, s>>>(blob, offsets, n, d_starts, k, a.top);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(&top, a.top, sizeof top, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&end, offsets + n, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));  // the meta array on the stack has been read, too
  info->first_unsorted = top.first_unsorted;
  if (top.first_unsorted != ~0ull) {
    const uint64_t i = top.first_unsorted;
    uint32_t r = 0;
    while (r + 1 < k && run_starts[r + 1] <= i) ++r;
    *msg = "merge: run " + std::to_string(r) + " is not byte-sorted: row " + std::to_string(i) +
           " is smaller than row " + std::to_string(i - 1);
    return S3IMPH_ERR_INVALID;
  }
  HIPCHECK(hipMemsetAsync(a.src, 0, n * 4, s));  // every entry a valid row whatever the rank pass writes
  k_merge_splitters<<<blocks(tiles * k), kMT, 0, s>>>(blob, offsets, n, d_starts, d_tbase, k, tiles, a.W);
  k_merge_rank<<<blocks(n), kMT, 0, s>>>(blob, offsets, n, d_starts, d_tbase, k, a.W, a.src);
  k_merge_heads<<<blocks(n + 1), kMT, 0, s>>>(blob, offsets, n, a.src, depth, a.flag, a.hlen, a.top);
  HIPCHECK(hipGetLastError());
  scan_u64(a.tmp, a.flag, n + 1, 0, s);
  scan_u64(a.tmp, a.hlen, n + 1, 0, s);
  k_merge_place<<<blocks(n), kMT, 0, s>>>(a.flag, n, a.headpos);
  HIPCHECK(hipGetLastError());
  uint64_t tot[2] = {0, 0};
  HIPCHECK(hipMemcpyAsync(&tot[0], a.flag + n, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&tot[1], a.hlen + n, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  const uint64_t n_out = tot[0];
  if (a.tiered) {
    k_merge_rows<true, false><<<blocks(n_out), kMT, 0, s>>>(a.src, a.headpos, n, n_out, offsets, depth, cnt, bytes, tc,
                                                           tb, stride, a.hlen, tot[1], nullptr, nullptr, nullptr,
                                                           nullptr, nullptr, nullptr, 0, nullptr, a.top);
    HIPCHECK(hipGetLastError());
  }
  HIPCHECK(hipMemcpyAsync(&top, a.top, sizeof top, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  info->n_out = n_out;
  info->blob_bytes = tot[1];
  info->max_depth_seen = top.maxd;
  info->present_mask = top.mask;
  if (n_out > kMaxRows) {
    *msg = "merge: more than 2^30 prefixes on one GPU (the MPHF's level 0 past 2^31 positions): "
           "shard them over several GPUs";
    return S3IMPH_ERR_INVALID;
  }
  a.blob = blob;
  a.offsets = offsets;
  a.depth = depth;
  a.cnt = cnt;
  a.bytes = bytes;
  a.tc = tc;
  a.tb = tb;
  a.stride = stride;
  a.n = n;
  a.n_out = n_out;
  a.blob_bytes = tot[1];
  a.end8 = (end + 7) & ~7ull;
  a.have_plan = true;
  return S3IMPH_OK;
}

// Fill: the merged rows of the last plan.  Waits for the stream.
int merge_fill(s3imph_ctx* c, uint8_t* blob, uint64_t blob_cap, uint64_t* offsets, uint32_t* depth, uint64_t* cnt,
               uint64_t* bytes, uint64_t* tc, uint64_t* tb, uint64_t n_cap, hipStream_t s, std::string* msg) {
  if (!c->mrg || !c->mrg->have_plan) {
    *msg = "merge: fill without a plan";
    return S3IMPH_ERR_STATE;
  }
  MergeScratch& a = *c->mrg;
  const uint64_t cap8 = (a.blob_bytes + 7) & ~7ull;
  if (n_cap < a.n_out || blob_cap < cap8) {
    *msg = "merge: the plan needs " + std::to_string(a.n_out) + " rows and " + std::to_string(cap8) + " blob bytes";
    return S3IMPH_ERR_INVALID;
  }
  if (!offsets || (a.n_out && (!depth || !cnt || !bytes)) || (a.blob_bytes && !blob) ||
      (a.n_out && a.tiered && (!tc || !tb))) {
    *msg = "merge: null output array";
    return S3IMPH_ERR_INVALID;
  }
  if (a.n_out == 0) {
    HIPCHECK(hipMemsetAsync(offsets, 0, 8, s));
    HIPCHECK(hipStreamSynchronize(s));
    return S3IMPH_OK;
  }
  if (a.tiered)
    k_merge_rows<true, true><<<blocks(a.n_out), kMT, 0, s>>>(a.src, a.headpos, a.n, a.n_out, a.offsets, a.depth, a.cnt,
                                                            a.bytes, a.tc, a.tb, a.stride, a.hlen, a.blob_bytes,
                                                            offsets, depth, cnt, bytes, tc, tb, n_cap, a.rowsrc,
                                                            a.top);
  else
    k_merge_rows<false, true><<<blocks(a.n_out), kMT, 0, s>>>(a.src, a.headpos, a.n, a.n_out, a.offsets, a.depth,
                                                             a.cnt, a.bytes, nullptr, nullptr, 0, a.hlen,
                                                             a.blob_bytes, offsets, depth, cnt, bytes, nullptr,
                                                             nullptr, n_cap, a.rowsrc, a.top);
  const uint64_t nw = (a.blob_bytes + 7) / 8;
  if (nw) {
    const uint64_t wchunks = (nw + kMT - 1) / kMT;
    grow(a.bounds, a.bounds_cap, wchunks);
    k_merge_bounds<<<blocks(wchunks), kMT, 0, s>>>(offsets, a.n_out + 1, 8ull * kMT, wchunks, a.bounds);
    k_merge_bytes<<<(unsigned)wchunks, kMT, 0, s>>>(a.blob, a.end8, offsets, a.rowsrc, a.bounds, a.n_out,
                                                    a.blob_bytes, blob);
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));
  return S3IMPH_OK;
}

// ---- runs in host memory ------------------------------------------------------------------

// A run the library owns (a round's result, or a run of a row set).
struct HostRun {
  std::vector<uint8_t> blob;
  std::vector<uint64_t> offsets, count, bytes, tcount, tbytes;
  std::vector<uint32_t> depth;
  uint64_t n = 0;
  bool tiers = false;
  s3imph_row_run view() const {
    s3imph_row_run r;
    r.blob = blob.data();
    r.offsets = offsets.data();
    r.depth = depth.data();
    r.count = count.data();
    r.bytes = bytes.data();
    r.tier_count = tiers ? tcount.data() : nullptr;
    r.tier_bytes = tiers ? tbytes.data() : nullptr;
    r.n = n;
    r.tier_stride = n;
    return r;
  }
};

// The shape checks of host runs; *tiers = whether they carry tier columns, *rows = their rows.
std::string runs_bad(const s3imph_row_run* runs, uint64_t k, bool* tiers, uint64_t* rows) {
  *tiers = false;
  *rows = 0;
  if (k && !runs) return "merge: null runs";
  bool seen = false;
  for (uint64_t r = 0; r < k; ++r) {
    const s3imph_row_run& u = runs[r];
    if (u.n == 0) continue;
    if (!u.offsets || !u.depth || !u.count || !u.bytes || (!u.blob && u.offsets[u.n] != u.offsets[0]))
      return "merge: run " + std::to_string(r) + " has a null array";
    if ((u.tier_count == nullptr) != (u.tier_bytes == nullptr))
      return "merge: run " + std::to_string(r) + " has one tier array without the other";
    const bool t = u.tier_count != nullptr;
    if (t && u.tier_stride < u.n) return "merge: run " + std::to_string(r) + " has a tier_stride below its rows";
    if (seen && t != *tiers) return "merge: runs with and without tier columns are mixed";
    seen = true;
    *tiers = t;
    if (u.offsets[u.n] < u.offsets[0]) return "merge: run " + std::to_string(r) + " has decreasing offsets";
    *rows += u.n;
  }
  return "";
}

// Rows in HBM -> a run in host memory.
void download_rows(s3imph_ctx* c, const DevRows& r, bool tiers, HostRun* h) {
  h->n = r.n;
  h->tiers = tiers;
  h->blob.resize(r.blob_bytes);
  h->offsets.resize(r.n + 1);
  h->depth.resize(r.n);
  h->count.resize(r.n);
  h->bytes.resize(r.n);
  if (tiers) {
    h->tcount.resize(kNT * r.n);
    h->tbytes.resize(kNT * r.n);
  }
  rows_to_host(c, r, tiers, h->blob.data(), h->offsets.data(), h->depth.data(), h->count.data(), h->bytes.data(),
               h->tcount.data(), h->tbytes.data());
}

// At most kMaxRuns host runs concatenated on upload (offsets rebased onto one blob), merged, the
// result left in HBM (owned by g); the input's device copy is freed before returning.  *info
// describes this group alone.  No row: out->n == 0 and nothing allocated.
int merge_group(s3imph_ctx* c, DevGuard& g, const s3imph_row_run* runs, uint32_t k, bool tiers, DevRows* out,
                s3imph_merge_info* info, std::string* msg) {
  hipStream_t s = c->own_stream;
  uint64_t starts[kMaxRuns + 1];
  uint64_t n = 0, nbytes = 0;
  starts[0] = 0;
  for (uint32_t r = 0; r < k; ++r) {
    n += runs[r].n;
    starts[r + 1] = n;
    if (runs[r].n) nbytes += runs[r].offsets[runs[r].n] - runs[r].offsets[0];
  }
  if (n >= (1ull << 32)) {
    *msg = "merge: 2^32 input rows or more in one round (the merged order is a uint32_t)";
    std::memset(info, 0, sizeof *info);
    info->first_unsorted = UINT64_MAX;
    info->n_in = n;
    info->n_runs = k;
    return S3IMPH_ERR_INVALID;
  }
  DevGuard gin;
  DevRows in;
  if (n) {
    gin.make(in.blob, ((nbytes + 7) & ~7ull) + 16);
    gin.make(in.offsets, n + 1);
    gin.make(in.depth, n);
    gin.make(in.ocnt, n);
    gin.make(in.tbytes, n);
    if (tiers) {
      gin.make(in.tier_count, kNT * n);
      gin.make(in.tier_bytes, kNT * n);
    }
    uint64_t at = 0;  // bytes placed so far
    for (uint32_t r = 0; r < k; ++r) {
      const s3imph_row_run& u = runs[r];
      if (!u.n) continue;
      const uint64_t row0 = starts[r], b0 = u.offsets[0], nb = u.offsets[u.n] - b0;
      if (nb) HIPCHECK(hipMemcpy(in.blob + at, u.blob + b0, nb, hipMemcpyHostToDevice));
      // offsets less b0 plus `at` (wrapping); entry row0 is rewritten with the value it had
      staged_copy(c, true, in.offsets + row0, u.offsets, (u.n + 1) * 8, b0 - at);
      staged_copy(c, true, in.depth + row0, u.depth, u.n * 4);
      staged_copy(c, true, in.ocnt + row0, u.count, u.n * 8);
      staged_copy(c, true, in.tbytes + row0, u.bytes, u.n * 8);
      for (int t = 0; tiers && t < kNT; ++t) {
        staged_copy(c, true, in.tier_count + t * n + row0, u.tier_count + t * u.tier_stride, u.n * 8);
        staged_copy(c, true, in.tier_bytes + t * n + row0, u.tier_bytes + t * u.tier_stride, u.n * 8);
      }
      at += nb;
    }
  }
  int rc = merge_plan(c, in.blob, in.offsets, in.depth, in.ocnt, in.tbytes, in.tier_count, in.tier_bytes, n, starts, k,
                      info, s, msg);
  if (rc != S3IMPH_OK) return rc;
  out->n = info->n_out;
  out->blob_bytes = info->blob_bytes;
  out->present_mask = info->present_mask;
  out->m = n;
  if (n) {
    const uint64_t cap8 = (info->blob_bytes + 7) & ~7ull;
    g.make(out->blob, cap8 + 16);
    g.make(out->offsets, out->n + 1);
    g.make(out->depth, out->n);
    g.make(out->ocnt, out->n);
    g.make(out->tbytes, out->n);
    if (tiers) {
      g.make(out->tier_count, kNT * out->n);
      g.make(out->tier_bytes, kNT * out->n);
    }
    rc = merge_fill(c, out->blob, cap8, out->offsets, out->depth, out->ocnt, out->tbytes, out->tier_count,
                    out->tier_bytes, out->n, s, msg);
  }
  c->mrg->have_plan = false;  // the input's device copy goes away with this call
  return rc;
}

// Any number of host runs merged into rows in HBM (owned by g): while there are more than
// kMaxRuns, groups of kMaxRuns CONTIGUOUS runs are merged and brought back to the host as the next
// round's runs (MergeAll's rounds).  *total describes the whole merge.
int merge_runs(s3imph_ctx* c, DevGuard& g, const s3imph_row_run* runs, uint64_t k, bool tiers, DevRows* out,
               s3imph_merge_info* total, std::string* msg) {
  std::memset(total, 0, sizeof *total);
  total->first_unsorted = UINT64_MAX;
  total->n_runs = (uint32_t)std::min<uint64_t>(k, UINT32_MAX);
  for (uint64_t r = 0; r < k; ++r) total->n_in += runs[r].n;
  std::vector<HostRun> held, next;
  std::vector<s3imph_row_run> views;
  bool first_round = true;
  while (k > kMaxRuns) {
    next.clear();
    uint64_t row0 = 0;
    for (uint64_t lo = 0; lo < k; lo += kMaxRuns) {
      const uint32_t cnt = (uint32_t)std::min<uint64_t>(kMaxRuns, k - lo);
      DevGuard g2;
      DevRows part;
      s3imph_merge_info gi;
      const int rc = merge_group(c, g2, runs + lo, cnt, tiers, &part, &gi, msg);
      if (rc != S3IMPH_OK) {
        if (first_round && gi.first_unsorted != UINT64_MAX) total->first_unsorted = row0 + gi.first_unsorted;
        return rc;
      }
      row0 += gi.n_in;
      next.emplace_back();
      if (part.n) download_rows(c, part, tiers, &next.back());
    }
    held.swap(next);
    views.clear();
    for (const HostRun& h : held) views.push_back(h.view());
    runs = views.data();
    k = views.size();
    first_round = false;
  }
  s3imph_merge_info gi;
  const int rc = merge_group(c, g, runs, (uint32_t)k, tiers, out, &gi, msg);
  if (first_round) total->first_unsorted = gi.first_unsorted;
  total->n_out = gi.n_out;
  total->blob_bytes = gi.blob_bytes;
  total->present_mask = gi.present_mask;
  total->max_depth_seen = gi.max_depth_seen;
  return rc;
}

// s3imph_index_from_rows_host: the merge, then the back half of the listing builds.
int index_from_rows(int device, const s3imph_row_run* runs, uint64_t k, const char* out_dir, char* err,
                    size_t errlen) {
  if (!out_dir) return S3IMPH_ERR_INVALID;
  bool tiers = false;
  uint64_t rows = 0;
  const std::string bad = runs_bad(runs, k, &tiers, &rows);
  if (!bad.empty()) {
    set_err(err, errlen, bad);
    return S3IMPH_ERR_INVALID;
  }
  const std::string dir = out_dir;
  if (!is_dir(dir)) {
    set_err(err, errlen, "create mph file: open " + dir + "/mph.bin: no such directory");
    return S3IMPH_ERR_IO;
  }
  IndexHostArrays h;
  if (rows) {
    // one device residency: the rows stay in HBM from the merge to the last array
    const int rc = host_entry(device, "merge: ", err, errlen, [&](s3imph_ctx* c, hipStream_t s, std::string& msg) {
      DevGuard g;
      DevRows r;
      s3imph_merge_info mi;
      const int rc2 = merge_runs(c, g, runs, k, tiers, &r, &mi, &msg);
      if (rc2 != S3IMPH_OK) return rc2;
      h.n = r.n;
      return index_arrays_from_rows(c, g, r, tiers, h, s, &msg);
    });
    if (rc != S3IMPH_OK) return rc;
  }
  return host_call("merge: ", err, errlen, [&](std::string& msg) { return write_index_dir(dir, h, tiers, &msg); });
}

}  // namespace

}  // namespace s3imph

using namespace s3imph;

// The runs of a chunked build, in host memory.
struct s3imph_rowset {
  int device = 0;
  uint32_t max_depth = 0;
  bool tiers = false;
  std::mutex mu;
  std::vector<HostRun> runs;
};

namespace {

// One chunk (a listing in any order, or CSV buffers) aggregated on the GPU into one more run.
int rowset_add_chunk(s3imph_rowset* rs, const uint8_t* keys, const uint64_t* koff, const uint64_t* sizes,
                     const uint8_t* tiers, uint64_t m, const CsvFiles* csv, char* err, size_t errlen) {
  static const uint8_t kWanted = 0;
  std::lock_guard<std::mutex> hold(rs->mu);
  uint64_t csv_bytes = 0;
  for (uint64_t i = 0; csv && i < csv->n_files; ++i) csv_bytes += csv->len[i];
  if (csv && csv->gz) csv_bytes += csv->n_files;  // a zero-length gzip file is an error the device reports
  if (!m && !csv_bytes) return S3IMPH_OK;  // a chunk without an object adds no run
  if (csv) tiers = rs->tiers ? &kWanted : nullptr;
  return host_entry(
      rs->device, "aggregate: ", err, errlen,
      [&](s3imph_ctx* c, hipStream_t, std::string& msg) {
        DevGuard g;
        DevRows r;
        const int rc2 = rows_from_host(c, g, keys, koff, sizes, m, rs->max_depth, &r, &msg, tiers, true, csv);
        if (rc2 == S3IMPH_OK && r.m && r.n) {  // the last step: a retry finds no run of this chunk
          HostRun run;
          download_rows(c, r, rs->tiers, &run);
          rs->runs.push_back(std::move(run));
        }
        return rc2;
      },
      csv ? "csv: " : nullptr);
}

}  // namespace

extern "C" {

void s3imph_merge_geometry(uint32_t* sample_step) {
  if (sample_step) *sample_step = kMS;
}

int s3imph_merge_rows_plan_device(s3imph_ctx* c, const uint8_t* d_blob, const uint64_t* d_offsets,
                                  const uint32_t* d_depth, const uint64_t* d_count, const uint64_t* d_bytes,
                                  const uint64_t* d_tier_count, const uint64_t* d_tier_bytes, uint64_t tier_stride,
                                  const uint64_t* run_starts, uint32_t k, s3imph_merge_info* info, void* stream) {
  if (!c || !info) return S3IMPH_ERR_INVALID;
  return device_entry(c, "merge: ", [&](std::string& msg) -> int {
    msg = merge_args_bad(d_blob, d_offsets, d_depth, d_count, d_bytes, d_tier_count, d_tier_bytes, tier_stride,
                         run_starts, k);
    if (!msg.empty()) {  // before any device work
      std::memset(info, 0, sizeof *info);
      info->first_unsorted = UINT64_MAX;
      info->n_runs = k;
      if (c->mrg) c->mrg->have_plan = false;
      return S3IMPH_ERR_INVALID;
    }
    const bool rows = run_starts && run_starts[k];  // no row: no device work
    hipStream_t s = rows ? use_device(c->device, stream, c->own_stream) : nullptr;
    return retry_on_nomem(c, s, &msg, [&] {
      return merge_plan(c, d_blob, d_offsets, d_depth, d_count, d_bytes, d_tier_count, d_tier_bytes, tier_stride,
                        run_starts, k, info, s, &msg);
    });
  });
}

int s3imph_merge_rows_fill_device(s3imph_ctx* c, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offsets,
                                  uint32_t* d_depth, uint64_t* d_count, uint64_t* d_bytes, uint64_t* d_tier_count,
                                  uint64_t* d_tier_bytes, uint64_t n_cap, void* stream) {
  if (!c) return S3IMPH_ERR_INVALID;
  return device_entry(c, "merge: ", [&](std::string& msg) {
    const bool plan = c->mrg && c->mrg->have_plan;  // without a plan: no device work
    hipStream_t s = plan ? use_device(c->device, stream, c->own_stream) : nullptr;
    return merge_fill(c, d_blob, blob_cap, d_offsets, d_depth, d_count, d_bytes, d_tier_count, d_tier_bytes, n_cap, s,
                      &msg);
  });
}

int s3imph_merge_rows_host(int device, const s3imph_row_run* runs, uint64_t k, uint8_t** blob, uint64_t** offsets,
                           uint32_t** depth, uint64_t** object_count, uint64_t** total_bytes, uint64_t** tier_count,
                           uint64_t** tier_bytes, uint64_t* present_mask, uint64_t* n, s3imph_merge_info* info,
                           char* err, size_t errlen) {
  if (!blob || !offsets || !depth || !object_count || !total_bytes || !n) return S3IMPH_ERR_INVALID;
  bool tiers = false;
  uint64_t rows = 0;
  const std::string bad = runs_bad(runs, k, &tiers, &rows);
  if (!bad.empty()) {
    set_err(err, errlen, bad);
    return S3IMPH_ERR_INVALID;
  }
  if (tiers && (!tier_count || !tier_bytes || !present_mask)) return S3IMPH_ERR_INVALID;
  s3imph_merge_info no_info;
  if (!info) info = &no_info;
  HostRows out(blob, offsets, depth, object_count, total_bytes, tier_count, tier_bytes, present_mask, n);
  out.reset();
  std::memset(info, 0, sizeof *info);
  info->first_unsorted = UINT64_MAX;
  info->n_runs = (uint32_t)std::min<uint64_t>(k, UINT32_MAX);
  if (rows == 0) return host_call("merge: ", err, errlen, [&](std::string&) { return out.none(); });
  const int rc = host_entry(device, "merge: ", err, errlen, [&](s3imph_ctx* c, hipStream_t, std::string& msg) {
    DevGuard g;
    DevRows r;
    const int rc2 = merge_runs(c, g, runs, k, tiers, &r, info, &msg);
    if (rc2 == S3IMPH_OK) out.download(c, r, tiers);
    return rc2;
  });
  if (rc != S3IMPH_OK) out.drop();
  return rc;
}

int s3imph_index_from_rows_host(int device, const s3imph_row_run* runs, uint64_t k, const char* out_dir, char* err,
                                size_t errlen) {
  return index_from_rows(device, runs, k, out_dir, err, errlen);
}

int s3imph_rowset_new(int device, uint32_t max_depth, int with_tiers, s3imph_rowset** out, char* err, size_t errlen) {
  if (!out) return S3IMPH_ERR_INVALID;
  *out = nullptr;
  if (device < 0) {
    set_err(err, errlen, "rowset: negative device");
    return S3IMPH_ERR_INVALID;
  }
  s3imph_rowset* rs = new (std::nothrow) s3imph_rowset();
  if (!rs) {
    set_err(err, errlen, "rowset: out of host memory");
    return S3IMPH_ERR_NOMEM;
  }
  rs->device = device;
  rs->max_depth = max_depth;
  rs->tiers = with_tiers != 0;
  *out = rs;
  return S3IMPH_OK;
}

int s3imph_rowset_add_objects(s3imph_rowset* rs, const uint8_t* keys, const uint64_t* key_offsets,
                              const uint64_t* sizes, const uint8_t* tiers, uint64_t m, char* err, size_t errlen) {
  if (!rs || !listing_given(keys, key_offsets, m)) return S3IMPH_ERR_INVALID;
  if (rs->tiers && m && !tiers) {
    set_err(err, errlen, "rowset: a set with tiers needs one tier id per object");
    return S3IMPH_ERR_INVALID;
  }
  return rowset_add_chunk(rs, keys, key_offsets, sizes, rs->tiers ? tiers : nullptr, m, nullptr, err, errlen);
}

int s3imph_rowset_add_csv(s3imph_rowset* rs, const uint8_t* const* csv, const uint64_t* csv_len, uint64_t n_files,
                          const s3imph_csv_schema* schema, char* err, size_t errlen) {
  if (!rs || !schema || (n_files && (!csv || !csv_len)) || schema->key_col < 0 || schema->size_col < 0)
    return S3IMPH_ERR_INVALID;
  for (uint64_t i = 0; i < n_files; ++i)
    if (csv_len[i] && !csv[i]) return S3IMPH_ERR_INVALID;
  const CsvFiles f{csv, csv_len, n_files, schema, rs->tiers, nullptr};
  return rowset_add_chunk(rs, nullptr, nullptr, nullptr, nullptr, 0, &f, err, errlen);
}

int s3imph_rowset_add_csv_gz(s3imph_rowset* rs, const uint8_t* const* gz, const uint64_t* gz_len, uint64_t n_files,
                             const s3imph_csv_schema* schema, uint64_t group_bytes, char* err, size_t errlen) {
  if (!rs || !schema || (n_files && (!gz || !gz_len)) || schema->key_col < 0 || schema->size_col < 0)
    return S3IMPH_ERR_INVALID;
  for (uint64_t i = 0; i < n_files; ++i)
    if (gz_len[i] && !gz[i]) return S3IMPH_ERR_INVALID;
  const CsvFiles f{gz, gz_len, n_files, schema, rs->tiers, nullptr, true, group_bytes};
  return rowset_add_chunk(rs, nullptr, nullptr, nullptr, nullptr, 0, &f, err, errlen);
}

int s3imph_rowset_add_rows(s3imph_rowset* rs, const s3imph_row_run* run, char* err, size_t errlen) {
  if (!rs || !run) return S3IMPH_ERR_INVALID;
  bool tiers = false;
  uint64_t rows = 0;
  const std::string bad = runs_bad(run, 1, &tiers, &rows);
  if (!bad.empty()) {
    set_err(err, errlen, bad);
    return S3IMPH_ERR_INVALID;
  }
  if (!rows) return S3IMPH_OK;
  if (tiers != rs->tiers) {
    set_err(err, errlen, "merge: runs with and without tier columns are mixed");
    return S3IMPH_ERR_INVALID;
  }
  try {
    HostRun h;
    const uint64_t n = run->n, b0 = run->offsets[0], nb = run->offsets[n] - b0;
    h.n = n;
    h.tiers = tiers;
    h.blob.assign(run->blob + (nb ? b0 : 0), run->blob + (nb ? b0 + nb : 0));
    h.offsets.resize(n + 1);
    for (uint64_t i = 0; i <= n; ++i) h.offsets[i] = run->offsets[i] - b0;
    h.depth.assign(run->depth, run->depth + n);
    h.count.assign(run->count, run->count + n);
    h.bytes.assign(run->bytes, run->bytes + n);
    if (tiers) {
      h.tcount.resize(kNT * n);
      h.tbytes.resize(kNT * n);
      for (int t = 0; t < kNT; ++t) {
        std::memcpy(h.tcount.data() + t * n, run->tier_count + t * run->tier_stride, n * 8);
        std::memcpy(h.tbytes.data() + t * n, run->tier_bytes + t * run->tier_stride, n * 8);
      }
    }
    std::lock_guard<std::mutex> hold(rs->mu);
    rs->runs.push_back(std::move(h));
    return S3IMPH_OK;
  } catch (const std::bad_alloc&) {
    set_err(err, errlen, "rowset: out of host memory");
    return S3IMPH_ERR_NOMEM;
  }
}

uint64_t s3imph_rowset_runs(const s3imph_rowset* rs) { return rs ? rs->runs.size() : 0; }

uint64_t s3imph_rowset_rows(const s3imph_rowset* rs) {
  uint64_t rows = 0;
  for (uint64_t r = 0; rs && r < rs->runs.size(); ++r) rows += rs->runs[r].n;
  return rows;
}

int s3imph_rowset_build(s3imph_rowset* rs, const char* out_dir, char* err, size_t errlen) {
  if (!rs || !out_dir) return S3IMPH_ERR_INVALID;
  std::lock_guard<std::mutex> hold(rs->mu);
  std::vector<s3imph_row_run> views;
  for (const HostRun& h : rs->runs) views.push_back(h.view());
  return index_from_rows(rs->device, views.data(), views.size(), out_dir, err, errlen);
}

int s3imph_rowset_close(s3imph_rowset* rs) {
  delete rs;
  return S3IMPH_OK;
}

}  // extern "C"
