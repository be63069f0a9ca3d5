// s3imph_index.hip — indexread.Index on the GPU (include/s3imph.h section 5c): an index
// handle whose arrays live in HBM, and batched forms of the reference reader's queries.
//
// Reference (pkg/indexread/index.go, pkg/format/depthindex.go):
//   Open                       index.go:31-86 (OpenArray, reader.go:81-119; OpenDepthIndex,
//                              depthindex.go:115-141; OpenMPHF, mphf.go:186-247);
//   Lookup / StatsForPrefix    index.go:128-152;
//   Stats / Depth / SubtreeEnd / MaxDepthInSubtree   index.go:135-176;
//   DescendantsAtDepth[Filtered] / DescendantsUpToDepth   index.go:206-297, over
//   GetPositionsInSubtree (depthindex.go:193-259, two binary searches in a depth's slice);
//   HasTierData / TierBreakdown / TierBreakdownAll / TierBreakdownForPrefix   index.go:360-399,
//   over OpenTierStats / GetBreakdown[All] (tierstats.go:108-215; include/s3imph.h section 5e);
//   query --estimate-cost: TierBreakdown(pos) -> pricing.ComputeMonthlyCost (internal/cli/cli.go:
//   227-296, pkg/pricing/pricing.go:159-240; include/s3imph.h section 5h), and the plan's rows
//   ranked by it (an extension: stable segmented sort of the filled rows, first k of each kept);
//   PrefixString   index.go:179 over the prefix blob OpenMPHF loads (mphf.go:226-238; OpenBlob and
//   BlobReader.Get, reader.go:213-270), for a batch; MPHF.LookupWithVerify (mphf.go:306-320);
//   VerifyMPHF (mphf.go:372-393).
//
// GPU formulation.  A batch of descendants queries is a CSR: `levels` per query, `row_ptr`
// over the result rows, and the flat list of positions.  The plan step runs one lane per
// row (the two binary searches side by side, so two dependent loads are in flight per
// lane; occupancy hides the rest) and scans the row lengths with a reduce / top / down
// triple.  Row lengths run from 0 to the whole index, so nothing after that is
// decomposed by row: the OUTPUT is cut into chunks of kChunk positions, one workgroup
// each, and every lane finds the row of its own output slot by a binary search in
// row_ptr over the few rows its chunk touches.  The filter works on the same chunks of
// the unfiltered list: flags are counted per chunk, the chunk counts scanned, the filtered
// row_ptr read off the flag prefix at each row's start, and the fill writes each kept
// position at its flag prefix (order kept).  No kernel here waits on another workgroup.
#include <sys/stat.h>

#include <cerrno>
#include <cstdio>
#include <cstring>

#include "s3imph_entry.h"
#include "s3imph_keys.h"
#include "s3imph_pricing.h"
#include "s3imph_prim.h"
#include "s3imph_tiers.h"

namespace s3imph {
namespace {

constexpr int kQT = 256;                   // lanes per workgroup of the per-query / per-row kernels
constexpr int kScanT = 256;                // row-length scan: 8 values per lane
constexpr int kScanPer = 8;
constexpr int kScanB = kScanT * kScanPer;  // values per scan block
constexpr int kChunkT = 256;               // the chunk kernels: kChunk / kChunkT slots per lane
constexpr int kChunk = 2048;               // output positions per chunk (a power of two)
constexpr int kChunkPer = kChunk / kChunkT;

struct IndexArrays {
  uint64_t n = 0;
  uint32_t max_depth = 0;
  const uint64_t *fp = nullptr, *pos = nullptr;
  const uint32_t *depth = nullptr, *mds = nullptr;
  const uint64_t *send = nullptr, *doff = nullptr, *dpos = nullptr;
  const uint64_t *ocnt = nullptr, *tbytes = nullptr;  // nullable
};

// Stats / Depth / SubtreeEnd / MaxDepthInSubtree for one position per lane; zero record
// with found = 0 when pos >= Count() (index.go:135-176).
__global__ __launch_bounds__(kQT) void k_index_nodes(IndexArrays a, const uint64_t* __restrict__ qpos, uint64_t nq,
                                                     s3imph_node* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * kQT + threadIdx.x;
  if (i >= nq) return;
  const uint64_t p = qpos[i];
  s3imph_node r{};
  if (p < a.n) {
    r.pos = p;
    r.subtree_end = a.send[p];
    r.object_count = a.ocnt ? a.ocnt[p] : 0;
    r.total_bytes = a.tbytes ? a.tbytes[p] : 0;
    r.depth = a.depth[p];
    r.max_depth_in_subtree = a.mds[p];
    r.found = 1;
  }
  out[i] = r;
}

// TierBreakdownAll / TierBreakdown (tierstats.go:157-215) for one (query, manifest slot) per
// lane.  The tier table is interleaved by position, tier[(p * T + s) * 2] = count and
// [.. + 1] = bytes of slot s, so the T lanes of a query read one contiguous run of 16 T bytes
// and write one.  A workgroup takes qb = kQT / T whole queries; their masks are gathered in LDS.
__global__ __launch_bounds__(kQT) void k_index_tiers(const uint64_t* __restrict__ tier, uint64_t n, uint32_t T,
                                                     uint32_t qb, const uint64_t* __restrict__ qpos, uint64_t nq,
                                                     uint64_t* __restrict__ out, uint32_t* __restrict__ mask) {
  __shared__ unsigned s_mask[kQT];
  s_mask[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t ql = threadIdx.x / T, s = threadIdx.x - ql * T;
  const uint64_t q = (uint64_t)blockIdx.x * qb + ql;
  const bool active = ql < qb && q < nq;
  if (active) {
    const uint64_t p = qpos[q];
    uint64_t c = 0, b = 0;
    if (p < n) {
      const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(tier + (p * T + s) * 2);
      c = v.x;
      b = v.y;
    }
    out[(q * T + s) * 2] = c;
    out[(q * T + s) * 2 + 1] = b;
    if (c | b) atomicOr(&s_mask[ql], 1u << s);
  }
  __syncthreads();
  if (active && s == 0) mask[q] = s_mask[ql];
}

struct TierSlots {
  uint8_t id[S3IMPH_NUM_TIERS];
};

// The interleaved table from the column-major arrays of the aggregation (column t at
// t * stride): one lane per position, reads coalesced along each column.
__global__ __launch_bounds__(kQT) void k_tier_interleave(const uint64_t* __restrict__ cnt,
                                                         const uint64_t* __restrict__ bytes, uint64_t stride,
                                                         uint64_t n, uint32_t T, TierSlots ids,
                                                         uint64_t* __restrict__ out) {
  const uint64_t p = (uint64_t)blockIdx.x * kQT + threadIdx.x;
  if (p >= n) return;
  for (uint32_t s = 0; s < T; ++s) {
    const uint64_t col = (uint64_t)ids.id[s] * stride + p;
    *reinterpret_cast<ulonglong2*>(out + (p * T + s) * 2) = make_ulonglong2(cnt[col], bytes[col]);
  }
}

// TierBreakdown(pos) -> ComputeMonthlyCost (pricing.go:159-240) for one (query, manifest slot) per
// lane: k_index_tiers's read, each lane pricing its slot by the shared rule (s3imph_pricing.h).
// The records of the workgroup's qb queries are summed in LDS (u64 sums wrap, so the order is
// free; per_tier[id] has one writer) and then written as one contiguous run of 17 qb words.
// Tl = max(T, 1) lanes per query: without tier data only `found` is set.
constexpr int kCostWords = (int)(sizeof(s3imph_cost) / 8);
static_assert(sizeof(s3imph_cost) == 136 && sizeof(s3imph_price_table) == 120, "section 5h layouts");
__global__ __launch_bounds__(kQT) void k_index_cost(const uint64_t* __restrict__ tier, uint64_t n, uint32_t T,
                                                    uint32_t Tl, uint32_t qb, TierSlots ids, s3imph_price_table pt,
                                                    const uint64_t* __restrict__ qpos, uint64_t nq,
                                                    uint64_t* __restrict__ out) {
  extern __shared__ unsigned long long s_rec[];  // qb records
  const uint64_t q0 = (uint64_t)blockIdx.x * qb;
  const uint32_t nact = (uint32_t)(nq - q0 < qb ? nq - q0 : qb);
  for (uint32_t w = threadIdx.x; w < nact * kCostWords; w += kQT) s_rec[w] = 0;
  __syncthreads();
  const uint32_t ql = threadIdx.x / Tl, s = threadIdx.x - ql * Tl;
  if (ql < nact) {
    const uint64_t p = qpos[q0 + ql];
    if (p < n) {
      unsigned long long* r = s_rec + ql * kCostWords;
      unsigned long long flags = s == 0 ? 1ull << 32 : 0;  // found
      if (s < T) {
        const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(tier + (p * T + s) * 2);
        const uint32_t id = ids.id[s];
        const SlotCost c = price_slot(id, v.x, v.y, pt);
        if (c.priced) {
          r[4 + id] = c.tier_total;
          if (c.tier_total + c.monitoring) atomicAdd(&r[0], c.tier_total + c.monitoring);
          if (c.monitoring) atomicAdd(&r[1], c.monitoring);
          if (c.min_size) atomicAdd(&r[2], c.min_size);
          if (c.overhead) atomicAdd(&r[3], c.overhead);
          if (v.x | v.y) flags |= 1ull << id;  // tier_mask
        }
      }
      if (flags) atomicOr(&r[4 + S3IMPH_NUM_TIERS], flags);
    }
  }
  __syncthreads();
  for (uint32_t w = threadIdx.x; w < nact * kCostWords; w += kQT) out[q0 * kCostWords + w] = s_rec[w];
}

// The ranking key of every planned position, one lane each: object_count, total_bytes, or
// s3imph_cost.total by the same rule, the lane walking its position's T slots.
__global__ __launch_bounds__(kQT) void k_rank_keys(IndexArrays a, const uint64_t* __restrict__ tier, uint32_t T,
                                                   TierSlots ids, s3imph_price_table pt, int key,
                                                   const uint64_t* __restrict__ pos, uint64_t total,
                                                   uint64_t* __restrict__ keys) {
  const uint64_t i = (uint64_t)blockIdx.x * kQT + threadIdx.x;
  if (i >= total) return;
  const uint64_t p = pos[i];
  uint64_t v = 0;
  if (p < a.n) {
    if (key == S3IMPH_RANK_OBJECT_COUNT) {
      v = a.ocnt[p];
    } else if (key == S3IMPH_RANK_TOTAL_BYTES) {
      v = a.tbytes[p];
    } else {
      for (uint32_t s = 0; s < T; ++s) {
        const ulonglong2 cb = *reinterpret_cast<const ulonglong2*>(tier + (p * T + s) * 2);
        const SlotCost c = price_slot(ids.id[s], cb.x, cb.y, pt);
        v += c.tier_total + c.monitoring;
      }
    }
  }
  keys[i] = v;
}

// Entry j of row r out of the sorted rows: the first min(k, len) pairs, then the padding.
// rp == nullptr: every row is empty.
__global__ __launch_bounds__(kQT) void k_rows_take(const uint64_t* __restrict__ rp, const uint64_t* __restrict__ spos,
                                                   const uint64_t* __restrict__ skey, uint64_t n_rows, uint32_t k,
                                                   uint64_t* __restrict__ top_pos, uint64_t* __restrict__ top_key,
                                                   uint32_t* __restrict__ top_n) {
  const uint64_t i = (uint64_t)blockIdx.x * kQT + threadIdx.x;
  if (i >= n_rows * k) return;
  const uint64_t r = i / k;
  const uint32_t j = (uint32_t)(i - r * k);
  const uint64_t lo = rp ? rp[r] : 0, len = rp ? rp[r + 1] - lo : 0;
  const uint32_t tn = len < k ? (uint32_t)len : k;
  top_pos[i] = j < tn ? spos[lo + j] : ~0ull;
  top_key[i] = j < tn ? skey[lo + j] : 0;
  if (j == 0) top_n[r] = tn;
}

// One lane per result row: the row's slice start in depth_positions and its unfiltered
// length; lane j == 0 of a query writes its `levels`.  AT: rel[q] levels below the query;
// UPTO: row j of query q is depth[pos] + 1 + j (R rows per query).
__global__ __launch_bounds__(kQT) void k_desc_ranges(IndexArrays a, const uint64_t* __restrict__ qpos,
                                                     const int32_t* __restrict__ rel, uint64_t n_rows, int upto,
                                                     uint32_t R, int32_t max_rel, int32_t* __restrict__ levels,
                                                     uint64_t* __restrict__ row_lo, uint64_t* __restrict__ row_len) {
  const uint64_t row = (uint64_t)blockIdx.x * kQT + threadIdx.x;
  if (row >= n_rows) return;
  const uint64_t q = upto ? row / R : row;
  const uint32_t j = upto ? (uint32_t)(row % R) : 0;
  const uint64_t pos = qpos[q];
  int32_t lv = 0;
  uint64_t lo = 0, len = 0;
  if (pos < a.n) {
    const uint64_t d = a.depth[pos];
    uint64_t t;
    bool ok;
    if (upto) {
      const int64_t diff = (int64_t)a.mds[pos] - (int64_t)d;
      const int64_t l = diff < (int64_t)max_rel ? diff : (int64_t)max_rel;
      lv = l <= 0 ? 0 : (l > (int64_t)R ? (int32_t)R : (int32_t)l);
      ok = (int64_t)j < (int64_t)lv;
      t = d + 1 + j;
    } else {
      const int32_t r = rel[q];
      t = d + (uint64_t)(r < 0 ? 0 : r);  // no wrap-around: d < 2^32, r < 2^31
      ok = r >= 0 && t <= (uint64_t)a.max_depth;
      lv = ok ? 1 : 0;
    }
    ok = ok && t <= (uint64_t)a.max_depth;
    if (ok) {
      const uint64_t s = a.doff[t], e = a.doff[t + 1], se = a.send[pos];
      // first index with p >= pos and first with p > subtree_end, both over [s, e): the two
      // searches advance together, selects instead of exits
      uint64_t l0 = s, n0 = e > s ? e - s : 0, l1 = l0, n1 = n0;
      while (n0 | n1) {
        const uint64_t h0 = n0 >> 1, h1 = n1 >> 1;
        const uint64_t v0 = n0 ? a.dpos[l0 + h0] : 0, v1 = n1 ? a.dpos[l1 + h1] : 0;
        const bool r0 = n0 && v0 < pos, r1 = n1 && v1 <= se;
        l0 = r0 ? l0 + h0 + 1 : l0;
        n0 = r0 ? n0 - h0 - 1 : h0;
        l1 = r1 ? l1 + h1 + 1 : l1;
        n1 = r1 ? n1 - h1 - 1 : h1;
      }
      lo = l0;
      len = l1 > l0 ? l1 - l0 : 0;
    }
  }
  if (j == 0) levels[q] = lv;
  row_lo[row] = lo;
  row_len[row] = len;
}

// ---- exclusive scan of n u64 values into n + 1 entries: reduce / top / down --------------
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t u = __shfl_up((unsigned long long)v, o);
    if ((int)lane_id() >= o) v += u;
  }
  return v;
}

__global__ __launch_bounds__(kScanT) void k_rows_reduce(const uint64_t* __restrict__ in, uint64_t n,
                                                        uint64_t* __restrict__ sums) {
  __shared__ uint64_t s_w[kScanT / 64];
  const uint64_t b0 = (uint64_t)blockIdx.x * kScanB;
  uint64_t v = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    const uint64_t i = b0 + threadIdx.x + (uint64_t)k * kScanT;
    if (i < n) v += in[i];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor((unsigned long long)v, o);
  if (lane_id() == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t t = 0;
    for (int w = 0; w < kScanT / 64; ++w) t += s_w[w];
    sums[blockIdx.x] = t;
  }
}

// One workgroup: sums[0 .. nb) -> exclusive prefix in place, sums[nb] = total.
__global__ __launch_bounds__(1024) void k_rows_top(uint64_t* __restrict__ sums, uint64_t nb) {
  __shared__ uint64_t s_w[16];
  __shared__ uint64_t s_carry;
  if (threadIdx.x == 0) s_carry = 0;
  __syncthreads();
  for (uint64_t b0 = 0; b0 < nb; b0 += 1024) {
    const uint64_t i = b0 + threadIdx.x;
    const uint64_t v = i < nb ? sums[i] : 0;
    const uint64_t inc = wave_incl_scan(v);
    if (lane_id() == 63) s_w[threadIdx.x >> 6] = inc;
    __syncthreads();
    uint64_t base = s_carry;
    for (unsigned w = 0; w < (threadIdx.x >> 6); ++w) base += s_w[w];
    if (i < nb) sums[i] = base + inc - v;
    __syncthreads();
    if (threadIdx.x == 1023) s_carry = base + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[nb] = s_carry;
}

// out[i] (and out2[i] when given) = sums[block] + prefix inside the block; entry n = total.
__global__ __launch_bounds__(kScanT) void k_rows_down(const uint64_t* __restrict__ in, uint64_t n,
                                                      const uint64_t* __restrict__ sums, uint64_t nb,
                                                      uint64_t* __restrict__ out, uint64_t* __restrict__ out2) {
  __shared__ uint64_t s_w[kScanT / 64];
  const uint64_t i0 = (uint64_t)blockIdx.x * kScanB + (uint64_t)threadIdx.x * kScanPer;
  uint64_t v[kScanPer], tot = 0;
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    v[k] = i0 + k < n ? in[i0 + k] : 0;
    tot += v[k];
  }
  const uint64_t inc = wave_incl_scan(tot);
  if (lane_id() == 63) s_w[threadIdx.x >> 6] = inc;
  __syncthreads();
  uint64_t run = sums[blockIdx.x] + inc - tot;
  for (unsigned w = 0; w < (threadIdx.x >> 6); ++w) run += s_w[w];
#pragma unroll
  for (int k = 0; k < kScanPer; ++k) {
    if (i0 + k < n) {
      out[i0 + k] = run;
      if (out2) out2[i0 + k] = run;
    }
    run += v[k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    out[n] = sums[nb];
    if (out2) out2[n] = sums[nb];
  }
}

// ---- the chunk kernels ---------------------------------------------------------------------
// The rows a chunk [base, end) of the flat list touches (end > base): the row of slot u is
// the last r with U[r] <= u (empty rows share their successor's start and are never that
// one); U has n_rows + 1 entries, U[n_rows] = total >= end.
struct ChunkRows {
  uint64_t r0, r1;
};
__device__ __forceinline__ ChunkRows chunk_rows(const uint64_t* __restrict__ U, uint64_t n_rows, uint64_t base,
                                                uint64_t end) {
  ChunkRows c;
  c.r0 = first_above(U, 0, n_rows + 1, base) - 1;
  c.r1 = first_above(U, c.r0 + 1, n_rows + 1, end - 1) - 1;
  return c;
}
// The position at slot u of the flat list, u in the chunk whose rows are c.
__device__ __forceinline__ uint64_t slot_position(const uint64_t* __restrict__ U, const uint64_t* __restrict__ row_lo,
                                                  const uint64_t* __restrict__ dpos, ChunkRows c, uint64_t u) {
  const uint64_t r = first_above(U, c.r0 + 1, c.r1 + 1, u) - 1;
  return dpos[row_lo[r] + (u - U[r])];
}

// Unfiltered fill: out[u] = position at slot u, one workgroup per chunk of the output.
__global__ __launch_bounds__(kChunkT) void k_desc_fill(const uint64_t* __restrict__ U,
                                                       const uint64_t* __restrict__ row_lo, uint64_t n_rows,
                                                       uint64_t total, const uint64_t* __restrict__ dpos,
                                                       uint64_t* __restrict__ out) {
  const uint64_t base = (uint64_t)blockIdx.x * kChunk;
  if (base >= total) return;
  const uint64_t end = base + kChunk < total ? base + kChunk : total;
  const ChunkRows c = chunk_rows(U, n_rows, base, end);
#pragma unroll
  for (int k = 0; k < kChunkPer; ++k) {
    const uint64_t u = base + threadIdx.x + (uint64_t)k * kChunkT;
    if (u < end) out[u] = slot_position(U, row_lo, dpos, c, u);
  }
}

// The filter over the chunks of the unfiltered list (U, total).  Every mode flags its chunk's
// candidates (object_count >= min_count && total_bytes >= min_bytes, unsigned) in list order.
//   kCount: csum[chunk] = flags of the chunk.
//   kRows:  row_ptr[r] = cbase[chunk] + flags before slot U[r], for the rows that start in the
//           chunk (U[r] in [base, base + kChunk)); launched on total / kChunk + 1 chunks, so
//           the rows starting at `total` are covered too.
//   kFill:  out[cbase[chunk] + flags before u] = position at u, for flagged u.
enum { kCount = 0, kRows = 1, kFill = 2 };
template <int MODE>
__global__ __launch_bounds__(kChunkT) void k_desc_filter(IndexArrays a, const uint64_t* __restrict__ U,
                                                         const uint64_t* __restrict__ row_lo, uint64_t n_rows,
                                                         uint64_t total, uint64_t min_count, uint64_t min_bytes,
                                                         uint64_t* __restrict__ csum,
                                                         const uint64_t* __restrict__ cbase,
                                                         uint64_t* __restrict__ row_ptr, uint64_t* __restrict__ out) {
  __shared__ unsigned s_w[kChunkT / 64];
  __shared__ unsigned s_pre[MODE == kRows ? kChunk + 1 : 1];
  const uint64_t base = (uint64_t)blockIdx.x * kChunk;
  if (base > total) return;
  const uint64_t end = base + kChunk < total ? base + kChunk : total;
  ChunkRows c{0, 0};
  if (end > base) c = chunk_rows(U, n_rows, base, end);
  const uint64_t cb = MODE == kCount ? 0 : cbase[blockIdx.x];
  const unsigned wave = threadIdx.x >> 6;
  unsigned running = 0;
  for (int k = 0; k < kChunkPer; ++k) {
    const unsigned slot = threadIdx.x + (unsigned)k * kChunkT;
    const uint64_t u = base + slot;
    uint64_t p = 0;
    bool flag = false;
    if (u < end) {
      p = slot_position(U, row_lo, a.dpos, c, u);
      flag = p < a.n && a.ocnt[p] >= min_count && a.tbytes[p] >= min_bytes;
    }
    const uint64_t bal = __ballot(flag);
    if (lane_id() == 0) s_w[wave] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned before = running + (unsigned)__popcll(bal & lanemask_lt()), all = 0;
#pragma unroll
    for (unsigned w = 0; w < kChunkT / 64; ++w) {
      before += w < wave ? s_w[w] : 0;
      all += s_w[w];
    }
    if (MODE == kRows) s_pre[slot] = before;
    if (MODE == kFill && flag) out[cb + before] = p;
    running += all;
    __syncthreads();
  }
  if (MODE == kCount && threadIdx.x == 0) csum[blockIdx.x] = running;
  if (MODE == kRows) {
    if (threadIdx.x == 0) s_pre[kChunk] = running;
    __syncthreads();
    const uint64_t ra = first_at_least(U, 0, n_rows + 1, base);
    const uint64_t rb = first_at_least(U, ra, n_rows + 1, base + kChunk);
    for (uint64_t r = ra + threadIdx.x; r < rb; r += kChunkT) row_ptr[r] = cb + s_pre[U[r] - base];
  }
}

// ---- the prefix blob: PrefixString, LookupWithVerify, VerifyMPHF -----------------------------
// The stored prefixes (prefix_blob.bin, prefix_offsets.u64) in HBM: n + 1 offsets that never
// decrease, the blob readable up to end8 = round_up(offsets[n], 8).
struct PrefixBlob {
  const uint8_t* blob = nullptr;
  const uint64_t* off = nullptr;
  uint64_t end8 = 0;
};

// PrefixString's length pass (BlobReader.Get, reader.go:250-270), one lane per query: the row's
// length, its source address in the blob (so the emit never goes back to offsets[pos]) and
// found; pos >= Count() is a 0-byte row with found = 0.
__global__ __launch_bounds__(kQT) void k_names_len(PrefixBlob pb, uint64_t n, const uint64_t* __restrict__ qpos,
                                                   uint64_t nq, uint64_t* __restrict__ src,
                                                   uint64_t* __restrict__ len, uint32_t* __restrict__ found) {
  const uint64_t i = (uint64_t)blockIdx.x * kQT + threadIdx.x;
  if (i >= nq) return;
  const uint64_t p = qpos[i];
  const bool ok = p < n;
  uint64_t o0 = 0, o1 = 0;
  if (ok) {
    o0 = pb.off[p];
    o1 = pb.off[p + 1];
  }
  src[i] = o0;
  len[i] = o1 - o0;
  if (found) found[i] = ok ? 1u : 0u;
}

// The emit's chunks: the row of each chunk's first output byte (chunk_owner), one lane per chunk.
__global__ __launch_bounds__(kChunkT) void k_names_bounds(const uint64_t* __restrict__ U, uint64_t entries,
                                                          uint64_t nchunks, uint64_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kChunkT + threadIdx.x;
  if (t < nchunks) out[t] = chunk_owner(U, entries, 8ull * kChunkT, 0, t);
}

// The rows back to back, by 8-byte word of the output (emit_word): row r from blob address src[r].
__global__ __launch_bounds__(kChunkT) void k_names_emit(PrefixBlob pb, const uint64_t* __restrict__ offsets,
                                                        const uint64_t* __restrict__ bounds,
                                                        const uint64_t* __restrict__ src, uint64_t n_rows,
                                                        uint64_t total, uint8_t* __restrict__ out) {
  emit_word<kChunkT>(pb.blob, pb.end8, offsets, bounds, n_rows, total, out, [&](uint64_t r) { return src[r]; });
}

// LookupWithVerify's second half (mphf.go:312-317), one lane per query: the position survives
// only if the stored prefix there has the query's length and bytes; lengths first, then words
// through load8 on both blobs (any alignment), the last word masked.
__global__ __launch_bounds__(kQT) void k_lookup_verify(PrefixBlob pb, uint64_t n, const uint8_t* __restrict__ qblob,
                                                       const uint64_t* __restrict__ qoff, uint64_t nq,
                                                       uint64_t* __restrict__ res) {
  const uint64_t i = (uint64_t)blockIdx.x * kQT + threadIdx.x;
  if (i >= nq) return;
  const uint64_t p = res[i];
  if (p == ~0ull) return;
  bool same = p < n;
  if (same) {
    const uint64_t q0 = qoff[i], len = qoff[i + 1] - q0;
    const uint64_t s0 = pb.off[p];
    same = pb.off[p + 1] - s0 == len;
    if (same && len) {
      const uint64_t qend8 = (qoff[nq] + 7) & ~7ull;
      for (uint64_t k = 0; k < len; k += 8) {
        uint64_t x = load8(qblob, q0 + k, qend8) ^ load8(pb.blob, s0 + k, pb.end8);
        if (len - k < 8) x &= (1ull << (8 * (len - k))) - 1;
        if (x) {
          same = false;
          break;
        }
      }
    }
  }
  if (!same) res[i] = ~0ull;
}

// VerifyMPHF's reduction (mphf.go:372-393) over got[i] = Lookup(prefix i): r[0] += the i with
// got[i] != i, r[1] = the smallest of them (r[1] starts at UINT64_MAX).  One atomic pair per wave
// that saw one.
__global__ __launch_bounds__(kQT) void k_verify_reduce(const uint64_t* __restrict__ got, uint64_t n,
                                                       unsigned long long* __restrict__ r) {
  unsigned long long bad = 0, first = ~0ull;
  for (uint64_t i = (uint64_t)blockIdx.x * kQT + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kQT)
    if (got[i] != i) {
      ++bad;
      first = first < i ? first : i;
    }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    bad += __shfl_xor(bad, o);
    const unsigned long long f = __shfl_xor(first, o);
    first = first < f ? first : f;
  }
  if (lane_id() == 0 && bad) {
    atomicAdd(&r[0], bad);
    atomicMin(&r[1], first);
  }
}
// r[2] = what the lookup gave at the first bad index.
__global__ void k_verify_got(const uint64_t* __restrict__ got, unsigned long long* __restrict__ r) {
  if (r[0]) r[2] = got[r[1]];
}

// ---- host side: files -------------------------------------------------------------------------
struct HostArray {
  std::vector<uint64_t> store;  // 8-byte aligned payload
  uint64_t count = 0;
  const uint64_t* u64() const { return store.data(); }
  const uint32_t* u32() const { return reinterpret_cast<const uint32_t*>(store.data()); }
};

// OpenArray (reader.go:81-119) with the expected width checked as well.
int read_array(const std::string& path, uint32_t width, HostArray* out, std::string* msg) {
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    *msg = "mmap file: open file: open " + path + ": " + std::strerror(errno);
    return S3IMPH_ERR_IO;
  }
  struct Close {
    FILE* f;
    ~Close() { std::fclose(f); }
  } closer{f};
  struct stat st;
  if (::fstat(fileno(f), &st) != 0) {
    *msg = "mmap file: stat file: " + path + ": " + std::strerror(errno);
    return S3IMPH_ERR_IO;
  }
  const uint64_t size = (uint64_t)st.st_size;
  uint8_t h[kS3idHeaderSize];
  if (size < kS3idHeaderSize || std::fread(h, 1, sizeof h, f) != sizeof h) {
    *msg = "invalid header";
    return S3IMPH_ERR_FORMAT;
  }
  auto le = [&](int at, int bytes) {
    uint64_t v = 0;
    for (int b = 0; b < bytes; ++b) v |= (uint64_t)h[at + b] << (8 * b);
    return v;
  };
  if (le(0, 4) != kS3idMagic) {
    *msg = "magic number mismatch";
    return S3IMPH_ERR_FORMAT;
  }
  if (le(4, 4) != kS3idVersion) {
    *msg = "version mismatch";
    return S3IMPH_ERR_FORMAT;
  }
  const uint64_t count = le(8, 8), w = le(16, 4);
  if (w != width) {
    *msg = "element width " + std::to_string(w) + ", want " + std::to_string(width);
    return S3IMPH_ERR_FORMAT;
  }
  if (count > (size - kS3idHeaderSize) / width) {
    *msg = "file too small: " + std::to_string(size) + " < " + std::to_string(kS3idHeaderSize) + " + " +
           std::to_string(count) + " * " + std::to_string(width);
    return S3IMPH_ERR_FORMAT;
  }
  static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "S3ID payloads are little-endian");
  const uint64_t bytes = count * width;
  out->store.assign((bytes + 7) / 8, 0);
  out->count = count;
  if (bytes && std::fread(out->store.data(), 1, bytes, f) != bytes) {
    *msg = "read " + path + ": " + std::strerror(errno);
    return S3IMPH_ERR_IO;
  }
  return S3IMPH_OK;
}

bool file_exists(const std::string& p) {
  struct stat st;
  return ::stat(p.c_str(), &st) == 0;
}

// MarshalBinary framing of mph.bin, as s3imph_ctx_load_mph_bin checks it, without a device.
bool mph_bin_framed(const uint8_t* p, uint64_t len, uint64_t* keys, std::string* msg) {
  *keys = 0;
  if (len == 0) return true;
  uint64_t at = 0;
  auto get = [&](uint64_t* v) {
    if (len - at < 8) return false;
    std::memcpy(v, p + at, 8);
    at += 8;
    return true;
  };
  uint64_t parts = 0, nl = 0;
  if (!get(&parts) || parts != kPartitions || !get(&nl) || nl == 0 || nl > (uint64_t)kMaxLevels) {
    *msg = "unmarshal: bad header";
    return false;
  }
  for (uint64_t L = 0; L < nl; ++L) {
    uint64_t w = 0;
    if (!get(&w) || w > (len - at) / 8) {
      *msg = "unmarshal: truncated level " + std::to_string(L);
      return false;
    }
    if (w == 0) {
      *msg = "unmarshal: empty level " + std::to_string(L);
      return false;
    }
    for (uint64_t q = 0; q < w; ++q) {
      uint64_t word;
      std::memcpy(&word, p + at + 8 * q, 8);
      *keys += (uint64_t)__builtin_popcountll(word);
    }
    at += 8 * w;
  }
  if (at != len) {
    *msg = "unmarshal: trailing bytes";
    return false;
  }
  return true;
}

// Everything Open reads, checked on the host.
struct HostIndex {
  HostArray send, depth, mds, doff, dpos, fp, pos, ocnt, tbytes;
  bool stats = false;
  std::vector<TierEntry> tiers;     // tiers.json's entries, in its order (none: no tier data)
  std::vector<uint64_t> tier_table;  // [n][2 T]: count, bytes per manifest slot
  std::vector<uint8_t> mph;
  uint64_t n = 0;
  uint32_t max_depth = 0;
};

// OpenTierStats (tierstats.go:108-146) for an index of n nodes: tiers.json's entries and both
// arrays of each, interleaved by position into h->tier_table.
int load_host_tiers(const std::string& dir, uint64_t n, HostIndex* h, std::string* msg) {
  std::string m;
  int rc = read_tier_manifest(dir, &h->tiers, &m);
  if (rc != S3IMPH_OK) {
    *msg = "open tier stats: " + m;
    return rc;
  }
  const uint64_t T = h->tiers.size();
  if (T == 0) return S3IMPH_OK;  // no tiers.json, or an empty list: no tier data
  auto refuse = [&](const std::string& what) {
    *msg = "open tier stats: read tier manifest: " + what;
    return (int)S3IMPH_ERR_FORMAT;
  };
  unsigned seen = 0;
  for (const TierEntry& e : h->tiers) {
    if (e.id >= (unsigned)S3IMPH_NUM_TIERS)
      return refuse("tier id " + std::to_string(e.id) + " is not below " + std::to_string(S3IMPH_NUM_TIERS));
    if ((seen >> e.id) & 1) return refuse("tier id " + std::to_string(e.id) + " is listed twice");
    seen |= 1u << e.id;
    if (e.file.empty() || e.file.find('/') != std::string::npos || e.file.find("..") != std::string::npos)
      return refuse("file \"" + e.file + "\" of tier " + std::to_string(e.id) + " is not a plain file prefix");
  }
  h->tier_table.assign(n * 2 * T, 0);
  for (uint64_t s = 0; s < T; ++s) {
    const TierEntry& e = h->tiers[s];
    for (int k = 0; k < 2; ++k) {  // the bytes array first, as the reference opens them
      const char* what = k ? " counts: " : " bytes: ";
      HostArray a;
      rc = read_array(dir + "/tier_stats/" + e.file + (k ? "_count.u64" : "_bytes.u64"), 8, &a, &m);
      if (rc == S3IMPH_OK && a.count != n) {
        m = "holds " + std::to_string(a.count) + " entries, subtree_end " + std::to_string(n);
        rc = S3IMPH_ERR_FORMAT;
      }
      if (rc != S3IMPH_OK) {
        *msg = "open tier stats: open " + e.name + what + m;
        return rc;
      }
      const uint64_t* v = a.u64();
      for (uint64_t p = 0; p < n; ++p) h->tier_table[(p * T + s) * 2 + (k ? 0 : 1)] = v[p];
    }
  }
  return S3IMPH_OK;
}

int load_host_index(const std::string& dir, HostIndex* h, std::string* msg) {
  std::string m;
  int rc;
  auto fail = [&](const char* what, int code) {
    *msg = std::string(what) + ": " + m;
    return code;
  };
  if ((rc = read_array(dir + "/subtree_end.u64", 8, &h->send, &m))) return fail("open subtree_end", rc);
  if ((rc = read_array(dir + "/depth.u32", 4, &h->depth, &m))) return fail("open depth", rc);
  // the caller's aggregation data: optional here (the reference's Open requires both)
  const bool oc = file_exists(dir + "/object_count.u64"), tb = file_exists(dir + "/total_bytes.u64");
  if (oc != tb) {
    m = "object_count.u64 and total_bytes.u64 must both be present or both be absent";
    return fail(oc ? "open total_bytes" : "open object_count", S3IMPH_ERR_IO);
  }
  h->stats = oc;
  if (oc) {
    if ((rc = read_array(dir + "/object_count.u64", 8, &h->ocnt, &m))) return fail("open object_count", rc);
    if ((rc = read_array(dir + "/total_bytes.u64", 8, &h->tbytes, &m))) return fail("open total_bytes", rc);
  }
  if ((rc = read_array(dir + "/max_depth_in_subtree.u32", 4, &h->mds, &m)))
    return fail("open max_depth_in_subtree", rc);
  if ((rc = read_array(dir + "/depth_offsets.u64", 8, &h->doff, &m))) {
    m = "open offsets: " + m;
    return fail("open depth index", rc);
  }
  if ((rc = read_array(dir + "/depth_positions.u64", 8, &h->dpos, &m))) {
    m = "open positions: " + m;
    return fail("open depth index", rc);
  }
  {
    FILE* f = std::fopen((dir + "/mph.bin").c_str(), "rb");
    if (!f) {
      m = "open " + dir + "/mph.bin: " + std::strerror(errno);
      return fail("open MPHF", S3IMPH_ERR_IO);
    }
    uint8_t buf[1 << 16];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) h->mph.insert(h->mph.end(), buf, buf + k);
    const bool bad = std::ferror(f) != 0;
    std::fclose(f);
    if (bad) {
      m = "read " + dir + "/mph.bin";
      return fail("open MPHF", S3IMPH_ERR_IO);
    }
  }
  uint64_t mph_keys = 0;
  if (!mph_bin_framed(h->mph.data(), h->mph.size(), &mph_keys, &m)) return fail("open MPHF", S3IMPH_ERR_FORMAT);
  if ((rc = read_array(dir + "/mph_fp.u64", 8, &h->fp, &m))) return fail("open MPHF: open fingerprints", rc);
  if ((rc = read_array(dir + "/mph_pos.u64", 8, &h->pos, &m))) return fail("open MPHF: open positions", rc);

  // beyond the headers (stricter than the reference, which trusts the files)
  const uint64_t n = h->send.count;
  h->n = n;
  auto counts = [&](const char* what, const char* name, uint64_t c) {
    if (c == n) return true;
    m = std::string(name) + " holds " + std::to_string(c) + " entries, subtree_end " + std::to_string(n);
    *msg = std::string(what) + ": " + m;
    return false;
  };
  if (!counts("open depth", "depth", h->depth.count)) return S3IMPH_ERR_FORMAT;
  if (oc && !counts("open object_count", "object_count", h->ocnt.count)) return S3IMPH_ERR_FORMAT;
  if (oc && !counts("open total_bytes", "total_bytes", h->tbytes.count)) return S3IMPH_ERR_FORMAT;
  if (!counts("open max_depth_in_subtree", "max_depth_in_subtree", h->mds.count)) return S3IMPH_ERR_FORMAT;
  if (!counts("open MPHF", "mph_fp", h->fp.count)) return S3IMPH_ERR_FORMAT;
  if (!counts("open MPHF", "mph_pos", h->pos.count)) return S3IMPH_ERR_FORMAT;
  if (mph_keys != n) {
    m = "mph.bin holds " + std::to_string(mph_keys) + " keys, the index " + std::to_string(n);
    return fail("open MPHF", S3IMPH_ERR_FORMAT);
  }
  if (n > 0xffffffffull) {
    m = "more than 2^32-1 nodes on one GPU";
    return fail("open subtree_end", S3IMPH_ERR_FORMAT);
  }
  const uint64_t no = h->doff.count;
  const uint64_t* o = h->doff.u64();
  if (no < 2 || no - 2 > 0xffffffffull) {
    m = "depth_offsets needs at least 2 entries";
    return fail("open depth index", S3IMPH_ERR_FORMAT);
  }
  if (o[0] != 0 || o[no - 1] != h->dpos.count) {
    m = "depth_offsets must run from 0 to the count of depth_positions";
    return fail("open depth index", S3IMPH_ERR_FORMAT);
  }
  for (uint64_t i = 1; i < no; ++i)
    if (o[i] < o[i - 1]) {
      m = "depth_offsets decreases at " + std::to_string(i);
      return fail("open depth index", S3IMPH_ERR_FORMAT);
    }
  h->max_depth = (uint32_t)(no - 2);  // OpenDepthIndex, depthindex.go:130-134
  const uint32_t* d = h->depth.u32();
  for (uint64_t i = 0; i < n; ++i)
    if (d[i] > h->max_depth) {
      m = "depth[" + std::to_string(i) + "] exceeds maxDepth " + std::to_string(h->max_depth);
      return fail("open depth", S3IMPH_ERR_FORMAT);
    }
  const uint64_t* dp = h->dpos.u64();
  for (uint64_t i = 0; i < h->dpos.count; ++i)
    if (dp[i] >= n) {
      m = "depth_positions[" + std::to_string(i) + "] is not a node";
      return fail("open depth index", S3IMPH_ERR_FORMAT);
    }
  const uint64_t* mp = h->pos.u64();
  for (uint64_t i = 0; i < n; ++i)
    if (mp[i] >= n) {
      m = "mph_pos[" + std::to_string(i) + "] is not a node";
      return fail("open MPHF", S3IMPH_ERR_FORMAT);
    }
  return load_host_tiers(dir, n, h, msg);
}

// What OpenMPHF loads for reverse lookup (mphf.go:226-238; OpenBlob, reader.go:213-229), checked
// on the host for an index of n nodes: no prefix_blob.bin is no prefixes, not an error.
struct HostPrefixes {
  bool present = false;
  HostArray off;
  std::vector<uint64_t> blob;  // round_up(size, 8) + 8 bytes, zero-padded (load8's contract)
};

int load_host_prefixes(const std::string& dir, uint64_t n, HostPrefixes* p, std::string* msg) {
  const std::string bp = dir + "/prefix_blob.bin";
  if (!file_exists(bp)) return S3IMPH_OK;
  auto fail = [&](const std::string& m, int code) {
    *msg = "open MPHF: open prefix blob: " + m;
    return code;
  };
  FILE* f = std::fopen(bp.c_str(), "rb");
  if (!f) return fail("open blob: open " + bp + ": " + std::strerror(errno), S3IMPH_ERR_IO);
  struct Close {
    FILE* f;
    ~Close() { std::fclose(f); }
  } closer{f};
  struct stat st;
  if (::fstat(fileno(f), &st) != 0) return fail("open blob: stat " + bp + ": " + std::strerror(errno), S3IMPH_ERR_IO);
  const uint64_t size = (uint64_t)st.st_size;
  std::string m;
  const int rc = read_array(dir + "/prefix_offsets.u64", 8, &p->off, &m);
  if (rc != S3IMPH_OK) return fail("open offsets: " + m, rc);
  // beyond the header: what the reference checks per Get (reader.go:250-270), once
  if (p->off.count != n + 1)
    return fail("prefix_offsets holds " + std::to_string(p->off.count) + " entries, the index " + std::to_string(n) +
                    " nodes",
                S3IMPH_ERR_FORMAT);
  const uint64_t* o = p->off.u64();
  for (uint64_t i = 1; i <= n; ++i)
    if (o[i] < o[i - 1]) return fail("prefix_offsets decreases at " + std::to_string(i), S3IMPH_ERR_FORMAT);
  if (o[n] > size)
    return fail("prefix_offsets ends at " + std::to_string(o[n]) + ", the blob holds " + std::to_string(size) +
                    " bytes",
                S3IMPH_ERR_FORMAT);
  p->blob.assign((size + 7) / 8 + 1, 0);
  if (size && std::fread(p->blob.data(), 1, size, f) != size)
    return fail("open blob: read " + bp + ": " + std::strerror(errno), S3IMPH_ERR_IO);
  p->present = true;
  return S3IMPH_OK;
}

}  // namespace
}  // namespace s3imph

using namespace s3imph;

// The handle: the arrays (owned after Open, borrowed after attach), a context for the MPHF
// levels and the rank directory, and the plan / fill workspace.
struct s3imph_index {
  int device = 0;
  s3imph_ctx* ctx = nullptr;
  std::mutex mu;
  std::string last_msg;
  IndexArrays a;
  std::vector<void*> owned;  // device allocations of Open
  // tier data (Open, or s3imph_index_attach_tiers): T manifest slots, their ids, the table
  // [n][2 T] in HBM (owned either way)
  uint32_t T = 0;
  uint8_t tier_ids[S3IMPH_NUM_TIERS] = {};
  uint64_t* tier_table = nullptr;
  // workspace of the last plan: per row the slice start, the unfiltered length and the
  // unfiltered row_ptr U (rows + 1); scan block sums; per chunk the flag counts and their prefix
  uint64_t *row_lo = nullptr, *row_len = nullptr, *U = nullptr, *sums = nullptr;
  uint64_t rows_cap = 0;
  uint64_t *csum = nullptr, *cbase = nullptr, *csums2 = nullptr;
  uint64_t chunks_cap = 0;
  bool have_plan = false;
  uint64_t plan_rows = 0, plan_total_u = 0, plan_total = 0, plan_mc = 0, plan_mb = 0;
  bool plan_filtered = false;
  // workspace of descendants_top: the filled positions, their keys and both sorted (4 x cap
  // words), the filtered row_ptr (rows + 1), the segmented sort's temporary
  uint64_t* top_buf = nullptr;
  uint64_t top_cap = 0;
  uint64_t* top_rp = nullptr;
  uint64_t top_rp_cap = 0;
  PrimTmp top_tmp;
  // the stored prefixes (Open with S3IMPH_OPEN_PREFIXES: owned; s3imph_index_attach_prefixes: borrowed)
  bool has_prefixes = false;
  PrefixBlob pb;
  // workspace of the last prefixes plan, apart from the descendants plan's: per row the source
  // address and the length, the output offsets (rows + 1), scan block sums; the emit's chunk owners
  uint64_t *nm_src = nullptr, *nm_len = nullptr, *nm_off = nullptr, *nm_sums = nullptr;
  uint64_t nm_cap = 0;
  uint64_t* nm_bounds = nullptr;
  uint64_t nm_bounds_cap = 0;
  bool have_names = false;
  uint64_t names_rows = 0, names_total = 0;
  // workspace of verify: the lookup's answers (n words), the reduction's three result words
  uint64_t* vf_got = nullptr;
  uint64_t vf_cap = 0;
  unsigned long long* vf_res = nullptr;
};

namespace s3imph {
namespace {

// A device call on the index: the device frame, with the last message cleared on entry.
template <class F>
int index_entry(s3imph_index* x, F&& body) {
  return device_entry(x, "", [&](std::string& msg) -> int {
    x->last_msg.clear();
    return body(msg);
  });
}

void index_free(s3imph_index* x) {
  if (!x) return;
  (void)hipSetDevice(x->device);
  if (x->ctx) (void)s3imph_ctx_destroy(x->ctx);  // drains its stream first
  for (void* p : x->owned)
    if (p) (void)hipFree(p);
  for (uint64_t** p : {&x->row_lo, &x->row_len, &x->U, &x->sums, &x->csum, &x->cbase, &x->csums2, &x->tier_table,
                       &x->top_buf, &x->top_rp, &x->nm_src, &x->nm_len, &x->nm_off, &x->nm_sums, &x->nm_bounds,
                       &x->vf_got})
    dfree(*p);
  dfree(x->vf_res);
  x->top_tmp.release();
  delete x;
}

template <typename T>
const T* upload(s3imph_index* x, const T* host, uint64_t count) {
  void* v = nullptr;
  HIPCHECK(hipMalloc(&v, std::max<uint64_t>(count, 1) * sizeof(T)));
  x->owned.push_back(v);
  if (count) HIPCHECK(hipMemcpy(v, host, count * sizeof(T), hipMemcpyHostToDevice));
  return static_cast<const T*>(v);
}

// A handle on `device` with the MPHF loaded; throws Fail.
s3imph_index* index_new(int device, const uint8_t* mph, uint64_t mph_len, uint64_t n) {
  s3imph_index* x = new s3imph_index();
  x->device = device;
  try {
    char err[256] = "";
    int rc = s3imph_ctx_create(device, &x->ctx, err, sizeof err);
    if (rc != S3IMPH_OK) throw Fail{rc, err};
    rc = s3imph_ctx_load_mph_bin(x->ctx, mph_len ? mph : nullptr, mph_len);
    if (rc != S3IMPH_OK) {
      const std::string m = s3imph_ctx_last_error(x->ctx);
      throw Fail{rc, m.empty() ? std::string("open MPHF: ") + s3imph_status_string(rc) : m};
    }
    if (x->ctx->last_n != n)
      throw Fail{S3IMPH_ERR_FORMAT, "open MPHF: mph.bin holds " + std::to_string(x->ctx->last_n) + " keys, the index " +
                                        std::to_string(n)};
    return x;
  } catch (...) {
    index_free(x);
    throw;
  }
}

uint64_t scan_blocks(uint64_t n) { return (n + kScanB - 1) / kScanB; }

// out[0 .. n] (and out2) = exclusive prefix of in[0 .. n); sums: scan_blocks(n) + 1 words.
void launch_rows_scan(const uint64_t* in, uint64_t n, uint64_t* sums, uint64_t* out, uint64_t* out2, hipStream_t s) {
  const uint64_t nb = scan_blocks(n);
  if (nb == 0) return;
  k_rows_reduce<<<(unsigned)nb, kScanT, 0, s>>>(in, n, sums);
  k_rows_top<<<1, 1024, 0, s>>>(sums, nb);
  k_rows_down<<<(unsigned)nb, kScanT, 0, s>>>(in, n, sums, nb, out, out2);
}

void ensure_rows(s3imph_index* x, uint64_t rows) {
  if (rows <= x->rows_cap) return;
  x->rows_cap = 0;
  dalloc(x->row_lo, rows);
  dalloc(x->row_len, rows);
  dalloc(x->U, rows + 1);
  dalloc(x->sums, scan_blocks(rows) + 1);
  x->rows_cap = rows;
}

void ensure_chunks(s3imph_index* x, uint64_t chunks) {
  if (chunks <= x->chunks_cap) return;
  x->chunks_cap = 0;
  dalloc(x->csum, chunks);
  dalloc(x->cbase, chunks + 1);
  dalloc(x->csums2, scan_blocks(chunks) + 1);
  x->chunks_cap = chunks;
}

int plan_locked(s3imph_index* x, const uint64_t* d_qpos, const int32_t* d_rel, uint64_t nq, int mode, int32_t max_rel,
                uint64_t min_count, uint64_t min_bytes, int32_t* d_levels, uint64_t* d_row_ptr, uint64_t row_ptr_cap,
                uint64_t* n_rows, uint64_t* total, hipStream_t s, std::string* msg) {
  const bool upto = mode == S3IMPH_DESC_UPTO, filtered = min_count || min_bytes;
  const uint64_t R = upto ? std::min<uint64_t>(max_rel > 0 ? (uint64_t)max_rel : 0, x->a.max_depth) : 1;
  x->have_plan = false;
  if (nq == 0) {
    x->have_plan = true;
    x->plan_rows = x->plan_total_u = x->plan_total = 0;
    x->plan_filtered = false;
    return S3IMPH_OK;
  }
  if (R && nq > ((1ull << 31) - 1) / R) {
    *msg = "descendants plan: 2^31 result rows or more in one batch";
    return S3IMPH_ERR_INVALID;
  }
  const uint64_t rows = nq * R;
  if (row_ptr_cap < rows + 1) {
    *msg = "descendants plan: row_ptr needs " + std::to_string(rows + 1) + " entries";
    return S3IMPH_ERR_INVALID;
  }
  *n_rows = rows;
  if (rows == 0) {  // UPTO with no level to return: every query answers nil
    HIPCHECK(hipMemsetAsync(d_levels, 0, nq * sizeof(int32_t), s));
    HIPCHECK(hipMemsetAsync(d_row_ptr, 0, sizeof(uint64_t), s));
    HIPCHECK(hipStreamSynchronize(s));
    x->have_plan = true;
    x->plan_rows = x->plan_total_u = x->plan_total = 0;
    x->plan_filtered = false;
    return S3IMPH_OK;
  }
  ensure_rows(x, rows);
  k_desc_ranges<<<(unsigned)((rows + kQT - 1) / kQT), kQT, 0, s>>>(x->a, d_qpos, d_rel, rows, upto ? 1 : 0, (uint32_t)R,
                                                                  max_rel, d_levels, x->row_lo, x->row_len);
  launch_rows_scan(x->row_len, rows, x->sums, x->U, filtered ? nullptr : d_row_ptr, s);
  HIPCHECK(hipGetLastError());
  uint64_t tu = 0;
  HIPCHECK(hipMemcpyAsync(&tu, x->U + rows, sizeof tu, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  uint64_t tf = tu;
  if (filtered) {
    if (tu == 0) {
      HIPCHECK(hipMemsetAsync(d_row_ptr, 0, (rows + 1) * sizeof(uint64_t), s));
    } else {
      const uint64_t chunks = (tu + kChunk - 1) / kChunk;
      if (chunks + 1 > 0x7fffffffull) {
        *msg = "descendants plan: more than 2^42 candidates in one batch";
        return S3IMPH_ERR_INVALID;
      }
      ensure_chunks(x, chunks);
      k_desc_filter<kCount><<<(unsigned)chunks, kChunkT, 0, s>>>(x->a, x->U, x->row_lo, rows, tu, min_count, min_bytes,
                                                                 x->csum, nullptr, nullptr, nullptr);
      launch_rows_scan(x->csum, chunks, x->csums2, x->cbase, nullptr, s);
      k_desc_filter<kRows><<<(unsigned)(tu / kChunk + 1), kChunkT, 0, s>>>(
          x->a, x->U, x->row_lo, rows, tu, min_count, min_bytes, nullptr, x->cbase, d_row_ptr, nullptr);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipMemcpyAsync(&tf, x->cbase + chunks, sizeof tf, hipMemcpyDeviceToHost, s));
    }
    HIPCHECK(hipStreamSynchronize(s));
    if (tu == 0) tf = 0;
  }
  *total = tf;
  x->have_plan = true;
  x->plan_rows = rows;
  x->plan_total_u = tu;
  x->plan_total = tf;
  x->plan_filtered = filtered;
  x->plan_mc = min_count;
  x->plan_mb = min_bytes;
  return S3IMPH_OK;
}

// The positions of the plan's rows into out (plan_total entries, > 0); the caller holds the lock.
int fill_locked(s3imph_index* x, uint64_t* out, const char* what, hipStream_t s, std::string* msg) {
  const uint64_t tu = x->plan_total_u, chunks = (tu + kChunk - 1) / kChunk;
  if (chunks > 0x7fffffffull) {
    *msg = std::string(what) + ": more than 2^42 positions in one batch";
    return S3IMPH_ERR_INVALID;
  }
  if (x->plan_filtered)
    k_desc_filter<kFill><<<(unsigned)chunks, kChunkT, 0, s>>>(x->a, x->U, x->row_lo, x->plan_rows, tu, x->plan_mc,
                                                             x->plan_mb, nullptr, x->cbase, nullptr, out);
  else
    k_desc_fill<<<(unsigned)chunks, kChunkT, 0, s>>>(x->U, x->row_lo, x->plan_rows, tu, x->a.dpos, out);
  HIPCHECK(hipGetLastError());
  return S3IMPH_OK;
}

int top_locked(s3imph_index* x, int key, const s3imph_price_table& pt, uint32_t k, uint64_t* d_top_pos,
               uint64_t* d_top_key, uint32_t* d_top_n, hipStream_t s, std::string* msg) {
  const uint64_t rows = x->plan_rows, total = x->plan_total;
  if (rows == 0) return S3IMPH_OK;
  const uint64_t* rp = nullptr;
  uint64_t *spos = nullptr, *skey = nullptr;
  if (total) {
    grow(x->top_buf, x->top_cap, 4 * total);
    uint64_t *pos = x->top_buf, *keys = pos + total;
    spos = keys + total;
    skey = spos + total;
    const int rc = fill_locked(x, pos, "descendants top", s, msg);
    if (rc != S3IMPH_OK) return rc;
    if (x->plan_filtered) {  // the plan wrote the filtered row_ptr to the caller only: read it off again
      grow(x->top_rp, x->top_rp_cap, rows + 1);
      const uint64_t tu = x->plan_total_u;
      k_desc_filter<kRows><<<(unsigned)(tu / kChunk + 1), kChunkT, 0, s>>>(
          x->a, x->U, x->row_lo, rows, tu, x->plan_mc, x->plan_mb, nullptr, x->cbase, x->top_rp, nullptr);
      rp = x->top_rp;
    } else {
      rp = x->U;
    }
    TierSlots slots{};
    std::memcpy(slots.id, x->tier_ids, sizeof slots.id);
    k_rank_keys<<<(unsigned)((total + kQT - 1) / kQT), kQT, 0, s>>>(x->a, x->tier_table, x->T, slots, pt, key, pos, total,
                                                                   keys);
    HIPCHECK(hipGetLastError());
    // the segmented sort gives a segment to one workgroup (1M positions in one row: 41 ms): a lone
    // row is sorted device-wide instead
    if (rows == 1)
      sort_pairs_desc(x->top_tmp, keys, skey, pos, spos, total, s);
    else
      sort_rows_pairs_desc(x->top_tmp, keys, skey, pos, spos, total, rows, rp, s);
  }
  k_rows_take<<<(unsigned)((rows * k + kQT - 1) / kQT), kQT, 0, s>>>(rp, spos, skey, rows, k, d_top_pos, d_top_key,
                                                                    d_top_n);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));
  return S3IMPH_OK;
}

// Every query over the stored prefixes on a handle without them (VerifyMPHF's words, mphf.go:374).
int no_prefixes(const char* what, std::string* msg) {
  *msg = std::string(what) + ": prefix blob not loaded";
  return S3IMPH_ERR_STATE;
}

int names_plan_locked(s3imph_index* x, const uint64_t* d_qpos, uint64_t nq, uint64_t* d_out_offsets, uint32_t* d_found,
                      uint64_t* total, hipStream_t s) {
  x->have_names = false;
  if (nq > x->nm_cap) {
    x->nm_cap = 0;
    dalloc(x->nm_src, nq);
    dalloc(x->nm_len, nq);
    dalloc(x->nm_off, nq + 1);
    dalloc(x->nm_sums, scan_blocks(nq) + 1);
    x->nm_cap = nq;
  }
  k_names_len<<<(unsigned)((nq + kQT - 1) / kQT), kQT, 0, s>>>(x->pb, x->a.n, d_qpos, nq, x->nm_src, x->nm_len, d_found);
  launch_rows_scan(x->nm_len, nq, x->nm_sums, x->nm_off, d_out_offsets, s);
  HIPCHECK(hipGetLastError());
  uint64_t t = 0;
  HIPCHECK(hipMemcpyAsync(&t, x->nm_off + nq, sizeof t, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  *total = t;
  x->names_rows = nq;
  x->names_total = t;
  x->have_names = true;
  return S3IMPH_OK;
}

int names_fill_locked(s3imph_index* x, uint8_t* d_out, hipStream_t s, std::string* msg) {
  const uint64_t total = x->names_total, nw = (total + 7) / 8, chunks = (nw + kChunkT - 1) / kChunkT;
  if (chunks > 0x7fffffffull) {
    *msg = "prefixes fill: more than 2^42 bytes in one batch";
    return S3IMPH_ERR_INVALID;
  }
  grow(x->nm_bounds, x->nm_bounds_cap, chunks);
  k_names_bounds<<<(unsigned)((chunks + kChunkT - 1) / kChunkT), kChunkT, 0, s>>>(x->nm_off, x->names_rows + 1, chunks,
                                                                                 x->nm_bounds);
  k_names_emit<<<(unsigned)chunks, kChunkT, 0, s>>>(x->pb, x->nm_off, x->nm_bounds, x->nm_src, x->names_rows, total,
                                                    d_out);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));
  return S3IMPH_OK;
}

// got[i] = Lookup(stored prefix i) for the whole index, reduced on the device.
int verify_locked(s3imph_index* x, uint64_t* n_bad, uint64_t* first_bad, uint64_t* first_got, hipStream_t s) {
  const uint64_t n = x->a.n;
  grow(x->vf_got, x->vf_cap, n);
  if (!x->vf_res) dalloc(x->vf_res, 3);
  const int rc = s3imph_lookup_device(x->ctx, x->pb.blob, x->pb.off, n, x->a.fp, x->a.pos, n, x->vf_got, s);
  if (rc != S3IMPH_OK) throw Fail{rc, std::string("verify: lookup: ") + s3imph_status_string(rc)};
  HIPCHECK(hipMemsetAsync(x->vf_res, 0, 8, s));
  HIPCHECK(hipMemsetAsync(x->vf_res + 1, 0xff, 16, s));
  const uint64_t blocks = std::min<uint64_t>((n + kQT - 1) / kQT, 4096);
  k_verify_reduce<<<(unsigned)blocks, kQT, 0, s>>>(x->vf_got, n, x->vf_res);
  k_verify_got<<<1, 1, 0, s>>>(x->vf_got, x->vf_res);
  HIPCHECK(hipGetLastError());
  unsigned long long r[3] = {0, 0, 0};
  HIPCHECK(hipMemcpyAsync(r, x->vf_res, sizeof r, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  *n_bad = r[0];
  *first_bad = r[1];
  *first_got = r[2];
  return S3IMPH_OK;
}

int open_index(int device, const char* dir, unsigned flags, s3imph_index** out, char* err, size_t errlen) {
  if (!out || !dir || (flags & ~(unsigned)S3IMPH_OPEN_PREFIXES)) {
    set_err(err, errlen, "invalid argument");
    return S3IMPH_ERR_INVALID;
  }
  *out = nullptr;
  try {
    HostIndex h;
    HostPrefixes hp;
    std::string msg;
    // all validation on the host, before the device is selected or anything allocated on it
    int rc = load_host_index(dir, &h, &msg);
    if (rc == S3IMPH_OK && (flags & S3IMPH_OPEN_PREFIXES)) rc = load_host_prefixes(dir, h.n, &hp, &msg);
    if (rc != S3IMPH_OK) {
      set_err(err, errlen, msg);
      return rc;
    }
    s3imph_index* x = nullptr;
    try {
      x = index_new(device, h.mph.data(), h.mph.size(), h.n);
      HIPCHECK(hipSetDevice(device));
      x->a.n = h.n;
      x->a.max_depth = h.max_depth;
      x->a.send = upload(x, h.send.u64(), h.n);
      x->a.depth = upload(x, h.depth.u32(), h.n);
      x->a.mds = upload(x, h.mds.u32(), h.n);
      x->a.doff = upload(x, h.doff.u64(), h.doff.count);
      x->a.dpos = upload(x, h.dpos.u64(), h.dpos.count);
      x->a.fp = upload(x, h.fp.u64(), h.n);
      x->a.pos = upload(x, h.pos.u64(), h.n);
      if (h.stats) {
        x->a.ocnt = upload(x, h.ocnt.u64(), h.n);
        x->a.tbytes = upload(x, h.tbytes.u64(), h.n);
      }
      if (!h.tiers.empty()) {
        dalloc(x->tier_table, h.tier_table.size());
        if (!h.tier_table.empty())
          HIPCHECK(hipMemcpy(x->tier_table, h.tier_table.data(), h.tier_table.size() * 8, hipMemcpyHostToDevice));
        x->T = (uint32_t)h.tiers.size();
        for (uint32_t k = 0; k < x->T; ++k) x->tier_ids[k] = (uint8_t)h.tiers[k].id;
      }
      if (hp.present) {
        x->pb.off = upload(x, hp.off.u64(), h.n + 1);
        x->pb.blob = reinterpret_cast<const uint8_t*>(upload(x, hp.blob.data(), hp.blob.size()));
        x->pb.end8 = (hp.off.u64()[h.n] + 7) & ~7ull;
        x->has_prefixes = true;
      }
    } catch (const Fail& f) {
      index_free(x);
      set_err(err, errlen, f.msg);
      return f.code;
    }
    *out = x;
    return S3IMPH_OK;
  } catch (const std::bad_alloc&) {
    set_err(err, errlen, "open index: out of host memory");
    return S3IMPH_ERR_NOMEM;
  }
}

}  // namespace
}  // namespace s3imph

extern "C" {

int s3imph_index_open(int device, const char* dir, s3imph_index** out, char* err, size_t errlen) {
  return open_index(device, dir, 0, out, err, errlen);
}

int s3imph_index_open_flags(int device, const char* dir, unsigned flags, s3imph_index** out, char* err,
                            size_t errlen) {
  return open_index(device, dir, flags, out, err, errlen);
}

int s3imph_index_attach(int device, const s3imph_index_arrays* a, s3imph_index** out, char* err, size_t errlen) {
  if (!out || !a || (a->mph_len && !a->mph_bin) || !a->d_depth_offsets ||
      (a->n && (!a->d_fp || !a->d_pos || !a->d_depth || !a->d_max_depth_in_subtree || !a->d_subtree_end ||
                !a->d_depth_positions)) ||
      (a->d_object_count == nullptr) != (a->d_total_bytes == nullptr) || a->n > 0xffffffffull ||
      (a->n == 0) != (a->mph_len == 0)) {
    set_err(err, errlen, "invalid argument");
    return S3IMPH_ERR_INVALID;
  }
  *out = nullptr;
  try {
    s3imph_index* x = index_new(device, a->mph_bin, a->mph_len, a->n);
    x->a.n = a->n;
    x->a.max_depth = a->max_depth;
    x->a.fp = a->d_fp;
    x->a.pos = a->d_pos;
    x->a.depth = a->d_depth;
    x->a.mds = a->d_max_depth_in_subtree;
    x->a.send = a->d_subtree_end;
    x->a.doff = a->d_depth_offsets;
    x->a.dpos = a->d_depth_positions;
    x->a.ocnt = a->d_object_count;
    x->a.tbytes = a->d_total_bytes;
    *out = x;
    return S3IMPH_OK;
  } catch (const Fail& f) {
    set_err(err, errlen, f.msg);
    return f.code;
  } catch (const std::bad_alloc&) {
    set_err(err, errlen, "attach index: out of host memory");
    return S3IMPH_ERR_NOMEM;
  }
}

int s3imph_index_close(s3imph_index* x) {
  index_free(x);
  return S3IMPH_OK;
}

uint64_t s3imph_index_count(const s3imph_index* x) { return x ? x->a.n : 0; }

uint64_t s3imph_index_max_depth(const s3imph_index* x) { return x ? x->a.max_depth : 0; }

const char* s3imph_index_last_error(s3imph_index* x) { return x ? x->last_msg.c_str() : ""; }

int s3imph_index_lookup_device(s3imph_index* x, const uint8_t* d_blob, const uint64_t* d_offsets, uint64_t nq,
                               uint64_t* d_pos_out, void* stream) {
  if (!x || (nq && (!d_blob || !d_offsets || !d_pos_out))) return S3IMPH_ERR_INVALID;
  std::lock_guard<std::mutex> lk(x->mu);
  x->last_msg.clear();
  const int rc = s3imph_lookup_device(x->ctx, d_blob, d_offsets, nq, x->a.fp, x->a.pos, x->a.n, d_pos_out, stream);
  if (rc != S3IMPH_OK) x->last_msg = std::string("lookup: ") + s3imph_status_string(rc);
  return rc;
}

int s3imph_index_nodes_device(s3imph_index* x, const uint64_t* d_qpos, uint64_t nq, s3imph_node* d_out, void* stream) {
  if (!x || (nq && (!d_qpos || !d_out))) return S3IMPH_ERR_INVALID;
  return index_entry(x, [&](std::string&) -> int {
    if (nq == 0) return S3IMPH_OK;
    hipStream_t s = use_device(x->device, stream, x->ctx->own_stream);
    k_index_nodes<<<(unsigned)((nq + kQT - 1) / kQT), kQT, 0, s>>>(x->a, d_qpos, nq, d_out);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    return S3IMPH_OK;
  });
}

int s3imph_index_attach_tiers(s3imph_index* x, const uint8_t* ids, uint64_t T, const uint64_t* d_tier_count,
                              const uint64_t* d_tier_bytes, uint64_t stride) {
  if (!x) return S3IMPH_ERR_INVALID;
  return index_entry(x, [&](std::string& msg) -> int {
    unsigned seen = 0;
    bool ok = T <= (uint64_t)S3IMPH_NUM_TIERS && (T == 0 || ids) && stride >= x->a.n &&
              (T == 0 || x->a.n == 0 || (d_tier_count && d_tier_bytes));
    for (uint64_t k = 0; ok && k < T; ++k) {
      ok = ids[k] < S3IMPH_NUM_TIERS && !((seen >> ids[k]) & 1);
      seen |= 1u << (ids[k] & 31);
    }
    if (!ok) {
      msg = "attach tiers: invalid argument";
      return S3IMPH_ERR_INVALID;
    }
    hipStream_t s = use_device(x->device, nullptr, x->ctx->own_stream);
    x->T = 0;
    dfree(x->tier_table);
    if (T == 0) return S3IMPH_OK;
    dalloc(x->tier_table, x->a.n * 2 * T);
    TierSlots slots{};
    for (uint64_t k = 0; k < T; ++k) slots.id[k] = ids[k];
    if (x->a.n) {
      k_tier_interleave<<<(unsigned)((x->a.n + kQT - 1) / kQT), kQT, 0, s>>>(d_tier_count, d_tier_bytes, stride, x->a.n,
                                                                            (uint32_t)T, slots, x->tier_table);
      HIPCHECK(hipGetLastError());
      HIPCHECK(hipStreamSynchronize(s));
    }
    std::memcpy(x->tier_ids, slots.id, sizeof slots.id);
    x->T = (uint32_t)T;
    return S3IMPH_OK;
  });
}

uint64_t s3imph_index_tier_count(const s3imph_index* x) { return x ? x->T : 0; }

uint64_t s3imph_index_tier_ids(const s3imph_index* x, uint8_t* ids, uint64_t cap) {
  if (!x) return 0;
  for (uint64_t k = 0; ids && k < x->T && k < cap; ++k) ids[k] = x->tier_ids[k];
  return x->T;
}

int s3imph_index_tiers_device(s3imph_index* x, const uint64_t* d_qpos, uint64_t nq, uint64_t* d_out, uint32_t* d_mask,
                              void* stream) {
  if (!x) return S3IMPH_ERR_INVALID;
  return index_entry(x, [&](std::string& msg) -> int {
    if (x->T == 0 || nq == 0) return S3IMPH_OK;  // no tier data: nothing is written
    if (!d_qpos || !d_out || !d_mask) return S3IMPH_ERR_INVALID;
    hipStream_t s = use_device(x->device, stream, x->ctx->own_stream);
    const uint32_t qb = kQT / x->T;
    const uint64_t blocks = (nq + qb - 1) / qb;
    if (blocks > 0x7fffffffull) {
      msg = "tier breakdown: more than 2^31 workgroups of queries in one batch";
      return S3IMPH_ERR_INVALID;
    }
    k_index_tiers<<<(unsigned)blocks, kQT, 0, s>>>(x->tier_table, x->a.n, x->T, qb, d_qpos, nq, d_out, d_mask);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    return S3IMPH_OK;
  });
}

int s3imph_index_descendants_plan(s3imph_index* x, const uint64_t* d_qpos, const int32_t* d_rel, uint64_t nq, int mode,
                                  int32_t max_rel, uint64_t min_count, uint64_t min_bytes, int32_t* d_levels,
                                  uint64_t* d_row_ptr, uint64_t row_ptr_cap, uint64_t* n_rows, uint64_t* total,
                                  void* stream) {
  if (!x || !n_rows || !total) return S3IMPH_ERR_INVALID;
  *n_rows = 0;
  *total = 0;
  return index_entry(x, [&](std::string& msg) -> int {
    const bool filtered = min_count || min_bytes;
    if ((mode != S3IMPH_DESC_AT && mode != S3IMPH_DESC_UPTO) || (mode == S3IMPH_DESC_UPTO && filtered) ||
        (nq && (!d_qpos || !d_levels || !d_row_ptr)) || (nq && mode == S3IMPH_DESC_AT && !d_rel)) {
      msg = mode == S3IMPH_DESC_UPTO && filtered ? "descendants plan: no filter with DescendantsUpToDepth"
                                                 : "descendants plan: invalid argument";
      return S3IMPH_ERR_INVALID;
    }
    if (filtered && !x->a.ocnt) {
      msg = "descendants plan: the index has no object_count / total_bytes to filter on";
      return S3IMPH_ERR_STATE;
    }
    x->have_plan = false;  // whatever is thrown from here on leaves no plan (plan_locked sets it)
    hipStream_t s = use_device(x->device, stream, x->ctx->own_stream);
    return retry_on_nomem(x->ctx, s, &msg, [&] {
      return plan_locked(x, d_qpos, d_rel, nq, mode, max_rel, min_count, min_bytes, d_levels, d_row_ptr, row_ptr_cap,
                         n_rows, total, s, &msg);
    });
  });
}

int s3imph_index_descendants_fill(s3imph_index* x, uint64_t* d_out, uint64_t cap, void* stream) {
  if (!x) return S3IMPH_ERR_INVALID;
  return index_entry(x, [&](std::string& msg) -> int {
    if (!x->have_plan) {
      msg = "descendants fill: no plan";
      return S3IMPH_ERR_STATE;
    }
    if (cap < x->plan_total || (x->plan_total && !d_out)) {
      msg = "descendants fill: out needs " + std::to_string(x->plan_total) + " entries";
      return S3IMPH_ERR_INVALID;
    }
    if (x->plan_total == 0) return S3IMPH_OK;
    hipStream_t s = use_device(x->device, stream, x->ctx->own_stream);
    const int rc = fill_locked(x, d_out, "descendants fill", s, &msg);
    if (rc != S3IMPH_OK) return rc;
    HIPCHECK(hipStreamSynchronize(s));
    return S3IMPH_OK;
  });
}

int s3imph_index_cost_device(s3imph_index* x, const uint64_t* d_qpos, uint64_t nq, const s3imph_price_table* pt,
                             s3imph_cost* d_out, void* stream) {
  if (!x || !pt || (nq && (!d_qpos || !d_out))) return S3IMPH_ERR_INVALID;
  return index_entry(x, [&](std::string& msg) -> int {
    if (*price_table_fault(*pt)) {
      msg = std::string("pricing: ") + price_table_fault(*pt);
      return S3IMPH_ERR_INVALID;
    }
    if (nq == 0) return S3IMPH_OK;
    hipStream_t s = use_device(x->device, stream, x->ctx->own_stream);
    const uint32_t Tl = x->T ? x->T : 1, qb = kQT / Tl;
    const uint64_t blocks = (nq + qb - 1) / qb;
    if (blocks > 0x7fffffffull) {
      msg = "pricing: more than 2^31 workgroups of queries in one batch";
      return S3IMPH_ERR_INVALID;
    }
    TierSlots slots{};
    std::memcpy(slots.id, x->tier_ids, sizeof slots.id);
    k_index_cost<<<(unsigned)blocks, kQT, qb * sizeof(s3imph_cost), s>>>(
        x->tier_table, x->a.n, x->T, Tl, qb, slots, *pt, d_qpos, nq, reinterpret_cast<uint64_t*>(d_out));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    return S3IMPH_OK;
  });
}

int s3imph_index_descendants_top(s3imph_index* x, int key, const s3imph_price_table* pt, uint32_t k,
                                 uint64_t* d_top_pos, uint64_t* d_top_key, uint32_t* d_top_n, void* stream) {
  if (!x) return S3IMPH_ERR_INVALID;
  return index_entry(x, [&](std::string& msg) -> int {
    const bool cost = key == S3IMPH_RANK_MONTHLY_COST;
    if (k == 0 || (key != S3IMPH_RANK_OBJECT_COUNT && key != S3IMPH_RANK_TOTAL_BYTES && !cost) || (cost && !pt)) {
      msg = "descendants top: invalid argument";
      return S3IMPH_ERR_INVALID;
    }
    if (cost && *price_table_fault(*pt)) {
      msg = std::string("pricing: ") + price_table_fault(*pt);
      return S3IMPH_ERR_INVALID;
    }
    if (!x->have_plan) {
      msg = "descendants top: no plan";
      return S3IMPH_ERR_STATE;
    }
    if (!cost && !x->a.ocnt) {
      msg = "descendants top: the index has no object_count / total_bytes to rank by";
      return S3IMPH_ERR_STATE;
    }
    if (cost && x->T == 0) {
      msg = "descendants top: the index has no tier data to price";
      return S3IMPH_ERR_STATE;
    }
    if (x->plan_rows * k >= (1ull << 31)) {
      msg = "descendants top: n_rows * k is 2^31 or more";
      return S3IMPH_ERR_INVALID;
    }
    if (x->plan_total >= (1ull << 32)) {
      msg = "descendants top: 2^32 positions or more in the plan";
      return S3IMPH_ERR_INVALID;
    }
    if (x->plan_rows && (!d_top_pos || !d_top_key || !d_top_n)) {
      msg = "descendants top: invalid argument";
      return S3IMPH_ERR_INVALID;
    }
    hipStream_t s = use_device(x->device, stream, x->ctx->own_stream);
    const s3imph_price_table none{};
    return retry_on_nomem(x->ctx, s, &msg, [&] {
      return top_locked(x, key, cost ? *pt : none, k, d_top_pos, d_top_key, d_top_n, s, &msg);
    });
  });
}

int s3imph_index_attach_prefixes(s3imph_index* x, const uint8_t* d_blob, const uint64_t* d_offsets) {
  if (!x) return S3IMPH_ERR_INVALID;
  return index_entry(x, [&](std::string& msg) -> int {
    if (!d_blob || !d_offsets) {
      msg = "attach prefixes: invalid argument";
      return S3IMPH_ERR_INVALID;
    }
    hipStream_t s = use_device(x->device, nullptr, x->ctx->own_stream);
    uint64_t end = 0;
    HIPCHECK(hipMemcpyAsync(&end, d_offsets + x->a.n, sizeof end, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    x->have_names = false;  // its source addresses were the earlier blob's
    x->pb.blob = d_blob;
    x->pb.off = d_offsets;
    x->pb.end8 = (end + 7) & ~7ull;
    x->has_prefixes = true;
    return S3IMPH_OK;
  });
}

int s3imph_index_has_prefixes(const s3imph_index* x) { return x && x->has_prefixes ? 1 : 0; }

int s3imph_index_prefixes_plan(s3imph_index* x, const uint64_t* d_qpos, uint64_t nq, uint64_t* d_out_offsets,
                               uint32_t* d_found, uint64_t* total, void* stream) {
  if (!x || !total) return S3IMPH_ERR_INVALID;
  *total = 0;
  return index_entry(x, [&](std::string& msg) -> int {
    if (!x->has_prefixes) return no_prefixes("prefixes plan", &msg);
    if (nq && (!d_qpos || !d_out_offsets)) {
      msg = "prefixes plan: invalid argument";
      return S3IMPH_ERR_INVALID;
    }
    if (nq >= (1ull << 31)) {
      msg = "prefixes plan: 2^31 positions or more in one batch";
      return S3IMPH_ERR_INVALID;
    }
    x->have_names = false;  // whatever is thrown from here on leaves no plan
    if (nq == 0) {
      if (d_out_offsets) {
        hipStream_t s0 = use_device(x->device, stream, x->ctx->own_stream);
        HIPCHECK(hipMemsetAsync(d_out_offsets, 0, sizeof(uint64_t), s0));
        HIPCHECK(hipStreamSynchronize(s0));
      }
      x->names_rows = x->names_total = 0;
      x->have_names = true;
      return S3IMPH_OK;
    }
    hipStream_t s = use_device(x->device, stream, x->ctx->own_stream);
    return retry_on_nomem(x->ctx, s, &msg,
                          [&] { return names_plan_locked(x, d_qpos, nq, d_out_offsets, d_found, total, s); });
  });
}

int s3imph_index_prefixes_fill(s3imph_index* x, uint8_t* d_out, uint64_t cap, void* stream) {
  if (!x) return S3IMPH_ERR_INVALID;
  return index_entry(x, [&](std::string& msg) -> int {
    if (!x->has_prefixes) return no_prefixes("prefixes fill", &msg);
    if (!x->have_names) {
      msg = "prefixes fill: no plan";
      return S3IMPH_ERR_STATE;
    }
    const uint64_t need = (x->names_total + 7) & ~7ull;
    if (cap < need || (need && !d_out)) {
      msg = "prefixes fill: out needs " + std::to_string(need) + " bytes";
      return S3IMPH_ERR_INVALID;
    }
    if (need == 0) return S3IMPH_OK;
    hipStream_t s = use_device(x->device, stream, x->ctx->own_stream);
    return retry_on_nomem(x->ctx, s, &msg, [&] { return names_fill_locked(x, d_out, s, &msg); });
  });
}

int s3imph_index_lookup_verify_device(s3imph_index* x, const uint8_t* d_blob, const uint64_t* d_offsets, uint64_t nq,
                                      uint64_t* d_pos_out, void* stream) {
  if (!x || (nq && (!d_blob || !d_offsets || !d_pos_out))) return S3IMPH_ERR_INVALID;
  return index_entry(x, [&](std::string& msg) -> int {
    if (!x->has_prefixes) return no_prefixes("lookup verify", &msg);
    if (nq == 0) return S3IMPH_OK;
    if (nq >= (1ull << 39)) {
      msg = "lookup verify: 2^39 keys or more in one batch";
      return S3IMPH_ERR_INVALID;
    }
    const int rc = s3imph_lookup_device(x->ctx, d_blob, d_offsets, nq, x->a.fp, x->a.pos, x->a.n, d_pos_out, stream);
    if (rc != S3IMPH_OK) {
      msg = std::string("lookup verify: ") + s3imph_status_string(rc);
      return rc;
    }
    hipStream_t s = use_device(x->device, stream, x->ctx->own_stream);
    k_lookup_verify<<<(unsigned)((nq + kQT - 1) / kQT), kQT, 0, s>>>(x->pb, x->a.n, d_blob, d_offsets, nq, d_pos_out);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipStreamSynchronize(s));
    return S3IMPH_OK;
  });
}

int s3imph_index_verify_device(s3imph_index* x, uint64_t* n_bad, uint64_t* first_bad, uint64_t* first_got,
                               void* stream) {
  if (!x || !n_bad || !first_bad || !first_got) return S3IMPH_ERR_INVALID;
  *n_bad = 0;
  *first_bad = *first_got = ~0ull;
  return index_entry(x, [&](std::string& msg) -> int {
    if (!x->has_prefixes) return no_prefixes("verify", &msg);
    if (x->a.n == 0) return S3IMPH_OK;
    hipStream_t s = use_device(x->device, stream, x->ctx->own_stream);
    return retry_on_nomem(x->ctx, s, &msg, [&] { return verify_locked(x, n_bad, first_bad, first_got, s); });
  });
}

}  // extern "C"
