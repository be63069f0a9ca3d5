// s3imph_aggregate.hip — the front of the pipeline on the GPU: a byte-sorted object listing
// (keys + sizes) in HBM becomes the prefix rows IndexBuilder.Add consumes, and from there a
// whole index directory (include/s3imph.h section 5d).
//
// Reference (pkg/extsort):
//   aggregator.go:44-76    AddObject: one accumulate("", 0) for the root and one per '/' of
//                          the key (prefix = key[:i+1], depth = ordinal of that '/'), cut at
//                          maxDepth when it is > 0; PrefixStats.Add sums count and bytes
//                          (uint64 +=, wrapping);
//   aggregator.go:138-     Drain: nil for no prefixes, else the rows sorted by prefix bytes;
//   indexbuild.go:154-199  IndexBuilder.Add: the consumer of the rows (prefix, depth, count,
//                          bytes), object_count.u64 / total_bytes.u64 written at :179-184.
//
// GPU formulation.  Keys k[0..m) are byte-sorted.  Per key: s = its number
// of '/', c = the number of '/' inside the longest common prefix with its predecessor
// (c[0] = 0), both capped at maxDepth.  Key i opens the rows of depths c'+1 .. s' — every
// shallower prefix was opened by an earlier key — and in that order the rows are already
// byte-sorted.  The row (i, d) covers the keys [i, e) where e is the first index > i with
// c[e] < d (or m): count = e - i, bytes = Z[e] - Z[i] over the wrapping prefix sum Z of the
// sizes.  One pass over the key bytes computes s, c, the row count and the row bytes of
// each key (with block / superblock minima of c beside it); three scans turn them into row
// bases, row byte bases and Z; the emit is partitioned by output rows and output bytes,
// not by key, so a key of thousands of '/' is spread over as many lanes.
//
// Per-tier columns (include/s3imph.h section 5e; PrefixStats.Add, types.go:200-205).  With one
// tier id per object, TierCounts[t] / TierBytes[t] of the row (i, d) are range sums over the same
// keys [i, e): a tile pass sums counts and bytes per tier over tiles of kTG keys (one wave each),
// one scan turns the 24 columns of tile sums into wrapping prefixes, and the emit — one lane per
// row, adjacent lanes adjacent rows, 24 coalesced column writes — takes the whole tiles of [i, e)
// from the table and walks the two partial tiles (fewer than 2 kTG elements, whatever e - i is).
#include <cstdlib>
#include <cstring>

#include "s3imph_entry.h"
#include "s3imph_keys.h"
#include "s3imph_prim.h"
#include "s3imph_tiers.h"

namespace s3imph {

namespace {

constexpr int kAB = 1024;  // keys per block (one block minimum of c)
constexpr int kAS = 1024;  // blocks per superblock
constexpr int kAT = 256;   // lanes per workgroup of the emit kernels: one row / one blob word each
constexpr uint64_t kMaxRows = 1ull << 30;  // what the MPHF build takes on one GPU
constexpr uint32_t kMaxDepth16 = 65535;    // PrefixRow.Depth is a uint16
constexpr int kNT = S3IMPH_NUM_TIERS;      // tiers
constexpr int kTG = 64;                    // keys per tile of the tier prefix table: one wave
constexpr int kTW = 4;                     // tiles (waves) per workgroup of the tile pass

// What the key pass reports: the smallest unsorted index, the smallest index of a key deeper
// than a uint16 depth, the deepest (capped) depth.
struct AggTop {
  unsigned long long first_unsorted, first_deep;
  unsigned maxd, pad;
};

// Key pass: per key i its '/' count s and the '/' count c inside the common prefix with key
// i - 1, found in one walk over the key's words against its predecessor's; the sortedness
// check k[i-1] <= k[i] falls out of the same comparison.  Writes c[i], rows[i] = s' - c' and
// rbytes[i] = the bytes of those rows (the sum of their lengths), the block minimum of c.
__global__ __launch_bounds__(kAB) void k_agg_keys(const uint8_t* __restrict__ blob,
                                                  const uint64_t* __restrict__ offsets, uint64_t m, uint32_t cap,
                                                  uint32_t* __restrict__ c_out, uint64_t* __restrict__ rows,
                                                  uint64_t* __restrict__ rbytes, uint32_t* __restrict__ bmin,
                                                  AggTop* __restrict__ top) {
  __shared__ uint32_t s_min[kAB / 64];
  __shared__ uint32_t s_max[kAB / 64];
  const uint64_t i = (uint64_t)blockIdx.x * kAB + threadIdx.x;
  const uint64_t end8 = (offsets[m] + 7) & ~7ull;
  uint32_t cmin = 0xffffffffu;  // neutral for the block minimum
  uint32_t sp = 0;
  if (i < m) {
    const uint64_t b0 = offsets[i], len = offsets[i + 1] - b0;
    const bool cmp = i > 0;
    const uint64_t p0 = cmp ? offsets[i - 1] : 0, plen = cmp ? b0 - p0 : 0;
    const uint64_t mm = min(len, plen);  // bytes both keys have
    bool diverged = !cmp;                // the common prefix has ended
    bool full = true;                    // ... and it covers all mm bytes
    bool less = false;                   // k[i] < k[i-1]
    uint32_t s = 0, cc = 0;
    uint64_t rb = 0;
    for (uint64_t k = 0; k < len; k += 8) {
      const uint64_t w = load8(blob, b0 + k, end8);
      const uint64_t z = slash_bits(w, len - k) & 0x8080808080808080ull;
      unsigned nd = 0;  // bytes of this word inside the common prefix
      if (!diverged) {
        if (k >= mm) {
          diverged = true;
        } else {
          const uint64_t pw = load8(blob, p0 + k, end8);
          const uint64_t x = w ^ pw;
          const unsigned avail = (unsigned)min((uint64_t)8, mm - k);
          const unsigned fd = x ? (unsigned)(__builtin_ctzll(x) >> 3) : 8u;
          if (fd < avail) {
            nd = fd;
            diverged = true;
            full = false;
            less = ((w >> (8 * fd)) & 0xff) < ((pw >> (8 * fd)) & 0xff);
          } else {
            nd = avail;
            diverged = avail < 8;
          }
        }
      }
      const uint64_t cm = nd >= 8 ? ~0ull : (1ull << (8 * nd)) - 1;
      const uint32_t inc = (uint32_t)__popcll(z & cm);
      s += inc;
      cc += inc;
      uint64_t zr = z & ~cm;  // the '/' past the common prefix: each opens a row (up to the cap)
      while (zr) {
        const unsigned j = (unsigned)(__builtin_ctzll(zr) >> 3);
        zr &= zr - 1;
        ++s;
        if (s <= cap) rb += k + j + 1;
      }
    }
    if (cmp && full && len < plen) less = true;  // a proper prefix of its predecessor
    sp = min(s, cap);
    const uint32_t cp = min(cc, cap);
    if (less) atomicMin(&top->first_unsorted, (unsigned long long)i);
    if (sp > kMaxDepth16) atomicMin(&top->first_deep, (unsigned long long)i);
    c_out[i] = cc;
    rows[i] = sp - cp;
    rbytes[i] = rb;
    cmin = cc;
  }
  uint32_t mn = cmin, mx = sp;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o));
    mx = max(mx, __shfl_xor(mx, o));
  }
  if (lane_id() == 0) {
    s_min[threadIdx.x >> 6] = mn;
    s_max[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < kAB / 64; ++w) {
      mn = min(mn, s_min[w]);
      mx = max(mx, s_max[w]);
    }
    bmin[blockIdx.x] = mn;
    if (mx) atomicMax(&top->maxd, mx);
  }
}

// Superblock minima of c over the block minima (one workgroup per superblock).
__global__ __launch_bounds__(kAS) void k_agg_super(const uint32_t* __restrict__ bmin, uint64_t nb,
                                                   uint32_t* __restrict__ smin) {
  __shared__ uint32_t s_min[kAS / 64];
  const uint64_t b = (uint64_t)blockIdx.x * kAS + threadIdx.x;
  uint32_t mn = b < nb ? bmin[b] : 0xffffffffu;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mn = min(mn, __shfl_xor(mn, o));
  if (lane_id() == 0) s_min[threadIdx.x >> 6] = mn;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 0; w < kAS / 64; ++w) mn = min(mn, s_min[w]);
    smin[blockIdx.x] = mn;
  }
}

// The emit kernels cut their output into chunks of kAT units (rows, or 8-byte words of the
// blob): the owner (key, or row) of each chunk's first unit, one lane per chunk (chunk_owner).
__global__ __launch_bounds__(kAT) void k_agg_bounds(const uint64_t* __restrict__ U, uint64_t entries, uint64_t step,
                                                    uint64_t first_min, uint64_t nchunks,
                                                    uint64_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * kAT + threadIdx.x;
  if (t < nchunks) out[t] = chunk_owner(U, entries, step, first_min, t);
}

// Emit, by output row: row r > 0 belongs to the key i with rowbase[i] <= r < rowbase[i+1]
// (upper-bound search inside the workgroup's keys, k_agg_bounds) and has depth d = c'[i] + 1 +
// (r - rowbase[i]).  A walk over the key finds its d-th '/' and the bytes of the key's
// earlier rows; the range end e = first index > i with c[e] < d comes from the element ->
// block -> superblock -> back down walk of k_fin_subtree.  Row 0 is the root.  kKeep (a plan with
// tiers): the row's key range goes to rowrange[2r] = i, rowrange[2r + 1] = e for the tier emit.
template <bool kKeep>
__global__ __launch_bounds__(kAT) void k_agg_rows(const uint8_t* __restrict__ blob,
                                                  const uint64_t* __restrict__ koff, uint64_t m, uint32_t cap,
                                                  const uint32_t* __restrict__ c, const uint64_t* __restrict__ rowbase,
                                                  const uint64_t* __restrict__ keybytes,
                                                  const uint64_t* __restrict__ bounds,
                                                  const uint64_t* __restrict__ Z, const uint32_t* __restrict__ bmin,
                                                  const uint32_t* __restrict__ smin, uint64_t nb, uint64_t nsb,
                                                  uint64_t n, uint64_t blob_bytes, uint64_t* __restrict__ offsets,
                                                  uint32_t* __restrict__ depth, uint64_t* __restrict__ ocnt,
                                                  uint64_t* __restrict__ tbytes, uint64_t* __restrict__ rowsrc,
                                                  uint64_t* __restrict__ rowrange) {
  const uint64_t base = (uint64_t)blockIdx.x * kAT;
  if (base >= n) return;
  const uint64_t end = min(n, base + kAT);
  const uint64_t r = base + threadIdx.x;
  if (r == 0) {
    offsets[0] = 0;
    offsets[n] = blob_bytes;
    depth[0] = 0;
    ocnt[0] = m;
    tbytes[0] = Z ? Z[m] : 0;
    rowsrc[0] = 0;
    if (kKeep) {
      rowrange[0] = 0;
      rowrange[1] = m;
    }
  }
  if (end < 2) return;  // the root alone
  // the keys this workgroup's rows come from (rowbase has m + 1 entries, rowbase[0] = 1,
  // rowbase[m] = n): from the key of its first row to the key of the next workgroup's
  const uint64_t k_lo = bounds[blockIdx.x];
  const uint64_t k_hi = blockIdx.x + 1 < gridDim.x ? bounds[blockIdx.x + 1] : m - 1;
  if (r == 0 || r >= end) return;
  const uint64_t i = first_above(rowbase, k_lo + 1, k_hi + 1, r) - 1;
  const uint32_t cp = min(c[i], cap);
  const uint32_t d = cp + (uint32_t)(r - rowbase[i]) + 1;
  // the d-th '/' of key i, and the lengths of the key's rows before this one
  const uint64_t b0 = koff[i], len = koff[i + 1] - b0;
  const uint64_t end8 = (koff[m] + 7) & ~7ull;
  uint64_t acc = 0;
  uint32_t s = 0;
  for (uint64_t k = 0; k < len; k += 8) {
    uint64_t z = slash_bits(load8(blob, b0 + k, end8), len - k) & 0x8080808080808080ull;
    const uint32_t cnt = (uint32_t)__popcll(z);
    if (s + cnt <= cp) {
      s += cnt;
      continue;
    }
    bool hit = false;
    while (z) {
      const unsigned j = (unsigned)(__builtin_ctzll(z) >> 3);
      z &= z - 1;
      ++s;
      if (s == d) {
        hit = true;
        break;
      }
      if (s > cp) acc += k + j + 1;
    }
    if (hit) break;
  }
  offsets[r] = keybytes[i] + acc;
  rowsrc[r] = b0;
  depth[r] = d;
  // e = first index > i with c[e] < d, or m
  auto scan = [&](uint64_t lo, uint64_t hi) -> uint64_t {
    for (uint64_t t = lo; t < hi; ++t)
      if (c[t] < d) return t;
    return hi;
  };
  const uint64_t b = i / kAB;
  const uint64_t bl_end = min(m, (b + 1) * kAB);
  uint64_t e = scan(i + 1, bl_end);
  if (e == bl_end && bl_end < m) {
    const uint64_t sb = b / kAS;
    const uint64_t bend = min(nb, (sb + 1) * kAS);
    uint64_t bb = b + 1;
    while (bb < bend && bmin[bb] >= d) ++bb;
    bool none = false;
    if (bb == bend) {
      uint64_t q = sb + 1;
      while (q < nsb && smin[q] >= d) ++q;
      if (q >= nsb) {
        none = true;
      } else {
        bb = q * kAS;  // smin[q] < d: one of its blocks is below d
        while (bmin[bb] >= d) ++bb;
      }
    }
    e = none ? m : scan(bb * kAB, min(m, (bb + 1) * kAB));
  }
  ocnt[r] = e - i;
  tbytes[r] = Z ? Z[e] - Z[i] : 0;
  if (kKeep) {
    rowrange[2 * r] = i;
    rowrange[2 * r + 1] = e;
  }
}

// Emit, by output bytes (emit_word): each lane assembles one 8-byte word of prefix_blob; the
// source of row r is its key, rowsrc[r], at the same distance from the key's start (rows average
// a few words, so a word mostly takes one or two reads).
__global__ __launch_bounds__(kAT) void k_agg_bytes(const uint8_t* __restrict__ blob, uint64_t key_end8,
                                                   const uint64_t* __restrict__ offsets,
                                                   const uint64_t* __restrict__ rowsrc,
                                                   const uint64_t* __restrict__ bounds, uint64_t n,
                                                   uint64_t blob_bytes, uint8_t* __restrict__ out) {
  emit_word<kAT>(blob, key_end8, offsets, bounds, n, blob_bytes, out, [&](uint64_t r) { return rowsrc[r]; });
}

// ---- the per-tier columns ----------------------------------------------------------------
// What the tier pass reports: the smallest index of a tier id >= kNT, the objects of each tier.
struct TierTop {
  unsigned long long first_bad;
  unsigned long long total[kNT];
};

// Tile pass: one wave per tile of kTG keys.  S is the prefix table before its scan, 2 kNT columns
// of ntp = tiles + 1 entries: column t the tile's objects of tier t, column kNT + t the sum of
// their sizes; entry `tiles` of every column is the zero the exclusive scan turns into the
// column's total.  Counts are ballots; a byte sum is a wave reduction, skipped (uniformly) for
// a tier the tile does not hold — a listing's neighbours mostly share their storage class.
__global__ __launch_bounds__(kTG* kTW) void k_agg_tier_tiles(const uint8_t* __restrict__ tiers,
                                                             const uint64_t* __restrict__ sizes, uint64_t m,
                                                             uint64_t tiles, uint64_t* __restrict__ S,
                                                             TierTop* __restrict__ top) {
  const uint64_t tile = (uint64_t)blockIdx.x * kTW + (threadIdx.x >> 6);
  if (tile >= tiles) return;  // whole waves leave; nothing below waits on another wave
  const uint64_t ntp = tiles + 1;
  const unsigned lane = lane_id();
  const uint64_t j = tile * kTG + lane;
  const bool valid = j < m;
  const unsigned t = valid ? tiers[j] : 0xffu;
  const uint64_t z = valid && sizes ? sizes[j] : 0;
  const uint64_t bad = __ballot(valid && t >= (unsigned)kNT);
  if (bad && lane == (unsigned)__builtin_ctzll(bad)) atomicMin(&top->first_bad, (unsigned long long)j);
#pragma unroll
  for (int tt = 0; tt < kNT; ++tt) {
    const bool mine = t == (unsigned)tt;  // false for the lanes past m (0xff)
    const uint64_t bal = __ballot(mine);
    uint64_t v = 0;
    if (bal && sizes) {
      v = mine ? z : 0;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor((unsigned long long)v, o);
    }
    if (lane == 0) {
      S[(uint64_t)tt * ntp + tile] = (uint64_t)__popcll(bal);
      S[(uint64_t)(kNT + tt) * ntp + tile] = v;
    }
  }
  if (tile == tiles - 1 && lane < 2 * kNT) S[(uint64_t)lane * ntp + tiles] = 0;
}

// After the scan: the objects of each tier (its column's last entry less its first; the scan
// runs through all columns, so a column starts at the sum of the ones before it).
__global__ void k_agg_tier_totals(const uint64_t* __restrict__ T, uint64_t ntp, TierTop* __restrict__ top) {
  const unsigned t = threadIdx.x;
  if (t < (unsigned)kNT) top->total[t] = T[(uint64_t)t * ntp + ntp - 1] - T[(uint64_t)t * ntp];
}

// Emit: one lane per row, adjacent lanes adjacent rows, so each of the 24 column writes is
// coalesced.  The row covers the keys [i, e): its whole tiles come from the prefix table T
// (differences inside one column, so the column's starting value cancels mod 2^64), the partial
// tiles at both ends are walked — fewer than 2 kTG elements for any e - i, and e - i itself for a
// row inside one tile.  An element's tier is matched against all kNT accumulators with selects
// (registers, no dynamic indexing); the columns of absent tiers come out as the zeros they are.
__global__ __launch_bounds__(kAT) void k_agg_tier_emit(const uint8_t* __restrict__ tiers,
                                                       const uint64_t* __restrict__ sizes,
                                                       const uint64_t* __restrict__ T, uint64_t ntp,
                                                       const uint64_t* __restrict__ rowrange, uint64_t n,
                                                       uint64_t n_cap, uint64_t* __restrict__ cnt_out,
                                                       uint64_t* __restrict__ bytes_out) {
  const uint64_t r = (uint64_t)blockIdx.x * kAT + threadIdx.x;
  if (r >= n) return;
  const uint64_t i = rowrange[2 * r], e = rowrange[2 * r + 1];
  uint32_t c[kNT];  // walked objects per tier: fewer than 2 kTG
  uint64_t b[kNT];
#pragma unroll
  for (int t = 0; t < kNT; ++t) {
    c[t] = 0;
    b[t] = 0;
  }
  auto walk = [&](uint64_t lo, uint64_t hi) {
    for (uint64_t j = lo; j < hi; ++j) {
      const unsigned tj = tiers[j];
      const uint64_t z = sizes ? sizes[j] : 0;
#pragma unroll
      for (int t = 0; t < kNT; ++t) {
        const bool mine = tj == (unsigned)t;
        c[t] += mine ? 1u : 0u;
        b[t] += mine ? z : 0;
      }
    }
  };
  const uint64_t ti = i / kTG, te = e / kTG;  // te <= tiles = ntp - 1
  const bool whole = ti != te;                // the row has whole tiles (or at least a tile edge) inside
  if (!whole) {
    walk(i, e);
  } else {
    walk(i, (ti + 1) * kTG);
    walk(te * kTG, e);
  }
#pragma unroll
  for (int t = 0; t < kNT; ++t) {
    uint64_t cc = c[t], bb = b[t];
    if (whole) {
      const uint64_t* Tc = T + (uint64_t)t * ntp;
      const uint64_t* Tb = T + (uint64_t)(kNT + t) * ntp;
      cc += Tc[te] - Tc[ti + 1];
      bb += Tb[te] - Tb[ti + 1];
    }
    cnt_out[(uint64_t)t * n_cap + r] = cc;
    bytes_out[(uint64_t)t * n_cap + r] = bb;
  }
}

}  // namespace

// Scratch of the aggregation and the last plan, kept in the context and grown as needed.
struct AggScratch {
  uint32_t* c = nullptr;
  uint64_t *rowbase = nullptr, *keybytes = nullptr, *Z = nullptr;
  uint32_t *bmin = nullptr, *smin = nullptr;
  AggTop* top = nullptr;
  uint64_t cap = 0;  // keys
  uint64_t* rowsrc = nullptr;
  uint64_t rows_cap = 0;
  uint64_t* bounds = nullptr;  // the emit chunks' first owners (k_agg_bounds)
  uint64_t bounds_cap = 0;
  PrimTmp tmp;
  // the tier columns: the prefix table (2 kNT columns of tiles + 1 entries), what the tile pass
  // reports, each row's key range [i, e) (kept by the fill of a plan with tiers)
  uint64_t* ttab = nullptr;
  uint64_t ttab_cap = 0;
  TierTop* ttop = nullptr;
  uint64_t* rowrange = nullptr;
  uint64_t range_cap = 0;
  // the last plan
  bool have_plan = false, sized = false;
  bool tiered = false, ranges_kept = false;  // planned with tiers; its fill has run
  const uint8_t* tiers = nullptr;
  const uint64_t* sizes = nullptr;
  uint64_t present_mask = 0;
  const uint8_t* keys = nullptr;
  const uint64_t* koff = nullptr;
  uint64_t m = 0, n = 0, blob_bytes = 0, key_end8 = 0;
  uint32_t depth_cap = 0;
  void release() {
    dfree(c);
    dfree(rowbase);
    dfree(keybytes);
    dfree(Z);
    dfree(bmin);
    dfree(smin);
    dfree(top);
    dfree(rowsrc);
    dfree(bounds);
    tmp.release();
    dfree(ttab);
    dfree(ttop);
    dfree(rowrange);
    cap = rows_cap = bounds_cap = ttab_cap = range_cap = 0;
    have_plan = false;
  }
};

void agg_scratch_free(s3imph_ctx* c) {
  if (c->agg) {
    c->agg->release();
    delete c->agg;
    c->agg = nullptr;
  }
}

// Plan: the key pass and the scans for m keys in HBM; fills *info, keeps the plan in the
// context.  Waits for the stream.
int aggregate_plan(s3imph_ctx* c, const uint8_t* keys, const uint64_t* koff, const uint64_t* sizes, uint64_t m,
                   uint32_t max_depth, s3imph_agg_info* info, hipStream_t s, std::string* msg) {
  std::memset(info, 0, sizeof *info);
  info->first_unsorted = UINT64_MAX;
  info->n_objects = m;
  if (!c->agg) c->agg = new AggScratch();
  AggScratch& a = *c->agg;
  a.have_plan = false;
  a.tiered = a.ranges_kept = false;
  if (m == 0) {
    a.keys = nullptr;
    a.koff = nullptr;
    a.m = a.n = a.blob_bytes = 0;
    a.have_plan = true;
    return S3IMPH_OK;
  }
  const uint64_t nb = (m + kAB - 1) / kAB, nsb = (nb + kAS - 1) / kAS;
  if (m > a.cap) {
    a.release();
    dalloc(a.c, m);
    dalloc(a.rowbase, m + 1);
    dalloc(a.keybytes, m + 1);
    dalloc(a.Z, m + 1);
    dalloc(a.bmin, nb);
    dalloc(a.smin, nsb);
    dalloc(a.top, 1);
    a.cap = m;
  }
  const uint32_t cap = max_depth ? max_depth : 0xffffffffu;
  const AggTop top0{~0ull, ~0ull, 0, 0};
  AggTop top = top0;
  HIPCHECK(hipMemcpyAsync(a.top, &top0, sizeof top0, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemsetAsync(a.rowbase + m, 0, 8, s));
  HIPCHECK(hipMemsetAsync(a.keybytes + m, 0, 8, s));
  k_agg_keys<<<(unsigned)nb, kAB, 0, s>>>(keys, koff, m, cap, a.c, a.rowbase, a.keybytes, a.bmin, a.top);
  k_agg_super<<<(unsigned)nsb, kAS, 0, s>>>(a.bmin, nb, a.smin);
  HIPCHECK(hipGetLastError());
  scan_u64(a.tmp, a.rowbase, m + 1, 1, s);  // + 1: the root row
  scan_u64(a.tmp, a.keybytes, m + 1, 0, s);
  a.sized = sizes != nullptr;
  uint64_t tot[4] = {0, 0, 0, 0};  // rows, row bytes, size sum, end of the key blob
  if (sizes) {
    HIPCHECK(hipMemcpyAsync(a.Z, sizes, m * 8, hipMemcpyDeviceToDevice, s));
    HIPCHECK(hipMemsetAsync(a.Z + m, 0, 8, s));
    scan_u64(a.tmp, a.Z, m + 1, 0, s);
    HIPCHECK(hipMemcpyAsync(&tot[2], a.Z + m, 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHECK(hipMemcpyAsync(&top, a.top, sizeof top, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&tot[3], koff + m, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&tot[0], a.rowbase + m, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&tot[1], a.keybytes + m, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  info->n_prefixes = tot[0];
  info->blob_bytes = tot[1];
  info->total_bytes = tot[2];
  info->max_depth_seen = top.maxd;
  info->first_unsorted = top.first_unsorted;
  if (top.first_unsorted != ~0ull) {
    *msg = "aggregate: object keys are not byte-sorted: key " + std::to_string(top.first_unsorted) +
           " is smaller than key " + std::to_string(top.first_unsorted - 1);
    return S3IMPH_ERR_INVALID;
  }
  if (top.first_deep != ~0ull) {
    *msg = "aggregate: key " + std::to_string(top.first_deep) + " has more than 65535 '/' (the depth is a uint16)";
    return S3IMPH_ERR_INVALID;
  }
  if (tot[0] > kMaxRows) {
    *msg = "aggregate: more than 2^30 prefixes on one GPU (the MPHF's level 0 past 2^31 positions): "
           "shard them over several GPUs";
    return S3IMPH_ERR_INVALID;
  }
  a.keys = keys;
  a.koff = koff;
  a.m = m;
  a.n = tot[0];
  a.blob_bytes = tot[1];
  a.key_end8 = (tot[3] + 7) & ~7ull;
  a.depth_cap = cap;
  a.have_plan = true;
  return S3IMPH_OK;
}

// Fill: the rows of the last plan.  Waits for the stream.
int aggregate_fill(s3imph_ctx* c, uint8_t* blob, uint64_t blob_cap, uint64_t* offsets, uint32_t* depth,
                   uint64_t* ocnt, uint64_t* tbytes, uint64_t n_cap, hipStream_t s, std::string* msg) {
  if (!c->agg || !c->agg->have_plan) {
    *msg = "aggregate: fill without a plan";
    return S3IMPH_ERR_STATE;
  }
  AggScratch& a = *c->agg;
  if (n_cap < a.n || blob_cap < ((a.blob_bytes + 7) & ~7ull)) {
    *msg = "aggregate: the plan needs " + std::to_string(a.n) + " rows and " +
           std::to_string((a.blob_bytes + 7) & ~7ull) + " blob bytes";
    return S3IMPH_ERR_INVALID;
  }
  if (!offsets || (a.n && (!depth || !ocnt || !tbytes)) || (a.blob_bytes && !blob)) {
    *msg = "aggregate: null output array";
    return S3IMPH_ERR_INVALID;
  }
  if (a.n == 0) {
    HIPCHECK(hipMemsetAsync(offsets, 0, 8, s));
    HIPCHECK(hipStreamSynchronize(s));
    a.ranges_kept = a.tiered;
    return S3IMPH_OK;
  }
  grow(a.rowsrc, a.rows_cap, a.n);
  const uint64_t nb = (a.m + kAB - 1) / kAB, nsb = (nb + kAS - 1) / kAS;
  const uint64_t nw = (a.blob_bytes + 7) / 8;
  const uint64_t rchunks = (a.n + kAT - 1) / kAT, wchunks = (nw + kAT - 1) / kAT;
  grow(a.bounds, a.bounds_cap, std::max(rchunks, wchunks));
  k_agg_bounds<<<(unsigned)((rchunks + kAT - 1) / kAT), kAT, 0, s>>>(a.rowbase, a.m + 1, kAT, 1, rchunks, a.bounds);
  if (a.tiered) {
    grow(a.rowrange, a.range_cap, 2 * a.n);
    k_agg_rows<true><<<(unsigned)rchunks, kAT, 0, s>>>(a.keys, a.koff, a.m, a.depth_cap, a.c, a.rowbase, a.keybytes,
                                                       a.bounds, a.sized ? a.Z : nullptr, a.bmin, a.smin, nb, nsb, a.n,
                                                       a.blob_bytes, offsets, depth, ocnt, tbytes, a.rowsrc,
                                                       a.rowrange);
  } else {
    k_agg_rows<false><<<(unsigned)rchunks, kAT, 0, s>>>(a.keys, a.koff, a.m, a.depth_cap, a.c, a.rowbase, a.keybytes,
                                                        a.bounds, a.sized ? a.Z : nullptr, a.bmin, a.smin, nb, nsb, a.n,
                                                        a.blob_bytes, offsets, depth, ocnt, tbytes, a.rowsrc, nullptr);
  }
  if (nw) {
    k_agg_bounds<<<(unsigned)((wchunks + kAT - 1) / kAT), kAT, 0, s>>>(offsets, a.n + 1, 8ull * kAT, 0, wchunks,
                                                                      a.bounds);
    k_agg_bytes<<<(unsigned)wchunks, kAT, 0, s>>>(a.keys, a.key_end8, offsets, a.rowsrc, a.bounds, a.n, a.blob_bytes,
                                                  blob);
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));
  a.ranges_kept = a.tiered;
  return S3IMPH_OK;
}

// Plan with tiers: the plain plan, then the tile pass over (tiers, sizes) and the scan of its
// table; fills *tinfo.  Waits for the stream.
int aggregate_plan_tiers(s3imph_ctx* c, const uint8_t* keys, const uint64_t* koff, const uint64_t* sizes,
                         const uint8_t* tiers, uint64_t m, uint32_t max_depth, s3imph_agg_info* info,
                         s3imph_agg_tier_info* tinfo, hipStream_t s, std::string* msg) {
  tinfo->present_mask = 0;
  tinfo->first_bad_tier = UINT64_MAX;
  const int rc = aggregate_plan(c, keys, koff, sizes, m, max_depth, info, s, msg);
  if (rc != S3IMPH_OK) return rc;
  AggScratch& a = *c->agg;
  a.have_plan = false;  // until the tiers are known to be good
  a.tiers = tiers;
  a.sizes = sizes;
  a.present_mask = 0;
  if (m) {
    const uint64_t tiles = (m + kTG - 1) / kTG, ntp = tiles + 1;
    grow(a.ttab, a.ttab_cap, 2 * kNT * ntp);
    if (!a.ttop) dalloc(a.ttop, 1);
    TierTop top;
    std::memset(&top, 0, sizeof top);
    top.first_bad = ~0ull;
    HIPCHECK(hipMemcpyAsync(a.ttop, &top, sizeof top, hipMemcpyHostToDevice, s));
    k_agg_tier_tiles<<<(unsigned)((tiles + kTW - 1) / kTW), kTG * kTW, 0, s>>>(tiers, sizes, m, tiles, a.ttab, a.ttop);
    HIPCHECK(hipGetLastError());
    scan_u64(a.tmp, a.ttab, 2 * kNT * ntp, 0, s);
    k_agg_tier_totals<<<1, 64, 0, s>>>(a.ttab, ntp, a.ttop);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipMemcpyAsync(&top, a.ttop, sizeof top, hipMemcpyDeviceToHost, s));
    HIPCHECK(hipStreamSynchronize(s));
    tinfo->first_bad_tier = top.first_bad;
    if (top.first_bad != ~0ull) {
      *msg = "aggregate: object " + std::to_string(top.first_bad) + " has a tier id of " +
             std::to_string(S3IMPH_NUM_TIERS) + " or more";
      return S3IMPH_ERR_INVALID;
    }
    for (int t = 0; t < kNT; ++t)
      if (top.total[t]) a.present_mask |= 1ull << t;
  }
  tinfo->present_mask = a.present_mask;
  a.tiered = true;
  a.have_plan = true;
  return S3IMPH_OK;
}

// The tier columns of the last plan's rows (after its fill).  Waits for the stream.
int aggregate_fill_tiers(s3imph_ctx* c, uint64_t* tcount, uint64_t* tbytes, uint64_t n_cap, hipStream_t s,
                         std::string* msg) {
  if (!c->agg || !c->agg->have_plan || !c->agg->tiered) {
    *msg = "aggregate: tier fill without a plan that had tiers";
    return S3IMPH_ERR_STATE;
  }
  AggScratch& a = *c->agg;
  if (!a.ranges_kept) {
    *msg = "aggregate: tier fill before the fill of the rows";
    return S3IMPH_ERR_STATE;
  }
  if (n_cap < a.n) {
    *msg = "aggregate: the plan needs " + std::to_string(a.n) + " rows per tier column";
    return S3IMPH_ERR_INVALID;
  }
  if (a.n == 0) return S3IMPH_OK;
  if (!tcount || !tbytes) {
    *msg = "aggregate: null output array";
    return S3IMPH_ERR_INVALID;
  }
  const uint64_t tiles = (a.m + kTG - 1) / kTG;
  k_agg_tier_emit<<<(unsigned)((a.n + kAT - 1) / kAT), kAT, 0, s>>>(a.tiers, a.sizes, a.ttab, tiles + 1, a.rowrange, a.n,
                                                                   n_cap, tcount, tbytes);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));
  return S3IMPH_OK;
}

bool listing_given(const uint8_t* keys, const uint64_t* koff, uint64_t m) {
  return m == 0 || (koff && (keys || koff[m] == koff[0]));
}

void upload_keys(s3imph_ctx* c, DevGuard& g, const uint8_t* keys, const uint64_t* koff, uint64_t m,
                    uint8_t*& d_keys, uint64_t*& d_koff) {
  const uint64_t b0 = koff[0], nbytes = koff[m] - b0;
  g.make(d_keys, ((nbytes + 7) & ~7ull) + 16);
  g.make(d_koff, m + 1);
  if (nbytes) HIPCHECK(hipMemcpy(d_keys, keys + b0, nbytes, hipMemcpyHostToDevice));
  staged_copy(c, true, d_koff, koff, (m + 1) * 8, b0);
}

namespace {

// The listing's device copy put into byte order (s3imph_sort.hip): sort, gather out of place,
// free the unsorted copy.  A listing found sorted stays as it is.
int sort_listing(s3imph_ctx* c, DevGuard& g, uint8_t*& d_keys, uint64_t*& d_koff, uint64_t*& d_sizes,
                 uint8_t*& d_tiers, uint64_t m, hipStream_t s, std::string* msg) {
  try {
    uint32_t* d_order = nullptr;
    g.make(d_order, m);
    s3imph_sort_info si;
    int rc = sort_objects(c, d_keys, d_koff, m, d_order, &si, s, msg);
    if (rc == S3IMPH_OK && si.first_unsorted != UINT64_MAX) {
      uint8_t *keys2 = nullptr, *tiers2 = nullptr;
      uint64_t *koff2 = nullptr, *sizes2 = nullptr;
      const uint64_t cap = (si.key_bytes + 7) & ~7ull;
      g.make(keys2, cap + 16);
      g.make(koff2, m + 1);
      if (d_sizes) g.make(sizes2, m);
      if (d_tiers) g.make(tiers2, m);
      rc = gather_objects(c, d_keys, d_koff, d_sizes, d_tiers, m, d_order, keys2, cap, koff2, sizes2, tiers2, s, msg);
      g.drop(d_keys);
      g.drop(d_koff);
      g.drop(d_sizes);
      g.drop(d_tiers);
      d_keys = keys2;
      d_koff = koff2;
      d_sizes = sizes2;
      d_tiers = tiers2;
    }
    g.drop(d_order);
    return rc;
  } catch (const Fail& f) {
    throw Fail{f.code, "sort: " + f.msg};
  }
}

}  // namespace

// H2D of the listing, plan, fill (with `tiers`: the tier forms and the tier columns too; with
// `unsorted`: the sort and the gather first); the listing's device copy is freed before returning.
// With `csv` the listing comes from CSV buffers parsed on the device (s3imph_csv.hip), always in
// file order, so sorted here; `tiers` then only says whether tiers are wanted.  No object at all:
// out->m == 0 and no rows.
int rows_from_host(s3imph_ctx* c, DevGuard& g, const uint8_t* keys, const uint64_t* koff, const uint64_t* sizes,
                   uint64_t m, uint32_t max_depth, DevRows* out, std::string* msg, const uint8_t* tiers, bool unsorted,
                   const CsvFiles* csv) {
  hipStream_t s = c->own_stream;
  uint8_t *d_keys = nullptr, *d_tiers = nullptr;
  uint64_t *d_koff = nullptr, *d_sizes = nullptr;
  if (csv) {
    try {
      const int rc0 = csv_listing(c, g, *csv, d_keys, d_koff, d_sizes, d_tiers, &m, s, msg);
      if (rc0 != S3IMPH_OK) return rc0;
    } catch (const Fail& f) {
      throw Fail{f.code, "csv: " + f.msg};
    }
    out->m = m;
    if (m == 0) return S3IMPH_OK;
    const int rc0 = sort_listing(c, g, d_keys, d_koff, d_sizes, d_tiers, m, s, msg);
    if (rc0 != S3IMPH_OK) return rc0;
  } else if (m) {
    out->m = m;
    upload_keys(c, g, keys, koff, m, d_keys, d_koff);
    if (sizes) {
      g.make(d_sizes, m);
      staged_copy(c, true, d_sizes, sizes, m * 8);
    }
    if (tiers) {
      g.make(d_tiers, m);
      HIPCHECK(hipMemcpy(d_tiers, tiers, m, hipMemcpyHostToDevice));
    }
    if (unsorted) {
      const int rc0 = sort_listing(c, g, d_keys, d_koff, d_sizes, d_tiers, m, s, msg);
      if (rc0 != S3IMPH_OK) return rc0;
    }
  }
  s3imph_agg_info info;
  s3imph_agg_tier_info tinfo;
  int rc = tiers ? aggregate_plan_tiers(c, d_keys, d_koff, d_sizes, d_tiers, m, max_depth, &info, &tinfo, s, msg)
                 : aggregate_plan(c, d_keys, d_koff, d_sizes, m, max_depth, &info, s, msg);
  if (rc != S3IMPH_OK) return rc;
  out->n = info.n_prefixes;
  out->blob_bytes = info.blob_bytes;
  g.make(out->blob, ((info.blob_bytes + 7) & ~7ull) + 16);
  g.make(out->offsets, out->n + 1);
  g.make(out->depth, out->n);
  g.make(out->ocnt, out->n);
  g.make(out->tbytes, out->n);
  rc = aggregate_fill(c, out->blob, (info.blob_bytes + 7) & ~7ull, out->offsets, out->depth, out->ocnt, out->tbytes,
                      out->n, s, msg);
  if (rc == S3IMPH_OK && tiers) {
    out->present_mask = tinfo.present_mask;
    g.make(out->tier_count, kNT * out->n);
    g.make(out->tier_bytes, kNT * out->n);
    rc = aggregate_fill_tiers(c, out->tier_count, out->tier_bytes, out->n, s, msg);
  }
  c->agg->have_plan = false;  // the listing's copy goes away with this call
  g.drop(d_keys);
  g.drop(d_koff);
  g.drop(d_sizes);
  g.drop(d_tiers);
  return rc;
}

}  // namespace s3imph

using namespace s3imph;

extern "C" {

int s3imph_aggregate_plan_tiers_device(s3imph_ctx* c, const uint8_t* d_keys, const uint64_t* d_key_offsets,
                                       const uint64_t* d_sizes, const uint8_t* d_tiers, uint64_t m,
                                       uint32_t max_depth, s3imph_agg_info* info, s3imph_agg_tier_info* tier_info,
                                       void* stream) {
  if (!c || !info || !tier_info || (m && (!d_keys || !d_key_offsets || !d_tiers))) return S3IMPH_ERR_INVALID;
  return device_entry(c, "", [&](std::string& msg) {
    hipStream_t s = use_device(c->device, stream, c->own_stream);
    return retry_on_nomem(c, s, &msg, [&] {
      return aggregate_plan_tiers(c, d_keys, d_key_offsets, d_sizes, d_tiers, m, max_depth, info, tier_info, s, &msg);
    });
  });
}

int s3imph_aggregate_fill_tiers_device(s3imph_ctx* c, uint64_t* d_tier_count, uint64_t* d_tier_bytes, uint64_t n_cap,
                                       void* stream) {
  if (!c) return S3IMPH_ERR_INVALID;
  return device_entry(c, "", [&](std::string& msg) {
    hipStream_t s = use_device(c->device, stream, c->own_stream);
    return aggregate_fill_tiers(c, d_tier_count, d_tier_bytes, n_cap, s, &msg);
  });
}

int s3imph_aggregate_plan_device(s3imph_ctx* c, const uint8_t* d_keys, const uint64_t* d_key_offsets,
                                 const uint64_t* d_sizes, uint64_t m, uint32_t max_depth, s3imph_agg_info* info,
                                 void* stream) {
  if (!c || !info || (m && (!d_keys || !d_key_offsets))) return S3IMPH_ERR_INVALID;
  return device_entry(c, "", [&](std::string& msg) {
    hipStream_t s = use_device(c->device, stream, c->own_stream);
    return retry_on_nomem(c, s, &msg, [&] {
      return aggregate_plan(c, d_keys, d_key_offsets, d_sizes, m, max_depth, info, s, &msg);
    });
  });
}

int s3imph_aggregate_fill_device(s3imph_ctx* c, uint8_t* d_blob, uint64_t blob_cap, uint64_t* d_offsets,
                                 uint32_t* d_depth, uint64_t* d_object_count, uint64_t* d_total_bytes,
                                 uint64_t n_cap, void* stream) {
  if (!c) return S3IMPH_ERR_INVALID;
  return device_entry(c, "", [&](std::string& msg) {
    hipStream_t s = use_device(c->device, stream, c->own_stream);
    return aggregate_fill(c, d_blob, blob_cap, d_offsets, d_depth, d_object_count, d_total_bytes, n_cap, s, &msg);
  });
}

// s3imph_aggregate_host, and with `tiers` s3imph_aggregate_tiers_host (tier_count, tier_bytes and
// present_mask are then given).
static int aggregate_host_impl(int device, const uint8_t* keys, const uint64_t* key_offsets, const uint64_t* sizes,
                               const uint8_t* tiers, uint64_t m, uint32_t max_depth, uint8_t** blob,
                               uint64_t** offsets, uint32_t** depth, uint64_t** object_count, uint64_t** total_bytes,
                               uint64_t** tier_count, uint64_t** tier_bytes, uint64_t* present_mask, uint64_t* n,
                               char* err, size_t errlen) {
  if (!blob || !offsets || !depth || !object_count || !total_bytes || !n || !listing_given(keys, key_offsets, m))
    return S3IMPH_ERR_INVALID;
  HostRows out(blob, offsets, depth, object_count, total_bytes, tiers ? tier_count : nullptr,
               tiers ? tier_bytes : nullptr, tiers ? present_mask : nullptr, n);
  out.reset();
  if (m == 0)  // Drain returns nil
    return host_call("aggregate: ", err, errlen, [&](std::string&) { return out.none(); });
  const int rc = host_entry(device, "aggregate: ", err, errlen, [&](s3imph_ctx* c, hipStream_t, std::string& msg) {
    DevGuard g;
    DevRows r;
    const int rc2 = rows_from_host(c, g, keys, key_offsets, sizes, m, max_depth, &r, &msg, tiers);
    if (rc2 == S3IMPH_OK) out.download(c, r, tiers != nullptr);
    return rc2;
  });
  if (rc != S3IMPH_OK) out.drop();
  return rc;
}

int s3imph_aggregate_host(int device, const uint8_t* keys, const uint64_t* key_offsets, const uint64_t* sizes,
                          uint64_t m, uint32_t max_depth, uint8_t** blob, uint64_t** offsets, uint32_t** depth,
                          uint64_t** object_count, uint64_t** total_bytes, uint64_t* n, char* err, size_t errlen) {
  return aggregate_host_impl(device, keys, key_offsets, sizes, nullptr, m, max_depth, blob, offsets, depth,
                             object_count, total_bytes, nullptr, nullptr, nullptr, n, err, errlen);
}

int s3imph_aggregate_tiers_host(int device, const uint8_t* keys, const uint64_t* key_offsets, const uint64_t* sizes,
                                const uint8_t* tiers, uint64_t m, uint32_t max_depth, uint8_t** blob,
                                uint64_t** offsets, uint32_t** depth, uint64_t** object_count, uint64_t** total_bytes,
                                uint64_t** tier_count, uint64_t** tier_bytes, uint64_t* present_mask, uint64_t* n,
                                char* err, size_t errlen) {
  static const uint8_t kNone = 0;
  if (!tier_count || !tier_bytes || !present_mask || (m && !tiers)) return S3IMPH_ERR_INVALID;
  return aggregate_host_impl(device, keys, key_offsets, sizes, tiers ? tiers : &kNone, m, max_depth, blob, offsets,
                             depth, object_count, total_bytes, tier_count, tier_bytes, present_mask, n, err, errlen);
}

}  // extern "C"

// Rows in HBM -> every array of the index directory on the host: the MPHF build over the rows'
// blob, the finalize with their depths, the D2H.  The rows stay in HBM throughout.
int s3imph::index_arrays_from_rows(s3imph_ctx* c, DevGuard& g, DevRows& r, bool tiers, IndexHostArrays& h,
                                   hipStream_t s, std::string* pmsg) {
  std::string& msg = *pmsg;
  const uint64_t n = h.n = r.n;
  int rc2;
  if (tiers) {  // the columns of the present tiers leave HBM before the build needs the room
    h.present_mask = r.present_mask;
    h.tcount.resize(kNT * n);
    h.tcbytes.resize(kNT * n);
    for (int t = 0; t < kNT; ++t) {
      if (!((h.present_mask >> t) & 1)) continue;
      staged_copy(c, false, h.tcount.data() + t * n, r.tier_count + t * n, n * 8);
      staged_copy(c, false, h.tcbytes.data() + t * n, r.tier_bytes + t * n, n * 8);
    }
    g.drop(r.tier_count);
    g.drop(r.tier_bytes);
  }
  uint64_t *d_fp = nullptr, *d_pos = nullptr, *d_send = nullptr, *d_dpos = nullptr, *d_doff = nullptr;
  uint32_t *d_depth = nullptr, *d_maxds = nullptr;
  g.make(d_fp, n);
  g.make(d_pos, n);
  s3imph_build_info binfo;
  rc2 = build_single(c, r.blob, r.offsets, nullptr, n, d_fp, d_pos, s, &binfo, &msg);
  if (rc2 != S3IMPH_OK) return rc2;
  HIPCHECK(hipStreamSynchronize(s));
  g.make(d_send, n);
  g.make(d_dpos, n);
  g.make(d_depth, n);
  g.make(d_maxds, n);
  rc2 = finalize_rows(c, g, r.blob, r.offsets, r.depth, n, d_depth, d_send, d_maxds, d_dpos, d_doff, &h.md, s, &msg);
  if (rc2 != S3IMPH_OK) return rc2;
  HIPCHECK(hipStreamSynchronize(s));
  uint64_t mlen = 0;
  h.mph.resize(binfo.mph_bin_len);
  rc2 = marshal_locked(c, h.mph.data(), h.mph.size(), &mlen, &msg);
  if (rc2 != S3IMPH_OK) return rc2;
  h.mph.resize(mlen);
  h.blob.resize(r.blob_bytes);
  h.offs.resize(n + 1);
  h.doff.resize((uint64_t)h.md + 2);
  for (auto* v : {&h.fp, &h.pos, &h.send, &h.dpos, &h.ocnt, &h.tbytes}) v->resize(n);
  h.depth.resize(n);
  h.maxds.resize(n);
  if (r.blob_bytes) HIPCHECK(hipMemcpy(h.blob.data(), r.blob, r.blob_bytes, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(h.doff.data(), d_doff, h.doff.size() * 8, hipMemcpyDeviceToHost));
  staged_copy(c, false, h.offs.data(), r.offsets, (n + 1) * 8);
  staged_copy(c, false, h.fp.data(), d_fp, n * 8);
  staged_copy(c, false, h.pos.data(), d_pos, n * 8);
  staged_copy(c, false, h.send.data(), d_send, n * 8);
  staged_copy(c, false, h.dpos.data(), d_dpos, n * 8);
  staged_copy(c, false, h.ocnt.data(), r.ocnt, n * 8);
  staged_copy(c, false, h.tbytes.data(), r.tbytes, n * 8);
  staged_copy(c, false, h.depth.data(), d_depth, n * 4);
  staged_copy(c, false, h.maxds.data(), d_maxds, n * 4);
  return S3IMPH_OK;
}

// The directory's files from the host arrays (n == 0: the empty index s3imph_index_open accepts).
int s3imph::write_index_dir(const std::string& dir, IndexHostArrays& h, bool tiers, std::string* msg) {
  const uint64_t n = h.n;
  if (n == 0) {
    h.offs = {0};
    h.doff = {0, 0};  // writeEmpty-like: maxDepth 0 -> offsets [0, 0]
  }
  int rc = write_index_files(dir, h.mph.data(), h.mph.size(), h.fp.data(), h.pos.data(), n, h.blob.data(),
                             h.offs.data(), msg);
  if (rc == S3IMPH_OK)
    rc = write_finalize_files(dir, h.depth.data(), h.send.data(), h.maxds.data(), h.doff.data(), h.doff.size(),
                              h.dpos.data(), n, msg);
  if (rc == S3IMPH_OK) rc = write_stats_files(dir, h.ocnt.data(), h.tbytes.data(), n, msg);
  if (rc == S3IMPH_OK && tiers)
    rc = write_tier_files(dir, h.present_mask, h.tcount.data(), h.tcbytes.data(), n, n, msg);
  if (rc == S3IMPH_OK) rc = write_manifest(dir, n, h.md, msg);
  return rc;
}

// s3imph_index_from_objects_host, with `tiers` s3imph_index_from_objects_tiers_host, and with
// `unsorted` s3imph_index_from_unsorted_objects_host (s3imph_sort.hip).
int s3imph::index_from_objects(int device, const uint8_t* keys, const uint64_t* key_offsets, const uint64_t* sizes,
                               const uint8_t* tiers, uint64_t m, uint32_t max_depth, const char* out_dir,
                               bool unsorted, char* err, size_t errlen, const CsvFiles* csv) {
  static const uint8_t kWanted = 0;
  if (csv) {
    keys = nullptr, key_offsets = sizes = nullptr, m = 0;
    tiers = csv->with_tiers ? &kWanted : nullptr;
  }
  if (!out_dir || !listing_given(keys, key_offsets, m)) return S3IMPH_ERR_INVALID;
  const std::string dir = out_dir;
  if (!is_dir(dir)) {
    set_err(err, errlen, "create mph file: open " + dir + "/mph.bin: no such directory");
    return S3IMPH_ERR_IO;
  }
  const bool with_tiers = tiers != nullptr;
  IndexHostArrays h;
  uint64_t csv_bytes = 0;
  for (uint64_t i = 0; csv && i < csv->n_files; ++i) csv_bytes += csv->len[i];
  if (csv && csv->gz) csv_bytes += csv->n_files;  // a zero-length gzip file is an error the device reports
  if (m || csv_bytes) {
    // one device residency: the rows stay in HBM from the aggregation to the last array
    const int rc = host_entry(
        device, "aggregate: ", err, errlen,
        [&](s3imph_ctx* c, hipStream_t s, std::string& msg) -> int {
          DevGuard g;
          DevRows r;
          const int rc2 = rows_from_host(c, g, keys, key_offsets, sizes, m, max_depth, &r, &msg, tiers, unsorted, csv);
          if (rc2 != S3IMPH_OK) return rc2;
          h.n = r.n;
          if (r.m == 0) return S3IMPH_OK;  // CSV text without an object: the empty index below
          return index_arrays_from_rows(c, g, r, with_tiers, h, s, &msg);
        },
        csv ? "csv: " : nullptr);
    if (rc != S3IMPH_OK) return rc;
  }
  return host_call("aggregate: ", err, errlen,
                   [&](std::string& msg) { return write_index_dir(dir, h, with_tiers, &msg); });
}

extern "C" {

int s3imph_index_from_objects_host(int device, const uint8_t* keys, const uint64_t* key_offsets,
                                   const uint64_t* sizes, uint64_t m, uint32_t max_depth, const char* out_dir,
                                   char* err, size_t errlen) {
  return index_from_objects(device, keys, key_offsets, sizes, nullptr, m, max_depth, out_dir, false, err, errlen);
}

int s3imph_index_from_objects_tiers_host(int device, const uint8_t* keys, const uint64_t* key_offsets,
                                         const uint64_t* sizes, const uint8_t* tiers, uint64_t m, uint32_t max_depth,
                                         const char* out_dir, char* err, size_t errlen) {
  static const uint8_t kNone = 0;
  if (m && !tiers) return S3IMPH_ERR_INVALID;
  return index_from_objects(device, keys, key_offsets, sizes, tiers ? tiers : &kNone, m, max_depth, out_dir, false,
                            err, errlen);
}

}  // extern "C"
