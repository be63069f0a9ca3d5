// s3imph_csv.hip — S3 inventory CSV text in HBM -> the object listing of sections 5d / 5f
// (include/s3imph.h section 5g): what pkg/inventory's CSVReader.Read (reader.go:250-297) and
// csvInventoryReader.Next (unified.go:121-161) return record by record, for a whole buffer at once.
//
// The grammar is encoding/csv's readRecord with Comma = ',', LazyQuotes and no comment character,
// restated as a five-state byte automaton:
//   R record start, F field start after a comma, U in an unquoted field, Q in a quoted field,
//   E in a quoted field just after a '"';
// over the bytes left once every '\r' that stands before a '\n' or at the very end is deleted.
// A state map (the image of all five states) composes associatively, so the state at any byte
// comes from a scan:
//   1. k_csv_maps       one tile of kCsvTile bytes per workgroup, staged into LDS; each lane
//                       walks kCsvRun bytes and makes its run's map; a block scan leaves each
//                       run's map from the tile's start and the tile's whole map;
//      k_csv_tile_scan  one workgroup composes the tile maps: every tile's entry state;
//   2. k_csv_ends       each run, its entry state now known, counts (then, in a second launch,
//                       writes) its record ends;
//   3. k_csv_fields     one lane per record walks it from state R and finds the key (length,
//                       source, whether its bytes stand contiguous in the text), the size, the
//                       tier and whether the reader keeps it; two scans give object numbers and
//                       key offsets;
//   4. k_csv_meta / k_csv_key_words / k_csv_key_rewalk   the fill.
// A record longer than a tile (only an unbalanced quote makes one) is walked by its one lane:
// correct and slow.
#include <cstring>

#include "s3imph_entry.h"
#include "s3imph_keys.h"
#include "s3imph_prim.h"
#include "s3imph_tiers.h"

namespace s3imph {

namespace {

constexpr int kCsvRun = kCsvRunBytes, kCsvTile = kCsvTileBytes;  // s3imph_ctx.h
constexpr int kCsvT = kCsvTile / kCsvRun;                         // lanes per tile
constexpr int kCsvScanT = 1024;  // lanes of the tile-map scan
constexpr int kCT = 256;         // lanes of the per-record and per-word kernels
static_assert(kCsvRun == 32 && kCsvT == 256, "a run is two 16-byte LDS reads; the block scans are sized for 256 lanes");

enum : unsigned { sR = 0, sF = 1, sU = 2, sQ = 3, sE = 4 };
enum : unsigned { cQuote = 0, cComma = 1, cNl = 2, cOther = 3 };

// A state map: bits [3 s, 3 s + 3) hold the image of state s.
constexpr unsigned pack5(unsigned r, unsigned f, unsigned u, unsigned q, unsigned e) {
  return r | f << 3 | u << 6 | q << 9 | e << 12;
}
constexpr unsigned kIdent = pack5(sR, sF, sU, sQ, sE);
constexpr unsigned kOnQuote = pack5(sQ, sQ, sU, sE, sQ);
constexpr unsigned kOnComma = pack5(sF, sF, sF, sQ, sF);
constexpr unsigned kOnNl = pack5(sR, sR, sR, sQ, sR);
constexpr unsigned kOnOther = pack5(sU, sU, sU, sQ, sQ);

__device__ __forceinline__ unsigned classify(unsigned c) {
  return c == '"' ? cQuote : c == ',' ? cComma : c == '\n' ? cNl : cOther;
}
__device__ __forceinline__ unsigned class_map(unsigned cls) {
  return cls == cQuote ? kOnQuote : cls == cComma ? kOnComma : cls == cNl ? kOnNl : kOnOther;
}
__device__ __forceinline__ unsigned apply(unsigned map, unsigned state) { return (map >> (3 * state)) & 7u; }
__device__ __forceinline__ unsigned step(unsigned state, unsigned cls) { return apply(class_map(cls), state); }
// first a, then b
__device__ __forceinline__ unsigned compose(unsigned a, unsigned b) {
  unsigned r = 0;
#pragma unroll
  for (unsigned st = 0; st < 5; ++st) r |= apply(b, apply(a, st)) << (3 * st);
  return r;
}
// a '\n' in one of these states ends a record; so does the end of the buffer in any state but R
__device__ __forceinline__ bool nl_ends_record(unsigned state) { return state == sF || state == sU || state == sE; }

// The tile at `base` (a multiple of 16) into LDS, and 16 bytes more for the look-ahead: whole
// 16-byte pieces while they end inside the readable round_up(len, 8), one 8-byte piece at the
// tail, zeros beyond.  A pointer that is not 16-byte aligned takes two 8-byte loads per piece.
__device__ __forceinline__ void stage_tile(const uint8_t* __restrict__ csv, uint64_t len8, uint64_t base,
                                           uint4* __restrict__ lds) {
  const bool al16 = ((uintptr_t)csv & 15) == 0;
  for (unsigned k = threadIdx.x; k < kCsvTile / 16 + 1; k += kCsvT) {
    const uint64_t off = base + 16ull * k;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (off + 16 <= len8) {
      if (al16) {
        v = *reinterpret_cast<const uint4*>(csv + off);
      } else {
        const uint64_t* w = reinterpret_cast<const uint64_t*>(csv + off);
        const uint64_t lo = w[0], hi = w[1];
        v = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32));
      }
    } else if (off + 8 <= len8) {
      const uint64_t lo = *reinterpret_cast<const uint64_t*>(csv + off);
      v = make_uint4((uint32_t)lo, (uint32_t)(lo >> 32), 0, 0);
    }
    lds[k] = v;
  }
  __syncthreads();
}

// One lane's run out of LDS: 32 bytes and the byte after them.
struct Run {
  uint32_t w[9];
  __device__ __forceinline__ void load(const uint4* __restrict__ lds) {
    const uint4 a = lds[2 * threadIdx.x], b = lds[2 * threadIdx.x + 1];
    w[0] = a.x, w[1] = a.y, w[2] = a.z, w[3] = a.w;
    w[4] = b.x, w[5] = b.y, w[6] = b.z, w[7] = b.w;
    w[8] = reinterpret_cast<const uint32_t*>(lds)[8 * threadIdx.x + 8];
  }
  __device__ __forceinline__ unsigned byte(int k) const { return (w[k >> 2] >> (8 * (k & 3))) & 0xffu; }
};

// The run's bytes as automaton input: f(i, cls) for every byte at offset i < len that is not
// a deleted '\r'.  Unrolled, so the byte picks are register selects.
template <class F>
__device__ __forceinline__ void for_run(const Run& r, uint64_t run_base, uint64_t len, F f) {
#pragma unroll
  for (int k = 0; k < kCsvRun; ++k) {
    const uint64_t i = run_base + k;
    const unsigned c = r.byte(k);
    const bool deleted = c == '\r' && (i + 1 >= len || r.byte(k + 1) == '\n');
    if (i < len && !deleted) f(i, classify(c));
  }
}

// Inclusive scan of `mine` over the workgroup's 256 lanes in sc[] (op(earlier, later)); returns
// the exclusive value, *total the whole workgroup's.
template <class T, class Op>
__device__ __forceinline__ T block_scan_excl(T mine, T ident, T* sc, Op op, T* total) {
  const unsigned t = threadIdx.x;
  sc[t] = mine;
  __syncthreads();
  for (unsigned d = 1; d < blockDim.x; d <<= 1) {
    const T v = t >= d ? op(sc[t - d], sc[t]) : sc[t];
    __syncthreads();
    sc[t] = v;
    __syncthreads();
  }
  const T ex = t ? sc[t - 1] : ident;
  *total = sc[blockDim.x - 1];
  __syncthreads();
  return ex;
}

// (1) per run: the map from the tile's start to the run's start; per tile: its whole map
__global__ __launch_bounds__(kCsvT) void k_csv_maps(const uint8_t* __restrict__ csv, uint64_t len,
                                                    uint16_t* __restrict__ runmap, uint16_t* __restrict__ tilemap) {
  __shared__ uint4 lds[kCsvTile / 16 + 1];
  __shared__ unsigned sc[kCsvT];
  const uint64_t base = (uint64_t)blockIdx.x * kCsvTile;
  stage_tile(csv, (len + 7) & ~7ull, base, lds);
  Run r;
  r.load(lds);
  unsigned m = kIdent;
  for_run(r, base + (uint64_t)threadIdx.x * kCsvRun, len, [&](uint64_t, unsigned cls) {
    unsigned n = 0;
#pragma unroll
    for (unsigned st = 0; st < 5; ++st) n |= step(apply(m, st), cls) << (3 * st);
    m = n;
  });
  unsigned total;
  const unsigned ex = block_scan_excl(m, kIdent, sc, [](unsigned a, unsigned b) { return compose(a, b); }, &total);
  runmap[(uint64_t)blockIdx.x * kCsvT + threadIdx.x] = (uint16_t)ex;
  if (threadIdx.x == 0) tilemap[blockIdx.x] = (uint16_t)total;
}

// (1) the entry state of every tile: one workgroup, a contiguous share of the tiles per lane
__global__ __launch_bounds__(kCsvScanT) void k_csv_tile_scan(const uint16_t* __restrict__ tilemap, uint64_t nt,
                                                             uint8_t* __restrict__ entry) {
  __shared__ unsigned sc[kCsvScanT];
  const uint64_t share = (nt + kCsvScanT - 1) / kCsvScanT;
  const uint64_t lo = min(nt, threadIdx.x * share), hi = min(nt, lo + share);
  unsigned m = kIdent;
  for (uint64_t b = lo; b < hi; ++b) m = compose(m, tilemap[b]);
  unsigned total;
  const unsigned ex = block_scan_excl(m, kIdent, sc, [](unsigned a, unsigned b) { return compose(a, b); }, &total);
  unsigned state = apply(ex, sR);
  for (uint64_t b = lo; b < hi; ++b) {
    entry[b] = (uint8_t)state;
    state = apply(tilemap[b], state);
  }
}

// (2) record ends.  An end is the offset just past the record: past its '\n', or len for a last
// record without one.  kWrite false: tile_count[tile] = ends in the tile.  kWrite true:
// tile_count holds the exclusive scan of those, and the ends go to ends[record number].
template <bool kWrite>
__global__ __launch_bounds__(kCsvT) void k_csv_ends(const uint8_t* __restrict__ csv, uint64_t len,
                                                    const uint16_t* __restrict__ runmap,
                                                    const uint8_t* __restrict__ entry, uint64_t* __restrict__ tile_count,
                                                    uint64_t* __restrict__ ends) {
  __shared__ uint4 lds[kCsvTile / 16 + 1];
  __shared__ unsigned sc[kCsvT];
  const uint64_t base = (uint64_t)blockIdx.x * kCsvTile;
  stage_tile(csv, (len + 7) & ~7ull, base, lds);
  Run r;
  r.load(lds);
  const uint64_t run_base = base + (uint64_t)threadIdx.x * kCsvRun;
  const unsigned state0 = apply(runmap[(uint64_t)blockIdx.x * kCsvT + threadIdx.x], entry[blockIdx.x]);
  const bool has_last = run_base < len && len - run_base <= (uint64_t)kCsvRun;  // the buffer's last byte is in this run
  unsigned state = state0, cnt = 0;
  for_run(r, run_base, len, [&](uint64_t, unsigned cls) {
    cnt += cls == cNl && nl_ends_record(state);
    state = step(state, cls);
  });
  cnt += has_last && state != sR;
  unsigned total;
  const unsigned ex = block_scan_excl(cnt, 0u, sc, [](unsigned a, unsigned b) { return a + b; }, &total);
  if (!kWrite) {
    if (threadIdx.x == 0) tile_count[blockIdx.x] = total;
    return;
  }
  uint64_t at = tile_count[blockIdx.x] + ex;
  state = state0;
  for_run(r, run_base, len, [&](uint64_t i, unsigned cls) {
    if (cls == cNl && nl_ends_record(state)) ends[at++] = i + 1;
    state = step(state, cls);
  });
  if (has_last && state != sR) ends[at] = len;
}

// The text read byte by byte through one aligned 8-byte word at a time (i < len, so the word
// lies inside round_up(len, 8)).
struct Bytes {
  const uint8_t* p;
  uint64_t w = 0, wi = ~0ull;
  __device__ __forceinline__ unsigned at(uint64_t i) {
    if ((i >> 3) != wi) {
      wi = i >> 3;
      w = *reinterpret_cast<const uint64_t*>(p + 8 * wi);
    }
    return (unsigned)(w >> (8 * (i & 7))) & 0xffu;
  }
};

// One record, [start, end) of the text, from state R: emit(field, offset, byte) for every byte
// the fields are made of, in order; returns the number of fields.  The '"' a lazy quote emits
// late (state E, then an ordinary byte) is the byte before that one: a deleted '\r' is never
// followed by an ordinary byte.
template <class Emit>
__device__ __forceinline__ unsigned walk_record(Bytes& in, uint64_t start, uint64_t end, uint64_t len, Emit emit) {
  unsigned state = sR, field = 0;
  for (uint64_t i = start; i < end; ++i) {
    const unsigned c = in.at(i);
    if (c == '\r' && (i + 1 >= len || in.at(i + 1) == '\n')) continue;
    const unsigned cls = classify(c);
    if (state == sQ) {
      if (cls != cQuote) emit(field, i, c);
    } else if (state == sE) {
      if (cls == cQuote) {
        emit(field, i, c);
      } else if (cls == cOther) {
        emit(field, i - 1, (unsigned)'"');
        emit(field, i, c);
      }
    } else if (cls == cOther || (cls == cQuote && state == sU)) {
      emit(field, i, c);
    }
    field += (cls == cComma && state != sQ) || (cls == cNl && nl_ends_record(state));
    state = step(state, cls);
  }
  return field + (state != sR);  // the end of the buffer ends the last field
}

struct CsvTop {
  unsigned long long n_short, n_empty_key, n_bad_size;
};

// strconv.ParseUint(strings.TrimSpace(s), 10, 64) fed byte by byte
struct SizeParse {
  uint64_t v = 0;
  unsigned phase = 0;  // 0 leading white space, 1 digits, 2 trailing white space
  bool bad = false;
  __device__ __forceinline__ void feed(unsigned c) {
    if (tier_space((unsigned char)c)) {
      phase = phase == 1 ? 2 : phase;
    } else if (c >= '0' && c <= '9' && phase < 2) {
      const uint64_t d = c - '0';
      bad |= v > (~0ull - d) / 10;
      v = v * 10 + d;
      phase = 1;
    } else {
      bad = true;
    }
  }
  __device__ __forceinline__ bool ok() const { return !bad && phase >= 1; }
};

// A tier name field trimmed as it arrives: the first 40 bytes from the first non-space one, and
// the trimmed length (a name longer than kTierNameMax matches nothing, so 40 are enough).  A copy,
// not a position in the text: matching the names out of the text again measured slower.
struct NameField {
  unsigned char b[40];
  unsigned n = 0, last = 0;
  __device__ __forceinline__ void feed(unsigned c) {
    const bool sp = tier_space((unsigned char)c);
    if (n == 0 && sp) return;
    if (n < 40) b[n] = (unsigned char)c;
    n += n < 64;
    if (!sp) last = n;
  }
};

constexpr uint64_t kRewalk = 1ull << 63;  // src flag: the key's bytes do not stand contiguous in the text

// (3) one lane per record; lane n_rec writes the scans' last inputs
__global__ __launch_bounds__(kCT) void k_csv_fields(const uint8_t* __restrict__ csv, uint64_t len,
                                                    const uint64_t* __restrict__ ends, uint64_t n_rec,
                                                    s3imph_csv_schema sch, uint64_t* __restrict__ keep,
                                                    uint64_t* __restrict__ koff, uint64_t* __restrict__ src,
                                                    uint64_t* __restrict__ size, uint8_t* __restrict__ tier,
                                                    CsvTop* __restrict__ top) {
  const uint64_t r = (uint64_t)blockIdx.x * kCT + threadIdx.x;
  if (r > n_rec) return;
  if (r == n_rec) {
    keep[r] = 0;
    koff[r] = 0;
    return;
  }
  Bytes in{csv};
  uint64_t klen = 0, ksrc = 0;
  bool contiguous = true;
  SizeParse sz;
  NameField sc, at;
  const unsigned nf = walk_record(in, r ? ends[r - 1] : 0, ends[r], len, [&](unsigned f, uint64_t pos, unsigned c) {
    if ((int64_t)f == sch.key_col) {
      if (klen == 0) ksrc = pos;
      contiguous &= pos == ksrc + klen;
      ++klen;
    }
    if ((int64_t)f == sch.size_col) sz.feed(c);
    if ((int64_t)f == sch.storage_col) sc.feed(c);
    if ((int64_t)f == sch.access_tier_col) at.feed(c);
  });
  const bool is_short = (int64_t)nf <= sch.key_col || (int64_t)nf <= sch.size_col;
  const bool kept = !is_short && klen > 0;
  if (is_short) atomicAdd(&top->n_short, 1ull);
  else if (!kept) atomicAdd(&top->n_empty_key, 1ull);
  else if (!sz.ok()) atomicAdd(&top->n_bad_size, 1ull);
  keep[r] = kept;
  koff[r] = kept ? klen : 0;
  src[r] = ksrc | (contiguous ? 0 : kRewalk);
  size[r] = kept && sz.ok() ? sz.v : 0;
  tier[r] = (uint8_t)tier_from_trimmed(sc.b, sc.last, at.b, at.last);
}

// (4) the kept records' offsets, sizes, tiers and key sources by object number (keep and koff
// are exclusive scans now); lane n_rec writes the last offset
__global__ __launch_bounds__(kCT) void k_csv_meta(const uint64_t* __restrict__ keep, const uint64_t* __restrict__ koff,
                                                  const uint64_t* __restrict__ src, const uint64_t* __restrict__ size,
                                                  const uint8_t* __restrict__ tier, uint64_t n_rec, uint64_t key_base,
                                                  uint64_t* __restrict__ offsets, uint64_t* __restrict__ sizes,
                                                  uint8_t* __restrict__ tiers, uint64_t* __restrict__ osrc) {
  const uint64_t r = (uint64_t)blockIdx.x * kCT + threadIdx.x;
  if (r > n_rec) return;
  const uint64_t k = keep[r];
  if (r == n_rec) {
    offsets[k] = key_base + koff[r];
    return;
  }
  if (keep[r + 1] == k) return;
  offsets[k] = key_base + koff[r];
  sizes[k] = size[r];
  if (tiers) tiers[k] = tier[r];
  osrc[k] = src[r];
}

// The first object of every chunk of kCT output words: the last one that starts at or before the
// chunk's first byte of this file (offsets[0] = key_base).
__global__ __launch_bounds__(kCT) void k_csv_key_bounds(const uint64_t* __restrict__ offsets, uint64_t n_obj,
                                                        uint64_t key_base, uint64_t word0, uint64_t chunks,
                                                        uint64_t* __restrict__ bounds) {
  const uint64_t t = (uint64_t)blockIdx.x * kCT + threadIdx.x;
  if (t >= chunks) return;
  bounds[t] = first_above(offsets, 0, n_obj + 1, max(8 * (word0 + t * kCT), key_base)) - 1;
}

// (4) the key bytes, by 8-byte words of the output blob counted from its start (emit_word's scheme,
// s3imph_keys.h, on a word grid that does not begin at this file's first byte: key_base is where
// the file before ended).  The bytes of the first word below key_base are left alone; the bytes of
// the last word past the keys are zeros.  A key that needs the re-walk gets bytes of its raw field
// here (never more than the field holds) and its own in k_csv_key_rewalk.
__global__ __launch_bounds__(kCT) void k_csv_key_words(const uint8_t* __restrict__ csv, uint64_t len8,
                                                       const uint64_t* __restrict__ offsets,
                                                       const uint64_t* __restrict__ osrc,
                                                       const uint64_t* __restrict__ bounds, uint64_t n_obj,
                                                       uint64_t key_base, uint64_t key_end, uint64_t word0,
                                                       uint64_t word1, uint8_t* __restrict__ out) {
  const uint64_t wi = word0 + (uint64_t)blockIdx.x * kCT + threadIdx.x;
  if (wi >= word1) return;
  const uint64_t a = 8 * wi, lo = max(a, key_base), hi = min(a + 8, key_end);
  uint64_t v = 0;
  if (lo < hi) {
    const uint64_t r_lo = bounds[blockIdx.x];
    const uint64_t r_hi = blockIdx.x + 1 < gridDim.x ? bounds[blockIdx.x + 1] : n_obj - 1;
    uint64_t r = first_above(offsets, r_lo + 1, r_hi + 1, lo) - 1;
    uint64_t o0 = offsets[r], o1 = offsets[r + 1];
    for (uint64_t p = lo; p < hi;) {
      while (o1 <= p) {  // offsets[n_obj] = key_end > p ends it
        ++r;
        o0 = o1;
        o1 = offsets[r + 1];
      }
      const uint64_t cnt = min(o1, hi) - p;  // bytes of object r in this word, 1..8
      const uint64_t x = load8(csv, (osrc[r] & ~kRewalk) + (p - o0), len8);
      v |= (cnt >= 8 ? x : x & ((1ull << (8 * cnt)) - 1)) << (8 * (p - a));
      p += cnt;
    }
  }
  if (lo == a && ((uintptr_t)out & 7) == 0) {
    *reinterpret_cast<uint64_t*>(out + a) = v;
  } else {
    for (uint64_t j = lo - a; j < 8; ++j) out[a + j] = (uint8_t)(v >> (8 * j));
  }
}

// (4) the keys whose bytes are not contiguous in the text ("" inside quotes, a '\r' deleted
// inside the key): walked again, written byte by byte
__global__ __launch_bounds__(kCT) void k_csv_key_rewalk(const uint8_t* __restrict__ csv, uint64_t len,
                                                        const uint64_t* __restrict__ ends, uint64_t n_rec,
                                                        int32_t key_col, const uint64_t* __restrict__ keep,
                                                        const uint64_t* __restrict__ src,
                                                        const uint64_t* __restrict__ offsets, uint8_t* __restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * kCT + threadIdx.x;
  if (r >= n_rec) return;
  const uint64_t k = keep[r];
  if (keep[r + 1] == k || !(src[r] & kRewalk)) return;
  Bytes in{csv};
  uint64_t at = offsets[k];
  walk_record(in, r ? ends[r - 1] : 0, ends[r], len, [&](unsigned f, uint64_t, unsigned c) {
    if ((int64_t)f == key_col) out[at++] = (uint8_t)c;
  });
}

unsigned blocks(uint64_t count) { return (unsigned)((count + kCT - 1) / kCT); }

}  // namespace

// Scratch of the parse and the last plan, kept in the context and grown as needed.
//   per input byte: the run maps, 2 B per kCsvRun bytes (1/16 B), and 11 B per tile of kCsvTile;
//   per record:     its end, the two scans, the key source and the size (5 x 8 B) and the tier
//                   (1 B): 41 B; per object 8 B more during the fill (the sources by object);
//   plus rocPRIM's temporary and 8 B per 2 KiB of key bytes (the fill's chunk bounds).
struct CsvScratch {
  uint16_t *runmap = nullptr, *tilemap = nullptr;
  uint8_t* entry = nullptr;
  uint64_t* tile_count = nullptr;
  uint64_t cap_tiles = 0;
  uint64_t *ends = nullptr, *keep = nullptr, *koff = nullptr, *src = nullptr, *size = nullptr;
  uint8_t* tier = nullptr;
  uint64_t cap_rec = 0;
  uint64_t* osrc = nullptr;
  uint64_t cap_obj = 0;
  uint64_t* bounds = nullptr;
  uint64_t bounds_cap = 0;
  CsvTop* top = nullptr;
  PrimTmp tmp;
  // the last plan
  bool have_plan = false;
  const uint8_t* csv = nullptr;
  uint64_t len = 0;
  s3imph_csv_schema schema{};
  uint64_t n_rec = 0, n_obj = 0, key_bytes = 0;
  void release() {
    dfree(runmap);
    dfree(tilemap);
    dfree(entry);
    dfree(tile_count);
    dfree(ends);
    dfree(keep);
    dfree(koff);
    dfree(src);
    dfree(size);
    dfree(tier);
    dfree(osrc);
    dfree(bounds);
    dfree(top);
    tmp.release();
    cap_tiles = cap_rec = cap_obj = bounds_cap = 0;
    have_plan = false;
  }
};

void csv_scratch_free(s3imph_ctx* c) {
  if (c->csv) {
    c->csv->release();
    delete c->csv;
    c->csv = nullptr;
  }
}

// Every pass that sizes the listing of one CSV buffer in HBM; keeps the plan.  Waits for the
// stream.  Two small D2H: the record count sizes the per-record arrays of the passes after it.
int csv_plan(s3imph_ctx* c, const uint8_t* csv, uint64_t len, const s3imph_csv_schema& sch, s3imph_csv_info* info,
             hipStream_t s, std::string* msg) {
  std::memset(info, 0, sizeof *info);
  if (!c->csv) c->csv = new CsvScratch();
  CsvScratch& a = *c->csv;
  a.have_plan = false;
  a.csv = csv;
  a.len = len;
  a.schema = sch;
  a.n_rec = a.n_obj = a.key_bytes = 0;
  if (len == 0) {
    a.have_plan = true;
    return S3IMPH_OK;
  }
  const uint64_t nt = (len + kCsvTile - 1) / kCsvTile;
  if (nt >> 31) {
    *msg = "csv: a buffer of 2^44 bytes or more";
    return S3IMPH_ERR_INVALID;
  }
  if (nt > a.cap_tiles) {
    a.cap_tiles = 0;
    dalloc(a.runmap, nt * kCsvT);
    dalloc(a.tilemap, nt);
    dalloc(a.entry, nt);
    dalloc(a.tile_count, nt + 1);
    a.cap_tiles = nt;
  }
  if (!a.top) dalloc(a.top, 1);
  k_csv_maps<<<(unsigned)nt, kCsvT, 0, s>>>(csv, len, a.runmap, a.tilemap);
  HIPCHECK(hipGetLastError());
  k_csv_tile_scan<<<1, kCsvScanT, 0, s>>>(a.tilemap, nt, a.entry);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemsetAsync(a.tile_count + nt, 0, 8, s));
  k_csv_ends<false><<<(unsigned)nt, kCsvT, 0, s>>>(csv, len, a.runmap, a.entry, a.tile_count, nullptr);
  HIPCHECK(hipGetLastError());
  scan_u64(a.tmp, a.tile_count, nt + 1, 0, s);
  uint64_t n_rec = 0;
  HIPCHECK(hipMemcpyAsync(&n_rec, a.tile_count + nt, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  info->n_records = n_rec;
  a.n_rec = n_rec;
  if (n_rec == 0) {
    a.have_plan = true;
    return S3IMPH_OK;
  }
  if (n_rec > a.cap_rec) {
    a.cap_rec = 0;
    dalloc(a.ends, n_rec);
    dalloc(a.keep, n_rec + 1);
    dalloc(a.koff, n_rec + 1);
    dalloc(a.src, n_rec);
    dalloc(a.size, n_rec);
    dalloc(a.tier, n_rec);
    a.cap_rec = n_rec;
  }
  HIPCHECK(hipMemsetAsync(a.top, 0, sizeof(CsvTop), s));
  k_csv_ends<true><<<(unsigned)nt, kCsvT, 0, s>>>(csv, len, a.runmap, a.entry, a.tile_count, a.ends);
  HIPCHECK(hipGetLastError());
  k_csv_fields<<<blocks(n_rec + 1), kCT, 0, s>>>(csv, len, a.ends, n_rec, sch, a.keep, a.koff, a.src, a.size, a.tier,
                                                 a.top);
  HIPCHECK(hipGetLastError());
  scan_u64(a.tmp, a.keep, n_rec + 1, 0, s);
  scan_u64(a.tmp, a.koff, n_rec + 1, 0, s);
  CsvTop top{};
  HIPCHECK(hipMemcpyAsync(&a.n_obj, a.keep + n_rec, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&a.key_bytes, a.koff + n_rec, 8, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipMemcpyAsync(&top, a.top, sizeof top, hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
  info->n_objects = a.n_obj;
  info->key_bytes = a.key_bytes;
  info->n_short = top.n_short;
  info->n_empty_key = top.n_empty_key;
  info->n_bad_size = top.n_bad_size;
  if (a.n_obj >> 32) {
    *msg = "csv: 2^32 objects or more in one buffer (the listing sort's order is a uint32)";
    return S3IMPH_ERR_INVALID;
  }
  a.have_plan = true;
  return S3IMPH_OK;
}

// The listing of the last plan.  Waits for the stream.
int csv_fill(s3imph_ctx* c, uint8_t* keys, uint64_t keys_cap, uint64_t key_base, uint64_t* offsets, uint64_t* sizes,
             uint8_t* tiers, hipStream_t s, std::string* msg) {
  if (!c->csv || !c->csv->have_plan) {
    *msg = "csv: fill without a plan";
    return S3IMPH_ERR_STATE;
  }
  CsvScratch& a = *c->csv;
  const uint64_t key_end = key_base + a.key_bytes;
  const uint64_t word0 = key_base >> 3, word1 = (key_end + 7) >> 3;
  if (keys_cap < 8 * word1) {
    *msg = "csv: the keys need " + std::to_string(8 * word1) + " blob bytes";
    return S3IMPH_ERR_INVALID;
  }
  if (!offsets || (word1 > word0 && !keys) || (a.n_obj && !sizes)) {
    *msg = "csv: null output array";
    return S3IMPH_ERR_INVALID;
  }
  if (a.n_obj == 0) {  // the single offset, and zeros up to the next word
    HIPCHECK(hipMemcpyAsync(offsets, &key_base, 8, hipMemcpyHostToDevice, s));
    if (8 * word1 > key_base) HIPCHECK(hipMemsetAsync(keys + key_base, 0, 8 * word1 - key_base, s));
    HIPCHECK(hipStreamSynchronize(s));
    return S3IMPH_OK;
  }
  grow(a.osrc, a.cap_obj, a.n_obj);
  k_csv_meta<<<blocks(a.n_rec + 1), kCT, 0, s>>>(a.keep, a.koff, a.src, a.size, a.tier, a.n_rec, key_base, offsets,
                                                 sizes, tiers, a.osrc);
  HIPCHECK(hipGetLastError());
  const uint64_t chunks = (word1 - word0 + kCT - 1) / kCT;
  grow(a.bounds, a.bounds_cap, chunks);
  k_csv_key_bounds<<<blocks(chunks), kCT, 0, s>>>(offsets, a.n_obj, key_base, word0, chunks, a.bounds);
  HIPCHECK(hipGetLastError());
  k_csv_key_words<<<(unsigned)chunks, kCT, 0, s>>>(a.csv, (a.len + 7) & ~7ull, offsets, a.osrc, a.bounds, a.n_obj,
                                                   key_base, key_end, word0, word1, keys);
  HIPCHECK(hipGetLastError());
  k_csv_key_rewalk<<<blocks(a.n_rec), kCT, 0, s>>>(a.csv, a.len, a.ends, a.n_rec, a.schema.key_col, a.keep, a.src,
                                                   offsets, keys);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipStreamSynchronize(s));
  return S3IMPH_OK;
}

namespace {

void add_info(s3imph_csv_info* t, const s3imph_csv_info& i) {
  t->n_records += i.n_records;
  t->n_objects += i.n_objects;
  t->key_bytes += i.key_bytes;
  t->n_short += i.n_short;
  t->n_empty_key += i.n_empty_key;
  t->n_bad_size += i.n_bad_size;
}

// A listing array of `used` elements given room for `need` (owned by g; the contents are kept).
template <typename T>
void keep_grow(DevGuard& g, T*& p, uint64_t& cap, uint64_t used, uint64_t need, hipStream_t s) {
  if (need <= cap) return;
  const uint64_t ncap = std::max(need, cap + cap / 2);
  T* q = nullptr;
  g.make(q, ncap);
  if (used) HIPCHECK(hipMemcpyAsync(q, p, used * sizeof(T), hipMemcpyDeviceToDevice, s));
  HIPCHECK(hipStreamSynchronize(s));
  g.drop(p);
  p = q;
  cap = ncap;
}

}  // namespace

// The CSV buffers of `f`, each parsed on its own, appended in order into one listing in HBM
// (owned by g; the keys readable 16 bytes past their end rounded up to 8, as upload_keys leaves
// them).  The first file's yield per byte sizes the arrays for all of them; they grow when a later
// file yields more.  *m == 0: no array is made.  With f.gz the buffers are gzip files: only the
// source of each file's text changes (s3imph_inflate.hip), the plan / fill loop is the same.
int csv_listing(s3imph_ctx* c, DevGuard& g, const CsvFiles& f, uint8_t*& d_keys, uint64_t*& d_koff,
                uint64_t*& d_sizes, uint8_t*& d_tiers, uint64_t* m, hipStream_t s, std::string* msg) {
  uint64_t cap_keys = 0, cap_off = 0, cap_sizes = 0, cap_tiers = 0, n = 0, nbytes = 0, left = 0;
  for (uint64_t i = 0; i < f.n_files; ++i) left += f.len[i];
  s3imph_csv_info total{};
  // One file's text in HBM (len bytes, readable to round_up(len, 8)) appended to the listing;
  // `weight` is the file's share of `left` (its bytes as they were given: compressed with gz).
  auto append = [&](const uint8_t* d_csv, uint64_t len, uint64_t weight, bool last) -> int {
    s3imph_csv_info info;
    const int rc = csv_plan(c, d_csv, len, *f.schema, &info, s, msg);
    if (rc != S3IMPH_OK) return rc;
    add_info(&total, info);
    if ((n + info.n_objects) >> 32) {
      *msg = "csv: 2^32 objects or more (the listing sort's order is a uint32)";
      return S3IMPH_ERR_INVALID;
    }
    if (info.n_objects) {
      // this file's yield, scaled to the bytes still to come, with a twentieth to spare
      const double scale = 1.05 * (double)left / (double)std::max<uint64_t>(weight, 1);
      const uint64_t want_n = n + (!last ? (uint64_t)(info.n_objects * scale) : info.n_objects);
      const uint64_t want_b = nbytes + (!last ? (uint64_t)(info.key_bytes * scale) : info.key_bytes);
      // the estimate counts only for the first allocation; afterwards an array grows when it must
      const uint64_t est_n = cap_off ? 0 : want_n, est_b = cap_keys ? 0 : want_b;
      const uint64_t need_n = std::max<uint64_t>(n + info.n_objects, est_n);
      const uint64_t need_b = ((std::max<uint64_t>(nbytes + info.key_bytes, est_b) + 7) & ~7ull) + 16;
      keep_grow(g, d_keys, cap_keys, nbytes, need_b, s);
      keep_grow(g, d_koff, cap_off, n + (n ? 1 : 0), need_n + 1, s);
      keep_grow(g, d_sizes, cap_sizes, n, need_n, s);
      if (f.with_tiers) keep_grow(g, d_tiers, cap_tiers, n, need_n, s);
      const int rc2 = csv_fill(c, d_keys, cap_keys - 16, nbytes, d_koff + n, d_sizes + n,
                               f.with_tiers ? d_tiers + n : nullptr, s, msg);
      if (rc2 != S3IMPH_OK) return rc2;
      n += info.n_objects;
      nbytes += info.key_bytes;
    }
    c->csv->have_plan = false;  // the text goes away here
    left -= weight;
    return S3IMPH_OK;
  };
  // gzip files: groups of consecutive files, in input order, each uploaded compressed, inflated in
  // one launch and parsed file by file from HBM
  for (uint64_t lo = 0; f.gz && lo < f.n_files;) {
    const uint64_t budget = f.group_bytes ? f.group_bytes : kGzGroupBytes;
    uint64_t hi = lo, sum = 0;
    while (hi < f.n_files) {
      const uint64_t cost = f.len[hi] + gunzip_room_hint(f.csv[hi], f.len[hi]);
      if (hi > lo && (cost > budget || sum > budget - cost)) break;
      sum += std::min(cost, budget);
      ++hi;
    }
    GzTexts t;
    const int rc = gunzip_group(c, g, f.csv, f.len, lo, hi, &t, s, msg);
    if (rc != S3IMPH_OK) return rc;
    for (uint64_t i = lo; i < hi; ++i) {
      const uint64_t len = t.info[i - lo].out_bytes;
      if (len == 0) {
        left -= f.len[i];
        continue;
      }
      const int rc2 = append(t.text[i - lo], len, f.len[i], i + 1 == f.n_files);
      if (rc2 != S3IMPH_OK) return rc2;
    }
    gunzip_group_free(g, &t);
    lo = hi;
  }
  for (uint64_t i = 0; !f.gz && i < f.n_files; ++i) {
    const uint64_t len = f.len[i];
    if (len == 0) continue;
    uint8_t* d_csv = nullptr;
    g.make(d_csv, (len + 7) & ~7ull);
    staged_copy(c, true, d_csv, f.csv[i], len);
    const int rc = append(d_csv, len, len, i + 1 == f.n_files);
    if (rc != S3IMPH_OK) return rc;
    g.drop(d_csv);
  }
  if (f.total) *f.total = total;
  *m = n;
  return S3IMPH_OK;
}

}  // namespace s3imph

using namespace s3imph;

extern "C" {

void s3imph_csv_geometry(uint32_t* run_bytes, uint32_t* tile_bytes) {
  if (run_bytes) *run_bytes = kCsvRunBytes;
  if (tile_bytes) *tile_bytes = kCsvTileBytes;
}

int s3imph_csv_plan_device(s3imph_ctx* c, const uint8_t* d_csv, uint64_t len, const s3imph_csv_schema* schema,
                           s3imph_csv_info* info, void* stream) {
  if (!c || !schema || !info || (len && !d_csv) || schema->key_col < 0 || schema->size_col < 0)
    return S3IMPH_ERR_INVALID;
  return device_entry(c, "csv: ", [&](std::string& msg) {
    hipStream_t s = use_device(c->device, stream, c->own_stream);
    return retry_on_nomem(c, s, &msg, [&] { return csv_plan(c, d_csv, len, *schema, info, s, &msg); });
  });
}

int s3imph_csv_fill_device(s3imph_ctx* c, uint8_t* d_keys, uint64_t keys_cap, uint64_t key_base,
                           uint64_t* d_key_offsets, uint64_t* d_sizes, uint8_t* d_tiers, void* stream) {
  if (!c) return S3IMPH_ERR_INVALID;
  return device_entry(c, "csv: ", [&](std::string& msg) {
    hipStream_t s = use_device(c->device, stream, c->own_stream);
    return csv_fill(c, d_keys, keys_cap, key_base, d_key_offsets, d_sizes, d_tiers, s, &msg);
  });
}

int s3imph_csv_parse_host(int device, const uint8_t* csv, uint64_t len, const s3imph_csv_schema* schema,
                          uint8_t** keys, uint64_t** key_offsets, uint64_t** sizes, uint8_t** tiers,
                          s3imph_csv_info* info, char* err, size_t errlen) {
  if (!schema || !keys || !key_offsets || !sizes || !tiers || !info || (len && !csv) || schema->key_col < 0 ||
      schema->size_col < 0)
    return S3IMPH_ERR_INVALID;
  *keys = *tiers = nullptr;
  *key_offsets = *sizes = nullptr;
  std::memset(info, 0, sizeof *info);
  auto drop = [&] {
    std::free(*keys);
    std::free(*key_offsets);
    std::free(*sizes);
    std::free(*tiers);
    *keys = *tiers = nullptr;
    *key_offsets = *sizes = nullptr;
  };
  if (len == 0)  // no device
    return host_call("csv: ", err, errlen, [&](std::string&) {
      *key_offsets = host_array<uint64_t>(1);
      (*key_offsets)[0] = 0;
      return S3IMPH_OK;
    });
  const int rc = host_entry(device, "csv: ", err, errlen, [&](s3imph_ctx* c, hipStream_t s, std::string& msg) -> int {
    DevGuard g;
    uint8_t *d_csv = nullptr, *d_keys = nullptr, *d_tiers = nullptr;
    uint64_t *d_off = nullptr, *d_sizes = nullptr;
    g.make(d_csv, (len + 7) & ~7ull);
    staged_copy(c, true, d_csv, csv, len);
    int rc2 = csv_plan(c, d_csv, len, *schema, info, s, &msg);
    if (rc2 != S3IMPH_OK) return rc2;
    const uint64_t n = info->n_objects, cap = (info->key_bytes + 7) & ~7ull;
    g.make(d_keys, cap);
    g.make(d_off, n + 1);
    g.make(d_sizes, n);
    g.make(d_tiers, n);
    rc2 = csv_fill(c, d_keys, cap, 0, d_off, d_sizes, d_tiers, s, &msg);
    c->csv->have_plan = false;  // the text's copy goes away with this call
    if (rc2 != S3IMPH_OK) return rc2;
    drop();
    *keys = host_array<uint8_t>(info->key_bytes);
    *key_offsets = host_array<uint64_t>(n + 1);
    *sizes = host_array<uint64_t>(n);
    *tiers = host_array<uint8_t>(n);
    if (info->key_bytes) HIPCHECK(hipMemcpy(*keys, d_keys, info->key_bytes, hipMemcpyDeviceToHost));
    staged_copy(c, false, *key_offsets, d_off, (n + 1) * 8);
    if (n) {
      staged_copy(c, false, *sizes, d_sizes, n * 8);
      HIPCHECK(hipMemcpy(*tiers, d_tiers, n, hipMemcpyDeviceToHost));
    }
    return S3IMPH_OK;
  });
  if (rc != S3IMPH_OK) drop();
  return rc;
}

int s3imph_index_from_csv_host(int device, const uint8_t* const* csv, const uint64_t* csv_len, uint64_t n_files,
                               const s3imph_csv_schema* schema, int with_tiers, uint32_t max_depth,
                               const char* out_dir, s3imph_csv_info* info_total, char* err, size_t errlen) {
  if (!schema || !out_dir || (n_files && (!csv || !csv_len)) || schema->key_col < 0 || schema->size_col < 0)
    return S3IMPH_ERR_INVALID;
  for (uint64_t i = 0; i < n_files; ++i)
    if (csv_len[i] && !csv[i]) return S3IMPH_ERR_INVALID;
  s3imph_csv_info total{};
  const CsvFiles f{csv, csv_len, n_files, schema, with_tiers != 0, &total};
  const int rc = index_from_objects(device, nullptr, nullptr, nullptr, nullptr, 0, max_depth, out_dir, true, err,
                                    errlen, &f);
  if (info_total) *info_total = total;
  return rc;
}

int s3imph_index_from_csv_gz_host(int device, const uint8_t* const* gz, const uint64_t* gz_len, uint64_t n_files,
                                  const s3imph_csv_schema* schema, int with_tiers, uint32_t max_depth,
                                  uint64_t group_bytes, const char* out_dir, s3imph_csv_info* info_total, char* err,
                                  size_t errlen) {
  if (!schema || !out_dir || (n_files && (!gz || !gz_len)) || schema->key_col < 0 || schema->size_col < 0)
    return S3IMPH_ERR_INVALID;
  for (uint64_t i = 0; i < n_files; ++i)
    if (gz_len[i] && !gz[i]) return S3IMPH_ERR_INVALID;
  s3imph_csv_info total{};
  const CsvFiles f{gz, gz_len, n_files, schema, with_tiers != 0, &total, true, group_bytes};
  const int rc = index_from_objects(device, nullptr, nullptr, nullptr, nullptr, 0, max_depth, out_dir, true, err,
                                    errlen, &f);
  if (info_total) *info_total = total;
  return rc;
}

}  // extern "C"
