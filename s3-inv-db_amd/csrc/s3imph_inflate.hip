// s3imph_inflate.hip — gzip files in HBM inflated on the GPU (include/s3imph.h section 5j): what
// gzip.NewReader / pgzip.NewReader do in front of the reference's CSV readers (unified.go:93-103,
// reader.go:81-86), checked against RFC 1951 / RFC 1952 and zlib.
//
// A DEFLATE stream is serial: a symbol's length decides where the next one begins, and a gzip
// member carries no block index.  The parallelism is across files:
//   k_inflate        one 64-lane wave per file, a workgroup of one wave; a persistent grid takes
//                    files, longest first, from a ticket counter.  Per wave in LDS: an input stage
//                    of kInChunk bytes filled by wave-wide loads, the decode tables and a queue of
//                    kBatch symbols.  Lane 0 runs the decode steps of s3imph_inflate.h and fills
//                    the queue; all 64 lanes then carry the batch out: an exclusive scan of the
//                    symbols' output lengths, the literals stored in parallel, the matches in
//                    order, each copied by the whole wave.  Tables are built by sixteen lanes, a
//                    code length each; stored blocks are a wave-wide copy from the input.
//   k_crc32_chunks   the CRC-32 of every kCrcChunk bytes of each good file's text, a chunk per lane,
//   k_crc32_fold     folded per file, in order, with the zero-extension operator and compared with
//                    the CRC the member trailers promise (lane 0 folded those the same way).
//
// Bounds: the reader never leaves its window, which load_stage fills with no byte outside the
// file; a table index is masked or checked (huff_decode); a distance is checked against the
// member's own output before it is queued; every store and every copy's load is below the file's
// room.  Corrupt data therefore ends a file with a status and nothing else.
//
// Termination: a file's loop runs step() until kEnd; the argument at step() shows that every
// round takes input bits or ends, and a refill always leaves kStepBytes in the window or reaches
// the file's end, so the round after a refill makes progress.
#include <algorithm>
#include <cstring>
#include <numeric>

#include "s3imph_entry.h"
#include "s3imph_inflate.h"

namespace s3imph {

namespace {

using namespace inflate;

constexpr uint32_t kInChunk = 2048;    // bytes of the input stage
constexpr uint32_t kBatch = 256;       // symbols per batch: four per lane
constexpr uint32_t kWavesPerCu = 16;   // LDS admits 23; 16 is four per SIMD
constexpr uint32_t kCrcChunk = 8192;   // bytes per lane of k_crc32_chunks
constexpr uint32_t kCrcT = 256;
constexpr uint32_t kRefill = 100;      // beside inflate::Event: the window is used up
static_assert(kBatch == 4 * 64, "carry_out gives each lane four symbols");
static_assert(kInChunk % 256 == 0 && kInChunk >= 4 * kStepBytes, "a refill must leave a step's bytes");

struct InflateShared {
  uint32_t stage[kInChunk / 4];
  uint32_t q[kBatch];
  uint32_t qoff[kBatch];
  Tabs t;
  uint64_t pos, ssrc;
  uint32_t ev, nq, slen, nlen, ndist, ok, ticket;
};
static_assert(sizeof(InflateShared) * kWavesPerCu <= 160 * 1024, "the waves of a CU share 160 KiB of LDS");

// A store of this wave must be complete before a later load of the same bytes by another lane of
// it.  The workgroup is this one wave, so workgroup scope covers every agent involved: the fence
// waits for the wave's outstanding vector memory operations (s_waitcnt vmcnt(0)), and the CU's
// vector L1, which the wave's stores write through and its loads read, is the same for both.
__device__ __forceinline__ void own_stores_visible() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup"); }

// The window over file bytes [pos - a, pos - a + kInChunk), a < 4 so that the words are aligned
// in memory; whole words are loaded where they lie inside the file, single bytes at its edges,
// and nothing outside [gz, gz + len).
__device__ void load_stage(InflateShared& sh, uint32_t lane, const uint8_t* gz, uint64_t len, uint64_t pos,
                           BitReader& r) {
  const uint32_t a = (uint32_t)((uintptr_t)(gz + pos) & 3);
  const int64_t base = (int64_t)pos - a;
  for (uint32_t w = lane; w < kInChunk / 4; w += 64) {
    const int64_t fi = base + 4 * (int64_t)w;
    uint32_t v = 0;
    if (fi >= 0 && (uint64_t)fi + 4 <= len) {
      v = *reinterpret_cast<const uint32_t*>(gz + fi);
    } else {
      for (int k = 0; k < 4; ++k) {
        const int64_t b = fi + k;
        if (b >= 0 && (uint64_t)b < len) v |= (uint32_t)gz[b] << (8 * k);
      }
    }
    sh.stage[w] = v;
  }
  r.win = reinterpret_cast<const uint8_t*>(sh.stage);
  r.base = base;
  r.lim = std::min<uint64_t>((uint64_t)(base + (int64_t)kInChunk), len);
}

template <class H>
__device__ bool build(InflateShared& sh, H& h, const uint8_t* lens, uint32_t n, uint32_t lane) {
  huff_count(h, lens, n, lane, 64);
  __syncthreads();
  if (lane == 0) sh.ok = huff_plan(h, n);
  __syncthreads();
  const bool ok = sh.ok != 0;
  if (ok) huff_place(h, lens, n, lane, 64);
  __syncthreads();
  return ok;
}

// The queue's nq symbols to the output from byte opos on; returns the position after them.  Past
// `room` bytes are counted and neither stored nor loaded.
__device__ uint64_t carry_out(InflateShared& sh, uint32_t lane, uint32_t nq, uint8_t* out, uint64_t opos,
                              uint64_t room) {
  uint32_t e[4], off[4], sum = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t i = 4 * lane + k;
    e[k] = i < nq ? sh.q[i] : 0;
    off[k] = sum;
    sum += i < nq ? ((e[k] & kMatch) ? (e[k] & 0x1FF) : 1) : 0;
  }
  uint32_t inc = sum;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t v = __shfl_up(inc, d, 64);
    if (lane >= d) inc += v;
  }
  const uint32_t ex = inc - sum, total = __shfl(inc, 63, 64);
  for (uint32_t k = 0; k < 4; ++k) {
    const uint32_t i = 4 * lane + k;
    if (i >= nq) break;
    sh.qoff[i] = ex + off[k];
    const uint64_t at = opos + ex + off[k];
    if (!(e[k] & kMatch) && at < room) out[at] = (uint8_t)e[k];
  }
  __syncthreads();
  // a match may copy what the literals above, a stored block or the batch before stored
  own_stores_visible();
  uint64_t wlo = UINT64_MAX;  // the lowest byte a match has stored since the last fence
  for (uint32_t i = 0; i < nq && opos < room; ++i) {
    const uint32_t s = sh.q[i];
    if (!(s & kMatch)) continue;
    const uint32_t len = s & 0x1FF, dist = (s & ~kMatch) >> 9;
    const uint64_t dst = opos + sh.qoff[i];
    if (dst >= room) break;
    if (dist == 0 || dist > dst) continue;  // step() refused these already
    const uint64_t src = dst - dist;
    if (wlo != UINT64_MAX && src + std::min(dist, len) > wlo) {
      own_stores_visible();
      wlo = UINT64_MAX;
    }
    // bytes [src, dst) are final; with dist < len the copy repeats them: src + (k mod dist)
    for (uint32_t k = lane; k < len; k += 64) {
      const uint64_t at = dst + k;
      if (at < room) out[at] = out[src + (dist < len ? k % dist : k)];
    }
    if (wlo == UINT64_MAX) wlo = dst;
  }
  return opos + total;
}

__device__ void inflate_file(InflateShared& sh, uint32_t lane, const uint8_t* gz, uint64_t len, uint8_t* out,
                             uint64_t room, s3imph_gunzip_info* info) {
  Dec d;
  BitReader r;
  r.len = len;
  r.pos = 0;
  r.bb = 0;
  r.bn = 0;
  r.zn = 0;
  uint64_t opos = 0;
  load_stage(sh, lane, gz, len, 0, r);
  __syncthreads();
  for (;;) {
    if (lane == 0) {
      uint32_t nq = 0, ev;
      for (;;) {
        if (!br_ready(r)) {
          ev = kRefill;
          break;
        }
        ev = step(d, r, sh.t, sh.q, &nq, kBatch);
        if (ev != kCont) break;
      }
      sh.ev = ev;
      sh.nq = nq;
      sh.pos = r.pos;
      sh.ssrc = d.ssrc;
      sh.slen = d.slen;
      sh.nlen = d.nlen;
      sh.ndist = d.ndist;
    }
    __syncthreads();
    uint32_t ev = sh.ev;
    const uint32_t nq = sh.nq;
    if (nq) opos = carry_out(sh, lane, nq, out, opos, room);
    if (ev == kRefill) {
      load_stage(sh, lane, gz, len, sh.pos, r);
    } else if (ev == kStored) {
      const uint64_t src = sh.ssrc;  // step() checked src + slen <= len
      for (uint32_t k = lane; k < sh.slen; k += 64)
        if (opos + k < room) out[opos + k] = gz[src + k];
      opos += sh.slen;
    } else if (ev == kBuildCl || ev == kBuildFixed || ev == kBuildDyn) {
      bool ok;
      if (ev == kBuildCl) {
        ok = build(sh, sh.t.cl, sh.t.cllens, 19, lane);
      } else {
        uint32_t nl = sh.nlen, nd = sh.ndist;
        if (ev == kBuildFixed) {
          nl = 288, nd = 32;
          for (uint32_t i = lane; i < 320; i += 64) sh.t.lens[i] = fixed_len(i);
          __syncthreads();
        }
        ok = build(sh, sh.t.ll, sh.t.lens, nl, lane);
        ok = build(sh, sh.t.dd, sh.t.lens + nl, nd, lane) && ok;
      }
      if (!ok) {
        d.status = kData;
        ev = kEnd;
      }
    }
    if (ev == kEnd) {
      if (lane == 0) {
        info->out_bytes = d.fout;
        info->in_used = br_byte_pos(r);
        info->members = d.members;
        info->status = d.status == kOk && d.fout > room ? (uint32_t)kMore : d.status;
        info->crc32 = d.crc_file;
        info->reserved = 0;
      }
      __syncthreads();
      return;
    }
    __syncthreads();
  }
}

// Four waves per SIMD, kWavesPerCu per CU: 128 registers per lane, which the decode fits without scratch.
__global__ __launch_bounds__(64, kWavesPerCu / 4) void k_inflate(const uint8_t* __restrict__ gz, uint8_t* out,
                                                const GzFile* __restrict__ files,
                                                const uint32_t* __restrict__ order, uint32_t n, unsigned* ticket,
                                                s3imph_gunzip_info* info) {
  __shared__ InflateShared sh;
  const uint32_t lane = threadIdx.x;
  for (;;) {
    if (lane == 0) sh.ticket = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t tk = sh.ticket;
    __syncthreads();
    if (tk >= n) return;
    const uint32_t fi = order[tk];
    const GzFile f = files[fi];
    inflate_file(sh, lane, gz + f.in_off, f.in_len, out + f.out_off, f.room, &info[fi]);
  }
}

// The file of chunk g: the last i with chunk_start[i] <= g.
__device__ uint32_t file_of_chunk(const uint64_t* chunk_start, uint32_t n, uint64_t g) {
  uint32_t lo = 0, hi = n;  // chunk_start[lo] <= g < chunk_start[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (chunk_start[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kCrcT) void k_crc32_chunks(const uint8_t* __restrict__ out,
                                                        const GzFile* __restrict__ files,
                                                        const uint64_t* __restrict__ chunk_start, uint32_t n,
                                                        const s3imph_gunzip_info* __restrict__ info,
                                                        uint32_t* __restrict__ crcs) {
  __shared__ uint32_t T[4][256];  // slicing by four
  const uint32_t t = threadIdx.x;
  T[0][t] = crc_byte(0, t);
  __syncthreads();
  for (int k = 1; k < 4; ++k) T[k][t] = (T[k - 1][t] >> 8) ^ T[0][T[k - 1][t] & 255];
  __syncthreads();
  const uint64_t g = (uint64_t)blockIdx.x * kCrcT + t;
  if (g >= chunk_start[n]) return;
  const uint32_t fi = file_of_chunk(chunk_start, n, g);
  if (info[fi].status != kOk) return;
  const uint64_t written = std::min<uint64_t>(info[fi].out_bytes, files[fi].room);
  const uint64_t lo = (g - chunk_start[fi]) * kCrcChunk;
  if (lo >= written) return;
  const uint8_t* p = out + files[fi].out_off + lo;
  const uint8_t* end = p + std::min<uint64_t>(kCrcChunk, written - lo);
  uint32_t c = ~0u;
  for (; p < end && ((uintptr_t)p & 3); ++p) c = (c >> 8) ^ T[0][(c ^ *p) & 255];
  for (; p + 4 <= end; p += 4) {
    c ^= *reinterpret_cast<const uint32_t*>(p);
    c = T[3][c & 255] ^ T[2][(c >> 8) & 255] ^ T[1][(c >> 16) & 255] ^ T[0][c >> 24];
  }
  for (; p < end; ++p) c = (c >> 8) ^ T[0][(c ^ *p) & 255];
  crcs[g] = ~c;
}

__global__ __launch_bounds__(kCrcT) void k_crc32_fold(const GzFile* __restrict__ files,
                                                      const uint64_t* __restrict__ chunk_start, uint32_t n,
                                                      const uint32_t* __restrict__ crcs, s3imph_gunzip_info* info) {
  const uint32_t fi = blockIdx.x * kCrcT + threadIdx.x;
  if (fi >= n || info[fi].status != kOk) return;
  const uint64_t written = std::min<uint64_t>(info[fi].out_bytes, files[fi].room);
  const uint32_t xfull = crc_xpow8(kCrcChunk);
  const uint32_t* cc = crcs + chunk_start[fi];
  uint32_t c = 0;
  uint64_t done = 0;
  for (; done + kCrcChunk <= written; done += kCrcChunk) c = crc_concat(c, *cc++, xfull);
  if (done < written) c = crc_concat(c, *cc, crc_xpow8(written - done));
  if (c != info[fi].crc32) info[fi].status = kChecksum;
}

const char* status_text(uint32_t st) {
  switch (st) {
    case kEof: return "unexpected EOF";
    case kHeader: return "invalid header";
    case kData: return "corrupt input";
    case kChecksum: return "invalid checksum";
    default: return "";
  }
}

uint64_t round8(uint64_t v) { return (v + 7) & ~7ull; }

}  // namespace

uint64_t gunzip_room_hint(const uint8_t* gz, uint64_t len) {
  if (!gz || len < 18) return 0;
  uint64_t isize = 0;
  for (int k = 0; k < 4; ++k) isize |= (uint64_t)gz[len - 4 + k] << (8 * k);
  // 1032 : 1 is DEFLATE's largest expansion (258 bytes from a 1-bit length and a 1-bit distance code)
  const uint64_t most = len > (UINT64_MAX - 64) / 1032 ? UINT64_MAX : 1032 * len + 64;
  return std::min(isize, most);
}

void gunzip_files(s3imph_ctx* c, const uint8_t* d_gz, uint8_t* d_out, const GzFile* files, uint64_t n,
                  s3imph_gunzip_info* info, hipStream_t s) {
  if (n == 0) return;
  if (n >> 31) throw Fail{S3IMPH_ERR_INVALID, "2^31 files or more in one call"};
  std::vector<uint32_t> order(n);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return files[a].in_len > files[b].in_len; });
  std::vector<uint64_t> chunk_start(n + 1, 0);
  for (uint64_t i = 0; i < n; ++i) chunk_start[i + 1] = chunk_start[i] + (files[i].room + kCrcChunk - 1) / kCrcChunk;
  const uint64_t chunks = chunk_start[n];
  if ((chunks + kCrcT - 1) / kCrcT >> 31) throw Fail{S3IMPH_ERR_INVALID, "2^52 bytes of room or more in one call"};
  int cus = 0;
  HIPCHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
  DevGuard g;
  GzFile* d_files = nullptr;
  uint32_t *d_order = nullptr, *d_crcs = nullptr;
  uint64_t* d_chunk = nullptr;
  unsigned* d_ticket = nullptr;
  s3imph_gunzip_info* d_info = nullptr;
  g.make(d_files, n);
  g.make(d_order, n);
  g.make(d_chunk, n + 1);
  g.make(d_crcs, chunks);
  g.make(d_ticket, 1);
  g.make(d_info, n);
  HIPCHECK(hipMemcpyAsync(d_files, files, n * sizeof(GzFile), hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(d_order, order.data(), n * 4, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemcpyAsync(d_chunk, chunk_start.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  HIPCHECK(hipMemsetAsync(d_ticket, 0, sizeof(unsigned), s));
  HIPCHECK(hipMemsetAsync(d_info, 0, n * sizeof(s3imph_gunzip_info), s));
  const unsigned grid = (unsigned)std::min<uint64_t>(n, (uint64_t)std::max(cus, 1) * kWavesPerCu);
  k_inflate<<<grid, 64, 0, s>>>(d_gz, d_out, d_files, d_order, (uint32_t)n, d_ticket, d_info);
  HIPCHECK(hipGetLastError());
  if (chunks) {
    k_crc32_chunks<<<(unsigned)((chunks + kCrcT - 1) / kCrcT), kCrcT, 0, s>>>(d_out, d_files, d_chunk, (uint32_t)n,
                                                                              d_info, d_crcs);
    HIPCHECK(hipGetLastError());
  }
  k_crc32_fold<<<(unsigned)((n + kCrcT - 1) / kCrcT), kCrcT, 0, s>>>(d_files, d_chunk, (uint32_t)n, d_crcs, d_info);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipMemcpyAsync(info, d_info, n * sizeof(s3imph_gunzip_info), hipMemcpyDeviceToHost, s));
  HIPCHECK(hipStreamSynchronize(s));
}

int gunzip_group(s3imph_ctx* c, DevGuard& g, const uint8_t* const* gz, const uint64_t* gz_len, uint64_t lo,
                 uint64_t hi, GzTexts* t, hipStream_t s, std::string* msg) {
  const uint64_t n = hi - lo;
  t->text.assign(n, nullptr);
  t->info.assign(n, s3imph_gunzip_info{});
  t->d_gz = t->d_out = t->d_again = nullptr;
  if (n == 0) return S3IMPH_OK;
  std::vector<GzFile> files(n);
  uint64_t in_total = 0, out_total = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t room = round8(gunzip_room_hint(gz[lo + i], gz_len[lo + i]));
    files[i] = GzFile{in_total, gz_len[lo + i], out_total, room};
    in_total += gz_len[lo + i];
    out_total += room;
  }
  g.make(t->d_gz, in_total);
  g.make(t->d_out, out_total);
  for (uint64_t i = 0; i < n; ++i)
    if (files[i].in_len) staged_copy(c, true, t->d_gz + files[i].in_off, gz[lo + i], files[i].in_len);
  gunzip_files(c, t->d_gz, t->d_out, files.data(), n, t->info.data(), s);
  // the files whose trailer did not tell their size, alone, with the room the first pass counted
  std::vector<GzFile> again;
  std::vector<uint64_t> which;
  uint64_t again_total = 0;
  for (uint64_t i = 0; i < n; ++i) {
    t->text[i] = t->d_out + files[i].out_off;
    if (t->info[i].status != kMore) continue;
    const uint64_t room = round8(t->info[i].out_bytes);
    again.push_back(GzFile{files[i].in_off, files[i].in_len, again_total, room});
    which.push_back(i);
    again_total += room;
  }
  if (!again.empty()) {
    g.make(t->d_again, again_total);
    std::vector<s3imph_gunzip_info> info2(again.size());
    gunzip_files(c, t->d_gz, t->d_again, again.data(), again.size(), info2.data(), s);
    for (uint64_t k = 0; k < again.size(); ++k) {
      t->info[which[k]] = info2[k];
      t->text[which[k]] = t->d_again + again[k].out_off;
    }
  }
  g.drop(t->d_gz);
  t->d_gz = nullptr;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t st = t->info[i].status;
    if (st == kOk) continue;
    if (st == kMore) {
      *msg = "gzip: file " + std::to_string(lo + i) + ": its size changed between two passes";
      return S3IMPH_ERR_INTERNAL;
    }
    *msg = "gzip: file " + std::to_string(lo + i) + ": " + status_text(st);
    return S3IMPH_ERR_FORMAT;
  }
  return S3IMPH_OK;
}

void gunzip_group_free(DevGuard& g, GzTexts* t) {
  g.drop(t->d_gz);
  g.drop(t->d_out);
  g.drop(t->d_again);
  t->d_gz = t->d_out = t->d_again = nullptr;
}

}  // namespace s3imph

using namespace s3imph;

extern "C" {

void s3imph_gunzip_geometry(uint32_t* in_chunk_bytes, uint32_t* batch_symbols, uint32_t* waves_per_cu) {
  if (in_chunk_bytes) *in_chunk_bytes = kInChunk;
  if (batch_symbols) *batch_symbols = kBatch;
  if (waves_per_cu) *waves_per_cu = kWavesPerCu;
}

uint64_t s3imph_gunzip_room_hint(const uint8_t* gz, uint64_t len) { return gunzip_room_hint(gz, len); }

int s3imph_gunzip_device(s3imph_ctx* c, const uint8_t* d_gz, const uint64_t* gz_offsets, uint64_t n_files,
                         uint8_t* d_out, const uint64_t* out_offsets, s3imph_gunzip_info* info, void* stream) {
  if (!c) return S3IMPH_ERR_INVALID;
  if (n_files == 0) return S3IMPH_OK;
  if (!d_gz || !gz_offsets || !d_out || !out_offsets || !info || (n_files >> 31)) return S3IMPH_ERR_INVALID;
  for (uint64_t i = 0; i < n_files; ++i)
    if (gz_offsets[i + 1] < gz_offsets[i] || out_offsets[i + 1] < out_offsets[i]) return S3IMPH_ERR_INVALID;
  return device_entry(c, "gzip: ", [&](std::string& msg) {
    hipStream_t s = use_device(c->device, stream, c->own_stream);
    return retry_on_nomem(c, s, &msg, [&] {
      std::vector<GzFile> files(n_files);
      for (uint64_t i = 0; i < n_files; ++i)
        files[i] = GzFile{gz_offsets[i], gz_offsets[i + 1] - gz_offsets[i], out_offsets[i],
                          out_offsets[i + 1] - out_offsets[i]};
      gunzip_files(c, d_gz, d_out, files.data(), n_files, info, s);
      return S3IMPH_OK;
    });
  });
}

int s3imph_gunzip_host(int device, const uint8_t* const* gz, const uint64_t* gz_len, uint64_t n_files, uint8_t** out,
                       uint64_t* out_len, s3imph_gunzip_info* info, char* err, size_t errlen) {
  if (n_files && (!gz || !gz_len || !out || !out_len)) return S3IMPH_ERR_INVALID;
  for (uint64_t i = 0; i < n_files; ++i)
    if (gz_len[i] && !gz[i]) return S3IMPH_ERR_INVALID;
  for (uint64_t i = 0; i < n_files; ++i) {
    out[i] = nullptr;
    out_len[i] = 0;
  }
  if (n_files == 0) return S3IMPH_OK;
  auto drop = [&] {
    for (uint64_t i = 0; i < n_files; ++i) {
      std::free(out[i]);
      out[i] = nullptr;
      out_len[i] = 0;
    }
  };
  const int rc = host_entry(device, "gzip: ", err, errlen, [&](s3imph_ctx* c, hipStream_t s, std::string& msg) -> int {
    DevGuard g;
    GzTexts t;
    drop();  // a retry starts over
    const int rc2 = gunzip_group(c, g, gz, gz_len, 0, n_files, &t, s, &msg);
    if (info) std::memcpy(info, t.info.data(), n_files * sizeof *info);
    if (rc2 != S3IMPH_OK) return rc2;
    for (uint64_t i = 0; i < n_files; ++i) {
      const uint64_t nb = t.info[i].out_bytes;
      out[i] = host_array<uint8_t>(nb);
      out_len[i] = nb;
      if (nb) staged_copy(c, false, out[i], t.text[i], nb);
    }
    return S3IMPH_OK;
  });
  if (rc != S3IMPH_OK) drop();
  return rc;
}

}  // extern "C"
