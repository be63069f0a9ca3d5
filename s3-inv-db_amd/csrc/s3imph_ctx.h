// s3imph_ctx.h — the device context and the pieces of the build orchestration shared by
// s3imph_build.hip (single-GPU and per-rank builds, the device-side C ABI) and
// s3imph_multi.hip (multi-GPU builds behind the host-memory boundary).  Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "s3imph.h"
#include "s3imph_internal.h"

namespace s3imph {

struct Fail {
  int code;
  std::string msg;
};

#define HIPCHECK(x)                                                                           \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess)                                                                     \
      throw Fail{e_ == hipErrorOutOfMemory ? S3IMPH_ERR_NOMEM : S3IMPH_ERR_HIP,               \
                 std::string(#x) + ": " + hipGetErrorString(e_)};                             \
  } while (0)

#define NCCLCHECK(x)                                                                          \
  do {                                                                                        \
    ncclResult_t r_ = (x);                                                                    \
    if (r_ != ncclSuccess)                                                                    \
      throw Fail{S3IMPH_ERR_RCCL, std::string(#x) + ": " + ncclGetErrorString(r_)};           \
  } while (0)

template <typename T>
void dfree(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

template <typename T>
void dalloc(T*& p, uint64_t count) {
  dfree(p);
  void* v = nullptr;
  HIPCHECK(hipMalloc(&v, std::max<uint64_t>(count, 1) * sizeof(T)));
  p = static_cast<T*>(v);
}

// A scratch array of `cap` elements made at least `need` long (its contents are not kept).  The
// capacity is zeroed before the allocation, so one that throws leaves no capacity over a null
// pointer for the next call to trust.
template <typename T>
void grow(T*& p, uint64_t& cap, uint64_t need) {
  if (need <= cap) return;
  cap = 0;
  dalloc(p, need);
  cap = need;
}

// Device arrays of one call, freed when it ends (or earlier, by drop).
struct DevGuard {
  std::vector<void*> p;
  template <typename T>
  void make(T*& q, uint64_t count) {
    dalloc(q, count);
    p.push_back(q);
  }
  void drop(void* q) {
    if (!q) return;
    for (void*& x : p)
      if (x == q) {
        (void)hipFree(x);
        x = nullptr;
      }
  }
  ~DevGuard() {
    for (void* q : p)
      if (q) (void)hipFree(q);
  }
};

// Collectives of the multi-GPU build, on device buffers, ordered on stream s.
struct Comm {
  int rank = 0, nranks = 1;
  virtual ~Comm() = default;
  // d_recv[r * bytes ..) <- rank r's d_send[0 .. bytes)
  virtual void allgather(const void* d_send, void* d_recv, uint64_t bytes, hipStream_t s) = 0;
  // d_recv[0 .. bytes) <- byte-wise sum over ranks of their d_send[rank * bytes ..) (u8, mod 256)
  virtual void reduce_scatter_u8(const void* d_send, void* d_recv, uint64_t bytes, hipStream_t s) = 0;
  // element-wise u64 sum over ranks
  virtual void allreduce_u64(const unsigned long long* d_in, unsigned long long* d_out, uint64_t count,
                             hipStream_t s) = 0;
  // d_send + soff[q] (sbytes[q] bytes) -> rank q; rank q's bytes -> d_recv + roff[q] (rbytes[q]); host arrays
  virtual void alltoallv(const void* d_send, const uint64_t* soff, const uint64_t* sbytes, void* d_recv,
                         const uint64_t* roff, const uint64_t* rbytes, hipStream_t s) = 0;
  // a peer failed: make every pending and future collective of this rank return (RCCL:
  // ncclCommAbort, whose kernels then exit); the communicator is unusable afterwards
  virtual void abort() {}
  // this rank has its GPU to itself (RCCL: one rank per device); the host transports let
  // ranks share one, so no kernel of a rank may wait for all of the GPU's CUs at once
  virtual bool owns_gpu() const { return false; }
};

constexpr uint64_t kDistSwitchKeysDefault = 2ull << 20;  // levels below this run replicated

// Decomposition of the multi-GPU levels (s3imph_ctx_set_dist_mode / S3IMPH_DIST_MODE).
constexpr int kDistRoute = 0;   // records routed to the owner of their position range (s3imph_dist.hip)
constexpr int kDistBitmap = 1;  // count-lane reduction of the collision bitmap (s3imph_bitmap.hip)

struct DistState {
  Comm* comm = nullptr;
  int rank = 0, nranks = 1;
  uint64_t cap_list = 0, cap_send = 0, cap_stage_words = 0;
  Rec* send = nullptr;                       // per-owner send regions / replicated gather staging
  uint64_t* stage_bits = nullptr;            // level bit-vector all-gather staging
  unsigned long long* scnt = nullptr;        // per-owner send counts (nranks)
  unsigned long long* mat = nullptr;         // all-gathered send counts (nranks x nranks)
  unsigned long long* gslot = nullptr;       // per-level global counts (kMaxLevels + 2)
  unsigned long long* small = nullptr;       // scratch for tiny collectives (2 x 64 x 64)
  unsigned long long* h_pinned = nullptr;    // host staging (64 x 64 + 256 u64)
  std::vector<uint64_t> seg;                 // last build: (p_lo, count, local_off) triples
  uint64_t out_n = 0;
  // bitmap decomposition workspace: local A / C marks, count lanes, this rank's summed
  // slice, the gathered final bits, their word prefix and block sums
  uint64_t *bm_a = nullptr, *bm_g = nullptr, *bm_dec = nullptr;
  uint8_t *bm_lanes = nullptr, *bm_slice = nullptr, *bm_recv = nullptr;
  unsigned long long* bm_tsum = nullptr;   // per-tile totals of a level (kScatterTiles)
  unsigned long long* bm_tbase = nullptr;  // per-tile (rank, slot) bases (2 kScatterTiles)
  uint64_t bm_cap_words = 0;
  Rec* bm_out = nullptr;  // this rank's settled (p, fp, pos) triples (the tail's tile kernels own the bucket)
  uint64_t bm_cap_out = 0;
  uint32_t* bm_bnd = nullptr;  // the output merge's window bounds (launch_bm_place_merge)
  uint64_t bm_bnd_cap = 0;
  int mode = kDistRoute;
  bool strict = false;  // S3IMPH_DIST_STRICT: the bitmap decomposition may not fall back to routing
  // level 0's exchange runs on its own stream, chunk by chunk, beside the next chunk's hash
  hipStream_t xs = nullptr;
  hipEvent_t ev_route = nullptr, ev_counts = nullptr, ev_x = nullptr;
  // the bitmap decomposition's output exchange by level group (levels 0 and 1 as soon as they
  // are settled, then the rest): per group the settle's per-slice counts, gathered
  // (device + pinned mirror), the merge's run descriptors; the received entries; the exchange's
  // stream, its group events and its completion; its communicator (RCCL: split from `comm`, so
  // the exchange runs beside the next levels' collectives; null: `comm` on the build's stream)
  unsigned long long* xch = nullptr;
  unsigned long long* h_xch = nullptr;
  uint8_t* xrecv = nullptr;
  uint64_t cap_xrecv = 0;  // bytes
  hipStream_t xo = nullptr;
  hipEvent_t ev_xg[4] = {}, ev_xdone = nullptr;
  Comm* xcomm = nullptr;
  std::string agree_msg;  // message of a failure agreed inside route0_chunked
};

// RCCL over xGMI: all-to-all as grouped point-to-point send/recv (xGMI is a full mesh
// of point-to-point links, so every pair streams on its own link), all-gathers and
// all-reduces as RCCL collectives; the rank's own share is a device-to-device copy.
struct RcclComm final : Comm {
  ncclComm_t comm = nullptr;  // written once, before any collective; never reset (abort keeps it)
  std::atomic<bool> aborted{false};
  ~RcclComm() override {
    if (comm && !aborted.load()) (void)ncclCommDestroy(comm);
  }
  // Called from a failing peer's thread (s3imph_multi.hip): ncclCommAbort makes this rank's
  // pending collectives return.  The handle is left as it is — the owning rank thread may be
  // reading it — and the owning thread's next collective throws instead of enqueueing on the
  // aborted communicator (a collective already being enqueued when the abort lands fails
  // inside RCCL and throws the same way).
  void abort() override {
    bool expected = false;
    if (comm && aborted.compare_exchange_strong(expected, true)) (void)ncclCommAbort(comm);
  }
  bool owns_gpu() const override { return true; }
  void live() const {
    if (aborted.load(std::memory_order_acquire))
      throw Fail{S3IMPH_ERR_RCCL, "RCCL communicator aborted: a peer rank failed"};
  }
  void allgather(const void* d_send, void* d_recv, uint64_t bytes, hipStream_t s) override {
    live();
    NCCLCHECK(ncclAllGather(d_send, d_recv, bytes, ncclUint8, comm, s));
  }
  void reduce_scatter_u8(const void* d_send, void* d_recv, uint64_t bytes, hipStream_t s) override {
    live();
    NCCLCHECK(ncclReduceScatter(d_send, d_recv, bytes, ncclUint8, ncclSum, comm, s));
  }
  void allreduce_u64(const unsigned long long* d_in, unsigned long long* d_out, uint64_t count,
                     hipStream_t s) override {
    live();
    NCCLCHECK(ncclAllReduce(d_in, d_out, count, ncclUint64, ncclSum, comm, s));
  }
  void alltoallv(const void* d_send, const uint64_t* soff, const uint64_t* sbytes, void* d_recv,
                 const uint64_t* roff, const uint64_t* rbytes, hipStream_t s) override {
    live();
    const char* sb = static_cast<const char*>(d_send);
    char* rb = static_cast<char*>(d_recv);
    NCCLCHECK(ncclGroupStart());
    for (int q = 0; q < nranks; ++q) {
      if (q == rank) continue;
      if (sbytes[q]) NCCLCHECK(ncclSend(sb + soff[q], sbytes[q], ncclUint8, q, comm, s));
      if (rbytes[q]) NCCLCHECK(ncclRecv(rb + roff[q], rbytes[q], ncclUint8, q, comm, s));
    }
    NCCLCHECK(ncclGroupEnd());
    if (sbytes[rank])
      HIPCHECK(hipMemcpyAsync(rb + roff[rank], sb + soff[rank], sbytes[rank], hipMemcpyDeviceToDevice, s));
  }
};

// Pinned staging for host-memory builds (the Go caller's buffers are pageable):
// kStageWorkers threads, each with its own pinned chunk buffer and stream, move the
// data through pinned memory, so the CPU copies of one worker overlap the DMA of the
// others and the PCIe link runs at its pinned rate.
constexpr int kStageWorkers = 8;
constexpr int kCopyPieces = 16;  // the host build's blob H2D pieces (at most; 256 MiB or more each)
constexpr uint64_t kStageChunk = 8ull << 20;

struct Stager {
  void* pin[kStageWorkers][2] = {};  // double-buffered: one chunk in DMA while the other is copied
  hipStream_t st[kStageWorkers] = {};
  hipEvent_t ev[kStageWorkers][2] = {};
  bool ready = false;
};

}  // namespace s3imph

using s3imph::DistState;
using s3imph::LevelState;
using s3imph::Rec;
using s3imph::Stager;

namespace s3imph {
struct FinScratch;  // s3imph_finalize.hip
struct AggScratch;  // s3imph_aggregate.hip
struct SortScratch;  // s3imph_sort.hip
struct CsvScratch;  // s3imph_csv.hip
struct MergeScratch;  // s3imph_merge.hip
}

struct s3imph_ctx {
  int device = 0;
  s3imph::FinScratch* fin = nullptr;  // finalize-pass scratch (s3imph_finalize.hip), lazily made
  s3imph::AggScratch* agg = nullptr;  // aggregation scratch and the last plan (s3imph_aggregate.hip), lazily made
  s3imph::SortScratch* srt = nullptr;  // listing sort / gather scratch (s3imph_sort.hip), lazily made
  s3imph::CsvScratch* csv = nullptr;  // CSV parse scratch and the last plan (s3imph_csv.hip), lazily made
  s3imph::MergeScratch* mrg = nullptr;  // row merge scratch and the last plan (s3imph_merge.hip), lazily made
  uint32_t* mid = nullptr;            // k_mid_levels scratch (kMidScratchU32), lazily made
  Rec* split = nullptr;               // k_tile_split scratch, made for sets big enough for 2^15+ tiles
  hipStream_t own_stream = nullptr;
  std::mutex mu;

  uint64_t cap_keys = 0, cap_words = 0, cap_blocks = 0;
  uint64_t *kh = nullptr, *fp = nullptr, *bits = nullptr, *rank_base = nullptr;
  uint64_t rank_base_cap = 0;  // words of rank_base (the Lookup directory, made on first lookup)
  unsigned long long* block_sums = nullptr;
  LevelState* d_st = nullptr;
  LevelState* h_st = nullptr;
  bool rank_valid = false;                   // rank_base matches the last build

  // single-GPU binned pipeline (s3imph_binned.hip)
  Rec* bucket = nullptr;
  Rec* list[2] = {nullptr, nullptr};
  uint64_t bucket_cap = 0;                   // records in bucket / each list
  unsigned *hist = nullptr, *hoff = nullptr, *tile_start = nullptr, *scan_sums = nullptr;
  unsigned long long* flags = nullptr;
  unsigned long long* sflags = nullptr;
  unsigned* tcnt = nullptr;  // reservation-path shard fills, kResLevels x kScatterTiles x kResShards
  uint64_t res_max_keys = s3imph::kResMaxKeys;
  // reservation slots hold >= 4x a tile's mean fill, 2x on levels above kResSmallKeys
  // (full 256-block grids: every XCD shard of a slot then fills evenly)
  uint64_t res_fill = 2;
  // test knobs (S3IMPH_RES_MAX / S3IMPH_RES0 / S3IMPH_RES_FILL) that force the fallback paths:
  // res0 = 0 puts level 0 on the counted path, 2 on the reservation path whatever its fill
  int res0 = 1;  // level 0 through the reservation scatter when its tiles are large
  bool route_self = false;  // S3IMPH_DIST_ROUTE_SELF: a one-rank sharded build routes like P > 1 (tests)
  int scat_cfg = 2;         // S3IMPH_SCAT_CFG=0: the 4096-counter reservation scatter on small sets (test hook)
  // P0 level 0 (s3imph_internal.h): tile slot fills / look-back words for up to p0_tiles
  // 2^14-position tiles, super-tile slot fills; made on first use.  S3IMPH_P0=0 keeps such
  // sets on the split kernel (A/B knob).
  int p0 = 1;
  uint64_t p0_tiles = 0;
  unsigned* p0_tcnt = nullptr;
  unsigned long long* p0_flags = nullptr;
  unsigned* p0_scnt = nullptr;
  unsigned* p0_pcnt = nullptr;  // the fused hash's region fills (kH0GridHost x kMaxRanks)
  s3imph::R20* p0_sup = nullptr;  // the super-tiles' records
  uint64_t p0_sup_cap = 0;
  uint16_t* p0_x = nullptr;       // bitmap decomposition: in-tile position of each level-0 R20 slot
  uint64_t p0_x_cap = 0;
  // R20 list levels (BinBuffers::l20): on unless S3IMPH_L20=0 (A/B knob); l20_mask is the
  // last build's mask (classify_stop reads its stop level's list in that format)
  bool l20 = true;
  unsigned l20_mask = 0;
  bool bm_counts = false;   // S3IMPH_BM_LANES=counts: the bitmap decomposition sums count lanes (A/B knob)
  bool debug = false;
  bool fault_dup = false;   // S3IMPH_FAULT_DUP_REC: test hook, duplicates a record mid-build (fault_dup_record)
  unsigned long long* tile_prof = nullptr;  // debug: tile phase timestamps
  bool lds_attr_set = false;

  // staging for host-memory builds
  hipStream_t copy_stream = nullptr;  // the blob's H2D pieces (build_from_host), beside the hash
  hipEvent_t copy_evs[s3imph::kCopyPieces] = {};
  const s3imph::HashFeed* feed = nullptr;  // set for the duration of one host build
  uint8_t* s_blob = nullptr;
  uint64_t s_blob_cap = 0;
  uint64_t *s_offsets = nullptr, *s_pos = nullptr, *s_fp = nullptr, *s_posout = nullptr;
  uint64_t s_cap = 0;
  uint64_t s_pos_cap = 0;  // s_pos is made only for builds with caller positions
  Stager stager;

  bool have_build = false;
  uint64_t last_n = 0;
  s3imph_build_info info{};

  int profiling = 0;  // 0 off, 1 every stage, 2 the level-0 hash (or route) stage only
  std::vector<hipEvent_t> events;
  std::vector<std::string> ev_names;
  int ev_used = 0;
  std::vector<float> stage_ms;
  std::vector<std::string> stage_names;

  std::string last_msg;  // message of the last failed device-resident call
  bool dist = false;
  uint64_t dist_switch = s3imph::kDistSwitchKeysDefault;  // global keys below which levels run replicated
  DistState d;
};

namespace s3imph {

// The process's context for `device`, made on first use and kept: what the host-memory entry
// points run on (s3imph_build.hip).  Null with *msg set when it cannot be made.
s3imph_ctx* default_ctx(int device, std::string* msg);
// Builds (s3imph_build.hip).  Both return an s3imph_status and throw Fail on HIP/RCCL errors.
int build_single(s3imph_ctx* c, const uint8_t* blob, const uint64_t* offsets, const uint64_t* pos, uint64_t n,
                 uint64_t* fp_out, uint64_t* pos_out, hipStream_t s, s3imph_build_info* info, std::string* msg);
int build_dist(s3imph_ctx* c, const uint8_t* blob, const uint64_t* offsets, const uint64_t* pos, uint64_t n_local,
               uint64_t key_base, uint64_t* fp_out, uint64_t* pos_out, uint64_t out_cap, uint64_t* out_n,
               hipStream_t s, s3imph_build_info* info, std::string* msg);
uint64_t dist_out_cap(const s3imph_ctx* c, uint64_t n_global);
// Chunked host <-> device copy through the ctx's pinned stager (h2d: device dst <- host src;
// with `bias`, src holds u64 words stored minus bias).
// conv 1: host u64 -> device u32 (h2d), conv 2: device u32 -> host u64 (d2h), conv 3: host
// u64 offsets -> device u16 key lengths (h2d; a length past 65535 sets *wide and stops the
// copy); `bytes` are device bytes.
void staged_copy(s3imph_ctx* c, bool h2d, void* dst, const void* src, uint64_t bytes, uint64_t bias = 0,
                 int conv = 0, std::atomic<bool>* wide = nullptr);
void launch_widen32(const uint32_t* in, uint64_t* out, uint64_t n, hipStream_t s);
void launch_narrow32(const uint64_t* in, uint32_t* out, uint64_t n, hipStream_t s);
// u16 key lengths -> u64 offsets (n + 1 of them); sums: len16_scratch_words(n) words
uint64_t len16_scratch_words(uint64_t n);
void launch_len16_offsets(const uint16_t* len, uint64_t n, uint64_t* sums, uint64_t* out, hipStream_t s);
// FNV-1a of keys [0, n) into out (the error path's recount of the original key hashes)
void launch_key_hashes(const uint8_t* blob, const uint64_t* offsets, uint64_t n, uint64_t* out, hipStream_t s);
int marshal_locked(s3imph_ctx* c, uint8_t* out, uint64_t cap, uint64_t* len, std::string* msg);
void ensure_s_pos(s3imph_ctx* c, uint64_t n);
void release_multi_sets();  // s3imph_multi.hip
int release_idle_multi_sets(const void* keep);  // s3imph_multi.hip: idle sets other than `keep`
// A build that ran out of HBM: free the workspaces this process caches for OTHER builds — the
// host builds' per-device default contexts and the idle multi-GPU sets (`keep_set` excepted)
// — plus `keep`'s finalize scratch; contexts or sets another thread is building on are left
// alone.  Returns whether anything was freed (s3imph_build.hip).
bool reclaim_cached(s3imph_ctx* keep, const void* keep_set = nullptr);
// Run the build step f (returns a status, may throw Fail); when it runs out of HBM, drain the
// stream, reclaim_cached(keep) and run it once more (cached workspaces of earlier
// builds must not fail a later, larger one).
template <class F>
int retry_on_nomem(s3imph_ctx* keep, hipStream_t s, std::string* msg, F&& f) {
  int rc;
  try {
    rc = f();
  } catch (const Fail& e) {
    if (e.code != S3IMPH_ERR_NOMEM) throw;
    rc = e.code;
    *msg = e.msg;
  }
  if (rc != S3IMPH_ERR_NOMEM) return rc;
  if (s) (void)hipStreamSynchronize(s);
  (void)hipGetLastError();
  if (!reclaim_cached(keep)) return rc;
  msg->clear();
  return f();
}
// Index finalize arrays (s3imph_finalize.hip): device pass over keys in HBM, and the
// host-memory form that writes the five files.
int finalize_device(s3imph_ctx* c, const uint8_t* blob, const uint64_t* offsets, const uint32_t* depths, uint64_t n,
                    uint32_t* depth, uint64_t* subtree_end, uint32_t* max_depth_sub, uint64_t* depth_positions,
                    uint64_t* depth_offsets, uint64_t doff_cap, uint32_t* max_depth, hipStream_t s, std::string* msg);
// finalize_device with depth_offsets made here (owned by g), grown once when 64 entries are too few
int finalize_rows(s3imph_ctx* c, DevGuard& g, const uint8_t* blob, const uint64_t* offsets, const uint32_t* depths,
                  uint64_t n, uint32_t* depth, uint64_t* subtree_end, uint32_t* max_depth_sub,
                  uint64_t* depth_positions, uint64_t*& depth_offsets, uint32_t* max_depth, hipStream_t s,
                  std::string* msg);
int finalize_from_host(int device, const uint8_t* blob, const uint64_t* offsets, const uint32_t* depths, uint64_t n,
                       const std::string& dir, std::string* msg);
void fin_scratch_free(s3imph_ctx* c);
// Prefix aggregation (s3imph_aggregate.hip): plan (key pass + scans, fills *info) and fill (the
// rows of the last plan) over an object listing in HBM; both wait for the stream.
int aggregate_plan(s3imph_ctx* c, const uint8_t* keys, const uint64_t* koff, const uint64_t* sizes, uint64_t m,
                   uint32_t max_depth, s3imph_agg_info* info, hipStream_t s, std::string* msg);
int aggregate_fill(s3imph_ctx* c, uint8_t* blob, uint64_t blob_cap, uint64_t* offsets, uint32_t* depth,
                   uint64_t* ocnt, uint64_t* tbytes, uint64_t n_cap, hipStream_t s, std::string* msg);
void agg_scratch_free(s3imph_ctx* c);
// Host keys as (blob, offsets) (s3imph_aggregate.hip).  listing_given: a listing's pointers are
// there — the offsets whenever there are keys, the blob whenever the keys have bytes (a listing of
// empty keys may come with a NULL blob).  upload_keys (m > 0): the keys on the device, owned by
// g — the key bytes from koff[0] on, readable 16 bytes past their end rounded up to 8, and the
// m + 1 offsets less koff[0].
bool listing_given(const uint8_t* keys, const uint64_t* koff, uint64_t m);
void upload_keys(s3imph_ctx* c, DevGuard& g, const uint8_t* keys, const uint64_t* koff, uint64_t m,
                    uint8_t*& d_keys, uint64_t*& d_koff);
// Listing to directory (s3imph_aggregate.hip): the row path behind s3imph_index_from_objects[_tiers]_host
// (tiers nullable); with `unsorted` the listing's device copy is sorted and gathered first
// (s3imph_index_from_unsorted_objects_host).
// With `csv` the listing is not given but parsed on the device from CSV buffers (s3imph_csv.hip;
// s3imph_index_from_csv_host): keys, key_offsets, sizes, tiers and m are then ignored.
struct CsvFiles;
int index_from_objects(int device, const uint8_t* keys, const uint64_t* key_offsets, const uint64_t* sizes,
                       const uint8_t* tiers, uint64_t m, uint32_t max_depth, const char* out_dir, bool unsorted,
                       char* err, size_t errlen, const CsvFiles* csv = nullptr);
// Listing sort (s3imph_sort.hip): the byte order of m object keys in HBM (order[j] = input index
// of the j-th key, equal keys in input order; fills *info) and the out-of-place gather of the
// listing into an order; both wait for the stream.
int sort_objects(s3imph_ctx* c, const uint8_t* keys, const uint64_t* koff, uint64_t m, uint32_t* order,
                 s3imph_sort_info* info, hipStream_t s, std::string* msg);
int gather_objects(s3imph_ctx* c, const uint8_t* keys, const uint64_t* koff, const uint64_t* sizes,
                   const uint8_t* tiers, uint64_t m, const uint32_t* order, uint8_t* keys_out, uint64_t keys_cap,
                   uint64_t* off_out, uint64_t* sizes_out, uint8_t* tiers_out, hipStream_t s, std::string* msg);
void sort_scratch_free(s3imph_ctx* c);
// Inventory CSV (s3imph_csv.hip).  A lane of the automaton passes walks a run of kCsvRunBytes, a
// workgroup a tile of kCsvTileBytes (s3imph_csv_geometry tells the tests).  plan: every pass that
// sizes the listing of one buffer in HBM (fills *info, keeps the plan); fill: the plan's listing,
// its keys from byte key_base of `keys` on; both wait for the stream.
constexpr int kCsvRunBytes = 32, kCsvTileBytes = 8192;
int csv_plan(s3imph_ctx* c, const uint8_t* csv, uint64_t len, const s3imph_csv_schema& schema, s3imph_csv_info* info,
             hipStream_t s, std::string* msg);
int csv_fill(s3imph_ctx* c, uint8_t* keys, uint64_t keys_cap, uint64_t key_base, uint64_t* offsets, uint64_t* sizes,
             uint8_t* tiers, hipStream_t s, std::string* msg);
void csv_scratch_free(s3imph_ctx* c);
// Host CSV buffers to one listing in HBM, file after file (owned by g; *m objects; *total sums
// the files' infos when given).  With `gz` the buffers are gzip files, inflated on the device in
// groups of consecutive files of about group_bytes (compressed bytes plus room; 0: kGzGroupBytes).
struct CsvFiles {
  const uint8_t* const* csv;
  const uint64_t* len;
  uint64_t n_files;
  const s3imph_csv_schema* schema;
  bool with_tiers;
  s3imph_csv_info* total;
  bool gz = false;
  uint64_t group_bytes = 0;
};
// gzip (s3imph_inflate.hip).  A group's footprint in HBM beside the listing: at 8 : 1 and 4 MiB of
// text per file 2 GiB hold some 450 files, a ninth of a full grid's waves, and stay a small share
// of HBM next to the listing arrays that grow with every file.
constexpr uint64_t kGzGroupBytes = 2ull << 30;
struct GzFile {
  uint64_t in_off, in_len;  // the file's bytes in the compressed buffer
  uint64_t out_off, room;   // where its text goes, and how many bytes may be written
};
// files[i] of d_gz inflated into d_out; info: n host entries.  Waits for the stream; throws Fail.
void gunzip_files(s3imph_ctx* c, const uint8_t* d_gz, uint8_t* d_out, const GzFile* files, uint64_t n,
                  s3imph_gunzip_info* info, hipStream_t s);
uint64_t gunzip_room_hint(const uint8_t* gz, uint64_t len);
// Host gzip files [lo, hi) uploaded packed and inflated with their room hints, the files that
// needed more again with their exact room: text[i] (8-byte aligned, readable to round_up(its
// length, 8)) and info[i] per file, the buffers owned by g.  A bad file: S3IMPH_ERR_FORMAT and
// "gzip: file <i>: ..." for the lowest i.
struct GzTexts {
  std::vector<const uint8_t*> text;
  std::vector<s3imph_gunzip_info> info;
  uint8_t *d_gz = nullptr, *d_out = nullptr, *d_again = nullptr;
};
int gunzip_group(s3imph_ctx* c, DevGuard& g, const uint8_t* const* gz, const uint64_t* gz_len, uint64_t lo,
                 uint64_t hi, GzTexts* t, hipStream_t s, std::string* msg);
void gunzip_group_free(DevGuard& g, GzTexts* t);
int csv_listing(s3imph_ctx* c, DevGuard& g, const CsvFiles& f, uint8_t*& d_keys, uint64_t*& d_koff,
                uint64_t*& d_sizes, uint8_t*& d_tiers, uint64_t* m, hipStream_t s, std::string* msg);
// The prefix rows of a listing or of a merge, left in HBM (owned by a DevGuard).
struct DevRows {
  uint64_t n = 0, blob_bytes = 0;
  uint8_t* blob = nullptr;
  uint64_t *offsets = nullptr, *ocnt = nullptr, *tbytes = nullptr;
  uint32_t* depth = nullptr;
  // with tiers: S3IMPH_NUM_TIERS columns of n entries each, the present tiers
  uint64_t *tier_count = nullptr, *tier_bytes = nullptr;
  uint64_t present_mask = 0;
  uint64_t m = 0;  // objects of the listing the rows were made from
};
// H2D of a host listing, plan, fill (s3imph_aggregate.hip); with `tiers` the tier columns too,
// with `unsorted` the sort and the gather first, with `csv` the listing parsed from CSV buffers
// (`tiers` then only says whether tiers are wanted).  The listing's device copy is freed before
// returning; no object at all: out->m == 0 and no rows.
int rows_from_host(s3imph_ctx* c, DevGuard& g, const uint8_t* keys, const uint64_t* koff, const uint64_t* sizes,
                   uint64_t m, uint32_t max_depth, DevRows* out, std::string* msg, const uint8_t* tiers = nullptr,
                   bool unsorted = false, const CsvFiles* csv = nullptr);
// The back half every "rows in HBM, index directory out" path shares (s3imph_aggregate.hip):
// index_arrays_from_rows builds the MPHF over r's blob, finalizes with r's depths and brings every
// array of the directory to the host (the tier columns first, freed before the build needs the
// room); write_index_dir writes the files and the manifest (n == 0: the empty index).
struct IndexHostArrays {
  uint64_t n = 0, present_mask = 0;
  uint32_t md = 0;
  std::vector<uint8_t> mph, blob;
  std::vector<uint64_t> fp, pos, offs, send, dpos, doff, ocnt, tbytes, tcount, tcbytes;
  std::vector<uint32_t> depth, maxds;
};
int index_arrays_from_rows(s3imph_ctx* c, DevGuard& g, DevRows& r, bool tiers, IndexHostArrays& h, hipStream_t s,
                           std::string* msg);
int write_index_dir(const std::string& dir, IndexHostArrays& h, bool tiers, std::string* msg);
// Row merge (s3imph_merge.hip): plan and fill over one row set in HBM sorted in k stretches; both
// wait for the stream.
void merge_scratch_free(s3imph_ctx* c);
// A context (s3imph_ctx_create) whose multi-GPU collectives go through `comm` (owned).
s3imph_ctx* make_dist_ctx(int device, Comm* comm, int rank, int nranks, std::string* msg);

}  // namespace s3imph
