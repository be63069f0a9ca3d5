/*
 * s3imph.h — C ABI of libs3imph.so, the MI355X-native MPHF (BBHash, gamma = 2.0)
 * builder for s3-inv-db indexes.
 *
 * This ABI is the drop-in boundary for the reference's MPHF stage,
 * format.StreamingMPHFBuilder (/root/reference/pkg/format/mphf_streaming.go).
 * The reference has no FFI layer of its own (pure Go, README.md:12); its caller
 * holds the concrete type at pkg/extsort/indexbuild.go:39 and constructs it at :81.
 * Each entry point below names the reference interface it replaces (file:line).
 * INTEGRATION.md shows the cgo binding a maintainer would add.
 *
 * Conventions
 *   - Plain pointers and sizes only; no C++ exceptions cross this boundary.
 *   - Every function returns an s3imph_status (0 = OK) unless stated otherwise;
 *     when `err`/`errlen` are given, a NUL-terminated message is written there,
 *     worded like the reference's Go errors ("build MPHF: ...").
 *   - Every call selects its own HIP device (cgo may call from any OS thread).
 *   - Keys are byte strings laid out as prefix_blob.bin + prefix_offsets.u64:
 *     key i = blob[offsets[i] .. offsets[i+1]), offsets has n+1 entries.
 *   - Outputs are byte-identical to the reference's mph.bin / mph_fp.u64 /
 *     mph_pos.u64 under the restated relab/bbhash spec ("parity").
 */
#ifndef S3IMPH_H
#define S3IMPH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S3IMPH_ABI_VERSION 1

typedef enum s3imph_status {
    S3IMPH_OK = 0,
    S3IMPH_ERR_INVALID = 1,          /* bad argument / misuse */
    S3IMPH_ERR_DUP_KEY_HASH = 2,     /* duplicate FNV-1a key hashes: bbhash.New cannot place them (mphf_streaming.go:141-144) */
    S3IMPH_ERR_TOO_MANY_LEVELS = 3,  /* level budget exhausted (relab/bbhash maxLevel analogue) */
    S3IMPH_ERR_KEY_HASH_ZERO = 4,    /* a key hashes to 0: "MPHF Key(%d) returned 0" (mphf_streaming.go:248-252) */
    S3IMPH_ERR_HIP = 5,
    S3IMPH_ERR_RCCL = 6,
    S3IMPH_ERR_IO = 7,
    S3IMPH_ERR_NOMEM = 8,
    S3IMPH_ERR_FORMAT = 9,
    S3IMPH_ERR_INTERNAL = 10,
    S3IMPH_ERR_STATE = 11            /* e.g. Add after Build, use after Close */
} s3imph_status;

int s3imph_abi_version(void);
const char *s3imph_status_string(int status);

/* ------------------------------------------------------------------------
 * 1. StreamingMPHFBuilder mirror (pkg/format/mphf_streaming.go:29-232).
 *    Same method set: New(tempDir) / Add(prefix, pos) / Count() / Build(outDir) / Close().
 * ------------------------------------------------------------------------ */
typedef struct s3imph_builder s3imph_builder;

/* NewStreamingMPHFBuilder(tempDir) — mphf_streaming.go:48-64.
 * temp_dir must name an existing directory (or be NULL/""), as os.CreateTemp requires.
 * Keys are staged in host memory instead of a temp file. */
int s3imph_builder_new(const char *temp_dir, int device, s3imph_builder **out, char *err, size_t errlen);

/* Add(prefix, pos) — mphf_streaming.go:68-97. Copies the bytes. */
int s3imph_builder_add(s3imph_builder *b, const uint8_t *prefix, uint64_t len, uint64_t pos,
                       char *err, size_t errlen);

/* Batched Add (n keys in blob/offsets layout; pos may be NULL => pos_i = Count()+i).
 * Same effect as n calls of Add; exists to amortise the per-call FFI cost. */
int s3imph_builder_add_batch(s3imph_builder *b, const uint8_t *blob, const uint64_t *offsets,
                             const uint64_t *pos, uint64_t n, char *err, size_t errlen);

/* Capacity hint (no reference counterpart; the reference's IndexBuilder sizes its own
 * arrays from NewIndexBuilderWithCapacity, indexbuild.go:72-127): the device copy of the keys
 * is allocated once for n_keys keys of n_bytes key bytes, so Add never grows it.  Optional;
 * exceeding it is allowed (the buffers then grow).  A device allocation failure is not an
 * error: the build then runs from the host copy. */
int s3imph_builder_reserve(s3imph_builder *b, uint64_t n_keys, uint64_t n_bytes, char *err, size_t errlen);

/* Count() — mphf_streaming.go:100-102. */
uint64_t s3imph_builder_count(const s3imph_builder *b);

/* Build(outDir) — mphf_streaming.go:122-232: builds on the GPU and writes mph.bin,
 * mph_fp.u64, mph_pos.u64, prefix_blob.bin, prefix_offsets.u64 into out_dir.
 * Count()==0 writes the empty set (writeEmpty, :506-541). On failure mph.bin is removed (:159-168). */
int s3imph_builder_build(s3imph_builder *b, const char *out_dir, char *err, size_t errlen);

/* Build on several GPUs (s3imph_build_host_multi's num_gpus / devices / flags); the
 * default is the one device given to s3imph_builder_new.  No reference counterpart (the
 * reference builds on one CPU thread, mphf_streaming.go:141). */
int s3imph_builder_set_gpus(s3imph_builder *b, int num_gpus, const int *devices, unsigned flags);

/* Close() — mphf_streaming.go:105-114. Frees everything; b is invalid afterwards. */
int s3imph_builder_close(s3imph_builder *b);

/* ------------------------------------------------------------------------
 * 2. One-shot host-memory build: replaces bbhash.New + MarshalBinary +
 *    computeHashPositionsReverseMap + the scatter loop (mphf_streaming.go:141-204).
 * ------------------------------------------------------------------------ */

/* fp_out/pos_out: caller-allocated n entries each. *mph_bin is allocated by the
 * library (free with s3imph_free); n == 0 gives *mph_bin = NULL, *mph_len = 0.
 * pos may be NULL => pos_i = i (the production caller, indexbuild.go:160-175). */
int s3imph_build_host(int device, const uint8_t *blob, const uint64_t *offsets, const uint64_t *pos,
                      uint64_t n, uint64_t *fp_out, uint64_t *pos_out, uint8_t **mph_bin,
                      uint64_t *mph_len, char *err, size_t errlen);

/* The same build with mph.bin marshalled into the caller's buffer (mph_cap bytes, at least
 * s3imph_mph_bin_bound(n); *mph_len gets its size), which a pipeline reuses across calls as it
 * reuses fp_out / pos_out: no library allocation, no fresh pages to fault in. */
int s3imph_build_host_into(int device, const uint8_t *blob, const uint64_t *offsets, const uint64_t *pos,
                           uint64_t n, uint64_t *fp_out, uint64_t *pos_out, uint8_t *mph_out, uint64_t mph_cap,
                           uint64_t *mph_len, char *err, size_t errlen);
/* An upper bound on mph.bin's size for n keys (0 for n == 0). */
uint64_t s3imph_mph_bin_bound(uint64_t n);

void s3imph_free(void *p);

/* Free the device workspaces the host-memory builds keep between calls (the default context
 * of every device, the cached per-rank contexts of s3imph_build_host_multi); the next build
 * allocates again.  Call when no build is running (a pipeline between index builds, or
 * before handing HBM to something else).  A build that runs out of HBM does the same for the
 * caches it is not using (those no other thread is building on) and retries once before
 * returning S3IMPH_ERR_NOMEM (s3imph_build_host[_into|_multi], s3imph_builder_build,
 * s3imph_build_device, s3imph_ctx_reserve). */
int s3imph_release_workspaces(void);

/* Multi-GPU host-memory build for ONE calling process (the reference's caller is one
 * process: indexbuild.go:506-518 -> Build).  num_gpus host threads, one per GPU, each
 * run the sharded rank build of section 4 on a contiguous key shard of about equal key
 * bytes; collectives are RCCL communicators made in-process (ncclCommInitAll, xGMI) or,
 * when `devices` repeat or S3IMPH_MULTI_HOST_TRANSPORT is set, in-process host copies.
 * Each rank writes its output segments straight to their global offsets in fp_out /
 * pos_out; mph.bin comes from rank 0 (identical on every rank).  devices may be NULL
 * (GPUs 0 .. num_gpus-1).  num_gpus == 1 without S3IMPH_MULTI_FORCE_SHARDED is
 * s3imph_build_host.  Outputs equal s3imph_build_host's byte for byte. */
#define S3IMPH_MULTI_FORCE_SHARDED 1u   /* the sharded (multi-GPU) build even for one GPU */
#define S3IMPH_MULTI_HOST_TRANSPORT 2u  /* host-copy collectives instead of RCCL */
#define S3IMPH_MULTI_BITMAP 4u          /* the bitmap decomposition (s3imph_ctx_set_dist_mode) */
int s3imph_build_host_multi(int num_gpus, const int *devices, unsigned flags, const uint8_t *blob,
                            const uint64_t *offsets, const uint64_t *pos, uint64_t n, uint64_t *fp_out,
                            uint64_t *pos_out, uint8_t **mph_bin, uint64_t *mph_len, char *err, size_t errlen);

/* Emit the 5 files of the MPHF stage with the reference's framing:
 * mph.bin raw (mphf_streaming.go:152-169), mph_fp.u64 / mph_pos.u64 as S3ID
 * u64 arrays (writeArraysParallel :546-596; ArrayWriter writer.go:19-46,79-96,113-140;
 * header format.go:6-32), prefix_blob.bin + prefix_offsets.u64 with the N+1 sentinel
 * (BlobWriter writer.go:148-237). n == 0 reproduces writeEmpty (:506-541). */
int s3imph_write_index_files(const char *out_dir, const uint8_t *mph_bin, uint64_t mph_len,
                             const uint64_t *fp, const uint64_t *pos, uint64_t n,
                             const uint8_t *blob, const uint64_t *offsets, char *err, size_t errlen);

/* ------------------------------------------------------------------------
 * 3. Device-resident build (inputs already in HBM; what bench.py times).
 * ------------------------------------------------------------------------ */
typedef struct s3imph_ctx s3imph_ctx;

typedef struct s3imph_build_info {
    int32_t status;            /* s3imph_status of the build */
    uint32_t num_levels;       /* BBHash levels */
    uint64_t total_words;      /* u64 words over all level bit vectors */
    uint64_t mph_bin_len;      /* bytes of the marshalled mph.bin */
    uint64_t big_levels;       /* levels run as full-grid kernels (rest: single-workgroup tail) */
    uint64_t n_keys;           /* keys in the whole build (all ranks) */
} s3imph_build_info;

int s3imph_ctx_create(int device, s3imph_ctx **out, char *err, size_t errlen);
int s3imph_ctx_destroy(s3imph_ctx *ctx);

/* Pre-size the workspace for up to max_keys keys on this GPU (optional: builds
 * grow it on demand, but a reserved workspace keeps allocation out of timed runs). */
int s3imph_ctx_reserve(s3imph_ctx *ctx, uint64_t max_keys, uint64_t max_global_keys);

/* Enqueue the whole build on `stream` (a hipStream_t; NULL = the ctx's own stream,
 * a blocking stream, i.e. ordered after work queued on the legacy NULL stream) and
 * wait for it.  d_blob must be readable up to offsets[n] rounded up to 8 bytes and
 * may have any byte alignment (a 16-byte aligned pointer takes the LDS-staged level-0
 * hashes, any other one the per-lane hash; the outputs are the same bytes).
 * d_pos may be NULL (identity).  d_fp_out / d_pos_out: n entries each.
 * The level bit vectors stay on the device until s3imph_ctx_mph_bin(). */
int s3imph_build_device(s3imph_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets,
                        const uint64_t *d_pos, uint64_t n, uint64_t *d_fp_out, uint64_t *d_pos_out,
                        void *stream, s3imph_build_info *info);

/* Marshal the last build's level bit vectors into mph.bin bytes (D2H + framing). */
int s3imph_ctx_mph_bin(s3imph_ctx *ctx, uint8_t *out, uint64_t cap, uint64_t *len);

/* Per-stage device times of the last build (ms), recorded with HIP events on the
 * build stream when profiling is on (on = 1: every stage; on = 2: only the level-0
 * hash / route stage, two events per build).  names: comma-separated stage names. */
int s3imph_ctx_set_profiling(s3imph_ctx *ctx, int on);
int s3imph_ctx_stage_times(s3imph_ctx *ctx, float *ms, int cap, int *count, char *names, size_t names_len);

/* ------------------------------------------------------------------------
 * 4. Multi-GPU build: one process per GPU, RCCL over xGMI.  No reference
 *    counterpart (the reference builds in one process, mphf_streaming.go:141);
 *    the outputs are byte-identical to the single-GPU build.
 *
 *    Keys are sharded in contiguous index ranges.  At each large BBHash level
 *    rank r owns a contiguous range of the level's bit positions: every rank
 *    routes its active records to the owners (one all-to-all), each owner
 *    resolves collisions and ranks for its range, and its settled keys fill
 *    consecutive local output slots.  Small levels run replicated on every rank
 *    (outputs written by rank 0).  A rank's outputs are therefore a few
 *    contiguous segments of mph_fp / mph_pos (s3imph_dist_segments), which the
 *    caller writes at their global offsets (e.g. pwrite into the column files).
 * ------------------------------------------------------------------------ */

/* Rank 0 creates the 128-byte RCCL unique id; the host broadcasts it.
 * s3imph_ctx_create_dist is collective: every rank calls it with the same id.  At
 * nranks > 1 it also splits a second communicator off the first (ncclCommSplit, kept only
 * if every rank got one): the bitmap decomposition's output exchange runs on it, on its own
 * stream, beside the next levels' collectives. */
int s3imph_dist_unique_id(uint8_t id_out[128]);

int s3imph_ctx_create_dist(int device, const uint8_t id[128], int rank, int nranks,
                           s3imph_ctx **out, char *err, size_t errlen);

/* Host-callback collectives (test transport: several ranks may share one GPU).
 * allgather: recv (nranks * bytes) = every rank's send, in rank order.
 * alltoallv: send_bytes[q] bytes at send + send_off[q] go to rank q; the bytes from
 *            rank q land at recv + recv_off[q] (recv_bytes[q]).  Host pointers.
 * Each returns 0 on success. */
typedef struct s3imph_host_comm {
    void *user;
    int (*allgather)(void *user, const void *send, void *recv, uint64_t bytes);
    int (*alltoallv)(void *user, const void *send, const uint64_t *send_off, const uint64_t *send_bytes,
                     void *recv, const uint64_t *recv_off, const uint64_t *recv_bytes);
} s3imph_host_comm;

int s3imph_ctx_create_dist_host(int device, const s3imph_host_comm *comm, int rank, int nranks,
                                s3imph_ctx **out, char *err, size_t errlen);

/* Decomposition of the sharded levels (every rank of a build must choose the same; the
 * default comes from S3IMPH_DIST_MODE=route|bitmap, else route):
 *   S3IMPH_DIST_ROUTE  — position-range ownership: each level's 24-byte records are routed
 *                        to the rank owning their position range (one all-to-all per level);
 *   S3IMPH_DIST_BITMAP — the per-level collision bitmap reduced over RCCL: count lanes
 *                        (min(local count, 2), one byte per position) reduce-scattered, the
 *                        final bits all-gathered, each rank settles its own keys; one
 *                        all-to-all of the settled (p, fp, pos) at the end.  A level larger
 *                        than its host-side bound reruns the build on ROUTE.
 * Both give byte-identical outputs.  No reference counterpart (bbhash.New runs on one
 * thread, mphf_streaming.go:141).  S3IMPH_DIST_STRICT or-ed into BITMAP: no fallback — a
 * level past its size bound fails the build (S3IMPH_ERR_INTERNAL) instead of rerunning on
 * ROUTE (a benchmark of the bitmap decomposition uses it so it never times the other one); a
 * capacity miss (a reservation-slot overflow, a settle-fed level without its buffers) reruns
 * the bitmap decomposition once in its conservative form in either mode.  With one rank,
 * ROUTE is the single-GPU build (nothing to route). */
#define S3IMPH_DIST_ROUTE 0
#define S3IMPH_DIST_BITMAP 1
#define S3IMPH_DIST_STRICT 0x100
int s3imph_ctx_set_dist_mode(s3imph_ctx *ctx, int mode);

/* This rank holds keys [key_base, key_base + n_local) of the global set (the
 * shard's blob/offsets/pos, offsets relative to d_blob; d_pos NULL => pos_i =
 * key_base + i).  On return *out_n local outputs are in d_fp_out / d_pos_out
 * (capacity out_cap entries, at least s3imph_dist_out_cap()).  mph.bin is
 * identical on every rank. */
int s3imph_build_device_dist(s3imph_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets,
                             const uint64_t *d_pos, uint64_t n_local, uint64_t key_base,
                             uint64_t *d_fp_out, uint64_t *d_pos_out, uint64_t out_cap,
                             uint64_t *out_n, void *stream, s3imph_build_info *info);

/* The last build's output segments of this rank: seg[3i] = first global position p,
 * seg[3i+1] = count, seg[3i+2] = offset in d_fp_out / d_pos_out.  *count = segments. */
int s3imph_dist_segments(s3imph_ctx *ctx, uint64_t *seg, uint64_t cap, uint64_t *count);

/* Output capacity (entries) one rank needs for a build of n_global keys. */
uint64_t s3imph_dist_out_cap(s3imph_ctx *ctx, uint64_t n_global);

/* Message of the last failed device-resident build on ctx ("" if none). */
const char *s3imph_ctx_last_error(s3imph_ctx *ctx);

/* ------------------------------------------------------------------------
 * 5. Batched lookup on the device: MPHF.Lookup (pkg/format/mphf.go:275-302)
 *    over the last build's levels, for n query keys; result[i] = pos or
 *    UINT64_MAX when not found.  Self-verifies a build (VerifyMPHF, :372-393).
 * ------------------------------------------------------------------------ */
/* OpenMPHF (pkg/format/mphf.go:186-247): load a marshalled mph.bin (any builder's, e.g.
 * an index on disk) into ctx in place of its last build, so that s3imph_lookup_device
 * answers MPHF.Lookup against it.  S3IMPH_ERR_FORMAT (message: s3imph_ctx_last_error)
 * on a malformed file; len == 0 is the empty MPHF (writeEmpty's 0-byte mph.bin). */
int s3imph_ctx_load_mph_bin(s3imph_ctx *ctx, const uint8_t *mph_bin, uint64_t len);

int s3imph_lookup_device(s3imph_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets, uint64_t n,
                         const uint64_t *d_fp, const uint64_t *d_pos, uint64_t count,
                         uint64_t *d_result, void *stream);

/* ------------------------------------------------------------------------
 * 5b. The rest of IndexBuilder.Finalize (pkg/extsort/indexbuild.go:393-415,
 *     474-503; pkg/format/depthindex.go:32-96), from the same sorted prefix blob:
 *       depth.u32                 per prefix: row.Depth (indexbuild.go:185), or when
 *                                 depths == NULL the aggregator's '/' count
 *                                 (aggregator.go:44-60);
 *       subtree_end.u64           last position of the prefix's subtree (the ancestor
 *                                 stack, indexbuild.go:154-248);
 *       max_depth_in_subtree.u32  deepest depth in that subtree;
 *       depth_offsets.u64         maxDepth + 2 offsets into depth_positions;
 *       depth_positions.u64       positions grouped by depth, ascending in a depth.
 *     Positions are the Add order 0..n-1 (indexbuild.go:160).  The prefixes must be
 *     byte-sorted (the reference's Add order); the blob on the device is readable up to
 *     round_up(offsets[n], 8) as for the build, and like the build's (and the lookup's)
 *     d_blob it may have any byte alignment.
 * ------------------------------------------------------------------------ */
/* Replaces DepthIndexBuilder.Build + writeSubtreeArrays + the depth.u32 writer: computes
 * on `device` and writes the five files into out_dir (S3ID framing, format.go:25-32). */
int s3imph_finalize_index_host(int device, const uint8_t *blob, const uint64_t *offsets,
                               const uint32_t *depths, uint64_t n, const char *out_dir, char *err,
                               size_t errlen);
/* Device form: all arrays in HBM (depths nullable).  depth_offsets holds offsets_cap
 * entries; *max_depth receives maxDepth, and S3IMPH_ERR_INVALID comes back (outputs other
 * than depth undefined) when offsets_cap < maxDepth + 2.  Synchronous on `stream`. */
int s3imph_finalize_index_device(s3imph_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets,
                                 const uint32_t *d_depths, uint64_t n, uint32_t *d_depth,
                                 uint64_t *d_subtree_end, uint32_t *d_max_depth_in_subtree,
                                 uint64_t *d_depth_positions, uint64_t *d_depth_offsets,
                                 uint64_t offsets_cap, uint32_t *max_depth, void *stream);

/* ------------------------------------------------------------------------
 * 5b. manifest.json (optional part): size + SHA-256 of every index file.
 *     Replaces format.WriteManifest / VerifyManifest (pkg/format/manifest.go:33-138), which
 *     IndexBuilder.Finalize calls after the other files (indexbuild.go:429-432).  The JSON
 *     text is Go's json.MarshalIndent output (map keys sorted; created_at RFC 3339 UTC).
 *     Host-only; files are hashed in parallel, with the x86 SHA extensions when present.
 * ------------------------------------------------------------------------ */
/* WriteManifest(dir, nodeCount, maxDepth): absent index files are skipped; error text
 * "write manifest: ..." as IndexBuilder wraps it. */
int s3imph_write_manifest(const char *out_dir, uint64_t node_count, uint32_t max_depth, char *err,
                          size_t errlen);
/* ReadManifest + VerifyManifest: S3IMPH_ERR_FORMAT on a size or checksum mismatch
 * ("file %s: checksum mismatch"), S3IMPH_ERR_IO when a listed file is missing. */
int s3imph_verify_manifest(const char *dir, char *err, size_t errlen);
/* checksumFile (manifest.go:140-155): lowercase hex SHA-256 of a file into hex_out (65 B,
 * NUL-terminated); portable != 0 forces the portable compression loop (tests). */
int s3imph_sha256_file(const char *path, int portable, char hex_out[65], char *err, size_t errlen);

/* ------------------------------------------------------------------------
 * 5c. indexread.Index (pkg/indexread/index.go): an index opened on the GPU and the
 *     reader's queries answered for a whole batch per call.  The arrays of sections 1-5b
 *     live in HBM; a handle owns an internal s3imph_ctx for the MPHF levels and the
 *     rank directory (s3imph_ctx_load_mph_bin / s3imph_lookup_device).
 *
 *     The reference's Index allows concurrent readers (index.go:13-16).  Here the calls
 *     on one handle are serialised by a mutex; open several handles for concurrency.
 *     Every query call waits for its stream before it returns.
 *
 *     Differences from the reference's Open, both deliberate:
 *       - object_count.u64 and total_bytes.u64 are optional (Open requires them,
 *         index.go:46-56): only s3imph_index_from_objects_host (section 5d) writes them, the
 *         other builds leave them to the caller's aggregation.  Without them object_count / total_bytes read 0 and
 *         a non-zero filter returns S3IMPH_ERR_STATE.
       - The per-tier statistics (tiers.json + tier_stats/, section 5e) are read when present,
         as format.OpenTierStats does; Open also checks that every tier array holds Count()
         entries of width 8 and that the manifest's ids and file names are sane.
 *       - Open validates the values, not only the headers (the reference trusts the
 *         files): see s3imph_index_open.  No kernel is ever handed an index that could
 *         make it read out of bounds.
 * ------------------------------------------------------------------------ */
typedef struct s3imph_index s3imph_index;

/* Open(dir) — pkg/indexread/index.go:31-86.  Reads subtree_end.u64, depth.u32,
 * max_depth_in_subtree.u32, depth_offsets.u64, depth_positions.u64 (OpenDepthIndex,
 * depthindex.go:115-141), mph.bin, mph_fp.u64, mph_pos.u64 (OpenMPHF, mphf.go:186-247) and,
 * when both are present, object_count.u64 / total_bytes.u64; every array's S3ID header is
 * checked as OpenArray does (reader.go:81-119), plus the element width.  Error texts follow
 * the reference ("open subtree_end: ...", "open depth: ...", "open depth index: ...",
 * "open MPHF: ..."): a missing file is S3IMPH_ERR_IO, a bad header S3IMPH_ERR_FORMAT.
 * All validation happens on the host, before the device is selected or anything is
 * allocated on it.  S3IMPH_ERR_FORMAT unless, beyond the headers:
 *   - subtree_end, depth, max_depth_in_subtree, mph_fp, mph_pos (and the two stats files
 *     when present) hold the same count n, and mph.bin's levels hold n keys;
 *   - depth_offsets has at least 2 entries, starts at 0, never decreases and ends at the
 *     count of depth_positions; maxDepth = its count - 2 (depthindex.go:130-134);
 *   - every depth[i] <= maxDepth, every depth_positions[i] < n, every mph_pos[i] < n.
 * The empty index (0-byte mph.bin, count-0 arrays, depth_offsets = [0, 0]) opens with
 * Count() = 0. */
int s3imph_index_open(int device, const char *dir, s3imph_index **out, char *err, size_t errlen);

/* The same over arrays already in HBM (borrowed: they must outlive the handle), e.g. straight
 * after s3imph_build_device + s3imph_finalize_index_device.  mph_bin is host bytes
 * (s3imph_ctx_mph_bin); d_object_count / d_total_bytes are nullable (both or neither).
 * The invariants s3imph_index_open checks are taken on trust here — the caller just built
 * the arrays; only null pointers and mph.bin's framing are checked. */
typedef struct s3imph_index_arrays {
    const uint8_t *mph_bin; uint64_t mph_len;
    uint64_t n;                       /* nodes */
    const uint64_t *d_fp, *d_pos;     /* mph_fp / mph_pos */
    const uint32_t *d_depth, *d_max_depth_in_subtree;
    const uint64_t *d_subtree_end, *d_depth_offsets, *d_depth_positions;
    uint32_t max_depth;               /* depth_offsets has max_depth + 2 entries */
    const uint64_t *d_object_count, *d_total_bytes;
} s3imph_index_arrays;
int s3imph_index_attach(int device, const s3imph_index_arrays *a, s3imph_index **out, char *err, size_t errlen);

/* Close() — index.go:108-119.  idx is invalid afterwards. */
int s3imph_index_close(s3imph_index *idx);
/* Count() — index.go:188. */
uint64_t s3imph_index_count(const s3imph_index *idx);
/* MaxDepth() — index.go:193. */
uint64_t s3imph_index_max_depth(const s3imph_index *idx);
/* Message of the last failed call on idx ("" if none). */
const char *s3imph_index_last_error(s3imph_index *idx);

/* Lookup — index.go:128 (MPHF.Lookup, mphf.go:275-302): nq query keys in the blob / offsets
 * layout (d_blob readable up to offsets[nq] rounded up to 8, any byte alignment);
 * d_pos_out[i] = pos, or UINT64_MAX when not found. */
int s3imph_index_lookup_device(s3imph_index *idx, const uint8_t *d_blob, const uint64_t *d_offsets,
                               uint64_t nq, uint64_t *d_pos_out, void *stream);

/* Stats / Depth / SubtreeEnd / MaxDepthInSubtree — index.go:135-176 — for nq positions.
 * pos >= Count() (the UINT64_MAX of a failed lookup included) gives an all-zero record with
 * found = 0, as those methods return zero; lookup followed by nodes is StatsForPrefix
 * (index.go:146-152). */
typedef struct s3imph_node {
    uint64_t pos, subtree_end, object_count, total_bytes;
    uint32_t depth, max_depth_in_subtree, found, pad;
} s3imph_node;
int s3imph_index_nodes_device(s3imph_index *idx, const uint64_t *d_qpos, uint64_t nq,
                              s3imph_node *d_out, void *stream);

/* DescendantsAtDepth[Filtered] / DescendantsUpToDepth — index.go:206-297 — as a CSR over the
 * batch, in two steps: plan computes d_levels (per query, the number of result rows the
 * reference returns; 0 = nil) and d_row_ptr (n_rows + 1 entries, the exclusive prefix of the
 * row lengths; *total = row_ptr[n_rows]); fill writes the positions of the last plan, row
 * after row, into d_out[0 .. total).
 *   S3IMPH_DESC_AT:   d_rel[q] = relDepth of query q; n_rows = nq.  levels = 0 when
 *     pos >= Count(), rel < 0 or depth[pos] + rel > maxDepth (index.go:207-219), else 1 and the
 *     row holds the positions p at that depth with pos <= p <= subtree_end[pos], in order
 *     (GetPositionsInSubtree, depthindex.go:193-259); a non-zero filter keeps the p with
 *     object_count[p] >= min_count && total_bytes[p] >= min_bytes (index.go:283-295).
 *   S3IMPH_DESC_UPTO: d_rel NULL, max_rel for the whole batch; R = min(max(max_rel, 0),
 *     maxDepth) rows per query, n_rows = nq * R, row q * R + j is depth depth[pos] + 1 + j;
 *     levels[q] = min(max_depth_in_subtree[pos] - depth[pos], max_rel), or 0 when that is
 *     <= 0 or pos >= Count() (index.go:239-268); rows j >= levels[q] are empty.  A filter
 *     with UPTO is S3IMPH_ERR_INVALID.
 * plan returns S3IMPH_ERR_INVALID when row_ptr_cap < n_rows + 1 or n_rows >= 2^31; nq == 0
 * or n_rows == 0 is OK with *total = 0.  fill returns S3IMPH_ERR_INVALID when cap < total and
 * S3IMPH_ERR_STATE without a plan; a later plan replaces the earlier one. */
#define S3IMPH_DESC_AT   0
#define S3IMPH_DESC_UPTO 1
int s3imph_index_descendants_plan(s3imph_index *idx, const uint64_t *d_qpos, const int32_t *d_rel,
                                  uint64_t nq, int mode, int32_t max_rel,
                                  uint64_t min_count, uint64_t min_bytes,
                                  int32_t *d_levels /* nq */, uint64_t *d_row_ptr /* n_rows + 1 */,
                                  uint64_t row_ptr_cap, uint64_t *n_rows, uint64_t *total, void *stream);
int s3imph_index_descendants_fill(s3imph_index *idx, uint64_t *d_out, uint64_t cap, void *stream);

/* The stored prefixes in HBM — what OpenMPHF loads "for reverse lookup" (mphf.go:226-238;
 * OpenBlob, reader.go:213-229) — and the three queries over them: PrefixString (index.go:179;
 * BlobReader.Get, reader.go:250-270), MPHF.LookupWithVerify (mphf.go:306-320) and VerifyMPHF
 * (mphf.go:372-393).  Every one of them returns S3IMPH_ERR_STATE, "prefix blob not loaded"
 * (mphf.go:374), on a handle without prefixes.
 *
 * s3imph_index_open_flags: flags == 0 is s3imph_index_open.  With S3IMPH_OPEN_PREFIXES a missing
 * prefix_blob.bin opens the handle without prefixes (no error, as in OpenMPHF); a present one needs
 * prefix_offsets.u64: error texts "open MPHF: open prefix blob: open offsets: ...", a missing
 * file S3IMPH_ERR_IO, a bad S3ID header or a width other than 8 S3IMPH_ERR_FORMAT.  What the
 * reference checks per Get is checked once here, on the host before the device is selected:
 * S3IMPH_ERR_FORMAT unless the offsets hold Count() + 1 entries, never decrease and end at or
 * before the blob's size (offsets[0] != 0 and slack after the last offset are allowed).  The blob
 * goes to HBM zero-padded to round_up(size, 8) + 8 bytes, the offsets as they are.  An unknown
 * flag is S3IMPH_ERR_INVALID. */
#define S3IMPH_OPEN_PREFIXES 1
int s3imph_index_open_flags(int device, const char *dir, unsigned flags, s3imph_index **out, char *err,
                            size_t errlen);
/* The same for a handle of s3imph_index_attach: Count() + 1 offsets and the blob they index, in
 * HBM, borrowed (they must outlive the handle) and taken on trust like the other attached arrays;
 * d_blob readable up to round_up(offsets[Count()], 8).  Null pointers are S3IMPH_ERR_INVALID; a
 * second attach replaces the first (and drops a prefixes plan). */
int s3imph_index_attach_prefixes(s3imph_index *idx, const uint8_t *d_blob, const uint64_t *d_offsets);
/* 1 when the handle holds the prefix blob, else 0. */
int s3imph_index_has_prefixes(const s3imph_index *idx);

/* PrefixString — index.go:179 (MPHF.GetPrefix; BlobReader.Get, reader.go:250-270) — for nq
 * positions, in two steps like the descendants: plan writes d_out_offsets (nq + 1 entries, the
 * exclusive prefix of the lengths; *total = d_out_offsets[nq]) and, when given, d_found; fill
 * writes the rows of the last plan back to back, row q at d_out[out_offsets[q] ..], so (d_out,
 * d_out_offsets) is a key blob in the layout of s3imph_index_lookup_device.  pos >= Count() (the
 * UINT64_MAX of a failed lookup included) is a 0-byte row with found = 0 — the reference's
 * ErrBoundsCheck; "" (the root) is a 0-byte row with found = 1.
 * fill writes whole 8-byte words: cap (bytes) must be >= round_up(total, 8), the bytes past total
 * in the last word are zeros; d_out may have any alignment.  S3IMPH_ERR_INVALID when cap is too
 * small or nq >= 2^31, S3IMPH_ERR_STATE without a plan.  The handle keeps what fill needs (d_qpos
 * may be freed after plan); a later prefixes plan replaces the earlier one; a prefixes plan and a
 * descendants plan do not disturb each other.  nq == 0 is OK with *total = 0. */
int s3imph_index_prefixes_plan(s3imph_index *idx, const uint64_t *d_qpos, uint64_t nq,
                               uint64_t *d_out_offsets /* nq + 1 */, uint32_t *d_found /* nq, nullable */,
                               uint64_t *total, void *stream);
int s3imph_index_prefixes_fill(s3imph_index *idx, uint8_t *d_out, uint64_t cap, void *stream);

/* MPHF.LookupWithVerify — mphf.go:306-320: s3imph_index_lookup_device's contract, and a position
 * survives only if the stored prefix there has the query's length and bytes (mphf.go:312-317);
 * otherwise UINT64_MAX.  The one lookup that cannot return a false positive. */
int s3imph_index_lookup_verify_device(s3imph_index *idx, const uint8_t *d_blob, const uint64_t *d_offsets,
                                      uint64_t nq, uint64_t *d_pos_out, void *stream);

/* VerifyMPHF — mphf.go:372-393: every stored prefix i is looked up; *n_bad = the number of i with
 * Lookup(prefix i) != i, *first_bad the smallest of them and *first_got what the lookup gave there
 * (UINT64_MAX: "lookup failed", mphf.go:384; else "lookup returned wrong pos", mphf.go:387); both
 * are UINT64_MAX when n_bad == 0, the reference's nil.  S3IMPH_OK whenever it ran; 8 Count() bytes
 * of HBM in the handle's workspace. */
int s3imph_index_verify_device(s3imph_index *idx, uint64_t *n_bad, uint64_t *first_bad, uint64_t *first_got,
                               void *stream);

/* ------------------------------------------------------------------------
 * 5d. extsort.Aggregator + SortPrefixRows (pkg/extsort/aggregator.go:44-76, :138-) on the
 *     GPU: a byte-sorted object listing (keys in the blob / offsets layout, one size per key)
 *     becomes the prefix rows IndexBuilder.Add consumes (indexbuild.go:154-199) — prefix
 *     bytes, depth, object count, total bytes — in the reference's sorted order, and from
 *     there a whole index directory.  The keys must be in non-decreasing byte order (equal
 *     neighbours allowed); the key blob on the device is readable up to round_up(offsets[m], 8)
 *     and may have any byte alignment.  max_depth is NewAggregator's maxDepth (aggregator.go:25,
 *     :53): 0 = unlimited.  Row 0 is the root "" (aggregator.go:48) with every object; m == 0
 *     gives no rows (Drain returns nil).  Sums wrap like Go's uint64 +=.  The per-tier columns
 *     (TierCounts / TierBytes) come from the *_tiers entry points of section 5e, which sit
 *     beside the ones below; the ones below neither read nor produce them.
 * ------------------------------------------------------------------------ */
typedef struct s3imph_agg_info {
    uint64_t n_prefixes;      /* rows, the root included */
    uint64_t blob_bytes;      /* bytes of all prefixes (prefix_blob.bin's size) */
    uint64_t n_objects;       /* m: Aggregator.ObjectCount (aggregator.go:84) */
    uint64_t total_bytes;     /* sum of the sizes mod 2^64: BytesProcessed (aggregator.go:89) */
    uint64_t first_unsorted;  /* smallest i with key[i] < key[i-1]; UINT64_MAX when sorted */
    uint32_t max_depth_seen;  /* deepest row depth (after the max_depth cut) */
    uint32_t pad;
} s3imph_agg_info;

/* AddObject over the whole listing (aggregator.go:44-61), first half: one pass over the keys
 * and the scans that size the result; fills *info.  d_sizes NULL: every size is 0.
 * S3IMPH_ERR_INVALID (message: s3imph_ctx_last_error) when the keys are not sorted
 * (info->first_unsorted holds the index), when a key has more than 65535 '/' within
 * max_depth (PrefixRow.Depth is a uint16, aggregator.go:50: refused, not wrapped), or when
 * there are more than 2^30 rows (s3imph_build_device could not take them).  m == 0 is OK with
 * zero rows.  The key arrays must stay valid and unchanged until the fill that follows; a
 * later plan replaces the earlier one.  The scratch lives in ctx and grows on demand.
 * Synchronous on `stream`. */
int s3imph_aggregate_plan_device(s3imph_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_key_offsets,
                                 const uint64_t *d_sizes, uint64_t m, uint32_t max_depth,
                                 s3imph_agg_info *info, void *stream);

/* Drain + SortPrefixRows (aggregator.go:138-): writes the rows of the last plan in byte order —
 * d_blob (blob_cap >= round_up(blob_bytes, 8) bytes; the padding is written as zeros, so the
 * result goes straight into s3imph_build_device), d_offsets (n_prefixes + 1 entries), and
 * n_cap >= n_prefixes entries each of d_depth (PrefixRow.Depth), d_object_count (Count) and
 * d_total_bytes (TotalBytes).  S3IMPH_ERR_STATE without a plan, S3IMPH_ERR_INVALID when a
 * capacity is short.  Synchronous on `stream`. */
int s3imph_aggregate_fill_device(s3imph_ctx *ctx, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offsets,
                                 uint32_t *d_depth, uint64_t *d_object_count, uint64_t *d_total_bytes,
                                 uint64_t n_cap, void *stream);

/* The same from host memory (H2D, plan, fill, D2H): replaces the AddObject loop + Drain
 * (aggregator.go:44-61, :138-).  The five arrays are allocated by the library (release each
 * with s3imph_free); *n = rows.  m == 0: *n = 0, *offsets = [0], the others NULL. */
int s3imph_aggregate_host(int device, const uint8_t *keys, const uint64_t *key_offsets, const uint64_t *sizes,
                          uint64_t m, uint32_t max_depth, uint8_t **blob, uint64_t **offsets, uint32_t **depth,
                          uint64_t **object_count, uint64_t **total_bytes, uint64_t *n, char *err,
                          size_t errlen);

/* Object listing in, index directory out, in one device residency: replaces Aggregator +
 * SortPrefixRows + the IndexBuilder.Add loop + Finalize (indexbuild.go:154-199, :393-432).
 * Aggregates, runs s3imph_build_device on the produced blob and s3imph_finalize_index_device
 * with the produced depths, then writes the five MPHF-stage files, the five finalize files,
 * object_count.u64 / total_bytes.u64 (S3ID u64 arrays, the ArrayWriters of indexbuild.go:179-184)
 * and manifest.json.  The rows visit the host only to be written.  m == 0 writes the empty
 * index s3imph_index_open accepts.  Error texts are wrapped like the reference's
 * ("aggregate: ...", "build MPHF: ..."); the out-of-memory retry of the host builds applies. */
int s3imph_index_from_objects_host(int device, const uint8_t *keys, const uint64_t *key_offsets,
                                   const uint64_t *sizes, uint64_t m, uint32_t max_depth, const char *out_dir,
                                   char *err, size_t errlen);

/* ------------------------------------------------------------------------
 * 5e. Per-storage-class tier statistics, from the listing to the reader: pkg/tiers
 *     (tiers.go:16-53, :85-115, :126-170), PrefixStats.Add's TierCounts / TierBytes
 *     (extsort/types.go:200-205), IndexBuilder.writeTierStats / writeTierManifest
 *     (indexbuild.go:251-314, :521-533), format.OpenTierStats / GetBreakdown[All]
 *     (tierstats.go:108-215) and Index.HasTierData / TierBreakdown* (indexread/index.go:360-399).
 *
 *     A tier id is a uint8_t below S3IMPH_NUM_TIERS.  Per prefix row and tier t:
 *     count[t] = objects of tier t under the prefix, bytes[t] = the sum of their sizes
 *     (mod 2^64).  A tier is PRESENT when some object has it (a size-0 object counts).
 *
 *     Files: for each present tier, in ascending id order, tier_stats/<file>_count.u64 and
 *     tier_stats/<file>_bytes.u64 (S3ID u64 arrays of n entries), then tiers.json as
 *     json.MarshalIndent(TierManifest, "", "  ") writes it ({"tiers": [{"id", "name", "file"}]},
 *     no trailing newline).  The reference lists the present tiers in Go map order, which is
 *     random; ascending id is this library's deterministic choice.  Without a present tier
 *     (m == 0) neither tier_stats/ nor tiers.json is written.  manifest.json does not list the
 *     tier files (WriteManifest hashes a fixed list, manifest.go:43-56).
 * ------------------------------------------------------------------------ */
#define S3IMPH_NUM_TIERS 12
#define S3IMPH_TIER_STANDARD 0
#define S3IMPH_TIER_STANDARD_IA 1
#define S3IMPH_TIER_ONEZONE_IA 2
#define S3IMPH_TIER_GLACIER_IR 3
#define S3IMPH_TIER_GLACIER_FR 4
#define S3IMPH_TIER_DEEP_ARCHIVE 5
#define S3IMPH_TIER_REDUCED_REDUNDANCY 6
#define S3IMPH_TIER_IT_FREQUENT 7
#define S3IMPH_TIER_IT_INFREQUENT 8
#define S3IMPH_TIER_IT_ARCHIVE_INSTANT 9
#define S3IMPH_TIER_IT_ARCHIVE 10
#define S3IMPH_TIER_IT_DEEP_ARCHIVE 11

/* Mapping.FromS3 (tiers.go:85-115): both arguments trimmed of white space and upper-cased
 * (NULL = ""); INTELLIGENT_TIERING takes its tier from access_tier (FREQUENT when that is
 * missing or unknown); an unknown storage class is STANDARD.  White space is the ASCII set
 * (\t \n \v \f \r and space), the library's one trim rule; the reference's strings.TrimSpace
 * also trims Unicode white space, which S3 does not write.  The CSV parse of section 5g applies
 * the same function on the device, per record. */
int s3imph_tier_from_s3(const char *storage_class, const char *access_tier);
/* Info.Name ("STANDARD", "GLACIER", ...) and Info.FilePrefix ("standard", "glacier_fr", ...) of
 * tiers.go:39-53; NULL for id >= S3IMPH_NUM_TIERS. */
const char *s3imph_tier_name(int id);
const char *s3imph_tier_file(int id);

typedef struct s3imph_agg_tier_info {
    uint64_t present_mask;    /* bit t set iff some object has tier t (presentTiers) */
    uint64_t first_bad_tier;  /* smallest i with d_tiers[i] >= S3IMPH_NUM_TIERS; UINT64_MAX when none */
} s3imph_agg_tier_info;

/* s3imph_aggregate_plan_device plus the tier pass over d_tiers (m tier ids, one per object):
 * fills *tier_info as well.  A tier id >= S3IMPH_NUM_TIERS is S3IMPH_ERR_INVALID with the index
 * in the message (in Go it would index past [MaxTiers]uint64 and panic; here it is refused) and
 * leaves no plan.  d_tiers and d_sizes, like the keys, must stay valid and unchanged until
 * s3imph_aggregate_fill_tiers_device has run.  Scratch: 192 / 64 = 3 bytes per object and
 * 16 bytes per row on top of the plain plan's. */
int s3imph_aggregate_plan_tiers_device(s3imph_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_key_offsets,
                                       const uint64_t *d_sizes, const uint8_t *d_tiers, uint64_t m,
                                       uint32_t max_depth, s3imph_agg_info *info,
                                       s3imph_agg_tier_info *tier_info, void *stream);

/* The tier columns of the last plan's rows, after s3imph_aggregate_fill_device of that plan:
 * S3IMPH_NUM_TIERS columns each of TierCounts and TierBytes, column t starting at element
 * t * n_cap, its first n_prefixes entries valid, in row order; the columns of absent tiers are
 * zeros.  d_sizes was NULL: the byte columns are zeros.  S3IMPH_ERR_STATE after a plan made
 * without tiers or before the fill, S3IMPH_ERR_INVALID when n_cap < n_prefixes.  Synchronous on
 * `stream`. */
int s3imph_aggregate_fill_tiers_device(s3imph_ctx *ctx, uint64_t *d_tier_count, uint64_t *d_tier_bytes,
                                       uint64_t n_cap, void *stream);

/* s3imph_aggregate_host with `tiers` (m ids) in and, beside its five arrays, *tier_count and
 * *tier_bytes out (S3IMPH_NUM_TIERS x *n u64 each, column t at t * *n; release with s3imph_free)
 * and *present_mask.  m == 0: both NULL, mask 0. */
int s3imph_aggregate_tiers_host(int device, const uint8_t *keys, const uint64_t *key_offsets, const uint64_t *sizes,
                                const uint8_t *tiers, uint64_t m, uint32_t max_depth, uint8_t **blob,
                                uint64_t **offsets, uint32_t **depth, uint64_t **object_count,
                                uint64_t **total_bytes, uint64_t **tier_count, uint64_t **tier_bytes,
                                uint64_t *present_mask, uint64_t *n, char *err, size_t errlen);

/* s3imph_index_from_objects_host plus the tier files described above. */
int s3imph_index_from_objects_tiers_host(int device, const uint8_t *keys, const uint64_t *key_offsets,
                                         const uint64_t *sizes, const uint8_t *tiers, uint64_t m,
                                         uint32_t max_depth, const char *out_dir, char *err, size_t errlen);

/* The writer alone (host-only): tier_stats/ and tiers.json for the tiers of present_mask from
 * column-major host arrays (column t at t * stride, n entries). */
int s3imph_write_tier_files(const char *out_dir, uint64_t present_mask, const uint64_t *tier_count,
                            const uint64_t *tier_bytes, uint64_t n, uint64_t stride, char *err, size_t errlen);

/* Reader.  s3imph_index_open does what OpenTierStats does: no tiers.json, or an empty "tiers"
 * list, is an index without tier data; otherwise both arrays of every listed tier are opened
 * through the manifest's "file" field, in the manifest's order (GetBreakdown iterates it, so a
 * reference-built index answers in its own order).  Error texts follow the reference:
 * "open tier stats: read tier manifest: parse tier manifest: ...", "open tier stats: open <NAME>
 * bytes: ...", "open tier stats: open <NAME> counts: ...".  Tightenings (S3IMPH_ERR_FORMAT): an
 * array whose count is not Count() or whose width is not 8, a duplicate id, an id >=
 * S3IMPH_NUM_TIERS, a "file" containing '/' or "..".  All on the host, before the device.
 * In HBM the columns are interleaved by position, [n][2 T] u64 (count, bytes per manifest slot):
 * one position's breakdown is one contiguous run of at most 192 bytes. */

/* Tier data for a handle of s3imph_index_attach: T tiers with the given ids, taken from the
 * column-major device arrays s3imph_aggregate_fill_tiers_device wrote (column ids[s] at
 * ids[s] * stride).  The handle copies what it needs; the arrays need not outlive the call.
 * T == 0 removes the tier data.  S3IMPH_ERR_INVALID for T > 12, a duplicate id or an id >= 12. */
int s3imph_index_attach_tiers(s3imph_index *idx, const uint8_t *ids, uint64_t T, const uint64_t *d_tier_count,
                              const uint64_t *d_tier_bytes, uint64_t stride);
/* len(PresentTiers()): 0 without tier data (HasTierData() false) — tierstats.go:217-228. */
uint64_t s3imph_index_tier_count(const s3imph_index *idx);
/* The ids in manifest order into ids[0 .. min(cap, T)); returns T. */
uint64_t s3imph_index_tier_ids(const s3imph_index *idx, uint8_t *ids, uint64_t cap);
/* TierBreakdownAll / TierBreakdown (index.go:368-392; GetBreakdownAll / GetBreakdown,
 * tierstats.go:157-215) for nq positions: d_out is nq x 2T u64, query q slot s holding the
 * count at [q * 2T + 2s] and the bytes at [q * 2T + 2s + 1] (TierBreakdownAll); bit s of
 * d_mask[q] (uint32_t, nq entries) is set iff either is non-zero — the set bits in slot order
 * are TierBreakdown.  pos >= Count() (the UINT64_MAX of a failed lookup included) gives zeros
 * and mask 0; T == 0 returns S3IMPH_OK and writes nothing.  s3imph_index_lookup_device followed
 * by this is TierBreakdownForPrefix (index.go:394-399). */
int s3imph_index_tiers_device(s3imph_index *idx, const uint64_t *d_qpos, uint64_t nq, uint64_t *d_out,
                              uint32_t *d_mask, void *stream);

/* ------------------------------------------------------------------------
 * 5f. An object listing in ANY order: the order the reference makes after the fact.
 *     Aggregator.AddObject (pkg/extsort/aggregator.go:44-76) accumulates into a map in whatever
 *     order the objects arrive, and SortPrefixRows (pkg/extsort/types.go:160-164) sorts
 *     afterwards; section 5d instead wants the listing byte-sorted.  The entry points below make
 *     that order on the GPU, so an S3 inventory (which is not sorted by key) needs no host sort.
 *
 *     Order: keys compare as unsigned bytes and a proper prefix comes before its extensions —
 *     Go's string <, what sort.Slice in SortPrefixRows uses; embedded 0x00 and bytes >= 0x80 are
 *     ordinary bytes.  The sort is stable: equal keys keep their input order.
 *     The input contract is section 5d's: the key blob on the device is readable up to
 *     round_up(offsets[m], 8), may have any byte alignment, and offsets[0] need not be 0.
 *     m >= 2^32 is S3IMPH_ERR_INVALID before any device work (the order is a uint32_t); null
 *     arguments likewise.  m == 0 is OK everywhere (no order, offsets_out = [0]); m == 1 is
 *     the identity.
 *
 *     Memory: the sort's scratch lives in ctx, grows on demand and is 48 bytes per object (two
 *     packed and two word buffers, a scan, the positions, two segment tables) plus the radix
 *     sort's temporary; a listing found sorted takes none.  The gather is out of place: the
 *     input and the output listing — keys, offsets, sizes, tiers — coexist in HBM, so the
 *     listing's footprint is doubled until the caller frees the input.
 * ------------------------------------------------------------------------ */
typedef struct s3imph_sort_info {
    uint64_t n_objects;       /* m */
    uint64_t key_bytes;       /* offsets[m] - offsets[0] */
    uint64_t first_unsorted;  /* of the INPUT, as in s3imph_agg_info; UINT64_MAX: it was sorted, order = identity */
    uint64_t n_equal;         /* sorted neighbours holding equal keys */
    uint32_t rounds;          /* refinement rounds run (0 for sorted input); reported, not contractual */
    uint32_t pad;
} s3imph_sort_info;           /* 40 bytes */

/* The order SortPrefixRows' comparison gives the object keys (aggregator.go:44-76 takes them in
 * any order, types.go:160-164 sorts): d_order[j] (m entries) = the input index of the j-th key
 * in sorted order; fills *info.  Sorted input is found by a first pass and answered with the
 * identity.  Message of a failure: s3imph_ctx_last_error ("sort: ...").  Synchronous on `stream`. */
int s3imph_sort_objects_device(s3imph_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_key_offsets,
                               uint64_t m, uint32_t *d_order, s3imph_sort_info *info, void *stream);

/* The listing put into the order d_order (aggregator.go:44-76, types.go:160-164: what the
 * reference's map + sort leave): d_keys_out (keys_cap >= round_up(key_bytes, 8) bytes, else
 * S3IMPH_ERR_INVALID; the padding is written as zeros), d_offsets_out (m + 1 entries, starting
 * at 0), d_sizes_out and d_tiers_out (m entries each).  d_sizes and d_sizes_out may both be
 * NULL, d_tiers and d_tiers_out likewise; one of a pair without the other is S3IMPH_ERR_INVALID,
 * as is an order entry >= m.  The outputs go straight into s3imph_aggregate_plan[_tiers]_device.
 * Synchronous on `stream`. */
int s3imph_gather_objects_device(s3imph_ctx *ctx, const uint8_t *d_keys, const uint64_t *d_key_offsets,
                                 const uint64_t *d_sizes, const uint8_t *d_tiers, uint64_t m,
                                 const uint32_t *d_order, uint8_t *d_keys_out, uint64_t keys_cap,
                                 uint64_t *d_offsets_out, uint64_t *d_sizes_out, uint8_t *d_tiers_out, void *stream);

/* The same order from host memory (H2D, sort, D2H; aggregator.go:44-76, types.go:160-164):
 * *order is allocated by the library (m entries; release with s3imph_free), NULL for m == 0,
 * which touches no device. */
int s3imph_sort_objects_host(int device, const uint8_t *keys, const uint64_t *key_offsets, uint64_t m,
                             uint32_t **order, s3imph_sort_info *info, char *err, size_t errlen);

/* s3imph_index_from_objects_host for a listing in any order (aggregator.go:44-76,
 * types.go:160-164): H2D, sort, gather, the unsorted copy freed, then exactly the row path of
 * s3imph_index_from_objects_host — s3imph_index_from_objects_tiers_host's when tiers is given
 * (NULL: no tier files).  The directory is the one those write for the same listing sorted
 * stably beforehand.  A missing out_dir is S3IMPH_ERR_IO before the device is selected; the
 * out-of-memory retry of the host builds applies; failures of the sort are worded "sort: ...". */
int s3imph_index_from_unsorted_objects_host(int device, const uint8_t *keys, const uint64_t *key_offsets,
                                            const uint64_t *sizes, const uint8_t *tiers, uint64_t m,
                                            uint32_t max_depth, const char *out_dir, char *err, size_t errlen);

/* ------------------------------------------------------------------------
 * 5g. S3 inventory CSV text -> the object listing of sections 5d / 5f, on the GPU: what
 *     pkg/inventory's CSVReader.Read (reader.go:250-297) and csvInventoryReader.Next
 *     (unified.go:121-161) return, record for record and in file order — the key blob, m + 1
 *     offsets, the sizes and the tier ids, ready for s3imph_sort_objects_device and
 *     s3imph_aggregate_plan[_tiers]_device.  The input is decompressed CSV bytes, usually
 *     without a header row (an S3 inventory has none; its manifest's fileSchema names the columns).
 *
 *     Parity is "vs restated spec", as for mph.bin (DESIGN.md sections 2 and 4.5d): Go's
 *     encoding/csv is restated, not linked.  The restatement is csv.Reader.readRecord with
 *     Comma = ',', no comment character, LazyQuotes = true, TrimLeadingSpace = false and
 *     FieldsPerRecord = -1:
 *       1. A '\r' is deleted when the next byte is '\n' or when it is the buffer's last byte
 *          (readLine's CRLF rule), inside quoted fields too; any other '\r' is data.
 *       2. Five states over the bytes left — R record start, F field start after a comma, U in
 *          an unquoted field, Q in a quoted field, E in a quoted field just after a '"':
 *            state  '"'            ','             '\n'                      other byte c
 *            R      -> Q           end field -> F  -> R (empty line)         emit c -> U
 *            F      -> Q           end field -> F  end field + record -> R   emit c -> U
 *            U      emit '"' -> U  end field -> F  end field + record -> R   emit c -> U
 *            Q      -> E           emit -> Q       emit -> Q                 emit c -> Q
 *            E      emit '"' -> Q  end field -> F  end field + record -> R   emit '"', c -> Q
 *          The end of the buffer in any state but R ends the field and the record.  Every byte
 *          string parses; there is no error.
 *       3. Per record: dropped when it has <= key_col or <= size_col fields (n_short), or an
 *          empty key field (n_empty_key).  The key is the field's emitted bytes, unchanged: no
 *          URL decoding, no UTF-8 validation, 0x00 and bytes >= 0x80 are ordinary.  The size is
 *          the field trimmed of white space at both ends, which must then be one or more ASCII
 *          digits of value <= 2^64 - 1 (strconv.ParseUint base 10: no sign, no '_', not empty,
 *          leading zeros allowed); anything else is size 0 (n_bad_size counts the kept records
 *          where that happened).  The tier is s3imph_tier_from_s3(storage, access_tier) on the
 *          two fields; a column that is -1 or beyond the record's fields gives "".
 *     White space is the ASCII set of s3imph_tier_from_s3 — one rule for tier names, header
 *     names and sizes; the reference trims Unicode white space as well.
 *
 *     Out of scope: Parquet, a listing larger than one GPU's memory, the multi-GPU builds
 *     (gzip files: section 5j).
 *
 *     Memory: the scratch lives in ctx, grows on demand and is released by
 *     s3imph_release_workspaces: 1/16 byte per input byte (a 2-byte state map per 32-byte run; 11
 *     bytes per 8 KiB tile besides), 41 bytes per record (its end, two scans, the key's source,
 *     the size: 5 x 8; the tier: 1) and 8 bytes per object during the fill, plus the scans'
 *     temporary.  A record far longer than a tile — only an unbalanced quote makes one — is walked
 *     by one lane: correct, and slow.
 * ------------------------------------------------------------------------ */
typedef struct s3imph_csv_schema {
    int32_t key_col, size_col, storage_col, access_tier_col;  /* the last two may be -1 */
} s3imph_csv_schema;

typedef struct s3imph_csv_info {
    uint64_t n_records;    /* records read (csv.Reader.Read calls that returned one) */
    uint64_t n_objects;    /* records kept: the listing's m */
    uint64_t key_bytes;    /* bytes of their keys */
    uint64_t n_short;      /* dropped: too few fields (reader.go:261) */
    uint64_t n_empty_key;  /* dropped: empty key (reader.go:267) */
    uint64_t n_bad_size;   /* kept with size 0 because the size did not parse (reader.go:273-276) */
} s3imph_csv_info;         /* 48 bytes */

/* The header row (OpenFileWithOptions, reader.go:96-135), host only: parses the first record by
 * the rules above and matches "key", "size", "storageclass", "intelligenttieringaccesstier"
 * against each field trimmed and ASCII-lower-cased; the last match wins; columns not found are
 * -1.  *data_start = the byte offset where the data rows begin (pass csv + *data_start on).
 * S3IMPH_ERR_FORMAT with "CSV header missing 'Key' column" / "CSV header missing 'Size' column"
 * (ErrNoKeyColumn / ErrNoSizeColumn) or, for a buffer without a record, "read CSV header: EOF". */
int s3imph_csv_header_schema(const uint8_t *csv, uint64_t len, s3imph_csv_schema *schema,
                             uint64_t *data_start, char *err, size_t errlen);

/* Every pass needed to know n_objects and key_bytes of one CSV buffer in HBM; fills *info and
 * keeps the plan in ctx (a later plan replaces it), as the aggregate plan is kept.  d_csv may
 * have any byte alignment and is readable up to round_up(len, 8) from its start; it must stay
 * valid and unchanged until the fill.  len == 0 is OK with zeros in *info.  Null arguments,
 * key_col < 0 or size_col < 0 are S3IMPH_ERR_INVALID before any device work; n_objects >= 2^32
 * is S3IMPH_ERR_INVALID (the listing sort's limit; message: s3imph_ctx_last_error, "csv: ...")
 * and leaves no plan.  Synchronous on `stream`. */
int s3imph_csv_plan_device(s3imph_ctx *ctx, const uint8_t *d_csv, uint64_t len,
                           const s3imph_csv_schema *schema, s3imph_csv_info *info, void *stream);

/* The plan's objects: the key bytes at d_keys + key_base, n_objects + 1 offsets in
 * d_key_offsets starting at key_base, n_objects entries of d_sizes and d_tiers (d_tiers NULL:
 * no tiers).  key_base != 0 appends file after file into one listing: the next file's offsets
 * pointer is d_key_offsets + n_objects and its key_base the last offset written.  The bytes from
 * key_base + key_bytes up to round_up(key_base + key_bytes, 8) are written as zeros, bytes below
 * key_base are left alone; keys_cap (bytes of d_keys from its start) below that rounded end is
 * S3IMPH_ERR_INVALID.  S3IMPH_ERR_STATE without a plan.  The plan stays: a fill may be repeated.
 * Synchronous on `stream`. */
int s3imph_csv_fill_device(s3imph_ctx *ctx, uint8_t *d_keys, uint64_t keys_cap, uint64_t key_base,
                           uint64_t *d_key_offsets, uint64_t *d_sizes, uint8_t *d_tiers, void *stream);

/* The same from host memory (H2D, plan, fill, D2H): replaces the CSVReader.Read loop.  The four
 * arrays are allocated by the library (release each with s3imph_free); the offsets start at 0.
 * No object: *key_offsets = [0] and the others NULL or empty; len == 0 touches no device. */
int s3imph_csv_parse_host(int device, const uint8_t *csv, uint64_t len, const s3imph_csv_schema *schema,
                          uint8_t **keys, uint64_t **key_offsets, uint64_t **sizes, uint8_t **tiers,
                          s3imph_csv_info *info, char *err, size_t errlen);

/* CSV buffers in, index directory out.  Each buffer is parsed on its own — state R at its start,
 * the end of the buffer at its end, so a lone quote in one file never swallows the next — and the
 * buffers' objects are appended in order into one listing on the device (each buffer's device
 * copy is freed after its fill).  From there exactly the path of
 * s3imph_index_from_unsorted_objects_host, in the same device residency; with_tiers != 0 writes
 * the tier files of section 5e.  *info_total (nullable) sums the buffers' infos.  A missing
 * out_dir is S3IMPH_ERR_IO before the device is selected; the out-of-memory retry of the host
 * builds applies; failures of the parse are worded "csv: ...". */
int s3imph_index_from_csv_host(int device, const uint8_t *const *csv, const uint64_t *csv_len,
                               uint64_t n_files, const s3imph_csv_schema *schema, int with_tiers,
                               uint32_t max_depth, const char *out_dir, s3imph_csv_info *info_total,
                               char *err, size_t errlen);

/* The automaton passes' geometry, for tests that place events on the edges: a lane walks a run of
 * *run_bytes, a workgroup a tile of *tile_bytes. */
void s3imph_csv_geometry(uint32_t *run_bytes, uint32_t *tile_bytes);

/* ------------------------------------------------------------------------
 * 5h. The monthly storage cost of a position, and descendant rows ranked by it: what the
 *     reference's `query --estimate-cost` does with an opened index — TierBreakdown(pos) fed into
 *     pricing.ComputeMonthlyCost (internal/cli/cli.go:227-296, pkg/pricing/pricing.go:159-240) —
 *     for a batch of positions on the GPU, and on top of it the rows of a descendants plan
 *     (section 5c) cut to their k largest by cost, bytes or object count.
 *
 *     The rule per tier slot (id, count, bytes) of a breakdown, restating ComputeMonthlyCost.  All
 *     floating point is IEEE binary64 in exactly this operation order, u64 -> f64 rounds to nearest,
 *     u64(x) truncates toward zero, every u64 sum and product wraps:
 *       an unpriced tier (bit id of priced_mask clear) is skipped;
 *       storage = u64((f64(bytes) / 2^30) * price * 1e6);
 *       avg = count ? bytes / count : 0;
 *       id in {STANDARD_IA, ONEZONE_IA, GLACIER_IR} and 0 < avg < 131072:
 *         penalty = u64((f64((131072 - avg) * count) / 2^30) * price * 1e6);
 *       id one of the five IT_* and monitoring_per_1000_objects > 0:
 *         mon = avg >= 131072 ? count : (avg > 0 ? count / 2 : 0);
 *         mon > 0: monitoring += u64(f64(mon) / 1000.0 * monitoring_per_1000_objects * 1e6);
 *       id in {GLACIER_FR, DEEP_ARCHIVE, IT_ARCHIVE, IT_DEEP_ARCHIVE} and count > 0:
 *         overhead = u64((f64(count * 32768) / 2^30) * price * 1e6)
 *                  + u64((f64(count * 8192) / 2^30) * standard_price_per_gb * 1e6);
 *       per_tier[id] = storage + penalty + overhead; total += per_tier[id];
 *     and at the end total += monitoring.  The host entry point and the kernel share one inline
 *     function for this (csrc/s3imph_pricing.h).
 *
 *     Differences from the reference, deliberate:
 *       - a double that is NaN or >= 2^64 converts to UINT64_MAX (Go leaves that conversion to the
 *         implementation);
 *       - a table with a negative, NaN or infinite price, fee or standard price is
 *         S3IMPH_ERR_INVALID ("pricing: ..."), refused before any device work; the loader refuses a
 *         negative value as S3IMPH_ERR_FORMAT;
 *       - tiers are keyed by id: PerGBMonth's name of id t is s3imph_tier_name(t); names in a
 *         price file that are none of the twelve are ignored (no breakdown can carry them);
 *       - a table without a priced tier is saved with "per_gb_month": {} (Go writes null for a
 *         nil map and {} for an empty one; the struct does not tell them apart).
 * ------------------------------------------------------------------------ */
typedef struct s3imph_price_table {
    double   per_gb_month[S3IMPH_NUM_TIERS];   /* by tier id */
    uint32_t priced_mask, pad;                 /* bit t: PerGBMonth has that name */
    double   monitoring_per_1000_objects, standard_price_per_gb;
} s3imph_price_table;                          /* 120 bytes */

typedef struct s3imph_cost {
    uint64_t total, monitoring, min_object_size, glacier_overhead;  /* CostResult's four, microdollars */
    uint64_t per_tier[S3IMPH_NUM_TIERS];       /* PerTierMicrodollars by tier id, 0 where absent */
    uint32_t tier_mask;                        /* bit t: the map has the key = tier t is priced AND in TierBreakdown(pos) (count | bytes != 0) */
    uint32_t found;                            /* pos < Count() */
} s3imph_cost;                                 /* 136 bytes */

/* DefaultUSEast1Prices (pricing.go:67-93). */
int s3imph_price_table_default(s3imph_price_table *pt);
/* LoadPriceTable (pricing.go:96-108), host only.  Field names match without regard to case, map
 * keys exactly; missing fields are 0 / empty, unknown fields are skipped.  A missing file is
 * S3IMPH_ERR_IO ("read price table: ..."); malformed or wrongly shaped JSON, a number outside
 * double's range or a negative value is S3IMPH_ERR_FORMAT ("parse price table: ..."). */
int s3imph_price_table_load(const char *path, s3imph_price_table *pt, char *err, size_t errlen);
/* SavePriceTable (pricing.go:111-122): the text json.MarshalIndent(pt, "", "  ") writes —
 * per_gb_month (the priced tiers, keys in byte order), monitoring_per_1000_objects,
 * standard_price_per_gb; numbers in shortest round-trip form, plain notation for decimal
 * exponents in [-6, 21), else Go's e form; no trailing newline; mode 0644. */
int s3imph_price_table_save(const char *path, const s3imph_price_table *pt, char *err, size_t errlen);
/* ComputeMonthlyCost over a TierBreakdownAll-shaped input (T slots: ids, count, bytes), host only;
 * found = 1.  S3IMPH_ERR_INVALID for T > 12, an id >= 12, a duplicate id or a refused table. */
int s3imph_compute_monthly_cost(const uint8_t *ids, const uint64_t *count, const uint64_t *bytes, uint64_t T,
                                const s3imph_price_table *pt, s3imph_cost *out);
/* The batched TierBreakdown(pos) -> ComputeMonthlyCost: one record per position into d_out (nq
 * entries, 8-byte aligned).  pos >= Count() (the UINT64_MAX of a failed lookup included) gives an
 * all-zero record; an index without tier data gives S3IMPH_OK and records that are zero apart
 * from `found`; nq == 0 is OK and touches nothing.  d_qpos may be the d_out of
 * s3imph_index_descendants_fill.  s3imph_index_lookup_device followed by this is `query
 * --estimate-cost` for a batch.  The table travels as a kernel argument.  More than 2^31 - 1
 * workgroups of queries in one batch is S3IMPH_ERR_INVALID.  Synchronous on `stream`. */
int s3imph_index_cost_device(s3imph_index *idx, const uint64_t *d_qpos, uint64_t nq, const s3imph_price_table *pt,
                             s3imph_cost *d_out, void *stream);

/* The rows of the last s3imph_index_descendants_plan (AT or UPTO, with its filter if it had one),
 * each cut to its k largest positions by `key` — an extension over the reference, whose Filtered
 * form only thresholds.  top_n[r] = min(k, len(row r)); entries [r * k, r * k + top_n[r]) of
 * d_top_pos / d_top_key hold the row's positions with the largest keys and those keys, in
 * descending key order as unsigned 64-bit, equal keys by ascending position; the remaining entries
 * of the row are pos = UINT64_MAX, key = 0.  The plan stays, so a fill may still follow.
 * S3IMPH_ERR_STATE without a plan, for COUNT / BYTES on an index without the two stats arrays and
 * for COST without tier data; S3IMPH_ERR_INVALID for k == 0, an unknown key, a NULL or refused
 * table with COST, n_rows * k >= 2^31 or a plan of 2^32 positions or more.  A plan with n_rows ==
 * 0 or total == 0 is OK and writes only the padding and top_n.  The scratch (32 bytes per planned
 * position plus the segmented sort's temporary) lives in the handle, grows on demand and is freed
 * on close.  Synchronous on `stream`. */
#define S3IMPH_RANK_OBJECT_COUNT 0
#define S3IMPH_RANK_TOTAL_BYTES  1
#define S3IMPH_RANK_MONTHLY_COST 2   /* s3imph_cost.total of the position */
int s3imph_index_descendants_top(s3imph_index *idx, int key, const s3imph_price_table *pt /* COST only */,
                                 uint32_t k, uint64_t *d_top_pos /* n_rows * k */, uint64_t *d_top_key /* n_rows * k */,
                                 uint32_t *d_top_n /* n_rows */, void *stream);

/* ------------------------------------------------------------------------
 * 5i. Sorted runs of prefix rows merged on the GPU, and an index built in chunks: the back of
 *     pkg/extsort's pipeline.  Pipeline.flushAggregator (pipeline.go:703-783) drains the
 *     aggregator into a sorted RUN of PrefixRows whenever memory fills; runMergeBuildPhase
 *     (pipeline.go:786-914) k-way merges the runs (MergeIterator.Next, merger.go:104-140, which
 *     sums equal prefixes with PrefixRow.Merge, types.go:82-91; the rounds are
 *     ParallelMerger.MergeAll, parallel_merge.go:122-190) and feeds IndexBuilder.  Here a listing
 *     that does not fit one GPU is cut into chunks, each chunk is parsed / sorted / aggregated on
 *     the GPU by sections 5d-5g into a run kept in HOST memory, and the runs — far fewer rows than
 *     objects — are merged in HBM at the end.
 *
 *     Input of the device merge: ONE row set in HBM sorted in K stretches — d_blob / d_offsets
 *     (N + 1 entries) under section 5d's contract (any byte alignment, offsets[0] need not be 0,
 *     readable to round_up(offsets[N], 8)), d_depth, d_count, d_bytes (N entries each), optionally
 *     the 12 + 12 tier columns, column-major (column t at t * tier_stride, tier_stride >= N; both
 *     NULL: no tier columns are read or produced; one without the other is S3IMPH_ERR_INVALID),
 *     and a HOST array run_starts[K + 1] with run_starts[0] = 0, non-decreasing, run_starts[K] = N:
 *     run r is rows run_starts[r] .. run_starts[r + 1]; empty runs are allowed.
 *
 *     What MergeIterator yields: the rows in byte order (Go's string <: a proper prefix first, 0x00
 *     and bytes >= 0x80 ordinary), one row per distinct prefix; Count, TotalBytes and every tier
 *     column summed mod 2^64 over ALL input rows with that prefix, equal neighbours inside one run
 *     included (the loop at merger.go:125-137 folds them too).  Depth is taken from the member in
 *     the lowest run, in a tie the lowest row index: the reference keeps whichever row its heap pops
 *     first, which is unspecified among equals; this is the library's deterministic choice.
 *     present_mask has bit t set iff some MERGED row has tier_count[t] | tier_bytes[t] != 0
 *     (indexbuild.go:192-196).
 *
 *     Refusals, all S3IMPH_ERR_INVALID with a message worded "merge: ..." (s3imph_ctx_last_error):
 *     a run that is not non-decreasing (first_unsorted = the global row index; the reference does
 *     not check — a tightening; a descent exactly at a run boundary is no error), run_starts
 *     malformed, K > S3IMPH_MERGE_MAX_RUNS, N >= 2^32 (this and every null or shape check come
 *     before any device work), more than 2^30 output rows.  N == 0 (any K, 0 included) is OK with
 *     zero rows.
 *
 *     Memory: the scratch lives in ctx, grows on demand and is released by
 *     s3imph_release_workspaces: 32 bytes per input row (the merged order 4, head flags and head
 *     lengths with their scans 8 + 8, the heads' places 4, the heads' sources 8) plus 4 K / S bytes
 *     per row for the splitter table (S = the sample step of s3imph_merge_geometry) and the scans'
 *     temporary.  The merge is out of place: input and output rows coexist in HBM.
 * ------------------------------------------------------------------------ */
#define S3IMPH_MERGE_MAX_RUNS 64
typedef struct s3imph_merge_info {
    uint64_t n_in;            /* N */
    uint64_t n_out;           /* distinct prefixes: the rows the fill writes */
    uint64_t blob_bytes;      /* bytes of the output prefixes */
    uint64_t first_unsorted;  /* smallest global i with row[i] < row[i-1] inside one run; UINT64_MAX when none */
    uint64_t present_mask;    /* of the merged rows; 0 without tier columns */
    uint32_t max_depth_seen;  /* deepest output depth */
    uint32_t n_runs;          /* K */
} s3imph_merge_info;          /* 48 bytes */

/* MergeIterator over K runs in HBM (merger.go:104-140), first half: the order, the fold and the
 * scans that size the result; fills *info and keeps the plan in ctx (a later plan replaces it).
 * The input arrays must stay valid and unchanged until the fill.  Synchronous on `stream`. */
int s3imph_merge_rows_plan_device(s3imph_ctx *ctx, const uint8_t *d_blob, const uint64_t *d_offsets,
                                  const uint32_t *d_depth, const uint64_t *d_count, const uint64_t *d_bytes,
                                  const uint64_t *d_tier_count, const uint64_t *d_tier_bytes, uint64_t tier_stride,
                                  const uint64_t *run_starts, uint32_t k, s3imph_merge_info *info, void *stream);

/* The merged rows of the last plan (PrefixRow.Merge, types.go:82-91), under
 * s3imph_aggregate_fill_device's contract: d_blob (blob_cap >= round_up(blob_bytes, 8); the padding
 * is written as zeros, so the result goes straight into s3imph_build_device), d_offsets (n_out + 1
 * entries, starting at 0), n_cap >= n_out entries each of d_depth, d_count, d_bytes, and — required
 * iff the plan had tier inputs — the tier columns, column t at t * n_cap.  S3IMPH_ERR_STATE without
 * a plan, S3IMPH_ERR_INVALID when a capacity is short.  Synchronous on `stream`. */
int s3imph_merge_rows_fill_device(s3imph_ctx *ctx, uint8_t *d_blob, uint64_t blob_cap, uint64_t *d_offsets,
                                  uint32_t *d_depth, uint64_t *d_count, uint64_t *d_bytes,
                                  uint64_t *d_tier_count, uint64_t *d_tier_bytes, uint64_t n_cap, void *stream);

/* The merge's geometry, for tests that place run lengths on its edges: every *sample_step-th row of
 * a run is a splitter. */
void s3imph_merge_geometry(uint32_t *sample_step);

/* One sorted run in host memory: n rows in the blob / offsets layout (offsets[0] need not be 0),
 * their depths, counts and bytes, and the tier columns (column t at t * tier_stride, tier_stride
 * >= n) — both NULL or both set.  n == 0 may leave every pointer NULL. */
typedef struct s3imph_row_run {
    const uint8_t *blob;
    const uint64_t *offsets;
    const uint32_t *depth;
    const uint64_t *count, *bytes, *tier_count, *tier_bytes;
    uint64_t n, tier_stride;
} s3imph_row_run;

/* The merge from host memory (merger.go:104-140; parallel_merge.go:122-190): the runs are
 * concatenated on upload, their offsets rebased, merged, and the rows brought back.  The outputs
 * are allocated by the library as in s3imph_aggregate_tiers_host (release each with s3imph_free);
 * the tier outputs are S3IMPH_NUM_TIERS x *n u64 each, column t at t * *n, and come back NULL when
 * the runs carry no tier columns (tier_count / tier_bytes / present_mask may then be NULL
 * themselves).  Runs that mix "with tiers" and "without" are S3IMPH_ERR_INVALID, before any device
 * work (an empty run counts with neither).  k > S3IMPH_MERGE_MAX_RUNS merges in rounds of at most
 * 64 CONTIGUOUS runs, as MergeAll does: contiguous groups keep "the lowest run wins" and the sums
 * are associative, so the result does not depend on the grouping.  *info (nullable) describes the
 * whole merge: n_in over all runs, first_unsorted as a row index into their concatenation.  No row
 * at all: *n = 0, *offsets = [0], the others NULL, no device touched. */
int s3imph_merge_rows_host(int device, const s3imph_row_run *runs, uint64_t k, uint8_t **blob, uint64_t **offsets,
                           uint32_t **depth, uint64_t **object_count, uint64_t **total_bytes,
                           uint64_t **tier_count, uint64_t **tier_bytes, uint64_t *present_mask, uint64_t *n,
                           s3imph_merge_info *info, char *err, size_t errlen);

/* runMergeBuildPhase (pipeline.go:786-914): the runs merged, then the back half of
 * s3imph_index_from_objects[_tiers]_host in the same device residency — MPHF build, finalize with
 * the merged depths, the twelve index files, the tier files when the runs carry tier columns,
 * manifest.json.  k == 0 or only empty runs writes the empty index s3imph_index_open accepts
 * (pipeline.go:796-806).  A missing out_dir is S3IMPH_ERR_IO before the device is selected; the
 * out-of-memory retry of the host builds applies; error texts are "merge: ...", then the existing
 * "build MPHF: ...". */
int s3imph_index_from_rows_host(int device, const s3imph_row_run *runs, uint64_t k, const char *out_dir,
                                char *err, size_t errlen);

/* The chunked build — Pipeline's ingest loop (pipeline.go:370-517, :703-783): a handle that holds
 * runs in host memory.  Each add_objects (a listing chunk in ANY order; tiers: one id per object,
 * required iff the set was made with_tiers, ignored otherwise) and each add_csv (CSV buffers as
 * in s3imph_index_from_csv_host) is one parse / sort / aggregate on the GPU with the handle's
 * max_depth, followed by a D2H of the rows into the handle: one run; a chunk without an object
 * adds none.  add_rows copies a caller's sorted run (its tier columns must match with_tiers).
 * build is s3imph_index_from_rows_host over the held runs and may be repeated.
 *
 * The contract: the directory equals, file for file, the one
 * s3imph_index_from_unsorted_objects_host (with tiers when with_tiers) writes for the concatenation
 * of the chunks — manifest.json's created_at excepted.  Only one chunk's listing is in HBM at a
 * time; the merge needs the runs' rows there twice (in and out).  Spilling runs to disk, run files
 * (runfile.go's EXTS format) and compressed runs are out of scope.  Calls on one handle are
 * serialized by the handle. */
typedef struct s3imph_rowset s3imph_rowset;
int s3imph_rowset_new(int device, uint32_t max_depth, int with_tiers, s3imph_rowset **out, char *err, size_t errlen);
int s3imph_rowset_add_objects(s3imph_rowset *rs, const uint8_t *keys, const uint64_t *key_offsets,
                              const uint64_t *sizes, const uint8_t *tiers, uint64_t m, char *err, size_t errlen);
int s3imph_rowset_add_csv(s3imph_rowset *rs, const uint8_t *const *csv, const uint64_t *csv_len, uint64_t n_files,
                          const s3imph_csv_schema *schema, char *err, size_t errlen);
int s3imph_rowset_add_rows(s3imph_rowset *rs, const s3imph_row_run *run, char *err, size_t errlen);
/* Runs held, and rows held over all runs. */
uint64_t s3imph_rowset_runs(const s3imph_rowset *rs);
uint64_t s3imph_rowset_rows(const s3imph_rowset *rs);
int s3imph_rowset_build(s3imph_rowset *rs, const char *out_dir, char *err, size_t errlen);
int s3imph_rowset_close(s3imph_rowset *rs);

/* ------------------------------------------------------------------------
 * 5j. gzip files inflated on the GPU, and the index built from .csv.gz inventory files: what
 *     pgzip.NewReader / gzip.NewReader do in front of the CSV readers (pkg/inventory/unified.go:93-103,
 *     reader.go:81-86, :216-221).  Parity is "vs the RFCs, checked against zlib": RFC 1951,
 *     RFC 1952 and compress/gzip's behaviour as stated here.
 *
 *     A gzip file is one or more members back to back (Go's multistream default).  Per member:
 *     magic 1f 8b and CM = 8, anything else "invalid header"; FEXTRA, FNAME and FCOMMENT are
 *     skipped; FHCRC (the low 16 bits of the CRC-32 of the header bytes) is verified, a mismatch
 *     is "invalid header"; reserved flag bits are ignored; a raw DEFLATE stream; CRC-32 and ISIZE,
 *     little-endian.  After a member the end of the input is a clean end, and anything else must
 *     be another member header: trailing bytes that are none, zero padding included, are "invalid
 *     header".  A zero-length file is "unexpected EOF".  A member's window starts empty: a
 *     distance that reaches before the member's own first byte is corrupt.
 *
 *     DEFLATE in full: stored blocks (LEN 0 to 65535, NLEN checked), fixed and dynamic Huffman
 *     blocks (the repeat symbols 16 - 18 may run across the literal/length - distance boundary),
 *     code lengths up to 15, lengths up to 258, distances up to 32768, overlapping copies.  A set
 *     of code lengths is refused when over-subscribed, and when incomplete unless it is a single
 *     code of length 1 or empty; a dynamic block without an end-of-block code is refused; block
 *     type 3, literal/length symbols 286 and 287 and distance symbols 30 and 31 are corrupt.
 *
 *     Out of scope: zlib and raw-deflate containers, preset dictionaries, parallel decoding inside
 *     one member (the parallelism is across files: a wave per file), returning the header fields.
 * ------------------------------------------------------------------------ */
enum { S3IMPH_GZ_OK = 0, S3IMPH_GZ_MORE = 1, S3IMPH_GZ_EOF = 2, S3IMPH_GZ_HEADER = 3,
       S3IMPH_GZ_DATA = 4, S3IMPH_GZ_CHECKSUM = 5 };

typedef struct s3imph_gunzip_info {   /* 32 bytes */
    uint64_t out_bytes;  /* inflated bytes of all members, counted past the room given as well */
    uint64_t in_used;    /* gzip bytes consumed; == the file's length when status is OK or MORE */
    uint32_t members;
    uint32_t status;     /* S3IMPH_GZ_* */
    uint32_t crc32;      /* the CRC-32 the trailers promise for the whole output */
    uint32_t reserved;   /* 0 */
} s3imph_gunzip_info;

/* The decoder's geometry, for tests that place events on the edges: the input stage holds
 * *in_chunk_bytes of a file, a batch *batch_symbols decoded symbols, and the grid is at most
 * CUs x *waves_per_cu waves (more files than that make the ticket loop wrap). */
void s3imph_gunzip_geometry(uint32_t *in_chunk_bytes, uint32_t *batch_symbols, uint32_t *waves_per_cu);

/* Host only: the room to offer a file, min(ISIZE read from its last four bytes, 1032 * len + 64),
 * 0 for len < 18.  1032 : 1 is DEFLATE's largest expansion, so a lying trailer cannot ask for
 * 4 GiB; for a single-member file under 4 GiB the hint is exact. */
uint64_t s3imph_gunzip_room_hint(const uint8_t *gz, uint64_t len);

/* n_files gzip files in HBM, one launch.  File i is d_gz[gz_offsets[i] .. gz_offsets[i+1]) at any
 * byte alignment and may write only d_out[out_offsets[i] .. out_offsets[i+1]); no byte outside
 * that range is written, whatever the input holds.  Returns S3IMPH_OK when it ran; the verdict per
 * file is info[i].status: OK; MORE (the file needs out_bytes of room; the bytes that fit were
 * written correctly); EOF, HEADER, DATA, CHECKSUM (the contents of the file's range are
 * unspecified).  The CRC-32 of the text is computed on the device and compared with the trailers'
 * for every file that is OK.  Null arguments with n_files > 0, non-monotonic offsets and
 * n_files >= 2^31 are S3IMPH_ERR_INVALID before any device work; n_files == 0 is OK without any.
 * Synchronous on `stream`. */
int s3imph_gunzip_device(s3imph_ctx *ctx, const uint8_t *d_gz, const uint64_t *gz_offsets /* host, n+1 */,
                         uint64_t n_files, uint8_t *d_out, const uint64_t *out_offsets /* host, n+1 */,
                         s3imph_gunzip_info *info /* host, n */, void *stream);

/* The same from host memory: H2D of the compressed bytes, one launch with the room hints, the
 * files that reported MORE once more with their exact room, D2H.  out[i] is allocated by the
 * library (release each with s3imph_free), out_len[i] its length; info (nullable) as above.  A bad
 * file is S3IMPH_ERR_FORMAT, worded "gzip: file <i>: unexpected EOF | invalid header | corrupt
 * input | invalid checksum" for the lowest such i, and leaves every out[i] NULL. */
int s3imph_gunzip_host(int device, const uint8_t *const *gz, const uint64_t *gz_len, uint64_t n_files,
                       uint8_t **out /* n pointers, each s3imph_free */, uint64_t *out_len,
                       s3imph_gunzip_info *info /* nullable */, char *err, size_t errlen);

/* s3imph_index_from_csv_host over .csv.gz files: consecutive files are uploaded compressed and
 * inflated on the device in groups of about group_bytes (compressed bytes plus room hints; 0: the
 * library's default; a file larger than that is a group of its own; the result does not depend on
 * it), then parsed file by file from HBM as the CSV call parses them.  A bad gzip file fails the
 * call as in s3imph_gunzip_host, before anything is written.  A missing out_dir is S3IMPH_ERR_IO
 * before the device is selected; the out-of-memory retry of the host builds applies. */
int s3imph_index_from_csv_gz_host(int device, const uint8_t *const *gz, const uint64_t *gz_len, uint64_t n_files,
                                  const s3imph_csv_schema *schema, int with_tiers, uint32_t max_depth,
                                  uint64_t group_bytes /* 0: default */, const char *out_dir,
                                  s3imph_csv_info *info_total, char *err, size_t errlen);

/* s3imph_rowset_add_csv over .csv.gz files; a bad gzip file adds no run. */
int s3imph_rowset_add_csv_gz(s3imph_rowset *rs, const uint8_t *const *gz, const uint64_t *gz_len, uint64_t n_files,
                             const s3imph_csv_schema *schema, uint64_t group_bytes, char *err, size_t errlen);

/* ------------------------------------------------------------------------
 * 6. Deterministic synthetic prefix sets (bench/test support, not on the path).
 *    kind: 0 = s3-like, lengths uniform in [max(10, avg/2), 3avg/2],
 *              distinct and byte-sorted;
 *          1 = lengths log-uniform in [1, 1024] (C5), each raised to the base-64 digit
 *              count of its index where that is longer (4 bytes hold 16.7M keys), so
 *              keys stay distinct; not byte-sorted.
 *    Key 0 = "" when lo == 0 (the root prefix).  Generate keys
 *    [lo, lo+n) of the global sequence: call once with blob == NULL to get the
 *    byte count, then again to fill.  offsets are relative to the shard start.
 * ------------------------------------------------------------------------ */
int s3imph_gen_keys(int kind, uint64_t seed, uint32_t avg_len, uint64_t lo, uint64_t n,
                    uint8_t *blob, uint64_t *offsets, uint64_t *total_bytes);

/* ------------------------------------------------------------------------
 * 7. Developer knobs (not on the path; no reference counterpart).
 *    The library reads its A/B geometry knobs, test-only fallbacks and fault-injection hooks
 *    (S3IMPH_P0, S3IMPH_L20, S3IMPH_FAULT_DUP_REC, S3IMPH_HASH_ONLY, S3IMPH_DIST_SWITCH, ...;
 *    DESIGN.md section 5) from the environment ONLY after s3imph_dev_knobs(1), so a stray
 *    variable in an embedding process cannot change a production build.  The documented user
 *    settings S3IMPH_DIST_MODE, S3IMPH_PINNED_KEEP and S3IMPH_DEBUG are read regardless.
 *    Knobs are sampled when a context is created (some on first use): call this first.
 * ------------------------------------------------------------------------ */
int s3imph_dev_knobs(int on);

#ifdef __cplusplus
}
#endif

#endif /* S3IMPH_H */
