// s3imph_entry.h — the boundary policy of the C ABI's stage entry points, written once: who
// locks, when the device is set, which stream a call runs on, the one retry after the device ran
// out of memory, how a failure is worded, and that no exception crosses the ABI.  device_entry
// frames the calls on a handle (s3imph_ctx, s3imph_index), host_entry the calls on host memory;
// HostRows owns the rows such a call hands to a C caller.  Host-only; not part of the ABI.
#pragma once

#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>

#include "s3imph_ctx.h"

namespace s3imph {

// Makes `device` current and picks the stream of a device call: the caller's, else the handle's
// own.  A wrapper calls it where it first needs the device, after the returns that need none.
inline hipStream_t use_device(int device, void* stream, hipStream_t own) {
  HIPCHECK(hipSetDevice(device));
  return stream ? static_cast<hipStream_t>(stream) : own;
}

// A device call on handle h (its mu, last_msg), under the handle's lock: body(msg) returns a
// status and leaves its message in msg, which becomes last_msg; a Fail becomes its code and
// prefix + its message, a failed host allocation S3IMPH_ERR_NOMEM.
template <class H, class F>
int device_entry(H* h, const char* prefix, F&& body) {
  std::lock_guard<std::mutex> lk(h->mu);
  try {
    std::string msg;
    const int rc = body(msg);
    h->last_msg = msg;
    return rc;
  } catch (const Fail& f) {
    h->last_msg = prefix + f.msg;
    return f.code;
  } catch (const std::bad_alloc&) {
    h->last_msg = std::string(prefix) + "out of host memory";
    return S3IMPH_ERR_NOMEM;
  }
}

// A part of a host call, with or without a device: f(msg) returns a status and leaves its
// message in msg, which goes into err unless the status is OK; what f throws becomes a status and
// a message worded with the stage's prefix.  A Fail already worded by the sort or the CSV stage
// (rows_from_host) keeps its wording.
template <class F>
int host_call(const char* prefix, char* err, size_t errlen, F&& f) {
  try {
    std::string msg;
    const int rc = f(msg);
    if (rc != S3IMPH_OK) set_err(err, errlen, msg);
    return rc;
  } catch (const Fail& e) {
    const bool worded = e.msg.compare(0, 6, "sort: ") == 0 || e.msg.compare(0, 5, "csv: ") == 0 ||
                        e.msg.compare(0, 6, "gzip: ") == 0;
    set_err(err, errlen, worded ? e.msg : prefix + e.msg);
    return e.code;
  } catch (const std::bad_alloc&) {
    set_err(err, errlen, std::string(prefix) + "out of host memory");
    return S3IMPH_ERR_NOMEM;
  }
}

// A host call's device work: on the process's context for `device`, under its lock, with the
// device current, body(c, stream, msg) runs, and once more after it ran out of HBM and something
// could be reclaimed.  No context: S3IMPH_ERR_HIP, worded with no_ctx_prefix (the stage of the
// entry point called, where that is not `prefix`).
template <class F>
int host_entry(int device, const char* prefix, char* err, size_t errlen, F&& body,
               const char* no_ctx_prefix = nullptr) {
  return host_call(prefix, err, errlen, [&](std::string& msg) -> int {
    s3imph_ctx* c = default_ctx(device, &msg);
    if (!c) {
      msg = (no_ctx_prefix ? no_ctx_prefix : prefix) + msg;
      return S3IMPH_ERR_HIP;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    HIPCHECK(hipSetDevice(c->device));
    hipStream_t s = c->own_stream;
    return retry_on_nomem(c, s, &msg, [&]() -> int { return body(c, s, msg); });
  });
}

// A malloc'd array for a C caller (s3imph_free), never a null one.
template <typename T>
T* host_array(uint64_t count) {
  T* p = static_cast<T*>(std::malloc(std::max<uint64_t>(count, 1) * sizeof(T)));
  if (!p) throw std::bad_alloc();
  return p;
}

// Rows in HBM to host arrays of their sizes (the tier columns only with `tiers`).
inline void rows_to_host(s3imph_ctx* c, const DevRows& r, bool tiers, uint8_t* blob, uint64_t* offsets,
                         uint32_t* depth, uint64_t* count, uint64_t* bytes, uint64_t* tier_count,
                         uint64_t* tier_bytes) {
  if (r.blob_bytes) HIPCHECK(hipMemcpy(blob, r.blob, r.blob_bytes, hipMemcpyDeviceToHost));
  staged_copy(c, false, offsets, r.offsets, (r.n + 1) * 8);
  staged_copy(c, false, depth, r.depth, r.n * 4);
  staged_copy(c, false, count, r.ocnt, r.n * 8);
  staged_copy(c, false, bytes, r.tbytes, r.n * 8);
  if (tiers) {
    staged_copy(c, false, tier_count, r.tier_count, S3IMPH_NUM_TIERS * r.n * 8);
    staged_copy(c, false, tier_bytes, r.tier_bytes, S3IMPH_NUM_TIERS * r.n * 8);
  }
}

// The rows a host call hands to a C caller: the caller's out-pointers, the arrays malloc'd here.
// The tier pointers may be null (a call without tiers): what would go there is then dropped.
struct HostRows {
  uint8_t** blob;
  uint64_t** offsets;
  uint32_t** depth;
  uint64_t **object_count, **total_bytes, **tier_count, **tier_bytes;
  uint64_t *present_mask, *n;
  uint64_t *no_count = nullptr, *no_bytes = nullptr, no_mask = 0;

  HostRows(uint8_t** blob_, uint64_t** offsets_, uint32_t** depth_, uint64_t** object_count_,
           uint64_t** total_bytes_, uint64_t** tier_count_, uint64_t** tier_bytes_, uint64_t* present_mask_,
           uint64_t* n_)
      : blob(blob_), offsets(offsets_), depth(depth_), object_count(object_count_), total_bytes(total_bytes_),
        tier_count(tier_count_ ? tier_count_ : &no_count), tier_bytes(tier_bytes_ ? tier_bytes_ : &no_bytes),
        present_mask(present_mask_ ? present_mask_ : &no_mask), n(n_) {}
  HostRows(const HostRows&) = delete;
  HostRows& operator=(const HostRows&) = delete;

  void reset() {
    *blob = nullptr;
    *offsets = nullptr;
    *depth = nullptr;
    *object_count = *total_bytes = nullptr;
    *tier_count = *tier_bytes = nullptr;
    *present_mask = 0;
    *n = 0;
  }
  void drop() {
    std::free(*blob);
    std::free(*offsets);
    std::free(*depth);
    std::free(*object_count);
    std::free(*total_bytes);
    std::free(*tier_count);
    std::free(*tier_bytes);
    reset();
  }
  // No row at all: one offset, 0.
  int none() {
    *offsets = host_array<uint64_t>(1);
    (*offsets)[0] = 0;
    return S3IMPH_OK;
  }
  void download(s3imph_ctx* c, const DevRows& r, bool tiers) {
    drop();
    *blob = host_array<uint8_t>(r.blob_bytes);
    *offsets = host_array<uint64_t>(r.n + 1);
    *depth = host_array<uint32_t>(r.n);
    *object_count = host_array<uint64_t>(r.n);
    *total_bytes = host_array<uint64_t>(r.n);
    if (tiers) {
      *tier_count = host_array<uint64_t>(S3IMPH_NUM_TIERS * r.n);
      *tier_bytes = host_array<uint64_t>(S3IMPH_NUM_TIERS * r.n);
      *present_mask = r.present_mask;
    }
    rows_to_host(c, r, tiers, *blob, *offsets, *depth, *object_count, *total_bytes, *tier_count, *tier_bytes);
    *n = r.n;
  }
};

}  // namespace s3imph
