// s3imph_prim.h — the rocPRIM calls of the listing stages (s3imph_finalize.hip,
// s3imph_aggregate.hip, s3imph_sort.hip) and of the reader's ranking (s3imph_index.hip), and the
// device temporary they run in.  rocPRIM is heavy to compile, so this is included by its four
// users only, not by s3imph_ctx.h.
#pragma once

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <type_traits>

#include "s3imph_ctx.h"

namespace s3imph {

// rocPRIM's temporary storage, grown to the largest request so far.  Each stage's scratch keeps
// its own: a call may return with its last rocPRIM kernel still in flight on the caller's stream
// (finalize_device does), and another stage on another stream must not free the buffer under it.
struct PrimTmp {
  uint8_t* p = nullptr;
  uint64_t cap = 0;  // bytes
  void reserve(uint64_t bytes) { grow(p, cap, bytes); }
  void release() {
    dfree(p);
    cap = 0;
  }
};

// The calls below are templates over the element type only so that a file compiles the
// rocPRIM kernels of the calls it makes, not of every call declared here; all uses are uint64_t.

// In-place exclusive prefix sum of v[0 .. count), starting from init (wrapping).
template <class T>
void scan_u64(PrimTmp& t, T* v, uint64_t count, std::common_type_t<T> init, hipStream_t s) {
  static_assert(std::is_same<T, uint64_t>::value, "scan_u64 scans uint64_t");
  size_t need = 0;
  HIPCHECK(rocprim::exclusive_scan(nullptr, need, v, v, init, count, rocprim::plus<T>(), s));
  t.reserve(need);
  HIPCHECK(rocprim::exclusive_scan(t.p, need, v, v, init, count, rocprim::plus<T>(), s));
}

// One stable radix sort of `count` (key, value) pairs on the key bits [lo, hi).
template <class T>
void sort_pairs(PrimTmp& t, const T* kin, T* kout, const T* vin, T* vout, uint64_t count, unsigned lo, unsigned hi,
                hipStream_t s) {
  size_t need = 0;
  HIPCHECK(rocprim::radix_sort_pairs(nullptr, need, kin, kout, vin, vout, (size_t)count, lo, hi, s));
  t.reserve(need);
  HIPCHECK(rocprim::radix_sort_pairs(t.p, need, kin, kout, vin, vout, (size_t)count, lo, hi, s));
}

// One stable descending radix sort of `count` (key, value) pairs on all key bits.
template <class T>
void sort_pairs_desc(PrimTmp& t, const T* kin, T* kout, const T* vin, T* vout, uint64_t count, hipStream_t s) {
  size_t need = 0;
  HIPCHECK(rocprim::radix_sort_pairs_desc(nullptr, need, kin, kout, vin, vout, (size_t)count, 0, 8 * sizeof(T), s));
  t.reserve(need);
  HIPCHECK(rocprim::radix_sort_pairs_desc(t.p, need, kin, kout, vin, vout, (size_t)count, 0, 8 * sizeof(T), s));
}

// One stable descending radix sort of (key, value) pairs inside each of `segments` rows, row r
// being [row_ptr[r], row_ptr[r + 1]).  rocPRIM reads the offsets as 32-bit: count < 2^32.
template <class T>
void sort_rows_pairs_desc(PrimTmp& t, const T* kin, T* kout, const T* vin, T* vout, uint64_t count, uint64_t segments,
                          const T* row_ptr, hipStream_t s) {
  size_t need = 0;
  HIPCHECK(rocprim::segmented_radix_sort_pairs_desc(nullptr, need, kin, kout, vin, vout, (unsigned)count,
                                                    (unsigned)segments, row_ptr, row_ptr + 1, 0, 8 * sizeof(T), s));
  t.reserve(need);
  HIPCHECK(rocprim::segmented_radix_sort_pairs_desc(t.p, need, kin, kout, vin, vout, (unsigned)count,
                                                    (unsigned)segments, row_ptr, row_ptr + 1, 0, 8 * sizeof(T), s));
}

}  // namespace s3imph
