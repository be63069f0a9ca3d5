// s3imph_prim.h — the rocPRIM calls of the listing stages (s3imph_finalize.hip,
// s3imph_aggregate.hip, s3imph_sort.hip) and the device temporary they run in.  rocPRIM is heavy
// to compile, so this is included by its three users only, not by s3imph_ctx.h.
#pragma once

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

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

// The two calls below are templates over the element type only so that a file compiles the
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

}  // namespace s3imph
