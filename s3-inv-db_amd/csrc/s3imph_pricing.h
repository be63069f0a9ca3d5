// s3imph_pricing.h — pricing.ComputeMonthlyCost's arithmetic for one tier slot (pkg/pricing/
// pricing.go:159-240; include/s3imph.h section 5h), shared by the host (s3imph_pricing.cpp) and
// the device (s3imph_index.hip) so the two cannot drift.  Not part of the ABI.
//
// All floating point is IEEE binary64 in the reference's operation order: (f64(x) / 2^30) * price
// * 1e6, left to right, truncated toward zero.  No float, no reassociation (g * (p * 1e6) differs
// from (g * p) * 1e6 after truncation for about 2 in 10 000 byte counts), and nothing here adds
// doubles, so no contraction into a fused multiply-add can occur.
//
// Differences from the reference, deliberate:
//   - a double that is NaN or >= 2^64 converts to UINT64_MAX (Go: implementation-specific; C++:
//     undefined), written out in f64_to_u64;
//   - a table with a negative, NaN or infinite price, fee or standard price is refused by the
//     entry points before this is called, so no negative double reaches the conversion;
//   - tiers are keyed by id: PerGBMonth's name of id t is s3imph_tier_name(t).
#pragma once

#include <stdint.h>

#include "s3imph.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define S3IMPH_PRICE_HD __host__ __device__ __forceinline__
#else
#define S3IMPH_PRICE_HD inline
#endif

namespace s3imph {

// pricing.go:39-61 by tier id
constexpr uint32_t kTiersWithMinObjectSize = 1u << S3IMPH_TIER_STANDARD_IA | 1u << S3IMPH_TIER_ONEZONE_IA |
                                             1u << S3IMPH_TIER_GLACIER_IR;
constexpr uint32_t kTiersWithMonitoringCost = 1u << S3IMPH_TIER_IT_FREQUENT | 1u << S3IMPH_TIER_IT_INFREQUENT |
                                              1u << S3IMPH_TIER_IT_ARCHIVE_INSTANT | 1u << S3IMPH_TIER_IT_ARCHIVE |
                                              1u << S3IMPH_TIER_IT_DEEP_ARCHIVE;
constexpr uint32_t kTiersWithGlacierOverhead = 1u << S3IMPH_TIER_GLACIER_FR | 1u << S3IMPH_TIER_DEEP_ARCHIVE |
                                               1u << S3IMPH_TIER_IT_ARCHIVE | 1u << S3IMPH_TIER_IT_DEEP_ARCHIVE;
constexpr uint64_t kMinObjectSizeBytes = 128 * 1024;

// Go's uint64(x) for x >= 0, with the two cases Go leaves open pinned to UINT64_MAX.
S3IMPH_PRICE_HD uint64_t f64_to_u64(double x) {
  if (!(x < 18446744073709551616.0)) return UINT64_MAX;  // NaN, +Inf, >= 2^64
  return (uint64_t)x;
}

// uint64(float64(b) / bytesPerGB * price * 1_000_000)
S3IMPH_PRICE_HD uint64_t gb_microdollars(uint64_t b, double price) {
  const double gb = (double)b / 1073741824.0;
  return f64_to_u64(gb * price * 1000000.0);
}

// What one tier of a breakdown adds to CostResult.
struct SlotCost {
  uint64_t tier_total = 0;  // PerTierMicrodollars[tier]: storage + min_size + overhead
  uint64_t min_size = 0, monitoring = 0, overhead = 0;
  uint32_t priced = 0;      // PerGBMonth has the tier: the map gets the key
};

S3IMPH_PRICE_HD SlotCost price_slot(uint32_t id, uint64_t count, uint64_t bytes, const s3imph_price_table& pt) {
  SlotCost r;
  if (id >= (uint32_t)S3IMPH_NUM_TIERS || !((pt.priced_mask >> id) & 1)) return r;
  r.priced = 1;
  const double price = pt.per_gb_month[id];
  const uint64_t storage = gb_microdollars(bytes, price);
  const uint64_t avg = count ? bytes / count : 0;
  const uint32_t bit = 1u << id;
  if ((kTiersWithMinObjectSize & bit) && avg < kMinObjectSizeBytes && avg > 0)
    r.min_size = gb_microdollars((kMinObjectSizeBytes - avg) * count, price);
  if ((kTiersWithMonitoringCost & bit) && pt.monitoring_per_1000_objects > 0) {
    const uint64_t mon = avg >= kMinObjectSizeBytes ? count : (avg > 0 ? count / 2 : 0);
    if (mon > 0) r.monitoring = f64_to_u64((double)mon / 1000.0 * pt.monitoring_per_1000_objects * 1000000.0);
  }
  if ((kTiersWithGlacierOverhead & bit) && count > 0)
    r.overhead = gb_microdollars(count * 32768, price) + gb_microdollars(count * 8192, pt.standard_price_per_gb);
  r.tier_total = storage + r.min_size + r.overhead;
  return r;
}

// "" for a table the entry points accept, else what is wrong with it.
inline const char* price_table_fault(const s3imph_price_table& pt) {
  auto bad = [](double v) { return !(v >= 0.0) || v > 1.7976931348623157e308; };
  for (int t = 0; t < S3IMPH_NUM_TIERS; ++t)
    if (((pt.priced_mask >> t) & 1) && bad(pt.per_gb_month[t])) return "a price is negative, NaN or infinite";
  if (bad(pt.monitoring_per_1000_objects)) return "the monitoring fee is negative, NaN or infinite";
  if (bad(pt.standard_price_per_gb)) return "the standard price is negative, NaN or infinite";
  return "";
}

}  // namespace s3imph
