// s3imph_tiers.h — host helpers of the per-tier statistics (s3imph_tiers.cpp), shared with the
// aggregation's host entry points and the reader's Open.  Not part of the ABI.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

namespace s3imph {

// One entry of tiers.json (tiers.Info); a field the entry does not give keeps Go's zero value.
struct TierEntry {
  unsigned id = 0;
  std::string name, file;
};

// tiers.json's text for the tiers of present_mask, ascending id: json.MarshalIndent(TierManifest,
// "", "  "), no trailing newline (tiers.go:126-150).
std::string tiers_json(uint64_t present_mask);

// tier_stats/<file>_count.u64, tier_stats/<file>_bytes.u64 for every tier of present_mask
// (column t at t * stride, n entries) and tiers.json; nothing at all for an empty mask.
int write_tier_files(const std::string& dir, uint64_t present_mask, const uint64_t* tier_count,
                     const uint64_t* tier_bytes, uint64_t n, uint64_t stride, std::string* msg);

// ReadManifest (tiers.go:153-170) as OpenTierStats calls it: the entries in file order; none
// when tiers.json is absent.  Messages start with "read tier manifest: ".
int read_tier_manifest(const std::string& dir, std::vector<TierEntry>* out, std::string* msg);

}  // namespace s3imph
