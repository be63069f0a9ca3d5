// s3imph_tiers.h — the tier table and Mapping.FromS3's rule, shared by the host
// (s3imph_tiers.cpp) and the device (s3imph_csv.hip) so the two cannot drift, and the host
// helpers of the per-tier statistics, shared with the aggregation's host entry points and the
// reader's Open.  Not part of the ABI.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define S3IMPH_HD __host__ __device__ __forceinline__
#else
#define S3IMPH_HD inline
#endif

// AllTiers (tiers.go:39-53): X(id, Info.Name, Info.FilePrefix), in id order.
#define S3IMPH_TIER_TABLE(X)                                            \
  X(0, "STANDARD", "standard")                                          \
  X(1, "STANDARD_IA", "standard_ia")                                    \
  X(2, "ONEZONE_IA", "onezone_ia")                                      \
  X(3, "GLACIER_IR", "glacier_ir")                                      \
  X(4, "GLACIER", "glacier_fr")                                         \
  X(5, "DEEP_ARCHIVE", "deep_archive")                                  \
  X(6, "REDUCED_REDUNDANCY", "reduced_redundancy")                      \
  X(7, "INTELLIGENT_TIERING_FREQUENT", "it_frequent")                   \
  X(8, "INTELLIGENT_TIERING_INFREQUENT", "it_infrequent")               \
  X(9, "INTELLIGENT_TIERING_ARCHIVE_INSTANT", "it_archive_instant")     \
  X(10, "INTELLIGENT_TIERING_ARCHIVE", "it_archive")                    \
  X(11, "INTELLIGENT_TIERING_DEEP_ARCHIVE", "it_deep_archive")

namespace s3imph {

// The longest name FromS3 compares with; a trimmed field longer than this matches nothing.
constexpr unsigned kTierNameMax = 35;

// strings.TrimSpace narrowed to its ASCII set (\t \n \v \f \r and space): the one white-space
// rule of the library — tier names, CSV header names and CSV sizes all trim by it.  The
// reference also trims Unicode white space (U+0085, U+00A0, ...), which S3 never writes.
S3IMPH_HD bool tier_space(unsigned char ch) { return ch == ' ' || (ch >= '\t' && ch <= '\r'); }
// strings.ToUpper for the ASCII names S3 uses.
S3IMPH_HD unsigned char tier_upper(unsigned char ch) { return ch >= 'a' && ch <= 'z' ? (unsigned char)(ch - 'a' + 'A') : ch; }

// p[0 .. n) upper-cased == name
S3IMPH_HD bool tier_is(const unsigned char* p, unsigned n, const char* name) {
  unsigned i = 0;
  for (; i < n && name[i]; ++i)
    if (tier_upper(p[i]) != (unsigned char)name[i]) return false;
  return i == n && !name[i];
}

// Mapping.FromS3 (tiers.go:85-115) on two fields already trimmed by tier_space (any letter
// case): sc[0 .. scn) the storage class, at[0 .. atn) the access tier.  A length above
// kTierNameMax is an unknown name; its bytes are not read.
S3IMPH_HD int tier_from_trimmed(const unsigned char* sc, unsigned scn, const unsigned char* at, unsigned atn) {
  if (scn > kTierNameMax) return 0;
  if (tier_is(sc, scn, "INTELLIGENT_TIERING")) {
    if (atn > kTierNameMax) return 7;
    if (tier_is(at, atn, "FREQUENT_ACCESS") || tier_is(at, atn, "FREQUENT")) return 7;
    if (tier_is(at, atn, "INFREQUENT_ACCESS") || tier_is(at, atn, "INFREQUENT")) return 8;
    if (tier_is(at, atn, "ARCHIVE_INSTANT_ACCESS")) return 9;
    if (tier_is(at, atn, "ARCHIVE_ACCESS") || tier_is(at, atn, "ARCHIVE")) return 10;
    if (tier_is(at, atn, "DEEP_ARCHIVE_ACCESS") || tier_is(at, atn, "DEEP_ARCHIVE")) return 11;
    return 7;  // missing or unknown access tier
  }
#define S3IMPH_TIER_MATCH(id, name, file) \
  if (tier_is(sc, scn, name)) return id;
  S3IMPH_TIER_TABLE(S3IMPH_TIER_MATCH)
#undef S3IMPH_TIER_MATCH
  return 0;  // unknown class: STANDARD
}

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
