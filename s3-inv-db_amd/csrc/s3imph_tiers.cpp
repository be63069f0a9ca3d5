// s3imph_tiers.cpp — the host side of the per-tier statistics (include/s3imph.h section 5e):
// the tier table and Mapping.FromS3 (pkg/tiers/tiers.go:16-115), tiers.json as WriteManifest
// writes it and ReadManifest reads it (:126-170), and the tier_stats/ arrays of
// IndexBuilder.createTierWriter (pkg/extsort/indexbuild.go:279-314).  No device call here.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <cstdio>
#include <cstring>

#include "s3imph_ctx.h"
#include "s3imph_json.h"
#include "s3imph_tiers.h"

namespace s3imph {
namespace {

struct TierInfo {
  const char *name, *file;
};
// AllTiers, tiers.go:39-53 (the table itself: s3imph_tiers.h)
#define S3IMPH_TIER_ROW(id, name, file) {name, file},
const TierInfo kTiers[S3IMPH_NUM_TIERS] = {S3IMPH_TIER_TABLE(S3IMPH_TIER_ROW)};
#undef S3IMPH_TIER_ROW

// strings.TrimSpace(s) by the shared rule (tier_space): the bytes left, any letter case
std::string trimmed(const char* s) {
  std::string t = s ? s : "";
  size_t b = 0, e = t.size();
  while (b < e && tier_space((unsigned char)t[b])) ++b;
  while (e > b && tier_space((unsigned char)t[e - 1])) --e;
  return t.substr(b, e - b);
}

bool make_dir(const std::string& p) {  // os.MkdirAll(tierDir, 0o755) below an existing out_dir
  if (::mkdir(p.c_str(), 0755) == 0) return true;
  struct stat st;
  return errno == EEXIST && ::stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

// An S3ID u64 array file of n entries (ArrayWriter, writer.go:19-46, :79-96).
bool write_u64_file(const std::string& path, const uint64_t* v, uint64_t n, std::string* msg) {
  static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "S3ID payloads are little-endian");
  uint8_t hdr[kS3idHeaderSize];
  s3id_header(hdr, n, 8);
  const uint8_t* payload = reinterpret_cast<const uint8_t*>(v);
  return write_pieces(path, 2,
                      [&](size_t k, const uint8_t** p, uint64_t* len, uint64_t* off) {
                        *p = k ? payload : hdr;
                        *len = k ? 8 * n : sizeof hdr;
                        *off = k ? sizeof hdr : 0;
                      },
                      msg);
}

}  // namespace

std::string tiers_json(uint64_t present_mask) {
  std::string j = "{\n  \"tiers\": [";
  bool first = true;
  for (int t = 0; t < S3IMPH_NUM_TIERS; ++t) {
    if (!((present_mask >> t) & 1)) continue;
    j += first ? "\n" : ",\n";
    first = false;
    j += "    {\n      \"id\": " + std::to_string(t) + ",\n      \"name\": \"" + kTiers[t].name +
         "\",\n      \"file\": \"" + kTiers[t].file + "\"\n    }";
  }
  j += first ? "]\n}" : "\n  ]\n}";
  return j;
}

int write_tier_files(const std::string& dir, uint64_t present_mask, const uint64_t* tier_count,
                     const uint64_t* tier_bytes, uint64_t n, uint64_t stride, std::string* msg) {
  present_mask &= (1ull << S3IMPH_NUM_TIERS) - 1;
  if (!present_mask) return S3IMPH_OK;  // no tier_stats/, no tiers.json (indexbuild.go:522-524)
  const std::string tdir = dir + "/tier_stats";
  if (!make_dir(tdir)) {
    *msg = "create tier_stats dir: mkdir " + tdir + ": " + std::strerror(errno);
    return S3IMPH_ERR_IO;
  }
  std::string m;
  for (int t = 0; t < S3IMPH_NUM_TIERS; ++t) {
    if (!((present_mask >> t) & 1)) continue;
    if (!write_u64_file(tdir + "/" + kTiers[t].file + "_count.u64", tier_count + t * stride, n, &m)) {
      *msg = std::string("create tier ") + kTiers[t].name + " count writer: " + m;
      return S3IMPH_ERR_IO;
    }
    if (!write_u64_file(tdir + "/" + kTiers[t].file + "_bytes.u64", tier_bytes + t * stride, n, &m)) {
      *msg = std::string("create tier ") + kTiers[t].name + " bytes writer: " + m;
      return S3IMPH_ERR_IO;
    }
  }
  const std::string text = tiers_json(present_mask);
  const std::string path = dir + "/tiers.json";
  const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_TRUNC, 0644);  // os.WriteFile(path, data, 0o644)
  bool ok = fd >= 0;
  for (size_t at = 0; ok && at < text.size();) {
    const ssize_t w = ::write(fd, text.data() + at, text.size() - at);
    if (w < 0 && errno == EINTR) continue;
    ok = w > 0;
    at += ok ? (size_t)w : 0;
  }
  if (fd >= 0 && ::close(fd) != 0) ok = false;
  if (!ok) {
    *msg = "write tier manifest: write tier manifest: open " + path + ": " + std::strerror(errno);
    return S3IMPH_ERR_IO;
  }
  return S3IMPH_OK;
}

int read_tier_manifest(const std::string& dir, std::vector<TierEntry>* out, std::string* msg) {
  out->clear();
  const std::string path = dir + "/tiers.json";
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    if (errno == ENOENT) return S3IMPH_OK;  // no tier data (tiers.go:157-159)
    *msg = "read tier manifest: read tier manifest: open " + path + ": " + std::strerror(errno);
    return S3IMPH_ERR_IO;
  }
  std::string text;
  char b[1 << 14];
  for (size_t r; (r = std::fread(b, 1, sizeof b, f)) > 0;) text.append(b, r);
  std::fclose(f);
  JsonIn j{text};
  auto bad = [&](const std::string& what) {
    *msg = "read tier manifest: parse tier manifest: " + what;
    return (int)S3IMPH_ERR_FORMAT;
  };
  std::string shape;  // a well-formed text of the wrong shape (json.Unmarshal's type errors)
  char kind;
  std::string t;
  auto entry = [&]() -> bool {
    TierEntry e;
    char k1;
    std::string t1;
    const bool ok = j.value(&k1, &t1, [&](const std::string& key) -> bool {
      char k2;
      std::string t2;
      if (!j.value(&k2, &t2)) return false;
      if (k2 == 'l' && t2 == "null") return true;  // null leaves the field alone
      if (same_fold(key, "id")) {
        if (k2 != 'n' || t2.find_first_not_of("0123456789") != std::string::npos || t2.size() > 3 ||
            std::stoul(t2) > 255) {
          if (shape.empty())
            shape = "json: cannot unmarshal " + (k2 == 'n' ? "number " + t2 : std::string("value")) +
                    " into Go struct field Info.tiers.id of type tiers.ID";
        } else {
          e.id = (unsigned)std::stoul(t2);
        }
      } else if (same_fold(key, "name") || same_fold(key, "file")) {
        if (k2 != 's') {
          if (shape.empty()) shape = "json: cannot unmarshal value into Go struct field Info.tiers." + key +
                                     " of type string";
        } else {
          (same_fold(key, "name") ? e.name : e.file) = t2;
        }
      }
      return true;
    });
    if (!ok) return false;
    if (k1 != 'o' && !(k1 == 'l' && t1 == "null") && shape.empty())
      shape = "json: cannot unmarshal value into Go struct field TierManifest.tiers of type tiers.Info";
    out->push_back(e);
    return true;
  };
  const bool ok = j.value(&kind, &t, [&](const std::string& key) -> bool {
    if (!same_fold(key, "tiers")) {
      char k2;
      std::string t2;
      return j.value(&k2, &t2);
    }
    out->clear();
    char k2;
    std::string t2;
    if (!j.value(&k2, &t2, nullptr, entry)) return false;
    if (k2 != 'a' && !(k2 == 'l' && t2 == "null") && shape.empty())
      shape = "json: cannot unmarshal value into Go struct field TierManifest.tiers of type []tiers.Info";
    return true;
  });
  if (ok) {
    j.ws();
    if (j.i != text.size()) j.fail("invalid character after top-level value");
  }
  if (!j.err.empty() || !ok) return bad(j.err.empty() ? "malformed JSON" : j.err);
  if (kind != 'o' && !(kind == 'l' && t == "null") && shape.empty())
    shape = "json: cannot unmarshal value into Go value of type tiers.TierManifest";
  if (!shape.empty()) return bad(shape);
  return S3IMPH_OK;
}

}  // namespace s3imph

using namespace s3imph;

extern "C" {

int s3imph_tier_from_s3(const char* storage_class, const char* access_tier) {
  const std::string sc = trimmed(storage_class), at = trimmed(access_tier);
  return tier_from_trimmed(reinterpret_cast<const unsigned char*>(sc.data()), (unsigned)std::min<size_t>(sc.size(), kTierNameMax + 1),
                           reinterpret_cast<const unsigned char*>(at.data()), (unsigned)std::min<size_t>(at.size(), kTierNameMax + 1));
}

const char* s3imph_tier_name(int id) { return id >= 0 && id < S3IMPH_NUM_TIERS ? kTiers[id].name : nullptr; }

const char* s3imph_tier_file(int id) { return id >= 0 && id < S3IMPH_NUM_TIERS ? kTiers[id].file : nullptr; }

int s3imph_write_tier_files(const char* out_dir, uint64_t present_mask, const uint64_t* tier_count,
                            const uint64_t* tier_bytes, uint64_t n, uint64_t stride, char* err, size_t errlen) {
  if (!out_dir || stride < n || ((present_mask & 0xfff) && n && (!tier_count || !tier_bytes))) return S3IMPH_ERR_INVALID;
  std::string msg;
  const int rc = write_tier_files(out_dir, present_mask, tier_count, tier_bytes, n, stride, &msg);
  if (rc != S3IMPH_OK) set_err(err, errlen, msg);
  return rc;
}

}  // extern "C"
