// s3imph_pricing.cpp — the host side of the cost estimate (include/s3imph.h section 5h):
// DefaultUSEast1Prices, LoadPriceTable and SavePriceTable (pkg/pricing/pricing.go:67-122) and
// ComputeMonthlyCost (:159-240) over the shared slot arithmetic of s3imph_pricing.h.  No device
// call here.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "s3imph_internal.h"
#include "s3imph_json.h"
#include "s3imph_pricing.h"

namespace s3imph {
namespace {

int tier_by_name(const std::string& name) {
  for (int t = 0; t < S3IMPH_NUM_TIERS; ++t)
    if (name == s3imph_tier_name(t)) return t;
  return -1;
}

// A JSON number's text as a double; false when it is outside double's range (Go's ParseFloat
// range error).  A value that underflows is its nearest double, as in Go.
bool json_double(const std::string& t, double* v) {
  const auto r = std::from_chars(t.data(), t.data() + t.size(), *v);
  if (r.ec == std::errc()) return true;
  *v = std::strtod(t.c_str(), nullptr);  // out of range: which side?
  return std::isfinite(*v);
}

// encoding/json's float64 text: shortest round trip, 'f' for 1e-6 <= |v| < 1e21 (and 0), else
// 'e' with the leading zero of a two-digit negative exponent dropped (encode.go floatEncoder).
std::string json_number(double v) {
  if (v == 0) return "0";
  char buf[64];
  const auto r = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific);  // d[.ddd]e+XX, shortest
  std::string s(buf, r.ptr);
  const double a = std::fabs(v);
  if (a < 1e-6 || a >= 1e21) {
    const size_t n = s.size();
    if (n >= 4 && s[n - 4] == 'e' && s[n - 3] == '-' && s[n - 2] == '0') s.erase(n - 2, 1);
    return s;
  }
  // 'f' from the same shortest digits (to_chars' own fixed form writes a large value's exact
  // digits, Go pads the shortest ones with zeros)
  const size_t e = s.find('e');
  const int exp10 = std::atoi(s.c_str() + e + 1);
  std::string digits;
  for (size_t k = 0; k < e; ++k)
    if (s[k] >= '0' && s[k] <= '9') digits += s[k];
  const std::string sign = v < 0 ? "-" : "";
  const int point = exp10 + 1;  // digits before the decimal point
  if (point <= 0) return sign + "0." + std::string((size_t)-point, '0') + digits;
  if ((size_t)point >= digits.size()) return sign + digits + std::string((size_t)point - digits.size(), '0');
  return sign + digits.substr(0, (size_t)point) + "." + digits.substr((size_t)point);
}

std::string price_table_json(const s3imph_price_table& pt) {
  // map keys in byte order
  std::vector<std::pair<std::string, double>> m;
  for (int t = 0; t < S3IMPH_NUM_TIERS; ++t)
    if ((pt.priced_mask >> t) & 1) m.emplace_back(s3imph_tier_name(t), pt.per_gb_month[t]);
  std::sort(m.begin(), m.end());
  std::string j = "{\n  \"per_gb_month\": {";
  for (size_t k = 0; k < m.size(); ++k)
    j += std::string(k ? ",\n" : "\n") + "    \"" + m[k].first + "\": " + json_number(m[k].second);
  j += m.empty() ? "},\n" : "\n  },\n";
  j += "  \"monitoring_per_1000_objects\": " + json_number(pt.monitoring_per_1000_objects) + ",\n";
  j += "  \"standard_price_per_gb\": " + json_number(pt.standard_price_per_gb) + "\n}";
  return j;
}

// json.Unmarshal(data, &PriceTable{}) restated; *msg is the text after "parse price table: ".
bool parse_price_table(const std::string& text, s3imph_price_table* pt, std::string* msg) {
  JsonIn j{text};
  std::string shape;  // well-formed text of the wrong shape, a number out of range, a negative value
  auto number = [&](const char* field, char kind, const std::string& t, double* out) {
    if (kind == 'l' && t == "null") return;  // null leaves the field alone
    double v = 0;
    if (kind != 'n') {
      if (shape.empty())
        shape = std::string("json: cannot unmarshal value into Go struct field PriceTable.") + field + " of type float64";
    } else if (!json_double(t, &v)) {
      if (shape.empty())
        shape = "json: cannot unmarshal number " + t + " into Go struct field PriceTable." + field + " of type float64";
    } else if (v < 0) {
      if (shape.empty()) shape = std::string("negative value ") + t + " in " + field;
    } else {
      *out = v;
    }
  };
  char kind;
  std::string t;
  const bool ok = j.value(&kind, &t, [&](const std::string& key) -> bool {
    char k2;
    std::string t2;
    if (same_fold(key, "per_gb_month")) {
      const bool in = j.value(&k2, &t2, [&](const std::string& name) -> bool {
        char k3;
        std::string t3;
        if (!j.value(&k3, &t3)) return false;
        double v = 0;
        if (!(k3 == 'l' && t3 == "null")) number("per_gb_month", k3, t3, &v);  // null: the key with 0
        const int id = tier_by_name(name);
        if (id >= 0) {  // a name that is none of the twelve is ignored
          pt->per_gb_month[id] = v;
          pt->priced_mask |= 1u << id;
        }
        return true;
      });
      if (!in) return false;
      if (k2 != 'o' && !(k2 == 'l' && t2 == "null") && shape.empty())
        shape = "json: cannot unmarshal value into Go struct field PriceTable.per_gb_month of type map[string]float64";
      return true;
    }
    if (!j.value(&k2, &t2)) return false;
    if (same_fold(key, "monitoring_per_1000_objects"))
      number("monitoring_per_1000_objects", k2, t2, &pt->monitoring_per_1000_objects);
    else if (same_fold(key, "standard_price_per_gb"))
      number("standard_price_per_gb", k2, t2, &pt->standard_price_per_gb);
    return true;  // an unknown field is skipped
  });
  if (ok) {
    j.ws();
    if (j.i != text.size()) j.fail("invalid character after top-level value");
  }
  if (!j.err.empty() || !ok) {
    *msg = j.err.empty() ? "malformed JSON" : j.err;
    return false;
  }
  if (kind != 'o' && !(kind == 'l' && t == "null") && shape.empty())
    shape = "json: cannot unmarshal value into Go value of type pricing.PriceTable";
  *msg = shape;
  return shape.empty();
}

}  // namespace
}  // namespace s3imph

using namespace s3imph;

extern "C" {

int s3imph_price_table_default(s3imph_price_table* pt) {
  if (!pt) return S3IMPH_ERR_INVALID;
  std::memset(pt, 0, sizeof *pt);
  pt->per_gb_month[S3IMPH_TIER_STANDARD] = 0.023;
  pt->per_gb_month[S3IMPH_TIER_STANDARD_IA] = 0.0125;
  pt->per_gb_month[S3IMPH_TIER_ONEZONE_IA] = 0.01;
  pt->per_gb_month[S3IMPH_TIER_REDUCED_REDUNDANCY] = 0.024;
  pt->per_gb_month[S3IMPH_TIER_GLACIER_IR] = 0.004;
  pt->per_gb_month[S3IMPH_TIER_GLACIER_FR] = 0.0036;
  pt->per_gb_month[S3IMPH_TIER_DEEP_ARCHIVE] = 0.00099;
  pt->per_gb_month[S3IMPH_TIER_IT_FREQUENT] = 0.023;
  pt->per_gb_month[S3IMPH_TIER_IT_INFREQUENT] = 0.0125;
  pt->per_gb_month[S3IMPH_TIER_IT_ARCHIVE_INSTANT] = 0.004;
  pt->per_gb_month[S3IMPH_TIER_IT_ARCHIVE] = 0.0036;
  pt->per_gb_month[S3IMPH_TIER_IT_DEEP_ARCHIVE] = 0.00099;
  pt->priced_mask = (1u << S3IMPH_NUM_TIERS) - 1;
  pt->monitoring_per_1000_objects = 0.0025;
  pt->standard_price_per_gb = 0.023;
  return S3IMPH_OK;
}

int s3imph_price_table_load(const char* path, s3imph_price_table* pt, char* err, size_t errlen) {
  if (!path || !pt) {
    set_err(err, errlen, "invalid argument");
    return S3IMPH_ERR_INVALID;
  }
  std::memset(pt, 0, sizeof *pt);
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    set_err(err, errlen, std::string("read price table: open ") + path + ": " + std::strerror(errno));
    return S3IMPH_ERR_IO;
  }
  std::string text;
  char b[1 << 14];
  for (size_t r; (r = std::fread(b, 1, sizeof b, f)) > 0;) text.append(b, r);
  const bool bad = std::ferror(f) != 0;
  std::fclose(f);
  if (bad) {
    set_err(err, errlen, std::string("read price table: read ") + path);
    return S3IMPH_ERR_IO;
  }
  s3imph_price_table got{};
  std::string msg;
  if (!parse_price_table(text, &got, &msg)) {
    set_err(err, errlen, "parse price table: " + msg);
    return S3IMPH_ERR_FORMAT;
  }
  *pt = got;
  return S3IMPH_OK;
}

int s3imph_price_table_save(const char* path, const s3imph_price_table* pt, char* err, size_t errlen) {
  if (!path || !pt) {
    set_err(err, errlen, "invalid argument");
    return S3IMPH_ERR_INVALID;
  }
  if (*price_table_fault(*pt)) {  // json.Marshal refuses NaN and Inf as well
    set_err(err, errlen, std::string("marshal price table: pricing: ") + price_table_fault(*pt));
    return S3IMPH_ERR_INVALID;
  }
  const std::string text = price_table_json(*pt);
  const int fd = ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644);  // os.WriteFile(path, data, 0o644)
  bool ok = fd >= 0;
  for (size_t at = 0; ok && at < text.size();) {
    const ssize_t w = ::write(fd, text.data() + at, text.size() - at);
    if (w < 0 && errno == EINTR) continue;
    ok = w > 0;
    at += ok ? (size_t)w : 0;
  }
  const int saved = errno;
  if (fd >= 0 && ::close(fd) != 0) ok = false;
  if (!ok) {
    set_err(err, errlen, std::string("write price table: open ") + path + ": " + std::strerror(saved));
    return S3IMPH_ERR_IO;
  }
  return S3IMPH_OK;
}

int s3imph_compute_monthly_cost(const uint8_t* ids, const uint64_t* count, const uint64_t* bytes, uint64_t T,
                                const s3imph_price_table* pt, s3imph_cost* out) {
  if (!pt || !out || T > (uint64_t)S3IMPH_NUM_TIERS || (T && (!ids || !count || !bytes)) || *price_table_fault(*pt))
    return S3IMPH_ERR_INVALID;
  unsigned seen = 0;
  for (uint64_t s = 0; s < T; ++s) {
    if (ids[s] >= S3IMPH_NUM_TIERS || ((seen >> ids[s]) & 1)) return S3IMPH_ERR_INVALID;
    seen |= 1u << ids[s];
  }
  s3imph_cost r{};
  for (uint64_t s = 0; s < T; ++s) {
    const SlotCost c = price_slot(ids[s], count[s], bytes[s], *pt);
    r.per_tier[ids[s]] = c.tier_total;
    r.total += c.tier_total + c.monitoring;
    r.monitoring += c.monitoring;
    r.min_object_size += c.min_size;
    r.glacier_overhead += c.overhead;
    if (c.priced && (count[s] | bytes[s])) r.tier_mask |= 1u << ids[s];
  }
  r.found = 1;
  *out = r;
  return S3IMPH_OK;
}

}  // extern "C"
