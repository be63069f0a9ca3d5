// s3imph_csv_header.cpp — the header row of an inventory CSV (include/s3imph.h section 5g):
// OpenFileWithOptions' column search (pkg/inventory/reader.go:96-135) over the first record,
// parsed by the byte automaton the device runs (s3imph_csv.hip).  Host only: no
// device call, no HIP header, so a stand-alone program can link this file alone.
#include <string>
#include <vector>

#include "s3imph.h"
#include "s3imph_tiers.h"

namespace s3imph {
void set_err(char* err, size_t errlen, const std::string& msg);  // s3imph_host.cpp
}

namespace {

enum State { R, F, U, Q, E };

// The first record of csv[0 .. len): its fields, and *end = the offset just past it.  False when
// the buffer holds no record (io.EOF).
bool first_record(const uint8_t* csv, uint64_t len, std::vector<std::string>* fields, uint64_t* end) {
  State st = R;
  std::string cur;
  fields->clear();
  for (uint64_t i = 0; i < len; ++i) {
    const uint8_t c = csv[i];
    if (c == '\r' && (i + 1 >= len || csv[i + 1] == '\n')) continue;  // readLine's CRLF rule
    const bool quote = c == '"', comma = c == ',', nl = c == '\n', other = !quote && !comma && !nl;
    if (st == Q) {
      if (quote) st = E;
      else cur += (char)c;
      continue;
    }
    if (st == E && (quote || other)) {  // "" inside quotes, or a lazy quote
      cur += '"';
      if (other) cur += (char)c;
      st = Q;
      continue;
    }
    if (quote) {
      if (st == U) cur += '"';  // a lazy quote in an unquoted field
      else st = Q;
    } else if (other) {
      cur += (char)c;
      st = U;
    } else if (comma) {
      fields->push_back(cur);
      cur.clear();
      st = F;
    } else if (st != R) {  // '\n' ends the record; at a record's start it is an empty line
      fields->push_back(cur);
      *end = i + 1;
      return true;
    }
  }
  if (st == R) return false;
  fields->push_back(cur);
  *end = len;
  return true;
}

// strings.TrimSpace(strings.ToLower(col)) == name, by the library's ASCII rules (s3imph_tiers.h)
bool names(const std::string& col, const char* name) {
  size_t b = 0, e = col.size();
  while (b < e && s3imph::tier_space((unsigned char)col[b])) ++b;
  while (e > b && s3imph::tier_space((unsigned char)col[e - 1])) --e;
  size_t k = 0;
  for (; b + k < e && name[k]; ++k) {
    unsigned char ch = (unsigned char)col[b + k];
    if (ch >= 'A' && ch <= 'Z') ch = (unsigned char)(ch - 'A' + 'a');
    if (ch != (unsigned char)name[k]) return false;
  }
  return b + k == e && !name[k];
}

}  // namespace

extern "C" int s3imph_csv_header_schema(const uint8_t* csv, uint64_t len, s3imph_csv_schema* schema,
                                        uint64_t* data_start, char* err, size_t errlen) {
  if (!schema || !data_start || (len && !csv)) return S3IMPH_ERR_INVALID;
  *schema = s3imph_csv_schema{-1, -1, -1, -1};
  *data_start = 0;
  std::vector<std::string> header;
  uint64_t end = 0;
  if (!first_record(csv, len, &header, &end)) {
    s3imph::set_err(err, errlen, "read CSV header: EOF");
    return S3IMPH_ERR_FORMAT;
  }
  for (size_t i = 0; i < header.size(); ++i) {  // the last match wins (reader.go:109-122)
    if (names(header[i], "key")) schema->key_col = (int32_t)i;
    else if (names(header[i], "size")) schema->size_col = (int32_t)i;
    else if (names(header[i], "storageclass")) schema->storage_col = (int32_t)i;
    else if (names(header[i], "intelligenttieringaccesstier")) schema->access_tier_col = (int32_t)i;
  }
  *data_start = end;
  if (schema->key_col < 0) {
    s3imph::set_err(err, errlen, "CSV header missing 'Key' column");
    return S3IMPH_ERR_FORMAT;
  }
  if (schema->size_col < 0) {
    s3imph::set_err(err, errlen, "CSV header missing 'Size' column");
    return S3IMPH_ERR_FORMAT;
  }
  return S3IMPH_OK;
}
