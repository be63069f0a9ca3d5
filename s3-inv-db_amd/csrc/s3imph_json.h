// s3imph_json.h — the small JSON reader of the host code: tiers.json (s3imph_tiers.cpp) and the
// price table (s3imph_pricing.cpp).  Not part of the ABI.
#pragma once

#include <cstring>
#include <functional>
#include <string>

namespace s3imph {

// A reader for the JSON files: any JSON value is accepted and skipped; for tiers.json the fields of
// {"tiers": [{"id": .., "name": "..", "file": ".."}]} are taken (field names matched without
// regard to case, as encoding/json does).
struct JsonIn {
  const std::string& s;
  size_t i = 0;
  std::string err;
  bool fail(const std::string& m) {
    if (err.empty()) err = m;
    return false;
  }
  void ws() {
    while (i < s.size() && (s[i] == ' ' || s[i] == '\n' || s[i] == '\r' || s[i] == '\t')) ++i;
  }
  bool lit(const char* w) {
    const size_t k = std::strlen(w);
    if (s.compare(i, k, w) != 0) return fail(std::string("invalid character near offset ") + std::to_string(i));
    i += k;
    return true;
  }
  bool str(std::string* out) {
    if (i >= s.size() || s[i] != '"') return fail("expected a string at offset " + std::to_string(i));
    for (++i; i < s.size() && s[i] != '"'; ++i) {
      if ((unsigned char)s[i] < 0x20) return fail("invalid character in string literal");
      if (s[i] == '\\') {
        if (++i >= s.size()) break;
        switch (s[i]) {
          case 'n': *out += '\n'; break;
          case 't': *out += '\t'; break;
          case 'r': *out += '\r'; break;
          case 'b': *out += '\b'; break;
          case 'f': *out += '\f'; break;
          case '"': case '\\': case '/': *out += s[i]; break;
          case 'u': {
            if (i + 4 >= s.size()) return fail("unexpected end of JSON input");
            unsigned v = 0;
            for (int k = 1; k <= 4; ++k) {
              const char ch = s[i + k];
              const int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10
                            : ch >= 'A' && ch <= 'F' ? ch - 'A' + 10 : -1;
              if (d < 0) return fail("invalid character in \\u escape");
              v = v * 16 + (unsigned)d;
            }
            i += 4;
            // tier names and file prefixes are ASCII; anything else is kept as UTF-8 of the BMP
            if (v < 0x80) {
              *out += (char)v;
            } else if (v < 0x800) {
              *out += (char)(0xc0 | (v >> 6));
              *out += (char)(0x80 | (v & 0x3f));
            } else {
              *out += (char)(0xe0 | (v >> 12));
              *out += (char)(0x80 | ((v >> 6) & 0x3f));
              *out += (char)(0x80 | (v & 0x3f));
            }
            break;
          }
          default: return fail("invalid character in string escape code");
        }
      } else {
        *out += s[i];
      }
    }
    if (i >= s.size()) return fail("unexpected end of JSON input");
    ++i;
    return true;
  }
  // a number's text (validated: -?digits[.digits][e[+-]digits])
  bool num(std::string* out) {
    const size_t b = i;
    if (i < s.size() && s[i] == '-') ++i;
    size_t d = i;
    while (i < s.size() && s[i] >= '0' && s[i] <= '9') ++i;
    if (i == d) return fail("invalid character near offset " + std::to_string(i));
    if (i < s.size() && s[i] == '.') {
      d = ++i;
      while (i < s.size() && s[i] >= '0' && s[i] <= '9') ++i;
      if (i == d) return fail("invalid character after decimal point in numeric literal");
    }
    if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
      ++i;
      if (i < s.size() && (s[i] == '+' || s[i] == '-')) ++i;
      d = i;
      while (i < s.size() && s[i] >= '0' && s[i] <= '9') ++i;
      if (i == d) return fail("invalid character in exponent of numeric literal");
    }
    *out = s.substr(b, i - b);
    return true;
  }
  // Any value.  kind: 's' string, 'n' number, 'o' object, 'a' array, 'l' true / false / null;
  // text: the string's or the number's.  on_member / on_item (nullable) see an object's members
  // and an array's items with the reader standing at the value, and consume it.
  using Member = std::function<bool(const std::string&)>;
  using Item = std::function<bool()>;
  bool value(char* kind, std::string* text, const Member& on_member = nullptr, const Item& on_item = nullptr,
             int depth = 0) {
    ws();
    if (i >= s.size()) return fail("unexpected end of JSON input");
    if (depth > 64) return fail("exceeded max depth");
    const char ch = s[i];
    if (ch == '"') {
      *kind = 's';
      text->clear();
      return str(text);
    }
    if (ch == '-' || (ch >= '0' && ch <= '9')) {
      *kind = 'n';
      return num(text);
    }
    if (ch == 't' || ch == 'f' || ch == 'n') {
      *kind = 'l';
      *text = ch == 't' ? "true" : ch == 'f' ? "false" : "null";
      return lit(text->c_str());
    }
    if (ch == '{') {
      *kind = 'o';
      ++i;
      ws();
      if (i < s.size() && s[i] == '}') return ++i, true;
      for (;;) {
        ws();
        std::string key;
        if (!str(&key)) return false;
        ws();
        if (i >= s.size() || s[i] != ':') return fail("invalid character after object key");
        ++i;
        if (on_member) {
          if (!on_member(key)) return false;
        } else {
          char k2;
          std::string t2;
          if (!value(&k2, &t2, nullptr, nullptr, depth + 1)) return false;
        }
        ws();
        if (i < s.size() && s[i] == ',') {
          ++i;
          continue;
        }
        if (i < s.size() && s[i] == '}') return ++i, true;
        return fail(i >= s.size() ? "unexpected end of JSON input" : "invalid character after object key:value pair");
      }
    }
    if (ch == '[') {
      *kind = 'a';
      ++i;
      ws();
      if (i < s.size() && s[i] == ']') return ++i, true;
      for (;;) {
        if (on_item) {
          if (!on_item()) return false;
        } else {
          char k2;
          std::string t2;
          if (!value(&k2, &t2, nullptr, nullptr, depth + 1)) return false;
        }
        ws();
        if (i < s.size() && s[i] == ',') {
          ++i;
          continue;
        }
        if (i < s.size() && s[i] == ']') return ++i, true;
        return fail(i >= s.size() ? "unexpected end of JSON input" : "invalid character after array element");
      }
    }
    return fail(std::string("invalid character '") + ch + "' looking for beginning of value");
  }
};

// key == name without regard to ASCII letter case (name is lower case)
inline bool same_fold(const std::string& a, const char* b) {
  if (a.size() != std::strlen(b)) return false;
  for (size_t k = 0; k < a.size(); ++k) {
    char ch = a[k];
    if (ch >= 'A' && ch <= 'Z') ch = (char)(ch - 'A' + 'a');
    if (ch != b[k]) return false;
  }
  return true;
}

}  // namespace s3imph
