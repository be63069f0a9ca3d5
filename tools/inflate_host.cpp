// inflate_host.cpp — the decode functions of s3imph_inflate.h driven on the host, one gzip file
// through step() as lane 0 of k_inflate drives it (s3imph_inflate.hip), with a host
// copy of the stage logic and everything the wave does in parallel done serially.  For the CPU
// test of those functions (tests/test_inflate_host.py, built there with the sanitizers) and for
// looking at a stream that decodes wrongly.
//
//   inflate_host FILE BATCH WINDOW...
//
// BATCH is the symbol queue's capacity.  Each WINDOW is a run of its own: the reader sees
// WINDOW bytes of the file from its position rounded down to four, in a buffer of exactly the
// window's size, filled anew whenever br_ready() is false; 0 is the whole file.  Per run one line
//   window=W status=S out_bytes=N in_used=N members=N crc32=N steps=N text=N
// and then the N bytes of text and a newline.  Exit status 0 when every run ended, whatever its
// status; 2 for bad arguments; 3 when a run took more than 64 + 16 x (bits in the file) steps,
// which the termination argument at step() rules out; 4 when a refill left br_ready() false.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "s3imph_inflate.h"

using namespace s3imph::inflate;

namespace {

constexpr uint32_t kCrcChunk = 8192;  // as k_crc32_chunks and k_crc32_fold cut the text

struct Stage {
  std::vector<uint8_t> buf;  // exactly the window: a read outside it is one the sanitizer sees
};

void load_stage(Stage& st, const std::vector<uint8_t>& file, uint64_t window, uint64_t pos, BitReader& r) {
  const uint64_t base = pos & ~3ull;
  const uint64_t lim = base + window < file.size() ? base + window : file.size();
  std::vector<uint8_t>(file.begin() + (base < lim ? base : lim), file.begin() + lim).swap(st.buf);
  r.win = st.buf.data();
  r.base = (int64_t)base;
  r.lim = lim;
}

template <class H>
bool build(H& h, const uint8_t* lens, uint32_t n) {
  huff_count(h, lens, n, 0, 1);
  if (!huff_plan(h, n)) return false;
  huff_place(h, lens, n, 0, 1);
  return true;
}

void carry_out(const std::vector<uint32_t>& q, uint32_t nq, std::vector<uint8_t>& out) {
  for (uint32_t i = 0; i < nq; ++i) {
    const uint32_t s = q[i];
    if (!(s & kMatch)) {
      out.push_back((uint8_t)s);
      continue;
    }
    const uint32_t len = s & 0x1FF, dist = (s & ~kMatch) >> 9;
    if (dist == 0 || dist > out.size()) {
      std::fprintf(stderr, "inflate_host: step() queued distance %u at byte %zu\n", dist, out.size());
      std::exit(5);
    }
    for (uint32_t k = 0; k < len; ++k) out.push_back(out[out.size() - dist]);
  }
}

// The CRC-32 of the text as the two CRC kernels make it: per chunk, folded with crc_concat.
uint32_t text_crc(const std::vector<uint8_t>& out) {
  const uint32_t xfull = crc_xpow8(kCrcChunk);
  uint32_t c = 0;
  for (uint64_t lo = 0; lo < out.size(); lo += kCrcChunk) {
    const uint64_t n = out.size() - lo < kCrcChunk ? out.size() - lo : kCrcChunk;
    uint32_t cc = ~0u;
    for (uint64_t k = 0; k < n; ++k) cc = crc_byte(cc, out[lo + k]);
    c = crc_concat(c, ~cc, n == kCrcChunk ? xfull : crc_xpow8(n));
  }
  return c;
}

int run(const std::vector<uint8_t>& file, uint32_t batch, uint64_t window_arg) {
  const uint64_t window = window_arg ? window_arg : file.size() + 4;
  const uint64_t max_steps = 64 + 16 * 8 * (uint64_t)file.size();
  Dec d;
  BitReader r{};
  r.len = file.size();
  Tabs* t = new Tabs();
  Stage st;
  std::vector<uint32_t> q(batch);
  std::vector<uint8_t> out;
  uint32_t nq = 0;
  uint64_t steps = 0;
  load_stage(st, file, window, 0, r);
  for (;;) {
    if (!br_ready(r)) {
      load_stage(st, file, window, r.pos, r);
      if (!br_ready(r)) {
        std::fprintf(stderr, "inflate_host: window %" PRIu64 ": a refill at byte %" PRIu64 " is not ready\n", window_arg,
                     (uint64_t)r.pos);
        return 4;
      }
    }
    uint32_t ev = step(d, r, *t, q.data(), &nq, batch);
    if (++steps > max_steps) {
      std::fprintf(stderr, "inflate_host: window %" PRIu64 ": more than %" PRIu64 " steps\n", window_arg, max_steps);
      return 3;
    }
    if (ev == kCont) continue;
    carry_out(q, nq, out);
    nq = 0;
    if (ev == kStored) {
      out.insert(out.end(), file.begin() + d.ssrc, file.begin() + d.ssrc + d.slen);  // step() checked the end
    } else if (ev == kBuildCl || ev == kBuildFixed || ev == kBuildDyn) {
      bool ok;
      if (ev == kBuildCl) {
        ok = build(t->cl, t->cllens, 19);
      } else {
        uint32_t nl = d.nlen, nd = d.ndist;
        if (ev == kBuildFixed) {
          nl = 288, nd = 32;
          for (uint32_t i = 0; i < 320; ++i) t->lens[i] = fixed_len(i);
        }
        ok = build(t->ll, t->lens, nl);
        ok = build(t->dd, t->lens + nl, nd) && ok;
      }
      if (!ok) {
        d.status = kData;
        ev = kEnd;
      }
    }
    if (ev == kEnd) break;
  }
  uint32_t status = d.status;
  if (status == kOk && text_crc(out) != d.crc_file) status = kChecksum;
  std::printf("window=%" PRIu64 " status=%u out_bytes=%" PRIu64 " in_used=%" PRIu64 " members=%u crc32=%u steps=%" PRIu64
              " text=%zu\n",
              window_arg, status, (uint64_t)d.fout, (uint64_t)br_byte_pos(r), d.members, d.crc_file, steps, out.size());
  if (!out.empty()) std::fwrite(out.data(), 1, out.size(), stdout);
  std::fputc('\n', stdout);
  delete t;
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: inflate_host FILE BATCH WINDOW...\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> file;
  uint8_t chunk[65536];
  for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + n);
  std::fclose(f);
  const uint32_t batch = (uint32_t)std::strtoul(argv[2], nullptr, 10);
  if (batch == 0) return 2;
  for (int a = 3; a < argc; ++a) {
    const uint64_t window = std::strtoull(argv[a], nullptr, 10);
    if (window && window < 4 * kStepBytes) {  // a refill must leave a step's bytes
      std::fprintf(stderr, "inflate_host: a window has at least %u bytes\n", 4 * kStepBytes);
      return 2;
    }
    if (const int rc = run(file, batch, window)) return rc;
  }
  return 0;
}
