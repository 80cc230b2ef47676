// Host emulation of the scan share of gather_struct_kernel (gather_device.h scan::), a stand-alone
// program that tests/test_scan_index_host.py compiles with the host compiler and
// -fsanitize=address,undefined and runs once per case; it is part of no library.
//
// It builds scan::Args and then does what kernels.hip's scan_share does, thread by thread and
// phase by phase — head, then per tile the load phase of all 256 threads, the kSteps doubling
// steps (each a phase of its own, as the barriers make them) and the store phase — through a
// memory policy that performs nothing unchecked:
//   (a) every input index lies in [0, count);
//   (b) every LDS index lies inside the scan's two rows, every slot read was written earlier in
//       this tile, and inside one phase no slot is written by two threads or written by one
//       and read by another (the barriers are the only ordering the kernel has);
//   (c) every output word below count + 1 (lengths) / count (offsets) is written exactly once and
//       none at or past it is written;
//   (d) every thread leaves a tile with the same carry;
//   (e) the words are written to `out_file` for the caller to compare with the formula.
//
//   scan_emulate count n wide offsets in_file out_file
//
// `in_file` holds `count` little-endian words of 4 (wide 0) or 8 bytes.  Exit status 0 and "ok"
// when every check held.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gather_device.h"

namespace {

namespace sc = dora::gather::scan;
constexpr uint32_t kThreads = dora::gather::kThreads;

[[noreturn]] void die(const char* what, int64_t a, int64_t b) {
  std::printf("FAIL %s (%" PRId64 ", %" PRId64 ")\n", what, a, b);
  std::exit(1);
}

struct EmuScan {
  std::vector<uint8_t> in;
  uint64_t count, words;  // input words, output words
  bool wide;
  std::vector<uint32_t> out;
  std::vector<uint8_t> writes;
  uint64_t lds[sc::kLds];
  uint64_t stamp[sc::kLds];  // tile + 1 of the last write
  // who touched a slot in the current phase: 0 nobody, thread + 1, or kMany
  static constexpr uint32_t kMany = 0xffffffffu;
  uint32_t rd[sc::kLds], wr[sc::kLds];
  uint64_t tile = 0;
  uint32_t thread = 0;
  uint64_t loads = 0;

  void begin_phase() {
    std::memset(rd, 0, sizeof(rd));
    std::memset(wr, 0, sizeof(wr));
  }
  void end_phase(const char* phase) {
    for (int i = 0; i < sc::kLds; ++i) {
      if (wr[i] == kMany) die("LDS slot written by two threads in one phase", i, int64_t(tile));
      if (wr[i] && rd[i] && rd[i] != wr[i]) {
        std::printf("(%s phase) ", phase);
        die("LDS slot written and read by different threads in one phase", i, int64_t(tile));
      }
    }
  }
  int64_t load_word(uint64_t i) {
    if (i >= count) die("input index outside [0, count)", int64_t(i), int64_t(count));
    ++loads;
    if (wide) {
      int64_t v;
      std::memcpy(&v, in.data() + 8 * i, 8);
      return v;
    }
    int32_t v;
    std::memcpy(&v, in.data() + 4 * i, 4);
    return v;
  }
  void lds_write(uint32_t i, uint64_t v) {
    if (i >= uint32_t(sc::kLds)) die("LDS index outside the buffer (write)", i, thread);
    wr[i] = wr[i] && wr[i] != thread + 1 ? kMany : thread + 1;
    lds[i] = v;
    stamp[i] = tile + 1;
  }
  uint64_t lds_read(uint32_t i) {
    if (i >= uint32_t(sc::kLds)) die("LDS index outside the buffer (read)", i, thread);
    if (stamp[i] != tile + 1) die("LDS slot read before this tile wrote it", i, int64_t(tile));
    rd[i] = rd[i] && rd[i] != thread + 1 ? kMany : thread + 1;
    return lds[i];
  }
  void store_word(uint64_t i, uint32_t v) {
    if (i >= words) die("output word at or past the offsets buffer", int64_t(i), int64_t(words));
    if (++writes[i] != 1) die("output word written twice", int64_t(i), 0);
    out[i] = v;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc != 7) {
    std::printf("usage: see the file's head\n");
    return 2;
  }
  dora::ScanDesc d{};
  d.count = std::strtoull(argv[1], nullptr, 10);
  d.n = std::strtoull(argv[2], nullptr, 10);
  d.wide = std::strtoul(argv[3], nullptr, 10) ? 1 : 0;
  d.offsets = std::strtoul(argv[4], nullptr, 10) ? 1 : 0;
  if (d.count > dora::kMaxScanEntries || d.n >> 31 || (d.offsets && !d.count)) {
    std::printf("FAIL bad case\n");
    return 2;
  }
  EmuScan m{};
  m.count = d.count;
  m.wide = d.wide;
  m.in.resize(d.count * (d.wide ? 8 : 4));
  if (!m.in.empty()) {
    FILE* f = std::fopen(argv[5], "rb");
    if (!f || std::fread(m.in.data(), 1, m.in.size(), f) != m.in.size()) {
      std::printf("FAIL input file: %zu bytes expected\n", m.in.size());
      return 2;
    }
    std::fclose(f);
  }
  // (only alignment matters of the addresses; neither is dereferenced)
  d.src = reinterpret_cast<const uint8_t*>(uintptr_t(0x7f1234560000));
  const sc::Args a = sc::make_args(d, reinterpret_cast<uint8_t*>(uintptr_t(0x7f0000001000)));
  m.words = sc::out_words(a);
  if (m.words != d.count + (d.offsets ? 0 : 1)) die("output word count", int64_t(m.words), 0);
  m.out.assign(m.words, 0xA5A5A5A5u);
  m.writes.assign(m.words, 0);

  for (m.thread = 0; m.thread < kThreads; ++m.thread) sc::head(a, m.thread, m);
  std::vector<sc::Local> loc(kThreads);
  std::vector<uint64_t> carry(kThreads, 0);
  const uint64_t nt = sc::tiles(a);
  for (m.tile = 0; m.tile < nt; ++m.tile) {
    m.begin_phase();
    for (m.thread = 0; m.thread < kThreads; ++m.thread)
      sc::load_phase(a, m.tile, m.thread, loc[m.thread], m);
    m.end_phase("load");
    for (int step = 0; step < sc::kSteps; ++step) {
      m.begin_phase();
      for (m.thread = 0; m.thread < kThreads; ++m.thread) sc::step_phase(a, m.thread, step, m);
      m.end_phase("step");
    }
    m.begin_phase();
    for (m.thread = 0; m.thread < kThreads; ++m.thread)
      carry[m.thread] = sc::store_phase(a, m.tile, m.thread, loc[m.thread], carry[m.thread], m);
    m.end_phase("store");
    for (uint32_t t = 1; t < kThreads; ++t)
      if (carry[t] != carry[0]) die("threads disagree on the carry", t, int64_t(m.tile));
    if (carry[0] > d.n) die("carry past the clamp", int64_t(carry[0]), int64_t(d.n));
  }
  for (uint64_t i = 0; i < m.words; ++i)
    if (m.writes[i] != 1) die("output word never written", int64_t(i), 0);
  FILE* f = std::fopen(argv[6], "wb");
  if (!f || (m.words && std::fwrite(m.out.data(), 4, m.words, f) != m.words)) {
    std::printf("FAIL output file\n");
    return 2;
  }
  std::fclose(f);
  std::printf("ok words=%" PRIu64 " tiles=%" PRIu64 " loads=%" PRIu64 "\n", m.words, nt, m.loads);
  return 0;
}
