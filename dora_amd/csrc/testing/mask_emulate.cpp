// Host emulation of mask_count_kernel and mask_compact_kernel (gather_device.h mask::), a
// stand-alone program that tests/test_mask_index_host.py compiles with the host compiler and
// -fsanitize=address,undefined and runs once per group of cases; it is part of no library.
//
// It builds mask::Args and then does what kernels.hip's two kernels do, thread by thread and
// phase by phase as the barriers make them — every workgroup of the count kernel first, then every
// workgroup of the compact kernel in descending order (the kernel boundary is the only ordering
// between workgroups, so no order among them may matter) — through a memory policy that performs
// nothing unchecked:
//   (a) every mask byte read is byte i of the mask with 0 <= i < N (the mask sits in a heap block
//       of exactly N bytes), and a 16-byte load is aligned at the address the kernel would see;
//   (b) every LDS index lies inside the buffer, every slot read was written since the last
//       reduction or scan began, and inside one phase no slot is written by two threads or
//       written by one and read by another;
//   (c) every index word, count word and total written lies inside the workspace: index[0, N),
//       C[0, N], totals[0, tiles);
//   (d) the count kernel writes every index word exactly once (-1) and every total exactly once;
//       the compact kernel reads only totals of tiles before its own;
//   (e) every C word is written exactly once, every set row is scattered exactly once, no index
//       word is scattered to twice, and the sample's two offsets are written once each when the
//       message is one list and never otherwise.
// Per case the index words, the N + 1 counts and the offsets (two words, 0xA5A5A5A5 when not
// written) are appended to `out_file` for the caller to compare with numpy.
//
//   mask_emulate spec_file mask_blob out_file
//
// `spec_file` holds whitespace-separated integers, one case after another:
//   n shift one_list grid blob_offset
// `n` rows whose mask bytes are `mask_blob`[blob_offset, +n), seen by the kernel at an address
// that is `shift` mod 16; `grid` workgroups stride over the tiles (0: one per tile, as launched).
// Exit status 0 and "ok" when every check held in every case.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <vector>

#include "gather_device.h"

namespace {

namespace mk = dora::gather::mask;
using dora::gather::U16;
constexpr uint32_t kThreads = dora::gather::kThreads;

int g_case = 0;

[[noreturn]] void die(const char* what, int64_t a, int64_t b) {
  std::printf("FAIL case %d: %s (%" PRId64 ", %" PRId64 ")\n", g_case, what, a, b);
  std::exit(1);
}

struct EmuMask {
  std::unique_ptr<uint8_t[]> mask;  // exactly N bytes
  uint64_t n, tiles;
  uint32_t shift;
  bool one_list;
  std::vector<int32_t> index;
  std::vector<uint32_t> counts, totals, offsets;
  std::vector<uint8_t> index_fill, index_scatter, count_writes, total_writes, scattered;
  uint8_t offset_writes[2] = {0, 0};
  uint32_t lds[mk::kLds];
  uint64_t stamp[mk::kLds];
  uint64_t epoch = 0;  // the reduction or scan in hand
  static constexpr uint32_t kMany = 0xffffffffu;
  uint32_t rd[mk::kLds], wr[mk::kLds];
  bool compacting = false;
  uint64_t tile = 0;
  uint32_t thread = 0;
  uint64_t loads16 = 0, loads1 = 0;

  void begin_phase() {
    std::memset(rd, 0, sizeof(rd));
    std::memset(wr, 0, sizeof(wr));
  }
  void end_phase(const char* phase) {
    for (int i = 0; i < mk::kLds; ++i) {
      if (wr[i] == kMany) die("LDS slot written by two threads in one phase", i, int64_t(tile));
      if (wr[i] && rd[i] && rd[i] != wr[i]) {
        std::printf("(%s phase) ", phase);
        die("LDS slot written and read by different threads in one phase", i, int64_t(tile));
      }
    }
  }
  U16 load16(uint64_t v) {
    if (v % 16) die("16-byte mask load off its alignment", int64_t(v), shift);
    if (v < shift || v - shift + 16 > n)
      die("16-byte mask load outside [0, N)", int64_t(v) - int64_t(shift), int64_t(n));
    ++loads16;
    U16 u;
    std::memcpy(u.w, mask.get() + (v - shift), 16);
    return u;
  }
  uint8_t load_byte(uint64_t row) {
    if (row >= n) die("mask byte outside [0, N)", int64_t(row), int64_t(n));
    ++loads1;
    return mask[row];
  }
  void lds_write(uint32_t i, uint32_t v) {
    if (i >= uint32_t(mk::kLds)) die("LDS index outside the buffer (write)", i, thread);
    wr[i] = wr[i] && wr[i] != thread + 1 ? kMany : thread + 1;
    lds[i] = v;
    stamp[i] = epoch;
  }
  uint32_t lds_read(uint32_t i) {
    if (i >= uint32_t(mk::kLds)) die("LDS index outside the buffer (read)", i, thread);
    if (stamp[i] != epoch) die("LDS slot read before this reduction wrote it", i, int64_t(tile));
    rd[i] = rd[i] && rd[i] != thread + 1 ? kMany : thread + 1;
    return lds[i];
  }
  void store_index(uint64_t i, int32_t v) {
    if (i >= n) die("index word outside the workspace", int64_t(i), int64_t(n));
    if (!compacting) {
      if (v != -1) die("the count kernel writes -1 only", int64_t(i), v);
      if (++index_fill[i] != 1) die("index word set to -1 twice", int64_t(i), 0);
    } else {
      if (v < 0 || uint64_t(v) >= n || !mask[v]) die("a row that is not set scattered", v, 0);
      if (++index_scatter[i] != 1) die("index word scattered to twice", int64_t(i), v);
      if (++scattered[v] != 1) die("set row scattered twice", v, int64_t(i));
    }
    index[i] = v;
  }
  void store_count(uint64_t i, uint32_t v) {
    if (i > n) die("count word outside the workspace", int64_t(i), int64_t(n));
    if (++count_writes[i] != 1) die("count word written twice", int64_t(i), 0);
    counts[i] = v;
  }
  void store_total(uint64_t t, uint32_t v) {
    if (compacting) die("the compact kernel writes no total", int64_t(t), 0);
    if (t >= tiles) die("total outside the workspace", int64_t(t), int64_t(tiles));
    if (++total_writes[t] != 1) die("total written twice", int64_t(t), 0);
    totals[t] = v;
  }
  uint32_t load_total(uint64_t t) {
    if (!compacting || t >= tile) die("total read that is not of a tile before", int64_t(t), int64_t(tile));
    if (total_writes[t] != 1) die("total read that was never written", int64_t(t), 0);
    return totals[t];
  }
  void store_offset(uint64_t i, uint32_t v) {
    if (!one_list || i > 1) die("offset written that the message does not have", int64_t(i), 0);
    if (++offset_writes[i] != 1) die("offset written twice", int64_t(i), 0);
    offsets[i] = v;
  }
};

template <class F>
void phase(EmuMask& m, const char* name, F f) {
  m.begin_phase();
  for (m.thread = 0; m.thread < kThreads; ++m.thread) f(m.thread);
  m.end_phase(name);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 4) {
    std::printf("usage: see the file's head\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  FILE* blob = std::fopen(argv[2], "rb");
  FILE* out = std::fopen(argv[3], "wb");
  if (!blob || !out) {
    std::printf("FAIL files\n");
    return 2;
  }
  uint64_t n = 0, tiles_sum = 0, loads16 = 0, loads1 = 0;
  while (in >> n) {
    uint64_t shift = 0, one_list = 0, grid = 0, at = 0;
    in >> shift >> one_list >> grid >> at;
    if (!in || shift > 15 || n > mk::kMaxRows) {
      std::printf("FAIL bad case %d\n", g_case);
      return 2;
    }
    EmuMask m;
    m.n = n;
    m.shift = uint32_t(shift);
    m.one_list = one_list != 0;
    m.mask.reset(new uint8_t[n]);
    if (std::fseek(blob, long(at), SEEK_SET) != 0 || std::fread(m.mask.get(), 1, n, blob) != n) {
      std::printf("FAIL mask bytes of case %d\n", g_case);
      return 2;
    }
    // (only the alignment of the mask's address matters to the arguments; nothing is
    // dereferenced through them)
    const uint8_t* fake = reinterpret_cast<const uint8_t*>(uintptr_t(0x7F0000001000u) + shift);
    uint8_t* dst = reinterpret_cast<uint8_t*>(uintptr_t(0x7E0000002000u));
    const mk::Workspace w = mk::workspace(8, n, 0);
    const mk::Args a = mk::make_args(fake, n, dst, w, m.one_list);
    m.tiles = mk::tiles(a);
    if (a.shift != shift || m.tiles != (n ? (n + shift + mk::kTile - 1) / mk::kTile : 0) ||
        w.counts - w.index != 4 * n || w.totals - w.counts != 4 * (n + 1) ||
        w.part - w.totals < 4 * m.tiles || w.end != w.part || (w.index & 3) || w.index < 8)
      die("the arguments or the workspace of the launch", int64_t(m.tiles), int64_t(w.end));
    m.index.assign(n, 0x5A5A5A5A);
    m.counts.assign(n + 1, 0xA5A5A5A5u);
    m.totals.assign(m.tiles, 0);
    m.offsets.assign(2, 0xA5A5A5A5u);
    m.index_fill.assign(n, 0);
    m.index_scatter.assign(n, 0);
    m.scattered.assign(n, 0);
    m.count_writes.assign(n + 1, 0);
    m.total_writes.assign(m.tiles, 0);
    std::memset(m.stamp, 0xff, sizeof(m.stamp));
    const uint64_t wgs = grid ? grid : m.tiles;
    // mask_count_kernel
    for (uint64_t wg = 0; wg < wgs; ++wg)
      for (uint64_t t = wg; t < m.tiles; t += wgs) {
        m.tile = t;
        ++m.epoch;
        phase(m, "count load", [&](uint32_t th) { mk::count_load(a, t, th, m); });
        for (int s = 0; s < mk::kSteps; ++s)
          phase(m, "reduce", [&](uint32_t th) { mk::reduce_phase(th, s, m); });
        phase(m, "count store", [&](uint32_t th) { mk::count_store(a, t, th, m); });
      }
    for (uint64_t i = 0; i < n; ++i)
      if (m.index_fill[i] != 1) die("index word never set to -1", int64_t(i), 0);
    for (uint64_t t = 0; t < m.tiles; ++t)
      if (m.total_writes[t] != 1) die("total never written", int64_t(t), 0);
    // mask_compact_kernel
    m.compacting = true;
    for (uint64_t wg = wgs; wg-- > 0;)
      for (uint64_t t = wg; t < m.tiles; t += wgs) {
        m.tile = t;
        ++m.epoch;
        phase(m, "carry load", [&](uint32_t th) { mk::carry_load(a, t, th, m); });
        for (int s = 0; s < mk::kSteps; ++s)
          phase(m, "reduce", [&](uint32_t th) { mk::reduce_phase(th, s, m); });
        std::vector<uint32_t> carry(kThreads), flags(kThreads);
        phase(m, "carry read", [&](uint32_t th) { carry[th] = mk::carry_read(m); });
        for (uint32_t th = 1; th < kThreads; ++th)
          if (carry[th] != carry[0]) die("threads disagree on the carry", th, carry[th]);
        ++m.epoch;
        phase(m, "scan load", [&](uint32_t th) { flags[th] = mk::scan_load(a, t, th, m); });
        for (int s = 0; s < mk::kSteps; ++s)
          phase(m, "scan step", [&](uint32_t th) { mk::scan_step(th, s, m); });
        phase(m, "scan store",
              [&](uint32_t th) { mk::scan_store(a, t, th, flags[th], carry[th], m); });
      }
    if (n) {
      for (uint64_t i = 0; i <= n; ++i)
        if (m.count_writes[i] != 1) die("count word never written", int64_t(i), 0);
      for (uint64_t i = 0; i < n; ++i)
        if (m.mask[i] && m.scattered[i] != 1) die("set row never scattered", int64_t(i), 0);
      if (m.one_list && (m.offset_writes[0] != 1 || m.offset_writes[1] != 1))
        die("offsets of the one list not written", m.offset_writes[0], m.offset_writes[1]);
    }
    if ((n && std::fwrite(m.index.data(), 4, n, out) != n) ||
        std::fwrite(m.counts.data(), 4, n + 1, out) != n + 1 ||
        std::fwrite(m.offsets.data(), 4, 2, out) != 2) {
      std::printf("FAIL output file\n");
      return 2;
    }
    tiles_sum += m.tiles;
    loads16 += m.loads16;
    loads1 += m.loads1;
    ++g_case;
  }
  std::fclose(out);
  std::fclose(blob);
  if (!g_case) {
    std::printf("FAIL no case\n");
    return 2;
  }
  std::printf("ok cases=%d tiles=%" PRIu64 " loads16=%" PRIu64 " loads1=%" PRIu64 "\n", g_case,
              tiles_sum, loads16, loads1);
  return 0;
}
