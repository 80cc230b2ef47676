// Host emulation of the strided gather (gather_device.h), a stand-alone program that
// tests/test_gather_index_host.py compiles with the host compiler and
// -fsanitize=address,undefined and runs once per view; it is part of no library.
//
// It runs gather_lane — the function every lane of gather_rows_kernel runs — for every lane of
// the grid the launch would use, through a memory policy that performs nothing unchecked:
//   (a) every source byte read lies in the plan's [lo, hi];
//   (c) every output byte in [0, total) is written exactly once, and no other;
//   (d) the bytes produced are written to `out_file` for the caller to compare.
// With --tile it runs gather_tile_kernel's phases instead — every workgroup of the grid, for each
// of its tiles the load phase of all 256 threads into an ordinary array that stands for the LDS
// tile, then the store phase — and also checks
//   (b) every LDS index lies inside the tile, and every element read from it was written by
//       this tile's load phase;
// a view the tile kernel does not apply to prints "n/a".  (gather_rows_kernel has no LDS.)
//
//   gather_emulate [--tile] elem row total lo hi src_addr dst_addr nd shape.. stride.. [src_file out_file]
//
// `src_addr` / `dst_addr` are the addresses the kernel would see (only their alignment matters;
// neither is dereferenced).  With `src_file` — the hi - lo + 1 bytes of [src + lo, src + hi] —
// loads return those bytes; without, only addresses are computed (views spanning more than
// memory holds).  Exit status 0 and "ok" when every check held.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "gather_device.h"

namespace {

using dora::gather::U16;

[[noreturn]] void die(const char* what, int64_t a, int64_t b) {
  std::printf("FAIL %s (%" PRId64 ", %" PRId64 ")\n", what, a, b);
  std::exit(1);
}

struct EmuMem {
  const uint8_t* win;  // bytes of [lo, hi], or null
  int64_t lo, hi;
  uint64_t total;
  std::vector<uint8_t> out, writes;
  uint64_t loads = 0;

  void src_check(int64_t s, int n) {
    if (s < lo || s > hi || hi - s < n - 1) die("source offset outside [lo, hi]", s, n);
    ++loads;
  }
  uint8_t src_byte(int64_t s) const { return win ? win[s - lo] : 0; }
  U16 load16(int64_t s) {
    src_check(s, 16);
    U16 v;
    uint8_t b[16];
    for (int i = 0; i < 16; ++i) b[i] = src_byte(s + i);
    std::memcpy(v.w, b, 16);
    return v;
  }
  template <int G>
  uint64_t load_piece(int64_t s) {
    src_check(s, G);
    uint64_t x = 0;
    for (int i = 0; i < G; ++i) x |= uint64_t(src_byte(s + i)) << (8 * i);
    return x;
  }
  U16 funnel(U16 l, U16 h, uint32_t mis) {
    if (mis >= 16) die("funnel shift", mis, 0);
    uint8_t b[32];
    std::memcpy(b, l.w, 16);
    std::memcpy(b + 16, h.w, 16);
    U16 v;
    std::memcpy(v.w, b + mis, 16);
    return v;
  }
  void dst_check(uint64_t o, uint64_t n) {
    if (o >= total || total - o < n) die("destination offset outside [0, total)", int64_t(o), int64_t(n));
    for (uint64_t i = 0; i < n; ++i)
      if (++writes[o + i] != 1) die("output byte written twice", int64_t(o + i), 0);
  }
  void store16(uint64_t o, U16 v) {
    dst_check(o, 16);
    std::memcpy(out.data() + o, v.w, 16);
  }
  void store1(uint64_t o, uint8_t v) {
    dst_check(o, 1);
    out[o] = v;
  }
};

// gather_tile_kernel's memory policy: elements travel as uint64_t whatever their size
struct EmuTile {
  EmuMem& m;
  uint32_t elem;
  std::vector<uint64_t> lds;
  std::vector<uint8_t> filled;
  void reset() {
    lds.assign(dora::gather::tile::kLds, 0);
    filled.assign(dora::gather::tile::kLds, 0);
  }
  uint64_t load_elem(int64_t s) {
    m.src_check(s, static_cast<int>(elem));
    uint64_t x = 0;
    for (uint32_t i = 0; i < elem; ++i) x |= uint64_t(m.src_byte(s + i)) << (8 * i);
    return x;
  }
  void lds_write(uint32_t i, uint64_t v) {
    if (i >= lds.size()) die("LDS index outside the tile (write)", i, 0);
    if (filled[i]++) die("LDS element written twice", i, 0);
    lds[i] = v;
  }
  uint64_t lds_read(uint32_t i) {
    if (i >= lds.size()) die("LDS index outside the tile (read)", i, 0);
    if (!filled[i]) die("LDS element read before it was written", i, 0);
    return lds[i];
  }
  void store_elem(uint64_t e, uint64_t v) {
    if (e > (m.total / elem)) die("destination element outside the output", int64_t(e), 0);
    m.dst_check(e * elem, elem);
    for (uint32_t i = 0; i < elem; ++i) m.out[e * elem + i] = uint8_t(v >> (8 * i));
  }
};

int64_t num(const char* s) { return static_cast<int64_t>(std::strtoll(s, nullptr, 0)); }

}  // namespace

int main(int argc, char** argv) {
  bool tiled = false;
  if (argc > 1 && std::strcmp(argv[1], "--tile") == 0) {
    tiled = true;
    ++argv;
    --argc;
  }
  if (argc < 9) {
    std::printf("usage: see the file's head\n");
    return 2;
  }
  dora::GatherDesc g{};
  g.elem = static_cast<uint32_t>(num(argv[1]));
  g.view.row = static_cast<uint64_t>(num(argv[2]));
  g.view.total = static_cast<uint64_t>(num(argv[3]));
  g.lo = num(argv[4]);
  g.hi = num(argv[5]);
  g.view.src = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(std::strtoull(argv[6], nullptr, 0)));
  uint8_t* dst = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(std::strtoull(argv[7], nullptr, 0)));
  g.view.nd = static_cast<int>(num(argv[8]));
  if (g.view.nd < 1 || g.view.nd > dora::kMaxTensorDims || argc < 9 + 2 * g.view.nd) {
    std::printf("FAIL bad dimension count %d\n", g.view.nd);
    return 2;
  }
  for (int i = 0; i < g.view.nd; ++i) {
    g.view.shape[i] = num(argv[9 + i]);
    g.view.stride[i] = num(argv[9 + g.view.nd + i]);
  }
  const int rest = 9 + 2 * g.view.nd;
  std::vector<uint8_t> win;
  if (argc > rest + 1) {
    const uint64_t want = static_cast<uint64_t>(g.hi - g.lo) + 1;
    win.resize(want);
    FILE* f = std::fopen(argv[rest], "rb");
    if (!f || std::fread(win.data(), 1, want, f) != want) {
      std::printf("FAIL source file: %" PRIu64 " bytes expected\n", want);
      return 2;
    }
    std::fclose(f);
  }
  EmuMem m{win.empty() ? nullptr : win.data(), g.lo, g.hi, g.view.total, {}, {}};
  m.out.assign(g.view.total, 0);
  m.writes.assign(g.view.total, 0);
  if (tiled) {
    namespace tl = dora::gather::tile;
    const int c = tl::contiguous_dim(g, dst);
    if (c < 0) {
      std::printf("n/a\n");
      return 0;
    }
    const tl::Args ta = tl::make_args(g, dst, c);
    EmuTile t{m, g.elem, {}, {}};
    const uint64_t grid = tl::grid_for(ta);
    for (uint64_t blk = 0; blk < grid; ++blk) {
      for (uint64_t tile = blk; tile < ta.ntiles; tile += grid) {
        const tl::Origin o = tl::origin(ta, tile);
        t.reset();
        for (uint32_t th = 0; th < uint32_t(dora::gather::kThreads); ++th) tl::load_phase(ta, o, th, t);
        for (uint32_t th = 0; th < uint32_t(dora::gather::kThreads); ++th) tl::store_phase(ta, o, th, t);
      }
    }
    for (uint64_t o = 0; o < g.view.total; ++o)
      if (m.writes[o] != 1) die("output byte never written", int64_t(o), 0);
    if (argc > rest + 1) {
      FILE* f = std::fopen(argv[rest + 1], "wb");
      if (!f || std::fwrite(m.out.data(), 1, m.out.size(), f) != m.out.size()) {
        std::printf("FAIL output file\n");
        return 2;
      }
      std::fclose(f);
    }
    std::printf("ok tiles=%" PRIu64 " grid=%" PRIu64 " c=%d loads=%" PRIu64 "\n", ta.ntiles, grid, c, m.loads);
    return 0;
  }
  const dora::gather::Args a = dora::gather::make_args(g, dst);
  const uint64_t lanes = dora::gather::grid_for(a) * dora::gather::kThreads;
  for (uint64_t lane = 0; lane < lanes; ++lane) dora::gather::gather_lane(a, lane, lanes, m);
  for (uint64_t o = 0; o < g.view.total; ++o)
    if (m.writes[o] != 1) die("output byte never written", int64_t(o), 0);
  if (argc > rest + 1) {
    FILE* f = std::fopen(argv[rest + 1], "wb");
    if (!f || std::fwrite(m.out.data(), 1, m.out.size(), f) != m.out.size()) {
      std::printf("FAIL output file\n");
      return 2;
    }
    std::fclose(f);
  }
  std::printf("ok lanes=%" PRIu64 " units=%" PRIu64 " head=%" PRIu64 " piece=%u loads=%" PRIu64 "\n",
              lanes, a.nunits, a.head, a.piece, m.loads);
  return 0;
}
