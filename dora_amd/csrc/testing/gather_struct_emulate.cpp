// Host emulation of gather_struct_kernel (gather_device.h multi::), a stand-alone program that
// tests/test_gather_struct_index_host.py compiles with the host compiler and
// -fsanitize=address,undefined and runs once per record; it is part of no library.
//
// It builds multi::Args with multi::make_args and then does what the kernel does for every
// workgroup of the grid: multi::field_of finds the field, and the field's own body runs with the
// workgroup numbered inside the field's share — gather_lane for all 256 threads, or for each of
// the workgroup's tiles the load phase of all threads into an array that stands for the LDS
// tile, then the store phase — through memory policies that perform nothing unchecked:
//   (a) every source byte read for field k lies in that field's [lo, hi];
//   (b) every LDS index lies inside the tile, and every element read from it was written by
//       this tile's load phase;
//   (c) every byte of every field's [off, off + bytes) is written exactly once, by that field;
//   (d) no byte between the fields and none at or past `size` is written;
//   (e) the sample is written to `out_file` (unwritten bytes 0xA5) for the caller to compare.
//
//   gather_struct_emulate spec_file [out_file]
//
// `spec_file` holds whitespace-separated integers: n dst_addr size, then per field
//   kind elem row total lo hi src_addr off nd shape[nd] stride[nd]
// followed by the name of a file with the hi - lo + 1 bytes of [src + lo, src + hi], or `-`
// (addresses only).  `kind` is what the launcher's selection gives the field: -1 the rows body,
// else the dimension the tile body transposes against.  `dst_addr` / `src_addr` are the
// addresses the kernel would see (only their alignment matters; neither is dereferenced).
// Exit status 0 and "ok" when every check held.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "gather_device.h"

namespace {

using dora::gather::U16;
namespace mt = dora::gather::multi;
namespace tl = dora::gather::tile;

[[noreturn]] void die(int field, const char* what, int64_t a, int64_t b) {
  std::printf("FAIL field %d: %s (%" PRId64 ", %" PRId64 ")\n", field, what, a, b);
  std::exit(1);
}

// The whole sample: which field may write which byte, and how often each was written.
struct Sample {
  uint64_t size;
  std::vector<int8_t> owner;  // field of each byte, -1: padding
  std::vector<uint8_t> out, writes;
  void write(int field, uint64_t at, uint8_t v) {
    if (at >= size) die(field, "write at or past the sample's size", int64_t(at), int64_t(size));
    if (owner[at] != field)
      die(field, owner[at] < 0 ? "padding byte written" : "another field's byte written",
          int64_t(at), owner[at]);
    if (++writes[at] != 1) die(field, "output byte written twice", int64_t(at), 0);
    out[at] = v;
  }
};

// One field's memory: loads from its window, stores into the sample at the offset its own
// arguments' destination has from the sample's.
struct EmuMem {
  int field;
  std::vector<uint8_t> win;  // bytes of [lo, hi], or empty
  int64_t lo, hi;
  uint64_t at;  // the field's dst minus the sample's
  Sample* s;
  uint64_t loads = 0;

  void src_check(int64_t o, int n) {
    if (o < lo || o > hi || hi - o < n - 1) die(field, "source offset outside [lo, hi]", o, n);
    ++loads;
  }
  uint8_t src_byte(int64_t o) const { return win.empty() ? 0 : win[size_t(o - lo)]; }
  U16 load16(int64_t o) {
    src_check(o, 16);
    uint8_t b[16];
    for (int i = 0; i < 16; ++i) b[i] = src_byte(o + i);
    U16 v;
    std::memcpy(v.w, b, 16);
    return v;
  }
  template <int G>
  uint64_t load_piece(int64_t o) {
    src_check(o, G);
    uint64_t x = 0;
    for (int i = 0; i < G; ++i) x |= uint64_t(src_byte(o + i)) << (8 * i);
    return x;
  }
  U16 funnel(U16 l, U16 h, uint32_t mis) {
    if (mis >= 16) die(field, "funnel shift", mis, 0);
    uint8_t b[32];
    std::memcpy(b, l.w, 16);
    std::memcpy(b + 16, h.w, 16);
    U16 v;
    std::memcpy(v.w, b + mis, 16);
    return v;
  }
  void store16(uint64_t o, U16 v) {
    uint8_t b[16];
    std::memcpy(b, v.w, 16);
    for (int i = 0; i < 16; ++i) s->write(field, at + o + uint64_t(i), b[i]);
  }
  void store1(uint64_t o, uint8_t v) { s->write(field, at + o, v); }
};

// The tile body's policy over the same memory: elements travel as uint64_t whatever their size.
struct EmuTile {
  EmuMem& m;
  uint32_t elem;
  std::vector<uint64_t> lds;
  std::vector<uint8_t> filled;
  void reset() {
    lds.assign(tl::kLds, 0);
    filled.assign(tl::kLds, 0);
  }
  uint64_t load_elem(int64_t o) {
    m.src_check(o, int(elem));
    uint64_t x = 0;
    for (uint32_t i = 0; i < elem; ++i) x |= uint64_t(m.src_byte(o + i)) << (8 * i);
    return x;
  }
  void lds_write(uint32_t i, uint64_t v) {
    if (i >= lds.size()) die(m.field, "LDS index outside the tile (write)", i, 0);
    if (filled[i]++) die(m.field, "LDS element written twice", i, 0);
    lds[i] = v;
  }
  uint64_t lds_read(uint32_t i) {
    if (i >= lds.size()) die(m.field, "LDS index outside the tile (read)", i, 0);
    if (!filled[i]) die(m.field, "LDS element read before it was written", i, 0);
    return lds[i];
  }
  void store_elem(uint64_t e, uint64_t v) {
    for (uint32_t i = 0; i < elem; ++i) m.s->write(m.field, m.at + e * elem + i, uint8_t(v >> (8 * i)));
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: see the file's head\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  int64_t n = 0;
  uint64_t dst_addr = 0, size = 0;
  in >> n >> dst_addr >> size;
  if (!in || n < 1 || n > mt::kMaxFields) {
    std::printf("FAIL bad field count\n");
    return 2;
  }
  uint8_t* dst = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(dst_addr));
  dora::GatherDesc g[mt::kMaxFields] = {};
  uint64_t off[mt::kMaxFields];
  int kind[mt::kMaxFields];
  Sample s{size, std::vector<int8_t>(size, -1), std::vector<uint8_t>(size, 0xA5),
           std::vector<uint8_t>(size, 0)};
  std::vector<EmuMem> mem(static_cast<size_t>(n));
  for (int k = 0; k < n; ++k) {
    uint64_t src = 0;
    std::string file;
    in >> kind[k] >> g[k].elem >> g[k].view.row >> g[k].view.total >> g[k].lo >> g[k].hi >> src >>
        off[k] >> g[k].view.nd;
    if (!in || g[k].view.nd < 0 || g[k].view.nd > dora::kMaxTensorDims) {
      std::printf("FAIL bad field %d\n", k);
      return 2;
    }
    for (int i = 0; i < g[k].view.nd; ++i) in >> g[k].view.shape[i];
    for (int i = 0; i < g[k].view.nd; ++i) in >> g[k].view.stride[i];
    in >> file;
    if (!in || off[k] > size || g[k].view.total > size - off[k]) {
      std::printf("FAIL field %d does not fit the sample\n", k);
      return 2;
    }
    g[k].view.src = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(src));
    for (uint64_t b = 0; b < g[k].view.total; ++b) {
      if (s.owner[off[k] + b] >= 0) die(k, "fields overlap", int64_t(off[k] + b), 0);
      s.owner[off[k] + b] = int8_t(k);
    }
    EmuMem& m = mem[size_t(k)];
    m.field = k;
    m.lo = g[k].lo;
    m.hi = g[k].hi;
    m.s = &s;
    if (file != "-") {
      const uint64_t want = uint64_t(g[k].hi - g[k].lo) + 1;
      m.win.resize(want);
      FILE* f = std::fopen(file.c_str(), "rb");
      if (!f || std::fread(m.win.data(), 1, want, f) != want) {
        std::printf("FAIL source file of field %d: %" PRIu64 " bytes expected\n", k, want);
        return 2;
      }
      std::fclose(f);
    }
    // a field the tile body is asked for must be one it applies to, with that dimension
    if (kind[k] >= 0 && tl::contiguous_dim(g[k], dst + off[k]) != kind[k])
      die(k, "the tile body does not apply with this dimension", kind[k], 0);
  }
  const mt::Args a = mt::make_args(g, off, kind, int(n), dst);
  const uint32_t grid = mt::grid_for(a);
  uint64_t tiles = 0;
  for (int k = 0; k < n; ++k) {
    const uint8_t* fd = a.f[k].kind == mt::kTile ? a.f[k].tile.dst : a.f[k].rows.dst;
    mem[size_t(k)].at = uint64_t(fd - dst);
    if (a.wg_begin[k + 1] <= a.wg_begin[k]) die(k, "field without a workgroup", a.wg_begin[k], 0);
  }
  for (uint32_t w = 0; w < grid; ++w) {
    const int k = mt::field_of(a, w);
    if (k < 0 || k >= n || w < a.wg_begin[k] || w >= a.wg_begin[k + 1])
      die(k, "workgroup outside its field's share", w, 0);
    const mt::Field& f = a.f[k];
    const uint64_t local = w - a.wg_begin[k], share = a.wg_begin[k + 1] - a.wg_begin[k];
    EmuMem& m = mem[size_t(k)];
    if (f.kind == mt::kRows) {
      for (uint32_t th = 0; th < uint32_t(dora::gather::kThreads); ++th)
        dora::gather::gather_lane(f.rows, local * dora::gather::kThreads + th,
                                  share * dora::gather::kThreads, m);
      continue;
    }
    EmuTile t{m, f.tile.elem, {}, {}};
    for (uint64_t tile = local; tile < f.tile.ntiles; tile += share) {
      const tl::Origin o = tl::origin(f.tile, tile);
      t.reset();
      for (uint32_t th = 0; th < uint32_t(dora::gather::kThreads); ++th) tl::load_phase(f.tile, o, th, t);
      for (uint32_t th = 0; th < uint32_t(dora::gather::kThreads); ++th) tl::store_phase(f.tile, o, th, t);
      ++tiles;
    }
  }
  for (uint64_t b = 0; b < size; ++b)
    if (s.owner[b] >= 0 && s.writes[b] != 1) die(s.owner[b], "output byte never written", int64_t(b), 0);
  if (argc > 2) {
    FILE* f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(s.out.data(), 1, s.out.size(), f) != s.out.size()) {
      std::printf("FAIL output file\n");
      return 2;
    }
    std::fclose(f);
  }
  uint64_t loads = 0;
  for (const EmuMem& m : mem) loads += m.loads;
  std::printf("ok fields=%" PRId64 " grid=%u tiles=%" PRIu64 " loads=%" PRIu64 "\n", n, grid, tiles, loads);
  return 0;
}
