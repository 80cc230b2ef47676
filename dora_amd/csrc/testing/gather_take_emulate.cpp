// Host emulation of the taken body of gather_struct_kernel (gather_device.h take::), a
// stand-alone program that tests/test_take_index_host.py compiles with the host compiler and
// -fsanitize=address,undefined and runs once per group of cases; it is part of no library.
//
// It builds multi::Args with multi::make_taken_args and then does what the kernel does for every
// workgroup of the grid: multi::field_of finds the field and take_lane runs for all 256 threads
// with the workgroup numbered inside the field's share, through a memory policy that performs
// nothing unchecked:
//   (a) every index word read is word i of the index with 0 <= i < K;
//   (b) every source byte read for field k lies in that field's [lo, hi];
//   (c) nothing is read from a source while the row in hand is missing, that is while the word
//       this lane read last is not in [0, N);
//   (d) every byte of every field's [off, off + bytes) is written exactly once, by that field;
//   (e) no byte between the fields and none at or past `size` is written;
//   (f) the sample is appended to `out_file` (unwritten bytes 0xA5) for the caller to compare.
//
//   gather_take_emulate spec_file [out_file]
//
// `spec_file` holds whitespace-separated integers, any number of cases one after another:
//   n dst_addr size K N wide index_file
// then per field
//   elem row total lo hi src_addr off stride0 nd shape[nd] stride[nd] source_file
// `index_file` holds the K words of 4 (wide 0) or 8 bytes; `source_file` the hi - lo + 1 bytes of
// [src + lo, src + hi], or `-` (addresses only; N == 0: nothing is reachable).  The view of a
// field is dimensions 1.. of the tensor (`total` the K taken rows' bytes), `stride0` the byte
// stride of dimension 0, as a take plan holds them.  `dst_addr` / `src_addr` are the addresses
// the kernel would see (only their alignment matters; neither is dereferenced).
// Exit status 0 and "ok" when every check held in every case.
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
namespace tk = dora::gather::take;

int g_case = 0;

[[noreturn]] void die(int field, const char* what, int64_t a, int64_t b) {
  std::printf("FAIL case %d field %d: %s (%" PRId64 ", %" PRId64 ")\n", g_case, field, what, a, b);
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

// The index: K words, read one at a time.
struct Index {
  std::vector<uint8_t> bytes;
  uint64_t k, n;
  bool wide;
  uint64_t loads = 0;
};

// One field's memory for one lane at a time: loads from the field's window, index words from
// the index, stores into the sample at the offset the field's destination has from the sample's.
struct EmuMem {
  int field;
  std::vector<uint8_t> win;  // bytes of [lo, hi], or empty
  int64_t lo, hi;
  uint64_t at;  // the field's dst minus the sample's
  Sample* s;
  Index* ix;
  bool row_valid = false;  // the word this lane read last is a row
  uint64_t loads = 0;

  int64_t load_index(uint64_t i) {
    if (i >= ix->k) die(field, "index word outside [0, K)", int64_t(i), int64_t(ix->k));
    ++ix->loads;
    int64_t w;
    if (ix->wide) {
      std::memcpy(&w, ix->bytes.data() + 8 * i, 8);
    } else {
      int32_t w32;
      std::memcpy(&w32, ix->bytes.data() + 4 * i, 4);
      w = w32;
    }
    row_valid = w >= 0 && uint64_t(w) < ix->n;
    return w;
  }
  void src_check(int64_t o, int n) {
    if (!row_valid) die(field, "source read for a missing row", o, n);
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

bool read_file(const std::string& name, std::vector<uint8_t>& into, uint64_t want) {
  into.resize(want);
  if (!want) return true;
  FILE* f = std::fopen(name.c_str(), "rb");
  const bool ok = f && std::fread(into.data(), 1, want, f) == want;
  if (f) std::fclose(f);
  return ok;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 2) {
    std::printf("usage: see the file's head\n");
    return 2;
  }
  std::ifstream in(argv[1]);
  FILE* out = argc > 2 ? std::fopen(argv[2], "wb") : nullptr;
  if (argc > 2 && !out) {
    std::printf("FAIL output file\n");
    return 2;
  }
  uint64_t loads = 0, index_loads = 0, grid_sum = 0;
  int64_t n = 0;
  while (in >> n) {
    uint64_t dst_addr = 0, size = 0;
    Index ix{};
    int wide = 0;
    std::string index_file;
    in >> dst_addr >> size >> ix.k >> ix.n >> wide >> index_file;
    if (!in || n < 1 || n > mt::kMaxFields || ix.k < 1 || (wide != 0 && wide != 1)) {
      std::printf("FAIL bad case %d\n", g_case);
      return 2;
    }
    ix.wide = wide != 0;
    if (!read_file(index_file, ix.bytes, ix.k * (ix.wide ? 8 : 4))) {
      std::printf("FAIL index file of case %d: %" PRIu64 " words expected\n", g_case, ix.k);
      return 2;
    }
    uint8_t* dst = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(dst_addr));
    dora::GatherDesc g[mt::kMaxFields] = {};
    uint64_t off[mt::kMaxFields];
    int64_t stride0[mt::kMaxFields];
    Sample s{size, std::vector<int8_t>(size, -1), std::vector<uint8_t>(size, 0xA5),
             std::vector<uint8_t>(size, 0)};
    std::vector<EmuMem> mem(static_cast<size_t>(n));
    for (int k = 0; k < n; ++k) {
      uint64_t src = 0;
      std::string file;
      in >> g[k].elem >> g[k].view.row >> g[k].view.total >> g[k].lo >> g[k].hi >> src >> off[k] >>
          stride0[k] >> g[k].view.nd;
      if (!in || g[k].view.nd < 0 || g[k].view.nd > dora::kMaxTensorDims) {
        std::printf("FAIL bad field %d of case %d\n", k, g_case);
        return 2;
      }
      for (int i = 0; i < g[k].view.nd; ++i) in >> g[k].view.shape[i];
      for (int i = 0; i < g[k].view.nd; ++i) in >> g[k].view.stride[i];
      in >> file;
      if (!in || off[k] > size || g[k].view.total > size - off[k] || !g[k].view.total) {
        std::printf("FAIL field %d of case %d does not fit the sample\n", k, g_case);
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
      m.ix = &ix;
      if (file != "-" && !read_file(file, m.win, uint64_t(g[k].hi - g[k].lo) + 1)) {
        std::printf("FAIL source file of field %d of case %d\n", k, g_case);
        return 2;
      }
    }
    dora::TakeDesc td{};
    td.src = nullptr;  // (the policy holds the words)
    td.count = ix.k;
    td.n = ix.n;
    td.wide = ix.wide ? 1 : 0;
    const mt::Args a = mt::make_taken_args(g, stride0, off, int(n), dst, td);
    const uint32_t grid = mt::grid_for(a);
    if (a.take.k != ix.k || a.take.n != ix.n || a.take.wide != td.wide)
      die(-1, "the index descriptor of the launch", int64_t(a.take.k), int64_t(a.take.n));
    for (int k = 0; k < n; ++k) {
      if (a.f[k].kind != mt::kRowsTaken) die(k, "not a taken field", a.f[k].kind, 0);
      mem[size_t(k)].at = uint64_t(a.f[k].taken.g.dst - dst);
      if (a.wg_begin[k + 1] <= a.wg_begin[k]) die(k, "field without a workgroup", a.wg_begin[k], 0);
    }
    for (uint32_t w = 0; w < grid; ++w) {
      const int k = mt::field_of(a, w);
      if (k < 0 || k >= n || w < a.wg_begin[k] || w >= a.wg_begin[k + 1])
        die(k, "workgroup outside its field's share", w, 0);
      const uint64_t local = w - a.wg_begin[k], share = a.wg_begin[k + 1] - a.wg_begin[k];
      EmuMem& m = mem[size_t(k)];
      for (uint32_t th = 0; th < uint32_t(dora::gather::kThreads); ++th) {
        m.row_valid = false;  // a lane starts with no row in hand
        tk::take_lane(a.f[k].taken, a.take, local * dora::gather::kThreads + th,
                      share * dora::gather::kThreads, m);
      }
    }
    for (uint64_t b = 0; b < size; ++b)
      if (s.owner[b] >= 0 && s.writes[b] != 1)
        die(s.owner[b], "output byte never written", int64_t(b), 0);
    if (out && std::fwrite(s.out.data(), 1, s.out.size(), out) != s.out.size()) {
      std::printf("FAIL output file\n");
      return 2;
    }
    for (const EmuMem& m : mem) loads += m.loads;
    index_loads += ix.loads;
    grid_sum += grid;
    ++g_case;
  }
  if (out) std::fclose(out);
  if (!g_case) {
    std::printf("FAIL no case\n");
    return 2;
  }
  std::printf("ok cases=%d grid=%" PRIu64 " loads=%" PRIu64 " index_loads=%" PRIu64 "\n", g_case,
              grid_sum, loads, index_loads);
  return 0;
}
