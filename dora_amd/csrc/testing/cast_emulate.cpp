// Host emulation of gather_cast_kernel and gather_quant_kernel (cast_device.h, and gather_device.h's rows body for the
// fields that are not cast), a stand-alone program that tests/test_cast_index_host.py compiles
// with the host compiler and -fsanitize=address,undefined and runs once per group of cases; it is
// part of no library.
//
// It builds multi::Args with multi::make_cast_args and then does what the kernel does for every
// workgroup of the grid: multi::field_of finds the field and cast_lane (or gather_lane) runs for
// all 256 threads with the workgroup numbered inside the field's share, through a memory policy
// that performs nothing unchecked:
//   (a) every source byte read for field k lies in that field's [lo, hi];
//   (b) every load of a cast field is naturally aligned at the address the kernel would see (a
//       vector load of 4, 8 or 16 bytes, an element load of its size), every 16-byte load of a
//       plain field a whole number of dwords;
//   (c) every 16-byte store lands on a 16-byte boundary, every element store on its own size;
//   (d) every byte of every field's [off, off + bytes) is written exactly once, by that field;
//   (e) no byte between the fields and none at or past `size` is written;
//   (f) the sample is appended to `out_file` (unwritten bytes 0xA5) for the caller to compare.
// Conversions are cast_device.h's plain-integer ones (HostCvt).
//
//   cast_emulate spec_file [out_file]
//
// `spec_file` holds whitespace-separated integers, any number of cases one after another:
//   n dst_addr size
// then per field
//   cast src_code src_bits dst_bits has_scale scale_bits count elem row src_total dst_bytes lo hi
//   src_addr off nd shape[nd] stride[nd] source_file
// `cast` 2: the field is quantised; two more integers follow `cast` at once, `dst_code` (DLPack: 0
// int, 1 uint) and `zero_point`, and `dst_bits` is 8 or 16 (tests/test_quant_index_host.py).
// `cast` 1: the field is converted (`src_code` / `src_bits` the DLPack source dtype, `dst_bits` 16
// or 32, `scale_bits` the float32 factor's bit pattern, `count` elements); `elem`, `row`,
// `src_total`, [lo, hi], shape and stride describe the source view in source bytes, `dst_bytes` /
// `off` the field's bytes in the sample.  `source_file` holds the hi - lo + 1 bytes of
// [src + lo, src + hi].  `dst_addr` / `src_addr` are the addresses the kernel would see (only
// their alignment matters; neither is dereferenced).
// `cast` 3: the field has an affine step (tests/test_affine_index_host.py) and its case is
// gather_affine_kernel's launch; these follow `cast` at once:
//   base inner channels has_bias bias_bits scale_addr bias_addr scale_file bias_file
// `base` 1 or 2, after which the field goes on as such a field does (2: `dst_code zero_point`);
// `inner` / `channels` the geometry of the axis, `bias_bits` the scalar bias' bit pattern,
// `scale_addr` / `bias_addr` the addresses the kernel would see of the tables (0: none, the file
// name is then ignored) and the files their `channels` float32 words.  Besides (a)-(f) every table
// load must have an index inside [0, channels) and a naturally aligned address.
// Exit status 0 and "ok" when every check held in every case; after cases with an affine step a
// second line counts them and their table loads.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "cast_device.h"

namespace {

using dora::gather::U16;
namespace mt = dora::gather::multi;
namespace ct = dora::gather::cast;

int g_case = 0;

[[noreturn]] void die(int field, const char* what, int64_t a, int64_t b) {
  std::printf("FAIL case %d field %d: %s (%" PRId64 ", %" PRId64 ")\n", g_case, field, what, a, b);
  std::exit(1);
}

// The whole sample: which field may write which byte, and how often each was written.
struct Sample {
  uint64_t size;
  uint64_t addr;  // the address the kernel would see
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

// One field's memory for one lane at a time, for the cast body and the rows body alike.
struct EmuMem : ct::HostCvt {
  int field;
  std::vector<uint8_t> win;  // bytes of [lo, hi]
  int64_t lo, hi;
  uint64_t src_addr;
  uint64_t at;  // the field's dst minus the sample's
  Sample* s;
  uint64_t loads = 0, vec_loads = 0;

  void src_check(int64_t o, int n, int align) {
    if (o < lo || o > hi || hi - o < n - 1) die(field, "source offset outside [lo, hi]", o, n);
    if (align > 1 && ((src_addr + uint64_t(o)) & uint64_t(align - 1)))
      die(field, "load not naturally aligned", o, align);
    ++loads;
  }
  uint64_t bytes(int64_t o, int n) const {
    uint64_t x = 0;
    for (int i = 0; i < n; ++i) x |= uint64_t(win[size_t(o - lo) + size_t(i)]) << (8 * i);
    return x;
  }
  U16 read16(int64_t o, int n) const {
    uint8_t b[16] = {0};
    for (int i = 0; i < n; ++i) b[i] = win[size_t(o - lo) + size_t(i)];
    U16 v;
    std::memcpy(v.w, b, 16);
    return v;
  }
  // the cast body
  template <int N>
  U16 load_vec(int64_t o) {
    src_check(o, N, N);
    ++vec_loads;
    return read16(o, N);
  }
  template <int S>
  uint32_t load_elem(int64_t o) {
    src_check(o, S, S);
    return static_cast<uint32_t>(bytes(o, S));
  }
  template <int D>
  void store_elem(uint64_t e, uint32_t bits) {
    if ((s->addr + at + e * D) % D) die(field, "element store not aligned", int64_t(e), D);
    for (int i = 0; i < D; ++i) s->write(field, at + e * D + uint64_t(i), uint8_t(bits >> (8 * i)));
  }
  // the affine step: word `c` of the table the kernel would see at `tab`
  std::vector<float> stab, btab;
  uint64_t stab_addr = 0, btab_addr = 0, channels = 0, table_loads = 0;
  float load_table(const uint8_t* tab, uint64_t c) {
    const uint64_t addr = reinterpret_cast<uintptr_t>(tab);
    if (!addr || (addr != stab_addr && addr != btab_addr)) die(field, "load from no table", int64_t(addr), 0);
    if (c >= channels) die(field, "table index outside [0, C)", int64_t(c), int64_t(channels));
    if ((addr + 4 * c) & 3) die(field, "table load not naturally aligned", int64_t(addr), int64_t(c));
    ++table_loads;
    // (the same address for both: the same words)
    return addr == stab_addr ? stab[size_t(c)] : btab[size_t(c)];
  }
  // the rows body
  U16 load16(int64_t o) {
    src_check(o, 16, 4);
    return read16(o, 16);
  }
  template <int G>
  uint64_t load_piece(int64_t o) {
    src_check(o, G, 1);
    return bytes(o, G);
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
    if ((s->addr + at + o) & 15) die(field, "16-byte store not aligned", int64_t(o), 0);
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
  uint64_t loads = 0, vec_loads = 0, grid_sum = 0, table_loads = 0, affine_cases = 0;
  int64_t n = 0;
  while (in >> n) {
    uint64_t dst_addr = 0, size = 0;
    in >> dst_addr >> size;
    if (!in || n < 1 || n > mt::kMaxFields) {
      std::printf("FAIL bad case %d\n", g_case);
      return 2;
    }
    uint8_t* dst = reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(dst_addr));
    dora::GatherDesc g[mt::kMaxFields] = {};
    dora::CastDesc c[mt::kMaxFields];
    uint64_t off[mt::kMaxFields], dst_bytes[mt::kMaxFields];
    int tile_c[mt::kMaxFields];
    Sample s{size, dst_addr, std::vector<int8_t>(size, -1), std::vector<uint8_t>(size, 0xA5),
             std::vector<uint8_t>(size, 0)};
    std::vector<EmuMem> mem(static_cast<size_t>(n));
    bool any_affine = false;
    for (int k = 0; k < n; ++k) {
      uint64_t src = 0;
      uint32_t on = 0, code = 0, sbits = 0, dbits = 0, has_scale = 0, scale_bits = 0, dcode = 2;
      int32_t zp = 0;
      std::string file, stab_file, btab_file;
      uint64_t stab_addr = 0, btab_addr = 0;
      uint32_t has_bias = 0, bias_bits = 0;
      bool affine = false;
      in >> on;
      if (on == 3) {
        affine = any_affine = true;
        in >> on >> c[k].inner >> c[k].channels >> has_bias >> bias_bits >> stab_addr >>
            btab_addr >> stab_file >> btab_file;
        if (!in || (on != 1 && on != 2) || !c[k].inner || !c[k].channels) {
          std::printf("FAIL bad affine field %d of case %d\n", k, g_case);
          return 2;
        }
      }
      if (on == 2) in >> dcode >> zp;
      in >> code >> sbits >> dbits >> has_scale >> scale_bits >> c[k].count >> g[k].elem >>
          g[k].view.row >> g[k].view.total >> dst_bytes[k] >> g[k].lo >> g[k].hi >> src >> off[k] >>
          g[k].view.nd;
      if (!in || g[k].view.nd < 0 || g[k].view.nd > dora::kMaxTensorDims || on > 2) {
        std::printf("FAIL bad field %d of case %d\n", k, g_case);
        return 2;
      }
      for (int i = 0; i < g[k].view.nd; ++i) in >> g[k].view.shape[i];
      for (int i = 0; i < g[k].view.nd; ++i) in >> g[k].view.stride[i];
      in >> file;
      if (!in || off[k] > size || dst_bytes[k] > size - off[k] || !dst_bytes[k] || g[k].hi < g[k].lo) {
        std::printf("FAIL field %d of case %d does not fit the sample\n", k, g_case);
        return 2;
      }
      c[k].on = on != 0;
      c[k].src_code = uint8_t(code);
      c[k].src_bits = uint8_t(sbits);
      c[k].dst_bits = uint8_t(dbits);
      c[k].has_scale = has_scale;
      c[k].scale = ct::f32_of(scale_bits);
      c[k].dst_code = uint8_t(dcode);
      c[k].zero_point = zp;
      const bool dst_ok =
          on == 2 ? ct::dst_kind(dcode, dbits) >= 0 &&
                        zp >= ct::dst_lo(uint32_t(ct::dst_kind(dcode, dbits))) &&
                        zp <= ct::dst_hi(uint32_t(ct::dst_kind(dcode, dbits)))
                  : dbits == 16 || dbits == 32;
      if (c[k].on && (ct::src_kind(code, sbits) < 0 || !dst_ok ||
                      c[k].count * (dbits / 8) != dst_bytes[k] || sbits / 8 != g[k].elem)) {
        std::printf("FAIL field %d of case %d is no cast\n", k, g_case);
        return 2;
      }
      tile_c[k] = -1;
      g[k].view.src = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(src));
      for (uint64_t b = 0; b < dst_bytes[k]; ++b) {
        if (s.owner[off[k] + b] >= 0) die(k, "fields overlap", int64_t(off[k] + b), 0);
        s.owner[off[k] + b] = int8_t(k);
      }
      EmuMem& m = mem[size_t(k)];
      m.field = k;
      m.lo = g[k].lo;
      m.hi = g[k].hi;
      m.src_addr = src;
      m.s = &s;
      if (!read_file(file, m.win, uint64_t(g[k].hi - g[k].lo) + 1)) {
        std::printf("FAIL source file of field %d of case %d\n", k, g_case);
        return 2;
      }
      if (affine) {
        c[k].has_bias = has_bias;
        c[k].bias = ct::f32_of(bias_bits);
        c[k].scale_tab = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(stab_addr));
        c[k].bias_tab = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(btab_addr));
        m.stab_addr = stab_addr;
        m.btab_addr = btab_addr;
        m.channels = c[k].channels;
        std::vector<uint8_t> raw;
        for (int t = 0; t < 2; ++t) {
          if (!(t ? btab_addr : stab_addr)) continue;
          if (!read_file(t ? btab_file : stab_file, raw, 4 * c[k].channels)) {
            std::printf("FAIL table file of field %d of case %d\n", k, g_case);
            return 2;
          }
          std::vector<float>& tab = t ? m.btab : m.stab;
          tab.resize(size_t(c[k].channels));
          std::memcpy(tab.data(), raw.data(), raw.size());
        }
      }
    }
    const mt::Args a = mt::make_cast_args(g, c, off, tile_c, int(n), dst);
    const uint32_t grid = mt::grid_for(a);
    for (int k = 0; k < n; ++k) {
      const uint32_t want = c[k].on ? mt::kRowsCast : mt::kRows;
      if (a.f[k].kind != want) die(k, "field of the wrong kind", a.f[k].kind, want);
      mem[size_t(k)].at = uint64_t((c[k].on ? a.f[k].cast.g.dst : a.f[k].rows.dst) - dst);
      if (mem[size_t(k)].at != off[k]) die(k, "field at the wrong offset", int64_t(off[k]), 0);
      if (a.wg_begin[k + 1] <= a.wg_begin[k]) die(k, "field without a workgroup", a.wg_begin[k], 0);
    }
    for (uint32_t w = 0; w < grid; ++w) {
      const int k = mt::field_of(a, w);
      if (k < 0 || k >= n || w < a.wg_begin[k] || w >= a.wg_begin[k + 1])
        die(k, "workgroup outside its field's share", w, 0);
      const uint64_t local = w - a.wg_begin[k], share = a.wg_begin[k + 1] - a.wg_begin[k];
      EmuMem& m = mem[size_t(k)];
      for (uint32_t th = 0; th < uint32_t(dora::gather::kThreads); ++th) {
        const uint64_t lane = local * dora::gather::kThreads + th;
        // (a case with an affine field is gather_affine_kernel's: all its converted fields)
        if (c[k].on && any_affine)
          ct::cast_lane_affine(a.f[k].cast, lane, share * dora::gather::kThreads, m);
        else if (c[k].on) ct::cast_lane(a.f[k].cast, lane, share * dora::gather::kThreads, m);
        else dora::gather::gather_lane(a.f[k].rows, lane, share * dora::gather::kThreads, m);
      }
    }
    for (uint64_t b = 0; b < size; ++b)
      if (s.owner[b] >= 0 && s.writes[b] != 1)
        die(s.owner[b], "output byte never written", int64_t(b), 0);
    if (out && std::fwrite(s.out.data(), 1, s.out.size(), out) != s.out.size()) {
      std::printf("FAIL output file\n");
      return 2;
    }
    for (const EmuMem& m : mem) {
      loads += m.loads;
      vec_loads += m.vec_loads;
      table_loads += m.table_loads;
    }
    affine_cases += any_affine;
    grid_sum += grid;
    ++g_case;
  }
  if (out) std::fclose(out);
  if (!g_case) {
    std::printf("FAIL no case\n");
    return 2;
  }
  std::printf("ok cases=%d grid=%" PRIu64 " loads=%" PRIu64 " vector_loads=%" PRIu64 "\n", g_case,
              grid_sum, loads, vec_loads);
  if (affine_cases)
    std::printf("affine cases=%" PRIu64 " table_loads=%" PRIu64 "\n", affine_cases, table_loads);
  return 0;
}
