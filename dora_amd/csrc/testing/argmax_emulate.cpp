// Host emulation of gather_reduce_kernel (reduce_device.h, and gather_device.h's rows body for
// the fields that are not reduced), a stand-alone program that tests/test_argmax_index_host.py
// compiles with the host compiler and -fsanitize=address,undefined and runs once per group of
// cases; it is part of no library.
//
// It builds multi::Args with multi::make_reduce_args and then does what the kernel does for every
// workgroup of the grid: multi::field_of finds the field and its body runs with the workgroup
// numbered inside the field's share — reduce_lane (or gather_lane) for all 256 threads one after
// the other; for the wave body the four waves of the workgroup one after the other, each in lock
// step: wave_partial for all 64 lanes, then each of the six wave_step exchanges for all 64 lanes
// against the pairs as they stood before the step, then wave_store for all 64 lanes — through a
// memory policy that performs nothing unchecked:
//   (a) every source byte read for field k lies in that field's [lo, hi];
//   (b) every load of a reduced field is naturally aligned at the address the kernel would see (a
//       vector load of 4, 8 or 16 bytes, an element load of its size), every 16-byte load of a
//       plain field a whole number of dwords;
//   (c) every 16-byte store lands on a 16-byte boundary, every element store on its own size;
//   (d) every byte of every field's [off, off + bytes) is written exactly once, by that field;
//   (e) no byte between the fields and none at or past `size` is written;
//   (f) a lane exchange reaches a lane of the same wave;
//   (g) the sample is appended to `out_file` (unwritten bytes 0xA5) for the caller to compare.
// Conversions are cast_device.h's plain-integer ones (HostCvt).
//
//   argmax_emulate spec_file [out_file]
//
// `spec_file` holds whitespace-separated integers, any number of cases one after another:
//   n dst_addr size
// then per field
//   on src_code src_bits idx_code idx_bits c cstride wave count elem row src_total dst_bytes lo hi
//   src_addr off nd shape[nd] stride[nd] source_file
// `on` 1: the field is reduced (`src_code` / `src_bits` the DLPack source dtype, `idx_code` /
// `idx_bits` the index dtype, `c` candidates `cstride` bytes apart, `wave` 1 for the wave body,
// `count` output elements); `elem`, `row`, `src_total`, shape and stride describe the view of the
// kept dimensions in source bytes, [lo, hi] its reach over all `c` steps, `dst_bytes` / `off` the
// field's bytes in the sample.  `on` 0: a plain field, the reduce numbers ignored.  `source_file`
// holds the hi - lo + 1 bytes of [src + lo, src + hi].  `dst_addr` / `src_addr` are the addresses
// the kernel would see (only their alignment matters; neither is dereferenced).
// Exit status 0 and a line "ok cases=.. grid=.. loads=.. vector_units=.. element_units=..
// wave_outputs=.." when every check held in every case.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "reduce_device.h"

namespace {

using dora::gather::U16;
namespace mt = dora::gather::multi;
namespace ct = dora::gather::cast;
namespace rd = dora::gather::reduce;

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

// One field's memory for one lane at a time, for the reduce bodies and the rows body alike.
struct EmuMem : ct::HostCvt {
  int field;
  std::vector<uint8_t> win;  // bytes of [lo, hi]
  int64_t lo, hi;
  uint64_t src_addr;
  uint64_t at;  // the field's dst minus the sample's
  Sample* s;
  uint64_t loads = 0, vec_loads = 0;
  // the wave body: the lane that runs and the wave's pairs as they stood before the step
  uint32_t lane = 0;
  const rd::Pair* before = nullptr;

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
  // the reduce bodies
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
  template <int S>
  uint32_t load_stream(int64_t o) {
    return load_elem<S>(o);
  }
  template <int D>
  void store_index(uint64_t e, uint64_t i) {
    if ((s->addr + at + e * D) % D) die(field, "element store not aligned", int64_t(e), D);
    for (int k = 0; k < D; ++k) s->write(field, at + e * D + uint64_t(k), uint8_t(i >> (8 * k)));
  }
  rd::Pair lane_xor(const rd::Pair& p, int d) {
    const uint32_t other = lane ^ uint32_t(d);
    if (!before || d < 1 || other >= uint32_t(rd::kWave)) die(field, "lane exchange", lane, d);
    if (before[lane].i != p.i || ct::bits_of(before[lane].v) != ct::bits_of(p.v))
      die(field, "lane out of step", lane, d);
    return before[other];
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

// One wave of the wave body in lock step: the output elements first, first + waves, ..
uint64_t run_wave(const rd::Args& a, uint64_t first, uint64_t waves, EmuMem& m) {
  uint64_t outputs = 0;
  rd::Pair p[rd::kWave], was[rd::kWave];
  for (uint64_t e = first; e < a.g.total; e += waves, ++outputs) {
    const int64_t s = rd::source_of(a, e);
    for (uint32_t l = 0; l < uint32_t(rd::kWave); ++l) p[l] = rd::wave_partial(a, s, l, m);
    for (int d = rd::kWave / 2; d; d >>= 1) {
      std::memcpy(was, p, sizeof(p));
      m.before = was;
      for (uint32_t l = 0; l < uint32_t(rd::kWave); ++l) {
        m.lane = l;
        rd::wave_step(p[l], d, m);
      }
      m.before = nullptr;
    }
    for (uint32_t l = 0; l < uint32_t(rd::kWave); ++l) {
      if (p[l].i != p[0].i) die(m.field, "lanes disagree after the butterfly", int64_t(e), l);
      rd::wave_store(a, e, l, p[l], m);
    }
  }
  return outputs;
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
  uint64_t loads = 0, grid_sum = 0, vec_units = 0, elem_units = 0, wave_outputs = 0;
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
    dora::ReduceDesc r[mt::kMaxFields];
    bool wave[mt::kMaxFields];
    uint64_t off[mt::kMaxFields], dst_bytes[mt::kMaxFields];
    int tile_c[mt::kMaxFields];
    Sample s{size, dst_addr, std::vector<int8_t>(size, -1), std::vector<uint8_t>(size, 0xA5),
             std::vector<uint8_t>(size, 0)};
    std::vector<EmuMem> mem(static_cast<size_t>(n));
    for (int k = 0; k < n; ++k) {
      uint64_t src = 0;
      uint32_t on = 0, code = 0, sbits = 0, icode = 0, ibits = 0, w = 0;
      std::string file;
      in >> on >> code >> sbits >> icode >> ibits >> r[k].c >> r[k].cstride >> w >> r[k].count >>
          g[k].elem >> g[k].view.row >> g[k].view.total >> dst_bytes[k] >> g[k].lo >> g[k].hi >>
          src >> off[k] >> g[k].view.nd;
      if (!in || g[k].view.nd < 0 || g[k].view.nd > dora::kMaxTensorDims || on > 1 || w > 1) {
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
      r[k].on = on != 0;
      r[k].src_code = uint8_t(code);
      r[k].src_bits = uint8_t(sbits);
      r[k].idx_code = uint8_t(icode);
      r[k].idx_bits = uint8_t(ibits);
      wave[k] = w != 0;
      if (r[k].on && (ct::src_kind(code, sbits) < 0 || !rd::index_size(icode, ibits) || !r[k].c ||
                      r[k].count * (ibits / 8) != dst_bytes[k] || sbits / 8 != g[k].elem ||
                      (wave[k] && !rd::wave_applies(g[k], r[k])))) {
        std::printf("FAIL field %d of case %d is no reduction\n", k, g_case);
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
    }
    const mt::Args a = mt::make_reduce_args(g, r, wave, off, tile_c, int(n), dst);
    const uint32_t grid = mt::grid_for(a);
    for (int k = 0; k < n; ++k) {
      const uint32_t want = !r[k].on ? mt::kRows : wave[k] ? mt::kReduceWave : mt::kReduceLane;
      if (a.f[k].kind != want) die(k, "field of the wrong kind", a.f[k].kind, want);
      mem[size_t(k)].at = uint64_t((r[k].on ? a.f[k].reduce.g.dst : a.f[k].rows.dst) - dst);
      if (mem[size_t(k)].at != off[k]) die(k, "field at the wrong offset", int64_t(off[k]), 0);
      if (a.wg_begin[k + 1] <= a.wg_begin[k]) die(k, "field without a workgroup", a.wg_begin[k], 0);
      if (r[k].on && !wave[k]) {
        const rd::Args& ra = a.f[k].reduce;
        for (uint64_t u = 0; u < ra.g.nunits; ++u) {
          rd::Start st;
          rd::start_of(ra, ra.g.head + (16 / ra.dsize) * u, st);
          const bool v = ra.dsize == 1   ? rd::unit_is_vector<1>(ra, st)
                         : ra.dsize == 2 ? rd::unit_is_vector<2>(ra, st)
                         : ra.dsize == 4 ? rd::unit_is_vector<4>(ra, st)
                                         : rd::unit_is_vector<8>(ra, st);
          ++(v ? vec_units : elem_units);
        }
      }
    }
    constexpr uint32_t kThreads = uint32_t(dora::gather::kThreads);
    for (uint32_t w = 0; w < grid; ++w) {
      const int k = mt::field_of(a, w);
      if (k < 0 || k >= n || w < a.wg_begin[k] || w >= a.wg_begin[k + 1])
        die(k, "workgroup outside its field's share", w, 0);
      const uint64_t local = w - a.wg_begin[k], share = a.wg_begin[k + 1] - a.wg_begin[k];
      EmuMem& m = mem[size_t(k)];
      if (r[k].on && wave[k]) {
        const uint64_t waves = share * kThreads / rd::kWave;
        for (uint32_t q = 0; q < kThreads / rd::kWave; ++q)
          wave_outputs += run_wave(a.f[k].reduce, local * (kThreads / rd::kWave) + q, waves, m);
        continue;
      }
      for (uint32_t th = 0; th < kThreads; ++th) {
        const uint64_t lane = local * kThreads + th;
        if (r[k].on) rd::reduce_lane(a.f[k].reduce, lane, share * kThreads, m);
        else dora::gather::gather_lane(a.f[k].rows, lane, share * kThreads, m);
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
    grid_sum += grid;
    ++g_case;
  }
  if (out) std::fclose(out);
  if (!g_case) {
    std::printf("FAIL no case\n");
    return 2;
  }
  std::printf("ok cases=%d grid=%" PRIu64 " loads=%" PRIu64 " vector_units=%" PRIu64
              " element_units=%" PRIu64 " wave_outputs=%" PRIu64 "\n",
              g_case, grid_sum, loads, vec_units, elem_units, wave_outputs);
  return 0;
}
