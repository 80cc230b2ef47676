// Host emulation of gather_resize_prep_kernel and gather_crop_prep_kernel (resize_device.h and
// crop_device.h under their model-input flag, and gather_device.h's rows body for the plain
// fields), a stand-alone program that tests/test_prep_index_host.py compiles with the host compiler
// and -fsanitize=address,undefined and runs once per group of cases; it is part of no library.
//
// It builds prep::Launch with prep::make_resize_launch or prep::make_crop_launch and then does
// what the kernel does for every workgroup of the grid: multi::field_of finds the field and its
// body runs with the workgroup numbered inside the field's share — resize_lane or crop_lane with
// the field's prep::Args (or gather_lane) for all 256 threads one after the other — through a
// memory policy that performs nothing unchecked:
//   (a) every source byte read for field k lies in that field's [lo, hi];
//   (b) every tap is an element load naturally aligned at the address the kernel would see;
//   (c) every word of the boxes read lies in [0, boxes_hi] and is an aligned dword;
//   (d) every table word read has an index below the table's C words, from a table the field has,
//       at a dword-aligned address;
//   (e) the taps read for a field are exactly those of its elements inside the placed image and
//       inside a non-empty box — 1 (nearest) or 4 (bilinear) each, counted here from the spec
//       alone — so none is read for an element outside the image or of an empty box;
//   (f) every 16-byte store lands on a 16-byte boundary, every element store on its own size;
//   (g) every byte of every field's [off, off + bytes) is written exactly once, by that field;
//   (h) no byte between the fields and none at or past `size` is written;
//   (i) the sample is appended to `out_file` (unwritten bytes 0xA5) for the caller to compare.
// Conversions and arithmetic are resize_device.h's HostArith, which the host plan uses as well.
//
//   prep_emulate spec_file [out_file]
//
// `spec_file` holds whitespace-separated integers, any number of cases one after another:
//   n dst_addr size
// then per field
//   on mode src_code src_bits dst_code dst_bits rnd ax0 ax1 in0 in1 rshape[rnd] rstride[rnd] count
//   elem row src_total dst_bytes lo hi src_addr off nd shape[nd] stride[nd] source_file
//   k boxes_addr boxes_hi boxes_file
//   prep stab_addr btab_addr channels axis has_scale has_bias scale_bits bias_bits placed inner0
//   inner1 lead0 lead1 fill_bits stab_file btab_file
// as crop_emulate.cpp takes the first three lines, but `on` 1 is a resized field (k 0, no K in
// `rshape`) and `on` 2 a field of crops.  `prep` 1: the field has a model-input step —
// `stab_addr` / `btab_addr` the tables' addresses as the kernel would see them (0: none) with
// `channels` words each in `stab_file` / `btab_file`, `axis` the dimension of `rshape` they run
// along, the scalars and `fill` as float32 bit patterns, `placed` 1 with the image of extents
// `inner` at `lead`.  `prep` 0: the other numbers are ignored and the files any word.
// Exit status 0 and a line "ok cases=.. grid=.. loads=.. box_loads=.. table_loads=..
// head_elements=.. units=.. tail_elements=.. outside=.." when every check held in every case.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "crop_device.h"

namespace {

using dora::gather::U16;
namespace mt = dora::gather::multi;
namespace ct = dora::gather::cast;
namespace rz = dora::gather::resize;
namespace cp = dora::gather::crop;
namespace pp = dora::gather::prep;

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

// One field's memory for one lane at a time, for the crop body and the rows body alike.
struct EmuMem : rz::HostArith {
  int field;
  std::vector<uint8_t> win;  // bytes of [lo, hi]
  int64_t lo, hi;
  uint64_t src_addr;
  uint64_t at;  // the field's dst minus the sample's
  Sample* s;
  uint64_t loads = 0;
  std::vector<uint8_t> boxes;  // the 16 * K bytes
  int64_t boxes_hi = -1;       // the last byte the plan lets the launch read
  uint64_t boxes_addr = 0;
  uint64_t box_loads = 0;

  std::vector<uint8_t> stab, btab;  // the tables' 4 * C bytes
  uint64_t stab_addr = 0, btab_addr = 0, channels = 0;
  uint64_t table_loads = 0;

  float load_table(const uint8_t* tab, uint64_t c) {
    const uint64_t addr = uint64_t(reinterpret_cast<uintptr_t>(tab));
    const bool s_ = addr == stab_addr && stab_addr, b_ = addr == btab_addr && btab_addr;
    if (!s_ && !b_) die(field, "table load from neither table", int64_t(addr), int64_t(c));
    if (c >= channels) die(field, "table index at or past its words", int64_t(c), int64_t(channels));
    if (addr & 3) die(field, "table load not aligned", int64_t(addr), 4);
    ++table_loads;
    float v;
    std::memcpy(&v, (s_ ? stab : btab).data() + 4 * c, 4);
    return v;
  }

  int32_t load_box(int64_t o) {
    if (o < 0 || o > boxes_hi || boxes_hi - o < 3) die(field, "boxes offset outside [0, hi]", o, 4);
    if ((boxes_addr + uint64_t(o)) & 3) die(field, "boxes load not aligned", o, 4);
    if (size_t(o) + 4 > boxes.size()) die(field, "boxes offset outside the boxes", o, 4);
    ++box_loads;
    int32_t v;
    std::memcpy(&v, boxes.data() + o, 4);
    return v;
  }

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
  // the crop body
  template <int S>
  uint32_t load_elem(int64_t o) {
    src_check(o, S, S);
    return static_cast<uint32_t>(bytes(o, S));
  }
  template <int D>
  void store_elem(uint64_t e, uint32_t v) {
    if ((s->addr + at + e * D) % D) die(field, "element store not aligned", int64_t(e), D);
    for (int k = 0; k < D; ++k) s->write(field, at + e * D + uint64_t(k), uint8_t(v >> (8 * k)));
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
  uint64_t loads = 0, box_loads = 0, table_loads = 0, grid_sum = 0, heads = 0, units = 0,
           tails = 0, outside = 0;
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
    dora::ResizeDesc r[mt::kMaxFields];
    dora::CropDesc c[mt::kMaxFields];
    dora::PrepDesc d[mt::kMaxFields];
    bool is_crop[mt::kMaxFields] = {};
    uint64_t want_loads[mt::kMaxFields] = {};
    uint64_t off[mt::kMaxFields], dst_bytes[mt::kMaxFields];
    int tile_c[mt::kMaxFields];
    Sample s{size, dst_addr, std::vector<int8_t>(size, -1), std::vector<uint8_t>(size, 0xA5),
             std::vector<uint8_t>(size, 0)};
    std::vector<EmuMem> mem(static_cast<size_t>(n));
    for (int k = 0; k < n; ++k) {
      uint64_t src = 0;
      uint32_t on = 0, mode = 0, scode = 0, sbits = 0, dcode = 0, dbits = 0;
      std::string file, boxes_file;
      uint64_t kboxes = 0, boxes_addr = 0;
      int64_t boxes_hi = -1;
      in >> on >> mode >> scode >> sbits >> dcode >> dbits >> r[k].nd >> r[k].ax[0] >> r[k].ax[1] >>
          r[k].in[0] >> r[k].in[1];
      if (!in || on > 2 || r[k].nd < 0 || r[k].nd > dora::kMaxTensorDims) {
        std::printf("FAIL bad field %d of case %d\n", k, g_case);
        return 2;
      }
      for (int i = 0; i < r[k].nd; ++i) in >> r[k].shape[i];
      for (int i = 0; i < r[k].nd; ++i) in >> r[k].stride[i];
      in >> r[k].count >> g[k].elem >> g[k].view.row >> g[k].view.total >> dst_bytes[k] >>
          g[k].lo >> g[k].hi >> src >> off[k] >> g[k].view.nd;
      if (!in || g[k].view.nd < 0 || g[k].view.nd > dora::kMaxTensorDims) {
        std::printf("FAIL bad field %d of case %d\n", k, g_case);
        return 2;
      }
      for (int i = 0; i < g[k].view.nd; ++i) in >> g[k].view.shape[i];
      for (int i = 0; i < g[k].view.nd; ++i) in >> g[k].view.stride[i];
      in >> file >> kboxes >> boxes_addr >> boxes_hi >> boxes_file;
      uint32_t pon = 0, has_scale = 0, has_bias = 0, sbits_ = 0, bbits_ = 0, placed = 0, fbits = 0;
      uint64_t stab_addr = 0, btab_addr = 0;
      std::string stab_file, btab_file;
      d[k] = dora::PrepDesc{};
      in >> pon >> stab_addr >> btab_addr >> d[k].channels >> d[k].axis >> has_scale >> has_bias >>
          sbits_ >> bbits_ >> placed >> d[k].inner[0] >> d[k].inner[1] >> d[k].lead[0] >>
          d[k].lead[1] >> fbits >> stab_file >> btab_file;
      d[k].on = pon != 0;
      d[k].scale_tab = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(stab_addr));
      d[k].bias_tab = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(btab_addr));
      d[k].has_scale = has_scale;
      d[k].has_bias = has_bias;
      d[k].scale = ct::f32_of(sbits_);
      d[k].bias = ct::f32_of(bbits_);
      d[k].placed = placed != 0;
      d[k].fill = ct::f32_of(fbits);
      if (!d[k].on) d[k] = dora::PrepDesc{};
      if (!in || off[k] > size || dst_bytes[k] > size - off[k] || !dst_bytes[k] || g[k].hi < g[k].lo) {
        std::printf("FAIL field %d of case %d does not fit the sample\n", k, g_case);
        return 2;
      }
      r[k].on = on != 0;
      r[k].mode = uint8_t(mode);
      r[k].src_code = uint8_t(scode);
      r[k].src_bits = uint8_t(sbits);
      r[k].dst_code = uint8_t(dcode);
      r[k].dst_bits = uint8_t(dbits);
      is_crop[k] = on == 2;
      if (on == 1) {
        // what the launcher holds a resized field to before it launches
        const bool dst_ok = dcode == 2 ? dbits == 16 || dbits == 32 : ct::dst_kind(dcode, dbits) >= 0;
        bool ok = ct::src_kind(scode, sbits) >= 0 && dst_ok && (mode == 1 || mode == 2) &&
                  r[k].nd >= 2 && r[k].ax[0] != r[k].ax[1] && sbits / 8 == g[k].elem &&
                  r[k].count * (dbits / 8) == dst_bytes[k] && kboxes == 0;
        uint64_t count = 1;
        for (int i = 0; ok && i < r[k].nd; ++i) count *= uint64_t(r[k].shape[i]);
        for (int j = 0; ok && j < 2; ++j)
          ok = r[k].ax[j] >= 0 && r[k].ax[j] < r[k].nd && r[k].in[j] >= 1 &&
               r[k].in[j] <= int64_t(rz::kMaxExtent) && r[k].shape[r[k].ax[j]] >= 1 &&
               r[k].shape[r[k].ax[j]] <= int64_t(rz::kMaxExtent);
        if (!ok || count != r[k].count) {
          std::printf("FAIL field %d of case %d is no resized field\n", k, g_case);
          return 2;
        }
      }
      if (on == 2) {
        // what the launcher holds a field of crops to before it launches
        const bool dst_ok = dcode == 2 ? dbits == 16 || dbits == 32 : ct::dst_kind(dcode, dbits) >= 0;
        bool ok = ct::src_kind(scode, sbits) >= 0 && dst_ok && (mode == 1 || mode == 2) &&
                  r[k].nd >= 3 && r[k].ax[0] != r[k].ax[1] && sbits / 8 == g[k].elem &&
                  r[k].count * (dbits / 8) == dst_bytes[k] && kboxes >= 1 &&
                  kboxes <= dora::kMaxCropBoxes && r[k].shape[0] == int64_t(kboxes) &&
                  r[k].stride[0] == 0 && !(boxes_addr & 3);
        uint64_t count = 1;
        for (int i = 0; ok && i < r[k].nd; ++i) count *= uint64_t(r[k].shape[i]);
        for (int j = 0; ok && j < 2; ++j)
          ok = r[k].ax[j] >= 1 && r[k].ax[j] < r[k].nd && r[k].in[j] >= 1 &&
               r[k].in[j] <= int64_t(rz::kMaxExtent) && r[k].shape[r[k].ax[j]] >= 1 &&
               r[k].shape[r[k].ax[j]] <= int64_t(rz::kMaxExtent);
        if (!ok || count != r[k].count) {
          std::printf("FAIL field %d of case %d is no field of crops\n", k, g_case);
          return 2;
        }
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
      m.boxes_hi = boxes_hi;
      m.boxes_addr = boxes_addr;
      c[k] = dora::CropDesc{};
      c[k].on = is_crop[k];
      c[k].rs = r[k];
      c[k].k = kboxes;
      c[k].boxes = reinterpret_cast<const uint8_t*>(static_cast<uintptr_t>(boxes_addr));
      if (is_crop[k] && !read_file(boxes_file, m.boxes, 16 * kboxes)) {
        std::printf("FAIL boxes file of field %d of case %d\n", k, g_case);
        return 2;
      }
      if (d[k].on) {
        // what the launcher holds a model-input step to before it launches
        bool ok = on != 0;
        if (d[k].placed) {
          ok = ok && on == 1;
          for (int j = 0; ok && j < 2; ++j)
            ok = d[k].inner[j] >= 1 && d[k].lead[j] >= 0 &&
                 d[k].inner[j] + d[k].lead[j] <= r[k].shape[r[k].ax[j]];
        }
        if (ok && (stab_addr || btab_addr))
          ok = d[k].axis >= 0 && d[k].axis < r[k].nd && d[k].axis != r[k].ax[0] &&
               d[k].axis != r[k].ax[1] && r[k].shape[d[k].axis] == int64_t(d[k].channels) &&
               !((stab_addr | btab_addr) & 3);
        if (!ok) {
          std::printf("FAIL field %d of case %d has no model-input step a kernel runs\n", k, g_case);
          return 2;
        }
        m.stab_addr = stab_addr;
        m.btab_addr = btab_addr;
        m.channels = d[k].channels;
        if ((stab_addr && !read_file(stab_file, m.stab, 4 * d[k].channels)) ||
            (btab_addr && !read_file(btab_file, m.btab, 4 * d[k].channels))) {
          std::printf("FAIL table file of field %d of case %d\n", k, g_case);
          return 2;
        }
      }
      if (on) {
        // the taps the field may read: those of its elements inside the image (a resized field)
        // or of a non-empty box (crops), counted from the spec alone
        const uint64_t taps = mode == 1 ? 1 : 4;
        const int64_t oa = r[k].shape[r[k].ax[0]], ob = r[k].shape[r[k].ax[1]];
        uint64_t rest = r[k].count / uint64_t(oa) / uint64_t(ob);  // the other dimensions
        if (on == 1) {
          const uint64_t ia = d[k].placed ? uint64_t(d[k].inner[0]) : uint64_t(oa);
          const uint64_t ib = d[k].placed ? uint64_t(d[k].inner[1]) : uint64_t(ob);
          want_loads[k] = taps * rest * ia * ib;
          outside += r[k].count - rest * ia * ib;
        } else {
          rest /= kboxes;
          uint64_t full = 0;
          for (uint64_t b = 0; b < kboxes; ++b) {
            int32_t w[4];
            std::memcpy(w, m.boxes.data() + 16 * b, 16);
            const uint32_t a0 = cp::clamp_to(w[0], uint32_t(r[k].in[0])),
                           a1 = cp::clamp_to(w[2], uint32_t(r[k].in[0])),
                           b0 = cp::clamp_to(w[1], uint32_t(r[k].in[1])),
                           b1 = cp::clamp_to(w[3], uint32_t(r[k].in[1]));
            full += a1 > a0 && b1 > b0;
          }
          want_loads[k] = taps * rest * uint64_t(oa) * uint64_t(ob) * full;
          outside += (kboxes - full) * rest * uint64_t(oa) * uint64_t(ob);
        }
      }
      if (!read_file(file, m.win, uint64_t(g[k].hi - g[k].lo) + 1)) {
        std::printf("FAIL source file of field %d of case %d\n", k, g_case);
        return 2;
      }
    }
    bool any_crop = false, any_resize = false;
    for (int k = 0; k < n; ++k) {
      any_crop |= is_crop[k];
      any_resize |= r[k].on && !is_crop[k];
      if (is_crop[k]) r[k].on = false;  // (make_resize_launch sees the resized fields alone)
    }
    if (any_crop && any_resize) {
      std::printf("FAIL case %d holds resized fields and crops\n", g_case);
      return 2;
    }
    const pp::Launch l = any_crop ? pp::make_crop_launch(g, c, d, off, tile_c, int(n), dst)
                                  : pp::make_resize_launch(g, r, d, off, tile_c, int(n), dst);
    for (int k = 0; k < n; ++k) r[k].on = r[k].on || is_crop[k];
    const mt::Args& a = l.a;
    const uint32_t grid = mt::grid_for(a);
    for (int k = 0; k < n; ++k) {
      const uint32_t want = is_crop[k] ? mt::kCrop : r[k].on ? mt::kResize : mt::kRows;
      if (a.f[k].kind != want) die(k, "field of the wrong kind", a.f[k].kind, want);
      mem[size_t(k)].at = uint64_t((is_crop[k] ? a.f[k].crop.r.g.dst
                                    : r[k].on  ? a.f[k].resize.g.dst
                                               : a.f[k].rows.dst) - dst);
      if (mem[size_t(k)].at != off[k]) die(k, "field at the wrong offset", int64_t(off[k]), 0);
      if (a.wg_begin[k + 1] <= a.wg_begin[k]) die(k, "field without a workgroup", a.wg_begin[k], 0);
      if (r[k].on) {
        const rz::Args& ra = is_crop[k] ? a.f[k].crop.r : a.f[k].resize;
        if (is_crop[k] &&
            (a.f[k].crop.boxes != c[k].boxes || ra.g.shape[a.f[k].crop.kax] != int64_t(c[k].k)))
          die(k, "the boxes or their axis are not the field's", a.f[k].crop.kax, 0);
        const pp::Args& pa = l.p[k];
        if ((pa.stab || pa.btab) && ra.g.shape[pa.cax] != int64_t(d[k].channels))
          die(k, "the tables' axis is not the field's", pa.cax, ra.g.shape[pa.cax]);
        for (int j = 0; j < 2; ++j)
          if (uint32_t(pa.inner[j]) + pa.lead[j] > ra.out[j] || !pa.inner[j])
            die(k, "the image does not lie inside the output", pa.inner[j], pa.lead[j]);
        heads += ra.g.head;
        units += ra.g.nunits;
        tails += ra.g.total - ra.g.head - (16u / ra.dsize) * ra.g.nunits;
      }
    }
    constexpr uint32_t kThreads = uint32_t(dora::gather::kThreads);
    for (uint32_t w = 0; w < grid; ++w) {
      const int k = mt::field_of(a, w);
      if (k < 0 || k >= n || w < a.wg_begin[k] || w >= a.wg_begin[k + 1])
        die(k, "workgroup outside its field's share", w, 0);
      const uint64_t local = w - a.wg_begin[k], share = a.wg_begin[k + 1] - a.wg_begin[k];
      EmuMem& m = mem[size_t(k)];
      for (uint32_t th = 0; th < kThreads; ++th) {
        const uint64_t lane = local * kThreads + th;
        if (is_crop[k]) cp::crop_lane(a.f[k].crop, lane, share * kThreads, m, l.p[k]);
        else if (r[k].on) rz::resize_lane(a.f[k].resize, lane, share * kThreads, m, l.p[k]);
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
    for (int k = 0; k < n; ++k) {
      const EmuMem& m = mem[size_t(k)];
      if (r[k].on && m.loads != want_loads[k])
        die(k, "taps read are not those of the elements inside the image or a non-empty box",
            int64_t(m.loads), int64_t(want_loads[k]));
      loads += m.loads;
      box_loads += m.box_loads;
      table_loads += m.table_loads;
    }
    grid_sum += grid;
    ++g_case;
  }
  if (out) std::fclose(out);
  if (!g_case) {
    std::printf("FAIL no case\n");
    return 2;
  }
  std::printf("ok cases=%d grid=%" PRIu64 " loads=%" PRIu64 " box_loads=%" PRIu64
              " table_loads=%" PRIu64 " head_elements=%" PRIu64 " units=%" PRIu64
              " tail_elements=%" PRIu64 " outside=%" PRIu64 "\n",
              g_case, grid_sum, loads, box_loads, table_loads, heads, units, tails, outside);
  return 0;
}
