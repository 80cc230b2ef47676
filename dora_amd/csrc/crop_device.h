// Device code of the cropping gather (a field of a crop plan, tensor_plan.cpp): K boxes, read from
// memory by the body itself, each cut from one frame and brought to the same two extents by
// resize's taps, written once as float16, float32, uint8, int8, uint16 or int16.
//
// The statement (include/dora_gpu.h has it in full).  Row k of the boxes is four int32 words
// (a_lo, b_lo, a_hi, b_hi), half-open ranges along the two cropped axes of the frame, whose
// extents there are Ia and Ib.  Each word is clamped on its own, a0 = min(max(a_lo, 0), Ia),
// a1 = min(max(a_hi, 0), Ia), the same for b, before any difference is taken.  If a1 <= a0 or
// b1 <= b0 every byte of crop k is zero.  Otherwise crop k is resize's statement
// (resize_device.h) with source extents a1 - a0 and b1 - b0 and the taps a0 + i, b0 + i.
//
// It is resize_device.h's body with one more coordinate: the output odometer has K as one more
// leading dimension of stride 0, and a lane reads its box when that coordinate changes and at the
// start of a walk — a 16-byte unit may span two crops.  The four words come through the policy's
// cached loads (the lanes of a wave read the same few rows), are clamped, and both axes' taps are
// invalidated; the taps themselves are resize::tap_of over the box's extents, moved by a0 and b0
// steps, and the blend is resize::value_at, neither restated here.  An element of an empty box is
// zero and reads no tap.  Everything else — units on absolute 16-byte boundaries of the
// destination, heads and tails element by element, a policy object `M` for all memory and
// arithmetic, compiled for host and device alike — is as resize_device.h says.
//
// Model inputs (gather_crop_prep_kernel): resize_device.h's step type is passed through; the
// tables' axis is counted with K in front like the two cropped axes, the affine step is applied to
// every element of a non-empty box, and an empty box's element is zero before any of it.
// Placement is not provided for crops.
#pragma once

#include <cstdint>

#include "resize_device.h"

namespace dora {
namespace gather {
namespace crop {

// Arguments of the crops of `g` (the whole frame: its base, element size and reach) by `c` into
// `dst`.
DORA_HD Args make_args(const GatherDesc& g, const CropDesc& c, uint8_t* dst) {
  Args a{};
  a.r = resize::make_args(g, c.rs, dst);
  a.boxes = c.boxes;
  a.kax = static_cast<uint8_t>(kDims - c.rs.nd);
  return a;
}

DORA_HD uint64_t grid_for(const Args& a) { return resize::grid_for(a.r); }

// Where a lane is: resize's walk (RW: resize::Walk, or resize::PrepWalk under the model-input
// step), the crop its box was read for (-1: none yet), and the box clamped: its first steps along
// the two axes and its extents, both 0 for an empty box.
template <class RW>
struct WalkT {
  RW w;
  int64_t ok;
  uint32_t a0, b0, ia, ib;
};
using Walk = WalkT<resize::Walk>;
template <class PA>
using WalkFor = WalkT<typename resize::WalkFor<PA>::type>;

// `v` clamped to [0, n], n <= 32768.
DORA_HDI uint32_t clamp_to(int32_t v, uint32_t n) {
  const int32_t hi = static_cast<int32_t>(n);
  return static_cast<uint32_t>(v < 0 ? 0 : v > hi ? hi : v);
}

// The box and the taps of the element the odometer stands on: the box again only where the crop
// differs from the one it was read for, an axis' taps where the box or its coordinate does.  With
// the step (`pa` a prep::Args) the terms of a non-empty box's element as resize fetches them.
template <class CW, class PA, class M>
DORA_HDI void refresh(const Args& a, CW& c, M& m, const PA& pa) {
  const int64_t k = resize::coord(c.w.p, a.kax);
  if (k != c.ok) {
    c.ok = k;
    const int64_t at = 16 * k;  // k < K <= 2^20
    const int32_t alo = m.load_box(at), blo = m.load_box(at + 4);
    const int32_t ahi = m.load_box(at + 8), bhi = m.load_box(at + 12);
    const uint32_t a0 = clamp_to(alo, a.r.in[0]), a1 = clamp_to(ahi, a.r.in[0]);
    const uint32_t b0 = clamp_to(blo, a.r.in[1]), b1 = clamp_to(bhi, a.r.in[1]);
    const bool full = a1 > a0 && b1 > b0;
    c.a0 = a0;
    c.b0 = b0;
    c.ia = full ? a1 - a0 : 0;
    c.ib = full ? b1 - b0 : 0;
    c.w.oa = c.w.ob = -1;
  }
  if (!c.ia) return;
  const int64_t oa = resize::coord(c.w.p, a.r.ax[0]), ob = resize::coord(c.w.p, a.r.ax[1]);
  if (oa != c.w.oa) {
    c.w.oa = oa;
    resize::tap_of(a.r.mode, c.ia, a.r.out[0], static_cast<uint32_t>(oa), a.r.sa[0], c.w.ta, m);
    const int64_t first = static_cast<int64_t>(c.a0) * a.r.sa[0];
    c.w.ta.s0 += first;
    c.w.ta.s1 += first;
  }
  if (ob != c.w.ob) {
    c.w.ob = ob;
    resize::tap_of(a.r.mode, c.ib, a.r.out[1], static_cast<uint32_t>(ob), a.r.sa[1], c.w.tb, m);
    const int64_t first = static_cast<int64_t>(c.b0) * a.r.sa[1];
    c.w.tb.s0 += first;
    c.w.tb.s1 += first;
  }
  if constexpr (PA::on) resize::refresh_terms(c.w.p, c.w, m, pa);
}

template <class CW, class PA, class M>
DORA_HDI void walk_start(const Args& a, uint64_t e, CW& c, M& m, const PA& pa) {
  row_pos(a.r.g, e, c.w.p);
  c.ok = -1;
  c.ia = c.ib = c.a0 = c.b0 = 0;
  if constexpr (PA::on) resize::start_terms(c.w, pa);
  refresh(a, c, m, pa);
}

template <class CW, class PA, class M>
DORA_HDI void walk_next(const Args& a, CW& c, M& m, const PA& pa) {
  next_row(a.r.g, c.w.p);
  refresh(a, c, m, pa);
}

// The element the walk stands on as a destination element of D bytes, zero-extended; its source
// of type K.  An empty box's element is zero before anything else, the step included.
template <uint32_t K, int D, class CW, class PA, class M>
DORA_HDI uint32_t elem_at(const Args& a, const CW& c, M& m, const PA& pa) {
  if (!c.ia) return 0u;
  if constexpr (PA::on)
    return resize::to_dst<D>(a.r, resize::step(resize::value_at<K>(a.r, c.w, m), c.w, m, pa), m);
  else
    return resize::to_dst<D>(a.r, resize::value_at<K>(a.r, c.w, m), m);
}

template <class M>
DORA_HDI void walk_start(const Args& a, uint64_t e, Walk& c, M& m) {
  walk_start(a, e, c, m, prep::None{});
}
template <class M>
DORA_HDI void walk_next(const Args& a, Walk& c, M& m) {
  walk_next(a, c, m, prep::None{});
}
template <uint32_t K, int D, class M>
DORA_HDI uint32_t elem_at(const Args& a, const Walk& c, M& m) {
  return elem_at<K, D>(a, c, m, prep::None{});
}

// Whole unit `u` of the output.
template <uint32_t K, int D, class PA, class M>
DORA_HDI void crop_unit(const Args& a, uint64_t u, M& m, const PA& pa) {
  constexpr int E = 16 / D;
  const uint64_t e = a.r.g.head + static_cast<uint64_t>(E) * u;
  WalkFor<PA> c;
  walk_start(a, e, c, m, pa);
  U16 out = {{0, 0, 0, 0}};
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const uint32_t q = elem_at<K, D>(a, c, m, pa);
    if constexpr (D == 1) out.w[j / 4] |= q << (8 * (j % 4));
    else if constexpr (D == 2) out.w[j / 2] |= q << (16 * (j % 2));
    else out.w[j] = q;
    if (j + 1 < E) walk_next(a, c, m, pa);
  }
  m.store16(e * D, out);
}

// Output element `e` on its own (before the first and after the last whole unit).
template <uint32_t K, int D, class PA, class M>
DORA_HDI void crop_elem(const Args& a, uint64_t e, M& m, const PA& pa) {
  WalkFor<PA> c;
  walk_start(a, e, c, m, pa);
  m.template store_elem<D>(e, elem_at<K, D>(a, c, m, pa));
}

// resize::lane_as' division of the work: lanes 0..15 a head element each, lanes 16..31 a tail
// element each, and every lane the whole units lane, lane + lanes, ..
template <uint32_t K, int D, class PA, class M>
DORA_HDI void lane_as(const Args& a, uint64_t lane, uint64_t lanes, M& m, const PA& pa) {
  constexpr int E = 16 / D;
  static_assert(E - 1 <= 15, "16 lanes each for the head's and the tail's elements");
  if (lane < 16) {
    if (lane < a.r.g.head) crop_elem<K, D>(a, lane, m, pa);
  } else if (lane < 32) {
    const uint64_t t0 = a.r.g.head + static_cast<uint64_t>(E) * a.r.g.nunits;  // <= total
    if (lane - 16 < a.r.g.total - t0) crop_elem<K, D>(a, t0 + (lane - 16), m, pa);
  }
  for (uint64_t u = lane; u < a.r.g.nunits; u += lanes) crop_unit<K, D>(a, u, m, pa);
}

template <uint32_t K, class PA, class M>
DORA_HDI void lane_of(const Args& a, uint64_t lane, uint64_t lanes, M& m, const PA& pa) {
  switch (a.r.dsize) {
    case 1: lane_as<K, 1>(a, lane, lanes, m, pa); break;
    case 2: lane_as<K, 2>(a, lane, lanes, m, pa); break;
    default: lane_as<K, 4>(a, lane, lanes, m, pa); break;
  }
}

// Everything lane `lane` of `lanes` does for a field of crops; with `pa` a prep::Args
// (gather_crop_prep_kernel) every element of a non-empty box goes through the affine step.
template <class PA, class M>
DORA_HDI void crop_lane(const Args& a, uint64_t lane, uint64_t lanes, M& m, const PA& pa) {
  switch (a.r.src) {
    case cast::kU8: lane_of<cast::kU8>(a, lane, lanes, m, pa); break;
    case cast::kI8: lane_of<cast::kI8>(a, lane, lanes, m, pa); break;
    case cast::kU16: lane_of<cast::kU16>(a, lane, lanes, m, pa); break;
    case cast::kI16: lane_of<cast::kI16>(a, lane, lanes, m, pa); break;
    case cast::kF16: lane_of<cast::kF16>(a, lane, lanes, m, pa); break;
    case cast::kBF16: lane_of<cast::kBF16>(a, lane, lanes, m, pa); break;
    default: lane_of<cast::kF32>(a, lane, lanes, m, pa); break;
  }
}

template <class M>
DORA_HDI void crop_lane(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  crop_lane(a, lane, lanes, m, prep::None{});
}

}  // namespace crop

namespace multi {

// Arguments of a crop plan's launch (gather_crop_kernel): field k through the crop body where
// c[k].on (g[k] its whole frame), else as make_args places it (rows or tile by tile_c[k]); each
// field gets the grid its body asks for.
DORA_HD Args make_crop_args(const GatherDesc* g, const CropDesc* c, const uint64_t* off,
                            const int* tile_c, int n, uint8_t* dst) {
  return make_args_by(n, dst, nullptr, [&](int k, Field& f) {
    if (!c[k].on) return place_plain(f, g[k], dst + off[k], tile_c[k]);
    f.kind = kCrop;
    f.crop = crop::make_args(g[k], c[k], dst + off[k]);
    return static_cast<uint32_t>(crop::grid_for(f.crop));
  });
}

}  // namespace multi

namespace prep {

// resize's make_resize_launch for a launch of gather_crop_prep_kernel: a crops field's step is
// held against its output with K in front (c[k].rs).
DORA_HD Launch make_crop_launch(const GatherDesc* g, const CropDesc* c, const PrepDesc* d,
                                const uint64_t* off, const int* tile_c, int n, uint8_t* dst) {
  Launch l{};
  l.a = multi::make_crop_args(g, c, off, tile_c, n, dst);
  for (int k = 0; k < n; ++k)
    if (c[k].on) l.p[k] = make_args(d[k], c[k].rs);
  return l;
}

}  // namespace prep

}  // namespace gather
}  // namespace dora
