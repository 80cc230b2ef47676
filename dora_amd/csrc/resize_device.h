// Device code of the resizing gather (a field of a resize plan, tensor_plan.cpp): the row-major
// elements of the output — the source's shape with two extents replaced — each read from the
// source in place by one tap (nearest) or blended from four (bilinear), and written once as
// float16, float32, uint8, int8, uint16 or int16.
//
// The statement (include/dora_gpu.h has it in full).  A resized axis has source extent I and
// output extent O, both in [1, 32768], so every integer below fits 32 bits and is an exact
// float32.  Output coordinate o reads
//   nearest:  the tap i = (o * I) / O;
//   bilinear: d = 2 * O, n = max((2 * o + 1) * I - O, 0), q = n / d; if q >= I - 1 the taps
//             i0 = i1 = I - 1 with w0 = 1, w1 = 0, else i0 = q, i1 = q + 1, r = n % d,
//             w1 = float32(r) / float32(d), w0 = float32(d - r) / float32(d).
// Every source element is widened to float32 (exact).  With a the first resized axis and b the
// second, top = v[a0][b0] * wb0 + v[a0][b1] * wb1, bot = v[a1][b0] * wb0 + v[a1][b1] * wb1,
// y = top * wa0 + bot * wa1: every product rounded, then every sum, never a fused multiply-add.
// y goes to the destination as the cast body's float or quantised destinations do (no scale,
// zero point 0).
//
// It is in the style of cast_device.h and reduce_device.h: every address and position
// computation is plain C++ in functions that compile for host and device alike; all memory,
// every conversion, product, sum and the weights' division go through a policy object `M`, and
// nothing here uses an intrinsic.  The kernel (kernels.hip, gather_resize_kernel) passes a policy
// of real loads, stores and the hardware's arithmetic, product and sum opaque to the compiler,
// which would contract them; the host plan passes the plain-integer conversions of cast_device.h;
// the emulation of tests/test_resize_index_host.py runs the same functions lane by lane over the
// whole grid with every offset and alignment checked.
//
// The output is cut into 16-byte units on absolute 16-byte boundaries of the destination,
// E = 16 / dsize elements each; the up to E - 1 elements before the first and after the last
// whole unit are written one by one, so nothing is written at or past the field's end.  A lane
// owns a unit: the output odometer (gather::RowPos over the output's shape, every element a row
// of its own, the two resized dimensions with stride 0) gives the coordinates of its first
// element and steps to the next; the two resized coordinates give the taps and weights of their
// axes, computed again only when a coordinate changes — the C channels of an HWC pixel share
// both axes' taps, the elements of a CHW unit those of the first axis.  Taps are naturally
// aligned element loads at off + ia * sa + ib * sb.  One 16-byte store a unit.
//
// Model inputs (gather_resize_prep_kernel, a prep plan of tensor_plan.cpp): the body takes the step
// as a type, prep::None or prep::Args, as cast_device.h's body takes its flag A — with None no line
// of the step is compiled.  With prep::Args three things are added.  Placement: an axis' taps are
// those of o - lead over `inner` output steps, and an element whose o is not in
// [lead, lead + inner) on either axis reads no tap and has the value `fill`.  Channel: the
// tables' index is the odometer's coordinate along their axis, so nothing is divided per element,
// and their words are fetched again only when that coordinate changes.  Step: y = r * S + B, the
// policy's product and then its sum, before to_dst.
#pragma once

#include <cstdint>

#include "cast_device.h"

namespace dora {
namespace gather {
namespace resize {

constexpr uint32_t kMaxExtent = 32768;

// Arguments of the resize of `g` (the whole source view: its base, element size and reach) by
// `r` into `dst`.
DORA_HD Args make_args(const GatherDesc& g, const ResizeDesc& r, uint8_t* dst) {
  Args a{};
  const uint32_t ds = r.dst_bits / 8u;
  a.g.src = g.view.src;
  a.g.dst = dst;
  a.g.total = r.count;
  a.g.row = 1;
  const uint64_t mis = ((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / ds;
  a.g.head = mis < a.g.total ? mis : a.g.total;
  a.g.nunits = (a.g.total - a.g.head) / (16u / ds);
  a.g.lo = g.lo;
  a.g.hi = g.hi;
  a.g.piece = g.elem;
  a.g.pad = 0;
  for (int k = 0; k < kDims; ++k) {
    const int i = k - (kDims - r.nd);
    const bool resized = i >= 0 && (i == r.ax[0] || i == r.ax[1]);
    a.g.shape[k] = i >= 0 ? r.shape[i] : 1;
    a.g.stride[k] = i >= 0 && !resized ? r.stride[i] : 0;
  }
  for (int j = 0; j < 2; ++j) {
    a.sa[j] = r.stride[r.ax[j]];
    a.in[j] = static_cast<uint32_t>(r.in[j]);
    a.out[j] = static_cast<uint32_t>(r.shape[r.ax[j]]);
    a.ax[j] = static_cast<uint8_t>(r.ax[j] + (kDims - r.nd));
  }
  a.mode = r.mode;
  const int kind = cast::src_kind(r.src_code, r.src_bits);
  a.src = static_cast<uint8_t>(kind < 0 ? 0 : kind);
  const int dk = r.dst_code == 2 ? int(cast::kDstFloat) : cast::dst_kind(r.dst_code, r.dst_bits);
  a.dst = static_cast<uint8_t>(dk < 0 ? 0 : dk);
  a.dsize = static_cast<uint8_t>(ds);
  return a;
}

DORA_HD uint64_t grid_for(const Args& a) { return gather::grid_for(a.g); }

// The taps of one axis at one output coordinate: the source byte offsets of the two taps along
// the axis and their weights (nearest: one tap, s1 == s0, and the weights are not read).
struct Tap {
  int64_t s0, s1;
  float w0, w1;
};

// Output coordinate `o` of an axis of `I` source and `O` output steps, `step` source bytes each.
template <class M>
DORA_HDI void tap_of(uint32_t mode, uint32_t I, uint32_t O, uint32_t o, int64_t step, Tap& t,
                     M& m) {
  if (mode == DORA_RESIZE_NEAREST) {
    const uint32_t i = (o * I) / O;  // < 2^15 * 2^15
    t.s0 = t.s1 = static_cast<int64_t>(i) * step;
    t.w0 = 1.0f;
    t.w1 = 0.0f;
    return;
  }
  const uint32_t d = 2 * O, x = (2 * o + 1) * I;  // x < 2^16 * 2^15
  const uint32_t n = x > O ? x - O : 0, q = n / d;
  if (q >= I - 1) {
    t.s0 = t.s1 = static_cast<int64_t>(I - 1) * step;
    t.w0 = 1.0f;
    t.w1 = 0.0f;
    return;
  }
  const uint32_t r = n - q * d;
  t.s0 = static_cast<int64_t>(q) * step;
  t.s1 = t.s0 + step;
  t.w1 = m.ratio(r, d);
  t.w0 = m.ratio(d - r, d);
}

// Where a lane is in the output: the odometer's position, the coordinates the two axes' taps
// were computed for (-1: none yet) and those taps.
struct Walk {
  RowPos p;
  int64_t oa, ob;
  Tap ta, tb;
};

// The same under the model-input step (prep::Args): whether the element lies outside the placed
// image along either axis, the channel the terms were fetched for (-1: none yet) and the terms.
struct PrepWalk : Walk {
  int64_t oc;
  float s, b;
  bool outa, outb;
};
template <class PA>
struct WalkFor {
  using type = Walk;
};
template <>
struct WalkFor<prep::Args> {
  using type = PrepWalk;
};

// Index `ax` of the odometer, as a chain of selects: no register array is indexed by a variable.
DORA_HDI int64_t coord(const RowPos& p, uint32_t ax) {
  int64_t c = 0;
#pragma unroll
  for (int k = 0; k < kDims; ++k) c = static_cast<uint32_t>(k) == ax ? p.idx[k] : c;
  return c;
}

// The terms of the element the odometer stands on: the tables' words again only where the
// coordinate along their axis differs from the one they were fetched for (CHW: rarely; HWC: every
// element, the same few words a wave shares).  The channel is a coordinate, never a division.
template <class W, class M>
DORA_HDI void refresh_terms(const RowPos& p, W& w, M& m, const prep::Args& pa) {
  if (!pa.stab && !pa.btab) return;
  const int64_t c = coord(p, pa.cax);
  if (c == w.oc) return;
  w.oc = c;  // < shape[cax], the tables' length
  if (pa.stab) w.s = m.load_table(pa.stab, static_cast<uint64_t>(c));
  if (pa.btab) w.b = m.load_table(pa.btab, static_cast<uint64_t>(c));
}

// The walk's terms before any element: the scalars, and no channel fetched.
template <class W>
DORA_HDI void start_terms(W& w, const prep::Args& pa) {
  w.oc = -1;
  w.s = pa.scale;
  w.b = pa.bias;
  w.outa = w.outb = false;
}

// The taps of the element the odometer stands on: an axis' taps again only where its coordinate
// differs from the one they were computed for.  With the step (`pa` a prep::Args) an axis' taps
// are those of o - lead over `inner` output steps, and the axis is marked outside where o is not
// in [lead, lead + inner): no tap is computed for it.
template <class W, class PA, class M>
DORA_HDI void refresh(const Args& a, W& w, M& m, const PA& pa) {
  const int64_t oa = coord(w.p, a.ax[0]), ob = coord(w.p, a.ax[1]);
  if (oa != w.oa) {
    w.oa = oa;
    if constexpr (PA::on) {
      const int64_t o = oa - pa.lead[0];
      w.outa = o < 0 || o >= pa.inner[0];
      if (!w.outa)
        tap_of(a.mode, a.in[0], pa.inner[0], static_cast<uint32_t>(o), a.sa[0], w.ta, m);
    } else {
      tap_of(a.mode, a.in[0], a.out[0], static_cast<uint32_t>(oa), a.sa[0], w.ta, m);
    }
  }
  if (ob != w.ob) {
    w.ob = ob;
    if constexpr (PA::on) {
      const int64_t o = ob - pa.lead[1];
      w.outb = o < 0 || o >= pa.inner[1];
      if (!w.outb)
        tap_of(a.mode, a.in[1], pa.inner[1], static_cast<uint32_t>(o), a.sa[1], w.tb, m);
    } else {
      tap_of(a.mode, a.in[1], a.out[1], static_cast<uint32_t>(ob), a.sa[1], w.tb, m);
    }
  }
  if constexpr (PA::on) refresh_terms(w.p, w, m, pa);
}

template <class W, class PA, class M>
DORA_HDI void walk_start(const Args& a, uint64_t e, W& w, M& m, const PA& pa) {
  row_pos(a.g, e, w.p);
  w.oa = w.ob = -1;
  if constexpr (PA::on) start_terms(w, pa);
  refresh(a, w, m, pa);
}

template <class W, class PA, class M>
DORA_HDI void walk_next(const Args& a, W& w, M& m, const PA& pa) {
  next_row(a.g, w.p);
  refresh(a, w, m, pa);
}

template <class M>
DORA_HDI void refresh(const Args& a, Walk& w, M& m) {
  refresh(a, w, m, prep::None{});
}
template <class M>
DORA_HDI void walk_start(const Args& a, uint64_t e, Walk& w, M& m) {
  walk_start(a, e, w, m, prep::None{});
}
template <class M>
DORA_HDI void walk_next(const Args& a, Walk& w, M& m) {
  walk_next(a, w, m, prep::None{});
}

// The value of the element the walk stands on, its source of type K.
template <uint32_t K, class M>
DORA_HDI float value_at(const Args& a, const Walk& w, M& m) {
  constexpr int S = cast::kSize<K>;
  const int64_t r0 = w.p.off + w.ta.s0;
  if (a.mode == DORA_RESIZE_NEAREST)
    return m.template to_f32<K>(m.template load_elem<S>(r0 + w.tb.s0));
  const int64_t r1 = w.p.off + w.ta.s1;
  const float v00 = m.template to_f32<K>(m.template load_elem<S>(r0 + w.tb.s0));
  const float v01 = m.template to_f32<K>(m.template load_elem<S>(r0 + w.tb.s1));
  const float v10 = m.template to_f32<K>(m.template load_elem<S>(r1 + w.tb.s0));
  const float v11 = m.template to_f32<K>(m.template load_elem<S>(r1 + w.tb.s1));
  const float top = m.add(m.mul(v00, w.tb.w0), m.mul(v01, w.tb.w1));
  const float bot = m.add(m.mul(v10, w.tb.w0), m.mul(v11, w.tb.w1));
  return m.add(m.mul(top, w.ta.w0), m.mul(bot, w.ta.w1));
}

// `y` as a destination element of D bytes, zero-extended.
template <int D, class M>
DORA_HDI uint32_t to_dst(const Args& a, float y, M& m) {
  if constexpr (D == 4) {
    return m.f32_bits(y);
  } else {
    if (D == 2 && a.dst == cast::kDstFloat) return m.to_f16(y);
    const uint32_t q =
        static_cast<uint32_t>(m.to_int(y, cast::dst_lo(a.dst), cast::dst_hi(a.dst), 0));
    return D == 1 ? q & 0xffu : q & 0xffffu;
  }
}

// The affine step of the model-input fields: the product rounded, then the sum, each applied only
// where its term is present (a zero product keeps its sign).
template <class W, class M>
DORA_HDI float step(float y, const W& w, M& m, const prep::Args& pa) {
  if (pa.has_scale) y = m.mul(y, w.s);
  if (pa.has_bias) y = m.add(y, w.b);
  return y;
}

// The value of the element the walk stands on before its conversion: value_at, or with the step
// the fill where the element lies outside the placed image (no tap is read), then the step.
template <uint32_t K, class W, class PA, class M>
DORA_HDI float prepped_at(const Args& a, const W& w, M& m, const PA& pa) {
  if constexpr (PA::on) {
    float r;
    if (w.outa || w.outb) r = pa.fill;
    else r = value_at<K>(a, w, m);
    return step(r, w, m, pa);
  } else {
    return value_at<K>(a, w, m);
  }
}

// Whole unit `u` of the output.
template <uint32_t K, int D, class PA, class M>
DORA_HDI void resize_unit(const Args& a, uint64_t u, M& m, const PA& pa) {
  constexpr int E = 16 / D;
  const uint64_t e = a.g.head + static_cast<uint64_t>(E) * u;
  typename WalkFor<PA>::type w;
  walk_start(a, e, w, m, pa);
  U16 out = {{0, 0, 0, 0}};
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const uint32_t q = to_dst<D>(a, prepped_at<K>(a, w, m, pa), m);
    if constexpr (D == 1) out.w[j / 4] |= q << (8 * (j % 4));
    else if constexpr (D == 2) out.w[j / 2] |= q << (16 * (j % 2));
    else out.w[j] = q;
    if (j + 1 < E) walk_next(a, w, m, pa);
  }
  m.store16(e * D, out);
}

// Output element `e` on its own (before the first and after the last whole unit).
template <uint32_t K, int D, class PA, class M>
DORA_HDI void resize_elem(const Args& a, uint64_t e, M& m, const PA& pa) {
  typename WalkFor<PA>::type w;
  walk_start(a, e, w, m, pa);
  m.template store_elem<D>(e, to_dst<D>(a, prepped_at<K>(a, w, m, pa), m));
}

// cast_lane_as' division of the work: lanes 0..15 a head element each, lanes 16..31 a tail
// element each (at most E - 1 <= 15 of either), and every lane the whole units lane,
// lane + lanes, ..
template <uint32_t K, int D, class PA, class M>
DORA_HDI void lane_as(const Args& a, uint64_t lane, uint64_t lanes, M& m, const PA& pa) {
  constexpr int E = 16 / D;
  static_assert(E - 1 <= 15, "16 lanes each for the head's and the tail's elements");
  if (lane < 16) {
    if (lane < a.g.head) resize_elem<K, D>(a, lane, m, pa);
  } else if (lane < 32) {
    const uint64_t t0 = a.g.head + static_cast<uint64_t>(E) * a.g.nunits;  // <= total
    if (lane - 16 < a.g.total - t0) resize_elem<K, D>(a, t0 + (lane - 16), m, pa);
  }
  for (uint64_t u = lane; u < a.g.nunits; u += lanes) resize_unit<K, D>(a, u, m, pa);
}

template <uint32_t K, class PA, class M>
DORA_HDI void lane_of(const Args& a, uint64_t lane, uint64_t lanes, M& m, const PA& pa) {
  switch (a.dsize) {
    case 1: lane_as<K, 1>(a, lane, lanes, m, pa); break;
    case 2: lane_as<K, 2>(a, lane, lanes, m, pa); break;
    default: lane_as<K, 4>(a, lane, lanes, m, pa); break;
  }
}

// Everything lane `lane` of `lanes` does for a resized field; with `pa` a prep::Args
// (gather_resize_prep_kernel) every element goes through placement and the affine step, without
// it (prep::None) no line of either is compiled.
template <class PA, class M>
DORA_HDI void resize_lane(const Args& a, uint64_t lane, uint64_t lanes, M& m, const PA& pa) {
  switch (a.src) {
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
DORA_HDI void resize_lane(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  resize_lane(a, lane, lanes, m, prep::None{});
}

// The conversions and arithmetic of a policy without the hardware's (host plans, the emulation):
// cast_device.h's plain-integer routines, and product, sum and quotient each read back through a
// volatile so that no compiler contracts a product into the sum that takes it.
struct HostArith : cast::HostCvt {
  float mul(float x, float s) const {
    volatile float p = x * s;
    return p;
  }
  float add(float x, float b) const {
    volatile float p = x, q = b;
    volatile float y = p + q;
    return y;
  }
  float ratio(uint32_t r, uint32_t d) const {
    volatile float y = static_cast<float>(r) / static_cast<float>(d);
    return y;
  }
};

}  // namespace resize

namespace multi {

// Arguments of a resize plan's launch (gather_resize_kernel): field k through the resize body
// where r[k].on (g[k] its whole source view), else as make_args places it (rows or tile by
// tile_c[k]); each field gets the grid its body asks for.
DORA_HD Args make_resize_args(const GatherDesc* g, const ResizeDesc* r, const uint64_t* off,
                              const int* tile_c, int n, uint8_t* dst) {
  return make_args_by(n, dst, nullptr, [&](int k, Field& f) {
    if (!r[k].on) return place_plain(f, g[k], dst + off[k], tile_c[k]);
    f.kind = kResize;
    f.resize = resize::make_args(g[k], r[k], dst + off[k]);
    return static_cast<uint32_t>(resize::grid_for(f.resize));
  });
}

}  // namespace multi

namespace prep {

// The step's arguments of a field whose output `r` describes (a crops field's with K in front,
// `d.axis` counted with it): the image fills the output unless `d` places it.
DORA_HD Args make_args(const PrepDesc& d, const ResizeDesc& r) {
  Args a{};
  a.stab = d.scale_tab;
  a.btab = d.bias_tab;
  a.scale = d.scale;
  a.bias = d.bias;
  a.fill = d.fill;
  for (int j = 0; j < 2; ++j) {
    a.inner[j] = static_cast<uint16_t>(d.placed ? d.inner[j] : r.shape[r.ax[j]]);
    a.lead[j] = static_cast<uint16_t>(d.placed ? d.lead[j] : 0);
  }
  a.cax = static_cast<uint8_t>(d.axis + (kDims - r.nd));
  a.has_scale = d.scale_tab || d.has_scale;
  a.has_bias = d.bias_tab || d.has_bias;
  return a;
}

// Arguments of a launch of gather_resize_prep_kernel or gather_crop_prep_kernel: the launch as
// the plain kernels take it and, beside f[], the step of every field (all zero but `inner` for a
// field without one), read by these two kernels alone.
struct Launch {
  multi::Args a;
  Args p[multi::kMaxFields];
};
static_assert(sizeof(Launch) <= 4096, "prep::Launch is passed by value: the kernel-argument limit");

DORA_HD Launch make_resize_launch(const GatherDesc* g, const ResizeDesc* r, const PrepDesc* d,
                                  const uint64_t* off, const int* tile_c, int n, uint8_t* dst) {
  Launch l{};
  l.a = multi::make_resize_args(g, r, off, tile_c, n, dst);
  for (int k = 0; k < n; ++k)
    if (r[k].on) l.p[k] = make_args(d[k], r[k]);
  return l;
}

}  // namespace prep

}  // namespace gather
}  // namespace dora
