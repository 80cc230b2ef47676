// Device code of the converting gather (a field of a cast plan, tensor_plan.cpp): the row-major
// elements of a strided view read once as their source type, converted, and written once as
// float16 or float32 — y = to_dst(to_f32(x) [* scale]), element by element — or, a quantised field,
// as uint8, int8, uint16 or int16: q = int(clip(rint(y), lo - zp, hi - zp)) + zp with a NaN taken
// as 0, [lo, hi] the destination's range and zp the zero point inside it.  With the affine step
// (template flag A, gather_affine_kernel) y = to_f32(x) * S + B first, S and B each a scalar, a
// per-channel table word or absent, product and sum rounded one after the other.
//
// It is gather_device.h's rows body restated per element, in the same style: every address
// computation is plain C++ in functions that compile for host and device alike, all memory and
// every conversion goes through a policy object `M`, and nothing here uses an intrinsic.  The
// kernel (kernels.hip, gather_cast_kernel and gather_quant_kernel) passes a policy of real loads, stores and the
// hardware's converts; the host emulation of tests/test_cast_index_host.py passes one that runs
// the same functions lane by lane over the whole grid with every offset and alignment checked,
// and converts with the plain-integer routines below, which the host plan uses as well.
//
// The view is gather::Args with rows counted in elements (cast::Args, gather_device.h); the
// odometer (RowPos, row_pos, next_row) is the gather's own.  The output is cut into 16-byte units
// on absolute 16-byte boundaries of the destination, E = 16 / dsize elements each; the up to
// E - 1 elements before the first and after the last whole unit are written one by one, so
// nothing is written at or past dst + total * dsize.  The destination is a multiple of dsize
// (the launcher refuses any other), the source of ssize (the plan does).
//
// A unit takes one of two paths.  Vector: its E elements lie in one contiguous run and their
// E * ssize bytes start on a multiple of min(E * ssize, 16): one load of 4, 8 or 16 bytes, or two
// or four of 16 (float32 -> float16 is 32 bytes a unit; an 8-bit destination has E = 16 and a
// source image of 16, 32 or 64 bytes), converted in registers.  Element: every other unit loads its
// elements one by one (ssize bytes each, naturally aligned), walking the odometer as rows end;
// permuted views (HWC -> CHW) take this path.  Either way one 16-byte store.  A tiled transpose
// that converts is not provided.
#pragma once

#include <cstdint>

#include "gather_device.h"

namespace dora {
namespace gather {
namespace cast {

// DLPack (code, bits) -> Src, or -1 when the dtype is no cast source.
DORA_HD int src_kind(unsigned code, unsigned bits) {
  if (code == 1) return bits == 8 ? int(kU8) : bits == 16 ? int(kU16) : -1;
  if (code == 0) return bits == 8 ? int(kI8) : bits == 16 ? int(kI16) : -1;
  if (code == 2) return bits == 16 ? int(kF16) : bits == 32 ? int(kF32) : -1;
  if (code == 4) return bits == 16 ? int(kBF16) : -1;
  return -1;
}

template <uint32_t K>
constexpr int kSize = K <= kI8 ? 1 : K <= kBF16 ? 2 : 4;

// ------------------------------------------------------------------------------------------
// Conversions in plain integer arithmetic, for policies without the hardware's (the host
// compiler may have no _Float16).  Bit patterns in, bit patterns out.
// ------------------------------------------------------------------------------------------
DORA_HD uint32_t bits_of(float x) {
  uint32_t u;
  __builtin_memcpy(&u, &x, 4);
  return u;
}
DORA_HD float f32_of(uint32_t u) {
  float x;
  __builtin_memcpy(&x, &u, 4);
  return x;
}

// float16 -> float32: exact, subnormals normalised, a NaN stays a NaN.
DORA_HD uint32_t f16_to_f32_bits(uint32_t h) {
  const uint32_t sign = (h & 0x8000u) << 16;
  const uint32_t exp = (h >> 10) & 31;
  uint32_t man = h & 0x3ffu;
  if (exp == 31) return sign | 0x7f800000u | (man << 13);
  if (exp) return sign | ((exp + 112) << 23) | (man << 13);
  if (!man) return sign;
  uint32_t shift = 0;  // man * 2^-24 = 1.f * 2^(-14 - shift)
  while (!(man & 0x400u)) {
    man <<= 1;
    ++shift;
  }
  return sign | ((113 - shift) << 23) | ((man & 0x3ffu) << 13);
}

// float32 -> float16, round to nearest even: overflow gives infinity (65520 and up), results
// below 2^-14 are float16 subnormals (not flushed), a NaN gives a quiet NaN.
DORA_HD uint32_t f32_to_f16_bits(uint32_t x) {
  const uint32_t sign = (x >> 16) & 0x8000u;
  const uint32_t mag = x & 0x7fffffffu;
  if (mag > 0x7f800000u) return sign | 0x7e00u;
  const int32_t e = static_cast<int32_t>(mag >> 23) - 112;  // the float16 exponent field
  if (e >= 31) return sign | 0x7c00u;
  uint32_t m = mag & 0x7fffffu, q, rem, half;
  if (e <= 0) {
    if (e < -10) return sign;  // below half the smallest subnormal (float32 subnormals too)
    m |= 0x800000u;            // m * 2^(e - 38): in units of 2^-24, m >> (14 - e)
    const uint32_t s = static_cast<uint32_t>(14 - e);  // 14..24
    q = m >> s;
    rem = m & ((1u << s) - 1);
    half = 1u << (s - 1);
  } else {
    q = (static_cast<uint32_t>(e) << 10) | (m >> 13);
    rem = m & 0x1fffu;
    half = 0x1000u;
  }
  if (rem > half || (rem == half && (q & 1))) ++q;  // (a carry runs into the exponent, up to inf)
  return sign | q;
}

// float32 -> clamped integer: the value rounded to the nearest integer, ties to even, a NaN as 0,
// clamped to [lo, hi] (|lo|, |hi| < 2^24, lo <= 0 <= hi: the caller's range less its zero point),
// plus zp.  On the bit pattern alone, so the floating-point environment has no say.
DORA_HD int32_t quantize_bits(uint32_t x, int32_t lo, int32_t hi, int32_t zp) {
  const bool neg = (x >> 31) != 0;
  const uint32_t mag = x & 0x7fffffffu, e = mag >> 23;
  int32_t r;
  if (mag > 0x7f800000u || e < 126) {
    r = 0;  // a NaN; |y| < 0.5
  } else if (e >= 150) {
    r = neg ? lo : hi;  // |y| >= 2^24 (an integer past either bound), +-inf
  } else {
    const uint32_t m = (mag & 0x7fffffu) | 0x800000u, s = 150 - e;  // |y| = m * 2^-s, s in 1..24
    uint32_t q = m >> s;
    const uint32_t rem = m & ((1u << s) - 1), half = 1u << (s - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    r = neg ? -static_cast<int32_t>(q) : static_cast<int32_t>(q);
    r = r < lo ? lo : r > hi ? hi : r;
  }
  return r + zp;
}

// The range of a quantised destination.
DORA_HD int32_t dst_lo(uint32_t d) { return d == kDstI8 ? -128 : d == kDstI16 ? -32768 : 0; }
DORA_HD int32_t dst_hi(uint32_t d) {
  return d == kDstU8 ? 255 : d == kDstI8 ? 127 : d == kDstU16 ? 65535 : 32767;
}
// DLPack (code, bits) -> Dst of a quantised field, or -1 when the dtype is no such destination.
DORA_HD int dst_kind(unsigned code, unsigned bits) {
  if (code == 1) return bits == 8 ? int(kDstU8) : bits == 16 ? int(kDstU16) : -1;
  if (code == 0) return bits == 8 ? int(kDstI8) : bits == 16 ? int(kDstI16) : -1;
  return -1;
}

// An integer source element (zero-extended raw bits) as float32: exact for 8 and 16 bits.
template <uint32_t K>
DORA_HD float int_to_f32(uint32_t raw) {
  if constexpr (K == kU8) return static_cast<float>(static_cast<uint8_t>(raw));
  if constexpr (K == kI8) return static_cast<float>(static_cast<int8_t>(raw));
  if constexpr (K == kU16) return static_cast<float>(static_cast<uint16_t>(raw));
  return static_cast<float>(static_cast<int16_t>(raw));
}

// The conversions of a policy without hardware converts (host plans, the emulation).  The
// product is the host's own float32 multiplication: IEEE, round to nearest even, subnormals kept.
struct HostCvt {
  template <uint32_t K>
  float to_f32(uint32_t raw) const {
    if constexpr (K == kF32) return f32_of(raw);
    else if constexpr (K == kBF16) return f32_of(raw << 16);
    else if constexpr (K == kF16) return f32_of(f16_to_f32_bits(raw));
    else return int_to_f32<K>(raw);
  }
  float mul(float x, float s) const { return x * s; }
  // The sum of the affine step, a rounding of its own: the product is read back through a
  // volatile so that no compiler contracts the pair into one fused multiply-add.
  float add(float x, float b) const {
    volatile float p = x;
    return p + b;
  }
  uint32_t to_f16(float y) const { return f32_to_f16_bits(bits_of(y)); }
  uint32_t f32_bits(float y) const { return bits_of(y); }
  int32_t to_int(float y, int32_t lo, int32_t hi, int32_t zp) const {
    return quantize_bits(bits_of(y), lo, hi, zp);
  }
};

// ------------------------------------------------------------------------------------------
// Arguments
// ------------------------------------------------------------------------------------------

// Arguments of the cast of `g` (the source view, in source bytes) by `c` into `dst`.
DORA_HD Args make_args(const GatherDesc& g, const CastDesc& c, uint8_t* dst) {
  Args a{};
  const uint32_t ss = g.elem, ds = c.dst_bits / 8u;
  a.g.src = g.view.src;
  a.g.dst = dst;
  a.g.total = c.count;
  a.g.row = g.view.row / ss;
  const uint64_t mis = ((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15) / ds;
  a.g.head = mis < a.g.total ? mis : a.g.total;
  a.g.nunits = (a.g.total - a.g.head) / (16u / ds);
  a.g.lo = g.lo;
  a.g.hi = g.hi;
  a.g.piece = ss;
  a.g.pad = 0;
  for (int k = 0; k < kDims; ++k) {
    const int i = k - (kDims - g.view.nd);
    a.g.shape[k] = i >= 0 ? g.view.shape[i] : 1;
    a.g.stride[k] = i >= 0 ? g.view.stride[i] : 0;
  }
  const int kind = src_kind(c.src_code, c.src_bits);
  a.src = static_cast<uint32_t>(kind < 0 ? 0 : kind);
  a.dsize = ds;
  a.has_scale = c.has_scale;
  a.scale = c.scale;
  const int dk = c.dst_code == 2 ? int(kDstFloat) : dst_kind(c.dst_code, c.dst_bits);
  a.dst = static_cast<uint32_t>(dk < 0 ? 0 : dk);
  a.zp = c.zero_point;
  a.stab = c.scale_tab;
  a.btab = c.bias_tab;
  a.inner = c.inner;
  a.channels = c.channels;
  a.has_bias = c.has_bias;
  a.bias = c.bias;
  return a;
}

DORA_HD uint64_t grid_for(const Args& a) { return gather::grid_for(a.g); }

// ------------------------------------------------------------------------------------------
// The body.  Loading is written once per destination size, with the source element size a
// run-time value (uniform over a field's share): it yields the unit's E * ssize source bytes as
// they would lie in one contiguous run.  Converting is written once per source type over that
// image, so every shift in it is a constant.
// ------------------------------------------------------------------------------------------

// 16-byte words of a unit's source image: E * 4 bytes at most.
template <int D>
constexpr int kImage = D == 1 ? 4 : 2;

// Element `j` of S bytes of the image `v` (little-endian), zero-extended.
template <int S>
DORA_HDI uint32_t elem_of(const U16* v, int j) {
  const int w = j * S / 4;
  if constexpr (S == 1) return (v[w / 4].w[w % 4] >> (8 * (j % 4))) & 0xffu;
  else if constexpr (S == 2) return (v[w / 4].w[w % 4] >> (16 * (j % 2))) & 0xffffu;
  else return v[w / 4].w[w % 4];
}

// The source bytes of the E elements from output element `e` on into v[0..kImage<D>): vector
// loads where they are contiguous and the first is naturally aligned, else element by element
// across rows.
template <int D, class M>
DORA_HDI void load_unit(const Args& a, uint64_t e, M& m, U16* v) {
  constexpr int E = 16 / D;
  const uint32_t ss = a.g.piece, n = E * ss;  // n: 4, 8, 16, 32 or 64 source bytes a unit
  uint64_t r, b;
  out_pos(a.g, e, &r, &b);
  RowPos p;
  row_pos(a.g, r, p);
#pragma unroll
  for (int k = 0; k < kImage<D>; ++k) v[k] = U16{{0, 0, 0, 0}};
  if (b + E <= a.g.row) {
    const int64_t s = p.off + static_cast<int64_t>(b * ss);
    const uint32_t align = n > 16 ? 16 : n;
    if (((reinterpret_cast<uintptr_t>(a.g.src) + static_cast<uint64_t>(s)) & (align - 1)) == 0) {
      switch (n) {
        case 4: v[0] = m.template load_vec<4>(s); break;
        case 8: v[0] = m.template load_vec<8>(s); break;
        case 16: v[0] = m.template load_vec<16>(s); break;
        case 32:
          v[0] = m.template load_vec<16>(s);
          v[1] = m.template load_vec<16>(s + 16);
          break;
        default:
          if constexpr (D == 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = m.template load_vec<16>(s + 16 * k);
          }
          break;
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int64_t s = p.off + static_cast<int64_t>(b * ss);
    switch (ss) {
      case 1: v[0].w[j / 4] |= m.template load_elem<1>(s) << (8 * (j % 4)); break;
      case 2: v[j / 8].w[(j % 8) / 2] |= m.template load_elem<2>(s) << (16 * (j % 2)); break;
      default: v[j / 4].w[j % 4] = m.template load_elem<4>(s); break;
    }
    if (++b >= a.g.row) {
      b = 0;
      next_row(a.g, p);
    }
  }
}

// The channel of an output element under the affine step: element e is of channel
// c = (e / inner) % channels, `rem` = e % inner elements into that channel's run.
struct Chan {
  uint64_t rem, c;
};

// Output element `e` -> Chan: one division and one remainder, 32-bit where the operands allow.
DORA_HDI void chan_pos(uint64_t inner, uint64_t channels, uint64_t e, Chan& ch) {
  if ((e | inner | channels) >> 32) {
    const uint64_t q = e / inner;
    ch.rem = e - q * inner;
    ch.c = q % channels;
  } else {
    const uint32_t e32 = static_cast<uint32_t>(e), i32 = static_cast<uint32_t>(inner);
    const uint32_t q = e32 / i32;
    ch.rem = e32 - q * i32;
    ch.c = q % static_cast<uint32_t>(channels);
  }
}

// The Chan of the next output element: `rem` counts up to inner, then `c` up to channels, so
// c < channels always and nothing is divided per element.
DORA_HDI void chan_next(uint64_t inner, uint64_t channels, Chan& ch) {
  if (++ch.rem < inner) return;
  ch.rem = 0;
  if (++ch.c >= channels) ch.c = 0;
}

// The image's E elements of source type K -> the unit's 16 output bytes: floats of D bytes, or
// with Q integers of D bytes, each the product quantised into the destination's range.  With A
// (gather_affine_kernel's body) the elements are output elements e, e + 1, .. and each is taken
// through y * S + B of its channel first, product and sum rounded one after the other; without
// it `e` is not read and no line of the affine step is compiled.
template <uint32_t K, int D, bool Q, bool A, class M>
DORA_HDI U16 convert_as(const Args& a, const U16* v, uint64_t e, M& m) {
  constexpr int E = 16 / D;
  U16 out = {{0, 0, 0, 0}};
  // (the clip bounds less the zero point: exact as integers and as float32)
  const int32_t lo = Q ? dst_lo(a.dst) - a.zp : 0, hi = Q ? dst_hi(a.dst) - a.zp : 0;
  Chan ch{0, 0};
  if constexpr (A) {
    if (a.stab || a.btab) chan_pos(a.inner, a.channels, e, ch);
  }
#pragma unroll
  for (int j = 0; j < E; ++j) {
    float y = m.template to_f32<K>(elem_of<kSize<K>>(v, j));
    if constexpr (A) {
      if (a.stab) y = m.mul(y, m.load_table(a.stab, ch.c));
      else if (a.has_scale) y = m.mul(y, a.scale);
      if (a.btab) y = m.add(y, m.load_table(a.btab, ch.c));
      else if (a.has_bias) y = m.add(y, a.bias);
      if (a.stab || a.btab) chan_next(a.inner, a.channels, ch);
    } else {
      if (a.has_scale) y = m.mul(y, a.scale);
    }
    if constexpr (Q) {
      const uint32_t q = static_cast<uint32_t>(m.to_int(y, lo, hi, a.zp));
      if constexpr (D == 1) out.w[j / 4] |= (q & 0xffu) << (8 * (j % 4));
      else out.w[j / 2] |= (q & 0xffffu) << (16 * (j % 2));
    } else {
      if constexpr (D == 2) out.w[j / 2] |= m.to_f16(y) << (16 * (j % 2));
      else out.w[j] = m.f32_bits(y);
    }
  }
  return out;
}

template <int D, bool Q, bool A, class M>
DORA_HDI U16 convert_unit(const Args& a, const U16* v, uint64_t e, M& m) {
  switch (a.src) {
    case kU8: return convert_as<kU8, D, Q, A>(a, v, e, m);
    case kI8: return convert_as<kI8, D, Q, A>(a, v, e, m);
    case kU16: return convert_as<kU16, D, Q, A>(a, v, e, m);
    case kI16: return convert_as<kI16, D, Q, A>(a, v, e, m);
    case kF16: return convert_as<kF16, D, Q, A>(a, v, e, m);
    case kBF16: return convert_as<kBF16, D, Q, A>(a, v, e, m);
    default: return convert_as<kF32, D, Q, A>(a, v, e, m);
  }
}

// Whole unit `u` of the output.
template <int D, bool Q, bool A, class M>
DORA_HDI void cast_unit(const Args& a, uint64_t u, M& m) {
  const uint64_t e = a.g.head + static_cast<uint64_t>(16 / D) * u;
  U16 v[kImage<D>];
  load_unit<D>(a, e, m, v);
  m.store16(e * D, convert_unit<D, Q, A>(a, v, e, m));
}

// Output element `e` on its own (the elements before the first and after the last whole unit):
// element 0 of an image that holds nothing else.
template <int D, bool Q, bool A, class M>
DORA_HDI void cast_elem(const Args& a, uint64_t e, M& m) {
  const uint32_t ss = a.g.piece;
  uint64_t r, b;
  out_pos(a.g, e, &r, &b);
  RowPos p;
  row_pos(a.g, r, p);
  const int64_t s = p.off + static_cast<int64_t>(b * ss);
  U16 v[kImage<D>] = {};
  v[0].w[0] = ss == 1 ? m.template load_elem<1>(s)
                      : ss == 2 ? m.template load_elem<2>(s) : m.template load_elem<4>(s);
  const U16 y = convert_unit<D, Q, A>(a, v, e, m);
  m.template store_elem<D>(e, D == 1 ? y.w[0] & 0xffu : D == 2 ? y.w[0] & 0xffffu : y.w[0]);
}

// gather_lane's division of the work: lanes 0..15 a head element each, lanes 16..31 a tail
// element each (at most E - 1 <= 15 of either: the head ends at the first 16-byte boundary, the
// tail is less than a unit), and every lane the whole units lane, lane + lanes, ..
template <int D, bool Q, bool A, class M>
DORA_HDI void cast_lane_as(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  constexpr int E = 16 / D;
  static_assert(E - 1 <= 15, "16 lanes each for the head's and the tail's elements");
  if (lane < 16) {
    if (lane < a.g.head) cast_elem<D, Q, A>(a, lane, m);
  } else if (lane < 32) {
    const uint64_t t0 = a.g.head + static_cast<uint64_t>(E) * a.g.nunits;  // <= total
    if (lane - 16 < a.g.total - t0) cast_elem<D, Q, A>(a, t0 + (lane - 16), m);
  }
  for (uint64_t u = lane; u < a.g.nunits; u += lanes) cast_unit<D, Q, A>(a, u, m);
}

// Everything lane `lane` of `lanes` does for a field cast to float16 or float32.
template <bool A = false, class M>
DORA_HDI void cast_lane_float(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  if (a.dsize == 2) cast_lane_as<2, false, A>(a, lane, lanes, m);
  else cast_lane_as<4, false, A>(a, lane, lanes, m);
}

// The same for a quantised field: 8- or 16-bit integers.
template <bool A = false, class M>
DORA_HDI void cast_lane_quant(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  if (a.dsize == 1) cast_lane_as<1, true, A>(a, lane, lanes, m);
  else cast_lane_as<2, true, A>(a, lane, lanes, m);
}

// Everything lane `lane` of `lanes` does.
template <class M>
DORA_HDI void cast_lane(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  if (a.dst == kDstFloat) cast_lane_float(a, lane, lanes, m);
  else cast_lane_quant(a, lane, lanes, m);
}

// The same with the affine step (gather_affine_kernel): every converted field of its launch,
// those without a table or a bias included.
template <class M>
DORA_HDI void cast_lane_affine(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  if (a.dst == kDstFloat) cast_lane_float<true>(a, lane, lanes, m);
  else cast_lane_quant<true>(a, lane, lanes, m);
}

}  // namespace cast

namespace multi {

// Arguments of a cast plan's launch (gather_cast_kernel): field k through the cast body where
// c[k].on (g[k] its source view), else as make_args places it (rows or tile by tile_c[k]); each
// field gets the grid its body would have on its own.
DORA_HD Args make_cast_args(const GatherDesc* g, const CastDesc* c, const uint64_t* off,
                            const int* tile_c, int n, uint8_t* dst) {
  return make_args_by(n, dst, nullptr, [&](int k, Field& f) {
    if (!c[k].on) return place_plain(f, g[k], dst + off[k], tile_c[k]);
    f.kind = kRowsCast;
    f.cast = cast::make_args(g[k], c[k], dst + off[k]);
    return static_cast<uint32_t>(cast::grid_for(f.cast));
  });
}

}  // namespace multi

}  // namespace gather
}  // namespace dora
