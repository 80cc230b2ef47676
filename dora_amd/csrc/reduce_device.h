// Device code of the reducing gather (a field of a reduce plan, tensor_plan.cpp): for every element
// of the view of the kept dimensions, the C candidates along the reduced axis are read once as
// their source type, widened to float32 (exact for every source) and the index of their maximum
// is written as uint8, uint16, int32 or int64: the smallest c whose candidate is a NaN, or without
// a NaN the smallest c whose candidate no other exceeds (-0.0 and +0.0 tie).
//
// It is in the style of cast_device.h: every address computation is plain C++ in functions that
// compile for host and device alike, all memory, every conversion and the one cross-lane step go
// through a policy object `M`, and nothing here uses an intrinsic.  The kernel (kernels.hip,
// gather_reduce_kernel) passes a policy of real loads, stores, converts and lane exchanges; the
// host emulation of tests/test_argmax_index_host.py passes one that runs the same functions lane
// by lane, and wave by wave for the cooperative body, with every offset and alignment checked.
//
// The view is gather::Args over the kept dimensions with rows counted in elements, as the cast
// body has it (total output elements, row contiguous elements, head elements before the first
// whole 16-byte unit of the output, nunits whole units, piece the source element size); candidate
// c of the output element at source offset s lies at s + c * cstride.  [lo, hi] covers all C steps.
//
// Lane body (kReduceLane): the output is cut into 16-byte units on absolute 16-byte boundaries
// of the destination, E = 16 / dsize indices each; the up to E - 1 elements before the first and
// after the last whole unit are written one by one, so nothing is written at or past the field's
// end.  A lane owns a unit.  Vector path: the unit's E sources lie in one contiguous run whose
// E * ssize bytes start on a multiple of min(E * ssize, 16) at every step (the axis stride is such
// a multiple too): the lane walks c with E running (value, index) pairs in registers, one image of
// 4 .. 64 bytes loaded per step — (C, H, W) along axis 0, where a wave reads one contiguous span a
// step.  Element path: every other unit takes its E outputs one after the other along the
// odometer, each a walk over c with one running pair and naturally aligned element loads —
// permuted, cut, reversed and broadcast views.  Candidate c replaces the running best iff
// v > best || (isnan(v) && !isnan(best)), so ties keep the first.  Either way one 16-byte store.
//
// Wave body (kReduceWave): for a reduced axis that is the source-contiguous dimension
// (cstride == ssize) and long.  The 64 lanes of a wave share one output element: lane l reduces
// candidates l, l + 64, .. in increasing c with coalesced loads (a lane without a candidate takes
// candidate 0 again), the 64 pairs are combined by a butterfly of six exchanges — (va, ia) beats
// (vb, ib) iff va is better than vb by the rule above, or neither is better and ia < ib — and lane
// 0 writes the element.  Waves take output elements w, w + waves, ..; every element is one store
// of its own, so this body has no units.
#pragma once

#include <cstdint>

#include "cast_device.h"

namespace dora {
namespace gather {
namespace reduce {

constexpr int kWave = 64;

// Whether candidate `v` replaces the running best `b`.
DORA_HDI bool better(float v, float b) { return v > b || (v != v && b == b); }

// DLPack (code, bits) of an index type -> its size in bytes, or 0 when it is none of the four.
DORA_HD unsigned index_size(unsigned code, unsigned bits) {
  if (code == 1) return bits == 8 ? 1 : bits == 16 ? 2 : 0;
  if (code == 0) return bits == 32 ? 4 : bits == 64 ? 8 : 0;
  return 0;
}

// Arguments of the reduction of `g` (the view of the kept dimensions, in source bytes, its reach
// over all C steps) by `r` into `dst`.
DORA_HD Args make_args(const GatherDesc& g, const ReduceDesc& r, uint8_t* dst) {
  Args a{};
  const uint32_t ss = g.elem, ds = r.idx_bits / 8u;
  a.g.src = g.view.src;
  a.g.dst = dst;
  a.g.total = r.count;
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
  a.c = r.c;
  a.cstride = r.cstride;
  const int kind = cast::src_kind(r.src_code, r.src_bits);
  a.src = static_cast<uint32_t>(kind < 0 ? 0 : kind);
  a.dsize = ds;
  return a;
}

// Whether the wave body may run `r` at all, and whether the library chooses it: the reduced axis
// source-contiguous and at least kWaveMinC long (DESIGN §4 has the sweep behind the number).
constexpr uint64_t kWaveMinC = 32;
DORA_HD bool wave_applies(const GatherDesc& g, const ReduceDesc& r) {
  return r.cstride == static_cast<int64_t>(g.elem) && r.c > 1;
}
DORA_HD bool wave_chosen(const GatherDesc& g, const ReduceDesc& r) {
  return wave_applies(g, r) && r.c >= kWaveMinC;
}

DORA_HD uint64_t lane_grid_for(const Args& a) { return gather::grid_for(a.g); }
// a wave an output element, kThreads / kWave waves a workgroup
DORA_HD uint64_t wave_grid_for(const Args& a) {
  constexpr uint64_t per = kThreads / kWave;
  const uint64_t g = (a.g.total + per - 1) / per;
  return g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g;
}

// The index type a body counts in: 64 bits only where the destination has them.
template <int D>
struct IdxOf {
  using type = uint32_t;
};
template <>
struct IdxOf<8> {
  using type = uint64_t;
};

// 16-byte words of a unit's source image of N bytes.
template <int N>
constexpr int kWords = N <= 16 ? 1 : N / 16;

// The N contiguous bytes at `s`: one load of 4, 8 or 16 bytes, or two or four of 16.
template <int N, class M>
DORA_HDI void load_image(int64_t s, M& m, U16* v) {
  if constexpr (N <= 16) {
    v[0] = m.template load_vec<N>(s);
  } else {
#pragma unroll
    for (int k = 0; k < N / 16; ++k) v[k] = m.template load_vec<16>(s + 16 * k);
  }
}

// Index `i` into slot `j` of a unit of D-byte indices.
template <int D, class I>
DORA_HDI void put_index(U16& out, int j, I i) {
  if constexpr (D == 1) out.w[j / 4] |= (static_cast<uint32_t>(i) & 0xffu) << (8 * (j % 4));
  else if constexpr (D == 2) out.w[j / 2] |= (static_cast<uint32_t>(i) & 0xffffu) << (16 * (j % 2));
  else if constexpr (D == 4) out.w[j] = static_cast<uint32_t>(i);
  else {
    out.w[2 * j] = static_cast<uint32_t>(i);
    out.w[2 * j + 1] = static_cast<uint32_t>(static_cast<uint64_t>(i) >> 32);
  }
}

// Where the lane body's unit (or single element) starting at output element `e` reads: the row
// position of `e`, its element in the row and the source offset of its candidate 0.
struct Start {
  RowPos p;
  uint64_t b;
  int64_t s;
};
DORA_HDI void start_of(const Args& a, uint64_t e, Start& st) {
  uint64_t r;
  out_pos(a.g, e, &r, &st.b);
  row_pos(a.g, r, st.p);
  st.s = st.p.off + static_cast<int64_t>(st.b * a.g.piece);
}

// Whether the unit of E outputs at `st` takes the vector path: its sources one contiguous run
// of n = E * ssize >= 4 bytes that starts on a multiple of min(n, 16) at every step.
template <int D>
DORA_HDI bool unit_is_vector(const Args& a, const Start& st) {
  constexpr uint32_t E = 16 / D;
  const uint32_t n = E * a.g.piece, align = n > 16 ? 16 : n;
  if (n < 4 || st.b + E > a.g.row) return false;
  const uint64_t at = reinterpret_cast<uintptr_t>(a.g.src) + static_cast<uint64_t>(st.s);
  return ((at | static_cast<uint64_t>(a.cstride)) & (align - 1)) == 0;
}

// The vector path: E running pairs over one image a step.
template <uint32_t K, int D, class M>
DORA_HDI U16 unit_vec(const Args& a, int64_t s, M& m) {
  constexpr int E = 16 / D, S = cast::kSize<K>, N = E * S;
  using I = typename IdxOf<D>::type;
  static_assert(N >= 4, "an image is at least one dword");
  float bv[E];
  I bi[E];
  U16 img[kWords<N>];
  load_image<N>(s, m, img);
#pragma unroll
  for (int j = 0; j < E; ++j) {
    bv[j] = m.template to_f32<K>(cast::elem_of<S>(img, j));
    bi[j] = 0;
  }
  for (uint64_t c = 1; c < a.c; ++c) {
    s += a.cstride;
    load_image<N>(s, m, img);
#pragma unroll
    for (int j = 0; j < E; ++j) {
      const float v = m.template to_f32<K>(cast::elem_of<S>(img, j));
      if (better(v, bv[j])) {
        bv[j] = v;
        bi[j] = static_cast<I>(c);
      }
    }
  }
  U16 out = {{0, 0, 0, 0}};
#pragma unroll
  for (int j = 0; j < E; ++j) put_index<D>(out, j, bi[j]);
  return out;
}

// One output element on its own: the walk over c with one running pair, element loads.
template <uint32_t K, class I, class M>
DORA_HDI I reduce_one(const Args& a, int64_t s, M& m) {
  constexpr int S = cast::kSize<K>;
  float bv = m.template to_f32<K>(m.template load_elem<S>(s));
  I bi = 0;
  for (uint64_t c = 1; c < a.c; ++c) {
    s += a.cstride;
    const float v = m.template to_f32<K>(m.template load_elem<S>(s));
    if (better(v, bv)) {
      bv = v;
      bi = static_cast<I>(c);
    }
  }
  return bi;
}

// Whole unit `u` of the output, its sources of type K.
template <uint32_t K, int D, class M>
DORA_HDI void reduce_unit(const Args& a, uint64_t u, M& m) {
  constexpr int E = 16 / D;
  using I = typename IdxOf<D>::type;
  const uint64_t e = a.g.head + static_cast<uint64_t>(E) * u;
  Start st;
  start_of(a, e, st);
  if constexpr (E * cast::kSize<K> >= 4) {
    if (unit_is_vector<D>(a, st)) {
      m.store16(e * D, unit_vec<K, D>(a, st.s, m));
      return;
    }
  }
  U16 out = {{0, 0, 0, 0}};
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int64_t s = st.p.off + static_cast<int64_t>(st.b * a.g.piece);
    put_index<D>(out, j, reduce_one<K, I>(a, s, m));
    if (++st.b >= a.g.row) {
      st.b = 0;
      next_row(a.g, st.p);
    }
  }
  m.store16(e * D, out);
}

// Output element `e` on its own (before the first and after the last whole unit).
template <uint32_t K, int D, class M>
DORA_HDI void reduce_elem(const Args& a, uint64_t e, M& m) {
  using I = typename IdxOf<D>::type;
  Start st;
  start_of(a, e, st);
  m.template store_index<D>(e, static_cast<uint64_t>(reduce_one<K, I>(a, st.s, m)));
}

// cast_lane_as' division of the work: lanes 0..15 a head element each, lanes 16..31 a tail
// element each (at most E - 1 <= 15 of either), and every lane the whole units lane,
// lane + lanes, ..
template <uint32_t K, int D, class M>
DORA_HDI void lane_as(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  constexpr int E = 16 / D;
  static_assert(E - 1 <= 15, "16 lanes each for the head's and the tail's elements");
  if (lane < 16) {
    if (lane < a.g.head) reduce_elem<K, D>(a, lane, m);
  } else if (lane < 32) {
    const uint64_t t0 = a.g.head + static_cast<uint64_t>(E) * a.g.nunits;  // <= total
    if (lane - 16 < a.g.total - t0) reduce_elem<K, D>(a, t0 + (lane - 16), m);
  }
  for (uint64_t u = lane; u < a.g.nunits; u += lanes) reduce_unit<K, D>(a, u, m);
}

template <uint32_t K, class M>
DORA_HDI void lane_of(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  switch (a.dsize) {
    case 1: lane_as<K, 1>(a, lane, lanes, m); break;
    case 2: lane_as<K, 2>(a, lane, lanes, m); break;
    case 4: lane_as<K, 4>(a, lane, lanes, m); break;
    default: lane_as<K, 8>(a, lane, lanes, m); break;
  }
}

// Everything lane `lane` of `lanes` does for a field of the lane body.
template <class M>
DORA_HDI void reduce_lane(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  switch (a.src) {
    case cast::kU8: lane_of<cast::kU8>(a, lane, lanes, m); break;
    case cast::kI8: lane_of<cast::kI8>(a, lane, lanes, m); break;
    case cast::kU16: lane_of<cast::kU16>(a, lane, lanes, m); break;
    case cast::kI16: lane_of<cast::kI16>(a, lane, lanes, m); break;
    case cast::kF16: lane_of<cast::kF16>(a, lane, lanes, m); break;
    case cast::kBF16: lane_of<cast::kBF16>(a, lane, lanes, m); break;
    default: lane_of<cast::kF32>(a, lane, lanes, m); break;
  }
}

// ------------------------------------------------------------------------------------------
// The wave body
// ------------------------------------------------------------------------------------------

// A lane's running best.
struct Pair {
  float v;
  uint64_t i;
};

// Whether `o` takes the place of `p` when two lanes' pairs meet.
DORA_HDI bool beats(const Pair& o, const Pair& p) {
  return better(o.v, p.v) || (!better(p.v, o.v) && o.i < p.i);
}

// The source offset of candidate 0 of output element `e`.
DORA_HDI int64_t source_of(const Args& a, uint64_t e) {
  Start st;
  start_of(a, e, st);
  return st.s;
}

// Lane `l`'s own candidates l, l + 64, .. of the output element at `s`, in increasing c; a lane
// past the last candidate takes candidate 0, which loses every tie it is not the answer of.
template <uint32_t K, class M>
DORA_HDI Pair wave_partial_as(const Args& a, int64_t s, uint32_t l, M& m) {
  constexpr int S = cast::kSize<K>;
  uint64_t c = l < a.c ? l : 0;
  Pair p;
  p.v = m.template to_f32<K>(m.template load_stream<S>(s + static_cast<int64_t>(c) * S));
  p.i = c;
  for (c += kWave; c < a.c; c += kWave) {
    const float v = m.template to_f32<K>(m.template load_stream<S>(s + static_cast<int64_t>(c) * S));
    if (better(v, p.v)) {
      p.v = v;
      p.i = c;
    }
  }
  return p;
}

template <class M>
DORA_HDI Pair wave_partial(const Args& a, int64_t s, uint32_t l, M& m) {
  switch (a.src) {
    case cast::kU8: return wave_partial_as<cast::kU8>(a, s, l, m);
    case cast::kI8: return wave_partial_as<cast::kI8>(a, s, l, m);
    case cast::kU16: return wave_partial_as<cast::kU16>(a, s, l, m);
    case cast::kI16: return wave_partial_as<cast::kI16>(a, s, l, m);
    case cast::kF16: return wave_partial_as<cast::kF16>(a, s, l, m);
    case cast::kBF16: return wave_partial_as<cast::kBF16>(a, s, l, m);
    default: return wave_partial_as<cast::kF32>(a, s, l, m);
  }
}

// One exchange of the butterfly: the pair of lane l ^ d meets this lane's.  After the steps
// d = 32, 16, .., 1 every lane holds the wave's answer.
template <class M>
DORA_HDI void wave_step(Pair& p, int d, M& m) {
  const Pair o = m.lane_xor(p, d);
  if (beats(o, p)) p = o;
}

// Lane 0 writes the element.
template <class M>
DORA_HDI void wave_store(const Args& a, uint64_t e, uint32_t l, const Pair& p, M& m) {
  if (l != 0) return;
  switch (a.dsize) {
    case 1: m.template store_index<1>(e, p.i); break;
    case 2: m.template store_index<2>(e, p.i); break;
    case 4: m.template store_index<4>(e, p.i); break;
    default: m.template store_index<8>(e, p.i); break;
  }
}

// Everything lane `lane` of `lanes` (both whole numbers of waves) does for a field of the wave
// body: its wave's output elements, every step uniform over the wave.
template <class M>
DORA_HDI void reduce_wave(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  const uint32_t l = static_cast<uint32_t>(lane % kWave);
  const uint64_t waves = lanes / kWave;
  for (uint64_t e = lane / kWave; e < a.g.total; e += waves) {
    Pair p = wave_partial(a, source_of(a, e), l, m);
#pragma unroll
    for (int d = kWave / 2; d; d >>= 1) wave_step(p, d, m);
    wave_store(a, e, l, p, m);
  }
}

}  // namespace reduce

namespace multi {

// Arguments of a reduce plan's launch (gather_reduce_kernel): field k through a reduce body
// where r[k].on (g[k] the view of its kept dimensions; the wave body where wave[k]), else as
// make_args places it (rows or tile by tile_c[k]); each field gets the grid its body asks for.
DORA_HD Args make_reduce_args(const GatherDesc* g, const ReduceDesc* r, const bool* wave,
                              const uint64_t* off, const int* tile_c, int n, uint8_t* dst) {
  return make_args_by(n, dst, nullptr, [&](int k, Field& f) {
    if (!r[k].on) return place_plain(f, g[k], dst + off[k], tile_c[k]);
    f.kind = wave[k] ? kReduceWave : kReduceLane;
    f.reduce = reduce::make_args(g[k], r[k], dst + off[k]);
    return static_cast<uint32_t>(wave[k] ? reduce::wave_grid_for(f.reduce)
                                         : reduce::lane_grid_for(f.reduce));
  });
}

}  // namespace multi

}  // namespace gather
}  // namespace dora
