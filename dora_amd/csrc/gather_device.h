// Device code of the strided gather (a device tensor view that is not dense, tensor_plan.cpp):
// the row-major bytes of the view written into a sample, read once and written once.
//
// Everything that computes an address — output unit -> (row, byte in row), the odometer -> source
// offset, which load reaches which bytes, which store writes which — is plain C++ in functions that
// compile for host and device alike, and all memory goes through a policy object `M`.  The kernel
// (kernels.hip) passes a policy of real loads and stores; the host emulation of
// tests/test_gather_index_host.py passes one that runs the same functions lane by lane over the
// whole grid with every offset checked.  Nothing here uses an intrinsic.
//
// Addressing is 64-bit throughout.  The output is cut into 16-byte units on absolute 16-byte
// boundaries of the destination; the up to 15 bytes before the first and after the last whole
// unit are written one by one, so nothing is ever written at or past dst + total.
#pragma once

#include <cstdint>

#include "plan.h"

// DORA_HD: a function of this header, for host and device.  DORA_HDI: one that is always inlined
// into its caller on the device (cast_device.h's body: a call there would pass the kernel's
// by-value arguments by address, which copies them into scratch).
#if defined(__HIPCC__)
#define DORA_HD __host__ __device__ inline
#define DORA_HDI __host__ __device__ inline __attribute__((always_inline))
#else
#define DORA_HD inline
#define DORA_HDI inline
#endif

namespace dora {
namespace gather {

constexpr int kDims = kMaxTensorDims;
constexpr int kThreads = 256;
// Workgroups at most: 32 per CU of an MI355X, every lane then walks its units a grid apart.
constexpr uint64_t kMaxGrid = 8192;

struct U16 {
  uint32_t w[4];
};

// Kernel arguments (by value).  The view's dimensions are right-aligned in shape[] / stride[]
// and padded on the left with extent 1, so every walk is over kDims dimensions.
struct Args {
  const uint8_t* src;  // element (0, .., 0)
  uint8_t* dst;
  uint64_t total;   // output bytes
  uint64_t row;     // contiguous source bytes per row (a multiple of `piece`)
  uint64_t head;    // output bytes before the first whole unit (< 16, <= total)
  uint64_t nunits;  // whole units: output bytes [head + 16 u, +16), u < nunits
  int64_t lo, hi;   // closed interval of offsets from `src` that may be read
  uint32_t piece;   // bytes per load where a unit is put together from several rows: the element
                    // size when units start on an element, else 1
  uint32_t pad;
  int64_t shape[kDims];
  int64_t stride[kDims];
};

// Arguments of the gather of `g` into `dst`.
DORA_HD Args make_args(const GatherDesc& g, uint8_t* dst) {
  Args a{};
  a.src = g.view.src;
  a.dst = dst;
  a.total = g.view.total;
  a.row = g.view.row;
  const uint64_t mis = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
  a.head = mis < a.total ? mis : a.total;
  a.nunits = (a.total - a.head) / 16;
  a.lo = g.lo;
  a.hi = g.hi;
  a.piece = (g.elem && a.head % g.elem == 0 && a.row % g.elem == 0) ? g.elem : 1;
  a.pad = 0;
  for (int k = 0; k < kDims; ++k) {
    const int i = k - (kDims - g.view.nd);
    a.shape[k] = i >= 0 ? g.view.shape[i] : 1;
    a.stride[k] = i >= 0 ? g.view.stride[i] : 0;
  }
  return a;
}

DORA_HD uint64_t grid_for(const Args& a) {
  const uint64_t g = (a.nunits + kThreads - 1) / kThreads;
  return g < 1 ? 1 : g > kMaxGrid ? kMaxGrid : g;
}

// A row of the view: its index in every dimension and the offset of its first byte from `src`.
struct RowPos {
  int64_t off;
  int64_t idx[kDims];
};

// Row `r` (row-major over shape[]) -> RowPos.  Every partial sum of idx * stride lies inside
// [lo, hi], which the plan computed without overflow.
DORA_HD void row_pos(const Args& a, uint64_t r, RowPos& p) {
  p.off = 0;
#pragma unroll
  for (int k = kDims - 1; k >= 0; --k) {
    const uint64_t n = static_cast<uint64_t>(a.shape[k]);
    uint64_t i = 0;
    if (n != 1) {
      if ((r | n) >> 32) {
        i = r % n;
        r = r / n;
      } else {  // the common case: a 32-bit division
        const uint32_t r32 = static_cast<uint32_t>(r), n32 = static_cast<uint32_t>(n);
        i = r32 % n32;
        r = r32 / n32;
      }
    }
    p.idx[k] = static_cast<int64_t>(i);
    p.off += static_cast<int64_t>(i) * a.stride[k];
  }
}

// The odometer: RowPos of the next row (the row after the last one is row 0).
DORA_HD void next_row(const Args& a, RowPos& p) {
  bool carry = true;
#pragma unroll
  for (int k = kDims - 1; k >= 0; --k) {
    if (!carry) continue;
    if (p.idx[k] + 1 < a.shape[k]) {
      ++p.idx[k];
      p.off += a.stride[k];
      carry = false;
    } else {
      p.off -= p.idx[k] * a.stride[k];
      p.idx[k] = 0;
    }
  }
}

// Output byte `o` -> its row and byte in the row.
DORA_HD void out_pos(const Args& a, uint64_t o, uint64_t* r, uint64_t* b) {
  if ((o | a.row) >> 32) {
    *r = o / a.row;
  } else {
    *r = static_cast<uint32_t>(o) / static_cast<uint32_t>(a.row);
  }
  *b = o - *r * a.row;
}

// 16 output bytes put together from loads of G bytes (G divides the row and the unit's offset in
// its row, so no load straddles two rows), walking the odometer as rows end.
template <int G, class M>
DORA_HD U16 gather_pieces(const Args& a, RowPos& p, uint64_t b, M& m) {
  U16 v = {{0, 0, 0, 0}};
#pragma unroll
  for (int j = 0; j < 16 / G; ++j) {
    const uint64_t x = m.template load_piece<G>(p.off + static_cast<int64_t>(b));
    constexpr int kPerWord = G >= 4 ? 1 : 4 / G;
    if constexpr (G == 8) {
      v.w[2 * j] = static_cast<uint32_t>(x);
      v.w[2 * j + 1] = static_cast<uint32_t>(x >> 32);
    } else {
      v.w[j / kPerWord] |= static_cast<uint32_t>(x) << (8 * G * (j % kPerWord));
    }
    b += G;
    if (b >= a.row) {
      b = 0;
      next_row(a, p);
    }
  }
  return v;
}

// Whole unit `u` of the output.  A unit inside one row is one 16-byte load when the source
// address is a whole number of dwords, else two aligned 16-byte loads funnel-shifted — where
// both lie inside [lo, hi]; every other unit is put together piece by piece.
template <class M>
DORA_HD void gather_unit(const Args& a, uint64_t u, M& m) {
  const uint64_t o = a.head + 16 * u;
  uint64_t r, b;
  out_pos(a, o, &r, &b);
  RowPos p;
  row_pos(a, r, p);
  if (b + 16 <= a.row) {
    const int64_t s = p.off + static_cast<int64_t>(b);
    const uint32_t mis = static_cast<uint32_t>(
        (reinterpret_cast<uintptr_t>(a.src) + static_cast<uint64_t>(s)) & 15);
    if ((mis & 3) == 0) {
      m.store16(o, m.load16(s));
      return;
    }
    // (hi - 31 cannot overflow: hi >= row - 1 >= 15 here)
    if (s - a.lo >= static_cast<int64_t>(mis) && s - static_cast<int64_t>(mis) <= a.hi - 31) {
      const int64_t w = s - static_cast<int64_t>(mis);
      m.store16(o, m.funnel(m.load16(w), m.load16(w + 16), mis));
      return;
    }
  }
  U16 v;
  switch (a.piece) {
    case 8: v = gather_pieces<8>(a, p, b, m); break;
    case 4: v = gather_pieces<4>(a, p, b, m); break;
    case 2: v = gather_pieces<2>(a, p, b, m); break;
    default: v = gather_pieces<1>(a, p, b, m); break;
  }
  m.store16(o, v);
}

// Output byte `o` on its own (the bytes before the first and after the last whole unit).
template <class M>
DORA_HD void gather_byte(const Args& a, uint64_t o, M& m) {
  uint64_t r, b;
  out_pos(a, o, &r, &b);
  RowPos p;
  row_pos(a, r, p);
  m.store1(o, static_cast<uint8_t>(m.template load_piece<1>(p.off + static_cast<int64_t>(b))));
}

// Everything lane `lane` of `lanes` does: lanes 0..15 a head byte each, lanes 16..31 a tail
// byte each, and every lane the whole units lane, lane + lanes, ..
template <class M>
DORA_HD void gather_lane(const Args& a, uint64_t lane, uint64_t lanes, M& m) {
  if (lane < 16) {
    if (lane < a.head) gather_byte(a, lane, m);
  } else if (lane < 32) {
    const uint64_t t0 = a.head + 16 * a.nunits;  // <= total
    if (lane - 16 < a.total - t0) gather_byte(a, t0 + (lane - 16), m);
  }
  for (uint64_t u = lane; u < a.nunits; u += lanes) gather_unit(a, u, m);
}


// ------------------------------------------------------------------------------------------
// The tiled transpose (gather_tile_kernel): for a view whose source-contiguous dimension `c`
// (byte stride == element size) is not the output's innermost one `j` (the last canonical
// dimension; row == elem).  One workgroup moves a kT x kT tile of the (c, j) plane through LDS:
// it loads along c (coalesced in the source), stores along j (coalesced in the output); the other
// dimensions are an outer odometer over tiles.  Every address — tile -> origin, (thread, step)
// -> source offset / LDS index / output element, and the partial-tile predicates — is computed
// here, in host/device code the emulation runs thread by thread, phase by phase.
// ------------------------------------------------------------------------------------------
namespace tile {

constexpr int kT = 32;           // tile edge in elements
constexpr int kPitch = kT + 1;   // LDS row pitch in elements: a column read hits kT different banks
constexpr int kLds = kT * kPitch;
constexpr int kSteps = kT * kT / kThreads;  // elements per thread and phase
constexpr uint64_t kMaxGrid = 1u << 20;

struct Args {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t total;
  int64_t lo, hi;
  uint32_t elem;
  uint32_t c;               // the source-contiguous dimension (right-aligned index; j = kDims - 1)
  uint64_t ntc, ntj, ntiles;  // tiles along c, along j, in all
  int64_t shape[kDims];
  int64_t stride[kDims];    // bytes
  uint64_t ostride[kDims];  // elements of the row-major output per step of each dimension
};

// The source-contiguous dimension of `g` the tile kernel would transpose against (index into
// g.view), or -1 when the kernel does not apply: the innermost dimension is itself contiguous,
// or source, strides or destination are not element-aligned.
DORA_HD int contiguous_dim(const GatherDesc& g, const uint8_t* dst) {
  const uint64_t e = g.elem;
  if (g.view.nd < 2 || g.view.row != e || (e != 1 && e != 2 && e != 4 && e != 8)) return -1;
  if ((reinterpret_cast<uintptr_t>(g.view.src) | reinterpret_cast<uintptr_t>(dst)) & (e - 1)) return -1;
  int c = -1;
  for (int k = 0; k < g.view.nd; ++k) {
    if (g.view.stride[k] & static_cast<int64_t>(e - 1)) return -1;
    if (k < g.view.nd - 1 && g.view.stride[k] == static_cast<int64_t>(e)) c = k;
  }
  return c;
}

DORA_HD Args make_args(const GatherDesc& g, uint8_t* dst, int c) {
  Args a{};
  a.src = g.view.src;
  a.dst = dst;
  a.total = g.view.total;
  a.lo = g.lo;
  a.hi = g.hi;
  a.elem = g.elem;
  const int shift = kDims - g.view.nd;
  a.c = static_cast<uint32_t>(c + shift);
  for (int k = 0; k < kDims; ++k) {
    const int i = k - shift;
    a.shape[k] = i >= 0 ? g.view.shape[i] : 1;
    a.stride[k] = i >= 0 ? g.view.stride[i] : 0;
  }
  a.ostride[kDims - 1] = 1;
  for (int k = kDims - 2; k >= 0; --k)
    a.ostride[k] = a.ostride[k + 1] * static_cast<uint64_t>(a.shape[k + 1]);
  a.ntc = (static_cast<uint64_t>(a.shape[a.c]) + kT - 1) / kT;
  a.ntj = (static_cast<uint64_t>(a.shape[kDims - 1]) + kT - 1) / kT;
  uint64_t outer = 1;
  for (int k = 0; k < kDims - 1; ++k)
    if (static_cast<uint32_t>(k) != a.c) outer *= static_cast<uint64_t>(a.shape[k]);
  a.ntiles = outer * a.ntc * a.ntj;  // <= the element count, which fits 64 bits
  return a;
}

DORA_HD uint64_t grid_for(const Args& a) { return a.ntiles < kMaxGrid ? a.ntiles : kMaxGrid; }

// Where tile `t` starts: first element along c and j, and the outer dimensions' share of the
// source offset (bytes) and of the output position (elements).
struct Origin {
  int64_t src_off;
  uint64_t out_elem;
  uint64_t c0, j0;
};

DORA_HD Origin origin(const Args& a, uint64_t t) {
  Origin o;
  o.j0 = (t % a.ntj) * kT;
  t /= a.ntj;
  o.c0 = (t % a.ntc) * kT;
  t /= a.ntc;
  o.src_off = 0;
  o.out_elem = 0;
#pragma unroll
  for (int k = kDims - 2; k >= 0; --k) {
    if (static_cast<uint32_t>(k) == a.c) continue;
    const uint64_t n = static_cast<uint64_t>(a.shape[k]);
    if (n == 1) continue;
    const uint64_t i = t % n;
    t /= n;
    o.src_off += static_cast<int64_t>(i) * a.stride[k];
    o.out_elem += i * a.ostride[k];
  }
  return o;
}

// One element a thread moves in one step of a phase; `on` false outside a partial tile.
struct Slot {
  bool on;
  int64_t src_off;    // load phase: bytes from src
  uint32_t lds;       // element index into the tile
  uint64_t out_elem;  // store phase: element of the output
};

// Load phase: consecutive threads walk c (contiguous in the source); tile[lj][lc].
DORA_HD Slot load_slot(const Args& a, const Origin& o, uint32_t thread, int step) {
  const uint32_t lc = thread % kT, lj = thread / kT + static_cast<uint32_t>(step) * (kThreads / kT);
  Slot s{};
  s.on = o.c0 + lc < static_cast<uint64_t>(a.shape[a.c]) &&
         o.j0 + lj < static_cast<uint64_t>(a.shape[kDims - 1]);
  if (!s.on) return s;
  s.src_off = o.src_off + static_cast<int64_t>(o.c0 + lc) * a.stride[a.c] +
              static_cast<int64_t>(o.j0 + lj) * a.stride[kDims - 1];
  s.lds = lj * kPitch + lc;
  return s;
}

// Store phase: consecutive threads walk j (contiguous in the output); reads tile[oj][oc].
DORA_HD Slot store_slot(const Args& a, const Origin& o, uint32_t thread, int step) {
  const uint32_t oj = thread % kT, oc = thread / kT + static_cast<uint32_t>(step) * (kThreads / kT);
  Slot s{};
  s.on = o.c0 + oc < static_cast<uint64_t>(a.shape[a.c]) &&
         o.j0 + oj < static_cast<uint64_t>(a.shape[kDims - 1]);
  if (!s.on) return s;
  s.lds = oj * kPitch + oc;
  s.out_elem = o.out_elem + (o.c0 + oc) * a.ostride[a.c] + (o.j0 + oj);
  return s;
}

template <class M>
DORA_HD void load_phase(const Args& a, const Origin& o, uint32_t thread, M& m) {
#pragma unroll
  for (int step = 0; step < kSteps; ++step) {
    const Slot s = load_slot(a, o, thread, step);
    if (s.on) m.lds_write(s.lds, m.load_elem(s.src_off));
  }
}

template <class M>
DORA_HD void store_phase(const Args& a, const Origin& o, uint32_t thread, M& m) {
#pragma unroll
  for (int step = 0; step < kSteps; ++step) {
    const Slot s = store_slot(a, o, thread, step);
    if (s.on) m.store_elem(s.out_elem, m.lds_read(s.lds));
  }
}

}  // namespace tile

// ------------------------------------------------------------------------------------------
// Several views in one launch (gather_struct_kernel): the fields of a struct-of-tensors plan,
// each written to its own byte range of one sample.  Every field keeps the arguments and the body
// it would have on its own (rows: gather_lane over the field's lanes; tile: the tile loop over
// the field's workgroups); the launch's workgroups are dealt to the fields in order, each field
// getting the grid its own kernel would have used, and a workgroup finds its field by scanning
// the table of first workgroups.  A field's writes stay inside [dst, dst + total) of its own
// arguments — the head / tail bytes and the tile predicates see to that — so the padding between
// fields and the neighbours' bytes are never touched.  The fields of a take (take:: below) are a
// third kind, all of a launch or none: the rows body reading row index[i] for row i, with the
// rows body's grid.
// ------------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------------
// The offsets of a ragged batch whose partition lives in HBM (one more share of
// gather_struct_kernel): one workgroup scans `count` words of 4 or 8 bytes into the sample's
// int32 offsets, all `count + 1 - offsets` of them.  Lengths: o[0] = 0 and o[i + 1] = min(n,
// sum_{j <= i} max(len_j, 0)), an inclusive sum written one word on.  Offsets: o[i] = min(n, max(0,
// max_{j <= i} in_j)), an inclusive maximum written in place.  Either way every input is clamped
// to [0, n] first and the running value saturates at n, so the words are monotone, inside [0, n]
// and no sum leaves 64 bits whatever the input holds.
//
// The scan goes in tiles of kTile words with a carried total: each thread reads its kItems
// consecutive words and scans them in registers (load_phase), the kThreads thread totals are
// scanned through two LDS rows by doubling (step_phase, kSteps of them, a barrier after each), and
// each thread combines carry, the totals before it and its own prefix into its output words
// (store_phase, which also returns the next carry: the same in every thread).  Tile -> word
// range, thread -> words, the LDS slots, the carry and the clamps are all here.
// ------------------------------------------------------------------------------------------
namespace scan {

constexpr int kItems = 4;                   // words per thread and tile
constexpr int kTile = kThreads * kItems;    // words per tile
constexpr int kSteps = 8;                   // log2(kThreads)
constexpr int kLds = 2 * kThreads;          // two rows of thread totals (8-byte words)
static_assert((1 << kSteps) == kThreads, "the doubling scan covers the workgroup");

struct Args {
  const uint8_t* src;  // the partition's words (null: no scan share in this launch)
  uint8_t* dst;        // the sample's offsets buffer
  uint64_t count;      // input words
  uint64_t n;          // the clamp: rows of the values
  uint32_t wide;       // 0: int32 words, 1: int64
  uint32_t offsets;    // 0: lengths (sum), 1: offsets (maximum)
};

DORA_HD Args make_args(const ScanDesc& s, uint8_t* dst) {
  Args a{};
  a.src = s.src;
  a.dst = dst;
  a.count = s.count;
  a.n = s.n;
  a.wide = s.wide;
  a.offsets = s.offsets;
  return a;
}

DORA_HD uint64_t tiles(const Args& a) { return (a.count + kTile - 1) / kTile; }
// output words in all
DORA_HD uint64_t out_words(const Args& a) { return a.count + (a.offsets ? 0 : 1); }

DORA_HD uint64_t clamp_in(const Args& a, int64_t v) {
  return v <= 0 ? 0 : static_cast<uint64_t>(v) > a.n ? a.n : static_cast<uint64_t>(v);
}
// the operator over clamped values, saturating at n (both operands <= n: no overflow)
DORA_HD uint64_t combine(const Args& a, uint64_t x, uint64_t y) {
  if (a.offsets) return x > y ? x : y;
  const uint64_t s = x + y;
  return s > a.n ? a.n : s;
}

// A thread's own words of a tile, scanned: pre[k] the inclusive prefix of its first k + 1 words.
struct Local {
  uint64_t pre[kItems];
};

// o[0] of the lengths form, which no input word produces.
template <class M>
DORA_HD void head(const Args& a, uint32_t thread, M& m) {
  if (thread == 0 && !a.offsets) m.store_word(0, 0);
}

template <class M>
DORA_HD void load_phase(const Args& a, uint64_t tile, uint32_t thread, Local& loc, M& m) {
  const uint64_t first = tile * kTile + static_cast<uint64_t>(thread) * kItems;
  uint64_t run = 0;  // the identity of both operators over [0, n]
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const uint64_t i = first + static_cast<uint64_t>(k);
    if (i < a.count) run = combine(a, run, clamp_in(a, m.load_word(i)));
    loc.pre[k] = run;
  }
  m.lds_write(thread, run);
}

// Step `step` of the doubling scan over the thread totals: row (step & 1) -> the other row.
template <class M>
DORA_HD void step_phase(const Args& a, uint32_t thread, int step, M& m) {
  const uint32_t from = static_cast<uint32_t>(step & 1) * kThreads, to = kThreads - from;
  const uint32_t d = 1u << step;
  uint64_t v = m.lds_read(from + thread);
  if (thread >= d) v = combine(a, m.lds_read(from + thread - d), v);
  m.lds_write(to + thread, v);
}

// After kSteps steps (an even number) the inclusive totals are back in row 0.  Writes the
// thread's words of the tile; returns the carry into the next tile.
template <class M>
DORA_HD uint64_t store_phase(const Args& a, uint64_t tile, uint32_t thread, const Local& loc,
                             uint64_t carry, M& m) {
  static_assert(kSteps % 2 == 0, "the totals end in row 0");
  const uint64_t before = thread ? combine(a, carry, m.lds_read(thread - 1)) : carry;
  const uint64_t first = tile * kTile + static_cast<uint64_t>(thread) * kItems;
  const uint64_t shift = a.offsets ? 0 : 1;
#pragma unroll
  for (int k = 0; k < kItems; ++k) {
    const uint64_t i = first + static_cast<uint64_t>(k);
    if (i < a.count) m.store_word(i + shift, static_cast<uint32_t>(combine(a, before, loc.pre[k])));
  }
  return combine(a, carry, m.lds_read(kThreads - 1));
}

}  // namespace scan

// ------------------------------------------------------------------------------------------
// Rows taken by an index (one more field kind of gather_struct_kernel): the output's row i0 of
// dimension 0 is the source's row index[i0], so the message is `values[index]` without the
// indexed copy.  It is the rows body with one level of indirection: the field's Args describe
// dimensions 1.. of the view (shape[] / stride[], `inner` rows of `row` bytes per taken row),
// and the dimension-0 term of a row's source offset is index[i0] * stride0 instead of
// i0 * stride0, in take_pos and in the odometer step alike.
//
// A word is valid when 0 <= word < N, compared as a signed 64-bit value before anything is
// multiplied (an int64 word whose low half alone would pass does not).  A row whose word is not
// valid is `missing`: every unit or byte of it is zero and nothing is loaded for it — in all
// three unit paths, the piece-by-piece one included, where one unit may span several taken rows
// of which some are missing.  [lo, hi] was computed over all N source rows, so a valid word cannot
// leave it whatever the index holds.  Index words go through the policy's load_index(i), i < K
// always: neighbouring units read the same words again, so these are plain cached loads.
// ------------------------------------------------------------------------------------------
namespace take {

// The index of a launch, shared by its fields.
struct Index {
  const uint8_t* src;  // K words
  uint64_t k;          // rows taken: the output's leading extent
  uint64_t n;          // rows of the source: valid words are [0, n)
  uint32_t wide;       // 0: int32 words, 1: int64
  uint32_t pad;
};

struct Args {
  gather::Args g;    // dimensions 1.. of the view; total = K * inner * row, [lo, hi] over N rows
  int64_t stride0;   // bytes per step of dimension 0 (signed, 0 allowed)
  uint64_t inner;    // rows of g.row bytes per taken row
};

// `g` holds dimensions 1.. of the field (total already K rows' worth), `stride0` dimension 0.
DORA_HD Args make_args(const GatherDesc& g, int64_t stride0, uint8_t* dst) {
  Args a{};
  a.g = gather::make_args(g, dst);
  a.stride0 = stride0;
  a.inner = 1;
  for (int i = 0; i < g.view.nd; ++i) a.inner *= static_cast<uint64_t>(g.view.shape[i]);
  return a;
}

// A row of a taken field: the taken row it belongs to, its place inside that row, and — unless
// the taken row's word is not valid — where the taken row starts in the source.
struct Pos {
  RowPos p;       // over dimensions 1..: p.off is the offset inside the taken row
  uint64_t i0;    // the taken row
  uint64_t in;    // the row inside it, < inner
  int64_t base;   // index[i0] * stride0
  bool missing;
};

// The word of taken row `i0` -> base / missing.  i0 == K (the row after the last) reads nothing.
template <class M>
DORA_HD void take_row(const Args& a, const Index& ix, uint64_t i0, Pos& t, M& m) {
  t.i0 = i0;
  t.base = 0;
  t.missing = true;
  if (i0 >= ix.k) return;
  const int64_t w = m.load_index(i0);
  if (w < 0 || w >= static_cast<int64_t>(ix.n)) return;
  t.missing = false;
  t.base = w * a.stride0;
}

// Row `r` of the output (row-major over K and shape[]) -> Pos.
template <class M>
DORA_HD void take_pos(const Args& a, const Index& ix, uint64_t r, Pos& t, M& m) {
  uint64_t i0 = r;
  t.in = 0;
  if (a.inner != 1) {
    if ((r | a.inner) >> 32) {
      i0 = r / a.inner;
    } else {
      i0 = static_cast<uint32_t>(r) / static_cast<uint32_t>(a.inner);
    }
    t.in = r - i0 * a.inner;
  }
  row_pos(a.g, t.in, t.p);
  take_row(a, ix, i0, t, m);
}

// The odometer: the next row; past the last row of a taken row, the next taken row's word.
template <class M>
DORA_HD void next_taken(const Args& a, const Index& ix, Pos& t, M& m) {
  next_row(a.g, t.p);  // (wraps to offset 0 after the last inner row)
  if (++t.in < a.inner) return;
  t.in = 0;
  take_row(a, ix, t.i0 + 1, t, m);
}

template <int G, class M>
DORA_HD U16 take_pieces(const Args& a, const Index& ix, Pos& t, uint64_t b, M& m) {
  U16 v = {{0, 0, 0, 0}};
#pragma unroll
  for (int j = 0; j < 16 / G; ++j) {
    const uint64_t x =
        t.missing ? 0 : m.template load_piece<G>(t.base + t.p.off + static_cast<int64_t>(b));
    constexpr int kPerWord = G >= 4 ? 1 : 4 / G;
    if constexpr (G == 8) {
      v.w[2 * j] = static_cast<uint32_t>(x);
      v.w[2 * j + 1] = static_cast<uint32_t>(x >> 32);
    } else {
      v.w[j / kPerWord] |= static_cast<uint32_t>(x) << (8 * G * (j % kPerWord));
    }
    b += G;
    if (b >= a.g.row) {
      b = 0;
      next_taken(a, ix, t, m);
    }
  }
  return v;
}

// Whole unit `u` of the output: gather_unit's three paths behind the indirection.
template <class M>
DORA_HD void take_unit(const Args& a, const Index& ix, uint64_t u, M& m) {
  const gather::Args& g = a.g;
  const uint64_t o = g.head + 16 * u;
  uint64_t r, b;
  out_pos(g, o, &r, &b);
  Pos t;
  take_pos(a, ix, r, t, m);
  if (b + 16 <= g.row) {
    if (t.missing) {
      m.store16(o, U16{{0, 0, 0, 0}});
      return;
    }
    const int64_t s = t.base + t.p.off + static_cast<int64_t>(b);
    const uint32_t mis = static_cast<uint32_t>(
        (reinterpret_cast<uintptr_t>(g.src) + static_cast<uint64_t>(s)) & 15);
    if ((mis & 3) == 0) {
      m.store16(o, m.load16(s));
      return;
    }
    if (s - g.lo >= static_cast<int64_t>(mis) && s - static_cast<int64_t>(mis) <= g.hi - 31) {
      const int64_t w = s - static_cast<int64_t>(mis);
      m.store16(o, m.funnel(m.load16(w), m.load16(w + 16), mis));
      return;
    }
  }
  U16 v;
  switch (g.piece) {
    case 8: v = take_pieces<8>(a, ix, t, b, m); break;
    case 4: v = take_pieces<4>(a, ix, t, b, m); break;
    case 2: v = take_pieces<2>(a, ix, t, b, m); break;
    default: v = take_pieces<1>(a, ix, t, b, m); break;
  }
  m.store16(o, v);
}

template <class M>
DORA_HD void take_byte(const Args& a, const Index& ix, uint64_t o, M& m) {
  uint64_t r, b;
  out_pos(a.g, o, &r, &b);
  Pos t;
  take_pos(a, ix, r, t, m);
  m.store1(o, t.missing ? uint8_t(0)
                        : static_cast<uint8_t>(m.template load_piece<1>(
                              t.base + t.p.off + static_cast<int64_t>(b))));
}

// gather_lane's division of the work, over the taken body.
template <class M>
DORA_HD void take_lane(const Args& a, const Index& ix, uint64_t lane, uint64_t lanes, M& m) {
  const gather::Args& g = a.g;
  if (lane < 16) {
    if (lane < g.head) take_byte(a, ix, lane, m);
  } else if (lane < 32) {
    const uint64_t t0 = g.head + 16 * g.nunits;  // <= total
    if (lane - 16 < g.total - t0) take_byte(a, ix, t0 + (lane - 16), m);
  }
  for (uint64_t u = lane; u < g.nunits; u += lanes) take_unit(a, ix, u, m);
}

}  // namespace take

// ------------------------------------------------------------------------------------------
// Rows selected by a mask of N bytes (two kernels in front of gather_struct_kernel): the stream
// compaction that turns the mask into what a take reads — N int32 index words, of which the
// first K are the selected rows in source order and the rest -1 (the taken body's zero rows) — and
// into the counts C[0..N], C[i] the number of selected rows among rows [0, i), which a ragged
// batch's offsets are looked up in.  Any non-zero byte selects.
//
// Rows are counted from the 16-byte line the mask starts in: position v = row + shift, shift the
// mask's address mod 16, so that a thread's kUnit positions are one aligned 16-byte load wherever
// all of them are rows; the positions of a unit that holds the mask's head or tail go byte by
// byte, rows only, so nothing outside [mask, mask + N) is read.  A tile is kTile positions, one
// unit per thread.
//
//   mask_count_kernel, per tile: count_load (the thread's count into LDS; the tile's index words
//   set to -1, consecutive threads consecutive words), kSteps reduce_phase steps, count_store
//   (totals[tile]).
//   mask_compact_kernel, per tile: carry_load (the totals of the tiles before it, strided over the
//   threads — at most 4097 words, which is what caps N at kMaxRows), kSteps reduce_phase steps,
//   carry_read; scan_load (the thread's flags again), kSteps scan_step steps of the doubling scan
//   through two LDS rows, scan_store (C[i] for its rows, index[C[i]] = i for the selected ones;
//   the last tile's last thread writes C[N] = K and, for a message of one list, its offsets).
// A barrier stands between any two phases.  No workgroup waits for another and nothing is atomic:
// the kernel boundary orders the index words' -1 before their rows and the totals before their sum.
// ------------------------------------------------------------------------------------------
namespace mask {

constexpr int kUnit = 16;                    // positions per thread and tile
constexpr int kTile = kThreads * kUnit;      // positions per tile
constexpr int kSteps = 8;                    // log2(kThreads)
constexpr int kLds = 2 * kThreads;           // two rows of thread counts (4-byte words)
constexpr uint64_t kMaxRows = 1ull << 24;
static_assert((1 << kSteps) == kThreads, "the doubling scan covers the workgroup");

struct Args {
  const uint8_t* mask;  // N bytes, any alignment
  uint64_t n;           // rows
  uint32_t shift;       // the mask's address mod 16
  uint32_t one_list;    // 1: the last tile writes the sample's offsets [0, K]
  uint8_t* index;       // N int32 words
  uint8_t* counts;      // N + 1 int32 words: C
  uint8_t* totals;      // one int32 word per tile
  uint8_t* offsets;     // the sample's offsets buffer (one_list)
};

DORA_HD uint64_t tiles_for(uint64_t n, uint32_t shift) {
  return n ? (n + shift + kTile - 1) / kTile : 0;
}
DORA_HD uint64_t tiles(const Args& a) { return tiles_for(a.n, a.shift); }

// The workspace of a mask plan behind a sample of `size` bytes: 4-byte words from the first
// multiple of 4 at or past `size` — the index, C, the totals and `part` words of a host
// partition's offsets.  Offsets from the sample's start; `end` is what the destination must hold.
struct Workspace {
  uint64_t index, counts, totals, part, end;
};
DORA_HD Workspace workspace(uint64_t size, uint64_t n, uint64_t part_words) {
  Workspace w{};
  w.index = (size + 3) & ~uint64_t(3);
  w.counts = w.index + 4 * n;
  w.totals = w.counts + 4 * (n + 1);
  w.part = w.totals + 4 * tiles_for(n, 15);  // (whatever the mask's alignment turns out to be)
  w.end = w.part + 4 * part_words;
  return w;
}

DORA_HD Args make_args(const uint8_t* mask, uint64_t n, uint8_t* dst, const Workspace& w,
                       bool one_list) {
  Args a{};
  a.mask = mask;
  a.n = n;
  a.shift = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(mask) & 15);
  a.one_list = one_list ? 1 : 0;
  a.index = dst + w.index;
  a.counts = dst + w.counts;
  a.totals = dst + w.totals;
  a.offsets = dst;
  return a;
}

// Bit j: byte j of the unit is not zero.
DORA_HD uint32_t nonzero_bytes(const U16& u) {
  uint32_t f = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t t = u.w[k];
    t |= t >> 4;
    t |= t >> 2;
    t |= t >> 1;
    t &= 0x01010101u;
    f |= ((t & 1) | ((t >> 7) & 2) | ((t >> 14) & 4) | ((t >> 21) & 8)) << (4 * k);
  }
  return f;
}

// Whether position v is a row; then v - shift is the row.
DORA_HD bool live(const Args& a, uint64_t v) { return v >= a.shift && v < a.n + a.shift; }

// The thread's unit of the tile: bit j set where position first + j is a selected row.
template <class M>
DORA_HD uint32_t unit_flags(const Args& a, uint64_t tile, uint32_t thread, M& m) {
  const uint64_t first = tile * kTile + static_cast<uint64_t>(thread) * kUnit;
  if (first >= a.n + a.shift || first + kUnit <= a.shift) return 0;
  if (first >= a.shift && first + kUnit <= a.n + a.shift) return nonzero_bytes(m.load16(first));
  uint32_t f = 0;
  for (int j = 0; j < kUnit; ++j) {
    const uint64_t v = first + static_cast<uint64_t>(j);
    if (live(a, v) && m.load_byte(v - a.shift)) f |= 1u << j;
  }
  return f;
}

DORA_HD uint32_t popcount(uint32_t f) { return static_cast<uint32_t>(__builtin_popcount(f)); }

// One halving step of a sum over row 0 of the LDS buffer: after kSteps of them slot 0 is the sum.
template <class M>
DORA_HD void reduce_phase(uint32_t thread, int step, M& m) {
  const uint32_t d = static_cast<uint32_t>(kThreads) >> (step + 1);
  if (thread < d) m.lds_write(thread, m.lds_read(thread) + m.lds_read(thread + d));
}

template <class M>
DORA_HD void count_load(const Args& a, uint64_t tile, uint32_t thread, M& m) {
  m.lds_write(thread, popcount(unit_flags(a, tile, thread, m)));
#pragma unroll
  for (int j = 0; j < kUnit; ++j) {
    const uint64_t v = tile * kTile + static_cast<uint64_t>(j) * kThreads + thread;
    if (live(a, v)) m.store_index(v - a.shift, -1);
  }
}

template <class M>
DORA_HD void count_store(const Args&, uint64_t tile, uint32_t thread, M& m) {
  if (thread == 0) m.store_total(tile, m.lds_read(0));
}

template <class M>
DORA_HD void carry_load(const Args&, uint64_t tile, uint32_t thread, M& m) {
  uint32_t s = 0;  // (at most N <= 2^24 in all)
  for (uint64_t i = thread; i < tile; i += kThreads) s += m.load_total(i);
  m.lds_write(thread, s);
}

template <class M>
DORA_HD uint32_t carry_read(M& m) { return m.lds_read(0); }

template <class M>
DORA_HD uint32_t scan_load(const Args& a, uint64_t tile, uint32_t thread, M& m) {
  const uint32_t f = unit_flags(a, tile, thread, m);
  m.lds_write(thread, popcount(f));
  return f;
}

// Step `step` of the doubling scan over the thread counts: row (step & 1) -> the other row.
template <class M>
DORA_HD void scan_step(uint32_t thread, int step, M& m) {
  const uint32_t from = static_cast<uint32_t>(step & 1) * kThreads, to = kThreads - from;
  const uint32_t d = 1u << step;
  uint32_t v = m.lds_read(from + thread);
  if (thread >= d) v += m.lds_read(from + thread - d);
  m.lds_write(to + thread, v);
}

// After kSteps steps (an even number) the inclusive counts are back in row 0.
template <class M>
DORA_HD void scan_store(const Args& a, uint64_t tile, uint32_t thread, uint32_t f, uint32_t carry,
                        M& m) {
  static_assert(kSteps % 2 == 0, "the counts end in row 0");
  const uint32_t before = carry + (thread ? m.lds_read(thread - 1) : 0);
  const uint64_t first = tile * kTile + static_cast<uint64_t>(thread) * kUnit;
#pragma unroll
  for (int j = 0; j < kUnit; ++j) {
    const uint64_t v = first + static_cast<uint64_t>(j);
    if (!live(a, v)) continue;
    const uint64_t row = v - a.shift;
    const uint32_t c = before + popcount(f & ((1u << j) - 1));  // < N: a scatter position
    m.store_count(row, c);
    if ((f >> j) & 1) m.store_index(c, static_cast<int32_t>(row));
  }
  if (tile + 1 == tiles(a) && thread == static_cast<uint32_t>(kThreads) - 1) {
    const uint32_t k = carry + m.lds_read(kThreads - 1);
    m.store_count(a.n, k);
    if (a.one_list) {
      m.store_offset(0, 0);
      m.store_offset(1, k);
    }
  }
}

}  // namespace mask

// ------------------------------------------------------------------------------------------
// A field converted on the way (one more field kind, run by gather_cast_kernel,
// gather_quant_kernel and gather_affine_kernel only): the rows
// body restated per element, source elements of one type read, converted and written as float16
// or float32, or quantised to an 8- or 16-bit integer.  Only the arguments live here, where multi::Field needs them; the body is
// cast_device.h.
// ------------------------------------------------------------------------------------------
namespace cast {

// What the source elements are; every value of each is exact in float32.
enum Src : uint32_t { kU8 = 0, kI8 = 1, kU16 = 2, kI16 = 3, kF16 = 4, kBF16 = 5, kF32 = 6 };
// What the destination elements are: a float of `dsize` bytes, or (a quantised field) an integer
// of `dsize` bytes that the rounded product is clamped to.
enum Dst : uint32_t { kDstFloat = 0, kDstU8 = 1, kDstI8 = 2, kDstU16 = 3, kDstI16 = 4 };

struct Args {
  // the view with rows counted in elements: `total` elements in all, `row` contiguous elements
  // per row, `head` elements before the first whole 16-byte unit of the output, `nunits` whole
  // units; `piece` the source element size; shape[] / stride[] and [lo, hi] in source bytes
  gather::Args g;
  uint32_t src;        // Src
  uint32_t dsize;      // destination element size: 2 (float16) or 4 (float32); quantised: 1 or 2
  uint32_t has_scale;
  float scale;
  uint32_t dst;        // Dst
  int32_t zp;          // a quantised field's zero point, inside the destination's range
  // the affine step (read by gather_affine_kernel only): per-channel
  // float32 tables that take the place of `scale` and `bias` where they are not null, output
  // element e being of channel (e / inner) % channels
  const uint8_t* stab;
  const uint8_t* btab;
  uint64_t inner;
  uint64_t channels;
  uint32_t has_bias;
  float bias;
};
static_assert(sizeof(Args) == sizeof(gather::Args) + 64, "the affine arguments fill the union");

}  // namespace cast

// ------------------------------------------------------------------------------------------
// A field reduced on the way (two more field kinds, run by gather_reduce_kernel only): the index
// of the maximum along one axis of the source, one index per element of the kept dimensions.
// Only the arguments live here, where multi::Field needs them; the bodies are reduce_device.h.
// ------------------------------------------------------------------------------------------
namespace reduce {

struct Args {
  // the view of the kept dimensions with rows counted in elements, as cast::Args has it: `total`
  // output elements, `row` contiguous source elements per row, `head` elements before the first
  // whole 16-byte unit of the output, `nunits` whole units, `piece` the source element size;
  // shape[] / stride[] in source bytes and [lo, hi] over all `c` steps of the reduced axis
  gather::Args g;
  uint64_t c;        // candidates per output element, >= 1
  int64_t cstride;   // bytes per step of the reduced axis (signed, 0 allowed)
  uint32_t src;      // cast::Src
  uint32_t dsize;    // index element size: 1, 2, 4 or 8
};

}  // namespace reduce

// ------------------------------------------------------------------------------------------
// A field resized on the way (one more field kind, run by gather_resize_kernel only): two
// dimensions of the source take new extents by nearest or bilinear taps.  Only the arguments live
// here, where multi::Field needs them; the body is resize_device.h.
// ------------------------------------------------------------------------------------------
namespace resize {

struct Args {
  // the output counted in elements: `total` output elements, `row` 1 (every element a row of the
  // odometer, whose shape[] is the output's), `head` elements before the first whole 16-byte unit
  // of the output, `nunits` whole units, `piece` the source element size; stride[] in source
  // bytes with 0 at the two resized dimensions, whose steps are sa[] below; [lo, hi] the reach of
  // the whole source view
  gather::Args g;
  int64_t sa[2];     // source bytes per step of the resized dimensions (signed, 0 allowed)
  uint32_t in[2];    // their source extents, 1 .. 32768
  uint32_t out[2];   // their output extents, 1 .. 32768 (shape[] at ax[])
  uint8_t ax[2];    // their places in shape[], in the order of the caller's axes
  uint8_t mode;      // DORA_RESIZE_NEAREST or DORA_RESIZE_BILINEAR
  uint8_t src;       // cast::Src
  uint8_t dst;       // cast::Dst
  uint8_t dsize;     // destination element size: 1, 2 or 4
  uint8_t pad[2];
};

}  // namespace resize

// ------------------------------------------------------------------------------------------
// A field of crops (one more field kind, run by gather_crop_kernel only): K boxes read from HBM,
// each cut from one frame and resized to the same extents.  Only the arguments live here, where
// multi::Field needs them; the body is crop_device.h.
// ------------------------------------------------------------------------------------------
namespace crop {

struct Args {
  // a resized field's arguments over all K crops: the output's odometer with K as one more leading
  // dimension of stride 0 at shape[kax], in[] the frame's extents along the two cropped
  // dimensions (what a box is clamped to), [lo, hi] the reach of the whole frame
  resize::Args r;
  const uint8_t* boxes;  // K rows of four int32 words: a_lo, b_lo, a_hi, b_hi; 4-byte aligned
  uint8_t kax;           // K's place in shape[]
  uint8_t pad[7];
};

}  // namespace crop

// ------------------------------------------------------------------------------------------
// What a model-input field adds to its resize or crops (run by gather_resize_prep_kernel and
// gather_crop_prep_kernel only): the resized image placed inside a filled output, and the affine
// step y = r * S[c] + B[c] before the conversion.  The arguments travel beside multi::Args
// (prep::Launch, resize_device.h), so resize::Args, crop::Args and multi::Args keep their sizes;
// the bodies are resize_device.h and crop_device.h under their flag.
// ------------------------------------------------------------------------------------------
namespace prep {

// The bodies' flag: with None no line of the step is compiled.
struct None {
  static constexpr bool on = false;
};

struct Args {
  static constexpr bool on = true;
  const uint8_t* stab;   // per-channel float32 tables along shape[cax], 4-byte aligned; null: the
  const uint8_t* btab;   // scalar below (or no term at all)
  float scale, bias;     // the scalar terms
  float fill;            // the value of an element outside the placed image, before the step
  uint16_t inner[2];     // the extents of the resized image, 1 .. out[j] (out[j]: it fills the axis)
  uint16_t lead[2];      // where it starts in the output, lead[j] + inner[j] <= out[j]
  uint8_t cax;           // the tables' place in shape[]; read only with a table
  uint8_t has_scale;     // a product is applied: by stab[c], else by `scale`
  uint8_t has_bias;      // a sum is applied: with btab[c], else with `bias`
  uint8_t pad;
};
static_assert(sizeof(Args) == 40, "eight of them travel beside multi::Args");

}  // namespace prep

namespace multi {

constexpr int kMaxFields = static_cast<int>(kMaxStructFields);
// (a scan share, kScan, is no Field: it has no view; it runs workgroups [0, wg_begin[0]))
// (kRowsCast fields are run by gather_cast_kernel / gather_quant_kernel / gather_affine_kernel
// only: gather_struct_kernel's launches hold none)
// (kReduceLane and kReduceWave fields are run by gather_reduce_kernel only, kResize fields by
// gather_resize_kernel only, kCrop fields by gather_crop_kernel only)
enum Kind : uint32_t {
  kRows = 0, kTile = 1, kScan = 2, kRowsTaken = 3, kRowsCast = 4, kReduceLane = 5, kReduceWave = 6,
  kResize = 7, kCrop = 8
};

struct Field {
  uint32_t kind;
  uint32_t pad;
  union {
    gather::Args rows;
    tile::Args tile;
    take::Args taken;
    cast::Args cast;
    reduce::Args reduce;
    resize::Args resize;
    crop::Args crop;
  };
};
static_assert(sizeof(take::Args) <= sizeof(tile::Args), "a taken field does not grow Field");
static_assert(sizeof(cast::Args) <= sizeof(tile::Args), "a cast field does not grow Field");
static_assert(sizeof(reduce::Args) <= sizeof(tile::Args), "a reduced field does not grow Field");
static_assert(sizeof(resize::Args) <= sizeof(tile::Args), "a resized field does not grow Field");
static_assert(sizeof(crop::Args) <= sizeof(tile::Args), "a field of crops does not grow Field");

struct Args {
  uint32_t n;
  uint32_t wg_begin[kMaxFields + 1];  // field k runs workgroups [wg_begin[k], wg_begin[k + 1])
  Field f[kMaxFields];
  scan::Args scan;  // src null: no scan share, wg_begin[0] == 0
  take::Index take; // the index of the kRowsTaken fields (all or none of a launch's fields)
  // a mask plan's launch (mask:: above): the counts C[0..n] its scan share's words are looked up
  // in on their way into the sample (o -> C[o], o <= n already); null for every other launch
  const uint8_t* lookup;
};
static_assert(sizeof(Args) <= 4096, "multi::Args is passed by value: the kernel-argument limit");

// What every launch's Args share: with `sc` the launch's first workgroup scans a ragged batch's
// partition into the offsets at dst + 0 and the fields' workgroups follow it (n may then be 0);
// field k runs the workgroups behind those of the fields before it — `place(k, f)` sets f.kind
// and the field's own arguments and returns its grid — and the rest of wg_begin repeats the end.
// The grid is wg_begin[n]: at most 8 * 2^20 + 1 workgroups.
template <class Place>
DORA_HD Args make_args_by(int n, uint8_t* dst, const ScanDesc* sc, Place place) {
  Args a{};
  a.n = static_cast<uint32_t>(n);
  uint32_t wg = 0;
  if (sc) {
    a.scan = scan::make_args(*sc, dst);
    wg = 1;
  }
  for (int k = 0; k < n; ++k) {
    a.wg_begin[k] = wg;
    wg += place(k, a.f[k]);
  }
  for (int k = n; k <= kMaxFields; ++k) a.wg_begin[k] = wg;
  return a;
}

// A field moved as it is: the tile body against its source-contiguous dimension `tile_c`, or the
// rows body when that is negative (the launcher's selection).
DORA_HD uint32_t place_plain(Field& f, const GatherDesc& g, uint8_t* dst, int tile_c) {
  if (tile_c >= 0) {
    f.kind = kTile;
    f.tile = tile::make_args(g, dst, tile_c);
    return static_cast<uint32_t>(tile::grid_for(f.tile));
  }
  f.kind = kRows;
  f.rows = gather::make_args(g, dst);
  return static_cast<uint32_t>(gather::grid_for(f.rows));
}

// Arguments of the gather of g[0..n) into dst + off[k], field k by tile_c[k]; `sc` as above.
DORA_HD Args make_args(const GatherDesc* g, const uint64_t* off, const int* tile_c, int n,
                       uint8_t* dst, const ScanDesc* sc = nullptr) {
  return make_args_by(n, dst, sc, [&](int k, Field& f) {
    return place_plain(f, g[k], dst + off[k], tile_c[k]);
  });
}

// Arguments of a take: every field g[k] (dimensions 1.. of its view, stride0[k] its dimension 0)
// through the taken body into dst + off[k], all by the index `tk`; each field gets the grid the
// rows body would have for its bytes.  `sc` as above.
DORA_HD Args make_taken_args(const GatherDesc* g, const int64_t* stride0, const uint64_t* off,
                             int n, uint8_t* dst, const TakeDesc& tk,
                             const ScanDesc* sc = nullptr) {
  Args a = make_args_by(n, dst, sc, [&](int k, Field& f) {
    f.kind = kRowsTaken;
    f.taken = take::make_args(g[k], stride0[k], dst + off[k]);
    return static_cast<uint32_t>(gather::grid_for(f.taken.g));
  });
  a.take.src = tk.src;
  a.take.k = tk.count;
  a.take.n = tk.n;
  a.take.wide = tk.wide;
  return a;
}

DORA_HD uint32_t grid_for(const Args& a) { return a.wg_begin[a.n]; }

// The field workgroup `w` (wg_begin[0] <= w < grid_for) belongs to: uniform over the workgroup, at most
// kMaxFields - 1 steps.
DORA_HD int field_of(const Args& a, uint32_t w) {
  int k = 0;
  while (k + 1 < static_cast<int>(a.n) && w >= a.wg_begin[k + 1]) ++k;
  return k;
}

}  // namespace multi

}  // namespace gather
}  // namespace dora
