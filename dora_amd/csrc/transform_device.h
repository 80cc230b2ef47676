// Device code of the transform segments of compacting plans (plan.cpp walk_compact): bitmap
// slices shifted to bit 0 and offsets rebased to 0.  Elementwise and tiny next to the value
// buffers (a bitmap is len/8 bytes, offsets 4-8 B per list), so one simple grid over all
// transform segments of a launch.
//
// Which block takes which elements of which segment, what is read and what is written is plain
// C++ that compiles for host and device alike, and every load and store goes through a policy
// object `M`.  transform_kernel (kernels.hip) passes a policy of plain loads and stores; the
// host emulation of tests/test_random_arrays_host.py (csrc/testing/transform_emulate.cpp) passes
// one that runs the same body for every block and thread over sources and a destination of
// exactly their sizes.  Nothing here uses an intrinsic.
#pragma once

#include <cstddef>
#include <cstdint>

#include "plan.h"

#if defined(__HIPCC__)
#define DORA_HD __host__ __device__ inline
#define DORA_HDI __host__ __device__ inline __attribute__((always_inline))
#else
#define DORA_HD inline
#define DORA_HDI inline
#endif

namespace dora {
namespace xform {

constexpr int kXThreads = 256;  // threads per workgroup (the pack's)
constexpr int kXMaxSegs = 32;   // segments of one launch (the pack's)

struct XSeg {
  const uint8_t* src;
  uint64_t dst_off;
  uint64_t len;      // output bytes
  uint64_t src_len;  // readable source bytes (bitshift)
  uint32_t op;
  uint32_t aux;      // bit offset (bitshift)
};

struct XArgs {
  uint8_t* dst;
  uint32_t nseg;
  uint32_t block_end[kXMaxSegs];
  XSeg seg[kXMaxSegs];
};

constexpr uint64_t kXElems = 4096;  // output elements per workgroup

DORA_HD uint64_t xseg_elems(const Segment& s) {
  return s.op == SEG_REBASE32 ? s.len / 4 : s.op == SEG_REBASE64 ? s.len / 8 : s.len;
}

// The arguments of one launch over `m` (<= kXMaxSegs) transform segments into `dst`: segment k
// takes blocks [block_end[k - 1], block_end[k]), at least one.  Returns the launch's blocks; 0:
// more than a block index holds (0x7fffffff).
DORA_HD uint32_t fill_xargs(XArgs& x, uint8_t* dst, const Segment* segs, size_t m) {
  x.dst = dst;
  uint64_t blocks = 0;
  for (size_t k = 0; k < m; ++k) {
    const Segment& s = segs[k];
    x.seg[k] = {static_cast<const uint8_t*>(s.src), s.dst_off, s.len, s.src_len, s.op, s.aux};
    const uint64_t b = (xseg_elems(s) + kXElems - 1) / kXElems;
    blocks += b ? b : 1;
    if (blocks > 0x7fffffffull) return 0;
    x.block_end[k] = static_cast<uint32_t>(blocks);
  }
  x.nseg = static_cast<uint32_t>(m);
  return static_cast<uint32_t>(blocks);
}

// Elements [e0, e1) of `count` offsets of type T, each minus the first of the segment.  Words at
// multiples of sizeof(T) on both sides move whole, others byte-wise (M::ldu / M::stu).
template <typename T, class M>
DORA_HDI void rebase(const uint8_t* src, uint8_t* dst, uint64_t count, uint64_t e0, uint64_t e1,
                     uint32_t thread, M& m) {
  const T base = m.template ldu<T>(src);
  const bool aligned = ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) &
                        (sizeof(T) - 1)) == 0;
  for (uint64_t i = e0 + thread; i < e1 && i < count; i += kXThreads) {
    if (aligned) {
      m.template st<T>(dst + i * sizeof(T), m.template ld<T>(src + i * sizeof(T)) - base);
    } else {
      T v = m.template ldu<T>(src + i * sizeof(T));
      v -= base;
      m.template stu<T>(dst + i * sizeof(T), v);
    }
  }
}

// What thread `thread` of block `blk` of a launch does: kXElems output elements of its segment.
template <class M>
DORA_HDI void transform_body(const XArgs& a, uint32_t blk, uint32_t thread, M& m) {
  uint32_t s = 0;
  while (s + 1 < a.nseg && blk >= a.block_end[s]) ++s;
  const XSeg g = a.seg[s];
  const uint64_t c = blk - (s ? a.block_end[s - 1] : 0u);
  const uint64_t e0 = c * kXElems, e1 = e0 + kXElems;
  uint8_t* dst = a.dst + g.dst_off;
  if (g.op == SEG_BITSHIFT) {
    for (uint64_t j = e0 + thread; j < e1 && j < g.len; j += kXThreads) {
      const uint32_t lo = m.template ld<uint8_t>(g.src + j);
      const uint32_t hi = j + 1 < g.src_len ? m.template ld<uint8_t>(g.src + (j + 1)) : 0u;
      const uint8_t v = static_cast<uint8_t>(g.aux ? ((lo >> g.aux) | (hi << (8 - g.aux))) : lo);
      m.template st<uint8_t>(dst + j, v);
    }
  } else if (g.op == SEG_REBASE32) {
    rebase<int32_t>(g.src, dst, g.len / 4, e0, e1, thread, m);
  } else if (g.op == SEG_REBASE64) {
    rebase<int64_t>(g.src, dst, g.len / 8, e0, e1, thread, m);
  }
}

}  // namespace xform
}  // namespace dora
