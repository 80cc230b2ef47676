// HIP kernels of the data plane (gfx950): launches of the batched segmented pack (device code in
// pack_device.h) that replaces `copy_array_into_sample` (apis/rust/node/src/node/
// arrow_utils.rs:23-71), the compacting transforms, the csum64 parity reduction and the
// splitmix64 payload generator.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <mutex>
#include <cstring>
#include <string>
#include <vector>

#include "aql.h"
#include "common.h"
#include "cast_device.h"
#include "reduce_device.h"
#include "resize_device.h"
#include "crop_device.h"
#include "gather_device.h"
#include "pack_device.h"
#include "plan.h"
#include "splitmix_device.h"
#include "transform_device.h"

namespace dora {
namespace {

using namespace pack;
using namespace xform;

template <int U, int NT>
__global__ __launch_bounds__(kThreads) void pack_kernel(PackArgs args) {
  // grid = chunks (one chunk per workgroup), or fewer workgroups striding over the chunks when
  // the launch signals its fill (fewer workgroups to count in)
  pack_body<U, NT>(args, blockIdx.x, gridDim.x);
}

// Workgroups at most of a pack the command processor signals: a synchronous 40.96 MB send
// (5,000 chunks) takes 21.7-22.0 us with 3584 workgroups against 22.0-22.7 with 4096, 22.9 with
// one per chunk, 22.7-23.3 with 3072 and 24.6-25.3 with fewer, larger chunks, in four interleaved
// rounds of 200 sends (profiles/r04_sync_ab.jsonl batches sy4-sy6; packs below 28 MiB have fewer
// chunks than that).
constexpr uint32_t kCpGrid = 3584;
// Workgroups at most of a multi-segment pack the command processor signals.  Such packs (C3's
// 13 MB clouds) run up to four at once, one per queue: 640 workgroups each (2.5 per CU) against
// the single-segment cap of 3584, C3's 20-cloud burst 0.67-0.72 -> 0.72-0.75 and its 200-cloud
// steady state 0.71-0.72 -> 0.77-0.79 of HBM (caps 512-1536 interleaved over four boxes,
// profiles/r05_c3_cp_grid_b.jsonl, r05_c3_multi_grid_*.jsonl).
constexpr uint32_t kCpGridMulti = 640;

// The HIP-launched pack: 4 x 16-B loads in flight per lane, non-temporal loads and stores (the
// r01 sweep, profiles/r01_pack_sweep*.jsonl: 10-12 % at 16-40 MB, the sample is consumed by
// another process; neutral below); its signalling launch stores write-through (NT = 2).  The
// sweep's other variants (2 / 8 loads, cached stores) and their tuning hooks were removed in r06
// (verdict r05 item 6): the product library carries no variant only a microbenchmark selects.
constexpr int kUnroll = 4;

// ------------------------------------------------------------------------------------------
// transform_kernel: the transform segments of compacting plans (transform_device.h holds the
// body and the table of a launch; this is its memory policy): plain loads and stores, whole
// words where source and destination allow it.
// ------------------------------------------------------------------------------------------
static_assert(kXThreads == kThreads && kXMaxSegs == kMaxSegs, "a transform launch is cut as a pack");

struct XformMem {
  template <typename T>
  __device__ __forceinline__ T ld(const uint8_t* p) const {
    return *reinterpret_cast<const T*>(p);
  }
  template <typename T>
  __device__ __forceinline__ void st(uint8_t* p, T v) const {
    *reinterpret_cast<T*>(p) = v;
  }
  template <typename T>
  __device__ __forceinline__ T ldu(const uint8_t* p) const {
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
  }
  template <typename T>
  __device__ __forceinline__ void stu(uint8_t* p, T v) const {
    __builtin_memcpy(p, &v, sizeof(T));
  }
};

__global__ __launch_bounds__(kThreads) void transform_kernel(XArgs a) {
  XformMem m;
  transform_body(a, blockIdx.x, threadIdx.x, m);
}

// Loads in flight per lane: 4 at every size.  r01's isolated-pack probes preferred 8 loads over
// 32 KiB chunks for 8-32 MB bodies; under the node's overlapping AQL packs (line-aligned chunks,
// no release fence) 4 loads over 8 KiB chunks are faster there: C3 4.70-4.91 -> 4.56 us per
// cloud, a flat 13 MB pack 4.81-4.91 -> 4.33-4.37 us, 16 MB unchanged
// (profiles/r02_u4_mid_ab.jsonl, r02_c3_final_knobs_ab.jsonl).
uint32_t choose_chunk_bytes(uint64_t body_bytes) {
  // r01 probes (profiles/r01_copy_probe.jsonl): at >= 32 MB the best shape is many small
  // workgroups (8 KiB each, 4 loads in flight per lane: 40.96 MB in 14.6 us launch-to-launch);
  // below that ~2k workgroups of >= 8 KiB.
  constexpr uint64_t kGrain = 8192;
  if (body_bytes >= (32u << 20)) return kGrain;
  uint64_t cb = (body_bytes / 2048 + kGrain - 1) / kGrain * kGrain;
  cb = std::max<uint64_t>(cb, kGrain);
  cb = std::min<uint64_t>(cb, uint64_t(1) << 22);
  return static_cast<uint32_t>(cb);
}

// ------------------------------------------------------------------------------------------
// csum64 (oracle/checksum_ref.py): S = sum_i fmix64(word_i ^ (i * GOLDEN + SEED)); fmix64(S+n)
// ------------------------------------------------------------------------------------------
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kSeed = 0xD0A5D0A5D0A5D0A5ull;

__host__ __device__ __forceinline__ uint64_t fmix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(kThreads) void csum_kernel(const uint8_t* __restrict__ p, uint64_t n,
                                                        unsigned long long* __restrict__ acc) {
  const uint64_t nw = (n + 7) / 8;
  const uint64_t full = n / 8;
  const bool aligned8 = (reinterpret_cast<uintptr_t>(p) & 7) == 0;
  uint64_t s = 0;
  for (uint64_t i = blockIdx.x * uint64_t(kThreads) + threadIdx.x; i < nw;
       i += uint64_t(gridDim.x) * kThreads) {
    uint64_t w = 0;
    if (aligned8 && i < full) {
      w = reinterpret_cast<const uint64_t*>(p)[i];
    } else {
      const uint64_t lim = (i < full) ? 8 : (n - 8 * i);
      for (uint64_t k = 0; k < lim; ++k) w |= uint64_t(p[8 * i + k]) << (8 * k);
    }
    s += fmix64(w ^ (i * kGolden + kSeed));
  }
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(acc, static_cast<unsigned long long>(s));
}

__global__ void csum_finalize(unsigned long long* acc, uint64_t n) {
  *acc = fmix64(static_cast<uint64_t>(*acc) + n);
}

// splitmix64 payload: word k = fmix64(seed + (k + 1) * GOLDEN), little-endian bytes.
__global__ __launch_bounds__(kThreads) void fill_kernel(uint8_t* __restrict__ p, uint64_t n,
                                                        uint64_t seed) {
  const uint64_t nw = (n + 7) / 8;
  const bool aligned8 = (reinterpret_cast<uintptr_t>(p) & 7) == 0;
  for (uint64_t i = blockIdx.x * uint64_t(kThreads) + threadIdx.x; i < nw;
       i += uint64_t(gridDim.x) * kThreads) {
    const uint64_t w = fmix64(seed + (i + 1) * kGolden);
    if (aligned8 && 8 * i + 8 <= n) {
      reinterpret_cast<uint64_t*>(p)[i] = w;
    } else {
      for (uint64_t k = 0; k < 8 && 8 * i + k < n; ++k) p[8 * i + k] = uint8_t(w >> (8 * k));
    }
  }
}

// The same payload written into a sample in place with write-through stores and published by the
// launch itself through the public device header (include/dora_gpu_device.h): the grid is the
// ticket's workgroup count, striding over the payload's 16-byte units.
__global__ __launch_bounds__(kThreads) void fill_ticket_kernel(uint8_t* p, uint64_t n,
                                                               uint64_t seed, dora_fill_ticket t) {
  splitmix::fill_and_publish<true>(p, n, seed, t);
}

// ------------------------------------------------------------------------------------------
// gather_rows_kernel: a strided device tensor view into row-major order (gather_device.h holds
// every address computation; this is its memory policy).  Rows are read with the pack's 16-byte
// non-temporal loads, elements of rows shorter than a unit with plain cached loads (a transposed
// source line is touched by many units), the sample is written with the pack's write-through
// stores.
// ------------------------------------------------------------------------------------------
struct GatherMem {
  const uint8_t* src;
  uint8_t* dst;
  typedef uint16_t u16_u __attribute__((aligned(1)));
  typedef uint32_t u32_u __attribute__((aligned(1)));
  typedef uint64_t u64_u __attribute__((aligned(1)));

  __device__ __forceinline__ gather::U16 load16(int64_t s) const {  // src + s: whole dwords
    const u32x4 v = ld16<1, true>(src + s);
    return {{v.x, v.y, v.z, v.w}};
  }
  template <int G>
  __device__ __forceinline__ uint64_t load_piece(int64_t s) const {
    const uint8_t* p = src + s;
    if constexpr (G == 8) return *reinterpret_cast<const u64_u*>(p);
    if constexpr (G == 4) return *reinterpret_cast<const u32_u*>(p);
    if constexpr (G == 2) return *reinterpret_cast<const u16_u*>(p);
    return *p;
  }
  // bytes [mis, mis + 16) of lo | hi
  __device__ __forceinline__ gather::U16 funnel(gather::U16 lo, gather::U16 hi,
                                                uint32_t mis) const {
    const u32x4 l = {lo.w[0], lo.w[1], lo.w[2], lo.w[3]}, h = {hi.w[0], hi.w[1], hi.w[2], hi.w[3]};
    u32x4 o;
    switch (mis >> 2) {
      case 0: o = pack::funnel<0>(l, h, mis & 3); break;
      case 1: o = pack::funnel<1>(l, h, mis & 3); break;
      case 2: o = pack::funnel<2>(l, h, mis & 3); break;
      default: o = pack::funnel<3>(l, h, mis & 3); break;
    }
    return {{o.x, o.y, o.z, o.w}};
  }
  __device__ __forceinline__ void store16(uint64_t o, gather::U16 v) const {
    st16<2>(dst + o, u32x4{v.w[0], v.w[1], v.w[2], v.w[3]});
  }
  __device__ __forceinline__ void store1(uint64_t o, uint8_t v) const { st1<2>(dst + o, v); }
};

// The taken body's memory (gather_device.h take::): a field's bytes as GatherMem moves them, and
// the launch's index words with plain cached loads — neighbouring units read the same words
// again, and the word is naturally aligned (the plan refuses an index that is not).
struct TakeMem : GatherMem {
  const uint8_t* index;
  uint32_t wide;
  __device__ __forceinline__ int64_t load_index(uint64_t i) const {
    return wide ? reinterpret_cast<const int64_t*>(index)[i]
                : static_cast<int64_t>(reinterpret_cast<const int32_t*>(index)[i]);
  }
};

__global__ __launch_bounds__(gather::kThreads) void gather_rows_kernel(gather::Args a) {
  GatherMem m{a.src, a.dst};
  gather::gather_lane(a, uint64_t(blockIdx.x) * gather::kThreads + threadIdx.x,
                      uint64_t(gridDim.x) * gather::kThreads, m);
}

// gather_tile_kernel: the (c, j) plane of a permuted view through a padded LDS tile
// (gather_device.h tile::): loads coalesced along the source-contiguous dimension, stores
// coalesced along the output's innermost one.  Source, strides and destination are
// element-aligned (tile::contiguous_dim), so every access is a natural one of T.
template <typename T>
struct TileMem {
  const uint8_t* src;
  uint8_t* dst;
  T* lds;
  __device__ __forceinline__ T load_elem(int64_t s) const {
    return *reinterpret_cast<const T*>(src + s);
  }
  __device__ __forceinline__ void lds_write(uint32_t i, T v) const { lds[i] = v; }
  __device__ __forceinline__ T lds_read(uint32_t i) const { return lds[i]; }
  __device__ __forceinline__ void store_elem(uint64_t e, T v) const {
    __builtin_nontemporal_store(v, reinterpret_cast<T*>(dst) + e);
  }
};

// Tiles first, first + step, .. of `a` through the workgroup's tile `lds`.
template <typename T>
__device__ __forceinline__ void tile_loop(const gather::tile::Args& a, uint64_t first,
                                          uint64_t step, T* lds) {
  TileMem<T> m{a.src, a.dst, lds};
  for (uint64_t t = first; t < a.ntiles; t += step) {
    const gather::tile::Origin o = gather::tile::origin(a, t);
    gather::tile::load_phase(a, o, threadIdx.x, m);
    __syncthreads();
    gather::tile::store_phase(a, o, threadIdx.x, m);
    __syncthreads();  // the tile is reused by this workgroup's next one
  }
}

template <typename T>
__global__ __launch_bounds__(gather::kThreads) void gather_tile_kernel(gather::tile::Args a) {
  __shared__ T lds[gather::tile::kLds];
  tile_loop<T>(a, blockIdx.x, gridDim.x, lds);
}

// The scan share's memory: the partition's words with plain loads (each is read once, by one
// thread), the thread totals in the workgroup's LDS buffer, the offsets with the pack's
// write-through stores, one aligned dword each.
struct ScanMem {
  const uint8_t* src;
  uint8_t* dst;
  uint64_t* lds;
  uint32_t wide;
  const uint8_t* lookup;  // a mask plan's counts C: the word stored is C[v] (null: v itself)
  __device__ __forceinline__ int64_t load_word(uint64_t i) const {
    return wide ? reinterpret_cast<const int64_t*>(src)[i]
                : static_cast<int64_t>(reinterpret_cast<const int32_t*>(src)[i]);
  }
  __device__ __forceinline__ void lds_write(uint32_t i, uint64_t v) const { lds[i] = v; }
  __device__ __forceinline__ uint64_t lds_read(uint32_t i) const { return lds[i]; }
  __device__ __forceinline__ void store_word(uint64_t i, uint32_t v) const {
    if (lookup) v = reinterpret_cast<const uint32_t*>(lookup)[v];
    st4<2>(dst + 4 * i, v);
  }
};

// The whole scan share, run by one workgroup: tile by tile with the carry in a register of every
// thread (gather_device.h scan::).  The barrier that ends a tile keeps the next tile's totals out
// of row 0 until every thread has read this tile's.
__device__ __forceinline__ void scan_share(const gather::scan::Args& a, uint64_t* lds,
                                           const uint8_t* lookup) {
  namespace sc = gather::scan;
  ScanMem m{a.src, a.dst, lds, a.wide, lookup};
  sc::head(a, threadIdx.x, m);
  uint64_t carry = 0;
  const uint64_t nt = sc::tiles(a);
  for (uint64_t t = 0; t < nt; ++t) {
    sc::Local loc;
    sc::load_phase(a, t, threadIdx.x, loc, m);
    __syncthreads();
#pragma unroll
    for (int step = 0; step < sc::kSteps; ++step) {
      sc::step_phase(a, threadIdx.x, step, m);
      __syncthreads();
    }
    carry = sc::store_phase(a, t, threadIdx.x, loc, carry, m);
    __syncthreads();
  }
}

// The cast body's memory and conversions (cast_device.h): a unit's contiguous source elements in
// one naturally aligned load of 4, 8 or 16 bytes, non-temporal like the rows body's (each is read
// once); single elements with plain cached loads (a permuted source line is touched by many
// units); the sample with the pack's write-through stores.  The conversions are plain casts,
// which the compiler turns into the hardware's (v_cvt_f32_ubyte0..3, v_cvt_f32_f16,
// v_cvt_pk_f16_f32 ..): round to nearest even, subnormals kept in both directions — the kernel
// descriptor's denormal modes are the default, and no build flag changes them.
struct CastMem {
  const uint8_t* src;
  uint8_t* dst;
  template <int N>
  __device__ __forceinline__ gather::U16 load_vec(int64_t s) const {
    const uint8_t* p = src + s;
    if constexpr (N == 16) {
      const u32x4 v = ld16<1, false>(p);
      return {{v.x, v.y, v.z, v.w}};
    } else if constexpr (N == 8) {
      const uint64_t v = __builtin_nontemporal_load(reinterpret_cast<const uint64_t*>(p));
      return {{static_cast<uint32_t>(v), static_cast<uint32_t>(v >> 32), 0, 0}};
    } else {
      return {{__builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p)), 0, 0, 0}};
    }
  }
  template <int S>
  __device__ __forceinline__ uint32_t load_elem(int64_t s) const {
    const uint8_t* p = src + s;
    if constexpr (S == 4) return *reinterpret_cast<const uint32_t*>(p);
    else if constexpr (S == 2) return *reinterpret_cast<const uint16_t*>(p);
    else return *p;
  }
  template <uint32_t K>
  __device__ __forceinline__ float to_f32(uint32_t raw) const {
    namespace c = gather::cast;
    if constexpr (K == c::kF32) {
      return __builtin_bit_cast(float, raw);
    } else if constexpr (K == c::kBF16) {
      return __builtin_bit_cast(float, raw << 16);
    } else if constexpr (K == c::kF16) {
      return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(raw)));
    } else {
      return c::int_to_f32<K>(raw);
    }
  }
  // The product is made opaque: left to itself the compiler fuses a float16 source's widening,
  // this multiplication and the rounding to float16 into one v_fma_mixlo_f16 x, s, 0, and
  // (-0) + (+0) is +0 — a zero product (x or s +-0) lost its sign.  Behind the empty asm it is a
  // v_mul_f32 and a v_cvt_f16_f32, which is the statement of record.
  __device__ __forceinline__ float mul(float x, float s) const {
    float y = x * s;
    asm volatile("" : "+v"(y));
    return y;
  }
  // The sum of the affine step, opaque in the same way and for the same reason: the contract is
  // a rounded product and then a rounded sum, and left to itself the compiler contracts the pair
  // into one v_fma_f32 — or, towards float16, a v_fma_mix* — which rounds once.
  __device__ __forceinline__ float add(float x, float b) const {
    float y = x + b;
    asm volatile("" : "+v"(y));
    return y;
  }
  // Word `c` of a per-channel table (c < channels always; the table a whole number of dwords):
  // a plain cached load, neighbouring lanes read the same few words.
  __device__ __forceinline__ float load_table(const uint8_t* tab, uint64_t c) const {
    return reinterpret_cast<const float*>(tab)[c];
  }
  __device__ __forceinline__ uint32_t to_f16(float y) const {
    return __builtin_bit_cast(uint16_t, static_cast<_Float16>(y));
  }
  __device__ __forceinline__ uint32_t f32_bits(float y) const {
    return __builtin_bit_cast(uint32_t, y);
  }
  // A quantised element: round to nearest even (v_rndne_f32), a NaN as 0, the clamp against the
  // two bounds (exact in float32) and only then the conversion, which so never sees a value
  // outside int32 (v_cvt_i32_f32).  The product comes from `mul` above, opaque as it is there.
  __device__ __forceinline__ int32_t to_int(float y, int32_t lo, int32_t hi, int32_t zp) const {
    float r = __builtin_rintf(y);
    r = y != y ? 0.0f : r;
    r = fminf(fmaxf(r, static_cast<float>(lo)), static_cast<float>(hi));
    return static_cast<int32_t>(r) + zp;
  }
  __device__ __forceinline__ void store16(uint64_t o, gather::U16 v) const {
    st16<2>(dst + o, u32x4{v.w[0], v.w[1], v.w[2], v.w[3]});
  }
  template <int D>
  __device__ __forceinline__ void store_elem(uint64_t e, uint32_t bits) const {
    if constexpr (D == 4) {
      st4<2>(dst + 4 * e, bits);
    } else if constexpr (D == 1) {
      st1<2>(dst + e, static_cast<uint8_t>(bits));
    } else {
      __builtin_nontemporal_store(static_cast<uint16_t>(bits), reinterpret_cast<uint16_t*>(dst) + e);
    }
  }
};

// gather_struct_kernel: the fields of a struct-of-tensors plan in one launch (gather_device.h
// multi::).  A workgroup finds its field in the table (a uniform scan of at most 7 steps) and
// runs that field's own body over the field's share of the grid: gather_lane with the lane
// numbered inside the share, or the tile loop over one LDS buffer of 8-byte words that serves
// every element size (8.25 KiB a workgroup: the four workgroups a CU holds at the rows body's
// register count take 33 of its 160 KiB, so the buffer costs the rows fields no occupancy,
// DESIGN §4).  A ragged batch whose partition is in HBM adds one workgroup in front of the
// fields' (w < wg_begin[0]): it scans the partition into the sample's offsets through the first
// 4 KiB of the same buffer.  The fields of a take run the taken body (kRowsTaken: the rows body
// reading row index[i] for row i, zeros where the word is not a row), a branch that is uniform
// over the workgroup like the other two.
static_assert(gather::scan::kLds <= gather::tile::kLds, "the scan's rows fit the tile buffer");

// What a workgroup of a multi-field launch does, for the kernels below.  kCast 0: no cast kind;
// 1: the cast kind with float destinations only; 2: with the quantised destinations too; 3: both
// with the affine step.  With
// kCast the cast kind takes the place of the scan share and the taken kind, which no cast plan has: with all of them
// in one kernel the compiler no longer follows every read back to the by-value arguments and
// keeps a copy of the 2.3 KB in scratch.
template <int kCast>
__device__ __forceinline__ void struct_share(const gather::multi::Args& a, uint64_t* lds) {
  const uint32_t w = blockIdx.x;
  if constexpr (!kCast) {
    if (w < a.wg_begin[0]) {
      scan_share(a.scan, lds, a.lookup);
      return;
    }
  }
  const int k = gather::multi::field_of(a, w);
  const gather::multi::Field& f = a.f[k];
  const uint64_t local = w - a.wg_begin[k], share = a.wg_begin[k + 1] - a.wg_begin[k];
  if (f.kind == gather::multi::kRows) {
    GatherMem m{f.rows.src, f.rows.dst};
    gather::gather_lane(f.rows, local * gather::kThreads + threadIdx.x, share * gather::kThreads, m);
    return;
  }
  if constexpr (!kCast) {
    if (f.kind == gather::multi::kRowsTaken) {
      TakeMem m{{f.taken.g.src, f.taken.g.dst}, a.take.src, a.take.wide};
      gather::take::take_lane(f.taken, a.take, local * gather::kThreads + threadIdx.x,
                              share * gather::kThreads, m);
      return;
    }
  }
  if constexpr (kCast) {
    if (f.kind == gather::multi::kRowsCast) {
      // (a copy of its own: the body reads its arguments in more places than the compiler
      // follows back to the kernel's by-value arguments, which it would then keep in scratch)
      const gather::cast::Args c = f.cast;
      CastMem m{c.g.src, c.g.dst};
      if constexpr (kCast == 1)
        gather::cast::cast_lane_float(c, local * gather::kThreads + threadIdx.x,
                                      share * gather::kThreads, m);
      else if constexpr (kCast == 3)
        gather::cast::cast_lane_affine(c, local * gather::kThreads + threadIdx.x,
                                       share * gather::kThreads, m);
      else
        gather::cast::cast_lane(c, local * gather::kThreads + threadIdx.x,
                                share * gather::kThreads, m);
      return;
    }
  }
  switch (f.tile.elem) {
    case 1: tile_loop(f.tile, local, share, reinterpret_cast<uint8_t*>(lds)); break;
    case 2: tile_loop(f.tile, local, share, reinterpret_cast<uint16_t*>(lds)); break;
    case 4: tile_loop(f.tile, local, share, reinterpret_cast<uint32_t*>(lds)); break;
    default: tile_loop(f.tile, local, share, lds); break;
  }
}

__global__ __launch_bounds__(gather::kThreads) void gather_struct_kernel(gather::multi::Args a) {
  __shared__ uint64_t lds[gather::tile::kLds];
  struct_share<0>(a, lds);
}

// gather_cast_kernel: the fields of a cast plan in one launch: the same body with the cast kind
// enabled, so a record that mixes converted and plain fields is still one launch, the plain ones
// through their usual rows or tile body.
__global__ __launch_bounds__(gather::kThreads) void gather_cast_kernel(gather::multi::Args a) {
  __shared__ uint64_t lds[gather::tile::kLds];
  struct_share<1>(a, lds);
}

// gather_quant_kernel: the same for a plan with a quantised field (integer destinations; its cast
// fields to float16 / float32 run here too).  In one kernel with the float destinations the body
// kept its 97 VGPRs, no scratch and four waves a SIMD but spilled 106 SGPRs into VGPR lanes
// instead of 49: a kernel of its own, chosen per plan, leaves the float casts the
// code they had.
__global__ __launch_bounds__(gather::kThreads) void gather_quant_kernel(gather::multi::Args a) {
  __shared__ uint64_t lds[gather::tile::kLds];
  struct_share<2>(a, lds);
}

// gather_affine_kernel: the same for a plan in which any converted field has a bias or a
// per-channel table (y = x * S[c] + B[c], cast_device.h): every converted field of such a plan
// runs the body with the affine step, float and integer destinations alike; the other two
// kernels hold no line of it.  One kernel, not a float and an integer one as for the plain
// conversions: it keeps 97 VGPRs, no scratch and four waves a SIMD with 152 SGPRs spilt into
// VGPR lanes, while the float destinations on their own spilt 85 SGPRs but took 20 bytes of
// scratch a lane.
__global__ __launch_bounds__(gather::kThreads) void gather_affine_kernel(gather::multi::Args a) {
  __shared__ uint64_t lds[gather::tile::kLds];
  struct_share<3>(a, lds);
}

// The reduce bodies' memory, conversions and lane exchange (reduce_device.h): the cast body's
// policy — a unit's contiguous candidates in naturally aligned non-temporal vector loads,
// elements of permuted lines with plain cached loads, the sample with the pack's write-through
// stores — plus the wave body's coalesced element loads, non-temporal like the vector loads (each
// candidate is read once), index elements of 8 bytes, and the butterfly's exchange: the pair of
// lane l ^ d, three 32-bit lane permutes.
struct ReduceMem : CastMem {
  template <int S>
  __device__ __forceinline__ uint32_t load_stream(int64_t s) const {
    const uint8_t* p = src + s;
    if constexpr (S == 4) return __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p));
    else if constexpr (S == 2) return __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p));
    else return __builtin_nontemporal_load(p);
  }
  template <int D>
  __device__ __forceinline__ void store_index(uint64_t e, uint64_t i) const {
    if constexpr (D == 8) {
      __builtin_nontemporal_store(i, reinterpret_cast<uint64_t*>(dst) + e);
    } else {
      store_elem<D>(e, static_cast<uint32_t>(i));
    }
  }
  __device__ __forceinline__ gather::reduce::Pair lane_xor(const gather::reduce::Pair& p,
                                                           int d) const {
    gather::reduce::Pair o;
    o.v = __shfl_xor(p.v, d, gather::reduce::kWave);
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(p.i), d, gather::reduce::kWave);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(p.i >> 32), d, gather::reduce::kWave);
    o.i = (static_cast<uint64_t>(hi) << 32) | lo;
    return o;
  }
};

// What a workgroup of gather_reduce_kernel does: struct_share's walk to its field, then the
// field's body over the field's share of the grid: the rows or the tile body of a plain field, the
// lane or the wave body of a reduced one (a branch uniform over the workgroup; the wave body's
// lanes are numbered so that a wave is 64 consecutive ones).  No scan, taken or cast share.
__device__ __forceinline__ void reduce_share(const gather::multi::Args& a, uint64_t* lds) {
  const uint32_t w = blockIdx.x;
  const int k = gather::multi::field_of(a, w);
  const gather::multi::Field& f = a.f[k];
  const uint64_t local = w - a.wg_begin[k], share = a.wg_begin[k + 1] - a.wg_begin[k];
  const uint64_t lane = local * gather::kThreads + threadIdx.x, lanes = share * gather::kThreads;
  if (f.kind == gather::multi::kRows) {
    GatherMem m{f.rows.src, f.rows.dst};
    gather::gather_lane(f.rows, lane, lanes, m);
    return;
  }
  if (f.kind == gather::multi::kReduceLane || f.kind == gather::multi::kReduceWave) {
    // (a copy of its own, as the cast body's arguments are)
    const gather::reduce::Args r = f.reduce;
    ReduceMem m{{r.g.src, r.g.dst}};
    if (f.kind == gather::multi::kReduceLane) gather::reduce::reduce_lane(r, lane, lanes, m);
    else gather::reduce::reduce_wave(r, lane, lanes, m);
    return;
  }
  switch (f.tile.elem) {
    case 1: tile_loop(f.tile, local, share, reinterpret_cast<uint8_t*>(lds)); break;
    case 2: tile_loop(f.tile, local, share, reinterpret_cast<uint16_t*>(lds)); break;
    case 4: tile_loop(f.tile, local, share, reinterpret_cast<uint32_t*>(lds)); break;
    default: tile_loop(f.tile, local, share, lds); break;
  }
}

// gather_reduce_kernel: the fields of a reduce plan in one launch: reduced fields through the
// lane or the wave body (reduce_device.h), plain ones through their usual rows or tile body.
// Chosen per plan, so the other kernels hold no line of it.
__global__ __launch_bounds__(gather::kThreads) void gather_reduce_kernel(gather::multi::Args a) {
  __shared__ uint64_t lds[gather::tile::kLds];
  reduce_share(a, lds);
}

// The resize body's memory and arithmetic (resize_device.h): the cast body's policy — taps with
// plain cached loads, one naturally aligned element each (neighbouring outputs read the same taps
// again), products and sums opaque so that none is contracted, the sample with the pack's
// write-through stores — plus a weight: the quotient of two exact integers, the compiler's
// correctly rounded float32 division (no build flag relaxes it).
struct ResizeMem : CastMem {
  __device__ __forceinline__ float ratio(uint32_t r, uint32_t d) const {
    return static_cast<float>(r) / static_cast<float>(d);
  }
};

// What a workgroup of gather_resize_kernel does: struct_share's walk to its field, then the
// field's body over the field's share of the grid: the rows or the tile body of a plain field, the
// resize body of a resized one (a branch uniform over the workgroup).  No scan, taken, cast or
// reduce share.
__device__ __forceinline__ void resize_share(const gather::multi::Args& a, uint64_t* lds) {
  const uint32_t w = blockIdx.x;
  const int k = gather::multi::field_of(a, w);
  const gather::multi::Field& f = a.f[k];
  const uint64_t local = w - a.wg_begin[k], share = a.wg_begin[k + 1] - a.wg_begin[k];
  const uint64_t lane = local * gather::kThreads + threadIdx.x, lanes = share * gather::kThreads;
  if (f.kind == gather::multi::kRows) {
    GatherMem m{f.rows.src, f.rows.dst};
    gather::gather_lane(f.rows, lane, lanes, m);
    return;
  }
  if (f.kind == gather::multi::kResize) {
    // (a copy of its own, as the cast body's arguments are)
    const gather::resize::Args r = f.resize;
    ResizeMem m{{r.g.src, r.g.dst}};
    gather::resize::resize_lane(r, lane, lanes, m);
    return;
  }
  switch (f.tile.elem) {
    case 1: tile_loop(f.tile, local, share, reinterpret_cast<uint8_t*>(lds)); break;
    case 2: tile_loop(f.tile, local, share, reinterpret_cast<uint16_t*>(lds)); break;
    case 4: tile_loop(f.tile, local, share, reinterpret_cast<uint32_t*>(lds)); break;
    default: tile_loop(f.tile, local, share, lds); break;
  }
}

// gather_resize_kernel: the fields of a resize plan in one launch: resized fields through the
// resize body (resize_device.h), plain ones through their usual rows or tile body.  Chosen per
// plan, so the other kernels hold no line of it.
__global__ __launch_bounds__(gather::kThreads) void gather_resize_kernel(gather::multi::Args a) {
  __shared__ uint64_t lds[gather::tile::kLds];
  resize_share(a, lds);
}

// The crop body's memory and arithmetic (crop_device.h): the resize body's policy plus a word of
// the boxes, a plain cached load of an aligned dword — the lanes of a wave read the same few rows,
// and a lane reads a row again for every unit it owns.
struct CropMem : ResizeMem {
  const uint8_t* boxes;
  __device__ __forceinline__ int32_t load_box(int64_t at) const {
    return *reinterpret_cast<const int32_t*>(boxes + at);
  }
};

// What a workgroup of gather_crop_kernel does: struct_share's walk to its field, then the field's
// body over the field's share of the grid: the rows or the tile body of a plain field, the crop
// body of a field of crops (a branch uniform over the workgroup).  No scan, taken, cast, reduce or
// resize share.
__device__ __forceinline__ void crop_share(const gather::multi::Args& a, uint64_t* lds) {
  const uint32_t w = blockIdx.x;
  const int k = gather::multi::field_of(a, w);
  const gather::multi::Field& f = a.f[k];
  const uint64_t local = w - a.wg_begin[k], share = a.wg_begin[k + 1] - a.wg_begin[k];
  const uint64_t lane = local * gather::kThreads + threadIdx.x, lanes = share * gather::kThreads;
  if (f.kind == gather::multi::kRows) {
    GatherMem m{f.rows.src, f.rows.dst};
    gather::gather_lane(f.rows, lane, lanes, m);
    return;
  }
  if (f.kind == gather::multi::kCrop) {
    // (a copy of its own, as the cast body's arguments are)
    const gather::crop::Args c = f.crop;
    CropMem m{{{c.r.g.src, c.r.g.dst}}, c.boxes};
    gather::crop::crop_lane(c, lane, lanes, m);
    return;
  }
  switch (f.tile.elem) {
    case 1: tile_loop(f.tile, local, share, reinterpret_cast<uint8_t*>(lds)); break;
    case 2: tile_loop(f.tile, local, share, reinterpret_cast<uint16_t*>(lds)); break;
    case 4: tile_loop(f.tile, local, share, reinterpret_cast<uint32_t*>(lds)); break;
    default: tile_loop(f.tile, local, share, lds); break;
  }
}

// gather_crop_kernel: the fields of a crop plan in one launch: fields of crops through the crop
// body (crop_device.h), plain ones through their usual rows or tile body.  Chosen per plan, so the
// other kernels hold no line of it.
__global__ __launch_bounds__(gather::kThreads) void gather_crop_kernel(gather::multi::Args a) {
  __shared__ uint64_t lds[gather::tile::kLds];
  crop_share(a, lds);
}

// What a workgroup of gather_resize_prep_kernel (kCrops false) or gather_crop_prep_kernel does:
// resize_share's or crop_share's walk, a resized field or a field of crops through its body with
// the model-input step of the field (l.p[k], beside the fields' own arguments), every such field
// of the launch, those whose entry adds nothing included.
template <bool kCrops>
__device__ __forceinline__ void prep_share(const gather::prep::Launch& l, uint64_t* lds) {
  const gather::multi::Args& a = l.a;
  const uint32_t w = blockIdx.x;
  const int k = gather::multi::field_of(a, w);
  const gather::multi::Field& f = a.f[k];
  const uint64_t local = w - a.wg_begin[k], share = a.wg_begin[k + 1] - a.wg_begin[k];
  const uint64_t lane = local * gather::kThreads + threadIdx.x, lanes = share * gather::kThreads;
  if (f.kind == gather::multi::kRows) {
    GatherMem m{f.rows.src, f.rows.dst};
    gather::gather_lane(f.rows, lane, lanes, m);
    return;
  }
  if constexpr (kCrops) {
    if (f.kind == gather::multi::kCrop) {
      // (copies of their own, as the cast body's arguments are)
      const gather::crop::Args c = f.crop;
      const gather::prep::Args pa = l.p[k];
      CropMem m{{{c.r.g.src, c.r.g.dst}}, c.boxes};
      gather::crop::crop_lane(c, lane, lanes, m, pa);
      return;
    }
  } else {
    if (f.kind == gather::multi::kResize) {
      const gather::resize::Args r = f.resize;
      const gather::prep::Args pa = l.p[k];
      ResizeMem m{{r.g.src, r.g.dst}};
      gather::resize::resize_lane(r, lane, lanes, m, pa);
      return;
    }
  }
  switch (f.tile.elem) {
    case 1: tile_loop(f.tile, local, share, reinterpret_cast<uint8_t*>(lds)); break;
    case 2: tile_loop(f.tile, local, share, reinterpret_cast<uint16_t*>(lds)); break;
    case 4: tile_loop(f.tile, local, share, reinterpret_cast<uint32_t*>(lds)); break;
    default: tile_loop(f.tile, local, share, lds); break;
  }
}

// gather_resize_prep_kernel: the fields of a prep plan over resizes in one launch: resized fields
// through the resize body with placement and the affine step (resize_device.h under its flag),
// plain ones through their usual rows or tile body.  Chosen per plan when any field has a prep
// entry, so gather_resize_kernel holds no line of the step and keeps its code.
__global__ __launch_bounds__(gather::kThreads) void gather_resize_prep_kernel(
    gather::prep::Launch l) {
  __shared__ uint64_t lds[gather::tile::kLds];
  prep_share<false>(l, lds);
}

// gather_crop_prep_kernel: the same over crops (crop_device.h under its flag): the affine step on
// every element of a non-empty box; gather_crop_kernel keeps its code.
__global__ __launch_bounds__(gather::kThreads) void gather_crop_prep_kernel(
    gather::prep::Launch l) {
  __shared__ uint64_t lds[gather::tile::kLds];
  prep_share<true>(l, lds);
}

// The mask kernels' memory (gather_device.h mask::): the mask with one aligned 16-byte
// non-temporal load per thread (each byte is read once by each kernel) or byte by byte at its
// head and tail; the thread counts in LDS; the workspace's index, counts and totals with plain
// stores and loads, which the kernel boundary orders for the launch that follows; the sample's
// own two offsets with the pack's write-through stores.
struct MaskMem {
  const uint8_t* mask;
  const uint8_t* line;  // mask - shift: the 16-byte line the mask starts in
  uint8_t* index;
  uint8_t* counts;
  uint8_t* totals;
  uint8_t* offsets;
  uint32_t* lds;
  __device__ __forceinline__ gather::U16 load16(uint64_t v) const {
    const u32x4 x = ld16<1, false>(line + v);
    return {{x.x, x.y, x.z, x.w}};
  }
  __device__ __forceinline__ uint8_t load_byte(uint64_t row) const { return mask[row]; }
  __device__ __forceinline__ void lds_write(uint32_t i, uint32_t v) const { lds[i] = v; }
  __device__ __forceinline__ uint32_t lds_read(uint32_t i) const { return lds[i]; }
  __device__ __forceinline__ void store_index(uint64_t i, int32_t v) const {
    reinterpret_cast<int32_t*>(index)[i] = v;
  }
  __device__ __forceinline__ void store_count(uint64_t i, uint32_t v) const {
    reinterpret_cast<uint32_t*>(counts)[i] = v;
  }
  __device__ __forceinline__ void store_total(uint64_t t, uint32_t v) const {
    reinterpret_cast<uint32_t*>(totals)[t] = v;
  }
  __device__ __forceinline__ uint32_t load_total(uint64_t t) const {
    return reinterpret_cast<const uint32_t*>(totals)[t];
  }
  __device__ __forceinline__ void store_offset(uint64_t i, uint32_t v) const {
    st4<2>(offsets + 4 * i, v);
  }
};

__device__ __forceinline__ MaskMem mask_mem(const gather::mask::Args& a, uint32_t* lds) {
  return MaskMem{a.mask, a.mask - a.shift, a.index, a.counts, a.totals, a.offsets, lds};
}

// mask_count_kernel: every tile's count of selected rows into totals[tile], its index words -1.
__global__ __launch_bounds__(gather::kThreads) void mask_count_kernel(gather::mask::Args a) {
  namespace mk = gather::mask;
  __shared__ uint32_t lds[mk::kLds];
  MaskMem m = mask_mem(a, lds);
  const uint64_t nt = mk::tiles(a);
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    mk::count_load(a, t, threadIdx.x, m);
    __syncthreads();
#pragma unroll
    for (int step = 0; step < mk::kSteps; ++step) {
      mk::reduce_phase(threadIdx.x, step, m);
      __syncthreads();
    }
    mk::count_store(a, t, threadIdx.x, m);
    __syncthreads();  // slot 0 is read before the next tile's counts land
  }
}

// mask_compact_kernel: every tile's rows scanned behind the sum of the totals before it: the
// counts C and the selected rows' numbers, in source order, into the index.
__global__ __launch_bounds__(gather::kThreads) void mask_compact_kernel(gather::mask::Args a) {
  namespace mk = gather::mask;
  __shared__ uint32_t lds[mk::kLds];
  MaskMem m = mask_mem(a, lds);
  const uint64_t nt = mk::tiles(a);
  for (uint64_t t = blockIdx.x; t < nt; t += gridDim.x) {
    mk::carry_load(a, t, threadIdx.x, m);
    __syncthreads();
#pragma unroll
    for (int step = 0; step < mk::kSteps; ++step) {
      mk::reduce_phase(threadIdx.x, step, m);
      __syncthreads();
    }
    const uint32_t carry = mk::carry_read(m);
    __syncthreads();
    const uint32_t f = mk::scan_load(a, t, threadIdx.x, m);
    __syncthreads();
#pragma unroll
    for (int step = 0; step < mk::kSteps; ++step) {
      mk::scan_step(threadIdx.x, step, m);
      __syncthreads();
    }
    mk::scan_store(a, t, threadIdx.x, f, carry, m);
    __syncthreads();
  }
}

unsigned grid_for(uint64_t items) {
  uint64_t g = (items + kThreads - 1) / kThreads;
  return static_cast<unsigned>(std::max<uint64_t>(1, std::min<uint64_t>(g, 4096)));
}

}  // namespace

// Boundary units written whole (PackArgsT::edge_mask) for one launch holding every segment of
// its plan: a segment's unaligned head / tail unit is stitched when it lies inside the writable
// destination [dst, dst + cap).  Segments must be sorted by destination offset and disjoint, as
// plans are (else nothing is stitched), so every byte of such a unit belongs to a segment of
// this launch or is padding.  cap 0 (unknown extent, host destinations): nothing is stitched.
uint64_t edge_mask(const Segment* segs, size_t n, const uint8_t* dst, uint64_t cap) {
  if (!cap || n > 32) return 0;
  for (size_t k = 1; k < n; ++k)
    if (segs[k].dst_off < segs[k - 1].dst_off + segs[k - 1].len) return 0;
  const uint64_t base = reinterpret_cast<uintptr_t>(dst);
  auto inside = [&](uint64_t unit) { return unit >= base && unit + 16 <= base + cap; };
  // The kernel leaves a stitched head unit to the lowest segment holding a byte of it
  // (pack_chunk own_head), and that segment takes the unit only if seg[j - 1] ends before it.  An
  // empty seg[j - 1] that starts inside the unit hides the owner from that rule: nobody would
  // write the unit, so no head in it is stitched (its bytes are stored one by one).  Plans drop
  // empty segments or are empty altogether; raw segment lists need not.
  auto hidden = [&](size_t k, uint64_t unit) {
    size_t j = k;  // the lowest non-empty segment holding a byte of the unit
    for (size_t p = k; p-- > 0;) {
      if (!segs[p].len) continue;
      if (base + segs[p].dst_off + segs[p].len <= unit) break;
      j = p;
    }
    // a segment that starts before the unit (or on it) writes it as its tail or body
    return base + segs[j].dst_off > unit && j > 0 && segs[j - 1].len == 0 &&
           base + segs[j - 1].dst_off > unit;
  };
  uint64_t mask = 0;
  for (size_t k = 0; k < n; ++k) {
    const uint64_t d0 = base + segs[k].dst_off, d1 = d0 + segs[k].len;
    if (d1 == d0) continue;
    const uint64_t A0 = (d0 + 15) & ~uint64_t(15);
    if (A0 > d0 && inside(A0 - 16) && !hidden(k, A0 - 16)) mask |= uint64_t(1) << (2 * k);
    if (A0 < d1 && (d1 & 15) && inside(d1 & ~uint64_t(15))) mask |= uint64_t(2) << (2 * k);
  }
  return mask;
}

// The chunk size a message's pack would use on its own (a batch holds messages of one size).
uint32_t aql_chunk_bytes(const Segment* segs, size_t n) {
  uint64_t body = 0;
  for (size_t k = 0; k < n; ++k) body += segs[k].len;
  return choose_chunk_bytes(body);  // the AQL kernels keep 4 loads in flight per lane
}

namespace {

// Who reports a launch's fill: nobody (a pack that is not its plan's last launch), the kernel
// (fill flag and done words) or the command processor (the dispatch's completion signal).
enum class Signal { kNone, kInKernel, kCp };

// Workgroups of a pack of `chunks` chunks: the grid policy, here alone.  Unsignalled: one per
// chunk.  In-kernel signals: the signalling grid (kSignalGrid).  Signalled by the command
// processor: nothing to poll, so up to kCpGrid workgroups for the single-segment kernels — a lone
// 40.96 MB pack capped at 1024 keeps 8 MiB in flight, half of what HBM needs — and
// kCpGridMulti for the multi-segment kernel.
uint32_t pack_grid(uint32_t chunks, Signal how, bool single) {
  const uint32_t cap = how == Signal::kInKernel ? kSignalGrid
                       : how == Signal::kCp     ? (single ? kCpGrid : kCpGridMulti)
                                                : chunks;
  return std::min(chunks, cap);
}

void set_segs(PackSeg* out, const Segment* segs, size_t n) {
  for (size_t k = 0; k < n; ++k)
    out[k] = {static_cast<const uint8_t*>(segs[k].src), segs[k].dst_off, segs[k].len};
}

// The head every pack's arguments share (PackArgsT<N>, AqlBatchArgs), filled here alone from
// a.seg[0 .. nseg): destination, signal, chunk layout (pack_device.h chunk_layout) and grid.
template <class A>
int finish_args(A& a, uint8_t* dst, const FillSignal& sig, size_t nseg, uint32_t chunk_bytes,
                uint64_t edge, Signal how, bool single) {
  a.dst = dst;
  a.flag = sig.flag;
  a.done = sig.done;
  a.epoch = sig.epoch;
  a.nseg = static_cast<uint32_t>(nseg);
  a.chunk_bytes = chunk_bytes;
  a.edge_mask = edge;
  a.n_chunks = chunk_layout(reinterpret_cast<uintptr_t>(dst), a.seg, a.nseg, chunk_bytes,
                            a.chunk_end);
  if (!a.n_chunks) return fail(DORA_ERR_INVALID, "pack: too many chunks");
  a.grid = pack_grid(a.n_chunks, how, single);
  return DORA_OK;
}

}  // namespace

// finish_args by argument type, for the pack probe of the testing library
// (testing/pack_probe.hip): `signals` selects the in-kernel signal's grid, else one workgroup per
// chunk.
int finish_pack_args(PackArgs& a, uint8_t* dst, const FillSignal& sig, size_t nseg,
                     uint32_t chunk_bytes, uint64_t edge, bool signals) {
  return finish_args(a, dst, sig, nseg, chunk_bytes, edge,
                     signals ? Signal::kInKernel : Signal::kNone, nseg == 1);
}
int finish_aql_args(AqlPackArgs& a, uint8_t* dst, const FillSignal& sig, size_t nseg,
                    uint32_t chunk_bytes, uint64_t edge, bool signals) {
  return finish_args(a, dst, sig, nseg, chunk_bytes, edge,
                     signals ? Signal::kInKernel : Signal::kNone, false);
}
int finish_batch_args(AqlBatchArgs& a, uint8_t* dst, const FillSignal& sig, size_t nseg,
                      uint32_t chunk_bytes, uint64_t edge, bool signals) {
  return finish_args(a, dst, sig, nseg, chunk_bytes, edge,
                     signals ? Signal::kInKernel : Signal::kNone, false);
}

namespace {

// One kernel launch on `stream`, timed or not: with an event it is the extended launch, whose
// dispatch packet stamps the kernel's begin into `ev_start` and its end into `ev_stop` (either
// may be null).
template <class A>
int launch_timed(void (*kern)(A), unsigned grid, unsigned block, hipStream_t stream,
                 hipEvent_t ev_start, hipEvent_t ev_stop, const A& a) {
  if (ev_start || ev_stop) {
    hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, stream, ev_start, ev_stop, 0, a);
  } else {
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, stream, a);
  }
  DORA_HIP(hipGetLastError());
  return DORA_OK;
}

}  // namespace

// Launch the pack of `n` segments into `dst` (device).  Copy segments with device sources go
// to pack_kernel in batches of kMaxSegs, transform segments (compacting plans) to
// transform_kernel; host sources are DMA'd with hipMemcpyAsync.  With timing events
// (launch_timed) the first kernel's begin is stamped into `ev_start` and the last kernel's end
// into `ev_stop`.
int launch_pack(const Segment* segs_in, size_t n_in, ArrowDeviceType dev, uint8_t* dst,
                hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop,
                const FillSignal* signal, bool* signalled, uint64_t dst_cap) {
  if (signalled) *signalled = false;
  bool any_x = false;
  for (size_t i = 0; i < n_in; ++i) any_x |= segs_in[i].op != SEG_COPY;
  if (dev == ARROW_DEVICE_CPU) {
    if (any_x) return fail(DORA_ERR_UNSUPPORTED, "compacting plans need device-resident arrays");
    for (size_t i = 0; i < n_in; ++i)
      DORA_HIP(hipMemcpyAsync(dst + segs_in[i].dst_off, segs_in[i].src, segs_in[i].len,
                              hipMemcpyHostToDevice, stream));
    return DORA_OK;
  }
  std::vector<Segment> copies, xforms;
  const Segment* segs = segs_in;
  size_t n = n_in;
  if (any_x) {
    for (size_t i = 0; i < n_in; ++i) (segs_in[i].op == SEG_COPY ? copies : xforms).push_back(segs_in[i]);
    segs = copies.data();
    n = copies.size();
  }
  const size_t n_launch_x = (xforms.size() + kMaxSegs - 1) / kMaxSegs;
  size_t launch = 0;
  const size_t n_launch = (n + kMaxSegs - 1) / kMaxSegs + n_launch_x;
  size_t i = 0;
  while (i < n) {
    PackArgs a;
    std::memset(&a, 0, sizeof(a));
    const size_t m = std::min<size_t>(kMaxSegs, n - i);
    const bool first = launch == 0, last = launch + 1 == n_launch;
    // the signalling launch: write-through stores, the signalling grid
    const bool signals = last && signal;
    // one launch holding the whole plan: its boundary units may be written whole
    const uint64_t edge = !any_x && m == n ? edge_mask(segs, n, dst, dst_cap) : 0;
    set_segs(a.seg, segs + i, m);
    const int rc = finish_args(a, dst, signals ? *signal : FillSignal{}, m,
                               aql_chunk_bytes(segs + i, m), edge,
                               signals ? Signal::kInKernel : Signal::kNone, m == 1);
    if (rc != DORA_OK) return rc;
    void (*kern)(PackArgs) = signals ? pack_kernel<kUnroll, 2> : pack_kernel<kUnroll, 1>;
    const int rl = launch_timed(kern, a.grid, kThreads, stream, first ? ev_start : nullptr,
                                last ? ev_stop : nullptr, a);
    if (rl != DORA_OK) return rl;
    if (a.flag && signalled) *signalled = true;
    i += m;
    ++launch;
  }
  for (size_t j = 0; j < xforms.size(); j += kMaxSegs) {
    XArgs x;
    std::memset(&x, 0, sizeof(x));
    const size_t m = std::min<size_t>(kMaxSegs, xforms.size() - j);
    const uint32_t blocks = fill_xargs(x, dst, xforms.data() + j, m);
    if (!blocks) return fail(DORA_ERR_INVALID, "pack: too many blocks");
    const bool first = launch == 0, last = launch + 1 == n_launch;
    const int rl = launch_timed(transform_kernel, blocks, kThreads, stream,
                                first ? ev_start : nullptr, last ? ev_stop : nullptr, x);
    if (rl != DORA_OK) return rl;
    ++launch;
  }
  return DORA_OK;
}

// A device tensor view is read only after the runtime has named the allocation that holds it:
// the strides come from the caller, and a read outside mapped memory faults the whole GPU.
int check_device_range(const GatherDesc& g, int device) {
  const uintptr_t base = reinterpret_cast<uintptr_t>(g.view.src);
  // the first and last byte read, as addresses (no wrap-around)
  uintptr_t first, last;
  const uintptr_t below = uintptr_t(0) - static_cast<uintptr_t>(g.lo);  // -lo, lo <= 0
  if (g.lo > 0 || g.hi < 0 || __builtin_sub_overflow(base, below, &first) ||
      __builtin_add_overflow(base, static_cast<uintptr_t>(g.hi), &last))
    return fail(DORA_ERR_INVALID, "tensor view [%lld, %lld] from %p wraps the address space",
                (long long)g.lo, (long long)g.hi, (const void*)g.view.src);
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  hipError_t e = hipPointerGetAttributes(&at, g.view.src);
  if (e != hipSuccess || at.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return fail(DORA_ERR_INVALID, "tensor data %p was declared device memory but the runtime "
                "knows it as %s", (const void*)g.view.src,
                e != hipSuccess ? "no allocation of its own"
                                : at.type == hipMemoryTypeHost ? "host memory" : "another kind");
  }
  if (device >= 0 && at.device != device)
    return fail(DORA_ERR_INVALID, "tensor data %p is on GPU %d, not on this node's GPU %d",
                (const void*)g.view.src, at.device, device);
  hipDeviceptr_t ab = nullptr;
  size_t asz = 0;
  e = hipMemGetAddressRange(&ab, &asz, const_cast<uint8_t*>(g.view.src));
  if (e != hipSuccess || !asz) {
    (void)hipGetLastError();
    return fail(DORA_ERR_INVALID, "the runtime cannot name the allocation that holds tensor "
                "data %p (%s)", (const void*)g.view.src, hipGetErrorString(e));
  }
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(ab), a1 = a0 + (asz - 1);  // closed
  if (first < a0 || last > a1)
    return fail(DORA_ERR_INVALID, "tensor view reaches bytes [%p, %p], outside its allocation "
                "[%p, %p]: nothing was launched", (const void*)first, (const void*)last,
                (const void*)a0, (const void*)a1);
  return DORA_OK;
}

namespace {

// check_device_range of one thing a plan reads, a refusal naming it in front.
int check_named(const GatherDesc& g, int device, const char* what) {
  const int rc = check_device_range(g, device);
  if (rc == DORA_OK) return rc;
  const std::string why = dora_gpu_last_error();
  return fail(rc, "%s: %s", what, why.c_str());
}

}  // namespace

// By launch kind, in one order: partition, mask, index, fields, the single view.
int check_plan_range(const dora_plan& plan, int device) {
  const PlanLaunch kind = plan.launch;
  if (plan.scan_in_hbm() && plan.scan.count) {  // its words like any field
    const int rc = check_named(scan_reach(plan.scan), device, "partition");
    if (rc != DORA_OK) return rc;
  }
  if (kind == PlanLaunch::kMasked) {  // a mask in HBM: its N bytes like any field
    const int rc = check_named(mask_reach(plan.mask), device, "mask");
    if (rc != DORA_OK) return rc;
  }
  if (kind == PlanLaunch::kTaken && plan.take.count) {  // a take's index in HBM: its words
    const int rc = check_named(take_reach(plan.take), device, "index");
    if (rc != DORA_OK) return rc;
    if (plan.take.n == 0) return DORA_OK;  // rows of zeros: no field is read
  }
  for (size_t k = 0; k < plan.fields.size(); ++k) {
    const CastDesc& c = plan.fields[k].cast;
    int rc = check_device_range(plan.fields[k].gd, device);
    const char* what = "";
    // an affine field's tables in HBM: their `channels` words like a take's index
    if (rc == DORA_OK && kind == PlanLaunch::kCast && c.on && c.scale_tab) {
      rc = check_device_range(table_reach(c.scale_tab, c.channels), device);
      what = "scale table: ";
    }
    if (rc == DORA_OK && kind == PlanLaunch::kCast && c.on && c.bias_tab) {
      rc = check_device_range(table_reach(c.bias_tab, c.channels), device);
      what = "bias table: ";
    }
    // a model-input field's tables in HBM, the same
    const PrepDesc& pd = plan.fields[k].prep;
    const bool prepped = kind == PlanLaunch::kResizePrep || kind == PlanLaunch::kCropPrep;
    if (rc == DORA_OK && prepped && pd.on && pd.scale_tab) {
      rc = check_device_range(table_reach(pd.scale_tab, pd.channels), device);
      what = "scale table: ";
    }
    if (rc == DORA_OK && prepped && pd.on && pd.bias_tab) {
      rc = check_device_range(table_reach(pd.bias_tab, pd.channels), device);
      what = "bias table: ";
    }
    // a crops field's boxes in HBM: their 16 * K bytes like a take's index
    if (rc == DORA_OK && crops(kind) && plan.fields[k].crop.on) {
      rc = check_device_range(crop_reach(plan.fields[k].crop), device);
      what = "boxes: ";
    }
    if (rc == DORA_OK) continue;
    const std::string why = dora_gpu_last_error();
    return fail(rc, "field %zu `%s`: %s%s", k, plan.fields[k].name.c_str(), what, why.c_str());
  }
  // a bare tensor: strided (kView), or dense and copied by `segs`
  const bool one_view = kind == PlanLaunch::kView ||
                        (kind == PlanLaunch::kSegments && plan.fields.empty());
  return one_view ? check_device_range(plan.gd, device) : DORA_OK;
}

// Which kernel gathers `g` into `dst`, stated once.  The tiled transpose, where it applies
// (tile::contiguous_dim: a source-contiguous dimension c that is not the output's innermost
// dimension j, everything element-aligned), when c is at least kTileMinC elements long and a row
// of the output along j at least kTileMinRowBytes; gather_rows_kernel for everything else:
// crops, slices, broadcasts, unaligned views, C = 3 of HWC->CHW (a 32-wide tile of it is nine
// tenths empty: 85 us against 8.7) and short output rows (NCHW->NHWC float16 with C = 64, 128-byte
// rows: 14.4 us against 10.7).  Measured rows against tile, five interleaved rounds
// (profiles/tensor_gather_kernels.jsonl): the tile wins at every other point tried,
// element sizes 1, 2, 4 and 8, c of 16 and 32 elements and 256-byte rows included.
constexpr int64_t kTileMinC = 16;
constexpr int64_t kTileMinRowBytes = 256;
std::atomic<int> g_gather_force{0};  // test hook: 1 rows, 2 tile wherever it applies

int select_tile_dim(const GatherDesc& g, const uint8_t* dst) {
  const int force = g_gather_force.load(std::memory_order_relaxed);
  if (force == 1) return -1;
  const int c = gather::tile::contiguous_dim(g, dst);
  if (c < 0 || force == 2) return c;
  const int64_t row_bytes = g.view.shape[g.view.nd - 1] * static_cast<int64_t>(g.elem);
  return g.view.shape[c] >= kTileMinC && row_bytes >= kTileMinRowBytes ? c : -1;
}

void gather_force(int mode) { g_gather_force.store(mode, std::memory_order_relaxed); }

// Test hook: launches of this process so far over the fields of a plan, by kernel:
// gather_struct_kernel, gather_cast_kernel, gather_quant_kernel, gather_affine_kernel.
std::atomic<int> g_reduce_force{0};  // test hook: 1 the lane body, 2 the wave body wherever it applies
void reduce_force(int mode) { g_reduce_force.store(mode, std::memory_order_relaxed); }

// Which body reduces field `g` by `r`, stated once: the wave body where the reduced axis is the
// source-contiguous dimension and at least reduce::kWaveMinC long, the lane body for everything
// else.
bool select_reduce_wave(const GatherDesc& g, const ReduceDesc& r) {
  const int force = g_reduce_force.load(std::memory_order_relaxed);
  if (force == 1) return false;
  if (force == 2) return gather::reduce::wave_applies(g, r);
  return gather::reduce::wave_chosen(g, r);
}

std::atomic<uint64_t> g_fields_launches[4];
void fields_launches(uint64_t out[4]) {
  for (int i = 0; i < 4; ++i) out[i] = g_fields_launches[i].load(std::memory_order_relaxed);
}

int launch_gather(const GatherDesc& g, uint8_t* dst, hipStream_t stream, hipEvent_t ev_start,
                  hipEvent_t ev_stop) {
  if (!g.view.total) return DORA_OK;
  const int c = select_tile_dim(g, dst);
  if (c >= 0) {
    const gather::tile::Args a = gather::tile::make_args(g, dst, c);
    void (*kern)(gather::tile::Args) = g.elem == 1   ? gather_tile_kernel<uint8_t>
                                       : g.elem == 2 ? gather_tile_kernel<uint16_t>
                                       : g.elem == 4 ? gather_tile_kernel<uint32_t>
                                                     : gather_tile_kernel<uint64_t>;
    return launch_timed(kern, static_cast<unsigned>(gather::tile::grid_for(a)), gather::kThreads,
                        stream, ev_start, ev_stop, a);
  }
  const gather::Args a = gather::make_args(g, dst);
  return launch_timed(gather_rows_kernel, static_cast<unsigned>(gather::grid_for(a)),
                      gather::kThreads, stream, ev_start, ev_stop, a);
}

namespace {

// What a launch of `kind` does to field `k`, `f`, held against what the kernel's body takes for
// granted — its loads whole source elements, its stores whole destination elements, every extent
// within its arithmetic.  Returns the size of the elements stored, with `*noun` what the field
// then is ("converted", "reduced", "resized", "cropped"); 0 with `*noun` NULL for a field that goes as it is;
// -1 after recording that this is not an op the kernel runs.  A new op is one more branch here.
int field_op_size(PlanLaunch kind, const PlanField& f, size_t k, const char** noun) {
  namespace gc = gather::cast;
  const uintptr_t src = reinterpret_cast<uintptr_t>(f.gd.view.src), elem_mask = f.gd.elem - 1;
  const char* op = nullptr;
  unsigned ds = 0;
  bool ok = true;
  *noun = nullptr;
  if ((resizes(kind) && f.resize.on) || (crops(kind) && f.crop.on)) {
    // (a field of crops: the same held against the output's dimensions, and its boxes)
    const bool crop = crops(kind);
    const ResizeDesc& r = crop ? f.crop.rs : f.resize;
    op = crop ? "a crop" : "a resize";
    *noun = crop ? "cropped" : "resized";
    ds = r.dst_bits / 8u;
    const bool dst_ok = r.dst_code == 2 ? ds == 2 || ds == 4
                                        : gc::dst_kind(r.dst_code, r.dst_bits) >= 0;
    ok = gc::src_kind(r.src_code, r.src_bits) >= 0 && dst_ok &&
         (r.mode == DORA_RESIZE_NEAREST || r.mode == DORA_RESIZE_BILINEAR) && r.nd >= 2 &&
         r.nd <= gather::kDims && r.ax[0] != r.ax[1] && !(src & elem_mask);
    for (int j = 0; ok && j < 2; ++j)
      ok = r.ax[j] >= 0 && r.ax[j] < r.nd && r.in[j] >= 1 &&
           r.in[j] <= int64_t(gather::resize::kMaxExtent) && r.shape[r.ax[j]] >= 1 &&
           r.shape[r.ax[j]] <= int64_t(gather::resize::kMaxExtent);
    for (int i = 0; ok && i < r.nd; ++i) ok = !(static_cast<uintptr_t>(r.stride[i]) & elem_mask);
    if (crop)
      ok = ok && f.crop.k >= 1 && f.crop.k <= kMaxCropBoxes && r.shape[0] == int64_t(f.crop.k) &&
           r.stride[0] == 0 && r.ax[0] >= 1 && r.ax[1] >= 1 && f.crop.boxes &&
           !(reinterpret_cast<uintptr_t>(f.crop.boxes) & 3);
    // (the model-input step: the image inside the output, the tables' axis a kept dimension of
    // as many steps as the tables have words, the tables whole dwords)
    const PrepDesc& d = f.prep;
    if (ok && d.on && d.placed) {
      ok = !crop;
      for (int j = 0; ok && j < 2; ++j)
        ok = d.inner[j] >= 1 && d.lead[j] >= 0 && d.inner[j] + d.lead[j] <= r.shape[r.ax[j]];
    }
    if (ok && d.on && (d.scale_tab || d.bias_tab))
      ok = d.axis >= 0 && d.axis < r.nd && d.axis != r.ax[0] && d.axis != r.ax[1] &&
           r.shape[d.axis] == int64_t(d.channels) &&
           !((reinterpret_cast<uintptr_t>(d.scale_tab) | reinterpret_cast<uintptr_t>(d.bias_tab)) & 3);
  } else if (kind == PlanLaunch::kReduce && f.reduce.on) {
    const ReduceDesc& r = f.reduce;
    op = "a reduction";
    *noun = "reduced";
    ds = gather::reduce::index_size(r.idx_code, r.idx_bits);
    ok = gc::src_kind(r.src_code, r.src_bits) >= 0 && ds && r.c &&
         !((src | static_cast<uintptr_t>(r.cstride)) & elem_mask);
  } else if (kind == PlanLaunch::kCast && f.cast.on) {
    // (the cast body's stores are whole elements and whole 16-byte units of them)
    const CastDesc& c = f.cast;
    op = "a cast";
    *noun = "converted";
    ds = c.dst_bits / 8u;
    const bool dst_ok = c.quant() ? gc::dst_kind(c.dst_code, c.dst_bits) >= 0 : ds == 2 || ds == 4;
    ok = gc::src_kind(c.src_code, c.src_bits) >= 0 && dst_ok && !(src & elem_mask);
  }
  if (ok) return static_cast<int>(ds);
  fail(DORA_ERR_INVALID, "field %zu `%s`: not %s this kernel runs", k, f.name.c_str(), op);
  return -1;
}

// One launch over fields[0..n) of a plan of `kind` into `dst + dst_off`: the fields marshalled
// into gather::multi::Args and the kernel chosen, here alone.
//   kFields: each field as it would go on its own (select_tile_dim), gather_struct_kernel.
//   kCast: the same, a converted field through the cast body; gather_cast_kernel, or
//     gather_quant_kernel when any field is quantised, or gather_affine_kernel when any has a
//     bias or a per-channel table.
//   kReduce: the same, a reduced field through the lane or the wave body (select_reduce_wave);
//     gather_reduce_kernel.
//   kResize: the same, a resized field through the resize body; gather_resize_kernel.
//   kCrop: the same, a field of crops through the crop body; gather_crop_kernel.
//   kResizePrep, kCropPrep: kResize and kCrop with the model-input step of every field beside the
//     fields (prep::Launch); gather_resize_prep_kernel, gather_crop_prep_kernel.
//   (these four: DORA_ERR_INVALID, nothing launched, when a field with an op, field_op_size,
//   would not start on a multiple of the size of the elements stored)
//   kTaken (`take` given): every field through the taken body, never a tile: row i0 of its bytes
//     is row take->src[i0] of the field, or zeros where that word is not in [0, take->n).
// With `scan` (a ragged batch's partition in HBM; n may then be 0) one more workgroup of the same
// launch writes the sample's offsets at dst + 0 (dst a whole number of dwords).  With `lookup` (a
// mask plan: scan->n + 1 int32 counts in HBM) the scan share stores lookup[o] where it would
// store the offset o.
int launch_fields(PlanLaunch kind, const PlanField* fields, size_t n, uint8_t* dst,
                  hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop,
                  const ScanDesc* scan = nullptr, const TakeDesc* take = nullptr,
                  const uint8_t* lookup = nullptr) {
  if ((n == 0 && !scan) || n > size_t(gather::multi::kMaxFields))
    return fail(DORA_ERR_INVALID, "gather of %zu struct fields", n);
  if (scan && (scan->count > kMaxScanEntries || (reinterpret_cast<uintptr_t>(dst) & 3) ||
               (scan->count && (reinterpret_cast<uintptr_t>(scan->src) & (scan->wide ? 7u : 3u)))))
    return fail(DORA_ERR_INVALID, "scan of %llu words into %p: at most %llu words, offsets and "
                "words aligned", static_cast<unsigned long long>(scan->count),
                static_cast<void*>(dst), static_cast<unsigned long long>(kMaxScanEntries));
  if (take && n && (!take->count || (reinterpret_cast<uintptr_t>(take->src) & (take->wide ? 7u : 3u))))
    return fail(DORA_ERR_INVALID, "take of %llu rows by the index at %p: at least one word, "
                "words aligned", static_cast<unsigned long long>(take->count),
                static_cast<const void*>(take->src));
  GatherDesc g[gather::multi::kMaxFields];
  CastDesc c[gather::multi::kMaxFields];
  uint64_t off[gather::multi::kMaxFields];
  int tile_c[gather::multi::kMaxFields];
  int64_t stride0[gather::multi::kMaxFields];
  ReduceDesc rd[gather::multi::kMaxFields];
  bool wave[gather::multi::kMaxFields];
  ResizeDesc rs[gather::multi::kMaxFields];
  CropDesc cr[gather::multi::kMaxFields];
  PrepDesc pd[gather::multi::kMaxFields];
  bool quant = false, affine = false;
  for (size_t k = 0; k < n; ++k) {
    const PlanField& f = fields[k];
    if (!f.bytes) return fail(DORA_ERR_INVALID, "gather of an empty struct field");
    g[k] = f.gd;
    off[k] = f.dst_off;
    stride0[k] = f.stride0;
    c[k] = kind == PlanLaunch::kCast ? f.cast : CastDesc{};
    rd[k] = kind == PlanLaunch::kReduce ? f.reduce : ReduceDesc{};
    rs[k] = resizes(kind) ? f.resize : ResizeDesc{};
    cr[k] = crops(kind) ? f.crop : CropDesc{};
    pd[k] = f.prep;
    quant |= c[k].quant();
    const char* noun = nullptr;
    const int ds = field_op_size(kind, f, k, &noun);
    if (ds < 0) return DORA_ERR_INVALID;
    tile_c[k] = take || noun ? -1 : select_tile_dim(g[k], dst + off[k]);
    if (noun && (reinterpret_cast<uintptr_t>(dst + off[k]) & (static_cast<unsigned>(ds) - 1)))
      return fail(DORA_ERR_INVALID, "field %zu `%s`: the %s field would start at %p, not a "
                  "multiple of its %u-byte elements: nothing was launched", k, f.name.c_str(), noun,
                  static_cast<void*>(dst + off[k]), static_cast<unsigned>(ds));
    wave[k] = rd[k].on && select_reduce_wave(g[k], rd[k]);
    if (!c[k].affine()) continue;
    affine = true;
    // the channel stepping never leaves [0, channels) of a table of whole dwords
    if (!c[k].inner || !c[k].channels ||
        ((reinterpret_cast<uintptr_t>(c[k].scale_tab) | reinterpret_cast<uintptr_t>(c[k].bias_tab)) & 3))
      return fail(DORA_ERR_INVALID, "field %zu `%s`: not an affine step this kernel runs", k,
                  f.name.c_str());
  }
  namespace gm = gather::multi;
  const int nf = static_cast<int>(n);
  if (kind == PlanLaunch::kResizePrep) {
    const gather::prep::Launch l = gather::prep::make_resize_launch(g, rs, pd, off, tile_c, nf, dst);
    return launch_timed(gather_resize_prep_kernel, gm::grid_for(l.a), gather::kThreads, stream,
                        ev_start, ev_stop, l);
  }
  if (kind == PlanLaunch::kCropPrep) {
    const gather::prep::Launch l = gather::prep::make_crop_launch(g, cr, pd, off, tile_c, nf, dst);
    return launch_timed(gather_crop_prep_kernel, gm::grid_for(l.a), gather::kThreads, stream,
                        ev_start, ev_stop, l);
  }
  gm::Args a = take                        ? gm::make_taken_args(g, stride0, off, nf, dst, *take, scan)
               : kind == PlanLaunch::kCast ? gm::make_cast_args(g, c, off, tile_c, nf, dst)
               : kind == PlanLaunch::kReduce
                   ? gm::make_reduce_args(g, rd, wave, off, tile_c, nf, dst)
               : kind == PlanLaunch::kResize
                   ? gm::make_resize_args(g, rs, off, tile_c, nf, dst)
               : kind == PlanLaunch::kCrop
                   ? gm::make_crop_args(g, cr, off, tile_c, nf, dst)
                   : gm::make_args(g, off, tile_c, nf, dst, scan);
  a.lookup = lookup;
  if (kind == PlanLaunch::kCrop)
    return launch_timed(gather_crop_kernel, gm::grid_for(a), gather::kThreads, stream, ev_start,
                        ev_stop, a);
  if (kind == PlanLaunch::kResize)
    return launch_timed(gather_resize_kernel, gm::grid_for(a), gather::kThreads, stream, ev_start,
                        ev_stop, a);
  if (kind == PlanLaunch::kReduce)
    return launch_timed(gather_reduce_kernel, gm::grid_for(a), gather::kThreads, stream, ev_start,
                        ev_stop, a);
  const int which = kind != PlanLaunch::kCast ? 0 : affine ? 3 : quant ? 2 : 1;
  void (*const kerns[4])(gm::Args) = {gather_struct_kernel, gather_cast_kernel,
                                      gather_quant_kernel, gather_affine_kernel};
  void (*kern)(gm::Args) = kerns[which];
  g_fields_launches[which].fetch_add(1, std::memory_order_relaxed);
  return launch_timed(kern, gm::grid_for(a), gather::kThreads, stream, ev_start, ev_stop, a);
}

}  // namespace

uint64_t plan_workspace(const dora_plan& plan) {
  if (plan.launch != PlanLaunch::kMasked) return 0;
  return gather::mask::workspace(plan.size, plan.mask.n, plan.mask.part_words).end - plan.size;
}

namespace {

// A mask plan's three launches on `stream`: count, compact, then the fields through the taken
// body by the workspace's index (with the scan share when the message has a partition, its words
// looked up in C).  The workspace follows the sample in `dst` (mask::workspace).
int launch_mask(const dora_plan& plan, uint8_t* dst, hipStream_t stream, hipEvent_t ev_start,
                hipEvent_t ev_stop) {
  namespace mk = gather::mask;
  const MaskDesc& md = plan.mask;
  if (!md.n || md.n > mk::kMaxRows || (reinterpret_cast<uintptr_t>(dst) & 3))
    return fail(DORA_ERR_INVALID, "mask of %llu rows into %p: 1 to %llu rows, the sample on a "
                "multiple of 4", static_cast<unsigned long long>(md.n), static_cast<void*>(dst),
                static_cast<unsigned long long>(mk::kMaxRows));
  const mk::Workspace w = mk::workspace(plan.size, md.n, md.part_words);
  const mk::Args a = mk::make_args(md.src, md.n, dst, w, !plan.scan_on);
  const unsigned grid = static_cast<unsigned>(mk::tiles(a));
  int rc = launch_timed(mask_count_kernel, grid, gather::kThreads, stream, ev_start, nullptr, a);
  if (rc != DORA_OK) return rc;
  rc = launch_timed(mask_compact_kernel, grid, gather::kThreads, stream, nullptr, nullptr, a);
  if (rc != DORA_OK) return rc;
  TakeDesc take{};
  take.src = a.index;
  take.count = md.n;
  take.n = md.n;
  take.wide = 0;
  ScanDesc scan = plan.scan;
  if (plan.scan_on && md.part_words) {
    // a host partition: its checked offsets, which the prefix copy has put into the workspace
    scan.src = dst + w.part;
    scan.count = md.part_words;
    scan.wide = 0;
    scan.offsets = 1;
  }
  return launch_fields(PlanLaunch::kTaken, plan.fields.data(), plan.fields.size(), dst, stream,
                       nullptr, ev_stop, plan.scan_on ? &scan : nullptr, &take,
                       plan.scan_on ? a.counts : nullptr);
}

}  // namespace

int launch_plan_gather(const dora_plan& plan, uint8_t* dst, hipStream_t stream,
                       hipEvent_t ev_start, hipEvent_t ev_stop) {
  const ScanDesc* scan = plan.scan_on ? &plan.scan : nullptr;
  switch (plan.launch) {
    case PlanLaunch::kSegments: break;  // launch_pack's
    case PlanLaunch::kView: return launch_gather(plan.gd, dst, stream, ev_start, ev_stop);
    case PlanLaunch::kFields:
    case PlanLaunch::kCast:
    case PlanLaunch::kReduce:
    case PlanLaunch::kResize:
    case PlanLaunch::kCrop:
    case PlanLaunch::kResizePrep:
    case PlanLaunch::kCropPrep:
    case PlanLaunch::kTaken:
      return launch_fields(plan.launch, plan.fields.data(), plan.fields.size(), dst, stream,
                           ev_start, ev_stop, scan,
                           plan.launch == PlanLaunch::kTaken ? &plan.take : nullptr);
    case PlanLaunch::kMasked: return launch_mask(plan, dst, stream, ev_start, ev_stop);
  }
  return fail(DORA_ERR_INVALID, "a plan of copy segments has no gather to launch");
}

int launch_plan_prefix(const dora_plan& plan, uint8_t* dst, hipStream_t stream) {
  for (const Segment& g : plan.prefix)
    DORA_HIP(hipMemcpyAsync(dst + g.dst_off, g.src, g.len, hipMemcpyHostToDevice, stream));
  return DORA_OK;
}

// Launch a pack and wait for it by spinning on a host flag the launch writes itself (a
// blocking stream synchronise sleeps and wakes tens of microseconds late).  Per thread and
// device: the pinned flag, its device view and the done words.  Falls back to a stream
// synchronise when the launch cannot signal (transform segments) or the flag does not come.
int launch_pack_wait(const Segment* segs, size_t n, uint8_t* dst, hipStream_t stream) {
  struct WaitCtx {
    int device = -1;
    uint64_t* host = nullptr;
    uint64_t* dev = nullptr;
    uint32_t* done = nullptr;
    uint64_t epoch = 0;
  };
  thread_local std::vector<WaitCtx> ctxs;
  int device = 0;
  DORA_HIP(hipGetDevice(&device));
  WaitCtx* c = nullptr;
  for (auto& x : ctxs)
    if (x.device == device) c = &x;
  if (!c) {
    WaitCtx x;
    x.device = device;
    void* dv = nullptr;
    DORA_HIP(hipHostMalloc(reinterpret_cast<void**>(&x.host), 64, hipHostMallocMapped));
    DORA_HIP(hipHostGetDevicePointer(&dv, x.host, 0));
    x.dev = static_cast<uint64_t*>(dv);
    *reinterpret_cast<volatile uint64_t*>(x.host) = 0;
    DORA_HIP(hipMalloc(&x.done, kMaxSignalWgs * sizeof(uint32_t)));
    DORA_HIP(hipMemset(x.done, 0, kMaxSignalWgs * sizeof(uint32_t)));
    DORA_HIP(hipDeviceSynchronize());
    ctxs.push_back(x);
    c = &ctxs.back();
  }
  FillSignal sig{c->dev, ++c->epoch, c->done};
  bool signalled = false;
  int rc = launch_pack(segs, n, ARROW_DEVICE_ROCM, dst, stream, nullptr, nullptr, &sig,
                       &signalled);
  if (rc != DORA_OK) return rc;
  if (signalled) {
    const volatile uint64_t* f = c->host;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (*f < sig.epoch) {
      __builtin_ia32_pause();
      if (++spins % 4096 == 0 &&
          std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200))
        break;  // slow or failed signal: the stream synchronise below decides
    }
    if (*f >= sig.epoch) return DORA_OK;
  }
  DORA_HIP(hipStreamSynchronize(stream));
  return DORA_OK;
}

size_t aql_args_size() { return sizeof(AqlPackArgs); }
size_t aql_batch_args_size() { return sizeof(dora::pack::AqlBatchArgs); }

// Arguments of dora_aql_packb_u4: the segments of `n` messages with absolute destinations,
// sorted by address, each message's stitched-edge bits carried over from its own edge_mask.
int build_aql_batch_args(const BatchItem* items, size_t n, uint8_t* out, size_t cap,
                         uint32_t* grid_out) {
  using dora::pack::AqlBatchArgs;
  using dora::pack::kMaxBatchMsgs;
  using dora::pack::kMaxBatchSegs;
  if (n == 0 || n > size_t(kMaxBatchMsgs)) return fail(DORA_ERR_INVALID, "batch of %zu", n);
  if (cap < sizeof(AqlBatchArgs)) return fail(DORA_ERR_INVALID, "AQL batch: argument buffer");
  struct S {
    uint64_t dst;
    const uint8_t* src;
    uint64_t len;
    uint32_t edge;
  };
  S all[kMaxBatchSegs];
  size_t ns = 0;
  const uint32_t chunk = aql_chunk_bytes(items[0].segs, items[0].n);
  for (size_t m = 0; m < n; ++m) {
    const BatchItem& it = items[m];
    if (ns + it.n > size_t(kMaxBatchSegs)) return fail(DORA_ERR_INVALID, "AQL batch: segments");
    if (aql_chunk_bytes(it.segs, it.n) != chunk)
      return fail(DORA_ERR_INVALID, "AQL batch: messages of different chunk sizes");
    const uint64_t em = edge_mask(it.segs, it.n, it.dst, it.dst_cap);
    for (size_t k = 0; k < it.n; ++k) {
      if (it.segs[k].op != SEG_COPY) return fail(DORA_ERR_INVALID, "AQL batch: transform");
      all[ns++] = {reinterpret_cast<uintptr_t>(it.dst) + it.segs[k].dst_off,
                   static_cast<const uint8_t*>(it.segs[k].src), it.segs[k].len,
                   static_cast<uint32_t>(em >> (2 * k)) & 3u};
    }
  }
  std::sort(all, all + ns, [](const S& a, const S& b) { return a.dst < b.dst; });
  AqlBatchArgs a;
  std::memset(&a, 0, sizeof(a));
  uint64_t edge = 0;
  for (size_t k = 0; k < ns; ++k) {
    a.seg[k] = {all[k].src, all[k].dst, all[k].len};
    edge |= uint64_t(all[k].edge) << (2 * k);
  }
  // a null destination: the segments' offsets are addresses; the first message's signal
  const int rc = finish_args(a, nullptr, items[0].sig, ns, chunk, edge, Signal::kInKernel, false);
  if (rc != DORA_OK) return rc;
  a.nmsg = static_cast<uint32_t>(n);
  for (size_t m = 0; m < n; ++m) a.msg[m] = {items[m].sig.flag, items[m].sig.epoch};
  std::memcpy(out, &a, sizeof(a));
  *grid_out = a.grid;
  return DORA_OK;
}

// Arguments of one AQL-dispatched signalling pack (aql.cpp): the same chunking and signalling
// grid as launch_pack's last launch; without a flag the command processor signals it.
int build_aql_args(const Segment* segs, size_t n, uint8_t* dst, const FillSignal& sig,
                   uint8_t* out, size_t cap, uint32_t* grid_out, uint64_t dst_cap) {
  if (n == 0 || n > size_t(kMaxAqlSegs)) return fail(DORA_ERR_INVALID, "AQL pack: %zu segments", n);
  if (cap < sizeof(AqlPackArgs)) return fail(DORA_ERR_INVALID, "AQL pack: argument buffer");
  for (size_t k = 0; k < n; ++k)
    if (segs[k].op != SEG_COPY) return fail(DORA_ERR_INVALID, "AQL pack: transform segment");
  AqlPackArgs a;
  std::memset(&a, 0, sizeof(a));
  set_segs(a.seg, segs, n);
  const int rc = finish_args(a, dst, sig, n, aql_chunk_bytes(segs, n),
                             edge_mask(segs, n, dst, dst_cap),
                             sig.flag ? Signal::kInKernel : Signal::kCp, false);
  if (rc != DORA_OK) return rc;
  std::memcpy(out, &a, sizeof(a));
  *grid_out = a.grid;
  return DORA_OK;
}

// Arguments of the preloaded single-segment AQL kernels (aql_kernels.hip dora_aql_pack1_*):
// dst, src, len, flag, done, epoch, chunk_bytes, grid — 56 bytes, the head of a one-segment pack
// at sample offset 0; the kernel derives the chunk layout itself.
int build_aql_args1(const Segment& sg, uint8_t* dst, const FillSignal& sig, uint8_t* out,
                    uint32_t* grid_out) {
  if (sg.op != SEG_COPY || sg.dst_off != 0)
    return fail(DORA_ERR_INVALID, "AQL single-segment pack: segment at offset %llu",
                (unsigned long long)sg.dst_off);
  PackArgsT<1> a;
  std::memset(&a, 0, sizeof(a));
  set_segs(a.seg, &sg, 1);
  const int rc = finish_args(a, dst, sig, 1, aql_chunk_bytes(&sg, 1), 0,
                             sig.flag ? Signal::kInKernel : Signal::kCp, true);
  if (rc != DORA_OK) return rc;
  const uint64_t words[6] = {reinterpret_cast<uintptr_t>(dst), reinterpret_cast<uintptr_t>(sg.src),
                             sg.len, reinterpret_cast<uintptr_t>(sig.flag),
                             reinterpret_cast<uintptr_t>(sig.done), sig.epoch};
  std::memcpy(out, words, sizeof(words));
  std::memcpy(out + 48, &a.chunk_bytes, 4);
  std::memcpy(out + 52, &a.grid, 4);
  *grid_out = a.grid;
  return DORA_OK;
}

int launch_csum(const void* data, size_t len, uint64_t* out_dev, hipStream_t stream) {
  DORA_HIP(hipMemsetAsync(out_dev, 0, sizeof(uint64_t), stream));
  if (len) {
    hipLaunchKernelGGL(csum_kernel, dim3(grid_for((len + 7) / 8)), dim3(kThreads), 0, stream,
                       static_cast<const uint8_t*>(data), uint64_t(len),
                       reinterpret_cast<unsigned long long*>(out_dev));
    DORA_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(csum_finalize, dim3(1), dim3(1), 0, stream,
                     reinterpret_cast<unsigned long long*>(out_dev), uint64_t(len));
  DORA_HIP(hipGetLastError());
  return DORA_OK;
}

int launch_fill(void* dst, size_t len, uint64_t seed, hipStream_t stream) {
  if (!len) return DORA_OK;
  hipLaunchKernelGGL(fill_kernel, dim3(grid_for((len + 7) / 8)), dim3(kThreads), 0, stream,
                     static_cast<uint8_t*>(dst), uint64_t(len), seed);
  DORA_HIP(hipGetLastError());
  return DORA_OK;
}

int launch_fill_ticket(void* dst, size_t len, uint64_t seed, const dora_fill_ticket& t,
                       hipStream_t stream) {
  hipLaunchKernelGGL(fill_ticket_kernel, dim3(t.workgroups), dim3(kThreads), 0, stream,
                     static_cast<uint8_t*>(dst), uint64_t(len), seed, t);
  DORA_HIP(hipGetLastError());
  return DORA_OK;
}

}  // namespace dora

extern "C" {

size_t dora_gpu_plan_workspace_size(const dora_plan* plan) {
  return plan ? static_cast<size_t>(dora::plan_workspace(*plan)) : 0;
}

int dora_gpu_pack(const dora_plan* plan, void* dst, size_t dst_len, dora_stream_t stream) {
  if (!plan) return dora::fail(DORA_ERR_INVALID, "plan is NULL");
  if (dst_len < plan->size)
    // arrow_utils.rs:37-42 asserts; the C ABI reports instead
    return dora::fail(DORA_ERR_TOO_SMALL,
                      "target buffer too small (total_len: %zu, required_len: %llu)", dst_len,
                      static_cast<unsigned long long>(plan->size));
  const bool gather = plan->launch != dora::PlanLaunch::kSegments;
  if (plan->segs.empty() && !gather) return DORA_OK;
  if (dst_len - plan->size < dora::plan_workspace(*plan))
    return dora::fail(DORA_ERR_INVALID, "a mask plan's target holds the sample and its workspace "
                      "(total_len: %zu, sample: %llu, workspace: %llu): nothing was launched",
                      dst_len, static_cast<unsigned long long>(plan->size),
                      static_cast<unsigned long long>(dora::plan_workspace(*plan)));
  if (!dst) return dora::fail(DORA_ERR_INVALID, "dst is NULL");
  if (plan->dev_tensor) {
    // a device tensor view: inside one allocation of the current GPU before anything reads it
    int device = 0;
    DORA_HIP(hipGetDevice(&device));
    int rc = dora::check_plan_range(*plan, device);
    if (rc != DORA_OK) return rc;
    rc = dora::launch_plan_prefix(*plan, static_cast<uint8_t*>(dst),
                                  static_cast<hipStream_t>(stream));
    if (rc != DORA_OK) return rc;
    if (gather)
      return dora::launch_plan_gather(*plan, static_cast<uint8_t*>(dst),
                                      static_cast<hipStream_t>(stream));
  }
  return dora::launch_pack(plan->segs.data(), plan->segs.size(), plan->dev,
                           static_cast<uint8_t*>(dst), static_cast<hipStream_t>(stream), nullptr,
                           nullptr, nullptr, nullptr, dst_len);
}

int dora_gpu_csum64(const void* data, size_t len, uint64_t* out_dev, dora_stream_t stream) {
  if (!out_dev || (!data && len)) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::launch_csum(data, len, out_dev, static_cast<hipStream_t>(stream));
}

int dora_gpu_csum64_sync(const void* data, size_t len, dora_stream_t stream, uint64_t* out) {
  if (!out || (!data && len)) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  uint64_t* d = nullptr;
  DORA_HIP(hipMalloc(&d, sizeof(uint64_t)));
  int rc = dora::launch_csum(data, len, d, static_cast<hipStream_t>(stream));
  if (rc == DORA_OK) {
    hipError_t e = hipMemcpyAsync(out, d, sizeof(uint64_t), hipMemcpyDeviceToHost,
                                  static_cast<hipStream_t>(stream));
    if (e == hipSuccess) e = hipStreamSynchronize(static_cast<hipStream_t>(stream));
    if (e != hipSuccess) rc = dora::fail(DORA_ERR_HIP, "csum64 readback: %s", hipGetErrorString(e));
  }
  (void)hipFree(d);
  return rc;
}

int dora_gpu_fill_splitmix(void* dst, size_t len, uint64_t seed, dora_stream_t stream) {
  if (!dst && len) return dora::fail(DORA_ERR_INVALID, "dst is NULL");
  return dora::launch_fill(dst, len, seed, static_cast<hipStream_t>(stream));
}

int dora_gpu_fill_splitmix_ticket(void* dst, size_t len, uint64_t seed,
                                  const dora_fill_ticket* ticket, dora_stream_t stream) {
  if (!dst || !ticket) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  if (reinterpret_cast<uintptr_t>(dst) & 15)
    return dora::fail(DORA_ERR_INVALID, "dst must be 16-byte aligned (a sample's data is)");
  if (!ticket->flag || !ticket->workgroups || ticket->workgroups > dora::kMaxSignalWgs ||
      (ticket->workgroups > 1 && !ticket->done))
    return dora::fail(DORA_ERR_INVALID, "not a ticket of dora_sample_fill_ticket");
  return dora::launch_fill_ticket(dst, len, seed, *ticket, static_cast<hipStream_t>(stream));
}

}  // extern "C"
