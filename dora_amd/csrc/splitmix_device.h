// The splitmix64 payload written into a sample in place by a kernel that publishes it itself
// (include/dora_gpu_device.h): the device body shared by dora_gpu_fill_splitmix_ticket
// (kernels.hip) and the test hook dora_gpu_test_publish_kernel (testing/publish_kernel.hip).
// Word k = fmix64(seed + (k + 1) * GOLDEN), little-endian bytes (oracle/checksum_ref.py).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "dora_gpu_device.h"

namespace dora {
namespace splitmix {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t word(uint64_t seed, uint64_t k) {
  uint64_t z = seed + (k + 1) * kGolden;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// Bytes [16u, 16u + 16) ∩ [0, n) of the payload at `p` (16-byte aligned), one unit per call.
// WT: through the write-through helpers (16 B whole units; an 8-byte word and single bytes in the
// unit the payload ends in); else ordinary stores.
template <bool WT>
__device__ __forceinline__ void store_unit(uint8_t* p, uint64_t n, uint64_t seed, uint64_t u) {
  const uint64_t w0 = word(seed, 2 * u), w1 = word(seed, 2 * u + 1);
  uint8_t* q = p + 16 * u;
  if (16 * u + 16 <= n) {
    const dora_u32x4 v = {uint32_t(w0), uint32_t(w0 >> 32), uint32_t(w1), uint32_t(w1 >> 32)};
    if constexpr (WT) dora_st16(q, v);
    else *reinterpret_cast<dora_u32x4*>(q) = v;
    return;
  }
  uint64_t done = 0;
  if (16 * u + 8 <= n) {
    if constexpr (WT) dora_st8(q, w0);
    else *reinterpret_cast<uint64_t*>(q) = w0;
    done = 8;
  }
  const uint64_t w = done ? w1 : w0;
  for (uint64_t b = done; 16 * u + b < n; ++b) {
    const uint8_t x = uint8_t(w >> (8 * (b - done)));
    if constexpr (WT) dora_st1(q + b, x);
    else q[b] = x;
  }
}

// The whole launch: its workgroups stride over the payload's 16-byte units, then publish.
template <bool WT>
__device__ __forceinline__ void fill_and_publish(uint8_t* p, uint64_t n, uint64_t seed,
                                                 const dora_fill_ticket& t) {
  const uint64_t t_start = blockIdx.x == 0 ? dora_fill_clock() : 0;
  const uint64_t units = (n + 15) / 16;
  for (uint64_t u = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x; u < units;
       u += uint64_t(gridDim.x) * blockDim.x)
    store_unit<WT>(p, n, seed, u);
  dora_fill_publish(t, blockIdx.x, gridDim.x, t_start);
}

}  // namespace splitmix
}  // namespace dora
