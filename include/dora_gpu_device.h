/*
 * dora_gpu_device.h — device side of the zero-copy sample API: let the kernel that writes a
 * sample in place publish it itself (gfx950 / MI355X, HIP device code, header-only).
 *
 *   host:    dora_node_allocate_data_sample -> dora_sample_fill_ticket -> launch -> send_output_sample
 *   kernel:  write the sample -> dora_fill_publish, called by EVERY thread of EVERY workgroup of
 *            the one launch the ticket was issued for, in uniform control flow, after the
 *            thread's last store to the sample.
 *
 * No second stream operation and no pack: receivers wait on the slot's fill flag, which the
 * launch's workgroup 0 raises once every workgroup's stores are complete.
 *
 * What makes the signal correct on this chip (8 XCDs with private L2s):
 *  - DORA_FILL_WRITE_THROUGH: every sample byte is stored through dora_st16 / dora_st8 / dora_st4 /
 *    dora_st1 (sc1: written through the XCD's L2), so nothing is left dirty and no cache write-back
 *    is needed.  DORA_FILL_PLAIN: ordinary stores; one lane per workgroup then releases at agent
 *    scope (an L2 write-back, ~2-7 us per workgroup: the slow mode, for kernels that cannot
 *    change their stores).
 *  - every storing wave waits for its own stores (s_waitcnt vmcnt(0)) BEFORE the workgroup
 *    barrier; a drain by the signalling lane alone leaves other waves' stores in flight.
 *  - done words and the flag are agent- / system-scope atomic stores, never plain stores.
 *
 * Function names are declared in parentheses, `void (dora_fill_publish)(...)`: the headers under
 * include/ are also read as the list of C symbols the shared library exports, and these are
 * device inlines, not exports.  Call them as usual.
 */
#ifndef DORA_GPU_DEVICE_H
#define DORA_GPU_DEVICE_H

#if !defined(__HIPCC__)
#error "dora_gpu_device.h is HIP device code: compile with hipcc (host code wants dora_gpu.h)"
#endif

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dora_fill_ticket.h"

typedef unsigned int dora_u32x4 __attribute__((ext_vector_type(4)));
/* The flag and the done words are accessed through global-address-space pointers (global_
 * instructions with sc bits), never flat ones. */
typedef __attribute__((address_space(1))) uint32_t dora_gu32;
typedef __attribute__((address_space(1))) uint64_t dora_gu64;

/* ------------------------------------------------------------------------------------------ */
/* Write-through stores (device scope).  `p` must be aligned to the store's size.             */
/* ------------------------------------------------------------------------------------------ */
__device__ __forceinline__ void (dora_st16)(void* p, dora_u32x4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc1 nt" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void (dora_st8)(void* p, uint64_t v) {
  asm volatile("global_store_dwordx2 %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void (dora_st4)(void* p, uint32_t v) {
  asm volatile("global_store_dword %0, %1, off sc1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void (dora_st1)(void* p, uint8_t v) {
  const uint32_t w = v;
  asm volatile("global_store_byte %0, %1, off sc1" ::"v"(p), "v"(w) : "memory");
}

/* The clock of the flag line's stamps (s_memrealtime, 100 MHz): take it on kernel entry and hand
 * it to dora_fill_publish as `t_start` to have the stamps span the whole kernel. */
__device__ __forceinline__ uint64_t (dora_fill_clock)() { return __builtin_amdgcn_s_memrealtime(); }

/* Stamp the flag line (start, signal time) and raise the flag: one lane of workgroup 0. */
__device__ __forceinline__ void (dora_fill_raise)(const dora_fill_ticket& t, uint64_t t_start) {
  dora_gu64* const flag = reinterpret_cast<dora_gu64*>(static_cast<uintptr_t>(t.flag));
  __hip_atomic_store(flag + 1, t_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(flag + 2, (dora_fill_clock)(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  /* relaxed: everything this store publishes is complete and written through or written back,
   * and it issues only after every done word was observed */
  __hip_atomic_store(flag, t.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

/*
 * Publish the sample.  `wg` / `nwg`: this workgroup's linear index and the launch's workgroup
 * count; `nwg` must equal the ticket's count (a launch of another size publishes nothing: the
 * flag stays unset and receivers report the fill as failed, as for a kernel that never ran).
 * Any workgroup size and shape.  `t_start`: the start stamp (0: now).
 *
 * Each workgroup raises its done word once its stores are complete; workgroup 0 polls all of
 * them and then raises the flag.  The poll is bounded (~2 s): a lost workgroup leaves the flag
 * unset and never hangs the device.  Uses 16 bytes of static LDS (a 16-byte-aligned vote word:
 * a dynamic LDS base stays 16-byte aligned).
 */
__device__ __forceinline__ void (dora_fill_publish)(const dora_fill_ticket t, uint32_t wg,
                                                    uint32_t nwg, uint64_t t_start = 0) {
  const uint32_t tid = threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z);
  const uint32_t nthreads = blockDim.x * blockDim.y * blockDim.z;
  if (wg == 0 && tid == 0 && !t_start) t_start = (dora_fill_clock)();
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); /* this wave's sample stores are complete */
  __syncthreads();
  if (nwg != t.workgroups || wg >= nwg) return; /* not the launch the ticket was issued for */
  if (t.mode == DORA_FILL_PLAIN && tid == 0) {
    /* ordinary stores sit dirty in this XCD's L2: write them back.  The asm wait after the
     * fence is needed: the compiler may drop the fence's own wait when it can prove this wave's
     * counter empty (it is, after the wait above), and the done word must not overtake the
     * write-back. */
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  if (nwg == 1) { /* nothing to wait for but this workgroup's own stores */
    if (tid == 0) (dora_fill_raise)(t, t_start);
    return;
  }
  const uint32_t e = static_cast<uint32_t>(t.epoch);
  dora_gu32* const done = reinterpret_cast<dora_gu32*>(static_cast<uintptr_t>(t.done));
  if (tid == 0) __hip_atomic_store(done + wg, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (wg != 0) return;
  /* vote[0]: some lane saw a done word below the epoch this round; vote[1]: give up */
  __shared__ __attribute__((aligned(16))) uint32_t vote[4];
  const uint64_t t0 = (dora_fill_clock)();
  bool ok = false;
  for (;;) {
    if (tid == 0) {
      vote[0] = 0;
      vote[1] = (dora_fill_clock)() - t0 > 200000000ull ? 1u : 0u;
    }
    __syncthreads();
    /* every done word once per round, eight independent loads in flight per lane */
    bool mine = true;
    for (uint32_t base = tid; base < nwg; base += 8 * nthreads) {
      uint32_t v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) { /* past the end: word 0 again, so the loads stay unconditional */
        const uint32_t i = base + k * nthreads;
        v[k] = __hip_atomic_load(done + (i < nwg ? i : 0u), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) mine &= v[k] == e;
    }
    if (!mine) vote[0] = 1;
    const bool give_up = vote[1] != 0;
    __syncthreads();
    const bool all = vote[0] == 0;
    __syncthreads();
    if (all) {
      ok = true;
      break;
    }
    if (give_up) break;
    __builtin_amdgcn_s_sleep(1);
  }
  if (tid == 0 && ok) (dora_fill_raise)(t, t_start);
}

/* The same for a launch whose workgroups are all of its grid: linearises blockIdx / gridDim. */
__device__ __forceinline__ void (dora_fill_publish)(const dora_fill_ticket t) {
  (dora_fill_publish)(t, blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                      gridDim.x * gridDim.y * gridDim.z);
}

#endif /* DORA_GPU_DEVICE_H */
