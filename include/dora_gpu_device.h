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

/* ------------------------------------------------------------------------------------------ */
/* The fill signal, in three steps.  This is its one home: dora_fill_publish below and the      */
/* library's own pack kernels are all built from these.  `wg` / `nwg`: the workgroup and the    */
/* launch's workgroup count; `tid` / `nthreads`: the lane's linear index in its workgroup and   */
/* the workgroup's size.  All passed in: nothing here reads blockDim or gridDim, so a kernel    */
/* dispatched without hidden arguments can call them.                                           */
/*                                                                                              */
/* Before the first step every wave waits for its own stores (s_waitcnt vmcnt(0)) and the       */
/* workgroup passes a barrier: the caller's part, because what is waited for differs (a pack's  */
/* stores, a read-signalled pack's loads, a plain-store kernel's write-back).  With the sample  */
/* written through to device scope (sc1) no dirty line is left in the per-XCD L2s, so nothing   */
/* below needs a release: no same-address atomics (those serialise at ~0.1 us each across XCDs) */
/* and no L2 write-back per workgroup (~0.1 us each, serial per XCD).  For the packs this       */
/* replaces the stream write-value packet, a ~4 us blit kernel plus a kernel boundary per       */
/* message on ROCm 7.                                                                           */
/* ------------------------------------------------------------------------------------------ */

/* Arrive: lane 0 stores the epoch's low word into the workgroup's own done word. */
__device__ __forceinline__ void (dora_fill_arrive)(dora_gu32* done, uint32_t wg, uint32_t e,
                                                   uint32_t tid) {
  if (tid == 0) __hip_atomic_store(done + wg, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/*
 * Wait for all: workgroup 0 only, every thread of it in uniform control flow.  Polls every done
 * word once per round, LOADS independent loads in flight per lane, so completion is seen one
 * load round trip after the last workgroup arrived.  True once every word holds `e`.  Bounded,
 * 2^22 rounds (seconds): a lost workgroup must not hang the device; the caller then leaves the
 * flag unset and the receiver reports the fill as failed.  The workgroup's vote goes through one
 * LDS word (__syncthreads_and would read the workgroup size from hidden arguments): 16 bytes of
 * static LDS, 16-byte aligned, so that a dynamic LDS base stays 16-byte aligned.
 */
template <int LOADS>
__device__ __forceinline__ bool (dora_fill_wait_all)(const dora_gu32* done, uint32_t nwg,
                                                     uint32_t e, uint32_t tid,
                                                     uint32_t nthreads) {
  __shared__ __attribute__((aligned(16))) uint32_t missing[4];
  for (uint32_t round = 0; round < (1u << 22); ++round) {
    if (tid == 0) missing[0] = 0;
    __syncthreads();
    bool mine = true;
    for (uint32_t base = tid; base < nwg; base += LOADS * nthreads) {
      uint32_t v[LOADS];
#pragma unroll
      for (int k = 0; k < LOADS; ++k) {
        const uint32_t i = base + k * nthreads;
        v[k] = i < nwg ? __hip_atomic_load(done + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                       : e;
      }
#pragma unroll
      for (int k = 0; k < LOADS; ++k) mine &= v[k] == e;
    }
    if (!mine) missing[0] = 1;
    __syncthreads();
    const bool all = missing[0] == 0;
    __syncthreads();
    if (all) return true;
    __builtin_amdgcn_s_sleep(1);
  }
  return false;
}

/* Raise: stamp the flag line (the launch's start, taken on entry, and the time it signals,
 * s_memrealtime: the fill's device time without a profiled queue or timing events) and store the
 * epoch into the flag.  One lane of workgroup 0. */
__device__ __forceinline__ void (dora_fill_raise)(dora_gu64* flag, uint64_t epoch,
                                                  uint64_t t_start) {
  __hip_atomic_store(flag + 1, t_start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __hip_atomic_store(flag + 2, (dora_fill_clock)(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  /* Relaxed: everything this store publishes is already complete and written through (sample
   * stores and done words are device-scope write-through) or written back, and it issues only
   * after every done word was observed; a release would write back this XCD's whole L2 for
   * nothing. */
  __hip_atomic_store(flag, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

/*
 * Publish the sample.  `wg` / `nwg`: this workgroup's linear index and the launch's workgroup
 * count; `nwg` must equal the ticket's count (a launch of another size publishes nothing: the
 * flag stays unset and receivers report the fill as failed, as for a kernel that never ran).
 * Any workgroup size and shape.  `t_start`: the start stamp (0: now).
 *
 * Each workgroup raises its done word once its stores are complete; workgroup 0 polls all of
 * them, eight loads in flight per lane, and then raises the flag.  The poll is bounded (2^22
 * rounds, seconds): a lost workgroup leaves the flag unset and never hangs the device.  Uses the
 * 16 bytes of static LDS of dora_fill_wait_all.
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
  if (nwg > 1) { /* else nothing to wait for but this workgroup's own stores */
    const uint32_t e = static_cast<uint32_t>(t.epoch);
    dora_gu32* const done = reinterpret_cast<dora_gu32*>(static_cast<uintptr_t>(t.done));
    (dora_fill_arrive)(done, wg, e, tid);
    if (wg != 0 || !(dora_fill_wait_all<8>)(done, nwg, e, tid, nthreads)) return;
  }
  if (tid == 0)
    (dora_fill_raise)(reinterpret_cast<dora_gu64*>(static_cast<uintptr_t>(t.flag)), t.epoch,
                      t_start);
}

/* The same for a launch whose workgroups are all of its grid: linearises blockIdx / gridDim. */
__device__ __forceinline__ void (dora_fill_publish)(const dora_fill_ticket t) {
  (dora_fill_publish)(t, blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z),
                      gridDim.x * gridDim.y * gridDim.z);
}

#endif /* DORA_GPU_DEVICE_H */
