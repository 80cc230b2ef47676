// Test hook of the self-published sample path (include/dora_gpu_device.h): the splitmix payload
// written in place by a kernel with a caller-chosen workgroup size, with write-through or
// ordinary stores, and published with dora_fill_publish.  It exists so that DORA_FILL_PLAIN and
// workgroup sizes other than the ticket kernel's 256 are exercised (tests/test_gpu_fill_ticket.py).
#include <hip/hip_runtime.h>

#include "common.h"
#include "dora_gpu_testing.h"
#include "plan.h"
#include "splitmix_device.h"

namespace {

template <bool WT>
__global__ __launch_bounds__(1024) void publish_kernel(uint8_t* p, uint64_t n, uint64_t seed,
                                                       dora_fill_ticket t) {
  dora::splitmix::fill_and_publish<WT>(p, n, seed, t);
}

}  // namespace

extern "C" int dora_gpu_test_publish_kernel(void* dst, size_t len, uint64_t seed,
                                            const dora_fill_ticket* ticket,
                                            uint32_t threads_per_wg, uint32_t store_mode,
                                            dora_stream_t stream) {
  if (!dst || !ticket) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  if (reinterpret_cast<uintptr_t>(dst) & 15)
    return dora::fail(DORA_ERR_INVALID, "dst must be 16-byte aligned");
  if (!threads_per_wg || threads_per_wg > 1024 || threads_per_wg % 64)
    return dora::fail(DORA_ERR_INVALID, "threads_per_wg: a multiple of 64 up to 1024");
  if (!ticket->flag || !ticket->workgroups || ticket->workgroups > dora::kMaxSignalWgs ||
      (ticket->workgroups > 1 && !ticket->done))
    return dora::fail(DORA_ERR_INVALID, "not a ticket of dora_sample_fill_ticket");
  if (store_mode > 1) return dora::fail(DORA_ERR_INVALID, "store_mode: 0 write-through, 1 plain");
  if (store_mode == 1 && ticket->mode != DORA_FILL_PLAIN)
    return dora::fail(DORA_ERR_INVALID,
                      "ordinary stores need a DORA_FILL_PLAIN ticket (nothing would write them "
                      "back before the flag)");
  const auto st = static_cast<hipStream_t>(stream);
  auto* p = static_cast<uint8_t*>(dst);
  if (store_mode == 0)
    hipLaunchKernelGGL(publish_kernel<true>, dim3(ticket->workgroups), dim3(threads_per_wg), 0, st,
                       p, uint64_t(len), seed, *ticket);
  else
    hipLaunchKernelGGL(publish_kernel<false>, dim3(ticket->workgroups), dim3(threads_per_wg), 0,
                       st, p, uint64_t(len), seed, *ticket);
  DORA_HIP(hipGetLastError());
  return DORA_OK;
}
