// The fence probes of libdora_gpu_testing.so (fence_probes.hip), called by the hooks in testing.cpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace dora {
int launch_l2_touch(const void* p, size_t len, hipStream_t stream);
int l1_stale_probe(int device, int mode, uint32_t* bad_first, uint32_t* stale, uint32_t* blocks);
}  // namespace dora
