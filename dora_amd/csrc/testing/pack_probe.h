// The pack probe of libdora_gpu_testing.so (pack_probe.hip), called by the hooks in testing.cpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace dora {
// One pack of caller-given segments through body `body` (include/dora_gpu_testing.h
// dora_gpu_test_pack_segments).  With `out` the filled argument block is copied there and nothing
// is launched (no GPU needed); else the pack runs on `stream`, which is synchronised.
int pack_probe(int body, size_t n_msgs, const size_t* seg_counts, const uint64_t* segs,
               const uint64_t* dsts, const uint64_t* dst_caps, uint32_t chunk_bytes, uint32_t grid,
               hipStream_t stream, uint32_t* flags_ok, uint8_t* out, size_t cap, size_t* out_len);
}  // namespace dora
