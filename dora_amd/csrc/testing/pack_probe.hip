// Test hook of the pack bodies (pack_device.h): one pack of caller-given segments through a named
// body, its arguments filled by the product's own builders (kernels.hip finish_args / edge_mask /
// build_aql_batch_args, pack_device.h chunk_layout), with the chunk size and the grid optionally
// overridden inside the ranges the product uses.  It exists so that tests/test_gpu_random_packs.py
// reaches the write-through body, the coherent-load body of the AQL arguments and the batch body
// with segment layouts no dataflow produces.  The kernels here compile the same header as
// aql_kernels.hip but without that object's kernarg-preload flag: they test the body's source, not
// that binary.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "pack_device.h"
#include "pack_probe.h"
#include "plan.h"

namespace dora {
// kernels.hip
uint64_t edge_mask(const Segment* segs, size_t n, const uint8_t* dst, uint64_t cap);
uint32_t aql_chunk_bytes(const Segment* segs, size_t n);
int build_aql_batch_args(const BatchItem* items, size_t n, uint8_t* out, size_t cap,
                         uint32_t* grid);
int finish_pack_args(pack::PackArgs& a, uint8_t* dst, const FillSignal& sig, size_t nseg,
                     uint32_t chunk_bytes, uint64_t edge, bool signals);
int finish_aql_args(pack::AqlPackArgs& a, uint8_t* dst, const FillSignal& sig, size_t nseg,
                    uint32_t chunk_bytes, uint64_t edge, bool signals);
int finish_batch_args(pack::AqlBatchArgs& a, uint8_t* dst, const FillSignal& sig, size_t nseg,
                      uint32_t chunk_bytes, uint64_t edge, bool signals);
}  // namespace dora

namespace {

using namespace dora::pack;

__global__ __launch_bounds__(kThreads) void probe_pack_wt(PackArgs a) {
  pack_body<4, 2>(a, blockIdx.x, a.grid);
}
__global__ __launch_bounds__(kThreads) void probe_pack_coherent(AqlPackArgs a) {
  pack_body<4, kCoherent>(a, blockIdx.x, a.grid);
}
__global__ __launch_bounds__(kThreads) void probe_pack_batch(AqlBatchArgs a) {
  pack_body<4, 2>(a, blockIdx.x, a.grid);
}

constexpr size_t kFlagBytes = 128;  // one flag line per message (shm.h FillFlag)

// Per device: pinned flag lines, their device view and the done words, as launch_pack_wait's.
struct Ctx {
  int device = -1;
  uint8_t* host = nullptr;
  uint8_t* dev = nullptr;
  uint32_t* done = nullptr;
};
std::vector<Ctx> g_ctx;
uint64_t g_epoch = 0x100;

int ctx_for(Ctx** out) {
  int device = 0;
  DORA_HIP(hipGetDevice(&device));
  for (auto& x : g_ctx)
    if (x.device == device) {
      *out = &x;
      return DORA_OK;
    }
  Ctx x;
  x.device = device;
  void* dv = nullptr;
  DORA_HIP(hipHostMalloc(reinterpret_cast<void**>(&x.host), kMaxBatchMsgs * kFlagBytes,
                         hipHostMallocMapped));
  DORA_HIP(hipHostGetDevicePointer(&dv, x.host, 0));
  x.dev = static_cast<uint8_t*>(dv);
  std::memset(x.host, 0, kMaxBatchMsgs * kFlagBytes);
  DORA_HIP(hipMalloc(&x.done, dora::kMaxSignalWgs * sizeof(uint32_t)));
  DORA_HIP(hipMemset(x.done, 0, dora::kMaxSignalWgs * sizeof(uint32_t)));
  DORA_HIP(hipDeviceSynchronize());
  g_ctx.push_back(x);
  *out = &g_ctx.back();
  return DORA_OK;
}

// [lo, hi) lies inside one device allocation: a probe never launches over memory it cannot name.
int check_range(uintptr_t lo, uintptr_t hi, const char* what) {
  hipDeviceptr_t ab = nullptr;
  size_t asz = 0;
  const hipError_t e = hipMemGetAddressRange(&ab, &asz, reinterpret_cast<void*>(lo));
  if (e != hipSuccess || !asz) {
    (void)hipGetLastError();
    return dora::fail(DORA_ERR_INVALID, "pack probe: %s %p is in no device allocation", what,
                      reinterpret_cast<void*>(lo));
  }
  const uintptr_t k0 = reinterpret_cast<uintptr_t>(ab), k1 = k0 + asz;
  if (lo < k0 || hi > k1)
    return dora::fail(DORA_ERR_INVALID, "pack probe: %s [%p, %p) leaves its allocation", what,
                      reinterpret_cast<void*>(lo), reinterpret_cast<void*>(hi));
  return DORA_OK;
}

// What a body may touch: the segment's bytes and the whole units of [dst, dst + cap) in the
// destination; in the source the two aligned units around every unit of the segment.
int check_ranges(const dora::BatchItem* items, size_t n) {
  for (size_t m = 0; m < n; ++m) {
    const uintptr_t d = reinterpret_cast<uintptr_t>(items[m].dst);
    uint64_t end = items[m].dst_cap;
    for (size_t k = 0; k < items[m].n; ++k) {
      const dora::Segment& g = items[m].segs[k];
      end = std::max<uint64_t>(end, g.dst_off + g.len);
      if (!g.len) continue;
      const uintptr_t s = reinterpret_cast<uintptr_t>(g.src);
      const int rc = check_range((s & ~uintptr_t(15)) - 16, ((s + g.len + 15) & ~uintptr_t(15)) + 16,
                                 "source");
      if (rc != DORA_OK) return rc;
    }
    const int rc = check_range(d, d + std::max<uint64_t>(end, 1), "destination");
    if (rc != DORA_OK) return rc;
  }
  return DORA_OK;
}

template <class A>
int override_grid(A& a, uint32_t grid) {
  if (!grid) return DORA_OK;
  if (grid > a.n_chunks || grid > dora::kMaxSignalWgs)
    return dora::fail(DORA_ERR_INVALID, "pack probe: grid %u outside [1, %u]", grid, a.n_chunks);
  a.grid = grid;
  return DORA_OK;
}

template <class A>
void set_segs(A& a, const dora::Segment* segs, size_t n) {
  for (size_t k = 0; k < n; ++k)
    a.seg[k] = {static_cast<const uint8_t*>(segs[k].src), segs[k].dst_off, segs[k].len};
}

template <class A>
int launch(void (*kern)(A), const A& a, hipStream_t stream) {
  hipLaunchKernelGGL(kern, dim3(a.grid), dim3(kThreads), 0, stream, a);
  DORA_HIP(hipGetLastError());
  return DORA_OK;
}

template <class A>
int copy_block(const A& a, uint8_t* out, size_t cap, size_t* out_len) {
  if (out_len) *out_len = sizeof(A);
  if (cap < sizeof(A)) return dora::fail(DORA_ERR_INVALID, "pack probe: argument buffer");
  std::memcpy(out, &a, sizeof(A));
  return DORA_OK;
}

}  // namespace

namespace dora {

int pack_probe(int body, size_t n_msgs, const size_t* seg_counts, const uint64_t* segs,
               const uint64_t* dsts, const uint64_t* dst_caps, uint32_t chunk_bytes, uint32_t grid,
               hipStream_t stream, uint32_t* flags_ok, uint8_t* out, size_t cap,
               size_t* out_len) {
  if (body < 0 || body > 3) return fail(DORA_ERR_INVALID, "pack probe: body %d", body);
  if (!n_msgs || n_msgs > size_t(kMaxBatchMsgs) || (body != 3 && n_msgs != 1))
    return fail(DORA_ERR_INVALID, "pack probe: %zu messages for body %d", n_msgs, body);
  if (chunk_bytes % 8192 || chunk_bytes > (4u << 20))
    return fail(DORA_ERR_INVALID, "pack probe: chunk_bytes %u is no multiple of 8192 up to 4 MiB",
                chunk_bytes);
  if (body == 0 && (chunk_bytes || grid))
    return fail(DORA_ERR_INVALID, "pack probe: body 0 takes the product's chunk size and grid");
  const bool dry = out != nullptr;

  std::vector<std::vector<Segment>> s(n_msgs);
  BatchItem items[kMaxBatchMsgs];
  Ctx* c = nullptr;
  if (!dry && body != 0) {
    const int rc = ctx_for(&c);
    if (rc != DORA_OK) return rc;
  }
  size_t k = 0;
  for (size_t m = 0; m < n_msgs; ++m) {
    for (size_t j = 0; j < seg_counts[m]; ++j, ++k)
      s[m].push_back({reinterpret_cast<const void*>(segs[3 * k]), segs[3 * k + 1], segs[3 * k + 2]});
    // a dry run's flags are never dereferenced: distinct non-null words
    uint64_t* const flag = reinterpret_cast<uint64_t*>(c ? c->dev + m * kFlagBytes
                                                          : reinterpret_cast<uint8_t*>(0x1000 + m * kFlagBytes));
    items[m] = {s[m].data(), s[m].size(), reinterpret_cast<uint8_t*>(dsts[m]),
                FillSignal{flag, ++g_epoch, c ? c->done : nullptr}, dst_caps[m]};
  }
  const Segment* const sg = items[0].segs;
  const size_t n = items[0].n;
  uint8_t* const dst = items[0].dst;
  const uint64_t dcap = items[0].dst_cap;
  if (body != 3 && !n) return fail(DORA_ERR_INVALID, "pack probe: no segment");
  const size_t max_segs = body == 2 ? size_t(kMaxAqlSegs) : size_t(kMaxSegs);
  if (body != 0 && body != 3 && n > max_segs)
    return fail(DORA_ERR_INVALID, "pack probe: %zu segments for body %d", n, body);
  if (!dry) {
    const int rc = check_ranges(items, n_msgs);
    if (rc != DORA_OK) return rc;
  }
  if (flags_ok) *flags_ok = 0;

  int rc = DORA_OK;
  if (body == 0) {
    if (dry) {  // launch_pack's first launch, restated: unsignalled, stitched only if it is the plan
      PackArgs a;
      std::memset(&a, 0, sizeof(a));
      const size_t m = std::min<size_t>(kMaxSegs, n);
      set_segs(a, sg, m);
      rc = finish_pack_args(a, dst, FillSignal{}, m, aql_chunk_bytes(sg, m),
                            m == n ? edge_mask(sg, n, dst, dcap) : 0, false);
      return rc != DORA_OK ? rc : copy_block(a, out, cap, out_len);
    }
    rc = launch_pack(sg, n, ARROW_DEVICE_ROCM, dst, stream, nullptr, nullptr, nullptr, nullptr,
                     dcap);
    if (rc != DORA_OK) return rc;
    DORA_HIP(hipStreamSynchronize(stream));
    return DORA_OK;
  }
  if (body == 1) {
    PackArgs a;
    std::memset(&a, 0, sizeof(a));
    set_segs(a, sg, n);
    rc = finish_pack_args(a, dst, items[0].sig, n, chunk_bytes ? chunk_bytes : aql_chunk_bytes(sg, n),
                          edge_mask(sg, n, dst, dcap), true);
    if (rc == DORA_OK) rc = override_grid(a, grid);
    if (rc != DORA_OK) return rc;
    if (dry) return copy_block(a, out, cap, out_len);
    rc = launch(probe_pack_wt, a, stream);
  } else if (body == 2) {
    AqlPackArgs a;
    std::memset(&a, 0, sizeof(a));
    set_segs(a, sg, n);
    rc = finish_aql_args(a, dst, items[0].sig, n, chunk_bytes ? chunk_bytes : aql_chunk_bytes(sg, n),
                         edge_mask(sg, n, dst, dcap), true);
    if (rc == DORA_OK) rc = override_grid(a, grid);
    if (rc != DORA_OK) return rc;
    if (dry) return copy_block(a, out, cap, out_len);
    rc = launch(probe_pack_coherent, a, stream);
  } else {
    AqlBatchArgs a;
    uint32_t g = 0;
    rc = build_aql_batch_args(items, n_msgs, reinterpret_cast<uint8_t*>(&a), sizeof(a), &g);
    // another chunk size: the head is filled again over the block's sorted segments
    if (rc == DORA_OK && chunk_bytes)
      rc = finish_batch_args(a, nullptr, items[0].sig, a.nseg, chunk_bytes, a.edge_mask, true);
    if (rc == DORA_OK) rc = override_grid(a, grid);
    if (rc != DORA_OK) return rc;
    if (dry) return copy_block(a, out, cap, out_len);
    rc = launch(probe_pack_batch, a, stream);
  }
  if (rc != DORA_OK) return rc;
  DORA_HIP(hipStreamSynchronize(stream));
  uint32_t ok = 0;
  for (size_t m = 0; m < n_msgs; ++m) {
    const volatile uint64_t* f = reinterpret_cast<const volatile uint64_t*>(c->host + m * kFlagBytes);
    if (*f == items[m].sig.epoch) ok |= 1u << m;
  }
  if (flags_ok) *flags_ok = ok;
  return DORA_OK;
}

}  // namespace dora
