// libdora_gpu_testing.so: the test and microbenchmark hooks of the data plane, built apart from
// the shipped library (dora_amd/build.py build_testing) and linked against it — the product's
// ABI (include/dora_gpu.h) carries none of them.  Declared in include/dora_gpu_testing.h; used by
// tests/ and scripts/ only.  Each hook calls into the library's internals (aql.cpp, kernels.hip,
// bincode.cpp, bcast.cpp, shm.h) or into this library's own kernels (fence_probes.hip).
#include <hip/hip_runtime_api.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <sys/prctl.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "aql.h"
#include "bcast.h"
#include "bincode.h"
#include "common.h"
#include "dora_gpu.h"
#include "dora_gpu_testing.h"
#include "fence_probes.h"
#include "gather_device.h"
#include "pack_probe.h"
#include "reduce_device.h"
#include "resize_device.h"
#include "crop_device.h"
#include "plan.h"
#include "shm.h"

namespace dora {
// kernels.hip
int build_aql_batch_args(const BatchItem* items, size_t n, uint8_t* out, size_t cap,
                         uint32_t* grid);
void gather_force(int mode);
void reduce_force(int mode);
bool select_reduce_wave(const GatherDesc& g, const ReduceDesc& r);
void fields_launches(uint64_t out[4]);
int select_tile_dim(const GatherDesc& g, const uint8_t* dst);
}  // namespace dora

namespace dora {
namespace {

int copy_out(const std::vector<uint8_t>& v, uint8_t* out, size_t cap, size_t* out_len) {
  if (out_len) *out_len = v.size();
  if (!out || cap < v.size())
    return dora::fail(DORA_ERR_INVALID, "buffer of %zu bytes, %zu needed", cap, v.size());
  std::memcpy(out, v.data(), v.size());
  return DORA_OK;
}

std::string hex(const uint8_t* p, size_t n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  s.reserve(2 * n);
  for (size_t i = 0; i < n; ++i) {
    s.push_back(d[p[i] >> 4]);
    s.push_back(d[p[i] & 15]);
  }
  return s;
}

std::string jstr(const std::string& v) {
  std::string s = "\"";
  for (unsigned char c : v) {
    if (c == '"' || c == '\\') {
      s.push_back('\\');
      s.push_back(static_cast<char>(c));
    } else if (c < 0x20) {
      char b[8];
      std::snprintf(b, sizeof(b), "\\u%04x", c);
      s += b;
    } else {
      s.push_back(static_cast<char>(c));
    }
  }
  return s + "\"";
}

}  // namespace
}  // namespace dora


extern "C" {

int dora_gpu_test_batch_args(size_t n_msgs, const size_t* seg_counts, const uint64_t* segs,
                             const uint64_t* dsts, const uint64_t* dst_caps,
                             const uint64_t* flags, const uint64_t* epochs, uint8_t* out,
                             size_t cap, uint32_t* grid) {
  if (!n_msgs || !seg_counts || !segs || !dsts || !dst_caps || !flags || !epochs || !out || !grid)
    return dora::fail(DORA_ERR_INVALID, "NULL argument");
  if (n_msgs > 8) return dora::fail(DORA_ERR_INVALID, "batch of %zu messages", n_msgs);
  std::vector<std::vector<dora::Segment>> s(n_msgs);
  dora::BatchItem items[8];
  size_t k = 0;
  for (size_t m = 0; m < n_msgs; ++m) {
    for (size_t j = 0; j < seg_counts[m]; ++j, ++k)
      s[m].push_back({reinterpret_cast<const void*>(segs[3 * k]), segs[3 * k + 1], segs[3 * k + 2]});
    items[m] = {s[m].data(), s[m].size(), reinterpret_cast<uint8_t*>(dsts[m]),
                dora::FillSignal{reinterpret_cast<uint64_t*>(flags[m]), epochs[m], nullptr},
                dst_caps[m]};
  }
  return dora::build_aql_batch_args(items, n_msgs, out, cap, grid);
}

int dora_gpu_test_pack_segments(int body, size_t n_msgs, const size_t* seg_counts,
                                const uint64_t* segs, const uint64_t* dsts,
                                const uint64_t* dst_caps, uint32_t chunk_bytes, uint32_t grid,
                                dora_stream_t stream, uint32_t* flags_ok) {
  if (!seg_counts || !segs || !dsts || !dst_caps)
    return dora::fail(DORA_ERR_INVALID, "NULL argument");
  DORA_GUARD_BEGIN
  return dora::pack_probe(body, n_msgs, seg_counts, segs, dsts, dst_caps, chunk_bytes, grid,
                          static_cast<hipStream_t>(stream), flags_ok, nullptr, 0, nullptr);
  DORA_GUARD_END
}

int dora_gpu_test_pack_args(int body, size_t n_msgs, const size_t* seg_counts,
                            const uint64_t* segs, const uint64_t* dsts, const uint64_t* dst_caps,
                            uint32_t chunk_bytes, uint32_t grid, uint8_t* out, size_t cap,
                            size_t* out_len) {
  if (!seg_counts || !segs || !dsts || !dst_caps || !out)
    return dora::fail(DORA_ERR_INVALID, "NULL argument");
  DORA_GUARD_BEGIN
  return dora::pack_probe(body, n_msgs, seg_counts, segs, dsts, dst_caps, chunk_bytes, grid,
                          nullptr, nullptr, out, cap, out_len);
  DORA_GUARD_END
}

int dora_gpu_test_l2_touch(const void* data, size_t len, dora_stream_t stream) {
  if (!data && len) return dora::fail(DORA_ERR_INVALID, "data is NULL");
  return dora::launch_l2_touch(data, len, static_cast<hipStream_t>(stream));
}

int dora_gpu_test_l1_stale(int device, int mode, uint32_t* bad_first, uint32_t* stale,
                           uint32_t* blocks) {
  if (!bad_first || !stale || !blocks || mode < 0 || mode > 2)
    return dora::fail(DORA_ERR_INVALID, "bad l1 stale probe arguments");
  DORA_GUARD_BEGIN
  return dora::l1_stale_probe(device, mode, bad_first, stale, blocks);
  DORA_GUARD_END
}

int dora_gpu_test_fill_reached(const void* flag, uint64_t epoch) {
  if (!flag || (reinterpret_cast<uintptr_t>(flag) & 63))
    return dora::fail(DORA_ERR_INVALID, "fill flag must be 64-byte aligned");
  return dora::fill_reached(static_cast<const std::atomic<uint64_t>*>(flag), epoch) ? 1 : 0;
}

int dora_gpu_test_cp_arm(void* flag, uint64_t epoch) {
  if (!flag || (reinterpret_cast<uintptr_t>(flag) & 63) || epoch == 0)
    return dora::fail(DORA_ERR_INVALID, "fill flag must be 64-byte aligned, epoch > 0");
  dora::cp_arm(static_cast<dora::FillFlag*>(flag), epoch);
  return DORA_OK;
}


int dora_gpu_test_aql_hold(int device, int hold) { return dora::aql_hold(device, hold != 0); }

namespace {
hsa_status_t find_cpu_agent(hsa_agent_t a, void* p) {
  hsa_device_type_t t;
  if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) == HSA_STATUS_SUCCESS &&
      t == HSA_DEVICE_TYPE_CPU) {
    *static_cast<hsa_agent_t*>(p) = a;
    return HSA_STATUS_INFO_BREAK;
  }
  return HSA_STATUS_SUCCESS;
}
}  // namespace

int dora_gpu_test_d2h_copy_probe(int device, int mode, uint64_t bytes, uint32_t n,
                                 uint64_t gap_ns, uint64_t* out_ns) {
  if (!out_ns || !n || !bytes) return dora::fail(DORA_ERR_INVALID, "copy probe: arguments");
  DORA_HIP(hipSetDevice(device));
  void* src = nullptr;
  void* dst = nullptr;
  hipStream_t st = nullptr;
  DORA_HIP(hipMalloc(&src, bytes));
  DORA_HIP(hipMemset(src, 0x5a, bytes));
  DORA_HIP(hipHostMalloc(&dst, bytes, 0));
  DORA_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  DORA_HIP(hipDeviceSynchronize());
  hsa_agent_t gpu{}, cpu{};
  hsa_signal_t sig{0};
  if (mode == 1) {
    hsa_amd_pointer_info_t pi{};
    pi.size = sizeof(pi);
    if (hsa_init() != HSA_STATUS_SUCCESS ||
        hsa_amd_pointer_info(src, &pi, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS ||
        hsa_iterate_agents(find_cpu_agent, &cpu) != HSA_STATUS_INFO_BREAK ||
        hsa_signal_create(1, 0, nullptr, &sig) != HSA_STATUS_SUCCESS)
      return dora::fail(DORA_ERR_HIP, "copy probe: HSA setup");
    gpu = pi.agentOwner;
  }
  using clock = std::chrono::steady_clock;
  int rc = DORA_OK;
  for (uint32_t i = 0; i < n && rc == DORA_OK; ++i) {
    const auto until = clock::now() + std::chrono::nanoseconds(gap_ns);
    while (clock::now() < until) std::this_thread::yield();
    const auto t0 = clock::now();
    if (mode == 1) {
      hsa_signal_store_relaxed(sig, 1);
      if (hsa_amd_memory_async_copy(dst, cpu, src, gpu, bytes, 0, nullptr, sig) !=
          HSA_STATUS_SUCCESS) {
        rc = dora::fail(DORA_ERR_HIP, "hsa_amd_memory_async_copy");
        break;
      }
      while (hsa_signal_load_scacquire(sig) != 0) {
        __builtin_ia32_pause();
        if (clock::now() - t0 > std::chrono::seconds(2)) {
          rc = dora::fail(DORA_ERR_TIMEOUT, "copy probe: no completion");
          break;
        }
      }
    } else if (hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
               hipStreamSynchronize(st) != hipSuccess) {
      rc = dora::fail(DORA_ERR_HIP, "hipMemcpyAsync");
    }
    out_ns[i] = uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(clock::now() - t0).count());
  }
  if (rc == DORA_OK && static_cast<const uint8_t*>(dst)[bytes - 1] != 0x5a)
    rc = dora::fail(DORA_ERR_INVALID, "copy probe: wrong bytes");
  if (sig.handle && rc == DORA_OK) hsa_signal_destroy(sig);
  (void)hipStreamDestroy(st);
  (void)hipHostFree(dst);
  (void)hipFree(src);
  return rc;
}

// Experiment: what ordering a sample written on the node stream costs per message
// (dora_node_send_output_sample -> order_fill): `n` kernels writing `bytes` on one stream, each
// followed by nothing (mode 0), hipStreamWriteValue64 into pinned host memory like a fill flag
// (1), or a second 8-byte kernel (2).  out_ns[0] = host enqueue ns per message, out_ns[1] =
// enqueue + drain ns per message.
int dora_gpu_test_stream_order_probe(int device, int mode, uint64_t bytes, uint32_t n,
                                     uint64_t* out_ns) {
  if (!out_ns || !n || !bytes || mode < 0 || mode > 2)
    return dora::fail(DORA_ERR_INVALID, "stream order probe: arguments");
  DORA_HIP(hipSetDevice(device));
  void* buf = nullptr;
  void* tiny = nullptr;
  uint64_t* word = nullptr;
  hipStream_t st = nullptr;
  DORA_HIP(hipMalloc(&buf, bytes));
  DORA_HIP(hipMalloc(&tiny, 64));
  DORA_HIP(hipHostMalloc(reinterpret_cast<void**>(&word), 64, hipHostMallocMapped));
  DORA_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  DORA_HIP(hipDeviceSynchronize());
  int rc = DORA_OK;
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  for (uint32_t i = 0; i < n && rc == DORA_OK; ++i) {
    rc = dora_gpu_fill_splitmix(buf, bytes, i, st);
    if (rc != DORA_OK) break;
    if (mode == 1 && hipStreamWriteValue64(st, word, i + 1, 0) != hipSuccess)
      rc = dora::fail(DORA_ERR_HIP, "hipStreamWriteValue64");
    if (mode == 2) rc = dora_gpu_fill_splitmix(tiny, 8, i, st);
  }
  const auto t1 = clock::now();
  if (hipStreamSynchronize(st) != hipSuccess && rc == DORA_OK)
    rc = dora::fail(DORA_ERR_HIP, "hipStreamSynchronize");
  const auto t2 = clock::now();
  out_ns[0] = uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count()) / n;
  out_ns[1] = uint64_t(std::chrono::duration_cast<std::chrono::nanoseconds>(t2 - t0).count()) / n;
  if (rc == DORA_OK && mode == 1 && *reinterpret_cast<volatile uint64_t*>(word) != n)
    rc = dora::fail(DORA_ERR_INVALID, "stream order probe: flag %llu", (unsigned long long)*word);
  (void)hipStreamDestroy(st);
  (void)hipHostFree(word);
  (void)hipFree(tiny);
  (void)hipFree(buf);
  return rc;
}

int dora_gpu_test_reduce_timeout(uint64_t ns) {
  dora::aql_reduce_timeout(ns);
  return DORA_OK;
}

int dora_gpu_test_abandoned_slots(int device, uint32_t* slots) {
  if (!slots) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  *slots = dora::aql_abandoned_slots(device);
  return DORA_OK;
}

int dora_gpu_test_keep_awake_stats(int device, uint64_t* heartbeats, int* parked) {
  if (!heartbeats || !parked) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  bool pk = false;
  *heartbeats = dora::aql_heartbeats(device, &pk);
  *parked = pk ? 1 : 0;
  return DORA_OK;
}

int dora_gpu_test_aql_ring_wc(int device, int* wc, int* where) {
  if (!wc) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  bool b = false;
  const int rc = dora::aql_ring_write_combined(device, &b, where);
  *wc = b ? 1 : 0;
  return rc;
}

int dora_gpu_test_bcast_group(int device, void* buf, uint64_t bytes, int* nranks, int* rank) {
  if (!buf || !nranks || !rank) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  DORA_GUARD_BEGIN
  DORA_HIP(hipSetDevice(device));
  uint8_t uid[dora::kBcastIdBytes];
  int rc = dora::bcast_unique_id(uid);
  if (rc != DORA_OK) return rc;
  dora::BcastComm* c = nullptr;
  rc = dora::bcast_join(uid, 1, 0, 30000, &c);
  if (rc != DORA_OK) return rc;
  *nranks = dora::bcast_nranks(c);
  *rank = dora::bcast_rank(c);
  hipStream_t st = nullptr;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
    dora::bcast_close(c, nullptr, 0);
    return dora::fail(DORA_ERR_HIP, "hipStreamCreate");
  }
  rc = dora::bcast_enqueue(c, buf, bytes, st);
  if (rc == DORA_OK && hipStreamSynchronize(st) != hipSuccess)
    rc = dora::fail(DORA_ERR_HIP, "broadcast stream: %s", hipGetErrorString(hipGetLastError()));
  dora::bcast_close(c, st, 10000);
  (void)hipStreamDestroy(st);
  return rc;
  DORA_GUARD_END
}

int dora_gpu_test_bar_alloc(int device, size_t bytes, void** out) {
  if (!out) return dora::fail(DORA_ERR_INVALID, "out is NULL");
  return dora::bar_alloc(device, bytes, out);
}

int dora_gpu_test_bar_write(int device, void* dst, const void* src, size_t bytes) {
  if ((!dst || !src) && bytes) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::bar_write(device, dst, src, bytes);
}

void dora_gpu_test_bar_free(void* ptr) { dora::bar_free(ptr); }

int dora_gpu_test_gather_kernel(int mode) {
  if (mode < 0 || mode > 2) return dora::fail(DORA_ERR_INVALID, "gather kernel mode %d", mode);
  dora::gather_force(mode);
  return DORA_OK;
}

int dora_gpu_test_plan_gather(const dora_plan* plan, int* gather, const void** src, int* nd,
                              uint64_t* row, uint32_t* elem, int64_t* shape, int64_t* stride,
                              int64_t* lo, int64_t* hi) {
  if (!plan || !plan->dev_tensor || !plan->fields.empty())
    return dora::fail(DORA_ERR_INVALID, "not a device tensor plan");
  const dora::GatherDesc& g = plan->gd;
  if (gather) *gather = plan->launch != dora::PlanLaunch::kSegments;
  if (src) *src = g.view.src;
  if (nd) *nd = g.view.nd;
  if (row) *row = g.view.row;
  if (elem) *elem = g.elem;
  for (int i = 0; i < dora::kMaxTensorDims; ++i) {
    if (shape) shape[i] = i < g.view.nd ? g.view.shape[i] : 0;
    if (stride) stride[i] = i < g.view.nd ? g.view.stride[i] : 0;
  }
  if (lo) *lo = g.lo;
  if (hi) *hi = g.hi;
  return DORA_OK;
}

int dora_gpu_test_plan_field(const dora_plan* plan, size_t i, const void* dst, size_t* n_fields,
                             int* gather, uint64_t* dst_off, uint64_t* bytes, int* kind,
                             const void** src, int* nd, uint64_t* row, uint32_t* elem,
                             int64_t* shape, int64_t* stride, int64_t* lo, int64_t* hi) {
  if (!plan || !plan->dev_tensor || i >= plan->fields.size())
    return dora::fail(DORA_ERR_INVALID, "not a device struct-of-tensors plan with a field %zu", i);
  const dora::PlanField& f = plan->fields[i];
  const dora::GatherDesc& g = f.gd;
  if (n_fields) *n_fields = plan->fields.size();
  if (gather) *gather = plan->launch != dora::PlanLaunch::kSegments;
  if (dst_off) *dst_off = f.dst_off;
  if (bytes) *bytes = f.bytes;
  const bool taken_body = plan->launch == dora::PlanLaunch::kTaken ||
                          plan->launch == dora::PlanLaunch::kMasked;
  if (kind && taken_body) *kind = -1;
  else if (kind) *kind = dora::select_tile_dim(g, static_cast<const uint8_t*>(dst) + f.dst_off);
  if (src) *src = g.view.src;
  if (nd) *nd = g.view.nd;
  if (row) *row = g.view.row;
  if (elem) *elem = g.elem;
  for (int k = 0; k < dora::kMaxTensorDims; ++k) {
    if (shape) shape[k] = k < g.view.nd ? g.view.shape[k] : 0;
    if (stride) stride[k] = k < g.view.nd ? g.view.stride[k] : 0;
  }
  if (lo) *lo = g.lo;
  if (hi) *hi = g.hi;
  return DORA_OK;
}

int dora_gpu_test_plan_list(const dora_plan* plan, int* scan, const void** src, uint64_t* count,
                            int* wide, int* offsets_form, uint64_t* rows, int64_t* lo, int64_t* hi,
                            uint64_t* prefix_bytes) {
  if (!plan || !plan->about.list) return dora::fail(DORA_ERR_INVALID, "not a ragged-batch plan");
  const dora::ScanDesc& s = plan->scan;
  if (scan) *scan = plan->scan_on;
  if (src) *src = s.src;
  if (count) *count = s.count;
  if (wide) *wide = static_cast<int>(s.wide);
  if (offsets_form) *offsets_form = static_cast<int>(s.offsets);
  if (rows) *rows = s.n;
  const bool hbm = plan->scan_in_hbm();
  if (lo) *lo = hbm ? dora::scan_reach(s).lo : 0;
  if (hi) *hi = hbm ? dora::scan_reach(s).hi : 0;
  if (prefix_bytes) *prefix_bytes = plan->prefix.empty() ? 0 : plan->prefix[0].len;
  return DORA_OK;
}

int dora_gpu_test_plan_take(const dora_plan* plan, int* device, const void** index,
                            uint64_t* k, uint64_t* n, int* wide, int64_t* lo, int64_t* hi,
                            int64_t* stride0) {
  if (!plan || !plan->about.taken) return dora::fail(DORA_ERR_INVALID, "not a take plan");
  const bool dev = plan->launch == dora::PlanLaunch::kTaken;
  const dora::TakeDesc& t = plan->take;
  if (device) *device = dev;
  if (index) *index = dev ? t.src : nullptr;
  if (k) *k = plan->about.take_k;
  if (n) *n = plan->about.take_n;
  if (wide) *wide = static_cast<int>(plan->about.take_wide);
  if (lo) *lo = dev ? dora::take_reach(t).lo : 0;
  if (hi) *hi = dev ? dora::take_reach(t).hi : -1;
  for (size_t i = 0; stride0 && i < dora::kMaxStructFields; ++i)
    stride0[i] = dev && i < plan->fields.size() ? plan->fields[i].stride0 : 0;
  return DORA_OK;
}

int dora_gpu_test_plan_cast(const dora_plan* plan, size_t i, size_t* n_fields, int* is_cast,
                            int* src_code, int* src_bits, int* dst_code, int* dst_bits,
                            int* has_scale, float* scale, uint64_t* elements,
                            uint64_t* src_bytes, uint64_t* dst_bytes) {
  if (!plan || !plan->dev_tensor || i >= plan->fields.size())
    return dora::fail(DORA_ERR_INVALID, "not a device plan with a field %zu", i);
  const dora::PlanField& f = plan->fields[i];
  const dora::CastDesc& c = f.cast;
  if (n_fields) *n_fields = plan->fields.size();
  if (is_cast) *is_cast = plan->launch == dora::PlanLaunch::kCast && c.on;
  if (src_code) *src_code = c.on ? c.src_code : -1;
  if (src_bits) *src_bits = c.on ? c.src_bits : static_cast<int>(f.gd.elem * 8);
  if (dst_code) *dst_code = c.on ? 2 : -1;
  if (dst_bits) *dst_bits = c.on ? c.dst_bits : static_cast<int>(f.gd.elem * 8);
  if (has_scale) *has_scale = c.on && c.has_scale;
  if (scale) *scale = c.on ? c.scale : 1.0f;
  if (elements) *elements = c.on ? c.count : f.bytes / f.gd.elem;
  if (src_bytes) *src_bytes = f.gd.view.total;
  if (dst_bytes) *dst_bytes = f.bytes;
  return DORA_OK;
}

int dora_gpu_test_plan_quant(const dora_plan* plan, size_t i, int* is_quant, int* dst_code,
                             int* dst_bits, int* zero_point) {
  if (!plan || !plan->dev_tensor || i >= plan->fields.size())
    return dora::fail(DORA_ERR_INVALID, "not a device plan with a field %zu", i);
  const dora::CastDesc& c = plan->fields[i].cast;
  const bool q = plan->launch == dora::PlanLaunch::kCast && c.quant();
  if (is_quant) *is_quant = q;
  if (dst_code) *dst_code = q ? c.dst_code : -1;
  if (dst_bits) *dst_bits = q ? c.dst_bits : 0;
  if (zero_point) *zero_point = q ? c.zero_point : 0;
  return DORA_OK;
}

int dora_gpu_test_plan_affine(const dora_plan* plan, size_t i, int* is_affine,
                              const void** scale_table, const void** bias_table, uint64_t* inner,
                              uint64_t* channels, int* has_bias, float* bias, int64_t* lo,
                              int64_t* hi) {
  if (!plan || !plan->dev_tensor || i >= plan->fields.size())
    return dora::fail(DORA_ERR_INVALID, "not a device plan with a field %zu", i);
  const dora::CastDesc& c = plan->fields[i].cast;
  const bool on = plan->launch == dora::PlanLaunch::kCast && c.affine();
  const bool tables = on && (c.scale_tab || c.bias_tab);
  if (is_affine) *is_affine = on;
  if (scale_table) *scale_table = on ? c.scale_tab : nullptr;
  if (bias_table) *bias_table = on ? c.bias_tab : nullptr;
  if (inner) *inner = tables ? c.inner : 0;
  if (channels) *channels = tables ? c.channels : 0;
  if (has_bias) *has_bias = on && c.has_bias;
  if (bias) *bias = on ? c.bias : 0.0f;
  if (lo) *lo = tables ? dora::table_reach(nullptr, c.channels).lo : 0;
  if (hi) *hi = tables ? dora::table_reach(nullptr, c.channels).hi : -1;
  return DORA_OK;
}

int dora_gpu_test_reduce_body(int mode) {
  if (mode < 0 || mode > 2) return dora::fail(DORA_ERR_INVALID, "reduce body mode %d", mode);
  dora::reduce_force(mode);
  return DORA_OK;
}

int dora_gpu_test_plan_reduce(const dora_plan* plan, size_t i, const void* dst, int* op,
                              uint64_t* c, int64_t* axis_stride, uint64_t* outputs,
                              int* index_bits, int* body, uint64_t* vector_units,
                              uint64_t* element_units) {
  if (!plan || !plan->dev_tensor || i >= plan->fields.size())
    return dora::fail(DORA_ERR_INVALID, "not a device plan with a field %zu", i);
  namespace rd = dora::gather::reduce;
  const dora::PlanField& f = plan->fields[i];
  const dora::ReduceDesc& r = f.reduce;
  const bool on = plan->launch == dora::PlanLaunch::kReduce && r.on;
  const bool wave = on && dora::select_reduce_wave(f.gd, r);
  if (op) *op = on ? int(DORA_REDUCE_ARGMAX) : 0;
  if (c) *c = on ? r.c : 0;
  if (axis_stride) *axis_stride = on ? r.cstride : 0;
  if (outputs) *outputs = on ? r.count : 0;
  if (index_bits) *index_bits = on ? r.idx_bits : 0;
  if (body) *body = !on ? 0 : wave ? 2 : 1;
  uint64_t vec = 0, elem = 0;
  if (on && !wave) {
    // the lane body's units by the path each takes into a sample at `dst`
    const rd::Args a = rd::make_args(
        f.gd, r, const_cast<uint8_t*>(static_cast<const uint8_t*>(dst)) + f.dst_off);
    for (uint64_t u = 0; u < a.g.nunits; ++u) {
      rd::Start st;
      rd::start_of(a, a.g.head + (16 / a.dsize) * u, st);
      const bool v = a.dsize == 1   ? rd::unit_is_vector<1>(a, st)
                     : a.dsize == 2 ? rd::unit_is_vector<2>(a, st)
                     : a.dsize == 4 ? rd::unit_is_vector<4>(a, st)
                                    : rd::unit_is_vector<8>(a, st);
      ++(v ? vec : elem);
    }
  }
  if (vector_units) *vector_units = vec;
  if (element_units) *element_units = elem;
  return DORA_OK;
}

int dora_gpu_test_plan_resize(const dora_plan* plan, size_t i, const void* dst, int* mode,
                              uint64_t* outputs, int* dst_bits, int64_t* in_extent,
                              int64_t* out_extent, int64_t* axis_stride, uint64_t* head_elements,
                              uint64_t* units, uint64_t* tail_elements) {
  if (!plan || !plan->dev_tensor || i >= plan->fields.size())
    return dora::fail(DORA_ERR_INVALID, "not a device plan with a field %zu", i);
  namespace rs = dora::gather::resize;
  const dora::PlanField& f = plan->fields[i];
  const dora::ResizeDesc& r = f.resize;
  const bool on = dora::resizes(plan->launch) && r.on;
  if (mode) *mode = on ? int(r.mode) : 0;
  if (outputs) *outputs = on ? r.count : 0;
  if (dst_bits) *dst_bits = on ? r.dst_bits : 0;
  for (int j = 0; j < 2; ++j) {
    if (in_extent) in_extent[j] = on ? r.in[j] : 0;
    if (out_extent) out_extent[j] = on ? r.shape[r.ax[j]] : 0;
    if (axis_stride) axis_stride[j] = on ? r.stride[r.ax[j]] : 0;
  }
  uint64_t head = 0, nunits = 0, tail = 0;
  if (on) {
    // the body's division of a sample at `dst`: single elements, whole units, single elements
    const rs::Args a = rs::make_args(
        f.gd, r, const_cast<uint8_t*>(static_cast<const uint8_t*>(dst)) + f.dst_off);
    head = a.g.head;
    nunits = a.g.nunits;
    tail = a.g.total - head - (16u / a.dsize) * nunits;
  }
  if (head_elements) *head_elements = head;
  if (units) *units = nunits;
  if (tail_elements) *tail_elements = tail;
  return DORA_OK;
}

int dora_gpu_test_plan_crop(const dora_plan* plan, size_t i, const void* dst, int* mode,
                            uint64_t* k, const void** boxes, int* boxes_device, int64_t* lo,
                            int64_t* hi, uint64_t* head_elements, uint64_t* units,
                            uint64_t* tail_elements) {
  if (!plan || i >= plan->fields.size())
    return dora::fail(DORA_ERR_INVALID, "not a plan that keeps a field %zu", i);
  const dora::PlanField& f = plan->fields[i];
  const dora::CropDesc& c = f.crop;
  const bool on = dora::crops(plan->launch) && c.on;
  if (mode) *mode = on ? int(c.rs.mode) : 0;
  if (k) *k = on ? c.k : 0;
  if (boxes) *boxes = on ? c.boxes : nullptr;
  if (boxes_device) *boxes_device = on && plan->dev_tensor;
  const dora::GatherDesc reach = on ? dora::crop_reach(c) : dora::GatherDesc{};
  if (lo) *lo = reach.lo;
  if (hi) *hi = reach.hi;
  uint64_t head = 0, nunits = 0, tail = 0;
  if (on) {
    // the body's division of a sample at `dst`: single elements, whole units, single elements
    const dora::gather::crop::Args a = dora::gather::crop::make_args(
        f.gd, c, const_cast<uint8_t*>(static_cast<const uint8_t*>(dst)) + f.dst_off);
    head = a.r.g.head;
    nunits = a.r.g.nunits;
    tail = a.r.g.total - head - (16u / a.r.dsize) * nunits;
  }
  if (head_elements) *head_elements = head;
  if (units) *units = nunits;
  if (tail_elements) *tail_elements = tail;
  return DORA_OK;
}

int dora_gpu_test_fields_launches(uint64_t* counts) {
  if (!counts) return dora::fail(DORA_ERR_INVALID, "counts is NULL");
  dora::fields_launches(counts);
  return DORA_OK;
}

int dora_gpu_test_plan_mask(const dora_plan* plan, int* device, const void** mask, uint64_t* n,
                            int64_t* lo, int64_t* hi, uint64_t* workspace, uint64_t* part_words,
                            int64_t* stride0) {
  if (!plan || !plan->about.masked) return dora::fail(DORA_ERR_INVALID, "not a mask plan");
  const bool dev = plan->launch == dora::PlanLaunch::kMasked;
  const dora::MaskDesc& m = plan->mask;
  if (device) *device = dev;
  if (mask) *mask = dev ? m.src : nullptr;
  if (n) *n = plan->about.mask_n;
  if (lo) *lo = dev ? dora::mask_reach(m).lo : 0;
  if (hi) *hi = dev ? dora::mask_reach(m).hi : -1;
  if (part_words) *part_words = dev ? m.part_words : 0;
  if (workspace) {
    const dora::gather::mask::Workspace w =
        dev ? dora::gather::mask::workspace(plan->size, m.n, m.part_words)
            : dora::gather::mask::Workspace{};
    const uint64_t at[5] = {w.index, w.counts, w.totals, w.part, w.end};
    for (int i = 0; i < 5; ++i) workspace[i] = at[i];
  }
  for (size_t i = 0; stride0 && i < dora::kMaxStructFields; ++i)
    stride0[i] = dev && i < plan->fields.size() ? plan->fields[i].stride0 : 0;
  return DORA_OK;
}

int dora_gpu_test_plan_prep(const dora_plan* plan, size_t i, int* on, const void** scale_table,
                            const void** bias_table, uint64_t* channels, int* axis,
                            int64_t* inner, int64_t* lead, float* fill, int64_t* lo, int64_t* hi) {
  if (!plan || !plan->dev_tensor || i >= plan->fields.size())
    return dora::fail(DORA_ERR_INVALID, "not a device plan with a field %zu", i);
  const dora::PrepDesc& d = plan->fields[i].prep;
  const bool is = (plan->launch == dora::PlanLaunch::kResizePrep ||
                   plan->launch == dora::PlanLaunch::kCropPrep) && d.on;
  const bool tables = is && (d.scale_tab || d.bias_tab);
  if (on) *on = is;
  if (scale_table) *scale_table = is ? d.scale_tab : nullptr;
  if (bias_table) *bias_table = is ? d.bias_tab : nullptr;
  if (channels) *channels = tables ? d.channels : 0;
  if (axis) *axis = tables ? d.axis : -1;
  for (int j = 0; j < 2; ++j) {
    if (inner) inner[j] = is && d.placed ? d.inner[j] : 0;
    if (lead) lead[j] = is && d.placed ? d.lead[j] : 0;
  }
  if (fill) *fill = is && d.placed ? d.fill : 0.0f;
  if (lo) *lo = 0;
  if (hi) *hi = tables ? dora::table_reach(d.scale_tab, d.channels).hi : -1;
  return DORA_OK;
}

int dora_gpu_test_plan_launch(const dora_plan* plan, int* launch, int* scan, int* checked) {
  if (!plan) return dora::fail(DORA_ERR_INVALID, "plan is NULL");
  if (launch) *launch = static_cast<int>(plan->launch);
  if (scan) *scan = plan->scan_on;
  if (checked) *checked = plan->dev_tensor;
  return DORA_OK;
}

int dora_gpu_test_plan_segment_op(const dora_plan* plan, size_t i, uint32_t* op, uint32_t* aux,
                                  uint64_t* src_len) {
  if (!plan || i >= plan->segs.size())
    return dora::fail(DORA_ERR_INVALID, "segment index %zu out of range", i);
  if (op) *op = plan->segs[i].op;
  if (aux) *aux = plan->segs[i].aux;
  if (src_len) *src_len = plan->segs[i].src_len;
  return DORA_OK;
}

int dora_gpu_test_ide_output(const char* dataflow_id, const char* node_id,
                                        const char* output_id, const uint8_t* type_info,
                                        size_t type_info_len, const uint8_t* params,
                                        size_t params_len, uint64_t meta_ns, uint64_t event_ns,
                                        const uint8_t* hlc_id, const uint8_t* data, size_t data_len,
                                        int has_data, uint8_t* out, size_t cap, size_t* out_len) {
  if (!dataflow_id || !node_id || !output_id || !type_info || !hlc_id || (params_len && !params) ||
      (data_len && !data))
    return dora::fail(DORA_ERR_INVALID, "NULL argument");
  dora::InterDaemonEvent e;
  e.kind = dora::IDE_OUTPUT;
  e.dataflow_id = dataflow_id;
  e.node_id = node_id;
  e.output_id = output_id;
  e.type_info.assign(type_info, type_info + type_info_len);
  if (params_len) e.parameters.assign(params, params + params_len);
  e.timestamp_ns = meta_ns;
  e.event_ns = event_ns;
  std::memcpy(e.hlc_id.data(), hlc_id, 16);
  e.has_data = has_data != 0;
  if (data_len) e.data.assign(data, data + data_len);
  std::vector<uint8_t> f;
  try {
    dora::encode_ide(e, f);
  } catch (const std::exception& ex) {
    return dora::fail(DORA_ERR_INVALID, "%s", ex.what());
  }
  return dora::copy_out(f, out, cap, out_len);
}

int dora_gpu_test_ide_inputs_closed(const char* dataflow_id,
                                               const char* const* receivers,
                                               const char* const* inputs, size_t n,
                                               uint64_t event_ns, const uint8_t* hlc_id,
                                               uint8_t* out, size_t cap, size_t* out_len) {
  if (!dataflow_id || !hlc_id || (n && (!receivers || !inputs)))
    return dora::fail(DORA_ERR_INVALID, "NULL argument");
  dora::InterDaemonEvent e;
  e.kind = dora::IDE_INPUTS_CLOSED;
  e.dataflow_id = dataflow_id;
  for (size_t i = 0; i < n; ++i) e.inputs.emplace_back(receivers[i], inputs[i]);
  e.event_ns = event_ns;
  std::memcpy(e.hlc_id.data(), hlc_id, 16);
  std::vector<uint8_t> f;
  try {
    dora::encode_ide(e, f);
  } catch (const std::exception& ex) {
    return dora::fail(DORA_ERR_INVALID, "%s", ex.what());
  }
  return dora::copy_out(f, out, cap, out_len);
}

int dora_gpu_test_ide_decode(const uint8_t* frame, size_t len, char* json, size_t cap,
                                        size_t* json_len) {
  if (!frame && len) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  dora::InterDaemonEvent e;
  try {
    e = dora::decode_ide(frame, len);
  } catch (const std::exception& ex) {
    return dora::fail(DORA_ERR_INVALID, "%s", ex.what());
  }
  using dora::hex;
  using dora::jstr;
  std::string j = "{\"kind\": " + std::to_string(e.kind) + ", \"dataflow_uuid\": \"" +
                  hex(e.dataflow_uuid.data(), 16) + "\", \"event_ns\": " +
                  std::to_string(e.event_ns);
  if (e.kind == dora::IDE_OUTPUT) {
    j += ", \"node_id\": " + jstr(e.node_id) + ", \"output_id\": " + jstr(e.output_id) +
         ", \"metadata_version\": " + std::to_string(e.meta_version) +
         ", \"meta_ns\": " + std::to_string(e.timestamp_ns) + ", \"type_info\": \"" +
         hex(e.type_info.data(), e.type_info.size()) + "\", \"parameters\": \"" +
         hex(e.parameters.data(), e.parameters.size()) + "\", \"has_data\": " +
         (e.has_data ? "true" : "false") + ", \"data\": \"" + hex(e.data.data(), e.data.size()) +
         "\"";
  } else {
    j += ", \"inputs\": [";
    for (size_t i = 0; i < e.inputs.size(); ++i)
      j += (i ? ", [" : "[") + jstr(e.inputs[i].first) + ", " + jstr(e.inputs[i].second) + "]";
    j += "]";
  }
  j += "}";
  std::vector<uint8_t> v(j.begin(), j.end());
  v.push_back(0);
  return dora::copy_out(v, reinterpret_cast<uint8_t*>(json), cap, json_len);
}

}  // extern "C"
