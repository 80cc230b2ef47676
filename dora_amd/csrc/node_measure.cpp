
// The benchmark's instrumentation: timing-event pairs of every n-th pack (PackTiming), the
// timed region and its packs' own stamps (TimedRegion), the host time per send phase.  The send
// path touches it only through the `prof` and `timed` members of dora_node.
#include "node_internal.h"

namespace dora {

// The stamps of a timed region's pack (the caller has seen `region_epoch` set on a slot with a
// flag), read from its flag line before the slot's next fill
// overwrites them (the flag must already show the pack's epoch).
void harvest_region_stamp(dora_node* n, Slot* s) {
  const FillFlag& ff = n->core->region->hdr()->nodes[n->core->idx].fill[s->flag];
  if (s->region_cp_area >= 0 && ff.epoch.load(std::memory_order_acquire) != s->region_epoch &&
      ff.cp_epoch.load(std::memory_order_acquire) == s->region_epoch) {
    n->timed.cp_used.push_back(uint32_t(s->region_cp_area));  // resolved at region_end
  } else if (ff.epoch.load(std::memory_order_acquire) == s->region_epoch) {
    // an in-kernel-signalled fill (its workgroup 0 stamps the line)
    n->timed.fold(ff.t_start, ff.t_end);
  }
  s->region_epoch = 0;
  s->region_cp_area = -1;
}

// Stamp areas for timed regions' CP-signalled packs (dora_node_region_begin), made and zeroed with
// the node's AQL queues at its first send, never inside or just before a region (without them,
// e.g. no large BAR, such packs signal in-kernel inside regions).
void ensure_cp_stamps(dora_node* n) {
  if (n->timed.cp_stamps || n->core->device < 0) return;
  const size_t bytes = size_t(kRegionCpAreas) * kCpAreaWords * 8;
  void* d = nullptr;
  if (bar_alloc(n->core->device, bytes, &d) != DORA_OK) {
    clear_error();
    return;  // no large BAR: a region's packs signal in-kernel
  }
  const std::vector<uint8_t> zero(bytes, 0);
  if (bar_write(n->core->device, d, zero.data(), bytes) != DORA_OK) {
    bar_free(d);
    clear_error();
    return;
  }
  n->timed.cp_stamps = static_cast<uint64_t*>(d);
  void* idx = nullptr;
  void* out = nullptr;
  if (hipHostMalloc(&idx, kRegionCpAreas * 4, hipHostMallocCoherent) == hipSuccess &&
      hipHostMalloc(&out, kRegionCpAreas * 16, hipHostMallocCoherent) == hipSuccess) {
    n->timed.reduce_idx = static_cast<uint32_t*>(idx);
    n->timed.reduce_out = static_cast<uint64_t*>(out);
  } else {
    (void)hipGetLastError();  // region ends read the areas through the BAR
    if (idx) (void)hipHostFree(idx);
  }
}

constexpr size_t kTimingPairs = 64;
constexpr size_t kMaxIntervals = 1 << 16;  // stamped packs whose (start, stop) are kept

void PackTiming::harvest(TimingPair& p) {
  if (!p.pending) return;
  float ms = 0;
  if (hipEventSynchronize(p.stop) == hipSuccess &&
      hipEventElapsedTime(&ms, p.start, p.stop) == hipSuccess) {
    pack_ms += ms;
    ++pack_count;
    pack_bytes += p.bytes;
    float a = 0, b = 0;
    if (timing_ref && intervals.size() < 2 * kMaxIntervals &&
        hipEventElapsedTime(&a, timing_ref, p.start) == hipSuccess &&
        hipEventElapsedTime(&b, timing_ref, p.stop) == hipSuccess) {
      intervals.push_back(a);
      intervals.push_back(b);
    }
  }
  (void)hipGetLastError();
  p.pending = false;
}

static int ensure_timing(dora_node* n) {
  PackTiming& t = n->prof;
  if (!t.timing.empty()) return DORA_OK;
  DeviceScope ds(n->core->device);
  DORA_HIP(hipEventCreate(&t.timing_ref));
  t.timing.resize(kTimingPairs);
  for (auto& p : t.timing) {
    DORA_HIP(hipEventCreate(&p.start));
    DORA_HIP(hipEventCreate(&p.stop));
  }
  return DORA_OK;
}

TimingPair* PackTiming::next_pair(uint64_t bytes) {
  if (timing.empty()) return nullptr;
  TimingPair& p = timing[timing_next++ % timing.size()];
  harvest(p);  // normally long complete
  p.bytes = bytes;
  p.pending = true;
  return &p;
}

PackTiming::~PackTiming() {
  harvest_all();
  for (auto& p : timing) {
    (void)hipEventDestroy(p.start);
    (void)hipEventDestroy(p.stop);
  }
  if (timing_ref) (void)hipEventDestroy(timing_ref);
}

// Runs when dora_node_free deletes the node, after it has freed the node's slots.
TimedRegion::~TimedRegion() {
  if (start) (void)hipEventDestroy(start);
  for (hipEvent_t e : stop) (void)hipEventDestroy(e);
  if (cp_stamps) {
    aql_fence_all();  // no pack of this node may still write its stamps
    bar_free(cp_stamps);
  }
  if (reduce_idx) (void)hipHostFree(reduce_idx);
  if (reduce_out) (void)hipHostFree(reduce_out);
}

}  // namespace dora

extern "C" {

int dora_node_pack_stats(dora_node* n, uint64_t* count, double* total_ms, uint64_t* bytes) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  n->prof.harvest_all();  // waits for the stamps of packs still in flight
  if (count) *count = n->prof.pack_count;
  if (total_ms) *total_ms = n->prof.pack_ms;
  if (bytes) *bytes = n->prof.pack_bytes;
  return DORA_OK;
}

}  // extern "C"

namespace dora {
namespace {

// Record the region's stop events: one after the last pack queued on each fill stream and on
// the node stream.  No wait.
int region_record_stops(dora_node* n) {
  DeviceScope ds(n->core->device);
  std::vector<hipStream_t> ss = n->core->fill_streams;
  ss.push_back(n->core->stream);
  while (n->timed.stop.size() < ss.size()) {  // fill streams are created lazily
    hipEvent_t e = nullptr;
    DORA_HIP(hipEventCreate(&e));
    n->timed.stop.push_back(e);
  }
  for (size_t i = 0; i < ss.size(); ++i) DORA_HIP(hipEventRecord(n->timed.stop[i], ss[i]));
  n->timed.marked = true;
  return DORA_OK;
}

}  // namespace
}  // namespace dora

extern "C" {

int dora_node_set_timing_period(dora_node* n, uint64_t period) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  n->prof.timing_period = period;
  return DORA_OK;
}

int dora_node_region_begin(dora_node* n) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (n->core->device < 0) return dora::fail(DORA_ERR_INVALID, "host-only node");
  dora::DeviceScope ds(n->core->device);
  dora::TimedRegion& r = n->timed;
  if (!r.start) DORA_HIP(hipEventCreate(&r.start));
  r.cp_next = 0;
  r.cp_used.clear();
  r.armed = true;
  r.started = false;
  r.packs = r.bytes = r.aql = 0;
  r.stamped = r.unstamped = r.tmin = r.tmax = 0;
  r.ticks.clear();
  return DORA_OK;
}

int dora_node_region_mark(dora_node* n) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (!n->timed.armed) return dora::fail(DORA_ERR_INVALID, "no region begun");
  if (!n->timed.started || !n->timed.unstamped) return DORA_OK;  // stamped packs need none
  return dora::region_record_stops(n);
}

int dora_node_region_end(dora_node* n, double* span_ms, uint64_t* packs, uint64_t* bytes) {
  if (!n || !span_ms) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  dora::TimedRegion& r = n->timed;
  if (!r.armed) return dora::fail(DORA_ERR_INVALID, "no region begun");
  dora::DeviceScope ds(n->core->device);
  r.armed = false;
  const bool marked = r.marked;
  r.marked = false;
  *span_ms = 0;
  if (packs) *packs = r.packs;
  if (bytes) *bytes = r.bytes;
  if (!r.unstamped) {
    // every pack stamped its own device time: first workgroup start of the earliest to the
    // signal of the last (s_memrealtime); harvest the stamps not yet read at slot reuse
    std::vector<dora::Slot*> live(n->cache.begin(), n->cache.end());
    for (auto& kv : n->sent_out) live.push_back(kv.second);
    for (dora::Slot* s : live)
      if (s->region_epoch && !dora::wait_slot_idle(n, s))
        return dora::fail(DORA_ERR_TIMEOUT, "a timed pack did not complete within 10 s");
    if (r.cp_next) {
      // CP-signalled packs: their first workgroup's start and their last workgroup's end, read
      // from the stamp areas through the BAR (written through by the packs, all of which have
      // completed).  An area's other words are older packs' (earlier regions), never the max.
      r.cp_next = 0;
      // one AQL dispatch reduces every used area to (start, latest end) in host memory; the
      // BAR read is the fallback (~0.3 ms of uncached reads per area)
      const uint32_t na = uint32_t(std::min<size_t>(r.cp_used.size(), dora::kRegionCpAreas));
      bool reduced = false;
      if (na && r.reduce_idx) {
        std::copy(r.cp_used.begin(), r.cp_used.begin() + na, r.reduce_idx);
        std::fill(r.reduce_out, r.reduce_out + 2 * na, uint64_t(0));
        const int rrc = dora::aql_stamp_reduce(n->core->device, r.cp_stamps,
                                               uint32_t(dora::kCpAreaWords), r.reduce_idx, na,
                                               r.reduce_out);
        reduced = rrc == DORA_OK;
        if (rrc == DORA_ERR_TIMEOUT) {
          // the reduction may still run and write them: leak both (later regions read the BAR)
          r.reduce_idx = nullptr;
          r.reduce_out = nullptr;
        }
        if (!reduced) dora::clear_error();
      }
      std::vector<uint64_t> w(dora::kCpAreaWords);
      for (uint32_t j = 0; j < r.cp_used.size(); ++j) {
        if (reduced && j < na) {
          r.fold(__atomic_load_n(r.reduce_out + 2 * j, __ATOMIC_ACQUIRE),
                 __atomic_load_n(r.reduce_out + 2 * j + 1, __ATOMIC_ACQUIRE));
        } else {
          std::memcpy(w.data(), r.cp_stamps + size_t(r.cp_used[j]) * dora::kCpAreaWords,
                      w.size() * 8);
          r.fold(w[0], *std::max_element(w.begin() + 1, w.end()));
        }
      }
      r.cp_used.clear();
    }
    if (r.stamped) *span_ms = double(r.tmax - r.tmin) / dora::kRealtimeHz * 1e3;
    if (packs) *packs = r.stamped;
    if (bytes && r.packs) *bytes = r.bytes / r.packs * r.stamped;
    return DORA_OK;
  }
  if (!r.started) return DORA_OK;
  // fallback (packs without kernel stamps): the first pack's start event to events recorded
  // after the last pack on each fill stream and the node stream, by dora_node_region_mark right
  // after the last send, or now
  if (!marked) {
    int rc = dora::region_record_stops(n);
    if (rc != DORA_OK) return rc;
    r.marked = false;
  }
  const size_t ns = n->core->fill_streams.size() + 1;
  for (size_t i = 0; i < ns && i < r.stop.size(); ++i) {
    DORA_HIP(hipEventSynchronize(r.stop[i]));
    float ms = 0;
    DORA_HIP(hipEventElapsedTime(&ms, r.start, r.stop[i]));
    *span_ms = std::max<double>(*span_ms, ms);
  }
  return DORA_OK;
}

int dora_node_pack_intervals(dora_node* n, double* out_ms, size_t cap, size_t* count) {
  if (!n || !count || (!out_ms && cap)) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  if (!n->timed.ticks.empty()) {
    // the last timed region's packs, from their own stamps, ms after the earliest start
    const size_t pairs = n->timed.ticks.size() / 2;
    *count = pairs;
    for (size_t i = 0; i < 2 * std::min(cap, pairs); ++i)
      out_ms[i] = double(n->timed.ticks[i] - n->timed.tmin) / dora::kRealtimeHz * 1e3;
    return DORA_OK;
  }
  n->prof.harvest_all();
  const size_t pairs = n->prof.intervals.size() / 2;
  *count = pairs;
  for (size_t i = 0; i < 2 * std::min(cap, pairs); ++i) out_ms[i] = n->prof.intervals[i];
  return DORA_OK;
}

int dora_node_send_profile(dora_node* n, double* out_us, size_t n_out, uint64_t* count) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  const dora::PackTiming& t = n->prof;
  const double c = t.phase_count ? double(t.phase_count) : 1.0;
  for (size_t i = 0; i < n_out && i < 4; ++i) out_us[i] = double(t.phase_ns[i]) / c / 1000.0;
  if (count) *count = t.phase_count;
  return DORA_OK;
}

int dora_node_set_profiling(dora_node* n, int enable) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (enable) {
    if (n->core->device < 0) return dora::fail(DORA_ERR_INVALID, "host-only node");
    int rc = dora::ensure_timing(n);
    if (rc != DORA_OK) return rc;
  }
  dora::PackTiming& t = n->prof;
  t.harvest_all();
  t.profile = enable != 0;
  t.intervals.clear();
  if (enable) {
    // time origin of dora_node_pack_intervals
    DORA_HIP(hipEventRecord(t.timing_ref, n->core->stream));
    DORA_HIP(hipEventSynchronize(t.timing_ref));
  }
  for (auto& x : t.phase_ns) x = 0;
  t.phase_count = 0;
  t.pack_count = 0;
  t.timing_seq = 0;
  t.pack_ms = 0;
  t.pack_bytes = 0;
  return DORA_OK;
}

}  // extern "C"
