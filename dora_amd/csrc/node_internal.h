
// The node's types and the functions its source files (node.cpp, node_slots.cpp, node_send.cpp,
// node_recv.cpp, node_measure.cpp) share.  Private to the library: not installed, and nothing
// under include/ names it.
#pragma once
#include <hip/hip_runtime_api.h>
#include <pthread.h>
#include <unistd.h>
#include <x86intrin.h>

#include <algorithm>
#include <chrono>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <memory_resource>
#include <mutex>
#include <new>
#include <thread>
#include <set>
#include <sstream>
#include <random>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "aql.h"
#include "bcast.h"
#include "common.h"
#include "device_array.h"
#include "dora_gpu.h"
#include "plan.h"
#include "shm.h"
#include "stdout_capture.h"
#include "subprof.h"
#include "trace.h"
#include "wire.h"

namespace dora {

// HIP's current device is per thread, and the library acts on the node's GPU from whichever
// thread calls it — an EventStream moved to another thread (the reference's is Send), an async
// pump, the event-stream thread: slots, IPC mappings, events, streams and receive buffers are
// created on the current device.  Every place that creates one (or launches through HIP) makes
// the node's device current for that step and gives the caller's back afterwards.  The steady
// send and receive paths (cached slot, cached mapping, AQL dispatch) create nothing and take no
// scope: hipGetDevice alone costs ~54 ns per call (scripts/get_device_probe.cpp).
struct DeviceScope {
  int prev = -1;
  explicit DeviceScope(int device) {
    int cur = -1;
    if (device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != device &&
        hipSetDevice(device) == hipSuccess)
      prev = cur;
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceScope(const DeviceScope&) = delete;
  DeviceScope& operator=(const DeviceScope&) = delete;
};

// FNV-1a over 64-bit words, continuing from `h` (the hash of IPC keys and of plan keys).
constexpr uint64_t kFnvBasis = 0xcbf29ce484222325ull;
inline uint64_t fnv1a_words(const uint64_t* w, size_t n, uint64_t h = kFnvBasis) {
  for (size_t i = 0; i < n; ++i) h = (h ^ w[i]) * 0x100000001b3ull;
  return h;
}

// A received slot's identity as a hash key without a heap allocation per lookup: the
// hipIpcMemHandle_t bytes plus the owner's pid and its process-unique slot id.  The handle alone
// is not enough: a freed slot's handle encoding can recur for a new allocation of the same size.
struct IpcKey {
  uint8_t b[64];
  int32_t pid;
  uint64_t slot;
  bool operator==(const IpcKey& o) const {
    return pid == o.pid && slot == o.slot && std::memcmp(b, o.b, 64) == 0;
  }
};
struct IpcKeyHash {
  size_t operator()(const IpcKey& k) const {
    uint64_t w[8];
    std::memcpy(w, k.b, 64);
    const uint64_t h = fnv1a_words(w, 8, kFnvBasis ^ k.slot ^ (uint64_t(uint32_t(k.pid)) << 40));
    return static_cast<size_t>(h ^ (h >> 29));
  }
};

// One hipIpcOpenMemHandle mapping of a producer's slot.  Shared by the receiver's mapping cache
// and every input that points into it; closed when the last of them lets go, so evicting a
// mapping from the cache never unmaps memory an input still reads.
struct IpcMapping {
  void* base = nullptr;
  uint64_t last_use = 0;
  ~IpcMapping() {
    if (base) (void)hipIpcCloseMemHandle(base);
  }
};

// A host-only producer's shared-memory sample region as mapped here (DataMessage::SharedMemory),
// shared like IpcMapping.  A device receiver registers it with HIP once, so its pull into HBM is a
// DMA from pinned pages rather than a staged copy.
struct ShmMapping {
  void* base = nullptr;
  size_t len = 0;
  bool registered = false, reg_tried = false;  // pinned for DMA on the first pull (ensure_local)
  uint64_t last_use = 0;
  ~ShmMapping() {
    if (registered) (void)hipHostUnregister(base);
    shmem_unmap(base, len);
  }
};

// Mappings a receiver keeps open for reuse (LRU beyond this).  Producers recycle at most
// kMaxCacheSlots slots plus those in flight, so a steady edge stays within it; slots a producer
// has freed (size changes) age out instead of pinning the producer's memory for good.
constexpr size_t kMaxIpcMappings = 128;
// Shared-memory regions a device receiver keeps mapped and pinned while nothing holds them: at
// most this many bytes (the least recently used unheld ones are unpinned and unmapped first), so
// regions a producer has dropped do not stay page-locked in every receiver.
constexpr uint64_t kMaxCachedShmBytes = uint64_t(1) << 30;

struct Slot {
  void* ptr = nullptr;
  // bytes the slot holds (its whole 2 MiB-grain allocation): the cache's best-fit key.  The
  // reference keys on the requested length (Shmem::len); a slot's full capacity lets a 4 MiB
  // sample reuse a slot first made for 4,096,000 B (the ladder's next size created fresh slots,
  // hipMalloc + export + the receiver's mapping, for ~20 of its sends).
  uint64_t cap = 0;
  uint64_t id = 0;
  hipIpcMemHandle_t handle;
  int flag = -1;              // FillFlag index in the node's region entry (async sends)
  uint64_t fill_epoch = 0;    // epoch the last fill into this slot stores into `flag`
  uint64_t region_epoch = 0;  // that fill belongs to a timed region: harvest its stamps
  int region_cp_area = -1;    // ... its stamp area, if the command processor signalled it
  hipEvent_t done = nullptr;  // fallback: interprocess completion event of the last fill
  hipIpcEventHandle_t done_handle;
  // node-stream work on the slot with no fill flag (a broadcast group's pack + broadcast):
  // recorded after it, waited on before the slot is reused or freed
  hipEvent_t use_ev = nullptr;
  bool use_pending = false;
  // host-only node: a POSIX shared-memory region (DataMessage::SharedMemory) instead of HBM
  bool host = false;
  std::string shm_name;
  // a device node's shared-memory slot (host_bound_sample): page-locked and mapped for the GPU,
  // which packs into it
  bool registered = false;
  // device slot mapped for the CPU through the large BAR (host sources written in place,
  // host_bar_fill): tried once per slot
  bool bar = false, bar_tried = false;
};

// Slots are whole 2 MiB allocations: HIP sub-allocates smaller hipMallocs from shared blocks,
// and an IPC import of such a slot failed ("invalid device pointer") when the exporting process
// freed other memory of the block meanwhile (two nodes in one process, r01).
inline uint64_t slot_bytes(uint64_t len) {
  constexpr uint64_t kSlotGrain = 2ull << 20;
  return (std::max<uint64_t>(len, 1) + kSlotGrain - 1) / kSlotGrain * kSlotGrain;
}

// Streams the HIP-launched fills of a node rotate over (host sources, compacting transforms,
// relays; device-source packs go to the AQL queues, aql.h).  Three (r01: HIP-launched device
// packs overlapped their ramps and tails over three hardware queues, 40.96 MB 17.1 -> 13.2 us per
// message, profiles/r01_stream_probe.jsonl) until r06: device packs have left for the AQL
// queues, and every HIP stream costs one of the GPU's 24 compute queues.
constexpr size_t kFillStreams = 1;

// With profiling on, every n-th pack launch is stamped with timing events (default period;
// dora_node_set_timing_period)
constexpr uint64_t kTimingPeriod = 8;

enum PeerCopyMode { PEER_KERNEL, PEER_SDMA };

// Slots of every node in this process by process-wide id: a sample whose owner is this process
// (another node here, or the node itself) is read in place — IPC handles cannot be opened in
// the process that exported them.
struct OwnSlots {
  std::mutex mu;
  std::unordered_map<uint64_t, void*> ptrs;
  std::atomic<uint64_t> next_id{1};
};
OwnSlots& own_slots();

// Buffers recycled by size: `get` hands out the smallest pooled one that holds `len` unless it
// is more than twice as large, else a new one of whole pages from `alloc`; `put` keeps at most
// kMaxPooled, evicting the smallest.  `mu` may guard more than this pool.
struct SizePool {
  std::mutex& mu;
  const int& device;
  void* (*alloc)(uint64_t bytes, int device);
  void (*release)(void* p);
  std::multimap<uint64_t, void*> pooled;
  static constexpr size_t kMaxPooled = 16;

  void* get(uint64_t len, uint64_t* cap) {
    {
      std::lock_guard<std::mutex> g(mu);
      auto it = pooled.lower_bound(len);
      if (it != pooled.end() && it->first <= 2 * len + 4096) {
        void* p = it->second;
        *cap = it->first;
        pooled.erase(it);
        return p;
      }
    }
    *cap = (len + 4095) / 4096 * 4096;
    return alloc(*cap, device);
  }
  void put(void* p, uint64_t cap) {
    std::lock_guard<std::mutex> g(mu);
    if (pooled.size() >= kMaxPooled) {
      auto it = pooled.begin();  // evict the smallest
      release(it->second);
      pooled.erase(it);
    }
    pooled.emplace(cap, p);
  }
  void clear() {
    for (auto& kv : pooled) release(kv.second);
    pooled.clear();
  }
};
inline void* alloc_hbm(uint64_t bytes, int device) {
  void* p = nullptr;
  DeviceScope ds(device);
  return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
}
inline void* alloc_pinned(uint64_t bytes, int) {
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes, hipHostMallocPortable | hipHostMallocMapped) == hipSuccess) return p;
  (void)hipGetLastError();
  return nullptr;
}

// Sender-side waits for a fill flag give up after this long.
constexpr uint64_t kFillWaitNs = 10000000000ull;
// Pause-spin until fill flag `f` shows `epoch`; false once mono_ns() has passed `deadline_ns`.
inline bool wait_fill(const std::atomic<uint64_t>* f, uint64_t epoch, uint64_t deadline_ns) {
  while (!fill_reached(f, epoch)) {
    if (mono_ns() > deadline_ns) return false;
    __builtin_ia32_pause();
  }
  return true;
}

// State shared between the node handle and input data that may outlive events.
struct NodeCore {
  std::unique_ptr<Region> region;
  int idx = -1;
  int device = 0;
  hipStream_t stream = nullptr;
  // Whether anything may be queued on `stream`: the caller once it has it (dora_node_stream), or
  // this library's own asynchronous node-stream work (pulls, forwards).  Until then a send needs
  // no query of the stream (~150 ns of hipStreamQuery per send and per released input).
  std::atomic<bool> stream_used{false};
  bool stream_busy() {
    return stream_used.load(std::memory_order_relaxed) && hipStreamQuery(stream) == hipErrorNotReady;
  }
  // Fill streams (kFillStreams): HIP-launched fills rotate over them.  Work already queued on the
  // node stream is ordered before a fill (node_ev), and fills are ordered before node-stream
  // work queued after dora_node_stream() hands the stream out (fence_fills).
  std::vector<hipStream_t> fill_streams;
  std::vector<hipEvent_t> fill_events;
  std::vector<uint8_t> fill_dirty;
  hipEvent_t node_ev = nullptr;
  hipEvent_t sync_ev = nullptr;  // dora_node_sync's marker
  size_t fill_next = 0;
  bool fill_streams_tried = false;
  // fills dispatched on the AQL queue and not yet seen complete (fence_fills waits for them)
  std::vector<std::pair<const std::atomic<uint64_t>*, uint64_t>> aql_pending;
  // every kernel-signalled fill not yet seen complete (AQL and fill streams): dora_node_sync
  // waits for their flags instead of synchronising streams
  std::vector<std::pair<const std::atomic<uint64_t>*, uint64_t>> flag_pending;
  std::vector<uint8_t> fill_unsignalled;  // per fill stream: work not covered by a fill flag

  // One entry per fill flag with the latest epoch ordered on it (a flag's epochs only grow, so
  // waiting for the latest covers the earlier ones).  Matching by pointer reads no flag: the
  // flags are host lines the GPU writes, and pruning by loading them cost a cache miss each
  // (64 per prune, ~0.4 us per send amortised over the two lists).  The list stays as long as
  // the node has slots with flags; only past 256 entries are completed ones pruned.
  static void note(std::vector<std::pair<const std::atomic<uint64_t>*, uint64_t>>& v,
                   const std::atomic<uint64_t>* f, uint64_t epoch) {
    for (auto& x : v)
      if (x.first == f) {
        x.second = std::max(x.second, epoch);
        return;
      }
    if (v.size() >= 256) {
      size_t k = 0;
      for (auto& x : v)
        if (!fill_reached(x.first, x.second)) v[k++] = x;
      v.resize(k);
    }
    v.push_back({f, epoch});
  }
  RingWriter req;
  RingReader ev;
  RingReader drops;
  std::mutex req_mu;
  std::mutex ipc_mu;
  // (handle, owner pid, slot id) -> open mapping; bounded LRU (kMaxIpcMappings)
  std::unordered_map<IpcKey, std::shared_ptr<IpcMapping>, IpcKeyHash> ipc_cache;
  uint64_t ipc_clock = 0;
  std::atomic<uint64_t> ipc_opens{0}, ipc_closes{0};

  // Drop the least recently used mappings that no input holds until the cache is within bound.
  void trim_ipc_cache() {
    while (ipc_cache.size() > kMaxIpcMappings) {
      auto victim = ipc_cache.end();
      for (auto it = ipc_cache.begin(); it != ipc_cache.end(); ++it)
        if (it->second.use_count() == 1 &&
            (victim == ipc_cache.end() || it->second->last_use < victim->second->last_use))
          victim = it;
      if (victim == ipc_cache.end()) return;  // every mapping is held by an input
      ipc_cache.erase(victim);
      ipc_closes.fetch_add(1, std::memory_order_relaxed);
    }
  }
  // shared-memory region name -> mapping (host-only producers' samples); bounded like ipc_cache
  std::unordered_map<std::string, std::shared_ptr<ShmMapping>> shm_cache;

  std::shared_ptr<ShmMapping> map_shmem(const std::string& name, uint64_t len, std::string* err) {
    std::lock_guard<std::mutex> g(ipc_mu);
    auto it = shm_cache.find(name);
    std::shared_ptr<ShmMapping> m;
    if (it != shm_cache.end()) {
      m = it->second;
    } else {
      m = std::make_shared<ShmMapping>();
      m->base = shmem_open(name, &m->len);
      if (!m->base) {
        *err = "shared-memory sample `" + name + "`: " + std::strerror(errno);
        return nullptr;
      }
      shm_cache.emplace(name, m);
      // bounded by count and by bytes; mappings an input still holds stay
      for (;;) {
        uint64_t bytes = 0;
        for (auto& kv : shm_cache) bytes += kv.second->len;
        if (shm_cache.size() <= kMaxIpcMappings && bytes <= kMaxCachedShmBytes) break;
        auto victim = shm_cache.end();
        for (auto v = shm_cache.begin(); v != shm_cache.end(); ++v)
          if (v->second != m && v->second.use_count() == 1 &&
              (victim == shm_cache.end() || v->second->last_use < victim->second->last_use))
            victim = v;
        if (victim == shm_cache.end()) break;
        shm_cache.erase(victim);
      }
    }
    if (len > m->len) {
      *err = "shared-memory sample `" + name + "` is shorter than its message";
      return nullptr;
    }
    m->last_use = ++ipc_clock;
    return m;
  }
  std::unordered_map<std::string, hipEvent_t> ipc_events;  // event handle bytes -> opened event
  // fill flags: the region is host-registered so the stream can write epochs into it
  uint8_t* region_dev = nullptr;
  uint32_t* fill_done = nullptr;  // device: per fill flag, kMaxSignalWgs workgroup done words
  dora::AqlQueue* aql = nullptr;  // this process's AQL queues of `device` (fill_sample)
  bool aql_tried = false;
  // The usable AQL queue or null; looked up once (a global lock), then kept.
  AqlQueue* aql_queue_once() {
    if (!aql_tried) {
      aql_tried = true;
      aql = aql_queue(device);
    }
    return aql_usable(aql) ? aql : nullptr;
  }
  std::vector<uint32_t> free_flags;
  uint64_t epoch = 0;

  // Receive pool for cross-GPU edges: local HBM copies of remote samples, recycled by size.
  std::mutex pool_mu;
  SizePool recv_pool{pool_mu, device, alloc_hbm, [](void* p) { (void)hipFree(p); }, {}};
  std::set<int> peer_enabled;  // peer devices this node's device may access (under ipc_mu)
  std::atomic<uint64_t> peer_copies{0}, peer_bytes{0};  // cross-GPU samples pulled

  // RCCL broadcast groups this node receives on (input id -> communicator); every receive is
  // posted on bcast_stream in the order the daemon routed the samples
  std::map<std::string, BcastComm*> bcast_in;
  hipStream_t bcast_stream = nullptr;
  std::string bcast_error;
  uint64_t bcast_recvs = 0, bcast_bytes = 0;

  // Host-only receiver (device < 0): device samples are staged into pinned host memory (one DMA
  // per input, stage_to_host), recycled by size like the receive pool.  Pinned allocations cost
  // milliseconds at the large sizes, so a steady edge reuses its buffers.
  SizePool host_pool{pool_mu, device, alloc_pinned, [](void* p) { (void)hipHostFree(p); }, {}};
  std::map<int, hipStream_t> stage_streams;  // per producer GPU (under pool_mu)
  std::atomic<uint64_t> host_staged{0}, host_staged_bytes{0};

  // A private stream of GPU `src_device` for copies waited for alone (a host-only receiver's
  // staging, a device receiver's pulls); the current device must be it
  hipStream_t stage_stream(int src_device) {
    std::lock_guard<std::mutex> g(pool_mu);
    auto it = stage_streams.find(src_device);
    if (it != stage_streams.end()) return it->second;
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    stage_streams[src_device] = s;
    return s;
  }

  uint64_t* flag_dev(int idx) const {
    const uint8_t* host = reinterpret_cast<const uint8_t*>(&region->hdr()->nodes[this->idx].fill[idx]);
    return reinterpret_cast<uint64_t*>(region_dev + (host - region->base()));
  }

  // True when the daemon was asleep and had to be woken (the message trace notes it).
  bool ring_doorbell() {
    // the daemon sets `daemon_sleeping` before it reads the doorbell and re-checks the rings;
    // the fence orders the request's head store before our load of the flag (shm.cpp's ring
    // wake-up argument), so the doorbell is only bumped for a sleeping daemon
    RegionHdr* h = region->hdr();
    std::atomic_thread_fence(std::memory_order_seq_cst);
    if (h->daemon_sleeping.load(std::memory_order_relaxed)) {
      h->doorbell.fetch_add(1, std::memory_order_seq_cst);
      futex_wake(&h->doorbell);
      return true;
    }
    return false;
  }
  bool last_rang = false;  // the last request woke the daemon (trace only)

  int request(uint32_t kind, const std::vector<uint8_t>& payload) {
    return request(kind, payload.data(), payload.size());
  }
  int request(uint32_t kind, const uint8_t* payload, size_t len) {
    {
      std::lock_guard<std::mutex> g(req_mu);
      if (!req.fits(len))
        return fail(DORA_ERR_INVALID, "message of %zu bytes exceeds the control ring", len);
      if (!req.push(kind, payload, len, 30000000))
        return fail(DORA_ERR_TIMEOUT, "daemon did not drain the request ring for 30 s");
    }
    last_rang = ring_doorbell();
    return DORA_OK;
  }

  void report_drop_token(const DropToken& t) {
    // count (u32) + token, encoded on the stack: released inputs allocate nothing
    uint8_t b[4 + sizeof(DropToken)];
    const uint32_t one = 1;
    std::memcpy(b, &one, 4);
    std::memcpy(b + 4, &t, sizeof(DropToken));
    (void)request(REQ_REPORT_DROP_TOKENS, b, sizeof(b));
  }

  // The stream the next fill runs on (round robin), ordered after the node stream's queued work.
  void ensure_fill_streams() {
    if (!fill_streams.empty() || fill_streams_tried) return;
    fill_streams_tried = true;
    DeviceScope ds(device);
    if (hipEventCreateWithFlags(&node_ev, hipEventDisableTiming) == hipSuccess) {
      for (size_t i = 0; i < kFillStreams; ++i) {
        hipStream_t s = nullptr;
        hipEvent_t e = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) break;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
          (void)hipStreamDestroy(s);
          break;
        }
        fill_streams.push_back(s);
        fill_events.push_back(e);
      }
      fill_dirty.assign(fill_streams.size(), 0);
      fill_unsignalled.assign(fill_streams.size(), 0);
    }
    (void)hipGetLastError();
  }

  // Order stream `s` after the work queued on the node stream so far (producer kernels of a source).
  void order_after_node_stream(hipStream_t s) {
    if (stream_busy()) {
      if (!node_ev) {
        DeviceScope ds(device);
        (void)hipEventCreateWithFlags(&node_ev, hipEventDisableTiming);
      }
      if (node_ev && hipEventRecord(node_ev, stream) == hipSuccess) (void)hipStreamWaitEvent(s, node_ev, 0);
    }
    (void)hipGetLastError();
  }

  hipStream_t next_fill_stream() {
    ensure_fill_streams();
    if (fill_streams.empty()) {
      stream_used.store(true, std::memory_order_relaxed);  // fills on the node stream itself
      return stream;
    }
    const size_t i = fill_next++ % fill_streams.size();
    hipStream_t s = fill_streams[i];
    if (stream_busy()) {
      // producer kernels of the source may still run on the node stream
      if (hipEventRecord(node_ev, stream) == hipSuccess) (void)hipStreamWaitEvent(s, node_ev, 0);
    }
    (void)hipGetLastError();
    fill_dirty[i] = 1;
    return s;
  }

  const std::atomic<uint64_t>* flag_host(int i) const {
    return &region->hdr()->nodes[idx].fill[i].epoch;
  }

  // Order every fill launched so far before work queued on the node stream from now on.
  void fence_fills() {
    // AQL fills are on no HIP stream: wait for their flags on the host (one bound for all)
    const uint64_t deadline = mono_ns() + kFillWaitNs;
    for (auto& x : aql_pending) (void)wait_fill(x.first, x.second, deadline);
    aql_pending.clear();
    for (size_t i = 0; i < fill_streams.size(); ++i) {
      if (!fill_dirty[i]) continue;
      fill_dirty[i] = 0;
      if (hipStreamQuery(fill_streams[i]) == hipSuccess) continue;  // already drained
      if (hipEventRecord(fill_events[i], fill_streams[i]) == hipSuccess)
        (void)hipStreamWaitEvent(stream, fill_events[i], 0);
    }
    (void)hipGetLastError();
  }

  ~NodeCore() {
    for (auto& kv : bcast_in) bcast_close(kv.second, bcast_stream, 10000);
    if (bcast_stream) (void)hipStreamDestroy(bcast_stream);
    // AQL argument slots must not keep pointing at this region's fill flags once it is unmapped
    if (device >= 0 && region) aql_forget_flags(device, region->base(), region->size());
    for (auto& kv : ipc_events) (void)hipEventDestroy(kv.second);
    ipc_cache.clear();
    for (hipStream_t s : fill_streams) {
      (void)hipStreamSynchronize(s);
      (void)hipStreamDestroy(s);
    }
    for (hipEvent_t e : fill_events) (void)hipEventDestroy(e);
    if (node_ev) (void)hipEventDestroy(node_ev);
    if (sync_ev) (void)hipEventDestroy(sync_ev);
    if (stream) (void)hipStreamSynchronize(stream);
    recv_pool.clear();
    for (auto& kv : stage_streams) {
      (void)hipStreamSynchronize(kv.second);
      (void)hipStreamDestroy(kv.second);
    }
    host_pool.clear();
    if (fill_done) (void)hipFree(fill_done);
    if (region_dev) (void)hipHostUnregister(region->base());
    if (stream) (void)hipStreamDestroy(stream);
  }
};

// The received sample of one input; reports the drop token when the last owner releases it.
struct InputData {
  std::shared_ptr<NodeCore> core;
  const void* ptr = nullptr;
  uint64_t len = 0;
  uint64_t ext_len = 0;       // bytes of the sample incl. its validity tail (>= len)
  bool has_token = false;
  DropToken token{};
  std::vector<uint8_t> vec;   // inline (Vec) samples stay on the host
  std::shared_ptr<IpcMapping> mapping;  // the producer's slot as mapped here (IPC edges)
  void* local = nullptr;      // cross-GPU edge: local copy in this node's receive pool
  uint64_t local_cap = 0;
  int remote_device = -1;     // >= 0: `ptr` is a peer GPU's slot not yet pulled (ensure_local)
  hipEvent_t bcast_ev = nullptr;  // broadcast group input: completion of its receive into `local`
  std::shared_ptr<ShmMapping> shm;  // a host-only producer's shared-memory sample, mapped here
  bool host_mem = false;   // host receiver: `ptr` is host memory (shared memory read in place,
                           // or a device sample staged into `host_local`)
  bool host_pull = false;  // device receiver: `ptr` is shared memory not yet pulled into HBM
  void* host_local = nullptr;  // host-only receiver: pinned copy of a device sample (stage_to_host)
  uint64_t host_local_cap = 0;
  ~InputData() {
    if (!core) return;
    if (bcast_ev) {
      (void)hipEventSynchronize(bcast_ev);
      (void)hipEventDestroy(bcast_ev);
    }
    if (has_token || local) {
      // consumer reads on the node stream must be complete before the memory is reused
      SubSpan sq(SP_STREAM_QUERY);
      if (core->stream && core->stream_used.load(std::memory_order_relaxed) &&
          hipStreamQuery(core->stream) != hipSuccess)
        (void)hipStreamSynchronize(core->stream);
    }
    if (has_token) {
      SubSpan sp(SP_RECV_RELEASE);
      core->report_drop_token(token);
      trace(TP_RELEASED, token);
    }
    if (local) core->recv_pool.put(local, local_cap);
    if (host_local) core->host_pool.put(host_local, host_local_cap);
  }
};

}  // namespace dora

struct dora_sample {
  dora::Slot* slot = nullptr;
  std::vector<uint8_t> vec;  // zero-length samples (Vec path)
  uint64_t len = 0;
  uint64_t ext_len = 0;      // slot bytes filled: len + the validity tail (0: len)
  uint8_t fill = dora::FILL_DONE;  // how the receiver learns the fill completed
  uint64_t epoch = 0;
  bool stamped = false;  // the pack kernel stamps its start / signal time into the flag line
  bool read_signalled = false;  // its pack raises the flag line's read word (aql.h aql_pack)
  // dora_sample_fill_ticket: the caller's own kernel raises the flag to `epoch`; the send queues
  // no stream operation for it
  bool self_published = false;
};

namespace dora {
// Kernel-duration stamps of async packs (hipExtLaunchKernel start/stop), harvested lazily.
struct TimingPair {
  hipEvent_t start = nullptr, stop = nullptr;
  uint64_t bytes = 0;
  bool pending = false;
};

// Profiling of the pack kernel (dora_node_set_profiling) and the host time per send phase.
struct PackTiming {
  bool profile = false;
  std::vector<TimingPair> timing;  // ring of kTimingPairs
  size_t timing_next = 0;
  uint64_t timing_seq = 0;
  uint64_t timing_period = 0;       // stamp every n-th pack (0: kTimingPeriod)
  hipEvent_t timing_ref = nullptr;  // recorded when profiling is (re)enabled
  std::vector<double> intervals;    // (start, stop) ms after timing_ref per stamped pack
  uint64_t pack_count = 0, pack_bytes = 0;
  double pack_ms = 0;
  // host time per send phase: allocate (incl. backpressure), launch, fill sync/record, send
  uint64_t phase_ns[4] = {0, 0, 0, 0};
  uint64_t phase_count = 0;
  void harvest(TimingPair& p);
  void harvest_all() {
    for (auto& p : timing) harvest(p);
  }
  TimingPair* next_pair(uint64_t bytes);
  ~PackTiming();
};

// Stamp areas of a timed region's CP-signalled packs: [0] start, [1 + k mod kCpStampWgs] the
// latest end of the workgroups k mapping there.
constexpr uint32_t kRegionCpAreas = 256;
constexpr size_t kCpAreaWords = 1 + kCpStampWgs;

// Timed region (dora_node_region_begin/end): the first pack after begin stamps its start;
// end records a stop event on every fill stream once the packs queued there have finished.
struct TimedRegion {
  bool armed = false, started = false, marked = false;
  uint64_t aql = 0;  // packs of the region dispatched on the AQL queue
  // kernel stamps (s_memrealtime ticks) of the region's packs, harvested from their flag lines
  uint64_t stamped = 0, unstamped = 0, tmin = 0, tmax = 0;
  std::vector<uint64_t> ticks;  // (start, end) stamps of the region's packs
  // stamp areas of a region's CP-signalled packs (aql.h aql_pack `cp_stamps`): device memory the
  // host reads through the BAR (stamps written to host memory held every pack's end for their
  // PCIe writes: C3 0.44-0.52 of HBM), made and zeroed at the node's first send (ensure_cp_stamps).
  // No HIP work around a
  // region: a memset or copy on a HIP stream right before a region made its first send take
  // 25-45 us instead of 4 (profiles/r03_cp_signal_ab.jsonl, first_send_ab).  Areas are never
  // re-zeroed: an area's stale words are an earlier pack's, older than the current pack's own.
  uint64_t* cp_stamps = nullptr;  // coarse-grained device memory, host-mapped (aql.h bar_alloc)
  // region end: the used areas' indices and their (start, end) pairs, pinned host memory the
  // stamp reduction (aql_stamp_reduce) reads and writes
  uint32_t* reduce_idx = nullptr;
  uint64_t* reduce_out = nullptr;
  uint32_t cp_next = 0;
  std::vector<uint32_t> cp_used;
  hipEvent_t start = nullptr;
  std::vector<hipEvent_t> stop;
  uint64_t packs = 0, bytes = 0;
  // Fold one pack's (start, end) stamps into the region's span, count and tick list: at slot
  // reuse (harvest_region_stamp) and at the region's end (CP-signalled packs).
  void fold(uint64_t a, uint64_t b) {
    if (!a || b < a) return;
    if (!stamped || a < tmin) tmin = a;
    if (!stamped || b > tmax) tmax = b;
    ++stamped;
    if (ticks.size() < 2 * (1u << 16)) {
      ticks.push_back(a);
      ticks.push_back(b);
    }
  }
  ~TimedRegion();
};

// Plans of recent device-array sends by plan_key (a sender re-sending the same buffers, e.g. a
// ring of preallocated frames, plans each once): the plan and its serialized type info
struct PlanCache {
  struct Entry {
    std::vector<uint64_t> key;
    dora_plan* plan = nullptr;
    std::vector<uint8_t> ti;
    uint64_t last_use = 0;
  };
  std::vector<Entry> entries;
  std::unordered_map<uint64_t, size_t> index;  // hash of a key -> its entry
  std::vector<uint64_t> key_buf;                // the key of the last find
  uint64_t clock = 0, hits = 0;
  static uint64_t hash(const std::vector<uint64_t>& key) {
    return fnv1a_words(key.data(), key.size());
  }
  // The cached plan of these buffers, or null; `*cacheable` then says whether the plan built
  // next may be inserted (the buffers have a key, and no other key holds its hash).
  Entry* find(const ArrowArray* array, const ArrowSchema* schema, bool* cacheable);
  // Keep `plan` under the key of the last find (the least recently used entry goes beyond 64).
  Entry* insert(dora_plan* plan);
  ~PlanCache() {
    for (auto& e : entries) delete e.plan;
  }
};
}  // namespace dora

struct dora_event {
  int type = 0;
  std::string id;
  dora::Metadata meta;
  std::shared_ptr<dora::InputData> data;
  std::string error;
  bool pending = false;  // device input not yet completed (fill wait / cross-GPU pull)
  uint64_t arrived_ns = 0;  // mono_ns when the descriptor was drained (transit age bound)
  dora::DeviceIpc ipc{};
  // dora_event_type_info's reference (inline-validity) form, built on first request when the
  // type info points into the sample's validity tail
  mutable bool ti_checked = false;
  mutable std::vector<uint8_t> ti_inline;
};

struct dora_node {
  std::shared_ptr<dora::NodeCore> core;
  std::string id;
  std::set<std::string> outputs;
  std::map<std::string, uint32_t> queue_size;
  size_t min_queue_size = 0;  // smallest value of queue_size
  std::deque<dora::Slot*> cache;
  // samples sent, by drop token (map nodes from a pool: no malloc per send)
  std::pmr::unsynchronized_pool_resource sent_pool;
  std::pmr::unordered_map<dora::DropToken, dora::Slot*, dora::DropTokenHash> sent_out{&sent_pool};
  dora::WBuf send_buf;                 // request encoding scratch of send_sample, reused
  std::vector<uint8_t> ti_buf;         // type-info scratch of pack_and_send, reused
  dora_plan bytes_plan;                // send_output_bytes: the one-buffer plan, re-pointed
  std::vector<uint8_t> bytes_ti;       // ... and its type info for a sample of bytes_ti_len
  uint64_t bytes_ti_len = 0;
  std::deque<std::unique_ptr<dora_event>> queue;
  bool ended = false;
  // samples dora_node_allocate_data_sample handed out and not yet sent or discarded
  std::unordered_set<dora_sample*> samples_live;
  // Event-stream thread (dora_node_set_event_thread; started by every node that joins an RCCL
  // broadcast group as a receiver): the reference's event_stream_loop (event_stream/thread.rs:
  // 81-188) — it drains the daemon's ring into `queue` continuously and applies the drop-oldest
  // policy there (node_communication/mod.rs:320-359), so inputs keep arriving, their broadcast
  // receives are posted and the tokens of dropped inputs go back while the user thread is busy
  // elsewhere.  `qmu` guards `queue` and `ended` while it runs.
  std::thread pump;
  std::mutex qmu;
  std::condition_variable qcv;
  std::atomic<bool> pump_on{false}, pump_stop{false};
  bool want_pump = false;  // a broadcast group was joined: start the thread at the next chance
  bool pin_pending = false;  // host-only node not yet in the dataflow's L3 domain (pin_host_node)
  // The benchmark's instrumentation (node_measure.cpp) and the plan cache; destroyed, with the
  // GPU resources they own, in reverse order when dora_node_free deletes the node, after it has
  // freed the slots.
  dora::TimedRegion timed;
  dora::PackTiming prof;
  dora::PlanCache plans;
  uint64_t aql_packs = 0, hip_packs = 0;  // fills by dispatch path
  uint64_t bar_fills = 0;  // host sources written into their slot by the CPU (host_bar_fill)
  // outputs whose every receiver has no GPU (the daemon's AllNodesReady): device sources up to
  // kHostPackMax are packed straight into shared memory for them (host_bound_sample)
  std::set<std::string, std::less<>> host_bound;
  // samples put straight into shared memory for such outputs: device arrays packed there by the
  // GPU (host_bound_sample), host sources copied there by the CPU
  uint64_t host_packs = 0, host_copies = 0;
  bool aql_ready = false;  // the process's AQL queues were set up (first non-empty sample)
  uint64_t slots_created = 0, cache_hits = 0, dropped_inputs = 0;
  std::vector<uint8_t> drop_buf;  // payload buffer of handle_finished_drop_tokens
  std::vector<uint8_t> ev_buf;    // payload buffer of drain_events
  bool compact = false;                    // send_output uses compacting plans
  // DORA_SEND_ASYNC for every send (DORA_GPU_SEND_ASYNC=1): device-source sends return before
  // their pack has read the source
  bool async_default = false;
  // RCCL broadcast groups of this node's fan-out outputs (rank 0 of each), DORA_GPU_FANOUT=rccl.
  // Each output packs and broadcasts on a stream of its own: a rank that stalls the collective
  // holds up that output only (its slots, then its in-flight cap), not the node stream nor the
  // node's other outputs.
  struct BcastOut {
    dora::BcastComm* comm = nullptr;
    hipStream_t stream = nullptr;
  };
  std::map<std::string, BcastOut> bcast_out;
  uint64_t bcast_seq = 0;
  dora::StdoutCapture* stdout_capture = nullptr;  // send_stdout_as (DORA_GPU_SEND_STDOUT_AS)
  // zero-copy forwards: the input re-sent in place, kept (and its producer's token held) until
  // the forward's own token returns
  std::unordered_map<dora::DropToken, std::shared_ptr<dora::InputData>, dora::DropTokenHash>
      forwarded;
  uint64_t zero_copy_forwards = 0;
  // in-place samples (dora_node_send_output_sample) by ordering: a stream operation of the send
  // after the node stream, or the caller's own kernel (dora_sample_fill_ticket)
  uint64_t samples_stream_ordered = 0, samples_self_published = 0;
};

namespace dora {

// Which of the node's pending lists a flag fill is noted on.  dora_node_sync and fence_fills
// reach a fill whose flag a stream operation writes (order_fill) through that stream, so it is
// noted nowhere.  A fill whose flag a kernel on a HIP stream raises (an in-kernel-signalled pack,
// a ticket's kernel) is noted for dora_node_sync, which waits for flags rather than for HIP to
// see the kernel end; fence_fills orders it through its stream.  An AQL fill is on no stream:
// both lists.
enum FillNote { NOTE_NONE, NOTE_SYNC, NOTE_SYNC_AND_FENCE };

// Make `s` a flag fill of `epoch`: receivers poll its slot's flag for it, and so does the
// slot's next reuse.
inline void mark_flag_fill(NodeCore* c, dora_sample* s, uint64_t epoch, FillNote note) {
  s->epoch = epoch;
  s->fill = FILL_FLAG;
  s->slot->fill_epoch = epoch;
  if (note == NOTE_NONE) return;
  const std::atomic<uint64_t>* f = c->flag_host(s->slot->flag);
  if (note == NOTE_SYNC_AND_FENCE) NodeCore::note(c->aql_pending, f, epoch);
  NodeCore::note(c->flag_pending, f, epoch);
}

// node_slots.cpp
void release_slot_memory(Slot* s);
int self_pid();
bool wait_slot_idle(dora_node* n, Slot* s, uint64_t timeout_ns = kFillWaitNs);
void free_slot(dora_node* n, Slot* s);
void drain_slot_reaper();
void add_to_cache(dora_node* n, Slot* s);
void on_token(dora_node* n, const DropToken& t);
int handle_finished_drop_tokens(dora_node* n);
int allocate_slot(dora_node* n, uint64_t len, Slot** out);
int allocate_host_slot(dora_node* n, uint64_t len, Slot** out);
// node_send.cpp
void discard_sample(dora_node* n, dora_sample* s);
dora_sample* vec_sample(const uint8_t* p, size_t len);
int proxy_send(dora_node* n, const char* output_id, const uint8_t* ti, size_t ti_len,
               const uint8_t* params, size_t params_len, dora_sample* sample, uint64_t ts);
// node_recv.cpp
PeerCopyMode peer_copy_mode();
bool edge_copy_forced();
int ensure_peer_access(NodeCore* c, int src_device);
int enqueue_peer_copy(NodeCore* c, void* dst, const void* src, int src_device, uint64_t len);
int ensure_local(InputData* in);
void encode_event(dora_node* n, uint32_t kind, const std::vector<uint8_t>& p);
void start_pump(dora_node* n);
void stop_pump(dora_node* n);
// node_measure.cpp
void harvest_region_stamp(dora_node* n, Slot* s);
void ensure_cp_stamps(dora_node* n);

}  // namespace dora
