
// The lifetime of a sender's slots: allocation, the best-fit cache of recycled ones, the wait
// for a slot's last fill before it is refilled or freed, and the returned drop tokens that put
// a slot back into the cache.
#include "node_internal.h"

namespace dora {
namespace {

// A sender's slot cache (mod.rs:365: 20 entries).  Device slots are HBM, and freeing one costs
// the sender 0.5-1 ms of hipFree and the GPU a TLB invalidation while its packs run; a sender
// whose message sizes change (the bench's ladders, variable point clouds) evicted slots at every
// size change.  So the cache keeps the reference's 20 entries and more, up to kMaxCacheSlots, as
// long as they hold at most slot_cache_bytes() (DORA_GPU_SLOT_CACHE_BYTES, default 4 GiB of the
// GPU's 288 GB; 0: the reference's 20 entries); evicted slots are freed off the send path.
constexpr size_t kMaxCacheSize = 20;          // mod.rs:365
constexpr size_t kMaxCacheSlots = 64;
uint64_t slot_cache_bytes() {
  static const uint64_t v = [] {
    const char* e = std::getenv("DORA_GPU_SLOT_CACHE_BYTES");
    return e ? std::strtoull(e, nullptr, 10) : uint64_t(4) << 30;
  }();
  return v;
}

}  // namespace

// The memory of a slot no fill can still write (its events, its HBM or shared-memory region).
void release_slot_memory(Slot* s) {
  if (s->host) {
    if (s->registered) (void)hipHostUnregister(s->ptr);
    shmem_unmap(s->ptr, s->cap);
    shmem_unlink(s->shm_name);
  } else {
    if (s->done) (void)hipEventDestroy(s->done);
    if (s->use_ev) (void)hipEventDestroy(s->use_ev);
    (void)hipFree(s->ptr);
  }
  delete s;
}

// getpid() is a system call on current glibc; the descriptor path asks for it per message.
// Cached per process, refreshed in a forked child.
int self_pid() {
  static std::atomic<int> pid{0};
  static std::once_flag once;
  std::call_once(once, [] { pthread_atfork(nullptr, nullptr, [] { pid.store(0); }); });
  int p = pid.load(std::memory_order_relaxed);
  if (!p) {
    p = static_cast<int>(getpid());
    pid.store(p, std::memory_order_relaxed);
  }
  return p;
}

OwnSlots& own_slots() {
  static OwnSlots* o = new OwnSlots();  // never destroyed: nodes may outlive static teardown
  return *o;
}

// A returned drop token does not prove that the slot's last fill has completed: the daemon
// returns the token at once for an output without receivers, a receiver's drop-oldest queue
// releases inputs it never waited on, and a finished receiver's tokens are released for it.
// Before a slot is refilled or freed, wait for its last fill (normally long complete: one load).
// False when the fill did not complete within `timeout_ns` — the slot must then be neither
// reused nor freed (a kernel may still write it).
bool wait_slot_idle(dora_node* n, Slot* s, uint64_t timeout_ns) {
  if (s->flag >= 0 && s->fill_epoch) {
    if (!wait_fill(n->core->flag_host(s->flag), s->fill_epoch, mono_ns() + timeout_ns))
      return false;
    if (s->region_epoch) harvest_region_stamp(n, s);
  }
  if (s->done && hipEventQuery(s->done) == hipErrorNotReady &&
      hipEventSynchronize(s->done) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  if (s->use_pending) {
    if (hipEventSynchronize(s->use_ev) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    s->use_pending = false;
  }
  return true;
}

// Retire a slot: out of own_slots, its last fill waited for, its fill flag back to the node.
// False when there is nothing to free — no slot, or a fill that never completed and may still
// write the slot (and its flag's done words): both are leaked rather than handed to another
// allocation.
static bool retire_slot(dora_node* n, Slot* s) {
  if (!s) return false;
  {
    std::lock_guard<std::mutex> g(own_slots().mu);
    own_slots().ptrs.erase(s->id);
  }
  if (!wait_slot_idle(n, s)) {
    std::fprintf(stderr, "dora-gpu: slot %llu: last fill did not complete; not freed\n",
                 (unsigned long long)s->id);
    return false;
  }
  if (s->flag >= 0) n->core->free_flags.push_back(static_cast<uint32_t>(s->flag));
  s->flag = -1;
  return true;
}

void free_slot(dora_node* n, Slot* s) {
  if (retire_slot(n, s)) release_slot_memory(s);
}

namespace {

// Slots evicted from a sender's cache are freed by a process-wide thread, not on the send path:
// hipFree of a 40.96 MB slot took 0.5-1 ms inside the first send after a size change (the
// eviction happens when returned tokens are handled in alloc_sample), which made one message in
// two hundred cost a millisecond — the slow mode of bench.py's 40.96 MB ladder step
// (first_send 0.5-1.0 ms, alloc_us, in profiles/r04_py40_first_send.jsonl).  Freed off the send
// path, the packs running meanwhile still slowed by ~0.3 us each (the unmapping), hence the
// larger cache above.  The sender still
// waits for the slot's last fill and takes back its fill flag; the thread only destroys the
// slot's events and frees its memory.  dora_node_free and exit drain it.
struct SlotReaper {
  std::mutex mu;
  std::condition_variable cv, idle;
  std::deque<std::pair<int, Slot*>> q;
  size_t busy = 0;
  bool started = false;

  void push(int device, Slot* s) {
    std::unique_lock<std::mutex> g(mu);
    if (!started) {
      started = true;
      std::thread([this] { run(); }).detach();
      std::atexit([] { reaper().drain(); });  // before HIP's own teardown (registered earlier)
      // a forked child has no reaper thread: it starts its own, and forgets the parent's queue
      pthread_atfork(nullptr, nullptr, [] {
        SlotReaper& r = reaper();
        new (&r.mu) std::mutex();
        new (&r.cv) std::condition_variable();
        new (&r.idle) std::condition_variable();
        r.q.clear();
        r.busy = 0;
        r.started = false;
      });
    }
    q.emplace_back(device, s);
    cv.notify_one();
  }
  void run() {
    std::unique_lock<std::mutex> g(mu);
    for (;;) {
      cv.wait(g, [this] { return !q.empty(); });
      auto [dev, s] = q.front();
      q.pop_front();
      ++busy;
      g.unlock();
      int prev = -1;
      (void)hipGetDevice(&prev);
      if (dev >= 0 && prev != dev) (void)hipSetDevice(dev);
      release_slot_memory(s);
      (void)hipGetLastError();
      g.lock();
      --busy;
      if (q.empty() && !busy) idle.notify_all();
    }
  }
  void drain() {
    std::unique_lock<std::mutex> g(mu);
    idle.wait(g, [this] { return q.empty() && !busy; });
  }
  static SlotReaper& reaper() {
    static SlotReaper* r = new SlotReaper();  // never destroyed: its thread is detached
    return *r;
  }
};

void free_slot_deferred(dora_node* n, Slot* s) {
  if (retire_slot(n, s)) SlotReaper::reaper().push(n->core->device, s);
}

}  // namespace

void drain_slot_reaper() { SlotReaper::reaper().drain(); }

void add_to_cache(dora_node* n, Slot* s) {  // mod.rs:364-371
  n->cache.push_back(s);
  auto over = [n] {
    if (n->cache.size() <= kMaxCacheSize) return false;
    if (n->cache.size() > kMaxCacheSlots) return true;
    uint64_t bytes = 0;
    for (const Slot* c : n->cache) bytes += c->cap;
    return bytes > slot_cache_bytes();
  };
  while (over()) {
    Slot* old = n->cache.front();
    n->cache.pop_front();
    free_slot_deferred(n, old);
  }
}

void on_token(dora_node* n, const DropToken& t) {
  trace(TP_TOKEN_BACK, t);
  auto f = n->forwarded.find(t);
  if (f != n->forwarded.end()) {  // a zero-copy forward: release the input it re-sent
    n->forwarded.erase(f);
    return;
  }
  auto it = n->sent_out.find(t);
  if (it == n->sent_out.end()) return;  // "received unknown finished drop token"
  Slot* s = it->second;
  n->sent_out.erase(it);
  // the slot's fill flag line was last written by the GPU: start pulling it in now, so the
  // last-fill check of its reuse (allocate_slot, oldest first) finds it in cache
  if (s->flag >= 0) _mm_prefetch(reinterpret_cast<const char*>(n->core->flag_host(s->flag)), _MM_HINT_T0);
  add_to_cache(n, s);
}

int handle_finished_drop_tokens(dora_node* n) {  // mod.rs:348-362
  uint32_t kind;
  std::vector<uint8_t>& p = n->drop_buf;  // reused: popping a token allocates nothing
  while (n->core->drops.try_pop(&kind, &p)) {
    if (kind != DROP_OUTPUT_DROPPED) continue;
    RBuf r(p);
    on_token(n, r.token());
  }
  return DORA_OK;
}

// Best fit among cached slots (mod.rs:321-346 `.rev()...min_by_key`); among slots of equal
// capacity the oldest returned one, whose last fill has had the longest to complete and whose
// flag line on_token has prefetched (the reference takes the newest; any fit is equivalent).
// `need`: the smallest capacity a new slot of `len` would have (an exact fit ends the search).
// `host`: a shared-memory slot is wanted (a device node caches both kinds).
static int best_fit(dora_node* n, uint64_t len, uint64_t need, bool host) {
  int best = -1;
  for (int i = 0; i < static_cast<int>(n->cache.size()); ++i) {
    Slot* s = n->cache[static_cast<size_t>(i)];
    if (s->host != host) continue;
    if (s->cap >= len && (best < 0 || s->cap < n->cache[static_cast<size_t>(best)]->cap)) {
      best = i;
      if (s->cap == need) break;  // an exact fit: no later slot fits better
    }
  }
  return best;
}

int allocate_slot(dora_node* n, uint64_t len, Slot** out) {  // mod.rs:321-346
  const int best = best_fit(n, len, slot_bytes(len), false);
  if (best >= 0) {
    Slot* s = n->cache[static_cast<size_t>(best)];
    n->cache.erase(n->cache.begin() + best);
    SubSpan sp_flag(SP_SLOT_FLAG);
    const bool idle = wait_slot_idle(n, s);
    sp_flag.stop();
    if (idle) {
      *out = s;
      ++n->cache_hits;
      return DORA_OK;
    }
    // its last fill never completed: leak the slot (a kernel may still write it), take a new one
    std::fprintf(stderr, "dora-gpu: slot %llu: last fill did not complete; not reused\n",
                 (unsigned long long)s->id);
    std::lock_guard<std::mutex> g(own_slots().mu);
    own_slots().ptrs.erase(s->id);
  }
  auto* s = new Slot();
  s->cap = slot_bytes(len);
  s->id = own_slots().next_id.fetch_add(1);
  DeviceScope ds(n->core->device);
  hipError_t e = hipMalloc(&s->ptr, slot_bytes(len));
  if (e == hipSuccess) e = hipIpcGetMemHandle(&s->handle, s->ptr);
  if (e == hipSuccess) {
    if (n->core->region_dev && !n->core->free_flags.empty()) {
      s->flag = static_cast<int>(n->core->free_flags.back());
      n->core->free_flags.pop_back();
    } else {
      e = hipEventCreateWithFlags(&s->done, hipEventInterprocess | hipEventDisableTiming);
      if (e == hipSuccess) e = hipIpcGetEventHandle(&s->done_handle, s->done);
    }
  }
  if (e != hipSuccess) {
    if (s->flag >= 0) n->core->free_flags.push_back(static_cast<uint32_t>(s->flag));
    if (s->done) (void)hipEventDestroy(s->done);
    if (s->ptr) (void)hipFree(s->ptr);
    delete s;
    return fail(DORA_ERR_HIP, "device slot of %llu bytes: %s", (unsigned long long)len,
                hipGetErrorString(e));
  }
  {
    std::lock_guard<std::mutex> g(own_slots().mu);
    own_slots().ptrs[s->id] = s->ptr;
  }
  ++n->slots_created;
  n->core->region->hdr()->nodes[n->core->idx].slots_created.fetch_add(1, std::memory_order_relaxed);
  *out = s;
  return DORA_OK;
}

// A host-only node's sample >= 4096 B (mod.rs:321-346): best fit from the slot cache, else a
// new POSIX shared-memory region of whole pages.  The node writes it with the CPU (as the
// reference's copy_array_into_sample); device receivers pull it into HBM by DMA.
int allocate_host_slot(dora_node* n, uint64_t len, Slot** out) {
  constexpr uint64_t kPage = 4096;
  const uint64_t need = (std::max<uint64_t>(len, 1) + kPage - 1) / kPage * kPage;
  const int best = best_fit(n, len, need, true);
  if (best >= 0) {
    *out = n->cache[static_cast<size_t>(best)];
    n->cache.erase(n->cache.begin() + best);
    ++n->cache_hits;
    return DORA_OK;
  }
  auto* s = new Slot();
  s->host = true;
  s->cap = need;
  s->id = own_slots().next_id.fetch_add(1);
  // pid + a per-process nonce + slot id: a receiver's cached mapping of a region is keyed by its
  // name, so a later process that got the same pid must not produce the same names
  static const uint32_t nonce = [] {
    std::random_device rd;
    return static_cast<uint32_t>(rd());
  }();
  char nbuf[16];
  std::snprintf(nbuf, sizeof(nbuf), "%08x", nonce);
  s->shm_name = "/dora-gpu-s-" + std::to_string(self_pid()) + "-" + nbuf + "-" + std::to_string(s->id);
  s->ptr = shmem_create(s->shm_name, s->cap);
  if (!s->ptr) {
    const int err = errno;
    delete s;
    return fail(DORA_ERR_INVALID, "shared-memory sample of %llu bytes: %s",
                (unsigned long long)len, std::strerror(err));
  }
  ++n->slots_created;
  n->core->region->hdr()->nodes[n->core->idx].slots_created.fetch_add(1, std::memory_order_relaxed);
  *out = s;
  return DORA_OK;
}

}  // namespace dora
