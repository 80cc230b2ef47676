// Node API of the device data plane — the MI355X counterpart of `DoraNode` + `EventStream`
// (apis/rust/node/src/node/mod.rs:42-503, apis/rust/node/src/event_stream/*).
//
// Sender (mod.rs:180-275, 303-371):
//   allocate_data_sample -> a device slot (hipMalloc, exported once with hipIpcGetMemHandle),
//   best-fit from a 20-entry cache of recycled slots exactly like `allocate_shared_memory`;
//   send_output -> plan + HIP pack kernel into the slot on the node's stream; the timestamp is
//   taken after the fill (mod.rs:258); the slot is kept in `sent_out` until its drop token
//   returns (mod.rs:269-272, 348-371).
// Receiver (event_stream/mod.rs:121-198, event.rs:35-126):
//   events are drained from the node's ring into a local queue with the daemon Listener's
//   drop-oldest-per-input policy (node_communication/mod.rs:320-359); a DeviceIpc sample is
//   mapped with hipIpcOpenMemHandle once per slot and cached (never per message); the drop token
//   is reported when the last reference to the input data is released, after the node's stream
//   has drained, so the owner can reuse the slot.
//
// This file: the node's life (init, free, sync, stream), its environment switches and the plain
// getters.  node_slots.cpp: slot lifetime; node_send.cpp: the send path; node_recv.cpp: the
// event stream; node_measure.cpp: the benchmark's instrumentation; node_internal.h: the types.
#include "node_internal.h"

namespace dora {
namespace {

constexpr uint64_t kDropWaitNs = 10000000000;  // 10 s per token on drop (mod.rs:397-426)

// DORA_GPU_PIN=0: leave the node's CPU affinity alone (shm.cpp pin_to_numa)
bool numa_pinning() {
  static const bool v = [] {
    const char* e = std::getenv("DORA_GPU_PIN");
    return !(e && *e == '0');
  }();
  return v;
}

// NUMA node of HIP device `device` (sysfs of its PCI function), -1 when unknown.
int gpu_numa_node(int device) {
  char bus[64] = {0};
  if (hipDeviceGetPCIBusId(bus, sizeof(bus), device) != hipSuccess) return -1;
  for (char* p = bus; *p; ++p) *p = char(std::tolower(*p));
  const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/numa_node";
  FILE* f = std::fopen(path.c_str(), "r");
  if (!f) return -1;
  int numa = -1;
  if (std::fscanf(f, "%d", &numa) != 1) numa = -1;
  std::fclose(f);
  return numa;
}

// DORA_GPU_FANOUT=rccl: this node's outputs with receivers on other GPUs form RCCL broadcast
// groups (bcast.h) instead of letting every receiver pull over its own link.
bool fanout_rccl() {
  static const bool v = [] {
    const char* e = std::getenv("DORA_GPU_FANOUT");
    return e && std::strcmp(e, "rccl") == 0;
  }();
  return v;
}

std::vector<std::string> split(const char* s, char sep) {
  std::vector<std::string> out;
  std::string cur;
  for (const char* p = s; *p; ++p) {
    if (*p == sep) {
      if (!cur.empty()) out.push_back(cur);
      cur.clear();
    } else {
      cur += *p;
    }
  }
  if (!cur.empty()) out.push_back(cur);
  return out;
}

// DORA_GPU_FANOUT=rccl, at init: ask the daemon for a broadcast group per output and, when it
// admits one (receivers each on their own GPU, none on ours), form the communicator as rank 0.
// Outputs without a group keep the pull path.  Every wait is bounded.
void form_bcast_groups(dora_node* n) {
  NodeCore* c = n->core.get();
  DeviceScope ds(c->device);  // the groups' streams and communicators belong to the node's GPU
  std::string why;
  if (!bcast_available(&why)) {
    c->bcast_error = why;
    return;
  }
  for (const std::string& o : n->outputs) {
    uint8_t uid[kBcastIdBytes];
    if (bcast_unique_id(uid) != DORA_OK) {
      c->bcast_error = dora_gpu_last_error();
      return;
    }
    WBuf w;
    w.str(o);
    w.raw(uid, sizeof(uid));
    if (c->request(REQ_BCAST_GROUP, w.data(), w.size()) != DORA_OK) return;
    uint32_t nranks = 0;
    bool answered = false;
    const uint64_t t0 = mono_ns();
    while (!answered && mono_ns() - t0 < 10000000000ull) {
      uint32_t kind;
      std::vector<uint8_t> p;
      if (!c->drops.try_pop(&kind, &p)) {
        c->drops.wait(10000);
        continue;
      }
      RBuf r(p);
      if (kind == DROP_OUTPUT_DROPPED) {
        on_token(n, r.token());
      } else if (kind == DROP_BCAST_GROUP && r.str() == o) {
        nranks = r.u32();
        answered = true;
      }
    }
    if (nranks < 2) {
      c->bcast_error = "output `" + o + "`: the daemon admitted no broadcast group (each receiver "
                       "must run on its own GPU, none on the producer's); receivers pull";
      continue;
    }
    BcastComm* comm = nullptr;
    hipStream_t st = nullptr;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
      (void)hipGetLastError();
      c->bcast_error = "broadcast stream of output `" + o + "`";
      continue;
    }
    if (bcast_join(uid, static_cast<int>(nranks), 0, 30000, &comm) == DORA_OK) {
      n->bcast_out[o] = {comm, st};
    } else {
      c->bcast_error = dora_gpu_last_error();
      (void)hipStreamDestroy(st);
    }
  }
}

}  // namespace
}  // namespace dora

extern "C" {

int dora_node_init(const char* shm_name, const char* node_id, int device, dora_node** out) {
  if (!shm_name || !node_id || !out) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  *out = nullptr;
  DORA_GUARD_BEGIN
  auto core = std::make_shared<dora::NodeCore>();
  try {
    core->region.reset(dora::Region::attach(shm_name));
  } catch (const std::exception& e) {
    return dora::fail(DORA_ERR_INVALID, "attach dataflow: %s", e.what());
  }
  core->idx = core->region->node_index(node_id);
  if (core->idx < 0)
    return dora::fail(DORA_ERR_NOT_FOUND, "node `%s` is not part of the dataflow", node_id);
  dora::NodeEntry& e = core->region->hdr()->nodes[core->idx];
  int32_t expected = 0;
  if (!e.pid.compare_exchange_strong(expected, static_cast<int32_t>(getpid())))
    return dora::fail(DORA_ERR_INVALID, "node `%s` is already running (pid %d)", node_id,
                      expected);
  core->req = dora::RingWriter(core->region.get(), &e.requests);
  core->ev = dora::RingReader(core->region.get(), &e.events);
  core->drops = dora::RingReader(core->region.get(), &e.drops);
  core->device = device;
  e.device.store(device < 0 ? -1 : device);
  dora::trace_set_name(node_id);
  if (device >= 0) {  // device < 0: host-only node (control plane + inline Vec samples only)
    DORA_HIP(hipSetDevice(device));
    // NUMA placement: the send/receive path writes the GPU's BAR (AQL arguments, doorbells)
    // and polls host memory the GPU writes (fill flags); keep this thread next to its GPU and
    // tell the daemon where that is (DORA_GPU_PIN=0: leave the affinity alone)
    if (dora::numa_pinning()) {
      const int numa = dora::gpu_numa_node(device);
      if (numa >= 0) {
        dora::RegionHdr* rh = core->region->hdr();
        (void)dora::pin_to_numa(numa, device, &rh->l3_cpu, int(rh->n_nodes) + 1);
        int32_t none = -1;
        core->region->hdr()->numa_hint.compare_exchange_strong(none, numa);
      }
    }
    DORA_HIP(hipStreamCreateWithFlags(&core->stream, hipStreamNonBlocking));
    // Fill streams are created on first use: device-source packs go to the AQL queues, so only
    // host sources, compacting transforms and node-stream-ordered fills need them, and a node
    // that never sends such a pack holds one HIP hardware queue, not four.
    {
      // host-register the control region so this node's stream can write fill epochs into it
      void* dev = nullptr;
      if (hipHostRegister(core->region->base(), core->region->size(), hipHostRegisterMapped) ==
              hipSuccess &&
          hipHostGetDevicePointer(&dev, core->region->base(), 0) == hipSuccess) {
        core->region_dev = static_cast<uint8_t*>(dev);
        for (uint32_t k = dora::kFillFlags; k-- > 0;) core->free_flags.push_back(k);
        const size_t cb = size_t(dora::kFillFlags) * dora::kMaxSignalWgs * sizeof(uint32_t);
        if (hipMalloc(&core->fill_done, cb) != hipSuccess ||
            hipMemset(core->fill_done, 0, cb) != hipSuccess ||
            hipDeviceSynchronize() != hipSuccess) {
          (void)hipGetLastError();  // the stream write-value packet signals instead
          if (core->fill_done) (void)hipFree(core->fill_done);
          core->fill_done = nullptr;
        }
      } else {
        (void)hipGetLastError();  // fall back to interprocess events
      }
    }
  }

  auto* n = new dora_node();
  n->pin_pending = device < 0 && dora::numa_pinning();
  if (const char* e = std::getenv("DORA_GPU_SEND_ASYNC")) n->async_default = *e == '1';
  n->core = core;
  n->id = node_id;
  for (auto& o : dora::split(e.outputs, ',')) n->outputs.insert(o);
  for (auto& kv : dora::split(e.inputs, ',')) {
    auto eq = kv.find('=');
    n->queue_size[kv.substr(0, eq)] = static_cast<uint32_t>(std::stoul(kv.substr(eq + 1)));
  }
  n->min_queue_size = SIZE_MAX;
  for (auto& kv : n->queue_size) n->min_queue_size = std::min<size_t>(n->min_queue_size, kv.second);
  // Subscribe and wait for AllNodesReady (event_stream/mod.rs:37-118, daemon PendingNodes)
  int rc = core->request(dora::REQ_SUBSCRIBE, {});
  if (rc != DORA_OK) {
    delete n;
    return rc;
  }
  const uint64_t t0 = dora::mono_ns();
  for (;;) {
    uint32_t kind;
    std::vector<uint8_t> p;
    if (core->ev.try_pop(&kind, &p)) {
      if (kind == dora::EV_READY) {
        // the outputs whose receivers all lack a GPU (daemon.cpp ready_payload); kept on a
        // host-only node too, for dora_node_host_bound_outputs, though only a device node packs
        if (p.size() >= 4) {
          dora::RBuf r(p);
          for (uint32_t k = r.u32(); k > 0; --k) n->host_bound.insert(r.str());
        }
        break;
      }
      dora::encode_event(n, kind, p);
      continue;
    }
    if (dora::mono_ns() - t0 > 60000000000ull) {
      delete n;
      return dora::fail(DORA_ERR_TIMEOUT, "no AllNodesReady from the daemon within 60 s");
    }
    core->ev.wait(100000);
  }
  if (device >= 0 && dora::fanout_rccl() && !n->outputs.empty()) dora::form_bcast_groups(n);
  if (n->want_pump) dora::start_pump(n);  // a broadcast group joined during init
  // send_stdout_as (spawn.rs:280-437): the descriptor names one of this node's outputs
  if (const char* so = std::getenv("DORA_GPU_SEND_STDOUT_AS")) {
    if (!n->outputs.count(so)) {
      delete n;
      return dora::fail(DORA_ERR_NOT_FOUND, "send_stdout_as names `%s`, not an output of `%s`",
                        so, node_id);
    }
    std::weak_ptr<dora::NodeCore> wc = core;
    n->stdout_capture = dora::stdout_capture_start(
        so, [wc](uint32_t kind, const std::vector<uint8_t>& p) {
          auto c = wc.lock();
          return c ? c->request(kind, p) : DORA_ERR_CLOSED;
        });
  }
  *out = n;
  return DORA_OK;
  DORA_GUARD_END
}

int dora_node_init_from_env(dora_node** out) {
  const char* shm = std::getenv("DORA_GPU_DATAFLOW");
  const char* id = std::getenv("DORA_NODE_ID");
  const char* dev = std::getenv("DORA_GPU_DEVICE");
  if (!shm || !id)
    return dora::fail(DORA_ERR_INVALID,
                      "env variables DORA_GPU_DATAFLOW and DORA_NODE_ID must be set. Are you sure "
                      "the node was started by the dataflow launcher?");
  return dora_node_init(shm, id, dev ? std::atoi(dev) : 0, out);
}

void dora_node_free(dora_node* n) {  // Drop for DoraNode (mod.rs:384-431)
  if (!n) return;
  struct Flush {
    ~Flush() { dora::trace_flush(); }
  } flush_trace_at_end;
  dora::stdout_capture_stop(n->stdout_capture);  // the last lines go out before the outputs close
  n->stdout_capture = nullptr;
  dora::stop_pump(n);  // the event-stream thread first: the queue is this thread's again
  std::vector<std::string> outs(n->outputs.begin(), n->outputs.end());
  dora::WBuf w;
  w.u32(static_cast<uint32_t>(outs.size()));
  for (auto& o : outs) w.str(o);
  (void)n->core->request(dora::REQ_CLOSE_OUTPUTS, w.data(), w.size());
  n->queue.clear();  // releases undelivered inputs (tokens reported)
  uint64_t t0 = dora::mono_ns();
  while (!n->sent_out.empty() || !n->forwarded.empty()) {
    dora::handle_finished_drop_tokens(n);
    if (n->sent_out.empty() && n->forwarded.empty()) break;
    if (dora::mono_ns() - t0 > dora::kDropWaitNs) break;  // "timeout while waiting for drop tokens"
    n->core->drops.wait(10000);
    if (n->core->region->hdr()->nodes[n->core->idx].state.load() == 2) break;
  }
  n->forwarded.clear();  // inputs still held by unanswered forwards: their tokens go back
  (void)n->core->request(dora::REQ_OUTPUTS_DONE, {});
  // broadcasts read the slots: the groups go (after their streams drain, bounded) first
  for (auto& kv : n->bcast_out) {
    dora::bcast_close(kv.second.comm, kv.second.stream, 10000);
    (void)hipStreamDestroy(kv.second.stream);
  }
  n->bcast_out.clear();
  for (dora_sample* s : n->samples_live) dora::discard_sample(n, s);  // allocated, never sent
  n->samples_live.clear();
  for (auto& kv : n->sent_out) dora::free_slot(n, kv.second);
  for (auto* s : n->cache) dora::free_slot(n, s);
  dora::drain_slot_reaper();  // evicted slots: freed before the node's state goes
  delete n;  // the plan cache, the timing pairs and the timed region release what they own
}

int dora_node_sync(dora_node* n) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (n->core->device < 0) return DORA_OK;
  dora::DeviceScope ds(n->core->device);
  dora::NodeCore* c = n->core.get();
  // Kernel-signalled fills (AQL and fill streams): their flags.  A stream query or synchronise
  // would wait for HIP to notice the kernels' completion, ~100-200 us after the flags are up.
  const uint64_t deadline = dora::mono_ns() + dora::kFillWaitNs;
  for (auto* v : {&c->aql_pending, &c->flag_pending}) {
    for (auto& x : *v)
      if (!dora::wait_fill(x.first, x.second, deadline))
        return dora::fail(DORA_ERR_TIMEOUT, "a fill did not complete within 10 s");
    v->clear();
  }
  // work no flag covers: fills signalled by the stream (kernel signal off, transforms, host
  // sources) and whatever the caller queued on the node stream
  for (size_t i = 0; i < c->fill_streams.size(); ++i) {
    if (!c->fill_unsignalled[i]) continue;
    DORA_HIP(hipStreamSynchronize(c->fill_streams[i]));
    c->fill_unsignalled[i] = 0;
  }
  if (hipStreamQuery(c->stream) == hipErrorNotReady) DORA_HIP(hipStreamSynchronize(c->stream));
  (void)hipGetLastError();
  return DORA_OK;
}

dora_stream_t dora_node_stream(dora_node* n) {
  if (!n) return nullptr;
  n->core->stream_used.store(true, std::memory_order_relaxed);
  n->core->fence_fills();  // work the caller queues next runs after every fill so far
  return n->core->stream;
}

const char* dora_node_dataflow_id(const dora_node* n) {
  return n ? n->core->region->hdr()->dataflow_id : "";
}

const char* dora_node_id(const dora_node* n) { return n ? n->id.c_str() : ""; }

int dora_node_stats(dora_node* n, uint64_t* slots_created, uint64_t* cache_hits,
                    uint64_t* in_flight, uint64_t* dropped_inputs) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (slots_created) *slots_created = n->slots_created;
  if (cache_hits) *cache_hits = n->cache_hits;
  if (in_flight) *in_flight = n->sent_out.size();
  if (dropped_inputs) *dropped_inputs = n->dropped_inputs;
  return DORA_OK;
}

int dora_node_dataflow_counters(dora_node* n, const char* node_id, uint64_t* slots_created,
                                uint64_t* ipc_opens, uint64_t* dropped_inputs) {
  if (!n || !node_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  const int i = n->core->region->node_index(node_id);
  if (i < 0) return dora::fail(DORA_ERR_NOT_FOUND, "node `%s` is not part of the dataflow", node_id);
  const dora::NodeEntry& e = n->core->region->hdr()->nodes[i];
  if (slots_created) *slots_created = e.slots_created.load(std::memory_order_relaxed);
  if (ipc_opens) *ipc_opens = e.ipc_opens.load(std::memory_order_relaxed);
  if (dropped_inputs) *dropped_inputs = e.dropped_inputs.load(std::memory_order_relaxed);
  return DORA_OK;
}

int dora_node_plan_cache_stats(dora_node* n, uint64_t* hits, uint64_t* entries) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (hits) *hits = n->plans.hits;
  if (entries) *entries = n->plans.entries.size();
  return DORA_OK;
}

int dora_node_fill_paths(dora_node* n, uint64_t* aql_packs, uint64_t* hip_packs) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (aql_packs) *aql_packs = n->aql_packs;
  if (hip_packs) *hip_packs = n->hip_packs;
  return DORA_OK;
}

int dora_node_host_paths(dora_node* n, uint64_t* bar_fills, uint64_t* staged,
                         uint64_t* staged_bytes, uint64_t* host_packs) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (bar_fills) *bar_fills = n->bar_fills;
  if (host_packs) *host_packs = n->host_packs + n->host_copies;
  if (staged) *staged = n->core->host_staged.load();
  if (staged_bytes) *staged_bytes = n->core->host_staged_bytes.load();
  return DORA_OK;
}

int dora_node_host_bound_outputs(dora_node* n, char* buf, uint64_t cap, uint64_t* len) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  std::string all;
  for (const auto& o : n->host_bound) all += o + "\n";
  if (len) *len = all.size();
  if (!buf) return DORA_OK;
  if (cap < all.size() + 1) return dora::fail(DORA_ERR_INVALID, "buffer too small");
  std::memcpy(buf, all.c_str(), all.size() + 1);
  return DORA_OK;
}

int dora_node_sample_paths(dora_node* n, uint64_t* stream_ordered, uint64_t* self_published) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (stream_ordered) *stream_ordered = n->samples_stream_ordered;
  if (self_published) *self_published = n->samples_self_published;
  return DORA_OK;
}

int dora_node_forward_stats(dora_node* n, uint64_t* in_place, uint64_t* held) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (in_place) *in_place = n->zero_copy_forwards;
  if (held) *held = n->forwarded.size();
  return DORA_OK;
}

int dora_node_peer_stats(dora_node* n, uint64_t* copies, uint64_t* bytes) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (copies) *copies = n->core->peer_copies.load();
  if (bytes) *bytes = n->core->peer_bytes.load();
  return DORA_OK;
}

int dora_node_bcast_stats(dora_node* n, uint64_t* groups_out, uint64_t* groups_in,
                          uint64_t* sent, uint64_t* received, uint64_t* received_bytes,
                          const char** error) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  if (groups_out) *groups_out = n->bcast_out.size();
  if (groups_in) *groups_in = n->core->bcast_in.size();
  if (sent) *sent = n->bcast_seq;
  if (received) *received = n->core->bcast_recvs;
  if (received_bytes) *received_bytes = n->core->bcast_bytes;
  if (error) *error = n->core->bcast_error.c_str();
  return DORA_OK;
}

int dora_node_bcast_ranks(dora_node* n, uint64_t* max_ranks) {
  if (!n || !max_ranks) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  *max_ranks = 0;
  for (const auto& kv : n->bcast_out)
    *max_ranks = std::max<uint64_t>(*max_ranks, uint64_t(dora::bcast_nranks(kv.second.comm)));
  return DORA_OK;
}

}  // extern "C"
