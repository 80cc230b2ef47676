
// The event stream: the daemon's events into the node's queue (encode_event, drain_events, the
// event-stream thread), an input's completion when it is handed out (finish_input), the pulls
// of samples that are not in this GPU's memory, and dora_node_next_event / dora_event_*.
#include "node_internal.h"

namespace dora {

// How cross-GPU samples are pulled: the pack kernel on the receiving GPU reading the peer's HBM
// (default) or the copy engines via hipMemcpyPeerAsync (DORA_GPU_PEER_COPY=sdma).
PeerCopyMode peer_copy_mode() {
  static const PeerCopyMode v = [] {
    const char* e = std::getenv("DORA_GPU_PEER_COPY");
    return (e && std::string(e) == "sdma") ? PEER_SDMA : PEER_KERNEL;
  }();
  return v;
}

// DORA_GPU_EDGE_COPY=1 (testing): the cross-GPU receive path on same-GPU edges, the one-GPU
// rehearsal of C4/C5 (tests, bench.py DORA_BENCH_GPUS).
bool edge_copy_forced() {
  static const bool v = [] {
    const char* e = std::getenv("DORA_GPU_EDGE_COPY");
    return e && *e && *e != '0';
  }();
  return v;
}

namespace {

// EV_BCAST_JOIN: become rank `rank` of the producer's broadcast group for input `input`.
void join_bcast_group(dora_node* n, const std::string& input, const uint8_t* uid, uint32_t nranks,
                      uint32_t rank) {
  NodeCore* c = n->core.get();
  if (c->device < 0) {
    c->bcast_error = "host-only node cannot join a broadcast group";
    return;
  }
  DeviceScope ds(c->device);
  if (!c->bcast_stream && hipStreamCreateWithFlags(&c->bcast_stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    c->bcast_stream = nullptr;
    c->bcast_error = "broadcast receive stream";
    return;
  }
  BcastComm* comm = nullptr;
  if (bcast_join(uid, static_cast<int>(nranks), static_cast<int>(rank), 30000, &comm) != DORA_OK) {
    c->bcast_error = dora_gpu_last_error();
    return;
  }
  auto it = c->bcast_in.find(input);
  if (it != c->bcast_in.end()) bcast_close(it->second, c->bcast_stream, 10000);
  c->bcast_in[input] = comm;
  // a rank that stops polling must not stall the collective for the others: post receives
  // from the event-stream thread (started by the user thread when it next returns from the
  // event loop, dora_node_next_event / init)
  n->want_pump = true;
}

// A FILL_BCAST sample: post this rank's receive of the producer's broadcast into the receive
// pool right away (at drain time, so every rank issues the group's broadcasts in routing order,
// whether or not the input is later dropped); the input is complete when `bcast_ev` fires.
int post_bcast_receive(NodeCore* c, InputData* in, const std::string& input) {
  auto it = c->bcast_in.find(input);
  if (it == c->bcast_in.end())
    return fail(DORA_ERR_INVALID, "input `%s`: broadcast sample but no group joined (%s)",
                input.c_str(), c->bcast_error.c_str());
  DeviceScope ds(c->device);
  uint64_t cap = 0;
  void* local = c->recv_pool.get(in->ext_len, &cap);
  if (!local)
    return fail(DORA_ERR_HIP, "receive slot of %llu bytes", (unsigned long long)in->ext_len);
  int rc = bcast_enqueue(it->second, local, in->ext_len, c->bcast_stream);
  hipEvent_t e = nullptr;
  if (rc == DORA_OK) {
    hipError_t he = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (he == hipSuccess) he = hipEventRecord(e, c->bcast_stream);
    if (he != hipSuccess) {
      // the receive is queued: wait for it here rather than lose track of it
      (void)hipStreamSynchronize(c->bcast_stream);
      if (e) (void)hipEventDestroy(e);
      e = nullptr;
    }
  }
  if (rc != DORA_OK) {
    c->recv_pool.put(local, cap);
    return rc;
  }
  in->local = local;
  in->local_cap = cap;
  in->ptr = local;
  in->bcast_ev = e;
  ++c->bcast_recvs;
  c->bcast_bytes += in->ext_len;
  return DORA_OK;
}

}  // namespace

void encode_event(dora_node* n, uint32_t kind, const std::vector<uint8_t>& p) {
  SubSpan sp(SP_RECV_ENCODE);
  auto ev = std::make_unique<dora_event>();
  RBuf r(p);
  switch (kind) {
    case EV_INPUT: {
      ev->type = DORA_EVENT_INPUT;
      ev->arrived_ns = mono_ns();
      ev->id = r.str();
      const uint64_t meta_len = r.u64();
      r.need(meta_len);
      RBuf mr(r.ptr(), meta_len);  // parsed in place: no copy of the metadata bytes
      ev->meta = mr.metadata();
      r.skip(meta_len);
      DataMsg d = r.data();
      auto in = std::make_shared<InputData>();
      in->core = n->core;
      const bool woke = ring_take_woke();
      if (d.kind != DATA_DEVICE_IPC && trace_enabled())
        trace(woke ? TP_POPPED_WOKE : TP_POPPED, ts_key(ev->meta.timestamp_ns));
      if (d.kind == DATA_VEC) {
        in->vec = std::move(d.vec);
        in->ptr = in->vec.data();
        in->len = in->vec.size();
        in->ext_len = in->len;
      } else if (d.kind == DATA_SHMEM) {
        // a host-only node's sample: read in place by a host receiver, pulled into HBM by DMA
        // on first access by a device receiver (ensure_local)
        in->has_token = true;
        in->token = d.shm.token;
        in->len = in->ext_len = d.shm.len;
        std::string err;
        in->shm = n->core->map_shmem(d.shm.name, d.shm.len, &err);
        if (!in->shm) {
          ev->type = DORA_EVENT_ERROR;
          ev->error = err;
        } else {
          in->ptr = in->shm->base;
          (n->core->device >= 0 ? in->host_pull : in->host_mem) = true;
        }
      } else if (d.kind == DATA_DEVICE_IPC) {
        in->has_token = true;  // set first: a mapping failure still returns the token
        in->token = d.ipc.token;
        trace(woke ? TP_POPPED_WOKE : TP_POPPED, in->token);
        in->len = d.ipc.len;
        in->ext_len = std::max(d.ipc.ext_len, d.ipc.len);
        void* base = nullptr;
        if (d.ipc.fill == FILL_BCAST) {
          // the sample arrives through the output's RCCL group, not the producer's slot
          if (post_bcast_receive(n->core.get(), in.get(), ev->id) != DORA_OK) {
            ev->type = DORA_EVENT_ERROR;
            ev->error = dora_gpu_last_error();
            in->ptr = nullptr;
          }
        } else if (d.ipc.owner_pid == self_pid()) {
          std::lock_guard<std::mutex> g(own_slots().mu);
          auto it = own_slots().ptrs.find(d.ipc.slot_id);
          if (it != own_slots().ptrs.end()) base = it->second;
        } else {
          IpcKey key;
          std::memcpy(key.b, d.ipc.handle, 64);
          key.pid = d.ipc.owner_pid;
          key.slot = d.ipc.slot_id;
          NodeCore* c = n->core.get();
          std::lock_guard<std::mutex> g(c->ipc_mu);
          auto it = c->ipc_cache.find(key);
          if (it != c->ipc_cache.end()) {
            in->mapping = it->second;
          } else {
            hipIpcMemHandle_t h;
            std::memcpy(&h, d.ipc.handle, sizeof(h));
            // a host-only receiver maps the slot on its producer's GPU, whose copy engine stages
            // it to host memory (stage_to_host)
            DeviceScope ds(c->device >= 0 ? c->device : int(d.ipc.device));
            hipError_t e = hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess) {
              ev->type = DORA_EVENT_ERROR;
              ev->error = std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(e) +
                          " (slot " + std::to_string(d.ipc.slot_id) + " of pid " +
                          std::to_string(d.ipc.owner_pid) + " on GPU " +
                          std::to_string(d.ipc.device) + ", " + std::to_string(d.ipc.len) + " B)";
              base = nullptr;
            } else {
              in->mapping = std::make_shared<IpcMapping>();
              in->mapping->base = base;
              c->ipc_cache.emplace(key, in->mapping);
              c->ipc_opens.fetch_add(1, std::memory_order_relaxed);
              n->core->region->hdr()->nodes[c->idx].ipc_opens.fetch_add(1, std::memory_order_relaxed);
              c->trim_ipc_cache();
            }
          }
          if (in->mapping) {
            in->mapping->last_use = ++c->ipc_clock;
            base = in->mapping->base;
          }
        }
        if (base) in->ptr = static_cast<uint8_t*>(base) + d.ipc.offset;
        // the fill wait and a cross-GPU pull happen when the event is handed out
        // (finish_input), so draining a burst never serialises on later fills
        ev->pending = true;
        ev->ipc = d.ipc;
      }
      ev->data = std::move(in);
      break;
    }
    case EV_INPUT_CLOSED:
      ev->type = DORA_EVENT_INPUT_CLOSED;
      ev->id = r.str();
      break;
    case EV_ALL_INPUTS_CLOSED:
      ev->type = DORA_EVENT_ALL_INPUTS_CLOSED;
      break;
    case EV_STOP:
      ev->type = DORA_EVENT_STOP;
      break;
    case EV_BCAST_JOIN: {
      const std::string input = r.str();
      uint8_t uid[kBcastIdBytes];
      r.raw(uid, sizeof(uid));
      const uint32_t nranks = r.u32();
      const uint32_t rank = r.u32();
      join_bcast_group(n, input, uid, nranks, rank);
      return;  // internal: no event for the user
    }
    default:
      return;  // EV_READY after init is ignored
  }
  n->queue.push_back(std::move(ev));
}

namespace {

// A device sample delivered to a node without a GPU (DORA_GPU_DEVICE < 0): one DMA by the
// producer GPU's copy engines into pinned host memory the input owns (recycled, host_pool), then
// the producer's token goes back at once and the input is a host input like a shared-memory one
// (the reference's receivers always get host ArrowData, event_stream/event.rs:35-91; a Python
// receiver a pyarrow array, apis/python/operator/src/lib.rs:135-144).  The copy is issued to the
// copy engines through HSA and its signal polled (aql.h hsa_copy_host): 4 KB in 6.9 us where
// hipMemcpyAsync + hipStreamSynchronize took 17 (scripts/d2h_copy_probe.py,
// profiles/r06_d2h_copy_probe.jsonl); a 4 KB message to such a receiver beside a device one,
// send call to receipt, 15.5-16.5 us p50 / 19-21 p99 against 20.9-21.9 / 37-38 with HIP's copy
// (profiles/r06_stage_copy_ab.txt, five interleaved rounds); HIP's copy stays the fallback.  40.96 MB: 56 GB/s on an
// MI355X box (profiles/r06_host_path_probe.jsonl, d2h_pinned).  The pack kernel writing pinned
// host memory from one raw AQL packet of the receiver was slower at every size tried, 23 / 27 /
// 30 us against 18 / 16 / 20 at 4 KB / 64 KB / 256 KB (profiles/r06_d2h_stage_ab.jsonl).
int stage_to_host(InputData* in, int src_device) {
  NodeCore* c = in->core.get();
  if (in->ext_len) {
    DeviceScope ds(src_device);
    uint64_t cap = 0;
    void* h = c->host_pool.get(in->ext_len, &cap);
    if (!h)
      return fail(DORA_ERR_HIP, "pinned staging buffer of %llu bytes",
                  (unsigned long long)in->ext_len);
    hipError_t e = hipSuccess;
    const int hrc = hsa_copy_host(h, in->ptr, in->ext_len, true);
    if (hrc == DORA_ERR_TIMEOUT) return hrc;  // the buffer is not reused: the copy may still land
    if (hrc != DORA_OK) {
      static std::atomic<bool> noted{false};
      if (std::getenv("DORA_GPU_TRACE") && !noted.exchange(true))
        std::fprintf(stderr, "dora-gpu: staging through HIP's copy: %s\n", dora_gpu_last_error());
      clear_error();
      hipStream_t st = c->stage_stream(src_device);
      e = st ? hipMemcpyAsync(h, in->ptr, in->ext_len, hipMemcpyDeviceToHost, st)
             : hipErrorInvalidResourceHandle;
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) {
      (void)hipGetLastError();
      c->host_pool.put(h, cap);
      return fail(DORA_ERR_HIP, "staging a device sample to host memory: %s",
                  hipGetErrorString(e));
    }
    in->host_local = h;
    in->host_local_cap = cap;
    c->host_staged.fetch_add(1, std::memory_order_relaxed);
    c->host_staged_bytes.fetch_add(in->ext_len, std::memory_order_relaxed);
  }
  in->ptr = in->host_local;
  in->host_mem = true;
  in->mapping.reset();
  if (in->has_token) {
    c->report_drop_token(in->token);
    trace(TP_RELEASED, in->token);
    in->has_token = false;
  }
  return DORA_OK;
}

// Complete a queued device input right before it is handed to the user: wait for the
// producer's fill (flag or interprocess event) and, for a slot on another GPU, pull it into a
// local receive slot with one peer copy and return the producer's token at once.
void finish_input(dora_node* n, dora_event* ev) {
  if (!ev->pending) return;
  SubSpan sp(SP_RECV_FINISH);
  ev->pending = false;
  InputData* in = ev->data.get();
  const DeviceIpc& d = ev->ipc;
  if (!in || !in->ptr) return;
  if (d.fill == FILL_BCAST) {
    // the receive was posted at drain time; hand the input out once it has completed
    hipError_t e = in->bcast_ev ? hipEventQuery(in->bcast_ev) : hipSuccess;
    const uint64_t t0 = mono_ns();
    while (e == hipErrorNotReady && mono_ns() - t0 < 60000000000ull) {
      if (mono_ns() - t0 > uint64_t(spin_budget_us()) * 1000) usleep(20);
      else __builtin_ia32_pause();
      e = hipEventQuery(in->bcast_ev);
    }
    if (e != hipSuccess) {
      ev->type = DORA_EVENT_ERROR;
      ev->error = e == hipErrorNotReady ? "broadcast receive did not complete within 60 s"
                                        : std::string("broadcast receive: ") + hipGetErrorString(e);
      in->ptr = nullptr;
      return;
    }
    trace(TP_FILLED, in->token);
    return;
  }
  if (d.fill == FILL_FLAG) {
    // the producer's stream writes the epoch into its fill flag after the pack: poll it
    RegionHdr* h = n->core->region->hdr();
    if (d.flag_node >= h->n_nodes || d.flag_index >= kFillFlags) {
      ev->type = DORA_EVENT_ERROR;
      ev->error = "fill flag out of range";
      in->ptr = nullptr;
      return;
    }
    const std::atomic<uint64_t>& f = h->nodes[d.flag_node].fill[d.flag_index].epoch;
    const uint64_t t0 = mono_ns();
    unsigned spins = 0;
    while (!fill_reached(&f, d.epoch)) {
      if (++spins < 4096) {
        __builtin_ia32_pause();
        continue;
      }
      spins = 0;
      if (mono_ns() - t0 > 60000000000ull) {
        ev->type = DORA_EVENT_ERROR;
        ev->error = "the producer's fill did not complete within 60 s";
        in->ptr = nullptr;
        return;
      }
      if (mono_ns() - t0 > uint64_t(spin_budget_us()) * 1000) usleep(20);
    }
    add_fill_wait_ns(mono_ns() - t0);
    if (trace_enabled()) {
      // the pack's own stamps (s_memrealtime), for the GPU side of a message's latency: only an
      // in-kernel-signalled fill of exactly this epoch writes them (a CP-signalled fill writes
      // none, and the line may already carry a later fill's stamps if the slot was refilled)
      const FillFlag& ff = h->nodes[d.flag_node].fill[d.flag_index];
      if (ff.epoch.load(std::memory_order_acquire) == d.epoch &&
          ff.cp_epoch.load(std::memory_order_acquire) != d.epoch) {
        // on the host's clock when the HSA runtime can map GPU ticks (aql.h), else GPU ns
        const uint64_t s0 = aql_gpu_tick_to_realtime_ns(n->core->device, ff.t_start);
        const uint64_t s1 = aql_gpu_tick_to_realtime_ns(n->core->device, ff.t_end);
        const double ns_per_tick = 1e9 / kRealtimeHz;
        trace_at(TP_GPU_START, in->token, s0 ? s0 : uint64_t(double(ff.t_start) * ns_per_tick));
        trace_at(TP_GPU_SIGNAL, in->token, s1 ? s1 : uint64_t(double(ff.t_end) * ns_per_tick));
      }
    }
  } else if (d.fill == FILL_EVENT) {
    // the producer's fill completes when its interprocess event fires
    hipEvent_t fill = nullptr;
    std::string key(reinterpret_cast<const char*>(d.event), 64);
    {
      std::lock_guard<std::mutex> g(n->core->ipc_mu);
      auto it = n->core->ipc_events.find(key);
      if (it != n->core->ipc_events.end()) {
        fill = it->second;
      } else {
        hipIpcEventHandle_t h;
        std::memcpy(&h, d.event, sizeof(h));
        DeviceScope ds(n->core->device);
        if (hipIpcOpenEventHandle(&fill, h) == hipSuccess) n->core->ipc_events[key] = fill;
        else fill = nullptr;
      }
    }
    // spin on the event (hipEventSynchronize sleeps in ~1 ms quanta on interprocess events
    // that are not yet complete), then fall back to the blocking wait
    hipError_t e = fill ? hipEventQuery(fill) : hipErrorInvalidHandle;
    const uint64_t t0 = mono_ns();
    while (e == hipErrorNotReady && mono_ns() - t0 < 20000000ull) {
      __builtin_ia32_pause();
      e = hipEventQuery(fill);
    }
    if (e == hipErrorNotReady) e = hipEventSynchronize(fill);
    if (e != hipSuccess) {
      ev->type = DORA_EVENT_ERROR;
      ev->error = std::string("waiting for the producer's fill event: ") + hipGetErrorString(e);
      in->ptr = nullptr;
      return;
    }
  }
  trace(TP_FILLED, in->token);
  if (n->core->device < 0) {
    // a receiver without a GPU gets the reference's host ArrowData (event.rs:35-91): the sample
    // is staged to host memory now and the producer's token goes back at once
    if (stage_to_host(in, int(d.device)) != DORA_OK) {
      ev->type = DORA_EVENT_ERROR;
      ev->error = dora_gpu_last_error();
      in->ptr = nullptr;
    }
    return;
  }
  if (in->len && (d.device != n->core->device || edge_copy_forced())) {
    // Cross-GPU edge: the sample is pulled over xGMI on first access to its data
    // (ensure_local), or straight into an outgoing slot by dora_node_forward.
    in->remote_device = d.device;
  }
}

}  // namespace

// Enqueue one copy of `len` bytes from a slot on `src_device` (IPC-mapped) into local HBM on
// the node stream: the pack kernel reading the peer's HBM over xGMI (default), or the copy
// engines (DORA_GPU_PEER_COPY=sdma).
int ensure_peer_access(NodeCore* c, int src_device) {
  if (src_device == c->device) return DORA_OK;
  std::lock_guard<std::mutex> g(c->ipc_mu);
  if (c->peer_enabled.count(src_device)) return DORA_OK;
  hipError_t e = hipDeviceEnablePeerAccess(src_device, 0);
  if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
    return fail(DORA_ERR_HIP, "enable peer access %d -> %d: %s", c->device, src_device,
                hipGetErrorString(e));
  (void)hipGetLastError();
  c->peer_enabled.insert(src_device);
  return DORA_OK;
}

int enqueue_peer_copy(NodeCore* c, void* dst, const void* src, int src_device, uint64_t len) {
  int rc = ensure_peer_access(c, src_device);
  if (rc != DORA_OK) return rc;
  c->stream_used.store(true, std::memory_order_relaxed);
  if (peer_copy_mode() == PEER_SDMA) {
    hipError_t e = hipMemcpyPeerAsync(dst, c->device, src, src_device, len, c->stream);
    if (e != hipSuccess) return fail(DORA_ERR_HIP, "hipMemcpyPeerAsync: %s", hipGetErrorString(e));
    return DORA_OK;
  }
  Segment seg{src, 0, len};
  return launch_pack(&seg, 1, ARROW_DEVICE_ROCM, static_cast<uint8_t*>(dst), c->stream, nullptr,
                     nullptr);
}

// Pull a cross-GPU input into this node's receive pool (complete on return) and hand the
// producer its slot back at once.
int ensure_local(InputData* in) {
  if (!in || (in->remote_device < 0 && !in->host_pull)) return DORA_OK;
  NodeCore* c = in->core.get();
  DeviceScope ds(c->device);
  uint64_t cap = 0;
  void* local = c->recv_pool.get(in->ext_len, &cap);
  if (!local)
    return fail(DORA_ERR_HIP, "receive slot of %llu bytes", (unsigned long long)in->ext_len);
  // The pull runs on a stream of its own and is waited for alone: on the node stream it would
  // queue behind (and its wait would wait for) every consumer kernel already there.
  // The pulled copy is complete on return, so any stream may read it.
  hipStream_t ps = c->stage_stream(c->device);
  if (!ps) ps = c->stream;
  int rc = DORA_OK;
  if (in->host_pull) {
    // a host-only producer's shared memory: pinned once per region on its first pull (not at
    // drain time, which may hold the event queue's lock), then one DMA into HBM
    {
      std::lock_guard<std::mutex> g(c->ipc_mu);
      if (!in->shm->reg_tried) {
        in->shm->reg_tried = true;
        in->shm->registered =
            hipHostRegister(in->shm->base, in->shm->len, hipHostRegisterDefault) == hipSuccess;
        (void)hipGetLastError();
      }
    }
    // the copy engines through HSA, its signal polled (as stage_to_host), once the region is
    // pinned; else HIP's copy.  Host-only 4 KB to a device receiver, send call to receipt:
    // 10.8-14.3 us p50 / 23-32 p99 against 17.5-20.3 / 45-58 (profiles/r06_pull_copy_ab.txt)
    rc = in->shm->registered ? hsa_copy_host(local, in->ptr, in->ext_len, false)
                             : int(DORA_ERR_UNSUPPORTED);
    if (rc == DORA_ERR_TIMEOUT) return rc;  // the receive slot is not reused: the copy may land
    if (rc != DORA_OK) {
      clear_error();
      rc = DORA_OK;
      hipError_t e = hipMemcpyAsync(local, in->ptr, in->ext_len, hipMemcpyHostToDevice, ps);
      if (e == hipSuccess) e = hipStreamSynchronize(ps);
      if (e != hipSuccess) rc = fail(DORA_ERR_HIP, "shared-memory pull: %s", hipGetErrorString(e));
    }
  } else if (peer_copy_mode() == PEER_SDMA) {
    rc = ensure_peer_access(c, in->remote_device);
    if (rc == DORA_OK) {
      hipError_t e =
          hipMemcpyPeerAsync(local, c->device, in->ptr, in->remote_device, in->ext_len, ps);
      if (e == hipSuccess) e = hipStreamSynchronize(ps);
      if (e != hipSuccess) rc = fail(DORA_ERR_HIP, "cross-GPU pull: %s", hipGetErrorString(e));
    }
  } else {
    // the pack kernel reads the peer's HBM over xGMI; wait on its own completion flag
    rc = ensure_peer_access(c, in->remote_device);
    Segment seg{in->ptr, 0, in->ext_len};
    if (rc == DORA_OK) rc = launch_pack_wait(&seg, 1, static_cast<uint8_t*>(local), ps);
  }
  if (rc != DORA_OK) {
    c->recv_pool.put(local, cap);
    return rc;
  }
  in->local = local;
  in->local_cap = cap;
  in->ptr = local;
  c->report_drop_token(in->token);
  trace(TP_RELEASED, in->token);
  in->has_token = false;
  if (in->host_pull) {
    in->host_pull = false;
    in->shm.reset();
    return DORA_OK;
  }
  in->remote_device = -1;
  c->peer_copies.fetch_add(1, std::memory_order_relaxed);
  c->peer_bytes.fetch_add(in->ext_len, std::memory_order_relaxed);
  return DORA_OK;
}

namespace {

// An input whose producer's fill is still running.  In the reference the sample is filled before
// the message leaves the sender (send_output returns after the copy), so such an input would not
// be queued here yet: the queue_size policy neither counts nor drops it.  Without this, an
// async sender with more samples in flight than a receiver's queue_size (12 vs the default 10)
// made the receiver drop inputs whenever it waited on the GPU: 20-25 % of a 1-4 MB burst from
// the Python node (scripts/py_tp.py), inputs the reference would have delivered.
// How long an input may sit in the queue uncounted because its producer's fill has not
// signalled: past 2 s the drop-oldest policy counts it again, so a fill that never completes (a
// lost queue, a GPU fault) cannot grow the queue beyond its queue_size.
constexpr uint64_t kTransitLimitNs = 2000000000ull;

bool fill_in_transit(dora_node* n, const dora_event* e) {
  if (!e->pending || e->ipc.fill != FILL_FLAG) return false;
  RegionHdr* h = n->core->region->hdr();
  if (e->ipc.flag_node >= h->n_nodes || e->ipc.flag_index >= kFillFlags) return false;
  if (fill_reached(&h->nodes[e->ipc.flag_node].fill[e->ipc.flag_index].epoch, e->ipc.epoch))
    return false;
  return mono_ns() - e->arrived_ns < kTransitLimitNs;
}

// drop_oldest_inputs (node_communication/mod.rs:320-359): newest first, keep queue_size per input.
// `held_front`: the queue's first event counts as taken (the event-stream thread's: the one the
// reference's thread holds in its channel, event_stream/thread.rs:139-157).
void drop_oldest_inputs(dora_node* n, bool held_front = false) {
  // no input can exceed its queue size while the whole queue holds no more events than the
  // smallest one (the common case of a receiver keeping up): nothing to count
  const size_t held = held_front ? 1 : 0;
  if (n->queue_size.empty() || n->queue.size() <= n->min_queue_size + held) return;
  SubSpan sp(SP_RECV_DROPOLD);
  std::map<std::string, uint32_t> remaining = n->queue_size;
  for (auto it = n->queue.rbegin(); it != n->queue.rend() - std::ptrdiff_t(held); ++it) {
    dora_event* e = it->get();
    if (!e || e->type != DORA_EVENT_INPUT) continue;
    auto q = remaining.find(e->id);
    if (q == remaining.end()) continue;
    if (fill_in_transit(n, e)) continue;
    if (q->second == 0) {
      it->reset();  // releases the InputData -> drop token reported
      ++n->dropped_inputs;
      n->core->region->hdr()->nodes[n->core->idx].dropped_inputs.fetch_add(
          1, std::memory_order_relaxed);
    } else {
      --q->second;
    }
  }
  n->queue.erase(std::remove_if(n->queue.begin(), n->queue.end(),
                                [](const std::unique_ptr<dora_event>& e) { return !e; }),
                 n->queue.end());
}

// Move every event the daemon has delivered into the node's queue; true when any arrived.
bool drain_events(dora_node* n) {
  uint32_t kind;
  std::vector<uint8_t>& p = n->ev_buf;  // reused across events
  SubSpan sp(SP_RECV_DRAIN);
  bool got = false;
  while (n->core->ev.try_pop(&kind, &p)) {
    encode_event(n, kind, p);
    got = true;
  }
  return got;
}

// A host-only node joins the L3 domain the dataflow's GPU nodes chose, once one has (it may
// start before them): its control-ring lines then move inside one L3 like theirs.
void pin_host_node(dora_node* n) {
  RegionHdr* rh = n->core->region->hdr();
  const int32_t numa = rh->numa_hint.load(std::memory_order_acquire);
  if (numa < 0 || rh->l3_cpu.load(std::memory_order_acquire) < 0) return;
  n->pin_pending = false;
  (void)pin_to_numa(numa, -1, &rh->l3_cpu, int(rh->n_nodes) + 1);
}

// The event-stream thread (dora_node::pump): drain, apply drop-oldest, wake the user thread.
// Draining allocates receive slots, opens IPC mappings, creates events and posts broadcast
// receives, all on the current HIP device of the calling thread: this thread's is the node's.
void pump_main(dora_node* n) {
  if (n->core->device >= 0) (void)hipSetDevice(n->core->device);
  while (!n->pump_stop.load(std::memory_order_acquire)) {
    bool got;
    {
      std::lock_guard<std::mutex> g(n->qmu);
      got = drain_events(n);
      if (got) drop_oldest_inputs(n, /*held_front=*/true);
    }
    if (got) n->qcv.notify_all();
    else n->core->ev.wait(10000);  // bounded: notices pump_stop
  }
}

}  // namespace

void start_pump(dora_node* n) {
  if (n->pump_on.load()) return;
  n->pump_stop.store(false);
  n->pump_on.store(true);
  n->pump = std::thread(pump_main, n);
}

void stop_pump(dora_node* n) {
  if (!n->pump_on.load()) return;
  n->pump_stop.store(true, std::memory_order_release);
  if (n->pump.joinable()) n->pump.join();
  n->pump_on.store(false);
}

}  // namespace dora

extern "C" {

int dora_node_set_event_thread(dora_node* n, int enable) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  DORA_GUARD_BEGIN
  if (enable) dora::start_pump(n);
  else dora::stop_pump(n);
  return DORA_OK;
  DORA_GUARD_END
}

int dora_node_next_event(dora_node* n, int64_t timeout_us, dora_event** out) {
  if (!n || !out) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  *out = nullptr;
  DORA_GUARD_BEGIN
  if (n->pin_pending) dora::pin_host_node(n);
  const uint64_t t0 = dora::mono_ns();
  if (n->want_pump && !n->pump_on.load()) dora::start_pump(n);
  if (n->pump_on.load()) {
    // the event-stream thread fills the queue: take its oldest event
    std::unique_lock<std::mutex> g(n->qmu);
    for (;;) {
      if (!n->queue.empty()) {
        *out = n->queue.front().release();
        n->queue.pop_front();
        if ((*out)->type == DORA_EVENT_ALL_INPUTS_CLOSED) n->ended = true;
        g.unlock();
        dora::finish_input(n, *out);
        return DORA_OK;
      }
      if (n->ended) return dora::fail(DORA_ERR_CLOSED, "event stream closed");
      if (timeout_us < 0) {
        n->qcv.wait_for(g, std::chrono::milliseconds(100));
        continue;
      }
      const int64_t left = timeout_us - int64_t(dora::mono_ns() - t0) / 1000;
      if (left <= 0) return dora::fail(DORA_ERR_TIMEOUT, "no event within timeout");
      n->qcv.wait_for(g, std::chrono::microseconds(left));
    }
  }
  for (;;) {
    const bool got = dora::drain_events(n);
    if (n->want_pump && !n->pump_on.load()) {
      // a broadcast group was joined while draining: the thread takes over from here
      dora::start_pump(n);
      return dora_node_next_event(n, timeout_us < 0 ? -1
                                     : std::max<int64_t>(0, timeout_us - int64_t(dora::mono_ns() - t0) / 1000), out);
    }
    if (!n->queue.empty()) {
      // The event handed over now is the node's, like the one the reference's event-stream
      // thread holds (event_stream/thread.rs:139-157: taken from the daemon's queue, in its
      // channel): the drop-oldest policy keeps queue_size inputs per input id among the rest.
      // So a sender with queue_size + 1 samples in flight (node_send.cpp max_in_flight) never makes
      // a default receiver drop, whenever that receiver pauses.
      *out = n->queue.front().release();
      n->queue.pop_front();
      if ((*out)->type == DORA_EVENT_ALL_INPUTS_CLOSED) n->ended = true;
      if (got) dora::drop_oldest_inputs(n);
      dora::finish_input(n, *out);
      return DORA_OK;
    }
    if (n->ended) return dora::fail(DORA_ERR_CLOSED, "event stream closed");
    int64_t left = -1;
    if (timeout_us >= 0) {
      left = timeout_us - int64_t(dora::mono_ns() - t0) / 1000;
      if (left <= 0) return dora::fail(DORA_ERR_TIMEOUT, "no event within timeout");
    }
    n->core->ev.wait(left < 0 ? 1000000 : left);
  }
  DORA_GUARD_END
}

int dora_event_type(const dora_event* e) { return e ? e->type : DORA_EVENT_ERROR; }

const char* dora_event_id(const dora_event* e) { return e ? e->id.c_str() : ""; }

const char* dora_event_error(const dora_event* e) { return e ? e->error.c_str() : ""; }

int dora_event_data(const dora_event* e, const void** ptr, size_t* len) {
  if (!e || !ptr || !len) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  if (!e->data) return dora::fail(DORA_ERR_INVALID, "event has no data");
  DORA_GUARD_BEGIN
  int rc = dora::ensure_local(e->data.get());
  if (rc != DORA_OK) return rc;
  DORA_GUARD_END
  *ptr = e->data->ptr;
  *len = e->data->len;
  return DORA_OK;
}

int dora_event_is_device(const dora_event* e) {
  return e && e->data && (e->data->has_token || e->data->local) && !e->data->host_mem;
}

int dora_event_type_info(const dora_event* e, const uint8_t** ti, size_t* len) {
  if (!e || !ti || !len) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  if (!e->ti_checked && e->type == DORA_EVENT_INPUT && e->data && e->data->ext_len > e->data->len) {
    // bitmaps in the sample's tail: restore the reference's inline ArrowTypeInfo bytes
    DORA_GUARD_BEGIN
    int rc = dora::ensure_local(e->data.get());
    if (rc != DORA_OK) return rc;
    bool changed = false;
    rc = dora::inline_type_info(e->meta.type_info.data(), e->meta.type_info.size(),
                                e->data->ptr, e->data->ext_len, &e->ti_inline, &changed,
                                e->data->host_mem);
    if (rc != DORA_OK) return rc;
    DORA_GUARD_END
  }
  e->ti_checked = true;
  const std::vector<uint8_t>& t = e->ti_inline.empty() ? e->meta.type_info : e->ti_inline;
  *ti = t.data();
  *len = t.size();
  return DORA_OK;
}

int dora_event_parameters(const dora_event* e, const uint8_t** p, size_t* len) {
  if (!e || !p || !len) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  *p = e->meta.parameters.data();
  *len = e->meta.parameters.size();
  return DORA_OK;
}

uint64_t dora_event_timestamp_ns(const dora_event* e) { return e ? e->meta.timestamp_ns : 0; }

int dora_event_array(const dora_event* e, struct ArrowArray* out_array,
                     struct ArrowSchema* out_schema) {
  if (!e || !out_array || !out_schema) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  if (e->type != DORA_EVENT_INPUT || !e->data)
    return dora::fail(DORA_ERR_INVALID, "not an input event");
  if (!e->data->ptr && e->data->len)
    return dora::fail(DORA_ERR_INVALID, "input data is not mapped: %s", e->error.c_str());
  DORA_GUARD_BEGIN
  int rc = dora::ensure_local(e->data.get());
  if (rc != DORA_OK) return rc;
  DORA_GUARD_END
  std::shared_ptr<void> keep = e->data;
  // an inline Vec sample, shared memory read in place or a device sample staged to host memory:
  // a host array over its bytes (a staged sample keeps its validity tail)
  if (e->data->host_mem || (!e->data->has_token && !e->data->local))
    return dora::import_sample(e->data->ptr, e->data->len, e->meta.type_info.data(),
                               e->meta.type_info.size(), keep, out_array, out_schema,
                               e->data->ext_len, true);
  return dora::import_sample(e->data->ptr, e->data->len, e->meta.type_info.data(),
                             e->meta.type_info.size(), keep, out_array, out_schema,
                             e->data->ext_len);
}

void dora_event_free(dora_event* e) { delete e; }

}  // extern "C"
