
// The send path: a sample's slot (alloc_sample, host_bound_sample), its fill and completion
// signal (fill_sample, order_fill, host_bar_fill), its descriptor (send_sample), forwards, the
// plan cache, and the send, sample and ticket entry points.
#include "node_internal.h"

namespace dora {
namespace {

// Samples a node may have in flight (sent, token not yet back) before an allocation waits.
constexpr uint64_t kSmallInFlightBytes = 8ull << 20;

// Samples a sender may have in flight (sent, token not back) before it waits for a returned
// slot.  Below 8 MiB a message's life is dominated by the dispatch-to-fill-flag latency
// (~5-8 us for a 4 KB-4 MB pack over the AQL queues, scripts/trace_report.py), so the pipeline
// depth sets the rate: 11 there, 8 for larger samples, which are HBM-bound and lose to more
// concurrent packs (C3, 13 MB: -20 % at 12).  11 = the reference's default queue_size (10) + the
// input a receiver is handed: every input queued at a receiver is in flight, and the drop-oldest
// policy runs after next_event has taken its event (dora_node_next_event), so a default receiver
// drops nothing whenever it pauses.  (r03 applied the policy before taking the event: a
// receiver that paused between releasing one input and taking the next then had 11 ready and
// dropped one, 0-5 per bench run in the throughput ladders.  A cap of 10 instead cost 4 MB
// sends ~6 %: 1.56-1.63 vs 1.41-1.50 us, profiles/r04_cap_ab.jsonl.)  DORA_GPU_MAX_IN_FLIGHT=N
// sets both, `S:L` each.
size_t max_in_flight(uint64_t len) {
  static const std::pair<long, long> env = [] {
    const char* e = std::getenv("DORA_GPU_MAX_IN_FLIGHT");
    if (!e) return std::make_pair(0L, 0L);
    char* end = nullptr;
    const long a = std::strtol(e, &end, 10);
    const long b = (end && *end == ':') ? std::atol(end + 1) : a;
    return std::make_pair(a, b);
  }();
  const long v = len < kSmallInFlightBytes ? env.first : env.second;
  if (v > 0) return static_cast<size_t>(v);
  return len < kSmallInFlightBytes ? 11 : 8;
}

// How long an allocation waits for a returned token at the in-flight cap before it allocates
// anyway, as the reference would (a receiver may legitimately hold many inputs)
constexpr uint64_t kSlotWaitNs = 5000000;

// The Metadata of a send as WBuf::bytes(WBuf::metadata(m)) would write it, straight into `w`
// (no Metadata copy of the type info and parameters per send).
void put_metadata(WBuf& w, const std::vector<uint8_t>& ti, const uint8_t* params,
                  size_t params_len, uint64_t ts) {
  const uint64_t n = 2 + 8 + 8 + ti.size() + 8 + (params ? params_len : 0);
  w.u64(n);
  w.u16(0);  // metadata version
  w.u64(ts);
  w.bytes(ti.data(), ti.size());
  w.bytes(params, params ? params_len : 0);
}

int send_sample(dora_node* n, const char* output_id, const std::vector<uint8_t>& ti,
                const uint8_t* params, size_t params_len, dora_sample* sample,
                DropToken* token_out = nullptr, uint64_t ts_override = 0) {
  {
    SubSpan sp(SP_SEND_TOKENS);
    handle_finished_drop_tokens(n);
  }
  SubSpan sp_lookup(SP_SEND_LOOKUP);
  if (!n->outputs.count(output_id)) {
    delete sample;  // the sample is consumed either way
    return fail(DORA_ERR_NOT_FOUND,
                "unknown dora node output `%s` called by `send_output`. Double-check if this "
                "output is defined within your dataflow YAML file.",
                output_id);
  }
  // Metadata::from_parameters(clock.new_timestamp(), ..) mod.rs:258; a proxy of a remote
  // node keeps the producer's timestamp (the inter-daemon message's metadata)
  sp_lookup.stop();
  SubSpan sp_req(SP_SEND_REQUEST);
  const uint64_t ts = ts_override ? ts_override : now_ns();
  DataMsg d;
  Slot* slot = nullptr;
  if (sample) {
    if (sample->slot && sample->slot->host) {
      slot = sample->slot;
      d.kind = DATA_SHMEM;
      d.shm.name = slot->shm_name;
      d.shm.len = sample->len;
      d.shm.token = generate_drop_token();
    } else if (sample->slot) {
      slot = sample->slot;
      d.kind = DATA_DEVICE_IPC;
      std::memcpy(d.ipc.handle, &slot->handle, 64);
      d.ipc.device = n->core->device;
      d.ipc.owner_pid = self_pid();
      d.ipc.slot_id = slot->id;
      d.ipc.offset = 0;
      d.ipc.len = sample->len;
      d.ipc.ext_len = std::max(sample->len, sample->ext_len);
      d.ipc.token = generate_drop_token();
      d.ipc.fill = sample->fill;
      auto g = n->bcast_out.find(output_id);
      if (g != n->bcast_out.end()) {
        // fan-out over the output's RCCL group: broadcast the slot on the output's stream, after
        // its pack there (pack_and_send), or — a sample the user filled — after the work queued on
        // the node stream and every fill so far
        hipStream_t bs = g->second.stream;
        DeviceScope ds(n->core->device);
        if (sample->fill != FILL_DONE) n->core->fence_fills();
        n->core->order_after_node_stream(bs);
        int rc = bcast_enqueue(g->second.comm, slot->ptr, d.ipc.ext_len, bs);
        // the broadcast reads the slot on its stream: the slot is idle after it
        if (!slot->use_ev && hipEventCreateWithFlags(&slot->use_ev, hipEventDisableTiming) != hipSuccess)
          slot->use_ev = nullptr;
        if (slot->use_ev && hipEventRecord(slot->use_ev, bs) == hipSuccess)
          slot->use_pending = true;
        else
          (void)hipStreamSynchronize(bs);
        (void)hipGetLastError();
        if (rc != DORA_OK) {
          add_to_cache(n, slot);
          delete sample;
          return rc;
        }
        d.ipc.fill = FILL_BCAST;
        d.ipc.epoch = ++n->bcast_seq;
      } else if (sample->fill == FILL_FLAG) {
        d.ipc.flag_node = static_cast<uint32_t>(n->core->idx);
        d.ipc.flag_index = static_cast<uint32_t>(slot->flag);
        d.ipc.epoch = sample->epoch;
      }
      if (d.ipc.fill == FILL_EVENT) std::memcpy(d.ipc.event, &slot->done_handle, 64);
    } else {
      d.kind = DATA_VEC;
      d.vec = std::move(sample->vec);
    }
    delete sample;
  }
  WBuf& w = n->send_buf;
  w.clear();
  w.str(output_id);
  put_metadata(w, ti, params, params_len, ts);
  w.data(d);
  int rc = n->core->request(REQ_SEND_MESSAGE, w.data(), w.size());
  sp_req.stop();
  if (rc != DORA_OK) {
    if (slot) add_to_cache(n, slot);
    return rc;
  }
  SubSpan sp_track(SP_SEND_TRACK);
  if (slot && d.kind == DATA_SHMEM) {
    n->sent_out[d.shm.token] = slot;
    if (token_out) *token_out = d.shm.token;
  } else if (slot) {
    n->sent_out[d.ipc.token] = slot;
    if (token_out) *token_out = d.ipc.token;
    trace(n->core->last_rang ? TP_SENT_RANG : TP_SENT, d.ipc.token);
  } else if (trace_enabled()) {
    trace(n->core->last_rang ? TP_SENT_RANG : TP_SENT, ts_key(ts));  // an inline sample
  }
  return DORA_OK;
}

constexpr uint64_t kZeroCopyThreshold = 4096;  // mod.rs:40

// Wait, up to kSlotWaitNs, for a returned token while `n` has max_in_flight(len) samples out;
// a node whose region entry says done (state 2) stops waiting.
void wait_for_send_credit(dora_node* n, uint64_t len) {
  const uint64_t t0 = mono_ns();
  while (n->sent_out.size() >= max_in_flight(len) && mono_ns() - t0 < kSlotWaitNs) {
    n->core->drops.wait(1000);
    handle_finished_drop_tokens(n);
    if (n->core->region->hdr()->nodes[n->core->idx].state.load() == 2) break;
  }
}

// `ext_len` > len: the slot also holds a validity tail (plans with in-sample bitmaps).
// `host_inline`: the sample will be written by the host (a host-resident source), so below the
// zero-copy threshold it takes the reference's inline `DataMessage::Vec` (mod.rs:303-319) on a
// device node too: no slot, no H2D copy, no fill signal.
// `workspace`: scratch bytes of the fill's launches behind the sample (a mask plan's): the slot
// holds them, the sample's lengths — what the descriptor names and anything downstream moves — do
// not.
int alloc_sample(dora_node* n, uint64_t len, dora_sample** out, uint64_t ext_len = 0,
                 bool host_inline = false, uint64_t workspace = 0) {  // mod.rs:303-319
  if (n->core->device < 0 && len >= kZeroCopyThreshold) {
    // host-only node: a POSIX shared-memory slot (the reference's allocate_shared_memory)
    auto* s = new dora_sample();
    s->len = len;
    handle_finished_drop_tokens(n);
    int rc = allocate_host_slot(n, len, &s->slot);
    if (rc != DORA_OK) {
      delete s;
      return rc;
    }
    *out = s;
    return DORA_OK;
  }
  if (n->core->device < 0 || (host_inline && std::max(len, ext_len) < kZeroCopyThreshold)) {
    auto* s = new dora_sample();
    s->len = len;
    s->vec.assign(len, 0);  // AVec::__from_elem(128, 0, len)
    *out = s;
    return DORA_OK;
  }
  SubSpan sp_new(SP_SAMPLE_NEW);
  auto* s = new dora_sample();
  s->len = len;
  sp_new.stop();
  if (len > 0) {
    if (!n->aql_ready) {
      // the first non-empty sample of this node sets up the process's AQL queues and loads the
      // pack code object (~20 ms), whatever its size: a later small send then finds them ready
      // instead of paying that inside its latency (nodes that never send data create none)
      n->aql_ready = true;
      if (aql_queue(n->core->device)) ensure_cp_stamps(n);
    }
    SubSpan sp_tok(SP_ALLOC_TOKENS);
    handle_finished_drop_tokens(n);
    sp_tok.stop();
    // Sends run ahead of the GPU; bound the samples in flight so the sender waits for a
    // returned slot instead of hipMalloc-ing new ones (a device slot costs far more to create
    // than a shm region).  After kSlotWaitNs without a returned token the slot is allocated
    // anyway, as the reference would (a receiver may legitimately hold many inputs).
    SubSpan sp_wait(SP_ALLOC_WAIT);
    wait_for_send_credit(n, len);
    sp_wait.stop();
    s->ext_len = std::max(len, ext_len);
    SubSpan sp_slot(SP_ALLOC_SLOT);
    int rc = allocate_slot(n, s->ext_len + workspace, &s->slot);
    if (rc != DORA_OK) {
      delete s;
      return rc;
    }
  }
  *out = s;
  return DORA_OK;
}

// Device-resident samples up to this size for an output whose receivers all lack a GPU are
// packed by the GPU straight into a shared-memory region (host_bound_sample): one dispatch on
// the sender's warm queues instead of a slot in HBM that each receiver copies out with a HIP copy
// of its own (stage_to_host, ~13 us of runtime overhead at any small size).  Larger samples keep
// that path: the copy engines move them at the box's DMA rate and leave the CUs free, where a
// pack writing over PCIe would hold its workgroups for the whole transfer.
constexpr uint64_t kHostPackMax = 1ull << 20;

// A sample for such an output: a shared-memory slot of this node (the reference's
// DataMessage::SharedMemory, which its receivers map), page-locked and mapped for the GPU once,
// with a fill flag for the pack to signal.  Null, with no error, when one cannot be made (no
// free fill flag, registration refused): the caller takes an HBM slot.
dora_sample* host_bound_sample(dora_node* n, uint64_t len, uint64_t ext_len) {
  NodeCore* c = n->core.get();
  if (!c->region_dev || !c->fill_done) return nullptr;
  handle_finished_drop_tokens(n);
  wait_for_send_credit(n, len);
  Slot* slot = nullptr;
  const uint64_t ext = std::max(len, ext_len);
  if (allocate_host_slot(n, ext, &slot) != DORA_OK) {
    clear_error();
    return nullptr;
  }
  if (!slot->registered) {
    DeviceScope ds(c->device);
    void* dp = nullptr;
    if (hipHostRegister(slot->ptr, slot->cap, hipHostRegisterMapped | hipHostRegisterPortable) !=
        hipSuccess) {
      (void)hipGetLastError();
      release_slot_memory(slot);
      return nullptr;
    }
    slot->registered = true;
    // the pack writes through the host address (one address space for host and GPU)
    if (hipHostGetDevicePointer(&dp, slot->ptr, 0) != hipSuccess || dp != slot->ptr) {
      (void)hipGetLastError();
      release_slot_memory(slot);
      return nullptr;
    }
  }
  if (slot->flag < 0) {
    if (c->free_flags.empty()) {
      add_to_cache(n, slot);
      return nullptr;
    }
    slot->flag = static_cast<int>(c->free_flags.back());
    c->free_flags.pop_back();
  }
  auto* s = new dora_sample();
  s->len = len;
  s->ext_len = ext;
  s->slot = slot;
  return s;
}

// A ticketed sample (dora_sample_fill_ticket) that will not be sent, or whose send failed: its
// kernel may have been launched or not, and nobody else will raise the flag.  Drain the node
// stream (a kernel queued there has then stored the epoch itself), then raise the flag to the
// ticket's epoch from the host if it is still below it — epochs only grow, so the store of a
// kernel that runs late is harmless — so that no later allocation, dora_node_sync or free_slot
// waits on an epoch nobody will store.
void settle_ticket(dora_node* n, dora_sample* s) {
  if (!s->self_published || !s->slot || s->slot->flag < 0) return;
  NodeCore* c = n->core.get();
  {
    DeviceScope ds(c->device);
    if (c->stream && hipStreamQuery(c->stream) == hipErrorNotReady)
      (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
  }
  auto& f = c->region->hdr()->nodes[c->idx].fill[s->slot->flag].epoch;
  uint64_t cur = f.load(std::memory_order_acquire);
  while (cur < s->epoch && !f.compare_exchange_weak(cur, s->epoch, std::memory_order_acq_rel)) {
  }
  s->self_published = false;
}

}  // namespace

// An unsent sample back to the node: its slot to the cache (an inline Vec is just freed).
void discard_sample(dora_node* n, dora_sample* s) {
  if (!s) return;
  settle_ticket(n, s);
  if (s->slot) add_to_cache(n, s->slot);
  delete s;
}

namespace {

// Tell receivers when the fill enqueued on stream `st` is complete.
hipError_t order_fill(dora_node* n, dora_sample* s, hipStream_t st) {
  if (s->slot->flag >= 0) {
    // async: the stream writes the send epoch into the slot's fill flag once the fill has
    // completed; the receiver polls it, the sender moves on
    mark_flag_fill(n->core.get(), s, ++n->core->epoch, NOTE_NONE);
    return hipStreamWriteValue64(st, n->core->flag_dev(s->slot->flag), s->epoch, 0);
  }
  if (s->slot->done) {
    // async fallback: interprocess event
    s->fill = FILL_EVENT;
    return hipEventRecord(s->slot->done, st);
  }
  // sync: the sample must be complete before its descriptor leaves the process
  return hipStreamSynchronize(st);
}

// Launch the fill of sample `s` (segments into its slot) on stream `st` and order its
// completion signal.
int fill_sample(dora_node* n, dora_sample* s, const Segment* segs, size_t nseg,
                ArrowDeviceType dev, hipStream_t st, hipEvent_t t_start, hipEvent_t t_stop,
                bool signal = true, bool sync = false) {
  if (!signal) {
    // the caller orders what follows on `st` (a broadcast-group send): no fill flag
    DeviceScope ds(n->core->device);
    ++n->hip_packs;
    return launch_pack(segs, nseg, dev, static_cast<uint8_t*>(s->slot->ptr), st, t_start, t_stop,
                       nullptr, nullptr, slot_bytes(s->slot->cap));
  }
  FillSignal sig{};
  const FillSignal* sp = nullptr;
  if (s->slot->flag >= 0 && n->core->fill_done) {
    sig.flag = n->core->flag_dev(s->slot->flag);
    sig.epoch = ++n->core->epoch;
    sig.done = n->core->fill_done + size_t(s->slot->flag) * kMaxSignalWgs;
    sp = &sig;
  }
  if (sp && !st && !t_start && !t_stop && dev == ARROW_DEVICE_ROCM &&
      nseg <= aql_max_segments() &&
      std::all_of(segs, segs + nseg, [](const Segment& g) { return g.op == SEG_COPY; }) &&
      [&] {
        SubSpan sq(SP_STREAM_QUERY);
        return !n->core->stream_busy();
      }()) {
    // host-bound size: one raw AQL packet instead of hipLaunchKernel (aql.h)
    if (AqlQueue* q = n->core->aql_queue_once()) {
      const std::atomic<uint64_t>* fh = n->core->flag_host(s->slot->flag);
      // a timed region's pack may be signalled by the command processor if it has a stamp area
      int area = -1;
      uint64_t* stamps = nullptr;
      // (only a pack aql_pack will CP-signal takes one: a region has kRegionCpAreas of them)
      if (n->timed.armed && n->timed.cp_stamps && n->timed.cp_next < kRegionCpAreas &&
          aql_cp_candidate(segs, nseg, sync)) {
        area = int(n->timed.cp_next++);
        stamps = n->timed.cp_stamps + size_t(area) * kCpAreaWords;
      }
      s->slot->region_cp_area = area;
      bool read = false;
      if (aql_pack(q, segs, nseg, static_cast<uint8_t*>(s->slot->ptr), sig, fh,
                   n->timed.armed, s->slot->host ? s->slot->cap : slot_bytes(s->slot->cap),
                   stamps, sync, &read) == DORA_OK) {
        s->read_signalled = read;
        mark_flag_fill(n->core.get(), s, sig.epoch, NOTE_SYNC_AND_FENCE);
        if (n->timed.armed) ++n->timed.aql;
        ++n->aql_packs;
        s->stamped = true;
        return DORA_OK;
      }
    }
  }
  // (a failed AQL dispatch lands here too: the HIP launch below reuses the epoch taken above)
  DeviceScope ds(n->core->device);  // HIP launches and event records below
  if (!st) st = n->core->next_fill_stream();
  ++n->hip_packs;
  bool signalled = false;
  int rc = launch_pack(segs, nseg, dev, static_cast<uint8_t*>(s->slot->ptr), st, t_start,
                       t_stop, sp, &signalled,
                       s->slot->host ? s->slot->cap : slot_bytes(s->slot->cap));
  if (rc != DORA_OK) return rc;
  if (signalled) {
    mark_flag_fill(n->core.get(), s, sig.epoch, NOTE_SYNC);
    s->stamped = true;
    return DORA_OK;
  }
  for (size_t i = 0; i < n->core->fill_streams.size(); ++i)
    if (n->core->fill_streams[i] == st) n->core->fill_unsignalled[i] = 1;
  hipError_t e = order_fill(n, s, st);
  if (e != hipSuccess) return fail(DORA_ERR_HIP, "fill signal: %s", hipGetErrorString(e));
  return DORA_OK;
}

// Launch the gather of a gather plan (tensor_plan.cpp: one strided device tensor view, or the
// fields of a struct of device tensors of which any is strided, in one launch) into sample
// `s` on stream `st` (null: the next fill stream, ordered after the node stream) and let the
// stream write the fill epoch behind it (order_fill): no AQL packet, no in-kernel signal.
int gather_sample(dora_node* n, dora_sample* s, const dora_plan& plan, hipStream_t st,
                  hipEvent_t t_start, hipEvent_t t_stop, bool signal) {
  DeviceScope ds(n->core->device);
  if (!st) st = n->core->next_fill_stream();
  ++n->hip_packs;
  int rc = launch_plan_gather(plan, static_cast<uint8_t*>(s->slot->ptr), st, t_start, t_stop);
  if (rc != DORA_OK || !signal) return rc;  // (a broadcast-group send orders what follows itself)
  for (size_t i = 0; i < n->core->fill_streams.size(); ++i)
    if (n->core->fill_streams[i] == st) n->core->fill_unsignalled[i] = 1;
  hipError_t e = order_fill(n, s, st);
  if (e != hipSuccess) return fail(DORA_ERR_HIP, "fill signal: %s", hipGetErrorString(e));
  return DORA_OK;
}

// A same-GPU device input re-sent in place: the descriptor points at the producer's slot (its
// fill is complete: the input was handed out), under a token of this node; the input — and with
// it the producer's token — is held until that token returns.  No copy, no new slot.
int forward_in_place(dora_node* n, const char* output_id, const dora_event* ev,
                     const uint8_t* params, size_t params_len) {
  handle_finished_drop_tokens(n);
  if (!n->outputs.count(output_id))
    return fail(DORA_ERR_NOT_FOUND, "unknown dora node output `%s`", output_id);
  DataMsg d;
  d.kind = DATA_DEVICE_IPC;
  d.ipc = ev->ipc;
  d.ipc.token = generate_drop_token();
  d.ipc.fill = FILL_DONE;
  d.ipc.flag_node = d.ipc.flag_index = 0;
  d.ipc.epoch = 0;
  WBuf& w = n->send_buf;
  w.clear();
  w.str(output_id);
  put_metadata(w, ev->meta.type_info, params, params_len, now_ns());
  w.data(d);
  int rc = n->core->request(REQ_SEND_MESSAGE, w.data(), w.size());
  if (rc != DORA_OK) return rc;
  n->forwarded[d.ipc.token] = ev->data;
  ++n->zero_copy_forwards;
  trace(TP_SENT, d.ipc.token);
  return DORA_OK;
}

// Re-send a received input on an output with its type info (a relay stage): one copy into a
// fresh slot of this node — for a cross-GPU input straight from the peer's slot over xGMI, so
// a pipeline hop moves the payload once.
int forward_input(dora_node* n, const char* output_id, const dora_event* ev, const uint8_t* params,
                  size_t params_len) {
  InputData* in = ev->data.get();
  if (in->host_pull) {  // a shared-memory input of a device receiver: into HBM first
    int rc = ensure_local(in);
    if (rc != DORA_OK) return rc;
  }
  if (in->has_token && !in->local && in->remote_device < 0 && in->len && !in->host_mem &&
      ev->ipc.device == n->core->device && ev->ipc.fill != FILL_BCAST && !edge_copy_forced() &&
      !n->bcast_out.count(output_id))
    return forward_in_place(n, output_id, ev, params, params_len);
  const uint64_t len = in->len;
  const uint64_t ext = std::max(in->ext_len, len);  // the validity tail travels along
  const bool device_src = (in->has_token || in->local) && !in->host_mem;
  dora_sample* s = nullptr;
  int rc = alloc_sample(n, len, &s, ext, !device_src);
  if (rc != DORA_OK) return rc;
  if (len && (!s->slot || s->slot->host)) {
    if (device_src) {
      discard_sample(n, s);
      return fail(DORA_ERR_INVALID, "host-only node cannot forward device-resident data");
    }
    std::memcpy(s->slot ? s->slot->ptr : s->vec.data(), in->ptr, len);
  } else if (len) {
    Segment seg{in->ptr, 0, ext};
    if (in->remote_device >= 0 && peer_copy_mode() == PEER_SDMA) {
      rc = enqueue_peer_copy(n->core.get(), s->slot->ptr, in->ptr, in->remote_device, ext);
      hipError_t e = rc == DORA_OK ? order_fill(n, s, n->core->stream) : hipSuccess;
      if (rc == DORA_OK && e != hipSuccess)
        rc = fail(DORA_ERR_HIP, "forward: %s", hipGetErrorString(e));
    } else {
      // the pack kernel, reading the peer's HBM over xGMI for a cross-GPU input; on the node
      // stream, which the input's destructor drains before its token goes back
      rc = in->remote_device >= 0 ? ensure_peer_access(n->core.get(), in->remote_device)
                                  : DORA_OK;
      n->core->stream_used.store(true, std::memory_order_relaxed);
      if (rc == DORA_OK)
        rc = fill_sample(n, s, &seg, 1, device_src ? ARROW_DEVICE_ROCM : ARROW_DEVICE_CPU,
                         n->core->stream, nullptr, nullptr);
    }
    if (rc == DORA_OK && in->remote_device >= 0) {
      n->core->peer_copies.fetch_add(1, std::memory_order_relaxed);
      n->core->peer_bytes.fetch_add(ext, std::memory_order_relaxed);
    }
    if (rc != DORA_OK) {
      add_to_cache(n, s->slot);
      delete s;
      return rc;
    }
  }
  // the input keeps the producer's token until this node's stream has passed the copy
  // (InputData's destructor), so the producer cannot refill the slot under it
  return send_sample(n, output_id, ev->meta.type_info, params, params_len, s);
}

// What a synchronous send of a device source waits for: the pack has read the whole source.
struct SourceWait {
  uint8_t kind = FILL_DONE;  // FILL_FLAG: flag >= epoch; FILL_EVENT: event; FILL_BCAST: stream
  bool read = false;  // FILL_FLAG of a read-signalled pack: its read word >= epoch suffices
  hipStream_t stream = nullptr;  // FILL_BCAST: the output's broadcast stream
  const std::atomic<uint64_t>* flag = nullptr;
  uint64_t epoch = 0;
  hipEvent_t event = nullptr;
};

// The reference copies a source inside send_output (arrow_utils.rs:48, node/mod.rs:206-209), so
// its caller may rewrite the source as soon as the call returns.  A device source is read by the
// pack kernel after the call has queued it; without DORA_SEND_ASYNC the call waits for that pack
// (spin, then yield; bounded) — after the descriptor has left, so receivers are not delayed.
int wait_source_read(dora_node* n, const SourceWait& w) {
  SubSpan sp(SP_SEND_SOURCE_WAIT);
  if (w.kind == FILL_FLAG && w.flag) {
    const uint64_t t0 = mono_ns();
    uint32_t spins = 0;
    const auto* ff = reinterpret_cast<const FillFlag*>(w.flag);
    while (!(w.read && ff->read_epoch.load(std::memory_order_acquire) >= w.epoch) &&
           !fill_reached(w.flag, w.epoch)) {
      if (++spins < 4096) {
        __builtin_ia32_pause();
        continue;
      }
      const uint64_t dt = mono_ns() - t0;
      if (dt > 10000000000ull) return fail(DORA_ERR_TIMEOUT, "pack did not read its source in 10 s");
      if (dt > 200000) std::this_thread::yield();
    }
  } else if (w.kind == FILL_EVENT && w.event) {
    DORA_HIP(hipEventSynchronize(w.event));
  } else if (w.kind == FILL_BCAST && w.stream) {
    DORA_HIP(hipStreamSynchronize(w.stream));
  }
  return DORA_OK;
}

// Host-resident sources up to this size are written into their device slot by the CPU through
// the large BAR (host_bar_fill); larger ones are DMA'd by HIP.  On an MI355X box the BAR path
// delivers 4 KB in 1.9 us and 1 MiB in 30 us (35 GB/s), HIP's copy takes 13-14 us up to 64 KB,
// 52 us at 1 MiB and wins from ~2 MiB (4 MiB: 89 vs 140 us; 40.96 MB: 56 GB/s)
// (profiles/r06_host_path_probe.jsonl).
constexpr uint64_t kBarFillMax = 2ull << 20;

// The reference copies a host source into its shared-memory sample on the CPU inside
// send_output (arrow_utils.rs:48, node/mod.rs:180-215).  A device node does the same into its
// HBM slot: the slot is mapped for the CPU once, the segments are written with streaming stores,
// and one HDP flush + read-back makes them visible before the descriptor leaves, so the sample
// is complete when the call returns (FILL_DONE: no GPU dispatch, no fill flag).  False when the
// slot cannot be mapped (no large BAR, no HSA): the caller takes the HIP copy.
bool host_bar_fill(dora_node* n, dora_sample* s, const std::vector<Segment>& segs) {
  Slot* slot = s->slot;
  if (!slot || slot->host || s->ext_len > kBarFillMax) return false;
  AqlQueue* q = n->core->aql_queue_once();
  if (!q) return false;
  if (!slot->bar_tried) {
    slot->bar_tried = true;
    slot->bar = bar_map(q, slot->ptr) == DORA_OK;
    if (!slot->bar) clear_error();
  }
  if (!slot->bar) return false;
  for (const Segment& g : segs)
    if (g.op != SEG_COPY) return false;
  auto* dst = static_cast<uint8_t*>(slot->ptr);
  const uint8_t* last = nullptr;
  for (const Segment& g : segs) {
    if (!g.len) continue;
    bar_copy(dst + g.dst_off, g.src, g.len);
    last = dst + g.dst_off + g.len - 1;
  }
  bar_publish(q, last);
  s->fill = FILL_DONE;
  ++n->bar_fills;
  return true;
}

int pack_and_send(dora_node* n, const char* output_id, const dora_plan* plan, const uint8_t* params,
                  size_t params_len, const std::vector<uint8_t>* ti_pre = nullptr,
                  uint32_t flags = 0) {
  dora_sample* s = nullptr;
  const uint64_t t0 = mono_ns();
  // a host-resident array below the zero-copy threshold goes inline, as in the reference
  const bool host_src = plan->dev != ARROW_DEVICE_ROCM;
  const bool gather = plan->launch != PlanLaunch::kSegments;  // a kernel, not `segs`, fills it
  if (plan->dev_tensor && plan->size && n->core->device >= 0) {
    // a device tensor view: its strides are the caller's, so the runtime names the allocation
    // it must lie in before anything is allocated or launched
    DeviceScope ds(n->core->device);
    const int rc = check_plan_range(*plan, n->core->device);
    if (rc != DORA_OK) return rc;
  }
  // a device array for receivers that all lack a GPU: packed into shared memory
  // (host_bound_sample; not inside a timed region, whose stamps live in HBM slots' flags, and
  // not a plan whose validity bitmaps travel in a tail past the sample: a SharedMemory message
  // has no room to name one)
  const bool host_bound = plan->size && plan->fill_size() == plan->size && !n->host_bound.empty() &&
                          !n->timed.armed && n->core->device >= 0 &&
                          n->host_bound.count(output_id) && !n->bcast_out.count(output_id);
  if (host_bound && !host_src && !gather && plan->prefix.empty() &&
      plan->size <= kHostPackMax) {
    // (a gather plan, or one with a host prefix, takes the HBM slot, which such receivers stage
    // as usual)
    s = host_bound_sample(n, plan->size, plan->size);
  } else if (host_bound && host_src && plan->size >= kZeroCopyThreshold) {
    // a host source for them: the CPU copies it into shared memory, as a node without a GPU
    // does (the reference's copy_array_into_sample) — no HBM slot for each receiver to copy out
    handle_finished_drop_tokens(n);
    Slot* slot = nullptr;
    if (allocate_host_slot(n, plan->size, &slot) == DORA_OK) {
      s = new dora_sample();
      s->len = plan->size;
      s->slot = slot;
      ++n->host_copies;
    } else {
      clear_error();
    }
  }
  int rc = s ? DORA_OK
             : alloc_sample(n, plan->size, &s, plan->fill_size(), host_src, plan_workspace(*plan));
  if (rc != DORA_OK) return rc;
  const uint64_t t1 = mono_ns();
  uint64_t t2 = t1, t3 = t1;
  if (plan->size && (!s->slot || (s->slot->host && (host_src || !s->slot->registered)))) {
    // an inline Vec or a host-only node's shared-memory slot: the host copies the buffers
    // (copy_array_into_sample, arrow_utils.rs:48)
    if (!host_src) {
      discard_sample(n, s);
      return fail(DORA_ERR_INVALID, "host-only node cannot send device-resident data");
    }
    uint8_t* dst = s->slot ? static_cast<uint8_t*>(s->slot->ptr) : s->vec.data();
    for (const Segment& g : plan->segs) std::memcpy(dst + g.dst_off, g.src, g.len);
    t2 = t3 = mono_ns();
  } else if (plan->size && host_src && plan->dev == ARROW_DEVICE_CPU &&
             host_bar_fill(n, s, plan->segs)) {
    t2 = t3 = mono_ns();
  } else if (plan->size) {
    // Kernel stamps cost host time and a timestamp packet on each side of the dispatch, so only
    // every n-th pack is stamped (dora_node_set_timing_period, default kTimingPeriod).
    const uint64_t period = n->prof.timing_period ? n->prof.timing_period : kTimingPeriod;
    const bool timed = n->prof.profile && plan->dev != ARROW_DEVICE_CPU &&
                       (n->prof.timing_seq++ % period) == 0;
    TimingPair* tp = timed ? n->prof.next_pair(plan->size) : nullptr;
    hipEvent_t t_start = tp ? tp->start : nullptr, t_stop = tp ? tp->stop : nullptr;
    // Timed region: packs that signal their own fill stamp their device time into the flag
    // line; only packs that cannot (kernel signal off, transforms) need timing events
    // (nor can a gather: the stream raises its flag)
    const bool stampable = n->core->fill_done && !plan->compact && !gather;
    if (n->timed.armed && plan->dev != ARROW_DEVICE_CPU) {
      if (!stampable && !n->timed.started && !tp) {  // its start is the fallback's origin
        t_start = n->timed.start;
        n->timed.started = true;
      }
      ++n->timed.packs;
      n->timed.bytes += plan->size;
    }
    // a broadcast-group output packs on its own stream, where its broadcast follows
    auto bo = n->bcast_out.find(output_id);
    const bool bcast = bo != n->bcast_out.end();
    if (bcast) n->core->order_after_node_stream(bo->second.stream);
    const bool sync = plan->dev == ARROW_DEVICE_ROCM &&
                      !((flags & DORA_SEND_ASYNC) || n->async_default);
    hipStream_t st = bcast ? bo->second.stream : nullptr;
    rc = DORA_OK;
    if (!plan->prefix.empty()) {
      // a ragged batch's host offsets beside device values: copied on the stream the pack or
      // gather then takes (a given stream keeps the pack off the AQL queue), so the fill signal
      // that follows covers them
      DeviceScope ds(n->core->device);
      if (!st) st = n->core->next_fill_stream();
      rc = launch_plan_prefix(*plan, static_cast<uint8_t*>(s->slot->ptr), st);
    }
    if (rc == DORA_OK)
      rc = gather
               ? gather_sample(n, s, *plan, st, t_start, t_stop, !bcast)
               : fill_sample(n, s, plan->segs.data(), plan->segs.size(), plan->dev, st, t_start,
                             t_stop, !bcast, sync);
    if (rc != DORA_OK) {
      if (tp) tp->pending = false;
      add_to_cache(n, s->slot);
      delete s;
      return rc;
    }
    if (n->timed.armed && plan->dev != ARROW_DEVICE_CPU) {
      if (s->stamped) s->slot->region_epoch = s->epoch;
      else ++n->timed.unstamped;
    }
    if (s->slot->host) {
      // packed into shared memory: its receivers read it on the host when it arrives (the
      // reference's SharedMemory sample is complete when sent), so the pack completes first
      SourceWait w;
      w.kind = s->fill;
      w.epoch = s->epoch;
      if (s->fill == FILL_FLAG) w.flag = n->core->flag_host(s->slot->flag);
      rc = wait_source_read(n, w);
      if (rc != DORA_OK) {
        delete s;  // a pack that may still write the region: its slot is not reused
        return rc;
      }
      s->fill = FILL_DONE;
      ++n->host_packs;
    }
    t2 = t3 = mono_ns();
  }
  SubSpan sp_ti(SP_SEND_TI);
  if (!ti_pre) {
    n->ti_buf.clear();
    serialize_type_info(plan->root, n->ti_buf);
  }
  const std::vector<uint8_t>& ti = ti_pre ? *ti_pre : n->ti_buf;
  sp_ti.stop();
  DropToken tok{};
  const bool traced = trace_enabled() && s->slot;
  SourceWait wait;
  const bool sync_src = plan->dev == ARROW_DEVICE_ROCM && s->slot && plan->size &&
                        !((flags & DORA_SEND_ASYNC) || n->async_default);
  if (sync_src) {
    auto bo = n->bcast_out.find(output_id);
    wait.kind = bo != n->bcast_out.end() ? uint8_t(FILL_BCAST) : s->fill;
    if (bo != n->bcast_out.end()) wait.stream = bo->second.stream;
    wait.epoch = s->epoch;
    wait.read = s->read_signalled;
    if (s->fill == FILL_FLAG) wait.flag = n->core->flag_host(s->slot->flag);
    if (s->fill == FILL_EVENT) wait.event = s->slot->done;
  }
  rc = send_sample(n, output_id, ti, params, params_len, s, &tok);
  if (rc == DORA_OK && sync_src) rc = wait_source_read(n, wait);
  const uint64_t t4 = mono_ns();
  if (traced && rc == DORA_OK) {
    const uint64_t off = now_ns() - mono_ns();  // mono -> realtime for the trace
    trace_at(TP_ALLOC_BEGIN, tok, t0 + off);
    trace_at(TP_ALLOC_END, tok, t1 + off);
    trace_at(TP_LAUNCHED, tok, t2 + off);
    trace_at(TP_FILL_ORDERED, tok, t3 + off);
  }
  n->prof.phase_ns[0] += t1 - t0;
  n->prof.phase_ns[1] += t2 - t1;
  n->prof.phase_ns[2] += t3 - t2;
  n->prof.phase_ns[3] += t4 - t3;
  ++n->prof.phase_count;
  return rc;
}

// Every tensor send (dora_node_send_output_tensor*): the plan `build` makes, its time counted as
// SP_SEND_PLAN, owned for the length of the send and sent like any other plan (what each builder
// turns its arguments into: plan.h).
template <class Build>
int send_plan(dora_node* n, const char* output_id, const uint8_t* params, size_t params_len,
              uint32_t flags, Build build) {
  DORA_GUARD_BEGIN
  dora_plan* plan = nullptr;
  {
    SubSpan sp(SP_SEND_PLAN);
    const int rc = build(&plan);
    if (rc != DORA_OK) return rc;
  }
  std::unique_ptr<dora_plan> owner(plan);
  return pack_and_send(n, output_id, plan, params, params_len, nullptr, flags);
  DORA_GUARD_END
}

}  // namespace

PlanCache::Entry* PlanCache::find(const ArrowArray* array, const ArrowSchema* schema,
                                  bool* cacheable) {
  *cacheable = plan_key(array, schema, key_buf);
  if (!*cacheable) return nullptr;
  auto it = index.find(hash(key_buf));
  if (it == index.end()) return nullptr;
  Entry& e = entries[it->second];
  if (e.key == key_buf) {
    e.last_use = ++clock;
    ++hits;
    return &e;
  }
  *cacheable = false;  // a hash collision: plan this one afresh, uncached
  return nullptr;
}

PlanCache::Entry* PlanCache::insert(dora_plan* plan) {
  // 64 entries cover a sender rotating over a few dozen preallocated arrays (C3 bench: 24)
  constexpr size_t kPlanCache = 64;
  size_t slot = entries.size();
  if (slot >= kPlanCache) {
    slot = 0;
    for (size_t k = 1; k < entries.size(); ++k)
      if (entries[k].last_use < entries[slot].last_use) slot = k;
    index.erase(hash(entries[slot].key));
    delete entries[slot].plan;
    entries[slot] = Entry();
  } else {
    entries.emplace_back();
  }
  Entry& e = entries[slot];
  e.key = key_buf;
  e.plan = plan;
  serialize_type_info(plan->root, e.ti);
  e.last_use = ++clock;
  index[hash(e.key)] = slot;
  return &e;
}

// An inline Vec sample holding `len` host bytes: a remote node's small message, delivered as the
// reference's receiving daemon delivers remote data (`data.map(DataMessage::Vec)`,
// binaries/daemon/src/lib.rs:567), with no slot and no upload.
dora_sample* vec_sample(const uint8_t* p, size_t len) {
  auto* s = new dora_sample();
  s->len = len;
  s->vec.assign(p, p + len);
  return s;
}

// A remote node's message re-sent by its proxy (interdaemon.cpp): the metadata keeps the
// producer's timestamp.
int proxy_send(dora_node* n, const char* output_id, const uint8_t* ti, size_t ti_len,
               const uint8_t* params, size_t params_len, dora_sample* sample, uint64_t ts) {
  DORA_GUARD_BEGIN
  n->samples_live.erase(sample);  // consumed here (an allocate_data_sample sample or inline)
  std::vector<uint8_t> t(ti, ti + ti_len);
  return send_sample(n, output_id, t, params, params_len, sample, nullptr, ts);
  DORA_GUARD_END
}

}  // namespace dora

extern "C" {

int dora_node_allocate_data_sample(dora_node* n, size_t len, dora_sample** out) {
  if (!n || !out) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  DORA_GUARD_BEGIN
  const int rc = dora::alloc_sample(n, len, out);
  if (rc == DORA_OK) n->samples_live.insert(*out);
  return rc;
  DORA_GUARD_END
}

void* dora_sample_data(dora_sample* s) {
  if (!s) return nullptr;
  return s->slot ? s->slot->ptr : s->vec.data();
}

size_t dora_sample_len(const dora_sample* s) { return s ? s->len : 0; }

void dora_sample_discard(dora_node* n, dora_sample* s) {
  if (!s || !n) return;
  // only a sample this node handed out and nobody consumed yet (a second discard, or a discard
  // after the send, would free it twice)
  if (!n->samples_live.erase(s)) {
    dora::fail(DORA_ERR_INVALID, "sample was already sent or discarded");
    return;
  }
  dora::discard_sample(n, s);
}

int dora_node_send_output_sample(dora_node* n, const char* output_id, const uint8_t* type_info,
                                 size_t type_info_len, const uint8_t* params, size_t params_len,
                                 dora_sample* sample) {
  if (!n || !output_id || (!type_info && type_info_len))
    return dora::fail(DORA_ERR_INVALID, "NULL argument");
  // the reference's DataSample is moved into send_output_sample (mod.rs:246-275): a C caller
  // may hold on to the pointer, so a sample that was already sent or discarded is refused
  if (sample && !n->samples_live.erase(sample))
    return dora::fail(DORA_ERR_INVALID,
                      "sample was already sent or discarded (or belongs to another node)");
  DORA_GUARD_BEGIN
  if (sample && sample->self_published) {
    // the caller's kernel raises the slot's fill flag itself (dora_sample_fill_ticket made the
    // sample a flag fill): no stream operation, on whichever stream the kernel runs
    ++n->samples_self_published;
    if (n->bcast_out.count(output_id)) {
      // a broadcast-group output reads the slot on its own stream, which nothing orders after
      // the caller's kernel: wait for the flag here
      if (!dora::wait_fill(n->core->flag_host(sample->slot->flag), sample->epoch,
                           dora::mono_ns() + dora::kFillWaitNs)) {
        dora::discard_sample(n, sample);
        return dora::fail(DORA_ERR_TIMEOUT, "the sample's kernel did not publish it within 10 s");
      }
    }
  } else if (sample && sample->slot && !sample->slot->host && sample->len &&
      n->core->stream_used.load(std::memory_order_relaxed)) {
    // a sample written by kernels on the node stream (dora_node_stream): receivers wait for
    // that work through the slot's fill flag, the sender does not (no host synchronisation)
    dora::DeviceScope ds(n->core->device);
    const hipError_t e = dora::order_fill(n, sample, n->core->stream);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      dora::discard_sample(n, sample);
      return dora::fail(DORA_ERR_HIP, "ordering the sample after the node stream: %s",
                        hipGetErrorString(e));
    }
    ++n->samples_stream_ordered;
  }
  std::vector<uint8_t> ti(type_info, type_info + type_info_len);
  return dora::send_sample(n, output_id, ti, params, params_len, sample);
  DORA_GUARD_END
}

int dora_sample_fill_ticket(dora_node* n, dora_sample* s, uint32_t workgroups, uint32_t mode,
                            dora_fill_ticket* out) {
  if (!n || !s || !out) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  DORA_GUARD_BEGIN
  if (!n->samples_live.count(s))
    return dora::fail(DORA_ERR_INVALID,
                      "fill ticket: the sample is not live on this node (already sent or "
                      "discarded, or another node's)");
  if (workgroups == 0 || workgroups > dora::kMaxSignalWgs)
    return dora::fail(DORA_ERR_INVALID, "fill ticket: %u workgroups (1..%u: a fill flag owns %u "
                      "done words)", workgroups, dora::kMaxSignalWgs, dora::kMaxSignalWgs);
  if (mode != DORA_FILL_WRITE_THROUGH && mode != DORA_FILL_PLAIN)
    return dora::fail(DORA_ERR_INVALID, "fill ticket: unknown mode %u", mode);
  if (s->self_published)
    return dora::fail(DORA_ERR_INVALID, "fill ticket: the sample already has a ticket");
  if (!s->slot)
    return dora::fail(DORA_ERR_UNSUPPORTED,
                      "fill ticket: an inline sample (no device slot: below 4096 B on a node "
                      "without a GPU, or empty) is written by the host");
  if (s->slot->host)
    return dora::fail(DORA_ERR_UNSUPPORTED,
                      "fill ticket: a shared-memory sample is written by the host");
  dora::NodeCore* c = n->core.get();
  if (c->device < 0) return dora::fail(DORA_ERR_UNSUPPORTED, "fill ticket: the node has no GPU");
  if (s->slot->flag < 0 || !c->region_dev)
    return dora::fail(DORA_ERR_UNSUPPORTED,
                      "fill ticket: the sample's slot has no fill flag (send it stream-ordered)");
  if (!c->fill_done)
    return dora::fail(DORA_ERR_UNSUPPORTED,
                      "fill ticket: the node has no done words (send the sample stream-ordered)");
  // the caller's kernel raises the flag where order_fill's stream write would
  dora::mark_flag_fill(c, s, ++c->epoch, dora::NOTE_SYNC);
  s->self_published = true;
  out->flag = reinterpret_cast<uint64_t>(c->flag_dev(s->slot->flag));
  out->done = reinterpret_cast<uint64_t>(c->fill_done + size_t(s->slot->flag) * dora::kMaxSignalWgs);
  out->epoch = s->epoch;
  out->workgroups = workgroups;
  out->mode = mode;
  return DORA_OK;
  DORA_GUARD_END
}

int dora_node_send_output(dora_node* n, const char* output_id, const struct ArrowArray* array,
                          const struct ArrowSchema* schema, ArrowDeviceType device_type,
                          const uint8_t* params, size_t params_len) {
  return dora_node_send_output_ex(n, output_id, array, schema, device_type, params, params_len, 0);
}

int dora_node_send_output_ex(dora_node* n, const char* output_id, const struct ArrowArray* array,
                             const struct ArrowSchema* schema, ArrowDeviceType device_type,
                             const uint8_t* params, size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  DORA_GUARD_BEGIN
  const bool device = device_type == ARROW_DEVICE_ROCM && n->core->device >= 0;
  bool cacheable = false;
  if (device && !n->compact && array && schema)
    if (auto* e = n->plans.find(array, schema, &cacheable))
      return dora::pack_and_send(n, output_id, e->plan, params, params_len, &e->ti, flags);
  dora_plan* plan = nullptr;
  int rc = (n->compact && device_type == ARROW_DEVICE_ROCM)
               ? dora::build_plan_compact(array, schema, device_type, &plan)
               : dora::build_plan(array, schema, device_type, &plan,
                                  device);
  if (rc != DORA_OK) return rc;
  if (cacheable && !plan->read_device) {
    // keep it: a later send of the same buffers reuses plan and type info
    auto* e = n->plans.insert(plan);
    return dora::pack_and_send(n, output_id, e->plan, params, params_len, &e->ti, flags);
  }
  rc = dora::pack_and_send(n, output_id, plan, params, params_len, nullptr, flags);
  delete plan;
  return rc;
  DORA_GUARD_END
}

int dora_node_send_output_bytes_ex(dora_node* n, const char* output_id, const void* data,
                                   size_t len, ArrowDeviceType device_type, const uint8_t* params,
                                   size_t params_len, uint32_t flags) {
  if (!n || !output_id || (!data && len)) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  DORA_GUARD_BEGIN
  dora::SubSpan sp(dora::SP_SEND_PLAN);
  // one UInt8 buffer: the plan and its type info are built once per node and re-pointed per send
  dora_plan& plan = n->bytes_plan;
  if (n->bytes_ti.empty()) {
    ArrowSchema u8{};
    u8.format = "C";
    dora::serialize_schema(&u8, true, plan.root.schema);
    plan.root.bufs.assign(1, {0, 0});
  }
  plan.dev = device_type;
  plan.size = len;
  plan.root.len = len;
  plan.root.bufs[0] = {0, len};
  plan.segs.clear();
  if (len) plan.segs.push_back({data, 0, len});
  // the type info depends on len only through the buffer length: re-serialize when it changes
  if (n->bytes_ti.empty() || n->bytes_ti_len != len) {
    n->bytes_ti.clear();
    dora::serialize_type_info(plan.root, n->bytes_ti);
    n->bytes_ti_len = len;
  }
  sp.stop();
  return dora::pack_and_send(n, output_id, &plan, params, params_len, &n->bytes_ti, flags);
  DORA_GUARD_END
}

int dora_node_send_output_tensor(dora_node* n, const char* output_id, const dora_tensor* tensor,
                                 ArrowDeviceType device_type, const uint8_t* params,
                                 size_t params_len, uint32_t flags) {
  if (!n || !output_id || !tensor) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_plan(tensor, device_type, plan);
  });
}

int dora_node_send_output_tensor_struct(dora_node* n, const char* output_id,
                                        const dora_tensor_field* fields, size_t count,
                                        ArrowDeviceType device_type, const uint8_t* params,
                                        size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_struct_plan(fields, count, device_type, plan);
  });
}

int dora_node_send_output_tensor_cast(dora_node* n, const char* output_id,
                                      const dora_tensor_field* fields, size_t count,
                                      const dora_tensor_cast* casts, ArrowDeviceType device_type,
                                      const uint8_t* params, size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_cast_plan(fields, count, casts, device_type, plan);
  });
}

int dora_node_send_output_tensor_convert(dora_node* n, const char* output_id,
                                         const dora_tensor_field* fields, size_t count,
                                         const dora_tensor_cast* casts,
                                         const dora_tensor_quant* quants,
                                         ArrowDeviceType device_type, const uint8_t* params,
                                         size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_convert_plan(fields, count, casts, quants, device_type, plan);
  });
}

int dora_node_send_output_tensor_affine(dora_node* n, const char* output_id,
                                        const dora_tensor_field* fields, size_t count,
                                        const dora_tensor_cast* casts,
                                        const dora_tensor_quant* quants,
                                        const dora_tensor_affine* affines,
                                        ArrowDeviceType device_type, const uint8_t* params,
                                        size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_affine_plan(fields, count, casts, quants, affines, device_type,
                                          plan);
  });
}

int dora_node_send_output_tensor_reduce(dora_node* n, const char* output_id,
                                        const dora_tensor_field* fields, size_t count,
                                        const dora_tensor_reduce* reduces,
                                        ArrowDeviceType device_type, const uint8_t* params,
                                        size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_reduce_plan(fields, count, reduces, device_type, plan);
  });
}

int dora_node_send_output_tensor_resize(dora_node* n, const char* output_id,
                                        const dora_tensor_field* fields, size_t count,
                                        const dora_tensor_resize* resizes,
                                        ArrowDeviceType device_type, const uint8_t* params,
                                        size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_resize_plan(fields, count, resizes, device_type, plan);
  });
}

int dora_node_send_output_tensor_crop(dora_node* n, const char* output_id,
                                      const dora_tensor_field* fields, size_t count,
                                      const dora_tensor_crop* crops, ArrowDeviceType device_type,
                                      const uint8_t* params, size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_crop_plan(fields, count, crops, device_type, plan);
  });
}

int dora_node_send_output_tensor_prep(dora_node* n, const char* output_id,
                                      const dora_tensor_field* fields, size_t count,
                                      const dora_tensor_resize* resizes,
                                      const dora_tensor_crop* crops, const dora_tensor_prep* preps,
                                      ArrowDeviceType device_type, const uint8_t* params,
                                      size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_prep_plan(fields, count, resizes, crops, preps, device_type, plan);
  });
}

int dora_node_send_output_tensor_list(dora_node* n, const char* output_id,
                                      const dora_tensor_list* list, ArrowDeviceType device_type,
                                      const uint8_t* params, size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_list_plan(list, device_type, plan);
  });
}

int dora_node_send_output_tensor_take(dora_node* n, const char* output_id,
                                      const dora_tensor_take* take, ArrowDeviceType device_type,
                                      const uint8_t* params, size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_take_plan(take, device_type, plan);
  });
}

int dora_node_send_output_tensor_mask(dora_node* n, const char* output_id,
                                      const dora_tensor_mask* mask, ArrowDeviceType device_type,
                                      const uint8_t* params, size_t params_len, uint32_t flags) {
  if (!n || !output_id) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  return dora::send_plan(n, output_id, params, params_len, flags, [&](dora_plan** plan) {
    return dora::build_tensor_mask_plan(mask, device_type, plan);
  });
}

int dora_node_send_output_bytes(dora_node* n, const char* output_id, const void* data, size_t len,
                                ArrowDeviceType device_type, const uint8_t* params,
                                size_t params_len) {
  return dora_node_send_output_bytes_ex(n, output_id, data, len, device_type, params, params_len,
                                        0);
}

int dora_node_set_async_sends(dora_node* n, int enable) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  n->async_default = enable != 0;
  return DORA_OK;
}

int dora_node_set_compact(dora_node* n, int enable) {
  if (!n) return dora::fail(DORA_ERR_INVALID, "NULL node");
  n->compact = enable != 0;
  return DORA_OK;
}

int dora_node_close_outputs(dora_node* n, const char* const* ids, size_t count) {
  if (!n || (!ids && count)) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  DORA_GUARD_BEGIN
  for (size_t i = 0; i < count; ++i)
    if (!n->outputs.count(ids[i])) return dora::fail(DORA_ERR_NOT_FOUND, "unknown output %s", ids[i]);
  dora::WBuf w;
  w.u32(static_cast<uint32_t>(count));
  for (size_t i = 0; i < count; ++i) {
    n->outputs.erase(ids[i]);
    w.str(ids[i]);
  }
  return n->core->request(dora::REQ_CLOSE_OUTPUTS, w.data(), w.size());
  DORA_GUARD_END
}

int dora_node_forward(dora_node* n, const char* output_id, const dora_event* ev,
                      const uint8_t* params, size_t params_len) {
  if (!n || !output_id || !ev) return dora::fail(DORA_ERR_INVALID, "NULL argument");
  if (ev->type != DORA_EVENT_INPUT || !ev->data)
    return dora::fail(DORA_ERR_INVALID, "only input events can be forwarded");
  if (!ev->data->ptr && ev->data->len)
    return dora::fail(DORA_ERR_INVALID, "input data is not mapped: %s", ev->error.c_str());
  dora::DeviceScope ds(n->core->device);
  DORA_GUARD_BEGIN
  return dora::forward_input(n, output_id, ev, params, params_len);
  DORA_GUARD_END
}

}  // extern "C"
