/*
 * dora_gpu_testing.h — test and microbenchmark hooks of the device data plane, exported by
 * libdora_gpu_testing.so (dora_amd/csrc/testing/testing.cpp), which is built apart from the
 * shipped libdora_gpu.so and links against it.  The pack-tuning knobs of r01-r05 (variants,
 * grids, in-flight caps, queue counts) are gone with their variants (r06): the product carries no
 * code path only a microbenchmark selects.  No reference counterpart: tests/ and scripts/
 * use these to reach internals (the AQL backlog, the BAR, the fill-flag protocol, the RCCL group
 * path, the inter-daemon codec) that the product ABI (dora_gpu.h) does not expose.
 */
#ifndef DORA_GPU_TESTING_H
#define DORA_GPU_TESTING_H

#include "dora_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test tool (no reference counterpart): one workgroup per CU reads all of [data, data + len)
 * with plain cached loads, leaving the lines in every XCD's L2 (the acquire-fence negative
 * control of tests/test_gpu_fence.py). */
int dora_gpu_test_l2_touch(const void* data, size_t len, dora_stream_t stream);
/* Test tools (no reference counterpart): device memory of `device`'s coarse-grained pool that
 * the host writes directly through the PCIe BAR (stores + HDP flush + read-back), behind every
 * XCD's L2 — the source rewrite of the acquire-fence negative control. */
int dora_gpu_test_bar_alloc(int device, size_t bytes, void** out);
/* Test tool: while `hold` is set, every batchable AQL send of this process on `device` waits in
 * the backlog; clearing it dispatches the backlog as batch packs.  Only for asynchronous sends
 * (DORA_SEND_ASYNC): a synchronous send waits for its own pack. */
int dora_gpu_test_aql_hold(int device, int hold);
/* Test hooks of the region-end stamp reduction (aql_stamp_reduce): how long it is waited for
 * (ns; 0 = the default 5 s) — a tiny value makes the wait time out while the packet still runs —
 * and the AQL argument slots left to reductions that timed out (never written again). */
int dora_gpu_test_reduce_timeout(uint64_t ns);
/* Experiment: `n` D2H copies of `bytes` from HBM into pinned host memory, `gap_ns` apart, each
 * timed call -> complete into out_ns[n]: mode 0 hipMemcpyAsync + hipStreamSynchronize on a
 * stream of its own, mode 1 hsa_amd_memory_async_copy + a busy wait on its signal. */
int dora_gpu_test_d2h_copy_probe(int device, int mode, uint64_t bytes, uint32_t n,
                                 uint64_t gap_ns, uint64_t* out_ns);
/* Experiment: per-message cost of ordering a sample written on a stream — `n` kernels writing
 * `bytes`, each followed by nothing (mode 0), hipStreamWriteValue64 into pinned host memory (1)
 * or an 8-byte kernel (2); out_ns[0] host enqueue, out_ns[1] enqueue + drain, ns per message. */
int dora_gpu_test_stream_order_probe(int device, int mode, uint64_t bytes, uint32_t n,
                                     uint64_t* out_ns);
int dora_gpu_test_abandoned_slots(int device, uint32_t* slots);
/* Test hook of the self-published sample path (include/dora_gpu_device.h): as
 * dora_gpu_fill_splitmix_ticket, with `threads_per_wg` threads per workgroup (a multiple of 64 up
 * to 1024) and, with `store_mode` 1, ordinary stores (the ticket must then be DORA_FILL_PLAIN);
 * 0 stores write-through.  One launch of the ticket's workgroup count on `stream`. */
int dora_gpu_test_publish_kernel(void* dst, size_t len, uint64_t seed,
                                 const dora_fill_ticket* ticket, uint32_t threads_per_wg,
                                 uint32_t store_mode, dora_stream_t stream);
/* Test tool: empty packets the keep-awake thread of `device` has published in this process
 * (dora_gpu_set_keep_awake), and whether it is parked (no send for 100 ms). */
int dora_gpu_test_keep_awake_stats(int device, uint64_t* heartbeats, int* parked);
/* Test tool: `wc` 1 if `device`'s AQL packet rings are published with store fences (the runtime
 * put them in this GPU's memory), 0 otherwise; `where` (may be NULL): the runtime's pointer type
 * of the ring * 4 + its owner (0 none, 1 the CPU agent, 2 this GPU, 3 another agent). */
int dora_gpu_test_aql_ring_wc(int device, int* wc, int* where);
/* Test tool (host only): the 640-byte argument block of a batch pack (dora_aql_packb_u4) for
 * `n_msgs` (<= 8) messages; message m has seg_counts[m] segments, given as (src, dst_off, len)
 * triples in `segs`, its slot at dsts[m] with dst_caps[m] writable bytes, and fill flag /
 * epoch flags[m] / epochs[m].  *grid = the workgroups the dispatch would launch. */
int dora_gpu_test_batch_args(size_t n_msgs, const size_t* seg_counts, const uint64_t* segs,
                             const uint64_t* dsts, const uint64_t* dst_caps,
                             const uint64_t* flags, const uint64_t* epochs, uint8_t* out,
                             size_t cap, uint32_t* grid);
/* Test hook of the pack bodies (dora_amd/csrc/pack_device.h): one pack of caller-given segments
 * through body `body`, then a synchronise of `stream`.  Messages as dora_gpu_test_batch_args gives
 * them: message m has seg_counts[m] segments, (src, dst_off, len) triples in `segs`, sorted and
 * disjoint, its destination at dsts[m] with dst_caps[m] writable bytes (0: unknown).  Bodies:
 * 0 the product's launch_pack, unsignalled (any segment count: launches of 32, none stitched
 * when there is more than one); 1 pack_body<4, 2> over PackArgs (<= 32 segments, write-through
 * stores); 2 pack_body<4, kCoherent> over AqlPackArgs (<= 8 segments); 3 pack_body<4, 2> over the
 * AqlBatchArgs that build_aql_batch_args makes of 1-8 messages (<= 16 segments), each with its
 * own flag and epoch.  Bodies 0-2 take one message.  Bodies 1-3 fill their arguments with the
 * product's finish_args / edge_mask / chunk_layout and signal pinned host flags and done words
 * of the hook's own; *flags_ok (may be NULL) gets bit m set if message m's flag holds exactly its
 * epoch after the synchronise.  `chunk_bytes` 0: the product's choice, else a multiple of 8192 up
 * to 4 MiB (what choose_chunk_bytes can return); `grid` 0: the product's choice, else a value in
 * [1, n_chunks]; body 0 takes neither.  Every source and destination range is checked against the
 * device allocation that holds it before anything is launched.  The kernels are compiled from
 * the same header as the AQL code object but without its kernarg-preload flag. */
int dora_gpu_test_pack_segments(int body, size_t n_msgs, const size_t* seg_counts,
                                const uint64_t* segs, const uint64_t* dsts,
                                const uint64_t* dst_caps, uint32_t chunk_bytes, uint32_t grid,
                                dora_stream_t stream, uint32_t* flags_ok);
/* Test tool (host only): the argument block dora_gpu_test_pack_segments would launch with, nothing
 * launched: PackArgs (bodies 0 and 1; of body 0 the first launch), AqlPackArgs (2) or AqlBatchArgs
 * (3), its size in *out_len.  The flags are placeholders. */
int dora_gpu_test_pack_args(int body, size_t n_msgs, const size_t* seg_counts,
                            const uint64_t* segs, const uint64_t* dsts, const uint64_t* dst_caps,
                            uint32_t chunk_bytes, uint32_t grid, uint8_t* out, size_t cap,
                            size_t* out_len);
/* Test tool (host only): what a device tensor plan (dora_gpu_plan_tensor with ARROW_DEVICE_ROCM)
 * reads.  *gather 1 if a gather kernel reads it (the plan then has no segments), 0 if it is
 * dense; *src element (0, .., 0); the canonical view as *nd (<= 8) extents and byte strides in
 * shape[8] / stride[8], each addressing *row contiguous bytes of *elem-byte elements; [*lo, *hi]
 * the closed interval of byte offsets from *src the view reaches.  DORA_ERR_INVALID for any
 * other plan. */
int dora_gpu_test_plan_gather(const dora_plan* plan, int* gather, const void** src, int* nd,
                              uint64_t* row, uint32_t* elem, int64_t* shape, int64_t* stride,
                              int64_t* lo, int64_t* hi);
/* Test tool (host only): field `i` of a device struct-of-tensors plan
 * (dora_gpu_plan_tensor_struct with ARROW_DEVICE_ROCM, d0 > 0).  *n_fields the plan's field count,
 * *gather 1 if gather_struct_kernel reads the fields (no segments), 0 if all are dense;
 * *dst_off / *bytes the field's byte range in the sample; *kind which body gathers it into a
 * sample at address `dst` under the current selection (dora_gpu_test_gather_kernel): -1 the rows
 * body, else the dimension of the view the tile body transposes against; the view, element size
 * and reach as dora_gpu_test_plan_gather gives them (nd == 0: dense).  DORA_ERR_INVALID for any
 * other plan or index. */
int dora_gpu_test_plan_field(const dora_plan* plan, size_t i, const void* dst, size_t* n_fields,
                             int* gather, uint64_t* dst_off, uint64_t* bytes, int* kind,
                             const void** src, int* nd, uint64_t* row, uint32_t* elem,
                             int64_t* shape, int64_t* stride, int64_t* lo, int64_t* hi);
/* Test tool (host only): how a ragged-batch plan (dora_gpu_plan_tensor_list) gets its offsets.
 * *scan 1 if the plan's launch scans a partition in HBM: then *src its words, *count how many,
 * *wide 1 for int64, *offsets_form 1 for offsets, *rows the clamp N, [*lo, *hi] the bytes from
 * *src that are checked against the allocation.  *scan 0: *prefix_bytes the length of the host
 * offsets copied ahead of a device plan's pack or gather (0: they are segment 0 of a host plan).
 * DORA_ERR_INVALID for any other plan. */
int dora_gpu_test_plan_list(const dora_plan* plan, int* scan, const void** src, uint64_t* count,
                            int* wide, int* offsets_form, uint64_t* rows, int64_t* lo, int64_t* hi,
                            uint64_t* prefix_bytes);
/* Test tool (host only): whether `plan` is a take (dora_gpu_plan_tensor_take; DORA_ERR_INVALID for
 * any other plan) and what it takes by.  *k the rows taken, *n the rows of the source, *wide 1 for
 * int64 words.  *device 1 if the plan's launch reads the index in HBM: then *index its words,
 * [*lo, *hi] the bytes from *index that are checked against the allocation, and stride0[8] the
 * byte stride of dimension 0 of every field, whose dimensions 1.. dora_gpu_test_plan_field
 * reports (its reach over all *n source rows, *kind always -1 under the taken body).  *device 0: a
 * host plan, the taken rows already in its staging buffer (or an empty message). */
int dora_gpu_test_plan_take(const dora_plan* plan, int* device, const void** index, uint64_t* k,
                            uint64_t* n, int* wide, int64_t* lo, int64_t* hi, int64_t* stride0);
/* Test tool (host only): field `i` of a device plan of dora_gpu_plan_tensor_cast (or of any device
 * plan that keeps its fields).  *is_cast 1 when gather_cast_kernel converts the field: then
 * *src_code / *src_bits the source dtype (DLPack), *dst_code / *dst_bits the destination's,
 * *has_scale and *scale the factor.  A field sent as it is reports codes of -1 and its element
 * width twice.  *elements the field's element count, *src_bytes the bytes of its source view,
 * *dst_bytes those it has in the sample.  dora_gpu_test_plan_field keeps reporting view and reach
 * (of a cast field: in source bytes). */
int dora_gpu_test_plan_cast(const dora_plan* plan, size_t i, size_t* n_fields, int* is_cast,
                            int* src_code, int* src_bits, int* dst_code, int* dst_bits,
                            int* has_scale, float* scale, uint64_t* elements,
                            uint64_t* src_bytes, uint64_t* dst_bytes);
/* Test tool (host only): whether field `i` of a device plan of dora_gpu_plan_tensor_convert is
 * quantised (*is_quant 1): then *dst_code / *dst_bits the integer destination (DLPack) and
 * *zero_point; else -1, 0 and 0.  dora_gpu_test_plan_cast reports the rest of such a field as it
 * does of a cast one — source dtype, scale, element and byte counts, *dst_bits — with *is_cast 1
 * and *dst_code 2 as for every converted field. */
int dora_gpu_test_plan_quant(const dora_plan* plan, size_t i, int* is_quant, int* dst_code,
                             int* dst_bits, int* zero_point);
/* Test tool (host only): whether field `i` of a device plan of dora_gpu_plan_tensor_affine has an
 * affine step (*is_affine 1: its launch is gather_affine_kernel): then *scale_table / *bias_table
 * the tables in HBM (NULL: none), *inner and *channels the geometry of the axis they run along and
 * [*lo, *hi] the bytes from either table that are checked against its allocation (0, 0, 0, -1
 * without a table), *has_bias and *bias the scalar bias.  dora_gpu_test_plan_cast and
 * dora_gpu_test_plan_quant report the rest of the field. */
int dora_gpu_test_plan_affine(const dora_plan* plan, size_t i, int* is_affine,
                              const void** scale_table, const void** bias_table, uint64_t* inner,
                              uint64_t* channels, int* has_bias, float* bias, int64_t* lo,
                              int64_t* hi);
/* Test tool (host only): whether field `i` of a device plan of dora_gpu_plan_tensor_reduce is
 * reduced (*op DORA_REDUCE_ARGMAX; 0 for a field sent as it is and for any other device plan that
 * keeps its fields): then *c the candidates per output element, *axis_stride the bytes between
 * them, *outputs the output elements, *index_bits the index type's width, and *body which body of
 * gather_reduce_kernel reduces it under the current selection (dora_gpu_test_reduce_body): 1 the
 * lane body, 2 the wave body (0: not reduced).  For the lane body *vector_units and *element_units
 * count the whole 16-byte units of a sample at address `dst` by the load path each takes (0 and 0
 * for the wave body, which has no units).  dora_gpu_test_plan_field keeps reporting the view of
 * the kept dimensions and the reach over all *c steps. */
int dora_gpu_test_plan_reduce(const dora_plan* plan, size_t i, const void* dst, int* op,
                              uint64_t* c, int64_t* axis_stride, uint64_t* outputs,
                              int* index_bits, int* body, uint64_t* vector_units,
                              uint64_t* element_units);
/* Test and probe tool: which body reduces the fields of this process' reduce plans from now on:
 * 0 the library's own selection, 1 the lane body always, 2 the wave body wherever it applies (a
 * source-contiguous reduced axis of at least two candidates). */
int dora_gpu_test_reduce_body(int mode);
/* Test tool (host only): whether field `i` of a device plan of dora_gpu_plan_tensor_resize is
 * resized (*mode DORA_RESIZE_NEAREST or DORA_RESIZE_BILINEAR; 0 for a field sent as it is and for
 * any other device plan that keeps its fields): then *outputs the output elements, *dst_bits the
 * destination's width, in_extent[2], out_extent[2] and axis_stride[2] the source extents, output
 * extents and source byte strides of the two resized axes in the caller's order, and the unit
 * paths the body takes into a sample at address `dst`: *head_elements and *tail_elements the
 * elements written singly before the first and after the last whole 16-byte unit, *units the whole
 * units.  dora_gpu_test_plan_field keeps reporting the view of the whole source and its reach. */
int dora_gpu_test_plan_resize(const dora_plan* plan, size_t i, const void* dst, int* mode,
                              uint64_t* outputs, int* dst_bits, int64_t* in_extent,
                              int64_t* out_extent, int64_t* axis_stride, uint64_t* head_elements,
                              uint64_t* units, uint64_t* tail_elements);
/* Test tool (host only): whether field `i` of a device plan of dora_gpu_plan_tensor_crop is a
 * field of crops (*mode DORA_RESIZE_NEAREST or DORA_RESIZE_BILINEAR; 0 for a field sent as it is
 * and for any other plan that keeps its fields; a host plan keeps none): then *k the K boxes,
 * *boxes their first byte, *boxes_device 1 if the launch reads them in HBM, [*lo, *hi] the bytes
 * from *boxes that are checked against their allocation, and the unit paths the body takes into a
 * sample at address `dst`: *head_elements and *tail_elements the elements written singly before
 * the first and after the last whole 16-byte unit, *units the whole units.
 * dora_gpu_test_plan_field keeps reporting the view of the whole frame and its reach. */
int dora_gpu_test_plan_crop(const dora_plan* plan, size_t i, const void* dst, int* mode,
                            uint64_t* k, const void** boxes, int* boxes_device, int64_t* lo,
                            int64_t* hi, uint64_t* head_elements, uint64_t* units,
                            uint64_t* tail_elements);
/* Test tool (host only): whether field `i` of a device plan of dora_gpu_plan_tensor_prep has a
 * model-input step (*on 1: its launch is gather_resize_prep_kernel or gather_crop_prep_kernel):
 * then *scale_table / *bias_table the tables in HBM (NULL: none), *channels their words and *axis
 * the dimension of the output they run along (a crops field's counted with K in front; 0 and -1
 * without a table), [*lo, *hi] the bytes from either table that are checked against its
 * allocation (0, -1 without one), and inner[2], lead[2] and *fill the placement (all 0: the image
 * fills the output).  dora_gpu_test_plan_resize and dora_gpu_test_plan_crop report the rest. */
int dora_gpu_test_plan_prep(const dora_plan* plan, size_t i, int* on, const void** scale_table,
                            const void** bias_table, uint64_t* channels, int* axis,
                            int64_t* inner, int64_t* lead, float* fill, int64_t* lo, int64_t* hi);
/* Test tool: counts[4], the launches of this process so far over the fields of a plan, by kernel:
 * gather_struct_kernel, gather_cast_kernel, gather_quant_kernel, gather_affine_kernel. */
int dora_gpu_test_fields_launches(uint64_t* counts);
/* Test tool (host only): whether `plan` is a mask plan (dora_gpu_plan_tensor_mask; DORA_ERR_INVALID
 * for any other plan) and what it selects by.  *n the rows of the source.  *device 1 if the plan's
 * launches read the mask in HBM: then *mask its bytes, [*lo, *hi] the bytes from *mask that are
 * checked against the allocation, workspace[5] the offsets from the sample's start of the index
 * words, the counts, the per-tile totals, a host partition's offsets (*part_words of them, 0:
 * none) and the workspace's end — dora_gpu_plan_size + dora_gpu_plan_workspace_size — and
 * stride0[8] the byte stride of dimension 0 of every field, whose dimensions 1..
 * dora_gpu_test_plan_field reports (reach over all *n rows, *kind always -1).  *device 0: a host
 * plan, the compacted rows already in its staging buffer (or a message without rows). */
int dora_gpu_test_plan_mask(const dora_plan* plan, int* device, const void** mask, uint64_t* n,
                            int64_t* lo, int64_t* hi, uint64_t* workspace, uint64_t* part_words,
                            int64_t* stride0);
/* Test tool (host only): what fills the sample of any plan.  *launch 0 its copy segments (every
 * host plan, dense device plans, empty plans), 1 the gather of its one strided view, 2
 * gather_struct_kernel over its fields, 3 gather_cast_kernel / gather_quant_kernel, 4 the taken
 * body by an index in HBM, 5 a mask's count, compact and taken launches, 6 gather_reduce_kernel,
 * 7 gather_resize_kernel, 8 gather_crop_kernel, 9 gather_resize_prep_kernel, 10
 * gather_crop_prep_kernel; *scan 1 if that launch
 * also scans a partition in HBM; *checked 1 if the plan reads HBM whose range is checked before
 * anything is launched. */
int dora_gpu_test_plan_launch(const dora_plan* plan, int* launch, int* scan, int* checked);
/* Test tool (host only): how segment `i` of any plan is moved (dora_gpu_plan_segment gives its
 * source, destination offset and length).  *op 0 a verbatim copy; of a compacting plan
 * (dora_gpu_plan_compact) also 1 a bitmap slice shifted to bit 0, starting *aux bits into the
 * source, of which *src_len bytes are readable; 2 / 3 int32 / int64 offsets minus the first.
 * DORA_ERR_INVALID for an index past the plan's segments. */
int dora_gpu_test_plan_segment_op(const dora_plan* plan, size_t i, uint32_t* op, uint32_t* aux,
                                  uint64_t* src_len);
/* Test and probe tool: which kernel gathers strided device tensor views of this process from now
 * on: 0 the library's own selection, 1 gather_rows_kernel always, 2 gather_tile_kernel wherever
 * it applies (short contiguous extents included). */
int dora_gpu_test_gather_kernel(int mode);
int dora_gpu_test_bar_write(int device, void* dst, const void* src, size_t bytes);
/* Test tools (host only) of the fill-flag protocol (FillFlag, 128 bytes, 64-byte aligned): the
 * completion test of epoch `epoch` (1: complete) and the sender's set-up of a fill the command
 * processor signals. */
int dora_gpu_test_fill_reached(const void* flag, uint64_t epoch);
int dora_gpu_test_cp_arm(void* flag, uint64_t epoch);
void dora_gpu_test_bar_free(void* ptr);
/* Test hook (RCCL path of the fan-out): form a broadcast group of one rank on
 * `device` (unique id -> join(nranks 1) -> ncclBroadcast of `bytes` at `buf` in place on a fresh
 * stream -> close), reporting the rank count and rank the communicator holds.  The one-GPU
 * exercise of bcast_unique_id / bcast_join / bcast_enqueue / bcast_close. */
int dora_gpu_test_bcast_group(int device, void* buf, uint64_t bytes, int* nranks, int* rank);
/* Test tool (the fence probe's failing control): one 64-lane workgroup per CU reads 64 words of
 * BAR-written device memory, the host rewrites them through the BAR, and the same waves read
 * them again within the same dispatch; `mode` 0 plain (L1-cached) loads, 1 non-temporal, 2
 * agent-coherent (sc1).  Workgroups whose first read was wrong, whose second read was stale,
 * and the workgroups launched. */
int dora_gpu_test_l1_stale(int device, int mode, uint32_t* bad_first, uint32_t* stale,
                           uint32_t* blocks);
/* Test hooks of the inter-daemon wire, bincode of Timestamped<InterDaemonEvent> (replaces
 * bincode::serialize in binaries/daemon/src/inter_daemon.rs:66 and its deserialize at :156;
 * layouts in csrc/bincode.h): an Output event built from this library's type-info and parameter
 * encodings, an InputsClosed event of `n` (receiver, input) pairs, and a frame decoded into
 * JSON.  `hlc_id`: 16 bytes.  A buffer too small fails with *len set to the size needed. */
int dora_gpu_test_ide_output(const char* dataflow_id, const char* node_id, const char* output_id,
                             const uint8_t* type_info, size_t type_info_len, const uint8_t* params,
                             size_t params_len, uint64_t meta_ns, uint64_t event_ns,
                             const uint8_t* hlc_id, const uint8_t* data, size_t data_len,
                             int has_data, uint8_t* out, size_t cap, size_t* out_len);
int dora_gpu_test_ide_inputs_closed(const char* dataflow_id, const char* const* receivers,
                                    const char* const* inputs, size_t n, uint64_t event_ns,
                                    const uint8_t* hlc_id, uint8_t* out, size_t cap,
                                    size_t* out_len);
int dora_gpu_test_ide_decode(const uint8_t* frame, size_t len, char* json, size_t cap,
                             size_t* json_len);

#ifdef __cplusplus
}
#endif
#endif /* DORA_GPU_TESTING_H */
