/*
 * dora_gpu.h — C ABI of the MI355X device-resident message data plane for dora.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, and returns an int status
 * (0 = ok, < 0 = error) with a thread-local message in dora_gpu_last_error(), following the
 * reference C node API convention (apis/c/node/src/lib.rs:245-259: 0 / -1 + logged error).
 * Reference interfaces replaced are cited per function (paths relative to the dora v0.3.6 tree).
 *
 * Arrow arrays cross the boundary through the Arrow C Data Interface — the same ABI the
 * reference's operator plugins use (apis/rust/operator/types/src/lib.rs:104-135) and that the
 * Python node imports pyarrow arrays through (apis/python/node/src/lib.rs:157-185).
 */
#ifndef DORA_GPU_H
#define DORA_GPU_H

#include <stddef.h>
#include <stdint.h>

#include "dora_fill_ticket.h" /* dora_fill_ticket, DORA_FILL_* (dora_sample_fill_ticket below) */

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------ */
/* Arrow C Data Interface + C Device Data Interface (public Arrow ABI, spec v1).              */
/* ------------------------------------------------------------------------------------------ */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
#define ARROW_FLAG_DICTIONARY_ORDERED 1
#define ARROW_FLAG_NULLABLE 2
#define ARROW_FLAG_MAP_KEYS_SORTED 4
struct ArrowSchema {
  const char* format;
  const char* name;
  const char* metadata;
  int64_t flags;
  int64_t n_children;
  struct ArrowSchema** children;
  struct ArrowSchema* dictionary;
  void (*release)(struct ArrowSchema*);
  void* private_data;
};
struct ArrowArray {
  int64_t length;
  int64_t null_count;
  int64_t offset;
  int64_t n_buffers;
  int64_t n_children;
  const void** buffers;
  struct ArrowArray** children;
  struct ArrowArray* dictionary;
  void (*release)(struct ArrowArray*);
  void* private_data;
};
#endif
#ifndef ARROW_C_DEVICE_DATA_INTERFACE
#define ARROW_C_DEVICE_DATA_INTERFACE
typedef int32_t ArrowDeviceType;
#define ARROW_DEVICE_CPU 1
#define ARROW_DEVICE_ROCM 10
#define ARROW_DEVICE_ROCM_HOST 11
struct ArrowDeviceArray {
  struct ArrowArray array;
  int64_t device_id;
  ArrowDeviceType device_type;
  void* sync_event;
  int64_t reserved[3];
};
#endif

/* ------------------------------------------------------------------------------------------ */
/* Status, errors, runtime plumbing                                                           */
/* ------------------------------------------------------------------------------------------ */
#define DORA_OK 0
#define DORA_ERR_INVALID (-1)      /* bad argument / unsupported type                       */
#define DORA_ERR_HIP (-2)          /* HIP runtime error                                     */
#define DORA_ERR_TOO_SMALL (-3)    /* target buffer too small (arrow_utils.rs:37-42 panic)  */
#define DORA_ERR_UNSUPPORTED (-4)  /* type outside the parity set (views, unions, ListView) */
#define DORA_ERR_CLOSED (-5)       /* channel / peer closed                                 */
#define DORA_ERR_TIMEOUT (-6)
#define DORA_ERR_NOT_FOUND (-7)    /* unknown output id / drop token                        */

typedef void* dora_stream_t; /* a hipStream_t; NULL = the device's null stream */

/* Thread-local message of the last failing call on this thread (never NULL). */
const char* dora_gpu_last_error(void);
/* Library version string "dora-gpu <semver> gfx950". */
const char* dora_gpu_version(void);
/* Diagnostics (no reference counterpart): this process's host time blocked on empty control
 * rings (node event/drop rings, the daemon's request rings) and spent spinning on producers'
 * fill flags, in ns since start.  Busy time = wall - idle locates a pipeline's bottleneck. */
int dora_gpu_busy_stats(uint64_t* idle_ns, uint64_t* fill_wait_ns);
/* Diagnostics (no reference counterpart): raw AQL packets this process dispatched on HIP device
 * `device`, per kernel of the embedded pack code object (min(cap, *n) entries written; *n = the
 * kernel count), and kernel k's symbol name ("" past the end).  The driver's smoke names the
 * kernels that packed its samples with these. */
int dora_gpu_aql_dispatch_counts(int device, uint64_t* counts, size_t cap, size_t* n);
const char* dora_gpu_aql_kernel_name(size_t k);
/* Diagnostics: batch packs dispatched on HIP device `device` by this process, the sends they
 * carried, and the sends that waited for queue capacity (aql.cpp: sends that find every AQL
 * queue busy leave together as one batch pack). */
int dora_gpu_aql_batch_stats(int device, uint64_t* batches, uint64_t* batched_msgs,
                             uint64_t* backlogged);
/* Diagnostics: packs on HIP device `device` whose fill the command processor signalled (the
 * packet's completion signal instead of the in-kernel flag store; mid-size single-segment packs
 * of 1-32 MiB, and synchronous single-segment sends from 1 MiB). */
int dora_gpu_aql_cp_signalled(int device, uint64_t* count);
/* Latency control (no reference counterpart): while this process sends device samples, a thread
 * per GPU publishes an empty AQL packet whenever nothing was dispatched for `period_us`, so the
 * command processor never idles long enough to need waking (~5.5 us per message otherwise, for
 * messages more than ~50 us apart); it parks 100 ms after the last send.  Default 25 us; 0 turns
 * it off (saves the thread's wake-ups); values below 5 are raised to 5.  Process-wide. */
int dora_gpu_set_keep_awake(double period_us);

int dora_gpu_device_count(int* count);
int dora_gpu_set_device(int ordinal);
int dora_gpu_get_device(int* ordinal);
int dora_gpu_stream_create(dora_stream_t* out);
int dora_gpu_stream_destroy(dora_stream_t stream);
int dora_gpu_stream_sync(dora_stream_t stream);
int dora_gpu_device_sync(void);
int dora_gpu_malloc(void** out, size_t nbytes);
int dora_gpu_free(void* ptr);
int dora_gpu_host_alloc(void** out, size_t nbytes); /* pinned host memory */
int dora_gpu_host_free(void* ptr);
/* Async copy on `stream` (direction inferred from the pointers, unified addressing). */
int dora_gpu_memcpy_async(void* dst, const void* src, size_t nbytes, dora_stream_t stream);
int dora_gpu_memset_async(void* dst, int value, size_t nbytes, dora_stream_t stream);

/* Timing on the stream the kernels run on (hipEvent pairs). */
typedef void* dora_event_t;
int dora_gpu_event_create(dora_event_t* out);
int dora_gpu_event_destroy(dora_event_t ev);
int dora_gpu_event_record(dora_event_t ev, dora_stream_t stream);
int dora_gpu_event_sync(dora_event_t ev);
int dora_gpu_event_elapsed_ms(dora_event_t start, dora_event_t stop, float* ms);

/* ------------------------------------------------------------------------------------------ */
/* Packing — replaces apis/rust/node/src/node/arrow_utils.rs:4-71                             */
/* ------------------------------------------------------------------------------------------ */
typedef struct dora_plan dora_plan;

/*
 * Host-side DFS over an Arrow array (a1, `required_data_size_inner`, arrow_utils.rs:9-21):
 * buffer lengths follow arrow-rs 53.2.0 FFI import, alignment follows arrow-data 53.2.0
 * `layout()`.  `device_type` says where the array's buffers live: ARROW_DEVICE_ROCM (HBM; the
 * pack is one HIP kernel) or ARROW_DEVICE_CPU (host memory; the pack is DMA into the slot).
 * Validity bitmaps and, for Utf8/Binary, the last offset are read to the host during planning
 * (the reference clones validity into metadata, arrow_utils.rs:66).
 * The array is borrowed: its buffers must stay valid until the pack completes on its stream.
 */
int dora_gpu_plan(const struct ArrowArray* array, const struct ArrowSchema* schema,
                  ArrowDeviceType device_type, dora_plan** out);
/*
 * Compacting plan (new capability; the reference copies sliced buffers whole and passes the
 * offset through): every node is reduced to its logical range — fixed-width values
 * sliced, Boolean bitmaps bit-shifted to bit 0, offsets rebased to 0 with the child / value
 * ranges they address sliced recursively, validity shifted for the type info — so the type info
 * has offset 0 everywhere and a slice moves only its own bytes.  Receivers are unchanged
 * (`into_arrow_array` yields a logically equal array).  Device-resident arrays only; run-end
 * encoded arrays are rejected.
 */
int dora_gpu_plan_compact(const struct ArrowArray* array, const struct ArrowSchema* schema,
                          ArrowDeviceType device_type, dora_plan** out);
/* Plan for `ArrowTypeInfo::byte_array(len)` over one contiguous buffer (metadata.rs:74-87):
 * what `send_output_raw`'s copy closure writes (node/mod.rs:180-196). */
int dora_gpu_plan_bytes(const void* src, size_t len, ArrowDeviceType device_type,
                        dora_plan** out);
/*
 * Tensors (new; no reference counterpart).  A strided n-dimensional view,
 * described by the fields of DLPack's DLTensor (nothing is vendored): element `i0, .., ik` lives
 * at `data + byte_offset + (i0 * strides[0] + .. + ik * strides[k]) * (dtype_bits / 8)`.
 * On the wire a tensor of shape (d0, d1, .., dk) and dtype T is the Arrow array of length d0 of
 * type FixedSizeList<..FixedSizeList<T>[dk]..>[d1] (child fields named `item`, nullable, as
 * pyarrow creates them; a 1-D tensor is the plain primitive array), whose sample is one buffer:
 * the row-major values.  The shape travels in the type, so a reference node can send or receive
 * the same message.
 *
 * dora_gpu_plan_tensor canonicalises the view (extents of 1 dropped, neighbours merged when
 * strides[i] == shape[i+1] * strides[i+1], an innermost unit stride folded into a row of bytes).
 * `device_type` says where the view lives, as in dora_gpu_plan:
 *   ARROW_DEVICE_CPU        a view that is dense after canonicalisation plans exactly as
 *                           dora_gpu_plan_bytes over `data + offset`, with the nested type info;
 *                           any other view is gathered by the CPU, inside this call, into a
 *                           row-major staging buffer the plan owns, and planned as a dense copy
 *                           of that buffer (what the caller's own copy to contiguous memory
 *                           would have done);
 *   ARROW_DEVICE_ROCM_HOST  pinned host memory: always copied into the staging buffer, dense or
 *                           not (a DMA or kernel reading pinned memory runs asynchronously to
 *                           the host; the copy keeps "read on return" true);
 *   ARROW_DEVICE_ROCM       HBM.  Planning reads nothing and calls nothing in HIP.  A view that is
 *                           dense after canonicalisation plans exactly as dora_gpu_plan_bytes
 *                           over `data + offset`, with the nested type info, and takes every
 *                           device path unchanged.  Any other view plans a gather: no segments,
 *                           and a kernel (gather_rows_kernel, gfx950) that reads the view once and
 *                           writes the row-major sample once.  Device strides are NOT trusted (a
 *                           read outside mapped memory faults the whole GPU): the closed interval
 *                           of byte offsets the view reaches — the negative (extent - 1) * stride
 *                           terms below element 0, the positive ones plus a row above — is
 *                           computed with overflow checks (DORA_ERR_INVALID if it leaves 64 bits),
 *                           and before anything is launched (dora_gpu_pack, a node's send) the
 *                           runtime must name one device allocation, on the current / the node's
 *                           GPU, that contains it: DORA_ERR_INVALID naming both otherwise, and
 *                           nothing is launched.  (A caching allocator's segment counts as the
 *                           allocation: the check keeps reads inside mapped memory.)  Stream
 *                           contract: the kernel runs on a stream ordered after the node stream
 *                           (dora_node_stream), so a producer orders its writes by queueing them
 *                           on, or making them precede, the node stream.  The view is borrowed
 *                           until the kernel has read it: a synchronous send returns after that
 *                           ("read on return"), see dora_node_send_output_tensor.
 *
 * Accepted dtypes: int and uint of 8/16/32/64 bits, float of 16/32/64 bits, lanes == 1.
 * DORA_ERR_UNSUPPORTED, with a message naming the dtype: bool (Arrow's is a bitmap), bfloat16 and
 * complex (Arrow has neither: send a view as uint16 or as pairs of floats; a bfloat16 tensor is
 * sent as float32 or float16 with dora_gpu_plan_tensor_cast, below), lanes != 1, and a
 * view of more than 8 dimensions after merging.  DORA_ERR_INVALID: ndim < 1, a negative extent,
 * an extent of 0 in any dimension but the first, a byte count that overflows 64 bits, a NULL
 * `data` with a non-zero element count.  d0 == 0 plans an empty message.
 * A dense ARROW_DEVICE_CPU view is borrowed until the pack completes; any other host view has
 * been read on return.  Shape and strides of a host view are trusted, as a DLPack producer's
 * are: beyond the checks above, the bytes it reaches are not bounded against any allocation, and
 * strides whose products with the extents do not fit 64 bits are the caller's error.
 */
typedef struct dora_tensor {
  const void* data;
  uint64_t byte_offset;
  uint8_t dtype_code; /* DLPack: 0 int, 1 uint, 2 float, 4 bfloat, 5 complex, 6 bool */
  uint8_t dtype_bits;
  uint16_t dtype_lanes;
  int32_t ndim;
  const int64_t* shape;
  const int64_t* strides; /* in elements, signed, 0 allowed; NULL = row-major */
} dora_tensor;
int dora_gpu_plan_tensor(const dora_tensor* tensor, ArrowDeviceType device_type, dora_plan** out);
/*
 * A record of tensors as one message: `n` named tensors, 1 <= n <= 8, that share shape[0] = d0
 * and live in the same place (`device_type`, as above, for all of them).  On the wire it is the
 * Arrow array of length d0 and type Struct<name_0: T_0, .., name_{n-1}: T_{n-1}>, T_k exactly the
 * type dora_gpu_plan_tensor gives field k alone, fields nullable (as
 * pyarrow.StructArray.from_arrays makes them).  The sample is the reference layout of that array:
 * the struct node and the list nodes carry no buffer, each leaf's row-major values sit at the
 * running offset padded to the leaf's element size, in field order; padding bytes are not
 * written.  d0 == 0 plans an empty message.  A reference node reads it as a StructArray.
 * Tensors of unrelated shapes travel as a struct of length 1: give each a leading extent of 1.
 *
 * Host fields: a dense pageable one is a copy segment over the caller's memory (borrowed until the
 * pack completes), a strided or pinned one has been gathered into the plan's staging buffer on
 * return; the plan is an ordinary multi-segment host plan.  Device fields are never dereferenced
 * here: when every field is dense the plan is n copy segments; when any is strided it carries no
 * segments and one launch of gather_struct_kernel (gfx950) reads every field, dense ones
 * included, and writes each into its own byte range.  Either way every field's reach is checked
 * against the allocation that holds it — fields may sit in different allocations — before
 * anything is launched; a refusal names the field.
 *
 * DORA_ERR_INVALID, naming the field: n == 0, a NULL or empty name, a duplicate name, a field
 * whose shape[0] differs from field 0's, a total size that overflows 64 bits.
 * DORA_ERR_UNSUPPORTED: n > 8.  Each tensor's own refusals (dora_gpu_plan_tensor) pass through
 * with the field's name prefixed.
 */
typedef struct dora_tensor_field {
  const char* name;
  dora_tensor tensor;
} dora_tensor_field;
int dora_gpu_plan_tensor_struct(const dora_tensor_field* fields, size_t n,
                                ArrowDeviceType device_type, dora_plan** out);
/*
 * A ragged batch as one message: the N rows of `fields` (a record as dora_gpu_plan_tensor_struct
 * takes it, or n == 1 with a NULL name: a bare tensor) cut into B lists by `partition`, a 1-D
 * dense tensor of int32 or int64 holding B lengths (partition_form DORA_PARTITION_LENGTHS) or
 * B + 1 offsets (DORA_PARTITION_OFFSETS).  On the wire it is the Arrow array of length B and type
 * List<item: T> (int32 offsets, child field `item`, nullable, as pyarrow.list_(T) makes it), T the
 * type the tensor or struct plan gives the values; the sample is the reference layout of
 * pyarrow.ListArray.from_arrays(offsets, child): the (B + 1) * 4 bytes of offsets first, then the
 * child's leaves as the struct plan lays them out, each padded to its element size.  A reference
 * node reads it as a ListArray.  B == 0 (one offset, N == 0) and N == 0 with B > 0 (empty lists)
 * are valid.  LargeList is not produced: N or B + 1 >= 2^31 is DORA_ERR_UNSUPPORTED.
 *
 * Where the partition lives (`partition_device`) decides how strict the plan is.
 *   On the host (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST), with values anywhere: it is read and
 *   checked here.  Lengths must be non-negative and sum to N; offsets must start at 0, never
 *   decrease and end at N; anything else is DORA_ERR_INVALID naming the first offending index.  The
 *   int32 offsets are a host source segment the plan owns: with host values segment 0 of an
 *   ordinary host plan; with device values a prefix that is copied into the sample on the stream
 *   of, and ahead of, the pack (all-dense fields: copy segments) or the one gather launch.
 *   In HBM (ARROW_DEVICE_ROCM; the values must be device values too, DORA_ERR_INVALID otherwise:
 *   pass the partition as a host list): it is never read on the host and the send adds no
 *   synchronisation.  One workgroup of the plan's one launch (gather_struct_kernel) scans it and
 *   writes the offsets.  Whatever the words hold, the message is a well-formed List,
 *   0 <= o[0] <= .. <= o[B] <= N: from lengths o[i] = min(N, sum_{j<i} max(len_j, 0)), from
 *   offsets o[i] = min(N, max(0, max_{j<=i} in_j)).  A partition that does not describe N rows is
 *   the producer's bug: it yields a well-formed message with other list boundaries, never a
 *   malformed one, where the host form refuses.  The words are range-checked against their
 *   allocation like every device field.  More than 2^20 words are DORA_ERR_UNSUPPORTED: one
 *   workgroup scans them.
 * The values' own refusals pass through unchanged (with the field prefix for a record).
 */
enum { DORA_PARTITION_LENGTHS = 0, DORA_PARTITION_OFFSETS = 1 };
typedef struct dora_tensor_list {
  const dora_tensor_field* fields;
  size_t n;
  dora_tensor partition;
  uint32_t partition_form;
  ArrowDeviceType partition_device;
} dora_tensor_list;
int dora_gpu_plan_tensor_list(const dora_tensor_list* list, ArrowDeviceType device_type,
                              dora_plan** out);
/*
 * Selected rows as one message: `values[index]` along dimension 0, without the indexed copy.
 * `fields` is a record as dora_gpu_plan_tensor_struct takes it, or n == 1 with a NULL name: a
 * bare tensor; every field has shape[0] = N.  `index` is a 1-D dense tensor of K int32 or int64
 * words (what NMS, a score threshold or top-k end in).  On the wire the message is exactly what
 * planning the materialised `values[index]` gives today: a bare tensor the nested FixedSizeList
 * array of length K, a record the Struct array of length K, and with `partition` (as
 * dora_tensor_list's, form and device included; NULL: no lists) the List over either, the
 * partition describing the K taken rows.  Type info, leaf offsets and padding are those plans'
 * with the leading extent K; there is no new Arrow type and a reference node reads the message
 * as before.  K == 0 is an empty message; K may exceed N (repeats).  A valid word is
 * 0 <= i < N: there is no negative wrap-around.
 *
 * Dimensions 1.. of a taken field are canonicalised as dora_gpu_plan_tensor does; dimension 0
 * keeps an entry of its own (extent N, its byte stride), never merged and never dropped, even at
 * extent 1 or stride 0.  More than 8 dimensions after that is DORA_ERR_UNSUPPORTED.
 *
 * The index lives where the values live (`index_device` against `device_type`): host values
 * (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST) take a host index, device values an index in this
 * node's HBM; any other pairing is DORA_ERR_INVALID (move the index next to the values; no upload
 * path exists).
 *   Host index (the host partition's rule): it is read and checked here; the first word outside
 *   [0, N) is DORA_ERR_INVALID naming its position and value.  The CPU gathers the taken rows into
 *   the plan's staging buffer — always, dense values and an identity index included — and the plan
 *   is an ordinary host plan taking every host path; every source has been read on return.
 *   Device index (the device partition's rule): it is never read on the host and adds no
 *   synchronisation.  The plan never has copy segments, dense fields included: it is one launch
 *   of gather_struct_kernel (n == 1 for a bare tensor), whose rows body reads row index[i] where
 *   the plain one reads row i; a device partition's scan share goes in front, a host partition's
 *   offsets as the small copy ahead of the launch.  A row whose word is not valid is written as
 *   zero bytes and nothing is read for it (an int64 word whose low 32 bits alone would be valid
 *   included): whatever the words hold, the message is well-formed and no address outside the
 *   checked reach is touched.  A bad index is the producer's bug and shows as zero rows.  Each
 *   field's reach is computed over all N source rows with the overflow checks of
 *   dora_gpu_plan_tensor and held against the field's allocation before anything is launched, so
 *   a valid word cannot leave it; the K index words are held against theirs the same way.
 *   N == 0 with K > 0 gives K zero rows (`data` may then be NULL).
 * DORA_ERR_INVALID on top of the values' own refusals: an index that is not 1-D, not dense
 * (stride != 1 with K > 1), not int32 or int64 with lanes == 1, a device index not aligned to its
 * word size, a NULL index with K > 0.  The partition rules of dora_gpu_plan_tensor_list apply with
 * N replaced by K: a host partition must describe K rows, a device partition is clamped to K and
 * needs device values; K or B + 1 >= 2^31 with a partition is DORA_ERR_UNSUPPORTED.
 * Selection by a boolean mask is dora_gpu_plan_tensor_mask below.  Not provided: selection along
 * another dimension, and a host index over device values.
 */
typedef struct dora_tensor_take {
  const dora_tensor_field* fields; /* a record, or n == 1 with a NULL name: a bare tensor */
  size_t n;
  dora_tensor index;               /* 1-D dense int32 / int64, K words */
  ArrowDeviceType index_device;
  const dora_tensor* partition;    /* NULL: no lists; else as dora_tensor_list, over the K taken rows */
  uint32_t partition_form;
  ArrowDeviceType partition_device;
} dora_tensor_take;
int dora_gpu_plan_tensor_take(const dora_tensor_take* take, ArrowDeviceType device_type,
                              dora_plan** out);
/*
 * Rows selected by a mask as one message, without `values[mask]`, without `nonzero` and, for
 * device values, without a host synchronisation.  `fields` is a record as
 * dora_gpu_plan_tensor_struct takes it, or n == 1 with a NULL name: a bare tensor; every field has
 * shape[0] = N.  `mask` is a 1-D dense tensor of N elements of bool (DLPack code 6, 8 bits) or
 * uint8, at any byte alignment; any non-zero byte selects its row.
 *
 * The number of selected rows K is only known where the mask is, so the message keeps the values'
 * capacity and says in its offsets how many rows are live.  Whether the values are in host memory
 * or in HBM, the message is `List<item: T>` of length B, T what dora_gpu_plan_tensor (bare) or
 * dora_gpu_plan_tensor_struct gives the values:
 *   the child has N rows: rows [0, K) are the selected rows in source order, rows [K, N) are zero
 *   bytes;
 *   offsets o[b] = C[p_b], C[i] the number of selected rows among source rows [0, i), p the
 *   partition of the N source rows (not of the K selected ones as under a take);
 *   without a partition (NULL) B = 1 and the offsets are [0, K].
 * Type info, leaf offsets and padding are those of dora_gpu_plan_tensor_list over the N rows:
 * there is no new Arrow type, and a reference node reads the message as before (a List whose
 * child is longer than its last offset is valid Arrow).  N == 0 is an empty child and all-zero
 * offsets.  A host producer that wants the tight message sends `values[mask]` itself.
 *
 * The mask lives where the values live (`mask_device` against `device_type`): host with host, this
 * node's HBM with device values; any other pairing is DORA_ERR_INVALID.
 *   Host: the CPU compacts the rows into the plan's staging buffer, zero-pads them to N rows and
 *   computes the offsets; a host partition is checked against N with the list plan's rules; the
 *   plan is an ordinary host plan and every source has been read on return.
 *   Device: the mask is never read on the host.  The plan is always a gather without segments, its
 *   fields described as a take describes them (dimension 0 kept apart, reach over all N rows, held
 *   against the field's allocation before anything is launched); the mask's N bytes are held
 *   against theirs the same way, a refusal naming `mask:`.  Three launches on one stream:
 *   mask_count_kernel and mask_compact_kernel turn the mask into N int32 index words (the first K
 *   the selected rows, the rest -1) and the counts C in a workspace, and gather_struct_kernel
 *   takes every field by that index, its scan share — over a device partition's words, clamped as
 *   dora_gpu_plan_tensor_list clamps them, or over a host partition's checked offsets — storing
 *   C[o] for the offset o.  No workgroup waits for another and nothing is atomic.
 *   The workspace is dora_gpu_plan_workspace_size bytes directly behind the sample: it is scratch
 *   of the launches, not part of the message, and nothing that moves the sample moves it.
 * DORA_ERR_INVALID on top of the values' own refusals: a mask that is not 1-D, not dense, not
 * bool or uint8 with lanes == 1, whose extent is not N, a NULL mask with N > 0.
 * DORA_ERR_UNSUPPORTED: N > 2^24 rows (one workgroup sums the per-tile totals before its tile, at
 * most 4097 words), a device partition of more than 2^20 entries.
 * Not provided: masks along another dimension, a host mask over device values, a cast under a
 * mask.
 */
typedef struct dora_tensor_mask {
  const dora_tensor_field* fields; /* a record, or n == 1 with a NULL name: a bare tensor */
  size_t n;
  dora_tensor mask;                /* 1-D dense bool / uint8, N elements */
  ArrowDeviceType mask_device;
  const dora_tensor* partition;    /* NULL: one list; else as dora_tensor_list, over the N source rows */
  uint32_t partition_form;
  ArrowDeviceType partition_device;
} dora_tensor_mask;
int dora_gpu_plan_tensor_mask(const dora_tensor_mask* mask, ArrowDeviceType device_type,
                              dora_plan** out);
/*
 * Converted tensors as one message: field k "converted to casts[k]'s dtype", the conversion run
 * inside the send's one read of the source and one write of the sample.  `fields` is a record as
 * dora_gpu_plan_tensor_struct takes it, or n == 1 with a NULL name: a bare tensor; `casts` has n
 * entries, and one with dtype_bits == 0 leaves its field as it is.  On the wire the message is
 * exactly what planning the converted tensors gives: type info, sample size and leaf offsets are
 * those of tensors of the destination dtypes with the same shapes (padding by the destination
 * element size); there is no new Arrow type and a reference node reads the message as before.
 * d0 == 0 is an empty message of that type.
 *
 * Element by element y = to_dst(to_f32(x) [* scale]).
 *   Sources: uint8, int8, uint16, int16, float16, bfloat16 (DLPack code 4, 16 bits) and float32;
 *   every value of each is exact in float32, so to_f32 never rounds.  int32, int64, float64, bool,
 *   complex and anything else are DORA_ERR_UNSUPPORTED as cast sources, naming the dtype.
 *   Destinations: float16 and float32 (code 2, 16 or 32 bits); anything else is
 *   DORA_ERR_UNSUPPORTED (float-to-integer and bfloat16 destinations are not provided by a cast;
 *   saturating integer destinations are dora_gpu_plan_tensor_convert's quantise, below).
 *   Scale (has_scale != 0): a finite float32; NaN or infinite is DORA_ERR_INVALID.  The product is
 *   one IEEE float32 multiplication, round to nearest even, subnormals kept.  to_dst for float16
 *   is one round-to-nearest-even conversion: overflow gives +-inf, float16 subnormals are produced,
 *   not flushed.
 *   The statement of record is numpy's (x.astype(float32) * float32(scale)).astype(dst), bfloat16
 *   taken as uint16 bits << 16: results are bit-exact against it for every input that is not a
 *   NaN; a NaN gives some NaN, payload unspecified.  Multiplying by float32(1/255) is not dividing
 *   by 255: the two differ in the last bit for some inputs, and the statement above is the contract.
 *   Identity: a cast whose destination equals the source dtype, without a scale, is no cast.  A
 *   call in which no field is cast plans exactly as dora_gpu_plan_tensor (bare) or
 *   dora_gpu_plan_tensor_struct does: segments, type info and gather.  With a scale it is a cast.
 *
 * Host values (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST): the CPU gathers and converts every cast
 * field inside this call into the plan's staging buffer, dense views included; the plan is an
 * ordinary host plan and every cast source has been read on return.
 * Device values: never read on the host.  Any cast field makes the plan one launch of
 * gather_cast_kernel (gfx950) and no segments, as "any field strided" does for a record; fields
 * that are not cast go through their usual body in the same launch.  Each field's reach is
 * computed with the source element size and the overflow checks of dora_gpu_plan_tensor and held
 * against the field's allocation before anything is launched.
 * DORA_ERR_INVALID, naming the field, on top of the record's and the tensors' own refusals: a
 * NULL `casts`, a cast field whose data + byte_offset is not a multiple of the source element
 * size.  dora_gpu_pack to a destination where a cast field would not start on a multiple of its
 * destination element size is DORA_ERR_INVALID with nothing launched (a node's samples never are).
 * Not provided: a cast under a ragged batch or a take.
 */
typedef struct dora_tensor_cast { /* dtype_bits == 0: this field is sent as it is */
  uint8_t dtype_code;
  uint8_t dtype_bits;
  uint16_t has_scale;
  float scale;
} dora_tensor_cast;
int dora_gpu_plan_tensor_cast(const dora_tensor_field* fields, size_t n,
                              const dora_tensor_cast* casts /* n entries */,
                              ArrowDeviceType device_type, dora_plan** out);
/*
 * Quantised tensors as one message: field k "quantised to quants[k]'s dtype", next to fields that
 * are cast (casts[k]) and fields sent as they are, through the same read of the source and the
 * same write of the sample as dora_gpu_plan_tensor_cast.  `fields` as there; `casts` and `quants`
 * are each NULL or n entries, and an entry with dtype_bits == 0 leaves its field alone.  On the
 * wire the message is exactly what planning the quantised tensors gives: type info, sample size
 * and leaf offsets of tensors of the destination dtypes with the same shapes.  With no quantised
 * field the call plans exactly as dora_gpu_plan_tensor_cast does (a NULL `casts`: as one whose
 * entries all have dtype_bits == 0).
 *
 * Element by element, [lo, hi] the destination's range:
 *   y = float32(x) [* float32(scale)]     one IEEE float32 multiplication, as in a cast
 *   r = rint(y)                           float32, ties to even (exact: no second rounding)
 *   r = 0 where y is a NaN                a NaN is the real value 0, so it becomes zero_point
 *   q = int32(clip(r, lo - zero_point, hi - zero_point)) + zero_point        +-inf saturate
 *   Sources: the seven cast sources; anything else is DORA_ERR_UNSUPPORTED, as in a cast.
 *   Destinations: uint8, int8, uint16, int16 (DLPack code 1 or 0, 8 or 16 bits); anything else
 *   (int32, uint32, int64, float, bool ..) is DORA_ERR_UNSUPPORTED, naming the dtype and the field.
 *   zero_point: an integer in [lo, hi], so both clip bounds are exact in float32; outside it
 *   DORA_ERR_INVALID.  Scale: a finite float32; NaN or infinite is DORA_ERR_INVALID.
 *   A field with both a cast and a quantise entry is DORA_ERR_INVALID.  There is no identity rule:
 *   a quantise is always a conversion (uint8 to uint8 without a scale runs, and changes nothing).
 *   The statement of record is numpy's: np.rint, np.where(np.isnan ..), np.clip, then
 *   .astype(int32) + zero_point, then .astype(dst).  Results are bit-exact against it for every
 *   input: NaNs, infinities, -0.0 and subnormals included.
 *
 * Host values: gathered and quantised by the CPU inside this call into the plan's staging buffer;
 * every source has been read on return.  Device values: never read on the host; any converted
 * field makes the plan one launch and no segments (gather_quant_kernel, gfx950, when a field is
 * quantised), each field's reach computed with the source
 * element size and held against its allocation before anything is launched.  dora_gpu_pack to a
 * destination where a 16-bit field would start on an odd address is DORA_ERR_INVALID with nothing
 * launched.
 * Not provided: a quantise under a ragged batch, a take or a mask; per-channel zero points
 * (per-channel scales and biases are dora_gpu_plan_tensor_affine's, below).
 */
typedef struct dora_tensor_quant { /* dtype_bits == 0: this field is not quantised */
  uint8_t dtype_code;
  uint8_t dtype_bits;
  uint16_t has_scale;
  float scale;
  int32_t zero_point;
} dora_tensor_quant;
int dora_gpu_plan_tensor_convert(const dora_tensor_field* fields, size_t n,
                                 const dora_tensor_cast* casts /* NULL or n entries */,
                                 const dora_tensor_quant* quants /* NULL or n entries */,
                                 ArrowDeviceType device_type, dora_plan** out);
/*
 * Normalised tensors as one message: the conversions of dora_gpu_plan_tensor_convert with an
 * affine step in front, a scale and a bias that are each one number or one value per channel —
 * (x / 255 - mean[c]) / std[c] as x * s[c] + b[c], per-channel int8 quantisation — in the same
 * read of the source and the same write of the sample.  `fields`, `casts` and `quants` as there;
 * `affines` is NULL or n entries, and an entry that is all zero adds nothing to its field.  With
 * `affines` NULL or all entries zero the call plans exactly as dora_gpu_plan_tensor_convert does.
 * The wire form — type info, sample size, leaf offsets — never depends on the affine step.
 *
 * `axis` names a dimension of the field as given (shape[axis] = C values along it), `inner` is the
 * product of the extents behind it, and for the output element with row-major index e,
 * c = (e / inner) % C and
 *   y = float32(x) * S + B      two IEEE float32 operations, each round to nearest even: the
 *                               product is rounded, then the sum; never one fused multiply-add
 *   S = scale[c], or the entry's scalar scale (casts[k] / quants[k]), or absent: no multiplication
 *   B = bias[c], or bias_value (has_bias), or absent: no addition, a zero product keeps its sign
 * and then the field's own conversion of y: to float16 / float32 (a cast) or rounded, clamped and
 * moved by zero_point (a quantise), exactly as above.  Subnormal products and sums are kept,
 * (-0) + (+0) is +0.  The statement of record is numpy's x.astype(float32) * s32 + b32 with the
 * tables reshaped to broadcast along `axis`; results are bit-exact against it, from host and from
 * device values, except for the payload of a NaN in a float destination.  A cast to the source's
 * own dtype is a conversion once it has an affine entry.
 *
 * Tables live where the values live.  Host values: a table is C float32 words in host memory,
 * read inside this call; a value that is not finite is DORA_ERR_INVALID.  Device values: a table
 * is C float32 words in HBM, never read on the host; whatever it holds the result is the formula
 * (a NaN or an infinity propagates, and under a quantise saturates or becomes zero_point), and
 * since c < C always no word outside the table is read.  Each table's 4 * C bytes are held against
 * its allocation before anything is launched, like a take's index; a refusal says which table.
 * Any field with a bias or a table makes a device plan one launch of gather_affine_kernel (gfx950).
 * A field with d0 == 0 (C == 0 included) is the empty message and nothing is launched.
 *
 * DORA_ERR_INVALID naming the field, on top of dora_gpu_plan_tensor_convert's refusals: an affine
 * entry on a field that is neither cast nor quantised; a table scale together with the entry's
 * has_scale; a table bias together with has_bias; `axis` outside the field's dimensions; a table
 * that is not 1-D, not of shape[axis] elements or not dense; a table whose data + byte_offset is
 * not a multiple of 4; a scalar bias or a host table's value that is not finite.  A table that is
 * not float32 is DORA_ERR_UNSUPPORTED, naming the dtype.
 * Not provided: per-channel zero points; a conversion under a ragged batch, a take or a mask;
 * bfloat16 destinations.
 */
typedef struct dora_tensor_affine { /* all zero: no affine step beyond the entry's own scalar scale */
  const dora_tensor* scale; /* NULL, or C float32 values along `axis`: takes the place of the scalar scale */
  const dora_tensor* bias;  /* NULL, or C float32 values along `axis` */
  int32_t axis;             /* 0 <= axis < ndim of the field; read only when a table is given */
  uint16_t has_bias;        /* a scalar bias */
  float bias_value;
} dora_tensor_affine;
int dora_gpu_plan_tensor_affine(const dora_tensor_field* fields, size_t n,
                                const dora_tensor_cast* casts /* NULL or n entries */,
                                const dora_tensor_quant* quants /* NULL or n entries */,
                                const dora_tensor_affine* affines /* NULL or n entries */,
                                ArrowDeviceType device_type, dora_plan** out);
/*
 * Class maps as one message: a field with an argmax entry is sent as the index of its maximum
 * along one axis — logits.argmax(0) of (C, H, W), logits.argmax(-1) of (B, 1000) — reduced in the
 * same read of the source, so only the index tensor is written.  `fields` as
 * dora_gpu_plan_tensor_struct takes them (one field with a NULL name: a bare tensor); `reduces` is
 * NULL or n entries, and an entry with op 0 leaves its field as it is.  With `reduces` NULL or
 * every op 0 the call plans exactly as dora_gpu_plan_tensor (bare) or dora_gpu_plan_tensor_struct
 * does, refusals included.
 *
 * A reduced field is a tensor of one of the seven cast sources (uint8, int8, uint16, int16,
 * float16, bfloat16, float32), any strided view of at least two dimensions; `axis` names a
 * dimension of it as given, of extent C >= 1.  Its wire form — type info, size, leaf offset and
 * padding — is that of the tensor of the index type (uint8, uint16, int32 or int64) whose shape
 * is the field's without `axis`; the fields of a record share the leading extent of these output
 * shapes.  For each output element with candidates v[0..C) in view order the result is the
 * smallest c such that v[c] is a NaN, or without a NaN the smallest c with v[c] >= v[k] for all k:
 * numpy's and torch's argmax of the values widened to float32 (exact for every source); -0.0 and
 * +0.0 tie.  Nothing is rounded: every send equals the statement exactly.
 *
 * Host values are reduced by the CPU inside this call (a host plan like any other, ROCM_HOST
 * sources too).  Device values are never read on the host: the field's reach over all C steps is
 * held against its allocation before anything is launched, and the plan is one launch of
 * gather_reduce_kernel (gfx950), plain fields through their usual bodies.  An empty leading
 * extent is the empty message and nothing is launched.
 *
 * Refusals, each naming the field in a record: fewer than two dimensions, `axis` outside them or
 * C == 0 (DORA_ERR_INVALID); C - 1 not representable in the index type — uint8 with C > 256,
 * uint16 with C > 65536, int32 with C > 2^31 (DORA_ERR_INVALID); a source that is not one of the
 * seven, an index type that is not one of the four, an `op` other than DORA_REDUCE_ARGMAX
 * (DORA_ERR_UNSUPPORTED, naming it).
 * Not provided: argmin, the maximum's value, a reduction beside a conversion in one record, a
 * reduction under a ragged batch, a take or a mask, more than one axis.
 */
#define DORA_REDUCE_ARGMAX 1u
typedef struct dora_tensor_reduce { /* op == 0: this field is sent as it is */
  uint32_t op;        /* DORA_REDUCE_ARGMAX */
  int32_t axis;       /* 0 <= axis < ndim of the field as given */
  uint8_t dtype_code; /* the index type (DLPack): uint 8/16, int 32/64 */
  uint8_t dtype_bits;
} dora_tensor_reduce;
int dora_gpu_plan_tensor_reduce(const dora_tensor_field* fields, size_t n,
                                const dora_tensor_reduce* reduces /* NULL or n entries */,
                                ArrowDeviceType device_type, dora_plan** out);
/*
 * Resized frames as one message: a field with a resize entry is sent with two of its dimensions
 * at new extents — a 1080x1920x3 camera frame as the 640x640x3 a detector reads — the taps read
 * from the source in place, so only the small tensor is written.  `fields` as
 * dora_gpu_plan_tensor_struct takes them (one field with a NULL name: a bare tensor); `resizes`
 * is NULL or n entries, and an entry with mode 0 leaves its field as it is.  With `resizes` NULL
 * or every mode 0 the call plans exactly as dora_gpu_plan_tensor (bare) or
 * dora_gpu_plan_tensor_struct does, refusals included.
 *
 * A resized field is a tensor of one of the seven cast sources (uint8, int8, uint16, int16,
 * float16, bfloat16, float32), any strided view of 2 to 8 dimensions; axis[0] and axis[1] name two
 * different dimensions of it as given and size[0], size[1] their new extents.  Its wire form —
 * type info, size, leaf offset and padding — is that of the tensor of the destination dtype
 * (dtype_bits 0: the source's own; else float16 or float32, or uint8, int8, uint16 or int16)
 * whose shape is the field's with those two extents replaced; the fields of a record share the
 * leading extent of these output shapes.
 *
 * The statement.  Each resized axis has source extent I and output extent O, both in [1, 32768].
 * Nearest: output coordinate o reads the one tap i = (o * I) / O (integer division).  Bilinear
 * (half-pixel centres, no antialiasing): d = 2 * O, n = max((2 * o + 1) * I - O, 0), q = n / d; if
 * q >= I - 1 then i0 = i1 = I - 1, w0 = 1, w1 = 0; else i0 = q, i1 = q + 1, r = n % d,
 * w1 = float32(r) / float32(d), w0 = float32(d - r) / float32(d), each one correctly rounded
 * float32 division of two exact integers.  Every source element is widened to float32 (exact).
 * Nearest: the value is the one tap.  Bilinear, a = axis[0], b = axis[1], v[ia][ib] the four taps:
 *   top = v[a0][b0] * wb0 + v[a0][b1] * wb1
 *   bot = v[a1][b0] * wb0 + v[a1][b1] * wb1
 *   y   = top * wa0 + bot * wa1
 * every product rounded to float32, then every sum; never a fused multiply-add.  y goes to the
 * destination as dora_gpu_plan_tensor_cast does (float16, float32: round to nearest even,
 * subnormals kept, overflow to infinity) or as dora_gpu_plan_tensor_convert does without a scale
 * and with zero point 0 (integers: nearest, ties to even, a NaN as 0, saturated).  Non-finite
 * sources give what the formula gives (inf * 0 is a NaN).  Nearest to the source's own dtype moves
 * elements unchanged.  Every send is bit-exact against this statement but for the payload of a
 * NaN in a float destination.
 *
 * Host values are resized by the CPU inside this call (a host plan like any other, ROCM_HOST
 * sources too).  Device values are never read on the host: the field's reach is that of its whole
 * view, held against its allocation before anything is launched, and the plan is one launch of
 * gather_resize_kernel (gfx950), plain fields through their usual bodies.  An empty kept leading
 * dimension is the empty message and nothing is launched.
 *
 * Refusals, each naming the field in a record: fewer than two dimensions, an axis outside them,
 * the two axes equal, I or O outside [1, 32768] (DORA_ERR_INVALID); a source that is not one of
 * the seven, a destination that is not one of the six, a bfloat16 source without a destination, a
 * mode other than the two (DORA_ERR_UNSUPPORTED, naming it).
 * Not provided: bicubic, area and antialiased modes, align_corners, one axis alone or more than
 * two, a resize beside a conversion or a reduction in one record, a resize under a ragged batch,
 * a take or a mask, bfloat16 destinations.
 */
#define DORA_RESIZE_NEAREST 1u
#define DORA_RESIZE_BILINEAR 2u
typedef struct dora_tensor_resize { /* mode == 0: this field is sent as it is */
  uint32_t mode;      /* DORA_RESIZE_NEAREST or DORA_RESIZE_BILINEAR */
  int32_t axis[2];    /* 0 <= axis < ndim of the field as given, different */
  int64_t size[2];    /* the new extents, in the order of axis */
  uint8_t dtype_code; /* the destination (DLPack); dtype_bits 0: the source's own dtype */
  uint8_t dtype_bits;
} dora_tensor_resize;
int dora_gpu_plan_tensor_resize(const dora_tensor_field* fields, size_t n,
                                const dora_tensor_resize* resizes /* NULL or n entries */,
                                ArrowDeviceType device_type, dora_plan** out);
/*
 * Crops as one message: a field with a crop entry is sent as K boxes cut out of one frame, each
 * brought to the same two extents — the detections of a 1080x1920x3 frame as the K x 128 x 64 x 3
 * a second-stage model reads — boxes and taps read where they live, so the boxes never come to
 * the host and only the small tensor is written.  `fields` as dora_gpu_plan_tensor_struct takes
 * them (one field with a NULL name: a bare tensor); `crops` is NULL or n entries, and an entry
 * with mode 0 leaves its field as it is.  With `crops` NULL or every mode 0 the call plans exactly
 * as dora_gpu_plan_tensor (bare) or dora_gpu_plan_tensor_struct does, refusals included.
 *
 * A field of crops is a frame — a tensor of one of the seven cast sources, any strided view of 2
 * to 7 dimensions — with `mode`, `axis`, `size`, `dtype_code` and `dtype_bits` exactly as
 * dora_tensor_resize has them, and `boxes`: a dense [K, 4] int32 tensor, 0 <= K <= 2^20, its
 * data + byte_offset a multiple of 4, living where the values live (`device_type`).  Row k is
 * (a_lo, b_lo, a_hi, b_hi): the half-open ranges [a_lo, a_hi) along axis[0] and [b_lo, b_hi)
 * along axis[1], in elements of the frame as given.  The wire form — type info, size, leaf offset
 * and padding — is that of the tensor of the destination dtype whose shape is (K,) followed by the
 * frame's with the two extents replaced by `size`; the fields of a record share the leading
 * extent, which for a field of crops is K.
 *
 * The statement.  The frame's extents along the two axes are Ia and Ib.  For box k:
 *   clamp:  a0 = min(max(a_lo, 0), Ia), a1 = min(max(a_hi, 0), Ia), the same for b — every word
 *           on its own, before any difference is taken, so no value of an int32 overflows;
 *   empty:  if a1 <= a0 or b1 <= b0 every byte of crop k is zero;
 *   else:   crop k is dora_gpu_plan_tensor_resize's statement with the source extents a1 - a0 and
 *           b1 - b0 and the taps a0 + i, b0 + i: the resize of frame[.., a0:a1, .., b0:b1, ..],
 *           bit for bit but for the payload of a NaN in a float destination.
 * Clamping and zeros are the meaning, not error handling: detectors emit boxes that overhang the
 * frame's edge, and outputs of a fixed capacity pad with boxes of zeros.
 *
 * Host values are cropped by the CPU inside this call, which reads the boxes (a host plan like any
 * other, ROCM_HOST sources too).  Device values and device boxes are never read on the host: the
 * frame's reach is that of its whole view, the boxes' their 16 * K bytes, each held against its
 * own allocation before anything is launched (a refusal says which), and the plan is one launch of
 * gather_crop_kernel (gfx950), plain fields through their usual bodies.  K == 0 is the empty
 * message and nothing is launched.
 *
 * Refusals, each naming the field in a record.  DORA_ERR_INVALID: a frame of fewer than 2 or more
 * than 7 dimensions, or of extent 0; an axis outside them, the two axes equal, a frame extent or
 * a size outside [1, 32768]; boxes that are NULL, not int32, not of shape [K, 4], not dense or not
 * on a multiple of 4; K above 2^20; device boxes outside device memory (boxes on the other side
 * from the values; the Python node refuses the pair before it plans); a record whose leading
 * extents differ.  DORA_ERR_UNSUPPORTED, naming it: a source that is not one of the seven, a
 * destination that is not one of the six, a bfloat16 source without a destination, a mode other
 * than the two.
 * Not provided: fractional boxes / ROI-align, rotated boxes, per-box sizes, a batch index per box,
 * int64 or float boxes, crops beside a conversion, a reduction or a resize in one record, crops
 * under a ragged batch, a take or a mask.
 */
typedef struct dora_tensor_crop { /* mode == 0: this field is sent as it is */
  uint32_t mode;      /* DORA_RESIZE_NEAREST or DORA_RESIZE_BILINEAR */
  int32_t axis[2];    /* 0 <= axis < ndim of the frame as given, different */
  int64_t size[2];    /* the extents of every crop, in the order of axis */
  uint8_t dtype_code; /* the destination (DLPack); dtype_bits 0: the source's own dtype */
  uint8_t dtype_bits;
  const dora_tensor* boxes; /* [K, 4] int32, dense, where the values live */
} dora_tensor_crop;
int dora_gpu_plan_tensor_crop(const dora_tensor_field* fields, size_t n,
                              const dora_tensor_crop* crops /* NULL or n entries */,
                              ArrowDeviceType device_type, dora_plan** out);
/*
 * Model inputs as one message: a resized field or a field of crops with what a model's input
 * still needs — the image placed inside a filled output (a letterbox) and a per-channel
 * normalisation — done in the same read of the source.  A 1080x1920x3 uint8 frame goes out as the
 * 3x640x640 float16 a detector reads: aspect kept, padded with grey 114, (x / 255 - mean[c]) /
 * std[c].  `fields` as dora_gpu_plan_tensor_struct takes them; `resizes` and `crops` as
 * dora_gpu_plan_tensor_resize and dora_gpu_plan_tensor_crop take them, one of the two NULL (or
 * without an active entry); `preps` is NULL or n entries, and an all-zero entry adds nothing to
 * its field.  With `preps` NULL or all zero the call plans exactly as
 * dora_gpu_plan_tensor_resize (`crops` NULL) or dora_gpu_plan_tensor_crop (`resizes` NULL) does,
 * refusals included.  The wire form — type info, sample size, leaf offsets, padding — never
 * depends on a prep entry: it is that of the field's resize or crops.
 *
 * The statement.  For every output element, r is a float32:
 *   placement (resize only; inner != {0, 0}): the resized image has extents inner = (Ra, Rb),
 *     1 <= R <= size, and starts at lead = (pa, pb), 0 <= p <= size - R, inside the output of
 *     extents `size`.  At output coordinates (oa, ob) along axis[0], axis[1]: if pa <= oa < pa + Ra
 *     and pb <= ob < pb + Rb, r is dora_gpu_plan_tensor_resize's value before its conversion with
 *     the output extents (Ra, Rb) at the coordinates (oa - pa, ob - pb); otherwise r = fill and no
 *     source element is read.  inner == {0, 0}: the image fills the output, r is the resize's (the
 *     crop's) value before its conversion.
 *   normalise: y = r * S + B, two IEEE float32 operations, the product rounded, then the sum,
 *     never one fused multiply-add.  S = scale[c] (a table), or scale_value (has_scale), or absent:
 *     no multiplication.  B = bias[c], or bias_value (has_bias), or absent: no addition, a zero
 *     product keeps its sign.  c is the output coordinate along `axis`, a dimension of the field
 *     (for crops: of the frame, not counting K) as given that is not one of the two resized ones.
 *     Padding goes through the same step: fill 114 under (x / 255 - mean) / std is what padding
 *     before normalising gives.
 *   conversion: y to the field's destination exactly as the resize or crops converts — float16 /
 *     float32 as dora_gpu_plan_tensor_cast, integers as dora_gpu_plan_tensor_convert without a
 *     scale and with zero point 0 (a normalise into the source's own integer dtype included).
 *   crops: every byte of an empty box's crop stays zero, the normalise step is not applied to it.
 * The statement of record is dora_amd.tensor.from_numpy_resize / from_numpy_crops with the same
 * arguments; results are bit-exact against it, from host and from device values, but for the
 * payload of a NaN in a float destination.  dora_amd.tensor.letterbox gives the integer geometry
 * (inner, lead) of an aspect-preserving fit, which a receiver uses to map boxes back.
 *
 * Tables live where the values live, as dora_gpu_plan_tensor_affine's do.  Host values: C float32
 * words in host memory, read inside this call, every value finite; the CPU resizes, places and
 * normalises inside this call.  Device values: C float32 words in HBM, never read on the host;
 * each table's 4 * C bytes are held against its own allocation before anything is launched, like
 * the frame's reach and the boxes (a refusal says which), and since c < C always no word outside
 * a table is read.  Any field with a non-zero prep entry makes a device plan one launch of
 * gather_resize_prep_kernel or gather_crop_prep_kernel (gfx950), plain fields through their
 * usual bodies.
 *
 * DORA_ERR_INVALID naming the field, on top of the resize's or the crops' own refusals: a prep
 * entry on a field that is neither resized nor crops; `axis` (with a table) outside the field's
 * dimensions or equal to a resized axis; a table together with its scalar (has_scale, has_bias);
 * a table that is not 1-D, not of shape[axis] elements, not dense or not on a multiple of 4; a
 * scalar or `fill` that is not finite; a host table's value that is not finite; inner[j] outside
 * [1, size[j]] or lead[j] outside [0, size[j] - inner[j]] (one of inner's two 0 included); `inner`
 * on a crops field; resize entries and crops entries both active in one call.  A table that is
 * not float32 is DORA_ERR_UNSUPPORTED, naming the dtype.
 * Not provided: zero points, placement for crops (per-box aspect would put a division per box on
 * the device), per-box fill, bfloat16 destinations, resize and crops in one record.
 */
typedef struct dora_tensor_prep { /* all zero: nothing is added to the field's resize or crops */
  const dora_tensor* scale; /* NULL, or C float32 values along `axis` */
  const dora_tensor* bias;  /* NULL, or C float32 values along `axis` */
  int32_t axis;             /* a dimension of the field (the frame) as given, not a resized one; read only with a table */
  uint16_t has_scale, has_bias;
  float scale_value, bias_value;
  int64_t inner[2];         /* 0, 0: the image fills the output; else 1 <= inner[j] <= size[j] */
  int64_t lead[2];          /* 0 <= lead[j] <= size[j] - inner[j] */
  float fill;               /* finite; read only with inner */
} dora_tensor_prep;
int dora_gpu_plan_tensor_prep(const dora_tensor_field* fields, size_t n,
                              const dora_tensor_resize* resizes /* NULL or n entries */,
                              const dora_tensor_crop* crops /* NULL or n entries */,
                              const dora_tensor_prep* preps /* NULL or n entries */,
                              ArrowDeviceType device_type, dora_plan** out);
void dora_gpu_plan_free(dora_plan* plan);
/* required_data_size (arrow_utils.rs:4-8). */
size_t dora_gpu_plan_size(const dora_plan* plan);
/* Scratch bytes the plan's launches need directly behind the sample, alignment slack included: a
 * device mask plan's index, counts and totals (dora_gpu_plan_tensor_mask); 0 for every other
 * plan.  They are no part of the message. */
size_t dora_gpu_plan_workspace_size(const dora_plan* plan);
size_t dora_gpu_plan_num_segments(const dora_plan* plan);
/* Segment i: source pointer, destination offset in the sample, length. */
int dora_gpu_plan_segment(const dora_plan* plan, size_t i, const void** src, uint64_t* dst_off,
                          uint64_t* len);
/*
 * Serialized ArrowTypeInfo (libraries/message/src/metadata.rs:51-59), little endian:
 *   str data_type (u32 n + n bytes: the DataType as a schema tree — str format, str name,
 *   i64 flags, u8 has_meta [str meta], u32 n_children × tree, u8 has_dict [tree]),
 *   u64 len, u64 null_count,
 *   u8 has_validity [u64 n + n bytes], u64 offset, u32 n_buffers × (u64 offset, u64 len),
 *   u32 n_children × TypeInfo.
 * Call with buf = NULL to get the size.
 */
int dora_gpu_plan_type_info(const dora_plan* plan, uint8_t* buf, size_t cap, size_t* len);
/*
 * copy_array_into_sample (arrow_utils.rs:23-71): copy every buffer to its aligned offset in
 * `dst` (device memory, `dst_len` >= plan size) on `stream`; async.  Padding is not written.
 * A device mask plan needs `dst_len` >= size + dora_gpu_plan_workspace_size and `dst` on a
 * multiple of 4: otherwise DORA_ERR_INVALID naming both numbers, with nothing launched.
 */
int dora_gpu_pack(const dora_plan* plan, void* dst, size_t dst_len, dora_stream_t stream);
/* ------------------------------------------------------------------------------------------ */
/* Device-resident Arrow arrays                                                               */
/* ------------------------------------------------------------------------------------------ */
/* Deep-copy a host Arrow array into HBM, same structure (offsets, lengths, children). The
 * result owns its device buffers; free with dora_gpu_array_release. */
int dora_gpu_array_upload(const struct ArrowArray* array, const struct ArrowSchema* schema,
                          struct ArrowArray* out);
/* Deep-copy a device Arrow array to host memory (for CPU consumers such as pyarrow). */
int dora_gpu_array_download(const struct ArrowArray* array, const struct ArrowSchema* schema,
                            struct ArrowArray* out);
/*
 * Receiver side of a sample — `RawData::into_arrow_array` / `buffer_into_arrow_array`
 * (apis/rust/node/src/event_stream/event.rs:35-91): a zero-copy device ArrowArray whose buffers
 * are slices of `sample` per BufferOffset (validity uploaded from the type info), plus its
 * ArrowSchema.  sample_len == 0 yields an empty array of the data type (event.rs:65-67).
 * `sample` must outlive the array.
 */
int dora_gpu_sample_import(const void* sample, size_t sample_len, const uint8_t* type_info,
                           size_t type_info_len, struct ArrowArray* out_array,
                           struct ArrowSchema* out_schema);
/* The DataType of a serialized ArrowTypeInfo as an ArrowSchema. */
int dora_gpu_type_info_schema(const uint8_t* type_info, size_t type_info_len,
                              struct ArrowSchema* out_schema);
void dora_gpu_array_release(struct ArrowArray* array);
void dora_gpu_schema_release(struct ArrowSchema* schema);

/* ------------------------------------------------------------------------------------------ */
/* Device checksums and payload generation (parity at full sizes; see oracle/checksum_ref.py) */
/* ------------------------------------------------------------------------------------------ */
/* csum64 of `len` device bytes; the result is written to device `out` (one u64), async. */
int dora_gpu_csum64(const void* data, size_t len, uint64_t* out_dev, dora_stream_t stream);
/* Blocking convenience: returns csum64 to the host. */
int dora_gpu_csum64_sync(const void* data, size_t len, dora_stream_t stream, uint64_t* out);
/* Fill `len` device bytes with the splitmix64 stream of `seed` (BASELINE.md §2 payloads). */
int dora_gpu_fill_splitmix(void* dst, size_t len, uint64_t seed, dora_stream_t stream);
/* The same payload written into a sample in place and published by the kernel itself: `ticket`
 * from dora_sample_fill_ticket for that sample (the kernel stores write-through:
 * DORA_FILL_WRITE_THROUGH is the mode to ask for), `dst` the sample's data (16-byte aligned), one launch of the ticket's workgroup count on `stream`.  The in-tree
 * user of include/dora_gpu_device.h; the kernel to copy from is examples/publish_kernel.hip. */
int dora_gpu_fill_splitmix_ticket(void* dst, size_t len, uint64_t seed,
                                  const dora_fill_ticket* ticket, dora_stream_t stream);
/* ------------------------------------------------------------------------------------------ */
/* Node API — replaces DoraNode / EventStream (apis/rust/node/src/node/mod.rs:42-503,         */
/* apis/rust/node/src/event_stream/mod.rs:27-235) and the C node API (apis/c/node/node_api.h) */
/* ------------------------------------------------------------------------------------------ */
typedef struct dora_node dora_node;
typedef struct dora_sample dora_sample;
typedef struct dora_event dora_event;

enum {
  DORA_EVENT_STOP = 0,             /* Event::Stop                       (event.rs:12)     */
  DORA_EVENT_INPUT = 1,            /* Event::Input{id, metadata, data}  (event.rs:17-21)  */
  DORA_EVENT_INPUT_CLOSED = 2,     /* Event::InputClosed{id}            (event.rs:22-24)  */
  DORA_EVENT_ERROR = 3,            /* Event::Error                      (event.rs:25)     */
  DORA_EVENT_ALL_INPUTS_CLOSED = 4 /* end of the event stream (NodeEvent::AllInputsClosed) */
};

/* DoraNode::init (mod.rs:121-155): attach to the dataflow region `shm_name`, register as
 * `node_id` on GPU `device`, subscribe and wait for every node of the dataflow to be ready. */
int dora_node_init(const char* shm_name, const char* node_id, int device, dora_node** out);
/* DoraNode::init_from_env (mod.rs:65-76): DORA_GPU_DATAFLOW, DORA_NODE_ID, DORA_GPU_DEVICE. */
int dora_node_init_from_env(dora_node** out);
/* Drop for DoraNode (mod.rs:384-431): close outputs, wait <= 10 s for drop tokens, done. */
void dora_node_free(dora_node* node);
/* DoraNode::dataflow_id / id (mod.rs:373-382): the dataflow's id as its daemon names it (the
 * reference's DataflowId is a uuid; a name that is not one maps to the UUID the inter-daemon
 * wire carries, dora_amd/dataflow.py dataflow_uuid) and this node's id.  Owned by the node. */
const char* dora_node_dataflow_id(const dora_node* node);
const char* dora_node_id(const dora_node* node);
/* The node's HIP stream; consumers must run their kernels on it so the drop token is only
 * returned after they have read the sample.  Sends spread their fills over the node's fill
 * streams (three): a fill runs after the work queued on this stream
 * when the send is made, and the call orders every fill launched so far before the work the
 * caller queues on the returned stream next (a device source may be rewritten there). */
dora_stream_t dora_node_stream(dora_node* node);

/* allocate_data_sample (mod.rs:303-346): a device slot of `len` bytes (best-fit from the
 * node's cache of recycled slots, else a new exported hipMalloc slot); len 0 -> empty Vec.  A
 * host-only node (device < 0) gets the reference's samples instead: an inline Vec below 4096 B,
 * else a POSIX shared-memory region (DataMessage::SharedMemory, mod.rs:321-346) it writes with
 * the CPU; dora_sample_data is then a host pointer. */
int dora_node_allocate_data_sample(dora_node* node, size_t len, dora_sample** out);
void* dora_sample_data(dora_sample* sample); /* device pointer (slot) */
size_t dora_sample_len(const dora_sample* sample);
/* An unsent sample back to the node's cache.  A sample that was already sent or discarded is
 * left alone (dora_gpu_last_error says so). */
void dora_sample_discard(dora_node* node, dora_sample* sample);
/* send_output_sample (mod.rs:246-275): consumes `sample` (may be NULL = no data); a sample that
 * was already sent or discarded is refused with DORA_ERR_INVALID (the reference moves its
 * DataSample into the call).  The sample must be written before the call: on the host, or by
 * work queued on dora_node_stream() — receivers then wait for that work through the slot's fill
 * signal, the call does not — or on another stream the caller synchronized, or by a kernel that
 * publishes it itself (dora_sample_fill_ticket below: no stream operation at all).  `params` is
 * the encoded MetadataParameters (u32 n, then per entry: u64 klen, key, u8 tag 0=bool 1=int 2=string,
 * value: u8 | i64 | u64 len + bytes). */
int dora_node_send_output_sample(dora_node* node, const char* output_id, const uint8_t* type_info,
                                 size_t type_info_len, const uint8_t* params, size_t params_len,
                                 dora_sample* sample);
/* Publishing a sample from the caller's own kernel (new; no reference counterpart).  Takes the
 * sample's send epoch and fills `out` for ONE launch of `workgroups` workgroups (1..4096) that
 * writes the sample and calls dora_fill_publish (include/dora_gpu_device.h); `mode` says how it
 * stores (DORA_FILL_WRITE_THROUGH / DORA_FILL_PLAIN).  dora_node_send_output_sample then queues
 * no stream operation for the sample: receivers wait on the slot's fill flag, which the kernel
 * raises.  The kernel may run on any stream and be launched before or after the send.  A ticket
 * whose kernel never runs (or runs with another workgroup count) delivers a sample that fails at
 * its receivers after DORA_GPU_TRANSIT_LIMIT_MS, like any fill that never completes, and
 * dora_node_sync then times out.  Discarding a ticketed sample (dora_sample_discard,
 * dora_node_free) drains the node stream and raises the flag from the host, so the slot is
 * reusable; a kernel launched for it on another stream must have completed before the discard.
 * Refused with DORA_ERR_UNSUPPORTED (the stream-ordered path of dora_node_send_output_sample
 * remains): an inline sample (no slot: below 4096 B on a host-only node, or empty), a
 * shared-memory slot, a node without a GPU, a slot without a fill flag or a node without done
 * words.  DORA_ERR_INVALID: workgroups 0 or > 4096, an unknown mode, a sample not live on this
 * node, a second ticket for one sample. */
int dora_sample_fill_ticket(dora_node* node, dora_sample* sample, uint32_t workgroups,
                            uint32_t mode, dora_fill_ticket* out);
/* send_output (mod.rs:198-215): plan + allocate + HIP pack + send.  `device_type` as in
 * dora_gpu_plan; a host-resident array whose sample is < 4096 B travels inline as the
 * reference's DataMessage::Vec (mod.rs:40,303-319: no slot, no GPU work).  Like the reference,
 * which copies the array inside the call
 * (arrow_utils.rs:48), the call returns once the sample no longer needs the source: for a
 * device source it waits (after the descriptor has left) until the pack kernel has read it, so
 * the caller may rewrite or free the source on any stream right away.  (A single-segment
 * sample of 1-192 MiB from a 16-byte-aligned source is packed read-first: the call returns
 * when every source byte is in the pack's registers, before its stores have drained.)  When
 * every receiver of the output runs without a GPU, a device sample <= 1 MiB is packed into
 * shared memory and a host sample >= 4096 B copied there by the CPU (DataMessage::SharedMemory,
 * complete when the call returns). */
int dora_node_send_output(dora_node* node, const char* output_id, const struct ArrowArray* array,
                          const struct ArrowSchema* schema, ArrowDeviceType device_type,
                          const uint8_t* params, size_t params_len);
/* send_output_raw / send_output_bytes (mod.rs:180-196, 217-228): `len` bytes as
 * ArrowTypeInfo::byte_array, copied into a device sample (kernel for HBM sources, DMA for host
 * sources); returns once the source has been read, as dora_node_send_output.  This is the
 * benchmark's send path (examples/benchmark/node/src/main.rs:46-48). */
int dora_node_send_output_bytes(dora_node* node, const char* output_id, const void* data,
                                size_t len, ArrowDeviceType device_type, const uint8_t* params,
                                size_t params_len);
/* Flags of the _ex variants (no reference counterpart). */
#define DORA_SEND_ASYNC 1u /* return before the pack has read a device source (below) */
/* dora_node_send_output / _bytes with `flags`.  With DORA_SEND_ASYNC a device-source send
 * returns as soon as its pack is queued: the caller must not write the source until the pack
 * has read it — i.e. until dora_node_sync(), or only by work queued on dora_node_stream()
 * fetched after the send (which orders every fill launched so far before it).  Senders that
 * never rewrite their sources (frame rings, the benchmark) overlap packs this way; a host
 * source is always safe to reuse on return. */
int dora_node_send_output_ex(dora_node* node, const char* output_id, const struct ArrowArray* array,
                             const struct ArrowSchema* schema, ArrowDeviceType device_type,
                             const uint8_t* params, size_t params_len, uint32_t flags);
int dora_node_send_output_bytes_ex(dora_node* node, const char* output_id, const void* data,
                                   size_t len, ArrowDeviceType device_type, const uint8_t* params,
                                   size_t params_len, uint32_t flags);
/* Send a tensor view (dora_gpu_plan_tensor: its wire type, `device_type`, accepted dtypes and
 * refusals).  A host or pinned source takes the paths of any host source: inline below 4096 B,
 * shared memory on a node without a GPU or for receivers that all lack one, else the BAR fill or
 * the DMA into a device slot; it has been read when the call returns (pageable memory declared
 * ARROW_DEVICE_CPU: as dora_node_send_output_bytes; memory that is in fact pinned must be
 * declared ARROW_DEVICE_ROCM_HOST).  A device source (ARROW_DEVICE_ROCM) must lie inside one
 * allocation of the node's GPU (DORA_ERR_INVALID otherwise, nothing sent); dense, it is packed as
 * dora_node_send_output_bytes packs device bytes; strided, it is gathered into an HBM slot on a
 * fill stream ordered after the node stream, and the stream raises the sample's fill flag.  The
 * call returns once the kernel has read the source.  `flags`: DORA_SEND_ASYNC changes nothing
 * for host sources; a device source's send then returns once the kernel is queued, and the
 * caller keeps the source alive and unwritten until dora_node_sync (or writes it only through
 * work queued on dora_node_stream fetched after the send). */
int dora_node_send_output_tensor(dora_node* node, const char* output_id, const dora_tensor* tensor,
                                 ArrowDeviceType device_type, const uint8_t* params,
                                 size_t params_len, uint32_t flags);
/* Send a record of tensors as one Struct message (dora_gpu_plan_tensor_struct: wire type, layout
 * and refusals).  Host fields and all-dense device fields take the paths of any multi-segment
 * plan.  Device fields of which any is strided are gathered by one kernel launch into an HBM slot,
 * as a single strided tensor is: on a fill stream ordered after the node stream (a
 * broadcast-group output: on its own stream), the stream raises the fill flag, receivers without
 * a GPU stage the slot as usual.  A synchronous send returns once the kernel has read every
 * field; with DORA_SEND_ASYNC, once it is queued, and the caller keeps every field alive and
 * unwritten until dora_node_sync. */
int dora_node_send_output_tensor_struct(dora_node* node, const char* output_id,
                                        const dora_tensor_field* fields, size_t n,
                                        ArrowDeviceType device_type, const uint8_t* params,
                                        size_t params_len, uint32_t flags);
/* Send a ragged batch as one List message (dora_gpu_plan_tensor_list: wire type, layout, where
 * the partition lives, refusals).  Host values take every path of a multi-segment host plan,
 * inline below 4096 B included.  Device values go where the struct send's go, the offsets with
 * them: a host partition's as a small copy on the fill stream ahead of the pack or gather, a
 * device partition's written by the launch itself.  A synchronous send returns once the kernel has
 * read every field and the partition; with DORA_SEND_ASYNC, once it is queued, and the caller
 * keeps the fields and a device partition alive and unwritten until dora_node_sync. */
int dora_node_send_output_tensor_list(dora_node* node, const char* output_id,
                                      const dora_tensor_list* list, ArrowDeviceType device_type,
                                      const uint8_t* params, size_t params_len, uint32_t flags);
/* Send selected rows (dora_gpu_plan_tensor_take: wire form, where the index lives, zero rows,
 * refusals).  Host values with a host index take every path of a host plan, inline below 4096 B
 * included, and everything has been read on return.  Device values with a device index go where
 * the struct and list sends' gathers go — one launch on a fill stream ordered after the node
 * stream, the stream raises the fill flag, receivers without a GPU stage the slot — with the
 * index as one more borrowed source: a synchronous send returns once the launch has read every
 * field, the index and a device partition; with DORA_SEND_ASYNC, once it is queued, and the
 * caller keeps all of them alive and unwritten until dora_node_sync. */
int dora_node_send_output_tensor_take(dora_node* node, const char* output_id,
                                      const dora_tensor_take* take, ArrowDeviceType device_type,
                                      const uint8_t* params, size_t params_len, uint32_t flags);
/* Send converted tensors (dora_gpu_plan_tensor_cast: semantics, wire form, refusals), with the
 * contract of dora_node_send_output_tensor_struct.  Host values have been read and converted on
 * return and take every path of a host plan.  Device values go where the struct send's gather
 * goes, one launch of gather_cast_kernel on a fill stream ordered after the node stream: a
 * synchronous send returns once the launch has read every field; with DORA_SEND_ASYNC, once it
 * is queued, and the caller keeps the fields alive and unwritten until dora_node_sync. */
int dora_node_send_output_tensor_cast(dora_node* node, const char* output_id,
                                      const dora_tensor_field* fields, size_t n,
                                      const dora_tensor_cast* casts, ArrowDeviceType device_type,
                                      const uint8_t* params, size_t params_len, uint32_t flags);
/* Send quantised, cast and plain tensors as one message (dora_gpu_plan_tensor_convert: semantics,
 * wire form, refusals), with the contract of dora_node_send_output_tensor_cast: host values read
 * and converted on return, device values in one launch on a fill stream. */
int dora_node_send_output_tensor_convert(dora_node* node, const char* output_id,
                                         const dora_tensor_field* fields, size_t n,
                                         const dora_tensor_cast* casts,
                                         const dora_tensor_quant* quants,
                                         ArrowDeviceType device_type, const uint8_t* params,
                                         size_t params_len, uint32_t flags);
/* Send normalised tensors (dora_gpu_plan_tensor_affine: semantics, where the tables live,
 * refusals), with the contract of dora_node_send_output_tensor_convert: host values and host
 * tables read on return, device values and device tables in one launch on a fill stream; with
 * DORA_SEND_ASYNC the caller keeps the tables alive and unwritten with the fields until
 * dora_node_sync. */
int dora_node_send_output_tensor_affine(dora_node* node, const char* output_id,
                                        const dora_tensor_field* fields, size_t n,
                                        const dora_tensor_cast* casts,
                                        const dora_tensor_quant* quants,
                                        const dora_tensor_affine* affines,
                                        ArrowDeviceType device_type, const uint8_t* params,
                                        size_t params_len, uint32_t flags);
/* Send class maps (dora_gpu_plan_tensor_reduce: semantics, refusals), with the contract of
 * dora_node_send_output_tensor_convert: host values are read and reduced on return, device values
 * are read by one launch on a fill stream, and the synchronous send waits for the read. */
int dora_node_send_output_tensor_reduce(dora_node* node, const char* output_id,
                                        const dora_tensor_field* fields, size_t n,
                                        const dora_tensor_reduce* reduces,
                                        ArrowDeviceType device_type, const uint8_t* params,
                                        size_t params_len, uint32_t flags);
/* Send resized frames (dora_gpu_plan_tensor_resize: the statement, refusals), with the contract
 * of dora_node_send_output_tensor_reduce: host values are read and resized on return, device
 * values are read by one launch on a fill stream, and the synchronous send waits for the read. */
int dora_node_send_output_tensor_resize(dora_node* node, const char* output_id,
                                        const dora_tensor_field* fields, size_t n,
                                        const dora_tensor_resize* resizes,
                                        ArrowDeviceType device_type, const uint8_t* params,
                                        size_t params_len, uint32_t flags);
/* Send crops (dora_gpu_plan_tensor_crop: the statement, where the boxes live, refusals), with the
 * contract of dora_node_send_output_tensor_resize: host values and host boxes are read and cropped
 * on return, device values and device boxes are read by one launch on a fill stream, and the
 * synchronous send waits for the read; with DORA_SEND_ASYNC the caller keeps the boxes alive and
 * unwritten with the fields until dora_node_sync. */
int dora_node_send_output_tensor_crop(dora_node* node, const char* output_id,
                                      const dora_tensor_field* fields, size_t n,
                                      const dora_tensor_crop* crops,
                                      ArrowDeviceType device_type, const uint8_t* params,
                                      size_t params_len, uint32_t flags);
/* Send model inputs (dora_gpu_plan_tensor_prep: the statement, where the tables live, refusals),
 * with the contract of dora_node_send_output_tensor_resize / _crop: host values, host tables and
 * host boxes are read on return, device values, tables and boxes are read by one launch on a fill
 * stream, and the synchronous send waits for the read; with DORA_SEND_ASYNC the caller keeps the
 * tables and the boxes alive and unwritten with the fields until dora_node_sync. */
int dora_node_send_output_tensor_prep(dora_node* node, const char* output_id,
                                      const dora_tensor_field* fields, size_t n,
                                      const dora_tensor_resize* resizes,
                                      const dora_tensor_crop* crops,
                                      const dora_tensor_prep* preps,
                                      ArrowDeviceType device_type, const uint8_t* params,
                                      size_t params_len, uint32_t flags);
/* Send rows selected by a mask (dora_gpu_plan_tensor_mask: wire form, where the mask lives,
 * refusals), with the contract of the take send: host values with a host mask take every path of
 * a host plan and everything has been read on return; device values with a device mask go where
 * the take's gather goes, the mask one more borrowed source and the workspace in the sample's own
 * slot behind the sample, so that samples in flight share nothing and receivers, relays and
 * staging move the sample alone.  A synchronous send returns once the launches have read every
 * field, the mask and a device partition; with DORA_SEND_ASYNC, once they are queued, and the
 * caller keeps all of them alive and unwritten until dora_node_sync. */
int dora_node_send_output_tensor_mask(dora_node* node, const char* output_id,
                                      const dora_tensor_mask* mask, ArrowDeviceType device_type,
                                      const uint8_t* params, size_t params_len, uint32_t flags);
/* Make DORA_SEND_ASYNC the default of every send of this node (also DORA_GPU_SEND_ASYNC=1). */
int dora_node_set_async_sends(dora_node* node, int enable);
/* Event-stream thread (the reference's event_stream_loop, apis/rust/node/src/event_stream/
 * thread.rs:81-188; no counterpart in the C API): `enable` starts a thread that drains the
 * daemon's events into the node's input queue continuously and applies the drop-oldest policy
 * there (node_communication/mod.rs:320-359), so inputs keep arriving — broadcast receives posted,
 * tokens of dropped inputs returned — while the user thread is busy; dora_node_next_event then
 * takes events from that queue.  Nodes that receive over an RCCL broadcast group start it
 * themselves.  0 stops it. */
int dora_node_set_event_thread(dora_node* node, int enable);
/* Use compacting plans (dora_gpu_plan_compact) in dora_node_send_output for device arrays. */
int dora_node_set_compact(dora_node* node, int enable);
/* close_outputs (mod.rs:277-289). */
int dora_node_close_outputs(dora_node* node, const char* const* output_ids, size_t count);

/* EventStream::recv / recv_timeout (event_stream/mod.rs:121-140); timeout_us < 0 blocks.
 * Returns DORA_ERR_TIMEOUT on timeout and DORA_ERR_CLOSED after the stream ended. */
int dora_node_next_event(dora_node* node, int64_t timeout_us, dora_event** out);
int dora_event_type(const dora_event* ev);
const char* dora_event_id(const dora_event* ev);
const char* dora_event_error(const dora_event* ev);
/* Raw sample of an input: device pointer (mapped IPC slot) or host pointer for inline Vec data
 * and for a host-only receiver's shared-memory samples (dora_event_is_device says which).  An
 * input whose slot lives on another GPU, or a host-only producer's shared-memory sample at a
 * device receiver, is pulled into local HBM on the first call (complete on return; the
 * producer's token goes back at once; see dora_node_peer_stats). */
int dora_event_data(const dora_event* ev, const void** ptr, size_t* len);
int dora_event_is_device(const dora_event* ev);
/* Serialized ArrowTypeInfo / MetadataParameters / timestamp of the input's Metadata. */
int dora_event_type_info(const dora_event* ev, const uint8_t** type_info, size_t* len);
int dora_event_parameters(const dora_event* ev, const uint8_t** params, size_t* len);
uint64_t dora_event_timestamp_ns(const dora_event* ev);
/* RawData::into_arrow_array (event.rs:35-91): zero-copy device ArrowArray over the sample; it
 * keeps the input (and its drop token) alive until released.  An inline Vec sample (< 4096 B
 * from a host source) and a host-only receiver's shared-memory sample import as a host
 * ArrowArray over their bytes instead. */
int dora_event_array(const dora_event* ev, struct ArrowArray* out_array,
                     struct ArrowSchema* out_schema);
/* Drop the event; the drop token is reported once no array references the data any more. */
void dora_event_free(dora_event* ev);
/* Relay stage (new; a reference relay node does recv -> send_output_sample with a copy of the
 * data, apis/rust/node/src/node/mod.rs:180-275): send the input `ev` on `output_id` with its
 * ArrowTypeInfo and the given parameters.  The payload moves once: a cross-GPU input is copied
 * from the peer's slot straight into this node's new slot.  `ev` stays valid (free it after). */
int dora_node_forward(dora_node* node, const char* output_id, const dora_event* ev,
                      const uint8_t* params, size_t params_len);
/* A same-GPU device input is forwarded in place: the new message points at the producer's slot
 * under a token of this node, and the input (with the producer's token) is held until that token
 * returns — no copy, no new slot.  Cross-GPU inputs, broadcast-group inputs and
 * copy into a fresh slot instead.  Forwards done in place, and forwards
 * whose token has not returned yet. */
int dora_node_forward_stats(dora_node* node, uint64_t* in_place, uint64_t* held);

int dora_node_stats(dora_node* node, uint64_t* slots_created, uint64_t* cache_hits,
                    uint64_t* in_flight, uint64_t* dropped_inputs);
/* Counters of any node of this node's dataflow (new; diagnostics, read through the shared
 * control region): device slots it created, producers' slots it mapped with
 * hipIpcOpenMemHandle, and inputs its queue_size policy dropped.  A steady edge creates and maps
 * nothing: a benchmark reads them around a timed region to show it paid no set-up cost inside
 * and that every message it counts was delivered. */
int dora_node_dataflow_counters(dora_node* node, const char* node_id, uint64_t* slots_created,
                                uint64_t* ipc_opens, uint64_t* dropped_inputs);
/* Fills (packs of sends) by dispatch path: raw AQL packets on the process's HSA queue (device
 * sources of <= 8 segments) or hipLaunchKernel on
 * the node's fill streams (larger, host sources, compacting transforms, relays). */
int dora_node_fill_paths(dora_node* node, uint64_t* aql_packs, uint64_t* hip_packs);
/* In-place samples (dora_node_send_output_sample) sent by each ordering: after the node stream by
 * a stream operation of the send, or published by the caller's own kernel
 * (dora_sample_fill_ticket).  Either pointer may be NULL. */
int dora_node_sample_paths(dora_node* node, uint64_t* stream_ordered, uint64_t* self_published);
/* The host side of the data plane (new; diagnostics): host-resident sources of 4096 B..2 MiB a
 * device node wrote into its slot with the CPU through the large BAR (the reference's memcpy
 * into its shared-memory sample, arrow_utils.rs:48: no GPU dispatch), and device samples a node
 * without a GPU (DORA_GPU_DEVICE < 0) staged into host memory on receipt (count, bytes): such a
 * receiver gets the reference's host ArrowData (event.rs:35-91); and samples this node put
 * straight into shared memory because every receiver of the output lacks a GPU (sent as the
 * reference's DataMessage::SharedMemory): device arrays <= 1 MiB packed there by the GPU, host
 * sources >= 4096 B copied there by the CPU.  Any pointer may be NULL. */
int dora_node_host_paths(dora_node* node, uint64_t* bar_fills, uint64_t* staged,
                         uint64_t* staged_bytes, uint64_t* host_packs);
/* The outputs of this node the daemon named host-bound in AllNodesReady (new; diagnostics):
 * every receiver is a running local node without a GPU and none is on another machine, so a
 * device node packs them into shared memory (above).  Newline-terminated names, sorted, NUL
 * after the last; *len (if not NULL) = their bytes without the NUL.  buf NULL: only *len;
 * cap < *len + 1: DORA_ERR_INVALID. */
int dora_node_host_bound_outputs(dora_node* node, char* buf, uint64_t cap, uint64_t* len);
/* dora_node_send_output of device arrays keeps the plans of recent sends that read no array
 * bytes (fixed-width and nested arrays with known null counts), keyed by everything such a plan
 * depends on (schema strings and flags, lengths, offsets, null counts, buffer addresses): a
 * sender re-sending the same buffers plans each once.  Sends served from it, plans kept. */
int dora_node_plan_cache_stats(dora_node* node, uint64_t* hits, uint64_t* entries);
/* Cross-GPU edges: an input whose slot lives on another GPU is pulled over xGMI
 * into a local receive slot on first access (dora_event_data / dora_event_array) and the
 * producer's token is returned at once; dora_node_forward pulls it straight into an outgoing
 * slot instead.  The pull is the pack kernel reading the peer's HBM (default) or the copy
 * engines (DORA_GPU_PEER_COPY=sdma).  Counts and bytes of such pulls.  DORA_GPU_EDGE_COPY=1
 * forces the path on same-GPU edges. */
int dora_node_peer_stats(dora_node* node, uint64_t* copies, uint64_t* bytes);
/* 1 -> N fan-out over RCCL (no reference counterpart: the reference has no GPU
 * transport).  A node started with DORA_GPU_FANOUT=rccl asks the daemon at init for a broadcast
 * group per output; the daemon admits one when each receiver of the output runs on its own GPU
 * and none on the producer's.  Sends on such an output broadcast the slot over the group
 * (ncclBroadcast rooted at the producer, on the node stream); receivers post the matching
 * receive into local HBM as the descriptor arrives and hand the input out once it completes.
 * Outputs without a group keep the per-receiver pulls.  Groups formed (as producer / as
 * receiver), samples broadcast / received, bytes received, and the last group error ("" if
 * none). */
int dora_node_bcast_stats(dora_node* node, uint64_t* groups_out, uint64_t* groups_in,
                          uint64_t* sent, uint64_t* received, uint64_t* received_bytes,
                          const char** error);
/* Ranks of this node's broadcast groups as RCCL formed them: the largest group's rank count
 * (producer included; 0 without a group). */
int dora_node_bcast_ranks(dora_node* node, uint64_t* max_ranks);
/* Pack-kernel timing: hipExtLaunchKernel start/stop stamps of every n-th pack launch
 * (dora_node_set_timing_period; 0 = the default, 8). */
int dora_node_set_profiling(dora_node* node, int enable);
int dora_node_set_timing_period(dora_node* node, uint64_t period);
int dora_node_pack_stats(dora_node* node, uint64_t* count, double* total_ms, uint64_t* bytes);
/* (start, stop) of each pack of the last timed region in ms after its earliest start, from the
 * packs' own stamps (below); without a region, of each event-stamped pack in ms after
 * profiling was enabled.  `cap` pairs at most (concurrent packs overlap: their union is the
 * pack busy time). */
int dora_node_pack_intervals(dora_node* node, double* out_ms, size_t cap, size_t* count);
/* Device span of a run of sends: every pack that signals its own fill also stamps its first
 * workgroup's start and its signal time (s_memrealtime, 100 MHz) into its fill flag's line;
 * the span is the earliest start to the latest signal over the packs sent between region_begin
 * and region_end (which waits for them).  Packs that cannot stamp (kernel signal off,
 * compacting transforms) fall back to HIP events: the first pack's start stamp to events
 * recorded after the last pack on every stream.  Packs and sample bytes timed. */
int dora_node_region_begin(dora_node* node);
/* Wait until every fill this node launched (AQL packets, fill streams) and the work on its node
 * stream have completed (new; the node-scoped counterpart of a device synchronise). */
int dora_node_sync(dora_node* node);
/* Record the region's stop events now (after the last send), without waiting; region_end then
 * waits for them.  Lets a caller close its clock before it waits on the device. */
int dora_node_region_mark(dora_node* node);
int dora_node_region_end(dora_node* node, double* span_ms, uint64_t* packs, uint64_t* bytes);
/* Mean host time (µs) per send phase since profiling was (re)enabled: [0] allocate incl.
 * backpressure, [1] pack launch, [2] fill event record / stream sync, [3] descriptor send. */
int dora_node_send_profile(dora_node* node, double* out_us, size_t n_out, uint64_t* count);

/* ------------------------------------------------------------------------------------------ */
/* Daemon — the data-plane part of binaries/daemon (send_out, drop tokens, input closing)     */
/* ------------------------------------------------------------------------------------------ */
typedef struct dora_daemon dora_daemon;
/* Create the dataflow region `shm_name` ("/name").  `spec` lines:
 *   node <id> | output <node> <output> | input <node> <input> <src_node> <src_output> <queue>
 * and, for dataflows spanning machines (InterDaemonEvent, libraries/message/src/
 * daemon_to_daemon.rs:9-21; the reference's `_unstable_deploy.machine`):
 *   dataflow <id>                      shared by the daemons of one dataflow
 *   listen <host> <port>               accept peer daemons (port 0: any free port)
 *   machine <name> <host> <port>       a peer daemon
 *   remote <node> <output> <machine>   this output has receivers under that machine's daemon:
 *                                      its messages are staged to the host and sent there
 *   proxy <node> <gpu>                 <node> runs on another machine and feeds local inputs:
 *                                      the daemon serves it, re-sending its messages locally
 *                                      (device samples on GPU <gpu>, -1: inline host samples) */
int dora_daemon_create(const char* shm_name, const char* spec, size_t ring_bytes,
                       dora_daemon** out);
/* Route until every node is done (0), or timeout_ms elapses (DORA_ERR_TIMEOUT). */
int dora_daemon_run(dora_daemon* daemon, int64_t timeout_ms);
/* Send Event::Stop to every node. */
int dora_daemon_request_stop(dora_daemon* daemon);
int dora_daemon_stats(dora_daemon* daemon, uint64_t* routed, uint64_t* pending_tokens);
/* The port peer daemons connect to (-1: the spec has no `listen` and no `proxy` line). */
int dora_daemon_listen_port(dora_daemon* daemon, int* port);
/* Messages forwarded to other machines, device bytes staged for them, messages received. */
int dora_daemon_remote_stats(dora_daemon* daemon, uint64_t* forwarded, uint64_t* staged_bytes,
                             uint64_t* received);
void dora_daemon_free(dora_daemon* daemon);

#ifdef __cplusplus
}
#endif
#endif /* DORA_GPU_H */
