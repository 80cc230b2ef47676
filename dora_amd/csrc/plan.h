// Internal plan structures shared by plan.cpp and the pack launcher.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "dora_gpu.h"

namespace dora {

struct BufSpec {
  enum Kind { Fixed, Bitmap, Var } kind;
  uint32_t width;  // bytes per element for Fixed
  uint32_t align;  // FixedWidth alignment (arrow-data layout())
};

// At most three buffer specs per Arrow layout: a fixed-capacity list (no heap allocation per
// planned node).
struct SpecList {
  BufSpec v[3];
  size_t n = 0;
  void push_back(const BufSpec& b) { v[n++] = b; }
  size_t size() const { return n; }
  bool empty() const { return n == 0; }
  const BufSpec& operator[](size_t i) const { return v[i]; }
  const BufSpec* begin() const { return v; }
  const BufSpec* end() const { return v + n; }
};

struct Layout {
  SpecList specs;
  bool can_null = true;
  bool offsets_first = false;  // first non-null buffer is an offsets buffer of len+1 entries
};

// ArrowTypeInfo (libraries/message/src/metadata.rs:51-59) with the data type as a signature.
struct TypeInfoNode {
  std::vector<uint8_t> schema;      // serialized DataType (see serialize_schema)
  uint64_t len = 0;
  uint64_t null_count = 0;
  bool has_validity = false;
  std::vector<uint8_t> validity;
  // Node sends of device arrays: the bitmap travels in the sample itself, in the slot's tail
  // past the reference layout's `size` bytes ([validity_off, +validity_len)), instead of inline
  // in the metadata; receivers import it zero-copy and dora_event_type_info restores the
  // inline form on demand.
  bool validity_in_sample = false;
  uint64_t validity_off = 0, validity_len = 0;
  uint64_t offset = 0;
  std::vector<std::pair<uint64_t, uint64_t>> bufs;  // BufferOffset {offset, len}
  std::vector<TypeInfoNode> children;
};

// One copy of `copy_array_into_sample_inner` (arrow_utils.rs:48): src -> sample[dst_off..+len].
// Compacting plans (dora_gpu_plan_compact) also carry transforms: a bit-shifted bitmap slice
// and rebased offsets.
enum SegOp : uint32_t {
  SEG_COPY = 0,      // len bytes verbatim
  SEG_BITSHIFT = 1,  // len bytes of bitmap starting `aux` bits into src (src_len readable bytes)
  SEG_REBASE32 = 2,  // len/4 int32 offsets minus src[0]
  SEG_REBASE64 = 3,  // len/8 int64 offsets minus src[0]
};

struct Segment {
  const void* src;
  uint64_t dst_off;
  uint64_t len;
  uint32_t op = SEG_COPY;
  uint32_t aux = 0;
  uint64_t src_len = 0;
};

// A strided tensor view after canonicalisation (tensor_plan.cpp), in bytes: `nd` dimensions of
// `shape[i]` steps of `stride[i]` bytes (signed, 0 allowed), each addressing a contiguous row of
// `row` bytes (an innermost unit stride folded in; else one element).
constexpr int kMaxTensorDims = 8;
struct StridedView {
  const uint8_t* src;  // element (0, .., 0)
  uint64_t total;      // output bytes
  uint64_t row;
  int nd;              // 0..kMaxTensorDims (0: dense)
  int64_t shape[kMaxTensorDims];
  int64_t stride[kMaxTensorDims];
};

// What a device tensor plan reads (ARROW_DEVICE_ROCM): the view, its element size and the closed
// interval [lo, hi] of byte offsets from `view.src` that any element of it can reach, computed
// without overflow.  A dense view (nd == 0) is read by the plan's one segment, a strided one by
// the gather kernel (gather_device.h); either way the interval is checked against the
// allocation that holds `view.src` before anything is launched (check_device_range).
struct GatherDesc {
  StridedView view;
  uint32_t elem;
  int64_t lo, hi;
};

// A field converted on send (dora_gpu_plan_tensor_cast): `count` elements of the source dtype
// (a DLPack code and width, bfloat16 included) become float16 or float32, through float32 and one
// optional float32 multiplication.  `on` false: the field is sent as it is.
// A quantised field (dora_gpu_plan_tensor_convert) is the same with an integer destination:
// `dst_code` DL_INT or DL_UINT, `dst_bits` 8 or 16, and the product rounded to the nearest
// integer, clamped and moved by `zero_point` (cast_device.h).
struct CastDesc {
  bool on = false;
  uint8_t src_code = 0, src_bits = 0, dst_bits = 0;
  uint32_t has_scale = 0;
  float scale = 1.0f;
  uint64_t count = 0;
  uint8_t dst_code = 2;  // DL_FLOAT: a cast
  int32_t zero_point = 0;
  // The affine step (dora_gpu_plan_tensor_affine): y = float32(x) * S + B, two roundings, with
  // S = scale_tab[c] or the scalar scale or absent, B = bias_tab[c] or the scalar bias or absent,
  // c = (e / inner) % channels for row-major output element e.  A table is `channels` dense
  // float32 words where the values live: read by the CPU while a host plan is built and not kept,
  // read by the launch of a device plan and never on the host (table_reach).
  const uint8_t* scale_tab = nullptr;
  const uint8_t* bias_tab = nullptr;
  uint64_t inner = 1, channels = 1;
  uint32_t has_bias = 0;
  float bias = 0.0f;
  bool quant() const { return on && dst_code != 2; }
  bool affine() const { return on && (has_bias || scale_tab || bias_tab); }
};

// A field reduced on send (dora_gpu_plan_tensor_reduce): the index of the maximum along one axis
// of the source.  `c` candidates per output element, `cstride` bytes apart (signed, 0 allowed),
// of the source dtype (a cast source); `count` output elements of the index type, DL_UINT of 8 or
// 16 bits or DL_INT of 32 or 64.  `on` false: the field is sent as it is.
struct ReduceDesc {
  bool on = false;
  uint8_t src_code = 0, src_bits = 0, idx_code = 0, idx_bits = 0;
  uint64_t c = 0;
  int64_t cstride = 0;
  uint64_t count = 0;
};

// A field resized on send (dora_gpu_plan_tensor_resize): two dimensions of the source take new
// extents by nearest or bilinear taps (resize_device.h).  `nd` dimensions as given: `shape[]` the
// output's extents, `stride[]` the source's byte strides (signed, 0 allowed), `ax[]` the two
// resized dimensions in the order of the caller's axes and `in[]` their source extents; `count`
// output elements of the destination dtype (float16, float32, or uint8, int8, uint16, int16).
// `on` false: the field is sent as it is.
struct ResizeDesc {
  bool on = false;
  uint8_t mode = 0, src_code = 0, src_bits = 0, dst_code = 0, dst_bits = 0;
  int nd = 0;
  int ax[2] = {0, 0};
  int64_t in[2] = {0, 0};
  int64_t shape[kMaxTensorDims] = {0};
  int64_t stride[kMaxTensorDims] = {0};
  uint64_t count = 0;
};

// A field of crops (dora_gpu_plan_tensor_crop): `k` boxes cut from one frame, each brought to one
// size by resize's taps over the box's own clamped extents (crop_device.h).  `rs` describes the
// output as a resize would: `rs.nd` is the frame's dimensions plus the leading one of the K crops
// (shape[0] = K, stride[0] = 0), `rs.ax[]` the two cropped dimensions counted with it, `rs.in[]`
// the frame's extents along them — what a box is clamped to — and `rs.count` all K crops'
// elements.  `boxes`: K dense rows of four int32 words (a_lo, b_lo, a_hi, b_hi) where the values
// live: read by the CPU while a host plan is built, read by the launch of a device plan and never
// on the host (crop_reach).  `on` false: the field is sent as it is.
constexpr uint64_t kMaxCropBoxes = 1u << 20;
struct CropDesc {
  bool on = false;
  ResizeDesc rs;
  const uint8_t* boxes = nullptr;
  uint64_t k = 0;
};

// What a model-input field adds to its resize or crops (dora_gpu_plan_tensor_prep): the resized
// image of extents `inner` placed at `lead` inside an output filled with `fill` (`placed`; resize
// only), and y = r * S + B before the conversion, S = scale_tab[c] or the scalar scale or absent,
// B = bias_tab[c] or the scalar bias or absent, c the output coordinate along `axis` — a dimension
// of the output as ResizeDesc counts them (a crops field's: with K in front).  A table is
// `channels` dense float32 words where the values live: read by the CPU while a host plan is
// built, read by the launch of a device plan and never on the host (table_reach).  `on` false:
// the field's resize or crops is as dora_gpu_plan_tensor_resize / _crop plans it.
struct PrepDesc {
  bool on = false;
  const uint8_t* scale_tab = nullptr;
  const uint8_t* bias_tab = nullptr;
  uint64_t channels = 0;
  int axis = 0;
  uint32_t has_scale = 0, has_bias = 0;
  float scale = 1.0f, bias = 0.0f;
  bool placed = false;
  int64_t inner[2] = {0, 0};
  int64_t lead[2] = {0, 0};
  float fill = 0.0f;
};

// One field of a struct-of-tensors plan (dora_gpu_plan_tensor_struct): the field's view as its
// own tensor plan would describe it (dense: nd == 0), where its row-major values start in the
// sample and how many bytes they are.  Fields follow one another in destination order.
constexpr size_t kMaxStructFields = 8;
struct PlanField {
  std::string name;
  GatherDesc gd;
  uint64_t dst_off;
  uint64_t bytes;
  // a take plan (dora_gpu_plan_tensor_take): `gd.view` is then dimensions 1.. of the field (its
  // total the K taken rows' bytes) and this the byte stride of dimension 0, which keeps an entry
  // of its own whatever its extent or stride; [gd.lo, gd.hi] covers all N source rows
  int64_t stride0 = 0;
  // a cast plan (dora_gpu_plan_tensor_cast), `cast.on`: `gd` is the source view in source bytes
  // (elem the source element size, view.total the source bytes), `bytes` the converted bytes
  CastDesc cast;
  // a reduce plan (dora_gpu_plan_tensor_reduce), `reduce.on`: `gd` is the view of the kept
  // dimensions in source bytes (elem the source element size, view.total the source bytes of one
  // candidate per output element), its [lo, hi] over all `reduce.c` steps of the reduced axis;
  // `bytes` the index bytes
  ReduceDesc reduce;
  // a resize plan (dora_gpu_plan_tensor_resize), `resize.on`: `gd` is the whole source view in
  // source bytes — any element of it may be a tap, so its [lo, hi] is the field's reach — and
  // `resize` the dimensions as given; `bytes` the resized bytes
  ResizeDesc resize;
  // a crop plan (dora_gpu_plan_tensor_crop), `crop.on`: `gd` is the whole frame in source bytes,
  // its [lo, hi] the field's reach as a resized field's is; `bytes` all K crops' bytes
  CropDesc crop;
  // a prep plan (dora_gpu_plan_tensor_prep), `prep.on`: what is added to `resize` or `crop`
  PrepDesc prep;
};

// `bytes` dense bytes of `elem`-byte elements from `src` as a view: what a plan reads of an
// index, a mask or a partition in HBM.
inline GatherDesc dense_reach(const uint8_t* src, uint64_t bytes, uint32_t elem) {
  GatherDesc r{};
  r.view.src = src;
  r.view.total = bytes;
  r.view.row = bytes;
  r.elem = elem;
  r.lo = 0;
  r.hi = static_cast<int64_t>(bytes) - 1;
  return r;
}

// A per-channel table of an affine field in HBM: what check_plan_range holds against the
// allocation of `tab`.
inline GatherDesc table_reach(const uint8_t* tab, uint64_t channels) {
  return dense_reach(tab, 4 * channels, 4);
}

// The boxes of a crops field in HBM: what check_plan_range holds against the allocation of
// `c.boxes`.
inline GatherDesc crop_reach(const CropDesc& c) { return dense_reach(c.boxes, 16 * c.k, 4); }

// The index of a take plan when it lives in HBM: `count` (K) dense words of 4 or 8 bytes at `src`,
// never read on the host; a word outside [0, n) yields a row of zero bytes (gather_device.h
// take::).  take_reach is what check_plan_range holds against the allocation of `src`.
struct TakeDesc {
  const uint8_t* src;
  uint64_t count;  // K: rows taken
  uint64_t n;      // N: rows of the source
  uint32_t wide;   // 0: int32 words, 1: int64
};
inline GatherDesc take_reach(const TakeDesc& t) {
  return dense_reach(t.src, t.count * (t.wide ? 8 : 4), t.wide ? 8 : 4);
}

// The mask of a mask plan (dora_gpu_plan_tensor_mask) when it lives in HBM: `n` dense bytes at
// `src`, any alignment, never read on the host; any non-zero byte selects its row.  `part_words`:
// the B + 1 checked offsets of a host partition, which travel in the plan's prefix into the
// workspace behind the sample, where the launch's scan share reads them (0: no partition, or one
// in HBM).  mask_reach is what check_plan_range holds against the allocation of `src`.
struct MaskDesc {
  const uint8_t* src;
  uint64_t n;
  uint64_t part_words;
};
inline GatherDesc mask_reach(const MaskDesc& m) { return dense_reach(m.src, m.n, 1); }

// The partition of a ragged-batch plan (dora_gpu_plan_tensor_list) when it lives in HBM: `count`
// dense words of 4 or 8 bytes at `src` (B lengths, or B + 1 offsets), never read on the host.  One
// workgroup of the plan's launch scans them into the sample's B + 1 int32 offsets, every one
// clamped to [0, n] (gather_device.h scan::).  scan_reach is what check_plan_range holds against
// the allocation of `src` before anything is launched.
constexpr uint64_t kMaxScanEntries = 1u << 20;
struct ScanDesc {
  const uint8_t* src;
  uint64_t count;   // input words
  uint64_t n;       // rows of the values: the clamp
  uint32_t wide;    // 0: int32 words, 1: int64
  uint32_t offsets; // 0: the words are lengths (sum), 1: offsets (running maximum)
};
inline GatherDesc scan_reach(const ScanDesc& s) {
  return dense_reach(s.src, s.count * (s.wide ? 8 : 4), s.wide ? 8 : 4);
}

// Fill signal written by a pack launch itself (kernels.hip): once every workgroup's stores are
// complete, a system-scope store of `epoch` into `flag` (device view of a host-registered fill
// flag), preceded by the launch's start / signal times into flag[1], flag[2] (the flag must own
// 24 bytes).  `done` = kMaxSignalWgs device words owned by this flag (zeroed once).
struct FillSignal {
  uint64_t* flag;
  uint64_t epoch;
  uint32_t* done;
};
constexpr uint32_t kMaxSignalWgs = 4096;
// Completion-stamp words of a CP-signalled pack inside a timed region (aql.h): workgroup k
// raises word 1 + (k mod kCpStampWgs) to its end time (atomic max), so a grid of any size fits.
// 1024 words: a few arrivals per word.  (16 words made every 40.96 MB pack of 5,000 workgroups
// take 33 instead of 15 us: ~300 system-scope atomics per address serialise at ~60 ns each.)
// The host does not read the words through the BAR (8 KiB of uncached reads per pack, ~57 ms
// for a 200-send region, r04 trace): one AQL dispatch reduces them (aql_stamp_reduce).
constexpr uint32_t kCpStampWgs = 1024;
// Read-signalled packs (aql_kernels.hip dora_aql_pack1r_u4): 16-byte units of the source each
// lane holds in VGPRs at most (62 VGPRs at 12: every workgroup of two 40.96 MB packs resident).
constexpr uint32_t kReadLaneUnits = 12;

// One message of a batch pack (aql.cpp): its copy segments, slot, fill signal, writable bytes.
struct BatchItem {
  const Segment* segs;
  size_t n;
  uint8_t* dst;
  FillSignal sig;
  uint64_t dst_cap;
};

// Launch the pack of `segs` into `dst` on `stream` (kernels.hip).  With `signal`, the last
// launch writes the fill flag itself when it can (`*signalled` says whether it did; compacting
// transforms and host sources leave it to the caller).  `dst_cap`: bytes writable from `dst`
// (0: unknown), which lets the boundary units of the segments be written whole.
int launch_pack(const Segment* segs, size_t n, ArrowDeviceType dev, uint8_t* dst,
                hipStream_t stream, hipEvent_t ev_start, hipEvent_t ev_stop,
                const FillSignal* signal = nullptr, bool* signalled = nullptr,
                uint64_t dst_cap = 0);

// The allocation holding `g.view.src` must be device memory of `device` and contain
// [src + lo, src + hi]; DORA_ERR_INVALID naming both otherwise (kernels.hip).
int check_device_range(const GatherDesc& g, int device);
// The same for everything a device tensor plan reads: its one view, or every field of a struct
// plan (each may sit in an allocation of its own; a refusal names the field).
int check_plan_range(const dora_plan& plan, int device);
// Launch the gather of a strided device view into `dst` (16-byte units of the row-major output,
// write-through stores; nothing at or past dst + g.view.total) on `stream` (kernels.hip); with
// timing events, the dispatch stamps its begin into `ev_start` and its end into `ev_stop`.
int launch_gather(const GatherDesc& g, uint8_t* dst, hipStream_t stream,
                  hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);
// The host-source segments a device plan carries beside what its kernel reads (a ragged batch's
// offsets computed in the plan): copied into `dst` on `stream`, ahead of the pack or gather that
// follows on the same stream.  The bytes are pageable memory of the plan: the runtime has staged
// them when the call returns.
int launch_plan_prefix(const dora_plan& plan, uint8_t* dst, hipStream_t stream);
// Everything a plan's launch kind asks for beyond `segs` (PlanLaunch below; never kSegments):
// launch_gather of its view; one launch over its fields — gather_struct_kernel, with the scan of a
// ragged batch's device partition and by the index of a take, or gather_cast_kernel /
// gather_quant_kernel / gather_affine_kernel for converted fields, gather_reduce_kernel for
// reduced ones, gather_resize_kernel for resized ones or gather_crop_kernel for crops — each field's bytes as launch_gather would write
// them, nothing between fields and nothing at or past the last field's end; for a mask plan the
// two compaction launches and then the fields by the index they wrote, `dst` then holding the
// sample and plan_workspace bytes behind it.  DORA_ERR_INVALID, nothing launched, when a
// converted, reduced, resized or cropped field would not start on a multiple of its destination element
// size.
int launch_plan_gather(const dora_plan& plan, uint8_t* dst, hipStream_t stream,
                       hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr);

// Pack device segments into `dst` (device or mapped host memory) and return once complete,
// waiting on the launch's own fill signal instead of a blocking stream synchronise.
int launch_pack_wait(const Segment* segs, size_t n, uint8_t* dst, hipStream_t stream);

void serialize_type_info(const TypeInfoNode& t, std::vector<uint8_t>& out);
// DataType as a schema tree: str format, str name, i64 flags, u8 has_meta [str meta],
// u32 n_children × Schema, u8 has_dict [Schema].  The top level carries no name and only the
// type-relevant flags (dictionary ordered / map keys sorted).
void serialize_schema(const ArrowSchema* s, bool top, std::vector<uint8_t>& out);
std::string schema_sig(const ArrowSchema* s);
uint64_t metadata_len(const char* meta);
// Everything a plan of (array, schema) depends on when it reads no array bytes, as words: per
// node in walk order the schema's identity and strings (hashed), flags, and the array's length,
// offset, null count, buffer addresses and child counts.  Equal keys give equal plans (a node's
// plan cache, node_internal.h PlanCache).  False when the tree is too large to key.
bool plan_key(const ArrowArray* array, const ArrowSchema* schema, std::vector<uint64_t>& out);

Layout layout_of(const char* format);
inline Layout layout_of(const std::string& format) { return layout_of(format.c_str()); }
int build_plan(const ArrowArray* array, const ArrowSchema* schema, ArrowDeviceType dev,
               dora_plan** out, bool validity_in_sample = false);
// A tensor view in host or device memory (dora_gpu_plan_tensor, tensor_plan.cpp).  A host view is
// one copy segment, over the caller's memory when dense and over the plan's staging buffer when
// strided: a host source, which the send has read when it returns.  A device view is one copy
// segment when dense and a gather when strided; the synchronous send waits until the kernel has
// read it.
int build_tensor_plan(const dora_tensor* tensor, ArrowDeviceType dev, dora_plan** out);
// Named tensors of one leading extent as one Struct message (dora_gpu_plan_tensor_struct).  Host
// fields and all-dense device fields: a multi-segment plan like any other; device fields of which
// any is strided: a gather plan, which goes where a single strided tensor's goes.
int build_tensor_struct_plan(const dora_tensor_field* fields, size_t n, ArrowDeviceType dev,
                             dora_plan** out);
// A ragged batch: the fields' rows cut into lists by a partition (dora_gpu_plan_tensor_list).
// Host values: a multi-segment host plan whose first segment is the offsets; device values: the
// struct plan behind the offsets, which a prefix copy or the launch's scan share writes.
int build_tensor_list_plan(const dora_tensor_list* list, ArrowDeviceType dev, dora_plan** out);
// Rows taken by an index, as a tensor, a record or a ragged batch (dora_gpu_plan_tensor_take).  A
// host index: the taken rows are in the plan's staging buffer, a host plan like any other; a
// device index: a gather plan, which goes where the struct and list plans' gathers go, the index
// one more source its launch reads.
int build_tensor_take_plan(const dora_tensor_take* take, ArrowDeviceType dev, dora_plan** out);
// Rows selected by a mask of N bytes, as one List message (dora_gpu_plan_tensor_mask).  A host
// mask: the compacted rows are in the plan's staging buffer, a host plan like any other; a device
// mask: a gather plan, which goes where the take's goes, its slot allocated with the workspace
// behind the sample.
int build_tensor_mask_plan(const dora_tensor_mask* mask, ArrowDeviceType dev, dora_plan** out);
// Bytes a mask plan's launches need behind the sample (dora_gpu_plan_workspace_size); 0 for
// every other plan (kernels.hip).
uint64_t plan_workspace(const dora_plan& plan);
// Tensors converted to float16 / float32 on send, bare or as a record (dora_gpu_plan_tensor_cast).
// Host values: converted in the plan's staging buffer, a host plan like any other; device values:
// a gather plan whose one launch converts, which goes where the struct plan's goes.
int build_tensor_cast_plan(const dora_tensor_field* fields, size_t n, const dora_tensor_cast* casts,
                           ArrowDeviceType dev, dora_plan** out);
// The same with fields quantised to uint8 / int8 / uint16 / int16 (dora_gpu_plan_tensor_convert).
int build_tensor_convert_plan(const dora_tensor_field* fields, size_t n,
                              const dora_tensor_cast* casts, const dora_tensor_quant* quants,
                              ArrowDeviceType dev, dora_plan** out);
// The same with a per-channel or scalar affine step on converted fields
// (dora_gpu_plan_tensor_affine); `affines` NULL or all zero: build_tensor_convert_plan's plan.
int build_tensor_affine_plan(const dora_tensor_field* fields, size_t n,
                             const dora_tensor_cast* casts, const dora_tensor_quant* quants,
                             const dora_tensor_affine* affines, ArrowDeviceType dev,
                             dora_plan** out);
// Tensors reduced on send, bare or as a record (dora_gpu_plan_tensor_reduce): a field with an
// argmax entry is the index tensor of its maximum along one axis.  Host values: reduced in the
// plan's staging buffer, a host plan like any other; device values: a gather plan whose one launch
// reduces (gather_reduce_kernel).  `reduces` NULL or every op 0: build_tensor_plan's (bare) or
// build_tensor_struct_plan's plan.
int build_tensor_reduce_plan(const dora_tensor_field* fields, size_t n,
                             const dora_tensor_reduce* reduces, ArrowDeviceType dev,
                             dora_plan** out);
// Tensors resized on send, bare or as a record (dora_gpu_plan_tensor_resize): a field with a
// resize entry is the tensor of its two new extents, nearest or bilinear.  Host values: resized
// in the plan's staging buffer, a host plan like any other; device values: a gather plan whose one
// launch resizes (gather_resize_kernel).  `resizes` NULL or every mode 0: build_tensor_plan's
// (bare) or build_tensor_struct_plan's plan.
int build_tensor_resize_plan(const dora_tensor_field* fields, size_t n,
                             const dora_tensor_resize* resizes, ArrowDeviceType dev,
                             dora_plan** out);
// Crops on send, bare or as a record (dora_gpu_plan_tensor_crop): a field with a crop entry is
// the tensor of its K boxes, each cut from the field's frame and brought to one size.  Host
// values: cropped in the plan's staging buffer by the CPU, which reads the boxes; device values: a
// gather plan whose one launch reads the boxes and crops (gather_crop_kernel).  `crops` NULL or
// every mode 0: build_tensor_plan's (bare) or build_tensor_struct_plan's plan.
int build_tensor_crop_plan(const dora_tensor_field* fields, size_t n,
                           const dora_tensor_crop* crops, ArrowDeviceType dev, dora_plan** out);
// Model inputs on send, bare or as a record (dora_gpu_plan_tensor_prep): a resize plan or a crop
// plan whose fields may carry a prep entry each — the image placed inside a filled output (resize
// only) and a per-channel or scalar affine step before the conversion.  Host values: by the CPU in
// the plan's staging buffer; device values: one launch of gather_resize_prep_kernel or
// gather_crop_prep_kernel.  `preps` NULL or all zero: build_tensor_resize_plan's (`crops` NULL)
// or build_tensor_crop_plan's plan.
int build_tensor_prep_plan(const dora_tensor_field* fields, size_t n,
                           const dora_tensor_resize* resizes, const dora_tensor_crop* crops,
                           const dora_tensor_prep* preps, ArrowDeviceType dev, dora_plan** out);
int build_plan_compact(const ArrowArray* array, const ArrowSchema* schema, ArrowDeviceType dev,
                       dora_plan** out);

// What fills a plan's sample, said once: the builder that decides sets it, and the range check,
// the launcher and the send path act on it alone.
enum class PlanLaunch : uint8_t {
  kSegments,  // `segs` (every host plan, dense device plans, empty plans)
  kView,      // launch_gather of `gd`
  kFields,    // gather_struct_kernel over `fields` (+ scan share when scan_on)
  kCast,      // gather_cast_kernel / gather_quant_kernel / gather_affine_kernel over `fields`
  kTaken,     // the taken body over `fields` by `take` (+ scan share when scan_on)
  kMasked,    // count, compact, then the taken body by the workspace's index
  kReduce,    // gather_reduce_kernel over `fields`
  kResize,    // gather_resize_kernel over `fields`
  kCrop,      // gather_crop_kernel over `fields`
  kResizePrep,  // gather_resize_prep_kernel over `fields`: kResize with a model-input step
  kCropPrep     // gather_crop_prep_kernel over `fields`: kCrop with a model-input step
};

// Whether a launch of `k` resizes its fields (`resize.on`) or crops them (`crop.on`), with the
// model-input step or without.
inline bool resizes(PlanLaunch k) { return k == PlanLaunch::kResize || k == PlanLaunch::kResizePrep; }
inline bool crops(PlanLaunch k) { return k == PlanLaunch::kCrop || k == PlanLaunch::kCropPrep; }

// What kind of message a tensor plan is, whichever way its bytes move: reported by the test probes
// (testing.cpp) and read by nothing on the send path.
struct PlanFacts {
  bool list = false;    // a List message (ragged batch, mask)
  bool taken = false;   // rows taken by an index, on the host or by the launch
  bool masked = false;  // rows kept by a mask, on the host or by the launch
  uint64_t take_k = 0, take_n = 0;  // a take: K words over N source rows
  uint32_t take_wide = 0;           // ... of 8 bytes
  uint64_t mask_n = 0;              // a mask: its N elements
};

}  // namespace dora

struct dora_plan {
  ArrowDeviceType dev = ARROW_DEVICE_ROCM;
  bool compact = false;  // built by dora_gpu_plan_compact (carries transform segments)
  uint64_t size = 0;      // required_data_size: the reference sample
  uint64_t ext_size = 0;  // bytes to allocate and fill incl. a validity tail (0: == size)
  bool read_device = false;  // planning read bytes of the array (last offsets, bitmaps)
  std::vector<dora::Segment> segs;
  dora::TypeInfoNode root;
  // tensor plans (tensor_plan.cpp): the row-major copy of a strided host view — the taken, kept or
  // converted rows of a host take, mask or cast — which the plan's segments then read
  std::vector<uint8_t> staged;
  // device tensor plans: everything the plan reads in HBM has its range checked before a launch
  // (check_plan_range), the dense ones that `segs` copies included
  bool dev_tensor = false;
  dora::PlanLaunch launch = dora::PlanLaunch::kSegments;
  // kView, and the dense bare tensor of a kSegments device plan: the one view
  dora::GatherDesc gd{};
  // kFields, kCast, kTaken, kMasked, and the dense fields of a kSegments device plan: one entry
  // per field of the record (a bare tensor's one included)
  std::vector<dora::PlanField> fields;
  dora::TakeDesc take{};  // kTaken: the index in HBM
  dora::MaskDesc mask{};  // kMasked: the mask in HBM
  // ragged-batch plans (tensor_plan.cpp): the int32 offsets computed from a host partition, read
  // by a segment — of `segs` in a host plan, of `prefix` in a device plan, whose other bytes a
  // kernel moves — or, for a partition in HBM, the scan the plan's one launch carries (kFields,
  // kTaken, kMasked; `scan.count` may be 0)
  std::vector<int32_t> list_offsets;
  std::vector<dora::Segment> prefix;
  bool scan_on = false;
  dora::ScanDesc scan{};
  dora::PlanFacts about;
  uint64_t fill_size() const { return ext_size > size ? ext_size : size; }
  // whether the scan share reads the caller's partition in HBM (a mask plan's host partition is
  // in the plan itself: its scan reads the copy the prefix puts into the workspace)
  bool scan_in_hbm() const {
    return scan_on && !(launch == dora::PlanLaunch::kMasked && mask.part_words);
  }
};
