// Planning of a tensor send (dora_gpu_plan_tensor, include/dora_gpu.h): validation of a strided
// view, its canonical form, the nested FixedSizeList type info, the CPU gather of host views
// that are not dense, and for views in device memory — which are never read here — the gather
// descriptor with the interval of offsets the view reaches.
//
// Wire form (no reference counterpart for tensors; the layout is the reference's for the
// equivalent array): shape (d0, .., dk) of T is FixedSizeList<..FixedSizeList<T>[dk]..>[d1] of
// length d0, child fields `item`, nullable.  `copy_array_into_sample` packs such an array as one
// buffer, the row-major values at offset 0, so the plan is one segment of `count * sizeof(T)`
// bytes and the type info a chain of nodes without buffers down to the leaf.
//
// A record of tensors (dora_gpu_plan_tensor_struct) is the Struct array of those columns: the
// same per-tensor work once per field, each leaf at the running offset padded to its element
// size, the struct node without a buffer; host fields as copy segments, device fields as copy
// segments when all are dense and as one multi-gather when any is strided.
//
// A ragged batch (dora_gpu_plan_tensor_list) is the List array over such a tensor or record: the
// int32 offsets first, then the same leaves behind them.  A host partition is checked and turned
// into offsets here; one in HBM is never read, and the plan's one launch scans it.
//
// Selected rows (dora_gpu_plan_tensor_take) are any of the three with the K words of an index in
// place of the leading extent: `values[index]` along dimension 0 without the indexed copy.  The
// same builders lay the message out; a taken field keeps dimension 0 apart from the canonical
// view of the others.  A host index is checked and the rows gathered here; one in HBM is never
// read, and the plan's one launch takes the rows by it (gather_device.h take::).
//
// Converted tensors (dora_gpu_plan_tensor_cast; with quantised fields,
// dora_gpu_plan_tensor_convert) are a tensor or a record laid out for the
// destination dtypes: a cast or quantised field is validated and viewed as its source, and converted on the way
// — by the CPU here for host values, by the plan's one launch for device values (cast_device.h).
// With an affine entry (dora_gpu_plan_tensor_affine) a converted field is taken through
// y = x * S + B first, S and B each a scalar or a per-channel table along one axis: host tables
// are read and checked here, tables in HBM never, their reach kept for check_plan_range.
//
// Reduced tensors (dora_gpu_plan_tensor_reduce) are a tensor or a record in which a field with an
// argmax entry is laid out as the index tensor of its maximum along one axis: the field is
// validated and viewed over its kept dimensions, the reduced axis kept apart as an extent and a
// byte stride, its reach over all the axis' steps — reduced by the CPU here for host values, by
// the plan's one launch for device values (reduce_device.h).
//
// Resized tensors (dora_gpu_plan_tensor_resize) are a tensor or a record in which a field with a
// resize entry is laid out as the tensor of its two new extents and its destination dtype: the
// field is validated and viewed as its whole source, whose reach is the field's since any element
// may be a tap, its dimensions kept as given beside it — resized by the CPU here for host values,
// by the plan's one launch for device values (resize_device.h).
//
// Crops (dora_gpu_plan_tensor_crop) are a tensor or a record in which a field with a crop entry is
// laid out as K tensors of its two new extents under one more leading dimension: the field is
// validated and viewed as a resized frame would be, the boxes as K dense rows of four int32 words
// beside it — read and cropped by the CPU here for host values; for device values never read, their
// 16 * K bytes kept for check_plan_range and the plan's one launch (crop_device.h).
//
// Model inputs (dora_gpu_plan_tensor_prep) are a resize plan or a crop plan whose fields may carry
// a prep entry each: the resized image placed inside a filled output (resize only) and a
// per-channel or scalar affine step before the conversion, the tables validated like an affine
// field's — by the CPU here for host values, by the plan's one launch of
// gather_resize_prep_kernel or gather_crop_prep_kernel for device values.  The wire form never
// depends on the entry.
#include <cstring>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include <cmath>

#include "cast_device.h"
#include "reduce_device.h"
#include "resize_device.h"
#include "crop_device.h"
#include "common.h"
#include "plan.h"

namespace dora {

namespace {

// Row-major walk of the view, an odometer over the dimensions: `row(off, done)` once per row,
// `off` the row's position as an offset from `src` (a negative stride steps below it and back),
// `done` what the rows before it came to, `step` a row, of `total` in all.
template <class Row>
void walk_rows(const StridedView& g, uint64_t total, uint64_t step, Row&& row) {
  int64_t idx[kMaxTensorDims] = {0};
  int64_t off = 0;
  for (uint64_t done = 0; done < total; done += step) {
    row(off, done);
    for (int k = g.nd - 1; k >= 0; --k) {
      off += g.stride[k];
      if (++idx[k] < g.shape[k]) break;
      off -= g.stride[k] * g.shape[k];
      idx[k] = 0;
    }
  }
}

// The view's bytes in row-major order: one memcpy per row.
void gather_host(const StridedView& g, uint8_t* dst) {
  walk_rows(g, g.total, g.row,
            [&](int64_t off, uint64_t done) { std::memcpy(dst + done, g.src + off, g.row); });
}

// `f(K)` with the source kind `kind` (gather::cast::src_kind, never -1 here) as the compile-time
// constant `decltype(K)::value`.
template <class F>
void with_src_kind(int kind, F&& f) {
  namespace gc = gather::cast;
  switch (kind) {
    case gc::kU8: f(std::integral_constant<uint32_t, gc::kU8>{}); break;
    case gc::kI8: f(std::integral_constant<uint32_t, gc::kI8>{}); break;
    case gc::kU16: f(std::integral_constant<uint32_t, gc::kU16>{}); break;
    case gc::kI16: f(std::integral_constant<uint32_t, gc::kI16>{}); break;
    case gc::kF16: f(std::integral_constant<uint32_t, gc::kF16>{}); break;
    case gc::kBF16: f(std::integral_constant<uint32_t, gc::kBF16>{}); break;
    default: f(std::integral_constant<uint32_t, gc::kF32>{}); break;
  }
}

// DLPack type codes (dlpack.h, DLDataTypeCode)
enum { DL_INT = 0, DL_UINT = 1, DL_FLOAT = 2, DL_BFLOAT = 4, DL_COMPLEX = 5, DL_BOOL = 6 };

// Arrow C format of a leaf of int, uint or float `code` and `bits`; NULL when Arrow has none.
const char* leaf_of(unsigned code, unsigned bits) {
  if (code == DL_INT || code == DL_UINT) {
    const bool u = code == DL_UINT;
    switch (bits) {
      case 8: return u ? "C" : "c";
      case 16: return u ? "S" : "s";
      case 32: return u ? "I" : "i";
      case 64: return u ? "L" : "l";
    }
  } else if (code == DL_FLOAT) {
    switch (bits) {
      case 16: return "e";
      case 32: return "f";
      case 64: return "g";
    }
  }
  return nullptr;
}

// Arrow C format of an accepted dtype; NULL after recording why it is refused.
const char* leaf_format(const dora_tensor& t) {
  const unsigned code = t.dtype_code, bits = t.dtype_bits, lanes = t.dtype_lanes;
  if (lanes != 1) {
    set_error("tensor dtype (code %u, %u bits) has %u lanes: only lanes == 1 is supported", code,
              bits, lanes);
    return nullptr;
  }
  if (code == DL_BOOL) {
    set_error("tensor dtype bool is not supported: Arrow's Boolean is a bitmap (send a view as "
              "uint8)");
    return nullptr;
  }
  if (code == DL_BFLOAT) {
    set_error("tensor dtype bfloat%u is not supported: Arrow has no bfloat16 (send a view as "
              "uint16)", bits);
    return nullptr;
  }
  if (code == DL_COMPLEX) {
    set_error("tensor dtype complex%u is not supported: Arrow has no complex type (send a view "
              "as pairs of floats)", bits);
    return nullptr;
  }
  if (const char* leaf = leaf_of(code, bits)) return leaf;
  set_error("tensor dtype (code %u, %u bits) is not supported: int and uint of 8/16/32/64 bits "
            "and float of 16/32/64 bits are", code, bits);
  return nullptr;
}

struct Dim {
  int64_t n, s;  // extent, stride in bytes
};

// The closed interval [lo, hi] of byte offsets from element (0, .., 0) that the view reaches: lo
// the sum of the negative (n - 1) * stride terms, hi the positive ones plus the row's last byte.
// False when a product or a sum leaves int64: a device view's strides are not trusted, since an
// out-of-range read on the GPU is a machine-wide event.
bool reach(const StridedView& g, int64_t* lo, int64_t* hi) {
  int64_t l = 0, h = 0;
  if (g.row == 0 || g.row - 1 > uint64_t(INT64_MAX)) return false;
  h = static_cast<int64_t>(g.row - 1);
  for (int i = 0; i < g.nd; ++i) {
    int64_t span;
    if (__builtin_mul_overflow(g.shape[i] - 1, g.stride[i], &span)) return false;
    if (__builtin_add_overflow(span < 0 ? l : h, span, span < 0 ? &l : &h)) return false;
  }
  // every offset in between must be representable from either end
  int64_t width;
  if (__builtin_sub_overflow(h, l, &width)) return false;
  *lo = l;
  *hi = h;
  return true;
}

// The Arrow C schema of a tensor of `leaf` and shape[0..ndim): the chain of fixed-size lists
// down to the leaf, child fields `item`, nullable; the head carries `name` (a struct's field) or
// none.  The nodes point into the vectors, which are sized once.
struct TypeChain {
  std::vector<ArrowSchema> sch;
  std::vector<ArrowSchema*> child;
  std::vector<std::string> fmt;
  TypeChain(const char* leaf, const int64_t* shape, int ndim, const char* name)
      : sch(static_cast<size_t>(ndim)), child(static_cast<size_t>(ndim), nullptr),
        fmt(static_cast<size_t>(ndim)) {
    for (int i = 0; i < ndim; ++i) {
      ArrowSchema& s = sch[size_t(i)];
      std::memset(&s, 0, sizeof(s));
      fmt[size_t(i)] = i + 1 < ndim ? "+w:" + std::to_string(shape[i + 1]) : std::string(leaf);
      s.format = fmt[size_t(i)].c_str();
      s.name = i ? "item" : name;
      s.flags = i || name[0] ? ARROW_FLAG_NULLABLE : 0;
      if (i + 1 < ndim) {
        child[size_t(i)] = &sch[size_t(i) + 1];
        s.children = &child[size_t(i)];
        s.n_children = 1;
      }
    }
  }
  TypeChain(const TypeChain&) = delete;
  TypeChain& operator=(const TypeChain&) = delete;
};

// The type info chain of shape[0..ndim) over a leaf of `bytes` bytes at sample offset `off`, as
// build_plan's walk serialises the equivalent array: every node carries its own type as a
// top-level schema.
void tensor_type_info(const TypeChain& c, const int64_t* shape, int ndim, uint64_t off,
                      uint64_t bytes, TypeInfoNode& root) {
  TypeInfoNode* node = &root;
  uint64_t len = 1;
  for (int i = 0; i < ndim; ++i) {
    len *= static_cast<uint64_t>(shape[i]);
    serialize_schema(&c.sch[size_t(i)], true, node->schema);
    node->len = len;
    if (i + 1 < ndim) {
      node->children.emplace_back();
      node = &node->children.back();
    } else {
      node->bufs.push_back({off, bytes});
    }
  }
}

// What planning one tensor yields, for a message of its own and for a field of a struct alike:
// the accepted leaf format, the byte count, and — unless it is empty — the canonical view over
// `data + byte_offset` (nd == 0: dense) with, for device memory, the interval it reaches.
struct TensorView {
  const char* leaf = nullptr;
  uint64_t bytes = 0;
  GatherDesc gd{};
};

// Validation, canonical view and reach of `t`; the failure recorded otherwise.
// (`need_data` false: a NULL `data` passes, for a view that will never be read)
int describe_tensor(const dora_tensor* t, ArrowDeviceType dev, TensorView& out,
                    bool need_data = true) {
  if (!t) return fail(DORA_ERR_INVALID, "tensor is NULL");
  const char* leaf = leaf_format(*t);
  if (!leaf) return DORA_ERR_UNSUPPORTED;
  const int64_t elem = t->dtype_bits / 8;
  if (t->ndim < 1) return fail(DORA_ERR_INVALID, "tensor has %d dimensions (at least 1)", t->ndim);
  if (!t->shape) return fail(DORA_ERR_INVALID, "tensor shape is NULL");
  uint64_t inner = 1;  // elements per step of the first dimension
  for (int i = 0; i < t->ndim; ++i) {
    if (t->shape[i] < 0)
      return fail(DORA_ERR_INVALID, "tensor extent %lld in dimension %d is negative",
                  static_cast<long long>(t->shape[i]), i);
    if (i && t->shape[i] == 0)
      return fail(DORA_ERR_INVALID, "tensor extent 0 in dimension %d (only the first may be 0: a "
                  "fixed-size list of 0 values has no length to recover)", i);
    if (i && __builtin_mul_overflow(inner, static_cast<uint64_t>(t->shape[i]), &inner))
      return fail(DORA_ERR_INVALID, "tensor byte count overflows 64 bits");
  }
  uint64_t count = 0, bytes = 0;
  if (__builtin_mul_overflow(inner, static_cast<uint64_t>(t->shape[0]), &count) ||
      __builtin_mul_overflow(count, static_cast<uint64_t>(elem), &bytes) || bytes >> 63)
    return fail(DORA_ERR_INVALID, "tensor byte count overflows 64 bits");
  if (!t->data && count && need_data) return fail(DORA_ERR_INVALID, "tensor data is NULL");

  // canonical view: no extents of 1, mergeable neighbours merged
  Dim dims[kMaxTensorDims];
  size_t nd = 0;
  {
    int64_t rm = elem;  // row-major stride when strides is NULL
    for (int i = t->ndim - 1; i >= 0; --i) {  // innermost first: merged into dims[0]
      int64_t sb;
      if (t->strides) {
        if (__builtin_mul_overflow(t->strides[i], elem, &sb))
          return fail(DORA_ERR_INVALID, "tensor stride %d overflows 64 bits", i);
      } else {
        sb = rm;
        rm *= t->shape[i] ? t->shape[i] : 1;
      }
      if (t->shape[i] == 1 || !count) continue;
      const Dim d{t->shape[i], sb};
      int64_t span;  // bytes one step of this dimension must cover to merge with the next inner
      if (nd && !__builtin_mul_overflow(dims[0].n, dims[0].s, &span) && d.s == span) {
        dims[0].n *= d.n;
      } else {
        if (nd == size_t(kMaxTensorDims))
          return fail(DORA_ERR_UNSUPPORTED,
                      "tensor view has more than %d dimensions after merging", kMaxTensorDims);
        for (size_t k = nd; k > 0; --k) dims[k] = dims[k - 1];
        dims[0] = d;
        ++nd;
      }
    }
  }
  out.leaf = leaf;
  out.bytes = bytes;
  if (bytes == 0) return DORA_OK;
  // an innermost unit stride folds into a row of bytes
  uint64_t row = static_cast<uint64_t>(elem);
  if (nd && dims[nd - 1].s == elem) {
    row = static_cast<uint64_t>(dims[nd - 1].n) * static_cast<uint64_t>(elem);
    --nd;
  }
  StridedView& g = out.gd.view;
  g.src = static_cast<const uint8_t*>(t->data) + t->byte_offset;
  g.total = bytes;
  g.row = row;
  g.nd = static_cast<int>(nd);
  for (size_t i = 0; i < nd; ++i) {
    g.shape[i] = dims[i].n;
    g.stride[i] = dims[i].s;
  }
  out.gd.elem = static_cast<uint32_t>(elem);
  // device strides are not trusted; a host view's reach is its producer's word
  if (dev == ARROW_DEVICE_ROCM && !reach(g, &out.gd.lo, &out.gd.hi))
    return fail(DORA_ERR_INVALID, "tensor view's reach overflows 64 bits (extent - 1 times "
                "stride, summed over its dimensions)");
  return DORA_OK;
}

// The reach of `g` over `steps` more positions `stride` bytes apart along one more axis (the
// rows of a take, the candidates of a reduction); refused when it leaves int64, as `reach` does.
int extend_reach(GatherDesc& g, int64_t steps, int64_t stride) {
  int64_t span, width;
  if (__builtin_mul_overflow(steps, stride, &span) ||
      __builtin_add_overflow(span < 0 ? g.lo : g.hi, span, span < 0 ? &g.lo : &g.hi) ||
      __builtin_sub_overflow(g.hi, g.lo, &width))
    return fail(DORA_ERR_INVALID, "tensor view's reach overflows 64 bits (extent - 1 times "
                "stride, summed over its dimensions)");
  return DORA_OK;
}

// A field of a take (dora_gpu_plan_tensor_take): `k` rows taken along dimension 0 of `t`.
// Dimensions 1.. are described as a tensor of their own — validated, canonicalised, an innermost
// unit stride folded into the row — while dimension 0 keeps its entry, extent N and `*stride0`
// bytes, whatever they are.  out.bytes and the view's total are the k taken rows'; a device
// field's reach covers all N source rows (nothing is read when N == 0).
int describe_taken(const dora_tensor& t, ArrowDeviceType dev, uint64_t k, TensorView& out,
                   int64_t* stride0) {
  if (t.ndim < 1) return fail(DORA_ERR_INVALID, "tensor has %d dimensions (at least 1)", t.ndim);
  if (!t.shape) return fail(DORA_ERR_INVALID, "tensor shape is NULL");
  for (int i = 0; i < t.ndim; ++i) {
    if (t.shape[i] < 0)
      return fail(DORA_ERR_INVALID, "tensor extent %lld in dimension %d is negative",
                  static_cast<long long>(t.shape[i]), i);
    if (i && t.shape[i] == 0)
      return fail(DORA_ERR_INVALID, "tensor extent 0 in dimension %d (only the first may be 0: a "
                  "fixed-size list of 0 values has no length to recover)", i);
  }
  const int64_t rows = t.shape[0];
  static const int64_t kOne = 1;
  dora_tensor in = t;  // dimensions 1.., or one element
  in.ndim = t.ndim > 1 ? t.ndim - 1 : 1;
  in.shape = t.ndim > 1 ? t.shape + 1 : &kOne;
  in.strides = t.ndim > 1 && t.strides ? t.strides + 1 : nullptr;
  const int rc = describe_tensor(&in, dev, out, rows != 0);
  if (rc != DORA_OK) return rc;
  const int64_t elem = t.dtype_bits / 8;
  const uint64_t inner = out.bytes;  // bytes per taken row, >= elem
  if (t.strides) {
    if (__builtin_mul_overflow(t.strides[0], elem, stride0))
      return fail(DORA_ERR_INVALID, "tensor stride 0 overflows 64 bits");
  } else {
    *stride0 = static_cast<int64_t>(inner);
  }
  if (__builtin_mul_overflow(inner, k, &out.bytes) || out.bytes >> 63)
    return fail(DORA_ERR_INVALID, "tensor byte count overflows 64 bits");
  if (out.bytes == 0) return DORA_OK;
  out.gd.view.total = out.bytes;
  if (dev != ARROW_DEVICE_ROCM) return DORA_OK;
  if (rows == 0) {  // k rows of zeros: no byte of the field is reachable
    out.gd.lo = 0;
    out.gd.hi = -1;
    return DORA_OK;
  }
  return extend_reach(out.gd, rows - 1, *stride0);
}

// A dtype by name, for refusals.
std::string dtype_name(unsigned code, unsigned bits, unsigned lanes) {
  static const char* const kNames[] = {"int", "uint", "float", nullptr, "bfloat", "complex", "bool"};
  std::string s = code < 7 && kNames[code] ? kNames[code] : "code" + std::to_string(code) + "_";
  if (code != DL_BOOL) s += std::to_string(bits);
  if (lanes != 1) s += "x" + std::to_string(lanes);
  return s;
}

// Whether an op (`noun`: cast, quantise, argmax, resize) reads elements of `t`'s dtype; the
// refusal naming it otherwise.  Every op ranks it among its entry's own refusals, so it stands
// apart from describe_source.
int check_source_dtype(const dora_tensor& t, const char* noun) {
  if (t.dtype_lanes == 1 && gather::cast::src_kind(t.dtype_code, t.dtype_bits) >= 0)
    return DORA_OK;
  return fail(DORA_ERR_UNSUPPORTED, "%s source dtype %s is not supported: uint8, int8, uint16, "
              "int16, float16, bfloat16 and float32 are", noun,
              dtype_name(t.dtype_code, t.dtype_bits, t.dtype_lanes).c_str());
}

// The view `v` of what an op (`noun`) reads of `t`, a tensor of an accepted source dtype: any
// accepted dtype of the source's width describes it (Arrow has no bfloat16, and the leaf is the
// destination's anyway), and the op's loads are whole elements.
int describe_source(const dora_tensor& t, const char* noun, ArrowDeviceType dev, TensorView& v) {
  dora_tensor src = t;
  src.dtype_code = DL_UINT;
  const int rc = describe_tensor(&src, dev, v);
  if (rc != DORA_OK) return rc;
  const unsigned ss = t.dtype_bits / 8u;
  if (v.bytes && (reinterpret_cast<uintptr_t>(v.gd.view.src) & (ss - 1)))
    return fail(DORA_ERR_INVALID, "%s source data %p (data + byte_offset) is not a multiple of "
                "its %u-byte elements", noun, static_cast<const void*>(v.gd.view.src), ss);
  return DORA_OK;
}

// Whether `c` converts `t` at all: dtype_bits == 0 and a destination equal to the source without
// a scale do not.  The cast's own refusals otherwise (UNSUPPORTED naming the dtype, INVALID).
// (`force`: the field has an affine entry, so a destination equal to the source converts too)
int describe_cast(const dora_tensor& t, const dora_tensor_cast& c, CastDesc& out,
                  bool force = false) {
  out = CastDesc{};
  if (c.dtype_bits == 0) return DORA_OK;
  if (c.dtype_code != DL_FLOAT || (c.dtype_bits != 16 && c.dtype_bits != 32))
    return fail(DORA_ERR_UNSUPPORTED, "cast destination dtype %s is not supported: float16 and "
                "float32 are (8- and 16-bit integers are quantised: "
                "dora_gpu_plan_tensor_convert)",
                dtype_name(c.dtype_code, c.dtype_bits, 1).c_str());
  if (c.has_scale && !std::isfinite(c.scale))
    return fail(DORA_ERR_INVALID, "cast scale %f is not finite", static_cast<double>(c.scale));
  if (const int rc = check_source_dtype(t, "cast"); rc != DORA_OK) return rc;
  if (!c.has_scale && !force && t.dtype_code == c.dtype_code && t.dtype_bits == c.dtype_bits)
    return DORA_OK;
  out.on = true;
  out.src_code = t.dtype_code;
  out.src_bits = t.dtype_bits;
  out.dst_bits = c.dtype_bits;
  out.has_scale = c.has_scale ? 1 : 0;
  out.scale = c.has_scale ? c.scale : 1.0f;
  return DORA_OK;
}

// What quantises `t` (dora_gpu_plan_tensor_convert): dtype_bits == 0 does not; any other entry
// does, whatever the source dtype (no identity rule).  UNSUPPORTED naming the dtype, INVALID.
int describe_quant(const dora_tensor& t, const dora_tensor_quant& q, CastDesc& out) {
  out = CastDesc{};
  if (q.dtype_bits == 0) return DORA_OK;
  const int kind = gather::cast::dst_kind(q.dtype_code, q.dtype_bits);
  if (kind < 0)
    return fail(DORA_ERR_UNSUPPORTED, "quantise destination dtype %s is not supported: uint8, "
                "int8, uint16 and int16 are",
                dtype_name(q.dtype_code, q.dtype_bits, 1).c_str());
  const int32_t lo = gather::cast::dst_lo(static_cast<uint32_t>(kind)),
                hi = gather::cast::dst_hi(static_cast<uint32_t>(kind));
  if (q.zero_point < lo || q.zero_point > hi)
    return fail(DORA_ERR_INVALID, "quantise zero point %d is outside the range [%d, %d] of %s",
                q.zero_point, lo, hi, dtype_name(q.dtype_code, q.dtype_bits, 1).c_str());
  if (q.has_scale && !std::isfinite(q.scale))
    return fail(DORA_ERR_INVALID, "quantise scale %f is not finite", static_cast<double>(q.scale));
  if (const int rc = check_source_dtype(t, "quantise"); rc != DORA_OK) return rc;
  out.on = true;
  out.src_code = t.dtype_code;
  out.src_bits = t.dtype_bits;
  out.dst_code = q.dtype_code;
  out.dst_bits = q.dtype_bits;
  out.has_scale = q.has_scale ? 1 : 0;
  out.scale = q.has_scale ? q.scale : 1.0f;
  out.zero_point = q.zero_point;
  return DORA_OK;
}

// What converts field `t`: its cast entry, its quantise entry, or neither (`c`, `q` may be NULL).
// A field with both is INVALID.
int describe_convert(const dora_tensor& t, const dora_tensor_cast* c, const dora_tensor_quant* q,
                     CastDesc& out, bool force = false) {
  out = CastDesc{};
  if (c && q && c->dtype_bits && q->dtype_bits)
    return fail(DORA_ERR_INVALID, "the field is both cast and quantised: one conversion a field");
  if (q && q->dtype_bits) return describe_quant(t, *q, out);
  return c ? describe_cast(t, *c, out, force) : DORA_OK;
}

// Whether an affine entry adds anything to its field (all zero: it does not).
bool affine_on(const dora_tensor_affine& a) { return a.scale || a.bias || a.has_bias; }

// A per-channel table of the affine step over axis `axis` of `t`: 1-D dense float32 of
// shape[axis] words on a multiple of 4, where the values live.  A host table is read here and
// every value must be finite; one in HBM is never read.
int describe_table(const dora_tensor& tab, const char* what, const dora_tensor& t, int axis,
                   ArrowDeviceType dev, const uint8_t** out) {
  if (tab.dtype_code != DL_FLOAT || tab.dtype_bits != 32 || tab.dtype_lanes != 1)
    return fail(DORA_ERR_UNSUPPORTED, "%s table dtype %s is not supported: float32 is", what,
                dtype_name(tab.dtype_code, tab.dtype_bits, tab.dtype_lanes).c_str());
  if (tab.ndim != 1 || !tab.shape)
    return fail(DORA_ERR_INVALID, "%s table has %d dimensions (a 1-D tensor of the %lld values "
                "along axis %d)", what, tab.ndim, static_cast<long long>(t.shape[axis]), axis);
  if (tab.shape[0] != t.shape[axis])
    return fail(DORA_ERR_INVALID, "%s table has %lld elements, the tensor has %lld along axis %d",
                what, static_cast<long long>(tab.shape[0]), static_cast<long long>(t.shape[axis]),
                axis);
  if (tab.strides && tab.shape[0] > 1 && tab.strides[0] != 1)
    return fail(DORA_ERR_INVALID, "%s table stride %lld: the table is dense", what,
                static_cast<long long>(tab.strides[0]));
  if (!tab.data && tab.shape[0]) return fail(DORA_ERR_INVALID, "%s table data is NULL", what);
  const uint8_t* p = static_cast<const uint8_t*>(tab.data) + tab.byte_offset;
  if (reinterpret_cast<uintptr_t>(p) & 3)
    return fail(DORA_ERR_INVALID, "%s table data %p (data + byte_offset) is not a multiple of 4",
                what, static_cast<const void*>(p));
  if (dev != ARROW_DEVICE_ROCM) {
    for (int64_t i = 0; i < tab.shape[0]; ++i) {
      float v;
      std::memcpy(&v, p + 4 * i, 4);
      if (!std::isfinite(v))
        return fail(DORA_ERR_INVALID, "%s table: value %lld is %f, not finite", what,
                    static_cast<long long>(i), static_cast<double>(v));
    }
  }
  *out = p;
  return DORA_OK;
}

// The affine step of a field `t` (validated) that `cd` converts or not, by the entry `af`
// (affine_on): its refusals, else `cd` with the tables, the axis' geometry and the bias.
int describe_affine(const dora_tensor& t, ArrowDeviceType dev, const dora_tensor_affine& af,
                    CastDesc& cd) {
  if (!cd.on)
    return fail(DORA_ERR_INVALID, "an affine entry on a field that is neither cast nor quantised "
                "(give it a cast to its own dtype)");
  if (af.scale && cd.has_scale)
    return fail(DORA_ERR_INVALID, "a scale table together with a scalar scale (has_scale): one "
                "scale a field");
  if (af.bias && af.has_bias)
    return fail(DORA_ERR_INVALID, "a bias table together with a scalar bias (has_bias): one bias "
                "a field");
  if (af.scale || af.bias) {
    if (af.axis < 0 || af.axis >= t.ndim)
      return fail(DORA_ERR_INVALID, "affine axis %d is outside the tensor's %d dimensions",
                  af.axis, t.ndim);
    int rc = af.scale ? describe_table(*af.scale, "scale", t, af.axis, dev, &cd.scale_tab)
                      : DORA_OK;
    if (rc == DORA_OK && af.bias)
      rc = describe_table(*af.bias, "bias", t, af.axis, dev, &cd.bias_tab);
    if (rc != DORA_OK) return rc;
    cd.channels = static_cast<uint64_t>(t.shape[af.axis]);
    cd.inner = 1;  // (a factor of the element count, which fits 64 bits)
    for (int i = af.axis + 1; i < t.ndim; ++i) cd.inner *= static_cast<uint64_t>(t.shape[i]);
  }
  if (af.has_bias && !std::isfinite(af.bias_value))
    return fail(DORA_ERR_INVALID, "affine bias %f is not finite",
                static_cast<double>(af.bias_value));
  cd.has_bias = af.has_bias ? 1 : 0;
  cd.bias = af.has_bias ? af.bias_value : 0.0f;
  return DORA_OK;
}

// The CPU's conversion of a cast field: the view's rows in row-major order, each element through
// the integer routines of cast_device.h, into `dst` (any alignment).
// `ch`: the channel of the row's first element under an affine step, stepped on to that of the
// element behind the row (the rows come in output order, so one Chan walks the whole field).
template <uint32_t K>
void cast_row(const uint8_t* src, uint64_t n, const CastDesc& c, uint8_t* dst,
              gather::cast::Chan& ch) {
  constexpr int S = gather::cast::kSize<K>;
  const gather::cast::HostCvt cv;
  const bool quant = c.quant();
  const int dk = quant ? gather::cast::dst_kind(c.dst_code, c.dst_bits) : 0;
  const int32_t lo = quant ? gather::cast::dst_lo(uint32_t(dk)) - c.zero_point : 0,
                hi = quant ? gather::cast::dst_hi(uint32_t(dk)) - c.zero_point : 0;
  const bool tables = c.scale_tab || c.bias_tab;
  auto word = [&](const uint8_t* tab) {
    float v;
    std::memcpy(&v, tab + 4 * ch.c, 4);
    return v;
  };
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t raw = 0;
    std::memcpy(&raw, src + i * S, S);  // (little-endian)
    float y = cv.to_f32<K>(raw);
    if (c.scale_tab) y = cv.mul(y, word(c.scale_tab));
    else if (c.has_scale) y = cv.mul(y, c.scale);
    if (c.bias_tab) y = cv.add(y, word(c.bias_tab));
    else if (c.has_bias) y = cv.add(y, c.bias);
    if (tables) gather::cast::chan_next(c.inner, c.channels, ch);
    if (quant) {
      const uint32_t q = static_cast<uint32_t>(cv.to_int(y, lo, hi, c.zero_point));
      std::memcpy(dst + (c.dst_bits / 8u) * i, &q, c.dst_bits / 8u);  // (little-endian)
    } else if (c.dst_bits == 16) {
      const uint16_t h = static_cast<uint16_t>(cv.to_f16(y));
      std::memcpy(dst + 2 * i, &h, 2);
    } else {
      std::memcpy(dst + 4 * i, &y, 4);
    }
  }
}

void cast_host(const StridedView& g, const CastDesc& c, uint8_t* dst) {
  namespace gc = gather::cast;
  const uint64_t ss = c.src_bits / 8u, ds = c.dst_bits / 8u, n = g.row / ss;
  gc::Chan ch{0, 0};
  with_src_kind(gc::src_kind(c.src_code, c.src_bits), [&](auto K) {
    walk_rows(g, c.count, n, [&](int64_t off, uint64_t done) {
      cast_row<decltype(K)::value>(g.src + off, n, c, dst + done * ds, ch);
    });
  });
}

// The index of the maximum of the `c` candidates `cstride` bytes apart from `src`, of type K:
// reduce_device.h's rule, the first NaN or else the first maximum.
template <uint32_t K>
uint64_t argmax_at(const uint8_t* src, uint64_t c, int64_t cstride) {
  constexpr int S = gather::cast::kSize<K>;
  const gather::cast::HostCvt cv;
  auto at = [&](uint64_t i) {
    uint32_t raw = 0;
    std::memcpy(&raw, src + static_cast<int64_t>(i) * cstride, S);  // (little-endian)
    return cv.to_f32<K>(raw);
  };
  float best = at(0);
  uint64_t bi = 0;
  for (uint64_t i = 1; i < c; ++i) {
    const float v = at(i);
    if (gather::reduce::better(v, best)) {
      best = v;
      bi = i;
    }
  }
  return bi;
}

// The CPU's reduction of a reduce field: the elements of the view of the kept dimensions in
// row-major order, each the argmax of its candidates, into `dst` (any alignment).
void reduce_host(const StridedView& g, const ReduceDesc& r, uint8_t* dst) {
  namespace gc = gather::cast;
  const uint64_t ss = r.src_bits / 8u, ds = r.idx_bits / 8u, n = g.row / ss;
  with_src_kind(gc::src_kind(r.src_code, r.src_bits), [&](auto K) {
    walk_rows(g, r.count, n, [&](int64_t off, uint64_t done) {
      for (uint64_t i = 0; i < n; ++i) {
        const uint64_t w = argmax_at<decltype(K)::value>(
            g.src + off + static_cast<int64_t>(i * ss), r.c, r.cstride);
        std::memcpy(dst + (done + i) * ds, &w, ds);  // (little-endian)
      }
    });
  });
}

// What reduces `t` (dora_gpu_plan_tensor_reduce, `r.op` != 0): the entry's and the tensor's
// refusals, else `rd`, the view `v` of the kept dimensions — validated and canonicalised as a
// tensor of its own, its reach over all C steps of the reduced axis, its leaf and byte count the
// index tensor's — and `kshape`, the shape of the message.
int describe_reduce(const dora_tensor& t, const dora_tensor_reduce& r, ArrowDeviceType dev,
                    ReduceDesc& rd, TensorView& v, std::vector<int64_t>& kshape) {
  rd = ReduceDesc{};
  if (r.op != DORA_REDUCE_ARGMAX)
    return fail(DORA_ERR_UNSUPPORTED, "reduce op %u is not supported: DORA_REDUCE_ARGMAX (%u) is",
                r.op, DORA_REDUCE_ARGMAX);
  const unsigned ib = gather::reduce::index_size(r.dtype_code, r.dtype_bits);
  if (!ib)
    return fail(DORA_ERR_UNSUPPORTED, "argmax index dtype %s is not supported: uint8, uint16, "
                "int32 and int64 are", dtype_name(r.dtype_code, r.dtype_bits, 1).c_str());
  if (const int rc = check_source_dtype(t, "argmax"); rc != DORA_OK) return rc;
  if (t.ndim < 2)
    return fail(DORA_ERR_INVALID, "argmax of a tensor of %d dimensions (at least 2: the reduced "
                "axis and one that is kept)", t.ndim);
  if (!t.shape) return fail(DORA_ERR_INVALID, "tensor shape is NULL");
  if (r.axis < 0 || r.axis >= t.ndim)
    return fail(DORA_ERR_INVALID, "argmax axis %d is outside the tensor's %d dimensions", r.axis,
                t.ndim);
  const int64_t c = t.shape[r.axis];
  if (c < 0)
    return fail(DORA_ERR_INVALID, "tensor extent %lld in dimension %d is negative",
                static_cast<long long>(c), r.axis);
  if (c == 0)
    return fail(DORA_ERR_INVALID, "argmax along axis %d of extent 0: there is no candidate",
                r.axis);
  if ((r.dtype_bits == 8 && c > 256) || (r.dtype_bits == 16 && c > 65536) ||
      (r.dtype_bits == 32 && c > (int64_t(1) << 31)))
    return fail(DORA_ERR_INVALID, "argmax along axis %d of extent %lld: the index %lld does not "
                "fit %s", r.axis, static_cast<long long>(c), static_cast<long long>(c - 1),
                dtype_name(r.dtype_code, r.dtype_bits, 1).c_str());
  // the strides in elements, the caller's or row-major
  std::vector<int64_t> strides(static_cast<size_t>(t.ndim));
  int64_t rm = 1;
  for (int i = t.ndim - 1; i >= 0; --i) {
    strides[size_t(i)] = t.strides ? t.strides[i] : rm;
    if (!t.strides && __builtin_mul_overflow(rm, t.shape[i] > 0 ? t.shape[i] : 1, &rm))
      return fail(DORA_ERR_INVALID, "tensor byte count overflows 64 bits");
  }
  kshape.clear();
  std::vector<int64_t> kstrides;
  for (int i = 0; i < t.ndim; ++i) {
    if (i == r.axis) continue;
    kshape.push_back(t.shape[i]);
    kstrides.push_back(strides[size_t(i)]);
  }
  dora_tensor kept = t;  // the kept dimensions
  kept.ndim = t.ndim - 1;
  kept.shape = kshape.data();
  kept.strides = kstrides.data();
  int rc = describe_source(kept, "argmax", dev, v);
  if (rc != DORA_OK) return rc;
  const int64_t ss = t.dtype_bits / 8;
  rd.on = true;
  rd.src_code = t.dtype_code;
  rd.src_bits = t.dtype_bits;
  rd.idx_code = r.dtype_code;
  rd.idx_bits = r.dtype_bits;
  rd.c = static_cast<uint64_t>(c);
  rd.count = v.bytes / static_cast<uint64_t>(ss);
  if (__builtin_mul_overflow(strides[size_t(r.axis)], ss, &rd.cstride))
    return fail(DORA_ERR_INVALID, "tensor stride %d overflows 64 bits", r.axis);
  // all C steps, held against the allocation later
  if (v.bytes && dev == ARROW_DEVICE_ROCM) rc = extend_reach(v.gd, c - 1, rd.cstride);
  if (rc != DORA_OK) return rc;
  v.leaf = leaf_of(r.dtype_code, r.dtype_bits);
  if (__builtin_mul_overflow(rd.count, static_cast<uint64_t>(ib), &v.bytes) || v.bytes >> 63)
    return fail(DORA_ERR_INVALID, "tensor byte count overflows 64 bits");
  return DORA_OK;
}

// The CPU's resize of a resize field: the output's elements in row-major order through
// resize_device.h's own walk, taps and blend, with cast_device.h's plain-integer conversions, into
// `dst` (any alignment).
struct ResizeHostMem : gather::resize::HostArith {
  const uint8_t* src;
  template <int S>
  uint32_t load_elem(int64_t s) const {
    uint32_t raw = 0;
    std::memcpy(&raw, src + s, S);  // (little-endian)
    return raw;
  }
  // (word `c` of a host table of the model-input step, any alignment)
  float load_table(const uint8_t* tab, uint64_t c) const {
    float v;
    std::memcpy(&v, tab + 4 * c, 4);
    return v;
  }
};

// (`pa`: gather::prep::None, or the model-input step's arguments)
template <uint32_t K, class PA>
void resize_all(const gather::resize::Args& a, uint8_t* dst, const PA& pa) {
  namespace rs = gather::resize;
  ResizeHostMem m{{}, a.g.src};
  typename rs::WalkFor<PA>::type w;
  rs::walk_start(a, 0, w, m, pa);
  for (uint64_t e = 0; e < a.g.total; ++e) {
    const float y = rs::prepped_at<K>(a, w, m, pa);
    const uint32_t q = a.dsize == 1   ? rs::to_dst<1>(a, y, m)
                       : a.dsize == 2 ? rs::to_dst<2>(a, y, m)
                                      : rs::to_dst<4>(a, y, m);
    std::memcpy(dst + e * a.dsize, &q, a.dsize);  // (little-endian)
    if (e + 1 < a.g.total) rs::walk_next(a, w, m, pa);
  }
}

void resize_host(const GatherDesc& g, const ResizeDesc& r, const PrepDesc& d, uint8_t* dst) {
  const gather::resize::Args a = gather::resize::make_args(g, r, dst);
  with_src_kind(static_cast<int>(a.src), [&](auto K) {
    if (d.on) resize_all<decltype(K)::value>(a, dst, gather::prep::make_args(d, r));
    else resize_all<decltype(K)::value>(a, dst, gather::prep::None{});
  });
}

// What resizes `t` (dora_gpu_plan_tensor_resize, `r.mode` != 0): the entry's and the tensor's
// refusals, else `rs`, the view `v` of the whole source — validated and canonicalised as a tensor
// of its own, its reach the field's; its leaf and byte count the resized tensor's — and `oshape`,
// the shape of the message.
int describe_resize(const dora_tensor& t, const dora_tensor_resize& r, ArrowDeviceType dev,
                    ResizeDesc& rs, TensorView& v, std::vector<int64_t>& oshape) {
  rs = ResizeDesc{};
  if (r.mode != DORA_RESIZE_NEAREST && r.mode != DORA_RESIZE_BILINEAR)
    return fail(DORA_ERR_UNSUPPORTED, "resize mode %u is not supported: DORA_RESIZE_NEAREST (%u) "
                "and DORA_RESIZE_BILINEAR (%u) are", r.mode, DORA_RESIZE_NEAREST,
                DORA_RESIZE_BILINEAR);
  if (const int rc = check_source_dtype(t, "resize"); rc != DORA_OK) return rc;
  const unsigned dcode = r.dtype_bits ? r.dtype_code : t.dtype_code;
  const unsigned dbits = r.dtype_bits ? r.dtype_bits : t.dtype_bits;
  if (!r.dtype_bits && t.dtype_code == DL_BFLOAT)
    return fail(DORA_ERR_UNSUPPORTED, "resize of a bfloat16 source without a destination dtype: "
                "Arrow has no bfloat16 (float16, float32, uint8, int8, uint16 and int16 are "
                "the destinations)");
  const bool dst_float = dcode == DL_FLOAT && (dbits == 16 || dbits == 32);
  if (!dst_float && gather::cast::dst_kind(dcode, dbits) < 0)
    return fail(DORA_ERR_UNSUPPORTED, "resize destination dtype %s is not supported: float16, "
                "float32, uint8, int8, uint16 and int16 are", dtype_name(dcode, dbits, 1).c_str());
  if (t.ndim < 2)
    return fail(DORA_ERR_INVALID, "resize of a tensor of %d dimensions (at least 2: the two "
                "resized axes)", t.ndim);
  if (t.ndim > kMaxTensorDims)
    return fail(DORA_ERR_UNSUPPORTED, "resize of a tensor of %d dimensions (at most %d)", t.ndim,
                kMaxTensorDims);
  if (!t.shape) return fail(DORA_ERR_INVALID, "tensor shape is NULL");
  for (int j = 0; j < 2; ++j)
    if (r.axis[j] < 0 || r.axis[j] >= t.ndim)
      return fail(DORA_ERR_INVALID, "resize axis %d is outside the tensor's %d dimensions",
                  r.axis[j], t.ndim);
  if (r.axis[0] == r.axis[1])
    return fail(DORA_ERR_INVALID, "resize axes %d and %d are the same dimension", r.axis[0],
                r.axis[1]);
  constexpr int64_t kMax = gather::resize::kMaxExtent;
  for (int j = 0; j < 2; ++j) {
    const int64_t in = t.shape[r.axis[j]];
    if (in < 1 || in > kMax)
      return fail(DORA_ERR_INVALID, "resize along axis %d of source extent %lld: 1 to %lld are "
                  "resized", r.axis[j], static_cast<long long>(in), static_cast<long long>(kMax));
    if (r.size[j] < 1 || r.size[j] > kMax)
      return fail(DORA_ERR_INVALID, "resize along axis %d to extent %lld: 1 to %lld are offered",
                  r.axis[j], static_cast<long long>(r.size[j]), static_cast<long long>(kMax));
  }
  const int rc = describe_source(t, "resize", dev, v);  // the whole source
  if (rc != DORA_OK) return rc;
  const int64_t ss = t.dtype_bits / 8;
  rs.on = true;
  rs.mode = static_cast<uint8_t>(r.mode);
  rs.src_code = t.dtype_code;
  rs.src_bits = t.dtype_bits;
  rs.dst_code = static_cast<uint8_t>(dcode);
  rs.dst_bits = static_cast<uint8_t>(dbits);
  rs.nd = t.ndim;
  oshape.assign(t.shape, t.shape + t.ndim);
  int64_t rm = ss;  // the byte strides, the caller's or row-major
  for (int i = t.ndim - 1; i >= 0; --i) {
    if (t.strides) {
      if (__builtin_mul_overflow(t.strides[i], ss, &rs.stride[i]))
        return fail(DORA_ERR_INVALID, "tensor stride %d overflows 64 bits", i);
    } else {
      rs.stride[i] = rm;
      rm *= t.shape[i] ? t.shape[i] : 1;  // (describe_tensor found the byte count to fit)
    }
  }
  for (int j = 0; j < 2; ++j) {
    rs.ax[j] = r.axis[j];
    rs.in[j] = t.shape[r.axis[j]];
    oshape[size_t(r.axis[j])] = r.size[j];
  }
  // the resized element count: the source's, which fits, over two extents >= 1 times two <= 2^15
  uint64_t count = v.bytes / static_cast<uint64_t>(ss);
  count = count / static_cast<uint64_t>(rs.in[0]) / static_cast<uint64_t>(rs.in[1]);
  if (__builtin_mul_overflow(count, static_cast<uint64_t>(r.size[0]), &count) ||
      __builtin_mul_overflow(count, static_cast<uint64_t>(r.size[1]), &count) ||
      __builtin_mul_overflow(count, static_cast<uint64_t>(dbits / 8u), &v.bytes) || v.bytes >> 63)
    return fail(DORA_ERR_INVALID, "tensor byte count overflows 64 bits");
  rs.count = count;
  for (int i = 0; i < t.ndim; ++i) rs.shape[i] = oshape[size_t(i)];
  v.leaf = leaf_of(dcode, dbits);
  return DORA_OK;
}

// The CPU's crops of a crops field: resize_all with crop_device.h's walk, which reads the boxes.
struct CropHostMem : ResizeHostMem {
  const uint8_t* boxes;
  int32_t load_box(int64_t at) const {
    int32_t v;
    std::memcpy(&v, boxes + at, 4);
    return v;
  }
};

template <uint32_t K, class PA>
void crop_all(const gather::crop::Args& a, uint8_t* dst, const PA& pa) {
  namespace cr = gather::crop;
  CropHostMem m{{{}, a.r.g.src}, a.boxes};
  cr::WalkFor<PA> w;
  cr::walk_start(a, 0, w, m, pa);
  for (uint64_t e = 0; e < a.r.g.total; ++e) {
    const uint32_t q = a.r.dsize == 1   ? cr::elem_at<K, 1>(a, w, m, pa)
                       : a.r.dsize == 2 ? cr::elem_at<K, 2>(a, w, m, pa)
                                        : cr::elem_at<K, 4>(a, w, m, pa);
    std::memcpy(dst + e * a.r.dsize, &q, a.r.dsize);  // (little-endian)
    if (e + 1 < a.r.g.total) cr::walk_next(a, w, m, pa);
  }
}

void crop_host(const GatherDesc& g, const CropDesc& c, const PrepDesc& d, uint8_t* dst) {
  const gather::crop::Args a = gather::crop::make_args(g, c, dst);
  with_src_kind(static_cast<int>(a.r.src), [&](auto K) {
    if (d.on) crop_all<decltype(K)::value>(a, dst, gather::prep::make_args(d, c.rs));
    else crop_all<decltype(K)::value>(a, dst, gather::prep::None{});
  });
}

// What crops `t` (dora_gpu_plan_tensor_crop, `c.mode` != 0): the frame's dimension count, then
// everything describe_resize refuses of the same frame, axes, size, mode and dtype, then the
// boxes' refusals; else `cd`, the view `v` of the whole frame — its leaf and byte count those of
// all K crops — and `oshape`, the shape of the message: K in front of the resized frame's.
int describe_crop(const dora_tensor& t, const dora_tensor_crop& c, ArrowDeviceType dev,
                  CropDesc& cd, TensorView& v, std::vector<int64_t>& oshape) {
  cd = CropDesc{};
  if (t.ndim < 2 || t.ndim > kMaxTensorDims - 1)
    return fail(DORA_ERR_INVALID, "crops of a frame of %d dimensions (2 to %d: the two cropped "
                "axes, and the message has one more)", t.ndim, kMaxTensorDims - 1);
  dora_tensor_resize r{};
  r.mode = c.mode;
  r.dtype_code = c.dtype_code;
  r.dtype_bits = c.dtype_bits;
  for (int j = 0; j < 2; ++j) {
    r.axis[j] = c.axis[j];
    r.size[j] = c.size[j];
  }
  ResizeDesc one;
  int rc = describe_resize(t, r, dev, one, v, oshape);
  if (rc != DORA_OK) return rc;
  if (!v.bytes)
    return fail(DORA_ERR_INVALID, "crops of a frame of extent 0 in dimension 0 (a fixed-size list "
                "of 0 values has no length to recover)");
  if (!c.boxes) return fail(DORA_ERR_INVALID, "boxes is NULL (K rows of four int32 words)");
  const dora_tensor& b = *c.boxes;
  if (b.dtype_code != DL_INT || b.dtype_bits != 32 || b.dtype_lanes != 1)
    return fail(DORA_ERR_INVALID, "boxes dtype %s is not int32",
                dtype_name(b.dtype_code, b.dtype_bits, b.dtype_lanes).c_str());
  if (b.ndim != 2 || !b.shape || b.shape[1] != 4)
    return fail(DORA_ERR_INVALID, "boxes are not of shape [K, 4] (%d dimensions%s): a row is "
                "(a_lo, b_lo, a_hi, b_hi)", b.ndim,
                b.ndim == 2 && b.shape ? ", rows of another length" : "");
  const int64_t k = b.shape[0];
  if (k < 0 || k > static_cast<int64_t>(kMaxCropBoxes))
    return fail(DORA_ERR_INVALID, "boxes hold %lld rows: 0 to %llu are cropped",
                static_cast<long long>(k), static_cast<unsigned long long>(kMaxCropBoxes));
  if (b.strides && k && (b.strides[1] != 1 || (k > 1 && b.strides[0] != 4)))
    return fail(DORA_ERR_INVALID, "boxes strides (%lld, %lld): the boxes are dense",
                static_cast<long long>(b.strides[0]), static_cast<long long>(b.strides[1]));
  if (!b.data && k) return fail(DORA_ERR_INVALID, "boxes data is NULL");
  cd.boxes = static_cast<const uint8_t*>(b.data) + b.byte_offset;
  if (k && (reinterpret_cast<uintptr_t>(cd.boxes) & 3u))
    return fail(DORA_ERR_INVALID, "boxes data %p is not aligned to its 4-byte words",
                static_cast<const void*>(cd.boxes));
  cd.on = true;
  cd.k = static_cast<uint64_t>(k);
  // the output's dimensions: K in front, never stepping through the frame
  ResizeDesc& rs = cd.rs;
  rs = one;
  rs.nd = one.nd + 1;
  rs.shape[0] = k;
  rs.stride[0] = 0;
  for (int i = 0; i < one.nd; ++i) {
    rs.shape[i + 1] = one.shape[i];
    rs.stride[i + 1] = one.stride[i];
  }
  for (int j = 0; j < 2; ++j) rs.ax[j] = one.ax[j] + 1;
  if (__builtin_mul_overflow(one.count, cd.k, &rs.count) ||
      __builtin_mul_overflow(v.bytes, cd.k, &v.bytes) || v.bytes >> 63)
    return fail(DORA_ERR_INVALID, "tensor byte count overflows 64 bits");
  oshape.insert(oshape.begin(), k);
  return DORA_OK;
}

// Whether a prep entry adds anything to its field (all zero: it does not; `fill` alone is not
// read).
bool prep_on(const dora_tensor_prep& p) {
  return p.scale || p.bias || p.has_scale || p.has_bias || p.inner[0] || p.inner[1] ||
         p.lead[0] || p.lead[1];
}

// The model-input step of a field `t` (validated) whose resize — or, `crop`, whose crops with K in
// front — `rs` describes, by the entry `pr` (prep_on): its refusals, else `out`.
int describe_prep(const dora_tensor& t, const dora_tensor_prep& pr, const ResizeDesc& rs, bool crop,
                  ArrowDeviceType dev, PrepDesc& out) {
  out = PrepDesc{};
  const int shift = crop ? 1 : 0;  // (K in front of the frame's dimensions)
  if (pr.scale && pr.has_scale)
    return fail(DORA_ERR_INVALID, "a scale table together with a scalar scale (has_scale): one "
                "scale a field");
  if (pr.bias && pr.has_bias)
    return fail(DORA_ERR_INVALID, "a bias table together with a scalar bias (has_bias): one bias "
                "a field");
  if (pr.scale || pr.bias) {
    if (pr.axis < 0 || pr.axis >= t.ndim)
      return fail(DORA_ERR_INVALID, "prep axis %d is outside the tensor's %d dimensions", pr.axis,
                  t.ndim);
    if (pr.axis + shift == rs.ax[0] || pr.axis + shift == rs.ax[1])
      return fail(DORA_ERR_INVALID, "prep axis %d is one of the two resized axes (%d and %d): the "
                  "tables run along a dimension that is kept", pr.axis, rs.ax[0] - shift,
                  rs.ax[1] - shift);
    int rc = pr.scale ? describe_table(*pr.scale, "scale", t, pr.axis, dev, &out.scale_tab)
                      : DORA_OK;
    if (rc == DORA_OK && pr.bias)
      rc = describe_table(*pr.bias, "bias", t, pr.axis, dev, &out.bias_tab);
    if (rc != DORA_OK) return rc;
    out.channels = static_cast<uint64_t>(t.shape[pr.axis]);
    out.axis = pr.axis + shift;
  }
  if (pr.has_scale && !std::isfinite(pr.scale_value))
    return fail(DORA_ERR_INVALID, "prep scale %f is not finite",
                static_cast<double>(pr.scale_value));
  if (pr.has_bias && !std::isfinite(pr.bias_value))
    return fail(DORA_ERR_INVALID, "prep bias %f is not finite",
                static_cast<double>(pr.bias_value));
  if (pr.inner[0] || pr.inner[1] || pr.lead[0] || pr.lead[1]) {
    if (crop)
      return fail(DORA_ERR_INVALID, "inner / lead on a field of crops: placement for crops is not "
                  "provided (per-box aspect would put a division per box on the device)");
    for (int j = 0; j < 2; ++j) {
      const int64_t size = rs.shape[rs.ax[j]];
      if (pr.inner[j] < 1 || pr.inner[j] > size)
        return fail(DORA_ERR_INVALID, "prep inner[%d] %lld is outside [1, %lld], the output's "
                    "extent along axis %d", j, static_cast<long long>(pr.inner[j]),
                    static_cast<long long>(size), rs.ax[j]);
      if (pr.lead[j] < 0 || pr.lead[j] > size - pr.inner[j])
        return fail(DORA_ERR_INVALID, "prep lead[%d] %lld is outside [0, %lld]: the image of "
                    "extent %lld lies inside the output's %lld along axis %d", j,
                    static_cast<long long>(pr.lead[j]),
                    static_cast<long long>(size - pr.inner[j]),
                    static_cast<long long>(pr.inner[j]), static_cast<long long>(size), rs.ax[j]);
      out.inner[j] = pr.inner[j];
      out.lead[j] = pr.lead[j];
    }
    if (!std::isfinite(pr.fill))
      return fail(DORA_ERR_INVALID, "prep fill %f is not finite", static_cast<double>(pr.fill));
    out.placed = true;
    out.fill = pr.fill;
  }
  out.on = true;
  out.has_scale = pr.has_scale ? 1 : 0;
  out.scale = pr.has_scale ? pr.scale_value : 1.0f;
  out.has_bias = pr.has_bias ? 1 : 0;
  out.bias = pr.has_bias ? pr.bias_value : 0.0f;
  return DORA_OK;
}

bool known_device(ArrowDeviceType dev) {
  return dev == ARROW_DEVICE_CPU || dev == ARROW_DEVICE_ROCM_HOST || dev == ARROW_DEVICE_ROCM;
}

// The recorded failure again, with the field it belongs to in front.
int field_fail(int rc, size_t k, const char* name) {
  const std::string why = dora_gpu_last_error();
  return fail(rc, "field %zu `%s`: %s", k, name ? name : "(null)", why.c_str());
}

}  // namespace

int build_tensor_plan(const dora_tensor* t, ArrowDeviceType dev, dora_plan** out) {
  if (!out) return fail(DORA_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!t) return fail(DORA_ERR_INVALID, "tensor is NULL");
  if (!known_device(dev)) return fail(DORA_ERR_INVALID, "unsupported device_type %d", dev);
  DORA_GUARD_BEGIN
  TensorView v;
  const int rc = describe_tensor(t, dev, v);
  if (rc != DORA_OK) return rc;
  std::unique_ptr<dora_plan> p(new dora_plan());
  p->dev = dev;
  p->size = v.bytes;
  tensor_type_info(TypeChain(v.leaf, t->shape, t->ndim, ""), t->shape, t->ndim, 0, v.bytes,
                   p->root);
  if (v.bytes == 0) {
    *out = p.release();
    return DORA_OK;
  }
  const StridedView& g = v.gd.view;
  // dense pageable memory: exactly dora_gpu_plan_bytes' plan, with the nested type info.  Pinned
  // memory is staged even when dense: copies and kernels reading it are asynchronous to the
  // host, and the send promises that the source has been read when it returns.
  if (g.nd == 0 && dev == ARROW_DEVICE_CPU) {
    p->segs.push_back({g.src, 0, v.bytes});
    *out = p.release();
    return DORA_OK;
  }
  if (dev == ARROW_DEVICE_ROCM) {
    // device memory is never dereferenced here: a dense view is dora_gpu_plan_bytes' plan with
    // the nested type info (every device path unchanged), a strided one the gather kernel's
    // descriptor and no segments
    p->dev_tensor = true;
    p->gd = v.gd;
    if (g.nd == 0) p->segs.push_back({g.src, 0, v.bytes});
    else p->launch = PlanLaunch::kView;
    *out = p.release();
    return DORA_OK;
  }
  // what the caller's own copy to contiguous memory would have done: every host path (inline
  // Vec, shared memory, BAR fill, DMA) then sees a dense pageable source
  p->staged.resize(v.bytes);
  gather_host(g, p->staged.data());
  p->dev = ARROW_DEVICE_CPU;  // pageable memory, whatever the view's was
  p->segs.push_back({p->staged.data(), 0, v.bytes});
  *out = p.release();
  return DORA_OK;
  DORA_GUARD_END
}

namespace {

// The entries of a message's fields, an optional array per op (n entries each, or NULL); none
// given: every field is sent as it is.  Never with a take; a field has one op at most, affine
// steps (describe_affine) going with a conversion (describe_convert).
struct FieldOps {
  const dora_tensor_cast* casts = nullptr;
  const dora_tensor_quant* quants = nullptr;
  const dora_tensor_affine* affines = nullptr;
  const dora_tensor_reduce* reduces = nullptr;  // describe_reduce
  const dora_tensor_resize* resizes = nullptr;  // describe_resize
  const dora_tensor_crop* crops = nullptr;      // describe_crop
  const dora_tensor_prep* preps = nullptr;      // describe_prep, with a resize or crops
};

// One field of a message, whatever is done to it on the way.  `v`: the view of what is read (a
// converted, reduced or resized field's in source bytes, with its reach) under the leaf and the
// byte count of what is sent.  As sent: `shape[0..ndim)` (in `own` where it is not the tensor's)
// and `elem`, the element size that pads the field's offset.  `launch`: what a device plan needs
// to fill the field, kFields when a gather will do.
struct FieldDesc {
  TensorView v;
  std::vector<int64_t> own;
  const int64_t* shape = nullptr;
  int ndim = 0;
  uint64_t elem = 0;
  PlanLaunch launch = PlanLaunch::kFields;
};

// Field `k` of a message with the entries `ops`, of `taken` rows when that is >= 0: the refusals
// of its entry and of the tensor, else `d` and the descriptors of `pf`.  A new op is one more
// array of FieldOps, one more branch here, and its own PlanLaunch.
int describe_field(const dora_tensor& t, size_t k, const FieldOps& ops, ArrowDeviceType dev,
                   int64_t taken, FieldDesc& d, PlanField& pf) {
  const bool affine = ops.affines && affine_on(ops.affines[k]);
  CastDesc& cd = pf.cast;
  int rc = describe_convert(t, ops.casts ? &ops.casts[k] : nullptr,
                            ops.quants ? &ops.quants[k] : nullptr, cd, affine);
  if (rc != DORA_OK) return rc;
  if (affine && !cd.on) {  // refused: the tensor's own refusals first, then the entry's
    rc = describe_tensor(&t, dev, d.v);
    return rc != DORA_OK ? rc : describe_affine(t, dev, ops.affines[k], cd);
  }
  d.ndim = t.ndim;
  d.elem = t.dtype_bits / 8u;
  const bool prep = ops.preps && prep_on(ops.preps[k]);
  if (ops.crops && ops.crops[k].mode) {
    rc = describe_crop(t, ops.crops[k], dev, pf.crop, d.v, d.own);
    if (rc == DORA_OK && prep) rc = describe_prep(t, ops.preps[k], pf.crop.rs, true, dev, pf.prep);
    d.launch = prep ? PlanLaunch::kCropPrep : PlanLaunch::kCrop;
    d.elem = pf.crop.rs.dst_bits / 8u;
    d.ndim = t.ndim + 1;
  } else if (ops.resizes && ops.resizes[k].mode) {
    rc = describe_resize(t, ops.resizes[k], dev, pf.resize, d.v, d.own);
    if (rc == DORA_OK && prep) rc = describe_prep(t, ops.preps[k], pf.resize, false, dev, pf.prep);
    d.launch = prep ? PlanLaunch::kResizePrep : PlanLaunch::kResize;
    d.elem = pf.resize.dst_bits / 8u;
  } else if (prep) {  // refused: the tensor's own refusals first, then the entry's
    rc = describe_tensor(&t, dev, d.v);
    if (rc == DORA_OK)
      rc = fail(DORA_ERR_INVALID, "a prep entry on a field that is neither resized nor crops");
  } else if (ops.reduces && ops.reduces[k].op) {
    rc = describe_reduce(t, ops.reduces[k], dev, pf.reduce, d.v, d.own);
    d.launch = PlanLaunch::kReduce;
    d.elem = pf.reduce.idx_bits / 8u;
    d.ndim = t.ndim - 1;
  } else if (cd.on) {
    rc = describe_source(t, "cast", dev, d.v);
    if (rc == DORA_OK && affine) rc = describe_affine(t, dev, ops.affines[k], cd);
    if (rc != DORA_OK) return rc;
    cd.count = d.v.bytes / (cd.src_bits / 8u);
    d.v.leaf = leaf_of(cd.dst_code, cd.dst_bits);
    d.v.bytes = cd.count * (cd.dst_bits / 8u);  // (at most twice the source's, which is < 2^63)
    if (d.v.bytes >> 63) return fail(DORA_ERR_INVALID, "tensor byte count overflows 64 bits");
    d.launch = PlanLaunch::kCast;
    d.elem = cd.dst_bits / 8u;
  } else if (taken >= 0) {
    rc = describe_taken(t, dev, static_cast<uint64_t>(taken), d.v, &pf.stride0);
    if (rc != DORA_OK) return rc;
    d.own.assign(t.shape, t.shape + t.ndim);
    d.own[0] = taken;
  } else {
    rc = describe_tensor(&t, dev, d.v);
  }
  d.shape = d.own.empty() ? t.shape : d.own.data();
  return rc;
}

// The fields of a record laid out from sample offset `off`: the schemas and what the loop over
// them found, for the struct plan and the ragged-batch plan alike.
struct FieldLayout {
  std::vector<std::unique_ptr<TypeChain>> chains;
  std::vector<ArrowSchema*> kids;
  uint64_t off = 0;     // in: where the first leaf may start; out: the end of the last
  int64_t taken = -1;   // in, >= 0: the fields of a take of that many rows (describe_taken)
  uint64_t staged = 0;  // bytes of host fields that are gathered or copied now
  bool strided = false;
  PlanLaunch launch = PlanLaunch::kFields;  // raised to what any field asks of a device plan
  uint64_t lead = 0;    // out: the leading extent the fields share, as sent
};

// Validation, view and type info of every field of `f[0..n)` with the entries `ops`
// (describe_field), each leaf at the running offset padded to its element size: PlanFields into
// `p`, type info into nodes[k].  `head` given: the one field is a bare tensor of its own (no
// name; its chain's head is called `head`).  With `lay.taken` every leaf, type and byte count
// has the leading extent `taken` where the field's own is N.
int layout_fields(const dora_tensor_field* f, size_t n, ArrowDeviceType dev, const char* head,
                  dora_plan& p, std::vector<TypeInfoNode>& nodes, FieldLayout& lay,
                  const FieldOps& ops = FieldOps()) {
  const bool bare = head != nullptr;
  p.fields.resize(n);
  lay.chains.resize(n);
  lay.kids.resize(n);
  nodes.resize(n);
  uint64_t off = lay.off;
  for (size_t k = 0; k < n; ++k) {
    const char* name = bare ? head : f[k].name;
    if (!bare) {
      if (!name || !name[0])
        return fail(DORA_ERR_INVALID, "field %zu has %s name", k, name ? "an empty" : "a NULL");
      for (size_t j = 0; j < k; ++j)
        if (std::strcmp(f[j].name, name) == 0)
          return fail(DORA_ERR_INVALID, "field %zu `%s` repeats the name of field %zu", k, name, j);
    }
    FieldDesc d;
    PlanField& pf = p.fields[k];
    const int rc = describe_field(f[k].tensor, k, ops, dev, lay.taken, d, pf);
    if (rc != DORA_OK) return bare ? rc : field_fail(rc, k, name);
    if (d.launch > lay.launch) lay.launch = d.launch;
    // (a taken field's leading extent is that of its N source rows)
    const int64_t lead = lay.taken >= 0 ? f[k].tensor.shape[0] : d.shape[0];
    if (k == 0) lay.lead = static_cast<uint64_t>(lead);
    if (static_cast<uint64_t>(lead) != lay.lead)
      return fail(DORA_ERR_INVALID, "field %zu `%s` has leading extent %lld, field 0 `%s` has "
                  "%lld: the fields of a struct share shape[0] (give tensors of unrelated shapes "
                  "a leading extent of 1)", k, name, static_cast<long long>(lead),
                  f[0].name, static_cast<long long>(lay.lead));
    // the running offset padded to the leaf's element size (a power of two)
    uint64_t padded, end;
    if (__builtin_add_overflow(off, d.elem - 1, &padded) ||
        __builtin_add_overflow(padded & ~(d.elem - 1), d.v.bytes, &end) || end >> 63)
      return fail(DORA_ERR_INVALID, "field %zu `%s`: the message's size overflows 64 bits", k,
                  bare ? "" : name);
    off = padded & ~(d.elem - 1);
    pf.name = bare ? "" : name;
    pf.gd = d.v.gd;
    pf.dst_off = off;
    pf.bytes = d.v.bytes;
    lay.chains[k].reset(new TypeChain(d.v.leaf, d.shape, d.ndim, name));
    lay.kids[k] = &lay.chains[k]->sch[0];
    tensor_type_info(*lay.chains[k], d.shape, d.ndim, off, d.v.bytes, nodes[k]);
    off = end;
    const bool stage = lay.taken >= 0 || d.launch != PlanLaunch::kFields ||
                       dev == ARROW_DEVICE_ROCM_HOST ||
                       (dev == ARROW_DEVICE_CPU && d.v.gd.view.nd);
    if (stage) lay.staged += d.v.bytes;  // (<= off)
    lay.strided |= d.v.gd.view.nd != 0;
  }
  lay.off = off;
  return DORA_OK;
}

// Host fields (none of them empty): dense pageable ones read in place, the others gathered — a
// cast field converted — now into one staging buffer — the segments of an ordinary multi-segment host plan.
void stage_host_fields(dora_plan& p, ArrowDeviceType dev, uint64_t staged) {
  p.staged.resize(staged);
  uint64_t at = 0;
  for (const PlanField& pf : p.fields) {
    if (dev == ARROW_DEVICE_CPU && pf.gd.view.nd == 0 && !pf.cast.on && !pf.reduce.on &&
        !pf.resize.on && !pf.crop.on) {
      p.segs.push_back({pf.gd.view.src, pf.dst_off, pf.bytes});
      continue;
    }
    if (pf.crop.on) crop_host(pf.gd, pf.crop, pf.prep, p.staged.data() + at);
    else if (pf.resize.on) resize_host(pf.gd, pf.resize, pf.prep, p.staged.data() + at);
    else if (pf.reduce.on) reduce_host(pf.gd.view, pf.reduce, p.staged.data() + at);
    else if (pf.cast.on) cast_host(pf.gd.view, pf.cast, p.staged.data() + at);
    else gather_host(pf.gd.view, p.staged.data() + at);
    p.segs.push_back({p.staged.data() + at, pf.dst_off, pf.bytes});
    at += pf.bytes;
  }
  p.fields.clear();  // (device plans keep them for the range check and the gather)
}

// Device fields (none of them empty), never dereferenced here.  All `dense`: the copy segments
// of any device plan (every device path, the AQL multi-segment packs included); otherwise no
// segments and one launch of kind `gather` over every field.  Either way each field's reach is
// checked first.
void place_device_fields(dora_plan& p, bool dense, PlanLaunch gather = PlanLaunch::kFields) {
  p.dev_tensor = true;
  if (!dense) {
    p.launch = gather;
    return;
  }
  for (const PlanField& pf : p.fields) p.segs.push_back({pf.gd.view.src, pf.dst_off, pf.bytes});
}

// What the record-like builders ask of their values before looking at one: at least one field
// (`noun` is refused by name) and, when `bounded`, no more than a launch carries.
int check_fields(const void* f, size_t n, const char* noun, const char* has = "values: ",
                 bool bounded = true) {
  if (n == 0 || !f) return fail(DORA_ERR_INVALID, "%s has %sat least one field", noun, has);
  if (bounded && n > kMaxStructFields)
    return fail(DORA_ERR_UNSUPPORTED, "a struct of tensors has at most %zu fields (%zu given)",
                kMaxStructFields, n);
  return DORA_OK;
}

// A 1-D dense tensor of int32 or int64 words: the partition of a ragged batch, the index of a
// take.
struct Partition {
  const uint8_t* src = nullptr;
  uint64_t count = 0;
  bool wide = false;
};

// Word `i` of a host one (any alignment).
int64_t word_at(const Partition& pt, uint64_t i) {
  if (pt.wide) {
    int64_t v;
    std::memcpy(&v, pt.src + 8 * i, 8);
    return v;
  }
  int32_t v;
  std::memcpy(&v, pt.src + 4 * i, 4);
  return v;
}

// The index of a take as its builders see it: K words, on the host or in HBM.
struct TakeIn {
  Partition ix;
  bool device = false;
};

// The message facts of a take, wherever its rows are taken: K words over `rows` source rows.
void note_take(dora_plan& p, const TakeIn& tk, uint64_t rows) {
  p.about.taken = true;
  p.about.take_k = tk.ix.count;
  p.about.take_n = rows;
  p.about.take_wide = tk.ix.wide ? 1 : 0;
}

// Where the taken fields' bytes come from (none of them empty: K > 0), after layout_fields.
//   Host: the index is read and checked — the first word outside [0, n) is refused, naming it —
//   and the CPU gathers row index[i] of every field into the staging buffer, dense fields and an
//   identity index included: the segments of an ordinary host plan.
//   Device: nothing is read; the plan is a gather with the index as one more source, each with
//   the reach check_plan_range holds against its allocation.
int place_taken(dora_plan& p, const TakeIn& tk, uint64_t rows, uint64_t staged) {
  const uint64_t k = tk.ix.count;
  if (tk.device) {
    p.dev_tensor = true;
    p.launch = PlanLaunch::kTaken;
    p.take = TakeDesc{tk.ix.src, k, rows, tk.ix.wide ? 1u : 0u};
    return DORA_OK;
  }
  for (uint64_t i = 0; i < k; ++i) {
    const int64_t w = word_at(tk.ix, i);
    if (w < 0 || w >= static_cast<int64_t>(rows))
      return fail(DORA_ERR_INVALID, "index: word %llu is %lld, outside the %llu rows of the values "
                  "(valid: 0 <= i < N, no negative wrap-around)",
                  static_cast<unsigned long long>(i), static_cast<long long>(w),
                  static_cast<unsigned long long>(rows));
  }
  p.staged.resize(staged);
  uint64_t at = 0;
  for (const PlanField& pf : p.fields) {
    StridedView one = pf.gd.view;  // one taken row: dimensions 1..
    one.total = pf.bytes / k;
    for (uint64_t i = 0; i < k; ++i) {
      one.src = pf.gd.view.src + word_at(tk.ix, i) * pf.stride0;
      gather_host(one, p.staged.data() + at + i * one.total);
    }
    p.segs.push_back({p.staged.data() + at, pf.dst_off, pf.bytes});
    at += pf.bytes;
  }
  p.fields.clear();
  return DORA_OK;
}

// The mask of a mask plan as its builder sees it: N bytes, on the host or in HBM.  `one_list`: the
// caller gave no partition (the builder was handed the one list of all N rows in its place).
struct MaskIn {
  const uint8_t* src = nullptr;
  uint64_t count = 0;
  bool device = false;
  bool one_list = false;
};

// Host values under a host mask (N > 0, after layout_fields with `taken` = N): the CPU reads the
// mask, gathers the selected rows of every field to the front of the field's N rows in the
// staging buffer (the rest stays zero) and replaces the checked offsets p_b by C[p_b]: the
// segments of an ordinary host plan.
void place_masked_host(dora_plan& p, const MaskIn& mk, uint64_t staged) {
  const uint64_t n = mk.count;
  std::vector<int32_t> c(n + 1);
  int32_t k = 0;
  for (uint64_t i = 0; i < n; ++i) {
    c[i] = k;
    k += mk.src[i] != 0;
  }
  c[n] = k;
  for (int32_t& o : p.list_offsets) o = c[static_cast<size_t>(o)];
  p.staged.assign(staged, 0);
  uint64_t at = 0;
  for (const PlanField& pf : p.fields) {
    StridedView one = pf.gd.view;  // one row: dimensions 1..
    one.total = pf.bytes / n;
    uint64_t j = 0;
    for (uint64_t i = 0; i < n; ++i) {
      if (!mk.src[i]) continue;
      one.src = pf.gd.view.src + static_cast<int64_t>(i) * pf.stride0;
      gather_host(one, p.staged.data() + at + j++ * one.total);
    }
    p.segs.push_back({p.staged.data() + at, pf.dst_off, pf.bytes});
    at += pf.bytes;
  }
  p.fields.clear();
}

// A tensor (`bare`: one field without a name) or a record of tensors as one message, its fields
// with the entries `ops`; with `tk` the rows of it that the index takes.
int build_record(const dora_tensor_field* f, size_t n, ArrowDeviceType dev, bool bare,
                 const TakeIn* tk, dora_plan** out, const FieldOps& ops = FieldOps()) {
  DORA_GUARD_BEGIN
  std::unique_ptr<dora_plan> p(new dora_plan());
  p->dev = dev == ARROW_DEVICE_ROCM ? ARROW_DEVICE_ROCM : ARROW_DEVICE_CPU;
  FieldLayout lay;
  if (tk) lay.taken = static_cast<int64_t>(tk->ix.count);
  std::vector<TypeInfoNode> solo;
  int rc = layout_fields(f, n, dev, bare ? "" : nullptr, *p, bare ? solo : p->root.children, lay,
                         ops);
  if (rc != DORA_OK) return rc;
  const uint64_t off = lay.off;
  if (bare) {
    p->root = std::move(solo[0]);
  } else {
    ArrowSchema top;
    std::memset(&top, 0, sizeof(top));
    top.format = "+s";
    top.name = "";
    top.children = lay.kids.data();
    top.n_children = static_cast<int64_t>(n);
    serialize_schema(&top, true, p->root.schema);
    p->root.len = tk ? tk->ix.count : lay.lead;
  }
  p->size = off;
  const uint64_t rows = static_cast<uint64_t>(f[0].tensor.shape[0]);
  if (tk) note_take(*p, *tk, rows);
  // what fills the sample: nothing (d0 == 0, an empty message); the taken rows; device fields as
  // segments when all are dense and sent as they are, else the one launch the fields ask for;
  // host fields
  if (off == 0) p->fields.clear();
  else if (tk) rc = place_taken(*p, *tk, rows, lay.staged);
  else if (dev == ARROW_DEVICE_ROCM)
    place_device_fields(*p, !lay.strided && lay.launch == PlanLaunch::kFields, lay.launch);
  else stage_host_fields(*p, dev, lay.staged);
  if (rc != DORA_OK) return rc;
  *out = p.release();
  return DORA_OK;
  DORA_GUARD_END
}

// What the builders of a message with entries do before they look at one: `out` and the device,
// then at least one field (`noun` is refused by name) and no more than a launch carries; between
// those two `missing`, when given: the refusal of an array of entries that is NULL.  `*bare`: the
// one field is a tensor of its own.
int begin_record(const dora_tensor_field* f, size_t n, ArrowDeviceType dev, dora_plan** out,
                 const char* noun, bool* bare, const char* missing = nullptr) {
  if (!out) return fail(DORA_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!known_device(dev)) return fail(DORA_ERR_INVALID, "unsupported device_type %d", dev);
  if (missing && n && f) return fail(DORA_ERR_INVALID, "%s", missing);
  const int rc = check_fields(f, n, noun);
  *bare = rc == DORA_OK && n == 1 && !f[0].name;
  return rc;
}

}  // namespace

int build_tensor_struct_plan(const dora_tensor_field* f, size_t n, ArrowDeviceType dev,
                             dora_plan** out) {
  if (!out) return fail(DORA_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!known_device(dev)) return fail(DORA_ERR_INVALID, "unsupported device_type %d", dev);
  const int rc = check_fields(f, n, "a struct of tensors", "");
  return rc != DORA_OK ? rc : build_record(f, n, dev, false, nullptr, out);
}

namespace {

// No entry does anything: the plain plan, whatever it is, refusals included.
int build_plain(const dora_tensor_field* f, size_t n, ArrowDeviceType dev, dora_plan** out) {
  if (f && n == 1 && !f[0].name) return build_tensor_plan(&f[0].tensor, dev, out);
  return build_tensor_struct_plan(f, n, dev, out);
}

}  // namespace

int build_tensor_cast_plan(const dora_tensor_field* f, size_t n, const dora_tensor_cast* casts,
                           ArrowDeviceType dev, dora_plan** out) {
  bool bare = false;
  const int rf = begin_record(f, n, dev, out, "a cast", &bare,
                              casts ? nullptr : "casts is NULL (one entry per field)");
  if (rf != DORA_OK) return rf;
  // no field converted at all (after every cast's own refusals): the plain plan
  bool any = false;
  for (size_t k = 0; k < n; ++k) {
    CastDesc cd;
    const int rc = describe_cast(f[k].tensor, casts[k], cd);
    if (rc != DORA_OK) return bare ? rc : field_fail(rc, k, f[k].name);
    any |= cd.on;
  }
  if (!any) return build_plain(f, n, dev, out);
  return build_record(f, n, dev, bare, nullptr, out, FieldOps{casts});
}

int build_tensor_convert_plan(const dora_tensor_field* f, size_t n, const dora_tensor_cast* casts,
                              const dora_tensor_quant* quants, ArrowDeviceType dev,
                              dora_plan** out) {
  bool bare = false;
  const int rf = begin_record(f, n, dev, out, "a conversion", &bare);
  if (rf != DORA_OK) return rf;
  // every entry's own refusals first; no field quantised: what the cast plan is, whatever it is
  bool quantised = false;
  for (size_t k = 0; k < n; ++k) {
    CastDesc cd;
    const int rc = describe_convert(f[k].tensor, casts ? &casts[k] : nullptr,
                                    quants ? &quants[k] : nullptr, cd);
    if (rc != DORA_OK) return bare ? rc : field_fail(rc, k, f[k].name);
    quantised |= cd.quant();
  }
  if (!quantised)
    return casts ? build_tensor_cast_plan(f, n, casts, dev, out) : build_plain(f, n, dev, out);
  return build_record(f, n, dev, bare, nullptr, out, FieldOps{casts, quants});
}

int build_tensor_affine_plan(const dora_tensor_field* f, size_t n, const dora_tensor_cast* casts,
                             const dora_tensor_quant* quants, const dora_tensor_affine* affines,
                             ArrowDeviceType dev, dora_plan** out) {
  bool any = false, bare = false;
  for (size_t k = 0; affines && f && k < n; ++k) any |= affine_on(affines[k]);
  // no affine step at all: the conversion's plan, whatever it is, refusals included
  if (!any) return build_tensor_convert_plan(f, n, casts, quants, dev, out);
  const int rf = begin_record(f, n, dev, out, "a conversion", &bare);
  if (rf != DORA_OK) return rf;
  // every field's own refusals, then its affine entry's, as the fields are laid out
  return build_record(f, n, dev, bare, nullptr, out, FieldOps{casts, quants, affines});
}

int build_tensor_reduce_plan(const dora_tensor_field* f, size_t n,
                             const dora_tensor_reduce* reduces, ArrowDeviceType dev,
                             dora_plan** out) {
  bool any = false, bare = false;
  for (size_t k = 0; reduces && f && k < n; ++k) any |= reduces[k].op != 0;
  if (!any) return build_plain(f, n, dev, out);
  const int rf = begin_record(f, n, dev, out, "a reduction", &bare);
  if (rf != DORA_OK) return rf;
  FieldOps ops;
  ops.reduces = reduces;
  return build_record(f, n, dev, bare, nullptr, out, ops);
}

int build_tensor_resize_plan(const dora_tensor_field* f, size_t n,
                             const dora_tensor_resize* resizes, ArrowDeviceType dev,
                             dora_plan** out) {
  bool any = false, bare = false;
  for (size_t k = 0; resizes && f && k < n; ++k) any |= resizes[k].mode != 0;
  if (!any) return build_plain(f, n, dev, out);
  const int rf = begin_record(f, n, dev, out, "a resize", &bare);
  if (rf != DORA_OK) return rf;
  FieldOps ops;
  ops.resizes = resizes;
  return build_record(f, n, dev, bare, nullptr, out, ops);
}

int build_tensor_crop_plan(const dora_tensor_field* f, size_t n, const dora_tensor_crop* crops,
                           ArrowDeviceType dev, dora_plan** out) {
  bool any = false, bare = false;
  for (size_t k = 0; crops && f && k < n; ++k) any |= crops[k].mode != 0;
  if (!any) return build_plain(f, n, dev, out);
  const int rf = begin_record(f, n, dev, out, "crops", &bare);
  if (rf != DORA_OK) return rf;
  FieldOps ops;
  ops.crops = crops;
  return build_record(f, n, dev, bare, nullptr, out, ops);
}

int build_tensor_prep_plan(const dora_tensor_field* f, size_t n, const dora_tensor_resize* resizes,
                           const dora_tensor_crop* crops, const dora_tensor_prep* preps,
                           ArrowDeviceType dev, dora_plan** out) {
  bool any = false, any_r = false, any_c = false, bare = false;
  for (size_t k = 0; f && k < n; ++k) {
    any |= preps && prep_on(preps[k]);
    any_r |= resizes && resizes[k].mode != 0;
    any_c |= crops && crops[k].mode != 0;
  }
  if (any_r && any_c) {
    if (out) *out = nullptr;
    return fail(DORA_ERR_INVALID, "resize entries and crops entries are both active in one call: "
                "resize and crops in one record are not provided");
  }
  // no prep entry at all: the resize's or the crops' plan, whatever it is, refusals included
  if (!any)
    return any_c ? build_tensor_crop_plan(f, n, crops, dev, out)
                 : build_tensor_resize_plan(f, n, resizes, dev, out);
  const int rf = begin_record(f, n, dev, out, "a model input", &bare);
  if (rf != DORA_OK) return rf;
  FieldOps ops;
  ops.resizes = any_r ? resizes : nullptr;
  ops.crops = any_c ? crops : nullptr;
  ops.preps = preps;
  return build_record(f, n, dev, bare, nullptr, out, ops);
}

namespace {

// The words of `what` (the partition of a ragged batch, holding `holds`; the index of a take).
// `aligned`: the words must sit on their own size (anything a kernel reads).
int describe_words(const dora_tensor& t, const char* what, const char* holds, bool aligned,
                   Partition& out) {
  if (t.dtype_code != DL_INT || t.dtype_lanes != 1 || (t.dtype_bits != 32 && t.dtype_bits != 64))
    return fail(DORA_ERR_INVALID, "%s dtype (code %u, %u bits, %u lanes) is not int32 or "
                "int64", what, unsigned(t.dtype_code), unsigned(t.dtype_bits),
                unsigned(t.dtype_lanes));
  if (t.ndim != 1 || !t.shape)
    return fail(DORA_ERR_INVALID, "%s has %d dimensions (a 1-D tensor of %s)", what, t.ndim,
                holds);
  if (t.shape[0] < 0)
    return fail(DORA_ERR_INVALID, "%s extent %lld is negative", what,
                static_cast<long long>(t.shape[0]));
  if (t.strides && t.shape[0] > 1 && t.strides[0] != 1)
    return fail(DORA_ERR_INVALID, "%s stride %lld: the %s is dense", what,
                static_cast<long long>(t.strides[0]), what);
  if (!t.data && t.shape[0]) return fail(DORA_ERR_INVALID, "%s data is NULL", what);
  out.src = static_cast<const uint8_t*>(t.data) + t.byte_offset;
  out.count = static_cast<uint64_t>(t.shape[0]);
  out.wide = t.dtype_bits == 64;
  if (aligned && out.count && (reinterpret_cast<uintptr_t>(out.src) & (out.wide ? 7u : 3u)))
    return fail(DORA_ERR_INVALID, "%s data %p is not aligned to its %d-byte words", what,
                static_cast<const void*>(out.src), out.wide ? 8 : 4);
  return DORA_OK;
}

int describe_partition(const dora_tensor& t, Partition& out) {
  return describe_words(t, "partition", "lengths or offsets", true, out);
}

// The B + 1 offsets of a host partition over `rows` rows, checked: DORA_ERR_INVALID naming the
// first word that breaks the rule.
int host_offsets(const Partition& pt, bool offsets_form, uint64_t rows, std::vector<int32_t>& o) {
  auto word = [&](uint64_t i) -> int64_t { return word_at(pt, i); };
  const int64_t n = static_cast<int64_t>(rows);
  if (offsets_form) {
    o.resize(pt.count);
    int64_t prev = 0;
    for (uint64_t i = 0; i < pt.count; ++i) {
      const int64_t v = word(i);
      if (i == 0 && v != 0)
        return fail(DORA_ERR_INVALID, "partition: offset 0 is %lld: offsets start at 0",
                    static_cast<long long>(v));
      if (v < prev)
        return fail(DORA_ERR_INVALID, "partition: offset %llu is %lld, below offset %llu (%lld): "
                    "offsets never decrease", static_cast<unsigned long long>(i),
                    static_cast<long long>(v), static_cast<unsigned long long>(i - 1),
                    static_cast<long long>(prev));
      if (v > n)
        return fail(DORA_ERR_INVALID, "partition: offset %llu is %lld, past the %lld rows of the "
                    "values", static_cast<unsigned long long>(i), static_cast<long long>(v),
                    static_cast<long long>(n));
      o[i] = static_cast<int32_t>(v);
      prev = v;
    }
    if (prev != n)
      return fail(DORA_ERR_INVALID, "partition: offset %llu, the last, is %lld: offsets end at "
                  "the %lld rows of the values", static_cast<unsigned long long>(pt.count - 1),
                  static_cast<long long>(prev), static_cast<long long>(n));
    return DORA_OK;
  }
  o.resize(pt.count + 1);
  int64_t sum = 0;
  o[0] = 0;
  for (uint64_t i = 0; i < pt.count; ++i) {
    const int64_t v = word(i);
    if (v < 0)
      return fail(DORA_ERR_INVALID, "partition: length %llu is %lld: lengths are not negative",
                  static_cast<unsigned long long>(i), static_cast<long long>(v));
    if (v > n - sum)
      return fail(DORA_ERR_INVALID, "partition: lengths 0..%llu sum past the %lld rows of the "
                  "values (length %llu is %lld)", static_cast<unsigned long long>(i),
                  static_cast<long long>(n), static_cast<unsigned long long>(i),
                  static_cast<long long>(v));
    sum += v;
    o[i + 1] = static_cast<int32_t>(sum);
  }
  if (sum != n)
    return fail(DORA_ERR_INVALID, "partition: the %llu lengths sum to %lld, the values have %lld "
                "rows (index %llu is where they fall short)",
                static_cast<unsigned long long>(pt.count), static_cast<long long>(sum),
                static_cast<long long>(n), static_cast<unsigned long long>(pt.count));
  return DORA_OK;
}

}  // namespace

namespace {

// A ragged batch over the fields' rows; with `tk` over the rows of them that the index takes;
// with `mk` (never with `tk`) over the N source rows of which the mask keeps K in front: the
// child keeps its N rows and the offsets become C[p_b].
int build_list(const dora_tensor_list* l, ArrowDeviceType dev, const TakeIn* tk, dora_plan** out,
               const MaskIn* mk = nullptr) {
  if (!known_device(dev)) return fail(DORA_ERR_INVALID, "unsupported device_type %d", dev);
  if (!known_device(l->partition_device))
    return fail(DORA_ERR_INVALID, "unsupported partition_device %d", l->partition_device);
  if (l->partition_form != DORA_PARTITION_LENGTHS && l->partition_form != DORA_PARTITION_OFFSETS)
    return fail(DORA_ERR_INVALID, "partition_form %u is neither lengths nor offsets",
                l->partition_form);
  const size_t n = l->n;
  const dora_tensor_field* f = l->fields;
  int rc = check_fields(f, n, "a ragged batch");
  if (rc != DORA_OK) return rc;
  const bool bare = n == 1 && !f[0].name;
  const bool offsets_form = l->partition_form == DORA_PARTITION_OFFSETS;
  const bool dev_part = l->partition_device == ARROW_DEVICE_ROCM;
  if (dev_part && dev != ARROW_DEVICE_ROCM)
    return fail(DORA_ERR_INVALID, "a partition in device memory needs values on this node's GPU: "
                "with host values pass the partition as a host list (.tolist())");
  DORA_GUARD_BEGIN
  Partition pt;
  rc = describe_partition(l->partition, pt);
  if (rc != DORA_OK) return rc;
  if (offsets_form && pt.count == 0)
    return fail(DORA_ERR_INVALID, "partition: offsets have at least one entry (B + 1 of them)");
  if (pt.count >= (uint64_t(1) << 31) - (offsets_form ? 0 : 1))
    return fail(DORA_ERR_UNSUPPORTED, "a ragged batch of %llu lists needs 64-bit offsets "
                "(LargeList), which is not produced",
                static_cast<unsigned long long>(pt.count - (offsets_form ? 1 : 0)));
  if (dev_part && pt.count > kMaxScanEntries)
    return fail(DORA_ERR_UNSUPPORTED, "a partition in device memory has at most %llu entries "
                "(%llu given): one workgroup scans them",
                static_cast<unsigned long long>(kMaxScanEntries),
                static_cast<unsigned long long>(pt.count));
  const uint64_t lists = pt.count - (offsets_form ? 1 : 0);
  const uint64_t obytes = (lists + 1) * 4;

  std::unique_ptr<dora_plan> p(new dora_plan());
  p->about.list = true;
  p->dev = dev == ARROW_DEVICE_ROCM ? ARROW_DEVICE_ROCM : ARROW_DEVICE_CPU;
  // the type info: the list node with its offsets buffer, under it the values' node — the
  // tensor's chain, or the struct node over the fields' chains
  p->root.children.resize(1);
  TypeInfoNode& child = p->root.children[0];
  FieldLayout lay;
  lay.off = obytes;
  std::vector<TypeInfoNode> solo;
  // (a mask's fields are described as a take of all N rows describes them; a first field that has
  // no shape[0] to read is refused by the layout whatever N is taken to be)
  const dora_tensor& t0 = f[0].tensor;
  const int64_t mask_rows = mk && t0.shape && t0.ndim >= 1 && t0.shape[0] > 0 ? t0.shape[0] : 0;
  lay.taken = tk ? static_cast<int64_t>(tk->ix.count) : mk ? mask_rows : -1;
  rc = layout_fields(f, n, dev, bare ? "item" : nullptr, *p, bare ? solo : child.children, lay);
  if (rc != DORA_OK) return rc;
  if (mk) {
    p->about.masked = true;
    p->about.mask_n = static_cast<uint64_t>(mask_rows);
    if (mk->count != static_cast<uint64_t>(mask_rows))
      return fail(DORA_ERR_INVALID, "mask has %llu elements, the values have %lld rows: one mask "
                  "element per row", static_cast<unsigned long long>(mk->count),
                  static_cast<long long>(mask_rows));
    if (mk->count > gather::mask::kMaxRows)
      return fail(DORA_ERR_UNSUPPORTED, "a mask over %llu rows: at most %llu (one workgroup sums "
                  "the totals of the tiles before its own)",
                  static_cast<unsigned long long>(mk->count),
                  static_cast<unsigned long long>(gather::mask::kMaxRows));
    // (a host partition's offsets are scanned on the device too, on their way through C)
    if (dev == ARROW_DEVICE_ROCM && !dev_part && !mk->one_list && lists + 1 > kMaxScanEntries)
      return fail(DORA_ERR_UNSUPPORTED, "a partition over masked device values has at most %llu "
                  "offsets (%llu given): one workgroup looks them up",
                  static_cast<unsigned long long>(kMaxScanEntries),
                  static_cast<unsigned long long>(lists + 1));
  }
  // the rows the partition cuts: the fields' own, or the K taken ones
  const uint64_t rows = tk ? tk->ix.count : static_cast<uint64_t>(f[0].tensor.shape[0]);
  const uint64_t src_rows = static_cast<uint64_t>(f[0].tensor.shape[0]);
  if (tk) note_take(*p, *tk, src_rows);
  if (rows >> 31)
    return fail(DORA_ERR_UNSUPPORTED, "a ragged batch over %llu rows needs 64-bit offsets "
                "(LargeList), which is not produced", static_cast<unsigned long long>(rows));
  ArrowSchema item;
  std::memset(&item, 0, sizeof(item));
  ArrowSchema* item_ptr = &item;
  if (bare) {
    child = std::move(solo[0]);
    item_ptr = lay.kids[0];
  } else {
    item.format = "+s";
    item.name = "item";
    item.flags = ARROW_FLAG_NULLABLE;
    item.children = lay.kids.data();
    item.n_children = static_cast<int64_t>(n);
    serialize_schema(&item, true, child.schema);
    child.len = rows;
  }
  ArrowSchema top;
  std::memset(&top, 0, sizeof(top));
  top.format = "+l";
  top.name = "";
  top.children = &item_ptr;
  top.n_children = 1;
  serialize_schema(&top, true, p->root.schema);
  p->root.len = lists;
  p->root.bufs.push_back({0, obytes});
  p->size = lay.off;
  const bool empty = rows == 0;  // every field is then empty: only the offsets travel
  if (empty) p->fields.clear();

  const bool dev_values = dev == ARROW_DEVICE_ROCM && !empty;
  // the offsets are known here: a host partition's, checked; or all 0 for a mask over no rows,
  // whatever its partition in HBM holds, which is then never read
  const bool host_part = !dev_part || (mk && empty);
  if (!dev_part) {
    rc = host_offsets(pt, offsets_form, rows, p->list_offsets);
    if (rc != DORA_OK) return rc;
  } else if (host_part) {
    p->list_offsets.assign(lists + 1, 0);
  }
  const Segment oseg{p->list_offsets.data(), 0, obytes};

  // what fills the sample, decided once
  if (host_part && !dev_values) {
    // host values (or none): an ordinary multi-segment host plan, the offsets its first segment
    p->dev = ARROW_DEVICE_CPU;
    p->segs.push_back(oseg);
    if (tk && !empty) rc = place_taken(*p, *tk, src_rows, lay.staged);
    else if (mk && !empty) place_masked_host(*p, *mk, lay.staged);
    else if (!empty) stage_host_fields(*p, dev, lay.staged);
  } else if (mk) {
    // a mask in HBM: never read here.  Always the three launches, no segments.  The checked
    // offsets of a host partition go ahead into the workspace, where the scan share finds them;
    // the words of one in HBM are scanned in place; either way they are looked up in the counts
    // the mask gives.  Without a partition there is no scan: the compaction writes [0, K].
    p->dev_tensor = true;
    p->launch = PlanLaunch::kMasked;
    const uint64_t part_words = host_part && !mk->one_list ? lists + 1 : 0;
    p->mask = MaskDesc{mk->src, rows, part_words};
    if (part_words) {
      p->scan_on = true;
      p->scan.count = part_words;
      p->scan.n = rows;
      p->scan.offsets = 1;
      p->prefix.push_back({p->list_offsets.data(),
                           gather::mask::workspace(p->size, rows, part_words).part, obytes});
    }
  } else if (host_part) {
    // device values: the offsets go ahead on the pack's stream, the fields as in the struct plan
    // (a take always the one launch, dense fields included)
    p->prefix.push_back(oseg);
    if (tk) rc = place_taken(*p, *tk, src_rows, lay.staged);
    else place_device_fields(*p, !lay.strided);
  }
  if (!host_part) {
    // a partition in HBM: never read here.  The plan's one launch (a mask plan's last) scans it
    // and gathers every field, dense ones included; over no rows it only writes the offsets.
    p->dev_tensor = true;
    p->scan_on = true;
    p->scan = ScanDesc{pt.src, pt.count, rows, pt.wide ? 1u : 0u, offsets_form ? 1u : 0u};
    if (tk && !empty) rc = place_taken(*p, *tk, src_rows, lay.staged);
    else if (!mk) p->launch = PlanLaunch::kFields;
  }
  if (rc != DORA_OK) return rc;
  *out = p.release();
  return DORA_OK;
  DORA_GUARD_END
}

}  // namespace

int build_tensor_list_plan(const dora_tensor_list* l, ArrowDeviceType dev, dora_plan** out) {
  if (!out) return fail(DORA_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!l) return fail(DORA_ERR_INVALID, "list is NULL");
  return build_list(l, dev, nullptr, out);
}

int build_tensor_take_plan(const dora_tensor_take* t, ArrowDeviceType dev, dora_plan** out) {
  if (!out) return fail(DORA_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!t) return fail(DORA_ERR_INVALID, "take is NULL");
  if (!known_device(dev)) return fail(DORA_ERR_INVALID, "unsupported device_type %d", dev);
  if (!known_device(t->index_device))
    return fail(DORA_ERR_INVALID, "unsupported index_device %d", t->index_device);
  int rc = check_fields(t->fields, t->n, "a take");
  if (rc != DORA_OK) return rc;
  TakeIn tk;
  tk.device = t->index_device == ARROW_DEVICE_ROCM;
  if (tk.device != (dev == ARROW_DEVICE_ROCM))
    return fail(DORA_ERR_INVALID, "the index is in %s memory and the values are in %s memory: "
                "move the index next to the values (a host index for host values, an index in "
                "this node's HBM for device values)", tk.device ? "device" : "host",
                tk.device ? "host" : "device");
  // (a host index may sit at any address: only a kernel needs its words aligned)
  rc = describe_words(t->index, "index", "row numbers", tk.device, tk.ix);
  if (rc != DORA_OK) return rc;
  if (t->partition) {
    if (tk.ix.count >> 31)
      return fail(DORA_ERR_UNSUPPORTED, "a ragged batch over %llu rows needs 64-bit offsets "
                  "(LargeList), which is not produced",
                  static_cast<unsigned long long>(tk.ix.count));
    dora_tensor_list l{};
    l.fields = t->fields;
    l.n = t->n;
    l.partition = *t->partition;
    l.partition_form = t->partition_form;
    l.partition_device = t->partition_device;
    return build_list(&l, dev, &tk, out);
  }
  return build_record(t->fields, t->n, dev, t->n == 1 && !t->fields[0].name, &tk, out);
}

int build_tensor_mask_plan(const dora_tensor_mask* m, ArrowDeviceType dev, dora_plan** out) {
  if (!out) return fail(DORA_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!m) return fail(DORA_ERR_INVALID, "mask is NULL");
  if (!known_device(dev)) return fail(DORA_ERR_INVALID, "unsupported device_type %d", dev);
  if (!known_device(m->mask_device))
    return fail(DORA_ERR_INVALID, "unsupported mask_device %d", m->mask_device);
  // (too many fields: refused by the ragged batch it becomes, behind its partition's refusals)
  const int rc = check_fields(m->fields, m->n, "a mask", "values: ", false);
  if (rc != DORA_OK) return rc;
  MaskIn mk;
  mk.device = m->mask_device == ARROW_DEVICE_ROCM;
  if (mk.device != (dev == ARROW_DEVICE_ROCM))
    return fail(DORA_ERR_INVALID, "the mask is in %s memory and the values are in %s memory: "
                "move the mask next to the values (a host mask for host values, a mask in this "
                "node's HBM for device values)", mk.device ? "device" : "host",
                mk.device ? "host" : "device");
  const dora_tensor& t = m->mask;
  if (t.dtype_lanes != 1 || t.dtype_bits != 8 || (t.dtype_code != DL_BOOL && t.dtype_code != DL_UINT))
    return fail(DORA_ERR_INVALID, "mask dtype %s is not bool or uint8",
                dtype_name(t.dtype_code, t.dtype_bits, t.dtype_lanes).c_str());
  if (t.ndim != 1 || !t.shape)
    return fail(DORA_ERR_INVALID, "mask has %d dimensions (a 1-D tensor, one element per row)",
                t.ndim);
  if (t.shape[0] < 0)
    return fail(DORA_ERR_INVALID, "mask extent %lld is negative",
                static_cast<long long>(t.shape[0]));
  if (t.strides && t.shape[0] > 1 && t.strides[0] != 1)
    return fail(DORA_ERR_INVALID, "mask stride %lld: the mask is dense",
                static_cast<long long>(t.strides[0]));
  if (!t.data && t.shape[0]) return fail(DORA_ERR_INVALID, "mask data is NULL");
  mk.src = static_cast<const uint8_t*>(t.data) + t.byte_offset;
  mk.count = static_cast<uint64_t>(t.shape[0]);
  dora_tensor_list l{};
  l.fields = m->fields;
  l.n = m->n;
  // without a partition: the one list of all N rows, whose offsets [0, N] become [0, K]
  const int64_t all = static_cast<int64_t>(mk.count), one = 1;
  if (m->partition) {
    l.partition = *m->partition;
    l.partition_form = m->partition_form;
    l.partition_device = m->partition_device;
  } else {
    mk.one_list = true;
    l.partition.data = const_cast<int64_t*>(&all);
    l.partition.dtype_code = DL_INT;
    l.partition.dtype_bits = 64;
    l.partition.dtype_lanes = 1;
    l.partition.ndim = 1;
    l.partition.shape = &one;
    l.partition_form = DORA_PARTITION_LENGTHS;
    l.partition_device = ARROW_DEVICE_CPU;
  }
  return build_list(&l, dev, nullptr, out, &mk);
}

}  // namespace dora

extern "C" {

int dora_gpu_plan_tensor_mask(const dora_tensor_mask* mask, ArrowDeviceType device_type,
                              dora_plan** out) {
  return dora::build_tensor_mask_plan(mask, device_type, out);
}

int dora_gpu_plan_tensor(const dora_tensor* tensor, ArrowDeviceType device_type,
                         dora_plan** out) {
  return dora::build_tensor_plan(tensor, device_type, out);
}

int dora_gpu_plan_tensor_struct(const dora_tensor_field* fields, size_t n,
                                ArrowDeviceType device_type, dora_plan** out) {
  return dora::build_tensor_struct_plan(fields, n, device_type, out);
}

int dora_gpu_plan_tensor_list(const dora_tensor_list* list, ArrowDeviceType device_type,
                              dora_plan** out) {
  return dora::build_tensor_list_plan(list, device_type, out);
}

int dora_gpu_plan_tensor_cast(const dora_tensor_field* fields, size_t n,
                              const dora_tensor_cast* casts, ArrowDeviceType device_type,
                              dora_plan** out) {
  return dora::build_tensor_cast_plan(fields, n, casts, device_type, out);
}

int dora_gpu_plan_tensor_convert(const dora_tensor_field* fields, size_t n,
                                 const dora_tensor_cast* casts, const dora_tensor_quant* quants,
                                 ArrowDeviceType device_type, dora_plan** out) {
  return dora::build_tensor_convert_plan(fields, n, casts, quants, device_type, out);
}

int dora_gpu_plan_tensor_reduce(const dora_tensor_field* fields, size_t n,
                                const dora_tensor_reduce* reduces, ArrowDeviceType device_type,
                                dora_plan** out) {
  return dora::build_tensor_reduce_plan(fields, n, reduces, device_type, out);
}

int dora_gpu_plan_tensor_crop(const dora_tensor_field* fields, size_t n,
                              const dora_tensor_crop* crops, ArrowDeviceType device_type,
                              dora_plan** out) {
  return dora::build_tensor_crop_plan(fields, n, crops, device_type, out);
}

int dora_gpu_plan_tensor_prep(const dora_tensor_field* fields, size_t n,
                              const dora_tensor_resize* resizes, const dora_tensor_crop* crops,
                              const dora_tensor_prep* preps, ArrowDeviceType device_type,
                              dora_plan** out) {
  return dora::build_tensor_prep_plan(fields, n, resizes, crops, preps, device_type, out);
}

int dora_gpu_plan_tensor_resize(const dora_tensor_field* fields, size_t n,
                                const dora_tensor_resize* resizes, ArrowDeviceType device_type,
                                dora_plan** out) {
  return dora::build_tensor_resize_plan(fields, n, resizes, device_type, out);
}

int dora_gpu_plan_tensor_affine(const dora_tensor_field* fields, size_t n,
                                const dora_tensor_cast* casts, const dora_tensor_quant* quants,
                                const dora_tensor_affine* affines, ArrowDeviceType device_type,
                                dora_plan** out) {
  return dora::build_tensor_affine_plan(fields, n, casts, quants, affines, device_type, out);
}

int dora_gpu_plan_tensor_take(const dora_tensor_take* take, ArrowDeviceType device_type,
                              dora_plan** out) {
  return dora::build_tensor_take_plan(take, device_type, out);
}

}  // extern "C"
