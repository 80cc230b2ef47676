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
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "common.h"
#include "plan.h"

namespace dora {

namespace {

// Row-major walk of the view: one memcpy per row, an odometer over the dimensions.  The source
// position is kept as an offset from `src` (a negative stride steps below it and back).
void gather_host(const StridedView& g, uint8_t* dst) {
  int64_t idx[kMaxTensorDims] = {0};
  int64_t off = 0;
  for (uint64_t done = 0; done < g.total; done += g.row) {
    std::memcpy(dst + done, g.src + off, g.row);
    for (int k = g.nd - 1; k >= 0; --k) {
      off += g.stride[k];
      if (++idx[k] < g.shape[k]) break;
      off -= g.stride[k] * g.shape[k];
      idx[k] = 0;
    }
  }
}

// DLPack type codes (dlpack.h, DLDataTypeCode)
enum { DL_INT = 0, DL_UINT = 1, DL_FLOAT = 2, DL_BFLOAT = 4, DL_COMPLEX = 5, DL_BOOL = 6 };

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
  set_error("tensor dtype (code %u, %u bits) is not supported: int and uint of 8/16/32/64 bits "
            "and float of 16/32/64 bits are", code, bits);
  return nullptr;
}

// The type info chain of shape[0..ndim) over a leaf of `bytes` bytes, as build_plan's walk
// serialises the equivalent array: every node carries its own type as a top-level schema.
void tensor_type_info(const char* leaf, const int64_t* shape, int ndim, uint64_t bytes,
                      TypeInfoNode& root) {
  std::vector<ArrowSchema> sch(static_cast<size_t>(ndim));
  std::vector<ArrowSchema*> child(static_cast<size_t>(ndim), nullptr);
  std::vector<std::string> fmt(static_cast<size_t>(ndim));
  for (int i = 0; i < ndim; ++i) {
    ArrowSchema& s = sch[size_t(i)];
    std::memset(&s, 0, sizeof(s));
    fmt[size_t(i)] = i + 1 < ndim ? "+w:" + std::to_string(shape[i + 1]) : std::string(leaf);
    s.format = fmt[size_t(i)].c_str();
    s.name = i ? "item" : "";
    s.flags = i ? ARROW_FLAG_NULLABLE : 0;
    if (i + 1 < ndim) {
      child[size_t(i)] = &sch[size_t(i) + 1];
      s.children = &child[size_t(i)];
      s.n_children = 1;
    }
  }
  TypeInfoNode* node = &root;
  uint64_t len = 1;
  for (int i = 0; i < ndim; ++i) {
    len *= static_cast<uint64_t>(shape[i]);
    serialize_schema(&sch[size_t(i)], true, node->schema);
    node->len = len;
    if (i + 1 < ndim) {
      node->children.emplace_back();
      node = &node->children.back();
    } else {
      node->bufs.push_back({0, bytes});
    }
  }
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

}  // namespace

int build_tensor_plan(const dora_tensor* t, ArrowDeviceType dev, dora_plan** out) {
  if (!out) return fail(DORA_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (!t) return fail(DORA_ERR_INVALID, "tensor is NULL");
  if (dev != ARROW_DEVICE_CPU && dev != ARROW_DEVICE_ROCM_HOST && dev != ARROW_DEVICE_ROCM)
    return fail(DORA_ERR_INVALID, "unsupported device_type %d", dev);
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
  if (!t->data && count) return fail(DORA_ERR_INVALID, "tensor data is NULL");

  // canonical view: no extents of 1, mergeable neighbours merged
  std::vector<Dim> dims;
  {
    int64_t rm = elem;  // row-major stride when strides is NULL
    std::vector<int64_t> sb(static_cast<size_t>(t->ndim));
    for (int i = t->ndim - 1; i >= 0; --i) {
      if (t->strides) {
        if (__builtin_mul_overflow(t->strides[i], elem, &sb[size_t(i)]))
          return fail(DORA_ERR_INVALID, "tensor stride %d overflows 64 bits", i);
      } else {
        sb[size_t(i)] = rm;
        rm *= t->shape[i] ? t->shape[i] : 1;
      }
    }
    for (int i = 0; i < t->ndim && count; ++i) {
      if (t->shape[i] == 1) continue;
      const Dim d{t->shape[i], sb[size_t(i)]};
      int64_t span;  // bytes one step of the previous dimension must cover to merge
      if (!dims.empty() && !__builtin_mul_overflow(d.n, d.s, &span) && dims.back().s == span) {
        dims.back().n *= d.n;
        dims.back().s = d.s;
      } else {
        dims.push_back(d);
      }
    }
  }
  if (dims.size() > size_t(kMaxTensorDims))
    return fail(DORA_ERR_UNSUPPORTED, "tensor view has %zu dimensions after merging (at most %d)",
                dims.size(), kMaxTensorDims);

  DORA_GUARD_BEGIN
  std::unique_ptr<dora_plan> p(new dora_plan());
  p->dev = dev;
  p->size = bytes;
  tensor_type_info(leaf, t->shape, t->ndim, bytes, p->root);
  if (bytes == 0) {
    *out = p.release();
    return DORA_OK;
  }
  const uint8_t* base = static_cast<const uint8_t*>(t->data) + t->byte_offset;
  // an innermost unit stride folds into a row of bytes
  uint64_t row = static_cast<uint64_t>(elem);
  if (!dims.empty() && dims.back().s == elem) {
    row = static_cast<uint64_t>(dims.back().n) * static_cast<uint64_t>(elem);
    dims.pop_back();
  }
  // dense pageable memory: exactly dora_gpu_plan_bytes' plan, with the nested type info.  Pinned
  // memory is staged even when dense: copies and kernels reading it are asynchronous to the
  // host, and the send promises that the source has been read when it returns.
  if (dims.empty() && dev == ARROW_DEVICE_CPU) {
    p->segs.push_back({base, 0, bytes});
    *out = p.release();
    return DORA_OK;
  }
  StridedView g{};
  g.src = base;
  g.total = bytes;
  g.row = row;
  g.nd = static_cast<int>(dims.size());
  for (size_t i = 0; i < dims.size(); ++i) {
    g.shape[i] = dims[i].n;
    g.stride[i] = dims[i].s;
  }
  if (dev == ARROW_DEVICE_ROCM) {
    // device memory is never dereferenced here: a dense view is dora_gpu_plan_bytes' plan with
    // the nested type info (every device path unchanged), a strided one the gather kernel's
    // descriptor and no segments
    p->dev_tensor = true;
    p->gd.view = g;
    p->gd.elem = static_cast<uint32_t>(elem);
    if (!reach(g, &p->gd.lo, &p->gd.hi))
      return fail(DORA_ERR_INVALID, "tensor view's reach overflows 64 bits (extent - 1 times "
                  "stride, summed over its dimensions)");
    if (dims.empty()) p->segs.push_back({base, 0, bytes});
    else p->gather = true;
    *out = p.release();
    return DORA_OK;
  }
  // what the caller's own copy to contiguous memory would have done: every host path (inline
  // Vec, shared memory, BAR fill, DMA) then sees a dense pageable source
  p->staged.resize(bytes);
  gather_host(g, p->staged.data());
  p->dev = ARROW_DEVICE_CPU;  // pageable memory, whatever the view's was
  p->segs.push_back({p->staged.data(), 0, bytes});
  *out = p.release();
  return DORA_OK;
  DORA_GUARD_END
}

}  // namespace dora

extern "C" {

int dora_gpu_plan_tensor(const dora_tensor* tensor, ArrowDeviceType device_type,
                         dora_plan** out) {
  return dora::build_tensor_plan(tensor, device_type, out);
}

}  // extern "C"
