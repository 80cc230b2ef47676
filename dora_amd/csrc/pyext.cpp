// dora_amd._dora_node: the per-send hot path of the Python node API as a CPython extension.
//
// The reference's Python node is a native extension too (PyO3: apis/python/node/src/lib.rs:
// 157-185 `send_output`, whose metadata goes through pydict_to_metadata,
// apis/python/operator/src/lib.rs:165-186).  Through ctypes a send paid ~1 us encoding the
// parameters in Python and ~0.9 us of ctypes argument conversion; here both are one METH_FASTCALL
// call.  The GIL is released around the library call: a send may wait for drop tokens that
// another Python thread of the same process returns.
//
// The receive side likewise: next_event returns an event's fields and decoded parameters in one
// call (the reference: PyO3 `Node.next` -> PyEvent, apis/python/node/src/lib.rs:89-108), instead
// of ~8 ctypes calls and a Python decode (30 us per inline 8-byte input through ctypes).
//
// Every function returns the library's status code; dora_amd/node.py raises on non-zero (the
// message comes from dora_gpu_last_error), so error behaviour is the ctypes path's.
#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <time.h>

#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "dora_gpu.h"

namespace {

void put_u32(std::string& o, uint32_t v) { o.append(reinterpret_cast<const char*>(&v), 4); }
void put_u64(std::string& o, uint64_t v) { o.append(reinterpret_cast<const char*>(&v), 8); }

// MetadataParameters encoding (include/dora_gpu.h, dora_node_send_output_sample): u32 count,
// then per entry in sorted key order: u64 key length, key, u8 tag (0 bool, 1 int, 2 string),
// value (u8 | i64 | u64 length + utf-8).  Anything else is stringified (str(v)), as
// pydict_to_metadata does.  Same bytes as dora_amd.node.encode_parameters_py.
bool encode(PyObject* meta, std::string& out) {
  out.clear();
  if (meta == nullptr || meta == Py_None) return true;
  if (!PyDict_Check(meta)) {
    PyErr_SetString(PyExc_TypeError, "metadata must be a dict or None");
    return false;
  }
  if (PyDict_GET_SIZE(meta) == 0) return true;
  PyObject* keys = PyDict_Keys(meta);
  if (!keys) return false;
  if (PyList_Sort(keys) < 0) {
    Py_DECREF(keys);
    return false;
  }
  const Py_ssize_t n = PyList_GET_SIZE(keys);
  put_u32(out, uint32_t(n));
  bool ok = true;
  for (Py_ssize_t i = 0; ok && i < n; ++i) {
    PyObject* k = PyList_GET_ITEM(keys, i);
    PyObject* ks = PyUnicode_Check(k) ? (Py_INCREF(k), k) : PyObject_Str(k);
    if (!ks) {
      ok = false;
      break;
    }
    Py_ssize_t kl = 0;
    const char* kb = PyUnicode_AsUTF8AndSize(ks, &kl);
    if (!kb) {
      Py_DECREF(ks);
      ok = false;
      break;
    }
    put_u64(out, uint64_t(kl));
    out.append(kb, size_t(kl));
    Py_DECREF(ks);
    PyObject* v = PyDict_GetItemWithError(meta, k);  // borrowed
    if (!v) {
      ok = false;
      break;
    }
    if (PyBool_Check(v)) {
      out.push_back(char(0));
      out.push_back(char(v == Py_True ? 1 : 0));
    } else if (PyLong_Check(v)) {
      const long long x = PyLong_AsLongLong(v);
      if (x == -1 && PyErr_Occurred()) {
        ok = false;  // OverflowError, as struct.pack("<q") raises
        break;
      }
      out.push_back(char(1));
      put_u64(out, uint64_t(x));
    } else {
      PyObject* s = PyUnicode_Check(v) ? (Py_INCREF(v), v) : PyObject_Str(v);
      if (!s) {
        ok = false;
        break;
      }
      Py_ssize_t sl = 0;
      const char* sb = PyUnicode_AsUTF8AndSize(s, &sl);
      if (!sb) {
        Py_DECREF(s);
        ok = false;
        break;
      }
      out.push_back(char(2));
      put_u64(out, uint64_t(sl));
      out.append(sb, size_t(sl));
      Py_DECREF(s);
    }
  }
  Py_DECREF(keys);
  return ok;
}

thread_local std::string t_params;

bool as_ptr(PyObject* o, void** p) {
  if (o == Py_None) {
    *p = nullptr;
    return true;
  }
  *p = PyLong_AsVoidPtr(o);
  return !(*p == nullptr && PyErr_Occurred());
}

const char* as_cstr(PyObject* o) {
  if (PyBytes_Check(o)) return PyBytes_AS_STRING(o);
  if (PyUnicode_Check(o)) return PyUnicode_AsUTF8(o);
  PyErr_SetString(PyExc_TypeError, "output id must be str or bytes");
  return nullptr;
}

PyObject* py_encode_parameters(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 1) {
    PyErr_SetString(PyExc_TypeError, "encode_parameters(metadata)");
    return nullptr;
  }
  if (!encode(args[0], t_params)) return nullptr;
  return PyBytes_FromStringAndSize(t_params.data(), Py_ssize_t(t_params.size()));
}

// Optional trailing `flags` argument (DORA_SEND_ASYNC) of send_bytes / send_array.
bool send_flags(PyObject* const* args, Py_ssize_t nargs, uint32_t* flags) {
  *flags = 0;
  if (nargs < 7) return true;
  const unsigned long f = PyLong_AsUnsignedLong(args[6]);
  if (f == static_cast<unsigned long>(-1) && PyErr_Occurred()) return false;
  *flags = static_cast<uint32_t>(f);
  return true;
}

// send_bytes(handle, output_id, data_ptr, len, device_type, metadata[, flags]) -> status
PyObject* py_send_bytes(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 6 && nargs != 7) {
    PyErr_SetString(PyExc_TypeError,
                    "send_bytes(handle, output_id, data_ptr, len, device_type, metadata[, flags])");
    return nullptr;
  }
  uint32_t flags = 0;
  if (!send_flags(args, nargs, &flags)) return nullptr;
  void *h = nullptr, *data = nullptr;
  if (!as_ptr(args[0], &h) || !as_ptr(args[2], &data)) return nullptr;
  const char* oid = as_cstr(args[1]);
  if (!oid) return nullptr;
  const size_t len = PyLong_AsSize_t(args[3]);
  if (len == size_t(-1) && PyErr_Occurred()) return nullptr;
  const long dev = PyLong_AsLong(args[4]);
  if (dev == -1 && PyErr_Occurred()) return nullptr;
  std::string& params = t_params;
  if (!encode(args[5], params)) return nullptr;
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_send_output_bytes_ex(static_cast<dora_node*>(h), oid, data, len,
                                      static_cast<ArrowDeviceType>(dev),
                                      reinterpret_cast<const uint8_t*>(params.data()),
                                      params.size(), flags);
  Py_END_ALLOW_THREADS
  return PyLong_FromLong(rc);
}

// send_buffer(handle, output_id, buffer, metadata) -> status: host bytes (any object with the
// buffer protocol: bytes, bytearray, memoryview, numpy) as send_output_bytes of a host source,
// read in place — the call copies them (inline below 4096 B, else into a slot) before it returns
PyObject* py_send_buffer(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 4) {
    PyErr_SetString(PyExc_TypeError, "send_buffer(handle, output_id, buffer, metadata)");
    return nullptr;
  }
  void* h = nullptr;
  if (!as_ptr(args[0], &h)) return nullptr;
  const char* oid = as_cstr(args[1]);
  if (!oid) return nullptr;
  Py_buffer view;
  if (PyObject_GetBuffer(args[2], &view, PyBUF_C_CONTIGUOUS) != 0) return nullptr;
  std::string& params = t_params;
  if (!encode(args[3], params)) {
    PyBuffer_Release(&view);
    return nullptr;
  }
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_send_output_bytes_ex(static_cast<dora_node*>(h), oid, view.buf,
                                      static_cast<size_t>(view.len), ARROW_DEVICE_CPU,
                                      reinterpret_cast<const uint8_t*>(params.data()),
                                      params.size(), 0);
  Py_END_ALLOW_THREADS
  PyBuffer_Release(&view);
  return PyLong_FromLong(rc);
}

// send_array(handle, output_id, array_addr, schema_addr, device_type, metadata[, flags])
PyObject* py_send_array(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 6 && nargs != 7) {
    PyErr_SetString(PyExc_TypeError, "send_array(handle, output_id, array_addr, schema_addr, "
                                     "device_type, metadata[, flags])");
    return nullptr;
  }
  uint32_t flags = 0;
  if (!send_flags(args, nargs, &flags)) return nullptr;
  void *h = nullptr, *arr = nullptr, *sch = nullptr;
  if (!as_ptr(args[0], &h) || !as_ptr(args[2], &arr) || !as_ptr(args[3], &sch)) return nullptr;
  const char* oid = as_cstr(args[1]);
  if (!oid) return nullptr;
  const long dev = PyLong_AsLong(args[4]);
  if (dev == -1 && PyErr_Occurred()) return nullptr;
  std::string& params = t_params;
  if (!encode(args[5], params)) return nullptr;
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_send_output_ex(static_cast<dora_node*>(h), oid,
                                static_cast<const struct ArrowArray*>(arr),
                                static_cast<const struct ArrowSchema*>(sch),
                                static_cast<ArrowDeviceType>(dev),
                                reinterpret_cast<const uint8_t*>(params.data()), params.size(),
                                flags);
  Py_END_ALLOW_THREADS
  return PyLong_FromLong(rc);
}

// The layout of DLPack's DLManagedTensor (dlpack.h, unversioned capsules named "dltensor");
// restated, not vendored.
struct DlTensor {
  void* data;
  int32_t device_type, device_id;
  int32_t ndim;
  uint8_t code, bits;
  uint16_t lanes;
  int64_t* shape;
  int64_t* strides;
  uint64_t byte_offset;
};
struct DlManaged {
  DlTensor t;
  void* ctx;
  void (*deleter)(DlManaged*);
};

void to_tensor(const DlTensor& d, dora_tensor& t) {
  t = dora_tensor{};
  t.data = d.data;
  t.byte_offset = d.byte_offset;
  t.dtype_code = d.code;
  t.dtype_bits = d.bits;
  t.dtype_lanes = d.lanes;
  t.ndim = d.ndim;
  t.shape = d.shape;
  t.strides = d.strides;
}

const char* const kUnused = "a DLPack capsule named \"dltensor\" (an unused, unversioned one)";

// The "dltensor" capsules of one tensor send and what becomes of them, as DLPack prescribes.
// First every capsule is taken and checked — the fields' (`take`), then whatever else travels
// with the call (`also`: a partition, an index, a mask; `table`: an affine table), each against
// all taken before it.  Nothing is touched yet: a call refused for any argument leaves its
// capsules as they were.  Then `consume` renames each "used_dltensor" and describes its tensor
// where the taker said.  The destructor runs the deleter of every capsule consumed, once: under
// the GIL and after the status has been taken, since it runs as the send function returns (a
// deleter may run Python code: numpy's and torch's drop a reference; it does not disturb the
// thread's error message, which the caller reads only when the status is not 0 and deleters do
// not call the library).
class Capsules {
 public:
  std::vector<dora_tensor_field> fields;

  Capsules() = default;
  Capsules(const Capsules&) = delete;
  Capsules& operator=(const Capsules&) = delete;
  ~Capsules() {
    for (const Item& it : items_)
      if (it.consumed && it.consumed->deleter) it.consumed->deleter(it.consumed);
  }

  // The fields: `names` a tuple of str as long as the tuple `caps`, or — `bare_ok` — None over a
  // tuple of one capsule (a bare tensor: no name); anything else is refused with `usage`.
  // `numbered`: the call has more capsules than fields, and two that are one are refused by their
  // numbers among all of them.
  bool take(PyObject* names, PyObject* caps, const char* usage, bool bare_ok, bool numbered) {
    if (!PyTuple_Check(caps) ||
        !(names == Py_None ? bare_ok && PyTuple_GET_SIZE(caps) == 1
                           : PyTuple_Check(names) &&
                                 PyTuple_GET_SIZE(names) == PyTuple_GET_SIZE(caps))) {
      PyErr_SetString(PyExc_TypeError, usage);
      return false;
    }
    const Py_ssize_t n = PyTuple_GET_SIZE(caps);
    fields.assign(static_cast<size_t>(n), dora_tensor_field{});
    items_.reserve(static_cast<size_t>(n) + 2);
    for (Py_ssize_t k = 0; k < n; ++k) {
      dora_tensor_field& f = fields[size_t(k)];
      if (names != Py_None && !(f.name = as_cstr(PyTuple_GET_ITEM(names, k)))) return false;
      PyObject* cap = PyTuple_GET_ITEM(caps, k);
      if (!PyCapsule_IsValid(cap, "dltensor")) {
        PyErr_Format(PyExc_TypeError, "field %zd: expected %s", k, kUnused);
        return false;
      }
      if (const Py_ssize_t j = find(cap); j >= 0) {
        PyErr_Format(PyExc_TypeError, numbered ? "capsules %zd and %zd are one capsule"
                                               : "fields %zd and %zd share one capsule", j, k);
        return false;
      }
      items_.push_back({cap, &f.tensor, nullptr});
    }
    return true;
  }

  // One more capsule, its tensor described into `*into`; `what` names it in a refusal (NULL: the
  // one tensor of send_tensor).
  bool also(PyObject* cap, dora_tensor* into, const char* what) {
    if (!PyCapsule_IsValid(cap, "dltensor")) {
      if (what) PyErr_Format(PyExc_TypeError, "%s: expected %s", what, kUnused);
      else PyErr_Format(PyExc_TypeError, "expected %s", kUnused);
      return false;
    }
    if (const Py_ssize_t j = find(cap); j >= 0) {
      PyErr_Format(PyExc_TypeError, "capsules %zd and %zd are one capsule", j,
                   static_cast<Py_ssize_t>(items_.size()));
      return false;
    }
    items_.push_back({cap, into, nullptr});
    return true;
  }

  // A per-channel table of field `k`.
  bool table(PyObject* cap, dora_tensor* into, Py_ssize_t k) {
    if (!PyCapsule_IsValid(cap, "dltensor")) {
      PyErr_Format(PyExc_TypeError, "field %zd: a table is %s", k, kUnused);
      return false;
    }
    if (const Py_ssize_t j = find(cap); j >= 0) {
      PyErr_Format(PyExc_TypeError, size_t(j) < fields.size()
                                        ? "field %zd: a table shares a field's capsule"
                                        : "field %zd: two tables share one capsule", k);
      return false;
    }
    items_.push_back({cap, into, nullptr});
    return true;
  }

  bool consume() {
    for (Item& it : items_) {
      auto* m = static_cast<DlManaged*>(PyCapsule_GetPointer(it.cap, "dltensor"));
      // (cannot fail after the checks above; the capsules renamed so far are released as all are)
      if (!m || PyCapsule_SetName(it.cap, "used_dltensor") != 0) return false;
      it.consumed = m;
      to_tensor(m->t, *it.into);
    }
    return true;
  }

 private:
  struct Item {
    PyObject* cap;
    dora_tensor* into;
    DlManaged* consumed;  // set once the capsule is renamed: its deleter is then ours to call
  };
  Py_ssize_t find(PyObject* cap) const {
    for (size_t j = 0; j < items_.size(); ++j)
      if (items_[j].cap == cap) return static_cast<Py_ssize_t>(j);
    return -1;
  }
  std::vector<Item> items_;
};

// What every tensor send takes beside its tensors: the node, the output id, the device type of
// the values, the metadata (encoded into t_params) and the flags.
struct Frame {
  dora_node* node;
  const char* oid;
  ArrowDeviceType dev;
  const uint8_t* params;
  size_t params_len;
  uint32_t flags;

  bool take(PyObject* handle, PyObject* output_id, PyObject* device_type, PyObject* metadata,
            PyObject* send_flags) {
    void* h = nullptr;
    if (!as_ptr(handle, &h) || !(oid = as_cstr(output_id))) return false;
    node = static_cast<dora_node*>(h);
    const long d = PyLong_AsLong(device_type);
    if (d == -1 && PyErr_Occurred()) return false;
    dev = static_cast<ArrowDeviceType>(d);
    const unsigned long f = PyLong_AsUnsignedLong(send_flags);
    if (f == static_cast<unsigned long>(-1) && PyErr_Occurred()) return false;
    flags = static_cast<uint32_t>(f);
    if (!encode(metadata, t_params)) return false;
    params = reinterpret_cast<const uint8_t*>(t_params.data());
    params_len = t_params.size();
    return true;
  }
};

// Whether `entries` is a tuple as long as the tuple `caps`.
bool as_long(PyObject* entries, PyObject* caps) {
  return PyTuple_Check(entries) && PyTuple_Check(caps) &&
         PyTuple_GET_SIZE(entries) == PyTuple_GET_SIZE(caps);
}

// send_tensor(handle, output_id, capsule, device_type, metadata, flags) -> status: the tensor of
// a "dltensor" capsule (an object's __dlpack__()) as dora_node_send_output_tensor.  The capsule
// is consumed (Capsules): renamed "used_dltensor", its deleter called once the call has returned
// (a host source has then been read).
PyObject* py_send_tensor(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 6) {
    PyErr_SetString(PyExc_TypeError,
                    "send_tensor(handle, output_id, capsule, device_type, metadata, flags)");
    return nullptr;
  }
  Capsules caps;
  Frame f;
  dora_tensor t;
  if (!caps.also(args[2], &t, nullptr) || !f.take(args[0], args[1], args[3], args[4], args[5]) ||
      !caps.consume())
    return nullptr;
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_send_output_tensor(f.node, f.oid, &t, f.dev, f.params, f.params_len, f.flags);
  Py_END_ALLOW_THREADS
  return PyLong_FromLong(rc);
}

// send_tensor_struct(handle, output_id, names, capsules, device_type, metadata, flags) -> status:
// the tensors of a tuple of "dltensor" capsules under a tuple of names as
// dora_node_send_output_tensor_struct.  Every capsule is consumed the way send_tensor consumes
// its one.
PyObject* py_send_tensor_struct(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  const char* usage = "send_tensor_struct(handle, output_id, names, capsules, device_type, "
                      "metadata, flags): names and capsules are tuples of one length";
  if (nargs != 7) {
    PyErr_SetString(PyExc_TypeError, usage);
    return nullptr;
  }
  Capsules caps;
  Frame f;
  if (!caps.take(args[2], args[3], usage, false, false) ||
      !f.take(args[0], args[1], args[4], args[5], args[6]) || !caps.consume())
    return nullptr;
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_send_output_tensor_struct(f.node, f.oid, caps.fields.data(), caps.fields.size(),
                                           f.dev, f.params, f.params_len, f.flags);
  Py_END_ALLOW_THREADS
  return PyLong_FromLong(rc);
}

// send_tensor_cast(handle, output_id, names, capsules, casts, device_type, metadata, flags) ->
// status: tensors converted on send as dora_node_send_output_tensor_cast.  `names` / `capsules` as
// send_tensor_list takes them; `casts` a tuple as long, each entry None (the field is sent as it
// is) or (dtype_code, dtype_bits, scale or None).  Every capsule is consumed as send_tensor_struct
// consumes its own.
// send_tensor_convert takes the same arguments and sends as dora_node_send_output_tensor_convert:
// an entry may then also be (dtype_code, dtype_bits, scale or None, zero_point), a quantised field.
// With a ninth argument `affines`, a tuple as long, it sends as
// dora_node_send_output_tensor_affine: each entry None or (scale table or None, bias table or
// None, axis, scalar bias or None), a table a "dltensor" capsule that is consumed like a field's.
PyObject* send_converted(PyObject* const* args, Py_ssize_t nargs, bool convert) {
  const char* usage = convert
      ? "send_tensor_convert(handle, output_id, names, capsules, entries, device_type, metadata, "
        "flags): names is None over one capsule or a tuple as long as the tuple of capsules; "
        "entries a tuple as long, of None, (code, bits, scale) or (code, bits, scale, zero_point)"
      : "send_tensor_cast(handle, output_id, names, capsules, casts, device_type, "
        "metadata, flags): names is None over one capsule or a tuple as long as the "
        "tuple of capsules; casts a tuple as long, of None or (code, bits, scale)";
  // (send_tensor_convert alone: a ninth argument, the affine entries)
  const bool with_affine = convert && nargs == 9;
  if ((nargs != 8 && !with_affine) || !as_long(args[4], args[3]) ||
      (with_affine && !as_long(args[8], args[3]))) {
    PyErr_SetString(PyExc_TypeError, usage);
    return nullptr;
  }
  Capsules caps;
  if (!caps.take(args[2], args[3], usage, true, false)) return nullptr;
  const size_t n = caps.fields.size();
  std::vector<dora_tensor_cast> casts(n);
  std::vector<dora_tensor_quant> quants(convert ? n : 0);
  for (size_t k = 0; k < n; ++k) {
    PyObject* entry = PyTuple_GET_ITEM(args[4], Py_ssize_t(k));
    if (entry == Py_None) continue;
    if (!PyTuple_Check(entry) ||
        !(PyTuple_GET_SIZE(entry) == 3 || (convert && PyTuple_GET_SIZE(entry) == 4))) {
      PyErr_SetString(PyExc_TypeError, usage);
      return nullptr;
    }
    const bool quant = PyTuple_GET_SIZE(entry) == 4;
    const long code = PyLong_AsLong(PyTuple_GET_ITEM(entry, 0));
    const long bits = PyLong_AsLong(PyTuple_GET_ITEM(entry, 1));
    if (PyErr_Occurred()) return nullptr;
    if (code < 0 || code > 255 || bits < 1 || bits > 255) {
      PyErr_Format(PyExc_TypeError, "field %zu: cast dtype (code %ld, %ld bits)", k, code, bits);
      return nullptr;
    }
    PyObject* scale = PyTuple_GET_ITEM(entry, 2);
    double factor = 0.0;
    if (scale != Py_None) {
      factor = PyFloat_AsDouble(scale);
      if (factor == -1.0 && PyErr_Occurred()) return nullptr;
    }
    if (quant) {
      const long zp = PyLong_AsLong(PyTuple_GET_ITEM(entry, 3));
      if (zp == -1 && PyErr_Occurred()) return nullptr;
      if (zp < INT32_MIN || zp > INT32_MAX) {
        PyErr_Format(PyExc_TypeError, "field %zu: zero point %ld", k, zp);
        return nullptr;
      }
      dora_tensor_quant& q = quants[k];
      q.dtype_code = static_cast<uint8_t>(code);
      q.dtype_bits = static_cast<uint8_t>(bits);
      q.has_scale = scale != Py_None;
      q.scale = static_cast<float>(factor);
      q.zero_point = static_cast<int32_t>(zp);
      continue;
    }
    dora_tensor_cast& c = casts[k];
    c.dtype_code = static_cast<uint8_t>(code);
    c.dtype_bits = static_cast<uint8_t>(bits);
    if (scale != Py_None) {
      c.has_scale = 1;
      c.scale = static_cast<float>(factor);
    }
  }
  // the affine entries: None, or (scale table capsule or None, bias table capsule or None, axis,
  // scalar bias or None); the tables' capsules are consumed with the fields'
  std::vector<dora_tensor_affine> affines(with_affine ? n : 0);
  std::vector<dora_tensor> tables(with_affine ? 2 * n : 0);  // field k's scale, then its bias
  for (size_t k = 0; with_affine && k < n; ++k) {
    PyObject* entry = PyTuple_GET_ITEM(args[8], Py_ssize_t(k));
    if (entry == Py_None) continue;
    if (!PyTuple_Check(entry) || PyTuple_GET_SIZE(entry) != 4) {
      PyErr_Format(PyExc_TypeError, "field %zu: an affine entry is None or (scale table, bias "
                                    "table, axis, bias)", k);
      return nullptr;
    }
    dora_tensor_affine& a = affines[k];
    for (size_t w = 0; w < 2; ++w) {
      PyObject* cap = PyTuple_GET_ITEM(entry, Py_ssize_t(w));
      if (cap == Py_None) continue;
      if (!caps.table(cap, &tables[2 * k + w], Py_ssize_t(k))) return nullptr;
      (w ? a.bias : a.scale) = &tables[2 * k + w];
    }
    const long axis = PyLong_AsLong(PyTuple_GET_ITEM(entry, 2));
    if (axis == -1 && PyErr_Occurred()) return nullptr;
    if (axis < INT32_MIN || axis > INT32_MAX) {
      PyErr_Format(PyExc_TypeError, "field %zu: axis %ld", k, axis);
      return nullptr;
    }
    a.axis = static_cast<int32_t>(axis);
    PyObject* bias = PyTuple_GET_ITEM(entry, 3);
    if (bias != Py_None) {
      const double b = PyFloat_AsDouble(bias);
      if (b == -1.0 && PyErr_Occurred()) return nullptr;
      a.has_bias = 1;
      a.bias_value = static_cast<float>(b);
    }
  }
  Frame f;
  if (!f.take(args[0], args[1], args[5], args[6], args[7]) || !caps.consume()) return nullptr;
  int rc;
  Py_BEGIN_ALLOW_THREADS
  if (with_affine)
    rc = dora_node_send_output_tensor_affine(f.node, f.oid, caps.fields.data(), n, casts.data(),
                                             quants.data(), affines.data(), f.dev, f.params,
                                             f.params_len, f.flags);
  else if (convert)
    rc = dora_node_send_output_tensor_convert(f.node, f.oid, caps.fields.data(), n, casts.data(),
                                              quants.data(), f.dev, f.params, f.params_len,
                                              f.flags);
  else
    rc = dora_node_send_output_tensor_cast(f.node, f.oid, caps.fields.data(), n, casts.data(),
                                           f.dev, f.params, f.params_len, f.flags);
  Py_END_ALLOW_THREADS
  return PyLong_FromLong(rc);
}

PyObject* py_send_tensor_cast(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  return send_converted(args, nargs, false);
}
PyObject* py_send_tensor_convert(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  return send_converted(args, nargs, true);
}

// send_tensor_reduce(handle, output_id, names, capsules, reduces, device_type, metadata, flags)
// -> status: tensors reduced on send as dora_node_send_output_tensor_reduce.  `names` / `capsules`
// as send_tensor_cast takes them; `reduces` a tuple as long, each entry None (the field is sent as
// it is) or (op, axis, dtype_code, dtype_bits).  Every capsule is consumed as send_tensor_struct
// consumes its own.
PyObject* py_send_tensor_reduce(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  const char* usage =
      "send_tensor_reduce(handle, output_id, names, capsules, reduces, device_type, metadata, "
      "flags): names is None over one capsule or a tuple as long as the tuple of capsules; "
      "reduces a tuple as long, of None or (op, axis, code, bits)";
  if (nargs != 8 || !as_long(args[4], args[3])) {
    PyErr_SetString(PyExc_TypeError, usage);
    return nullptr;
  }
  Capsules caps;
  if (!caps.take(args[2], args[3], usage, true, false)) return nullptr;
  const size_t n = caps.fields.size();
  std::vector<dora_tensor_reduce> reduces(n);
  for (size_t k = 0; k < n; ++k) {
    PyObject* entry = PyTuple_GET_ITEM(args[4], Py_ssize_t(k));
    if (entry == Py_None) continue;
    if (!PyTuple_Check(entry) || PyTuple_GET_SIZE(entry) != 4) {
      PyErr_SetString(PyExc_TypeError, usage);
      return nullptr;
    }
    const long op = PyLong_AsLong(PyTuple_GET_ITEM(entry, 0));
    const long axis = PyLong_AsLong(PyTuple_GET_ITEM(entry, 1));
    const long code = PyLong_AsLong(PyTuple_GET_ITEM(entry, 2));
    const long bits = PyLong_AsLong(PyTuple_GET_ITEM(entry, 3));
    if (PyErr_Occurred()) return nullptr;
    if (op < 1 || op > INT32_MAX || axis < INT32_MIN || axis > INT32_MAX || code < 0 ||
        code > 255 || bits < 1 || bits > 255) {
      PyErr_Format(PyExc_TypeError, "field %zu: reduce entry (op %ld, axis %ld, code %ld, %ld "
                                    "bits)", k, op, axis, code, bits);
      return nullptr;
    }
    dora_tensor_reduce& r = reduces[k];
    r.op = static_cast<uint32_t>(op);
    r.axis = static_cast<int32_t>(axis);
    r.dtype_code = static_cast<uint8_t>(code);
    r.dtype_bits = static_cast<uint8_t>(bits);
  }
  Frame f;
  if (!f.take(args[0], args[1], args[5], args[6], args[7]) || !caps.consume()) return nullptr;
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_send_output_tensor_reduce(f.node, f.oid, caps.fields.data(), n, reduces.data(),
                                           f.dev, f.params, f.params_len, f.flags);
  Py_END_ALLOW_THREADS
  return PyLong_FromLong(rc);
}

// send_tensor_resize(handle, output_id, names, capsules, resizes, device_type, metadata, flags)
// -> status: tensors resized on send as dora_node_send_output_tensor_resize.  `names` / `capsules`
// as send_tensor_cast takes them; `resizes` a tuple as long, each entry None (the field is sent as
// it is) or (mode, axis0, axis1, size0, size1, dtype_code, dtype_bits).  Every capsule is consumed
// as send_tensor_struct consumes its own.
PyObject* py_send_tensor_resize(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  const char* usage =
      "send_tensor_resize(handle, output_id, names, capsules, resizes, device_type, metadata, "
      "flags): names is None over one capsule or a tuple as long as the tuple of capsules; "
      "resizes a tuple as long, of None or (mode, axis0, axis1, size0, size1, code, bits)";
  if (nargs != 8 || !as_long(args[4], args[3])) {
    PyErr_SetString(PyExc_TypeError, usage);
    return nullptr;
  }
  Capsules caps;
  if (!caps.take(args[2], args[3], usage, true, false)) return nullptr;
  const size_t n = caps.fields.size();
  std::vector<dora_tensor_resize> resizes(n);
  for (size_t k = 0; k < n; ++k) {
    PyObject* entry = PyTuple_GET_ITEM(args[4], Py_ssize_t(k));
    if (entry == Py_None) continue;
    if (!PyTuple_Check(entry) || PyTuple_GET_SIZE(entry) != 7) {
      PyErr_SetString(PyExc_TypeError, usage);
      return nullptr;
    }
    long long w[7];
    for (int j = 0; j < 7; ++j) w[j] = PyLong_AsLongLong(PyTuple_GET_ITEM(entry, j));
    if (PyErr_Occurred()) return nullptr;
    if (w[0] < 1 || w[0] > INT32_MAX || w[1] < INT32_MIN || w[1] > INT32_MAX ||
        w[2] < INT32_MIN || w[2] > INT32_MAX || w[5] < 0 || w[5] > 255 || w[6] < 0 ||
        w[6] > 255) {
      PyErr_Format(PyExc_TypeError, "field %zu: resize entry (mode %lld, axes %lld and %lld, "
                                    "code %lld, %lld bits)", k, w[0], w[1], w[2], w[5], w[6]);
      return nullptr;
    }
    dora_tensor_resize& r = resizes[k];
    r.mode = static_cast<uint32_t>(w[0]);
    r.axis[0] = static_cast<int32_t>(w[1]);
    r.axis[1] = static_cast<int32_t>(w[2]);
    r.size[0] = static_cast<int64_t>(w[3]);
    r.size[1] = static_cast<int64_t>(w[4]);
    r.dtype_code = static_cast<uint8_t>(w[5]);
    r.dtype_bits = static_cast<uint8_t>(w[6]);
  }
  Frame f;
  if (!f.take(args[0], args[1], args[5], args[6], args[7]) || !caps.consume()) return nullptr;
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_send_output_tensor_resize(f.node, f.oid, caps.fields.data(), n, resizes.data(),
                                           f.dev, f.params, f.params_len, f.flags);
  Py_END_ALLOW_THREADS
  return PyLong_FromLong(rc);
}

// send_tensor_crops(handle, output_id, names, capsules, crops, device_type, metadata, flags)
// -> status: crops cut and resized on send as dora_node_send_output_tensor_crop.  `names` /
// `capsules` as send_tensor_cast takes them; `crops` a tuple as long, each entry None (the field is
// sent as it is) or (mode, axis0, axis1, size0, size1, dtype_code, dtype_bits, boxes), `boxes` a
// "dltensor" capsule of the [K, 4] int32 boxes, which joins the fields' capsules: every capsule is
// consumed as send_tensor_struct consumes its own.
PyObject* py_send_tensor_crops(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  const char* usage =
      "send_tensor_crops(handle, output_id, names, capsules, crops, device_type, metadata, "
      "flags): names is None over one capsule or a tuple as long as the tuple of capsules; "
      "crops a tuple as long, of None or (mode, axis0, axis1, size0, size1, code, bits, boxes)";
  if (nargs != 8 || !as_long(args[4], args[3])) {
    PyErr_SetString(PyExc_TypeError, usage);
    return nullptr;
  }
  Capsules caps;
  if (!caps.take(args[2], args[3], usage, true, false)) return nullptr;
  const size_t n = caps.fields.size();
  std::vector<dora_tensor_crop> crops(n);
  std::vector<dora_tensor> boxes(n);
  for (size_t k = 0; k < n; ++k) {
    PyObject* entry = PyTuple_GET_ITEM(args[4], Py_ssize_t(k));
    if (entry == Py_None) continue;
    if (!PyTuple_Check(entry) || PyTuple_GET_SIZE(entry) != 8) {
      PyErr_SetString(PyExc_TypeError, usage);
      return nullptr;
    }
    long long w[7];
    for (int j = 0; j < 7; ++j) w[j] = PyLong_AsLongLong(PyTuple_GET_ITEM(entry, j));
    if (PyErr_Occurred()) return nullptr;
    if (w[0] < 1 || w[0] > INT32_MAX || w[1] < INT32_MIN || w[1] > INT32_MAX ||
        w[2] < INT32_MIN || w[2] > INT32_MAX || w[5] < 0 || w[5] > 255 || w[6] < 0 ||
        w[6] > 255) {
      PyErr_Format(PyExc_TypeError, "field %zu: crops entry (mode %lld, axes %lld and %lld, "
                                    "code %lld, %lld bits)", k, w[0], w[1], w[2], w[5], w[6]);
      return nullptr;
    }
    char what[48];
    std::snprintf(what, sizeof(what), "field %zu: the boxes", k);
    if (!caps.also(PyTuple_GET_ITEM(entry, 7), &boxes[k], what)) return nullptr;
    dora_tensor_crop& c = crops[k];
    c.mode = static_cast<uint32_t>(w[0]);
    c.axis[0] = static_cast<int32_t>(w[1]);
    c.axis[1] = static_cast<int32_t>(w[2]);
    c.size[0] = static_cast<int64_t>(w[3]);
    c.size[1] = static_cast<int64_t>(w[4]);
    c.dtype_code = static_cast<uint8_t>(w[5]);
    c.dtype_bits = static_cast<uint8_t>(w[6]);
    c.boxes = &boxes[k];
  }
  Frame f;
  if (!f.take(args[0], args[1], args[5], args[6], args[7]) || !caps.consume()) return nullptr;
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_send_output_tensor_crop(f.node, f.oid, caps.fields.data(), n, crops.data(),
                                         f.dev, f.params, f.params_len, f.flags);
  Py_END_ALLOW_THREADS
  return PyLong_FromLong(rc);
}

// send_tensor_prep(handle, output_id, names, capsules, entries, preps, device_type, metadata,
// flags) -> status: model inputs as dora_node_send_output_tensor_prep.  `names` / `capsules` as
// send_tensor_cast takes them; `entries` a tuple as long, each entry None, a resize entry (7
// items, send_tensor_resize) or a crops entry (8 items, send_tensor_crops); `preps` a tuple as
// long, each entry None or (scale table or None, bias table or None, axis, scalar scale or None,
// scalar bias or None, inner0, inner1, lead0, lead1, fill), a table a "dltensor" capsule.  Every
// capsule, the boxes' and the tables' included, is consumed as send_tensor_struct consumes its
// own.
PyObject* py_send_tensor_prep(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  const char* usage =
      "send_tensor_prep(handle, output_id, names, capsules, entries, preps, device_type, "
      "metadata, flags): names is None over one capsule or a tuple as long as the tuple of "
      "capsules; entries a tuple as long, of None, (mode, axis0, axis1, size0, size1, code, bits) "
      "or the same with boxes; preps a tuple as long, of None or (scale table, bias table, axis, "
      "scale, bias, inner0, inner1, lead0, lead1, fill)";
  if (nargs != 9 || !as_long(args[4], args[3]) || !as_long(args[5], args[3])) {
    PyErr_SetString(PyExc_TypeError, usage);
    return nullptr;
  }
  Capsules caps;
  if (!caps.take(args[2], args[3], usage, true, false)) return nullptr;
  const size_t n = caps.fields.size();
  std::vector<dora_tensor_resize> resizes(n);
  std::vector<dora_tensor_crop> crops(n);
  std::vector<dora_tensor_prep> preps(n);
  std::vector<dora_tensor> boxes(n), tables(2 * n);  // field k's scale table, then its bias
  for (size_t k = 0; k < n; ++k) {
    PyObject* entry = PyTuple_GET_ITEM(args[4], Py_ssize_t(k));
    if (entry != Py_None) {
      if (!PyTuple_Check(entry) || (PyTuple_GET_SIZE(entry) != 7 && PyTuple_GET_SIZE(entry) != 8)) {
        PyErr_SetString(PyExc_TypeError, usage);
        return nullptr;
      }
      long long w[7];
      for (int j = 0; j < 7; ++j) w[j] = PyLong_AsLongLong(PyTuple_GET_ITEM(entry, j));
      if (PyErr_Occurred()) return nullptr;
      if (w[0] < 1 || w[0] > INT32_MAX || w[1] < INT32_MIN || w[1] > INT32_MAX ||
          w[2] < INT32_MIN || w[2] > INT32_MAX || w[5] < 0 || w[5] > 255 || w[6] < 0 ||
          w[6] > 255) {
        PyErr_Format(PyExc_TypeError, "field %zu: entry (mode %lld, axes %lld and %lld, code "
                                      "%lld, %lld bits)", k, w[0], w[1], w[2], w[5], w[6]);
        return nullptr;
      }
      if (PyTuple_GET_SIZE(entry) == 8) {
        char what[48];
        std::snprintf(what, sizeof(what), "field %zu: the boxes", k);
        if (!caps.also(PyTuple_GET_ITEM(entry, 7), &boxes[k], what)) return nullptr;
        dora_tensor_crop& c = crops[k];
        c.mode = static_cast<uint32_t>(w[0]);
        c.axis[0] = static_cast<int32_t>(w[1]);
        c.axis[1] = static_cast<int32_t>(w[2]);
        c.size[0] = static_cast<int64_t>(w[3]);
        c.size[1] = static_cast<int64_t>(w[4]);
        c.dtype_code = static_cast<uint8_t>(w[5]);
        c.dtype_bits = static_cast<uint8_t>(w[6]);
        c.boxes = &boxes[k];
      } else {
        dora_tensor_resize& r = resizes[k];
        r.mode = static_cast<uint32_t>(w[0]);
        r.axis[0] = static_cast<int32_t>(w[1]);
        r.axis[1] = static_cast<int32_t>(w[2]);
        r.size[0] = static_cast<int64_t>(w[3]);
        r.size[1] = static_cast<int64_t>(w[4]);
        r.dtype_code = static_cast<uint8_t>(w[5]);
        r.dtype_bits = static_cast<uint8_t>(w[6]);
      }
    }
    PyObject* prep = PyTuple_GET_ITEM(args[5], Py_ssize_t(k));
    if (prep == Py_None) continue;
    if (!PyTuple_Check(prep) || PyTuple_GET_SIZE(prep) != 10) {
      PyErr_Format(PyExc_TypeError, "field %zu: a prep entry is None or (scale table, bias table, "
                                    "axis, scale, bias, inner0, inner1, lead0, lead1, fill)", k);
      return nullptr;
    }
    dora_tensor_prep& p = preps[k];
    for (size_t t = 0; t < 2; ++t) {
      PyObject* cap = PyTuple_GET_ITEM(prep, Py_ssize_t(t));
      if (cap == Py_None) continue;
      if (!caps.table(cap, &tables[2 * k + t], Py_ssize_t(k))) return nullptr;
      (t ? p.bias : p.scale) = &tables[2 * k + t];
    }
    const long axis = PyLong_AsLong(PyTuple_GET_ITEM(prep, 2));
    if (axis == -1 && PyErr_Occurred()) return nullptr;
    if (axis < INT32_MIN || axis > INT32_MAX) {
      PyErr_Format(PyExc_TypeError, "field %zu: axis %ld", k, axis);
      return nullptr;
    }
    p.axis = static_cast<int32_t>(axis);
    for (int t = 0; t < 2; ++t) {
      PyObject* v = PyTuple_GET_ITEM(prep, 3 + t);
      if (v == Py_None) continue;
      const double x = PyFloat_AsDouble(v);
      if (x == -1.0 && PyErr_Occurred()) return nullptr;
      (t ? p.has_bias : p.has_scale) = 1;
      (t ? p.bias_value : p.scale_value) = static_cast<float>(x);
    }
    for (int j = 0; j < 4; ++j) {
      const long long v = PyLong_AsLongLong(PyTuple_GET_ITEM(prep, 5 + j));
      if (v == -1 && PyErr_Occurred()) return nullptr;
      (j < 2 ? p.inner[j] : p.lead[j - 2]) = static_cast<int64_t>(v);
    }
    const double fill = PyFloat_AsDouble(PyTuple_GET_ITEM(prep, 9));
    if (fill == -1.0 && PyErr_Occurred()) return nullptr;
    p.fill = static_cast<float>(fill);
  }
  Frame f;
  if (!f.take(args[0], args[1], args[6], args[7], args[8]) || !caps.consume()) return nullptr;
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_send_output_tensor_prep(f.node, f.oid, caps.fields.data(), n, resizes.data(),
                                         crops.data(), preps.data(), f.dev, f.params,
                                         f.params_len, f.flags);
  Py_END_ALLOW_THREADS
  return PyLong_FromLong(rc);
}

// send_tensor_list(handle, output_id, names, capsules, partition, form, partition_device,
// device_type, metadata, flags) -> status: a ragged batch as dora_node_send_output_tensor_list.
// `names` is a tuple of str over the tuple `capsules`, or None over a tuple of one capsule (a bare
// tensor); `partition` a "dltensor" capsule of the 1-D lengths or offsets.  Every capsule, the
// partition's included, is consumed as send_tensor_struct consumes its own.
PyObject* py_send_tensor_list(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  const char* usage = "send_tensor_list(handle, output_id, names, capsules, partition, form, "
                      "partition_device, device_type, metadata, flags): names is None over one "
                      "capsule or a tuple as long as the tuple of capsules";
  if (nargs != 10) {
    PyErr_SetString(PyExc_TypeError, usage);
    return nullptr;
  }
  Capsules caps;
  dora_tensor_list list{};
  if (!caps.take(args[2], args[3], usage, true, true) ||
      !caps.also(args[4], &list.partition, "partition"))
    return nullptr;
  const long form = PyLong_AsLong(args[5]);
  if (form == -1 && PyErr_Occurred()) return nullptr;
  const long pdev = PyLong_AsLong(args[6]);
  if (pdev == -1 && PyErr_Occurred()) return nullptr;
  Frame f;
  if (!f.take(args[0], args[1], args[7], args[8], args[9]) || !caps.consume()) return nullptr;
  list.fields = caps.fields.data();
  list.n = caps.fields.size();
  list.partition_form = static_cast<uint32_t>(form);
  list.partition_device = static_cast<ArrowDeviceType>(pdev);
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_send_output_tensor_list(f.node, f.oid, &list, f.dev, f.params, f.params_len,
                                         f.flags);
  Py_END_ALLOW_THREADS
  return PyLong_FromLong(rc);
}

// send_tensor_take(handle, output_id, names, capsules, index, index_device, partition, form,
// partition_device, device_type, metadata, flags) -> status: rows taken by an index as
// dora_node_send_output_tensor_take.  `names` / `capsules` as send_tensor_list takes them; `index`
// a "dltensor" capsule of the 1-D row numbers; `partition` one of lengths or offsets over the
// taken rows, or None (no lists).  Every capsule is consumed as send_tensor_list consumes its own.
//
// send_tensor_masked takes the same twelve arguments with the mask (a "dltensor" capsule of the N
// bool or uint8 elements) and its device where the index and its device are, the partition over
// the N source rows, and sends as dora_node_send_output_tensor_mask.
PyObject* send_selected(PyObject* const* args, Py_ssize_t nargs, bool masked) {
  const char* usage = masked
      ? "send_tensor_masked(handle, output_id, names, capsules, mask, mask_device, "
        "partition, form, partition_device, device_type, metadata, flags): names is "
        "None over one capsule or a tuple as long as the tuple of capsules"
      : "send_tensor_take(handle, output_id, names, capsules, index, index_device, "
        "partition, form, partition_device, device_type, metadata, flags): names is "
        "None over one capsule or a tuple as long as the tuple of capsules";
  if (nargs != 12) {
    PyErr_SetString(PyExc_TypeError, usage);
    return nullptr;
  }
  const bool lists = args[6] != Py_None;
  Capsules caps;
  dora_tensor_take take{};
  dora_tensor_mask mask{};
  dora_tensor partition{};
  if (!caps.take(args[2], args[3], usage, true, true) ||
      !(masked ? caps.also(args[4], &mask.mask, "mask") : caps.also(args[4], &take.index, "index")) ||
      (lists && !caps.also(args[6], &partition, "partition")))
    return nullptr;
  long num[3];  // index_device, form, partition_device
  for (int i = 0; i < 3; ++i) {
    num[i] = PyLong_AsLong(args[i ? 6 + i : 5]);
    if (num[i] == -1 && PyErr_Occurred()) return nullptr;
  }
  Frame f;
  if (!f.take(args[0], args[1], args[9], args[10], args[11]) || !caps.consume()) return nullptr;
  take.fields = caps.fields.data();
  take.n = caps.fields.size();
  take.index_device = static_cast<ArrowDeviceType>(num[0]);
  take.partition = lists ? &partition : nullptr;
  take.partition_form = static_cast<uint32_t>(num[1]);
  take.partition_device = static_cast<ArrowDeviceType>(num[2]);
  mask.fields = take.fields;
  mask.n = take.n;
  mask.mask_device = take.index_device;
  mask.partition = take.partition;
  mask.partition_form = take.partition_form;
  mask.partition_device = take.partition_device;
  int rc;
  Py_BEGIN_ALLOW_THREADS
  if (masked)
    rc = dora_node_send_output_tensor_mask(f.node, f.oid, &mask, f.dev, f.params, f.params_len,
                                           f.flags);
  else
    rc = dora_node_send_output_tensor_take(f.node, f.oid, &take, f.dev, f.params, f.params_len,
                                           f.flags);
  Py_END_ALLOW_THREADS
  return PyLong_FromLong(rc);
}

PyObject* py_send_tensor_take(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  return send_selected(args, nargs, false);
}

PyObject* py_send_tensor_masked(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  return send_selected(args, nargs, true);
}

// MetadataParameters bytes -> dict (the inverse of encode; dora_amd.node.decode_parameters).
PyObject* decode(const uint8_t* p, size_t n) {
  PyObject* out = PyDict_New();
  if (!out || n < 4) return out;
  auto rd = [&](size_t at, size_t w, void* v) {
    if (at + w > n) return false;
    std::memcpy(v, p + at, w);
    return true;
  };
  uint32_t count = 0;
  rd(0, 4, &count);
  size_t i = 4;
  for (uint32_t e = 0; e < count; ++e) {
    uint64_t kl = 0;
    if (!rd(i, 8, &kl) || kl > n - i - 8) goto bad;
    i += 8;
    {
      PyObject* key = PyUnicode_DecodeUTF8(reinterpret_cast<const char*>(p + i), Py_ssize_t(kl), nullptr);
      if (!key) goto fail;
      i += kl;
      PyObject* val = nullptr;
      if (i >= n) {
        Py_DECREF(key);
        goto bad;
      }
      const uint8_t tag = p[i++];
      if (tag == 0) {
        if (i >= n) {
          Py_DECREF(key);
          goto bad;
        }
        val = PyBool_FromLong(p[i++] != 0);
      } else if (tag == 1) {
        int64_t x = 0;
        if (!rd(i, 8, &x)) {
          Py_DECREF(key);
          goto bad;
        }
        i += 8;
        val = PyLong_FromLongLong(x);
      } else {
        uint64_t sl = 0;
        if (!rd(i, 8, &sl) || sl > n - i - 8) {
          Py_DECREF(key);
          goto bad;
        }
        i += 8;
        val = PyUnicode_DecodeUTF8(reinterpret_cast<const char*>(p + i), Py_ssize_t(sl), nullptr);
        i += sl;
      }
      if (!val) {
        Py_DECREF(key);
        goto fail;
      }
      const int rc = PyDict_SetItem(out, key, val);
      Py_DECREF(key);
      Py_DECREF(val);
      if (rc < 0) goto fail;
    }
  }
  return out;
bad:
  PyErr_SetString(PyExc_ValueError, "truncated metadata parameters");
fail:
  Py_DECREF(out);
  return nullptr;
}

PyObject* params_of(const dora_event* ev) {
  const uint8_t* p = nullptr;
  size_t n = 0;
  if (dora_event_parameters(ev, &p, &n) != 0) return PyDict_New();
  return decode(p, n);
}

// next_event(handle, timeout_us) -> status (int) | (event_ptr, type, id, parameters, timestamp_ns,
// data_ptr, data_len, on_device, error).  The caller owns event_ptr (dora_event_free).  Inputs
// carry their decoded parameters; other events None.
PyObject* py_next_event(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 2) {
    PyErr_SetString(PyExc_TypeError, "next_event(handle, timeout_us)");
    return nullptr;
  }
  void* h = nullptr;
  if (!as_ptr(args[0], &h)) return nullptr;
  const long long timeout = PyLong_AsLongLong(args[1]);
  if (timeout == -1 && PyErr_Occurred()) return nullptr;
  dora_event* ev = nullptr;
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_next_event(static_cast<dora_node*>(h), timeout, &ev);
  Py_END_ALLOW_THREADS
  if (rc != 0) return PyLong_FromLong(rc);
  const int type = dora_event_type(ev);
  PyObject* params = nullptr;
  const void* dp = nullptr;
  size_t dn = 0;
  int dev = 0;
  if (type == DORA_EVENT_INPUT) {
    params = params_of(ev);
    if (!params) {
      dora_event_free(ev);
      return nullptr;
    }
    // the data's address (a device input's mapping is opened here); its failure is the call's
    const int drc = dora_event_data(ev, &dp, &dn);
    if (drc != 0) {
      Py_DECREF(params);
      dora_event_free(ev);
      return PyLong_FromLong(drc);
    }
    dev = dora_event_is_device(ev);
  } else {
    Py_INCREF(Py_None);
    params = Py_None;
  }
  const char* err = type == DORA_EVENT_ERROR ? dora_event_error(ev) : "";
  PyObject* out =
      Py_BuildValue("(KisNKKnis)", static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(ev)),
                    type, dora_event_id(ev), params,
                    static_cast<unsigned long long>(dora_event_timestamp_ns(ev)),
                    static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(dp)),
                    static_cast<Py_ssize_t>(dn), dev, err);
  if (!out) dora_event_free(ev);  // (an id or error that is not UTF-8)
  return out;
}

// wait_input(handle, input_id, key, value, timeout_us) -> status (int) | parameters: the next
// input on `input_id` whose parameters have key == value; other events are consumed and freed.
PyObject* py_wait_input(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 5) {
    PyErr_SetString(PyExc_TypeError, "wait_input(handle, input_id, key, value, timeout_us)");
    return nullptr;
  }
  void* h = nullptr;
  if (!as_ptr(args[0], &h)) return nullptr;
  const char* want = as_cstr(args[1]);
  if (!want) return nullptr;
  long long left = PyLong_AsLongLong(args[4]);
  if (left == -1 && PyErr_Occurred()) return nullptr;
  const std::string want_id(want);
  PyObject* key = args[2];
  PyObject* value = args[3];
  for (;;) {
    dora_event* ev = nullptr;
    int rc;
    uint64_t t0 = 0, t1 = 0;
    Py_BEGIN_ALLOW_THREADS
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    t0 = uint64_t(ts.tv_sec) * 1000000000ull + uint64_t(ts.tv_nsec);
    rc = dora_node_next_event(static_cast<dora_node*>(h), left, &ev);
    clock_gettime(CLOCK_MONOTONIC, &ts);
    t1 = uint64_t(ts.tv_sec) * 1000000000ull + uint64_t(ts.tv_nsec);
    Py_END_ALLOW_THREADS
    if (rc != 0) return PyLong_FromLong(rc);
    left -= static_cast<long long>((t1 - t0) / 1000);
    if (dora_event_type(ev) == DORA_EVENT_INPUT && want_id == dora_event_id(ev)) {
      PyObject* params = params_of(ev);
      if (!params) {
        dora_event_free(ev);
        return nullptr;
      }
      PyObject* v = PyDict_GetItemWithError(params, key);  // borrowed
      const int eq = v ? PyObject_RichCompareBool(v, value, Py_EQ) : (PyErr_Occurred() ? -1 : 0);
      dora_event_free(ev);
      if (eq < 0) {
        Py_DECREF(params);
        return nullptr;
      }
      if (eq) return params;
      Py_DECREF(params);
    } else {
      dora_event_free(ev);
    }
    if (left <= 0) return PyLong_FromLong(DORA_ERR_TIMEOUT);
  }
}

// A pyarrow type's exported ArrowSchema, kept: a send lends it (dora_node_send_output borrows
// the schema), so a node sending arrays of one type exports each array only, not its type again
// (~3 us for a struct).  Looked up by the type object itself first, then by equality (a new
// array of an equal type) confirmed with field metadata (DataType.__eq__ ignores it, the
// serialized type keeps it); at most 64 types are kept.
void free_schema_capsule(PyObject* cap) {
  auto* s = static_cast<ArrowSchema*>(PyCapsule_GetPointer(cap, "dora_schema"));
  if (s && s->release) s->release(s);
  std::free(s);
}

PyObject* g_schemas = nullptr;   // type -> (type, capsule)
PyObject* g_last_type = nullptr;  // the last type sent and its capsule (strong references)
PyObject* g_last_cap = nullptr;

// A new reference to the capsule of `type`'s schema.  The caller keeps it for as long as the
// schema is in use (a send releases the GIL: another thread may evict the entry meanwhile).
PyObject* schema_for(PyObject* type) {
  if (type == g_last_type) {
    Py_INCREF(g_last_cap);
    return g_last_cap;
  }
  if (!g_schemas && !(g_schemas = PyDict_New())) return nullptr;
  PyObject* cap = nullptr;
  PyObject* hit = PyDict_GetItemWithError(g_schemas, type);  // borrowed (type, capsule)
  if (!hit && PyErr_Occurred()) return nullptr;
  if (hit) {
    // a strong reference for the call into Python below: code there may release the GIL, and
    // another sending thread may then clear g_schemas or replace this entry
    Py_INCREF(hit);
    PyObject* key = PyTuple_GET_ITEM(hit, 0);
    int same = key == type;
    if (!same) {
      // type.equals(key, check_metadata=True)
      static PyObject* kw = Py_BuildValue("{s:O}", "check_metadata", Py_True);
      PyObject* eq = kw ? PyObject_GetAttrString(type, "equals") : nullptr;
      PyObject* a = eq ? PyTuple_Pack(1, key) : nullptr;
      PyObject* r = a ? PyObject_Call(eq, a, kw) : nullptr;
      Py_XDECREF(a);
      Py_XDECREF(eq);
      if (!r) {
        Py_DECREF(hit);
        return nullptr;
      }
      same = PyObject_IsTrue(r);
      Py_DECREF(r);
      if (same < 0) {
        Py_DECREF(hit);
        return nullptr;
      }
    }
    if (same) {
      cap = PyTuple_GET_ITEM(hit, 1);
      Py_INCREF(cap);
    }
    Py_DECREF(hit);
  }
  if (!cap) {  // export it (replacing an entry equal but for field metadata)
    if (PyDict_GET_SIZE(g_schemas) >= 64) PyDict_Clear(g_schemas);
    auto* sc = static_cast<ArrowSchema*>(std::calloc(1, sizeof(ArrowSchema)));
    if (!sc) return PyErr_NoMemory();
    PyObject* r = PyObject_CallMethod(type, "_export_to_c", "K",
                                      static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(sc)));
    if (!r) {
      std::free(sc);
      return nullptr;
    }
    Py_DECREF(r);
    cap = PyCapsule_New(sc, "dora_schema", free_schema_capsule);
    if (!cap) {
      if (sc->release) sc->release(sc);
      std::free(sc);
      return nullptr;
    }
    PyObject* entry = PyTuple_Pack(2, type, cap);
    if (!entry || PyDict_SetItem(g_schemas, type, entry) < 0) {
      Py_XDECREF(entry);
      Py_DECREF(cap);
      return nullptr;
    }
    Py_DECREF(entry);
  }
  Py_INCREF(type);
  Py_XSETREF(g_last_type, type);
  Py_INCREF(cap);
  Py_XSETREF(g_last_cap, cap);
  return cap;
}

// send_pyarrow(handle, output_id, array, metadata) -> status: a host pyarrow.Array, exported
// (its type's schema from schema_for) and sent as dora_node_send_output of a host source, which
// copies it before returning (apis/python/node/src/lib.rs:157-185 -> arrow_utils.rs:23-71).
PyObject* py_send_pyarrow(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 4) {
    PyErr_SetString(PyExc_TypeError, "send_pyarrow(handle, output_id, array, metadata)");
    return nullptr;
  }
  void* h = nullptr;
  if (!as_ptr(args[0], &h)) return nullptr;
  const char* oid = as_cstr(args[1]);
  if (!oid) return nullptr;
  PyObject* type = PyObject_GetAttrString(args[2], "type");
  if (!type) return nullptr;
  PyObject* cap = schema_for(type);
  Py_DECREF(type);
  if (!cap) return nullptr;
  auto* schema = static_cast<ArrowSchema*>(PyCapsule_GetPointer(cap, "dora_schema"));
  std::string& params = t_params;
  ArrowArray a{};
  PyObject* r = encode(args[3], params) && schema
                    ? PyObject_CallMethod(args[2], "_export_to_c", "K",
                                          static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(&a)))
                    : nullptr;
  if (!r) {
    Py_DECREF(cap);
    return nullptr;
  }
  Py_DECREF(r);
  int rc;
  Py_BEGIN_ALLOW_THREADS
  rc = dora_node_send_output_ex(static_cast<dora_node*>(h), oid, &a, schema, ARROW_DEVICE_CPU,
                                reinterpret_cast<const uint8_t*>(params.data()), params.size(), 0);
  Py_END_ALLOW_THREADS
  if (a.release) a.release(&a);
  Py_DECREF(cap);
  return PyLong_FromLong(rc);
}

// export_array(event_ptr) -> status (int) | (array_addr, schema_addr): the input's Arrow C
// structs (dora_event_array) in memory of this module, for pyarrow's _import_from_c, which moves
// their contents out; free_arrow(array_addr, schema_addr) then releases what is left and frees
// them (one native call each instead of two ctypes structures and a ctypes call).
PyObject* py_export_array(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 1) {
    PyErr_SetString(PyExc_TypeError, "export_array(event_ptr)");
    return nullptr;
  }
  void* ev = nullptr;
  if (!as_ptr(args[0], &ev)) return nullptr;
  auto* a = static_cast<ArrowArray*>(std::calloc(1, sizeof(ArrowArray)));
  auto* s = static_cast<ArrowSchema*>(std::calloc(1, sizeof(ArrowSchema)));
  if (!a || !s) {
    std::free(a);
    std::free(s);
    return PyErr_NoMemory();
  }
  const int rc = dora_event_array(static_cast<const dora_event*>(ev), a, s);
  if (rc != 0) {
    std::free(a);
    std::free(s);
    return PyLong_FromLong(rc);
  }
  return Py_BuildValue("(KK)", static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(a)),
                       static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(s)));
}

// A schema's identity as bytes: format, name, flags, metadata and children, recursively.
void schema_key(const ArrowSchema* s, std::string& k) {
  k += s->format ? s->format : "";
  k.push_back('\0');
  k += s->name ? s->name : "";
  k.push_back('\0');
  put_u64(k, uint64_t(s->flags));
  if (s->metadata) {  // int32 count, then per pair int32 length + bytes, twice
    const char* m = s->metadata;
    int32_t n = 0;
    std::memcpy(&n, m, 4);
    size_t len = 4;
    for (int32_t i = 0; i < 2 * n; ++i) {
      int32_t l = 0;
      std::memcpy(&l, m + len, 4);
      len += 4 + size_t(l);
    }
    put_u64(k, len);
    k.append(m, len);
  } else {
    put_u64(k, 0);
  }
  put_u64(k, uint64_t(s->n_children));
  for (int64_t i = 0; i < s->n_children; ++i) schema_key(s->children[i], k);
  k.push_back(s->dictionary ? 'D' : 'N');
  if (s->dictionary) schema_key(s->dictionary, k);
}

PyObject* g_types = nullptr;     // schema key -> pyarrow.DataType
PyObject* g_pa_dtype = nullptr;  // pyarrow.DataType

// export_typed(event_ptr) -> status (int) | (array_addr, pyarrow.DataType): as export_array, but
// the input's type comes from a cache keyed by its schema (pyarrow imports a schema in ~1-1.4 us
// per event; Array._import_from_c takes the DataType instead).  free_arrow(array_addr, 0) after
// the import.
PyObject* py_export_typed(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 1) {
    PyErr_SetString(PyExc_TypeError, "export_typed(event_ptr)");
    return nullptr;
  }
  void* ev = nullptr;
  if (!as_ptr(args[0], &ev)) return nullptr;
  if (!g_pa_dtype) {
    PyObject* pa = PyImport_ImportModule("pyarrow");
    if (!pa) return nullptr;
    g_pa_dtype = PyObject_GetAttrString(pa, "DataType");
    Py_DECREF(pa);
    if (!g_pa_dtype) return nullptr;
  }
  if (!g_types && !(g_types = PyDict_New())) return nullptr;
  auto* a = static_cast<ArrowArray*>(std::calloc(1, sizeof(ArrowArray)));
  ArrowSchema s{};
  if (!a) return PyErr_NoMemory();
  const int rc = dora_event_array(static_cast<const dora_event*>(ev), a, &s);
  if (rc != 0) {
    std::free(a);
    return PyLong_FromLong(rc);
  }
  std::string key;
  schema_key(&s, key);
  PyObject* kb = PyBytes_FromStringAndSize(key.data(), Py_ssize_t(key.size()));
  PyObject* dtype = kb ? PyDict_GetItemWithError(g_types, kb) : nullptr;  // borrowed
  if (dtype) {
    Py_INCREF(dtype);
  } else if (kb && !PyErr_Occurred()) {
    dtype = PyObject_CallMethod(g_pa_dtype, "_import_from_c", "K",
                                static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(&s)));
    if (dtype) {
      if (PyDict_GET_SIZE(g_types) >= 256) PyDict_Clear(g_types);
      if (PyDict_SetItem(g_types, kb, dtype) < 0) Py_CLEAR(dtype);
    }
  }
  Py_XDECREF(kb);
  if (s.release) s.release(&s);  // (moved out when pyarrow imported it)
  if (!dtype) {
    if (a->release) a->release(a);
    std::free(a);
    return nullptr;
  }
  return Py_BuildValue("(KN)", static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(a)),
                       dtype);
}

PyObject* py_free_arrow(PyObject*, PyObject* const* args, Py_ssize_t nargs) {
  if (nargs != 2) {
    PyErr_SetString(PyExc_TypeError, "free_arrow(array_addr, schema_addr)");
    return nullptr;
  }
  void *a = nullptr, *s = nullptr;
  if (!as_ptr(args[0], &a) || !as_ptr(args[1], &s)) return nullptr;
  auto* arr = static_cast<ArrowArray*>(a);
  auto* sch = static_cast<ArrowSchema*>(s);
  if (arr && arr->release) arr->release(arr);  // not imported (an error before the move)
  if (sch && sch->release) sch->release(sch);
  std::free(arr);
  std::free(sch);
  Py_RETURN_NONE;
}

PyMethodDef methods[] = {
    {"send_pyarrow", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_pyarrow)),
     METH_FASTCALL, "dora_node_send_output of a host pyarrow.Array (its type's schema kept)."},
    {"export_array", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_export_array)),
     METH_FASTCALL, "An input's Arrow C structs (dora_event_array), for pyarrow's _import_from_c."},
    {"export_typed", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_export_typed)),
     METH_FASTCALL, "An input's ArrowArray and its pyarrow.DataType (cached by schema)."},
    {"free_arrow", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_free_arrow)),
     METH_FASTCALL, "Release what is left of export_array's structs and free them."},
    {"next_event", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_next_event)),
     METH_FASTCALL, "dora_node_next_event with the event's fields and decoded parameters."},
    {"wait_input", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_wait_input)),
     METH_FASTCALL, "The next input on an id whose parameters have key == value."},
    {"encode_parameters", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_encode_parameters)),
     METH_FASTCALL, "MetadataParameters bytes of a dict (bool / int / str, else str(v))."},
    {"send_bytes", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_bytes)),
     METH_FASTCALL, "dora_node_send_output_bytes with parameters encoded from a dict."},
    {"send_buffer", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_buffer)),
     METH_FASTCALL, "dora_node_send_output_bytes of host bytes read in place (buffer protocol)."},
    {"send_tensor", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_tensor)),
     METH_FASTCALL, "dora_node_send_output_tensor of a DLPack capsule, which it consumes."},
    {"send_tensor_struct",
     reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_tensor_struct)),
     METH_FASTCALL, "dora_node_send_output_tensor_struct of named DLPack capsules, which it consumes."},
    {"send_tensor_list",
     reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_tensor_list)),
     METH_FASTCALL, "dora_node_send_output_tensor_list of DLPack capsules, which it consumes."},
    {"send_tensor_cast",
     reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_tensor_cast)),
     METH_FASTCALL, "dora_node_send_output_tensor_cast of DLPack capsules, which it consumes."},
    {"send_tensor_convert",
     reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_tensor_convert)),
     METH_FASTCALL, "dora_node_send_output_tensor_convert of DLPack capsules, which it consumes."},
    {"send_tensor_reduce",
     reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_tensor_reduce)),
     METH_FASTCALL, "dora_node_send_output_tensor_reduce of DLPack capsules, which it consumes."},
    {"send_tensor_prep",
     reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_tensor_prep)),
     METH_FASTCALL, "dora_node_send_output_tensor_prep of DLPack capsules, which it consumes."},
    {"send_tensor_crops",
     reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_tensor_crops)),
     METH_FASTCALL, "dora_node_send_output_tensor_crop of DLPack capsules, which it consumes."},
    {"send_tensor_resize",
     reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_tensor_resize)),
     METH_FASTCALL, "dora_node_send_output_tensor_resize of DLPack capsules, which it consumes."},
    {"send_tensor_take",
     reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_tensor_take)),
     METH_FASTCALL, "dora_node_send_output_tensor_take of DLPack capsules, which it consumes."},
    {"send_tensor_masked",
     reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_tensor_masked)),
     METH_FASTCALL, "dora_node_send_output_tensor_mask of DLPack capsules, which it consumes."},
    {"send_array", reinterpret_cast<PyCFunction>(reinterpret_cast<void (*)()>(py_send_array)),
     METH_FASTCALL, "dora_node_send_output with parameters encoded from a dict."},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef module = {PyModuleDef_HEAD_INIT, "_dora_node",
                      "Per-send hot path of dora_amd.node (native, like the reference's PyO3 node).",
                      -1, methods, nullptr, nullptr, nullptr, nullptr};

}  // namespace

PyMODINIT_FUNC PyInit__dora_node(void) { return PyModule_Create(&module); }
