"""Python node API on the device data plane — mirrors the reference Python `Node`
(apis/python/node/src/lib.rs:29-185) and its event dicts (apis/python/operator/src/lib.rs:81-165).

    node = Node()                                   # from env (DORA_GPU_DATAFLOW, DORA_NODE_ID)
    for event in node:                              # or node.next(timeout)
        if event["type"] == "INPUT":
            arr = event["value"]                    # DeviceArray: zero-copy view of the HBM sample
            host = arr.to_pyarrow()                 # host staging for pyarrow consumers (F12)
    node.send_output("out", pa.array([...]), {"k": 1})   # host pyarrow: inline < 4096 B, else DMA
    node.send_output("out", device_array)                 # HBM array -> HIP pack kernel
    node.send_output("out", b"raw bytes")                 # ArrowTypeInfo::byte_array
    node.send_output("out", frame.transpose(2, 0, 1))     # a host tensor view (dora_amd.tensor)
    node.send_output("out", frame_cuda.permute(2, 0, 1))  # a torch view in HBM: gathered by a kernel
"""
from __future__ import annotations

import ctypes
import os
import struct
import sys
import time
from ctypes import byref, c_double, c_size_t, c_uint8, c_uint64, c_void_p
from typing import Optional

from . import _lib
from ._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST, DoraGpuError,
                   call, load)
from .arrow_c import ArrowArray, ArrowSchema, CArray

SEND_ASYNC = 1  # DORA_SEND_ASYNC (include/dora_gpu.h)
_DL_ROCM = 10          # DLPack device types: kDLROCM
_DL_CPU = 1
_DL_HOST = (1, 3, 11)  # kDLCPU, kDLCUDAHost, kDLROCMHost (the latter two: pinned)
from .device import DeviceArray, DeviceBuffer
from .tensor import Argmax as _Argmax
from .tensor import Cast as _Cast
from .tensor import Crops as _Crops
from .tensor import Quantized as _Quantized
from .tensor import Ragged as _Ragged
from .tensor import Resized as _Resized
from .tensor import Masked as _Masked
from .tensor import Taken as _Taken
from .type_info import decode

try:
    from . import _dora_node as _fast
except ImportError as e:  # no fallback: the send path is native
    raise ImportError(f"dora_amd._dora_node is missing ({e}): build it with "
                      "`python -m dora_amd.build`") from e

# MetadataParameters bytes of a dict, natively (the send paths encode inside _fast)
encode_parameters = _fast.encode_parameters

EVENT_TYPES = {0: "STOP", 1: "INPUT", 2: "INPUT_CLOSED", 3: "ERROR", 4: "ALL_INPUTS_CLOSED"}


_U32 = struct.Struct("<I").pack
_U64 = struct.Struct("<Q").pack
_TAG_BOOL = struct.Struct("<BB").pack
_TAG_INT = struct.Struct("<Bq").pack
_TAG_STR = struct.Struct("<BQ").pack
_KEYS: dict = {}  # encoded key prefix by key (u64 length + utf-8)


def encode_parameters_py(metadata: Optional[dict]) -> bytes:
    """MetadataParameters encoding (pydict_to_metadata, apis/python/operator/src/lib.rs:165-186:
    bool / int / str, anything else stringified), in Python: the statement of the format that
    tests hold the native encoder (`encode_parameters`, csrc/pyext.cpp) to."""
    if not metadata:
        return b""
    out = [_U32(len(metadata))]
    for k in sorted(metadata):
        v = metadata[k]
        kp = _KEYS.get(k)
        if kp is None:
            kb = str(k).encode()
            kp = _U64(len(kb)) + kb
            if len(_KEYS) < 4096:
                _KEYS[k] = kp
        out.append(kp)
        t = type(v)
        if t is int:
            out.append(_TAG_INT(1, v))
        elif t is bool or isinstance(v, bool):
            out.append(_TAG_BOOL(0, int(v)))
        elif isinstance(v, int):
            out.append(_TAG_INT(1, v))
        else:
            sb = (v if isinstance(v, str) else str(v)).encode()
            out.append(_TAG_STR(2, len(sb)) + sb)
    return b"".join(out)


def decode_parameters(raw: bytes) -> dict:
    if len(raw) < 4:
        return {}
    (n,), i, out = struct.unpack_from("<I", raw), 4, {}
    for _ in range(n):
        (kl,) = struct.unpack_from("<Q", raw, i)
        i += 8
        key = raw[i:i + kl].decode()
        i += kl
        tag = raw[i]
        i += 1
        if tag == 0:
            out[key] = bool(raw[i])
            i += 1
        elif tag == 1:
            (out[key],) = struct.unpack_from("<q", raw, i)
            i += 8
        else:
            (sl,) = struct.unpack_from("<Q", raw, i)
            i += 8
            out[key] = raw[i:i + sl].decode()
            i += sl
    return out


def descriptor_path(region: str) -> str:
    """Where a dataflow's launcher leaves its parsed descriptor (JSON) for its nodes: beside its
    control region in /dev/shm, removed with it."""
    return "/dev/shm/" + region.lstrip("/") + ".descriptor.json"


def _is_pyarrow_array(data) -> bool:
    pa = sys.modules.get("pyarrow")  # an Array exists only once pyarrow is imported
    return pa is not None and isinstance(data, pa.Array)


class _EventHandle:
    """Owns a C dora_event; freeing it (explicitly or by GC) releases the drop token once no
    DeviceArray view references the sample any more."""

    def __init__(self, ptr):
        self.ptr = ptr
        self._lib = load()

    def free(self):
        if self.ptr:
            self._lib.dora_event_free(self.ptr)
            self.ptr = None

    def __del__(self):
        self.free()


class _Event(dict):
    """Event dict whose "type_info" (the input's ArrowTypeInfo, reference inline form) is
    decoded on first access: restoring bitmaps that travelled in the sample's validity tail
    reads them back from HBM, and a receiver that only uses "value" never pays for it."""

    def __missing__(self, key):
        if key != "type_info" or "_event" not in self:
            raise KeyError(key)
        p, n = ctypes.POINTER(c_uint8)(), c_size_t()
        call("dora_event_type_info", self["_event"].ptr, byref(p), byref(n))
        ti = decode(ctypes.string_at(p, n.value))
        self["type_info"] = ti
        return ti


_hip_runtime_checked = False


def _require_one_hip_runtime():
    """A device tensor's producer and this library must share one HIP runtime: a stream or an
    allocation of one runtime means nothing to another.  torch's ROCm wheels carry their own
    libamdhip64; when torch is imported before dora_amd the library binds to it, the other way
    round the process holds two.  Checked once, at the first device tensor send (the producer's
    library is loaded by then)."""
    global _hip_runtime_checked
    if _hip_runtime_checked:
        return
    libs = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                path = line.rsplit(None, 1)[-1]
                if os.path.basename(path).startswith("libamdhip64"):
                    libs.add(os.path.realpath(path))
    except OSError:
        pass
    if len(libs) > 1:
        raise RuntimeError("two HIP runtimes are loaded in this process (" + ", ".join(sorted(libs))
                           + "): a device tensor of one cannot be read through the other. "
                           "Import the tensor's library (torch) before dora_amd, so that both "
                           "use the same one")
    _hip_runtime_checked = True


class Node:
    """The reference's `Node` pyclass (apis/python/node/src/lib.rs:29-209): `Node(node_id=None)`,
    `next(timeout=None)`, iteration (`__iter__` / `__next__`), `send_output(output_id, data,
    metadata=None)`, `dataflow_descriptor()`, `dataflow_id()`, `merge_external_events(...)`.
    Added here: `dataflow` / `device` to join a dataflow by its region name on a given GPU (the
    reference finds a dynamic node's daemon by node id), and the device-side calls below."""

    def __init__(self, node_id: Optional[str] = None, dataflow: Optional[str] = None,
                 device: Optional[int] = None):
        self._lib = load()
        h = c_void_p()
        if node_id is None and dataflow is None:
            call("dora_node_init_from_env", byref(h))
        else:
            shm = dataflow or os.environ["DORA_GPU_DATAFLOW"]
            dev = device if device is not None else int(os.environ.get("DORA_GPU_DEVICE", "0"))
            call("dora_node_init", shm.encode(), node_id.encode(), dev, byref(h))
        self.handle = h.value
        self.id = self._lib.dora_node_id(self.handle).decode()
        self.device = device if device is not None else int(os.environ.get("DORA_GPU_DEVICE", "0"))
        self._region = dataflow or os.environ.get("DORA_GPU_DATAFLOW", "")
        self._async_tensors = []  # device tensors of asynchronous sends, held until sync()
        # the node's own default (dora_node_init reads the same variable; set_async_sends)
        self._async_default = os.environ.get("DORA_GPU_SEND_ASYNC", "")[:1] == "1"

    # -------------------------------------------------------------------------------- sending
    def send_output(self, output_id: str, data, metadata: Optional[dict] = None, *,
                    asynchronous: bool = False):
        """send_output (apis/python/node/src/lib.rs:157-185).  Returns once the sample no longer
        needs `data`, as the reference (which copies inside the call): a device source's pack
        has read it.  `asynchronous=True` (DORA_SEND_ASYNC) returns as soon as the pack is
        queued; the caller then must not write a device source until `sync()`, or only by work
        queued on `stream` fetched after the send."""
        f = SEND_ASYNC if asynchronous else 0
        if isinstance(data, DeviceArray):
            a, s = data.send_addrs()
            rc = _fast.send_array(self.handle, output_id, a, s, ARROW_DEVICE_ROCM, metadata, f)
        elif isinstance(data, (bytes, bytearray, memoryview)):
            # read in place; the call copies them before it returns (inline below 4096 B)
            rc = _fast.send_buffer(self.handle, output_id, data, metadata)
        elif isinstance(data, DeviceBuffer):
            rc = _fast.send_bytes(self.handle, output_id, data.ptr, data.size, ARROW_DEVICE_ROCM,
                                  metadata, f)
        elif _is_pyarrow_array(data):
            # exported natively; the type's schema is exported once and lent to later sends
            rc = _fast.send_pyarrow(self.handle, output_id, data, metadata)
        elif hasattr(data, "_export_to_c"):
            with CArray.from_pyarrow(data) as c:
                rc = _fast.send_array(self.handle, output_id, ctypes.addressof(c.array),
                                      ctypes.addressof(c.schema), ARROW_DEVICE_CPU, metadata)
        elif hasattr(data, "__dlpack__") and hasattr(data, "__dlpack_device__"):
            rc = self._send_tensor(output_id, data, metadata, f)
        elif isinstance(data, _Crops) or (isinstance(data, dict) and any(
                isinstance(v, _Crops) for v in data.values())):
            rc = self._send_tensor_crops(output_id, data, metadata, f)
        elif isinstance(data, _Resized) or (isinstance(data, dict) and any(
                isinstance(v, _Resized) for v in data.values())):
            rc = self._send_tensor_resize(output_id, data, metadata, f)
        elif isinstance(data, _Argmax) or (isinstance(data, dict) and any(
                isinstance(v, _Argmax) for v in data.values())):
            rc = self._send_tensor_reduce(output_id, data, metadata, f)
        elif isinstance(data, _Quantized) or (isinstance(data, dict) and any(
                isinstance(v, _Quantized) for v in data.values())):
            rc = self._send_tensor_convert(output_id, data, metadata, f)
        elif isinstance(data, _Cast) or (isinstance(data, dict) and
                                         any(isinstance(v, _Cast) for v in data.values())):
            rc = self._send_tensor_cast(output_id, data, metadata, f)
        elif isinstance(data, dict):
            rc = self._send_tensor_struct(output_id, data, metadata, f)
        elif isinstance(data, _Ragged):
            rc = self._send_ragged(output_id, data, metadata, f)
        elif isinstance(data, _Taken):
            rc = self._send_take(output_id, data, None, metadata, f)
        elif isinstance(data, _Masked):
            rc = self._send_tensor_masked(output_id, data, None, metadata, f)
        else:
            raise TypeError("data must be bytes, a pyarrow.Array, a DeviceArray, a DeviceBuffer, "
                            "a tensor with __dlpack__ (numpy, torch; host memory or this node's GPU), "
                            "a dict of such tensors, rows of either taken by an index "
                            "(dora_amd.tensor.take) or selected by a mask "
                            "(dora_amd.tensor.masked), a ragged batch of any of these "
                            "(dora_amd.tensor.ragged) or tensors converted, reduced, resized "
                            "or cropped on send (dora_amd.tensor.cast, dora_amd.tensor.quantize, "
                            "dora_amd.tensor.argmax, dora_amd.tensor.resize, "
                            "dora_amd.tensor.crops)")
        if rc:
            _lib.check(rc)

    # asynchronous device tensor sends whose source is held until the next sync(): past this
    # many, the send syncs first (each entry pins a tensor's storage)
    _ASYNC_TENSORS_MAX = 64

    def _device_caps(self, flags: int, tensors, also=(), count=None):
        """The device side of every tensor send: `tensors`, the values, and `also`, whatever else
        the launch reads on this node's GPU (an index, a mask, a partition; None entries are
        skipped).  An asynchronous send is about to hold `count` tensors (default: the values)
        until `sync()`: past `_ASYNC_TENSORS_MAX` of them the send syncs first.  Every tensor
        does DLPack's handshake, `__dlpack__(stream=<the node stream>)`, which orders the node
        stream after the producer's current stream (dora_node_stream: the node then knows its
        stream is in use, and fills wait on it).  Returns the values' capsules, those of `also`
        and `done`, which takes the send's status, records what must be held after a successful
        asynchronous send and returns the status."""
        _require_one_hip_runtime()
        held = bool(flags & SEND_ASYNC) or self._async_default
        need = len(tensors) if count is None else count
        if held and len(self._async_tensors) + need > self._ASYNC_TENSORS_MAX:
            self.sync()
        stream = int(self._lib.dora_node_stream(self.handle))
        caps = tuple(v.__dlpack__(stream=stream) for v in tensors)
        acaps = tuple(None if v is None else v.__dlpack__(stream=stream) for v in also)

        def done(rc: int) -> int:
            if held and not rc:
                self._async_tensors.extend(tensors)
                self._async_tensors.extend(v for v in also if v is not None)
            return rc
        return caps, acaps, done

    @staticmethod
    def _host_caps(tensors):
        """(dev, caps) of host tensors: pinned memory in any of them makes the whole message
        pinned (copied inside the call).  `caps` is None when numpy refuses to export one of them:
        a read-only array (np.broadcast_to, an array over a received pyarrow buffer) cannot be an
        unversioned capsule, which cannot say "read-only"; the send only reads, so the caller
        then describes every tensor through its array interface."""
        pinned = any(int(v.__dlpack_device__()[0]) != _DL_CPU for v in tensors)
        dev = ARROW_DEVICE_ROCM_HOST if pinned else ARROW_DEVICE_CPU
        try:
            return dev, tuple(v.__dlpack__() for v in tensors)
        except BufferError:
            if not all(hasattr(v, "__array_interface__") for v in tensors):
                raise
            return dev, None

    def _send_tensor(self, output_id: str, data, metadata, flags: int) -> int:
        """A DLPack producer (numpy.ndarray, a CPU, pinned or device torch.Tensor), strided views
        included, as the nested FixedSizeList array of its shape (dora_node_send_output_tensor;
        dora_amd.tensor).  A host tensor has been read on return: pinned memory, which the GPU
        reads asynchronously to the host, is declared as such and copied inside the call.

        A device tensor (kDLROCM, on this node's GPU) is read by a kernel: in place when it is
        dense, gathered into row-major order when it is a strided view, after the handshake of
        `_device_caps`: the kernel runs after the node stream.  Without `asynchronous` the call
        returns once the kernel has read the tensor; with it, once the kernel is queued, and the
        node holds the tensor until the next `sync()` or `close()` (at most `_ASYNC_TENSORS_MAX`
        of them: the send then syncs first).  The caller must not overwrite it before that
        `sync()`."""
        dl_dev = data.__dlpack_device__()
        dev_type = int(dl_dev[0])
        if dev_type == _DL_ROCM:
            ordinal = int(dl_dev[1])
            if ordinal != self.device:
                raise TypeError(f"the tensor is on GPU {ordinal}, this node on GPU {self.device}: "
                                "a node sends tensors of its own GPU")
            (cap,), _, done = self._device_caps(flags, [data])
            return done(_fast.send_tensor(self.handle, output_id, cap, ARROW_DEVICE_ROCM, metadata,
                                          flags))
        if dev_type not in _DL_HOST:
            raise TypeError(f"tensors of DLPack device type {dev_type} cannot be sent")
        dev, caps = self._host_caps([data])
        if caps is None:
            from .tensor import _describe_array
            t, keep = _describe_array(data)
            params = encode_parameters(metadata)
            rc = self._lib.dora_node_send_output_tensor(self.handle, output_id.encode(), byref(t),
                                                        dev, params, len(params), flags)
            del keep
            return rc
        return _fast.send_tensor(self.handle, output_id, caps[0], dev, metadata, flags)

    def _entries_of(self, data, wrappers) -> tuple:
        """(items, kind, tensors, names, entries) of `data`, a tensor or a dict of tensors of
        which some are wrapped in one of `wrappers`: `items` the values as given, under their
        names (None: the one tensor), `kind`, `tensors` and `names` what `_values_kind` finds of
        the tensors inside, `entries` each wrapped value's `_entry()` and None for the others
        (without `wrappers`: None, no value has one)."""
        record = isinstance(data, dict)
        items = data if record else {None: data}
        if not wrappers:
            return (items, *self._values_kind(data), None)
        plain = {k: (v.values if isinstance(v, wrappers) else v) for k, v in items.items()}
        kind, tensors, names = self._values_kind(plain if record else plain[None])
        entries = tuple(v._entry() if isinstance(v, wrappers) else None for v in items.values())
        return items, kind, tensors, names, entries

    def _send_entries(self, output_id: str, data, wrappers, fast, entry, metadata, flags: int,
                      pre=None) -> int:
        """Every send of a tensor or a dict of tensors whose fields may carry an entry each, done
        once: `wrappers` the classes whose entries this send takes, `fast` the extension's
        function — (handle, output_id, names, capsules, entries, device_type, metadata, flags),
        without `entries` when there are no wrappers — and `entry` the library's C entry, which
        takes one array per class of `wrappers` behind the fields (`pre`: `_entries_of` the two,
        when the caller has it).

        Host tensors have been read — converted, reduced, resized by the CPU — on return.
        Tensors on this node's GPU do the handshake of `_device_caps` each and are read by one
        kernel launch; an asynchronous send holds them until `sync()`.  Host tensors that numpy
        refuses to export (`_host_caps`) are described through their array interface and go
        through ctypes."""
        items, kind, tensors, names, entries = pre or self._entries_of(data, wrappers)
        mid = () if entries is None else (entries,)
        if kind == "device":
            caps, _, done = self._device_caps(flags, tensors)
            return done(fast(self.handle, output_id, names, caps, *mid, ARROW_DEVICE_ROCM,
                             metadata, flags))
        dev, caps = self._host_caps(tensors)
        if caps is not None:
            return fast(self.handle, output_id, names, caps, *mid, dev, metadata, flags)
        from ._lib import Tensor
        from .tensor import _describe_array, _describe_entries, _describe_list
        described = [_describe_array(v) for v in tensors]
        lst, keep = _describe_list(names, [t for t, _ in described], Tensor(), 0, ARROW_DEVICE_CPU)
        arrays = [_describe_entries(list(items.values()), cls) for cls in wrappers]
        params = encode_parameters(metadata)
        rc = entry(self.handle, output_id.encode(), lst.fields, len(tensors), *arrays, dev, params,
                   len(params), flags)
        del keep, described
        return rc

    def _send_tensor_struct(self, output_id: str, data: dict, metadata, flags: int) -> int:
        """A dict of DLPack producers as one Struct message with a field per entry, in the dict's
        order (dora_node_send_output_tensor_struct; dora_amd.tensor): every tensor shares
        shape[0], and all are host tensors or all are on this node's GPU (`_send_entries`, no
        field with an entry)."""
        return self._send_entries(output_id, data, (), _fast.send_tensor_struct,
                                  self._lib.dora_node_send_output_tensor_struct, metadata, flags)

    def _tensor_kind(self, v, what: str) -> str:
        """"host" or "device" of a DLPack producer `v` (`what` names it in a refusal)."""
        if not (hasattr(v, "__dlpack__") and hasattr(v, "__dlpack_device__")):
            raise TypeError(f"{what} is not a tensor with __dlpack__")
        dl_dev = v.__dlpack_device__()
        dev_type = int(dl_dev[0])
        if dev_type == _DL_ROCM:
            if int(dl_dev[1]) != self.device:
                raise TypeError(f"{what} is on GPU {int(dl_dev[1])}, this node on GPU "
                                f"{self.device}: a node sends tensors of its own GPU")
            return "device"
        if dev_type in _DL_HOST:
            return "host"
        raise TypeError(f"{what}: tensors of DLPack device type {dev_type} cannot be sent")

    def _values_kind(self, values) -> tuple:
        """(kind, tensors, names) of the values of a message: a tensor (`names` None) or a dict
        of tensors, all "host" or all "device"."""
        if not isinstance(values, dict):
            return self._tensor_kind(values, "the values"), [values], None
        if not values:
            raise TypeError("a struct of tensors has at least one field")
        for name in values:
            if not isinstance(name, str):
                raise TypeError(f"field names are str, not {type(name).__name__}")
        kinds = {name: self._tensor_kind(v, f"field `{name}`") for name, v in values.items()}
        first = next(iter(kinds))
        for name, kind in kinds.items():
            if kind != kinds[first]:
                raise TypeError(f"field `{first}` is a {kinds[first]} tensor and field `{name}` "
                                f"a {kind} tensor: the fields of one message are all host "
                                "tensors or all on this node's GPU")
        return kinds[first], list(values.values()), tuple(values)

    def _host_words(self, words, what: str):
        """A fresh 1-D int32 or int64 numpy array of host `words` (a sequence, numpy, a CPU
        tensor), which the call reads and drops."""
        import numpy as np
        a = np.asarray(words)
        if a.size == 0:
            a = a.astype(np.int64)
        if a.dtype.kind not in "iu":
            raise TypeError(f"the {what} holds {a.dtype}, not integers")
        return np.array(a.reshape(-1), dtype=a.dtype if a.dtype in (np.int32, np.int64)
                        else np.int64, copy=True)

    def _partition_of(self, data, kind: str) -> tuple:
        """(partition, form, device) of a ragged batch over values of `kind`: a device tensor
        as it is, anything on the host as `_host_words`."""
        from ._lib import PARTITION_LENGTHS, PARTITION_OFFSETS
        part = data.offsets if data.offsets is not None else data._lengths
        form = PARTITION_OFFSETS if data.offsets is not None else PARTITION_LENGTHS
        if hasattr(part, "__dlpack_device__") and int(part.__dlpack_device__()[0]) not in _DL_HOST:
            if self._tensor_kind(part, "the partition") == "device" and kind != "device":
                raise TypeError("a partition in device memory needs values on this node's GPU: "
                                "with host values pass the partition as a host list (.tolist())")
            return part, form, ARROW_DEVICE_ROCM
        return self._host_words(part, "partition"), form, ARROW_DEVICE_CPU

    def _send_tensor_cast(self, output_id: str, data, metadata, flags: int) -> int:
        """A tensor converted on send (dora_amd.tensor.cast), or a dict of tensors of which some
        are, as the tensor or Struct message of the converted values
        (dora_node_send_output_tensor_cast): `_send_tensor_convert` without quantise entries.  A
        torch bfloat16 tensor goes through DLPack like any other (type code 4)."""
        return self._send_tensor_convert(output_id, data, metadata, flags, quantise=False)

    def _send_tensor_convert(self, output_id: str, data, metadata, flags: int,
                             quantise: bool = True) -> int:
        """A tensor quantised on send (dora_amd.tensor.quantize), or a dict of tensors of which
        some are quantised, some perhaps cast and the rest plain, as the tensor or Struct message
        of the converted values (dora_node_send_output_tensor_convert; without `quantise`, no
        entry is a quantise entry and the call is dora_node_send_output_tensor_cast), by
        `_send_entries` (a cast entry has three items, a quantise entry four) — or, when a field
        has a bias or a per-channel table, by `_send_tensor_affine`."""
        conv = (_Cast, _Quantized)
        pre = self._entries_of(data, conv)
        affines = [v._affine() if isinstance(v, conv) else None for v in pre[0].values()]
        if any(a is not None for a in affines):
            return self._send_tensor_affine(output_id, *pre, affines, metadata, flags)
        if quantise:
            return self._send_entries(output_id, data, conv, _fast.send_tensor_convert,
                                      self._lib.dora_node_send_output_tensor_convert, metadata,
                                      flags, pre)
        return self._send_entries(output_id, data, (_Cast,), _fast.send_tensor_cast,
                                  self._lib.dora_node_send_output_tensor_cast, metadata, flags, pre)

    def _send_tensor_affine(self, output_id: str, items, kind, tensors, names, entries, affines,
                            metadata, flags: int) -> int:
        """`_send_tensor_convert` when a field has a bias or a per-channel table
        (dora_node_send_output_tensor_affine): `affines` holds, per field, None or (scale table,
        bias table, axis, scalar bias).

        Tables live where the values live.  With host values a table is a sequence, a numpy
        array or a CPU tensor: it is converted to float32 here and checked inside the call — its
        length, every value finite — else the call raises and nothing is sent.  With values on
        this node's GPU a table is a float32 tensor there: it does the
        `__dlpack__(stream=<the node stream>)` handshake like every field, is never read on the
        host, and an asynchronous send holds it with the values until `sync()`."""
        import numpy as np
        tabs = [t for a in affines if a is not None for t in a[:2] if t is not None]
        for t in tabs:
            on_device = hasattr(t, "__dlpack_device__") and \
                int(t.__dlpack_device__()[0]) not in _DL_HOST
            if on_device:
                self._tensor_kind(t, "a per-channel table")
            if kind == "device" and not on_device:
                raise TypeError("a per-channel table in host memory over values on this node's "
                                "GPU: make the table once on the device (a float32 tensor) and "
                                "send with that")
            if kind != "device" and on_device:
                raise TypeError("a per-channel table in device memory over host values: move the "
                                "table next to the values (.tolist())")
        if kind == "device":
            caps, tcaps, done = self._device_caps(flags, tensors, tabs, len(tensors) + len(tabs))
            tcaps = iter(tcaps)
            aff = tuple(None if a is None else
                        (None if a[0] is None else next(tcaps),
                         None if a[1] is None else next(tcaps), a[2], a[3]) for a in affines)
            return done(_fast.send_tensor_convert(self.handle, output_id, names, caps, entries,
                                                  ARROW_DEVICE_ROCM, metadata, flags, aff))
        host = {id(t): np.ascontiguousarray(np.asarray(t, dtype=np.float32)) for t in tabs}
        dev, caps = self._host_caps(tensors)
        if caps is None:
            from ._lib import Tensor
            from .tensor import (_describe_affines, _describe_array, _describe_entries,
                                 _describe_list)
            described = [_describe_array(v) for v in tensors]
            tdesc = {k: _describe_array(a) for k, a in host.items()}
            lst, keep = _describe_list(names, [t for t, _ in described], Tensor(), 0,
                                       ARROW_DEVICE_CPU)
            carr = _describe_entries(list(items.values()), _Cast)
            qarr = _describe_entries(list(items.values()), _Quantized)
            aarr, akeep = _describe_affines([
                None if a is None else (None if a[0] is None else tdesc[id(a[0])][0],
                                        None if a[1] is None else tdesc[id(a[1])][0], a[2], a[3])
                for a in affines])
            params = encode_parameters(metadata)
            rc = self._lib.dora_node_send_output_tensor_affine(
                self.handle, output_id.encode(), lst.fields, len(tensors), carr, qarr, aarr, dev,
                params, len(params), flags)
            del keep, described, tdesc, akeep
            return rc
        aff = tuple(None if a is None else
                    (None if a[0] is None else host[id(a[0])].__dlpack__(),
                     None if a[1] is None else host[id(a[1])].__dlpack__(), a[2], a[3])
                    for a in affines)
        return _fast.send_tensor_convert(self.handle, output_id, names, caps, entries, dev,
                                         metadata, flags, aff)

    def _send_tensor_reduce(self, output_id: str, data, metadata, flags: int) -> int:
        """A tensor reduced on send (dora_amd.tensor.argmax), or a dict of tensors of which some
        are reduced and the rest plain, as the tensor or Struct message of the index tensors and
        the plain values (dora_node_send_output_tensor_reduce; `_send_entries`).  A dict that
        also holds a cast or a quantised field is not offered: nothing is sent."""
        for name, v in (data.items() if isinstance(data, dict) else ()):
            if isinstance(v, (_Cast, _Quantized)):
                raise _lib.UnsupportedType(-4, f"field `{name}`: a conversion beside an argmax in "
                                               "one message is not offered (send the converted "
                                               "field in a message of its own)")
        return self._send_entries(output_id, data, (_Argmax,), _fast.send_tensor_reduce,
                                  self._lib.dora_node_send_output_tensor_reduce, metadata, flags)

    def _send_tensor_resize(self, output_id: str, data, metadata, flags: int) -> int:
        """A tensor resized on send (dora_amd.tensor.resize), or a dict of tensors of which some
        are resized and the rest plain, as the tensor or Struct message of the resized tensors and
        the plain values (dora_node_send_output_tensor_resize; `_send_entries`).  A dict that
        also holds a cast, a quantised or an argmax field is not offered: nothing is sent."""
        for name, v in (data.items() if isinstance(data, dict) else ()):
            if isinstance(v, (_Cast, _Quantized, _Argmax)):
                raise _lib.UnsupportedType(-4, f"field `{name}`: a conversion or an argmax beside "
                                               "a resize in one message is not offered (send the "
                                               "field in a message of its own)")
        if any(isinstance(v, _Resized) and v._prep() is not None
               for v in (data.values() if isinstance(data, dict) else (data,))):
            return self._send_tensor_prep(output_id, data, _Resized, metadata, flags)
        return self._send_entries(output_id, data, (_Resized,), _fast.send_tensor_resize,
                                  self._lib.dora_node_send_output_tensor_resize, metadata, flags)

    def _boxes_of(self, items, kind: str) -> list:
        """The boxes of every crops field of `items`, in order, as the send hands them on: held
        against where the frame lives (`kind`), host boxes as something numpy exports."""
        import numpy as np
        boxes = []
        for name, v in items.items():
            if not isinstance(v, _Crops):
                continue
            what = "the boxes" if name is None else f"field `{name}`: the boxes"
            b = v.boxes
            on_device = hasattr(b, "__dlpack_device__") and \
                int(b.__dlpack_device__()[0]) not in _DL_HOST
            if on_device:
                self._tensor_kind(b, what)
            if kind == "device" and not on_device:
                raise TypeError(f"{what} are in host memory and the frame on this node's GPU: "
                                "boxes live where the frame lives (make them an int32 tensor on "
                                "the device)")
            if kind != "device" and on_device:
                raise TypeError(f"{what} are in device memory and the frame in host memory: "
                                "boxes live where the frame lives (move them to the host once)")
            if kind != "device":
                if not hasattr(b, "dtype"):  # a sequence
                    b = np.asarray(b, dtype=np.int32)
                    b = b.reshape(0, 4) if b.size == 0 else b
                elif isinstance(b, np.ndarray) and not b.flags.writeable:
                    b = np.array(b)  # (numpy exports no read-only array)
            boxes.append(b)
        return boxes

    def _send_tensor_prep(self, output_id: str, data, cls, metadata, flags: int) -> int:
        """`_send_tensor_resize` (`cls` `_Resized`) or `_send_tensor_crops` (`_Crops`) when a field
        is a model input — it has a scale, a bias or a placement
        (dora_node_send_output_tensor_prep).  It keeps a dispatch of its own, as
        `_send_tensor_affine` does: a field brings up to two more tensors, its tables, and a
        crops field its boxes.

        Tables live where the values live, as `_send_tensor_affine` has it: with host values a
        sequence, a numpy array or a CPU tensor, converted to float32 here and checked inside the
        call; with values on this node's GPU a float32 tensor there, which does the
        `__dlpack__(stream=<the node stream>)` handshake like every field, is never read on the
        host, and is held with the values by an asynchronous send until `sync()`."""
        import numpy as np
        items, kind, tensors, names, entries = self._entries_of(data, (cls,))
        preps = [v._prep() if isinstance(v, cls) else None for v in items.values()]
        tabs = [t for p in preps if p is not None for t in p[:2] if t is not None]
        for t in tabs:
            on_device = hasattr(t, "__dlpack_device__") and \
                int(t.__dlpack_device__()[0]) not in _DL_HOST
            if on_device:
                self._tensor_kind(t, "a per-channel table")
            if kind == "device" and not on_device:
                raise TypeError("a per-channel table in host memory over values on this node's "
                                "GPU: make the table once on the device (a float32 tensor) and "
                                "send with that")
            if kind != "device" and on_device:
                raise TypeError("a per-channel table in device memory over host values: move the "
                                "table next to the values (.tolist())")
        boxes = self._boxes_of(items, kind)

        def described(bcaps, tcaps):
            """(entries, preps) with the boxes' and the tables' capsules in their places."""
            bcaps, tcaps = iter(bcaps), iter(tcaps)
            ent = tuple(e if e is None or len(e) == 7 else (*e[:7], next(bcaps)) for e in entries)
            pre = tuple(None if p is None else
                        (None if p[0] is None else next(tcaps),
                         None if p[1] is None else next(tcaps), *p[2:]) for p in preps)
            return ent, pre
        if kind == "device":
            also = boxes + tabs
            caps, acaps, done = self._device_caps(flags, tensors, also, len(tensors) + len(also))
            ent, pre = described(acaps[:len(boxes)], acaps[len(boxes):])
            return done(_fast.send_tensor_prep(self.handle, output_id, names, caps, ent, pre,
                                               ARROW_DEVICE_ROCM, metadata, flags))
        dev, caps = self._host_caps(tensors)
        if caps is None:
            # (numpy exports no read-only array: the call reads a copy of each and drops it)
            dev, caps = self._host_caps([np.array(v) if isinstance(v, np.ndarray) and
                                         not v.flags.writeable else v for v in tensors])
        host = [np.ascontiguousarray(np.asarray(t, dtype=np.float32)) for t in tabs]
        ent, pre = described([b.__dlpack__() for b in boxes], [t.__dlpack__() for t in host])
        return _fast.send_tensor_prep(self.handle, output_id, names, caps, ent, pre, dev, metadata,
                                      flags)

    def _send_tensor_crops(self, output_id: str, data, metadata, flags: int) -> int:
        """Boxes cut from a frame and resized on send (dora_amd.tensor.crops), or a dict of
        tensors of which some are crops and the rest plain, as the tensor or Struct message of the
        crops and the plain values (dora_node_send_output_tensor_crop).  A dict that also holds a
        cast, a quantised, an argmax or a resized field is not offered: nothing is sent.  It keeps
        a dispatch of its own, as `_send_tensor_affine` does: every field of crops brings one more
        tensor, its boxes.

        Boxes live where the frame lives.  With host values they are a sequence, a numpy array or
        a CPU tensor, read inside the call.  With values on this node's GPU they are an int32
        tensor there: they do the `__dlpack__(stream=<the node stream>)` handshake like every
        field, are never read on the host, and an asynchronous send holds them with the values
        until `sync()`."""
        import numpy as np
        for name, v in (data.items() if isinstance(data, dict) else ()):
            if isinstance(v, (_Cast, _Quantized, _Argmax, _Resized)):
                raise _lib.UnsupportedType(-4, f"field `{name}`: a conversion, an argmax or a "
                                               "resize beside crops in one message is not offered "
                                               "(send the field in a message of its own)")
        if any(isinstance(v, _Crops) and v._prep() is not None
               for v in (data.values() if isinstance(data, dict) else (data,))):
            return self._send_tensor_prep(output_id, data, _Crops, metadata, flags)
        items, kind, tensors, names, entries = self._entries_of(data, (_Crops,))
        boxes = self._boxes_of(items, kind)
        if kind == "device":
            caps, bcaps, done = self._device_caps(flags, tensors, boxes, len(tensors) + len(boxes))
            bcaps = iter(bcaps)
            ent = tuple(None if e is None else (*e[:7], next(bcaps)) for e in entries)
            return done(_fast.send_tensor_crops(self.handle, output_id, names, caps, ent,
                                                ARROW_DEVICE_ROCM, metadata, flags))
        dev, caps = self._host_caps(tensors)
        if caps is None:
            from ctypes import pointer
            from ._lib import Tensor, TensorCrop
            from .tensor import _describe_array, _describe_list
            described = [_describe_array(v) for v in tensors]
            bdesc = iter([_describe_array(np.asarray(b)) for b in boxes])
            lst, keep = _describe_list(names, [t for t, _ in described], Tensor(), 0,
                                       ARROW_DEVICE_CPU)
            arr, bkeep = (TensorCrop * len(tensors))(), []
            for k, v in enumerate(items.values()):
                if isinstance(v, _Crops):
                    bkeep.append(next(bdesc))
                    v._fill(arr[k], pointer(bkeep[-1][0]))
            params = encode_parameters(metadata)
            rc = self._lib.dora_node_send_output_tensor_crop(
                self.handle, output_id.encode(), lst.fields, len(tensors), arr, dev, params,
                len(params), flags)
            del keep, described, bkeep
            return rc
        bcaps = iter([b.__dlpack__() for b in boxes])
        ent = tuple(None if e is None else (*e[:7], next(bcaps)) for e in entries)
        return _fast.send_tensor_crops(self.handle, output_id, names, caps, ent, dev, metadata,
                                       flags)

    def _send_take(self, output_id: str, taken, batch, metadata, flags: int) -> int:
        """Rows taken by an index (dora_amd.tensor.take) as the tensor, Struct or — with
        `batch`, the ragged batch over them — List message of `values[index]`
        (dora_node_send_output_tensor_take), without the indexed copy.

        The index lives where the values live.  Host values take an index on the host (a
        sequence, numpy, a CPU tensor), which is checked inside the call: a word outside
        [0, N) raises, naming it, and nothing is sent.  Values on this node's GPU take an index
        there: it does the `__dlpack__(stream=<the node stream>)` handshake like every field, is
        never read on the host, a word outside [0, N) gives a row of zeros, and an asynchronous
        send holds it with the values until `sync()`."""
        from ._lib import PARTITION_LENGTHS
        kind, tensors, names = self._values_kind(taken.values)
        index = taken.index
        on_device = hasattr(index, "__dlpack_device__") and \
            int(index.__dlpack_device__()[0]) not in _DL_HOST
        if on_device:
            self._tensor_kind(index, "the index")
        if on_device != (kind == "device"):
            raise TypeError(f"the index is in {'device' if on_device else 'host'} memory and the "
                            f"values are {kind} tensors: move the index next to the values")
        part, form, part_dev = None, PARTITION_LENGTHS, ARROW_DEVICE_CPU
        if batch is not None:
            part, form, part_dev = self._partition_of(batch, kind)
        if kind == "device":
            dev_part = part if part_dev == ARROW_DEVICE_ROCM else None
            caps, (icap, pcap), done = self._device_caps(flags, tensors, (index, dev_part),
                                                         len(tensors) + 2)
            if part is not None and dev_part is None:
                pcap = part.__dlpack__()
            return done(_fast.send_tensor_take(self.handle, output_id, names, caps, icap,
                                               ARROW_DEVICE_ROCM, pcap, form, part_dev,
                                               ARROW_DEVICE_ROCM, metadata, flags))
        index = self._host_words(index, "index")
        dev, caps = self._host_caps(tensors)
        if caps is None:
            from .tensor import _describe_array, _describe_take
            described = [_describe_array(v) for v in tensors]
            it, ikeep = _describe_array(index)
            pt, pkeep = _describe_array(part) if part is not None else (None, None)
            tk, keep = _describe_take(names, [t for t, _ in described], it, ARROW_DEVICE_CPU, pt,
                                      form, part_dev)
            params = encode_parameters(metadata)
            rc = self._lib.dora_node_send_output_tensor_take(
                self.handle, output_id.encode(), byref(tk), dev, params, len(params), flags)
            del keep, described, ikeep, pkeep
            return rc
        return _fast.send_tensor_take(self.handle, output_id, names, caps, index.__dlpack__(),
                                      ARROW_DEVICE_CPU,
                                      part.__dlpack__() if part is not None else None, form,
                                      part_dev, dev, metadata, flags)

    def _send_tensor_masked(self, output_id: str, sel, batch, metadata, flags: int) -> int:
        """Rows selected by a mask (dora_amd.tensor.masked) as the List message of
        `from_numpy_masked` (dora_node_send_output_tensor_mask): N rows, the K selected ones in
        front, the offsets `[0, K]` or — with `batch`, the ragged batch over the N source rows —
        `C[p]`, without `values[mask]` and without `nonzero`.

        The mask lives where the values live.  Host values take a mask on the host (a sequence,
        numpy, a CPU tensor of bool or uint8), which the CPU reads inside the call.  Values on
        this node's GPU take a mask there: it does the `__dlpack__(stream=<the node stream>)`
        handshake like every field and a device partition, is never read on the host, and an
        asynchronous send holds it with the values until `sync()`."""
        import numpy as np
        from ._lib import PARTITION_LENGTHS
        kind, tensors, names = self._values_kind(sel.values)
        mask = sel.mask
        on_device = hasattr(mask, "__dlpack_device__") and \
            int(mask.__dlpack_device__()[0]) not in _DL_HOST
        if on_device:
            self._tensor_kind(mask, "the mask")
        if on_device != (kind == "device"):
            raise TypeError(f"the mask is in {'device' if on_device else 'host'} memory and the "
                            f"values are {kind} tensors: move the mask next to the values")
        part, form, part_dev = None, PARTITION_LENGTHS, ARROW_DEVICE_CPU
        if batch is not None:
            part, form, part_dev = self._partition_of(batch, kind)
        if kind == "device":
            dev_part = part if part_dev == ARROW_DEVICE_ROCM else None
            caps, (mcap, pcap), done = self._device_caps(flags, tensors, (mask, dev_part),
                                                         len(tensors) + 2)
            if part is not None and dev_part is None:
                pcap = part.__dlpack__()
            return done(_fast.send_tensor_masked(self.handle, output_id, names, caps, mcap,
                                                 ARROW_DEVICE_ROCM, pcap, form, part_dev,
                                                 ARROW_DEVICE_ROCM, metadata, flags))
        # (the mask as it is: the call has read it when it returns, and what it cannot take — a
        # dtype, a shape, a stride — is refused there)
        mask = np.asarray(mask)
        pinned = any(int(v.__dlpack_device__()[0]) != _DL_CPU for v in tensors)
        dev = ARROW_DEVICE_ROCM_HOST if pinned else ARROW_DEVICE_CPU
        # (numpy exports no bool through DLPack before 1.25, and read-only arrays never: the
        # array interface describes every field, the mask and the partition alike)
        from .tensor import _describe_array, _describe_mask
        if not all(hasattr(v, "__array_interface__") for v in tensors):
            tensors = [np.from_dlpack(v) for v in tensors]
        described = [_describe_array(v) for v in tensors]
        mt, mkeep = _describe_array(mask)
        pt, pkeep = _describe_array(part) if part is not None else (None, None)
        mk, keep = _describe_mask(names, [t for t, _ in described], mt, ARROW_DEVICE_CPU, pt,
                                  form, part_dev)
        params = encode_parameters(metadata)
        rc = self._lib.dora_node_send_output_tensor_mask(
            self.handle, output_id.encode(), byref(mk), dev, params, len(params), flags)
        del keep, described, mkeep, pkeep
        return rc

    def _send_ragged(self, output_id: str, data, metadata, flags: int) -> int:
        """A ragged batch (dora_amd.tensor.ragged) as one List message
        (dora_node_send_output_tensor_list): the values as `_send_tensor` or `_send_tensor_struct`
        would take them, cut into lists by the partition.

        A partition on the host — a Python sequence, a numpy array, a CPU tensor — goes with any
        values and is checked inside the call: a refusal names the first offending index and
        nothing is sent.  A partition on this node's GPU needs device values; it does the
        `__dlpack__(stream=<the node stream>)` handshake like every field, is never read on the
        host, and is held with the values until `sync()` by an asynchronous send.  Its words are
        clamped into a well-formed List by the kernel, not checked (dora_amd.tensor)."""
        if isinstance(data.values, _Taken):
            return self._send_take(output_id, data.values, data, metadata, flags)
        if isinstance(data.values, _Masked):
            return self._send_tensor_masked(output_id, data.values, data, metadata, flags)
        kind, tensors, names = self._values_kind(data.values)
        part, form, part_dev = self._partition_of(data, kind)
        if kind == "device":
            dev_part = part if part_dev == ARROW_DEVICE_ROCM else None
            caps, (pcap,), done = self._device_caps(flags, tensors, (dev_part,), len(tensors) + 1)
            if dev_part is None:
                pcap = part.__dlpack__()
            return done(_fast.send_tensor_list(self.handle, output_id, names, caps, pcap, form,
                                               part_dev, ARROW_DEVICE_ROCM, metadata, flags))
        dev, caps = self._host_caps(tensors)
        if caps is None:
            from .tensor import _describe_array, _describe_list
            described = [_describe_array(v) for v in tensors]
            pt, pkeep = _describe_array(part)
            lst, keep = _describe_list(names, [t for t, _ in described], pt, form, part_dev)
            params = encode_parameters(metadata)
            rc = self._lib.dora_node_send_output_tensor_list(
                self.handle, output_id.encode(), byref(lst), dev, params, len(params), flags)
            del keep, described, pkeep
            return rc
        return _fast.send_tensor_list(self.handle, output_id, names, caps, part.__dlpack__(), form,
                                      part_dev, dev, metadata, flags)

    def send_output_async(self, output_id: str, data, metadata: Optional[dict] = None):
        """send_output(..., asynchronous=True)."""
        self.send_output(output_id, data, metadata, asynchronous=True)

    def set_async_sends(self, enable: bool = True):
        """Make every send of this node asynchronous (dora_node_set_async_sends)."""
        call("dora_node_set_async_sends", self.handle, int(enable))
        self._async_default = bool(enable)

    def set_event_thread(self, enable: bool = True):
        """Drain the daemon's events on a background thread (the reference's event-stream thread;
        dora_node_set_event_thread): inputs keep arriving, with the drop-oldest policy applied,
        while this node's user thread is busy elsewhere."""
        call("dora_node_set_event_thread", self.handle, int(enable))

    def send_output_device_bytes(self, output_id: str, ptr: int, n: int,
                                 metadata: Optional[dict] = None, *, asynchronous: bool = False):
        """send_output_raw with an HBM source: one pack kernel into a fresh device sample;
        returns once the pack has read the source unless `asynchronous` (send_output)."""
        rc = _fast.send_bytes(self.handle, output_id, ptr, n, ARROW_DEVICE_ROCM, metadata,
                              SEND_ASYNC if asynchronous else 0)
        if rc:
            _lib.check(rc)

    def sample_fill_ticket(self, sample_ptr, workgroups: int,
                           mode: int = _lib.FILL_WRITE_THROUGH) -> "_lib.FillTicket":
        """dora_sample_fill_ticket: the ticket with which one kernel launch of `workgroups`
        workgroups publishes the sample `sample_ptr` (of dora_node_allocate_data_sample) it
        writes in place; the send then queues no stream operation for it."""
        t = _lib.FillTicket()
        call("dora_sample_fill_ticket", self.handle, sample_ptr, workgroups, mode, byref(t))
        return t

    def set_compact(self, enable: bool = True):
        """Send device arrays with compacting plans (slices move only their own bytes)."""
        call("dora_node_set_compact", self.handle, int(enable))

    def forward(self, output_id: str, event: dict, metadata: Optional[dict] = None):
        """Re-send a received input on `output_id` with its type info (dora_node_forward): one
        copy, a cross-GPU input straight from the peer's slot.  Parameters default to the
        input's own."""
        params = encode_parameters(event.get("metadata") if metadata is None else metadata)
        call("dora_node_forward", self.handle, output_id.encode(), event["_event"].ptr,
             params, len(params))

    def close_outputs(self, outputs):
        arr = (ctypes.c_char_p * len(outputs))(*[o.encode() for o in outputs])
        call("dora_node_close_outputs", self.handle, arr, len(outputs))

    # ------------------------------------------------------------------------------ receiving
    def next(self, timeout: Optional[float] = None):
        """Next event dict, or None when the stream has ended (or on timeout)."""
        # one native call: the event's fields, its decoded parameters and its data's address
        r = _fast.next_event(self.handle, -1 if timeout is None else int(timeout * 1e6))
        if r.__class__ is int:
            if r in (-5, -6):   # closed / timeout
                return None
            _lib.check(r)
        ptr, t, eid, params, ts, dptr, dlen, on_dev, err = r
        ev = _EventHandle(ptr)
        kind = EVENT_TYPES.get(t, "UNKNOWN")
        if kind == "ALL_INPUTS_CLOSED":
            ev.free()
            return None
        out = _Event(type=kind, id=eid)
        if kind == "ERROR":
            out["error"] = err
        if kind == "INPUT":
            out["metadata"] = params
            out["timestamp_ns"] = ts
            out["_event"] = ev  # "type_info" is decoded on first access (_Event)
            out["data_ptr"], out["data_len"] = (dptr or None), dlen
            out["on_device"] = bool(on_dev)
            if dlen == 0:       # RawData::Vec(empty) -> ArrayData::new_empty(data_type)
                import pyarrow as pa
                out["value"] = pa.array([], type=out["type_info"].arrow_type())
            elif out["on_device"]:
                a, s = ArrowArray(), ArrowSchema()
                call("dora_event_array", ev.ptr, byref(a), byref(s))
                import pyarrow as pa
                t = pa.DataType._import_from_c(ctypes.addressof(s))
                # the array keeps the input alive; the event handle can go
                out["value"] = DeviceArray(a, t)
                out["value"]._device_id = self.device
            else:
                # an inline DataMessage::Vec sample (< 4096 B from a host source), or a host-only
                # producer's shared memory read in place: a host pyarrow array over its bytes,
                # as the reference's PyEvent::value; it keeps the input alive
                # (its type from a cache keyed by the schema: no schema import per event)
                r = _fast.export_typed(ev.ptr)
                if r.__class__ is int:
                    _lib.check(r)
                import pyarrow as pa
                try:
                    out["value"] = pa.Array._import_from_c(r[0], r[1])
                finally:
                    _fast.free_arrow(r[0], 0)
        out["_event"] = ev
        return out

    def wait_input(self, input_id: str, key: str, value, timeout: float = 60.0) -> dict:
        """Wait for an input event on `input_id` whose parameters have `key == value` and return
        its parameters; other events are skipped.  A control-message fast path: only the id and
        the parameters are decoded (no data mapping, no Arrow value), in one native call
        (_dora_node.wait_input), so the wait costs about one ring hop, not a Python event
        construction."""
        r = _fast.wait_input(self.handle, input_id, key, value, int(timeout * 1e6))
        if r.__class__ is int:
            if r == -6:
                raise TimeoutError(f"no `{input_id}` input with {key}={value!r}")
            _lib.check(r)
        return r

    def __iter__(self):
        return self

    def __next__(self):
        """`next(node)`: the next event (blocking); StopIteration once the stream has ended, as
        the reference's `__next__` returning None (lib.rs:118-120)."""
        ev = self.next()
        if ev is None:
            raise StopIteration
        return ev

    # ------------------------------------------------------------------------------ dataflow
    def dataflow_id(self) -> str:
        """The dataflow's id (lib.rs:196-202: DataflowId, a uuid): the one in the node's
        DORA_NODE_CONFIG, else the daemon's dataflow name as the inter-daemon wire maps it."""
        from .dataflow import dataflow_uuid
        cfg = self._node_config()
        if cfg and cfg.get("dataflow_id"):
            return str(cfg["dataflow_id"])
        return dataflow_uuid(self._lib.dora_node_dataflow_id(self.handle).decode())

    def dataflow_descriptor(self) -> dict:
        """The dataflow's descriptor as parsed from its YAML (lib.rs:186-194), written next to the
        dataflow's control region by its launcher (dora_amd.dataflow.Dataflow); else the
        descriptor of the node's DORA_NODE_CONFIG."""
        import json
        p = descriptor_path(self._region) if self._region else None
        if p and os.path.exists(p):
            with open(p) as f:
                return json.load(f)
        cfg = self._node_config()
        if cfg and "dataflow_descriptor" in cfg:
            return cfg["dataflow_descriptor"]
        raise RuntimeError(f"no descriptor for dataflow region `{self._region}`")

    def merge_external_events(self, subscription):
        """Merging an external event stream (lib.rs:204-209) exists in the reference only for
        ROS2 subscriptions (dora_ros2_bridge_python), which is outside this data plane: refused."""
        raise NotImplementedError(
            "merge_external_events takes a dora.Ros2Subscription; the ROS2 bridge is not part of "
            "the device data plane")

    def _node_config(self) -> Optional[dict]:
        raw = os.environ.get("DORA_NODE_CONFIG")
        if not raw:
            return None
        import yaml
        cfg = yaml.safe_load(raw)
        return cfg if isinstance(cfg, dict) and cfg.get("node_id") == self.id else None

    # -------------------------------------------------------------------------------- stats
    @property
    def stream(self) -> int:
        return self._lib.dora_node_stream(self.handle)

    def stats(self) -> dict:
        v = [c_uint64() for _ in range(4)]
        call("dora_node_stats", self.handle, *[byref(x) for x in v])
        out = dict(zip(["slots_created", "cache_hits", "in_flight", "dropped_inputs"],
                       [x.value for x in v]))
        c, b = c_uint64(), c_uint64()
        call("dora_node_peer_stats", self.handle, byref(c), byref(b))
        out["peer_copies"], out["peer_bytes"] = c.value, b.value
        call("dora_node_forward_stats", self.handle, byref(c), byref(b))
        out["zero_copy_forwards"], out["forwards_held"] = c.value, b.value
        return out

    def set_profiling(self, enable: bool = True):
        call("dora_node_set_profiling", self.handle, int(enable))

    def dataflow_counters(self, node_id: str) -> dict:
        """Slots created and IPC mappings opened by any node of the dataflow
        (dora_node_dataflow_counters)."""
        a, b, c = c_uint64(), c_uint64(), c_uint64()
        call("dora_node_dataflow_counters", self.handle, node_id.encode(), byref(a), byref(b),
             byref(c))
        return {"slots_created": a.value, "ipc_opens": b.value, "dropped_inputs": c.value}

    def plan_cache_stats(self) -> dict:
        """Device-array sends served by the node's plan cache (dora_node_plan_cache_stats)."""
        a, b = c_uint64(), c_uint64()
        call("dora_node_plan_cache_stats", self.handle, byref(a), byref(b))
        return {"hits": a.value, "entries": b.value}

    def fill_paths(self) -> dict:
        """Fills by dispatch path: raw AQL packets vs hipLaunchKernel (dora_node_fill_paths)."""
        a, h = c_uint64(), c_uint64()
        call("dora_node_fill_paths", self.handle, byref(a), byref(h))
        return {"aql": a.value, "hip": h.value}

    def host_paths(self) -> dict:
        """Host sources written into their slot by the CPU through the BAR, device samples this
        node (without a GPU) staged to host memory, and device samples this node packed straight
        into shared memory for receivers that all lack a GPU (dora_node_host_paths)."""
        a, b, c, d = c_uint64(), c_uint64(), c_uint64(), c_uint64()
        call("dora_node_host_paths", self.handle, byref(a), byref(b), byref(c), byref(d))
        return {"bar_fills": a.value, "staged": b.value, "staged_bytes": c.value,
                "host_packs": d.value}

    def host_bound_outputs(self) -> list:
        """The outputs the daemon named host-bound in AllNodesReady: all receivers lack a GPU
        (dora_node_host_bound_outputs)."""
        n = c_uint64()
        call("dora_node_host_bound_outputs", self.handle, None, 0, byref(n))
        buf = ctypes.create_string_buffer(n.value + 1)
        call("dora_node_host_bound_outputs", self.handle, buf, n.value + 1, byref(n))
        return buf.value.decode().split("\n")[:-1] if n.value else []

    def set_timing_period(self, period: int):
        """Stamp every `period`-th pack launch (0: the default, every 8th)."""
        call("dora_node_set_timing_period", self.handle, int(period))

    def pack_intervals(self, cap: int = 1 << 16):
        """[(start_ms, stop_ms)] of the stamped packs since profiling was enabled."""
        out, n = (c_double * (2 * cap))(), c_size_t()
        call("dora_node_pack_intervals", self.handle, out, cap, byref(n))
        k = min(n.value, cap)
        return [(out[2 * i], out[2 * i + 1]) for i in range(k)]

    def region_begin(self):
        """Start a device-timed run of sends (dora_node_region_begin)."""
        call("dora_node_region_begin", self.handle)

    def sync(self):
        """Wait for every fill of this node and its node stream (dora_node_sync); device tensors
        sent asynchronously since the last call have then been read and are let go."""
        call("dora_node_sync", self.handle)
        self._async_tensors.clear()

    def region_mark(self):
        """Record the region's stop events after the last send, without waiting on them."""
        call("dora_node_region_mark", self.handle)

    def region_end(self) -> dict:
        """Device span of the sends since region_begin: first pack start -> last pack end."""
        ms, packs, b = c_double(), c_uint64(), c_uint64()
        call("dora_node_region_end", self.handle, byref(ms), byref(packs), byref(b))
        return {"span_ms": ms.value, "packs": packs.value, "bytes": b.value}

    def pack_stats(self) -> dict:
        c, ms, b = c_uint64(), c_double(), c_uint64()
        call("dora_node_pack_stats", self.handle, byref(c), byref(ms), byref(b))
        return {"count": c.value, "total_ms": ms.value, "bytes": b.value}

    def send_profile(self) -> dict:
        out, cnt = (c_double * 4)(), c_uint64()
        call("dora_node_send_profile", self.handle, out, 4, byref(cnt))
        return {"alloc_us": out[0], "launch_us": out[1], "fill_us": out[2], "send_us": out[3],
                "count": cnt.value}

    def close(self):
        if self.handle:
            if self._async_tensors:
                self._lib.dora_node_sync(self.handle)  # their gathers read them until then
            self._lib.dora_node_free(self.handle)
            self.handle = None
            self._async_tensors.clear()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


__all__ = ["Node", "encode_parameters", "decode_parameters", "DoraGpuError"]
