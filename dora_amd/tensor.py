"""Tensors as messages.

A tensor of shape `(d0, d1, .., dk)` and dtype `T` travels as the Arrow array of length `d0` and
type `FixedSizeList<..FixedSizeList<T>[dk]..>[d1]` built from its row-major values (child fields
named `item`, nullable, as pyarrow creates them); a 1-D tensor is the plain primitive array.  Its
sample is one buffer, the row-major bytes, so the shape travels in the type and a node of the
reference can send or receive the same message.

    node.send_output("image", frame.transpose(2, 0, 1))   # numpy or CPU torch: any host DLPack tensor
    node.send_output("image", frame_cuda.permute(2, 0, 1))  # a torch tensor in this node's HBM
    chw = tensor.to_torch(event["value"])                  # device receiver: zero-copy, in HBM
    chw = tensor.to_numpy(event["value"])                  # host receiver: the nested pyarrow array
    chw = tensor.to_numpy(event["value"].to_pyarrow())     # device receiver: downloaded first

A record of tensors that share their leading extent travels as one message, the Arrow array of
type `Struct<name: T, ..>` whose fields are those tensor columns (nullable, as
`pa.StructArray.from_arrays` makes them); tensors of unrelated shapes get a leading extent of 1
(`unsqueeze(0)`), a struct of length 1:

    node.send_output("det", {"bbox": out[:, :4], "conf": out[:, 4], "cls": out[:, 5]})
    det = tensor.to_torch(event["value"])                  # {"bbox": .., "conf": .., "cls": ..}

A strided host view is gathered into row-major order by the CPU inside the send; pinned memory
is copied once, so every source has been read when `send_output` returns.  A tensor in device
memory is read by a kernel: in place when dense, gathered by the gfx950 gather kernel when it is a
strided view (one read and one write of HBM, no `.contiguous()` first).  The producer must share
the HIP runtime of this library: import torch before dora_amd (Node._send_tensor).
"""
from __future__ import annotations

from ctypes import c_int64

from ._lib import Tensor, TensorField

_DL_CODES = {"i": 0, "u": 1, "f": 2, "b": 6, "c": 5}  # numpy dtype kind -> DLPack type code


def tensor_type(dtype, shape):
    """The pyarrow type of a tensor message of numpy `dtype` and `shape`."""
    import numpy as np
    import pyarrow as pa
    t = pa.from_numpy_dtype(np.dtype(dtype))
    for d in reversed(tuple(shape)[1:]):
        t = pa.list_(t, int(d))
    return t


def from_numpy(x):
    """The nested pyarrow array of a numpy array (copied to row-major order if it is a view)."""
    import numpy as np
    import pyarrow as pa
    x = np.asarray(x)
    if x.ndim < 1:
        raise ValueError("a tensor message has at least one dimension")
    arr = pa.array(np.ascontiguousarray(x).reshape(-1))
    for d in reversed(x.shape[1:]):
        arr = pa.FixedSizeListArray.from_arrays(arr, int(d))
    return arr


def struct_type(fields):
    """The pyarrow type of a struct-of-tensors message: `fields` maps each name to the
    `(dtype, shape)` of its tensor (the counterpart of `tensor_type`)."""
    import pyarrow as pa
    return pa.struct([pa.field(name, tensor_type(dtype, shape))
                      for name, (dtype, shape) in dict(fields).items()])


def from_numpy_struct(fields):
    """The pyarrow StructArray of a dict of numpy arrays that share their leading extent (the
    counterpart of `from_numpy`): what `send_output(output_id, fields)` puts on the wire."""
    import pyarrow as pa
    fields = dict(fields)
    if not fields:
        raise ValueError("a struct of tensors has at least one field")
    return pa.StructArray.from_arrays([from_numpy(v) for v in fields.values()], names=list(fields))


def to_numpy(arr):
    """The numpy array of a nested pyarrow array (a host receiver's `event["value"]`): shape
    `(len, s1, .., sk)`; of a struct of tensor columns, the dict `{name: array}`.  Nulls at any
    level, the struct's own included, are refused."""
    import pyarrow as pa
    if pa.types.is_struct(arr.type):
        if arr.null_count:
            raise TypeError("a tensor message has no nulls")
        # (field(i) of a sliced struct is the whole child: flatten() gives this slice's)
        return {arr.type.field(i).name: to_numpy(col) for i, col in enumerate(arr.flatten())}
    shape = [len(arr)]
    while pa.types.is_fixed_size_list(arr.type):
        if arr.null_count:
            raise TypeError("a tensor message has no nulls")
        shape.append(arr.type.list_size)
        arr = arr.flatten()  # the values of this array's own slice
    if arr.null_count:
        raise TypeError("a tensor message has no nulls")
    return arr.to_numpy(zero_copy_only=False).reshape(shape)


def to_torch(value):
    """The torch tensor of a received tensor message: zero-copy over the HBM sample for a device
    receiver's `event["value"]` (DLPack, kDLROCM; the tensor keeps the input alive), a copy of
    the nested pyarrow array for a host receiver's.  A struct of tensor columns gives the dict
    `{name: tensor}`, each a view of the one sample.  Nulls at any level are refused."""
    import torch
    import pyarrow as pa
    t = getattr(value, "type", None)
    if t is not None and pa.types.is_struct(t):
        if hasattr(value, "field_views"):  # a DeviceArray: zero-copy children
            return {name: torch.from_dlpack(v) for name, v in value.field_views().items()}
        import numpy as np
        return {name: torch.from_numpy(np.array(x)) for name, x in to_numpy(value).items()}
    if hasattr(value, "__dlpack__"):
        return torch.from_dlpack(value)
    import numpy as np
    return torch.from_numpy(np.array(to_numpy(value)))


def _describe(ptr: int, shape, strides, dtype, byte_offset: int = 0) -> tuple:
    """A `dora_tensor` over `ptr` (strides in elements, or None for row-major) and the ctypes
    arrays it points at, which the caller keeps alive with it."""
    import numpy as np
    dt = np.dtype(dtype)
    t = Tensor()
    t.data = ptr
    t.byte_offset = byte_offset
    t.dtype_code = _DL_CODES.get(dt.kind, 255)
    t.dtype_bits = dt.itemsize * 8
    t.dtype_lanes = 1
    t.ndim = len(shape)
    sh = (c_int64 * max(len(shape), 1))(*shape)
    t.shape = sh
    st = None
    if strides is not None:
        st = (c_int64 * max(len(strides), 1))(*strides)
        t.strides = st
    return t, (sh, st)


def _describe_array(x) -> tuple:
    """`_describe` of an object with `__array_interface__` (a numpy array, read-only ones
    included, which numpy's own `__dlpack__` refuses to export)."""
    import numpy as np
    x = np.asarray(x)
    strides = [s // x.dtype.itemsize for s in x.strides]
    t, keep = _describe(x.__array_interface__["data"][0], x.shape, strides, x.dtype)
    return t, (x, keep)


def _describe_fields(names, tensors) -> tuple:
    """The `dora_tensor_field` array of `names` over the `Tensor`s of `_describe`, and what the
    caller keeps alive with it (besides each tensor's own keep)."""
    arr = (TensorField * len(names))()
    enc = [n.encode() for n in names]
    for k, (n, t) in enumerate(zip(enc, tensors)):
        arr[k].name = n
        arr[k].tensor = t
    return arr, (enc, tensors)


__all__ = ["tensor_type", "struct_type", "from_numpy", "from_numpy_struct", "to_numpy", "to_torch"]
