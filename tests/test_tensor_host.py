"""Tensor sends on the CPU (no GPU): dora_gpu_plan_tensor over host numpy views — size, type info
and gathered bytes against the oracle's pack of the equivalent nested FixedSizeList array, the
canonical form of a view (dense views are copied in place, everything else is staged), every
refusal — and strided tensors through a host-only two-node dataflow."""
import ctypes
from ctypes import byref, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST, DoraGpuError
from dora_amd.arrow_utils import Plan
from oracle.pack_ref import pack
from tests.test_dataflow_host import InProcessDaemon, _start_nodes

DTYPES = [np.uint8, np.float16, np.float32, np.float64]  # 1, 2, 4 and 8 bytes
SHAPES = [(7,), (5, 7), (2, 3, 4, 5)]

# name -> (view of x, or None where the view needs more dimensions; is it dense by construction)
VIEWS = {
    "identity": (lambda x: x, True),
    "batch_slice": (lambda x: x[1:4], True),
    "inner_slice": (lambda x: x[:, 1:6] if x.ndim > 1 else None, False),
    "transpose": (lambda x: x.T, None),
    "moveaxis": (lambda x: np.moveaxis(x, 0, -1), None),
    "reversed": (lambda x: x[::-1], False),
    "step2": (lambda x: x[:, ::2] if x.ndim > 1 else None, False),
    "broadcast": (lambda x: np.broadcast_to(x, (3,) + x.shape), False),
    "unsqueeze": (lambda x: x[:, None], True),
    "double_transpose": (lambda x: x.T.T, True),
}


def describe(ptr, shape, strides, dtype, byte_offset=0):
    return tensor._describe(ptr, shape, strides, dtype, byte_offset)


def plan_of(x, dev=ARROW_DEVICE_CPU):
    """dora_gpu_plan_tensor of the numpy array x, over its own memory."""
    t, keep = tensor._describe_array(x)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor", byref(t), dev, byref(h))
    return Plan(h.value, keep)


def base(dtype, shape):
    n = int(np.prod(shape))
    return (np.arange(n, dtype=np.int64) * 37 + 11).astype(dtype).reshape(shape)


def cases():
    for dt in DTYPES:
        for sh in SHAPES:
            for name in VIEWS:
                if VIEWS[name][0](base(np.uint8, sh)) is not None:
                    yield pytest.param(dt, sh, name, id=f"{np.dtype(dt).name}-{'x'.join(map(str, sh))}-{name}")


_ORACLE = {}


def oracle(x):
    """(bytes, type info JSON) of the oracle's pack of the nested array of x, computed once per
    dtype, shape and content."""
    c = np.ascontiguousarray(x)
    key = (c.dtype.str, c.shape, c.tobytes())
    if key not in _ORACLE:
        want, info = pack(tensor.from_numpy(c))
        _ORACLE[key] = (bytes(want), info.to_json())
    return _ORACLE[key]


@pytest.mark.parametrize("dtype,shape,view", cases())
def test_host_plan_matches_oracle(lib, dtype, shape, view):
    """Size, type info and the bytes a host plan copies equal the oracle's for the contiguous
    copy of the view."""
    x = VIEWS[view][0](base(dtype, shape))
    want, info = oracle(x)
    assert want == np.ascontiguousarray(x).tobytes()
    with plan_of(x) as p:
        assert p.size == len(want)
        assert p.type_info().to_json() == info
        segs = p.segments()
        assert len(segs) == 1
        src, off, n = segs[0]
        assert off == 0 and n == len(want)
        assert ctypes.string_at(src, n) == want


@pytest.mark.parametrize("dtype,shape,view", cases())
def test_canonical_form(lib, dtype, shape, view):
    """A view whose elements already lie in row-major order — batch slices, unsqueezed and
    double-transposed views among them — is one segment over `data + offset`, read in place;
    every other view is one segment over a staging buffer outside the array."""
    b = base(dtype, shape)
    x = VIEWS[view][0](b)
    addr = x.__array_interface__["data"][0]
    b0 = b.__array_interface__["data"][0]
    dense = VIEWS[view][1]
    if dense is None:  # a transpose of a 1-D array is the array
        dense = x.flags.c_contiguous
    assert dense == x.flags.c_contiguous
    with plan_of(x) as p:
        (src, off, n), = p.segments()
        assert off == 0 and n == p.size == x.size * x.itemsize
        if dense:
            assert src == addr
            assert addr - b0 == (b.strides[0] if view == "batch_slice" else 0)
        else:
            assert not (b0 <= src < b0 + b.nbytes)


def _plan_raw(t, dev=ARROW_DEVICE_CPU):
    h = c_void_p()
    try:
        _lib.call("dora_gpu_plan_tensor", byref(t), dev, byref(h))
    finally:
        if h.value:
            _lib.load().dora_gpu_plan_free(h.value)


def test_refusals(lib):
    buf = np.zeros(64, np.uint8)
    addr = buf.__array_interface__["data"][0]

    def t(shape=(4,), strides=None, dtype=np.uint8, **over):
        d, keep = describe(addr, shape, strides, dtype)
        for k, v in over.items():
            setattr(d, k, v)
        d._keep = keep
        return d

    unsupported = {
        "bool": t(dtype=np.bool_),
        "bfloat16": t(dtype_code=4, dtype_bits=16),
        "complex64": t(dtype=np.complex64),
        "lanes": t(dtype_lanes=2),
        "int of 24 bits": t(dtype_code=0, dtype_bits=24),
        "float of 8 bits": t(dtype_code=2, dtype_bits=8),
    }
    for name, d in unsupported.items():
        with pytest.raises(DoraGpuError) as e:
            _plan_raw(d)
        assert e.value.code == -4, name
    assert "bool" in str(_err(unsupported["bool"]))
    assert "bfloat16" in str(_err(unsupported["bfloat16"])) and "uint16" in str(_err(unsupported["bfloat16"]))
    assert "complex64" in str(_err(unsupported["complex64"]))
    assert "lanes" in str(_err(unsupported["lanes"]))
    # nine dimensions that do not merge
    nine = np.zeros((4,) * 9, np.uint8)[(slice(None, None, 2),) * 9]
    with pytest.raises(DoraGpuError) as e:
        plan_of(nine)
    assert e.value.code == -4
    invalid = {
        "ndim 0": t(shape=(), ndim=0),
        "negative extent": t(shape=(4, -1)),
        "inner extent 0": t(shape=(4, 0)),
        "overflow": t(shape=(1 << 40, 1 << 40)),
        "overflow by the element size": t(shape=(1 << 31, 1 << 31), dtype=np.float64),
        "NULL data": t(data=None),
    }
    for name, d in invalid.items():
        with pytest.raises(DoraGpuError) as e:
            _plan_raw(d)
        assert e.value.code == -1, name
    # d0 == 0 is an empty message, with or without data
    for d in (t(shape=(0, 3)), t(shape=(0, 3), data=None)):
        h = c_void_p()
        _lib.call("dora_gpu_plan_tensor", byref(d), ARROW_DEVICE_CPU, byref(h))
        assert lib.dora_gpu_plan_size(h.value) == 0 and lib.dora_gpu_plan_num_segments(h.value) == 0
        lib.dora_gpu_plan_free(h.value)
    with pytest.raises(DoraGpuError) as e:
        _plan_raw(t(), dev=7)
    assert e.value.code == -1


def _planned_bytes(t, dev=ARROW_DEVICE_CPU):
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor", byref(t), dev, byref(h))
    with Plan(h.value, None) as p:
        (src, off, n), = p.segments()
        assert off == 0 and n == p.size
        return src, ctypes.string_at(src, n), p.type_info().to_json()


def test_byte_offset_null_strides_and_pinned_declaration(lib):
    """The descriptor fields numpy's and torch's capsules never vary: a non-zero byte_offset, NULL
    strides (row-major), and memory declared pinned, which is copied even when dense."""
    b = base(np.float32, (6, 5, 4))
    addr = b.__array_interface__["data"][0]
    # NULL strides: row-major over `shape`, starting byte_offset bytes into the buffer
    view = b[1:3]
    t, keep = describe(addr, view.shape, None, b.dtype, byte_offset=b.strides[0])
    src, got, info = _planned_bytes(t)
    assert src == addr + b.strides[0] and (got, info) == oracle(view)
    # byte_offset with strides: b[2:, ::2, 1] from the base pointer
    view = b[2:, ::2, 1]
    off = view.__array_interface__["data"][0] - addr
    assert off > 0
    t, keep = describe(addr, view.shape, [s // 4 for s in view.strides], b.dtype, byte_offset=off)
    src, got, info = _planned_bytes(t)
    assert not (addr <= src < addr + b.nbytes) and (got, info) == oracle(view)
    # declared pinned: dense and strided views alike are copied out of the caller's memory
    for view in (b, b[1:3], b.transpose(2, 0, 1)):
        t, keep = tensor._describe_array(view)
        src, got, info = _planned_bytes(t, ARROW_DEVICE_ROCM_HOST)
        assert not (addr <= src < addr + b.nbytes) and (got, info) == oracle(view)


def _err(d):
    with pytest.raises(DoraGpuError) as e:
        _plan_raw(d)
    return e.value


def test_empty_tensor_type_info_matches_oracle(lib):
    x = np.zeros((0, 3, 2), np.float32)
    want, info = pack(tensor.from_numpy(x))
    with plan_of(x) as p:
        assert p.size == len(want) == 0
        assert p.type_info().to_json() == info.to_json()


def test_tensor_module_roundtrip():
    import pyarrow as pa
    x = base(np.int16, (2, 3, 4))
    a = tensor.from_numpy(x.transpose(2, 0, 1))
    assert a.type == tensor.tensor_type(np.int16, (4, 2, 3)) == pa.list_(pa.list_(pa.int16(), 3), 2)
    assert len(a) == 4
    got = tensor.to_numpy(a)
    assert got.shape == (4, 2, 3) and np.array_equal(got, x.transpose(2, 0, 1))
    assert np.array_equal(tensor.to_numpy(a[1:3]), x.transpose(2, 0, 1)[1:3])
    assert np.array_equal(tensor.to_numpy(tensor.from_numpy(x[0, 0])), x[0, 0])
    with pytest.raises(TypeError):
        tensor.to_numpy(pa.array([[1, 2], None], pa.list_(pa.int16(), 2)))


DESC = {"nodes": [
    {"id": "src", "outputs": ["out"]},
    {"id": "dst", "inputs": {"in": {"source": "src/out", "queue_size": 100}}, "outputs": []},
]}


def _bases():
    return [base(np.float32, (33, 65)), base(np.uint8, (37, 53, 3)), base(np.float32, (5, 7)),
            base(np.uint8, (7, 5, 3)), base(np.int16, (4, 6))]


def _views():
    """x.T of a float32 matrix and an HWC uint8 image moved to CHW, each above and below the
    4096-byte threshold between shared-memory and inline samples; a dense one; a reversed one."""
    b = _bases()
    return [b[0].T, np.moveaxis(b[1], -1, 0), b[2].T, np.moveaxis(b[3], -1, 0), b[4],
            base(np.float64, (3, 4))[::-1]]


def _roundtrip(sent):
    d = InProcessDaemon(DESC)
    nodes = _start_nodes(d.shm, ["src", "dst"])
    a, b = nodes["src"], nodes["dst"]
    try:
        for k, x in enumerate(sent):
            a.send_output("out", x, {"k": k})
        got = []
        for k in range(len(sent)):
            ev = b.next(timeout=5)
            assert ev["type"] == "INPUT" and ev["metadata"] == {"k": k}
            got.append((tensor.to_numpy(ev["value"]), ev["type_info"].to_json()))
    finally:
        a.close()
        b.close()
        d.join()
    return got


def test_host_dataflow_delivers_strided_numpy_views(lib):
    views = _views()
    sizes = [v.size * v.itemsize for v in views]
    assert min(sizes[:2]) >= 4096 > max(sizes[2:4])
    for x, (y, info) in zip(views, _roundtrip(views)):
        assert y.shape == x.shape and y.dtype == x.dtype and np.array_equal(y, x)
        assert info == oracle(x)[1]


def test_host_dataflow_delivers_read_only_numpy_arrays(lib):
    """numpy refuses to export a read-only array through DLPack: np.broadcast_to, and what
    tensor.to_numpy returns for a received message (an array over a pyarrow buffer), so a relay
    re-sending a received tensor or a view of it.  They go out all the same."""
    small, big = base(np.float32, (1, 5)), base(np.int16, (3, 40, 30))
    received = tensor.to_numpy(tensor.from_numpy(big))
    assert not received.flags.writeable
    with pytest.raises(BufferError):
        received.__dlpack__()
    views = [np.broadcast_to(small, (4, 5)), received, received.transpose(2, 0, 1),
             np.broadcast_to(big[:, :1, :], (3, 40, 30))]
    sizes = [v.size * v.itemsize for v in views]
    assert sizes[0] < 4096 <= min(sizes[1:])
    for x, (y, info) in zip(views, _roundtrip(views)):
        assert y.shape == x.shape and y.dtype == x.dtype and np.array_equal(y, x)
        assert info == oracle(x)[1]


def test_pinned_dlpack_producers_are_accepted(lib):
    """A producer that reports kDLCUDAHost / kDLROCMHost (a pinned torch tensor) is a host source
    (sent declared pinned, so copied inside the call); memory of another vendor's device is a
    TypeError."""
    class Reports:
        def __init__(self, x, dev):
            self.x, self.dev = x, dev

        def __dlpack_device__(self):
            return (self.dev, 0)

        def __dlpack__(self, **kw):
            return self.x.__dlpack__()
    x = base(np.float32, (40, 30))
    sent = [Reports(x.T, 3), Reports(x, 11)]
    for v, (y, info) in zip((x.T, x), _roundtrip(sent)):
        assert y.shape == v.shape and np.array_equal(y, v) and info == oracle(v)[1]
    d = InProcessDaemon({"nodes": [{"id": "src", "outputs": ["out"]}]})
    a = _start_nodes(d.shm, ["src"])["src"]
    try:
        for dev in (2, 8):   # kDLCUDA, kDLMetal
            with pytest.raises(TypeError):
                a.send_output("out", Reports(x, dev))
    finally:
        a.close()
        d.join()


def test_host_dataflow_delivers_cpu_torch_views(lib):
    import torch
    views = _views()[:5]  # (torch has no negative strides)
    b = [torch.from_numpy(x) for x in _bases()]
    sent = [b[0].T, b[1].permute(2, 0, 1), b[2].T, b[3].permute(2, 0, 1), b[4]]
    for t, v in zip(sent, views):
        assert tuple(t.shape) == v.shape and (not v.flags.c_contiguous) == (not t.is_contiguous())
    for x, (y, info) in zip(views, _roundtrip(sent)):
        assert y.shape == x.shape and np.array_equal(y, x)
        assert info == oracle(x)[1]


def test_send_output_refuses_what_is_not_a_tensor(lib):
    d = InProcessDaemon({"nodes": [{"id": "src", "outputs": ["out"]}]})
    a = _start_nodes(d.shm, ["src"])["src"]
    try:
        with pytest.raises(TypeError):
            a.send_output("out", object())
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", np.zeros((2, 2), np.bool_))
        assert e.value.code == -4 and "bool" in str(e.value)
        with pytest.raises(DoraGpuError) as e:
            a.send_output("out", np.zeros((2, 2), np.complex64))
        assert e.value.code == -4
    finally:
        a.close()
        d.join()
