"""Planning of device tensor sends on the CPU (no GPU): dora_gpu_plan_tensor with
ARROW_DEVICE_ROCM over made-up pointers (planning calls nothing in HIP and reads no tensor byte).
Dense views are one copy segment at data + byte_offset with the oracle's type info for the
equivalent nested array; strided views carry the canonical gather descriptor and the closed
interval [lo, hi] of offsets they reach (the testing library's getter) and no segments; strides
whose reach overflows int64 are refused; dtype and dimension refusals are the host path's."""
from ctypes import byref, c_int, c_int64, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, DoraGpuError
from dora_amd.arrow_utils import Plan
from oracle.pack_ref import pack

PTR = 0x7E00_0000_0000  # never dereferenced


def plan(shape, strides, dtype, byte_offset=0, ptr=PTR, dev=ARROW_DEVICE_ROCM, **over):
    t, keep = tensor._describe(ptr, shape, strides, dtype, byte_offset)
    for k, v in over.items():
        setattr(t, k, v)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor", byref(t), dev, byref(h))
    return Plan(h.value, keep)


def desc(p):
    g, src, nd, row, elem = c_int(), c_void_p(), c_int(), c_uint64(), c_uint32()
    shp, std = (c_int64 * 8)(), (c_int64 * 8)()
    lo, hi = c_int64(), c_int64()
    _lib.call("dora_gpu_test_plan_gather", p.handle, byref(g), byref(src), byref(nd), byref(row),
              byref(elem), shp, std, byref(lo), byref(hi))
    return {"gather": bool(g.value), "src": src.value, "row": row.value, "elem": elem.value,
            "dims": list(zip(list(shp)[:nd.value], list(std)[:nd.value])), "lo": lo.value,
            "hi": hi.value}


def el_strides(v):
    return [s // v.dtype.itemsize for s in v.strides]


def oracle_info(v):
    return pack(tensor.from_numpy(np.ascontiguousarray(v)))[1].to_json()


@pytest.mark.parametrize("dtype", [np.uint8, np.float16, np.int32, np.float64])
def test_dense_views_are_one_segment_in_place(lib, dtype):
    b = np.zeros((6, 5, 4), dtype)
    item = b.itemsize
    for v, off in [(b, 0), (b[1:4], b.strides[0]), (b[:, None], 0), (b.T.T, 0), (b[2:3, 1:2], 2 * b.strides[0] + b.strides[1])]:
        with plan(v.shape, el_strides(v), dtype, byte_offset=off) as p:
            assert p.segments() == [(PTR + off, 0, v.size * item)]
            assert p.size == v.size * item
            assert p.type_info().to_json() == oracle_info(v)
            d = desc(p)
            assert not d["gather"] and d["dims"] == [] and (d["lo"], d["hi"]) == (0, v.size * item - 1)
    # NULL strides: row-major
    with plan((3, 4), None, dtype, byte_offset=8) as p:
        assert p.segments() == [(PTR + 8, 0, 12 * item)]


def test_strided_views_carry_the_canonical_descriptor(lib):
    f = np.zeros((6, 5, 4), np.float32)
    cases = [
        # view, canonical (extent, byte stride) list, row bytes, lo, hi
        (f.transpose(2, 0, 1), [(4, 4), (30, 16)], 4, 0, 3 * 4 + 29 * 16 + 3),
        (f[:, 1:4], [(6, 80)], 48, 0, 5 * 80 + 47),              # inner two dimensions merge and fold
        (f[::-1], [(6, -80)], 80, -400, 79),                     # negative stride: below the first element
        (f[::-1, ::-1, ::-1], [(120, -4)], 4, -476, 3),          # all reversed: merges into one dimension
        (f[:, ::2, 0], [(6, 80), (3, 32)], 4, 0, 400 + 64 + 3),
        (np.broadcast_to(f[0, 0], (7, 4)), [(7, 0)], 16, 0, 15),  # zero stride
        (np.broadcast_to(f[:, :1, :1], (6, 5, 4)), [(6, 80), (20, 0)], 4, 0, 403),
    ]
    for v, dims, row, lo, hi in cases:
        off = v.__array_interface__["data"][0] - f.__array_interface__["data"][0]
        with plan(v.shape, el_strides(v), np.float32, byte_offset=off) as p:
            d = desc(p)
            assert d["gather"] and p.segments() == [], v.shape
            assert (d["src"], d["elem"], d["row"], d["dims"]) == (PTR + off, 4, row, dims), v.shape
            assert (d["lo"], d["hi"]) == (lo, hi), v.shape
            # the interval is exactly what the view reaches inside its base
            assert off + lo >= 0 and off + hi < f.nbytes
            assert p.size == v.size * 4
            assert p.type_info().to_json() == oracle_info(v)


def test_overflowing_strides_are_refused(lib):
    big = 2 ** 62
    for shape, strides, dtype in [
        ((4, 4), (big, 1), np.uint8),            # (n - 1) * stride overflows
        ((3, 3, 2), (big // 2, big // 2 + 1, 7), np.uint8),  # each product fits, their sum does not
        ((3, 2), (2 ** 61, 3), np.float64),      # stride * element size overflows
        ((2, 2), (2 ** 62 + 5, -(2 ** 62)), np.uint8),  # hi - lo overflows
        ((3, 3), (-(2 ** 62), 5), np.uint8),
    ]:
        with pytest.raises(DoraGpuError) as e:
            plan(shape, strides, dtype)
        assert e.value.code == -1, (shape, strides)
    # the same strides are fine when they do not overflow
    with plan((4, 4), (2 ** 40, 1), np.uint8) as p:
        assert desc(p)["hi"] == 3 * 2 ** 40 + 3


def test_refusals_match_the_host_path(lib):
    def code(dev, *a, **k):
        with pytest.raises(DoraGpuError) as e:
            plan(*a, dev=dev, **k)
        return e.value.code, str(e.value)

    buf = np.zeros(4096, np.uint8)
    host = buf.__array_interface__["data"][0]
    nine = ((4,) * 9, [2 * 8 ** k for k in range(8, -1, -1)], np.uint8)
    for args, over in [
        (((4,), None, np.bool_), {}),
        (((4,), None, np.uint8), {"dtype_code": 4, "dtype_bits": 16}),
        (((4,), None, np.complex64), {}),
        (((4,), None, np.uint8), {"dtype_lanes": 2}),
        (((4,), None, np.uint8), {"dtype_code": 0, "dtype_bits": 24}),
        (nine, {}),
        (((), None, np.uint8), {"ndim": 0}),
        (((4, -1), None, np.uint8), {}),
        (((4, 0), None, np.uint8), {}),
        (((1 << 40, 1 << 40), None, np.uint8), {}),
        (((4,), None, np.uint8), {"data": None}),
    ]:
        got = code(ARROW_DEVICE_ROCM, *args, **over)
        want = code(ARROW_DEVICE_CPU, *args, ptr=host, **over) if args is not nine else (-4, got[1])
        assert got == want, (args, over)
    assert code(ARROW_DEVICE_ROCM, *nine)[0] == -4


def test_empty_tensor_plans_an_empty_message(lib):
    x = np.zeros((0, 3, 2), np.float32)
    for data in (PTR, None):
        with plan(x.shape, None, np.float32, data=data) as p:
            assert p.size == 0 and p.segments() == []
            assert p.type_info().to_json() == oracle_info(x)
