"""Device tensor views through dora_gpu_pack on the GPU (kernel level, no torch): a numpy base is
uploaded, the view described over the device pointer (tensor._describe), planned with
ARROW_DEVICE_ROCM and packed into a poisoned destination with 4 KiB guard bands on both sides.
The bytes equal numpy's row-major copy of the view, the guard bands keep their poison, the type
info is the oracle's for the equivalent nested array.  Views: tests/gather_views.py (every one
passed the sanitized host emulation of test_gather_index_host.py, for gather_rows_kernel and for
gather_tile_kernel; each runs with the library's selection and with either kernel forced), dense ones, d0 == 0, and one
source spanning more than 4 GiB.  A view that leaves its allocation by one byte, or a host
pointer declared as device memory, is refused with nothing launched."""
import ctypes
from ctypes import byref, c_void_p

import numpy as np
import pytest

from tests import gather_views

pytestmark = pytest.mark.gpu

GUARD = 4096
POISON = 0xA5


@pytest.fixture(scope="module")
def dev():
    from dora_amd import device
    assert device.device_count() >= 1
    device.set_device(0)
    s = device.Stream()
    yield s
    s.close()


def plan_device(ptr, shape, strides, dtype, byte_offset=0):
    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from dora_amd.arrow_utils import Plan
    t, keep = tensor._describe(ptr, shape, strides, dtype, byte_offset)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor", byref(t), ARROW_DEVICE_ROCM, byref(h))
    return Plan(h.value, keep)


def pack_guarded(plan, stream, mis=0):
    """Pack `plan` into a poisoned buffer at GUARD + mis; (sample bytes, guards intact)."""
    from dora_amd.device import DeviceBuffer
    n = plan.size
    buf = DeviceBuffer(n + 2 * GUARD + 16)
    try:
        buf.fill(POISON, stream)
        plan.pack(buf.ptr + GUARD + mis, n, stream)
        stream.sync()
        raw = buf.to_bytes(stream=stream)
    finally:
        buf.free()
    lo, hi = raw[:GUARD + mis], raw[GUARD + mis + n:]
    return raw[GUARD + mis:GUARD + mis + n], lo == bytes([POISON]) * len(lo) and hi == bytes([POISON]) * len(hi)


def check_view(b, v, stream, misaligned=(0,)):
    from dora_amd import tensor
    from dora_amd.device import DeviceBuffer
    from oracle.pack_ref import pack
    want, info = pack(tensor.from_numpy(v))
    assert bytes(want) == np.ascontiguousarray(v).tobytes()
    src = DeviceBuffer.from_bytes(b.tobytes(), stream)
    try:
        shape, strides, dtype, off = gather_views.describe_view(b, v, src.ptr)
        with plan_device(src.ptr, shape, strides, dtype, off) as p:
            assert p.size == len(want)
            assert p.type_info().to_json() == info.to_json()
            # the library's own selection, then each kernel forced (rows; tile wherever it applies)
            from dora_amd import _lib
            try:
                for mode in (0, 1, 2):
                    _lib.call("dora_gpu_test_gather_kernel", mode)
                    for mis in misaligned:
                        got, intact = pack_guarded(p, stream, mis)
                        assert intact, f"guard bands overwritten (destination {mis} mod 16, kernel {mode})"
                        assert got == bytes(want), f"destination {mis} mod 16, kernel {mode}"
            finally:
                _lib.call("dora_gpu_test_gather_kernel", 0)
    finally:
        src.free()


BIG = {"u8_frame_hwc_to_chw", "f32_1100x1024_T"}


@pytest.mark.parametrize("name", list(gather_views.VIEWS))
def test_strided_view_matches_numpy_and_oracle(dev, name):
    b, v = gather_views.make(name)
    assert not v.flags.c_contiguous
    check_view(b, v, dev, (0,) if name in BIG else (0, 3, 8))


def test_dense_and_single_element_views(dev):
    b = gather_views.base(np.float32, (6, 5, 4))
    for v in (b, b[2:5], b[1:2, 3:4, 2:3], b[:, None]):
        check_view(b, v, dev)
    one = gather_views.base(np.int16, (1, 1))
    check_view(one, one, dev)


def test_empty_tensor(dev):
    from dora_amd import tensor
    from oracle.pack_ref import pack
    x = np.zeros((0, 3, 2), np.float32)
    want, info = pack(tensor.from_numpy(x))
    with plan_device(None, x.shape, None, x.dtype) as p:
        assert p.size == len(want) == 0
        assert p.type_info().to_json() == info.to_json()
        p.pack(None, 0, dev)
        dev.sync()


def test_source_spanning_more_than_4_gib(dev):
    """(4300, 64) uint8 with a row stride of 2^20 + 3 over splitmix64 bytes: source offsets past
    2^32; the expected bytes are the generator's at those offsets."""
    from dora_amd import _lib
    from dora_amd._lib import DoraGpuError
    from dora_amd.device import DeviceBuffer
    from oracle import checksum_ref as cr
    rows, cols, stride, seed = 4300, 64, 2 ** 20 + 3, 0xD05A
    span = (rows - 1) * stride + cols
    assert span > 2 ** 32
    try:
        src = DeviceBuffer(span)
    except DoraGpuError as e:
        pytest.skip(f"no {span} byte allocation on this GPU: {e}")
    try:
        _lib.call("dora_gpu_fill_splitmix", src.ptr, span, seed, dev.handle)
        dev.sync()
        # generator word k = fmix64(seed + (k + 1) * GOLDEN), little-endian (splitmix_bytes)
        offs = (np.arange(rows, dtype=np.uint64)[:, None] * np.uint64(stride) +
                np.arange(cols, dtype=np.uint64)[None, :])
        with np.errstate(over="ignore"):
            words = cr.fmix64_np(np.uint64(seed & cr.MASK) + (offs // np.uint64(8) + np.uint64(1)) * cr.GOLDEN)
        want = ((words >> ((offs % np.uint64(8)) * np.uint64(8))) & np.uint64(0xFF)).astype(np.uint8)
        assert want[0].tobytes() == cr.splitmix_bytes(cols, seed)
        with plan_device(src.ptr, (rows, cols), (stride, 1), np.uint8) as p:
            got, intact = pack_guarded(p, dev)
        assert intact and got == want.tobytes()
    finally:
        src.free()


def test_views_outside_their_allocation_launch_nothing(dev):
    from dora_amd._lib import DoraGpuError
    from dora_amd.device import DeviceBuffer
    n = 1 << 20
    src = DeviceBuffer(n)
    dst = DeviceBuffer(n)
    try:
        dst.fill(POISON, dev)
        dev.sync()
        cases = {
            # 64 rows of 16 bytes, the last ending one byte past the allocation
            "one byte past the end": ((64, 16), (n // 64, 1), n - (63 * (n // 64) + 16) + 1),
            # reversed rows, the lowest starting one byte before the allocation
            "one byte before the start": ((64, 16), (-(n // 64), 1), 63 * (n // 64) - 1),
            "dense, one byte past the end": ((n,), None, 1),
        }
        for name, (shape, strides, off) in cases.items():
            with plan_device(src.ptr, shape, strides, np.uint8, off) as p:
                with pytest.raises(DoraGpuError) as e:
                    p.pack(dst.ptr, n, dev)
                assert e.value.code == -1, name
                assert "allocation" in str(e.value), name
        # a host pointer declared as device memory
        host = ctypes.create_string_buffer(4096)
        with plan_device(ctypes.addressof(host), (8, 16), (32, 1), np.uint8) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, n, dev)
            assert e.value.code == -1
        dev.sync()
        assert dst.to_bytes(stream=dev) == bytes([POISON]) * n  # nothing was launched
        # the same views moved back inside are accepted
        with plan_device(src.ptr, (64, 16), (n // 64, 1), np.uint8, n - (63 * (n // 64) + 16)) as p:
            p.pack(dst.ptr, n, dev)
        with plan_device(src.ptr, (64, 16), (-(n // 64), 1), np.uint8, 63 * (n // 64)) as p:
            p.pack(dst.ptr + 4096, n - 4096, dev)
        dev.sync()
    finally:
        src.free()
        dst.free()
