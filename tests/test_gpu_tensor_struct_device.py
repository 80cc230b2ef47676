"""Struct-of-tensors plans through dora_gpu_pack on the GPU (kernel level, no torch): the bases of
a record (tests/struct_records.py) are uploaded, every field described over its device pointer,
planned with dora_gpu_plan_tensor_struct (ARROW_DEVICE_ROCM) and packed — one launch of
gather_struct_kernel when any field is strided — into a poisoned destination with 4 KiB guard
bands on both sides.  Every field's region equals the oracle's, the guard bands and every padding
byte keep the poison, the type info is the oracle's for the StructArray.  Every record passed the
sanitized host emulation of test_gather_struct_index_host.py; each runs with the library's
selection and with either body forced, at destinations 0, 3 and 8 mod 16.  Fields may sit in
different allocations; one that leaves its allocation by a byte is refused, naming the field,
with nothing launched."""
import numpy as np
import pytest

from tests import struct_records as sr

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


class Uploaded:
    """The distinct bases of a record in device memory, one allocation each."""

    def __init__(self, rec, stream):
        from dora_amd.device import DeviceBuffer
        self.bases = sr.bases_of(rec)
        self.bufs = [DeviceBuffer.from_bytes(b.tobytes(), stream) for b in self.bases]

    def ptr_of(self, b):
        return self.bufs[next(i for i, x in enumerate(self.bases) if x is b)].ptr

    def free(self):
        for b in self.bufs:
            b.free()


def pack_guarded(plan, stream, mis):
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


def check_sample(got, sample, ranges, what):
    pad = bytearray(got)
    for k, (off, ln) in enumerate(ranges):
        assert got[off:off + ln] == sample[off:off + ln], f"field {k}, {what}"
        pad[off:off + ln] = bytes([POISON]) * ln
    assert bytes(pad) == bytes([POISON]) * len(got), f"padding written, {what}"


@pytest.mark.parametrize("name", list(sr.RECORDS))
def test_record_matches_the_oracle(dev, name):
    from dora_amd import _lib
    from dora_amd._lib import ARROW_DEVICE_ROCM
    rec = sr.RECORDS[name]()
    sample, info, ranges = sr.oracle(rec)
    up = Uploaded(rec, dev)
    try:
        with sr.plan_record(rec, up.ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample)
            assert p.type_info().to_json() == info.to_json()
            assert p.segments() == []  # a multi-gather plan
            try:
                for mode in (0, 1, 2):
                    _lib.call("dora_gpu_test_gather_kernel", mode)
                    for mis in (0, 3, 8):
                        what = f"destination {mis} mod 16, kernel {mode}"
                        got, intact = pack_guarded(p, dev, mis)
                        assert intact, "guard bands overwritten, " + what
                        check_sample(got, sample, ranges, what)
            finally:
                _lib.call("dora_gpu_test_gather_kernel", 0)
    finally:
        up.free()


def test_all_dense_fields_take_the_segment_pack(dev):
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from tests.gather_views import base
    a, b, c = base(np.float32, (67, 4)), base(np.float16, (67,)), base(np.uint8, (69, 3))
    rec = [("a", a, a), ("b", b, b), ("c", c, c[1:68])]
    sample, info, ranges = sr.oracle(rec)
    up = Uploaded(rec, dev)
    try:
        with sr.plan_record(rec, up.ptr_of, ARROW_DEVICE_ROCM) as p:
            assert len(p.segments()) == 3 and p.type_info().to_json() == info.to_json()
            for mis in (0, 3, 8):
                got, intact = pack_guarded(p, dev, mis)
                assert intact
                check_sample(got, sample, ranges, f"destination {mis} mod 16")
    finally:
        up.free()


def test_a_field_outside_its_allocation_launches_nothing(dev):
    """Fields in two allocations pass; the second field reaching one byte past its own
    allocation is refused by name, strided or dense, and the destination keeps its poison."""
    from dora_amd import tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM, DoraGpuError
    from dora_amd.device import DeviceBuffer
    n = 1 << 20
    one, two, dst = DeviceBuffer(n), DeviceBuffer(n), DeviceBuffer(n)
    try:
        dst.fill(POISON, dev)
        dev.sync()

        def plan(second_off, second_strides):
            # `first`: 64 rows of 16 bytes cut from rows of 32, inside `one`; `second`: 64 rows
            # of 16 bytes in `two`, ending at its last byte when second_off is 0
            end = 63 * (second_strides[0] if second_strides else 16) + 16
            ts = [tensor._describe(one.ptr, (64, 16), (32, 1), np.uint8),
                  tensor._describe(two.ptr, (64, 16), second_strides, np.uint8, n - end + second_off)]
            fields, keep = tensor._describe_fields(["first", "second"], [t for t, _ in ts])
            from ctypes import byref, c_void_p
            from dora_amd import _lib
            from dora_amd.arrow_utils import Plan
            h = c_void_p()
            _lib.call("dora_gpu_plan_tensor_struct", fields, 2, ARROW_DEVICE_ROCM, byref(h))
            return Plan(h.value, (fields, keep, ts))

        for strides in ((n // 64, 1), None):  # `second` strided, then dense: a multi-gather either way
            with plan(1, strides) as p:
                with pytest.raises(DoraGpuError) as e:
                    p.pack(dst.ptr, n, dev)
                assert e.value.code == -1
                assert "field 1 `second`" in str(e.value) and "allocation" in str(e.value)
        dev.sync()
        assert dst.to_bytes(stream=dev) == bytes([POISON]) * n  # nothing was launched
        # moved back inside, the same fields in their two allocations are accepted
        with plan(0, (n // 64, 1)) as p:
            p.pack(dst.ptr, n, dev)
        dev.sync()
    finally:
        for b in (one, two, dst):
            b.free()
