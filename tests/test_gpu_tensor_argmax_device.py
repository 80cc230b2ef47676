"""Reduce plans through dora_gpu_pack on the GPU (kernel level, no torch): the bases of an argmax
record (tests/argmax_records.py) are uploaded, every field described over its device pointer,
planned with dora_gpu_plan_tensor_reduce (ARROW_DEVICE_ROCM) and packed — one launch of
gather_reduce_kernel — into a poisoned destination with 4 KiB guard bands on both sides.  Every
field's region equals numpy's `np.argmax(x32, axis).astype(dtype)` bit for bit, the guard bands
and every padding byte keep the poison, the type info is the oracle's.  The cases are those of
test_argmax_index_host.py, each of which passed the sanitized host emulation there, under the
library's own choice of body and with the lane body and the wave body forced.  A field whose last
C step leaves its allocation by one byte and a destination that is not a multiple of the index
element size are refused with nothing launched."""
import numpy as np
import pytest

from tests import argmax_records as ar
from tests.test_gpu_tensor_struct_device import GUARD, POISON, Uploaded, check_sample

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from dora_amd import device
    assert device.device_count() >= 1
    device.set_device(0)
    s = device.Stream()
    yield s
    s.close()


def pack_at(plan, buf, stream, mis):
    """Pack `plan` into the poisoned `buf` at GUARD + mis; (sample bytes, guards intact)."""
    n = plan.size
    buf.fill(POISON, stream)
    plan.pack(buf.ptr + GUARD + mis, n, stream)
    stream.sync()
    raw = buf.to_bytes(stream=stream)
    lo, hi = raw[:GUARD + mis], raw[GUARD + mis + n:]
    return raw[GUARD + mis:GUARD + mis + n], lo == bytes([POISON]) * len(lo) and hi == bytes([POISON]) * len(hi)


def run_record(rec, stream, offsets, what):
    """Plan `rec` over uploaded bases and pack it at every offset of `offsets`; the bodies it ran."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from dora_amd.device import DeviceBuffer
    sample, info, ranges = ar.oracle(rec)
    up = Uploaded([r[:3] for r in rec], stream)
    buf = DeviceBuffer(len(sample) + 2 * GUARD + 16)
    bodies = set()
    try:
        with ar.plan_reduce(rec, up.ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample), what
            assert p.type_info().to_json() == info.to_json(), what
            assert p.segments() == [], what
            for mis in offsets:
                for k in ar.plan_reduces(p, len(rec), buf.ptr + GUARD + mis):
                    if k["op"]:
                        bodies.add("wave" if k["body"] == 2 else "lane")
                        bodies |= {n for n in ("vector_units", "element_units") if k[n]}
                got, intact = pack_at(p, buf, stream, mis)
                assert intact, f"guard bands overwritten, {what}, destination {mis} mod 16"
                for (off, ln), (_, _, v, r) in zip(ranges, rec):
                    ar.same(got[off:off + ln], ar.want(v, r), f"{what}, destination {mis} mod 16")
                check_sample(got, sample, ranges, f"{what}, destination {mis} mod 16")
    finally:
        buf.free()
        up.free()
    return bodies


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_every_case(dev, mode):
    """mode 0: the library's choice; 1: the lane body everywhere; 2: the wave body wherever the
    reduced axis is source-contiguous."""
    from dora_amd import _lib
    bodies = set()
    _lib.call("dora_gpu_test_reduce_body", mode)
    try:
        for label, rec, offsets in ar.cases():
            bodies |= run_record(rec, dev, offsets, f"{label}, body mode {mode}")
    finally:
        _lib.call("dora_gpu_test_reduce_body", 0)
    want = {"lane", "vector_units", "element_units"} | ({"wave"} if mode != 1 else set())
    assert want <= bodies, (mode, bodies)


def test_refused_with_nothing_launched(dev):
    """A reduced field whose last C step reaches one byte past its allocation, named; a
    destination that is odd for uint16 indices: DORA_ERR_INVALID, the destination keeps its
    poison.  Moved back inside and aligned, the same plans pack."""
    from ctypes import byref, c_void_p
    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM, REDUCE_ARGMAX, DoraGpuError, TensorReduce
    from dora_amd.arrow_utils import Plan
    from dora_amd.device import DeviceBuffer
    n = 1 << 20
    one, two, dst = DeviceBuffer(n), DeviceBuffer(n), DeviceBuffer(n)
    try:
        dst.fill(POISON, dev)
        one.fill(0, dev)
        two.fill(0, dev)
        dev.sync()

        def plan(second_off):
            # `first`: 64 rows of 16 bytes cut from rows of 32, sent as they are; `second`: 64
            # outputs of 16 uint8 candidates each, n / 16 bytes apart, reduced along axis 0: the
            # last candidate of the last output is the allocation's last byte when second_off is 0
            stride = n // 16
            end = 15 * stride + 64
            ts = [tensor._describe(one.ptr, (64, 16), (32, 1), np.uint8),
                  tensor._describe(two.ptr, (16, 64), (stride, 1), np.uint8, n - end + second_off)]
            lst, keep = tensor._describe_list(["first", "second"], [t for t, _ in ts], ts[0][0], 0, 0)
            reds = (TensorReduce * 2)()
            reds[1].op, reds[1].axis, reds[1].dtype_code, reds[1].dtype_bits = REDUCE_ARGMAX, 0, 1, 16
            h = c_void_p()
            _lib.call("dora_gpu_plan_tensor_reduce", lst.fields, 2, reds, ARROW_DEVICE_ROCM, byref(h))
            return Plan(h.value, (lst, keep, ts, reds))

        with plan(1) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, n, dev)
            assert e.value.code == -1
            assert "field 1 `second`" in str(e.value) and "allocation" in str(e.value)
        with plan(0) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr + 1, n - 16, dev)
            assert e.value.code == -1
            assert "field 1 `second`" in str(e.value) and "nothing was launched" in str(e.value)
        dev.sync()
        assert dst.to_bytes(stream=dev) == bytes([POISON]) * n  # nothing was launched
        with plan(0) as p:
            p.pack(dst.ptr, n, dev)
            dev.sync()
            got = dst.to_bytes(stream=dev)[:p.size]
            assert got[64 * 16:] == bytes(64 * 2)  # all zero candidates: index 0 everywhere
    finally:
        for b in (one, two, dst):
            b.free()
