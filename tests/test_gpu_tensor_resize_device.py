"""Resize plans through dora_gpu_pack on the GPU (kernel level, no torch): the bases of a resize
record (tests/resize_records.py) are uploaded, every field described over its device pointer,
planned with dora_gpu_plan_tensor_resize (ARROW_DEVICE_ROCM) and packed — one launch of
gather_resize_kernel — into a poisoned destination with 4 KiB guard bands on both sides.  Every
field's region equals `tensor.from_numpy_resize` bit for bit (NaN for NaN), the guard bands and
every padding byte keep the poison, the type info is the oracle's.  The cases are those of
test_resize_index_host.py, each of which passed the sanitized host emulation there.  A view that
reaches one byte past its allocation and a destination that is odd for a 16-bit dtype are refused
with nothing launched."""
import numpy as np
import pytest

from tests import resize_records as rr
from tests.test_gpu_tensor_struct_device import GUARD, POISON, Uploaded

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
    """Plan `rec` over uploaded bases and pack it at every offset of `offsets`; the unit paths
    the probe reports for the launches that ran."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from dora_amd.device import DeviceBuffer
    sample, info, ranges = rr.oracle(rec)
    up = Uploaded([r[:3] for r in rec], stream)
    buf = DeviceBuffer(len(sample) + 2 * GUARD + 16)
    paths = set()
    try:
        with rr.plan_resize(rec, up.ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample), what
            assert p.type_info().to_json() == info.to_json(), what
            assert p.segments() == [], what
            for mis in offsets:
                for k in rr.plan_resizes(p, len(rec), buf.ptr + GUARD + mis):
                    if k["mode"]:
                        paths |= {n for n in ("head", "units", "tail") if k[n]}
                got, intact = pack_at(p, buf, stream, mis)
                assert intact, f"guard bands overwritten, {what}, destination {mis} mod 16"
                for (off, ln), (_, _, v, r) in zip(ranges, rec):
                    rr.same(got[off:off + ln], rr.want(v, r), f"{what}, destination {mis} mod 16")
                pad = bytearray(got)  # every byte outside the fields keeps the poison
                for off, ln in ranges:
                    pad[off:off + ln] = bytes([POISON]) * ln
                assert bytes(pad) == bytes([POISON]) * len(pad), (what, mis)
    finally:
        buf.free()
        up.free()
    return paths


def test_every_case(dev):
    paths = set()
    for label, rec, offsets in rr.cases():
        paths |= run_record(rec, dev, offsets, label)
    assert paths == {"head", "units", "tail"}, paths


def test_more_than_one_workgroup(dev):
    """300 x 300 outputs of uint8 are 5625 units: 22 workgroups, lanes past the head and tail
    lanes, a view cut from a wider base."""
    b = rr.cr.source("uint8", (70, 90, 3), seed=61)
    for mode in rr.MODES:
        rec = [(None, b, b[1:, 2:88], rr.rs("uint8", (0, 1), (100, 300), mode))]
        run_record(rec, dev, (0, 7), f"frame {mode}")
    f = rr.cr.source("float16", (3, 40, 50), seed=62)
    rec = [(None, f, f, rr.rs("float16", (-2, -1), (97, 131), "bilinear", "float32"))]
    run_record(rec, dev, (4,), "planes")


def test_the_limit_of_the_contract(dev):
    """resize_records.limit_cases(): axes of 32768 source and output steps and the weights read
    directly, each after it passed the emulation in test_resize_index_host.py.  The device's
    weights are its own float32 divisions: these cases hold them to the statement's bit for bit."""
    for label, rec, offsets in rr.limit_cases():
        run_record(rec, dev, offsets, label)


def test_refused_with_nothing_launched(dev):
    """A resized field whose view reaches one byte past its allocation, named; a destination that
    is odd for int16: DORA_ERR_INVALID, the destination keeps its poison.  Moved back inside and
    aligned, the same plans pack."""
    from ctypes import byref, c_void_p
    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM, RESIZE_BILINEAR, DoraGpuError, TensorResize
    from dora_amd.arrow_utils import Plan
    from dora_amd.device import DeviceBuffer
    n = 1 << 20
    one, two, dst = DeviceBuffer(n), DeviceBuffer(n), DeviceBuffer(n)
    try:
        dst.fill(POISON, dev)
        one.fill(0, dev)
        two.fill(3, dev)
        dev.sync()

        def plan(second_off):
            # `first`: 8 rows of 16 bytes cut from rows of 32, sent as they are; `second`: 8 x 16 x
            # 64 uint8 with rows n / 16 bytes apart, resized along its last two axes to 5 x 9 int16:
            # the last element of the view is the allocation's last byte when second_off is 0
            stride = n // 16
            end = 7 * 16 * 64 + 15 * stride + 64
            ts = [tensor._describe(one.ptr, (8, 16), (32, 1), np.uint8),
                  tensor._describe(two.ptr, (8, 16, 64), (16 * 64, stride, 1), np.uint8,
                                   n - end + second_off)]
            lst, keep = tensor._describe_list(["first", "second"], [t for t, _ in ts], ts[0][0], 0, 0)
            arr = (TensorResize * 2)()
            arr[1].mode, arr[1].dtype_code, arr[1].dtype_bits = RESIZE_BILINEAR, 0, 16
            arr[1].axis[0], arr[1].axis[1], arr[1].size[0], arr[1].size[1] = 1, 2, 5, 9
            h = c_void_p()
            _lib.call("dora_gpu_plan_tensor_resize", lst.fields, 2, arr, ARROW_DEVICE_ROCM, byref(h))
            return Plan(h.value, (lst, keep, ts, arr))

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
            assert got[:8 * 16] == bytes(8 * 16)
            assert got[8 * 16:] == np.full(8 * 5 * 9, 3, np.int16).tobytes()  # a constant frame
    finally:
        for b in (one, two, dst):
            b.free()
