"""Crop plans through dora_gpu_pack on the GPU (kernel level, no torch): the bases of a crop record
(tests/crop_records.py), its boxes among them, are uploaded, every field and its boxes described
over their device pointers, planned with dora_gpu_plan_tensor_crop (ARROW_DEVICE_ROCM) and packed —
one launch of gather_crop_kernel, which reads the boxes in HBM — into a poisoned destination with
4 KiB guard bands on both sides.  Every field's region equals `tensor.from_numpy_crops` bit for bit
(NaN for NaN), the guard bands and every padding byte keep the poison, the type info is the
oracle's.  The cases are those of test_crop_index_host.py, each of which passed the sanitized host
emulation there.  Boxes or a frame that end one byte past their allocation and a destination that
is odd for a 16-bit dtype are refused with nothing launched."""
import numpy as np
import pytest

from tests import crop_records as kr
from tests.test_gpu_tensor_resize_device import pack_at
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


def run_record(rec, stream, offsets, what):
    """Plan `rec` over uploaded bases and pack it at every offset of `offsets`; the unit paths
    the probe reports for the launches that ran."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from dora_amd.device import DeviceBuffer
    sample, info, ranges = kr.oracle(rec)
    up = Uploaded(kr.triples(rec), stream)
    buf = DeviceBuffer(len(sample) + 2 * GUARD + 16)
    paths = set()
    try:
        with kr.plan_crop(rec, up.ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample), what
            assert p.type_info().to_json() == info.to_json(), what
            assert p.segments() == [], what
            for mis in offsets:
                for k in kr.plan_crops(p, len(rec), buf.ptr + GUARD + mis) if len(sample) else ():
                    if k["mode"]:
                        assert k["device"] == 1, what
                        paths |= {n for n in ("head", "units", "tail") if k[n]}
                got, intact = pack_at(p, buf, stream, mis)
                assert intact, f"guard bands overwritten, {what}, destination {mis} mod 16"
                for (off, ln), (_, _, v, c) in zip(ranges, rec):
                    kr.same(got[off:off + ln], kr.want(v, c), f"{what}, destination {mis} mod 16")
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
    for label, rec, offsets in kr.cases():
        paths |= run_record(rec, dev, offsets, label)
    assert paths == {"head", "units", "tail"}, paths


def test_more_than_one_workgroup(dev):
    """K = 40 crops of 32 x 32 x 3 uint8 are 7680 units: 30 workgroups, lanes past the head and
    tail lanes, a view cut from a wider base, boxes that overhang and boxes that are empty — of
    which at most 10, so that zeros cannot stand in for the crops."""
    for label, rec in kr.many():
        (_, _, v, c), = rec
        expect = kr.want(v, c)
        full = sum(bool(expect[k].any()) for k in range(40))
        over = sum(bool(r[0] < 0 or r[1] < 0 or r[2] > 70 or r[3] > 90) for r in c["boxes"].tolist())
        assert expect.shape == (40, 32, 32, 3) and 30 <= full < 40 and over >= 5, (full, over)
        run_record(rec, dev, (0, 7), label)


def test_the_limit_of_the_contract(dev):
    """crop_records.limit_cases(): a frame axis of 32768 steps under boxes over all of it, its
    last row and the int32 extremes, each after it passed the emulation in
    test_crop_index_host.py."""
    for label, rec, offsets in kr.limit_cases():
        run_record(rec, dev, offsets, label)


def test_refused_with_nothing_launched(dev):
    """Boxes that end one byte past their allocation, named; a frame whose view does; a destination
    that is odd for int16: DORA_ERR_INVALID, the destination keeps its poison.  Moved back inside
    and aligned, the same plan packs."""
    from ctypes import byref, c_void_p, pointer
    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM, RESIZE_BILINEAR, DoraGpuError, TensorCrop
    from dora_amd.arrow_utils import Plan
    from dora_amd.device import DeviceBuffer
    n = 1 << 20
    k = 6
    rows = np.array([(0, 0, 16, 64), (3, 5, 9, 40), (-2, -2, 4, 4), (5, 5, 5, 9), (10, 60, 99, 99),
                     (0, 0, 1, 1)], np.int32)
    # the boxes' last byte is their allocation's last byte
    frame, dst = DeviceBuffer(n), DeviceBuffer(n)
    boxes = DeviceBuffer.from_bytes(bytes(n - 16 * k) + rows.tobytes(), dev)
    short = DeviceBuffer.from_bytes(bytes(n - 16 * k) + rows.tobytes()[:-1], dev)  # one byte less
    try:
        dst.fill(POISON, dev)
        frame.fill(3, dev)
        dev.sync()

        def plan(frame_off, boxes_in):
            # a 16 x 64 uint8 frame with rows n / 16 bytes apart, its last element the allocation's
            # last byte when frame_off is 0; k boxes ending at the last byte of `boxes` and one
            # byte past the end of `short`; crops of 5 x 9 int16
            stride = n // 16
            end = 15 * stride + 64
            ft = tensor._describe(frame.ptr, (16, 64), (stride, 1), np.uint8, n - end + frame_off)
            bt = tensor._describe(boxes_in.ptr, (k, 4), (4, 1), np.int32, n - 16 * k)
            lst, keep = tensor._describe_list(None, [ft[0]], ft[0], 0, 0)
            arr = (TensorCrop * 1)()
            arr[0].mode, arr[0].dtype_code, arr[0].dtype_bits = RESIZE_BILINEAR, 0, 16
            arr[0].axis[0], arr[0].axis[1], arr[0].size[0], arr[0].size[1] = 0, 1, 5, 9
            arr[0].boxes = pointer(bt[0])
            h = c_void_p()
            _lib.call("dora_gpu_plan_tensor_crop", lst.fields, 1, arr, ARROW_DEVICE_ROCM, byref(h))
            return Plan(h.value, (lst, keep, ft, bt, arr))

        with plan(0, short) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, n, dev)
            assert e.value.code == -1
            assert "boxes" in str(e.value) and "allocation" in str(e.value)
        with plan(1, boxes) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, n, dev)
            assert e.value.code == -1
            assert "boxes" not in str(e.value) and "allocation" in str(e.value)
        with plan(0, boxes) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr + 1, n - 16, dev)
            assert e.value.code == -1 and "nothing was launched" in str(e.value)
        dev.sync()
        assert dst.to_bytes(stream=dev) == bytes([POISON]) * n  # nothing was launched
        # inside and aligned, frame and boxes each ending on their allocation's last byte: a
        # constant frame gives constant crops, empty boxes zeros
        with plan(0, boxes) as p:
            p.pack(dst.ptr, n, dev)
            dev.sync()
            got = np.frombuffer(dst.to_bytes(stream=dev)[:p.size], np.int16).reshape(k, 5, 9)
            for i, r in enumerate(rows.tolist()):
                empty = min(max(r[2], 0), 16) <= min(max(r[0], 0), 16) or \
                    min(max(r[3], 0), 64) <= min(max(r[1], 0), 64)
                assert (got[i] == (0 if empty else 3)).all(), (i, r)
            assert not got[3].any() and got[0].all()
    finally:
        for b in (frame, boxes, short, dst):
            b.free()
