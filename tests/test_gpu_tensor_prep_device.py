"""Model-input plans through dora_gpu_pack on the GPU (kernel level, no torch): the bases of a prep
record (tests/prep_records.py), its tables and boxes among them, are uploaded, every field, table
and box tensor described over its device pointer, planned with dora_gpu_plan_tensor_prep
(ARROW_DEVICE_ROCM) and packed — one launch of gather_resize_prep_kernel or
gather_crop_prep_kernel, which reads tables and boxes in HBM — into a poisoned destination with
4 KiB guard bands on both sides.  Every field's region equals `tensor.from_numpy_resize` /
`tensor.from_numpy_crops` bit for bit (NaN for NaN), the guard bands and every padding byte keep
the poison, the type info is the oracle's.  The cases are those of test_prep_index_host.py, each of
which passed the sanitized host emulation there.  A table that ends one byte past its allocation
is refused with nothing launched."""
import numpy as np
import pytest

from tests import crop_records as kr
from tests import prep_records as pr
from tests import resize_records as rr
from tests.test_gpu_tensor_resize_device import pack_at
from tests.test_gpu_tensor_struct_device import GUARD, POISON, Uploaded
from tests.test_tensor_prep_host import oracle

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
    sample, info, ranges = oracle(rec)
    up = Uploaded(pr.triples(rec), stream)
    buf = DeviceBuffer(len(sample) + 2 * GUARD + 16)
    crops = any(c and "boxes" in c for _, _, _, c in rec)
    paths = set()
    try:
        with pr.plan_prep(rec, up.ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample), what
            assert p.type_info().to_json() == info.to_json(), what
            # one launch, of the new kernel: gather_crop_prep_kernel (10) or gather_resize_prep_kernel (9)
            assert p.segments() == [] and pr.plan_launch(p) == (10 if crops else 9), what
            for mis in offsets:
                at = buf.ptr + GUARD + mis
                for k in kr.plan_crops(p, len(rec), at) if crops else rr.plan_resizes(p, len(rec), at):
                    if k["mode"]:
                        paths |= {n for n in ("head", "units", "tail") if k[n]}
                got, intact = pack_at(p, buf, stream, mis)
                assert intact, f"guard bands overwritten, {what}, destination {mis} mod 16"
                for (off, ln), (_, _, v, c) in zip(ranges, rec):
                    pr.same(got[off:off + ln], pr.want(v, c), f"{what}, destination {mis} mod 16")
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
    for label, rec, offsets in pr.cases():
        paths |= run_record(rec, dev, offsets, label)
    assert paths == {"head", "units", "tail"}, paths


def test_more_than_one_workgroup(dev):
    """A (70, 90, 3) uint8 frame letterboxed into 300 x 300 with tables: 16875 units of uint8, 66
    workgroups, a view cut from a wider base, padding above and below the image."""
    for label, rec in pr.many():
        (_, _, v, c), = rec
        assert c["prep"]["inner"] == (233, 300) and c["prep"]["lead"] == (33, 0), c["prep"]
        assert pr.want(v, c).size == 300 * 300 * 3
        run_record(rec, dev, (0, 6), label)


def test_the_limit_of_the_contract(dev):
    """prep_records.limit_cases(): an output axis of 32768 steps whose image ends with it, each
    after it passed the emulation in test_prep_index_host.py."""
    for label, rec, offsets in pr.limit_cases():
        run_record(rec, dev, offsets, label)


def test_refused_with_nothing_launched(dev):
    """A bias table that reaches one byte past its allocation, named: DORA_ERR_INVALID, the
    destination keeps its poison.  Moved inside, its last word the allocation's last, the same
    plan packs."""
    from ctypes import byref, c_void_p, pointer
    from dora_amd import _lib, tensor
    from dora_amd._lib import (ARROW_DEVICE_ROCM, RESIZE_NEAREST, DoraGpuError, TensorPrep,
                               TensorResize)
    from dora_amd.arrow_utils import Plan
    from dora_amd.device import DeviceBuffer
    n = 1 << 16
    words = np.array([1.0, 2.0, 3.0], np.float32)
    frame, dst = DeviceBuffer(n), DeviceBuffer(n)
    table = DeviceBuffer.from_bytes(bytes(n - 12) + words.tobytes(), dev)
    short = DeviceBuffer.from_bytes(bytes(n - 12) + words.tobytes()[:-1], dev)  # one byte less
    try:
        dst.fill(POISON, dev)
        frame.fill(5, dev)
        dev.sync()

        def plan(table_in):
            # a 8 x 8 x 3 uint8 frame -> 4 x 6 x 3 float32 placed at (1, 1) in a 6 x 8 output of
            # fill 2, plus bias[c]; the bias ends at the last byte of `table`, one past `short`
            ft = tensor._describe(frame.ptr, (8, 8, 3), None, np.uint8, 0)
            bt = tensor._describe(table_in.ptr, (3,), (1,), np.float32, n - 12)
            lst, keep = tensor._describe_list(None, [ft[0]], ft[0], 0, 0)
            arr, parr = (TensorResize * 1)(), (TensorPrep * 1)()
            arr[0].mode, arr[0].dtype_code, arr[0].dtype_bits = RESIZE_NEAREST, 2, 32
            arr[0].axis[0], arr[0].axis[1], arr[0].size[0], arr[0].size[1] = 0, 1, 6, 8
            parr[0].bias, parr[0].axis = pointer(bt[0]), 2
            parr[0].inner[0], parr[0].inner[1], parr[0].lead[0], parr[0].lead[1] = 4, 6, 1, 1
            parr[0].fill = 2.0
            h = c_void_p()
            _lib.call("dora_gpu_plan_tensor_prep", lst.fields, 1, arr, None, parr, ARROW_DEVICE_ROCM,
                      byref(h))
            return Plan(h.value, (lst, keep, ft, bt, arr, parr))

        with plan(short) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, n, dev)
            assert e.value.code == -1
            assert "bias table" in str(e.value) and "allocation" in str(e.value)
        dev.sync()
        assert dst.to_bytes(stream=dev) == bytes([POISON]) * n  # nothing was launched
        with plan(table) as p:
            assert pr.plan_launch(p) == 9
            p.pack(dst.ptr, n, dev)
            dev.sync()
            got = np.frombuffer(dst.to_bytes(stream=dev)[:p.size], np.float32).reshape(6, 8, 3)
            want = np.full((6, 8, 3), 2.0, np.float32)
            want[1:5, 1:7] = 5.0
            assert (got == want + words).all()
    finally:
        for b in (frame, table, short, dst):
            b.free()
