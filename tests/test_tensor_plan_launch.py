"""What fills the sample of every kind of tensor plan, on the CPU (no GPU): small plans over real
numpy memory — passed as ARROW_DEVICE_ROCM where a device plan is wanted: planning calls nothing in
HIP and reads no device byte — whose launch kind dora_gpu_test_plan_launch reports, and the same
fact as the older probes state it: `gather` of dora_gpu_test_plan_gather / _field is
`launch != kSegments`, `device` of _take / _mask is `launch == kTaken / kMasked`, and a field that
_cast reports as cast sits in a kCast plan."""
from ctypes import byref, c_int, c_int64, c_uint32, c_uint64, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, PARTITION_LENGTHS,
                           PARTITION_OFFSETS, DoraGpuError)
from dora_amd.arrow_utils import Plan
from tests import cast_records as cr
from tests import list_records as lr
from tests import mask_records as mr
from tests import quant_records as qr
from tests import struct_records as sr
from tests import take_records as tr
from tests.gather_views import describe_view

SEGMENTS, VIEW, FIELDS, CAST, TAKEN, MASKED = range(6)
CPU, GPU = ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM


def host_ptr(b):
    return b.__array_interface__["data"][0]


def grid(rows=4, cols=3, dtype=np.float32):
    return np.arange(rows * cols, dtype=dtype).reshape(rows, cols)


def plan_tensor(b, v, dev):
    shape, strides, dtype, off = describe_view(b, v, None)
    t, keep = tensor._describe(host_ptr(b), shape, strides, dtype, off)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor", byref(t), dev, byref(h))
    return Plan(h.value, (keep, b))


def launch_of(p):
    launch, scan, checked = c_int(-1), c_int(-1), c_int(-1)
    _lib.call("dora_gpu_test_plan_launch", p.handle, byref(launch), byref(scan), byref(checked))
    return launch.value, bool(scan.value), bool(checked.value)


def desc(p):
    """dora_gpu_test_plan_gather of a bare device tensor plan."""
    g, src, nd, row, elem = c_int(), c_void_p(), c_int(), c_uint64(), c_uint32()
    shp, std, lo, hi = (c_int64 * 8)(), (c_int64 * 8)(), c_int64(), c_int64()
    _lib.call("dora_gpu_test_plan_gather", p.handle, byref(g), byref(src), byref(nd), byref(row),
              byref(elem), shp, std, byref(lo), byref(hi))
    return {"gather": bool(g.value)}


def probe(fn, p):
    """What an older probe says of `p`, or None where it refuses the plan as not its kind."""
    try:
        return fn(p)
    except DoraGpuError:
        return None


def agrees(p, launch, scan, checked):
    """The older probes state the same facts."""
    one, fields = probe(desc, p), probe(sr.plan_fields, p)
    assert (one is not None or fields is not None) <= checked  # both describe device plans only
    if one is not None:
        assert one["gather"] == (launch != SEGMENTS)
    if fields is not None:
        assert all(f["gather"] == (launch != SEGMENTS) for f in fields)
        assert all(f["kind"] == -1 for f in fields) or launch not in (TAKEN, MASKED)
        casts = cr.plan_casts(p)
        assert any(c["cast"] for c in casts) == (launch == CAST)
    if not checked:
        assert launch == SEGMENTS  # a host plan, or an empty one
    ragged = probe(lr.plan_scan, p)
    assert scan == (ragged is not None and ragged["scan"])
    take, mask = probe(tr.plan_index, p), probe(mr.plan_info, p)
    assert (launch == TAKEN) == (take is not None and take["device"])
    assert (launch == MASKED) == (mask is not None and mask["device"])
    assert mr.workspace_size(p) > 0 if launch == MASKED else mr.workspace_size(p) == 0


def record(strided, rows=4):
    """Two fields of `rows` rows: three float32 (or two of them, cut from the three) and an int16."""
    b, k = grid(rows, 3), grid(rows, 2, np.int16)
    return [("a", b, b[:, ::2] if strided else b), ("k", k, k)]


def bare(strided, rows=4):
    b = grid(rows, 3)
    return [(None, b, b[:, ::2] if strided else b)]


def with_casts(rec, casts):
    return [(n, b, v, c) for (n, b, v), c in zip(rec, casts)]


I32 = lambda *w: np.array(w, np.int32)  # noqa: E731
I64 = lambda *w: np.array(w, np.int64)  # noqa: E731
F32_TO_F16 = cr.cast("float32", "float16")
F32_TO_U8 = qr.quant("float32", "uint8", 0.5, 3)
MASK = np.array([1, 0, 1, 1], np.uint8)

# name -> (plan builder, launch kind, scan share, range checked)
CASES = {
    # a tensor, bare
    "tensor host dense": (lambda: plan_tensor(*bare(False)[0][1:], CPU), SEGMENTS, False, False),
    "tensor host strided": (lambda: plan_tensor(*bare(True)[0][1:], CPU), SEGMENTS, False, False),
    "tensor device dense": (lambda: plan_tensor(*bare(False)[0][1:], GPU), SEGMENTS, False, True),
    "tensor device strided": (lambda: plan_tensor(*bare(True)[0][1:], GPU), VIEW, False, True),
    "tensor host empty": (lambda: plan_tensor(*bare(False, 0)[0][1:], CPU), SEGMENTS, False, False),
    "tensor device empty": (lambda: plan_tensor(*bare(True, 0)[0][1:], GPU), SEGMENTS, False,
                            False),
    # a record
    "record host": (lambda: sr.plan_record(record(True), host_ptr, CPU), SEGMENTS, False, False),
    "record device dense": (lambda: sr.plan_record(record(False), host_ptr, GPU), SEGMENTS, False,
                            True),
    "record device strided": (lambda: sr.plan_record(record(True), host_ptr, GPU), FIELDS, False,
                              True),
    # a cast: no field converted (the plain plan's kind), one field converted
    "cast none dense": (lambda: cr.plan_cast(with_casts(record(False), [None, None]), host_ptr,
                                             GPU), SEGMENTS, False, True),
    "cast none strided": (lambda: cr.plan_cast(with_casts(record(True), [None, None]), host_ptr,
                                               GPU), FIELDS, False, True),
    "cast none bare strided": (lambda: cr.plan_cast(with_casts(bare(True), [None]), host_ptr, GPU),
                               VIEW, False, True),
    "cast identity": (lambda: cr.plan_cast(
        with_casts(record(False), [cr.cast("float32", "float32"), None]), host_ptr, GPU),
        SEGMENTS, False, True),
    "cast one field": (lambda: cr.plan_cast(with_casts(record(False), [F32_TO_F16, None]),
                                            host_ptr, GPU), CAST, False, True),
    "cast bare": (lambda: cr.plan_cast(with_casts(bare(True), [F32_TO_F16]), host_ptr, GPU), CAST,
                  False, True),
    "cast host": (lambda: cr.plan_cast(with_casts(record(True), [F32_TO_F16, None]), host_ptr,
                                       CPU), SEGMENTS, False, False),
    # a quantised field
    "quant one field": (lambda: qr.plan_convert(with_casts(record(True), [F32_TO_U8, None]),
                                                host_ptr, GPU), CAST, False, True),
    "quant beside a cast": (lambda: qr.plan_convert(
        with_casts(record(False) + [("c", *bare(False)[0][1:])], [F32_TO_U8, None, F32_TO_F16]),
        host_ptr, GPU), CAST, False, True),
    "quant host": (lambda: qr.plan_convert(with_casts(bare(False), [F32_TO_U8]), host_ptr, CPU),
                   SEGMENTS, False, False),
    # a list
    "list host partition, host values": (lambda: lr.plan_list(
        record(True), host_ptr, CPU, I32(1, 3), PARTITION_LENGTHS, CPU), SEGMENTS, False, False),
    "list host partition, device dense": (lambda: lr.plan_list(
        record(False), host_ptr, GPU, I64(0, 1, 4), PARTITION_OFFSETS, CPU), SEGMENTS, False,
        True),
    "list host partition, device strided": (lambda: lr.plan_list(
        record(True), host_ptr, GPU, I32(1, 3), PARTITION_LENGTHS, CPU), FIELDS, False, True),
    "list device partition": (lambda: lr.plan_list(
        record(False), host_ptr, GPU, I32(1, 3), PARTITION_LENGTHS, GPU), FIELDS, True, True),
    "list device partition, bare": (lambda: lr.plan_list(
        bare(False), host_ptr, GPU, I64(0, 4, 4), PARTITION_OFFSETS, GPU), FIELDS, True, True),
    "list zero rows": (lambda: lr.plan_list(
        record(False, 0), host_ptr, GPU, I32(0, 0), PARTITION_LENGTHS, CPU), SEGMENTS, False,
        False),
    "list zero rows, device partition": (lambda: lr.plan_list(
        record(False, 0), host_ptr, GPU, I32(0, 0), PARTITION_LENGTHS, GPU), FIELDS, True, True),
    # a take
    "take host index": (lambda: tr.plan_take(record(True), host_ptr, CPU, I32(3, 0, 3), CPU),
                        SEGMENTS, False, False),
    "take device index": (lambda: tr.plan_take(record(False), host_ptr, GPU, I64(3, 0), GPU),
                          TAKEN, False, True),
    "take device index, bare": (lambda: tr.plan_take(bare(True), host_ptr, GPU, I32(2, 2, 1), GPU),
                                TAKEN, False, True),
    "take device index, host partition": (lambda: tr.plan_take(
        record(False), host_ptr, GPU, I32(3, 0, 1), GPU, part=I32(1, 2), form=PARTITION_LENGTHS,
        part_dev=CPU), TAKEN, False, True),
    "take device index, device partition": (lambda: tr.plan_take(
        record(True), host_ptr, GPU, I32(3, 0, 1), GPU, part=I32(0, 1, 3), form=PARTITION_OFFSETS,
        part_dev=GPU), TAKEN, True, True),
    "take K = 0, host": (lambda: tr.plan_take(record(False), host_ptr, CPU, I32(), CPU), SEGMENTS,
                         False, False),
    "take K = 0, device": (lambda: tr.plan_take(record(True), host_ptr, GPU, I32(), GPU), SEGMENTS,
                           False, False),
    "take K = 0, device partition": (lambda: tr.plan_take(
        record(False), host_ptr, GPU, I32(), GPU, part=I32(0, 0), form=PARTITION_LENGTHS,
        part_dev=GPU), FIELDS, True, True),
    # a mask
    "mask host": (lambda: mr.plan_mask(record(True), host_ptr, CPU, MASK, CPU), SEGMENTS, False,
                  False),
    "mask host, host partition": (lambda: mr.plan_mask(
        record(False), host_ptr, CPU, MASK, CPU, part=I32(1, 3), form=PARTITION_LENGTHS,
        part_dev=CPU), SEGMENTS, False, False),
    "mask device": (lambda: mr.plan_mask(record(False), host_ptr, GPU, MASK, GPU), MASKED, False,
                    True),
    "mask device, host partition": (lambda: mr.plan_mask(
        record(True), host_ptr, GPU, MASK, GPU, part=I32(1, 3), form=PARTITION_LENGTHS,
        part_dev=CPU), MASKED, True, True),
    "mask device, device partition": (lambda: mr.plan_mask(
        bare(False), host_ptr, GPU, MASK, GPU, part=I64(0, 2, 4), form=PARTITION_OFFSETS,
        part_dev=GPU), MASKED, True, True),
    "mask N = 0, host": (lambda: mr.plan_mask(record(False, 0), host_ptr, CPU, MASK[:0], CPU),
                         SEGMENTS, False, False),
    "mask N = 0, device": (lambda: mr.plan_mask(record(True, 0), host_ptr, GPU, MASK[:0], GPU),
                           SEGMENTS, False, False),
    "mask N = 0, device partition": (lambda: mr.plan_mask(
        record(False, 0), host_ptr, GPU, MASK[:0], GPU, part=I32(0, 0), form=PARTITION_LENGTHS,
        part_dev=GPU), SEGMENTS, False, False),
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_plan_says_once_what_fills_its_sample(lib, name):
    build, launch, scan, checked = CASES[name]
    with build() as p:
        assert launch_of(p) == (launch, scan, checked)
        agrees(p, launch, scan, checked)


def test_a_plan_is_needed(lib):
    with pytest.raises(DoraGpuError):
        _lib.call("dora_gpu_test_plan_launch", None, None, None, None)
