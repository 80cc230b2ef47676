"""Planning of ragged-batch messages on the CPU (no GPU): dora_gpu_plan_tensor_list over real
numpy memory and over made-up device pointers (planning calls nothing in HIP and reads no device
byte).  Size, segment offsets and type info are the reference packing's of
pa.ListArray.from_arrays(offsets, child) (oracle.pack_ref) for a bare tensor child, the C3-shaped
record, a record whose first leaf is float64 and the detector record, each cut by lengths and by
offsets given as int32, as int64 and as a Python list, B in {0, 1, 2, 16} with empty lists at
the front, in the middle and at the end, and N == 0 with B == 3; a device partition plans a scan
and is never read; every refusal carries its code and names its index or field."""
from ctypes import byref, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST,
                           PARTITION_LENGTHS, PARTITION_OFFSETS, DoraGpuError)
from oracle.pack_ref import sample_regions
from tests import list_records as lr
from tests import struct_records as sr

PTR = 0x7E00_0000_0000  # never dereferenced


def fake_ptrs(rec):
    bases = sr.bases_of(rec)
    return lambda b: PTR + (1 << 20) * next(i for i, x in enumerate(bases) if x is b)


def host_ptr(b):
    return b.__array_interface__["data"][0]


def forms(lengths):
    """(label, partition array, form) for one list of lengths: lengths and offsets, each as
    int32, as int64 and as a Python list (which the Python layer hands over as int64)."""
    offs = lr.offsets_of(lengths)
    for label, words, form in (("lengths", lengths, PARTITION_LENGTHS),
                               ("offsets", offs.tolist(), PARTITION_OFFSETS)):
        yield f"{label} int32", np.array(words, dtype=np.int32), form
        yield f"{label} int64", np.array(words, dtype=np.int64), form
        yield f"{label} list", np.asarray(list(words), dtype=np.int64).reshape(-1), form


def test_the_c3_layout_of_the_design():
    """DESIGN section 3's C3 layout from the oracle alone: the offsets first, the leaves behind."""
    rec = lr.clouds(67)
    sample, info, ranges = lr.oracle(rec, lr.offsets_of([60, 7]))
    assert info.data_type == "+l[item:?+s[x:?f,y:?f,z:?f,intensity:?C]]"
    assert [(b.offset, b.len) for b in info.buffer_offsets] == [(0, 12)]
    assert ranges == [(12, 268), (280, 268), (548, 268), (816, 67)] and len(sample) == 883
    # behind 12 bytes of offsets a float64 leaf starts after 4 bytes of padding
    _, info, ranges = lr.oracle(lr.f64_first(67), lr.offsets_of([60, 7]))
    assert ranges[0] == (16, 67 * 8)


@pytest.mark.parametrize("n", [67, 0])
@pytest.mark.parametrize("name", list(lr.RECORDS))
def test_host_plan_matches_the_oracle(lib, name, n):
    rec = lr.RECORDS[name](n)
    for lengths in lr.partitions(n):
        offs = lr.offsets_of(lengths)
        sample, info, ranges = lr.oracle(rec, offs)
        for what, part, form in forms(lengths):
            for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
                with lr.plan_list(rec, host_ptr, dev, part, form, ARROW_DEVICE_CPU) as p:
                    ctx = f"{name} n={n} lengths={lengths} {what} dev={dev}"
                    assert p.size == len(sample), ctx
                    assert p.type_info().to_json() == info.to_json(), ctx
                    segs = p.segments()
                    want = [(0, 4 * (len(lengths) + 1))] + ([] if n == 0 else ranges)
                    assert [(off, ln) for _, off, ln in segs] == want, ctx
                    # what any host path does with the segments, into a poisoned sample
                    got = np.full(p.size, 0xA5, np.uint8)
                    for src, off, ln in segs:
                        got[off:off + ln] = np.ctypeslib.as_array(
                            (np.ctypeslib.ctypes.c_uint8 * ln).from_address(src))
                    assert sample_regions(got.tobytes(), info) == sample_regions(sample, info), ctx
                    assert got[:want[0][1]].tobytes() == offs.astype(np.int32).tobytes(), ctx
                    pad = np.ones(p.size, bool)
                    for off, ln in want:
                        pad[off:off + ln] = False
                    assert (got[pad] == 0xA5).all(), ctx


@pytest.mark.parametrize("name", list(lr.RECORDS))
def test_device_values_with_a_host_partition(lib, name):
    """The offsets are a host prefix, the fields the struct plan's: a gather when any is strided."""
    rec = lr.RECORDS[name](67)
    ptr_of = fake_ptrs(rec)
    for lengths in lr.partitions(67):
        sample, info, ranges = lr.oracle(rec, lr.offsets_of(lengths))
        for what, part, form in forms(lengths):
            with lr.plan_list(rec, ptr_of, ARROW_DEVICE_ROCM, part, form, ARROW_DEVICE_CPU) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), what
                f = sr.plan_fields(p)
                assert [(d["off"], d["bytes"]) for d in f] == ranges
                assert all(d["gather"] for d in f) and p.segments() == []
                s = lr.plan_scan(p)
                assert not s["scan"] and s["prefix"] == 4 * (len(lengths) + 1)
    # N == 0: only the offsets travel, as a host plan
    for lengths in lr.partitions(0):
        rec0 = lr.RECORDS[name](0)
        sample, info, _ = lr.oracle(rec0, lr.offsets_of(lengths))
        with lr.plan_list(rec0, lambda b: PTR, ARROW_DEVICE_ROCM, np.array(lengths, np.int64),
                          PARTITION_LENGTHS, ARROW_DEVICE_CPU) as p:
            assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
            assert [(off, ln) for _, off, ln in p.segments()] == [(0, 4 * (len(lengths) + 1))]


def test_all_dense_device_values_with_a_host_partition_are_copy_segments(lib):
    a, b = lr.base(np.float32, (67, 4)), lr.base(np.uint8, (67,))
    rec = [("a", a, a), ("b", b, b)]
    ptr_of = fake_ptrs(rec)
    sample, info, ranges = lr.oracle(rec, [0, 60, 67])
    with lr.plan_list(rec, ptr_of, ARROW_DEVICE_ROCM, np.array([60, 7], np.int32),
                      PARTITION_LENGTHS, ARROW_DEVICE_CPU) as p:
        assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
        assert p.segments() == [(ptr_of(a), ranges[0][0], a.nbytes), (ptr_of(b), ranges[1][0], 67)]
        assert lr.plan_scan(p)["prefix"] == 12


@pytest.mark.parametrize("name", list(lr.RECORDS))
def test_device_partition_plans_a_scan(lib, name):
    """A partition in HBM is never read: the plan carries its words' address, width, form and
    reach, and one launch gathers every field, dense ones included.  The type info is the
    oracle's for any partition of that B (the offsets are not part of it)."""
    rec = lr.RECORDS[name](67)
    ptr_of = fake_ptrs(rec)
    pp = PTR + (64 << 20)
    for b in (0, 1, 5, 257):
        lengths = [0] * b
        if b:
            lengths[-1] = 67
        sample, info, ranges = lr.oracle(rec, lr.offsets_of(lengths))
        for dt in (np.int32, np.int64):
            for form, count in ((PARTITION_LENGTHS, b), (PARTITION_OFFSETS, b + 1)):
                part = np.zeros(count, dt)  # (the plan does not look at it: see part_ptr)
                with lr.plan_list(rec, ptr_of, ARROW_DEVICE_ROCM, part, form, ARROW_DEVICE_ROCM,
                                  part_ptr=pp) as p:
                    assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
                    assert p.segments() == []
                    f = sr.plan_fields(p)
                    assert [(d["off"], d["bytes"]) for d in f] == ranges and all(d["gather"] for d in f)
                    s = lr.plan_scan(p)
                    w = np.dtype(dt).itemsize
                    assert s == {"scan": True, "src": pp, "count": count, "wide": w == 8,
                                 "offsets": form == PARTITION_OFFSETS, "rows": 67, "lo": 0,
                                 "hi": count * w - 1, "prefix": 0}


def plan_raw(fields, part, form=PARTITION_LENGTHS, part_dev=ARROW_DEVICE_CPU, dev=ARROW_DEVICE_CPU,
             part_over=None, part_ptr=None, n=None):
    """fields: [(name bytes or None, shape, strides, dtype, overrides)] over PTR (never read: the
    refusals come first, or the fields are empty); `part` a numpy array or (shape, strides,
    dtype) over part_ptr."""
    tensors, keeps = [], []
    for _, shape, strides, dtype, over in fields:
        t, keep = tensor._describe(PTR, shape, strides, dtype)
        for k, v in over.items():
            setattr(t, k, v)
        tensors.append(t)
        keeps.append(keep)
    if isinstance(part, tuple):
        pt, pkeep = tensor._describe(part_ptr or PTR, *part)
    else:
        part = np.ascontiguousarray(part)
        pt, pkeep = tensor._describe(part.__array_interface__["data"][0] if part_ptr is None
                                     else part_ptr, part.shape, None, part.dtype)
    for k, v in (part_over or {}).items():
        setattr(pt, k, v)
    lst, keep = tensor._describe_list(None, tensors, pt, form, part_dev)
    for k, f in enumerate(fields):
        lst.fields[k].name = f[0]
    if n is not None:
        lst.n = n
    h = c_void_p()
    try:
        _lib.call("dora_gpu_plan_tensor_list", byref(lst), dev, byref(h))
    finally:
        if h.value:
            _lib.load().dora_gpu_plan_free(h)


def refused(*a, **kw):
    with pytest.raises(DoraGpuError) as e:
        plan_raw(*a, **kw)
    return e.value.code, str(e.value)


def test_host_partition_refusals_name_the_index(lib):
    v = [(None, (10, 2), None, np.float32, {})]
    ok = dict(dev=ARROW_DEVICE_ROCM)  # device values at PTR are not read either
    plan_raw(v, np.array([4, 6], np.int32), **ok)
    for dt in (np.int32, np.int64):
        code, msg = refused(v, np.array([4, -1, 7], dt), **ok)
        assert code == -1 and "length 1 is -1" in msg
        code, msg = refused(v, np.array([4, 7], dt), **ok)
        assert code == -1 and "lengths 0..1 sum past the 10 rows" in msg
        code, msg = refused(v, np.array([4, 5], dt), **ok)
        assert code == -1 and "sum to 9" in msg and "index 2" in msg
        code, msg = refused(v, np.array([1, 4, 10], dt), PARTITION_OFFSETS, **ok)
        assert code == -1 and "offset 0 is 1" in msg
        code, msg = refused(v, np.array([0, 6, 4, 10], dt), PARTITION_OFFSETS, **ok)
        assert code == -1 and "offset 2 is 4, below offset 1 (6)" in msg
        code, msg = refused(v, np.array([0, 4, 11], dt), PARTITION_OFFSETS, **ok)
        assert code == -1 and "offset 2 is 11, past the 10 rows" in msg
        code, msg = refused(v, np.array([0, 4, 9], dt), PARTITION_OFFSETS, **ok)
        assert code == -1 and "offset 2, the last, is 9" in msg
    # int64 words beyond 32 bits are refused by value, not truncated
    code, msg = refused(v, np.array([(1 << 32) + 10], np.int64), **ok)
    assert code == -1 and "length 0" in msg
    code, msg = refused(v, np.array([0, (1 << 32) + 10], np.int64), PARTITION_OFFSETS, **ok)
    assert code == -1 and "offset 1" in msg
    code, msg = refused(v, np.array([], np.int64), PARTITION_OFFSETS, **ok)
    assert code == -1 and "at least one" in msg
    # B == 0 with N > 0 does not describe the rows either
    code, msg = refused(v, np.array([], np.int64), **ok)
    assert code == -1 and "index 0" in msg


def test_partition_tensor_refusals(lib):
    v = [(None, (10, 2), None, np.float32, {})]
    for bad, word in [(((2,), None, np.float32), "int32 or int64"),
                      (((2,), None, np.uint32), "int32 or int64"),
                      (((2,), None, np.int16), "int32 or int64"),
                      (((2, 1), None, np.int32), "dimensions"),
                      (((4,), (2,), np.int32), "dense")]:
        code, msg = refused(v, bad)
        assert code == -1 and word in msg, (bad, msg)
    code, msg = refused(v, ((2,), None, np.int64), part_ptr=PTR + 4, part_dev=ARROW_DEVICE_ROCM,
                        dev=ARROW_DEVICE_ROCM)
    assert code == -1 and "aligned" in msg
    code, msg = refused(v, np.array([10], np.int32), form=2)
    assert code == -1 and "partition_form" in msg
    # a device partition with host values: refused, the message says what to pass instead
    for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
        code, msg = refused(v, ((2,), None, np.int32), part_dev=ARROW_DEVICE_ROCM, dev=dev)
        assert code == -1 and ".tolist()" in msg
    # one workgroup scans a device partition: at most 2^20 words; a host one may be longer
    big = ((1 << 20) + 1,)
    code, msg = refused(v, (big, None, np.int32), part_dev=ARROW_DEVICE_ROCM, dev=ARROW_DEVICE_ROCM)
    assert code == -4 and "one workgroup" in msg
    plan_raw(v, ((1 << 20,), None, np.int32), part_dev=ARROW_DEVICE_ROCM, dev=ARROW_DEVICE_ROCM)
    # no LargeList: B + 1 or N at 2^31 (an empty partition tensor of that extent is not read)
    code, msg = refused(v, ((1 << 31,), None, np.int32), PARTITION_OFFSETS, part_over={"data": PTR})
    assert code == -4 and "LargeList" in msg
    code, msg = refused(v, (((1 << 31) - 1,), None, np.int32), part_over={"data": PTR})
    assert code == -4 and "LargeList" in msg
    wide = [(None, (1 << 31,), None, np.uint8, {})]
    code, msg = refused(wide, np.array([1], np.int32), dev=ARROW_DEVICE_ROCM)
    assert code == -4 and "LargeList" in msg


def test_the_values_own_refusals_pass_through(lib):
    part = np.array([4], np.int32)
    # a bare tensor: the single tensor's message, unprefixed
    for bad, want in [((None, (4,), None, np.bool_, {}), -4),
                      ((None, (4, 0), None, np.uint8, {}), -1),
                      ((None, (4, 4), (1 << 62, 1), np.uint8, {}), -1)]:
        code, msg = refused([bad], part, dev=ARROW_DEVICE_ROCM)
        t, keep = tensor._describe(PTR, *bad[1:4])
        with pytest.raises(DoraGpuError) as e:
            _lib.call("dora_gpu_plan_tensor", byref(t), ARROW_DEVICE_ROCM, byref(c_void_p()))
        assert code == want and msg == str(e.value)
    # a record: the struct plan's refusals, prefix and all
    ok = (b"a", (4, 2), None, np.float32, {})
    code, msg = refused([ok, (b"m", (4,), None, np.bool_, {})], part, dev=ARROW_DEVICE_ROCM)
    assert code == -4 and "field 1 `m`: " in msg and "bool" in msg
    code, msg = refused([ok, (b"b", (5,), None, np.uint8, {})], part, dev=ARROW_DEVICE_ROCM)
    assert code == -1 and "field 1 `b`" in msg and "leading extent 5" in msg
    code, msg = refused([ok, (b"a", (4,), None, np.uint8, {})], part, dev=ARROW_DEVICE_ROCM)
    assert code == -1 and "field 1 `a`" in msg and "field 0" in msg
    code, msg = refused([ok, (None, (4,), None, np.uint8, {})], part, dev=ARROW_DEVICE_ROCM)
    assert code == -1 and "field 1" in msg and "NULL" in msg
    nine = [(b"f%d" % k, (4,), None, np.uint8, {}) for k in range(9)]
    assert refused(nine, part, dev=ARROW_DEVICE_ROCM)[0] == -4
    assert refused([ok], part, n=0)[0] == -1
