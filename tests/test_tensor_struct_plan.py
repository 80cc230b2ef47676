"""Planning of struct-of-tensors messages on the CPU (no GPU): dora_gpu_plan_tensor_struct over
made-up device pointers (planning calls nothing in HIP and reads no tensor byte) and over real
numpy memory.  Size, type info and per-field offsets are the reference packing's of
pa.StructArray.from_arrays([tensor.from_numpy(v) ..], names) (oracle.pack_ref); all-dense device
fields plan n copy segments, one strided field makes the plan a multi-gather of every field; a
host plan's packed regions equal the oracle's; d0 == 0, n == 1 and every refusal."""
from ctypes import byref, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST,
                           DoraGpuError)
from oracle.pack_ref import sample_regions
from tests import struct_records as sr
from tests.gather_views import base

PTR = 0x7E00_0000_0000  # never dereferenced


def fake_ptrs(rec):
    """A made-up device address per base, 1 MiB apart."""
    bases = sr.bases_of(rec)
    return lambda b: PTR + (1 << 20) * next(i for i, x in enumerate(bases) if x is b)


def host_ptr(b):
    return b.__array_interface__["data"][0]


def test_the_issues_layout_table():
    """The figures the feature was specified with, from the oracle alone."""
    sample, info, ranges = sr.oracle(sr.detector(5))
    assert ranges == [(0, 80), (80, 10), (96, 40), (136, 15)] and len(sample) == 151
    assert info.data_type == "+s[bbox:?+w:4[item:?f],conf:?e,label:?l,rgb:?+w:3[item:?C]]"


@pytest.mark.parametrize("n", [5, 67])
def test_device_record_matches_the_oracle(lib, n):
    rec = sr.detector(n)
    sample, info, ranges = sr.oracle(rec)
    ptr_of = fake_ptrs(rec)
    with sr.plan_record(rec, ptr_of, ARROW_DEVICE_ROCM) as p:
        assert p.size == len(sample)
        assert p.type_info().to_json() == info.to_json()
        f = sr.plan_fields(p)
        assert [(d["off"], d["bytes"]) for d in f] == ranges
        # one strided field makes the whole plan a multi-gather: no segments, every field a view
        assert all(d["gather"] for d in f) and p.segments() == []
        out, lab, img = rec[0][1], rec[2][1], rec[3][1]
        bbox, conf, label, rgb = f
        assert (bbox["src"], bbox["elem"], bbox["row"], bbox["shape"], bbox["stride"]) == \
            (ptr_of(out), 4, 16, [n], [24])
        assert (bbox["lo"], bbox["hi"]) == (0, (n - 1) * 24 + 15)
        assert (conf["src"], conf["elem"], conf["row"], conf["shape"], conf["stride"]) == \
            (ptr_of(out) + 16, 2, 2, [n], [24])
        assert (conf["lo"], conf["hi"]) == (0, (n - 1) * 24 + 1)
        # the dense field is a view with nd == 0: one row of all its bytes
        assert (label["src"], label["nd"], label["row"], label["lo"], label["hi"]) == \
            (ptr_of(lab), 0, 8 * n, 0, 8 * n - 1)
        assert (rgb["src"], rgb["elem"], rgb["row"], rgb["shape"], rgb["stride"]) == \
            (ptr_of(img), 1, 3, [n], [4])
        # every interval is exactly what the view reaches inside its base
        for (_, b, v), d in zip(rec, f):
            off = host_ptr(v) - host_ptr(b)
            assert off + d["lo"] >= 0 and off + d["hi"] < b.nbytes


@pytest.mark.parametrize("n", [5, 67])
def test_all_dense_device_fields_are_copy_segments(lib, n):
    a, b, c = base(np.float32, (n, 4)), base(np.float16, (n,)), base(np.uint8, (n + 2, 3))
    rec = [("a", a, a), ("b", b, b), ("c", c, c[1:n + 1])]
    sample, info, ranges = sr.oracle(rec)
    ptr_of = fake_ptrs(rec)
    with sr.plan_record(rec, ptr_of, ARROW_DEVICE_ROCM) as p:
        assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
        assert p.segments() == [(ptr_of(a), ranges[0][0], a.nbytes), (ptr_of(b), ranges[1][0], b.nbytes),
                                (ptr_of(c) + 3, ranges[2][0], 3 * n)]
        f = sr.plan_fields(p)  # kept for the per-field allocation check
        assert len(f) == 3 and not any(d["gather"] for d in f) and all(d["nd"] == 0 for d in f)


@pytest.mark.parametrize("dev", [ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST])
@pytest.mark.parametrize("n", [5, 67])
def test_host_record_packs_the_oracles_regions(lib, n, dev):
    rec = sr.detector(n)
    sample, info, ranges = sr.oracle(rec)
    with sr.plan_record(rec, host_ptr, dev) as p:
        assert p.size == len(sample)
        assert p.type_info().to_json() == info.to_json()
        segs = p.segments()
        assert [(off, ln) for _, off, ln in segs] == ranges
        # a dense pageable field is read in place, the others from the plan's staging buffer
        lab = rec[2][1]
        assert (segs[2][0] == host_ptr(lab)) == (dev == ARROW_DEVICE_CPU)
        assert all(s[0] not in (host_ptr(b) for _, b, _ in rec) for k, s in enumerate(segs) if k != 2)
        # what any host path does with the segments, into a poisoned sample: regions only
        got = np.full(p.size, 0xA5, np.uint8)
        for src, off, ln in segs:
            got[off:off + ln] = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * ln).from_address(src))
        assert sample_regions(got.tobytes(), info) == sample_regions(sample, info)
        pad = np.ones(p.size, bool)
        for off, ln in ranges:
            pad[off:off + ln] = False
        assert (got[pad] == 0xA5).all()
        with pytest.raises(DoraGpuError):  # a host plan is an ordinary multi-segment plan
            sr.plan_fields(p)


def test_empty_record(lib):
    a, b = np.zeros((0, 4), np.float32), np.zeros((0,), np.int64)
    rec = [("a", a, a), ("b", b, b)]
    sample, info, ranges = sr.oracle(rec)
    assert len(sample) == 0 and ranges == [(0, 0), (0, 0)]
    for dev, ptr_of in [(ARROW_DEVICE_ROCM, lambda b: PTR), (ARROW_DEVICE_ROCM, lambda b: None),
                        (ARROW_DEVICE_CPU, lambda b: None)]:
        with sr.plan_record(rec, ptr_of, dev) as p:
            assert p.size == 0 and p.segments() == []
            assert p.type_info().to_json() == info.to_json()


@pytest.mark.parametrize("dev", [ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM])
def test_one_field(lib, dev):
    b = base(np.int16, (7, 5))
    for v in (b, b[:, 1:4]):
        rec = [("only", b, v)]
        sample, info, ranges = sr.oracle(rec)
        ptr_of = host_ptr if dev == ARROW_DEVICE_CPU else fake_ptrs(rec)
        with sr.plan_record(rec, ptr_of, dev) as p:
            assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
            if dev == ARROW_DEVICE_ROCM:
                assert sr.plan_fields(p)[0]["gather"] == (v is not b)
                assert len(p.segments()) == (1 if v is b else 0)
            else:
                assert [(off, ln) for _, off, ln in p.segments()] == ranges


def plan_raw(fields, dev=ARROW_DEVICE_ROCM, n=None):
    """fields: [(name bytes or None, shape, strides, dtype, overrides)] over PTR."""
    tensors, keeps = [], []
    for _, shape, strides, dtype, over in fields:
        t, keep = tensor._describe(PTR, shape, strides, dtype)
        for k, v in over.items():
            setattr(t, k, v)
        tensors.append(t)
        keeps.append(keep)
    arr = (_lib.TensorField * max(len(fields), 1))()
    for k, (f, t) in enumerate(zip(fields, tensors)):
        arr[k].name = f[0]
        arr[k].tensor = t
    h = c_void_p()
    try:
        _lib.call("dora_gpu_plan_tensor_struct", arr, len(fields) if n is None else n, dev, byref(h))
    finally:
        if h.value:
            _lib.load().dora_gpu_plan_free(h)


def refused(fields, **kw):
    with pytest.raises(DoraGpuError) as e:
        plan_raw(fields, **kw)
    return e.value.code, str(e.value)


def test_refusals_name_the_field(lib):
    ok = (b"a", (4, 2), None, np.float32, {})
    plan_raw([ok])
    assert refused([ok], n=0)[0] == -1
    code, msg = refused([ok, (None, (4,), None, np.uint8, {})])
    assert code == -1 and "field 1" in msg and "NULL" in msg
    code, msg = refused([ok, (b"", (4,), None, np.uint8, {})])
    assert code == -1 and "field 1" in msg and "empty" in msg
    code, msg = refused([ok, (b"b", (4,), None, np.uint8, {}), (b"a", (4,), None, np.uint8, {})])
    assert code == -1 and "field 2 `a`" in msg and "field 0" in msg
    code, msg = refused([ok, (b"b", (5,), None, np.uint8, {})])
    assert code == -1 and "field 1 `b`" in msg and "leading extent 5" in msg
    # each field fits 63 bits, the two together do not
    code, msg = refused([(b"x", (1 << 62,), None, np.uint8, {}), (b"y", (1 << 62,), None, np.uint8, {})])
    assert code == -1 and "field 1 `y`" in msg and "overflows" in msg
    nine = [(b"f%d" % k, (4,), None, np.uint8, {}) for k in range(9)]
    assert refused(nine)[0] == -4
    plan_raw(nine[:8])
    # a tensor's own refusals pass through under the field's name, with the tensor's own code
    for bad, want in [((b"m", (4,), None, np.bool_, {}), -4),
                      ((b"m", (4,), None, np.uint8, {"dtype_lanes": 2}), -4),
                      ((b"m", (4, 0), None, np.uint8, {}), -1),
                      ((b"m", (4, 4), (1 << 62, 1), np.uint8, {}), -1),
                      ((b"m", (4,), None, np.uint8, {"data": None}), -1)]:
        code, msg = refused([ok, bad])
        assert code == want and "field 1 `m`: " in msg, (bad, msg)
        # the message behind the prefix is the single tensor's
        t, keep = tensor._describe(PTR, *bad[1:4])
        for k, v in bad[4].items():
            setattr(t, k, v)
        with pytest.raises(DoraGpuError) as e:
            _lib.call("dora_gpu_plan_tensor", byref(t), ARROW_DEVICE_ROCM, byref(c_void_p()))
        assert msg.split("field 1 `m`: ", 1)[1] == str(e.value).split("] ", 1)[1]
