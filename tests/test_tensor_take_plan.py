"""Planning of take messages on the CPU (no GPU): dora_gpu_plan_tensor_take over real numpy memory
and over made-up device pointers (planning calls nothing in HIP and reads no device byte).  For a
bare tensor, a record and ragged batches over either, type info and size are the reference
packing's (oracle.pack_ref) of tensor.from_numpy_take(..), the message `values[index]` is today;
leaf offsets follow the struct and list plans' rule; a host plan's staged bytes are that packing;
a device plan carries no segment, its index is never read and dora_gpu_test_plan_take reports it;
every refusal carries its code and names the field or the index position."""
from ctypes import byref, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST,
                           PARTITION_LENGTHS, PARTITION_OFFSETS, DoraGpuError)
from oracle.pack_ref import pack, sample_regions
from tests import list_records as lr
from tests import struct_records as sr
from tests import take_records as tr

PTR = 0x7E00_0000_0000  # never dereferenced
N = 67
RECORDS = dict(lr.RECORDS, negative_and_broadcast=lambda n: sr.negative_and_broadcast())


def fake_ptrs(rec):
    bases = sr.bases_of(rec)
    return lambda b: PTR + (1 << 20) * next(i for i, x in enumerate(bases) if x is b)


def host_ptr(b):
    return b.__array_interface__["data"][0]


def message(rec, index, **part):
    """tensor.from_numpy_take of the record's views."""
    values = rec[0][2] if rec[0][0] is None else {name: v for name, _, v in rec}
    return tensor.from_numpy_take(values, index, **part)


def valid_indices(k, n):
    for wide in (0, 1):
        for label, index in tr.indices(k, n, wide)[:4]:
            yield f"{label} int{64 if wide else 32}", index


def staged(p):
    """What any host path does with a host plan's segments, into a poisoned sample."""
    got = np.full(p.size, 0xA5, np.uint8)
    for src, off, ln in p.segments():
        got[off:off + ln] = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * ln).from_address(src))
    return got.tobytes()


def test_from_numpy_take_is_the_message_of_the_indexed_copy():
    out = lr.base(np.float32, (10, 6))
    keep = np.array([7, 0, 7, 9])
    assert tensor.from_numpy_take(out[:, :4], keep).equals(tensor.from_numpy(out[keep, :4]))
    rec = {"bbox": out[:, :4], "conf": out[:, 4]}
    assert tensor.from_numpy_take(rec, keep).equals(
        tensor.from_numpy_struct({"bbox": out[keep, :4], "conf": out[keep, 4]}))
    assert tensor.from_numpy_take(rec, keep, lengths=[1, 3]).equals(
        tensor.from_numpy_ragged({"bbox": out[keep, :4], "conf": out[keep, 4]}, lengths=[1, 3]))
    assert len(tensor.from_numpy_take(out, [])) == 0
    for bad in ([-1], [10]):
        with pytest.raises(IndexError):
            tensor.from_numpy_take(out, bad)
    assert isinstance(tensor.take(out, keep), tensor.Taken) and "take" in tensor.__all__


@pytest.mark.parametrize("name", list(RECORDS))
def test_host_plans_stage_the_oracles_bytes(lib, name):
    rec = RECORDS[name](N)
    n = rec[0][2].shape[0]
    for k in (0, 1, 5, 70):
        for what, index in valid_indices(k, n):
            sample, info = pack(message(rec, index))
            for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
                ctx = f"{name} K={k} {what} dev={dev}"
                with tr.plan_take(rec, host_ptr, dev, index, ARROW_DEVICE_CPU) as p:
                    assert p.size == len(sample), ctx
                    assert p.type_info().to_json() == info.to_json(), ctx
                    ix = tr.plan_index(p)
                    assert (ix["device"], ix["k"], ix["n"]) == (False, k, n), ctx
                    assert [(off, ln) for _, off, ln in p.segments()] == \
                        ([] if k == 0 else tr.oracle(rec, index)[2]), ctx
                    assert sample_regions(staged(p), info) == sample_regions(sample, info), ctx
                    # always staged, dense fields and an identity index included: no segment
                    # reads the caller's memory
                    for src, _, ln in p.segments():
                        for _, b, _ in rec:
                            assert not (host_ptr(b) <= src < host_ptr(b) + max(b.nbytes, 1)), ctx
            # a ragged batch over the taken rows: lengths and offsets, int32 and int64
            lengths = [0, k // 3, k - k // 3, 0]
            offs = lr.offsets_of(lengths)
            sample, info = pack(message(rec, index, lengths=lengths))
            for part, form in ((np.array(lengths, np.int32), PARTITION_LENGTHS),
                               (offs.astype(np.int64), PARTITION_OFFSETS)):
                with tr.plan_take(rec, host_ptr, ARROW_DEVICE_CPU, index, ARROW_DEVICE_CPU,
                                  part=part, form=form) as p:
                    ctx = f"{name} K={k} {what} ragged form={form}"
                    assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), ctx
                    want = [(0, 20)] + ([] if k == 0 else tr.oracle(rec, index, offs)[2])
                    assert [(off, ln) for _, off, ln in p.segments()] == want, ctx
                    got = staged(p)
                    assert sample_regions(got, info) == sample_regions(sample, info), ctx
                    assert got[:20] == offs.astype(np.int32).tobytes(), ctx


@pytest.mark.parametrize("name", list(RECORDS))
def test_device_plans_are_one_launch_and_never_read(lib, name):
    """Type info and size are the oracle's, every field's bytes sit where the struct or list plan
    puts them, no segment whatever the fields are, and the index is reported, not read."""
    rec = RECORDS[name](N)
    n = rec[0][2].shape[0]
    ptr_of = fake_ptrs(rec)
    ip, pp = PTR + (64 << 20), PTR + (65 << 20)
    for k in (1, 5, 70):
        for wide in (0, 1):
            index = tr.indices(k, n, wide)[3][1]
            sample, info = pack(message(rec, index))
            with tr.plan_take(rec, ptr_of, ARROW_DEVICE_ROCM, np.zeros_like(index),
                              ARROW_DEVICE_ROCM, index_ptr=ip) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
                assert p.segments() == []
                f = sr.plan_fields(p)
                assert [(d["off"], d["bytes"]) for d in f] == tr.oracle(rec, index)[2]
                assert all(d["gather"] and d["kind"] == -1 for d in f)
                ix = tr.plan_index(p)
                assert ix["stride0"][:len(rec)] == [v.strides[0] for _, _, v in rec]
                del ix["stride0"]
                assert ix == {"device": True, "index": ip, "k": k, "n": n, "wide": bool(wide),
                              "lo": 0, "hi": index.nbytes - 1}
                # dimension 0 keeps its own entry; the reach covers all n source rows
                for (_, b, v), d in zip(rec, f):
                    off = d["src"] - ptr_of(b)
                    first = v.__array_interface__["data"][0] - host_ptr(b)
                    assert off == first and 0 <= off + d["lo"] and off + d["hi"] < b.nbytes
            lengths = [0, k // 3, k - k // 3, 0]
            offs = lr.offsets_of(lengths)
            sample, info = pack(message(rec, index, lengths=lengths))
            ranges = tr.oracle(rec, index, offs)[2]
            # a host partition: the offsets a prefix, still one launch and no segment
            with tr.plan_take(rec, ptr_of, ARROW_DEVICE_ROCM, np.zeros_like(index),
                              ARROW_DEVICE_ROCM, index_ptr=ip, part=np.array(lengths, np.int64)) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
                assert p.segments() == [] and tr.plan_index(p)["device"]
                assert [(d["off"], d["bytes"]) for d in sr.plan_fields(p)] == ranges
                s = lr.plan_scan(p)
                assert not s["scan"] and s["prefix"] == 20
            # a partition in HBM: the scan share in front, clamped to K
            with tr.plan_take(rec, ptr_of, ARROW_DEVICE_ROCM, np.zeros_like(index),
                              ARROW_DEVICE_ROCM, index_ptr=ip, part=np.zeros(5, np.int32),
                              form=PARTITION_OFFSETS, part_dev=ARROW_DEVICE_ROCM, part_ptr=pp) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
                assert p.segments() == [] and tr.plan_index(p)["device"]
                assert [(d["off"], d["bytes"]) for d in sr.plan_fields(p)] == ranges
                s = lr.plan_scan(p)
                assert (s["scan"], s["src"], s["count"], s["rows"], s["offsets"]) == (True, pp, 5, k, True)


def test_dimension_0_is_never_merged_or_dropped(lib):
    """Dense (n, 4) values merge into one row of 16 n bytes as a tensor; taken, dimension 0 stays:
    rows of 16 bytes, stride 16.  Extent 1 and stride 0 keep their entry too."""
    ip = PTR + (64 << 20)
    index = np.zeros(3, np.int32)
    for b, v, row, stride0 in [(lr.base(np.float32, (9, 4)),) * 2 + (16, 16),
                               (lr.base(np.float32, (1, 4)),) * 2 + (16, 16),
                               (lr.base(np.float32, (1, 4)), None, 16, 0),
                               (lr.base(np.uint8, (9,)),) * 2 + (1, 1)]:
        if v is None:
            v = np.broadcast_to(b, (9, 4))
        with tr.plan_take([(None, b, v)], lambda _: PTR, ARROW_DEVICE_ROCM, index,
                          ARROW_DEVICE_ROCM, index_ptr=ip) as p:
            (d,) = sr.plan_fields(p)
            assert (d["nd"], d["row"], d["bytes"]) == (0, row, 3 * row)
            assert tr.plan_index(p)["stride0"][0] == stride0
            assert (d["lo"], d["hi"]) == (0, (v.shape[0] - 1) * stride0 + row - 1)
    # eight dimensions after dimension 0 are the most; nine are DORA_ERR_UNSUPPORTED
    for inner, ok in ((8, True), (9, False)):
        shape = (4,) + (2,) * inner
        strides = [1 << (2 * inner)] + [1 << (2 * i + 1) for i in range(inner)][::-1]
        t, keep = tensor._describe(PTR, shape, strides, np.uint8)
        it, ikeep = tensor._describe(ip, (3,), None, np.int32)
        tk, keep2 = tensor._describe_take(None, [t], it, ARROW_DEVICE_ROCM, None, 0, ARROW_DEVICE_CPU)
        h = c_void_p()
        if ok:
            _lib.call("dora_gpu_plan_tensor_take", byref(tk), ARROW_DEVICE_ROCM, byref(h))
            _lib.load().dora_gpu_plan_free(h)
        else:
            with pytest.raises(DoraGpuError) as e:
                _lib.call("dora_gpu_plan_tensor_take", byref(tk), ARROW_DEVICE_ROCM, byref(h))
            assert e.value.code == -4 and "more than 8 dimensions" in str(e.value)


def test_empty_and_sourceless_takes(lib):
    out = lr.base(np.float32, (10, 6))
    rec = [("bbox", out, out[:, :4]), ("conf", out, out[:, 4])]
    ip = PTR + (64 << 20)
    for dev, idev, ptr_of in ((ARROW_DEVICE_CPU, ARROW_DEVICE_CPU, host_ptr),
                              (ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM, lambda b: PTR)):
        # K == 0: an empty message; a NULL index is then fine
        sample, info = pack(message(rec, []))
        with tr.plan_take(rec, ptr_of, dev, np.zeros(0, np.int64), idev, index_ptr=0) as p:
            assert p.size == len(sample) == 0 and p.type_info().to_json() == info.to_json()
            assert p.segments() == [] and tr.plan_index(p)["k"] == 0
    # N == 0 with K > 0 on the device: K zero rows, `data` may be NULL
    none = np.zeros((0, 6), np.float32)
    sample, info = pack(tensor.from_numpy(np.zeros((3, 4), np.float32)))
    with tr.plan_take([(None, none, none[:, :4])], lambda b: 0, ARROW_DEVICE_ROCM,
                      np.zeros(3, np.int32), ARROW_DEVICE_ROCM, index_ptr=ip) as p:
        assert p.size == len(sample) == 48 and p.type_info().to_json() == info.to_json()
        ix = tr.plan_index(p)
        assert (ix["device"], ix["k"], ix["n"]) == (True, 3, 0)
    # on the host every word is then invalid
    with pytest.raises(DoraGpuError) as e:
        tr.plan_take([(None, none, none[:, :4])], host_ptr, ARROW_DEVICE_CPU, np.zeros(3, np.int32),
                     ARROW_DEVICE_CPU)
    assert e.value.code == -1 and "word 0 is 0" in str(e.value)


def plan_raw(fields, index, index_dev=ARROW_DEVICE_CPU, dev=ARROW_DEVICE_CPU, index_ptr=None,
             index_over=None, part=None, form=PARTITION_LENGTHS, part_dev=ARROW_DEVICE_CPU, n=None,
             values_ptr=PTR):
    """fields: [(name bytes or None, shape, strides, dtype)] over `values_ptr` (PTR is never
    read: the refusals come first, or the plan is a device plan); `index` / `part` a numpy array
    or (shape, strides, dtype) over a pointer."""
    def words(w, ptr):
        if isinstance(w, tuple):
            return tensor._describe(ptr or PTR, *w)
        w = np.ascontiguousarray(w)
        t, keep = tensor._describe(w.__array_interface__["data"][0] if ptr is None else ptr,
                                   w.shape, None, w.dtype)
        return t, (keep, w)
    tensors, keeps = [], []
    for _, shape, strides, dtype in fields:
        t, keep = tensor._describe(values_ptr, shape, strides, dtype)
        tensors.append(t)
        keeps.append(keep)
    it, ikeep = words(index, index_ptr)
    for k, v in (index_over or {}).items():
        setattr(it, k, v)
    pt, pkeep = words(part, None) if part is not None else (None, None)
    tk, keep = tensor._describe_take(None, tensors, it, index_dev, pt, form, part_dev)
    for k, f in enumerate(fields):
        tk.fields[k].name = f[0]
    if n is not None:
        tk.n = n
    h = c_void_p()
    try:
        _lib.call("dora_gpu_plan_tensor_take", byref(tk), dev, byref(h))
    finally:
        if h.value:
            _lib.load().dora_gpu_plan_free(h)


def refused(*a, **kw):
    with pytest.raises(DoraGpuError) as e:
        plan_raw(*a, **kw)
    return e.value.code, str(e.value)


V = [(None, (10, 2), None, np.float32)]
ON_DEVICE = dict(index_dev=ARROW_DEVICE_ROCM, dev=ARROW_DEVICE_ROCM)


def test_the_index_lives_where_the_values_live(lib):
    idx = ((3,), None, np.int32)
    plan_raw(V, idx, **ON_DEVICE)
    for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
        code, msg = refused(V, idx, index_dev=ARROW_DEVICE_ROCM, dev=dev)
        assert code == -1 and "move the index next to the values" in msg
    for idev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
        code, msg = refused(V, np.array([1], np.int32), index_dev=idev, dev=ARROW_DEVICE_ROCM)
        assert code == -1 and "move the index next to the values" in msg
    assert refused(V, idx, index_dev=7)[0] == -1


def test_index_tensor_refusals(lib):
    for bad, word in [(((2,), None, np.float32), "int32 or int64"),
                      (((2,), None, np.uint32), "int32 or int64"),
                      (((2,), None, np.int16), "int32 or int64"),
                      (((2, 1), None, np.int32), "dimensions"),
                      (((4,), (2,), np.int32), "dense")]:
        for where in ({}, ON_DEVICE):
            code, msg = refused(V, bad, **where)
            assert code == -1 and word in msg and "] index " in msg, (bad, msg)
    code, msg = refused(V, ((2,), None, np.int32), index_over={"dtype_lanes": 2}, **ON_DEVICE)
    assert code == -1 and "lanes" in msg
    # a device index is read by a kernel: aligned to its words; a host one may sit anywhere
    for dt, step in ((np.int64, 4), (np.int32, 2)):
        code, msg = refused(V, ((2,), None, dt), index_ptr=PTR + step, **ON_DEVICE)
        assert code == -1 and "aligned" in msg
    raw = np.zeros(13, np.uint8)
    raw[1:9] = np.frombuffer(np.array([3, 9], np.int32).tobytes(), np.uint8)
    plan_raw([(None, (10, 2), None, np.uint8)], ((2,), None, np.int32),
             index_ptr=raw.__array_interface__["data"][0] + 1, values_ptr=host_ptr(np.zeros(20, np.uint8)))
    # NULL with K > 0
    for where in ({}, ON_DEVICE):
        code, msg = refused(V, ((2,), None, np.int32), index_over={"data": None}, **where)
        assert code == -1 and "index data is NULL" in msg


def test_a_host_index_is_checked_word_by_word(lib):
    for dt in (np.int32, np.int64):
        code, msg = refused(V, np.array([0, 9, -1, 10], dt))
        assert code == -1 and "word 2 is -1" in msg and "10 rows" in msg
        code, msg = refused(V, np.array([0, 10, -1], dt))
        assert code == -1 and "word 1 is 10" in msg
    code, msg = refused(V, np.array([(1 << 32) + 1], np.int64))
    assert code == -1 and f"word 0 is {(1 << 32) + 1}" in msg
    # the record's refusal names the position all the same
    rec = [(b"a", (10, 2), None, np.float32), (b"b", (10,), None, np.uint8)]
    code, msg = refused(rec, np.array([10], np.int32))
    assert code == -1 and "word 0 is 10" in msg


def test_the_partition_describes_the_taken_rows(lib):
    index = np.array([9, 9, 0, 3, 3], np.int32)
    vals = [(None, (10, 2), None, np.float32)]
    for part, form, word in [(np.array([2, 2], np.int32), PARTITION_LENGTHS, "sum to 4"),
                             (np.array([2, 4], np.int32), PARTITION_LENGTHS, "sum past the 5 rows"),
                             (np.array([0, 2, 10], np.int64), PARTITION_OFFSETS, "past the 5 rows"),
                             (np.array([0, 2, 4], np.int64), PARTITION_OFFSETS, "the last, is 4")]:
        code, msg = refused(vals, ((5,), None, np.int32), part=part, form=form, **ON_DEVICE)
        assert code == -1 and word in msg, msg
    # a partition of the N source rows is not one of the K taken rows
    code, msg = refused(vals, ((5,), None, np.int32), part=np.array([10], np.int32), **ON_DEVICE)
    assert code == -1 and "5 rows" in msg
    # a device partition needs device values, as in the list plan
    code, msg = refused(vals, index, part=((2,), None, np.int32), part_dev=ARROW_DEVICE_ROCM)
    assert code == -1 and ".tolist()" in msg
    # no LargeList: K or B + 1 at 2^31 (neither tensor is read)
    code, msg = refused([(None, (10,), None, np.uint8)], ((1 << 31,), None, np.int32),
                        part=np.array([1], np.int32), **ON_DEVICE)
    assert code == -4 and "LargeList" in msg
    code, msg = refused(vals, ((5,), None, np.int32), part=(((1 << 31) - 1,), None, np.int32),
                        **ON_DEVICE)
    assert code == -4 and "LargeList" in msg


def test_the_values_own_refusals_pass_through(lib):
    idx = ((3,), None, np.int32)
    for bad, want, word in [((None, (4,), None, np.bool_), -4, "bool"),
                            ((None, (4, 0), None, np.uint8), -1, "extent 0 in dimension 1"),
                            ((None, (4, 4), (1 << 62, 1), np.uint8), -1, "reach overflows"),
                            ((None, (4, 4), (1 << 62, 1), np.float64), -1, "stride 0 overflows")]:
        code, msg = refused([bad], idx, **ON_DEVICE)
        assert code == want and word in msg, msg
    ok = (b"a", (4, 2), None, np.float32)
    code, msg = refused([ok, (b"m", (4,), None, np.bool_)], idx, **ON_DEVICE)
    assert code == -4 and "field 1 `m`: " in msg and "bool" in msg
    code, msg = refused([ok, (b"b", (5,), None, np.uint8)], idx, **ON_DEVICE)
    assert code == -1 and "field 1 `b`" in msg and "leading extent 5" in msg
    code, msg = refused([ok, (b"a", (4,), None, np.uint8)], idx, **ON_DEVICE)
    assert code == -1 and "field 1 `a`" in msg and "field 0" in msg
    nine = [(b"f%d" % k, (4,), None, np.uint8) for k in range(9)]
    assert refused(nine, idx, **ON_DEVICE)[0] == -4
    assert refused([ok], idx, n=0, **ON_DEVICE)[0] == -1
    # any other plan is not a take
    t, keep = tensor._describe(PTR, (4, 2), None, np.float32)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor", byref(t), ARROW_DEVICE_ROCM, byref(h))
    with pytest.raises(DoraGpuError):
        _lib.call("dora_gpu_test_plan_take", h, None, None, None, None, None, None, None, None)
    _lib.load().dora_gpu_plan_free(h)
