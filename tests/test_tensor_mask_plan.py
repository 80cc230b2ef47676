"""Planning of mask messages on the CPU (no GPU): dora_gpu_plan_tensor_mask over real numpy memory
and over made-up device pointers (planning calls nothing in HIP and reads no device byte).  For a
bare tensor and for the records of tests/list_records.py, sizes, type info and leaf ranges are the
reference packing's (oracle.pack_ref) of tensor.from_numpy_masked(..): the List whose child keeps
its N rows, the K selected ones in front, under offsets C[p].  A host plan's staged bytes are that
packing; a device plan carries no segment, its mask is never read, and dora_gpu_test_plan_mask
reports mask, reach and workspace; every refusal carries its code and says what it refuses."""
from ctypes import byref, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST,
                           PARTITION_LENGTHS, PARTITION_OFFSETS, DoraGpuError)
from oracle.pack_ref import pack, sample_regions
from tests import list_records as lr
from tests import mask_records as mr
from tests import struct_records as sr

PTR = 0x7E00_0000_0000  # never dereferenced
N = 67


def xyi(n):
    """Two float32 columns of one (n, 3) base and a dense uint8: 12 + 268 + 268 + 67 = 615 bytes
    at n = 67 under three offsets."""
    p, i = lr.base(np.float32, (n, 3)), lr.base(np.uint8, (n,))
    return [("x", p, p[:, 0]), ("y", p, p[:, 1]), ("intensity", i, i)]


RECORDS = dict(lr.RECORDS, xyi=xyi)


def fake_ptrs(rec):
    bases = sr.bases_of(rec)
    return lambda b: PTR + (1 << 20) * next(i for i, x in enumerate(bases) if x is b)


def host_ptr(b):
    return b.__array_interface__["data"][0]


def message(rec, mask, **part):
    return tensor.from_numpy_masked(mr.values_of(rec), mask, **part)


def staged(p):
    """What any host path does with a host plan's segments, into a poisoned sample."""
    got = np.full(p.size, 0xA5, np.uint8)
    for src, off, ln in p.segments():
        got[off:off + ln] = np.ctypeslib.as_array((np.ctypeslib.ctypes.c_uint8 * ln).from_address(src))
    return got.tobytes()


def test_from_numpy_masked_is_the_capacity_list():
    out = lr.base(np.float32, (10, 6))
    keep = np.array([0, 1, 1, 0, 0, 0, 1, 0, 0, 1], np.bool_)
    arr = tensor.from_numpy_masked(out[:, :4], keep)
    arr.validate(full=True)
    pad = np.zeros((10, 4), np.float32)
    pad[:4] = out[keep, :4]
    assert arr.offsets.to_pylist() == [0, 4] and arr.values.equals(tensor.from_numpy(pad))
    rec = {"bbox": out[:, :4], "conf": out[:, 4]}
    arr = tensor.from_numpy_masked(rec, keep.astype(np.uint8) * 0x80, lengths=[3, 0, 7])
    arr.validate(full=True)
    assert arr.offsets.to_pylist() == [0, 2, 2, 4] and len(arr.values) == 10
    conf = np.zeros(10, np.float32)
    conf[:4] = out[keep, 4]
    assert arr.values.equals(tensor.from_numpy_struct({"bbox": pad, "conf": conf}))
    # the selected rows are what unbind() cuts at the offsets
    assert tensor.to_numpy(arr.values)["conf"][:4].tolist() == out[keep, 4].tolist()
    empty = tensor.from_numpy_masked(out[:0], np.zeros(0, np.bool_))
    assert empty.offsets.to_pylist() == [0, 0] and len(empty.values) == 0
    with pytest.raises(ValueError):
        tensor.from_numpy_masked(out, keep[:9])
    with pytest.raises(TypeError):
        tensor.from_numpy_masked(out, keep.astype(np.int32))
    with pytest.raises(ValueError):
        tensor.from_numpy_masked(out, keep, lengths=[4])  # the partition describes the N source rows
    assert isinstance(tensor.masked(out, keep), tensor.Masked) and "masked" in tensor.__all__


def test_the_python_builders_refuse_what_is_not_offered():
    out = lr.base(np.float32, (10, 6))
    keep = np.ones(10, np.bool_)
    m = tensor.masked(out, keep)
    assert isinstance(tensor.ragged(m, lengths=[10]).values, tensor.Masked)
    for inner in (tensor.take(out, [1]), m, tensor.ragged(out, lengths=[10]),
                  tensor.cast(out, "float16"), {"a": tensor.cast(out, "float16")}):
        with pytest.raises(TypeError):
            tensor.masked(inner, keep)
    with pytest.raises(TypeError):
        tensor.take(m, [1])
    with pytest.raises(TypeError):
        tensor.cast(m, "float16")


def test_the_67_row_case(lib):
    """615 bytes, offsets [0, 13, 29]: the same layout and type info as the full ragged batch."""
    rec, mask = xyi(67), mr.the_67_row_mask()
    arr = message(rec, mask, offsets=[0, 31, 67])
    arr.validate(full=True)
    assert arr.offsets.to_pylist() == [0, 13, 29] and len(arr.values) == 67
    sample, info = pack(arr)
    full, full_info = pack(tensor.from_numpy_ragged(mr.values_of(rec), offsets=[0, 31, 67]))
    assert len(sample) == len(full) == 615 and info.to_json() == full_info.to_json()
    part = np.array([0, 31, 67], np.int32)
    with mr.plan_mask(rec, host_ptr, ARROW_DEVICE_CPU, mask, ARROW_DEVICE_CPU, part=part,
                      form=PARTITION_OFFSETS, part_dev=ARROW_DEVICE_CPU) as p:
        assert p.size == 615 and p.type_info().to_json() == info.to_json()
        assert sample_regions(staged(p), info) == sample_regions(sample, info)
        assert staged(p)[:12] == np.array([0, 13, 29], np.int32).tobytes()
    with mr.plan_mask(rec, fake_ptrs(rec), ARROW_DEVICE_ROCM, mask, ARROW_DEVICE_ROCM,
                      mask_ptr=PTR + (64 << 20) + 3, part=part, form=PARTITION_OFFSETS,
                      part_dev=ARROW_DEVICE_CPU) as p:
        assert p.size == 615 and p.type_info().to_json() == info.to_json()
        assert p.segments() == []


@pytest.mark.parametrize("name", list(RECORDS))
def test_host_plans_stage_the_oracles_bytes(lib, name):
    rec = RECORDS[name](N)
    for label, mask in mr.masks(N):
        for as_bool in (False, True):
            m = mask.astype(np.bool_) if as_bool and mask.max(initial=0) <= 1 else mask
            sample, info = pack(message(rec, m))
            for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
                ctx = f"{name} {label} {m.dtype} dev={dev}"
                with mr.plan_mask(rec, host_ptr, dev, m, ARROW_DEVICE_CPU) as p:
                    assert p.size == len(sample), ctx
                    assert p.type_info().to_json() == info.to_json(), ctx
                    got = mr.plan_info(p)
                    assert (got["device"], got["n"], mr.workspace_size(p)) == (False, N, 0), ctx
                    assert [(off, ln) for _, off, ln in p.segments()] == \
                        [(0, 8)] + mr.oracle(rec, m)[2], ctx
                    assert sample_regions(staged(p), info) == sample_regions(sample, info), ctx
                    assert staged(p)[:8] == np.array([0, int((m != 0).sum())], np.int32).tobytes()
                    # always staged: no segment reads the caller's memory
                    for src, _, ln in p.segments():
                        for _, b, _ in rec:
                            assert not (host_ptr(b) <= src < host_ptr(b) + max(b.nbytes, 1)), ctx
        for lengths in lr.partitions(N):
            offs = lr.offsets_of(lengths)
            sample, info = pack(message(rec, mask, lengths=lengths))
            for part, form in ((np.array(lengths, np.int32), PARTITION_LENGTHS),
                               (offs.astype(np.int64), PARTITION_OFFSETS)):
                with mr.plan_mask(rec, host_ptr, ARROW_DEVICE_CPU, mask, ARROW_DEVICE_CPU,
                                  part=part, form=form) as p:
                    ctx = f"{name} {label} B={len(lengths)} form={form}"
                    assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), ctx
                    got = staged(p)
                    assert sample_regions(got, info) == sample_regions(sample, info), ctx
                    assert got[:4 * len(offs)] == mr.counts(mask)[offs].tobytes(), ctx
    # an unaligned mask (mask[3:] is dense) and no rows at all
    rec3 = RECORDS[name](N + 3)
    cut = [(nm, b, v[3:]) for nm, b, v in rec3]
    mask = mr.masks(N + 3)[3][1]
    sample, info = pack(message(cut, mask[3:]))
    with mr.plan_mask(cut, host_ptr, ARROW_DEVICE_CPU, mask,
                      ARROW_DEVICE_CPU, mask_ptr=host_ptr(mask) + 3,
                      mask_desc=((N,), None, np.uint8)) as p:
        assert sample_regions(staged(p), info) == sample_regions(sample, info)
    rec0 = RECORDS[name](0)
    for lengths in [None] + lr.partitions(0):
        part = {} if lengths is None else {"lengths": lengths}
        sample, info = pack(message(rec0, np.zeros(0, np.uint8), **part))
        kw = {} if lengths is None else {"part": np.array(lengths, np.int64), "form": PARTITION_LENGTHS}
        with mr.plan_mask(rec0, host_ptr, ARROW_DEVICE_CPU, np.zeros(0, np.uint8),
                          ARROW_DEVICE_CPU, **kw) as p:
            assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
            assert sample_regions(staged(p), info) == sample_regions(sample, info)
            b = 1 if lengths is None else len(lengths)
            assert staged(p)[:4 * (b + 1)] == bytes(4 * (b + 1))


@pytest.mark.parametrize("name", list(RECORDS))
def test_device_plans_have_no_segments_and_never_read(lib, name):
    """Type info and size are the oracle's, every field's bytes sit where the list plan puts them,
    no segment whatever the fields are, and mask, reach and workspace are reported, not read."""
    rec = RECORDS[name](N)
    ptr_of = fake_ptrs(rec)
    mp, pp = PTR + (64 << 20), PTR + (65 << 20)
    mask = mr.masks(N)[3][1]
    for shift in mr.SHIFTS:
        sample, info = pack(message(rec, mask))
        with mr.plan_mask(rec, ptr_of, ARROW_DEVICE_ROCM, np.zeros_like(mask), ARROW_DEVICE_ROCM,
                          mask_ptr=mp + shift) as p:
            assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
            assert p.segments() == []
            f = sr.plan_fields(p)
            assert [(d["off"], d["bytes"]) for d in f] == mr.oracle(rec, mask)[2]
            assert all(d["gather"] and d["kind"] == -1 for d in f)
            got = mr.plan_info(p)
            assert got["stride0"][:len(rec)] == [v.strides[0] for _, _, v in rec]
            first = (p.size + 3) & ~3
            tiles = 1  # ceil((N + 15) / 4096)
            assert {k: got[k] for k in ("device", "mask", "n", "lo", "hi", "part_words")} == \
                {"device": True, "mask": mp + shift, "n": N, "lo": 0, "hi": N - 1, "part_words": 0}
            assert (got["index"], got["counts"], got["totals"], got["part"], got["end"]) == \
                (first, first + 4 * N, first + 4 * (2 * N + 1), first + 4 * (2 * N + 1 + tiles),
                 first + 4 * (2 * N + 1 + tiles))
            assert mr.workspace_size(p) == got["end"] - p.size
            # dimension 0 keeps its own entry; the reach covers all N source rows
            for (_, b, v), d in zip(rec, f):
                off = d["src"] - ptr_of(b)
                assert off == host_ptr(v) - host_ptr(b)
                assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes
    lengths = lr.partitions(N)[4]
    offs = lr.offsets_of(lengths)
    sample, info = pack(message(rec, mask, lengths=lengths))
    # a host partition: checked, and its B + 1 offsets travel into the workspace as the prefix
    with mr.plan_mask(rec, ptr_of, ARROW_DEVICE_ROCM, np.zeros_like(mask), ARROW_DEVICE_ROCM,
                      mask_ptr=mp, part=np.array(lengths, np.int32), form=PARTITION_LENGTHS,
                      part_dev=ARROW_DEVICE_CPU) as p:
        assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
        assert p.segments() == []
        got, sc = mr.plan_info(p), lr.plan_scan(p)
        assert got["part_words"] == len(offs) and got["end"] == got["part"] + 4 * len(offs)
        assert mr.workspace_size(p) == got["end"] - p.size
        assert sc["prefix"] == 4 * len(offs)
        assert [(d["off"], d["bytes"]) for d in sr.plan_fields(p)] == \
            mr.oracle(rec, mask, offs)[2]
    # a partition in HBM: never read, scanned by the launch, its words looked up in C
    for part, form in ((np.array(lengths, np.int64), PARTITION_LENGTHS),
                       (offs.astype(np.int32), PARTITION_OFFSETS)):
        with mr.plan_mask(rec, ptr_of, ARROW_DEVICE_ROCM, np.zeros_like(mask), ARROW_DEVICE_ROCM,
                          mask_ptr=mp, part=np.zeros_like(part), form=form,
                          part_dev=ARROW_DEVICE_ROCM, part_ptr=pp) as p:
            assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
            assert p.segments() == []
            got, sc = mr.plan_info(p), lr.plan_scan(p)
            assert got["part_words"] == 0 and got["end"] == got["part"]
            assert (sc["scan"], sc["src"], sc["count"], sc["rows"], sc["prefix"]) == \
                (True, pp, len(part), N, 0)
            assert (sc["lo"], sc["hi"]) == (0, part.nbytes - 1)
    # no rows: all-zero offsets, nothing to launch and nothing to read, wherever the partition is
    rec0 = RECORDS[name](0)
    for kw in ({}, {"part": np.zeros(3, np.int32), "form": PARTITION_LENGTHS,
                    "part_dev": ARROW_DEVICE_ROCM, "part_ptr": pp}):
        with mr.plan_mask(rec0, fake_ptrs(rec0), ARROW_DEVICE_ROCM, np.zeros(0, np.uint8),
                          ARROW_DEVICE_ROCM, mask_ptr=mp, **kw) as p:
            b = 3 if kw else 1
            sample, info = pack(message(rec0, np.zeros(0, np.uint8),
                                        **({"lengths": [0, 0, 0]} if kw else {})))
            assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
            assert mr.workspace_size(p) == 0 and p.segments()[0][1:] == (0, 4 * (b + 1))
            assert staged(p)[:4 * (b + 1)] == bytes(4 * (b + 1))
            assert mr.plan_info(p)["device"] is False


def test_other_plans_need_no_workspace(lib):
    rec = lr.clouds(N)
    with lr.plan_list(rec, fake_ptrs(rec), ARROW_DEVICE_ROCM, np.array([N], np.int32),
                      PARTITION_LENGTHS, ARROW_DEVICE_CPU) as p:
        assert mr.workspace_size(p) == 0
        with pytest.raises(DoraGpuError, match="not a mask plan"):
            mr.plan_info(p)


def refused(code, match, rec, ptr_of, dev, mask, mask_dev, **kw):
    with pytest.raises(DoraGpuError, match=match) as e:
        mr.plan_mask(rec, ptr_of, dev, mask, mask_dev, **kw)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals(lib):
    DORA_ERR_INVALID, DORA_ERR_UNSUPPORTED = -1, -4  # include/dora_gpu.h
    rec = lr.clouds(N)
    mask = np.ones(N, np.uint8)
    dev, host = ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU
    fake = fake_ptrs(rec)
    mp = PTR + (64 << 20)
    # mixed devices, both ways
    refused(DORA_ERR_INVALID, "the mask is in host memory and the values are in device memory",
            rec, fake, dev, mask, host)
    refused(DORA_ERR_INVALID, "the mask is in device memory and the values are in host memory",
            rec, host_ptr, host, mask, dev, mask_ptr=mp)
    # not dense, 2-D, wrong dtypes
    refused(DORA_ERR_INVALID, "mask stride 2: the mask is dense", rec, host_ptr, host, mask, host,
            mask_desc=((N,), (2,), np.uint8))
    refused(DORA_ERR_INVALID, "mask has 2 dimensions", rec, host_ptr, host, mask, host,
            mask_desc=((N, 1), None, np.uint8))
    for dt in (np.int8, np.int32, np.float32, np.uint16):
        refused(DORA_ERR_INVALID, "is not bool or uint8", rec, host_ptr, host,
                np.ones(N, dt), host)
    # N mismatch, on both sides
    for n in (N - 1, N + 1, 0):
        refused(DORA_ERR_INVALID, f"mask has {n} elements, the values have {N} rows", rec,
                host_ptr, host, np.ones(n, np.uint8), host)
        refused(DORA_ERR_INVALID, f"mask has {n} elements, the values have {N} rows", rec, fake,
                dev, np.ones(n, np.uint8), dev, mask_ptr=mp)
    # N > 2^24 rows (made-up pointers: nothing is read)
    big = mr.MAX_ROWS + 1

    def plan_big(n):
        t, k1 = tensor._describe(PTR, (n, 2), None, np.float32)
        m, k2 = tensor._describe(mp, (n,), None, np.uint8)
        mk, keep = tensor._describe_mask(None, [t], m, dev, None, 0, host)
        h = c_void_p()
        _lib.call("dora_gpu_plan_tensor_mask", byref(mk), dev, byref(h))
        return h
    with pytest.raises(DoraGpuError, match=f"a mask over {big} rows: at most {mr.MAX_ROWS}") as e:
        plan_big(big)
    assert e.value.code == DORA_ERR_UNSUPPORTED
    h = plan_big(mr.MAX_ROWS)  # the cap itself plans
    assert _lib.load().dora_gpu_plan_workspace_size(h) == 4 * (2 * mr.MAX_ROWS + 1 + 4097)
    _lib.load().dora_gpu_plan_free(h)
    # a host partition that does not describe the N source rows (the list plan's rules), whatever
    # K is: the mask below selects 33 rows, and a partition of 33 rows is refused
    half = mr.masks(N)[2][1]
    for where, ptrs, kw in ((host, host_ptr, {}), (dev, fake, {"mask_ptr": mp})):
        refused(DORA_ERR_INVALID, "the 2 lengths sum to 33, the values have 67 rows", rec, ptrs,
                where, half, where, part=np.array([13, 20], np.int32), form=PARTITION_LENGTHS,
                part_dev=host, **kw)
        refused(DORA_ERR_INVALID, "offset 2 is 68, past the 67 rows", rec, ptrs, where, half,
                where, part=np.array([0, 5, 68], np.int32), form=PARTITION_OFFSETS,
                part_dev=host, **kw)
        refused(DORA_ERR_INVALID, "lengths are not negative", rec, ptrs, where, half, where,
                part=np.array([-1, 68], np.int32), form=PARTITION_LENGTHS, part_dev=host, **kw)
    # a device partition needs device values
    refused(DORA_ERR_INVALID, "a partition in device memory needs values on this node's GPU",
            rec, host_ptr, host, mask, host, part=np.array([N], np.int32),
            form=PARTITION_LENGTHS, part_dev=dev, part_ptr=mp)
    # the values' own refusals come through, naming the field
    bad = [("x", rec[0][1], rec[0][2]), ("x", rec[1][1], rec[1][2])]
    refused(DORA_ERR_INVALID, "repeats the name of field 0", bad, host_ptr, host, mask, host)
