"""Planning of cast messages on the CPU (no GPU): dora_gpu_plan_tensor_cast over made-up device
pointers (planning calls nothing in HIP and reads no tensor byte) and over real numpy memory.
Size, type info and leaf offsets are the reference packing's of the materialised converted
arrays (oracle.pack_ref); the identity cast plans exactly as the plain tensor or record; a device
plan with any cast field has no segments and per field the reach numpy computes from the view's
strides and the source itemsize, for every source/destination pair, both orders of size,
negative and zero strides; every refusal with its code, naming the field."""
from ctypes import byref, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST,
                           DoraGpuError, TensorCast)
from tests import cast_records as cr
from tests import struct_records as sr

PTR = 0x7E00_0000_0000  # never dereferenced


def fake_ptrs(rec):
    bases = cr.bases_of(rec)
    return lambda b: PTR + (1 << 20) * next(i for i, x in enumerate(bases) if x is b)


def host_ptr(b):
    return b.__array_interface__["data"][0]


def views(src):
    out = [("dense", *cr.run_view(src, 17, True)), ("cut", *cr.run_view(src, 17, False)),
           ("image", *cr.image_view(src))]
    return out + cr.strided_views(src)


@pytest.mark.parametrize("src,dst", cr.PAIRS)
def test_device_plans_of_every_pair(lib, src, dst):
    """Bare tensors and a record of them: no segments, the oracle's size, type info and offsets,
    and per field [lo, hi] as numpy's strides give it with the source itemsize."""
    rec = []
    for label, b, v in views(src):
        c = cr.cast(src, dst, 1 / 255 if label == "cut" else None)
        if src == dst and c["scale"] is None:
            c = cr.cast(src, dst, 0.5)  # (the identity is no cast: its own test below)
        one = [(None, b, v, c)]
        sample, info, ranges = cr.oracle(one)
        ptr_of = fake_ptrs(one)
        with cr.plan_cast(one, ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample) == v.size * np.dtype(dst).itemsize, label
            assert p.type_info().to_json() == info.to_json(), label
            assert p.segments() == [], label
            (f,), (k,) = sr.plan_fields(p), cr.plan_casts(p)
            assert f["gather"] and (f["off"], f["bytes"]) == ranges[0], label
            assert f["src"] == ptr_of(b) + host_ptr(v) - host_ptr(b), label
            assert (f["lo"], f["hi"]) == cr.reach(b, v) and f["elem"] == v.itemsize, label
            assert k == {"cast": True, "src_code": cr.SOURCES[src][1], "src_bits": v.itemsize * 8,
                         "dst_code": 2, "dst_bits": np.dtype(dst).itemsize * 8,
                         "has_scale": c["scale"] is not None,
                         "scale": float(np.float32(c["scale"] if c["scale"] is not None else 1.0)),
                         "count": v.size, "src_bytes": v.size * v.itemsize,
                         "dst_bytes": len(sample)}, label
        if v.shape[0] == 5:
            rec.append((label, b, v, c))
    # the views of leading extent 5 as one record, a plain field between them
    plain = cr.source("int16", (5, 3), 9)
    rec.insert(1, ("plain", plain, plain[:, ::2], None))
    sample, info, ranges = cr.oracle(rec)
    ptr_of = fake_ptrs(rec)
    with cr.plan_cast(rec, ptr_of, ARROW_DEVICE_ROCM) as p:
        assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
        assert p.segments() == []
        fs, ks = sr.plan_fields(p), cr.plan_casts(p)
        assert [(f["off"], f["bytes"]) for f in fs] == ranges
        assert [k["cast"] for k in ks] == [True, False, True]
        for (_, b, v, _), f in zip(rec, fs):
            assert (f["lo"], f["hi"]) == cr.reach(b, v) and f["elem"] == v.itemsize
            off = host_ptr(v) - host_ptr(b)
            assert off + f["lo"] >= 0 and off + f["hi"] < b.nbytes


def test_identity_plans_as_the_plain_tensor(lib):
    """Source == destination without a scale: the plain plan, bare and as a record, dense and
    strided, device and host; with a scale a real cast."""
    b = cr.source("float32", (9, 6))
    for v in (b, b[:, 1:5]):
        for dev in (ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU):
            ptr_of = (lambda x: PTR) if dev == ARROW_DEVICE_ROCM else host_ptr
            same, real = cr.cast("float32", "float32"), cr.cast("float32", "float32", 2.0)
            with cr.plan_cast([(None, b, v, same)], ptr_of, dev) as p, \
                    cr.plan_cast([(None, b, v, None)], ptr_of, dev) as q:
                shape, strides, dtype, off = cr.describe_view(b, v, None)
                t, keep = tensor._describe(ptr_of(b), shape, strides, dtype, off)
                h = c_void_p()
                _lib.call("dora_gpu_plan_tensor", byref(t), dev, byref(h))
                from dora_amd.arrow_utils import Plan
                with Plan(h.value, keep) as plain:
                    for x in (p, q):
                        assert x.size == plain.size and x.type_info_bytes() == plain.type_info_bytes()
                        if dev == ARROW_DEVICE_ROCM or v is b:
                            assert x.segments() == plain.segments()
                        else:  # (staged: the segment reads a buffer of the plan's own)
                            assert [s[1:] for s in x.segments()] == [s[1:] for s in plain.segments()]
                    if dev == ARROW_DEVICE_ROCM:
                        # (a plan of one view, as dora_gpu_plan_tensor's: not a record of one field)
                        _lib.call("dora_gpu_test_plan_gather", p.handle, None, None, None, None,
                                  None, None, None, None, None)
            rec = [("a", b, v, same), ("n", b, b[:, 0], None)]
            with cr.plan_cast(rec, ptr_of, dev) as p, \
                    sr.plan_record([r[:3] for r in rec], ptr_of, dev) as plain:
                assert p.size == plain.size and p.type_info_bytes() == plain.type_info_bytes()
                if dev == ARROW_DEVICE_ROCM:
                    assert p.segments() == plain.segments()
                    assert sr.plan_fields(p) == sr.plan_fields(plain)
                    assert not any(k["cast"] for k in cr.plan_casts(p))
            if dev == ARROW_DEVICE_ROCM:
                with cr.plan_cast([(None, b, v, real)], ptr_of, dev) as p:
                    assert p.segments() == [] and cr.plan_casts(p)[0]["cast"]


def test_float16_identity_and_empty(lib):
    h = cr.source("float16", (4, 3))
    with cr.plan_cast([(None, h, h, cr.cast("float16", "float16"))], lambda b: PTR,
                      ARROW_DEVICE_ROCM) as p:
        assert p.segments() == [(PTR, 0, h.nbytes)]
    # d0 == 0: an empty message of the destination type
    e = np.zeros((0, 3), np.uint8)
    for rec in ([(None, e, e, cr.cast("uint8", "float16", 0.5))],
                [("a", e, e, cr.cast("uint8", "float32")), ("b", e, e, None)]):
        sample, info, _ = cr.oracle(rec)
        for dev in (ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU):
            with cr.plan_cast(rec, lambda b: PTR, dev) as p:
                assert p.size == 0 == len(sample) and p.segments() == []
                assert p.type_info().to_json() == info.to_json()


def test_host_plans_convert_inside_the_call(lib):
    """Host values, pageable and pinned alike: one staged segment per cast field, dense views
    included, holding the converted bytes on return; a plain dense field is read in place."""
    rec = cr.three_fields()
    sample, info, ranges = cr.oracle(rec)
    for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
        with cr.plan_cast(rec, host_ptr, dev) as p:
            assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
            segs = p.segments()
            assert [(s[1], s[2]) for s in segs] == ranges
            if dev == ARROW_DEVICE_CPU:
                assert segs[1][0] == host_ptr(rec[1][1])
            import ctypes
            for (ptr, off, n), (_, _, v, c) in zip(segs, rec):
                cr.same(ctypes.string_at(ptr, n), cr.want(v, c))


def plan_raw(fields, n, casts, dev=ARROW_DEVICE_ROCM):
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_cast", fields, n, casts, dev, byref(h))
    _lib.load().dora_gpu_plan_free(h)


def refused(rec, code, *words, dev=ARROW_DEVICE_ROCM, edit=None):
    fields, casts, n, keep = cr.describe(rec, lambda b: PTR)
    if edit:
        edit(fields, casts)
    with pytest.raises(DoraGpuError) as e:
        plan_raw(fields, n, casts, dev)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(lib):
    INVALID, UNSUPPORTED = -1, -4
    u8, f32 = cr.source("uint8", (4, 3)), cr.source("float32", (4, 3))
    ok = cr.cast("uint8", "float16")

    def named(bad_base, c):  # the offending field second, behind a good one
        return [("good", u8, u8, ok), ("bad", bad_base, bad_base, c)]

    # sources that are no cast source: UNSUPPORTED naming the dtype and the field
    for dt, name in ((np.int32, "int32"), (np.int64, "int64"), (np.float64, "float64"),
                     (np.uint32, "uint32"), (np.bool_, "bool"), (np.complex64, "complex64")):
        b = np.zeros((4, 2), dt)
        refused(named(b, cr.cast(name, "float32")), UNSUPPORTED, "field 1 `bad`", name,
                "cast source")
    # destinations other than float16 / float32
    for code, bits, name in ((2, 64, "float64"), (0, 32, "int32"), (1, 8, "uint8"), (4, 16, "bfloat16")):
        def dest(fields, casts, code=code, bits=bits):
            casts[1].dtype_code, casts[1].dtype_bits = code, bits
        refused(named(f32, cr.cast("float32", "float32", 1.0)), UNSUPPORTED, "field 1 `bad`", name,
                "destination", edit=dest)
    # the scale
    for s in (float("nan"), float("inf"), float("-inf")):
        refused(named(f32, cr.cast("float32", "float16", s)), INVALID, "field 1 `bad`", "scale")
    # a source that does not sit on its element size
    i16 = cr.source("int16", (4, 3))

    def odd(fields, casts):
        fields[1].tensor.byte_offset = 1
    refused(named(i16, cr.cast("int16", "float32")), INVALID, "field 1 `bad`", "multiple", edit=odd)
    for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
        refused(named(i16, cr.cast("int16", "float32")), INVALID, "field 1 `bad`", dev=dev, edit=odd)
    # the record's own refusals pass through: a leading extent that differs, a duplicate name
    refused([("a", u8, u8, ok), ("b", f32, f32[:3], cr.cast("float32", "float16"))], INVALID,
            "field 1 `b`", "leading extent")
    refused([("a", u8, u8, ok), ("a", f32, f32, None)], INVALID, "field 1 `a`", "repeats")
    # reach overflow is computed with the source element size
    def huge(fields, casts):
        fields[0].tensor.strides[0] = 1 << 62
    refused([(None, i16, i16[:, :2], cr.cast("int16", "float32"))], INVALID, "overflows", edit=huge)
    # arguments
    fields, casts, n, keep = cr.describe(named(f32, cr.cast("float32", "float16")), lambda b: PTR)
    for args in ((fields, n, None), (None, n, casts), (fields, 0, casts)):
        with pytest.raises(DoraGpuError) as e:
            plan_raw(*args)
        assert e.value.code == INVALID
    with pytest.raises(DoraGpuError) as e:
        plan_raw((_lib.TensorField * 9)(), 9, (TensorCast * 9)())
    assert e.value.code == UNSUPPORTED
    with pytest.raises(DoraGpuError) as e:
        plan_raw(fields, n, casts, dev=99)
    assert e.value.code == INVALID
    # the plain tensor plan still refuses bfloat16 with its own words
    t, keep = tensor._describe(PTR, (4,), None, np.uint16)
    t.dtype_code = 4
    h = c_void_p()
    with pytest.raises(DoraGpuError) as e:
        _lib.call("dora_gpu_plan_tensor", byref(t), ARROW_DEVICE_ROCM, byref(h))
    assert e.value.code == UNSUPPORTED and "Arrow has no bfloat16 (send a view as uint16)" in str(e.value)


def test_python_refuses_cast_under_ragged_and_take(lib):
    x = np.zeros((4, 3), np.uint8)
    c = tensor.cast(x, "float16", scale=1 / 255)
    assert (c._code, c._bits, c.scale) == (2, 16, 1 / 255)
    assert tensor.cast(x, np.float32)._bits == 32 and tensor.cast(x, np.dtype("float16"))._bits == 16
    for make, word in ((lambda v: tensor.ragged(v, lengths=[4]), "ragged"),
                       (lambda v: tensor.take(v, [0]), "take")):
        for v in (c, {"a": c, "b": x}):
            with pytest.raises(TypeError) as e:
                make(v)
            assert "cast" in str(e.value) and word in str(e.value)
    with pytest.raises(TypeError):
        tensor.cast({"a": x}, "float16")
    with pytest.raises(TypeError):
        tensor.cast(tensor.take(x, [0]), "float16")
    import pyarrow as pa
    got = tensor.from_numpy_cast(x, "float16", 1 / 255)
    assert got.type == pa.list_(pa.float16(), 3) and len(got) == 4
