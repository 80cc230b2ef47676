"""Planning of argmax messages on the CPU (no GPU): dora_gpu_plan_tensor_reduce over made-up device
pointers (planning calls nothing in HIP and reads no tensor byte) and over real numpy memory.
Size, type info and leaf offsets are the reference packing's of the materialised index tensors
(oracle.pack_ref); a device plan with a reduced field has no segments, the launch kind of
gather_reduce_kernel and per field a reach that covers all C steps; entries that are all op 0 plan
exactly as the plain tensor or record; every refusal with its code, naming the field; the Python
TypeErrors."""
import ctypes
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST,
                           DoraGpuError, TensorReduce)
from tests import argmax_records as ar
from tests import cast_records as cr
from tests import struct_records as sr

PTR = 0x7E00_0000_0000  # never dereferenced


def fake_ptrs(rec):
    bases = ar.bases_of(rec)
    return lambda b: PTR + (1 << 26) * next(i for i, x in enumerate(bases) if x is b)


def host_ptr(b):
    return b.__array_interface__["data"][0]


def launch_of(p):
    launch, scan, checked = c_int(), c_int(), c_int()
    _lib.call("dora_gpu_test_plan_launch", p.handle, byref(launch), byref(scan), byref(checked))
    return launch.value, scan.value, checked.value


def test_device_plans_of_every_case(lib):
    """No segments, launch kind 6, the oracle's size, type info and offsets, and per field the
    reach numpy's strides give over every dimension, the reduced one included."""
    bodies = set()
    for label, rec, _ in ar.cases():
        sample, info, ranges = ar.oracle(rec)
        ptr_of = fake_ptrs(rec)
        with ar.plan_reduce(rec, ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample), label
            assert p.type_info().to_json() == info.to_json(), label
            assert p.segments() == [] and launch_of(p) == (6, 0, 1), label
            fs, ks = sr.plan_fields(p), ar.plan_reduces(p, len(rec))
            assert [(f["off"], f["bytes"]) for f in fs] == ranges, label
            for (_, b, v, r), f, k in zip(rec, fs, ks):
                assert f["src"] == ptr_of(b) + host_ptr(v) - host_ptr(b), label
                assert f["elem"] == v.itemsize, label
                if r is None:
                    assert k["op"] == 0 and k["body"] == 0 and (f["lo"], f["hi"]) == cr.reach(b, v)
                    continue
                ax = r["axis"] % v.ndim
                assert (f["lo"], f["hi"]) == ar.reach(v, ax), label
                off = host_ptr(v) - host_ptr(b)
                assert off + f["lo"] >= 0 and off + f["hi"] < b.nbytes, label
                assert k == {"op": 1, "c": v.shape[ax], "cstride": v.strides[ax],
                             "count": v.size // v.shape[ax], "bits": ar.INDEX[r["dtype"]][1],
                             "body": k["body"], "vector_units": k["vector_units"],
                             "element_units": k["element_units"]}, label
                wave = v.strides[ax] == v.itemsize and v.shape[ax] >= 32
                assert k["body"] == (2 if wave else 1), (label, k)
                bodies.add(k["body"])
                if k["body"] == 1:
                    e = 16 // (k["bits"] // 8)
                    assert k["vector_units"] + k["element_units"] == k["count"] // e, label
                    bodies |= {n for n in ("vector_units", "element_units") if k[n]}
    assert bodies == {1, 2, "vector_units", "element_units"}


def test_no_reduction_plans_as_the_plain_entry(lib):
    """`reduces` NULL or every op 0: dora_gpu_plan_tensor's plan (bare) or
    dora_gpu_plan_tensor_struct's, device and host."""
    from dora_amd.arrow_utils import Plan
    b = cr.source("float32", (9, 6))
    for v in (b, b[:, 1:5]):
        for dev in (ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU):
            ptr_of = (lambda x: PTR) if dev == ARROW_DEVICE_ROCM else host_ptr
            shape, strides, dtype, off = cr.describe_view(b, v, None)
            t, keep = tensor._describe(ptr_of(b), shape, strides, dtype, off)
            h = c_void_p()
            _lib.call("dora_gpu_plan_tensor", byref(t), dev, byref(h))
            with Plan(h.value, keep) as plain:
                for null in (False, True):
                    fields, reds, n, keep2 = ar.describe([(None, b, v, None)], ptr_of)
                    h = c_void_p()
                    _lib.call("dora_gpu_plan_tensor_reduce", fields, n, None if null else reds, dev,
                              byref(h))
                    with Plan(h.value, keep2) as p:
                        assert p.size == plain.size
                        assert p.type_info_bytes() == plain.type_info_bytes()
                        assert launch_of(p) == launch_of(plain)
                        if dev == ARROW_DEVICE_ROCM or v is b:
                            assert p.segments() == plain.segments()
            rec = [("a", b, v, None), ("n", b, b[:, 0], None)]
            with ar.plan_reduce(rec, ptr_of, dev) as p, \
                    sr.plan_record([r[:3] for r in rec], ptr_of, dev) as plain:
                assert p.size == plain.size and p.type_info_bytes() == plain.type_info_bytes()
                assert launch_of(p) == launch_of(plain)
                if dev == ARROW_DEVICE_ROCM:
                    assert p.segments() == plain.segments()
                    assert sr.plan_fields(p) == sr.plan_fields(plain)
    # the plain entries' refusals pass through: bfloat16 without a reduction
    fields, reds, n, keep = ar.describe([(None, b, b, None)], lambda x: PTR)
    fields[0].tensor.dtype_code, fields[0].tensor.dtype_bits = 4, 16
    with pytest.raises(DoraGpuError) as e:
        _lib.call("dora_gpu_plan_tensor_reduce", fields, n, reds, ARROW_DEVICE_ROCM, byref(c_void_p()))
    assert e.value.code == -4 and "Arrow has no bfloat16" in str(e.value)


def test_empty_leading_extent(lib):
    e = np.zeros((0, 3), np.float32)
    z = np.zeros((5, 0, 2), np.float16)
    for rec in ([(None, e, e, ar.red("float32", 1, "uint8"))],
                [(None, z, z, ar.red("float16", 0, "int32"))],
                [("a", e, e, ar.red("float32", 1, "uint8")), ("b", e, e, None)]):
        sample, info, _ = ar.oracle(rec)
        for dev in (ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU):
            with ar.plan_reduce(rec, lambda b: PTR, dev) as p:
                assert p.size == 0 == len(sample) and p.segments() == []
                assert p.type_info().to_json() == info.to_json()
                assert launch_of(p)[0] == 0


def test_host_plans_reduce_inside_the_call(lib):
    """Host values, pageable and pinned alike: one staged segment per reduced field holding the
    index bytes on return; a plain dense field is read in place."""
    for label, rec, _ in ar.cases():
        sample, info, ranges = ar.oracle(rec)
        for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
            with ar.plan_reduce(rec, host_ptr, dev) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), label
                assert launch_of(p) == (0, 0, 0), label
                segs = p.segments()
                assert [(s[1], s[2]) for s in segs] == ranges, label
                for (ptr, off, n), (_, _, v, r) in zip(segs, rec):
                    ar.same(ctypes.string_at(ptr, n), ar.want(v, r), label)


def plan_raw(fields, n, reds, dev=ARROW_DEVICE_ROCM):
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_reduce", fields, n, reds, dev, byref(h))
    _lib.load().dora_gpu_plan_free(h)


def refused(rec, code, *words, dev=ARROW_DEVICE_ROCM, edit=None):
    fields, reds, n, keep = ar.describe(rec, lambda b: PTR)
    if edit:
        edit(fields, reds)
    with pytest.raises(DoraGpuError) as e:
        plan_raw(fields, n, reds, dev)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(lib):
    INVALID, UNSUPPORTED = -1, -4
    f32 = cr.source("float32", (4, 3))
    ok = ar.red("float32", 1, "uint8")

    def named(bad_base, r, view=None):  # the offending field second, behind a good one
        return [("good", f32, f32, ok), ("bad", bad_base, bad_base if view is None else view, r)]

    for dev in (ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
        # fewer than two dimensions
        one = cr.source("float32", (4,))
        refused([(None, one, one, ar.red("float32", 0))], INVALID, "1 dimensions", dev=dev)
        # the axis
        for ax in (2, -1, 7):
            def axis(fields, reds, ax=ax):
                reds[1].axis = ax
            refused(named(f32, ok), INVALID, "field 1 `bad`", "axis", dev=dev, edit=axis)
        # C == 0
        z = np.zeros((4, 0), np.float32)
        refused(named(z, ar.red("float32", 1, "uint8")), INVALID, "field 1 `bad`", "extent 0", dev=dev)
        # C - 1 not representable
        for c, dt in ((257, "uint8"), (65537, "uint16")):
            b = np.zeros((4, c), np.uint8)
            refused(named(b, ar.red("uint8", 1, dt)), INVALID, "field 1 `bad`", str(c - 1), dt, dev=dev)
        wide = np.broadcast_to(np.zeros((4, 1), np.uint8), (4, 2 ** 31 + 1))
        refused(named(np.zeros((4, 1), np.uint8), ar.red("uint8", 1, "int32"), wide), INVALID,
                "field 1 `bad`", str(2 ** 31), "int32", dev=dev)
        # sources that are none of the seven
        for dt, name in ((np.int32, "int32"), (np.int64, "int64"), (np.float64, "float64"),
                         (np.uint32, "uint32"), (np.bool_, "bool")):
            b = np.zeros((4, 2), dt)
            refused(named(b, ar.red(name, 1, "uint8")), UNSUPPORTED, "field 1 `bad`", name,
                    "argmax source", dev=dev)
        # index dtypes that are none of the four
        for code, bits, name in ((0, 8, "int8"), (0, 16, "int16"), (1, 32, "uint32"), (1, 64, "uint64"),
                                 (2, 32, "float32")):
            def index(fields, reds, code=code, bits=bits):
                reds[1].dtype_code, reds[1].dtype_bits = code, bits
            refused(named(f32, ok), UNSUPPORTED, "field 1 `bad`", name, "index", dev=dev, edit=index)
        # another op
        def op(fields, reds):
            reds[1].op = 2
        refused(named(f32, ok), UNSUPPORTED, "field 1 `bad`", "op 2", dev=dev, edit=op)
        # a source that does not sit on its element size
        i16 = cr.source("int16", (4, 3))

        def odd(fields, reds):
            fields[1].tensor.byte_offset = 1
        refused(named(i16, ar.red("int16", 1, "uint8")), INVALID, "field 1 `bad`", "multiple",
                dev=dev, edit=odd)
    # the fields share the leading extent of their output shapes
    refused([("a", f32, f32, ok), ("b", f32, f32, ar.red("float32", 0, "uint8"))], INVALID,
            "field 1 `b`", "leading extent")
    t = cr.source("float32", (3, 4))
    rec = [("a", f32, f32, ok), ("b", t, t, ar.red("float32", 0, "uint8"))]  # (4,) and (4,)
    with ar.plan_reduce(rec, lambda b: PTR, ARROW_DEVICE_ROCM) as p:
        assert p.type_info().to_json() == ar.oracle(rec)[1].to_json()
    refused([("a", f32, f32, ok), ("a", f32, f32, None)], INVALID, "field 1 `a`", "repeats")
    # reach overflow counts the reduced axis
    def huge(fields, reds):
        fields[0].tensor.strides[1] = 1 << 61
    refused([(None, f32, f32, ok)], INVALID, "overflows", edit=huge)
    # arguments
    fields, reds, n, keep = ar.describe(named(f32, ok), lambda b: PTR)
    for args in ((None, n, reds), (fields, 0, reds)):
        with pytest.raises(DoraGpuError) as e:
            plan_raw(*args)
        assert e.value.code == INVALID
    with pytest.raises(DoraGpuError) as e:
        bad = (TensorReduce * 9)()
        bad[0].op = 1
        plan_raw((_lib.TensorField * 9)(), 9, bad)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(DoraGpuError) as e:
        plan_raw(fields, n, reds, dev=99)
    assert e.value.code == INVALID


def test_python_refusals(lib):
    x = np.zeros((4, 3), np.float32)
    a = tensor.argmax(x, -1, "uint8")
    assert a._entry() == (1, 1, 1, 8) and tensor.argmax(x, 0)._entry() == (1, 0, 0, 64)
    assert tensor.argmax(x, 1, np.int32)._entry() == (1, 1, 0, 32)
    for make, word in ((lambda v: tensor.ragged(v, lengths=[4]), "ragged"),
                       (lambda v: tensor.take(v, [0]), "take"),
                       (lambda v: tensor.masked(v, [1, 0, 1, 1]), "mask")):
        for v in (a, {"a": a, "b": x}):
            with pytest.raises(TypeError) as e:
                make(v)
            assert "argmax" in str(e.value) and word in str(e.value)
    for inner in (tensor.cast(x, "float16"), tensor.quantize(x, "uint8"), tensor.take(x, [0]),
                  tensor.masked(x, [1, 0, 1, 1]), tensor.ragged(x, lengths=[4]), {"a": x}, a):
        with pytest.raises(TypeError) as e:
            tensor.argmax(inner, 0)
        assert "argmax" in str(e.value)
    for outer in (lambda v: tensor.cast(v, "float32"), lambda v: tensor.quantize(v, "uint8")):
        with pytest.raises(TypeError) as e:
            outer(a)
        assert "argmax" in str(e.value)
    import pyarrow as pa
    got = tensor.from_numpy_argmax(np.array([[1, np.nan, 3, np.nan], [2, 5, 5, 1]], np.float32), 1, "uint8")
    assert got.type == pa.uint8() and got.to_pylist() == [1, 1]
    got = tensor.from_numpy_argmax(np.array([[0.0, -0.0, 0, 0], [-np.inf] * 4], np.float32), -1)
    assert got.type == pa.int64() and got.to_pylist() == [0, 0]
    bits = ar.bf16_last_bit()
    assert tensor.from_numpy_argmax(bits, 1, "uint16", bfloat16=True).to_pylist() == [1, 0, 1, 2]
    assert set(("Argmax", "argmax", "from_numpy_argmax")) <= set(tensor.__all__)
