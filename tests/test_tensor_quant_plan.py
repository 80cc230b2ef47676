"""Planning of quantised messages on the CPU (no GPU): dora_gpu_plan_tensor_convert over made-up
device pointers (planning calls nothing in HIP and reads no tensor byte) and over real numpy
memory.  Size, type info and leaf offsets are the reference packing's of the quantised numpy
arrays (oracle.pack_ref over `tensor.from_numpy_quantize`); a device plan with any quantised field
has no segments and per field the reach numpy computes from the view's strides and the source
itemsize, for all 28 pairs; host plans convert inside the call, bit-exact over every value set;
every refusal with its code, naming the field."""
import ctypes
from ctypes import byref, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST,
                           DoraGpuError, TensorCast, TensorQuant)
from tests import cast_records as cr
from tests import quant_records as qr
from tests import struct_records as sr
from tests.test_tensor_cast_plan import PTR, fake_ptrs, host_ptr, views


@pytest.mark.parametrize("src,dst", qr.PAIRS)
def test_device_plans_of_every_pair(lib, src, dst):
    """Bare tensors and a record of them: no segments, the oracle's size, type info and offsets,
    and per field [lo, hi] as numpy's strides give it with the source itemsize."""
    rec = []
    zps = qr.zero_points(dst)
    for i, (label, b, v) in enumerate(views(src)):
        c = qr.quant(src, dst, 0.5 if label == "cut" else None, zps[i % len(zps)])
        one = [(None, b, v, c)]
        sample, info, ranges = qr.oracle(one)
        ptr_of = fake_ptrs(one)
        with qr.plan_convert(one, ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample) == v.size * np.dtype(dst).itemsize, label
            assert p.type_info().to_json() == info.to_json(), label
            assert p.segments() == [], label
            (f,), (k,) = sr.plan_fields(p), qr.plan_converts(p)
            assert f["gather"] and (f["off"], f["bytes"]) == ranges[0], label
            assert f["src"] == ptr_of(b) + host_ptr(v) - host_ptr(b), label
            assert (f["lo"], f["hi"]) == cr.reach(b, v) and f["elem"] == v.itemsize, label
            assert k == {"cast": True, "src_code": cr.SOURCES[src][1], "src_bits": v.itemsize * 8,
                         "dst_code": 2, "dst_bits": np.dtype(dst).itemsize * 8,
                         "has_scale": c["scale"] is not None,
                         "scale": float(np.float32(c["scale"] if c["scale"] is not None else 1.0)),
                         "count": v.size, "src_bytes": v.size * v.itemsize,
                         "dst_bytes": len(sample), "quant": True, "q_code": qr.DESTS[dst][1],
                         "q_bits": np.dtype(dst).itemsize * 8, "zp": c["zp"]}, label
        if v.shape[0] == 5:
            rec.append((label, b, v, c))
    # the views of leading extent 5 as one record, a plain field between them
    plain = cr.source("int16", (5, 3), 9)
    rec.insert(1, ("plain", plain, plain[:, ::2], None))
    sample, info, ranges = qr.oracle(rec)
    ptr_of = fake_ptrs(rec)
    with qr.plan_convert(rec, ptr_of, ARROW_DEVICE_ROCM) as p:
        assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
        assert p.segments() == []
        fs, ks = sr.plan_fields(p), qr.plan_converts(p)
        assert [(f["off"], f["bytes"]) for f in fs] == ranges
        assert [k["quant"] for k in ks] == [True, False, True]
        for (_, b, v, _), f in zip(rec, fs):
            assert (f["lo"], f["hi"]) == cr.reach(b, v) and f["elem"] == v.itemsize
            off = host_ptr(v) - host_ptr(b)
            assert off + f["lo"] >= 0 and off + f["hi"] < b.nbytes


def segments_equal(p, rec, what):
    segs = p.segments()
    assert len(segs) == len(rec), what
    for (ptr, off, n), (_, _, v, c) in zip(segs, rec):
        qr.same(ctypes.string_at(ptr, n), qr.want(v, c), what)


@pytest.mark.parametrize("k", range(qr.N_VALUE_SETS))
def test_host_plans_are_bit_exact_over_the_value_sets(lib, k):
    """Host plans, pageable and pinned alike, convert inside the call: every value set under
    every scale and zero point, dense and cut from a wider base, equals the statement."""
    label, x, qs = qr.value_sets()[k]
    b, v = cr.cut_from_wider(x)
    for i, q in enumerate(qs):
        dev = ARROW_DEVICE_ROCM_HOST if i % 2 else ARROW_DEVICE_CPU
        for base, view in ((x, x), (b, v)):
            rec = [(None, base, view, q)]
            with qr.plan_convert(rec, host_ptr, dev) as p:
                assert p.size == view.size * np.dtype(q["dst"]).itemsize
                segments_equal(p, rec, label + qr.label_of(q))


def test_a_mixed_record_plans_as_the_three_converted_arrays(lib):
    """A quantised, a plain and a cast field: the oracle's plan of the three converted arrays, on
    the device without segments, on the host converted on return."""
    rec = qr.three_fields()
    sample, info, ranges = qr.oracle(rec)
    with qr.plan_convert(rec, fake_ptrs(rec), ARROW_DEVICE_ROCM) as p:
        assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
        assert p.segments() == []
        ks = qr.plan_converts(p)
        assert [(k["cast"], k["quant"]) for k in ks] == [(True, True), (False, False), (True, False)]
        assert [(f["off"], f["bytes"]) for f in sr.plan_fields(p)] == ranges
    for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
        with qr.plan_convert(rec, host_ptr, dev) as p:
            assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
            assert [(s[1], s[2]) for s in p.segments()] == ranges
            if dev == ARROW_DEVICE_CPU:
                assert p.segments()[1][0] == host_ptr(rec[1][1])  # (the plain field, in place)
            segments_equal(p, rec, "three fields")


def test_without_a_quantised_field_it_is_the_cast_plan(lib):
    """No quantise entry, or none at all: exactly dora_gpu_plan_tensor_cast's plan; neither array:
    the plain record's."""
    rec = cr.three_fields()
    ptr_of = fake_ptrs(rec)
    fields, casts, quants, n, keep = qr.describe(rec, ptr_of)
    from dora_amd.arrow_utils import Plan
    with cr.plan_cast(rec, ptr_of, ARROW_DEVICE_ROCM) as want:
        for q in (quants, None):
            h = c_void_p()
            _lib.call("dora_gpu_plan_tensor_convert", fields, n, casts, q, ARROW_DEVICE_ROCM, byref(h))
            with Plan(h.value, keep) as p:
                assert p.size == want.size and p.type_info_bytes() == want.type_info_bytes()
                assert p.segments() == want.segments() == []
                assert sr.plan_fields(p) == sr.plan_fields(want)
                assert cr.plan_casts(p) == cr.plan_casts(want)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_convert", fields, n, None, None, ARROW_DEVICE_ROCM, byref(h))
    with Plan(h.value, keep) as p, sr.plan_record([r[:3] for r in rec], ptr_of, ARROW_DEVICE_ROCM) as plain:
        assert p.size == plain.size and p.type_info_bytes() == plain.type_info_bytes()
        assert sr.plan_fields(p) == sr.plan_fields(plain)


def test_no_identity_and_empty(lib):
    """uint8 -> uint8 without a scale is still a conversion; d0 == 0 is an empty message of the
    destination type."""
    u = cr.source("uint8", (4, 3))
    with qr.plan_convert([(None, u, u, qr.quant("uint8", "uint8"))], lambda b: PTR,
                         ARROW_DEVICE_ROCM) as p:
        assert p.segments() == [] and qr.plan_converts(p)[0]["quant"]
    e = np.zeros((0, 3), np.float32)
    for rec in ([(None, e, e, qr.quant("float32", "uint8", 255.0))],
                [("a", e, e, qr.quant("float32", "int16", None, -7)), ("b", e, e, None)]):
        sample, info, _ = qr.oracle(rec)
        for dev in (ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU):
            with qr.plan_convert(rec, lambda b: PTR, dev) as p:
                assert p.size == 0 == len(sample) and p.segments() == []
                assert p.type_info().to_json() == info.to_json()


def plan_raw(fields, n, casts, quants, dev=ARROW_DEVICE_ROCM):
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_convert", fields, n, casts, quants, dev, byref(h))
    _lib.load().dora_gpu_plan_free(h)


def refused(rec, code, *words, dev=ARROW_DEVICE_ROCM, edit=None):
    fields, casts, quants, n, keep = qr.describe(rec, lambda b: PTR)
    if edit:
        edit(fields, casts, quants)
    with pytest.raises(DoraGpuError) as e:
        plan_raw(fields, n, casts, quants, dev)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(lib):
    INVALID, UNSUPPORTED = -1, -4
    u8, f32 = cr.source("uint8", (4, 3)), cr.source("float32", (4, 3))
    ok = qr.quant("uint8", "int8", 0.5)

    def named(bad_base, c):  # the offending field second, behind a good one
        return [("good", u8, u8, ok), ("bad", bad_base, bad_base, c)]

    # destinations other than the four: UNSUPPORTED naming the dtype and the field
    for code, bits, name in ((0, 32, "int32"), (1, 32, "uint32"), (0, 64, "int64"),
                             (2, 16, "float16"), (2, 32, "float32"), (6, 8, "bool")):
        def dest(fields, casts, quants, code=code, bits=bits):
            quants[1].dtype_code, quants[1].dtype_bits = code, bits
        refused(named(f32, qr.quant("float32", "uint8")), UNSUPPORTED, "field 1 `bad`", name,
                "destination", edit=dest)
    # the zero point outside [lo, hi]
    for dst, zp in (("uint8", -1), ("uint8", 256), ("int8", -129), ("int8", 128),
                    ("uint16", 65536), ("uint16", -1), ("int16", 32768), ("int16", -32769)):
        refused(named(f32, qr.quant("float32", dst, None, zp)), INVALID, "field 1 `bad`", "zero point")
    # the scale
    for s in (float("nan"), float("inf"), float("-inf")):
        refused(named(f32, qr.quant("float32", "uint8", s)), INVALID, "field 1 `bad`", "scale")

    # a field that is both cast and quantised
    def both(fields, casts, quants):
        casts[1].dtype_code, casts[1].dtype_bits = 2, 16
    refused(named(f32, qr.quant("float32", "uint8")), INVALID, "field 1 `bad`", "both", edit=both)
    # sources that are no cast source
    for dt, name in ((np.int32, "int32"), (np.int64, "int64"), (np.float64, "float64"),
                     (np.uint32, "uint32"), (np.bool_, "bool")):
        b = np.zeros((4, 2), dt)
        refused(named(b, qr.quant(name, "uint8")), UNSUPPORTED, "field 1 `bad`", name, "source")
    # a source that does not sit on its element size
    i16 = cr.source("int16", (4, 3))

    def odd(fields, casts, quants):
        fields[1].tensor.byte_offset = 1
    for dev in (ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
        refused(named(i16, qr.quant("int16", "uint8")), INVALID, "field 1 `bad`", "multiple",
                dev=dev, edit=odd)
    # the record's own refusals pass through
    refused([("a", u8, u8, ok), ("b", f32, f32[:3], qr.quant("float32", "uint8"))], INVALID,
            "field 1 `b`", "leading extent")
    # reach overflow is computed with the source element size

    def huge(fields, casts, quants):
        fields[0].tensor.strides[0] = 1 << 62
    refused([(None, i16, i16[:, :2], qr.quant("int16", "uint8"))], INVALID, "overflows", edit=huge)
    # a bare tensor's refusal names the dtype
    refused([(None, f32, f32, qr.quant("float32", "uint8", None, 300))], INVALID, "zero point", "uint8")
    # arguments
    fields, casts, quants, n, keep = qr.describe(named(f32, qr.quant("float32", "uint8")), lambda b: PTR)
    for args in ((None, n, casts, quants), (fields, 0, casts, quants)):
        with pytest.raises(DoraGpuError) as e:
            plan_raw(*args)
        assert e.value.code == INVALID
    with pytest.raises(DoraGpuError) as e:
        plan_raw((_lib.TensorField * 9)(), 9, (TensorCast * 9)(), (TensorQuant * 9)())
    assert e.value.code == UNSUPPORTED
    with pytest.raises(DoraGpuError) as e:
        plan_raw(fields, n, casts, quants, dev=99)
    assert e.value.code == INVALID
    # the cast entry keeps refusing an integer destination, now pointing to the new call
    fields, casts, n, keep = cr.describe([(None, f32, f32, cr.cast("float32", "float32", 1.0))],
                                         lambda b: PTR)
    casts[0].dtype_code, casts[0].dtype_bits = 1, 8
    h = c_void_p()
    with pytest.raises(DoraGpuError) as e:
        _lib.call("dora_gpu_plan_tensor_cast", fields, n, casts, ARROW_DEVICE_ROCM, byref(h))
    assert e.value.code == UNSUPPORTED and "uint8" in str(e.value)
    assert "dora_gpu_plan_tensor_convert" in str(e.value)


def test_python_api_and_its_refusals(lib):
    import pyarrow as pa
    import torch
    x = np.linspace(-1, 2, 12, dtype=np.float32).reshape(4, 3)
    q = tensor.quantize(x, "uint8", scale=255, zero_point=3)
    assert q._entry() == (1, 8, 255.0, 3) and q.values is x
    assert tensor.quantize(x, np.int16)._entry() == (0, 16, None, 0)
    assert tensor.quantize(x, np.dtype("uint16"))._entry()[:2] == (1, 16)
    assert tensor.quantize(x, torch.int8)._entry()[:2] == (0, 8)
    assert tensor.quantize(x, torch.uint8, np.float32(0.5))._entry() == (1, 8, 0.5, 0)
    for name in ("Quantized", "quantize", "from_numpy_quantize"):
        assert name in tensor.__all__
    c = tensor.cast(x, "float16")
    for make, word in ((lambda v: tensor.ragged(v, lengths=[4]), "ragged"),
                       (lambda v: tensor.take(v, [0]), "take"),
                       (lambda v: tensor.masked(v, [1, 0, 1, 1]), "mask")):
        for v in (q, {"a": q, "b": x}):
            with pytest.raises(TypeError) as e:
                make(v)
            assert "quantize" in str(e.value) and word in str(e.value)
    with pytest.raises(TypeError) as e:
        tensor.cast(q, "float16")
    assert "quantised" in str(e.value)
    for bad in (c, {"a": x}, tensor.take(x, [0]), q):
        with pytest.raises(TypeError):
            tensor.quantize(bad, "uint8")
    with pytest.raises(TypeError) as e:  # per-channel scales
        tensor.quantize(x, "uint8", scale=np.ones(3, np.float32))
    assert "per-channel" in str(e.value)
    with pytest.raises(TypeError) as e:
        tensor.quantize(x, "uint8", zero_point=[1, 2, 3])
    assert "per-channel" in str(e.value)
    got = tensor.from_numpy_quantize(x, "uint8", 255, 3)
    assert got.type == pa.list_(pa.uint8(), 3) and len(got) == 4
    want = np.clip(np.rint(x * np.float32(255)), -3, 252).astype(np.int32) + 3
    assert got.flatten().to_numpy().tolist() == want.reshape(-1).tolist()
    # the edge values of the contract
    edge = np.array([0.5, 1.5, 2.5, 254.5, 255.5, -128.5, -0.5, np.nan, np.inf, -np.inf, 1e30,
                     -1e30, 3e9], np.float32)
    for dst, zp, expect in (("uint8", 0, [0, 2, 2, 254, 255, 0, 0, 0, 255, 0, 255, 0, 255]),
                            ("uint8", 128, [128, 130, 130, 255, 255, 0, 128, 128, 255, 0, 255, 0, 255]),
                            ("int8", -7, [-7, -5, -5, 127, 127, -128, -7, -7, 127, -128, 127, -128, 127]),
                            ("uint16", 65535, [65535, 65535, 65535, 65535, 65535, 65407, 65535, 65535,
                                               65535, 0, 65535, 0, 65535])):
        got = tensor.from_numpy_quantize(edge, dst, None, zp).to_numpy().tolist()
        assert got == expect, (dst, zp, got)
