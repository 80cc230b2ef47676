"""Planning of crops messages on the CPU (no GPU): dora_gpu_plan_tensor_crop over made-up device
pointers (planning calls nothing in HIP and reads no byte of a frame or of the boxes) and over real
numpy memory.  Size, type info and leaf offsets are the reference packing's of the materialised
crops (oracle.pack_ref); a device plan with a field of crops has no segments, the launch kind of
gather_crop_kernel, per field the reach of its whole frame and the 16 * K bytes of its boxes;
entries that are all mode 0 plan exactly as the plain tensor or record; every refusal with its
code, naming the field; the Python TypeErrors; and the statement itself: the whole frame as a box
is `from_numpy_resize` of the frame."""
import ctypes
from ctypes import byref, c_int, c_void_p

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST,
                           DoraGpuError, TensorCrop)
from tests import cast_records as cr
from tests import crop_records as kr
from tests import struct_records as sr

PTR = 0x7E00_0000_0000  # never dereferenced


def fake_ptrs(rec):
    bases = kr.bases_of(rec)
    return lambda b: PTR + (1 << 26) * next(i for i, x in enumerate(bases) if x is b)


def host_ptr(b):
    return b.__array_interface__["data"][0]


def launch_of(p):
    launch, scan, checked = c_int(), c_int(), c_int()
    _lib.call("dora_gpu_test_plan_launch", p.handle, byref(launch), byref(scan), byref(checked))
    return launch.value, scan.value, checked.value


def test_device_plans_of_every_case(lib):
    """No segments, launch kind 8, the oracle's size, type info and offsets, per field the reach
    numpy's strides give over the whole frame, and the boxes where they were given: K rows, 16 * K
    bytes checked, on the device.  K == 0 is the empty message: nothing to launch."""
    paths, box_starts = set(), set()
    for label, rec, offsets in kr.cases():
        sample, info, ranges = kr.oracle(rec)
        ptr_of = fake_ptrs(rec)
        with kr.plan_crop(rec, ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample), label
            assert p.type_info().to_json() == info.to_json(), label
            if len(sample) == 0:
                assert p.segments() == [] and launch_of(p)[0] == 0, label
                continue
            assert p.segments() == [] and launch_of(p) == (8, 0, 1), label
            for mis in offsets:
                fs, ks = sr.plan_fields(p), kr.plan_crops(p, len(rec), 4096 + mis)
                assert [(f["off"], f["bytes"]) for f in fs] == ranges, label
                for (_, b, v, c), f, k in zip(rec, fs, ks):
                    assert f["src"] == ptr_of(b) + host_ptr(v) - host_ptr(b), label
                    assert f["elem"] == v.itemsize, label
                    assert (f["lo"], f["hi"]) == cr.reach(b, v), label
                    off = host_ptr(v) - host_ptr(b)
                    assert off + f["lo"] >= 0 and off + f["hi"] < b.nbytes, label
                    if c is None:
                        assert k["mode"] == 0 and k["k"] == 0 and k["boxes"] == 0, label
                        continue
                    n = len(c["boxes"])
                    at = ptr_of(c["boxes_base"]) + host_ptr(c["boxes"]) - host_ptr(c["boxes_base"])
                    assert k["mode"] == kr.MODES[c["mode"]] and k["k"] == n, label
                    assert k["boxes"] == at and k["device"] == 1, label
                    assert (k["lo"], k["hi"]) == (0, 16 * n - 1), label
                    box_starts.add(at % 16)
                    bits = kr.DESTS[kr.dst_name(c)][1]
                    count, e = f["bytes"] * 8 // bits, 128 // bits
                    assert k["head"] + e * k["units"] + k["tail"] == count, label
                    assert k["head"] < e and k["tail"] < e, label
                    if k["units"] or k["head"] == 0:
                        assert (4096 + mis + f["off"] + k["head"] * bits // 8) % 16 == 0, label
                    paths |= {n for n in ("head", "units", "tail") if k[n]}
    assert paths == {"head", "units", "tail"}
    assert box_starts == {0, 4, 8, 12}


def test_no_crop_plans_as_the_plain_entry(lib):
    """`crops` NULL or every mode 0: dora_gpu_plan_tensor's plan (bare) or
    dora_gpu_plan_tensor_struct's, device and host, refusals included."""
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
                    fields, arr, n, keep2 = kr.describe([(None, b, v, None)], ptr_of)
                    h = c_void_p()
                    _lib.call("dora_gpu_plan_tensor_crop", fields, n, None if null else arr, dev,
                              byref(h))
                    with Plan(h.value, keep2) as p:
                        assert p.size == plain.size
                        assert p.type_info_bytes() == plain.type_info_bytes()
                        assert launch_of(p) == launch_of(plain)
                        if dev == ARROW_DEVICE_ROCM or v is b:
                            assert p.segments() == plain.segments()
            rec = [("a", b, v, None), ("n", b, b[:, 0], None)]
            with kr.plan_crop(rec, ptr_of, dev) as p, \
                    sr.plan_record([r[:3] for r in rec], ptr_of, dev) as plain:
                assert p.size == plain.size and p.type_info_bytes() == plain.type_info_bytes()
                assert launch_of(p) == launch_of(plain)
                if dev == ARROW_DEVICE_ROCM:
                    assert p.segments() == plain.segments()
                    assert sr.plan_fields(p) == sr.plan_fields(plain)
    fields, arr, n, keep = kr.describe([(None, b, b, None)], lambda x: PTR)
    fields[0].tensor.dtype_code, fields[0].tensor.dtype_bits = 4, 16
    with pytest.raises(DoraGpuError) as e:
        _lib.call("dora_gpu_plan_tensor_crop", fields, n, arr, ARROW_DEVICE_ROCM, byref(c_void_p()))
    assert e.value.code == -4 and "Arrow has no bfloat16" in str(e.value)


def test_host_plans_crop_inside_the_call(lib):
    """Host values, pageable and pinned alike: one staged segment per field of crops holding the
    crops' bytes on return; a plain dense field is read in place."""
    for label, rec, _ in kr.cases():
        sample, info, ranges = kr.oracle(rec)
        for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
            with kr.plan_crop(rec, host_ptr, dev) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), label
                assert launch_of(p) == (0, 0, 0), label
                segs = p.segments()
                if len(sample) == 0:
                    assert segs == [], label
                    continue
                assert [(s[1], s[2]) for s in segs] == ranges, label
                for (ptr, off, n), (_, _, v, c) in zip(segs, rec):
                    kr.same(ctypes.string_at(ptr, n), kr.want(v, c), label)


def test_the_statement(lib):
    """The whole frame as a box is the resize of the frame; a box of the crops' own extents moves
    elements unchanged; an empty box is zeros; int32's extremes clamp to the whole frame."""
    x = cr.source("uint8", (8, 10, 3), seed=31)
    for mode in kr.MODES:
        for dtype in (None, "float16", "int16"):
            whole = tensor._numpy_resize(x, (4, 6), (0, 1), mode, dtype)
            rows = [(0, 0, 8, 10), (kr.I32_MIN, kr.I32_MIN, kr.I32_MAX, kr.I32_MAX), (-5, -5, 99, 99)]
            got = tensor._numpy_crops(x, rows, (4, 6), (0, 1), mode, dtype)
            assert got.shape == (3, 4, 6, 3) and got.dtype == whole.dtype
            for k in range(3):
                assert got[k].tobytes() == whole.tobytes(), (mode, dtype, k)
        got = tensor._numpy_crops(x, [(2, 3, 6, 9), (5, 5, 5, 9), (6, 0, 2, 10)], (4, 6), (0, 1), mode)
        assert got[0].tobytes() == np.ascontiguousarray(x[2:6, 3:9]).tobytes()
        assert not got[1].any() and not got[2].any()
    import pyarrow as pa
    arr = tensor.from_numpy_crops(x, np.zeros((0, 4), np.int32), (4, 6), axes=(0, 1))
    assert len(arr) == 0 and arr.type == pa.list_(pa.list_(pa.list_(pa.uint8(), 3), 6), 4)
    # at least as many non-empty boxes as a test that counts on them needs
    kinds = kr.box_kinds(8, 10, (4, 6))
    full = [label for label, row in kinds
            if tensor._numpy_crops(x, [row], (4, 6), (0, 1)).any()]
    assert len(full) == 9 and len(kinds) == 20, full


def plan_raw(fields, n, arr, dev=ARROW_DEVICE_ROCM):
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_crop", fields, n, arr, dev, byref(h))
    _lib.load().dora_gpu_plan_free(h)


def refused(rec, code, *words, dev=ARROW_DEVICE_ROCM, edit=None):
    fields, arr, n, keep = kr.describe(rec, lambda b: PTR)
    if edit:
        edit(fields, arr)
    with pytest.raises(DoraGpuError) as e:
        plan_raw(fields, n, arr, dev)
    assert e.value.code == code, str(e.value)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_refusals(lib):
    INVALID, UNSUPPORTED = -1, -4
    f32 = cr.source("float32", (4, 3))
    rows = [(0, 0, 2, 2), (1, 1, 4, 3)]

    def ok(**kw):
        return kr.crop("float32", (0, 1), (4, 5), rows, "bilinear", "float16", **kw)

    def named(bad_base, c, view=None):  # the offending field second, behind a good one
        return [("good", f32, f32, ok()), ("bad", bad_base, bad_base if view is None else view, c)]

    for dev in (ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
        # a frame of fewer than 2 or more than 7 dimensions
        one = cr.source("float32", (4,))
        refused([(None, one, one, kr.crop("float32", (0, 0), (2, 2), rows))], INVALID,
                "1 dimensions", dev=dev)
        eight = cr.source("uint8", (1, 1, 1, 1, 1, 1, 4, 3))
        refused(named(eight, kr.crop("uint8", (6, 7), (2, 2), rows)), INVALID, "field 1 `bad`",
                "8 dimensions", dev=dev)
        # resize's axis and extent refusals
        for axes in ((2, 0), (0, -1), (7, 1)):
            def axis(fields, arr, axes=axes):
                arr[1].axis[0], arr[1].axis[1] = axes
            refused(named(f32, ok()), INVALID, "field 1 `bad`", "axis", dev=dev, edit=axis)

        def equal(fields, arr):
            arr[1].axis[0] = arr[1].axis[1] = 1
        refused(named(f32, ok()), INVALID, "field 1 `bad`", "same dimension", dev=dev, edit=equal)
        wide = np.broadcast_to(np.zeros((4, 1), np.uint8), (4, 32769))
        refused(named(np.zeros((4, 1), np.uint8), kr.crop("uint8", (0, 1), (4, 4), rows), wide),
                INVALID, "field 1 `bad`", "32769", dev=dev)
        for size in ((0, 3), (4, 32769), (-1, 3)):
            refused(named(f32, kr.crop("float32", (0, 1), size, rows)), INVALID, "field 1 `bad`",
                    str([s for s in size if not 1 <= s <= 32768][0]), dev=dev)
        z = np.zeros((0, 3, 4), np.float32)
        refused(named(z, kr.crop("float32", (1, 2), (2, 2), rows)), INVALID, "field 1 `bad`",
                "extent 0", dev=dev)
        # sources, destinations, mode
        for dt, name in ((np.int32, "int32"), (np.float64, "float64"), (np.bool_, "bool")):
            b = np.zeros((4, 2), dt)
            refused(named(b, kr.crop(name, (0, 1), (4, 2), rows, "nearest", "uint8")), UNSUPPORTED,
                    "field 1 `bad`", name, "source", dev=dev)
        for code, bits, name in ((0, 32, "int32"), (2, 64, "float64"), (4, 16, "bfloat16")):
            def dest(fields, arr, code=code, bits=bits):
                arr[1].dtype_code, arr[1].dtype_bits = code, bits
            refused(named(f32, ok()), UNSUPPORTED, "field 1 `bad`", name, "destination", dev=dev,
                    edit=dest)
        bf = cr.source("bfloat16", (4, 3))
        refused(named(bf, kr.crop("bfloat16", (0, 1), (4, 2), rows)), UNSUPPORTED, "field 1 `bad`",
                "bfloat16", "destination", dev=dev)

        def mode(fields, arr):
            arr[1].mode = 3
        refused(named(f32, ok()), UNSUPPORTED, "field 1 `bad`", "mode 3", dev=dev, edit=mode)

        # the boxes: NULL, not int32, not [K, 4], not dense, misaligned, too many
        def null(fields, arr):
            arr[1].boxes = None
        refused(named(f32, ok()), INVALID, "field 1 `bad`", "boxes is NULL", dev=dev, edit=null)
        for code, bits, word in ((0, 64, "int64"), (1, 32, "uint32"), (2, 32, "float32")):
            def dtype(fields, arr, code=code, bits=bits):
                arr[1].boxes.contents.dtype_code, arr[1].boxes.contents.dtype_bits = code, bits
            refused(named(f32, ok()), INVALID, "field 1 `bad`", "boxes dtype", word, "not int32",
                    dev=dev, edit=dtype)

        def flat(fields, arr):
            arr[1].boxes.contents.ndim = 1
        refused(named(f32, ok()), INVALID, "field 1 `bad`", "[K, 4]", dev=dev, edit=flat)

        def five(fields, arr):
            arr[1].boxes.contents.shape[1] = 5
        refused(named(f32, ok()), INVALID, "field 1 `bad`", "[K, 4]", dev=dev, edit=five)
        for st in ((8, 1), (4, 2), (1, 2)):
            def strided(fields, arr, st=st):
                arr[1].boxes.contents.strides[0], arr[1].boxes.contents.strides[1] = st
            refused(named(f32, ok()), INVALID, "field 1 `bad`", "dense", dev=dev, edit=strided)
        for shift in (1, 2, 3):
            def odd(fields, arr, shift=shift):
                arr[1].boxes.contents.byte_offset += shift
            refused(named(f32, ok()), INVALID, "field 1 `bad`", "boxes", "aligned", dev=dev, edit=odd)

        def many(fields, arr):
            arr[0].boxes.contents.shape[0] = arr[1].boxes.contents.shape[0] = (1 << 20) + 1
        refused(named(f32, ok()), INVALID, "field 0 `good`", "1048577", dev=dev, edit=many)

        def negative(fields, arr):
            arr[1].boxes.contents.shape[0] = -1
        refused(named(f32, ok()), INVALID, "field 1 `bad`", "-1 rows", dev=dev, edit=negative)
        # a frame that does not sit on its element size
        i16 = cr.source("int16", (4, 3))

        def off1(fields, arr):
            fields[1].tensor.byte_offset = 1
        refused(named(i16, kr.crop("int16", (0, 1), (4, 2), rows)), INVALID, "field 1 `bad`",
                "multiple", dev=dev, edit=off1)
    # K of 2^20 itself plans (over made-up pointers: nothing is read)
    fields, arr, n, keep = kr.describe([(None, f32, f32, ok())], lambda b: PTR)
    arr[0].boxes.contents.shape[0] = 1 << 20
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_crop", fields, n, arr, ARROW_DEVICE_ROCM, byref(h))
    assert _lib.load().dora_gpu_plan_size(h) == (1 << 20) * 4 * 5 * 2
    _lib.load().dora_gpu_plan_free(h)
    # a record whose leading extents differ: K against K', K against a plain field's rows
    three = kr.crop("float32", (0, 1), (4, 5), rows + [(0, 0, 1, 1)])
    refused([("a", f32, f32, ok()), ("b", f32, f32, three)], INVALID, "field 1 `b`", "leading extent")
    refused([("a", f32, f32, ok()), ("b", f32, f32, None)], INVALID, "field 1 `b`", "leading extent")
    refused([("a", f32, f32, ok()), ("a", f32, f32[:2], None)], INVALID, "field 1 `a`", "repeats")

    def huge(fields, arr):
        fields[0].tensor.strides[1] = 1 << 61
    refused([(None, f32, f32, ok())], INVALID, "overflows", edit=huge)
    # arguments
    fields, arr, n, keep = kr.describe(named(f32, ok()), lambda b: PTR)
    for args in ((None, n, arr), (fields, 0, arr)):
        with pytest.raises(DoraGpuError) as e:
            plan_raw(*args)
        assert e.value.code == INVALID
    with pytest.raises(DoraGpuError) as e:
        bad = (TensorCrop * 9)()
        bad[0].mode = 1
        plan_raw((_lib.TensorField * 9)(), 9, bad)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(DoraGpuError) as e:
        plan_raw(fields, n, arr, dev=99)
    assert e.value.code == INVALID


def test_python_refusals(lib):
    x = np.zeros((4, 3), np.float32)
    bx = np.zeros((2, 4), np.int32)
    a = tensor.crops(x, bx, (2, 5), dtype="uint8")
    assert a._entry()[:7] == (2, 0, 1, 2, 5, 1, 8) and a._entry()[7] is bx
    assert tensor.crops(x, bx, (2, 5), axes=(1, 0), mode="nearest")._entry()[:7] == (1, 1, 0, 2, 5, 0, 0)
    for make, word in ((lambda v: tensor.ragged(v, lengths=[2]), "ragged"),
                       (lambda v: tensor.take(v, [0]), "take"),
                       (lambda v: tensor.masked(v, [1, 0]), "mask")):
        for v in (a, {"a": a, "b": bx}):
            with pytest.raises(TypeError) as e:
                make(v)
            assert "crops" in str(e.value) and word in str(e.value)
    for inner in (tensor.cast(x, "float16"), tensor.quantize(x, "uint8"), tensor.argmax(x, 0),
                  tensor.resize(x, (2, 2)), tensor.take(x, [0]), tensor.masked(x, [1, 0, 1, 1]),
                  tensor.ragged(x, lengths=[4]), {"a": x}, a):
        with pytest.raises(TypeError) as e:
            tensor.crops(inner, bx, (2, 2))
        assert "crops" in str(e.value)
    for outer in (lambda v: tensor.cast(v, "float32"), lambda v: tensor.quantize(v, "uint8"),
                  lambda v: tensor.argmax(v, 0), lambda v: tensor.resize(v, (2, 2))):
        with pytest.raises(TypeError) as e:
            outer(a)
        assert "crops" in str(e.value)
    with pytest.raises(ValueError) as e:
        tensor.crops(x, bx, (2, 2), mode="bicubic")
    assert "crops:" in str(e.value)
    for bad in ((2,), (1, 2, 3), 4):
        with pytest.raises(TypeError):
            tensor.crops(x, bx, bad)
    with pytest.raises(TypeError):
        tensor.crops(x, bx, (2, 2), axes=(0,))
    with pytest.raises(TypeError):
        tensor.crops(3.0, bx, (2, 2))
    with pytest.raises(TypeError):
        tensor.crops(x, 7, (2, 2))
    assert set(("Crops", "crops", "from_numpy_crops")) <= set(tensor.__all__)
