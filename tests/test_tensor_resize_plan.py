"""Planning of resize messages on the CPU (no GPU): dora_gpu_plan_tensor_resize over made-up device
pointers (planning calls nothing in HIP and reads no tensor byte) and over real numpy memory.
Size, type info and leaf offsets are the reference packing's of the materialised resized tensors
(oracle.pack_ref); a device plan with a resized field has no segments, the launch kind of
gather_resize_kernel and per field the reach of its whole source view; entries that are all mode 0
plan exactly as the plain tensor or record; every refusal with its code, naming the field; the
Python TypeErrors; and the statement itself against a float64 evaluation with exact weights."""
import ctypes
from ctypes import byref, c_int, c_void_p
from fractions import Fraction

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST,
                           DoraGpuError, TensorResize)
from tests import cast_records as cr
from tests import resize_records as rr
from tests import struct_records as sr

PTR = 0x7E00_0000_0000  # never dereferenced


def fake_ptrs(rec):
    bases = rr.bases_of(rec)
    return lambda b: PTR + (1 << 26) * next(i for i, x in enumerate(bases) if x is b)


def host_ptr(b):
    return b.__array_interface__["data"][0]


def launch_of(p):
    launch, scan, checked = c_int(), c_int(), c_int()
    _lib.call("dora_gpu_test_plan_launch", p.handle, byref(launch), byref(scan), byref(checked))
    return launch.value, scan.value, checked.value


def test_device_plans_of_every_case(lib):
    """No segments, launch kind 7, the oracle's size, type info and offsets, and per field the
    reach numpy's strides give over the whole source view."""
    paths = set()
    for label, rec, offsets in rr.cases():
        sample, info, ranges = rr.oracle(rec)
        ptr_of = fake_ptrs(rec)
        with rr.plan_resize(rec, ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample), label
            assert p.type_info().to_json() == info.to_json(), label
            assert p.segments() == [] and launch_of(p) == (7, 0, 1), label
            for mis in offsets:
                fs, ks = sr.plan_fields(p), rr.plan_resizes(p, len(rec), 4096 + mis)
                assert [(f["off"], f["bytes"]) for f in fs] == ranges, label
                for (_, b, v, r), f, k in zip(rec, fs, ks):
                    assert f["src"] == ptr_of(b) + host_ptr(v) - host_ptr(b), label
                    assert f["elem"] == v.itemsize, label
                    assert (f["lo"], f["hi"]) == cr.reach(b, v), label
                    off = host_ptr(v) - host_ptr(b)
                    assert off + f["lo"] >= 0 and off + f["hi"] < b.nbytes, label
                    if r is None:
                        assert k["mode"] == 0 and k["count"] == 0, label
                        continue
                    a = [x % v.ndim for x in r["axes"]]
                    bits = rr.DESTS[rr.dst_name(r)][1]
                    count = v.size // (v.shape[a[0]] * v.shape[a[1]]) * r["size"][0] * r["size"][1]
                    e = 128 // bits
                    assert k["mode"] == rr.MODES[r["mode"]] and k["count"] == count, label
                    assert k["bits"] == bits and k["out"] == r["size"], label
                    assert k["in"] == (v.shape[a[0]], v.shape[a[1]]), label
                    assert k["stride"] == (v.strides[a[0]], v.strides[a[1]]), label
                    assert k["head"] + e * k["units"] + k["tail"] == count, label
                    assert k["head"] < e and k["tail"] < e, label
                    if k["units"] or k["head"] == 0:
                        assert (4096 + mis + f["off"] + k["head"] * bits // 8) % 16 == 0, label
                    paths |= {n for n in ("head", "units", "tail") if k[n]}
    assert paths == {"head", "units", "tail"}


def test_no_resize_plans_as_the_plain_entry(lib):
    """`resizes` NULL or every mode 0: dora_gpu_plan_tensor's plan (bare) or
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
                    fields, arr, n, keep2 = rr.describe([(None, b, v, None)], ptr_of)
                    h = c_void_p()
                    _lib.call("dora_gpu_plan_tensor_resize", fields, n, None if null else arr, dev,
                              byref(h))
                    with Plan(h.value, keep2) as p:
                        assert p.size == plain.size
                        assert p.type_info_bytes() == plain.type_info_bytes()
                        assert launch_of(p) == launch_of(plain)
                        if dev == ARROW_DEVICE_ROCM or v is b:
                            assert p.segments() == plain.segments()
            rec = [("a", b, v, None), ("n", b, b[:, 0], None)]
            with rr.plan_resize(rec, ptr_of, dev) as p, \
                    sr.plan_record([r[:3] for r in rec], ptr_of, dev) as plain:
                assert p.size == plain.size and p.type_info_bytes() == plain.type_info_bytes()
                assert launch_of(p) == launch_of(plain)
                if dev == ARROW_DEVICE_ROCM:
                    assert p.segments() == plain.segments()
                    assert sr.plan_fields(p) == sr.plan_fields(plain)
    # the plain entries' refusals pass through: bfloat16 without a resize
    fields, arr, n, keep = rr.describe([(None, b, b, None)], lambda x: PTR)
    fields[0].tensor.dtype_code, fields[0].tensor.dtype_bits = 4, 16
    with pytest.raises(DoraGpuError) as e:
        _lib.call("dora_gpu_plan_tensor_resize", fields, n, arr, ARROW_DEVICE_ROCM, byref(c_void_p()))
    assert e.value.code == -4 and "Arrow has no bfloat16" in str(e.value)


def test_empty_kept_leading_dimension(lib):
    e = np.zeros((0, 3, 4), np.float32)
    for rec in ([(None, e, e, rr.rs("float32", (1, 2), (5, 6), "bilinear", "uint8"))],
                [("a", e, e, rr.rs("float32", (-2, -1), (2, 2))), ("b", e, e, None)]):
        sample, info, _ = rr.oracle(rec)
        for dev in (ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU):
            with rr.plan_resize(rec, lambda b: PTR, dev) as p:
                assert p.size == 0 == len(sample) and p.segments() == []
                assert p.type_info().to_json() == info.to_json()
                assert launch_of(p)[0] == 0


def test_host_plans_resize_inside_the_call(lib):
    """Host values, pageable and pinned alike: one staged segment per resized field holding the
    resized bytes on return; a plain dense field is read in place."""
    for label, rec, _ in rr.cases():
        sample, info, ranges = rr.oracle(rec)
        for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
            with rr.plan_resize(rec, host_ptr, dev) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), label
                assert launch_of(p) == (0, 0, 0), label
                segs = p.segments()
                assert [(s[1], s[2]) for s in segs] == ranges, label
                for (ptr, off, n), (_, _, v, r) in zip(segs, rec):
                    rr.same(ctypes.string_at(ptr, n), rr.want(v, r), label)


def plan_raw(fields, n, arr, dev=ARROW_DEVICE_ROCM):
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_resize", fields, n, arr, dev, byref(h))
    _lib.load().dora_gpu_plan_free(h)


def refused(rec, code, *words, dev=ARROW_DEVICE_ROCM, edit=None):
    fields, arr, n, keep = rr.describe(rec, lambda b: PTR)
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
    ok = rr.rs("float32", (0, 1), (4, 5), "bilinear", "float16")

    def named(bad_base, r, view=None):  # the offending field second, behind a good one
        return [("good", f32, f32, ok), ("bad", bad_base, bad_base if view is None else view, r)]

    for dev in (ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
        # fewer than two dimensions
        one = cr.source("float32", (4,))
        refused([(None, one, one, rr.rs("float32", (0, 0), (2, 2)))], INVALID, "1 dimensions", dev=dev)
        # an axis outside the dimensions, the two axes equal
        for axes in ((2, 0), (0, -1), (7, 1)):
            def axis(fields, arr, axes=axes):
                arr[1].axis[0], arr[1].axis[1] = axes
            refused(named(f32, ok), INVALID, "field 1 `bad`", "axis", dev=dev, edit=axis)

        def equal(fields, arr):
            arr[1].axis[0] = arr[1].axis[1] = 1
        refused(named(f32, ok), INVALID, "field 1 `bad`", "same dimension", dev=dev, edit=equal)
        # I or O outside [1, 32768]
        wide = np.broadcast_to(np.zeros((4, 1), np.uint8), (4, 32769))
        refused(named(np.zeros((4, 1), np.uint8), rr.rs("uint8", (0, 1), (4, 4)), wide), INVALID,
                "field 1 `bad`", "32769", dev=dev)
        z = np.zeros((0, 3), np.float32)  # (the leading extents differ too: the resize is refused first)
        refused(named(z, rr.rs("float32", (0, 1), (4, 3))), INVALID, "field 1 `bad`", "extent 0", dev=dev)
        for size in ((0, 3), (4, 32769), (-1, 3)):
            refused(named(f32, rr.rs("float32", (0, 1), size)), INVALID, "field 1 `bad`",
                    str([s for s in size if not 1 <= s <= 32768][0]), dev=dev)
        # sources that are none of the seven
        for dt, name in ((np.int32, "int32"), (np.int64, "int64"), (np.float64, "float64"),
                         (np.uint32, "uint32"), (np.bool_, "bool")):
            b = np.zeros((4, 2), dt)
            refused(named(b, rr.rs(name, (0, 1), (4, 2), "nearest", "uint8")), UNSUPPORTED,
                    "field 1 `bad`", name, "resize source", dev=dev)
        # destinations that are none of the six
        for code, bits, name in ((0, 32, "int32"), (1, 32, "uint32"), (1, 64, "uint64"),
                                 (2, 64, "float64"), (4, 16, "bfloat16")):
            def dest(fields, arr, code=code, bits=bits):
                arr[1].dtype_code, arr[1].dtype_bits = code, bits
            refused(named(f32, ok), UNSUPPORTED, "field 1 `bad`", name, "destination", dev=dev,
                    edit=dest)
        # a bfloat16 source without a destination
        bf = cr.source("bfloat16", (4, 3))
        refused(named(bf, rr.rs("bfloat16", (0, 1), (4, 2))), UNSUPPORTED, "field 1 `bad`",
                "bfloat16", "destination", dev=dev)
        # another mode
        def mode(fields, arr):
            arr[1].mode = 3
        refused(named(f32, ok), UNSUPPORTED, "field 1 `bad`", "mode 3", dev=dev, edit=mode)
        # a source that does not sit on its element size
        i16 = cr.source("int16", (4, 3))

        def odd(fields, arr):
            fields[1].tensor.byte_offset = 1
        refused(named(i16, rr.rs("int16", (0, 1), (4, 2))), INVALID, "field 1 `bad`", "multiple",
                dev=dev, edit=odd)
    # the fields share the leading extent of their output shapes
    refused([("a", f32, f32, ok), ("b", f32, f32, rr.rs("float32", (0, 1), (5, 3)))], INVALID,
            "field 1 `b`", "leading extent")
    t = cr.source("float32", (3, 4))
    rec = [("a", f32, f32, ok), ("b", t, t, rr.rs("float32", (0, 1), (4, 2)))]  # (4, 5) and (4, 2)
    with rr.plan_resize(rec, lambda b: PTR, ARROW_DEVICE_ROCM) as p:
        assert p.type_info().to_json() == rr.oracle(rec)[1].to_json()
    refused([("a", f32, f32, ok), ("a", f32, f32, None)], INVALID, "field 1 `a`", "repeats")
    # reach overflow
    def huge(fields, arr):
        fields[0].tensor.strides[1] = 1 << 61
    refused([(None, f32, f32, ok)], INVALID, "overflows", edit=huge)
    # arguments
    fields, arr, n, keep = rr.describe(named(f32, ok), lambda b: PTR)
    for args in ((None, n, arr), (fields, 0, arr)):
        with pytest.raises(DoraGpuError) as e:
            plan_raw(*args)
        assert e.value.code == INVALID
    with pytest.raises(DoraGpuError) as e:
        bad = (TensorResize * 9)()
        bad[0].mode = 1
        plan_raw((_lib.TensorField * 9)(), 9, bad)
    assert e.value.code == UNSUPPORTED
    with pytest.raises(DoraGpuError) as e:
        plan_raw(fields, n, arr, dev=99)
    assert e.value.code == INVALID


def test_python_refusals(lib):
    x = np.zeros((4, 3), np.float32)
    a = tensor.resize(x, (2, 5), mode="bilinear", dtype="uint8")
    assert a._entry() == (2, 0, 1, 2, 5, 1, 8)
    assert tensor.resize(x, (2, 5), axes=(1, 0))._entry() == (1, 1, 0, 2, 5, 0, 0)
    assert tensor.resize(np.zeros((2, 3, 4)), (9, 9), axes=(0, -1), dtype=np.float16)._entry() == \
        (1, 0, 2, 9, 9, 2, 16)
    for make, word in ((lambda v: tensor.ragged(v, lengths=[4]), "ragged"),
                       (lambda v: tensor.take(v, [0]), "take"),
                       (lambda v: tensor.masked(v, [1, 0, 1, 1]), "mask")):
        for v in (a, {"a": a, "b": x}):
            with pytest.raises(TypeError) as e:
                make(v)
            assert "resize" in str(e.value) and word in str(e.value)
    for inner in (tensor.cast(x, "float16"), tensor.quantize(x, "uint8"), tensor.argmax(x, 0),
                  tensor.take(x, [0]), tensor.masked(x, [1, 0, 1, 1]), tensor.ragged(x, lengths=[4]),
                  {"a": x}, a):
        with pytest.raises(TypeError) as e:
            tensor.resize(inner, (2, 2))
        assert "resize" in str(e.value)
    for outer in (lambda v: tensor.cast(v, "float32"), lambda v: tensor.quantize(v, "uint8"),
                  lambda v: tensor.argmax(v, 0)):
        with pytest.raises(TypeError) as e:
            outer(a)
        assert "resize" in str(e.value)
    with pytest.raises(ValueError):
        tensor.resize(x, (2, 2), mode="bicubic")
    for bad in ((2,), (1, 2, 3), 4):
        with pytest.raises(TypeError):
            tensor.resize(x, bad)
    with pytest.raises(TypeError):
        tensor.resize(x, (2, 2), axes=(0,))
    with pytest.raises(TypeError):
        tensor.resize(3.0, (2, 2))
    assert set(("Resized", "resize", "from_numpy_resize")) <= set(tensor.__all__)
    import pyarrow as pa
    got = tensor.from_numpy_resize(rr.ties_u8(), (2, 4), axes=(0, 1), mode="bilinear")
    assert got.type == pa.list_(pa.uint8(), 4)
    assert got.to_pylist() == [[0, 254, 2, 2], [255, 0, 4, 4]]
    with pytest.raises(ValueError):
        tensor.from_numpy_resize(np.zeros((2, 2), np.uint16), (1, 1), bfloat16=True)


def exact(x, axes, size):
    """The bilinear statement in exact rational arithmetic over float64-exact sources."""
    a, b = axes
    xs = np.moveaxis(x, (a, b), (0, 1))

    def taps(n_in, n_out, o):
        d = 2 * n_out
        n = max((2 * o + 1) * n_in - n_out, 0)
        q = n // d
        if q >= n_in - 1:
            return n_in - 1, n_in - 1, Fraction(1), Fraction(0)
        r = n % d
        return q, q + 1, Fraction(d - r, d), Fraction(r, d)
    out = np.empty((size[0], size[1]) + xs.shape[2:], object)
    for oa in range(size[0]):
        a0, a1, wa0, wa1 = taps(xs.shape[0], size[0], oa)
        for ob in range(size[1]):
            b0, b1, wb0, wb1 = taps(xs.shape[1], size[1], ob)
            for rest in np.ndindex(*xs.shape[2:]):
                v = [[Fraction(float(xs[(i, j) + rest])) for j in (b0, b1)] for i in (a0, a1)]
                out[(oa, ob) + rest] = (v[0][0] * wb0 + v[0][1] * wb1) * wa0 + \
                                       (v[1][0] * wb0 + v[1][1] * wb1) * wa1
    return np.moveaxis(out, (0, 1), (a, b))


def test_the_statement_against_exact_weights(lib):
    """|y - exact| <= 8 * 2^-24 * max|x|: three roundings per blend level over two levels plus
    one per weight stay under 8 units; identity sizes return the source exactly."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for shape, axes, size in (((7, 9, 3), (0, 1), (5, 4)), ((13, 17), (0, 1), (13, 6)),
                              ((5, 6, 2), (0, 1), (11, 13)), ((2, 12, 16), (2, 1), (5, 5)),
                              ((33, 31), (1, 0), (64, 16))):
        x = (rng.standard_normal(shape) * 100).astype(np.float32)
        got = tensor._numpy_resize(x, size, axes, "bilinear")
        assert got.dtype == np.float32
        want = exact(x, axes, size)
        unit = Fraction(float(np.abs(x).max())) / 2 ** 24
        err = max(abs(Fraction(float(g)) - w) / unit for g, w in zip(got.ravel(), want.ravel()))
        print(shape, axes, size, "worst error", float(err), "units of 2^-24 * max|x|")
        worst = max(worst, float(err))
        assert err <= 8, (shape, float(err))
        assert np.array_equal(tensor._numpy_resize(x, (shape[axes[0]], shape[axes[1]]), axes, "bilinear"), x)
        for src in ("uint8", "int16", "float16"):
            y = cr.source(src, shape, seed=3)
            same_size = (shape[axes[0]], shape[axes[1]])
            for mode in ("nearest", "bilinear"):
                assert tensor._numpy_resize(y, same_size, axes, mode).tobytes() == y.tobytes()
    print("worst of all", worst)
