"""Planning of model-input messages on the CPU (no GPU): dora_gpu_plan_tensor_prep over made-up
device pointers (planning calls nothing in HIP and reads no tensor byte) and over real numpy
memory.  Size, type info and leaf offsets are the reference packing's of the materialised tensors
(oracle.pack_ref) and never depend on a prep entry; a device plan with a prep entry has no
segments, the launch kind of gather_resize_prep_kernel or gather_crop_prep_kernel and per field
its tables' reach; a host plan holds the statement's bytes; entries that are all zero plan exactly
as dora_gpu_plan_tensor_resize / _crop; every refusal with its code, naming the field or the
table; `tensor.letterbox`'s geometry; and the Python TypeErrors."""
import ctypes
from ctypes import byref, c_int, c_void_p
from fractions import Fraction
from math import floor

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST,
                           DoraGpuError)
from tests import cast_records as cr
from tests import crop_records as kr
from tests import prep_records as pr
from tests import resize_records as rr
from tests import struct_records as sr
from tests.test_tensor_prep_host import oracle

PTR = 0x7E00_0000_0000  # never dereferenced


def fake_ptrs(rec):
    bases = pr.bases_of(rec)
    return lambda b: PTR + (1 << 26) * next(i for i, x in enumerate(bases) if x is b)


def host_ptr(b):
    return b.__array_interface__["data"][0]


def launch_of(p):
    launch, scan, checked = c_int(), c_int(), c_int()
    _lib.call("dora_gpu_test_plan_launch", p.handle, byref(launch), byref(scan), byref(checked))
    return launch.value, scan.value, checked.value


def test_device_plans_of_every_case(lib):
    """No segments, launch kind 9 (resize) or 10 (crops), the oracle's size, type info and
    offsets, and per field the tables, their reach and the placement as given."""
    sizes = {}
    for label, rec, offsets in pr.cases() + pr.limit_cases():
        sample, info, ranges = oracle(rec)
        ptr_of = fake_ptrs(rec)
        crops = any(c and "boxes" in c for _, _, _, c in rec)
        with pr.plan_prep(rec, ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample), label
            assert p.type_info().to_json() == info.to_json(), label
            assert p.segments() == [] and launch_of(p) == (10 if crops else 9, 0, 1), label
            fs, ps = sr.plan_fields(p), pr.plan_preps(p, len(rec))
            assert [(f["off"], f["bytes"]) for f in fs] == ranges, label
            for (_, b, v, c), d in zip(rec, ps):
                q = (c or {}).get("prep")
                assert d["on"] == bool(q), label
                if not q:
                    continue
                for w in ("scale", "bias"):
                    if pr.is_table(q[w]):
                        tb, tv = q[w]
                        assert d[w + "_table"] == ptr_of(tb) + host_ptr(tv) - host_ptr(tb), label
                        # tight: the reach ends with the table's base
                        assert (d["lo"], d["hi"]) == (0, tv.nbytes - 1), label
                        assert host_ptr(tv) - host_ptr(tb) + d["hi"] + 1 == tb.nbytes, label
                        assert d["channels"] == len(tv), label
                        assert d["axis"] == q["axis"] % v.ndim + crops, label
                    else:
                        assert d[w + "_table"] == 0, label
                if q["inner"] is not None:
                    assert (d["inner"], d["lead"]) == (tuple(q["inner"]), tuple(q["lead"] or (0, 0))), label
                    assert np.float32(d["fill"]).tobytes() == np.float32(q["fill"]).tobytes(), label
                else:
                    assert (d["inner"], d["lead"], d["fill"]) == ((0, 0), (0, 0), 0.0), label
        op = next(c for _, _, _, c in rec if c)
        sizes.setdefault(pr.DESTS[pr.dst_name(op)][1] // 8, set()).update(offsets)
    # every element size is packed at 0 and at two or more other offsets mod 16
    assert set(sizes) == {1, 2, 4}
    for size, offs in sizes.items():
        assert 0 in offs and len(offs - {0}) >= 2 and all(o % size == 0 for o in offs), (size, offs)


def test_host_plans_prepare_inside_the_call(lib):
    """Host values, pageable and pinned alike: one staged segment per field with an op holding the
    statement's bytes, tables and boxes read inside the call."""
    for label, rec, _ in pr.cases() + pr.limit_cases():
        sample, info, ranges = oracle(rec)
        for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
            with pr.plan_prep(rec, host_ptr, dev) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), label
                assert launch_of(p) == (0, 0, 0), label
                segs = p.segments()
                assert [(s[1], s[2]) for s in segs] == ranges, label
                for (ptr, off, n), (_, _, v, c) in zip(segs, rec):
                    pr.same(ctypes.string_at(ptr, n), pr.want(v, c), label)


def test_all_zero_entries_plan_as_the_resize_or_the_crops(lib):
    """`preps` NULL or all zero: size, type info, launch kind and fields of
    dora_gpu_plan_tensor_resize / _crop, a non-zero `fill` alone included."""
    b = cr.source("uint8", (7, 9, 3), seed=1)
    recs = [([(None, b, b, pr.resized("uint8", (0, 1), (5, 4), "bilinear", "float16"))], rr.plan_resize, 7),
            (rr.cases()[-1][1], rr.plan_resize, 7),
            ([(None, b, b, pr.cropped("uint8", (0, 1), (5, 4), kr.THREE))], kr.plan_crop, 8),
            (kr.record(), kr.plan_crop, 8)]
    for rec, plain_plan, kind in recs:
        ptr_of = fake_ptrs(rec)
        for dev in (ARROW_DEVICE_ROCM, ARROW_DEVICE_CPU):
            for preps in ("null", "zero", "fill"):
                fields, rarr, carr, parr, n, keep = pr.describe(rec, ptr_of if dev == ARROW_DEVICE_ROCM else host_ptr)
                if preps == "fill":
                    parr[0].fill = 7.0
                h = c_void_p()
                _lib.call("dora_gpu_plan_tensor_prep", fields, n, rarr, carr,
                          None if preps == "null" else parr, dev, byref(h))
                from dora_amd.arrow_utils import Plan
                with Plan(h.value, keep) as p, \
                        plain_plan(rec, ptr_of if dev == ARROW_DEVICE_ROCM else host_ptr, dev) as plain:
                    assert p.size == plain.size and p.type_info_bytes() == plain.type_info_bytes()
                    assert launch_of(p) == launch_of(plain)
                    assert launch_of(p)[0] == (kind if dev == ARROW_DEVICE_ROCM else 0)
                    if dev == ARROW_DEVICE_ROCM:
                        assert sr.plan_fields(p) == sr.plan_fields(plain)
                        assert not any(d["on"] for d in pr.plan_preps(p, n))
                    else:
                        assert [(s[1], s[2]) for s in p.segments()] == [(s[1], s[2]) for s in plain.segments()]
                        for s, t in zip(p.segments(), plain.segments()):
                            assert ctypes.string_at(s[0], s[2]) == ctypes.string_at(t[0], t[2])


def refused(rec, edit=None, dev=ARROW_DEVICE_ROCM, both=False):
    """The DoraGpuError of planning `rec` after `edit(fields, rarr, carr, parr)`."""
    ptr_of = fake_ptrs(rec) if dev == ARROW_DEVICE_ROCM else host_ptr
    fields, rarr, carr, parr, n, keep = pr.describe(rec, ptr_of)
    extra = None
    if edit:
        extra = edit(fields, rarr, carr, parr)
    if both:  # an active resize entry beside the crops
        from dora_amd._lib import TensorResize
        rarr = (TensorResize * n)()
        rarr[0].mode, rarr[0].axis[1], rarr[0].size[0], rarr[0].size[1] = 1, 1, 2, 2
    h = c_void_p()
    with pytest.raises(DoraGpuError) as e:
        _lib.call("dora_gpu_plan_tensor_prep", fields, n, rarr, carr, parr, dev, byref(h))
    del extra, keep
    return e.value


def test_refusals(lib):
    b = cr.source("uint8", (7, 9, 3), seed=2)
    s3, b3 = pr.norm_tables()

    def rec_of(**kw):
        return [("a", b, b, None),
                ("img", b, b, pr.resized("uint8", (0, 1), (7, 4), "bilinear", "float16", **kw))]
    base = dict(scale=s3, bias=b3, axis=2)

    def table_edit(which, fn):
        def edit(fields, rarr, carr, parr):
            t = (parr[1].scale if which == "scale" else parr[1].bias).contents
            return fn(t)
        return edit

    def setattrs(**kw):
        def fn(t):
            keep = []
            for k, v in kw.items():
                if k in ("shape", "strides"):
                    arr = (ctypes.c_int64 * len(v))(*v)
                    keep.append(arr)
                    setattr(t, k, arr)
                else:
                    setattr(t, k, v)
            return keep
        return fn
    cases = [
        # a prep entry on a field that is neither resized nor crops
        (rec_of(**base), lambda f, r, c, p: setattr(p[0], "has_bias", 1), -1, ("field 0 `a`", "neither resized nor crops")),
        # axis outside the dimensions, or a resized axis
        (rec_of(scale=s3, axis=3), None, -1, ("field 1 `img`", "axis 3", "outside")),
        (rec_of(scale=s3, axis=2), lambda f, r, c, p: setattr(p[1], "axis", -1), -1, ("field 1 `img`", "axis -1")),
        (rec_of(scale=s3, axis=2), lambda f, r, c, p: setattr(p[1], "axis", 1), -1, ("field 1 `img`", "resized axes")),
        # a table together with its scalar
        (rec_of(**base), lambda f, r, c, p: setattr(p[1], "has_scale", 1), -1, ("field 1 `img`", "scale table together")),
        (rec_of(**base), lambda f, r, c, p: setattr(p[1], "has_bias", 1), -1, ("field 1 `img`", "bias table together")),
        # tables: not 1-D, not shape[axis] long, not dense, not aligned, not float32
        (rec_of(**base), table_edit("scale", setattrs(ndim=2, shape=(3, 1))), -1, ("field 1 `img`", "scale table", "dimensions")),
        (rec_of(**base), table_edit("bias", setattrs(shape=(4,))), -1, ("field 1 `img`", "bias table", "4 elements")),
        (rec_of(**base), table_edit("scale", setattrs(strides=(2,))), -1, ("field 1 `img`", "scale table", "dense")),
        (rec_of(**base), table_edit("bias", setattrs(byte_offset=14)), -1, ("field 1 `img`", "bias table", "multiple of 4")),
        (rec_of(**base), table_edit("scale", setattrs(dtype_bits=16)), -4, ("field 1 `img`", "scale table", "float16")),
        (rec_of(**base), table_edit("bias", setattrs(dtype_code=0)), -4, ("field 1 `img`", "bias table", "int32")),
        # scalars and fill that are not finite
        (rec_of(scale=float("inf")), None, -1, ("field 1 `img`", "scale", "not finite")),
        (rec_of(bias=float("nan")), None, -1, ("field 1 `img`", "bias", "not finite")),
        (rec_of(inner=(3, 3), lead=(0, 0), fill=float("inf")), None, -1, ("field 1 `img`", "fill", "not finite")),
        # inner / lead out of range
        (rec_of(inner=(8, 3), lead=(0, 0)), None, -1, ("field 1 `img`", "inner[0] 8", "[1, 7]")),
        (rec_of(inner=(3, 0), lead=(0, 0)), None, -1, ("field 1 `img`", "inner[1] 0")),
        (rec_of(inner=(3, 3), lead=(5, 0)), None, -1, ("field 1 `img`", "lead[0] 5", "[0, 4]")),
        (rec_of(inner=(3, 3), lead=(0, -1)), None, -1, ("field 1 `img`", "lead[1] -1")),
        (rec_of(bias=1.0), lambda f, r, c, p: p[1].lead.__setitem__(1, 1), -1, ("field 1 `img`", "inner[0] 0")),
    ]
    for rec, edit, code, words in cases:
        e = refused(rec, edit)
        assert e.code == code and all(w in str(e) for w in words), (str(e), words)
    # a host table value that is not finite (device tables are never read)
    bad = pr.table([1.0, np.inf, 2.0])
    e = refused(rec_of(scale=bad, axis=2), dev=ARROW_DEVICE_CPU)
    assert e.code == -1 and "scale table" in str(e) and "value 1" in str(e) and "field 1 `img`" in str(e)
    with pr.plan_prep(rec_of(scale=bad, axis=2), fake_ptrs(rec_of(scale=bad, axis=2)), ARROW_DEVICE_ROCM) as p:
        assert launch_of(p)[0] == 9
    # crops: inner on a crops field; resize entries and crops entries both active
    crec = [("crop", b, b, pr.cropped("uint8", (0, 1), (4, 4), kr.THREE, scale=0.5)),
            ("box", np.zeros((3, 4), np.int32), np.zeros((3, 4), np.int32), None)]

    def place(f, r, c, p):
        p[0].inner[0], p[0].inner[1] = 2, 2
    e = refused(crec, place)
    assert e.code == -1 and "field 0 `crop`" in str(e) and "placement for crops is not provided" in str(e)
    e = refused(crec, both=True)
    assert e.code == -1 and "both active" in str(e)
    # the resize's own refusals come first
    e = refused(rec_of(**base), lambda f, r, c, p: r[1].axis.__setitem__(1, 0))
    assert e.code == -1 and "same dimension" in str(e)


def test_letterbox_geometry():
    assert tensor.letterbox((1080, 1920), (640, 640)) == ((360, 640), (140, 0))
    assert tensor.letterbox((1080, 1920), (640, 640), "start") == ((360, 640), (0, 0))
    assert tensor.letterbox((1920, 1080), (640, 640)) == ((640, 360), (0, 140))
    assert tensor.letterbox((11, 17), (16, 16)) == ((10, 16), (3, 0))
    # square to square; size smaller than the source; one source extent 1 (never below 1 step)
    assert tensor.letterbox((5, 5), (9, 9)) == ((9, 9), (0, 0))
    assert tensor.letterbox((100, 50), (10, 10)) == ((10, 5), (0, 2))
    assert tensor.letterbox((1, 1000), (8, 8)) == ((1, 8), (3, 0))
    assert tensor.letterbox((1000, 1), (8, 8)) == ((8, 1), (0, 3))
    assert tensor.letterbox((1, 1), (3, 7)) == ((3, 3), (0, 2))
    # the inner extents lie inside the output and one of them fills it, whatever the extents
    rng = np.random.default_rng(5)
    for ia, ib, oa, ob in rng.integers(1, 2000, (200, 4)).tolist():
        (ra, rb), (pa, pb) = tensor.letterbox((ia, ib), (oa, ob))
        assert 1 <= ra <= oa and 1 <= rb <= ob and (ra == oa or rb == ob)
        assert 0 <= pa <= oa - ra and 0 <= pb <= ob - rb
        # the free extent is the exact quotient rounded half up, held to [1, O]
        if oa * ib <= ob * ia:
            assert ra == oa and rb == min(max(floor(Fraction(ib * oa, ia) + Fraction(1, 2)), 1), ob)
        else:
            assert rb == ob and ra == min(max(floor(Fraction(ia * ob, ib) + Fraction(1, 2)), 1), oa)
    with pytest.raises(ValueError):
        tensor.letterbox((0, 5), (4, 4))
    with pytest.raises(ValueError):
        tensor.letterbox((5, 5), (4, 4), "end")
    with pytest.raises(TypeError):
        tensor.letterbox((5,), (4, 4))


def test_python_interface(lib):
    x = cr.source("uint8", (11, 17, 3), seed=3)
    r = tensor.resize(x, (16, 16), axes=(0, 1), fit="letterbox", fill=114, scale=[1, 2, 3], axis=-1)
    assert (r.inner, r.lead, r.fill, r.axis) == ((10, 16), (3, 0), 114.0, 2)
    assert r._prep()[2:] == (2, None, None, 10, 16, 3, 0, 114.0)
    assert tensor.resize(x, (16, 16), axes=(0, 1))._prep() is None
    assert tensor.crops(x, [[0, 0, 4, 4]], (4, 4), axes=(0, 1))._prep() is None
    assert tensor.crops(x, [[0, 0, 4, 4]], (4, 4), axes=(0, 1), bias=2)._prep()[:5] == (None, None, 0, None, 2.0)
    for kw in (dict(inner=(2, 2)), dict(fit="letterbox"), dict(fill=1.0), dict(lead=(0, 0))):
        with pytest.raises(TypeError, match="placement for crops is not provided"):
            tensor.crops(x, [[0, 0, 4, 4]], (4, 4), axes=(0, 1), **kw)
        with pytest.raises(TypeError, match="placement for crops is not provided"):
            tensor.from_numpy_crops(x, [[0, 0, 4, 4]], (4, 4), axes=(0, 1), **kw)
    with pytest.raises(TypeError, match="give either"):
        tensor.resize(x, (16, 16), axes=(0, 1), fit="letterbox", inner=(10, 16))
    with pytest.raises(TypeError, match="axis="):
        tensor.resize(x, (16, 16), axes=(0, 1), scale=[1, 2, 3])
    with pytest.raises(TypeError, match="axis="):
        tensor.crops(x, [[0, 0, 4, 4]], (4, 4), axes=(0, 1), bias=[1, 2, 3])
    with pytest.raises(TypeError, match="inner="):
        tensor.resize(x, (16, 16), axes=(0, 1), lead=(1, 1))
    with pytest.raises(ValueError, match="fit"):
        tensor.resize(x, (16, 16), axes=(0, 1), fit="pad")
    with pytest.raises(TypeError, match="not offered"):
        tensor.cast(r, "float16")
    # the statement: without the new arguments exactly what it was; padding through the step
    plain = tensor._numpy_resize(x, (16, 16), (0, 1), "bilinear", "float16")
    assert tensor._numpy_resize(x, (16, 16), (0, 1), "bilinear", "float16", inner=(16, 16)).tobytes() == plain.tobytes()
    y = tensor._numpy_resize(x, (16, 16), (0, 1), "bilinear", "float32", scale=[0.5, 1, 2], bias=1.0, axis=2,
                             inner=(10, 16), lead=(3, 0), fill=114.0)
    assert (y[:3] == np.float32([58, 115, 229])).all() and (y[13:] == np.float32([58, 115, 229])).all()
    inner = tensor._numpy_resize(x, (10, 16), (0, 1), "bilinear", "float32", scale=[0.5, 1, 2], bias=1.0, axis=2)
    assert y[3:13].tobytes() == inner.tobytes()
    z = tensor._numpy_crops(x, [[0, 0, 0, 0], [1, 1, 5, 9]], (4, 4), (0, 1), "bilinear", "float32", bias=5.0)
    assert not z[0].any() and (z[1] >= 5).all()
    for bad in (dict(axis=0, scale=[1] * 11), dict(inner=(17, 1)), dict(inner=(4, 4), lead=(13, 0)),
                dict(inner=(4, 4), fill=float("nan")), dict(scale=[1, 2], axis=2)):
        with pytest.raises(ValueError):
            tensor._numpy_resize(x, (16, 16), (0, 1), "bilinear", "float32", **bad)
