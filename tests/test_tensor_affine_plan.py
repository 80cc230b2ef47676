"""Planning of affine messages on the CPU (no GPU): dora_gpu_plan_tensor_affine over made-up
device pointers and over host memory.  Every refusal of the C entry, naming the field, and of the
Python interface; calls whose affine entries are NULL or all zero plan byte for byte as
dora_gpu_plan_tensor_convert does (size, type info, segments, launch kind); a device plan with a
table is kCast with no segments and reports each table's reach; host plans convert inside the call,
bit-exact against `tensor.from_numpy_cast` / `tensor.from_numpy_quantize`; the wire form never
depends on the affine step; an empty message launches nothing."""
import ctypes
from ctypes import byref, c_int, c_void_p, pointer

import numpy as np
import pytest

from dora_amd import _lib, tensor
from dora_amd._lib import (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, ARROW_DEVICE_ROCM_HOST,
                           DoraGpuError, TensorAffine, TensorCast, TensorQuant)
from dora_amd.arrow_utils import Plan
from tests import affine_records as ar
from tests import cast_records as cr
from tests import quant_records as qr
from tests import struct_records as sr

PTR = 0x7F20_0000_0000  # never dereferenced
TAB = 0x7F30_0000_0040
K_CAST = 3


def fake_ptrs(rec):
    bases = sr.bases_of([r[:3] for r in rec])
    return lambda b: PTR + (1 << 20) * next(i for i, x in enumerate(bases) if x is b)


def fake_tabs(rec):
    tabs = ar.tables_of(rec)
    return lambda t: TAB + 4096 * next(i for i, x in enumerate(tabs) if x is t)


def host_ptr(b):
    return b.__array_interface__["data"][0]


def launch_of(p):
    launch, scan, checked = c_int(), c_int(), c_int()
    _lib.call("dora_gpu_test_plan_launch", p.handle, byref(launch), byref(scan), byref(checked))
    return launch.value


def facts(p):
    return (p.size, p.type_info().to_json(), p.segments(), launch_of(p))


def test_null_and_zero_affines_plan_as_the_conversion_does(lib):
    """With `affines` NULL or all zero: size, type info, segments and launch kind of
    dora_gpu_plan_tensor_convert, for device and host values, converted and plain records."""
    x = cr.source("float32", (9, 6), 1)
    recs = [qr.three_fields(), cr.three_fields(), [(None, x, x[:, 1:5], qr.quant("float32", "int8", 2.0, 1))],
            [(None, x, x, cr.cast("float32", "float32"))],  # the identity: the plain, dense plan
            [("a", x, x, None), ("b", x, x[:, :3], None)]]
    for rec in recs:
        for dev, ptr in ((ARROW_DEVICE_ROCM, fake_ptrs([r + (None,) for r in rec])),
                         (ARROW_DEVICE_CPU, host_ptr), (ARROW_DEVICE_ROCM_HOST, host_ptr)):
            fields, casts, quants, n, keep = qr.describe(rec, ptr)
            plans = []
            for affs in ("convert", None, (TensorAffine * n)()):
                h = c_void_p()
                if affs == "convert":
                    _lib.call("dora_gpu_plan_tensor_convert", fields, n, casts, quants, dev, byref(h))
                else:
                    _lib.call("dora_gpu_plan_tensor_affine", fields, n, casts, quants, affs, dev,
                              byref(h))
                plans.append(Plan(h.value, keep))
            got = []
            for p in plans:
                size, info, segs, launch = facts(p)
                if dev != ARROW_DEVICE_ROCM:  # staged bytes, not the staging buffer's address
                    segs = [(ctypes.string_at(s, ln), off, ln) for s, off, ln in segs]
                got.append((size, info, segs, launch))
                p.close() if hasattr(p, "close") else None
            assert got[0] == got[1] == got[2], rec[0][0]


def test_a_device_plan_with_a_table_is_one_cast_launch(lib):
    """kCast, no segments, the oracle's size and type info — the same as without the affine step
    — and each table's pointer, geometry and reach reported."""
    for conv in ar.CONVS:
        for label, rec in ar.shape_cases(conv)[:12] + ar.mode_cases(conv):
            sample, info, ranges = ar.oracle(rec)
            with ar.plan_affine(rec, fake_ptrs(rec), ARROW_DEVICE_ROCM, fake_tabs(rec)) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), label
                assert p.segments() == [] and launch_of(p) == K_CAST, label
                (f,), (_, _, v, c, a) = ar.plan_affines(p, 1), rec[0]
                assert f["affine"]
                tabs = fake_tabs(rec)
                for name in ("scale", "bias"):
                    assert f[name] == (tabs(a[name]) if a[name] is not None else 0), label
                if a["scale"] is not None or a["bias"] is not None:
                    axis = a["axis"] % v.ndim
                    assert (f["channels"], f["inner"]) == \
                        (v.shape[axis], int(np.prod(v.shape[axis + 1:], dtype=np.int64))), label
                    assert (f["lo"], f["hi"]) == (0, 4 * v.shape[axis] - 1), label
                else:
                    assert (f["lo"], f["hi"], f["channels"]) == (0, -1, 0)
                assert f["has_bias"] == (a["bias_value"] is not None)
            plain = [r[:4] for r in rec]
            with qr.plan_convert(plain, fake_ptrs(rec), ARROW_DEVICE_ROCM) as q:  # the wire form
                assert q.size == len(sample) and q.type_info().to_json() == info.to_json(), label
    rec = ar.mixed_record()
    sample, info, _ = ar.oracle(rec)
    with ar.plan_affine(rec, fake_ptrs(rec), ARROW_DEVICE_ROCM, fake_tabs(rec)) as p:
        assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
        assert p.segments() == [] and launch_of(p) == K_CAST
        assert [f["affine"] for f in ar.plan_affines(p, 4)] == [True, True, False, False]


def test_host_plans_convert_inside_the_call(lib):
    """Pageable and pinned alike: the staged bytes are the statement of record's."""
    for conv in ar.CONVS:
        cases = ar.shape_cases(conv) + ar.mode_cases(conv) + [("short", ar.short_totals(conv)[1])]
        for label, rec in cases:
            for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
                with ar.plan_affine(rec, host_ptr, dev) as p:
                    (ptr, off, n), = p.segments()
                    _, _, v, c, a = rec[0]
                    assert off == 0 and n == p.size
                    ar.same(ctypes.string_at(ptr, n), ar.want(v, c, a), f"{ar.conv_label(conv)} {label}")
    rec = ar.mixed_record()
    sample, info, ranges = ar.oracle(rec)
    with ar.plan_affine(rec, host_ptr, ARROW_DEVICE_CPU) as p:
        assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
        segs = p.segments()
        assert [(off, n) for _, off, n in segs] == ranges
        for (ptr, off, n), (_, _, v, c, a) in zip(segs, rec):
            ar.same(ctypes.string_at(ptr, n), ar.want(v, c, a), "mixed")


def test_an_empty_message_launches_nothing(lib):
    x = np.zeros((0, 3), np.float32)
    t0 = np.zeros(0, np.float32)
    for a in (ar.affine(np.ones(3), None, 1), ar.affine(t0, t0, 0)):
        rec = [(None, x, x, cr.cast("float32", "float16"), a)]
        for dev, ptr, tab in ((ARROW_DEVICE_ROCM, lambda b: PTR, lambda t: TAB),
                              (ARROW_DEVICE_CPU, host_ptr, None)):
            with ar.plan_affine(rec, ptr, dev, tab) as p:
                assert p.size == 0 and p.segments() == [] and launch_of(p) == 0
                assert p.type_info().to_json() == ar.oracle(rec)[1].to_json()


def refused(rec_fields, casts, quants, affs, dev=ARROW_DEVICE_ROCM):
    h = c_void_p()
    with pytest.raises(DoraGpuError) as e:
        _lib.call("dora_gpu_plan_tensor_affine", rec_fields, len(casts), casts, quants, affs, dev,
                  byref(h))
    assert not h.value
    return e.value.code, str(e.value)


def test_refusals_of_the_c_entry_name_the_field(lib):
    x = cr.source("uint8", (4, 3, 5), 1)
    y = cr.source("float32", (4, 2), 2)

    def call(dev=ARROW_DEVICE_ROCM, cast_scale=None, quant=False, plain=False, **aff):
        """Field `img` next to a plain field, `img` cast (or quantised, or plain) with `aff`."""
        ptr = host_ptr if dev != ARROW_DEVICE_ROCM else (lambda b: PTR if b is x else PTR + (1 << 20))
        tx, kx = tensor._describe(ptr(x), x.shape, None, x.dtype)
        ty, ky = tensor._describe(ptr(y), y.shape, None, y.dtype)
        lst, keep = tensor._describe_list(["xy", "img"], [ty, tx], ty, 0, 0)
        casts, quants, affs = (TensorCast * 2)(), (TensorQuant * 2)(), (TensorAffine * 2)()
        if quant:
            quants[1].dtype_code, quants[1].dtype_bits = 0, 8
            quants[1].has_scale, quants[1].scale = int(cast_scale is not None), cast_scale or 0.0
        elif not plain:
            casts[1].dtype_code, casts[1].dtype_bits = 2, 16
            casts[1].has_scale, casts[1].scale = int(cast_scale is not None), cast_scale or 0.0
        keeps = []
        for name in ("scale", "bias"):
            t = aff.get(name)
            if t is None:
                continue
            if isinstance(t, tuple):  # (ptr, shape, strides, dtype, byte_offset)
                d, kp = tensor._describe(*t)
            else:
                d, kp = tensor._describe(host_ptr(t) if dev != ARROW_DEVICE_ROCM else TAB, t.shape,
                                         None, t.dtype)
            keeps.append((d, kp, t))
            setattr(affs[1], name, pointer(d))
        affs[1].axis = aff.get("axis", 0)
        if "bias_value" in aff:
            affs[1].has_bias, affs[1].bias_value = 1, aff["bias_value"]
        out = refused(lst.fields, casts, quants, affs, dev)
        del keep, keeps, kx, ky
        return out

    ones = np.ones(3, np.float32)
    checks = [
        (dict(plain=True, bias_value=1.0), -1, "neither cast nor quantised"),
        (dict(plain=True, scale=ones, axis=1), -1, "neither cast nor quantised"),
        (dict(cast_scale=2.0, scale=ones, axis=1), -1, "scalar scale"),
        (dict(quant=True, cast_scale=2.0, scale=ones, axis=1), -1, "scalar scale"),
        (dict(bias=ones, axis=1, bias_value=1.0), -1, "scalar bias"),
        (dict(scale=ones, axis=3), -1, "axis 3"),
        (dict(scale=ones, axis=-1), -1, "axis -1"),
        (dict(scale=np.ones(3, np.float64), axis=1), -4, "float64"),
        (dict(bias=np.ones(3, np.float16), axis=1), -4, "float16"),
        (dict(scale=np.ones(3, np.int32), axis=1), -4, "int32"),
        (dict(scale=np.ones((3, 1), np.float32), axis=1), -1, "2 dimensions"),
        (dict(scale=np.ones(4, np.float32), axis=1), -1, "4 elements"),
        (dict(bias=np.ones(3, np.float32), axis=2), -1, "3 elements"),
        (dict(scale=(TAB, (3,), (2,), np.float32, 0), axis=1), -1, "dense"),
        (dict(scale=(TAB, (3,), None, np.float32, 2), axis=1), -1, "multiple of 4"),
        (dict(bias=(TAB + 1, (3,), None, np.float32, 0), axis=1), -1, "multiple of 4"),
        (dict(bias=(0, (3,), None, np.float32, 0), axis=1), -1, "NULL"),
        (dict(bias_value=float("inf")), -1, "not finite"),
        (dict(bias_value=float("nan")), -1, "not finite"),
    ]
    for kw, code, word in checks:
        got = call(**kw)
        assert got[0] == code and word in got[1] and "field 1 `img`" in got[1], (kw, got)
    # a host table is read: a value that is not finite is refused; one in HBM is never read
    for bad in (np.inf, -np.inf, np.nan):
        t = np.array([1.0, bad, 2.0], np.float32)
        for name in ("scale", "bias"):
            for dev in (ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM_HOST):
                got = call(dev=dev, axis=1, **{name: t})
                assert got[0] == -1 and "value 1" in got[1] and "not finite" in got[1] \
                    and f"{name} table" in got[1] and "field 1 `img`" in got[1], got
    # the conversion's own refusals still come first, and a bare tensor's go without a name
    got = call(cast_scale=float("nan"), bias_value=1.0)
    assert got[0] == -1 and "scale" in got[1] and "field 1 `img`" in got[1]
    tx, kx = tensor._describe(PTR, x.shape, None, x.dtype)
    lst, keep = tensor._describe_list(None, [tx], tx, 0, 0)
    affs = (TensorAffine * 1)()
    affs[0].has_bias, affs[0].bias_value = 1, 1.0
    code, text = refused(lst.fields, (TensorCast * 1)(), None, affs)
    assert code == -1 and "neither cast nor quantised" in text
    h = c_void_p()
    with pytest.raises(DoraGpuError):  # no field at all, as the conversion refuses it
        _lib.call("dora_gpu_plan_tensor_affine", None, 0, None, None, affs, ARROW_DEVICE_ROCM, byref(h))


def test_calls_without_bias_and_axis_refuse_as_before(lib):
    """The conversion's refusals through the new entry with NULL affines: the same codes and
    texts as through dora_gpu_plan_tensor_convert."""
    x = cr.source("float32", (4, 3), 1)
    tx, kx = tensor._describe(PTR, x.shape, None, x.dtype)
    lst, keep = tensor._describe_list(["x"], [tx], tx, 0, 0)
    for code, bits, zp, scale in ((1, 32, 0, None), (1, 8, 256, None), (1, 8, 0, float("inf"))):
        quants = (TensorQuant * 1)()
        quants[0].dtype_code, quants[0].dtype_bits, quants[0].zero_point = code, bits, zp
        if scale is not None:
            quants[0].has_scale, quants[0].scale = 1, scale
        texts = []
        for name, extra in (("dora_gpu_plan_tensor_convert", ()), ("dora_gpu_plan_tensor_affine", (None,))):
            h = c_void_p()
            with pytest.raises(DoraGpuError) as e:
                _lib.call(name, lst.fields, 1, None, quants, *extra, ARROW_DEVICE_ROCM, byref(h))
            texts.append((e.value.code, str(e.value)))
        assert texts[0] == texts[1]
