"""Affine plans through dora_gpu_pack on the GPU (kernel level, no torch): the bases and the tables
of a record (tests/affine_records.py) are uploaded, every field and table described over its device
pointer, planned with dora_gpu_plan_tensor_affine (ARROW_DEVICE_ROCM) and packed — one launch of
gather_affine_kernel — into a poisoned destination with 4 KiB guard bands on both sides.  Every
field's region equals `tensor.from_numpy_cast` / `tensor.from_numpy_quantize` bit for bit with
nothing exempt but a NaN's payload in a float destination, the guard bands and every padding byte
keep the poison, the type info is the oracle's.  The shapes are those of
test_affine_index_host.py, each of which passed the sanitized host emulation there.

The value sets run at one dense shape and at one cut from a wider base, a channel a row.  They are
where the hardware's product and sum meet numpy's two roundings: every uint8 value under the
ImageNet constants; every float16 pattern under a scale table holding 1/255, 3, -1, +-0, 2^-14 and
a subnormal, with biases of +-0, with for each of those scales a bias that is the exact negative
of a rounded product (two roundings give exactly 0 there, a fused multiply-add the rounding error),
with sums inside the float32 and the float16 subnormal ranges and sums that overflow float16;
quantise ties k + 0.5 that the bias produces; and device tables holding NaN, +inf and -inf.

A table that leaves its allocation by one element and a field that leaves it by one source byte are
refused with nothing launched; the launch counters name gather_affine_kernel for affine plans and
the old kernels for plans without an affine step."""
from ctypes import c_uint64

import numpy as np
import pytest

from tests import affine_records as ar
from tests import cast_records as cr
from tests import quant_records as qr
from tests.test_gpu_tensor_quant_device import pack_at
from tests.test_gpu_tensor_struct_device import GUARD, POISON, Uploaded, check_sample

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from dora_amd import device
    assert device.device_count() >= 1
    device.set_device(0)
    s = device.Stream()
    yield s
    s.close()


class Tables:
    """The distinct tables of a record in device memory, each 4 bytes into an allocation of its
    own (4 mod 16)."""

    def __init__(self, rec, stream):
        from dora_amd.device import DeviceBuffer
        self.tabs = ar.tables_of(rec)
        self.bufs = [DeviceBuffer.from_bytes(b"\0" * 4 + t.tobytes(), stream) for t in self.tabs]

    def ptr_of(self, t):
        return self.bufs[next(i for i, x in enumerate(self.tabs) if x is t)].ptr + 4

    def free(self):
        for b in self.bufs:
            b.free()


def launches():
    from dora_amd import _lib
    c = (c_uint64 * 4)()
    _lib.call("dora_gpu_test_fields_launches", c)
    return dict(zip(("struct", "cast", "quant", "affine"), c))


def run_record(rec, stream, offsets, what):
    """Plan `rec` over uploaded bases and tables and pack it at every offset."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from dora_amd.device import DeviceBuffer
    sample, info, ranges = ar.oracle(rec)
    up, tabs = Uploaded([r[:3] for r in rec], stream), Tables(rec, stream)
    buf = DeviceBuffer(len(sample) + 2 * GUARD + 16)
    try:
        with ar.plan_affine(rec, up.ptr_of, ARROW_DEVICE_ROCM, tabs.ptr_of) as p:
            assert p.size == len(sample), what
            assert p.type_info().to_json() == info.to_json(), what
            assert p.segments() == [], what
            before = launches()
            for mis in offsets:
                got, intact = pack_at(p, buf, stream, mis)
                assert intact, f"guard bands overwritten, {what}, destination {mis} mod 16"
                pad = bytearray(got)
                for (off, ln), (_, _, v, c, a) in zip(ranges, rec):
                    ar.same(got[off:off + ln], ar.want(v, c, a), f"{what}, destination {mis} mod 16")
                    pad[off:off + ln] = bytes([POISON]) * ln
                assert bytes(pad) == bytes([POISON]) * len(got), f"padding written, {what}"
            after = launches()
            assert after["affine"] - before["affine"] == len(list(offsets)), what
            assert all(after[k] == before[k] for k in ("struct", "cast", "quant")), what
    finally:
        buf.free()
        tabs.free()
        up.free()


@pytest.mark.parametrize("conv", ar.CONVS, ids=ar.conv_label)
def test_every_shape_at_every_destination(dev, conv):
    for label, rec in ar.shape_cases(conv):
        run_record(rec, dev, ar.dst_offsets(conv), f"{ar.conv_label(conv)} {label}")


@pytest.mark.parametrize("conv", ar.CONVS, ids=ar.conv_label)
def test_tables_and_scalars_in_every_combination(dev, conv):
    for label, rec in ar.mode_cases(conv):
        run_record(rec, dev, (0, 4, 12), f"{ar.conv_label(conv)} {label}")
    mis, rec = ar.short_totals(conv)
    run_record(rec, dev, (mis, 0), f"{ar.conv_label(conv)} 3 elements")


def test_a_record_mixes_affine_and_plain_conversions(dev):
    for d0 in (3, 9, 64):
        run_record(ar.mixed_record(d0), dev, range(0, 16, 2), f"mixed record d0={d0}")


# ---------------------------------------------------------------------------------------------
# Value sets: a channel a row, the value set along it (axis 0, inner = len(x)).
# ---------------------------------------------------------------------------------------------
F32 = np.float32
SCALES = np.array([1 / 255, 3.0, -1.0, 0.0, -0.0, 2.0 ** -14, 1e-40], F32)  # (the last: a subnormal)


def rows(x, channels):
    """[(label, base, view)]: `x` as `channels` rows, dense and cut from rows 3 wider."""
    dense = np.ascontiguousarray(np.broadcast_to(x, (channels, len(x))))
    wide = np.full((channels, len(x) + 3), x[0], x.dtype)
    wide[:, 1:len(x) + 1] = x
    return [("dense", dense, dense), ("cut from a wider base", wide, wide[:, 1:len(x) + 1])]


def negated_products(x0, scales):
    """The exact negatives of the rounded float32 products x0 * s."""
    with np.errstate(under="ignore"):
        return -(F32(x0) * scales)


def value_sets():
    """[(label, 1-D source array, conversion, affine)]."""
    s, b = ar.imagenet()
    u8, f16 = cr.all_patterns("uint8"), cr.all_patterns("float16")
    out = []
    for dst in ("float16", "float32"):
        out.append((f"uint8 imagenet -> {dst}", u8, cr.cast("uint8", dst), ar.affine(s, b, 0)))
    for x0 in (200, 77, 255):
        out.append((f"uint8 imagenet, bias -fl({x0} * s)", u8, cr.cast("uint8", "float32"),
                    ar.affine(s, negated_products(x0, s), 0)))
    zeros = np.array([0.0, -0.0] * 4, F32)
    for dst in ("float16", "float32"):
        out.append((f"float16 -> {dst}, bias +-0", f16, cr.cast("float16", dst),
                    ar.affine(SCALES, zeros[:7], 0)))
        out.append((f"float16 -> {dst}, bias -+0", f16, cr.cast("float16", dst),
                    ar.affine(SCALES, zeros[1:], 0)))
    for x0 in (0.3, 1000.0, 6.1e-5, -65504.0):
        x0 = float(np.float16(x0))
        out.append((f"float16, bias -fl({x0!r} * s)", f16, cr.cast("float16", "float32"),
                    ar.affine(SCALES, negated_products(x0, SCALES), 0)))
    tiny = np.array([2.0 ** -130, -2.0 ** -135, 2.0 ** -20, -2.0 ** -24, 2.0 ** -126, 1e-40, -1e-45], F32)
    big = np.array([65000.0, -65000.0, 65504.0, 6e4, -6e4, 65519.0, -65520.0], F32)
    for dst in ("float16", "float32"):
        out.append((f"float16 -> {dst}, subnormal sums", f16, cr.cast("float16", dst),
                    ar.affine(SCALES, tiny, 0)))
    out.append(("float16 -> float16, overflowing sums", f16, cr.cast("float16", "float16"),
                ar.affine(SCALES, big, 0)))
    ties = np.array([0.5, -0.5, 1.5, 2.5, 0.49999997, -1.5], F32)
    out.append(("int16 -> int8, ties from the bias", cr.all_patterns("int16"),
                qr.quant("int16", "int8", None, -7), ar.affine(None, ties, 0)))
    out.append(("uint8 -> uint8, ties from the bias", u8, qr.quant("uint8", "uint8", None, 3),
                ar.affine(np.array([0.5, 1.0, 0.25, 1.0, 0.5, 1.0], F32), ties, 0)))
    out.append(("float16 -> int16, ties from the bias", f16, qr.quant("float16", "int16", None, 0),
                ar.affine(None, ties, 0)))
    bad = np.array([np.nan, np.inf, -np.inf, 1.0, 0.0, -1.0, 2.0], F32)
    for conv in (cr.cast("float16", "float32"), cr.cast("float16", "float16"),
                 qr.quant("float16", "int8", None, 5)):
        out.append((f"{ar.conv_label(conv)}, NaN and infinities in the scale table", f16, conv,
                    ar.affine(bad, None, 0)))
        out.append((f"{ar.conv_label(conv)}, NaN and infinities in the bias table", f16, conv,
                    ar.affine(SCALES, bad, 0)))
    return out


N_VALUE_SETS = 2 + 3 + 4 + 4 + 2 + 1 + 3 + 6


@pytest.mark.parametrize("k", range(N_VALUE_SETS))
def test_the_hardwares_product_and_sum_over_the_value_sets(dev, k):
    sets = value_sets()
    assert len(sets) == N_VALUE_SETS
    label, x, conv, a = sets[k]
    channels = len(a["scale"] if a["scale"] is not None else a["bias"])
    for how, b, v in rows(x, channels):
        run_record([(None, b, v, conv, a)], dev, (0,), f"{label}, {how}")


def test_plans_without_an_affine_step_launch_the_old_kernels(dev):
    """dora_gpu_plan_tensor_affine with no affine entry is the conversion's plan: a cast runs
    gather_cast_kernel, a quantise gather_quant_kernel, and neither counts as an affine launch."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from dora_amd.device import DeviceBuffer
    b = cr.source("float32", (9, 8), seed=1)
    for conv, name in ((cr.cast("float32", "float16", 0.5), "cast"),
                       (qr.quant("float32", "uint8", 255.0, 0), "quant")):
        rec = [(None, b, b[:, 1:7], conv, None)]
        up = Uploaded([r[:3] for r in rec], dev)
        buf = DeviceBuffer(4096)
        try:
            with ar.plan_affine(rec, up.ptr_of, ARROW_DEVICE_ROCM) as p:
                before = launches()
                p.pack(buf.ptr, p.size, dev)
                dev.sync()
                after = launches()
                got = buf.to_bytes(stream=dev)[:p.size]
            assert {k: after[k] - before[k] for k in after} == \
                {"struct": 0, "cast": 0, "quant": 0, "affine": 0, name: 1}
            ar.same(got, ar.want(b[:, 1:7], conv, None), name)
        finally:
            buf.free()
            up.free()


def test_refused_with_nothing_launched(dev):
    """A bias table reaching one element past its allocation, named; a field reaching one source
    byte past its own: DORA_ERR_INVALID, the destination keeps its poison.  Moved back inside, the
    same plans pack."""
    from ctypes import byref, c_void_p, pointer
    from dora_amd import _lib, tensor
    from dora_amd._lib import (ARROW_DEVICE_ROCM, DoraGpuError, TensorAffine, TensorCast)
    from dora_amd.arrow_utils import Plan
    from dora_amd.device import DeviceBuffer
    n = 1 << 20
    one, tab, dst = DeviceBuffer(n), DeviceBuffer(n), DeviceBuffer(n)
    try:
        dst.fill(POISON, dev)
        one.fill(0, dev)
        tab.fill(0, dev)
        dev.sync()

        def plan(field_off, table_off):
            # 64 rows of 16 uint8 in `one`, the last ending at its last byte when field_off is 0,
            # cast to float16 under a bias table of 16 float32 that ends at the last byte of `tab`
            # when table_off is 0
            stride = n // 64
            end = 63 * stride + 16
            t = tensor._describe(one.ptr, (64, 16), (stride, 1), np.uint8, n - end + field_off)
            bt = tensor._describe(tab.ptr, (16,), (1,), np.float32, n - 64 + 4 * table_off)
            lst, keep = tensor._describe_list(["x"], [t[0]], t[0], 0, 0)
            casts = (TensorCast * 1)()
            casts[0].dtype_code, casts[0].dtype_bits = 2, 16
            affs = (TensorAffine * 1)()
            affs[0].bias, affs[0].axis = pointer(bt[0]), 1
            h = c_void_p()
            _lib.call("dora_gpu_plan_tensor_affine", lst.fields, 1, casts, None, affs,
                      ARROW_DEVICE_ROCM, byref(h))
            return Plan(h.value, (lst, keep, t, bt, casts, affs))

        before = launches()
        with plan(0, 1) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, n, dev)
            assert e.value.code == -1
            assert "field 0 `x`" in str(e.value) and "bias table" in str(e.value) \
                and "allocation" in str(e.value)
        with plan(1, 0) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, n, dev)
            assert e.value.code == -1
            assert "field 0 `x`" in str(e.value) and "allocation" in str(e.value) \
                and "table" not in str(e.value)
        dev.sync()
        assert launches() == before
        assert dst.to_bytes(stream=dev) == bytes([POISON]) * n  # nothing was launched
        with plan(0, 0) as p:
            p.pack(dst.ptr, n, dev)
        dev.sync()
        assert launches()["affine"] == before["affine"] + 1
    finally:
        for b in (one, tab, dst):
            b.free()
