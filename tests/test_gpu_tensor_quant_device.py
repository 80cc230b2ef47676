"""Quantise plans through dora_gpu_pack on the GPU (kernel level, no torch): the bases of a record
(tests/quant_records.py) are uploaded, every field described over its device pointer, planned with
dora_gpu_plan_tensor_convert (ARROW_DEVICE_ROCM) and packed — one launch of gather_quant_kernel —
into a poisoned destination with 4 KiB guard bands on both sides.  Every field's region equals
`tensor.from_numpy_quantize` bit for bit with nothing exempt, the guard bands and every padding
byte keep the poison, the type info is the oracle's.  The shapes are those of
test_quant_index_host.py, each of which passed the sanitized host emulation there; the value sets
run at one dense shape and at one cut from a wider base, which is where v_rndne_f32, the clamp and
v_cvt_i32_f32 meet numpy: ties, NaNs, infinities, signed zeros, subnormals and products whose
rounding decides the tie, under every scale and zero point.  A field that leaves its allocation by
one source byte and a 16-bit destination at an odd address are refused with nothing launched."""
import numpy as np
import pytest

from tests import cast_records as cr
from tests import quant_records as qr
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


def pack_at(plan, buf, stream, mis):
    """Pack `plan` into the poisoned `buf` at GUARD + mis; (sample bytes, guards intact)."""
    n = plan.size
    buf.fill(POISON, stream)
    plan.pack(buf.ptr + GUARD + mis, n, stream)
    stream.sync()
    raw = buf.to_bytes(stream=stream)
    lo, hi = raw[:GUARD + mis], raw[GUARD + mis + n:]
    return raw[GUARD + mis:GUARD + mis + n], lo == bytes([POISON]) * len(lo) and hi == bytes([POISON]) * len(hi)


def run_record(rec, stream, offsets, what, up=None):
    """Plan `rec` over uploaded bases (`up`: already there) and pack it at every offset."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from dora_amd.device import DeviceBuffer
    sample, info, ranges = qr.oracle(rec)
    own = up is None
    if own:
        up = Uploaded([r[:3] for r in rec], stream)
    buf = DeviceBuffer(len(sample) + 2 * GUARD + 16)
    try:
        with qr.plan_convert(rec, up.ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample), what
            assert p.type_info().to_json() == info.to_json(), what
            assert p.segments() == [], what
            for mis in offsets:
                got, intact = pack_at(p, buf, stream, mis)
                assert intact, f"guard bands overwritten, {what}, destination {mis} mod 16"
                for (off, ln), (_, _, v, c) in zip(ranges, rec):
                    if qr.is_quant(c):  # (names the first wrong element)
                        qr.same(got[off:off + ln], qr.want(v, c), f"{what}, destination {mis} mod 16")
                check_sample(got, sample, ranges, f"{what}, destination {mis} mod 16")
    finally:
        buf.free()
        if own:
            up.free()


@pytest.mark.parametrize("src,dst", qr.PAIRS)
def test_every_shape_of_every_pair(dev, src, dst):
    for label, rec in qr.shape_cases(src, dst):
        run_record(rec, dev, qr.dst_offsets(dst), f"{src}->{dst} {label}")


@pytest.mark.parametrize("dst", list(qr.DESTS))
def test_totals_smaller_than_the_head(dev, dst):
    mis, rec = qr.short_totals(dst)
    run_record(rec, dev, (mis, 0), f"3 elements of {dst}")


def test_a_record_of_three_fields(dev):
    for d0 in (3, 9, 64):
        run_record(qr.three_fields(d0), dev, range(0, 16, 2), f"three fields d0={d0}")


@pytest.mark.parametrize("k", range(qr.N_VALUE_SETS))
def test_the_hardwares_quantise_over_the_value_sets(dev, k):
    label, x, qs = qr.value_sets()[k]
    b, v = cr.cut_from_wider(x)
    up = Uploaded([(None, x, x), (None, b, v)], dev)
    try:
        for q in qs:
            run_record([(None, x, x, q)], dev, (0,), label + qr.label_of(q), up)
            run_record([(None, b, v, q)], dev, (0,), label + qr.label_of(q) + ", cut from a wider base", up)
    finally:
        up.free()


def test_refused_with_nothing_launched(dev):
    """A quantised field reaching one source byte past its allocation, named; a 16-bit destination
    at an odd address: DORA_ERR_INVALID, the destination keeps its poison.  Moved back inside and
    aligned — and an 8-bit destination at any address — the same plans pack."""
    from ctypes import byref, c_void_p
    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM, DoraGpuError, TensorQuant
    from dora_amd.arrow_utils import Plan
    from dora_amd.device import DeviceBuffer
    n = 1 << 20
    one, two, dst = DeviceBuffer(n), DeviceBuffer(n), DeviceBuffer(n)
    try:
        dst.fill(POISON, dev)
        dev.sync()

        def plan(second_off, dst_bits):
            # `first`: 64 rows of 16 bytes cut from rows of 32, sent as they are; `second`: 64
            # rows of 16 uint8 in `two`, the last ending at its last byte when second_off is 0
            stride = n // 64
            end = 63 * stride + 16
            ts = [tensor._describe(one.ptr, (64, 16), (32, 1), np.uint8),
                  tensor._describe(two.ptr, (64, 16), (stride, 1), np.uint8, n - end + second_off)]
            lst, keep = tensor._describe_list(["first", "second"], [t for t, _ in ts], ts[0][0], 0, 0)
            quants = (TensorQuant * 2)()
            quants[1].dtype_code, quants[1].dtype_bits, quants[1].zero_point = 1, dst_bits, 7
            h = c_void_p()
            _lib.call("dora_gpu_plan_tensor_convert", lst.fields, 2, None, quants,
                      ARROW_DEVICE_ROCM, byref(h))
            return Plan(h.value, (lst, keep, ts, quants))

        with plan(1, 8) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, n, dev)
            assert e.value.code == -1
            assert "field 1 `second`" in str(e.value) and "allocation" in str(e.value)
        with plan(0, 16) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr + 1, n - 16, dev)
            assert e.value.code == -1
            assert "field 1 `second`" in str(e.value) and "nothing was launched" in str(e.value)
        dev.sync()
        assert dst.to_bytes(stream=dev) == bytes([POISON]) * n  # nothing was launched
        with plan(0, 16) as p:
            p.pack(dst.ptr, n, dev)
        with plan(0, 8) as p:
            p.pack(dst.ptr + 1, n - 16, dev)
        dev.sync()
    finally:
        for b in (one, two, dst):
            b.free()
