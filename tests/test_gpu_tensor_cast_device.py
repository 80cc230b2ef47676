"""Cast plans through dora_gpu_pack on the GPU (kernel level, no torch): the bases of a cast record
(tests/cast_records.py) are uploaded, every field described over its device pointer, planned with
dora_gpu_plan_tensor_cast (ARROW_DEVICE_ROCM) and packed — one launch of gather_cast_kernel —
into a poisoned destination with 4 KiB guard bands on both sides.  Every field's region equals
numpy's `(x.astype(float32) * float32(scale)).astype(dst)` bit for bit (a NaN for a NaN), the
guard bands and every padding byte keep the poison, the type info is the oracle's.  The shapes are
those of test_cast_index_host.py, each of which passed the sanitized host emulation there; the
value sets of test_tensor_cast_host.py run at one dense shape each and at one cut from a wider base,
which is where the hardware's converts and its float32 multiplication meet numpy: subnormal
products, signed zeros, overflow and NaNs under every scale of tests/cast_records.py included.  A field that leaves its allocation by one source byte
and a destination that is not a multiple of the destination element size are refused with
nothing launched."""
import numpy as np
import pytest

from tests import cast_records as cr
from tests.test_cast_index_host import shape_cases
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


def run_record(rec, stream, offsets, what):
    """Plan `rec` over uploaded bases and pack it at every offset of `offsets`."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from dora_amd.device import DeviceBuffer
    sample, info, ranges = cr.oracle(rec)
    up = Uploaded([r[:3] for r in rec], stream)
    buf = DeviceBuffer(len(sample) + 2 * GUARD + 16)
    try:
        with cr.plan_cast(rec, up.ptr_of, ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample), what
            assert p.type_info().to_json() == info.to_json(), what
            assert p.segments() == [], what
            for mis in offsets:
                got, intact = pack_at(p, buf, stream, mis)
                assert intact, f"guard bands overwritten, {what}, destination {mis} mod 16"
                if any(np.isnan(cr.want(v, c)).any() for _, _, v, c in rec if c is not None):
                    pad = bytearray(got)
                    for (off, ln), (_, _, v, c) in zip(ranges, rec):
                        cr.same(got[off:off + ln], cr.want(v, c), what)
                        pad[off:off + ln] = bytes([POISON]) * ln
                    assert bytes(pad) == bytes([POISON]) * len(got), f"padding written, {what}"
                else:
                    check_sample(got, sample, ranges, f"{what}, destination {mis} mod 16")
    finally:
        buf.free()
        up.free()


@pytest.mark.parametrize("src,dst", cr.PAIRS)
def test_every_shape_of_every_pair(dev, src, dst):
    for label, rec in shape_cases(src, dst):
        run_record(rec, dev, cr.dst_offsets(dst), f"{src}->{dst} {label}")


def test_a_record_of_three_fields(dev):
    for d0 in (3, 9, 64):
        run_record(cr.three_fields(d0), dev, range(0, 16, 2), f"three fields d0={d0}")


def test_a_plain_field_takes_the_tile_body_beside_a_cast(dev):
    """A permuted float32 field sent as it is, which the library's selection tiles wherever the
    destination is a multiple of 4 (the rows body at 2 mod 4), in one launch with a cast field."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from tests import struct_records as sr
    rec = cr.tiled_plain_and_cast()
    with cr.plan_cast(rec, lambda b: 0x7E00_0000_0000, ARROW_DEVICE_ROCM) as p:  # (never packed)
        kinds = {mis: sr.plan_fields(p, 0x7F50_0000_1000 + mis)[1]["kind"] for mis in (0, 2, 4, 8)}
        assert [k["cast"] for k in cr.plan_casts(p)] == [True, False]
    assert kinds[0] >= 0 and kinds[4] >= 0 and kinds[8] >= 0 and kinds[2] < 0, kinds
    run_record(rec, dev, (0, 2, 4, 8), "tile beside cast")


@pytest.mark.parametrize("k", range(cr.N_VALUE_SETS))
def test_the_hardwares_conversions_over_their_domain(dev, k):
    label, x, c = cr.value_sets()[k]
    run_record([(None, x, x, c)], dev, (0,), label)
    b, v = cr.cut_from_wider(x)
    run_record([(None, b, v, c)], dev, (0,), label + ", cut from a wider base")


def test_refused_with_nothing_launched(dev):
    """A cast field reaching one source byte past its allocation, named; a destination that is
    odd for float16 (and 2 mod 4 for float32): DORA_ERR_INVALID, the destination keeps its
    poison.  Moved back inside and aligned, the same plans pack."""
    from ctypes import byref, c_void_p
    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM, DoraGpuError, TensorCast
    from dora_amd.arrow_utils import Plan
    from dora_amd.device import DeviceBuffer
    n = 1 << 20
    one, two, dst = DeviceBuffer(n), DeviceBuffer(n), DeviceBuffer(4 * n)
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
            casts = (TensorCast * 2)()
            casts[1].dtype_code, casts[1].dtype_bits = 2, dst_bits
            h = c_void_p()
            _lib.call("dora_gpu_plan_tensor_cast", lst.fields, 2, casts, ARROW_DEVICE_ROCM, byref(h))
            return Plan(h.value, (lst, keep, ts, casts))

        with plan(1, 16) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, 4 * n, dev)
            assert e.value.code == -1
            assert "field 1 `second`" in str(e.value) and "allocation" in str(e.value)
        for bits, mis in ((16, 1), (32, 2), (32, 1)):
            with plan(0, bits) as p:
                with pytest.raises(DoraGpuError) as e:
                    p.pack(dst.ptr + mis, 4 * n - 16, dev)
                assert e.value.code == -1
                assert "field 1 `second`" in str(e.value) and "nothing was launched" in str(e.value)
        dev.sync()
        assert dst.to_bytes(stream=dev) == bytes([POISON]) * (4 * n)  # nothing was launched
        for bits in (16, 32):
            with plan(0, bits) as p:
                p.pack(dst.ptr, 4 * n, dev)
        dev.sync()
    finally:
        for b in (one, two, dst):
            b.free()
