"""Ragged-batch plans through dora_gpu_pack on the GPU (kernel level, no torch): the bases of a
record (tests/list_records.py, N = 67) are uploaded, every field described over its device
pointer, planned with dora_gpu_plan_tensor_list (ARROW_DEVICE_ROCM) for B in {1, 5, 257} and
packed into a poisoned destination with 4 KiB guard bands on both sides.  The sample is byte-equal
to the oracle's packing of pa.ListArray.from_arrays(offsets, child) in every region, and the
guard bands and every padding byte keep the poison.  Covered: a host partition with strided fields
(a prefix copy and one gather launch) and with all-dense fields (a prefix copy and copy segments),
and a partition in HBM as int32 and int64, as lengths and as offsets (one launch that scans it and
gathers the fields).  A partition in HBM that does not describe the rows — a sum short of N, a sum
past N, a negative length — delivers exactly the clamped formula's offsets and a List that pyarrow
validates.  Every scan shape passed the sanitized emulation of test_scan_index_host.py.  Nothing
here reads outside an allocation: the partition's reach is checked on the CPU plan with made-up
addresses (test_tensor_list_plan.py), and the one refusal exercised here launches nothing."""
import numpy as np
import pytest

from tests import list_records as lr
from tests.test_gpu_tensor_struct_device import GUARD, POISON, Uploaded, check_sample

pytestmark = pytest.mark.gpu

N = 67
MIS = (0, 4, 8)  # the sample a whole number of dwords (its offsets are int32): fields at 8, 12, 0 mod 16


@pytest.fixture(scope="module")
def dev():
    from dora_amd import device
    assert device.device_count() >= 1
    device.set_device(0)
    s = device.Stream()
    yield s
    s.close()


def lengths_for(b):
    """b lengths that sum to N with empty lists at the front, in the middle and at the end."""
    if b == 1:
        return [N]
    ln = [0] * b
    ln[1], ln[b // 2], ln[b - 2] = 20, 7, N - 27
    return ln


def pack_guarded(plan, stream, mis):
    from dora_amd.device import DeviceBuffer
    n = plan.size
    buf = DeviceBuffer(n + 2 * GUARD + 16)
    try:
        buf.fill(POISON, stream)
        plan.pack(buf.ptr + GUARD + mis, n, stream)
        stream.sync()
        raw = buf.to_bytes(stream=stream)
    finally:
        buf.free()
    lo, hi = raw[:GUARD + mis], raw[GUARD + mis + n:]
    return raw[GUARD + mis:GUARD + mis + n], lo == bytes([POISON]) * len(lo) and hi == bytes([POISON]) * len(hi)


def check_list_sample(got, sample, obytes, ranges, what):
    assert got[:obytes] == sample[:obytes], "offsets, " + what
    check_sample(got, sample, [(0, obytes)] + ranges, what)


@pytest.mark.parametrize("b", [1, 5, 257])
@pytest.mark.parametrize("name", list(lr.RECORDS))
def test_host_partition_with_strided_fields(dev, name, b):
    from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, PARTITION_LENGTHS, PARTITION_OFFSETS
    rec = lr.RECORDS[name](N)
    lengths = lengths_for(b)
    offs = lr.offsets_of(lengths)
    sample, info, ranges = lr.oracle(rec, offs)
    up = Uploaded(rec, dev)
    try:
        for part, form in ((np.array(lengths, np.int32), PARTITION_LENGTHS), (offs, PARTITION_OFFSETS)):
            with lr.plan_list(rec, up.ptr_of, ARROW_DEVICE_ROCM, part, form, ARROW_DEVICE_CPU) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
                assert p.segments() == [] and lr.plan_scan(p)["prefix"] == 4 * (b + 1)
                for mis in MIS:
                    what = f"{name} B={b} form {form}, destination {mis} mod 16"
                    got, intact = pack_guarded(p, dev, mis)
                    assert intact, "guard bands overwritten, " + what
                    check_list_sample(got, sample, 4 * (b + 1), ranges, what)
    finally:
        up.free()


@pytest.mark.parametrize("b", [1, 5, 257])
def test_host_partition_with_all_dense_fields(dev, b):
    from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, PARTITION_LENGTHS
    x, y, z = lr.base(np.float32, (N, 4)), lr.base(np.float64, (N,)), lr.base(np.uint8, (N + 2, 3))
    rec = [("x", x, x), ("y", y, y), ("z", z, z[1:N + 1])]
    lengths = lengths_for(b)
    sample, info, ranges = lr.oracle(rec, lr.offsets_of(lengths))
    up = Uploaded(rec, dev)
    try:
        with lr.plan_list(rec, up.ptr_of, ARROW_DEVICE_ROCM, np.array(lengths, np.int64),
                          PARTITION_LENGTHS, ARROW_DEVICE_CPU) as p:
            assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
            assert len(p.segments()) == 3  # no gather: the prefix copy and the segment pack
            for mis in MIS:
                what = f"dense B={b}, destination {mis} mod 16"
                got, intact = pack_guarded(p, dev, mis)
                assert intact, "guard bands overwritten, " + what
                check_list_sample(got, sample, 4 * (b + 1), ranges, what)
    finally:
        up.free()


@pytest.mark.parametrize("b", [1, 5, 257])
@pytest.mark.parametrize("name", list(lr.RECORDS))
def test_device_partition(dev, name, b):
    """int32 and int64, lengths and offsets: one launch writes offsets and fields."""
    from dora_amd._lib import ARROW_DEVICE_ROCM, PARTITION_LENGTHS, PARTITION_OFFSETS
    from dora_amd.device import DeviceBuffer
    rec = lr.RECORDS[name](N)
    lengths = lengths_for(b)
    offs = lr.offsets_of(lengths)
    sample, info, ranges = lr.oracle(rec, offs)
    up = Uploaded(rec, dev)
    try:
        for dt in (np.int32, np.int64):
            for words, form in ((np.array(lengths, dt), PARTITION_LENGTHS), (offs.astype(dt), PARTITION_OFFSETS)):
                part = DeviceBuffer.from_bytes(words.tobytes(), dev)
                try:
                    with lr.plan_list(rec, up.ptr_of, ARROW_DEVICE_ROCM, words, form,
                                      ARROW_DEVICE_ROCM, part_ptr=part.ptr) as p:
                        assert p.size == len(sample) and p.type_info().to_json() == info.to_json()
                        assert p.segments() == [] and lr.plan_scan(p)["scan"]
                        for mis in MIS:
                            what = f"{name} B={b} {np.dtype(dt)} form {form}, destination {mis} mod 16"
                            got, intact = pack_guarded(p, dev, mis)
                            assert intact, "guard bands overwritten, " + what
                            check_list_sample(got, sample, 4 * (b + 1), ranges, what)
                finally:
                    part.free()
    finally:
        up.free()


def test_all_dense_fields_with_a_device_partition_take_the_one_launch(dev):
    from dora_amd._lib import ARROW_DEVICE_ROCM, PARTITION_LENGTHS
    from dora_amd.device import DeviceBuffer
    x, y = lr.base(np.float32, (N, 4)), lr.base(np.uint8, (N,))
    rec = [("x", x, x), ("y", y, y)]
    lengths = np.array(lengths_for(5), np.int32)
    sample, info, ranges = lr.oracle(rec, lr.offsets_of(lengths))
    up = Uploaded(rec, dev)
    part = DeviceBuffer.from_bytes(lengths.tobytes(), dev)
    try:
        with lr.plan_list(rec, up.ptr_of, ARROW_DEVICE_ROCM, lengths, PARTITION_LENGTHS,
                          ARROW_DEVICE_ROCM, part_ptr=part.ptr) as p:
            assert p.segments() == [] and p.size == len(sample)
            got, intact = pack_guarded(p, dev, 0)
            assert intact
            check_list_sample(got, sample, 24, ranges, "dense fields, device partition")
    finally:
        part.free()
        up.free()


@pytest.mark.parametrize("what,lengths", [("a sum short of N", [10, 0, 20, 5, 0]),
                                          ("a sum past N", [30, 30, 30, 30, 30]),
                                          ("a negative length", [40, -7, 27, -1, 0])])
def test_an_inconsistent_device_partition_is_clamped_into_a_valid_list(dev, what, lengths):
    """The producer's bug, not a malformed message: exactly the clamped formula's offsets, every
    field as sent, and a ListArray that pyarrow validates in full after download."""
    import pyarrow as pa
    from dora_amd._lib import ARROW_DEVICE_ROCM, PARTITION_LENGTHS, PARTITION_OFFSETS
    from dora_amd.device import DeviceBuffer
    rec = lr.clouds(N)
    up = Uploaded(rec, dev)
    try:
        for dt in (np.int32, np.int64):
            raw_offs = np.concatenate([[0], np.cumsum(lengths)])
            for words, form in ((np.array(lengths, dt), PARTITION_LENGTHS),
                                (raw_offs.astype(dt), PARTITION_OFFSETS)):
                want = lr.clamped_offsets(words, form == PARTITION_OFFSETS, N)
                assert want[0] >= 0 and want[-1] <= N and (np.diff(want) >= 0).all()
                sample, info, ranges = lr.oracle(rec, want)
                part = DeviceBuffer.from_bytes(words.tobytes(), dev)
                try:
                    with lr.plan_list(rec, up.ptr_of, ARROW_DEVICE_ROCM, words, form,
                                      ARROW_DEVICE_ROCM, part_ptr=part.ptr) as p:
                        assert p.size == len(sample)
                        got, intact = pack_guarded(p, dev, 0)
                finally:
                    part.free()
                ctx = f"{what}, {np.dtype(dt)} form {form}"
                assert intact, ctx
                assert np.frombuffer(got[:24], np.int32).tolist() == want.tolist(), ctx
                check_list_sample(got, sample, 24, ranges, ctx)
                # the downloaded sample as the array a receiver builds from it
                child = pa.StructArray.from_arrays(
                    [pa.array(np.frombuffer(got[off:off + ln], v.dtype)) for (off, ln), (_, _, v) in zip(ranges, rec)],
                    names=[name for name, _, _ in rec])
                arr = pa.ListArray.from_arrays(pa.array(np.frombuffer(got[:24], np.int32)), child)
                arr.validate(full=True)
                assert arr.equals(pa.ListArray.from_arrays(pa.array(want), lr.child_of(rec)))
    finally:
        up.free()


def test_a_partition_outside_its_allocation_is_named_and_launches_nothing(dev):
    """Four words of which the last lies past the buffer's end: refused by name before anything
    is launched (so nothing reads it), and the destination keeps its poison."""
    from dora_amd._lib import ARROW_DEVICE_ROCM, PARTITION_LENGTHS, DoraGpuError
    from dora_amd.device import DeviceBuffer
    rec = lr.bare(N)
    up = Uploaded(rec, dev)
    n = 1 << 20
    part, dst = DeviceBuffer(n), DeviceBuffer(n)
    try:
        dst.fill(POISON, dev)
        dev.sync()
        with lr.plan_list(rec, up.ptr_of, ARROW_DEVICE_ROCM, np.zeros(4, np.int32), PARTITION_LENGTHS,
                          ARROW_DEVICE_ROCM, part_ptr=part.ptr + n - 12) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, n, dev)
            assert e.value.code == -1 and "partition: " in str(e.value) and "allocation" in str(e.value)
        dev.sync()
        assert dst.to_bytes(stream=dev) == bytes([POISON]) * n
    finally:
        part.free()
        dst.free()
        up.free()
