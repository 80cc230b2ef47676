"""Mask plans through dora_gpu_pack on the GPU (kernel level, no torch): bases and mask are
uploaded, every field described over its device pointer, planned with dora_gpu_plan_tensor_mask
(ARROW_DEVICE_ROCM) and packed into a poisoned destination that holds the sample and the plan's
workspace, with 4 KiB guard bands around both.  The shapes and masks are those of the sanitized
emulation (tests/test_mask_index_host.py, from tests/mask_records.py), every one of which passed
there: N across every seam of the 4096-row tile and one case of 257 tiles, the mask at 0, 1, 3
and 13 mod 16, destinations at 0, 4, 8 and 12 mod 16.  The sample's bytes equal the numpy
statement — the K selected rows in source order, zero rows up to N, offsets C[p] — the guard
bands and every padding byte keep the poison, and the type info is the oracle's.  Ragged masks
with the partition on the host and in HBM, garbage words included, get the clamped formula's
offsets looked up in C.  A mask one byte past its allocation and a destination one byte short of
sample plus workspace are refused with nothing launched.  Nothing here hands the GPU an address
it could fault on."""
import numpy as np
import pytest

from tests import list_records as lr
from tests import mask_records as mr
from tests import take_records as tr
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


class Arena:
    """One destination and one mask buffer for the cases of a test: the destination poisoned
    anew for every pack, guard bands included."""

    def __init__(self, stream, size, rows):
        from dora_amd.device import DeviceBuffer
        self.stream = stream
        self.dst = DeviceBuffer(size + 2 * GUARD + 16)
        self.mask = DeviceBuffer(rows + 32)

    def upload(self, mask, shift):
        """The mask's bytes at `shift` mod 16 (allocations are 256-byte aligned)."""
        from dora_amd import _lib
        assert self.mask.ptr % 16 == 0 and len(mask) + shift <= self.mask.size
        if mask.nbytes:
            self.keep = np.ascontiguousarray(mask)  # until the pack's sync
            _lib.call("dora_gpu_memcpy_async", self.mask.ptr + shift, self.keep.ctypes.data,
                      mask.nbytes, self.stream.handle)
        return self.mask.ptr + shift

    def pack(self, plan, mis):
        """(sample bytes, guards intact) of `plan` packed at GUARD + mis, its workspace behind."""
        from dora_amd import _lib
        n, room = plan.size, plan.size + mr.workspace_size(plan)
        span = room + 2 * GUARD + 16
        assert span <= self.dst.size
        _lib.call("dora_gpu_memset_async", self.dst.ptr, POISON, span, self.stream.handle)
        plan.pack(self.dst.ptr + GUARD + mis, room, self.stream)
        self.stream.sync()
        raw = self.dst.to_bytes(span, stream=self.stream)
        lo, hi = raw[:GUARD + mis], raw[GUARD + mis + room:]
        return raw[GUARD + mis:GUARD + mis + n], \
            lo == bytes([POISON]) * len(lo) and hi == bytes([POISON]) * len(hi)

    def free(self):
        self.dst.free()
        self.mask.free()


def room_for(rec, n, lists=1):
    """Bytes a destination needs for `rec` over n rows: sample, padding and workspace."""
    row = sum(int(np.prod(v.shape[1:])) * v.itemsize for _, _, v in rec)
    return n * row + 64 + 4 * (lists + 1) * 2 + 4 * (2 * n + 2 + (n + 15) // mr.TILE + 1) + 16


def run_mask(arena, up, rec, label, mask, shift, mis, **part):
    """Plan, pack and check one mask: offsets, fields' bytes, padding, guards, type info."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    offsets = part.pop("offsets_want", None)
    with mr.plan_mask(rec, up.ptr_of, ARROW_DEVICE_ROCM, mask, ARROW_DEVICE_ROCM,
                      mask_ptr=arena.upload(mask, shift), **part) as p:
        n = len(mask)
        sample, info, ranges = mr.oracle(rec, mask, None if offsets is None else [0] * len(offsets))
        assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), label
        assert p.segments() == [] and mr.workspace_size(p) >= 4 * (2 * n + 2), label
        got, intact = arena.pack(p, mis)
    assert intact, "guard bands overwritten, " + label
    want = [0, int((mask != 0).sum())] if offsets is None else list(offsets)
    obytes = 4 * len(want)
    assert np.frombuffer(got[:obytes], np.int32).tolist() == want, "offsets, " + label
    check_sample(got[obytes:], sample[obytes:], [(o - obytes, ln) for o, ln in ranges], label)


@pytest.mark.parametrize("shift", mr.SHIFTS)
def test_the_emulations_shapes_and_masks(dev, shift):
    turn = 0
    for n in mr.SIZES[1:]:
        rec = lr.bare(n)
        up = Uploaded(rec, dev)
        arena = Arena(dev, room_for(rec, n), n)
        try:
            for label, mask in mr.masks(n):
                mis = mr.DSTS[turn % len(mr.DSTS)]
                turn += 1
                run_mask(arena, up, rec, f"N={n} {label} mask%16={shift} dst%16={mis}", mask,
                         shift, mis)
        finally:
            arena.free()
            up.free()


def test_more_tiles_than_threads(dev):
    n = mr.MANY_TILES
    b, v = tr.rows_view(n, 4, False)
    rec = [(None, b, v)]
    up = Uploaded(rec, dev)
    arena = Arena(dev, room_for(rec, n), n)
    try:
        run_mask(arena, up, rec, "257 tiles and 3 rows", mr.masks(n)[3][1], 3, 8)
    finally:
        arena.free()
        up.free()


def test_no_rows(dev):
    """N == 0: all-zero offsets from the plan itself, nothing launched, no workspace."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    rec = lr.clouds(0)
    arena = Arena(dev, 256, 0)
    try:
        with mr.plan_mask(rec, lambda b: 0, ARROW_DEVICE_ROCM, np.zeros(0, np.uint8),
                          ARROW_DEVICE_ROCM, mask_ptr=0) as p:
            assert p.size == 8 and mr.workspace_size(p) == 0
            got, intact = arena.pack(p, 4)
        assert intact and got == bytes(8)
    finally:
        arena.free()


@pytest.mark.parametrize("n", [97, 257, mr.TILE + 1])
def test_a_record_bare_and_under_a_host_partition(dev, n):
    """tests/take_records.py's record of three fields (rows of 16, 8 and 3 bytes, each cut from a
    wider base): one list, and the lists of a checked host partition whose offsets the launch
    looks up in C — lengths and offsets, int32 and int64."""
    from dora_amd._lib import ARROW_DEVICE_CPU, PARTITION_LENGTHS, PARTITION_OFFSETS
    rec, _ = tr.three_fields(n)
    up = Uploaded(rec, dev)
    arena = Arena(dev, room_for(rec, n, 16), n)
    turn = 0
    try:
        for label, mask in mr.masks(n):
            for shift in (0, 13):
                mis = mr.DSTS[turn % len(mr.DSTS)]
                turn += 1
                run_mask(arena, up, rec, f"record N={n} {label} mask%16={shift} dst%16={mis}",
                         mask, shift, mis)
            for lengths in lr.partitions(n):
                offs = lr.offsets_of(lengths)
                want = mr.counts(mask)[offs].tolist()
                for part, form in ((np.array(lengths, np.int32), PARTITION_LENGTHS),
                                   (offs.astype(np.int64), PARTITION_OFFSETS)):
                    mis = mr.DSTS[turn % len(mr.DSTS)]
                    turn += 1
                    run_mask(arena, up, rec, f"record N={n} {label} B={len(lengths)} form={form} "
                             f"dst%16={mis}", mask, 3, mis, part=part, form=form,
                             part_dev=ARROW_DEVICE_CPU, offsets_want=want)
    finally:
        arena.free()
        up.free()


@pytest.mark.parametrize("what,lengths", [("describes the N rows", [0, 100, 0, 157, 0]),
                                          ("a sum short of N", [10, 0, 20, 5, 0]),
                                          ("a sum past N", [200, 200, 17, 0, 0]),
                                          ("a negative length", [40, -7, 25, -1, 0]),
                                          ("garbage", [1 << 30, -(1 << 31), 7, (1 << 31) - 1, 3])])
def test_ragged_masks_with_the_partition_in_hbm(dev, what, lengths):
    """The launch scans the partition, clamped to the N = 257 source rows, and stores C[o] for
    the offset o: monotone, at most K, whatever the words hold — int32 and int64, lengths and
    offsets."""
    from dora_amd._lib import ARROW_DEVICE_ROCM, PARTITION_LENGTHS, PARTITION_OFFSETS
    from dora_amd.device import DeviceBuffer
    n = 257
    rec, _ = tr.three_fields(n)
    up = Uploaded(rec, dev)
    arena = Arena(dev, room_for(rec, n, 8), n)
    try:
        for wide in (0, 1):
            dt = np.int64 if wide else np.int32
            raw_offs = np.concatenate([[0], np.cumsum(np.array(lengths, np.int64))])
            if not wide:
                raw_offs = raw_offs.astype(np.int32)  # (wrapped words are garbage like any other)
            for label, mask in (mr.masks(n)[i] for i in (0, 1, 3, 6)):
                c = mr.counts(mask)
                for words, form in ((np.array(lengths, dt), PARTITION_LENGTHS),
                                    (raw_offs.astype(dt), PARTITION_OFFSETS)):
                    o = lr.clamped_offsets(words, form == PARTITION_OFFSETS, n)
                    want = c[o]
                    assert want[0] >= 0 and want[-1] <= c[-1] and (np.diff(want) >= 0).all()
                    part = DeviceBuffer.from_bytes(words.tobytes(), dev)
                    try:
                        run_mask(arena, up, rec, f"{what}, {np.dtype(dt)} form {form}, {label}",
                                 mask, 1, 4 * form + 4, part=words, form=form,
                                 part_dev=ARROW_DEVICE_ROCM, part_ptr=part.ptr,
                                 offsets_want=want.tolist())
                    finally:
                        part.free()
    finally:
        arena.free()
        up.free()


def plan_bare(ptr, shape, dtype, mask_ptr, n):
    """The mask plan of one unnamed dense tensor over `ptr` by `n` bytes at `mask_ptr`."""
    from ctypes import byref, c_void_p
    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM
    from dora_amd.arrow_utils import Plan
    t, keep = tensor._describe(ptr, shape, None, dtype)
    mt, mkeep = tensor._describe(mask_ptr, (n,), None, np.uint8)
    mk, keep2 = tensor._describe_mask(None, [t], mt, ARROW_DEVICE_ROCM, None, 0, ARROW_DEVICE_CPU)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_mask", byref(mk), ARROW_DEVICE_ROCM, byref(h))
    return Plan(h.value, (mk, keep, keep2, mkeep))


def test_a_mask_outside_its_allocation_or_a_short_destination_launches_nothing(dev):
    """The mask's last byte past its buffer's end, and a destination one byte short of sample
    plus workspace: each refused before anything is launched, naming the mask or both numbers,
    and the destination keeps its poison.  Moved back inside, both are accepted."""
    from dora_amd._lib import DoraGpuError
    from dora_amd.device import DeviceBuffer
    n = 1 << 16
    src, msk, dst = DeviceBuffer(16 * n), DeviceBuffer(n), DeviceBuffer(32 * n)
    try:
        dst.fill(POISON, dev)
        msk.fill(1, dev)
        src.fill(7, dev)
        dev.sync()
        with plan_bare(src.ptr, (n - 8, 4), np.float32, msk.ptr + 9, n - 8) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, dst.size, dev)
            assert e.value.code == -1 and "mask: " in str(e.value) and "allocation" in str(e.value)
        with plan_bare(src.ptr, (n - 8, 4), np.float32, msk.ptr + 8, n - 8) as p:
            size, ws = p.size, mr.workspace_size(p)
            assert ws > 8 * (n - 8) and size + ws <= dst.size
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, size + ws - 1, dev)
            assert e.value.code == -1 and f"sample: {size}" in str(e.value) and \
                f"workspace: {ws}" in str(e.value)
            dev.sync()
            assert dst.to_bytes(stream=dev) == bytes([POISON]) * dst.size  # nothing was launched
            p.pack(dst.ptr, size + ws, dev)
            dev.sync()
            got = dst.to_bytes(size, stream=dev)
            assert np.frombuffer(got[:8], np.int32).tolist() == [0, n - 8]
            assert got[8:] == bytes([7]) * (size - 8)
    finally:
        src.free()
        msk.free()
        dst.free()
