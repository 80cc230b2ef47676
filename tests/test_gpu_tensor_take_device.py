"""Take plans through dora_gpu_pack on the GPU (kernel level, no torch): bases and index are
uploaded, every field described over its device pointer, planned with dora_gpu_plan_tensor_take
(ARROW_DEVICE_ROCM) and packed into a poisoned destination with 4 KiB guard bands on both sides.
The cases are those of the sanitized emulation (tests/test_take_index_host.py, from
tests/take_records.py: the same views, K, indices and destinations), every one of which passed
there.  Each field's bytes equal the numpy statement — `values[index]`, a row of zeros where a
word is no row — the guard bands and every padding byte keep the poison, and the type info is the
oracle's for the materialised message.  Ragged takes with the partition in HBM get the clamped
formula's offsets over the K taken rows; one source whose taken rows lie more than 4 GiB apart is
read at 64-bit offsets (only the touched rows are uploaded).  An index whose last word lies past
its allocation and a field that leaves its allocation by one byte are refused with nothing
launched.  Nothing here hands the GPU an address it could fault on: words that are no row are the
defined zero-row case, which reads nothing."""
import numpy as np
import pytest

from tests import gather_views as gv
from tests import list_records as lr
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
    """One destination and one index buffer for the cases of a test: the destination poisoned
    anew for every pack, guard bands included."""

    def __init__(self, stream, size, index_bytes=8 * max(tr.KS)):
        from dora_amd.device import DeviceBuffer
        self.stream = stream
        self.dst = DeviceBuffer(size + 2 * GUARD + 16)
        self.index = DeviceBuffer(max(index_bytes, 8))

    def upload(self, index):
        from dora_amd import _lib
        if index.nbytes:
            self.keep = np.ascontiguousarray(index)  # until the pack's sync
            _lib.call("dora_gpu_memcpy_async", self.index.ptr, self.keep.ctypes.data, index.nbytes,
                      self.stream.handle)
        return self.index.ptr

    def pack(self, plan, mis):
        """(sample bytes, guards intact) of `plan` packed at GUARD + mis."""
        from dora_amd import _lib
        n = plan.size
        span = n + 2 * GUARD + 16
        assert span <= self.dst.size
        _lib.call("dora_gpu_memset_async", self.dst.ptr, POISON, span, self.stream.handle)
        plan.pack(self.dst.ptr + GUARD + mis, n, self.stream)
        self.stream.sync()
        raw = self.dst.to_bytes(span, stream=self.stream)
        lo, hi = raw[:GUARD + mis], raw[GUARD + mis + n:]
        return raw[GUARD + mis:GUARD + mis + n], \
            lo == bytes([POISON]) * len(lo) and hi == bytes([POISON]) * len(hi)

    def free(self):
        self.dst.free()
        self.index.free()


def run_take(arena, up, rec, label, index, mis, **part):
    """Plan, pack and check one take: the fields' bytes, the padding, the guards, the type info."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    offsets = part.pop("offsets_want", None)
    with tr.plan_take(rec, up.ptr_of, ARROW_DEVICE_ROCM, index, ARROW_DEVICE_ROCM,
                      index_ptr=arena.upload(index), **part) as p:
        sample, info, ranges = tr.oracle(rec, index, offsets)
        assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), label
        assert p.segments() == [], label
        got, intact = arena.pack(p, mis)
    assert intact, "guard bands overwritten, " + label
    if offsets is not None:
        obytes = 4 * len(offsets)
        assert np.frombuffer(got[:obytes], np.int32).tolist() == list(offsets), "offsets, " + label
        ranges = [(0, obytes)] + ranges
    check_sample(got, sample, ranges, label)


def plan_bare(ptr, shape, strides, dtype, byte_offset, index_ptr, k, index_dtype):
    """The take plan of one unnamed tensor over `ptr` by `k` words at `index_ptr`."""
    from ctypes import byref, c_void_p
    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM
    from dora_amd.arrow_utils import Plan
    t, keep = tensor._describe(ptr, shape, strides, dtype, byte_offset)
    it, ikeep = tensor._describe(index_ptr, (k,), None, index_dtype)
    tk, keep2 = tensor._describe_take(None, [t], it, ARROW_DEVICE_ROCM, None, 0, ARROW_DEVICE_CPU)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_take", byref(tk), ARROW_DEVICE_ROCM, byref(h))
    return Plan(h.value, (tk, keep, keep2, ikeep))


def sweep(dev, name, b, v):
    rec = [(None, b, v)]
    up = Uploaded(rec, dev)
    arena = Arena(dev, max(tr.KS) * int(np.prod(v.shape[1:])) * v.itemsize)
    try:
        for label, index, mis in tr.sweep(v):
            run_take(arena, up, rec, f"{name} {label}", index, mis)
    finally:
        arena.free()
        up.free()


@pytest.mark.parametrize("dense", [False, True], ids=["cut", "dense"])
@pytest.mark.parametrize("n", [1, 97])
@pytest.mark.parametrize("row", tr.ROWS)
def test_rows_of_every_size(dev, row, n, dense):
    b, v = tr.rows_view(n, row, dense)
    sweep(dev, f"row={row} N={n}", b, v)


@pytest.mark.parametrize("name", tr.VIEWS)
def test_views_whose_dimension_0_differs_in_kind(dev, name):
    b, v = gv.make(name)
    sweep(dev, name, b, v)


def test_a_record_behind_a_host_partitions_offsets(dev):
    from dora_amd._lib import ARROW_DEVICE_CPU, PARTITION_LENGTHS
    rec, cases = tr.three_fields()
    up = Uploaded(rec, dev)
    arena = Arena(dev, 257 * 32 + 64)
    try:
        for label, index, lengths, mis in cases:
            run_take(arena, up, rec, label, index, mis, part=lengths, form=PARTITION_LENGTHS,
                     part_dev=ARROW_DEVICE_CPU, offsets_want=lr.offsets_of(lengths).tolist())
    finally:
        arena.free()
        up.free()


@pytest.mark.parametrize("what,lengths", [("describes the K rows", [0, 30, 0, 35, 0]),
                                          ("a sum short of K", [10, 0, 20, 5, 0]),
                                          ("a sum past K: a partition of the N source rows", [40, 40, 17, 0, 0]),
                                          ("a negative length", [40, -7, 25, -1, 0])])
def test_ragged_takes_with_the_partition_in_hbm(dev, what, lengths):
    """One launch scans the partition, clamped to K, and takes the rows: the offsets are the
    clamped formula's over K = 65 taken rows (N = 97), int32 and int64, lengths and offsets."""
    from dora_amd._lib import ARROW_DEVICE_ROCM, PARTITION_LENGTHS, PARTITION_OFFSETS
    from dora_amd.device import DeviceBuffer
    rec, _ = tr.three_fields()
    k = 65
    up = Uploaded(rec, dev)
    arena = Arena(dev, k * 32 + 64)
    try:
        for wide in (0, 1):
            dt = np.int64 if wide else np.int32
            raw_offs = np.concatenate([[0], np.cumsum(lengths)])
            for label, index in tr.indices(k, 97, wide)[3:]:
                for words, form in ((np.array(lengths, dt), PARTITION_LENGTHS),
                                    (raw_offs.astype(dt), PARTITION_OFFSETS)):
                    want = lr.clamped_offsets(words, form == PARTITION_OFFSETS, k)
                    assert want[0] >= 0 and want[-1] <= k and (np.diff(want) >= 0).all()
                    part = DeviceBuffer.from_bytes(words.tobytes(), dev)
                    try:
                        run_take(arena, up, rec, f"{what}, {np.dtype(dt)} form {form}, {label}", index,
                                 4 * form, part=words, form=form, part_dev=ARROW_DEVICE_ROCM,
                                 part_ptr=part.ptr, offsets_want=want.tolist())
                    finally:
                        part.free()
    finally:
        arena.free()
        up.free()


def test_no_rows_taken_and_no_source_rows(dev):
    """K == 0 is an empty message: nothing to pack.  N == 0 with K > 0 is K rows of zeros from a
    NULL source, whatever the words."""
    from dora_amd._lib import ARROW_DEVICE_ROCM
    out = lr.base(np.float32, (10, 6))
    rec = [(None, out, out[:, :4])]
    up = Uploaded(rec, dev)
    arena = Arena(dev, 4096)
    try:
        with tr.plan_take(rec, up.ptr_of, ARROW_DEVICE_ROCM, np.zeros(0, np.int64), ARROW_DEVICE_ROCM,
                          index_ptr=0) as p:
            assert p.size == 0
            p.pack(None, 0, dev)
            dev.sync()
        none = np.zeros((0, 6), np.float32)
        rec0 = [(None, none, none[:, :4])]
        for index in (np.array([0, -1, 5, 1 << 20], np.int32), np.array([3, 1 << 40, 0], np.int64)):
            with tr.plan_take(rec0, lambda b: 0, ARROW_DEVICE_ROCM, index, ARROW_DEVICE_ROCM,
                              index_ptr=arena.upload(index)) as p:
                assert p.size == 16 * len(index)
                got, intact = arena.pack(p, 4)
            assert intact and got == bytes(16 * len(index))
    finally:
        arena.free()
        up.free()


def test_taken_rows_more_than_4_gib_apart(dev):
    """A (4300, 64) uint8 source with a row stride of 2^20 + 3: rows 0, 1, 4097 and 4299 start
    more than 4 GiB apart.  Only those rows are uploaded, and only they are taken (with one word
    that is no row): the offsets are 64-bit all the way."""
    from dora_amd import _lib
    from dora_amd._lib import DoraGpuError
    from dora_amd.device import DeviceBuffer
    rows, cols, stride = 4300, 64, 2 ** 20 + 3
    span = (rows - 1) * stride + cols
    assert 4097 * stride > 2 ** 32
    try:
        src = DeviceBuffer(span)
    except DoraGpuError as e:
        pytest.skip(f"no {span} byte allocation on this GPU: {e}")
    arena = Arena(dev, 16 * cols)
    try:
        touched = {r: gv.base(np.uint8, (cols,)) + np.uint8(r % 251) for r in (0, 1, 4097, 4299)}
        for r, data in touched.items():
            _lib.call("dora_gpu_memcpy_async", src.ptr + r * stride, data.ctypes.data, cols, dev.handle)
        dev.sync()
        for index in (np.array([4299, 0, 4097, 4300, 1, 4299], np.int64),
                      np.array([1, 4097, -1, 4299, 0], np.int32)):
            with plan_bare(src.ptr, (rows, cols), (stride, 1), np.uint8, 0, arena.upload(index),
                           len(index), index.dtype) as p:
                assert p.size == len(index) * cols
                got, intact = arena.pack(p, 3)
            want = b"".join(touched[int(w)].tobytes() if int(w) in touched else bytes(cols) for w in index)
            assert intact and got == want
    finally:
        arena.free()
        src.free()


def test_an_index_or_a_field_outside_its_allocation_launches_nothing(dev):
    """The index's last word past its buffer's end, and a field whose last source row ends one
    byte past its buffer: each refused by name before anything is launched, and the destination
    keeps its poison.  Moved back inside, both are accepted."""
    from dora_amd._lib import DoraGpuError
    from dora_amd.device import DeviceBuffer
    n = 1 << 20
    src, idx, dst = DeviceBuffer(n), DeviceBuffer(n), DeviceBuffer(n)

    def plan(index_ptr, k, off):
        # 64 source rows of 16 bytes, n / 64 apart, the last ending at byte off + 63 * (n / 64) + 16
        return plan_bare(src.ptr, (64, 16), (n // 64, 1), np.uint8, off, index_ptr, k, np.int32)

    try:
        dst.fill(POISON, dev)
        idx.fill(0, dev)
        dev.sync()
        inside = n - (63 * (n // 64) + 16)
        with plan(idx.ptr + n - 12, 4, inside) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, n, dev)
            assert e.value.code == -1 and "index: " in str(e.value) and "allocation" in str(e.value)
        with plan(idx.ptr, 4, inside + 1) as p:
            with pytest.raises(DoraGpuError) as e:
                p.pack(dst.ptr, n, dev)
            assert e.value.code == -1 and "allocation" in str(e.value) and "index" not in str(e.value)
        dev.sync()
        assert dst.to_bytes(stream=dev) == bytes([POISON]) * n  # nothing was launched
        with plan(idx.ptr + n - 16, 4, inside) as p:
            p.pack(dst.ptr, n, dev)
        dev.sync()
    finally:
        src.free()
        idx.free()
        dst.free()
