"""The seeded sweep of tests/test_random_views_host.py on the GPU (kernel level, no torch): the same
cases, a fixed subset of each body's seeds, through dora_gpu_pack into a poisoned destination with
4 KiB guard bands on both sides.  This is what the emulation cannot see: the real memory policies
(the funnel at every shift, the write-through stores, the tile kernel's LDS round trip, the cast
body's vector loads) at shapes and alignments nobody chose.

Every case: the bytes equal numpy's, the type info is the oracle's, both guard bands and every
padding byte keep the poison.  Device indices hold words that are no row, device partitions hold
garbage.  Every view was first checked to lie inside its base, and every base lies inside the
one source buffer a test allocates: nothing here hands the GPU an address it could fault on.  A
cast whose source is off its element size is refused with nothing launched.

The op kernels (quantise, affine, argmax, resize, crops, and the model-input forms of the last two,
gather_resize_prep_kernel and gather_crop_prep_kernel) run the first 200 seeds of their host
ranges through `run_op`: the bytes of every field equal the op's `want` through its `same`.  Affine
tables go to the words buffer at 4, 8, 12 and 0 mod 16 in turn; a crop's boxes are bases like its
frame, and garbage lives only in their words, which the kernel clamps by contract.  Argmax packs
every seed under the body the library chooses and, wherever the wave body applies, under the other
one.  20 seeds per op put the op on a source off its element size: refused by the field's name,
the destination keeps its poison.

Each test allocates its buffers once, for its largest case, and poisons the destination anew for
every pack.  A failure prints `seed=`: tests/random_views.py reproduces the case from it."""
import numpy as np
import pytest

from tests import affine_records as ar
from tests import argmax_records as am
from tests import cast_records as cr
from tests import crop_records as kr
from tests import mask_records as mr
from tests import prep_records as pr
from tests import quant_records as qr
from tests import random_views as rv
from tests import resize_records as rr
from tests import struct_records as sr
from tests import take_records as tr
from tests import test_random_views_host as host
from tests.gather_views import describe_view, misalignment
from tests.test_gpu_tensor_mask_device import run_mask
from tests.test_gpu_tensor_struct_device import GUARD, POISON, check_sample
from tests.test_gpu_tensor_take_device import run_take

pytestmark = pytest.mark.gpu

BARE_SEEDS = host.BARE_SEEDS[:200]
RECORD_SEEDS = host.RECORD_SEEDS[:150]
TAKE_SEEDS = host.TAKE_SEEDS[:200]
CAST_SEEDS = host.CAST_SEEDS[:200]
MASK_SEEDS = host.MASK_SEEDS[:150]
QUANT_SEEDS = host.QUANT_SEEDS[:200]
AFFINE_SEEDS = host.AFFINE_SEEDS[:200]
ARGMAX_SEEDS = host.ARGMAX_SEEDS[:200]
RESIZE_SEEDS = host.RESIZE_SEEDS[:200]
CROP_SEEDS = host.CROP_SEEDS[:200]
PREP_RESIZE_SEEDS = host.PREP_RESIZE_SEEDS[:200]
PREP_CROP_SEEDS = host.PREP_CROP_SEEDS[:200]


@pytest.fixture(scope="module")
def dev():
    from dora_amd import device
    assert device.device_count() >= 1
    device.set_device(0)
    s = device.Stream()
    yield s
    s.close()


def slot(nbytes):
    """The room a base takes in the source buffer: its bytes, its misalignment, 256-byte slots."""
    return (nbytes + 16 + 255) // 256 * 256


class Buffers:
    """One source buffer, one destination and one buffer for index, mask and partition words,
    allocated once for the cases of a test: the bases of a case are copied into 256-byte slots of
    the source buffer, each as many bytes past its slot's start as it is misaligned on the host,
    and the destination is poisoned anew for every pack, guard bands and workspace included."""

    def __init__(self, stream, src_bytes, dst_bytes, words_bytes=64):
        from dora_amd.device import DeviceBuffer
        self.stream = stream
        self.src = DeviceBuffer(max(src_bytes, 256))
        self.dst = DeviceBuffer(dst_bytes + 2 * GUARD + 16)
        self.words = DeviceBuffer(words_bytes + 64)
        self.ptrs, self.keep = {}, []
        assert self.src.ptr % 256 == 0 and self.words.ptr % 16 == 0

    def copy(self, ptr, array):
        from dora_amd import _lib
        host_copy = np.frombuffer(array.tobytes(), np.uint8)
        if host_copy.nbytes:
            self.keep.append(host_copy)  # until the next sync
            _lib.call("dora_gpu_memcpy_async", ptr, host_copy.ctypes.data, host_copy.nbytes,
                      self.stream.handle)

    def place(self, bases):
        self.ptrs, at = {}, 0
        for b in bases:
            assert at + slot(b.nbytes) <= self.src.size
            self.ptrs[id(b)] = self.src.ptr + at + misalignment(b)
            self.copy(self.ptrs[id(b)], b)
            at += slot(b.nbytes)

    def ptr_of(self, b):
        return self.ptrs[id(b)]

    def upload(self, words, shift=0):
        """Index or mask words at `shift` mod 16 of the words buffer."""
        assert shift + words.nbytes <= self.words.size
        self.copy(self.words.ptr + shift, words)
        return self.words.ptr + shift

    def pack(self, plan, mis):
        """(sample bytes, guards intact) of `plan` packed at GUARD + mis, its workspace behind."""
        from dora_amd import _lib
        n, room = plan.size, plan.size + mr.workspace_size(plan)
        span = room + 2 * GUARD + 16
        assert span <= self.dst.size
        _lib.call("dora_gpu_memset_async", self.dst.ptr, POISON, span, self.stream.handle)
        plan.pack(self.dst.ptr + GUARD + mis, room, self.stream)
        self.stream.sync()
        self.keep = []
        raw = self.dst.to_bytes(span, stream=self.stream)
        lo, hi = raw[:GUARD + mis], raw[GUARD + mis + room:]
        return raw[GUARD + mis:GUARD + mis + n], \
            lo == bytes([POISON]) * len(lo) and hi == bytes([POISON]) * len(hi)

    def untouched(self, n):
        """The first n bytes of the destination still hold the poison."""
        self.stream.sync()
        return self.dst.to_bytes(n, stream=self.stream) == bytes([POISON]) * n

    def free(self):
        for b in (self.src, self.dst, self.words):
            b.free()


def source_room(recs):
    return max(sum(slot(b.nbytes) for b in sr.bases_of(rec)) for rec in recs)


def sample_room(recs, lists=8):
    """Bytes the largest sample of `recs` takes: fields, padding, offsets; the mask workspace."""
    out = 0
    for rec in recs:
        n = rec[0][2].shape[0]
        row = sum(int(np.prod(v.shape[1:])) * v.itemsize for _, _, v in rec)
        out = max(out, n * row + 64 * (len(rec) + 1) + 8 * (lists + 1) +
                  4 * (2 * n + 2 + (n + 15) // mr.TILE + 1) + 64)
    return out


def test_bare_views(dev):
    from dora_amd import _lib, tensor
    from oracle.pack_ref import pack
    from tests.test_gpu_tensor_device import plan_device
    cases = [host.bare_case(seed) for seed in BARE_SEEDS]
    bufs = Buffers(dev, source_room([[(None, b, v)] for b, v, _, _ in cases]),
                   max(v.size * v.itemsize for _, v, _, _ in cases))
    try:
        for seed, (b, v, mis, tile_mis) in zip(BARE_SEEDS, cases):
            assert rv.inside(b, v), seed
            want, info = pack(tensor.from_numpy(v))
            assert bytes(want) == np.ascontiguousarray(v).tobytes()
            bufs.place([b])
            shape, strides, dtype, off = describe_view(b, v, None)
            with plan_device(bufs.ptr_of(b), shape, strides, dtype, off) as p:
                assert p.size == len(want) and p.type_info().to_json() == info.to_json(), seed
                # the library's selection, the rows body forced, the tile body wherever it applies
                for mode, at in ((0, mis), (1, mis), (2, tile_mis), (0, tile_mis)):
                    _lib.call("dora_gpu_test_gather_kernel", mode)
                    what = f"seed={seed} kernel {mode} dst%16={at}"
                    got, intact = bufs.pack(p, at)
                    assert intact, "guard bands overwritten, " + what
                    assert got == bytes(want), what
    finally:
        _lib.call("dora_gpu_test_gather_kernel", 0)
        bufs.free()


def test_records(dev):
    from dora_amd import _lib
    from dora_amd._lib import ARROW_DEVICE_ROCM
    cases = [host.record_case(seed) for seed in RECORD_SEEDS]
    recs = [rec for rec, _ in cases]
    bufs = Buffers(dev, source_room(recs), sample_room(recs))
    try:
        for seed, (rec, mis) in zip(RECORD_SEEDS, cases):
            assert all(rv.inside(b, v) for _, b, v in rec), seed
            sample, info, ranges = sr.oracle(rec)
            bufs.place(sr.bases_of(rec))
            with sr.plan_record(rec, bufs.ptr_of, ARROW_DEVICE_ROCM) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), seed
                for mode in (0, 1, 2):
                    _lib.call("dora_gpu_test_gather_kernel", mode)
                    what = f"seed={seed} kernel {mode} dst%16={mis}"
                    got, intact = bufs.pack(p, mis)
                    assert intact, "guard bands overwritten, " + what
                    check_sample(got, sample, ranges, what)
    finally:
        _lib.call("dora_gpu_test_gather_kernel", 0)
        bufs.free()


def test_takes(dev):
    """Every seed's take (words that are no row among them, a checked host partition for half),
    and once more behind a garbage partition in HBM, which the launch scans and clamps."""
    from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, PARTITION_LENGTHS, PARTITION_OFFSETS
    cases = [host.take_case(seed) for seed in TAKE_SEEDS]
    invalid = garbage = 0
    rows = max(len(c[2]) for c in cases)
    taken = [tr.taken_record(rec, np.zeros(rows, np.int32)) for rec, *_ in cases]
    bufs = Buffers(dev, source_room([c[0] for c in cases]), sample_room(taken), 8 * rows + 256)
    try:
        for seed, (rec, label, index, mis, lengths, (words, form, offs)) in zip(TAKE_SEEDS, cases):
            assert all(rv.inside(b, v) for _, b, v in rec), seed
            n = rec[0][2].shape[0]
            invalid += bool(((index < 0) | (index >= n)).any())
            garbage += bool(((words < 0) | (words > len(index))).any())
            bufs.place(sr.bases_of(rec))
            what = f"seed={seed} {label} dst%16={mis}"
            if lengths is None:
                run_take(bufs, bufs, rec, what, index, mis)
            else:
                run_take(bufs, bufs, rec, what, index, mis, part=lengths, form=PARTITION_LENGTHS,
                         part_dev=ARROW_DEVICE_CPU,
                         offsets_want=np.concatenate([[0], np.cumsum(lengths)]).tolist())
            # (the index's words first, the partition's behind them on a multiple of 16)
            part_ptr = bufs.upload(words, (index.nbytes + 15) // 16 * 16)
            run_take(bufs, bufs, rec, what + ", garbage partition in HBM", index, mis // 4 * 4,
                     part=words, form=PARTITION_OFFSETS if form else PARTITION_LENGTHS,
                     part_dev=ARROW_DEVICE_ROCM, part_ptr=part_ptr, offsets_want=offs.tolist())
        assert invalid >= 20 and garbage >= 20, (invalid, garbage)
    finally:
        bufs.free()


def test_casts(dev):
    from dora_amd._lib import ARROW_DEVICE_ROCM, DoraGpuError
    cases = [host.cast_case(seed) for seed in CAST_SEEDS]
    refused = [rv.misaligned_cast(rv.rng(seed)) for seed in host.MISALIGNED_CAST_SEEDS]
    recs = [[r[:3] for r in rec] for rec, _ in cases] + [[r[:3] for r in rec] for rec in refused]
    bufs = Buffers(dev, source_room(recs), max(len(cr.oracle(rec)[0]) for rec, _ in cases) + 64)
    try:
        for seed, (rec, mis) in zip(CAST_SEEDS, cases):
            assert all(rv.inside(b, v) for _, b, v, _ in rec), seed
            what = f"seed={seed} dst%16={mis}"
            sample, info, ranges = cr.oracle(rec)
            bufs.place(cr.bases_of(rec))
            with cr.plan_cast(rec, bufs.ptr_of, ARROW_DEVICE_ROCM) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), what
                assert p.segments() == [], what
                got, intact = bufs.pack(p, mis)
            assert intact, "guard bands overwritten, " + what
            pad = bytearray(got)
            for (off, ln), (_, _, v, c) in zip(ranges, rec):
                cr.same(got[off:off + ln], cr.want(v, c), what)
                pad[off:off + ln] = bytes([POISON]) * ln
            assert bytes(pad) == bytes([POISON]) * len(got), "padding written, " + what
        # a cast of a source off its element size: refused by name, nothing launched
        bufs.dst.fill(POISON, dev)
        for seed, rec in zip(host.MISALIGNED_CAST_SEEDS, refused):
            bufs.place(cr.bases_of(rec))
            assert bufs.ptr_of(rec[1][1]) % rec[1][1].itemsize in (1, 3)
            with pytest.raises(DoraGpuError) as e:
                with cr.plan_cast(rec, bufs.ptr_of, ARROW_DEVICE_ROCM) as p:
                    p.pack(bufs.dst.ptr + GUARD, p.size, dev)
            assert e.value.code == -1 and "field 1 `f1`" in str(e.value), (seed, str(e.value))
        assert bufs.untouched(bufs.dst.size)
    finally:
        bufs.free()


# ---------------------------------------------------------------------------------------------
# The op bodies: quantise, affine, argmax, resize, crops
# ---------------------------------------------------------------------------------------------
class Op:
    """What the sweep of one op kernel needs of its tests/*_records.py: the record's (name, base,
    view) triples (a crop's boxes and nothing else are bases too), its oracle, its plan over the
    buffers, the wanted array of a field and the comparison."""

    def __init__(self, name, triples, oracle, plan, want, same):
        self.name, self.triples, self.oracle, self.plan = name, triples, oracle, plan
        self.want, self.same = want, same


def first_three(rec):
    return [x[:3] for x in rec]


def upload_tables(bufs, rec):
    """The tables of an affine record in the words buffer, each at 4, 8, 12 or 0 mod 16 in turn;
    {id(table): device pointer}."""
    ptrs, at = {}, 0
    for k, t in enumerate(ar.tables_of(rec)):
        at = (at + 15) // 16 * 16 + 4 * ((k + 1) % 4)
        ptrs[id(t)] = bufs.upload(t, at)
        at += t.nbytes
    return ptrs


def plan_affine(rec, bufs):
    from dora_amd._lib import ARROW_DEVICE_ROCM
    ptrs = upload_tables(bufs, rec)
    return ar.plan_affine(rec, bufs.ptr_of, ARROW_DEVICE_ROCM, lambda t: ptrs[id(t)])


def device_plan(plan):
    from dora_amd._lib import ARROW_DEVICE_ROCM
    return lambda rec, bufs: plan(rec, bufs.ptr_of, ARROW_DEVICE_ROCM)


OPS = {
    "quant": Op("quant", first_three, qr.oracle, device_plan(qr.plan_convert),
                lambda x: qr.want(x[2], x[3]), qr.same),
    "affine": Op("affine", first_three, ar.oracle, plan_affine,
                 lambda x: ar.want(x[2], x[3], x[4]), ar.same),
    "argmax": Op("argmax", first_three, am.oracle, device_plan(am.plan_reduce),
                 lambda x: am.want(x[2], x[3]), am.same),
    "resize": Op("resize", first_three, rr.oracle, device_plan(rr.plan_resize),
                 lambda x: rr.want(x[2], x[3]), rr.same),
    "crop": Op("crop", kr.triples, kr.oracle, device_plan(kr.plan_crop),
               lambda x: kr.want(x[2], x[3]), kr.same),
    # (tables and boxes are bases of the record: placed in the source buffer like the frames)
    "prep_resize": Op("prep_resize", pr.triples, pr.oracle, device_plan(pr.plan_prep),
                      lambda x: pr.want(x[2], x[3]), pr.same),
    "prep_crop": Op("prep_crop", pr.triples, pr.oracle, device_plan(pr.plan_prep),
                    lambda x: pr.want(x[2], x[3]), pr.same),
}


def table_room(recs):
    return max([sum(t.nbytes + 32 for t in ar.tables_of(rec)) for rec in recs if len(rec[0]) == 5]
               + [64])


def check_fields(op, got, rec, ranges, what):
    """Every field's bytes are the op's `want`, every byte outside the fields keeps the poison."""
    pad = bytearray(got)
    for (off, ln), x in zip(ranges, rec):
        op.same(got[off:off + ln], op.want(x), what)
        pad[off:off + ln] = bytes([POISON]) * ln
    assert bytes(pad) == bytes([POISON]) * len(got), "padding written, " + what


def run_op(dev, op, seeds, cases, refused_seeds, other_bodies=None):
    """The sweep of one op kernel: every case of `cases` ((record, destination mod 16, ..) of
    `seeds`) packed and compared, then the misaligned records of `refused_seeds` refused by name
    with nothing launched.  `other_bodies(plan, rec, mis)` yields what to pack once more."""
    from dora_amd._lib import DoraGpuError
    refused = [rv.misaligned_op(rv.rng(seed), op.name) for seed in refused_seeds]
    recs = [c[0] for c in cases]
    oracles = [op.oracle(rec) for rec in recs]
    bufs = Buffers(dev, source_room([op.triples(rec) for rec in recs + refused]),
                   max(len(o[0]) for o in oracles) + 64, table_room(recs + refused))
    try:
        for seed, case, (sample, info, ranges) in zip(seeds, cases, oracles):
            rec, mis = case[0], case[1]
            what = f"seed={seed} dst%16={mis}"
            assert all(rv.inside(b, v) for _, b, v in op.triples(rec)), what
            bufs.place(sr.bases_of(op.triples(rec)))
            with op.plan(rec, bufs) as p:
                assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), what
                assert p.segments() == [], what
                got, intact = bufs.pack(p, mis)
                assert intact, "guard bands overwritten, " + what
                check_fields(op, got, rec, ranges, what)
            for label in (other_bodies(rec, mis, bufs) if other_bodies else ()):
                with op.plan(rec, bufs) as p:
                    got, intact = bufs.pack(p, mis)
                assert intact, f"guard bands overwritten, {what} {label}"
                check_fields(op, got, rec, ranges, f"{what} {label}")
        # an op on a source off its element size: refused by name, nothing launched
        bufs.dst.fill(POISON, dev)
        for seed, rec in zip(refused_seeds, refused):
            bufs.place(sr.bases_of(op.triples(rec)))
            assert bufs.ptr_of(rec[1][1]) % rec[1][1].itemsize in (1, 3)
            with pytest.raises(DoraGpuError) as e:
                with op.plan(rec, bufs) as p:
                    p.pack(bufs.dst.ptr + GUARD, p.size, dev)
            assert e.value.code == -1 and "field 1 `f1`" in str(e.value), (f"seed={seed}", str(e.value))
        assert bufs.untouched(bufs.dst.size)
    finally:
        bufs.free()


def test_quants(dev):
    run_op(dev, OPS["quant"], QUANT_SEEDS, [host.quant_case(s) for s in QUANT_SEEDS],
           host.MISALIGNED_QUANT_SEEDS)


def test_affines(dev):
    run_op(dev, OPS["affine"], AFFINE_SEEDS, [host.affine_case(s) for s in AFFINE_SEEDS],
           host.MISALIGNED_AFFINE_SEEDS)


def test_argmaxes(dev):
    """Every seed under the body the library chooses, and wherever the wave body applies under
    the one it did not choose."""
    from dora_amd import _lib
    from dora_amd._lib import ARROW_DEVICE_ROCM
    others = [0]

    def bodies(rec, bufs, mis):
        with am.plan_reduce(rec, bufs.ptr_of, ARROW_DEVICE_ROCM) as p:
            return [k["body"] for k in am.plan_reduces(p, len(rec), bufs.dst.ptr + GUARD + mis)]

    def other_bodies(rec, mis, bufs):
        chosen = bodies(rec, bufs, mis)
        for mode in (1, 2):
            _lib.call("dora_gpu_test_reduce_body", mode)
            if bodies(rec, bufs, mis) != chosen:
                others[0] += 1
                yield f"body {mode}"
        _lib.call("dora_gpu_test_reduce_body", 0)

    try:
        run_op(dev, OPS["argmax"], ARGMAX_SEEDS, [host.argmax_case(s) for s in ARGMAX_SEEDS],
               host.MISALIGNED_ARGMAX_SEEDS, other_bodies)
    finally:
        _lib.call("dora_gpu_test_reduce_body", 0)
    assert others[0] >= 20, others


def test_resizes(dev):
    run_op(dev, OPS["resize"], RESIZE_SEEDS, [host.resize_case(s) for s in RESIZE_SEEDS],
           host.MISALIGNED_RESIZE_SEEDS)


def test_crops(dev):
    """Garbage lives only in the words of the boxes, which the kernel clamps by contract."""
    cases = [host.crop_case(s) for s in CROP_SEEDS]
    assert any(not len(rec[0][3]["boxes"]) for rec, _ in cases if rec[0][3])  # K = 0 among them
    run_op(dev, OPS["crop"], CROP_SEEDS, cases, host.MISALIGNED_CROP_SEEDS)


def test_prep_resizes(dev):
    """gather_resize_prep_kernel: placement, fill, per-channel tables at 0, 4, 8 and 12 mod 16 and
    the affine step of every field that has one, at the seeds' shapes and residues."""
    run_op(dev, OPS["prep_resize"], PREP_RESIZE_SEEDS, [host.prep_resize_case(s) for s in PREP_RESIZE_SEEDS],
           host.MISALIGNED_PREP_RESIZE_SEEDS)


def test_prep_crops(dev):
    """gather_crop_prep_kernel: the channel coordinate behind K, empty boxes beside a bias."""
    cases = [host.prep_crop_case(s) for s in PREP_CROP_SEEDS]
    assert any(not len(rec[0][3]["boxes"]) for rec, _ in cases if rec[0][3])  # K = 0 among them
    run_op(dev, OPS["prep_crop"], PREP_CROP_SEEDS, cases, host.MISALIGNED_PREP_CROP_SEEDS)


def test_masks(dev):
    """Every seed's mask (a checked host partition for half), and once more behind a garbage
    partition in HBM, whose clamped offsets the launch looks up in the counts."""
    from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, PARTITION_LENGTHS, PARTITION_OFFSETS
    cases = [host.mask_case(seed) for seed in MASK_SEEDS]
    recs = [c[0] for c in cases]
    rows = max(len(c[2]) for c in cases)
    bufs = Buffers(dev, source_room(recs), sample_room(recs), rows + 16 + 8 * 8 + 64)
    garbage = 0
    try:
        for seed, (rec, label, mask, shift, mis, part, (words, form, offs)) in zip(MASK_SEEDS, cases):
            assert all(rv.inside(b, v) for _, b, v in rec), seed
            what = f"seed={seed} {label} mask%16={shift} dst%16={mis}"
            counts = mr.counts(mask)
            garbage += bool(((words < 0) | (words > len(mask))).any())
            bufs.place(sr.bases_of(rec))
            if part is None:
                run_mask(bufs, bufs, rec, what, mask, shift, mis)
            else:
                run_mask(bufs, bufs, rec, what, mask, shift, mis, part=part[0],
                         form=PARTITION_OFFSETS if part[1] else PARTITION_LENGTHS,
                         part_dev=ARROW_DEVICE_CPU, offsets_want=counts[part[2]].tolist())
            # (the mask's bytes first, the partition's words behind them on a multiple of 16)
            part_ptr = bufs.upload(words, (shift + mask.nbytes + 15) // 16 * 16)
            run_mask(bufs, bufs, rec, what + ", garbage partition in HBM", mask, shift, mis,
                     part=words, form=PARTITION_OFFSETS if form else PARTITION_LENGTHS,
                     part_dev=ARROW_DEVICE_ROCM, part_ptr=part_ptr, offsets_want=counts[offs].tolist())
        assert garbage >= 20, garbage
    finally:
        bufs.free()
