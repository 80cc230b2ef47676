"""Seeded random views through every gather body on the CPU (no GPU): the cases of
tests/random_views.py, one integer seed each, through the stand-alone emulations of
csrc/testing/*_emulate.cpp, each built here with the host compiler under AddressSanitizer and
UBSan exactly as the hand-picked host tests build them (test_gather_index_host.py,
test_gather_struct_index_host.py, test_take_index_host.py, test_cast_index_host.py,
test_mask_index_host.py, test_scan_index_host.py, whose helpers run here).  Every emulation fails
on a source offset outside the plan's [lo, hi], an output byte written twice, not at all or outside
the sample; the bytes are compared here with numpy.

To reproduce a failure take the `seed=` of its message: `r = random_views.rng(seed)` and the calls
of the failing test's loop body in their order give the same case.

The sweeps assert that they test something: at most a tenth of the bare seeds plan dense (skipped,
counted), the tile body runs for at least a tenth of the others, every body (rows, tile, taken,
cast, scan share, mask) and every element size runs at least 20 times, every destination residue a
body allows is hit, at least 5 records hold 8 fields.

The five op bodies (quantise, affine, argmax, resize, crops: gather_quant_kernel,
gather_affine_kernel, gather_reduce_kernel, gather_resize_kernel, gather_crop_kernel) run the same
way through cast_emulate, argmax_emulate, resize_emulate and crop_emulate and the `Batch` of their
test_*_index_host.py, bit for bit against each op's `want`, padding bytes included; argmax under
the body the library chooses and, wherever the wave body applies, under the other one.
`quant_case(seed)` .. `crop_case(seed)` reproduce a case.  Their conditions, each computed from
the reference and the plan alone: every source, destination or index dtype, mode and destination
residue at least 10 times; a tile-share and a rows-share plain field beside the op at least 10
times each; argmax: vector units, element units and the wave body in at least 20 seeds each, in at
least 30 a tie, a NaN behind a finite first value or -0.0 against +0.0 decides an output, at most
half of all indices are 0; quantise and affine: at least 20 seeds saturate, at most half of all
outputs sit on a bound, every combination of scale and bias terms 10 times, the channel axis is
dimension 0, the innermost, a broadcast and a reversed one 5 times each; resize: head, units and
tail occur, at most a tenth of the seeds is the identity, a resized coordinate changes inside a
unit in at least 20 seeds and stays in at least 20; crops: a unit straddles two crops and a box
lies outside int16 in at least 20 seeds each, at most a third of all crops is all zeros, every K
occurs, 0 among them.  One test per op alters a word of what the emulator is given and asserts
that the comparison fails; one per op asserts that a source off its element size is refused by
name.

The two model-input bodies (gather_resize_prep_kernel, gather_crop_prep_kernel: resize_device.h and
crop_device.h under their step) run `prep_resize_case(seed)` and `prep_crop_case(seed)` through
prep_emulate and the `Batch` of test_prep_index_host.py, bit for bit against `pr.want`, and once
more as host plans, whose staged segments are tensor_plan.cpp's own statement of the same values.
`PrepStats` counts what the seeds hold and `check` asserts it: every source, destination, mode and
residue and both plain shares 10 times; each of the eight combinations of an absent, a scalar and
a table scale and bias 10 times; no placement, a letterbox, a free one and a placement without
any term 10 times each; 20 records with two steps, 10 with a resized field without one beside a
step, 10 whose first step is not in field 0; the tables' axis first, in the middle, innermost,
broadcast, reversed and given negative 10 times each, of extent 1 once, under five dimensions or
more 20 times; tables at 0, 4, 8 and 12 mod 16; units in which the channel coordinate changes and
units in which it stays in 20 seeds each; a unit with elements inside and outside the image in 20
seeds, `lead == 0` and `lead + inner == size` on each axis, a fill of -0.0 to a float and a
saturating one to an integer destination; for crops a unit across two crops, a box outside int16
and an empty box beside a full one under a bias in 20 seeds each, and every K.  Four shares of the
reference cap what a pass may mean: at most half of the integer outputs on a bound, at most half
of the placed elements outside the image, at most a tenth of the steps without effect on the
statement, at most a twentieth of the float outputs not finite.  Tests alter `lead` and `inner`,
a table's word and a box's word and assert that the comparison fails.

tests/test_gpu_random_views.py runs the same seeds on the kernels."""
import collections
import subprocess

import numpy as np
import pytest

from dora_amd import _lib
from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, PARTITION_LENGTHS, PARTITION_OFFSETS
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
from tests.gather_views import describe_view, misalignment
from tests.test_affine_index_host import Batch as AffineBatch
from tests.test_argmax_index_host import Batch as ArgmaxBatch
from tests.test_cast_index_host import Batch as CastBatch
from tests.test_crop_index_host import Batch as CropBatch
from tests.test_quant_index_host import Batch as QuantBatch
from tests.test_resize_index_host import Batch as ResizeBatch
from tests.test_prep_index_host import Batch as PrepBatch
from tests.test_gather_index_host import gather_desc
from tests.test_gather_index_host import run as run_gather
from tests.test_gather_struct_index_host import run as run_struct
from tests.test_gather_struct_index_host import write_spec
from tests.test_mask_index_host import emulate as emulate_masks
from tests.test_scan_index_host import build
from tests.test_take_index_host import Batch as TakeBatch

FAKE = 0x7F12_3456_0000  # made-up device addresses, 16-byte aligned: planning never reads them
MASK = 0x7F30_0000_0000
DST = 0x7F50_0000_1000
POISON = 0xA5

# The seeds of each sweep.  A seed that ever failed stays: pin it here if a range changes.
BARE_SEEDS = range(0, 300)
RECORD_SEEDS = range(1000, 1150)
TAKE_SEEDS = range(2000, 2300)
CAST_SEEDS = range(3000, 3300)
MASK_SEEDS = range(4000, 4200)
MISALIGNED_CAST_SEEDS = range(5000, 5020)
QUANT_SEEDS = range(6000, 6300)
AFFINE_SEEDS = range(7000, 7300)
ARGMAX_SEEDS = range(8000, 8300)
RESIZE_SEEDS = range(9000, 9300)
CROP_SEEDS = range(10000, 10300)
MISALIGNED_QUANT_SEEDS = range(5100, 5120)
MISALIGNED_AFFINE_SEEDS = range(5200, 5220)
MISALIGNED_ARGMAX_SEEDS = range(5300, 5320)
MISALIGNED_RESIZE_SEEDS = range(5400, 5420)
MISALIGNED_CROP_SEEDS = range(5500, 5520)
PREP_RESIZE_SEEDS = range(11000, 11300)
PREP_CROP_SEEDS = range(12000, 12300)
MISALIGNED_PREP_RESIZE_SEEDS = range(5600, 5620)
MISALIGNED_PREP_CROP_SEEDS = range(5700, 5720)
MASK_ROWS = rv.EXTENTS + (255, 257, mr.TILE - 1, mr.TILE + 1)


@pytest.fixture(scope="module")
def gather_emulator(tmp_path_factory):
    return build(tmp_path_factory, "gather_emulate")


@pytest.fixture(scope="module")
def struct_emulator(tmp_path_factory):
    return build(tmp_path_factory, "gather_struct_emulate")


@pytest.fixture(scope="module")
def take_emulator(tmp_path_factory):
    return build(tmp_path_factory, "gather_take_emulate")


@pytest.fixture(scope="module")
def cast_emulator(tmp_path_factory):
    return build(tmp_path_factory, "cast_emulate")


@pytest.fixture(scope="module")
def mask_emulator(tmp_path_factory):
    return build(tmp_path_factory, "mask_emulate")


@pytest.fixture(scope="module")
def scan_emulator(tmp_path_factory):
    return build(tmp_path_factory, "scan_emulate")


# ---------------------------------------------------------------------------------------------
# The cases of each sweep, shared with the GPU test: functions of the seed alone.
# ---------------------------------------------------------------------------------------------
def bare_case(seed):
    """(base, view, destination mod 16 for the rows body, element-aligned one for the tile body)."""
    r = rv.rng(seed)
    b, v = rv.bare(r)
    return b, v, int(r.integers(0, 16)), int(r.integers(0, 16 // v.itemsize)) * v.itemsize


def record_case(seed):
    """(record, destination mod 16)."""
    r = rv.rng(seed)
    return rv.record(r), int(r.integers(0, 16))


def values_case(r):
    """A bare tensor or a record of named fields, half and half."""
    if r.random() < 0.5:
        b, v = rv.bare(r)
        return [(None, b, v)]
    return rv.record(r)


def take_case(seed):
    """(record, index label, index, destination mod 16, host partition's lengths or None,
    garbage partition for the scan share: (words, offsets form?, offsets))."""
    r = rv.rng(seed)
    rec = values_case(r)
    n = rec[0][2].shape[0]
    k = int(r.choice([1, 2, 3, 15, 16, 17, 63, 64, 65, 257]))
    label, index = rv.index(r, k, n, bool(r.integers(0, 2)))
    lengths = None
    if r.random() < 0.5:
        words, form, offs = rv.partition(r, k)
        lengths = np.diff(offs.astype(np.int64)).astype(words.dtype)
    # (behind a partition's offsets the sample starts on a multiple of their 4 bytes)
    mis = int(r.integers(0, 4)) * 4 if lengths is not None else int(r.integers(0, 16))
    return rec, label, index, mis, lengths, rv.partition(r, k, garbage=True)


def cast_case(seed):
    """(cast record, destination mod 16: a multiple of the largest converted element)."""
    r = rv.rng(seed)
    rec = rv.cast_record(r)
    d0 = rec[0][2].shape[0]
    if len(rec) > 1 and d0 <= 7 and r.random() < 0.5:
        # a permuted float32 field that the library's own selection tiles (output rows of 280
        # bytes along the source-contiguous dimension), at whatever offset the record gives it
        from tests.gather_views import base
        b = base(np.float32, (65, d0, 70))
        rec.insert(int(r.integers(0, len(rec) + 1)), ("planes", b, b.transpose(1, 2, 0), None))
    step = max(np.dtype(c["dst"]).itemsize for _, _, _, c in rec if c is not None)
    return rec, int(r.integers(0, 16 // step)) * step


def mask_case(seed):
    """(record, mask label, mask, mask address mod 16, destination mod 16, host partition:
    (words, offsets form?, offsets) or None, a garbage partition for the scan share)."""
    r = rv.rng(seed)
    n = int(r.choice(MASK_ROWS))
    if r.random() < 0.5:
        dtype = rv.DTYPES[int(r.integers(0, len(rv.DTYPES)))]
        rec = [(None, *rv.view(r, dtype, d0=n, max_elems=max(rv.MAX_ELEMS, 4 * n)))]
    else:
        rec = rv.record(r, d0=n, max_elems=max(rv.MAX_ELEMS, 16 * n))
    label, mask = rv.mask(r, n)
    part = rv.partition(r, n) if r.random() < 0.5 else None
    return rec, label, mask, int(r.integers(0, 16)), int(r.integers(0, 4)) * 4, part, \
        rv.partition(r, n, garbage=True)


def addresses(bases, spacing=1 << 26):
    """A made-up device address for every base, its misalignment kept."""
    return {id(b): FAKE + spacing * i + misalignment(b) for i, b in enumerate(bases)}


def reached(b, d, addr):
    """The bytes [lo, hi] of descriptor `d` over base `b`, after checking they are inside it."""
    off = d["src"] - addr
    assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes, d
    return b.tobytes()[off + d["lo"]: off + d["hi"] + 1]


# ---------------------------------------------------------------------------------------------
# Bare views: the rows body and the tile body
# ---------------------------------------------------------------------------------------------
def run_bare(exe, tmp_path, b, v, dst, tile):
    """The emulated bytes of view `v` packed at `dst` (None: dense plan, or the tile body does
    not apply)."""
    assert rv.inside(b, v)
    shape, strides, dtype, off = describe_view(b, v, None)
    ptr = FAKE + misalignment(b)
    d = gather_desc(ptr, shape, strides, dtype, off)
    if d is None:
        return None
    assert d["total"] == v.size * v.itemsize
    src_file, out_file = str(tmp_path / "src.bin"), str(tmp_path / "out.bin")
    with open(src_file, "wb") as f:
        f.write(reached(b, d, ptr))
    if not run_gather(exe, d, dst, (src_file, out_file), tile=tile).startswith("ok"):
        return None
    with open(out_file, "rb") as f:
        return f.read()


def test_bare_views(lib, gather_emulator, tmp_path):
    dense, rows, tiled, sizes, residues = 0, 0, 0, collections.Counter(), set()
    for seed in BARE_SEEDS:
        b, v, mis, tile_mis = bare_case(seed)
        want = np.ascontiguousarray(v).tobytes()
        got = run_bare(gather_emulator, tmp_path, b, v, DST + mis, False)
        if got is None:
            dense += 1
            continue
        assert got == want, f"rows body, seed={seed} dst%16={mis}"
        rows += 1
        sizes[v.itemsize] += 1
        residues.add(mis)
        got = run_bare(gather_emulator, tmp_path, b, v, DST + tile_mis, True)
        if got is not None:
            assert got == want, f"tile body, seed={seed} dst%16={tile_mis}"
            tiled += 1
    assert dense <= len(BARE_SEEDS) // 10, dense
    assert tiled >= max(20, rows // 10), (tiled, rows)
    assert rows >= 20 and all(sizes[s] >= 20 for s in (1, 2, 4, 8)), sizes
    assert residues == set(range(16)), residues


def test_the_sweep_notices_a_changed_stride(lib, gather_emulator, tmp_path):
    """The checks bite: the same comparison against the view with one stride's sign changed
    fails."""
    seed = 7
    b, v, mis, _ = bare_case(seed)
    got = run_bare(gather_emulator, tmp_path, b, v, DST + mis, False)
    assert got == np.ascontiguousarray(v).tobytes()
    k = next(k for k in range(v.ndim) if v.shape[k] > 1 and v.strides[k] != 0)
    other = np.flip(v, axis=k)
    assert other.shape == v.shape and other.strides[k] == -v.strides[k]
    with pytest.raises(AssertionError):
        assert got == np.ascontiguousarray(other).tobytes(), f"rows body, seed={seed}"


# ---------------------------------------------------------------------------------------------
# Records: gather_struct_kernel's mixed shares
# ---------------------------------------------------------------------------------------------
def test_records(lib, struct_emulator, tmp_path):
    dense, runs, tiles, eight, sizes, residues = 0, 0, 0, 0, collections.Counter(), set()
    for seed in RECORD_SEEDS:
        rec, mis = record_case(seed)
        assert all(rv.inside(b, v) for _, b, v in rec)
        sample, info, ranges = sr.oracle(rec)
        addr = addresses(sr.bases_of(rec), 1 << 24)
        with sr.plan_record(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
            assert p.size == len(sample), seed
            if p.segments():  # every field dense: no gather
                dense += 1
                continue
            eight += len(rec) == 8
            residues.add(mis)
            seen = []
            try:
                for mode in (1, 0, 2):  # rows forced, the selection, tile forced where it applies
                    _lib.call("dora_gpu_test_gather_kernel", mode)
                    fields = sr.plan_fields(p, DST + mis)
                    if fields in seen:  # (this mode chooses what an earlier one did)
                        continue
                    seen.append(fields)
                    what = f"seed={seed} mode={mode} dst%16={mis}"
                    assert all(d["gather"] for d in fields), what
                    assert [(d["off"], d["bytes"]) for d in fields] == ranges, what
                    files = []
                    for k, ((_, b, _), d) in enumerate(zip(rec, fields)):
                        files.append(str(tmp_path / f"src{k}.bin"))
                        with open(files[-1], "wb") as f:
                            f.write(reached(b, d, addr[id(b)]))
                    spec, out = str(tmp_path / "spec.txt"), str(tmp_path / "out.bin")
                    write_spec(spec, fields, DST + mis, p.size, files)
                    rc, text = run_struct(struct_emulator, spec, out)
                    assert rc == 0 and text.startswith("ok"), (what, text)
                    with open(out, "rb") as f:
                        got = f.read()
                    assert len(got) == len(sample), what
                    pad = bytearray(got)
                    for k, (off, ln) in enumerate(ranges):
                        assert got[off:off + ln] == sample[off:off + ln], f"field {k}, {what}"
                        pad[off:off + ln] = bytes([POISON]) * ln
                    assert bytes(pad) == bytes([POISON]) * len(got), "padding written, " + what
                    runs += 1
                    tiles += sum(d["kind"] >= 0 for d in fields)
                    if mode == 1:
                        for _, _, v in rec:
                            sizes[v.itemsize] += 1
            finally:
                _lib.call("dora_gpu_test_gather_kernel", 0)
    assert dense <= len(RECORD_SEEDS) // 10, dense
    assert eight >= 5 and tiles >= 20 and runs >= 20, (eight, tiles, runs)
    assert all(sizes[s] >= 20 for s in (1, 2, 4, 8)), sizes
    assert residues == set(range(16)), residues


# ---------------------------------------------------------------------------------------------
# Takes, and the scan share over garbage partitions
# ---------------------------------------------------------------------------------------------
def emulate_scan(exe, tmp_path, words, form, n, want, what):
    src, out = str(tmp_path / "scan_in.bin"), str(tmp_path / "scan_out.bin")
    words.tofile(src)
    r = subprocess.run([exe, str(len(words)), str(n), str(int(words.dtype.itemsize == 8)),
                        str(int(form)), src, out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok"), (what, r.stdout + r.stderr[-2000:])
    got = np.fromfile(out, dtype=np.int32)
    assert got.tobytes() == np.asarray(want, np.int32).tobytes(), (what, got, want)
    assert got[0] >= 0 and got[-1] <= n and (np.diff(got) >= 0).all(), what


def test_takes(lib, take_emulator, scan_emulator, tmp_path):
    batch = TakeBatch(tmp_path)
    parts, scans, eight, sizes, residues = 0, 0, 0, collections.Counter(), set()
    for seed in TAKE_SEEDS:
        rec, label, index, mis, lengths, (words, form, offs) = take_case(seed)
        assert all(rv.inside(b, v) for _, b, v in rec)
        batch.add(f"seed={seed} {label} dst%16={mis}", rec, index, DST + mis, part=lengths)
        parts += lengths is not None
        eight += len(rec) == 8
        residues.add(mis)
        for _, _, v in rec:
            sizes[v.itemsize] += 1
        if seed % 4 == 0:
            emulate_scan(scan_emulator, tmp_path, words, form, len(index), offs, f"seed={seed}")
            scans += 1
    assert "index_loads=" in batch.run(take_emulator)
    assert len(batch.want) == len(TAKE_SEEDS) and parts >= 20 and scans >= 20 and eight >= 5
    assert all(sizes[s] >= 20 for s in (1, 2, 4, 8)), sizes
    assert residues == set(range(16)), residues


# ---------------------------------------------------------------------------------------------
# Casts
# ---------------------------------------------------------------------------------------------
def test_casts(lib, cast_emulator, tmp_path):
    batch = CastBatch(tmp_path)
    pairs, scales, plain, tiled, residues = collections.Counter(), collections.Counter(), 0, 0, set()
    for seed in CAST_SEEDS:
        rec, mis = cast_case(seed)
        assert all(rv.inside(b, v) for _, b, v, _ in rec)
        batch.add(f"seed={seed} dst%16={mis}", rec, DST + mis)
        residues.add(mis)
        for _, _, _, c in rec:
            if c is None:
                plain += 1
            else:
                pairs[c["src"], c["dst"]] += 1
                scales[c["scale"]] += 1
        if any(name == "planes" for name, _, _, _ in rec):
            addr = addresses(cr.bases_of(rec))
            with cr.plan_cast(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
                kinds = [d["kind"] for d, r in zip(sr.plan_fields(p, DST + mis), rec) if r[0] == "planes"]
            tiled += kinds[0] >= 0
    assert " vector_loads=" in batch.run(cast_emulator)
    assert all(pairs[p] >= 5 for p in cr.PAIRS) and sum(pairs.values()) >= 20, pairs
    assert all(scales[s] >= 20 for s in (None, 1 / 255, 3.0)), scales
    assert plain >= 20 and tiled >= 5, (plain, tiled)
    assert residues == set(range(0, 16, 2)), residues


def test_a_cast_of_an_element_misaligned_source_is_refused(lib):
    """The plain bodies take a source at any byte (the sweeps above hold such bases); a cast reads
    whole elements, and a source off its element size is refused by name before any launch."""
    from dora_amd._lib import DoraGpuError
    for seed in MISALIGNED_CAST_SEEDS:
        rec = rv.misaligned_cast(rv.rng(seed))
        assert misalignment(rec[1][1]) in (1, 3)
        addr = addresses(cr.bases_of(rec))
        with pytest.raises(DoraGpuError) as e:
            cr.plan_cast(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM).close()
        assert e.value.code == -1 and "field 1 `f1`" in str(e.value), (seed, str(e.value))


# ---------------------------------------------------------------------------------------------
# Masks: the compaction, then the fields by the index it wrote
# ---------------------------------------------------------------------------------------------
def test_masks(lib, mask_emulator, take_emulator, scan_emulator, tmp_path):
    cases = [mask_case(seed) for seed in MASK_SEEDS]
    # (one list without a partition; with one the compaction leaves the offsets to the lookup)
    _, found = emulate_masks(mask_emulator, tmp_path,
                             [(f"seed={seed} {label}", mask, shift, part is None, 0)
                              for seed, (_, label, mask, shift, _, part, _) in zip(MASK_SEEDS, cases)])
    lines, wants, files = [], [], 0
    parts, scans, eight, sizes, shifts, residues = 0, 0, 0, collections.Counter(), set(), set()
    for seed, (rec, label, mask, shift, mis, part, garbage), index in zip(MASK_SEEDS, cases, found):
        what = f"seed={seed} {label} mask%16={shift} dst%16={mis}"
        assert all(rv.inside(b, v) for _, b, v in rec)
        n = len(mask)
        kw, offsets = {}, None
        if part is not None:
            words, form, offsets = part
            kw = dict(part=words, form=PARTITION_OFFSETS if form else PARTITION_LENGTHS,
                      part_dev=ARROW_DEVICE_CPU)
        sample, info, ranges = mr.oracle(rec, mask, offsets)
        addr = addresses(sr.bases_of(rec))
        with mr.plan_mask(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM, np.zeros_like(mask),
                          ARROW_DEVICE_ROCM, mask_ptr=MASK + shift, **kw) as p:
            assert p.size == len(sample) and p.segments() == [], what
            got = mr.plan_info(p)
            fields = sr.plan_fields(p, DST + mis)
            ifile = str(tmp_path / f"index{seed}.bin")
            index.tofile(ifile)
            lines.append(f"{len(rec)} {DST + mis} {p.size} {n} {n} 0 {ifile}")
            for k, ((_, b, v), d) in enumerate(zip(rec, fields)):
                assert d["gather"] and d["kind"] == -1 and (d["off"], d["bytes"]) == ranges[k], what
                src = str(tmp_path / f"m{files}.bin")
                files += 1
                with open(src, "wb") as f:
                    f.write(reached(b, d, addr[id(b)]))
                lines.append(" ".join(map(str, [d["elem"], d["row"], d["bytes"], d["lo"], d["hi"],
                                                d["src"], d["off"], got["stride0"][k], d["nd"],
                                                *d["shape"], *d["stride"], src])))
                sizes[v.itemsize] += 1
            wants.append((what, sample, ranges))
        parts += part is not None
        eight += len(rec) == 8
        shifts.add(shift)
        residues.add(mis)
        if seed % 4 == 0:
            words, form, offs = garbage
            emulate_scan(scan_emulator, tmp_path, words, form, n, offs, what)
            scans += 1
    spec, out = str(tmp_path / "take.txt"), str(tmp_path / "take.bin")
    with open(spec, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([take_emulator, spec, out], capture_output=True, text=True)
    text = r.stdout + r.stderr[-3000:]
    assert r.returncode == 0 and text.startswith(f"ok cases={len(wants)} "), text
    with open(out, "rb") as f:
        have = f.read()
    at = 0
    for what, sample, ranges in wants:
        got = bytearray(have[at:at + len(sample)])
        at += len(sample)
        for k, (off, ln) in enumerate(ranges):
            assert got[off:off + ln] == sample[off:off + ln], f"field {k}, {what}"
            got[off:off + ln] = bytes([POISON]) * ln
        assert bytes(got) == bytes([POISON]) * len(got), "a byte outside the fields written, " + what
    assert at == len(have)
    assert len(wants) >= 20 and parts >= 20 and scans >= 20 and eight >= 5, (parts, scans, eight)
    assert all(sizes[s] >= 20 for s in (1, 2, 4, 8)), sizes
    assert shifts == set(range(16)) and residues == {0, 4, 8, 12}, (shifts, residues)


# ---------------------------------------------------------------------------------------------
# The op bodies: quantise, affine, argmax, resize, crops.  A case is (record, destination mod 16: a
# multiple of the widest op destination element); the affine case adds its scale and bias terms.
# ---------------------------------------------------------------------------------------------
def narrow(seed):
    """Seven seeds of every ten take 8-bit destinations only, so that their records go to odd
    addresses: dealt along the seeds, not drawn, so that every residue gets a known share."""
    return seed % 10 < 7


def residue(seed, sizes):
    """A multiple of the widest op destination element, dealt in turn along the narrow and along
    the other seeds; the residues that wider elements rule out get two turns."""
    step = max(sizes)
    turns = [m for m in range(0, 16, step) for _ in range(2 if m % max(4, 2 * step) else 1)]
    tens, ones = divmod(seed % 1000, 10)
    return turns[(7 * tens + ones if narrow(seed) else 3 * tens + ones - 7) % len(turns)]


def quant_case(seed):
    r = rv.rng(seed)
    rec = rv.quant_record(r, narrow=narrow(seed))
    return rec, residue(seed, [np.dtype(x[3]["dst"]).itemsize for x in rec if x[3]])


def affine_case(seed):
    """(record, destination mod 16, [(scale term, bias term) of every converted field])."""
    r = rv.rng(seed)
    rec, terms = rv.affine_record(r, narrow=narrow(seed))
    return rec, residue(seed, [np.dtype(x[3]["dst"]).itemsize for x in rec if x[3]]), terms


def argmax_case(seed):
    """Of every ten seeds seven reduce a random view to the narrowest index, two a dense base
    along its first dimension and one along its last."""
    r = rv.rng(seed)
    dense = rv.DENSE[0 if narrow(seed) else 2 if seed % 10 == 9 else 1]
    rec = rv.argmax_record(r, narrow=narrow(seed), dense=dense)
    return rec, residue(seed, [am.INDEX[x[3]["dtype"]][1] // 8 for x in rec if x[3]])


def resize_case(seed):
    r = rv.rng(seed)
    rec = rv.resize_record(r, narrow=narrow(seed))
    return rec, residue(seed, [rr.DESTS[rr.dst_name(x[3])][1] // 8 for x in rec if x[3]])


def crop_case(seed):
    r = rv.rng(seed)
    rec = rv.crop_record(r, narrow=narrow(seed))
    return rec, residue(seed, [kr.DESTS[kr.dst_name(x[3])][1] // 8 for x in rec if x[3]])


@pytest.fixture(scope="module")
def argmax_emulator(tmp_path_factory):
    return build(tmp_path_factory, "argmax_emulate")


@pytest.fixture(scope="module")
def resize_emulator(tmp_path_factory):
    return build(tmp_path_factory, "resize_emulate")


@pytest.fixture(scope="module")
def crop_emulator(tmp_path_factory):
    return build(tmp_path_factory, "crop_emulate")


def plain_shares(plan, rec, mis, shares):
    """Count the plain fields of `rec` that the op kernel's own tile share and rows share take."""
    for d, x in zip(sr.plan_fields(plan, DST + mis), rec):
        if x[3] is None:
            shares["tile" if d["kind"] >= 0 else "rows"] += 1


def at_least(counter, keys, n, what):
    """Every key of `keys` was counted at least `n` times (the counts are printed: pytest -s)."""
    print(f"{what}: " + ", ".join(f"{k}: {counter[k]}" for k in keys))
    assert all(counter[k] >= n for k in keys), (what, {k: counter[k] for k in keys if counter[k] < n})


def on_a_bound(out):
    info = np.iinfo(out.dtype)
    return int(((out == info.min) | (out == info.max)).sum())


def refused_by_name(plan, rec, bases):
    from dora_amd._lib import DoraGpuError
    assert misalignment(rec[1][1]) in (1, 3)
    addr = addresses(bases)
    with pytest.raises(DoraGpuError) as e:
        plan(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM).close()
    return e.value.code == -1 and "field 1 `f1`" in str(e.value), str(e.value)


def altered(batch, emulator, field, token, change):
    """Run `batch` with one word of the last case's field line changed: the comparison fails."""
    lines = batch.spec[-1].split("\n")
    words = lines[1 + field].split(" ")
    words[token] = str(change(int(words[token])))
    lines[1 + field] = " ".join(words)
    batch.spec[-1] = "\n".join(lines)
    with pytest.raises(AssertionError):
        batch.run(emulator)


# ---------------------------------------------------------------------------------------------
# Quantise: gather_quant_kernel
# ---------------------------------------------------------------------------------------------
def test_quants(lib, cast_emulator, tmp_path):
    batch = QuantBatch(tmp_path)
    srcs, dsts, residues, shares = (collections.Counter() for _ in range(4))
    saturated, bound, outputs = 0, 0, 0
    for seed in QUANT_SEEDS:
        rec, mis = quant_case(seed)
        assert all(rv.inside(b, v) for _, b, v, _ in rec), seed
        batch.add(f"seed={seed} dst%16={mis}", rec, DST + mis)
        residues[mis] += 1
        some = 0
        for _, _, v, c in rec:
            if qr.is_quant(c):
                srcs[c["src"]] += 1
                dsts[c["dst"]] += 1
                out = qr.want(v, c)
                some += on_a_bound(out)
                outputs += out.size
        saturated += some > 0
        bound += some
        addr = addresses(cr.bases_of(rec))
        with qr.plan_convert(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
            plain_shares(p, rec, mis, shares)
    assert " vector_loads=" in batch.run(cast_emulator)
    at_least(srcs, qr.SOURCES, 10, "sources")
    at_least(dsts, qr.DESTS, 10, "destinations")
    at_least(residues, range(16), 10, "residues")
    at_least(shares, ("tile", "rows"), 10, "plain fields")
    print(f"{saturated} seeds saturate; {bound} of {outputs} quantised outputs sit on a bound")
    assert saturated >= 20 and 2 * bound <= outputs, (saturated, bound, outputs)


def first_strided(seeds, case, field_ok):
    """The first seed whose first field has a dimension of more than one step and a stride."""
    for seed in seeds:
        rec = case(seed)[0]
        v = rec[0][2]
        if field_ok(rec) and any(n > 1 and s for n, s in zip(v.shape, v.strides)):
            return seed
    raise AssertionError("no such seed")


def stride_token(batch, field=0):
    """Index of the first stride of a dimension of more than one step, in the field's line."""
    words = batch.spec[-1].split("\n")[1 + field].split(" ")
    nd = next(n for n in range(8, 0, -1) if len(words) > 2 * n + 1 and words[-2 * n - 2] == str(n))
    shape = [int(w) for w in words[-2 * nd - 1:-nd - 1]]
    k = next(k for k in range(nd) if shape[k] > 1 and int(words[-nd - 1 + k]))
    return len(words) - nd - 1 + k


def test_the_quant_sweep_notices_a_changed_stride(lib, cast_emulator, tmp_path):
    seed = first_strided(QUANT_SEEDS, quant_case, lambda rec: True)
    rec, mis = quant_case(seed)
    batch = QuantBatch(tmp_path)
    batch.add(f"seed={seed}", rec, DST + mis)
    batch.run(cast_emulator)
    altered(batch, cast_emulator, 0, stride_token(batch), lambda s: -s)


def test_a_quantise_of_an_element_misaligned_source_is_refused(lib):
    for seed in MISALIGNED_QUANT_SEEDS:
        rec = rv.misaligned_op(rv.rng(seed), "quant")
        ok, text = refused_by_name(qr.plan_convert, rec, cr.bases_of(rec))
        assert ok, (seed, text)


# ---------------------------------------------------------------------------------------------
# Affine: gather_affine_kernel
# ---------------------------------------------------------------------------------------------
def channel_axis_kinds(v, a):
    """Which of the sweep's kinds the channel axis of affine `a` over view `v` is."""
    if a is None or a["axis"] is None:
        return []
    ax = a["axis"] % v.ndim
    return [name for name, yes in (("dimension 0", ax == 0), ("innermost", ax == v.ndim - 1),
                                   ("broadcast", v.strides[ax] == 0 and v.shape[ax] > 1),
                                   ("reversed", v.strides[ax] < 0)) if yes]


def test_affines(lib, cast_emulator, tmp_path):
    batch = AffineBatch(tmp_path)
    srcs, dsts, residues, shares, combos, axes = (collections.Counter() for _ in range(6))
    saturated, bound, outputs = 0, 0, 0
    for seed in AFFINE_SEEDS:
        rec, mis, terms = affine_case(seed)
        assert all(rv.inside(x[1], x[2]) for x in rec), seed
        batch.add(f"seed={seed} dst%16={mis}", rec, DST + mis)
        residues[mis] += 1
        combos.update(terms)
        some = 0
        for _, _, v, c, a in rec:
            if c is None:
                continue
            srcs[c["src"]] += 1
            dsts[c["dst"]] += 1
            axes.update(channel_axis_kinds(v, a))
            if qr.is_quant(c):
                out = ar.want(v, c, a)
                some += on_a_bound(out)
                outputs += out.size
        saturated += some > 0
        bound += some
        addr = addresses(sr.bases_of([x[:3] for x in rec]))
        with ar.plan_affine(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM, lambda t: FAKE) as p:
            plain_shares(p, rec, mis, shares)
    batch.run(cast_emulator)
    at_least(srcs, qr.SOURCES, 10, "sources")
    at_least(dsts, list(qr.DESTS) + ["float16", "float32"], 10, "destinations")
    at_least(residues, range(16), 10, "residues")
    at_least(shares, ("tile", "rows"), 10, "plain fields")
    at_least(combos, [(s, b) for s in rv.AFFINE_TERMS for b in rv.AFFINE_TERMS], 10, "terms")
    at_least(axes, ("dimension 0", "innermost", "broadcast", "reversed"), 5, "channel axes")
    print(f"{saturated} seeds saturate; {bound} of {outputs} quantised outputs sit on a bound")
    assert saturated >= 20 and 2 * bound <= outputs, (saturated, bound, outputs)


def test_the_affine_sweep_notices_a_changed_stride(lib, cast_emulator, tmp_path):
    seed = first_strided(AFFINE_SEEDS, affine_case, lambda rec: True)
    rec, mis, _ = affine_case(seed)
    batch = AffineBatch(tmp_path)
    batch.add(f"seed={seed}", rec, DST + mis)
    batch.run(cast_emulator)
    altered(batch, cast_emulator, 0, stride_token(batch), lambda s: -s)


def test_the_affine_sweep_notices_a_changed_table_entry(lib, cast_emulator, tmp_path):
    """Every word of the first field's table replaced by its negative less one: the bytes differ."""
    seed = next(s for s in AFFINE_SEEDS if affine_case(s)[2][0][0] == "table")
    rec, mis, _ = affine_case(seed)
    batch = AffineBatch(tmp_path)
    batch.add(f"seed={seed}", rec, DST + mis)
    batch.run(cast_emulator)
    words = batch.spec[-1].split("\n")[1].split(" ")
    assert words[0] == "3" and words[8] != "-"
    table = np.fromfile(words[8], np.float32)
    assert table.tobytes() == rec[0][4]["scale"].tobytes()
    (-table - 1).astype(np.float32).tofile(words[8])
    with pytest.raises(AssertionError):
        batch.run(cast_emulator)


def test_an_affine_of_an_element_misaligned_source_is_refused(lib):
    for seed in MISALIGNED_AFFINE_SEEDS:
        rec = rv.misaligned_op(rv.rng(seed), "affine")
        plan = lambda rec, ptr_of, dev: ar.plan_affine(rec, ptr_of, dev, lambda t: FAKE)  # noqa: E731
        ok, text = refused_by_name(plan, rec, sr.bases_of([x[:3] for x in rec]))
        assert ok, (seed, text)


# ---------------------------------------------------------------------------------------------
# Argmax: gather_reduce_kernel, the lane body and the wave body
# ---------------------------------------------------------------------------------------------
def rule_decides(v, red):
    """Some output of the reduction is decided by the rule and not by one largest value: equal
    maxima tie, a NaN stands behind a finite first value, or -0.0 meets +0.0 at the maximum."""
    x = np.moveaxis(cr.to_f32(v, red["src"]), red["axis"], -1).reshape(-1, v.shape[red["axis"]])
    nan = np.isnan(x)
    behind = nan.any(1) & (nan.argmax(1) > 0) & np.isfinite(x[:, 0])
    y = np.where(nan, -np.inf, x)
    top = y == y.max(1, keepdims=True)
    tie = ~nan.any(1) & (top.sum(1) > 1)
    zeros = ~nan.any(1) & (top & (x == 0) & np.signbit(x)).any(1) & (top & (x == 0) & ~np.signbit(x)).any(1)
    return bool((behind | tie | zeros).any())


def reduce_bodies(rec, mis):
    """plan_reduces of `rec` under the current body selection."""
    addr = addresses(am.bases_of(rec))
    with am.plan_reduce(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
        shares = collections.Counter()
        plain_shares(p, rec, mis, shares)
        return am.plan_reduces(p, len(rec), DST + mis), shares


def test_argmaxes(lib, argmax_emulator, tmp_path):
    (tmp_path / "other").mkdir()
    batch, other = ArgmaxBatch(tmp_path), ArgmaxBatch(tmp_path / "other")
    srcs, dsts, residues, shares, paths = (collections.Counter() for _ in range(5))
    decided, zeros, indices = 0, 0, 0
    try:
        for seed in ARGMAX_SEEDS:
            rec, mis = argmax_case(seed)
            what = f"seed={seed} dst%16={mis}"
            assert all(rv.inside(b, v) for _, b, v, _ in rec), seed
            _lib.call("dora_gpu_test_reduce_body", 0)
            batch.add(what, rec, DST + mis)
            chosen, plain = reduce_bodies(rec, mis)
            shares.update(plain)
            residues[mis] += 1
            paths["vector"] += any(k["vector_units"] for k in chosen)
            paths["element"] += any(k["element_units"] for k in chosen)
            paths["wave"] += any(k["op"] and k["body"] == 2 for k in chosen)
            rule = False
            for _, _, v, red in rec:
                if red:
                    srcs[red["src"]] += 1
                    dsts[red["dtype"]] += 1
                    out = am.want(v, red)
                    zeros += int((out == 0).sum())
                    indices += out.size
                    rule = rule or rule_decides(v, red)
            decided += rule
            # wherever the wave body applies: the body the library did not choose
            for mode in (1, 2):
                _lib.call("dora_gpu_test_reduce_body", mode)
                forced, _ = reduce_bodies(rec, mis)
                if [k["body"] for k in forced] != [k["body"] for k in chosen]:
                    other.add(f"{what} body {mode}", rec, DST + mis)
                    paths["other body"] += 1
    finally:
        _lib.call("dora_gpu_test_reduce_body", 0)
    counts = batch.run(argmax_emulator)
    assert counts["vector_units"] and counts["element_units"] and counts["wave_outputs"], counts
    assert other.run(argmax_emulator)["wave_outputs"]
    at_least(srcs, am.SOURCES, 10, "sources")
    at_least(dsts, am.INDEX, 10, "index dtypes")
    at_least(residues, range(16), 10, "residues")
    at_least(shares, ("tile", "rows"), 10, "plain fields")
    at_least(paths, ("vector", "element", "wave", "other body"), 20, "bodies")
    print(f"the rule decides in {decided} seeds; {zeros} of {indices} indices are 0")
    assert decided >= 30 and 2 * zeros <= indices, (decided, zeros, indices)


def test_the_argmax_sweep_notices_a_changed_axis_stride(lib, argmax_emulator, tmp_path):
    """The axis stride zero: every candidate is the first, every index 0."""
    for seed in ARGMAX_SEEDS:
        rec, mis = argmax_case(seed)
        if rec[0][3] and am.want(rec[0][2], rec[0][3]).any():
            break
    batch = ArgmaxBatch(tmp_path)
    batch.add(f"seed={seed}", rec, DST + mis)
    batch.run(argmax_emulator)
    altered(batch, argmax_emulator, 0, 6, lambda s: 0)


def test_an_argmax_of_an_element_misaligned_source_is_refused(lib):
    for seed in MISALIGNED_ARGMAX_SEEDS:
        rec = rv.misaligned_op(rv.rng(seed), "argmax")
        ok, text = refused_by_name(am.plan_reduce, rec, am.bases_of(rec))
        assert ok, (seed, text)


# ---------------------------------------------------------------------------------------------
# Resize: gather_resize_kernel
# ---------------------------------------------------------------------------------------------
def units_of(shape, axes, k, elem):
    """(a unit in which a coordinate of `axes` changes exists, one in which none does) for the
    whole 16-byte units of a field of output `shape` whose plan reports head and units `k`."""
    per = 16 // elem
    if not k["units"]:
        return False, False
    e = k["head"] + np.arange(k["units"] * per, dtype=np.int64).reshape(-1, per)
    changes = np.zeros(len(e), bool)
    for ax in axes:
        o = (e // int(np.prod(shape[ax + 1:], dtype=np.int64))) % shape[ax]
        changes |= (o != o[:, :1]).any(1)
    return bool(changes.any()), bool((~changes).any())


def test_resizes(lib, resize_emulator, tmp_path):
    batch = ResizeBatch(tmp_path)
    srcs, dsts, modes, residues, shares, units = (collections.Counter() for _ in range(6))
    identity = 0
    for seed in RESIZE_SEEDS:
        rec, mis = resize_case(seed)
        assert all(rv.inside(b, v) for _, b, v, _ in rec), seed
        batch.add(f"seed={seed} dst%16={mis}", rec, DST + mis)
        residues[mis] += 1
        addr = addresses(rr.bases_of(rec))
        with rr.plan_resize(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
            plain_shares(p, rec, mis, shares)
            ks = rr.plan_resizes(p, len(rec), DST + mis)
        same, inside, across = True, False, False
        for (_, _, v, op), k in zip(rec, ks):
            if not op:
                continue
            srcs[op["src"]] += 1
            dsts[op["dst"]] += 1
            modes[op["mode"]] += 1
            shape = rv.out_shape(v, op)
            same = same and shape == list(v.shape)
            a, b = units_of(shape, op["axes"], k, k["bits"] // 8)
            inside, across = inside or a, across or b
        identity += same
        units["changes"] += inside
        units["keeps"] += across
    counts = batch.run(resize_emulator)
    assert batch.paths == {"head", "units", "tail"}, batch.paths
    assert counts["head_elements"] and counts["units"] and counts["tail_elements"], counts
    at_least(srcs, rr.SOURCES, 10, "sources")
    at_least(dsts, [None] + list(rr.DESTS), 10, "destinations")
    at_least(modes, rr.MODES, 10, "modes")
    at_least(residues, range(16), 10, "residues")
    at_least(shares, ("tile", "rows"), 10, "plain fields")
    at_least(units, ("changes", "keeps"), 20, "units")
    print(f"identity: {identity} of {len(RESIZE_SEEDS)} seeds; emulator: {counts}")
    assert 10 * identity <= len(RESIZE_SEEDS), identity


def test_the_resize_sweep_notices_a_changed_input_extent(lib, resize_emulator, tmp_path):
    """A resized axis one source step shorter: other taps."""
    for seed in RESIZE_SEEDS:
        rec, mis = resize_case(seed)
        op, v = rec[0][3], rec[0][2]
        if not op or v.shape[op["axes"][0]] < 3:
            continue
        cut = tuple(slice(0, -1) if k == op["axes"][0] else slice(None) for k in range(v.ndim))
        if rr.want(v[cut], op).tobytes() != rr.want(v, op).tobytes():  # (the reference notices)
            break
    batch = ResizeBatch(tmp_path)
    batch.add(f"seed={seed}", rec, DST + mis)
    batch.run(resize_emulator)
    words = batch.spec[-1].split("\n")[1].split(" ")
    assert int(words[9]) == v.shape[op["axes"][0]]
    altered(batch, resize_emulator, 0, 9, lambda n: n - 1)


def test_a_resize_of_an_element_misaligned_source_is_refused(lib):
    for seed in MISALIGNED_RESIZE_SEEDS:
        rec = rv.misaligned_op(rv.rng(seed), "resize")
        ok, text = refused_by_name(rr.plan_resize, rec, rr.bases_of(rec))
        assert ok, (seed, text)


# ---------------------------------------------------------------------------------------------
# Crops: gather_crop_kernel
# ---------------------------------------------------------------------------------------------
def straddles(k, crop_elems, elem):
    """Some whole 16-byte unit holds elements of two crops (test_crop_index_host.py's
    test_units_straddle_crops has the arithmetic)."""
    per = 16 // elem
    firsts = k["head"] + per * np.arange(k["units"], dtype=np.int64)
    return bool((firsts // crop_elems != (firsts + per - 1) // crop_elems).any())


def test_crops(lib, crop_emulator, tmp_path):
    batch = CropBatch(tmp_path)
    srcs, dsts, modes, residues, shares, counts, at = (collections.Counter() for _ in range(7))
    crops, empty = 0, 0
    for seed in CROP_SEEDS:
        rec, mis = crop_case(seed)
        what = f"seed={seed} dst%16={mis}"
        assert all(rv.inside(b, v) for _, b, v in kr.triples(rec)), seed
        k0 = len(rec[0][3]["boxes"]) if rec[0][3] else len(rec[1][3]["boxes"])
        counts[k0] += 1
        addr = addresses(kr.bases_of(rec))
        with kr.plan_crop(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
            assert p.size == len(kr.oracle(rec)[0]) and p.segments() == [], what
            if not k0:
                continue  # K == 0: the empty message, nothing is launched
            plain_shares(p, rec, mis, shares)
            ks = kr.plan_crops(p, len(rec), DST + mis)
        batch.add(what, rec, DST + mis)
        residues[mis] += 1
        straddle, wide = False, False
        for (_, _, v, c), k in zip(rec, ks):
            if not c:
                continue
            srcs[c["src"]] += 1
            dsts[c["dst"]] += 1
            modes[c["mode"]] += 1
            at[misalignment(c["boxes_base"]) + (c["boxes"].__array_interface__["data"][0] -
                                                c["boxes_base"].__array_interface__["data"][0])] += 1
            out = kr.want(v, c)
            ia, ib = (v.shape[a] for a in c["axes"])
            clamped = np.clip(c["boxes"].astype(np.int64), 0, [ia, ib, ia, ib])
            assert ((clamped[:, 2] > clamped[:, 0]) & (clamped[:, 3] > clamped[:, 1])).any(), what
            crops += len(out)
            empty += sum(not out[j].any() for j in range(len(out)))
            straddle = straddle or straddles(k, out[0].size, out.itemsize)
            wide = wide or bool(((c["boxes"] > 32767) | (c["boxes"] < -32768)).any())
        counts["straddle"] += straddle
        counts["outside int16"] += wide
    text = batch.run(crop_emulator)
    assert batch.paths == {"head", "units", "tail"}, batch.paths
    assert text["head_elements"] and text["units"] and text["tail_elements"] and text["box_loads"]
    at_least(srcs, kr.SOURCES, 10, "sources")
    at_least(dsts, [None] + list(kr.DESTS), 10, "destinations")
    at_least(modes, kr.MODES, 10, "modes")
    at_least(residues, range(16), 10, "residues")
    at_least(at, (0, 4, 8, 12), 10, "boxes mod 16")
    at_least(shares, ("tile", "rows"), 10, "plain fields")
    at_least(counts, ("straddle", "outside int16"), 20, "crops")
    at_least(counts, rv.CROP_COUNTS, 1, "K")
    print(f"crops all zeros: {empty} of {crops}")
    assert 3 * empty <= crops, (empty, crops)


def test_the_crop_sweep_notices_a_changed_box_word(lib, crop_emulator, tmp_path):
    """The first box moved one step along its second axis."""
    for seed in CROP_SEEDS:
        rec, mis = crop_case(seed)
        c, v = rec[0][3], rec[0][2]
        if c and len(c["boxes"]) and v.shape[c["axes"][1]] > 3 and \
                tuple(c["boxes"][0]) == (0, 0, v.shape[c["axes"][0]], v.shape[c["axes"][1]]):
            break
    else:
        raise AssertionError("no seed whose first box is the whole frame")
    batch = CropBatch(tmp_path)
    batch.add(f"seed={seed}", rec, DST + mis)
    batch.run(crop_emulator)
    name = batch.spec[-1].split("\n")[1].split(" ")[-1]
    words = np.fromfile(name, np.int32)
    words[1] += 2
    words.tofile(name)
    with pytest.raises(AssertionError):
        batch.run(crop_emulator)


def test_crops_of_an_element_misaligned_source_are_refused(lib):
    for seed in MISALIGNED_CROP_SEEDS:
        rec = rv.misaligned_op(rv.rng(seed), "crop")
        ok, text = refused_by_name(kr.plan_crop, rec, kr.bases_of(rec))
        assert ok, (seed, text)


# ---------------------------------------------------------------------------------------------
# Model inputs: gather_resize_prep_kernel and gather_crop_prep_kernel.  A case is (record of
# tests/prep_records.py, destination mod 16); what the sweeps must see is counted by `PrepStats`
# from the record, the plan and `pr.want` alone.
# ---------------------------------------------------------------------------------------------
def prep_resize_case(seed):
    r = rv.rng(seed)
    rec = rv.prep_resize_record(r, narrow=narrow(seed))
    return rec, residue(seed, [pr.DESTS[pr.dst_name(x[3])][1] // 8 for x in rec if x[3]])


def prep_crop_case(seed):
    r = rv.rng(seed)
    rec = rv.prep_crop_record(r, narrow=narrow(seed))
    return rec, residue(seed, [pr.DESTS[pr.dst_name(x[3])][1] // 8 for x in rec if x[3]])


@pytest.fixture(scope="module")
def prep_emulator(tmp_path_factory):
    return build(tmp_path_factory, "prep_emulate")


def host_ptr(b):
    return b.__array_interface__["data"][0]


def form(term):
    return "none" if term is None else "table" if pr.is_table(term) else "scalar"


def inside_of(shape, op):
    """The elements of an output of `shape` that lie inside the image `op`'s step places."""
    q = op["prep"]
    inside = np.zeros(shape, bool)
    at = [slice(None)] * len(shape)
    for ax, n, l in zip(op["axes"], q["inner"], q["lead"]):
        at[ax % len(shape)] = slice(l, l + n)
    inside[tuple(at)] = True
    return inside


def mixed_units(inside, k, elem):
    """Some whole 16-byte unit of a field whose plan reports head and units `k` holds elements
    inside and outside the image."""
    per = 16 // elem
    flat = inside.reshape(-1)[k["head"]: k["head"] + k["units"] * per].reshape(-1, per)
    return bool((flat.any(1) & ~flat.all(1)).any())


def box_areas(v, c):
    """The clamped area of every box of crop `c` over frame `v`."""
    ia, ib = (v.shape[a] for a in c["axes"])
    w = np.clip(c["boxes"].astype(np.int64), 0, [ia, ib, ia, ib])
    return np.maximum(w[:, 2] - w[:, 0], 0) * np.maximum(w[:, 3] - w[:, 1], 0)


class PrepStats:
    """What a sweep of model-input records saw, counted per field with a step (`field`) and per
    seed (`seed`), and the four shares of the reference that cap what a pass may mean."""

    def __init__(self, crops):
        self.crops = crops
        names = ("srcs", "dsts", "modes", "residues", "shares", "combos", "places", "records",
                 "axes", "tables", "units", "placed", "fills", "counts")
        for name in names:
            setattr(self, name, collections.Counter())
        self.bound = self.ints = self.outside = self.placed_elems = 0
        self.nothing = self.steps = self.nonfinite = self.floats = 0

    def field(self, v, c, k, seen):
        """Field of view `v` under op `c` with a step, `k` its head and units in the plan; `seen`
        collects what is counted once per seed."""
        from dora_amd import tensor
        q, nd, up = c["prep"], v.ndim, int(self.crops)
        self.srcs[c["src"]] += 1
        self.dsts[c["dst"]] += 1
        self.modes[c["mode"]] += 1
        self.combos[form(q["scale"]), form(q["bias"])] += 1
        out = pr.want(v, c)
        elem = out.itemsize
        self.steps += 1
        self.nothing += out.tobytes() == pr.want(v, dict(c, prep=None)).tobytes()
        if out.dtype.kind == "f":
            self.floats += out.size
            self.nonfinite += int((~np.isfinite(out)).sum())
        else:
            self.ints += out.size
            self.bound += on_a_bound(out)
        # the tables and their axis
        if q["axis"] is not None:
            ax = q["axis"] % nd
            self.axes["first" if ax == 0 else "innermost" if ax == nd - 1 else "middle"] += 1
            self.axes["broadcast"] += v.strides[ax] == 0 and v.shape[ax] > 1
            self.axes["reversed"] += v.strides[ax] < 0
            self.axes["extent 1"] += v.shape[ax] == 1
            self.axes["negative"] += q["axis"] < 0
            self.axes["five dimensions or more"] += nd >= 5
            for w in ("scale", "bias"):
                if pr.is_table(q[w]):
                    tb, tv = q[w]
                    self.tables[(misalignment(tb) + host_ptr(tv) - host_ptr(tb)) % 16] += 1
                    self.tables["an exact 0.0, -0.0 or 1.0"] += bool(np.isin(tv, [0.0, 1.0]).any())
            changes, keeps = units_of(list(out.shape), (ax + up,), k, elem)
            seen.update(["changes"] * changes + ["keeps"] * keeps)
        # the placement
        if q["inner"] is None:
            self.places["none"] += 1
            return
        sizes = tuple(v.shape[a % nd] for a in c["axes"])
        boxed = (tuple(q["inner"]), tuple(q["lead"])) == tensor.letterbox(sizes, c["size"])
        self.places["letterbox" if boxed else "free"] += 1
        self.places["placement alone"] += q["scale"] is None and q["bias"] is None
        inside = inside_of(out.shape, c)
        self.placed_elems += out.size
        self.outside += int((~inside).sum())
        if mixed_units(inside, k, elem):
            seen.add("mixed")
        for j in (0, 1):
            self.placed[f"lead[{j}] == 0"] += q["lead"][j] == 0
            self.placed[f"lead[{j}] + inner[{j}] == size[{j}]"] += q["lead"][j] + q["inner"][j] == c["size"][j]
        pad = out[~inside]
        if pad.size and out.dtype.kind == "f":
            self.fills["-0.0 to a float"] += q["fill"] == 0 and bool(np.signbit(np.float32(q["fill"])))
        if pad.size and out.dtype.kind != "f":
            info = np.iinfo(out.dtype)
            self.fills["saturating to an integer"] += not info.min <= q["fill"] <= info.max and \
                on_a_bound(pad) == pad.size

    def record(self, rec, mis, plan):
        """One seed's record under its device plan."""
        dst = DST + mis
        ks = kr.plan_crops(plan, len(rec), dst) if self.crops else rr.plan_resizes(plan, len(rec), dst)
        self.residues[mis] += 1
        plain_shares(plan, rec, mis, self.shares)
        seen, stepped = set(), [i for i, x in enumerate(rec) if x[3] and x[3].get("prep")]
        assert stepped and stepped[0] == next(i for i, x in enumerate(rec) if x[3])
        for i in stepped:
            self.field(rec[i][2], rec[i][3], ks[i], seen)
        self.records["two fields with a step"] += len(stepped) >= 2
        self.records["a resized field without a step"] += any(x[3] and not x[3].get("prep") for x in rec)
        self.records["the first step not in field 0"] += stepped[0] > 0
        if self.crops:
            straddle = wide = False
            for (_, _, v, c), k in zip(rec, ks):
                if not c:
                    continue
                n = pr.want(v, c)
                straddle = straddle or straddles(k, n[0].size, n.itemsize)
                wide = wide or bool(((c["boxes"] > 32767) | (c["boxes"] < -32768)).any())
                area = box_areas(v, c)
                if (c.get("prep") or {}).get("bias") is not None and (area == 0).any() and area.any():
                    seen.add("empty beside a bias")
            seen.update(["straddle"] * straddle + ["outside int16"] * wide)
        self.units.update(seen)

    def check(self):
        """The conditions of the sweep, every count printed (pytest -s)."""
        at_least(self.srcs, pr.SOURCES, 10, "sources")
        at_least(self.dsts, [None] + list(pr.DESTS), 10, "destinations")
        at_least(self.modes, pr.MODES, 10, "modes")
        at_least(self.residues, range(16), 10, "residues")
        at_least(self.shares, ("tile", "rows"), 10, "plain fields")
        terms = [(s, b) for s in rv.AFFINE_TERMS for b in rv.AFFINE_TERMS if (s, b) != ("none", "none")]
        at_least(self.combos, terms, 10, "(scale, bias)")
        if not self.crops:
            at_least(self.places, ("none", "letterbox", "free", "placement alone"), 10, "placement")
            at_least(self.placed, [f"lead[{j}] == 0" for j in (0, 1)] +
                     [f"lead[{j}] + inner[{j}] == size[{j}]" for j in (0, 1)], 10, "placed")
            at_least(self.fills, ("-0.0 to a float", "saturating to an integer"), 10, "fills")
            at_least(self.units, ("mixed",), 20, "units inside and outside the image")
        at_least(self.records, ("two fields with a step",), 20, "records")
        at_least(self.records, ("a resized field without a step", "the first step not in field 0"), 10, "records")
        at_least(self.axes, ("first", "middle", "innermost", "broadcast", "reversed", "negative"), 10, "channel axis")
        at_least(self.axes, ("extent 1",), 1, "channel axis")
        at_least(self.axes, ("five dimensions or more",), 20, "channel axis")
        at_least(self.tables, (0, 4, 8, 12, "an exact 0.0, -0.0 or 1.0"), 10, "tables mod 16")
        at_least(self.units, ("changes", "keeps"), 20, "units and the channel coordinate")
        if self.crops:
            at_least(self.units, ("straddle", "outside int16", "empty beside a bias"), 20, "crops")
            at_least(self.counts, rv.CROP_COUNTS, 1, "K")
        # the caps on the reference
        print(f"shares: {self.bound} of {self.ints} integer outputs on a bound; {self.outside} of "
              f"{self.placed_elems} placed elements outside the image; {self.nothing} of {self.steps} "
              f"steps change nothing; {self.nonfinite} of {self.floats} float outputs not finite")
        assert 2 * self.bound <= self.ints, (self.bound, self.ints)
        assert 2 * self.outside <= self.placed_elems, (self.outside, self.placed_elems)
        assert 10 * self.nothing <= self.steps, (self.nothing, self.steps)
        assert 20 * self.nonfinite <= self.floats, (self.nonfinite, self.floats)


def prep_sweep(seeds, case, crops, emulator, tmp_path):
    """Every seed through the emulated body, bit for bit against `pr.want`; the conditions."""
    batch, stats = PrepBatch(tmp_path), PrepStats(crops)
    for seed in seeds:
        rec, mis = case(seed)
        what = f"seed={seed} dst%16={mis}"
        assert all(rv.inside(b, v) for _, b, v in pr.triples(rec)), what
        if crops:
            k0 = len(next(x[3] for x in rec if x[3])["boxes"])
            stats.counts[k0] += 1
        addr = addresses(pr.bases_of(rec))
        with pr.plan_prep(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
            assert p.size == len(pr.oracle(rec)[0]) and p.segments() == [], what
            if crops and not k0:
                continue  # K == 0: the empty message, nothing is launched
            assert pr.plan_launch(p) == (10 if crops else 9), what
            stats.record(rec, mis, p)
        batch.add(what, rec, DST + mis)
    counts = batch.run(emulator)
    print(f"emulator: {counts}")
    assert batch.paths == {"head", "units", "tail"}, batch.paths
    assert counts["head_elements"] and counts["units"] and counts["tail_elements"], counts
    assert counts["table_loads"] and (counts["box_loads"] if crops else counts["outside"]), counts
    stats.check()


def test_prep_resizes(lib, prep_emulator, tmp_path):
    prep_sweep(PREP_RESIZE_SEEDS, prep_resize_case, False, prep_emulator, tmp_path)


def test_prep_crops(lib, prep_emulator, tmp_path):
    prep_sweep(PREP_CROP_SEEDS, prep_crop_case, True, prep_emulator, tmp_path)


def host_plans(seeds, case):
    """Every seed planned over host memory: resize_host and crop_host of tensor_plan.cpp write the
    staged segments, which laid out by their offsets hold `pr.want` of every field."""
    import ctypes
    for seed in seeds:
        rec, _ = case(seed)
        what = f"seed={seed}"
        sample, info, ranges = pr.oracle(rec)
        with pr.plan_prep(rec, host_ptr, ARROW_DEVICE_CPU) as p:
            assert p.size == len(sample) and p.type_info().to_json() == info.to_json(), what
            got = bytearray([POISON]) * p.size
            for ptr, off, n in p.segments():
                assert got[off:off + n] == bytes([POISON]) * n and off + n <= p.size, what
                got[off:off + n] = ctypes.string_at(ptr, n)
            for (off, ln), (_, _, v, c) in zip(ranges, rec):
                pr.same(got[off:off + ln], pr.want(v, c), what)
                got[off:off + ln] = bytes([POISON]) * ln
            assert bytes(got) == bytes([POISON]) * p.size, "padding staged, " + what


def test_prep_resizes_over_host_memory(lib):
    host_plans(PREP_RESIZE_SEEDS, prep_resize_case)


def test_prep_crops_over_host_memory(lib):
    host_plans(PREP_CROP_SEEDS, prep_crop_case)


def stepped_field(rec):
    return next(i for i, x in enumerate(rec) if x[3] and x[3].get("prep"))


def one_case(tmp_path, emulator, seed, case):
    """The batch of one seed's case, run once."""
    rec, mis = case(seed)
    batch = PrepBatch(tmp_path)
    batch.add(f"seed={seed}", rec, DST + mis)
    batch.run(emulator)
    return batch


def test_the_prep_resize_sweep_notices_a_moved_image(lib, prep_emulator, tmp_path):
    """`lead` of the first placed seed one step further along an axis and `inner` one step shorter,
    so that the image still lies inside the output: another statement, the comparison fails."""
    for seed in PREP_RESIZE_SEEDS:
        rec, _ = prep_resize_case(seed)
        i = stepped_field(rec)
        v, c = rec[i][2], rec[i][3]
        q = c["prep"]
        j = next((j for j in (0, 1) if q["inner"] is not None and q["inner"][j] >= 2), None)
        if j is None:
            continue
        moved = dict(q, inner=tuple(n - (k == j) for k, n in enumerate(q["inner"])),
                     lead=tuple(n + (k == j) for k, n in enumerate(q["lead"])))
        if pr.want(v, dict(c, prep=moved)).tobytes() != pr.want(v, c).tobytes():  # (the reference notices)
            break
    else:
        raise AssertionError("no placed seed")
    batch = one_case(tmp_path, prep_emulator, seed, prep_resize_case)
    lines = batch.spec[-1].split("\n")
    words = lines[1 + i].split(" ")
    assert [int(w) for w in words[-7:-3]] == [*q["inner"], *q["lead"]]
    words[-7 + j], words[-5 + j] = str(q["inner"][j] - 1), str(q["lead"][j] + 1)
    lines[1 + i] = " ".join(words)
    batch.spec[-1] = "\n".join(lines)
    with pytest.raises(AssertionError):
        batch.run(prep_emulator)


def changed_table_word(tmp_path, emulator, seeds, case):
    """One float32 word of the first table of the first seed that has one under a float destination
    (where no saturation hides it) replaced by another number: the comparison fails."""
    for seed in seeds:
        rec, _ = case(seed)
        i = stepped_field(rec)
        v, c = rec[i][2], rec[i][3]
        w = next((w for w in ("scale", "bias") if pr.is_table(c["prep"][w])), None)
        if w is None or c["dst"] not in ("float16", "float32") or not v.size:
            continue
        tb, tv = c["prep"][w]
        other = tv.copy()
        other[0] = -2.0 * other[0] - 3.0
        changed = dict(c, prep=dict(c["prep"], **{w: (other, other)}))
        if pr.want(v, changed).tobytes() != pr.want(v, c).tobytes():  # (the reference notices)
            break
    else:
        raise AssertionError("no seed with a table under a float destination")
    batch = one_case(tmp_path, emulator, seed, case)
    name = batch.spec[-1].split("\n")[1 + i].split(" ")[-2 if w == "scale" else -1]
    words = np.fromfile(name, np.float32)
    assert words.tobytes() == tv.tobytes()
    other.tofile(name)
    with pytest.raises(AssertionError):
        batch.run(emulator)


def test_the_prep_resize_sweep_notices_a_changed_table_word(lib, prep_emulator, tmp_path):
    changed_table_word(tmp_path, prep_emulator, PREP_RESIZE_SEEDS, prep_resize_case)


def test_the_prep_crop_sweep_notices_a_changed_table_word(lib, prep_emulator, tmp_path):
    changed_table_word(tmp_path, prep_emulator, PREP_CROP_SEEDS, prep_crop_case)


def test_the_prep_crop_sweep_notices_a_changed_box_word(lib, prep_emulator, tmp_path):
    """The first box, a whole frame, two steps shorter along its second axis."""
    for seed in PREP_CROP_SEEDS:
        rec, _ = prep_crop_case(seed)
        i = stepped_field(rec)
        v, c = rec[i][2], rec[i][3]
        if len(c["boxes"]) and v.shape[c["axes"][1]] > 3 and \
                tuple(c["boxes"][0]) == (0, 0, v.shape[c["axes"][0]], v.shape[c["axes"][1]]):
            rows = c["boxes"].copy()
            rows[0, 1] += 2
            if pr.want(v, dict(c, boxes=rows)).tobytes() != pr.want(v, c).tobytes():
                break
    else:
        raise AssertionError("no seed whose first box is the whole frame")
    batch = one_case(tmp_path, prep_emulator, seed, prep_crop_case)
    name = batch.spec[-1].split("\n")[1 + i].split(" ")[-18]
    words = np.fromfile(name, np.int32)
    assert words.tobytes() == c["boxes"].tobytes()
    words[1] += 2
    words.tofile(name)
    with pytest.raises(AssertionError):
        batch.run(prep_emulator)


def test_a_prep_resize_of_an_element_misaligned_source_is_refused(lib):
    for seed in MISALIGNED_PREP_RESIZE_SEEDS:
        rec = rv.misaligned_op(rv.rng(seed), "prep_resize")
        ok, text = refused_by_name(pr.plan_prep, rec, pr.bases_of(rec))
        assert ok, (seed, text)


def test_prep_crops_of_an_element_misaligned_source_are_refused(lib):
    for seed in MISALIGNED_PREP_CROP_SEEDS:
        rec = rv.misaligned_op(rv.rng(seed), "prep_crop")
        ok, text = refused_by_name(pr.plan_prep, rec, pr.bases_of(rec))
        assert ok, (seed, text)
