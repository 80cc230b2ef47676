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

tests/test_gpu_random_views.py runs the same seeds on the kernels."""
import collections
import subprocess

import numpy as np
import pytest

from dora_amd import _lib
from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, PARTITION_LENGTHS, PARTITION_OFFSETS
from tests import cast_records as cr
from tests import mask_records as mr
from tests import random_views as rv
from tests import struct_records as sr
from tests.gather_views import describe_view, misalignment
from tests.test_cast_index_host import Batch as CastBatch
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
