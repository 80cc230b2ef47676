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
