"""The two compaction kernels of a mask plan on the CPU (no GPU): csrc/testing/mask_emulate.cpp, a
stand-alone program built here with the host compiler under AddressSanitizer and UBSan, runs
gather_device.h's mask:: — tile -> rows, thread -> bytes, the LDS slots of the reduction and of the
doubling scan, the carry and the scatter position — thread by thread and phase by phase, the
count kernel's workgroups first and the compact kernel's in descending order.  It fails on any
mask byte read outside [0, N), any LDS index outside the buffer, any slot written by two threads
or written by one and read by another inside one phase, any index or count word written outside
the workspace, any C word not written exactly once and any set row not scattered exactly once; the
words it writes are compared here with numpy.

N in 0, 1, 15, 16, 17, 255, 256, 257, T - 1, T, T + 1, 2T + 1 and 3T + 5 (T = mask::kTile, 4096
rows), one case of 257 T + 3 rows (more tiles than threads in the sum of the totals), the mask at
0, 1, 3 and 13 mod 16, masks all zero, all set, alternating, random, only the first row, only the
last row, and set bytes of 2, 0x80 and 0xFF.  Then the taken body's emulation
(csrc/testing/gather_take_emulate.cpp) runs the fields of device mask plans by the emulated
index, and the bytes are those of tensor.from_numpy_masked.

tests/test_gpu_tensor_mask_device.py runs the same shapes and masks on the GPU."""
import subprocess

import numpy as np
import pytest

from dora_amd._lib import ARROW_DEVICE_ROCM
from oracle.pack_ref import pack
from dora_amd import tensor
from tests import list_records as lr
from tests import mask_records as mr
from tests import struct_records as sr
from tests import take_records as tr
from tests.test_scan_index_host import build

FAKE = 0x7F10_0000_0000  # never dereferenced
MASK = 0x7F30_0000_0000
DST = 0x7F50_0000_1000
UNWRITTEN = 0xA5A5A5A5


@pytest.fixture(scope="module")
def mask_emulator(tmp_path_factory):
    return build(tmp_path_factory, "mask_emulate")


@pytest.fixture(scope="module")
def take_emulator(tmp_path_factory):
    return build(tmp_path_factory, "gather_take_emulate")


def want_index(mask):
    ix = np.full(len(mask), -1, np.int32)
    rows = np.flatnonzero(mask)
    ix[:len(rows)] = rows
    return ix


def emulate(exe, tmp_path, cases):
    """Run `cases`, (label, mask, shift, one_list, grid) each, in one run of the emulator and
    compare every case's words with numpy; returns the emulator's summary line."""
    spec, blob, out = (str(tmp_path / f) for f in ("spec.txt", "masks.bin", "out.bin"))
    at = 0
    with open(spec, "w") as s, open(blob, "wb") as b:
        for _, mask, shift, one_list, grid in cases:
            s.write(f"{len(mask)} {shift} {int(one_list)} {grid} {at}\n")
            b.write(mask.tobytes())
            at += len(mask)
    r = subprocess.run([exe, spec, blob, out], capture_output=True, text=True)
    text = r.stdout + r.stderr[-3000:]
    assert r.returncode == 0 and text.startswith(f"ok cases={len(cases)} "), text
    got = np.fromfile(out, dtype=np.int32)
    at, found = 0, []
    for label, mask, shift, one_list, grid in cases:
        n = len(mask)
        index, counts, offs = got[at:at + n], got[at + n:at + 2 * n + 1], got[at + 2 * n + 1:at + 2 * n + 3]
        at += 2 * n + 3
        ctx = (label, n, shift, one_list, grid)
        assert index.tobytes() == want_index(mask).tobytes(), ctx
        k = int((mask != 0).sum())
        if n:
            assert counts.tobytes() == mr.counts(mask).tobytes(), ctx
            want = [0, k] if one_list else [UNWRITTEN - (1 << 32)] * 2
            assert offs.tolist() == want, ctx
        else:  # no tile, no workgroup: nothing is written (the plan sends zero offsets itself)
            assert counts.view(np.uint32).tolist() == [UNWRITTEN], ctx
        found.append(index.copy())
    assert at == len(got)
    return text, found


@pytest.mark.parametrize("shift", mr.SHIFTS)
def test_emulated_compaction(mask_emulator, tmp_path, shift):
    cases, turn = [], 0
    for n in mr.SIZES:
        for label, mask in mr.masks(n):
            # one list and a partition in turn; several tiles also with fewer workgroups than tiles
            cases.append((label, mask, shift, turn % 2 == 0, 0))
            if n + shift > mr.TILE:
                cases.append((label + ", two workgroups", mask, shift, turn % 2 == 1, 2))
            turn += 1
    text, _ = emulate(mask_emulator, tmp_path, cases)
    tiles = sum((len(m) + s + mr.TILE - 1) // mr.TILE if len(m) else 0 for _, m, s, _, _ in cases)
    assert f"tiles={tiles} " in text, text


def test_more_tiles_than_threads(mask_emulator, tmp_path):
    mask = mr.masks(mr.MANY_TILES)[3][1]
    text, _ = emulate(mask_emulator, tmp_path, [("random at 0.5", mask, 3, True, 0)])
    assert "tiles=258 " in text, text  # (257 T + 3 rows from position 3: 258 tiles)


def xyi(n):
    p, i = lr.base(np.float32, (n, 3)), lr.base(np.uint8, (n,))
    return [("x", p, p[:, 0]), ("y", p, p[:, 1]), ("intensity", i, i)]


@pytest.mark.parametrize("name", ["bare", "three_fields", "xyi"])
def test_taken_fields_by_the_emulated_index(lib, mask_emulator, take_emulator, tmp_path, name):
    """A device mask plan's fields through the taken body by the index the compaction wrote,
    K = N words: every field's bytes are tensor.from_numpy_masked's, zero rows behind the K
    selected ones included."""
    for n in (17, 257, mr.TILE + 1):
        rec = {"bare": lr.bare, "xyi": xyi, "three_fields": lambda n: tr.three_fields(n)[0]}[name](n)
        bases = sr.bases_of(rec)
        addr = {id(b): FAKE + (1 << 26) * i for i, b in enumerate(bases)}
        masks = [mr.masks(n)[i] for i in (0, 2, 3, 5, 6)]
        _, found = emulate(mask_emulator, tmp_path, [(lb, m, 3, True, 0) for lb, m in masks])
        for (label, mask), index in zip(masks, found):
            sample, info = pack(tensor.from_numpy_masked(mr.values_of(rec), mask))
            ranges = mr.oracle(rec, mask)[2]
            with mr.plan_mask(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM, np.zeros_like(mask),
                              ARROW_DEVICE_ROCM, mask_ptr=MASK + 3) as p:
                assert p.size == len(sample) and p.segments() == []
                got = mr.plan_info(p)
                fields = sr.plan_fields(p, DST)
                ifile = str(tmp_path / "index.bin")
                index.tofile(ifile)
                lines = [f"{len(rec)} {DST} {p.size} {n} {n} 0 {ifile}"]
                for k, ((_, b, v), d) in enumerate(zip(rec, fields)):
                    assert d["gather"] and d["kind"] == -1 and (d["off"], d["bytes"]) == ranges[k]
                    off = d["src"] - addr[id(b)]
                    assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes, (label, k, d)
                    src = str(tmp_path / f"src{k}.bin")
                    with open(src, "wb") as f:
                        f.write(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
                    lines.append(" ".join(map(str, [d["elem"], d["row"], d["bytes"], d["lo"], d["hi"],
                                                    d["src"], d["off"], got["stride0"][k], d["nd"],
                                                    *d["shape"], *d["stride"], src])))
            spec, out = str(tmp_path / "take.txt"), str(tmp_path / "take.bin")
            with open(spec, "w") as f:
                f.write("\n".join(lines) + "\n")
            r = subprocess.run([take_emulator, spec, out], capture_output=True, text=True)
            text = r.stdout + r.stderr[-3000:]
            assert r.returncode == 0 and text.startswith("ok cases=1 "), (name, n, label, text)
            with open(out, "rb") as f:
                have = f.read()
            assert len(have) == len(sample)
            for off, ln in ranges:
                assert have[off:off + ln] == sample[off:off + ln], (name, n, label, off)


def test_the_emulation_notices_what_it_checks(mask_emulator, tmp_path):
    """Mask bytes that are not there are refused before anything runs, and N past the cap is no
    case at all."""
    spec, blob, out = (str(tmp_path / f) for f in ("spec.txt", "masks.bin", "out.bin"))
    np.ones(5, np.uint8).tofile(blob)
    for line, what in (("6 0 1 0 0\n", "mask bytes"), (f"{mr.MAX_ROWS + 1} 0 1 0 0\n", "bad case")):
        with open(spec, "w") as f:
            f.write(line)
        r = subprocess.run([mask_emulator, spec, blob, out], capture_output=True, text=True)
        assert r.returncode == 2 and what in r.stdout, r.stdout
