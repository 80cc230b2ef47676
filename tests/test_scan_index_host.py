"""The scan share of gather_struct_kernel on the CPU (no GPU): csrc/testing/scan_emulate.cpp, a
stand-alone program built here with the host compiler under AddressSanitizer and UBSan, runs
gather_device.h's scan:: — tile -> word range, thread -> words, the LDS slots of the doubling
scan, the carry and the clamps — thread by thread and phase by phase.  It fails on any LDS index
outside the buffer, any slot touched by two threads inside one phase, any input index outside
[0, count), and any output word not written exactly once or written past (B + 1) * 4 bytes; the
words it writes are compared here with a numpy statement of the two formulas.  Both operators and
both input widths run at 1, 2, 63, 64, 65, 255, 256, 257, 1025 and 4097 words (the tile is 1024
words: the last two carry across one and four tile boundaries) over zeros, negative words, sums
that pass N mid-way, words beyond 32 bits and offsets that are not monotone.

The fields' shares behind an offsets buffer start at 4 mod 16 and other odd alignments: the struct
emulation (csrc/testing/gather_struct_emulate.cpp) runs the records of a ragged-batch plan at
destinations 4, 5 and 12 mod 16."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, PARTITION_LENGTHS
from tests import list_records as lr
from tests import struct_records as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1025, 4097)
POISON = 0xA5


def build(tmp_path_factory, name):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if not cxx:
        pytest.fail("no host C++ compiler to build the emulation with")
    exe = str(tmp_path_factory.mktemp(name) / name)
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dora_amd", "csrc"),
           os.path.join(ROOT, "dora_amd", "csrc", "testing", name + ".cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


@pytest.fixture(scope="module")
def scan_emulator(tmp_path_factory):
    return build(tmp_path_factory, "scan_emulate")


@pytest.fixture(scope="module")
def struct_emulator(tmp_path_factory):
    return build(tmp_path_factory, "gather_struct_emulate")


def cases(count, wide, offsets_form):
    """(label, words, N) for one size, width and form."""
    rng = np.random.default_rng(1000 * count + 10 * wide + offsets_form)
    dt = np.int64 if wide else np.int32
    small = rng.integers(0, 10, count)
    out = [("zeros", np.zeros(count, dt), 0), ("zeros, N > 0", np.zeros(count, dt), 7)]
    if offsets_form:
        mono = np.cumsum(small) - small[0]
        out.append(("a partition", mono.astype(dt), int(mono[-1])))
        out.append(("ends past N", mono.astype(dt), int(mono[-1]) // 2))
        walk = np.cumsum(rng.integers(-6, 9, count))
        out.append(("not monotone, negative words", walk.astype(dt), int(max(walk.max(), 0)) // 2 + 3))
        out.append(("starts above 0", (mono + 5).astype(dt), int(mono[-1]) + 2))
    else:
        out.append(("a partition", small.astype(dt), int(small.sum())))
        out.append(("the sum passes N mid-way", small.astype(dt), int(small.sum()) // 2))
        neg = rng.integers(-5, 10, count)
        out.append(("negative words", neg.astype(dt), int(np.maximum(neg, 0).sum())))
        out.append(("negative words, short of N", neg.astype(dt), int(np.maximum(neg, 0).sum()) + 9))
    info = np.iinfo(dt)
    edge = rng.choice(np.array([info.max, info.min, 0, 1, -1, 3], dtype=dt), count)
    out.append(("extreme words", edge, (1 << 31) - 1))
    out.append(("extreme words, small N", edge, 5))
    if wide:
        big = rng.choice(np.array([(1 << 31) + 1, 1 << 40, -(1 << 33), 2, 0, 1 << 62], dtype=dt), count)
        out.append(("words beyond 32 bits", big, 1000))
        out.append(("words beyond 32 bits, N at its cap", big, (1 << 31) - 1))
    return out


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("wide", [0, 1], ids=["int32", "int64"])
@pytest.mark.parametrize("offsets_form", [0, 1], ids=["lengths", "offsets"])
def test_emulated_scan(scan_emulator, tmp_path, offsets_form, wide, count):
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    for label, words, n in cases(count, wide, offsets_form):
        assert words.dtype == (np.int64 if wide else np.int32) and len(words) == count
        words.tofile(src)
        r = subprocess.run([scan_emulator, str(count), str(n), str(wide), str(offsets_form), src, out],
                           capture_output=True, text=True)
        text = r.stdout + r.stderr[-2000:]
        assert r.returncode == 0 and text.startswith("ok"), (label, text)
        got = np.fromfile(out, dtype=np.int32)
        want = lr.clamped_offsets(words, offsets_form, n)
        assert len(got) == len(want) == count + (0 if offsets_form else 1), label
        assert got.tobytes() == want.tobytes(), (label, np.flatnonzero(got != want)[:5])
        # whatever the words hold: 0 <= o[0] <= .. <= o[B] <= N
        assert got[0] >= 0 and got[-1] <= n and (np.diff(got) >= 0).all(), label
        assert f"tiles={(count + 1023) // 1024}" in text, text


def test_no_lists(scan_emulator, tmp_path):
    """B == 0 from lengths: no word is read and one offset, 0, is written."""
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    open(src, "wb").close()
    r = subprocess.run([scan_emulator, "0", "5", "1", "0", src, out], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok words=1 tiles=0 loads=0"), r.stdout
    assert np.fromfile(out, dtype=np.int32).tolist() == [0]


@pytest.mark.parametrize("name", list(lr.RECORDS))
def test_field_shares_behind_an_offsets_buffer(lib, struct_emulator, tmp_path, name):
    """The fields of a ragged-batch plan (device values, B == 1: 8 bytes of offsets in front)
    through the struct emulation with the sample at 12, 13 and 4 mod 16, so that the first field
    starts at 4, 5 and 12 mod 16: every field's bytes are the oracle's, and neither the offsets
    buffer nor any padding byte is written by a field's share."""
    from tests.test_gather_struct_index_host import FAKE, run, write_spec
    rec = lr.RECORDS[name](67)
    sample, info, ranges = lr.oracle(rec, [0, 67])
    bases = sr.bases_of(rec)
    addr = {id(b): FAKE + (1 << 24) * i for i, b in enumerate(bases)}
    with lr.plan_list(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM, np.array([67], np.int32),
                      PARTITION_LENGTHS, ARROW_DEVICE_CPU) as p:
        assert p.size == len(sample)
        for dst, first in ((0x7F00_0000_100C, 4), (0x7F00_0000_100D, 5), (0x7F00_0000_2004, 12)):
            fields = sr.plan_fields(p, dst)
            assert [(d["off"], d["bytes"]) for d in fields] == ranges
            assert (dst + fields[0]["off"]) % 16 == first
            files = []
            for k, ((_, b, _), d) in enumerate(zip(rec, fields)):
                off = d["src"] - addr[id(b)]
                assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes
                files.append(str(tmp_path / f"src{k}.bin"))
                with open(files[-1], "wb") as f:
                    f.write(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
            spec, out = str(tmp_path / "spec.txt"), str(tmp_path / "out.bin")
            write_spec(spec, fields, dst, p.size, files)
            rc, text = run(struct_emulator, spec, out)
            assert rc == 0 and text.startswith("ok"), (name, hex(dst), text)
            with open(out, "rb") as f:
                got = f.read()
            pad = bytearray(got)
            for off, ln in ranges:
                assert got[off:off + ln] == sample[off:off + ln], (name, hex(dst), off)
                pad[off:off + ln] = bytes([POISON]) * ln
            assert bytes(pad) == bytes([POISON]) * len(got), (name, hex(dst))


def test_the_scan_emulation_notices_what_it_checks(scan_emulator, tmp_path):
    """An input file shorter than `count` words is refused before anything runs, and a count past
    the cap of one workgroup's scan is no case at all."""
    src, out = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.zeros(3, np.int32).tofile(src)
    r = subprocess.run([scan_emulator, "4", "5", "0", "0", src, out], capture_output=True, text=True)
    assert r.returncode == 2 and "input file" in r.stdout
    r = subprocess.run([scan_emulator, str((1 << 20) + 1), "5", "0", "0", src, out],
                       capture_output=True, text=True)
    assert r.returncode == 2 and "bad case" in r.stdout
