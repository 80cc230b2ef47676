"""The bodies of gather_reduce_kernel on the CPU (no GPU): csrc/testing/argmax_emulate.cpp, a
stand-alone program built here with the host compiler under AddressSanitizer and UBSan, runs
reduce_device.h — output unit -> element -> row and place in it, the odometer, the lane body's
vector and element path, its head and tail elements, and the wave body with all 64 lanes of a wave
in lock step through the butterfly — over the whole grid of device reduce plans made over made-up
pointers.  It fails on any source read outside the field's [lo, hi], any load that is not naturally
aligned, any output byte not written exactly once and any written at or past the field's end; the
bytes it writes are compared here with `np.argmax(x32, axis).astype(dtype)`.

The cases are tests/argmax_records.py's; every one runs under the library's own choice of body and
again with the lane body and the wave body forced wherever each applies, so both bodies see every
C on either side of the crossover.  tests/test_gpu_tensor_argmax_device.py runs the same cases on
the GPU, each after it passed here."""
import os
import re
import shutil
import subprocess

import pytest

from dora_amd import _lib
from dora_amd._lib import ARROW_DEVICE_ROCM
from tests import argmax_records as ar
from tests import struct_records as sr
from tests.gather_views import misalignment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F10_0000_0000  # never dereferenced
DST = 0x7F50_0000_1000
POISON = 0xA5


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if not cxx:
        pytest.fail("no host C++ compiler to build the emulation with")
    exe = str(tmp_path_factory.mktemp("argmax_emulate") / "argmax_emulate")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dora_amd", "csrc"),
           os.path.join(ROOT, "dora_amd", "csrc", "testing", "argmax_emulate.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


@pytest.fixture
def body(lib):
    """Sets which body reduces (dora_gpu_test_reduce_body); the library's own choice afterwards."""
    def force(mode):
        _lib.call("dora_gpu_test_reduce_body", mode)
    yield force
    _lib.call("dora_gpu_test_reduce_body", 0)


class Batch:
    """Cases gathered into one spec file for one run of the emulator: each a device reduce plan of
    a record over made-up pointers and the bytes every field must come out as."""

    def __init__(self, tmp_path):
        self.dir, self.spec, self.want, self.files = tmp_path, [], [], 0
        self.bodies = set()

    def _file(self, data):
        name = str(self.dir / f"f{self.files}.bin")
        self.files += 1
        with open(name, "wb") as f:
            f.write(data)
        return name

    def add(self, label, rec, dst):
        bases = ar.bases_of(rec)
        addr = {id(b): FAKE + (1 << 26) * i + misalignment(b) for i, b in enumerate(bases)}
        with ar.plan_reduce(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
            assert p.segments() == [], label
            fields, reds = sr.plan_fields(p, dst), ar.plan_reduces(p, len(rec), dst)
            assert len(fields) == len(rec), label
            lines = [f"{len(rec)} {dst} {p.size}"]
            ranges = []
            for (_, b, v, r), d, k in zip(rec, fields, reds):
                assert d["gather"] and bool(k["op"]) == (r is not None), label
                off = d["src"] - addr[id(b)]
                assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes, (label, d)
                src = self._file(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
                code = ar.SOURCES[r["src"]][1] if r else 0
                icode = ar.INDEX[r["dtype"]][0] if r else 0
                lines.append(" ".join(map(str, [
                    int(r is not None), code, d["elem"] * 8 if r else 0, icode, k["bits"], k["c"],
                    k["cstride"], int(k["body"] == 2), k["count"], d["elem"], d["row"],
                    k["count"] * d["elem"] if r else d["bytes"], d["bytes"], d["lo"], d["hi"],
                    d["src"], d["off"], d["nd"], *d["shape"], *d["stride"], src])))
                ranges.append((d["off"], ar.want(v, r)))
                assert ranges[-1][1].nbytes == d["bytes"], label
                if r:
                    self.bodies.add("wave" if k["body"] == 2 else "lane")
                    self.bodies |= {name for name, units in (("vector", k["vector_units"]),
                                                             ("element", k["element_units"])) if units}
            self.spec.append("\n".join(lines))
            self.want.append((label, p.size, ranges))

    def run(self, emulator):
        spec, out = str(self.dir / "spec.txt"), str(self.dir / "out.bin")
        with open(spec, "w") as f:
            f.write("\n".join(self.spec) + "\n")
        r = subprocess.run([emulator, spec, out], capture_output=True, text=True)
        text = r.stdout + r.stderr[-3000:]
        assert r.returncode == 0 and text.startswith(f"ok cases={len(self.want)} "), text
        with open(out, "rb") as f:
            got = f.read()
        at = 0
        for label, size, ranges in self.want:
            sample = bytearray(got[at:at + size])
            at += size
            for off, want in ranges:
                ar.same(sample[off:off + want.nbytes], want, label)
                sample[off:off + want.nbytes] = bytes([POISON]) * want.nbytes
            assert bytes(sample) == bytes([POISON]) * size, (label, "a byte outside the fields was written")
        assert at == len(got)
        return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", text)}


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_every_case_through_the_emulated_bodies(lib, emulator, tmp_path, body, mode):
    """mode 0: the library's choice; 1: the lane body everywhere; 2: the wave body wherever the
    reduced axis is source-contiguous."""
    body(mode)
    batch = Batch(tmp_path)
    for label, rec, offsets in ar.cases():
        for mis in offsets:
            batch.add(f"{label} dst%16={mis}", rec, DST + mis)
    counts = batch.run(emulator)
    # the list reaches every body and both load paths of the lane body, whatever the crossover is
    want = {"lane", "vector", "element"} | ({"wave"} if mode != 1 else set())
    assert want <= batch.bodies, (mode, batch.bodies)
    assert counts["vector_units"] and counts["element_units"], counts
    assert bool(counts["wave_outputs"]) == (mode != 1), counts


def test_the_record_fields_start_at_2_and_4(lib):
    starts = set()
    for mis in (0, 2, 4):
        with ar.plan_reduce(ar.record(9), lambda b: FAKE, ARROW_DEVICE_ROCM) as p:
            fields = sr.plan_fields(p, DST + mis)
            starts |= {(DST + mis + fields[k]["off"]) % 16 for k in (0, 2)}
            assert fields[1]["off"] % 4 == 0
    assert {2, 4} <= starts, starts


def test_the_emulation_notices_what_it_checks(emulator, tmp_path):
    """A reach one byte short is a source offset outside [lo, hi]; a source address that is odd is
    a load not naturally aligned; a sample one byte short does not fit."""
    import numpy as np
    np.arange(64, dtype=np.uint8).tofile(str(tmp_path / "src.bin"))
    src = str(tmp_path / "src.bin")

    def run(size, hi, addr=FAKE, wave=0):
        spec = str(tmp_path / "spec.txt")
        with open(spec, "w") as f:  # 4 x 8 int16 along axis 1 (wave) or 8 x 4 along axis 0 -> int32
            c, stride, count = (8, 2, 4) if wave else (8, 8, 4)
            row = 2 if wave else 8
            nd = "1 4 16" if wave else "0"
            f.write(f"1 {DST} {size}\n1 0 16 0 32 {c} {stride} {wave} {count} 2 {row} 8 16 0 {hi} "
                    f"{addr} 0 {nd} {src}\n")
        r = subprocess.run([emulator, spec], capture_output=True, text=True)
        return r.returncode, r.stdout

    rc, text = run(16, 63)
    assert rc == 0 and text.startswith("ok cases=1 grid=1 loads=8 vector_units=1 "), text
    rc, text = run(16, 63, wave=1)
    assert rc == 0 and "wave_outputs=4" in text, text
    rc, text = run(16, 62)
    assert rc == 1 and "source offset outside [lo, hi]" in text
    rc, text = run(16, 63, FAKE + 1)
    assert rc == 1 and "not naturally aligned" in text
    rc, text = run(15, 63)
    assert rc == 2 and "does not fit" in text
