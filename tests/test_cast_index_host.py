"""The body of gather_cast_kernel on the CPU (no GPU): csrc/testing/cast_emulate.cpp, a
stand-alone program built here with the host compiler under AddressSanitizer and UBSan, runs
cast_device.h — output unit -> element -> row and place in it, the odometer, the vector and the
element path, the head and tail elements — lane by lane over the whole grid of device cast plans
made over made-up pointers.  It fails on any source read outside the field's [lo, hi], any load
that is not naturally aligned, any output byte not written exactly once and any written at or past
dst + total; the bytes it writes are compared here with numpy's
`(x.astype(float32) * float32(scale)).astype(dst)`.

Contiguous runs of 1, 3, 7, 8, 9, 17 and 1024 elements (dense and cut from a wider base), a
5 x 7 x 3 image permuted to 3 x 5 x 7, a negative and a zero stride in dimension 0, d0 in 1, 63,
64, 65 and 257, destinations at every multiple of the destination element size mod 16, every
source/destination pair, and a record of a cast from uint8, a plain float32 field and a cast from
float32 to float16 whose fields start at 2 and 4 mod 16.  The value sets of scaled float sources
(tests/cast_records.py) run dense and cut from a wider base.

tests/test_gpu_tensor_cast_device.py runs the same cases on the GPU, each after it passed here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from dora_amd._lib import ARROW_DEVICE_ROCM
from tests import cast_records as cr
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
    exe = str(tmp_path_factory.mktemp("cast_emulate") / "cast_emulate")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dora_amd", "csrc"),
           os.path.join(ROOT, "dora_amd", "csrc", "testing", "cast_emulate.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


class Batch:
    """Cases gathered into one spec file for one run of the emulator: each a device cast plan of
    a record over made-up pointers and the bytes every field must come out as."""

    def __init__(self, tmp_path):
        self.dir, self.spec, self.want, self.files = tmp_path, [], [], 0

    def _file(self, data):
        name = str(self.dir / f"f{self.files}.bin")
        self.files += 1
        with open(name, "wb") as f:
            f.write(data)
        return name

    def add(self, label, rec, dst):
        bases = cr.bases_of(rec)
        addr = {id(b): FAKE + (1 << 26) * i + misalignment(b) for i, b in enumerate(bases)}
        with cr.plan_cast(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
            assert p.segments() == [], label
            fields, casts = sr.plan_fields(p, dst), cr.plan_casts(p)
            assert len(fields) == len(casts) == len(rec), label
            lines = [f"{len(rec)} {dst} {p.size}"]
            ranges = []
            for (_, b, v, c), d, k in zip(rec, fields, casts):
                assert d["gather"] and k["cast"] == (c is not None), label
                off = d["src"] - addr[id(b)]
                assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes, (label, d)
                src = self._file(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
                scale_bits = int(np.float32(k["scale"]).view(np.uint32))
                lines.append(" ".join(map(str, [
                    int(k["cast"]), max(k["src_code"], 0), k["src_bits"], k["dst_bits"],
                    int(k["has_scale"]), scale_bits, k["count"], d["elem"], d["row"],
                    k["src_bytes"], d["bytes"], d["lo"], d["hi"], d["src"], d["off"], d["nd"],
                    *d["shape"], *d["stride"], src])))
                ranges.append((d["off"], cr.want(v, c)))
                assert ranges[-1][1].nbytes == d["bytes"], label
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
                cr.same(sample[off:off + want.nbytes], want, label)
                sample[off:off + want.nbytes] = bytes([POISON]) * want.nbytes
            assert bytes(sample) == bytes([POISON]) * size, (label, "a byte outside the fields was written")
        assert at == len(got)
        return text


def shape_cases(src, dst):
    """[(label, record)] of bare tensors of `src` cast to `dst`: every shape of the list above."""
    c, cs = cr.cast(src, dst), cr.cast(src, dst, 1 / 255)
    if src == dst:
        c = cr.cast(src, dst, 3.0)  # (without a scale it would be no cast)
    out = []
    for run in cr.RUNS:
        for dense in (True, False):
            b, v = cr.run_view(src, run, dense, d0=3 if run == 1024 else 5)
            out.append((f"run={run} dense={dense}", [(None, b, v, c)]))
    b, v = cr.image_view(src)
    out.append(("image", [(None, b, v, cs)]))
    for label, b, v in cr.strided_views(src):
        out.append((label, [(None, b, v, c)]))
    for d0 in cr.D0:
        b, v = cr.run_view(src, 3, False, d0=d0)
        out.append((f"d0={d0}", [(None, b, v, cs)]))
    return out


@pytest.mark.parametrize("src,dst", cr.PAIRS)
def test_every_shape_of_every_pair(lib, emulator, tmp_path, src, dst):
    batch = Batch(tmp_path)
    for label, rec in shape_cases(src, dst):
        for mis in cr.dst_offsets(dst):
            batch.add(f"{src}->{dst} {label} dst%16={mis}", rec, DST + mis)
    assert " vector_loads=" in batch.run(emulator)


def test_a_record_of_three_fields(lib, emulator, tmp_path):
    """A cast from uint8, a plain float32 field and a cast from float32 to float16, at every even
    destination mod 16 (all the float16 fields allow): the cast fields start at 2 and 4 mod 16
    among others, the plain field is padded to 4 behind an odd number of float16 elements."""
    batch = Batch(tmp_path)
    starts = set()
    for d0 in (3, 9, 64):
        rec = cr.three_fields(d0)
        for mis in range(0, 16, 2):
            batch.add(f"three fields d0={d0} dst%16={mis}", rec, DST + mis)
            ranges = batch.want[-1][2]
            starts |= {(DST + mis + ranges[k][0]) % 16 for k in (0, 2)}
            assert ranges[1][0] % 4 == 0
    assert {2, 4} <= starts, starts
    batch.run(emulator)


@pytest.mark.parametrize("k", range(3 + 4 * 2 * 3, cr.N_VALUE_SETS))
def test_scaled_float_sources_over_their_domain(lib, emulator, tmp_path, k):
    """The value sets of scaled float sources (tests/cast_records.py) through the emulated body,
    dense and cut from a wider base: the plain-integer converts and the host's float32 product
    give numpy's bits, subnormal products, signed zeros and overflow included."""
    label, x, c = cr.value_sets()[k]
    batch = Batch(tmp_path)
    batch.add(label, [(None, x, x, c)], DST)
    b, v = cr.cut_from_wider(x)
    batch.add(label + ", cut from a wider base", [(None, b, v, c)], DST + 4)
    batch.run(emulator)


def test_the_emulation_notices_what_it_checks(emulator, tmp_path):
    """A reach one byte short is a source offset outside [lo, hi]; a source address that is odd
    is a load not naturally aligned; a sample one byte short does not fit."""
    np.arange(64, dtype=np.uint8).tofile(str(tmp_path / "src.bin"))
    src = str(tmp_path / "src.bin")

    def run(size, hi, addr=FAKE):
        spec = str(tmp_path / "spec.txt")
        with open(spec, "w") as f:  # 16 int16 -> float32, one dense row
            f.write(f"1 {DST} {size}\n1 0 16 32 0 0 16 2 32 32 64 0 {hi} {addr} 0 0 {src}\n")
        r = subprocess.run([emulator, spec], capture_output=True, text=True)
        return r.returncode, r.stdout

    assert run(64, 31) == (0, "ok cases=1 grid=1 loads=4 vector_loads=4\n")
    rc, text = run(64, 30)
    assert rc == 1 and "source offset outside [lo, hi]" in text
    rc, text = run(64, 31, FAKE + 1)
    assert rc == 1 and "not naturally aligned" in text
    rc, text = run(63, 31)
    assert rc == 2 and "does not fit" in text
