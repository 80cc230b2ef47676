"""The body of gather_resize_kernel on the CPU (no GPU): csrc/testing/resize_emulate.cpp, a
stand-alone program built here with the host compiler under AddressSanitizer and UBSan, runs
resize_device.h — output unit -> element -> coordinates, the odometer, the taps and weights of the
two resized axes, the blend, the head and tail elements — over the whole grid of device resize
plans made over made-up pointers.  It fails on any source read outside the field's [lo, hi], any
tap that is not a naturally aligned element load, any output byte not written exactly once and any
written at or past the field's end; the bytes it writes are compared here with
`tensor.from_numpy_resize`.

The cases are tests/resize_records.py's, at every destination offset each names.
tests/test_gpu_tensor_resize_device.py runs the same cases on the GPU, each after it passed
here."""
import os
import re
import shutil
import subprocess

import pytest

from dora_amd._lib import ARROW_DEVICE_ROCM
from tests import resize_records as rr
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
    exe = str(tmp_path_factory.mktemp("resize_emulate") / "resize_emulate")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dora_amd", "csrc"),
           os.path.join(ROOT, "dora_amd", "csrc", "testing", "resize_emulate.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


class Batch:
    """Cases gathered into one spec file for one run of the emulator: each a device resize plan of
    a record over made-up pointers and the bytes every field must come out as."""

    def __init__(self, tmp_path):
        self.dir, self.spec, self.want, self.files = tmp_path, [], [], 0
        self.paths = set()

    def _file(self, data):
        name = str(self.dir / f"f{self.files}.bin")
        self.files += 1
        with open(name, "wb") as f:
            f.write(data)
        return name

    def add(self, label, rec, dst):
        bases = rr.bases_of(rec)
        addr = {id(b): FAKE + (1 << 26) * i + misalignment(b) for i, b in enumerate(bases)}
        with rr.plan_resize(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
            assert p.segments() == [], label
            fields, ks = sr.plan_fields(p, dst), rr.plan_resizes(p, len(rec), dst)
            assert len(fields) == len(rec), label
            lines = [f"{len(rec)} {dst} {p.size}"]
            ranges = []
            for (_, b, v, r), d, k in zip(rec, fields, ks):
                assert d["gather"] and bool(k["mode"]) == (r is not None), label
                off = d["src"] - addr[id(b)]
                assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes, (label, d)
                src = self._file(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
                expect = rr.want(v, r)
                if r:
                    ax = [a % v.ndim for a in r["axes"]]
                    head = [1, k["mode"], rr.SOURCES[r["src"]][1], d["elem"] * 8,
                            rr.DESTS[rr.dst_name(r)][0], k["bits"], v.ndim, *ax, *k["in"],
                            *expect.shape, *v.strides, k["count"]]
                    self.paths |= {n for n in ("head", "units", "tail") if k[n]}
                else:
                    head = [0] * 11 + [0]
                lines.append(" ".join(map(str, [
                    *head, d["elem"], d["row"], v.nbytes, d["bytes"], d["lo"], d["hi"], d["src"],
                    d["off"], d["nd"], *d["shape"], *d["stride"], src])))
                ranges.append((d["off"], expect))
                assert expect.nbytes == d["bytes"], label
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
                rr.same(sample[off:off + want.nbytes], want, label)
                sample[off:off + want.nbytes] = bytes([POISON]) * want.nbytes
            assert bytes(sample) == bytes([POISON]) * size, (label, "a byte outside the fields was written")
        assert at == len(got)
        return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", text)}


def test_every_case_through_the_emulated_body(lib, emulator, tmp_path):
    batch = Batch(tmp_path)
    for label, rec, offsets in rr.cases():
        for mis in offsets:
            batch.add(f"{label} dst%16={mis}", rec, DST + mis)
    counts = batch.run(emulator)
    assert batch.paths == {"head", "units", "tail"}, batch.paths
    assert counts["head_elements"] and counts["units"] and counts["tail_elements"], counts


def test_the_limit_of_the_contract_through_the_emulated_body(lib, emulator, tmp_path):
    """Axes of 32768 source and output steps, where the statement's integers come closest to 2^31
    and d = 2 * O is 65536, and the weights read directly: a column [0, 1] resized along axis 0
    is w1 of every output coordinate, [1, 0] is w0.  The statement of record's own weights are
    first held against the integer formula divided in float64 and rounded once."""
    import numpy as np
    for label, rec, _ in rr.limit_cases():
        if label.startswith(("w1 ", "w0 ")):
            (_, _, v, r), = rec
            w0, w1, last = rr.weights_in_float64(2, r["size"][0])
            want = rr.want(v, r)
            # (where the last element stands alone the output is that element: 1 or 0)
            expect = np.where(last, v[1, 0], w1 if label.startswith("w1 ") else w0)
            assert want.tobytes() == expect.astype(np.float32).tobytes(), label
            assert len(np.unique(want)) > r["size"][0] // 2, label  # (weights, not a constant)
    batch = Batch(tmp_path)
    for label, rec, offsets in rr.limit_cases():
        assert rr.want(rec[0][2], rec[0][3]).size <= 5 * rr.LIMIT, label
        for mis in offsets:
            batch.add(f"{label} dst%16={mis}", rec, DST + mis)
    counts = batch.run(emulator)
    assert counts["units"] > 10 * rr.LIMIT // 16, counts


def test_the_record_fields_meet_heads_and_tails(lib):
    starts = set()
    for mis in (0, 2, 8):
        with rr.plan_resize(rr.record(5), lambda b: FAKE, ARROW_DEVICE_ROCM) as p:
            fields = sr.plan_fields(p, DST + mis)
            starts |= {(DST + mis + fields[k]["off"]) % 16 for k in (1, 3)}
            assert fields[2]["off"] % 4 == 0 and fields[3]["off"] % 2 == 0
    assert len(starts) >= 3, starts


def test_the_emulation_notices_what_it_checks(emulator, tmp_path):
    """A reach one byte short is a source offset outside [lo, hi]; a source address that is odd is
    a load not naturally aligned; a sample one byte short does not fit."""
    import numpy as np
    np.arange(64, dtype=np.uint8).tofile(str(tmp_path / "src.bin"))
    src = str(tmp_path / "src.bin")

    def run(size, hi, addr=FAKE):
        spec = str(tmp_path / "spec.txt")
        with open(spec, "w") as f:  # 4 x 8 int16 -> 2 x 4 int16, bilinear
            f.write(f"1 {DST} {size}\n1 2 0 16 0 16 2 0 1 4 8 2 4 16 2 8 2 64 64 16 0 {hi} "
                    f"{addr} 0 0 {src}\n")
        r = subprocess.run([emulator, spec], capture_output=True, text=True)
        return r.returncode, r.stdout

    rc, text = run(16, 63)
    assert rc == 0 and text.startswith("ok cases=1 grid=1 loads=32 head_elements=0 units=1 "), text
    rc, text = run(16, 62)
    assert rc == 1 and "source offset outside [lo, hi]" in text
    rc, text = run(16, 63, FAKE + 1)
    assert rc == 1 and "not naturally aligned" in text
    rc, text = run(15, 63)
    assert rc == 2 and "does not fit" in text
