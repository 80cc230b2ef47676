"""The body of gather_crop_kernel on the CPU (no GPU): csrc/testing/crop_emulate.cpp, a stand-alone
program built here with the host compiler under AddressSanitizer and UBSan, runs crop_device.h —
output unit -> element -> coordinates, the odometer with K in front, the box read and clamped where
the crop changes, the taps and weights over the box's extents, the blend, the head and tail
elements — over the whole grid of device crop plans made over made-up pointers.  It fails on any
frame read outside the field's [lo, hi], any tap that is not a naturally aligned element load, any
word of the boxes outside [0, 16 K) or off its dword, any output byte not written exactly once and
any written at or past the field's end; the bytes it writes are compared here with
`tensor.from_numpy_crops`.

The cases are tests/crop_records.py's, at every destination offset each names.
tests/test_gpu_tensor_crops_device.py runs the same cases on the GPU, each after it passed here."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from dora_amd._lib import ARROW_DEVICE_ROCM
from tests import crop_records as kr
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
    exe = str(tmp_path_factory.mktemp("crop_emulate") / "crop_emulate")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dora_amd", "csrc"),
           os.path.join(ROOT, "dora_amd", "csrc", "testing", "crop_emulate.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


class Batch:
    """Cases gathered into one spec file for one run of the emulator: each a device crop plan of a
    record over made-up pointers and the bytes every field must come out as."""

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
        bases = kr.bases_of(rec)
        addr = {id(b): FAKE + (1 << 26) * i + misalignment(b) for i, b in enumerate(bases)}
        with kr.plan_crop(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
            assert p.segments() == [], label
            fields, ks = sr.plan_fields(p, dst), kr.plan_crops(p, len(rec), dst)
            assert len(fields) == len(rec), label
            lines = [f"{len(rec)} {dst} {p.size}"]
            ranges = []
            for (_, b, v, c), d, k in zip(rec, fields, ks):
                assert d["gather"] and bool(k["mode"]) == (c is not None), label
                off = d["src"] - addr[id(b)]
                assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes, (label, d)
                src = self._file(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
                expect = kr.want(v, c)
                if c:
                    ax = [a % v.ndim + 1 for a in c["axes"]]
                    ins = [v.shape[a - 1] for a in ax]
                    bits = kr.DESTS[kr.dst_name(c)][1]
                    head = [1, k["mode"], kr.SOURCES[c["src"]][1], d["elem"] * 8,
                            kr.DESTS[kr.dst_name(c)][0], bits, v.ndim + 1, *ax, *ins,
                            *expect.shape, 0, *v.strides, expect.size]
                    # the boxes: what the plan holds of them, checked against their own base
                    boff = k["boxes"] - addr[id(c["boxes_base"])]
                    assert k["lo"] == 0 and 0 <= boff and boff + k["hi"] < c["boxes_base"].nbytes, label
                    raw = c["boxes_base"].tobytes()[boff: boff + k["hi"] + 1]
                    assert raw == c["boxes"].tobytes(), label
                    tail = [k["k"], k["boxes"], k["hi"], self._file(raw)]
                    self.paths |= {n for n in ("head", "units", "tail") if k[n]}
                else:
                    head = [0] * 11 + [0]
                    tail = [0, 0, -1, "-"]
                lines.append(" ".join(map(str, [
                    *head, d["elem"], d["row"], v.nbytes, d["bytes"], d["lo"], d["hi"], d["src"],
                    d["off"], d["nd"], *d["shape"], *d["stride"], src, *tail])))
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
                kr.same(sample[off:off + want.nbytes], want, label)
                sample[off:off + want.nbytes] = bytes([POISON]) * want.nbytes
            assert bytes(sample) == bytes([POISON]) * size, (label, "a byte outside the fields was written")
        assert at == len(got)
        return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", text)}


def test_every_case_through_the_emulated_body(lib, emulator, tmp_path):
    batch = Batch(tmp_path)
    for label, rec, offsets in kr.cases():
        if not len(rec[0][3]["boxes"] if rec[0][3] else [1]):
            continue  # K == 0: nothing is launched (test_tensor_crops_plan.py)
        for mis in offsets:
            batch.add(f"{label} dst%16={mis}", rec, DST + mis)
    counts = batch.run(emulator)
    assert batch.paths == {"head", "units", "tail"}, batch.paths
    assert counts["head_elements"] and counts["units"] and counts["tail_elements"], counts
    assert counts["box_loads"] and counts["box_loads"] % 4 == 0, counts


def test_more_than_one_workgroup_through_the_emulated_body(lib, emulator, tmp_path):
    """The 40 crops the GPU test packs with 30 workgroups, at its two destination offsets."""
    batch = Batch(tmp_path)
    for label, rec in kr.many():
        for mis in (0, 7):
            batch.add(f"{label} dst%16={mis}", rec, DST + mis)
    counts = batch.run(emulator)
    assert counts["grid"] == 4 * 30 and counts["units"] >= 4 * 7679, counts


def test_the_limit_of_the_contract_through_the_emulated_body(lib, emulator, tmp_path):
    """A frame axis of 32768 steps under boxes over all of it, its last row alone and the int32
    extremes, to crops of 32768 x 1 and 7 x 2."""
    batch = Batch(tmp_path)
    for label, rec, offsets in kr.limit_cases():
        expect = kr.want(rec[0][2], rec[0][3])
        assert expect.size <= 100000 and sum(bool(e.any()) for e in expect) >= 2, label
        for mis in offsets:
            batch.add(f"{label} dst%16={mis}", rec, DST + mis)
    counts = batch.run(emulator)
    assert counts["units"] > 6 * 32768 // 16, counts


def test_units_straddle_crops(lib):
    """The crops of 15 uint8 elements: at each destination offset some whole unit holds the last
    elements of one crop and the first of the next, into the empty second crop and out of it."""
    label, rec, offsets = next(c for c in kr.cases() if c[0].startswith("units across crops"))
    assert offsets == (0, 1, 15) and kr.want(rec[0][2], rec[0][3]).shape == (5, 3, 5)
    assert not kr.want(rec[0][2], rec[0][3])[1].any()
    with kr.plan_crop(rec, lambda b: FAKE, ARROW_DEVICE_ROCM) as p:
        for mis in offsets:
            k = kr.plan_crops(p, 1, DST + mis)[0]
            firsts = [k["head"] + 16 * u for u in range(k["units"])]
            spans = {(e // 15, (e + 15) // 15) for e in firsts if e // 15 != (e + 15) // 15}
            # (at 1 mod 16 the head is the whole first crop: the first unit starts the empty one)
            assert (1, 2) in spans and ((0, 1) in spans or k["head"] == 15), (mis, spans)


def test_the_emulation_notices_what_it_checks(emulator, tmp_path):
    """A frame reach one byte short is a source offset outside [lo, hi]; a boxes reach one byte
    short is a boxes offset outside [0, hi]; boxes that do not sit on a dword are not launched; a
    sample one byte short does not fit."""
    np.arange(64, dtype=np.uint8).tofile(str(tmp_path / "src.bin"))
    np.array([[0, 0, 4, 8], [1, 2, 3, 6]], np.int32).tofile(str(tmp_path / "boxes.bin"))
    src, boxes = str(tmp_path / "src.bin"), str(tmp_path / "boxes.bin")

    def run(size, hi, boxes_hi=31, boxes_addr=FAKE + 4096):
        spec = str(tmp_path / "spec.txt")
        with open(spec, "w") as f:  # 2 boxes of a 4 x 8 int16 frame -> 2 x 2 x 4 int16, bilinear
            f.write(f"1 {DST} {size}\n1 2 0 16 0 16 3 1 2 4 8 2 2 4 0 16 2 16 2 64 64 32 0 {hi} "
                    f"{FAKE} 0 0 {src} 2 {boxes_addr} {boxes_hi} {boxes}\n")
        r = subprocess.run([emulator, spec], capture_output=True, text=True)
        return r.returncode, r.stdout

    rc, text = run(32, 63)  # two units, a crop each: 16 outputs of four taps, two boxes of four words
    assert rc == 0 and text.startswith("ok cases=1 grid=1 loads=64 box_loads=8 head_elements=0 units=2 "), text
    rc, text = run(32, 62)
    assert rc == 1 and "source offset outside [lo, hi]" in text
    rc, text = run(32, 63, boxes_hi=30)
    assert rc == 1 and "boxes offset outside [0, hi]" in text
    rc, text = run(32, 63, boxes_addr=FAKE + 4098)
    assert rc == 2 and "no field of crops" in text
    rc, text = run(31, 63)
    assert rc == 2 and "does not fit" in text
