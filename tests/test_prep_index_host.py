"""The bodies of gather_resize_prep_kernel and gather_crop_prep_kernel on the CPU (no GPU):
csrc/testing/prep_emulate.cpp, a stand-alone program built here with the host compiler under
AddressSanitizer and UBSan, runs resize_device.h and crop_device.h under their model-input flag —
the placement of the image, the fill outside it, the channel as a coordinate of the odometer, the
tables' words, product and sum — lane by lane over the whole grid of device prep plans made over
made-up pointers.  It fails on any source read outside the field's [lo, hi], any table index at
or past the table's words, any tap read for an element outside the image or of an empty box, any
misaligned load, any output byte not written exactly once and any written at or past the field's
end; the bytes it writes are compared here with `tensor.from_numpy_resize` /
`tensor.from_numpy_crops`.

The cases are tests/prep_records.py's, at every destination offset each names.
tests/test_gpu_tensor_prep_device.py runs the same cases on the GPU, each after it passed here."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from dora_amd._lib import ARROW_DEVICE_ROCM
from tests import crop_records as kr
from tests import prep_records as pr
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
    exe = str(tmp_path_factory.mktemp("prep_emulate") / "prep_emulate")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dora_amd", "csrc"),
           os.path.join(ROOT, "dora_amd", "csrc", "testing", "prep_emulate.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def f32_bits(x):
    return int(np.float32(x).view(np.uint32))


class Batch:
    """Cases gathered into one spec file for one run of the emulator: each a device prep plan of a
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
        bases = pr.bases_of(rec)
        addr = {id(b): FAKE + (1 << 26) * i + misalignment(b) for i, b in enumerate(bases)}
        crops = any(c and "boxes" in c for _, _, _, c in rec)
        with pr.plan_prep(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
            assert p.segments() == [] and pr.plan_launch(p) == (10 if crops else 9), label
            n = len(rec)
            fields, ps = sr.plan_fields(p, dst), pr.plan_preps(p, n)
            ks = kr.plan_crops(p, n, dst) if crops else rr.plan_resizes(p, n, dst)
            assert len(fields) == n, label
            lines = [f"{n} {dst} {p.size}"]
            ranges = []
            for (_, b, v, c), d, k, q in zip(rec, fields, ks, ps):
                assert d["gather"] and bool(k["mode"]) == (c is not None), label
                off = d["src"] - addr[id(b)]
                assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes, (label, d)
                src = self._file(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
                expect = pr.want(v, c)
                tail, prep = [0, 0, -1, "-"], [0] * 15 + ["-", "-"]
                if c:
                    up = 1 if crops else 0  # (K in front)
                    ax = [a % v.ndim + up for a in c["axes"]]
                    ins = [v.shape[a - up] for a in ax]
                    bits = pr.DESTS[pr.dst_name(c)][1]
                    head = [2 if crops else 1, k["mode"], pr.SOURCES[c["src"]][1], d["elem"] * 8,
                            pr.DESTS[pr.dst_name(c)][0], bits, v.ndim + up, *ax, *ins,
                            *expect.shape, *([0] * up), *v.strides, expect.size]
                    self.paths |= {name for name in ("head", "units", "tail") if k[name]}
                else:
                    head = [0] * 11 + [0]
                if c and crops:
                    # the boxes: what the plan holds of them, checked against their own base
                    boff = k["boxes"] - addr[id(c["boxes_base"])]
                    assert k["lo"] == 0 and 0 <= boff and boff + k["hi"] < c["boxes_base"].nbytes, label
                    raw = c["boxes_base"].tobytes()[boff: boff + k["hi"] + 1]
                    assert raw == c["boxes"].tobytes(), label
                    tail = [k["k"], k["boxes"], k["hi"], self._file(raw)]
                if c and c.get("prep"):
                    g = c["prep"]
                    files = []
                    for w in ("scale", "bias"):
                        if not pr.is_table(g[w]):
                            assert q[w + "_table"] == 0, label
                            files.append("-")
                            continue
                        # the table: what the plan holds of it, checked against its own base
                        tb, tv = g[w]
                        toff = q[w + "_table"] - addr[id(tb)]
                        assert q["lo"] == 0 and 0 <= toff and toff + q["hi"] < tb.nbytes, label
                        raw = tb.tobytes()[toff: toff + q["hi"] + 1]
                        assert raw == tv.tobytes(), label
                        files.append(self._file(raw))
                    scal = [None if pr.is_table(g[w]) else g[w] for w in ("scale", "bias")]
                    placed = g["inner"] is not None
                    prep = [1, q["scale_table"], q["bias_table"], q["channels"], max(q["axis"], 0),
                            *(int(x is not None) for x in scal),
                            *(f32_bits(1.0 if x is None else x) for x in scal), int(placed),
                            *q["inner"], *q["lead"], f32_bits(g["fill"] if placed else 0.0), *files]
                else:
                    assert not q["on"], label
                lines.append(" ".join(map(str, [
                    *head, d["elem"], d["row"], v.nbytes, d["bytes"], d["lo"], d["hi"], d["src"],
                    d["off"], d["nd"], *d["shape"], *d["stride"], src, *tail, *prep])))
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
                pr.same(sample[off:off + want.nbytes], want, label)
                sample[off:off + want.nbytes] = bytes([POISON]) * want.nbytes
            assert bytes(sample) == bytes([POISON]) * size, (label, "a byte outside the fields was written")
        assert at == len(got)
        return {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", text)}


def test_every_case_through_the_emulated_bodies(lib, emulator, tmp_path):
    batch = Batch(tmp_path)
    for label, rec, offsets in pr.cases():
        for mis in offsets:
            batch.add(f"{label} dst%16={mis}", rec, DST + mis)
    counts = batch.run(emulator)
    assert batch.paths == {"head", "units", "tail"}, batch.paths
    assert counts["head_elements"] and counts["units"] and counts["tail_elements"], counts
    assert counts["table_loads"] and counts["outside"], counts
    assert counts["box_loads"] and counts["box_loads"] % 4 == 0, counts


def test_more_than_one_workgroup_through_the_emulated_bodies(lib, emulator, tmp_path):
    """The 300 x 300 letterboxes the GPU test packs with 66 workgroups and more."""
    batch = Batch(tmp_path)
    for label, rec in pr.many():
        batch.add(f"{label} dst%16=0", rec, DST)
    counts = batch.run(emulator)
    assert counts["grid"] >= 2 * 66 and counts["units"] >= 16875 + 33750, counts


def test_the_limit_of_the_contract_through_the_emulated_bodies(lib, emulator, tmp_path):
    """An output axis of 32768 steps whose image ends with it."""
    batch = Batch(tmp_path)
    for label, rec, offsets in pr.limit_cases():
        q = rec[0][3]["prep"]
        assert q["inner"][0] + q["lead"][0] == pr.LIMIT == rec[0][3]["size"][0], label
        for mis in offsets:
            batch.add(f"{label} dst%16={mis}", rec, DST + mis)
    counts = batch.run(emulator)
    assert counts["units"] >= 4 * (2 * pr.LIMIT // 16 - 1), counts


def test_the_emulation_notices_what_it_checks(emulator, tmp_path):
    """A table one word short is a table index at or past its words; a source reach one byte
    short is a source offset outside [lo, hi]; an image that overhangs the output, a table off its
    dword or along a resized axis are not launched; a tap read too many or too few is noticed."""
    np.arange(96, dtype=np.uint8).tofile(str(tmp_path / "src.bin"))
    np.array([1.0, 2.0, 3.0], np.float32).tofile(str(tmp_path / "tab.bin"))
    src, tab = str(tmp_path / "src.bin"), str(tmp_path / "tab.bin")
    one = f32_bits(1.0)

    def run(hi=95, channels=3, stab=FAKE + 4096, axis=2, inner=(2, 4), lead=(1, 2), size=96):
        spec = str(tmp_path / "spec.txt")
        with open(spec, "w") as f:  # a 4 x 8 x 3 uint8 frame -> 4 x 8 x 3 uint8, nearest
            f.write(f"1 {DST} {size}\n1 1 1 8 1 8 3 0 1 4 8 4 8 3 24 3 1 96 1 96 96 96 0 {hi} "
                    f"{FAKE} 0 0 {src} 0 0 -1 - 1 {stab} 0 {channels} {axis} 0 1 {one} {one} 1 "
                    f"{inner[0]} {inner[1]} {lead[0]} {lead[1]} {f32_bits(114.0)} {tab} -\n")
        r = subprocess.run([emulator, spec], capture_output=True, text=True)
        return r.returncode, r.stdout

    rc, text = run()  # 6 units; 2 x 4 x 3 elements inside, a tap each
    assert rc == 0 and text.startswith("ok cases=1 grid=1 loads=24 box_loads=0 "), text
    assert "units=6" in text and "outside=72" in text, text
    rc, text = run(hi=67)  # (the last tap is the last byte of element (2, 6, 2))
    assert rc == 1 and "source offset outside [lo, hi]" in text
    rc, text = run(channels=2)
    assert rc == 2 and "no model-input step" in text  # (the axis has three steps)
    rc, text = run(stab=FAKE + 4098)
    assert rc == 2 and "no model-input step" in text
    rc, text = run(axis=1)
    assert rc == 2 and "no model-input step" in text
    rc, text = run(inner=(2, 7))
    assert rc == 2 and "no model-input step" in text
    rc, text = run(size=95)
    assert rc == 2 and "does not fit" in text
