"""The body of gather_quant_kernel on the CPU (no GPU): csrc/testing/cast_emulate.cpp, a
stand-alone program built here with the host compiler under AddressSanitizer and UBSan, runs
cast_device.h lane by lane over the whole grid of device plans of dora_gpu_plan_tensor_convert
made over made-up pointers: the 16-element unit of an 8-bit destination with its source image of
16, 32 or 64 bytes, the 8-element unit of a 16-bit one, heads and tails of up to 15 elements.  It
fails on any source read outside the field's [lo, hi], any load that is not naturally aligned, any
output byte not written exactly once and any written at or past dst + total; the bytes it writes
are compared here with `tensor.from_numpy_quantize`, bit for bit.

Contiguous runs of 1, 3, 15, 16, 17, 31, 33 and 1024 elements (dense and cut from a wider base),
totals smaller than the head, destinations at every multiple of the destination element size mod
16 (heads of 0..15 for 8 bits), the 5 x 7 x 3 image permuted to 3 x 5 x 7 and the reverse, a
negative and a zero stride in dimension 0, d0 in 1, 63, 64, 65 and 257, all 28 pairs, a float32
source whose runs are 4- but not 16-aligned, and a record of a quantise float32 -> uint8, a plain
float32 field and a cast float32 -> float16.  The value sets (tests/quant_records.py) run dense
and cut from a wider base.

tests/test_gpu_tensor_quant_device.py runs the same cases on the GPU, each after it passed here."""
import subprocess

import numpy as np
import pytest

from dora_amd._lib import ARROW_DEVICE_ROCM
from tests import cast_records as cr
from tests import quant_records as qr
from tests import struct_records as sr
from tests.gather_views import misalignment
from tests.test_cast_index_host import DST, FAKE, POISON, emulator  # noqa: F401  (the fixture)


def spec_lines(rec, p, dst, addr, file_of):
    """The emulator's lines of device plan `p` of `rec` at `dst`, and [(offset, wanted array)]."""
    fields, ks = sr.plan_fields(p, dst), qr.plan_converts(p)
    assert len(fields) == len(ks) == len(rec)
    lines, ranges = [f"{len(rec)} {dst} {p.size}"], []
    for (_, b, v, c), d, k in zip(rec, fields, ks):
        assert d["gather"] and k["cast"] == (c is not None) and k["quant"] == qr.is_quant(c)
        off = d["src"] - addr[id(b)]
        assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes, d
        src = file_of(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
        scale_bits = int(np.float32(k["scale"]).view(np.uint32))
        head = [2, k["q_code"], k["zp"]] if k["quant"] else [int(k["cast"])]
        lines.append(" ".join(map(str, [
            *head, max(k["src_code"], 0), k["src_bits"], k["dst_bits"], int(k["has_scale"]),
            scale_bits, k["count"], d["elem"], d["row"], k["src_bytes"], d["bytes"], d["lo"],
            d["hi"], d["src"], d["off"], d["nd"], *d["shape"], *d["stride"], src])))
        ranges.append((d["off"], qr.want(v, c)))
        assert ranges[-1][1].nbytes == d["bytes"]
    return lines, ranges


class Batch:
    """Cases gathered into one spec file for one run of the emulator."""

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
        with qr.plan_convert(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM) as p:
            assert p.segments() == [], label
            lines, ranges = spec_lines(rec, p, dst, addr, self._file)
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
                qr.same(sample[off:off + want.nbytes], want, label)
                sample[off:off + want.nbytes] = bytes([POISON]) * want.nbytes
            assert bytes(sample) == bytes([POISON]) * size, (label, "a byte outside the fields was written")
        assert at == len(got)
        return text


@pytest.mark.parametrize("src,dst", qr.PAIRS)
def test_every_shape_of_every_pair(lib, emulator, tmp_path, src, dst):
    batch = Batch(tmp_path)
    for label, rec in qr.shape_cases(src, dst):
        for mis in qr.dst_offsets(dst):
            batch.add(f"{src}->{dst} {label} dst%16={mis}", rec, DST + mis)
    text = batch.run(emulator)
    vec = int(text.split(" vector_loads=")[1].split()[0])
    assert vec > 0, text


@pytest.mark.parametrize("dst", list(qr.DESTS))
def test_totals_smaller_than_the_head(lib, emulator, tmp_path, dst):
    mis, rec = qr.short_totals(dst)
    batch = Batch(tmp_path)
    batch.add(f"3 elements at {mis} mod 16", rec, DST + mis)
    batch.add("3 elements at 0 mod 16", rec, DST)
    text = batch.run(emulator)
    assert " vector_loads=0\n" in text, text  # (no whole unit: element by element)


def test_a_float32_run_off_16_takes_the_element_path(lib, emulator, tmp_path):
    b, v = qr.f32_run_off_16()
    batch = Batch(tmp_path)
    batch.add("run 4-aligned, not 16", [(None, b, v, qr.quant("float32", "uint8", 0.25, 128))], DST)
    text = batch.run(emulator)
    assert " loads=96 vector_loads=0\n" in text, text  # (6 rows of 16 elements, one load each)


def test_a_record_of_three_fields(lib, emulator, tmp_path):
    """A quantise float32 -> uint8, a plain float32 field and a cast float32 -> float16, at every
    even destination mod 16 (all the float16 field allows)."""
    batch = Batch(tmp_path)
    for d0 in (3, 9, 64):
        rec = qr.three_fields(d0)
        for mis in range(0, 16, 2):
            batch.add(f"three fields d0={d0} dst%16={mis}", rec, DST + mis)
            ranges = batch.want[-1][2]
            assert ranges[1][0] % 4 == 0 and ranges[2][0] % 2 == 0
    batch.run(emulator)


@pytest.mark.parametrize("k", range(qr.N_VALUE_SETS))
def test_the_value_sets(lib, emulator, tmp_path, k):
    """Every value set through the emulated body, dense and cut from a wider base: the
    plain-integer quantise gives numpy's bits, NaNs, infinities, ties and subnormals included."""
    label, x, qs = qr.value_sets()[k]
    b, v = cr.cut_from_wider(x)
    batch = Batch(tmp_path)
    for i, q in enumerate(qs):
        if i % 2 == 0:
            batch.add(label + qr.label_of(q), [(None, x, x, q)], DST)
        else:
            batch.add(label + qr.label_of(q) + ", cut from a wider base", [(None, b, v, q)], DST + 4)
    batch.run(emulator)


def test_the_emulation_notices_what_it_checks(emulator, tmp_path):
    """A reach one byte short is a source offset outside [lo, hi]; a source address off its
    element size is a load not naturally aligned; a sample one byte short does not fit; a zero
    point outside the destination's range is no quantise."""
    np.arange(32, dtype=np.float32).tofile(str(tmp_path / "src.bin"))
    src = str(tmp_path / "src.bin")

    def run(size, hi, addr=FAKE, zp=128):
        spec = str(tmp_path / "spec.txt")
        with open(spec, "w") as f:  # 32 float32 -> uint8, one dense row
            f.write(f"1 {DST} {size}\n2 1 {zp} 2 32 8 0 0 32 4 128 128 32 0 {hi} {addr} 0 0 {src}\n")
        r = subprocess.run([emulator, spec], capture_output=True, text=True)
        return r.returncode, r.stdout

    assert run(32, 127) == (0, "ok cases=1 grid=1 loads=8 vector_loads=8\n")
    rc, text = run(32, 126)
    assert rc == 1 and "source offset outside [lo, hi]" in text
    rc, text = run(32, 127, FAKE + 2)
    assert rc == 1 and "not naturally aligned" in text
    rc, text = run(31, 127)
    assert rc == 2 and "does not fit" in text
    rc, text = run(32, 127, zp=256)
    assert rc == 2 and "is no cast" in text
