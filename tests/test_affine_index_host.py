"""The body of gather_affine_kernel on the CPU (no GPU): csrc/testing/cast_emulate.cpp, the
stand-alone program built with the host compiler under AddressSanitizer and UBSan, runs
cast_device.h's body with the affine step lane by lane over the whole grid of device plans of
dora_gpu_plan_tensor_affine made over made-up pointers.  Besides what it checks of every cast plan
(reads inside [lo, hi], natural alignment, every output byte written once and none outside the
fields) it fails on a table index outside [0, C) and on a misaligned table load; the bytes it
writes are compared here with `tensor.from_numpy_cast` / `tensor.from_numpy_quantize`, bit for bit.

The shapes are those where the channel stepping can go wrong and nothing larger
(tests/affine_records.py): C in 1, 3, 4, 5 and 17; the axis innermost (inner = 1: a unit wraps C
several times) and outermost with inner in 3, 7, 16, 17 and 35 (units that cross one, several or
no channel boundary); a middle axis of a 4-D tensor; the 5 x 7 x 3 image permuted to 3 x 5 x 7 with
axis 0 and as it lies with axis -1; dense and cut from a wider base; a negative and a zero stride
in dimension 0; totals smaller than the head; destinations at every multiple of the destination
element size mod 16; tables at 4 mod 16; scale table only, bias table only, both, a table with a
scalar; and one record that mixes an affine cast, an affine quantise, a plain field and a scalar
cast.

tests/test_gpu_tensor_affine_device.py runs the same cases on the GPU, each after it passed here."""
import subprocess

import numpy as np
import pytest

from dora_amd._lib import ARROW_DEVICE_ROCM
from tests import affine_records as ar
from tests import quant_records as qr
from tests import struct_records as sr
from tests.gather_views import misalignment
from tests.test_cast_index_host import DST, FAKE, POISON, emulator  # noqa: F401  (the fixture)

TABLES = FAKE + (1 << 40)  # made-up table addresses, each 4 mod 16


def spec_lines(rec, p, dst, addr, taddr, file_of):
    """The emulator's lines of device plan `p` of `rec` at `dst`, and [(offset, wanted array)]."""
    fields, ks, afs = sr.plan_fields(p, dst), qr.plan_converts(p), ar.plan_affines(p, len(rec))
    assert len(fields) == len(ks) == len(rec)
    lines, ranges = [f"{len(rec)} {dst} {p.size}"], []
    for (_, b, v, c, a), d, k, f in zip(rec, fields, ks, afs):
        assert d["gather"] and k["cast"] == (c is not None) and k["quant"] == qr.is_quant(c)
        assert f["affine"] == (a is not None)
        off = d["src"] - addr[id(b)]
        assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes, d
        src = file_of(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
        scale_bits = int(np.float32(k["scale"]).view(np.uint32))
        head = [2, k["q_code"], k["zp"]] if k["quant"] else [int(k["cast"])]
        if a is not None:
            for name in ("scale", "bias"):
                assert f[name] == (taddr[id(a[name])] if a[name] is not None else 0)
            if a["scale"] is not None or a["bias"] is not None:
                axis = a["axis"] % v.ndim
                assert f["channels"] == v.shape[axis]
                assert f["inner"] == int(np.prod(v.shape[axis + 1:], dtype=np.int64))
                assert (f["lo"], f["hi"]) == (0, 4 * v.shape[axis] - 1)
            files = [file_of(a[n].tobytes()) if a[n] is not None else "-" for n in ("scale", "bias")]
            head = [3, head[0], max(f["inner"], 1), max(f["channels"], 1), int(f["has_bias"]),
                    int(np.float32(f["bias_value"]).view(np.uint32)), f["scale"], f["bias"],
                    *files, *head[1:]]
        lines.append(" ".join(map(str, [
            *head, max(k["src_code"], 0), k["src_bits"], k["dst_bits"], int(k["has_scale"]),
            scale_bits, k["count"], d["elem"], d["row"], k["src_bytes"], d["bytes"], d["lo"],
            d["hi"], d["src"], d["off"], d["nd"], *d["shape"], *d["stride"], src])))
        ranges.append((d["off"], ar.want(v, c, a)))
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
        bases = sr.bases_of([r[:3] for r in rec])
        addr = {id(b): FAKE + (1 << 26) * i + misalignment(b) for i, b in enumerate(bases)}
        taddr = {id(t): TABLES + 256 * i + 4 for i, t in enumerate(ar.tables_of(rec))}
        with ar.plan_affine(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM,
                            lambda t: taddr[id(t)]) as p:
            assert p.segments() == [], label
            lines, ranges = spec_lines(rec, p, dst, addr, taddr, self._file)
            self.spec.append("\n".join(lines))
            self.want.append((label, p.size, ranges))

    def run(self, emulator):
        spec, out = str(self.dir / "spec.txt"), str(self.dir / "out.bin")
        with open(spec, "w") as f:
            f.write("\n".join(self.spec) + "\n")
        r = subprocess.run([emulator, spec, out], capture_output=True, text=True)
        text = r.stdout + r.stderr[-3000:]
        assert r.returncode == 0 and text.startswith(f"ok cases={len(self.want)} "), text
        assert f"\naffine cases={len(self.want)} table_loads=" in text, text
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
        return text


@pytest.mark.parametrize("conv", ar.CONVS, ids=ar.conv_label)
def test_every_shape_at_every_destination(lib, emulator, tmp_path, conv):
    batch = Batch(tmp_path)
    for label, rec in ar.shape_cases(conv):
        for mis in ar.dst_offsets(conv):
            batch.add(f"{ar.conv_label(conv)} {label} dst%16={mis}", rec, DST + mis)
    batch.run(emulator)


@pytest.mark.parametrize("conv", ar.CONVS, ids=ar.conv_label)
def test_tables_and_scalars_in_every_combination(lib, emulator, tmp_path, conv):
    batch = Batch(tmp_path)
    for label, rec in ar.mode_cases(conv):
        for mis in (0, 4, 12):
            batch.add(f"{ar.conv_label(conv)} {label} dst%16={mis}", rec, DST + mis)
    batch.run(emulator)


@pytest.mark.parametrize("conv", ar.CONVS, ids=ar.conv_label)
def test_totals_smaller_than_the_head(lib, emulator, tmp_path, conv):
    mis, rec = ar.short_totals(conv)
    batch = Batch(tmp_path)
    batch.add(f"3 elements at {mis} mod 16", rec, DST + mis)
    batch.add("3 elements at 0 mod 16", rec, DST)
    text = batch.run(emulator)
    assert " vector_loads=0\n" in text, text  # (no whole unit: element by element)


def test_a_record_mixes_affine_and_plain_conversions(lib, emulator, tmp_path):
    batch = Batch(tmp_path)
    for d0 in (3, 9, 64):
        for mis in range(0, 16, 2):
            batch.add(f"mixed record d0={d0} dst%16={mis}", ar.mixed_record(d0), DST + mis)
    batch.run(emulator)


def test_the_emulation_notices_a_bad_table_load(emulator, tmp_path):
    """A table address off a multiple of 4 is a misaligned table load.  (An index outside [0, C)
    cannot be provoked from a spec: the stepping wraps at C, which is what the check holds.)"""
    np.arange(32, dtype=np.float32).tofile(str(tmp_path / "src.bin"))
    np.arange(4, dtype=np.float32).tofile(str(tmp_path / "tab.bin"))
    src, tab = str(tmp_path / "src.bin"), str(tmp_path / "tab.bin")

    def run(taddr, channels=4):
        spec = str(tmp_path / "spec.txt")
        with open(spec, "w") as f:  # 32 float32 -> float16 as 8 x 4, axis 1: inner 1, C 4
            f.write(f"1 {DST} 64\n3 1 1 {channels} 0 0 {taddr} 0 {tab} - "
                    f"2 32 16 0 0 32 4 128 128 64 0 127 {FAKE} 0 0 {src}\n")
        r = subprocess.run([emulator, spec], capture_output=True, text=True)
        return r.returncode, r.stdout

    rc, text = run(TABLES + 4)
    assert rc == 0 and "affine cases=1 table_loads=32" in text, text
    rc, text = run(TABLES + 6)
    assert rc == 1 and "table load not naturally aligned" in text, text
