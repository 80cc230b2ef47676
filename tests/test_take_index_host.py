"""The taken body of gather_struct_kernel on the CPU (no GPU): csrc/testing/gather_take_emulate.cpp,
a stand-alone program built here with the host compiler under AddressSanitizer and UBSan, runs
gather_device.h's take:: — output unit -> taken row and row inside it, the index word -> base or
missing, the odometer across taken rows, the three unit paths — lane by lane over the whole grid
of device take plans made over made-up pointers.  It fails on any index word read outside
[0, K), any source offset outside the field's [lo, hi], any source read while the row in hand is
missing, and any output byte not written exactly once or written at or past dst + total; the bytes
it writes are compared here with numpy: `values[index]`, zero rows where a word is no row.

Rows of 1, 2, 4, 12, 16, 20, 24 and 4096 bytes (dense and cut from a wider base), views whose
dimension 0 differs in kind (a positive, negative and zero stride, dimension 0 the contiguous one,
a misaligned source, a permuted image), K in 0, 1, 63, 64, 65, 257 and 1025 against N of 1 and 97,
both word widths, destinations 0, 3, 4, 8 and 12 mod 16, and for each the identity, the reversed
identity, one row repeated, random words with repeats and words mixed with -1, N, the type's
minimum and maximum and, for int64, 2^32 + 1 and -2^33; a record of three fields of different
row sizes behind a ragged batch's offsets, so that its fields start at 4 mod 16.

tests/test_gpu_tensor_take_device.py runs the same cases on the GPU, each after it passed here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from dora_amd._lib import ARROW_DEVICE_CPU, ARROW_DEVICE_ROCM, PARTITION_LENGTHS
from tests import gather_views as gv
from tests import struct_records as sr
from tests.gather_views import misalignment
from tests import take_records as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F10_0000_0000  # never dereferenced
INDEX = 0x7F30_0000_0000
DST = 0x7F50_0000_1000
POISON = 0xA5


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if not cxx:
        pytest.fail("no host C++ compiler to build the emulation with")
    exe = str(tmp_path_factory.mktemp("take_emulate") / "gather_take_emulate")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dora_amd", "csrc"),
           os.path.join(ROOT, "dora_amd", "csrc", "testing", "gather_take_emulate.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


class Batch:
    """Cases gathered into one spec file for one run of the emulator: each a device take plan of
    a record over made-up pointers, its index, and the bytes every field must come out as."""

    def __init__(self, tmp_path):
        self.dir, self.spec, self.want, self.files = tmp_path, [], [], 0

    def _file(self, data):
        name = str(self.dir / f"f{self.files}.bin")
        self.files += 1
        with open(name, "wb") as f:
            f.write(data)
        return name

    def add(self, label, rec, index, dst, part=None):
        """Plan the take of `rec` by `index` (with `part`: the ragged batch over it, lengths on
        the host) for a sample at `dst`; K == 0 plans an empty message and no case."""
        bases = sr.bases_of(rec)
        addr = {id(b): FAKE + (1 << 26) * i + misalignment(b) for i, b in enumerate(bases)}
        kw = {} if part is None else dict(part=part, form=PARTITION_LENGTHS, part_dev=ARROW_DEVICE_CPU)
        with tr.plan_take(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM, index, ARROW_DEVICE_ROCM,
                          index_ptr=INDEX, **kw) as p:
            ix = tr.plan_index(p)
            n = rec[0][2].shape[0]
            assert (ix["k"], ix["n"], ix["wide"]) == (len(index), n, index.dtype.itemsize == 8), label
            if len(index) == 0:
                assert p.segments() == [] and not ix["device"], label
                assert p.size == (0 if part is None else 4 * (len(part) + 1)), label
                return
            assert ix["device"] and ix["index"] == INDEX and p.segments() == [], label
            assert (ix["lo"], ix["hi"]) == (0, index.nbytes - 1), label
            fields = sr.plan_fields(p, dst)
            assert len(fields) == len(rec), label
            lines = [f"{len(rec)} {dst} {p.size} {len(index)} {n} {int(ix['wide'])} "
                     f"{self._file(index.tobytes())}"]
            ranges = []
            for k, ((_, b, v), d) in enumerate(zip(rec, fields)):
                assert d["gather"] and d["kind"] == -1, label
                assert d["bytes"] == len(index) * int(np.prod(v.shape[1:])) * v.itemsize, label
                off = d["src"] - addr[id(b)]
                # the reach covers every source row and stays inside the base
                assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes, (label, k, d)
                src = self._file(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
                lines.append(" ".join(map(str, [d["elem"], d["row"], d["bytes"], d["lo"], d["hi"],
                                                d["src"], d["off"], ix["stride0"][k], d["nd"],
                                                *d["shape"], *d["stride"], src])))
                ranges.append((d["off"], tr.taken(v, index).tobytes()))
                assert len(ranges[-1][1]) == d["bytes"], label
            self.spec.append("\n".join(lines))
            self.want.append((label, p.size, ranges))

    def run(self, emulator):
        if not self.spec:
            return ""
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
                have = bytes(sample[off:off + len(want)])
                assert have == want, (label, off, next(i for i in range(len(want)) if have[i] != want[i]))
                sample[off:off + len(want)] = bytes([POISON]) * len(want)
            assert bytes(sample) == bytes([POISON]) * size, (label, "a byte outside the fields was written")
        assert at == len(got)
        return text


def sweep(batch, name, b, v):
    for label, index, mis in tr.sweep(v):
        batch.add(f"{name} {label}", [(None, b, v)], index, DST + mis)


@pytest.mark.parametrize("dense", [False, True], ids=["cut", "dense"])
@pytest.mark.parametrize("n", [1, 97])
@pytest.mark.parametrize("row", tr.ROWS)
def test_rows_of_every_size(lib, emulator, tmp_path, row, n, dense):
    b, v = tr.rows_view(n, row, dense)
    batch = Batch(tmp_path)
    sweep(batch, f"row={row} N={n}", b, v)
    assert "index_loads=" in batch.run(emulator)


@pytest.mark.parametrize("name", tr.VIEWS)
def test_views_whose_dimension_0_differs_in_kind(lib, emulator, tmp_path, name):
    b, v = gv.make(name)
    batch = Batch(tmp_path)
    sweep(batch, name, b, v)
    batch.run(emulator)


def test_a_record_behind_an_offsets_buffer(lib, emulator, tmp_path):
    """Three fields of different row sizes, taken by one index, behind the 20 bytes of offsets of
    a ragged batch of 4 lists: with the sample on a 16-byte boundary the first field starts at
    4 mod 16; a float64 field is padded to 8 behind it."""
    rec, cases = tr.three_fields()
    batch = Batch(tmp_path)
    for label, index, lengths, mis in cases:
        batch.add(label, rec, index, DST + mis, part=lengths)
    assert batch.want[0][2][0][0] == 20  # the first leaf's offset in the sample
    batch.run(emulator)


def test_no_source_rows(lib, emulator, tmp_path):
    """N == 0 with K > 0: K zero rows, whatever the words, and no byte of any source is read."""
    b = np.zeros((0, 6), np.float32)
    batch = Batch(tmp_path)
    for wide in (0, 1):
        index = np.array([0, -1, 5, 1 << 20], np.int64 if wide else np.int32)
        batch.add(f"N=0 wide={wide}", [(None, b, b[:, :4])], index, DST + 4)
    assert " loads=0 " in batch.run(emulator)


def test_the_emulation_notices_what_it_checks(emulator, tmp_path):
    """A reach one byte short of the last source row is a source offset outside [lo, hi]; a
    sample one byte short is a write past its size; a missing index file is refused."""
    index = np.array([2, 0], np.int32)
    index.tofile(str(tmp_path / "ix.bin"))
    np.arange(48, dtype=np.uint8).tofile(str(tmp_path / "src.bin"))
    ix, src = str(tmp_path / "ix.bin"), str(tmp_path / "src.bin")

    def run(size, hi, index_file=ix):
        spec = str(tmp_path / "spec.txt")
        with open(spec, "w") as f:
            f.write(f"1 {DST} {size} 2 3 0 {index_file}\n1 16 32 0 {hi} {FAKE} 0 16 0 {src}\n")
        r = subprocess.run([emulator, spec], capture_output=True, text=True)
        return r.returncode, r.stdout

    assert run(32, 47) == (0, "ok cases=1 grid=1 loads=2 index_loads=2\n")
    rc, text = run(32, 46)
    assert rc == 1 and "source offset outside [lo, hi]" in text
    rc, text = run(31, 47)
    assert rc == 2 and "does not fit" in text
    rc, text = run(32, 47, str(tmp_path / "none.bin"))
    assert rc == 2 and "index file" in text
