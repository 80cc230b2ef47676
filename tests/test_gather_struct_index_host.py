"""gather_struct_kernel's address arithmetic on the CPU (no GPU):
csrc/testing/gather_struct_emulate.cpp, a stand-alone program built here with the host compiler
under AddressSanitizer and UBSan, runs multi::make_args, the workgroup-to-field lookup and each
field's own body (csrc/gather_device.h) for every workgroup and thread of the grid, over the
descriptors dora_gpu_plan_tensor_struct gives for the records the GPU test uses
(tests/struct_records.py).  It fails unless every source offset of a field lies in that field's
[lo, hi], every LDS index lies inside the tile, every byte of every field's range is written
exactly once and no padding byte or byte at or past the size is written; the bytes it writes are
compared here with the oracle's regions (numpy's row-major copies).  Each record runs with the
library's selection and with the rows body forced, at destinations 0, 3 and 8 mod 16."""
import os
import shutil
import subprocess

import pytest

from dora_amd import _lib
from dora_amd._lib import ARROW_DEVICE_ROCM
from tests import struct_records as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x7F12_3456_0000  # made-up device addresses, 16-byte aligned: planning never reads them
DSTS = (0x7F00_0000_1000, 0x7F00_0000_1003, 0x7F00_0000_2008)
POISON = 0xA5


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or shutil.which("hipcc")
    if not cxx:
        pytest.fail("no host C++ compiler to build the gather emulation with")
    exe = str(tmp_path_factory.mktemp("gather_struct") / "gather_struct_emulate")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dora_amd", "csrc"),
           os.path.join(ROOT, "dora_amd", "csrc", "testing", "gather_struct_emulate.cpp"), "-o", exe]
    subprocess.run(cmd, check=True)
    return exe


def write_spec(path, fields, dst, size, files):
    words = [len(fields), dst, size]
    for d, f in zip(fields, files):
        words += [d["kind"], d["elem"], d["row"], d["bytes"], d["lo"], d["hi"], d["src"], d["off"],
                  d["nd"], *d["shape"], *d["stride"], f]
    with open(path, "w") as fh:
        fh.write(" ".join(str(w) for w in words) + "\n")


def run(exe, spec, out=None):
    r = subprocess.run([exe, spec] + ([out] if out else []), capture_output=True, text=True)
    return r.returncode, r.stdout + r.stderr[-2000:]


def planned(rec):
    bases = sr.bases_of(rec)
    addr = {id(b): FAKE + (1 << 24) * i for i, b in enumerate(bases)}
    return sr.plan_record(rec, lambda b: addr[id(b)], ARROW_DEVICE_ROCM), addr


@pytest.mark.parametrize("mode", [0, 1], ids=["selected", "rows"])
@pytest.mark.parametrize("name", list(sr.RECORDS))
def test_emulated_grid(lib, emulator, tmp_path, name, mode):
    rec = sr.RECORDS[name]()
    sample, info, ranges = sr.oracle(rec)
    p, addr = planned(rec)
    kinds = set()
    with p:
        assert p.size == len(sample)
        try:
            _lib.call("dora_gpu_test_gather_kernel", mode)
            for dst in DSTS:
                fields = sr.plan_fields(p, dst)
                assert all(d["gather"] for d in fields)
                assert [(d["off"], d["bytes"]) for d in fields] == ranges
                files = []
                for k, ((_, b, _), d) in enumerate(zip(rec, fields)):
                    off = d["src"] - addr[id(b)]
                    assert 0 <= off + d["lo"] and off + d["hi"] < b.nbytes
                    files.append(str(tmp_path / f"src{k}.bin"))
                    with open(files[-1], "wb") as f:
                        f.write(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
                spec, out = str(tmp_path / "spec.txt"), str(tmp_path / "out.bin")
                write_spec(spec, fields, dst, p.size, files)
                rc, text = run(emulator, spec, out)
                assert rc == 0 and text.startswith("ok"), (name, hex(dst), text)
                with open(out, "rb") as f:
                    got = f.read()
                assert len(got) == len(sample)
                pad = bytearray(got)
                for off, ln in ranges:
                    assert got[off:off + ln] == sample[off:off + ln], (name, hex(dst), off)
                    pad[off:off + ln] = bytes([POISON]) * ln
                assert bytes(pad) == bytes([POISON]) * len(got), (name, hex(dst))
                kinds |= {d["kind"] >= 0 for d in fields}
        finally:
            _lib.call("dora_gpu_test_gather_kernel", 0)
    if mode == 1:
        assert kinds == {False}
    elif name == "tile_selected":
        assert kinds == {False, True}  # both bodies in one launch, by the library's own choice


def test_tile_forced_where_it_applies(lib, emulator, tmp_path):
    """The permuted field through the tile body (forced: the selection prefers rows for its
    160-byte output rows) next to a rows field, partial tiles on every edge."""
    rec = sr.RECORDS["permuted_and_bytes"]()
    sample, info, ranges = sr.oracle(rec)
    p, addr = planned(rec)
    with p:
        for dst in DSTS:
            try:
                _lib.call("dora_gpu_test_gather_kernel", 2)
                fields = sr.plan_fields(p, dst)
            finally:
                _lib.call("dora_gpu_test_gather_kernel", 0)
            # a destination that is not element-aligned is never tiled
            assert [d["kind"] >= 0 for d in fields] == [dst % 4 == 0, False]
            files = []
            for k, ((_, b, _), d) in enumerate(zip(rec, fields)):
                off = d["src"] - addr[id(b)]
                files.append(str(tmp_path / f"src{k}.bin"))
                with open(files[-1], "wb") as f:
                    f.write(b.tobytes()[off + d["lo"]: off + d["hi"] + 1])
            spec, out = str(tmp_path / "spec.txt"), str(tmp_path / "out.bin")
            write_spec(spec, fields, dst, p.size, files)
            rc, text = run(emulator, spec, out)
            # (the view's 33 x 40 merge into 1320: a 67 x 1320 plane, 3 x 42 tiles, the last of
            # each row and column partial)
            assert rc == 0 and text.startswith("ok"), text
            assert ("tiles=126" if dst % 4 == 0 else "tiles=0") in text, text
            with open(out, "rb") as f:
                got = f.read()
            for off, ln in ranges:
                assert got[off:off + ln] == sample[off:off + ln]


def test_the_emulation_notices_what_it_checks(lib, emulator, tmp_path):
    """The checks bite: a reach cut by one byte at either end fails the same run, and a layout
    whose fields overlap or leave the sample is not run at all."""
    rec = sr.detector(67, cls=True)
    p, addr = planned(rec)
    with p:
        fields = sr.plan_fields(p, DSTS[0])
        size = p.size
    spec = str(tmp_path / "spec.txt")
    nofiles = ["-"] * len(fields)
    write_spec(spec, fields, DSTS[0], size, nofiles)
    assert run(emulator, spec)[0] == 0
    for k, key, delta in [(0, "hi", -1), (1, "hi", -1), (3, "lo", 1)]:
        cut = [dict(d) for d in fields]
        cut[k][key] += delta
        write_spec(spec, cut, DSTS[0], size, nofiles)
        rc, text = run(emulator, spec)
        assert rc == 1 and text.startswith(f"FAIL field {k}: source offset"), text
    # a field pushed into its neighbour, and a sample one byte short of the last field's end
    moved = [dict(d) for d in fields]
    moved[1]["off"] += 3
    write_spec(spec, moved, DSTS[0], size, nofiles)
    rc, text = run(emulator, spec)
    assert rc == 1 and "fields overlap" in text, text
    write_spec(spec, fields, DSTS[0], size - 1, nofiles)
    rc, text = run(emulator, spec)
    assert rc == 2 and "does not fit the sample" in text, text
