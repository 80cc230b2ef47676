"""Seeded random Arrow arrays through both plans of an Arrow `send_output` and through
transform_kernel's body, on the CPU (no GPU).

* Reference plan (plan.cpp `walk`): `Plan.of(arr)` of the host array has the oracle's size and
  type info, and its segments, materialised here, give the oracle's bytes region by region with
  nothing written outside the regions.
* Compact plan (`walk_compact`): `Plan.of(arr, compact=True)` of the host array; its segment table
  is read through dora_gpu_test_plan_segment_op; the test places the copy segments and
  csrc/testing/transform_emulate.cpp — a stand-alone program built here under AddressSanitizer and
  UBSan — places the transform segments with transform_device.h's own table builder and body, for
  every block and every thread, over sources and a destination of exactly their sizes.  The result
  is `oracle.pack_ref.pack` of a deep copy with offset 0 at every level (tests/random_arrays.py).
* Limit cases: every op at 4095, 4096, 4097 and 2 * 4096 + 1 elements, every (bit offset,
  len mod 8) at 1-3 output bytes, 40 transform segments (two launches), three blocks before
  segments of one, and — synthetic segments, for the emulator only — offsets whose base is near
  INT32_MAX and 2^40 and sources and destinations at 1, 2 and 4 mod 8 (rebase's byte-wise branch).
* The generator's conditions, counted over the 300 seeds (DESIGN.md lists the counts).
"""
import ctypes
import subprocess
from collections import Counter
from ctypes import byref, c_uint32, c_uint64

import numpy as np
import pytest

from dora_amd import _lib
from dora_amd.arrow_utils import Plan
from tests import random_arrays as ra
from tests.test_scan_index_host import build

SEEDS = 300
OPS = {1: "bitshift", 2: "rebase32", 3: "rebase64"}


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build(tmp_path_factory, "transform_emulate")


def table(plan):
    """The plan's segments: (src, dst_off, len, op, aux, src_len)."""
    out = []
    for i, (src, off, n) in enumerate(plan.segments()):
        op, aux, src_len = c_uint32(), c_uint32(), c_uint64()
        _lib.call("dora_gpu_test_plan_segment_op", plan.handle, i, byref(op), byref(aux),
                  byref(src_len))
        out.append((src, off, n, op.value, aux.value, src_len.value))
    return out


def emulate(emulator, tmp_path, size, segs, dst_mis=0):
    """Run the emulator over `segs`: dicts of op, aux, dst_off, len, src_len, bytes (the readable
    source) and optionally src_mis.  Returns (destination bytes, the figures of its last line)."""
    spec, blob, out = (str(tmp_path / n) for n in ("spec.txt", "blob.bin", "out.bin"))
    lines, data = [f"{size} {dst_mis} {len(segs)}"], bytearray()
    for s in segs:
        lines.append(f"{s['op']} {s['aux']} {s['dst_off']} {s['len']} {s['src_len']} "
                     f"{s.get('src_mis', 0)} {len(data)}")
        data += s["bytes"]
    with open(spec, "w") as f:
        f.write("\n".join(lines) + "\n")
    with open(blob, "wb") as f:
        f.write(bytes(data))
    r = subprocess.run([emulator, spec, blob, out], capture_output=True, text=True)
    text = r.stdout + r.stderr[-3000:]
    assert r.returncode == 0 and text.startswith("ok"), text
    with open(out, "rb") as f:
        got = f.read()
    assert len(got) == size
    return got, {k: int(v) for k, v in (w.split("=") for w in r.stdout.split()[1:])}


def compact_on_host(emulator, tmp_path, arr, label):
    """The compact plan of a host array, placed: copies by this test, transforms by the emulator.
    Returns (buffer of size + SLACK, plan size, type info, the table, the emulator's figures)."""
    with Plan.of(arr, compact=True) as p:
        size, ti, segs = p.size, p.type_info(), table(p)
        buf = bytearray([ra.POISON]) * (size + ra.SLACK)
        written = np.zeros(size, np.uint8)
        xs = []
        for src, off, n, op, aux, src_len in segs:
            assert n > 0 and off + n <= size, (label, off, n, size)
            written[off:off + n] += 1
            if op == 0:
                buf[off:off + n] = ctypes.string_at(src, n)
            else:
                readable = src_len if op == 1 else n
                xs.append({"op": op, "aux": aux, "dst_off": off, "len": n, "src_len": src_len,
                           "bytes": ctypes.string_at(src, readable)})
        assert written.max(initial=0) <= 1, (label, "segments overlap")
        got, stats = emulate(emulator, tmp_path, size, xs)
    for s in xs:
        o, n = s["dst_off"], s["len"]
        buf[o:o + n] = got[o:o + n]
    return buf, size, ti, segs, stats


def check_compact(emulator, tmp_path, arr, label):
    want, info = ra.reference(arr, compact=True)
    buf, size, ti, segs, stats = compact_on_host(emulator, tmp_path, arr, label)
    assert size == len(want), (label, size, len(want))
    assert ra.mask_validity(ti) == ra.mask_validity(info), label
    ra.compare(buf, want, info, compact=True, label=label)
    return segs, stats


@pytest.fixture(scope="module")
def arrays():
    return [ra.array(seed) for seed in range(SEEDS)]


def test_reference_plan_of_every_seed(arrays):
    for seed, arr in enumerate(arrays):
        want, info = ra.reference(arr, compact=False)
        with Plan.of(arr) as p:
            assert p.size == len(want), seed
            assert p.type_info().to_json() == info.to_json(), seed
            buf = bytearray([ra.POISON]) * (p.size + ra.SLACK)
            for src, off, n, op, aux, src_len in table(p):
                assert op == 0 and off + n <= p.size, seed
                buf[off:off + n] = ctypes.string_at(src, n)
        ra.compare(buf, want, info, compact=False, label=seed)


def test_compact_plan_of_every_seed_through_the_emulator(emulator, tmp_path, arrays):
    """All 300 seeds, none left out, and the conditions the compact plans decide: each op on at
    least 20 seeds, each bit offset 1-7 at least 5 times, at least 10 seeds with a transform
    segment of two or more blocks."""
    c, done = Counter(), 0
    for seed, arr in enumerate(arrays):
        segs, stats = check_compact(emulator, tmp_path, arr, seed)
        ops = {op for *_, op, aux, src_len in segs if op}
        for op in ops:
            c[OPS[op]] += 1
        for *_, op, aux, src_len in segs:
            if op == 1:
                c[f"bit offset {aux}"] += 1
        c["two or more blocks"] += stats["later_blocks"] > 0
        c["a later segment after one of two or more blocks"] += stats["after_long"] > 0
        done += 1
    print(sorted(c.items()))
    assert done == SEEDS
    for op in OPS.values():
        assert c[op] >= 20, (op, c)
    for b in range(1, 8):
        assert c[f"bit offset {b}"] >= 5, (b, c)
    assert c["two or more blocks"] >= 10, c
    assert c["a later segment after one of two or more blocks"] >= 5, c


def test_conditions_of_the_generator(arrays):
    """At least 20 seeds of 300 each: a top-level offset, a child with an offset of its own, an
    empty result, a dictionary whose values are a slice, a list inside a list, validity kept,
    validity present but dropped — and no nulls at all, and a node that is all null.  Every class
    of layout_of occurs."""
    c, fmts = Counter(), set()
    for arr in arrays:
        for k, v in ra.facts(arr).items():
            c[k] += bool(v)
        fmts |= {x["fmt"].split(",")[0] if x["fmt"].startswith("d:") else x["fmt"]
                 for x in ra.nodes(arr)}
        fmts |= {"d256" for x in ra.nodes(arr) if x["fmt"].endswith(",256")}
        c["at most 64 elements"] += len(arr) <= ra.SMALL
    print(sorted(c.items()))
    for k in ("top_offset", "child_offset", "empty", "dict_sliced_values", "list_in_list",
              "validity_kept", "validity_dropped", "no_nulls", "all_null"):
        assert c[k] >= 20, (k, c)
    assert c["at most 64 elements"] >= SEEDS * 0.85 and SEEDS - c["at most 64 elements"] >= 20
    want = {"n", "b", "c", "s", "i", "l", "d:38", "d256", "tin", "w:0", "w:3", "u", "z", "U", "Z",
            "+l", "+L", "+m", "+w:1", "+s"}
    assert want <= fmts, want - fmts


LIMITS = ra.limit_arrays()


@pytest.mark.parametrize("k", range(len(LIMITS)), ids=[l for l, _ in LIMITS])
def test_limit_arrays_through_the_emulator(emulator, tmp_path, k):
    label, arr = LIMITS[k]
    segs, stats = check_compact(emulator, tmp_path, arr, label)
    nx = sum(1 for s in segs if s[3])
    if label.startswith(("bitshift", "rebase")):
        e = int(label.split()[1])
        op = {"bitshift": 1, "rebase32": 2, "rebase64": 3}[label.split()[0]]
        mine = [s for s in segs if s[3] == op]
        assert len(mine) == 1 and mine[0][2] == e * {1: 1, 2: 4, 3: 8}[op], (label, mine)
        assert stats["blocks"] == (e + ra.X_ELEMS - 1) // ra.X_ELEMS
    elif label.startswith("bit offsets"):
        assert sorted(s[4] for s in segs if s[3] == 1) == list(range(8)), label
    elif label.startswith("40"):
        assert nx == 40 and stats["launches"] == 2, (nx, stats)
    else:
        assert [s[3] for s in segs if s[3]] == [2, 2, 1] and stats["blocks"] == 5, stats
        assert stats["later_blocks"] == 2 and stats["after_long"] == 1, stats


@pytest.mark.parametrize("base", [(1 << 31) - 1 - 70000, (1 << 40) - 3, (1 << 62) + 5])
@pytest.mark.parametrize("count", [1, 257, 4097])
def test_offsets_with_a_large_base(emulator, tmp_path, base, count):
    """The transform never reads the values: offsets that start near INT32_MAX (int32) and near
    2^40 and 2^62 (int64) come out minus the first, with no signed overflow on the way."""
    rng = np.random.default_rng(count)
    steps = np.concatenate([[0], np.cumsum(rng.integers(0, 17, count - 1))])
    segs, want = [], bytearray()
    for op, dt in ((2, np.int32), (3, np.int64)):
        if base + int(steps[-1]) > np.iinfo(dt).max:
            continue
        off = (base + steps).astype(dt)
        want += b"\xa5" * (-len(want) % 8)
        segs.append({"op": op, "aux": 0, "dst_off": len(want), "len": off.nbytes, "src_len": 0,
                     "bytes": off.tobytes()})
        want += steps.astype(dt).tobytes()
    assert segs
    got, _ = emulate(emulator, tmp_path, len(want), segs)
    assert got == bytes(want)


@pytest.mark.parametrize("wide", [0, 1], ids=["int32", "int64"])
@pytest.mark.parametrize("src_mis, dst_mis", [(1, 0), (0, 1), (2, 2), (4, 4), (4, 0), (0, 4),
                                              (1, 2), (8, 8), (0, 0)])
def test_rebase_at_odd_addresses(emulator, tmp_path, wide, src_mis, dst_mis):
    """rebase's byte-wise branch: source or destination off a multiple of the word — every offset
    moves through ldu / stu (`pieces`), none through a whole-word access that UBSan would stop —
    and the whole-word branch wherever both allow it (4 mod 8 is aligned for int32)."""
    dt, w = (np.int64, 8) if wide else (np.int32, 4)
    count = 4097
    steps = np.concatenate([[0], np.cumsum(np.random.default_rng(7).integers(0, 9, count - 1))])
    off = (1000 + steps).astype(dt)
    seg = {"op": 3 if wide else 2, "aux": 0, "dst_off": 0, "len": off.nbytes, "src_len": 0,
           "src_mis": src_mis, "bytes": off.tobytes()}
    got, stats = emulate(emulator, tmp_path, off.nbytes, [seg], dst_mis=dst_mis)
    assert got == steps.astype(dt).tobytes()
    aligned = (src_mis | dst_mis) % w == 0
    assert (stats["words"], stats["pieces"]) == ((count, 0) if aligned else (0, count)), stats


def test_the_emulation_notices_what_it_checks(emulator, tmp_path):
    """A bitmap slice of exactly its source bytes comes out shifted, the byte past the source
    read as zero; transform segments that share a byte are refused."""
    src = bytes(range(1, 4))
    seg = {"op": 1, "aux": 3, "dst_off": 0, "len": 3, "src_len": 3, "bytes": src}
    got, _ = emulate(emulator, tmp_path, 3, [seg])
    bits = np.unpackbits(np.frombuffer(src + b"\0", np.uint8), bitorder="little")[3:27]
    assert got == np.packbits(bits, bitorder="little").tobytes()
    with pytest.raises(AssertionError, match="overlap"):
        emulate(emulator, tmp_path, 5, [seg, dict(seg, dst_off=2)])
