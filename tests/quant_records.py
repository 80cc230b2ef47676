"""Quantise records for the tensor-quantise tests (dora_gpu_plan_tensor_convert), shared by the CPU
plan test, the sanitized host emulation of the cast body and the GPU tests.  A record is
tests/cast_records.py's list of (field name or None, base array, view of that base, conversion or
None); a conversion is a cast of that module or a quantise, a dict {"src": source dtype name,
"dst": "uint8" | "int8" | "uint16" | "int16", "scale": float or None, "zp": int}.  bfloat16
sources are held as their bits in uint16 arrays.  `want` is the statement of record,
`tensor.from_numpy_quantize`; `same` compares with it bit for bit, nothing exempt."""
import functools
from ctypes import byref, c_int, c_void_p

import numpy as np

from tests import cast_records as cr

SOURCES = cr.SOURCES
# destination dtype name -> (numpy dtype, DLPack type code)
DESTS = {"uint8": (np.uint8, 1), "int8": (np.int8, 0), "uint16": (np.uint16, 1),
         "int16": (np.int16, 0)}
PAIRS = [(s, d) for s in SOURCES for d in DESTS]
assert len(PAIRS) == 28


def quant(src, dst, scale=None, zp=0):
    return {"src": src, "dst": dst, "scale": scale, "zp": zp}


def is_quant(c):
    return c is not None and "zp" in c


def zero_points(dst):
    """0, lo and hi of `dst`; 128 for uint8 and -7 for the signed ones."""
    info = np.iinfo(DESTS[dst][0])
    extra = {"uint8": [128], "int8": [-7], "int16": [-7], "uint16": []}[dst]
    return sorted({0, int(info.min), int(info.max), *extra})


def want(view, c):
    """The statement of record for `view` under conversion `c` (a cast: cast_records.want)."""
    if not is_quant(c):
        return cr.want(view, c)
    from dora_amd import tensor
    view = np.asarray(view)
    arr = tensor.from_numpy_quantize(view, c["dst"], c["scale"], c["zp"],
                                     bfloat16=c["src"] == "bfloat16")
    import pyarrow as pa
    while isinstance(arr, pa.FixedSizeListArray):
        arr = arr.flatten()
    out = arr.to_numpy(zero_copy_only=False).reshape(view.shape)
    assert out.dtype == np.dtype(DESTS[c["dst"]][0])
    return out


def same(got, expect, what=""):
    """`got` (bytes) equals array `expect` bit for bit; a float field of a mixed record NaN for
    NaN, as cast_records.same."""
    expect = np.ascontiguousarray(expect)
    if expect.dtype.kind == "f":
        return cr.same(got, expect, what)
    assert len(got) == expect.nbytes, (what, len(got), expect.nbytes)
    if bytes(got) != expect.tobytes():
        g = np.frombuffer(bytes(got), expect.dtype).reshape(-1)
        bad = np.flatnonzero(g != expect.reshape(-1))
        raise AssertionError((what, "element", int(bad[0]), "got", int(g[bad[0]]), "want",
                              int(expect.reshape(-1)[bad[0]]), "of", len(bad), "wrong"))


def describe(rec, ptr_of):
    """(fields, casts, quants, n, keepalive) of `rec` over `ptr_of`: cast_records.describe with the
    quantised fields' sources described as cast sources and their entries in `quants`."""
    from dora_amd._lib import TensorQuant
    as_cast = [(n, b, v, (cr.cast(c["src"], "float32") if is_quant(c) else c)) for n, b, v, c in rec]
    fields, casts, n, keep = cr.describe(as_cast, ptr_of)
    quants = (TensorQuant * len(rec))()
    for k, (_, _, _, c) in enumerate(rec):
        if not is_quant(c):
            continue
        casts[k].dtype_code = casts[k].dtype_bits = casts[k].has_scale = 0
        casts[k].scale = 0.0
        quants[k].dtype_code = DESTS[c["dst"]][1]
        quants[k].dtype_bits = np.dtype(DESTS[c["dst"]][0]).itemsize * 8
        quants[k].has_scale = 0 if c["scale"] is None else 1
        quants[k].scale = 0.0 if c["scale"] is None else c["scale"]
        quants[k].zero_point = c["zp"]
    return fields, casts, quants, n, keep


def plan_convert(rec, ptr_of, dev):
    """Plan `rec` with dora_gpu_plan_tensor_convert; the Plan keeps the ctypes."""
    from dora_amd import _lib
    from dora_amd.arrow_utils import Plan
    fields, casts, quants, n, keep = describe(rec, ptr_of)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_convert", fields, n, casts, quants, dev, byref(h))
    return Plan(h.value, (fields, casts, quants, keep))


def plan_converts(plan):
    """cast_records.plan_casts with what dora_gpu_test_plan_quant adds per field."""
    from dora_amd import _lib
    out = cr.plan_casts(plan)
    for i, k in enumerate(out):
        on, code, bits, zp = c_int(), c_int(), c_int(), c_int()
        _lib.call("dora_gpu_test_plan_quant", plan.handle, i, byref(on), byref(code), byref(bits),
                  byref(zp))
        k.update(quant=bool(on.value), q_code=code.value, q_bits=bits.value, zp=zp.value)
    return out


def oracle(rec):
    """cast_records.oracle over this module's `want`."""
    import pyarrow as pa
    from dora_amd import tensor
    from oracle.pack_ref import pack
    cols = [tensor.from_numpy(want(v, c)) for _, _, v, c in rec]
    bare = len(rec) == 1 and rec[0][0] is None
    arr = cols[0] if bare else pa.StructArray.from_arrays(cols, names=[r[0] for r in rec])
    sample, info = pack(arr)
    ranges = []
    for c in ([info] if bare else info.child_data):
        while c.child_data:
            c = c.child_data[0]
        ranges.append((c.buffer_offsets[0].offset, c.buffer_offsets[0].len))
    return sample, info, ranges


# ---------------------------------------------------------------------------------------------
# Value sets
# ---------------------------------------------------------------------------------------------
INT_SCALES = (None, 0.5, 1 / 3, -1.0, 255.0)
FLOAT_SCALES = (1.0, 255.0, 1 / 256, 0.5, 3.0, -1.0, 0.0, -0.0)


def _neighbours(x):
    x = np.asarray(x, np.float32)
    inf = np.float32(np.inf)
    return np.concatenate([x, np.nextafter(x, -inf), np.nextafter(x, inf)])


@functools.lru_cache(maxsize=None)
def f32_inputs():
    """The float32 edge values: k + 0.5 and its two neighbours for every integer k in
    [-300, 300] and around +-32767, +-32768 and 65535; lo - 0.5 and hi + 0.5 with their neighbours
    for all four destinations; +-2^24, +-2^31 and one ulp either side, +-3e9, +-1e30, +-inf; quiet,
    signalling and negative NaNs; +-0 and subnormals; 0.49999997; and k / 255 for every k in
    [0, 255] and its neighbours, whose product with 255 is rounded before it is a tie or not."""
    ks = list(range(-300, 301)) + [s * m + d for s in (1, -1) for m in (32767, 32768)
                                   for d in (-1, 0)] + [65534, 65535]
    ties = _neighbours(np.array(ks, np.float64) + 0.5)
    edges = []
    for dt, _ in DESTS.values():
        info = np.iinfo(dt)
        edges += [info.min - 0.5, info.max + 0.5, info.min, info.max]
    edges = _neighbours(np.array(edges, np.float64))
    big = _neighbours(np.array([2.0 ** 24, -2.0 ** 24, 2.0 ** 31, -2.0 ** 31], np.float64))
    named = np.array([3e9, -3e9, 1e30, -1e30, np.inf, -np.inf, 0.49999997, -0.49999997, 0.5, -0.5,
                      1.5, 2.5, 254.5, 255.5, -128.5], np.float32)
    bits = np.array([0x7fc00000, 0x7f800001, 0xffc00000, 0xff800001, 0x7fffffff, 0xffffffff,
                     0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x807fffff,
                     0x00800000, 0x80800000], np.uint32).view(np.float32)
    frac = _neighbours(np.arange(256, dtype=np.float64) / 255)
    thirds = _neighbours((np.arange(-40, 41, dtype=np.float64) + 0.5) / 3)
    return np.concatenate([ties, edges, big, named, bits, frac, thirds]).astype(np.float32)


F32_SCALES = (None, 255.0, 1000.0, 3.0, -1.0, 1 / 256, 0.0, -0.0)
# len(value_sets()), for parametrising without computing them at collection time
N_VALUE_SETS = 4 * 4 + 2 * 4 + 4


@functools.lru_cache(maxsize=None)
def value_sets():
    """[(label, 1-D source array, [quantise ..])]: one entry per (source, destination), the source
    array all its patterns (float32: f32_inputs) and the quantises every scale with the
    destination's zero points dealt round them, so that every scale and every zero point occurs.
    The callers run every quantise of an entry over its array and leave the arrays as they are."""
    out = []
    for src in SOURCES:
        if src == "float32":
            x, scales = f32_inputs(), F32_SCALES
        else:
            x = cr.all_patterns(src)
            scales = FLOAT_SCALES if src in ("float16", "bfloat16") else INT_SCALES
        for dst in DESTS:
            zps = zero_points(dst)
            qs = [quant(src, dst, s, zps[i % len(zps)]) for i, s in enumerate(scales)]
            # every zero point under the first scales too, lo and hi included
            qs += [quant(src, dst, scales[1], z) for z in zps] + [quant(src, dst, None, z) for z in zps]
            out.append((f"{src}->{dst}", x, qs))
    assert len(out) == N_VALUE_SETS
    return out


def label_of(c):
    return f"*{c['scale']!r}+{c['zp']}"


# ---------------------------------------------------------------------------------------------
# Shapes: the smallest at which the 16-element unit can go wrong.
# ---------------------------------------------------------------------------------------------
RUNS = (1, 3, 15, 16, 17, 31, 33, 1024)
D0 = cr.D0


def dst_offsets(dst):
    """Every multiple of the destination element size mod 16."""
    return range(0, 16, np.dtype(DESTS[dst][0]).itemsize)


def hwc_view(src):
    """The 3 x 5 x 7 planes permuted to 5 x 7 x 3: CHW -> HWC, the reverse of cr.image_view."""
    b = cr.source(src, (3, 5, 7), seed=11)
    return b, b.transpose(1, 2, 0)


def f32_run_off_16():
    """A float32 source whose contiguous runs are 4-aligned but never 16-aligned: rows of 16
    elements cut from rows of 20 starting at element 1, 20 * 4 = 80 bytes = 0 mod 16, so every
    row starts 4 mod 16: the vector path is refused and the element path taken."""
    b = cr.source("float32", (6, 20), seed=13)
    return b, b[:, 1:17]


def three_fields(d0=9):
    """A quantise float32 -> uint8, a plain float32 field and a cast float32 -> float16."""
    m, x, w = (cr.source("float32", (d0, 5), 1), cr.source("float32", (d0, 2), 2),
               cr.source("float32", (d0, 6), 3))
    return [("mask", m, m[:, 1:4], quant("float32", "uint8", 255.0, 0)),
            ("xy", x, x, None),
            ("w", w, w[:, 1:6], cr.cast("float32", "float16"))]


def shape_cases(src, dst):
    """[(label, record)] of bare tensors of `src` quantised to `dst`: every shape of the list."""
    info = np.iinfo(DESTS[dst][0])
    zp = {"uint8": 128, "int8": -7, "uint16": 0, "int16": -7}[dst]
    scale = 3.0 if np.dtype(SOURCES[src][0]).kind == "f" else 0.5
    c, cs = quant(src, dst, None, 0), quant(src, dst, scale, zp)
    assert info.min <= zp <= info.max
    out = []
    for run in RUNS:
        for dense in (True, False):
            b, v = cr.run_view(src, run, dense, d0=3 if run == 1024 else 5)
            out.append((f"run={run} dense={dense}", [(None, b, v, cs if dense else c)]))
    b, v = cr.image_view(src)
    out.append(("image", [(None, b, v, cs)]))
    b, v = hwc_view(src)
    out.append(("chw->hwc", [(None, b, v, cs)]))
    for label, b, v in cr.strided_views(src):
        out.append((label, [(None, b, v, c)]))
    for d0 in D0:
        b, v = cr.run_view(src, 3, False, d0=d0)
        out.append((f"d0={d0}", [(None, b, v, cs)]))
    if src == "float32":
        b, v = f32_run_off_16()
        out.append(("run 4-aligned, not 16", [(None, b, v, cs)]))
    return out


def short_totals(dst):
    """Totals smaller than the head: 3 elements at destination 13 mod 16 (8-bit), 3 elements at 12
    mod 16 (16-bit: a head of 2 and a tail of 1)."""
    src = "float32"
    b = cr.source(src, (3,), seed=5)
    mis = 13 if np.dtype(DESTS[dst][0]).itemsize == 1 else 12
    return mis, [(None, b, b, quant(src, dst, 2.0, 0))]
