"""Resize records for the tensor-resize tests (dora_gpu_plan_tensor_resize), shared by the CPU plan
test, the host tests, the sanitized host emulation of gather_resize_kernel and the GPU tests: a
record is a list of (field name or None, base array, view of that base, resize or None), a resize a
dict {"src": source dtype name, "axes": (a, b), "size": (Oa, Ob), "mode": "nearest" | "bilinear",
"dst": destination dtype name or None (the source's own)}.  bfloat16 sources are held as their bits
in uint16 arrays (numpy has no such dtype).  `want` is the statement of record,
`tensor.from_numpy_resize`'s values; `same` compares with it bit for bit except where it is a NaN.

`cases()` is the list every runner goes through: the smallest shapes at which each path of the body
can go wrong."""
import functools
from ctypes import byref, c_int, c_int64, c_uint64, c_void_p

import numpy as np

from tests import cast_records as cr
from tests import struct_records as sr
from tests.gather_views import describe_view

SOURCES = cr.SOURCES
# destination dtype name -> (DLPack code, bits)
DESTS = {"float16": (2, 16), "float32": (2, 32), "uint8": (1, 8), "int8": (0, 8),
         "uint16": (1, 16), "int16": (0, 16)}
MODES = {"nearest": 1, "bilinear": 2}
same = cr.same


def rs(src, axes, size, mode="nearest", dst=None):
    return {"src": src, "axes": tuple(axes), "size": tuple(size), "mode": mode, "dst": dst}


def dst_name(r):
    return r["dst"] if r["dst"] is not None else r["src"]


def want(view, r):
    """The statement of record for `view` under resize `r` (None: the view as it is)."""
    if r is None:
        return np.ascontiguousarray(view)
    from dora_amd import tensor
    return tensor._numpy_resize(view, r["size"], r["axes"], r["mode"], r["dst"],
                                r["src"] == "bfloat16")


def describe(rec, ptr_of):
    """(dora_tensor_field array, dora_tensor_resize array, n, keepalive) of `rec` over `ptr_of`."""
    from dora_amd import tensor
    from dora_amd._lib import TensorResize
    tensors, keeps = [], []
    for _, b, v, r in rec:
        shape, strides, dtype, off = describe_view(b, v, None)
        t, keep = tensor._describe(ptr_of(b), shape, strides, dtype, off)
        if r is not None and r["src"] == "bfloat16":
            t.dtype_code = SOURCES["bfloat16"][1]
        tensors.append(t)
        keeps.append(keep)
    names = None if len(rec) == 1 and rec[0][0] is None else [x[0] for x in rec]
    lst, keep = tensor._describe_list(names, tensors, tensors[0], 0, 0)
    arr = (TensorResize * len(rec))()
    for k, (_, _, v, r) in enumerate(rec):
        if r is None:
            continue
        arr[k].mode = MODES[r["mode"]]
        for j in range(2):
            a = r["axes"][j]
            arr[k].axis[j] = a % v.ndim if -v.ndim <= a < v.ndim else a
            arr[k].size[j] = r["size"][j]
        if r["dst"] is not None:
            arr[k].dtype_code, arr[k].dtype_bits = DESTS[r["dst"]]
    return lst.fields, arr, len(rec), (lst, keep, keeps, rec)


def plan_resize(rec, ptr_of, dev):
    """Plan `rec` with dora_gpu_plan_tensor_resize; the Plan keeps the ctypes."""
    from dora_amd import _lib
    from dora_amd.arrow_utils import Plan
    fields, arr, n, keep = describe(rec, ptr_of)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_resize", fields, n, arr, dev, byref(h))
    return Plan(h.value, (fields, arr, keep))


def plan_resizes(plan, n, dst=0):
    """The per-field resize descriptors of a device plan of `n` fields
    (dora_gpu_test_plan_resize) for a sample at address `dst`."""
    from dora_amd import _lib
    out = []
    for i in range(n):
        mode, bits = c_int(), c_int()
        count, head, units, tail = c_uint64(), c_uint64(), c_uint64(), c_uint64()
        ins, outs, steps = (c_int64 * 2)(), (c_int64 * 2)(), (c_int64 * 2)()
        _lib.call("dora_gpu_test_plan_resize", plan.handle, i, dst, byref(mode), byref(count),
                  byref(bits), ins, outs, steps, byref(head), byref(units), byref(tail))
        out.append({"mode": mode.value, "count": count.value, "bits": bits.value,
                    "in": tuple(ins), "out": tuple(outs), "stride": tuple(steps),
                    "head": head.value, "units": units.value, "tail": tail.value})
    return out


def oracle(rec):
    """(sample bytes, ArrowTypeInfo, [(offset, length) of each field's leaf]) of the reference
    packing of the materialised record: the nested array of a bare resized tensor, else the
    StructArray of the fields."""
    import pyarrow as pa
    from dora_amd import tensor
    from oracle.pack_ref import pack
    cols = [tensor.from_numpy(want(v, r)) for _, _, v, r in rec]
    bare = len(rec) == 1 and rec[0][0] is None
    arr = cols[0] if bare else pa.StructArray.from_arrays(cols, names=[x[0] for x in rec])
    sample, info = pack(arr)
    ranges = []
    for c in ([info] if bare else info.child_data):
        while c.child_data:
            c = c.child_data[0]
        ranges.append((c.buffer_offsets[0].offset, c.buffer_offsets[0].len))
    return sample, info, ranges


def bases_of(rec):
    return sr.bases_of([(n, b, v) for n, b, v, _ in rec])


def dst_offsets(dst):
    """Every multiple of the destination element size mod 16."""
    return range(0, 16, DESTS[dst][1] // 8)


def dests_of(src):
    return ([] if src == "bfloat16" else [None]) + list(DESTS)


# ---------------------------------------------------------------------------------------------
# Values
# ---------------------------------------------------------------------------------------------
def from_f32(x, src):
    """float32 values (exactly representable in `src`) as the array that holds them."""
    x = np.asarray(x, np.float32)
    if src == "bfloat16":
        return (x.view(np.uint32) >> 16).astype(np.uint16)
    return x.astype(SOURCES[src][0])


def special_floats(src):
    """A 4 x 5 array of `src` (a float source): +-inf, NaN, +-0.0, subnormals of float16 and
    float32, large and small finite values."""
    tiny32 = np.float32(1e-45)                     # the smallest float32 subnormal
    sub16 = np.float32(2.0 ** -24)                 # the smallest float16 subnormal
    big = np.float32(60000.0)
    x = np.array([[np.inf, 1.0, -0.0, 0.0, -np.inf],
                  [np.nan, -2.5, sub16, -sub16, 3.0],
                  [big, -big, tiny32, -tiny32, 0.5],
                  [2.0 ** -14, -(2.0 ** -15), 7.0, np.nan, 65520.0]], np.float32)
    if src == "float16":
        with np.errstate(over="ignore", under="ignore"):
            return x.astype(np.float16)
    return from_f32(x, src)


def ties_u8():
    """uint8 rows whose halved width blends pairs with w = 0.5: (0, 1) -> 0.5 -> 0, (254, 255) ->
    254.5 -> 254, (1, 2) -> 1.5 -> 2, (2, 3) -> 2.5 -> 2: ties to even."""
    return np.array([[0, 1, 254, 255, 1, 2, 2, 3], [255, 255, 0, 0, 3, 4, 4, 5]], np.uint8)


# ---------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------
# (label, base shape, view of the base, axes, size)
GEOMETRY = [
    ("HWC down coprime", (7, 9, 3), None, (0, 1), (5, 4)),
    ("CHW up coprime", (3, 5, 6), None, (-2, -1), (11, 13)),
    ("one axis changes", (13, 17), None, (0, 1), (13, 6)),
    ("identity", (6, 5, 2), None, (0, 1), (6, 5)),
    ("I = 1", (1, 9, 2), None, (0, 1), (3, 4)),
    ("I = 1 both", (3, 1, 1), None, (1, 2), (4, 5)),
    ("O = 1", (5, 6), None, (0, 1), (1, 1)),
    ("O > 2 I", (2, 3), None, (0, 1), (7, 9)),
    ("4-D batch", (2, 3, 5, 6), None, (-2, -1), (4, 7)),
    ("axes (0, 2)", (5, 3, 6), None, (0, 2), (3, 8)),
    ("axes reversed", (7, 9, 3), None, (1, 0), (4, 5)),
    ("axes reversed CHW", (2, 6, 5), None, (-1, -2), (9, 4)),
    ("permuted HWC -> CHW", (7, 9, 3), lambda b: b.transpose(2, 0, 1), (-2, -1), (5, 4)),
    ("cut", (9, 8), lambda b: b[::2, 1:], (0, 1), (7, 4)),
    ("reversed rows", (6, 7), lambda b: b[::-1], (0, 1), (4, 9)),
    ("reversed columns", (6, 7, 2), lambda b: b[:, ::-1], (0, 1), (8, 3)),
    ("broadcast on a resized axis", (1, 7), lambda b: np.broadcast_to(b, (5, 7)), (0, 1), (3, 10)),
    ("broadcast on a kept axis", (4, 5, 1), lambda b: np.broadcast_to(b, (4, 5, 3)), (0, 1), (6, 3)),
    ("8-D", (2, 1, 2, 3, 1, 2, 4, 2), None, (3, 6), (5, 3)),
]


@functools.lru_cache(maxsize=None)
def cases():
    """[(label, record, destination offsets mod 16)]."""
    out = []
    srcs = list(SOURCES)
    # all seven sources x the destinations allowed x both modes, an HWC image downscaled
    for i, src in enumerate(srcs):
        b = cr.source(src, (7, 9, 3), seed=i)
        for dst in dests_of(src):
            for mode in MODES:
                out.append((f"{src}->{dst} {mode}", [(None, b, b, rs(src, (0, 1), (5, 4), mode, dst))],
                            (0,)))
    # geometry and views, both modes, sources and destinations taking turns
    k = 0
    for label, shape, view, axes, size in GEOMETRY:
        for mode in MODES:
            src = srcs[k % len(srcs)]
            dst = dests_of(src)[k % len(dests_of(src))]
            k += 1
            b = cr.source(src, shape, seed=k)
            v = b if view is None else view(b)
            r = rs(src, axes, size, mode, dst)
            out.append((f"{label} {mode} {src}->{dst}", [(None, b, v, r)],
                        (0, 3 * DESTS[dst_name(r)][1] // 8)))
    # destinations: every multiple of the destination element size mod 16, so heads and tails occur
    for dst in ("uint8", "int16", "float16", "float32"):
        b = cr.source("uint8", (5, 6, 3), seed=41)
        out.append((f"dst {dst} every misalignment",
                    [(None, b, b, rs("uint8", (0, 1), (3, 5), "bilinear", dst))],
                    tuple(dst_offsets(dst))))
    # fields of 1 to 40 elements: shorter than a unit, a unit, a few
    b = cr.source("uint8", (2, 3), seed=42)
    f = cr.source("float32", (3, 2), seed=43)
    for n in range(1, 41):
        mode = "bilinear" if n % 2 else "nearest"
        out.append((f"{n} elements uint8", [(None, b, b, rs("uint8", (0, 1), (1, n), mode))],
                    (0, 5, 15)))
        out.append((f"{n} elements float32->float16",
                    [(None, f, f, rs("float32", (0, 1), (n, 1), mode, "float16"))], (0, 14)))
    # values: non-finite and subnormal floats, through every float destination and an integer one
    for src in ("float16", "bfloat16", "float32"):
        x = special_floats(src)
        for dst in dests_of(src)[:4]:
            for mode in MODES:
                out.append((f"special values {src}->{dst} {mode}",
                            [(None, x, x, rs(src, (0, 1), (7, 9), mode, dst))], (0,)))
        out.append((f"special values {src} identity",
                    [(None, x, x, rs(src, (0, 1), (4, 5), "bilinear", "float32"))], (0,)))
    # exact .5 ties and saturation
    t = ties_u8()
    out.append(("ties to even uint8", [(None, t, t, rs("uint8", (0, 1), (2, 4), "bilinear"))], (0,)))
    out.append(("ties to even uint8 both axes", [(None, t, t, rs("uint8", (0, 1), (1, 4), "bilinear"))], (0,)))
    w = np.array([[300, -5, 70000 // 3, -32768], [255, 256, -129, 127]], np.int16)
    for dst in ("uint8", "int8", "uint16"):
        out.append((f"saturation int16->{dst}", [(None, w, w, rs("int16", (0, 1), (3, 7), "bilinear", dst))], (0,)))
    g = np.array([[1e9, -1e9, np.nan], [40000.0, -40000.0, 0.5]], np.float32)
    for dst in ("int16", "uint16", "float16"):
        out.append((f"saturation float32->{dst}", [(None, g, g, rs("float32", (0, 1), (2, 3), "nearest", dst))], (0,)))
    # records: a resized field between plain fields, two resized fields
    for d0 in (2, 5):
        out.append((f"record d0={d0}", record(d0), (0, 2, 8)))
    return out


LIMIT = 32768  # the largest I and O of the statement
# output extents at which the weights are read directly: small odd ones, either side of 2^8 and
# 2^12, 2^16 / 3, and the limit and the one below it
WEIGHT_EXTENTS = (3, 5, 7, 255, 256, 257, 4095, 4097, 21845, LIMIT - 1, LIMIT)
# float32 frames of one column whose bilinear resize along axis 0 is a weight of every output
# coordinate: w1, w0, and with I = 3 the other residues
WEIGHT_FRAMES = (("w1", [[0], [1]]), ("w0", [[1], [0]]), ("I = 3", [[0], [0], [1]]))


@functools.lru_cache(maxsize=None)
def limit_cases():
    """[(label, record, destination offsets mod 16)] at the edge of the contract, beside `cases()`:
    axes of 32768 source or output steps over small frames, where (2 * o + 1) * I reaches
    2^31 - 32768 and d = 2 * O is 65536, and the weights of WEIGHT_EXTENTS read directly.  None
    has more than 100 000 output elements."""
    out = []
    u = cr.source("uint8", (LIMIT, 3), seed=71)
    for mode in MODES:
        for size in ((LIMIT - 1, 2), (LIMIT, 3)):
            out.append((f"({LIMIT}, 3) uint8 -> {size} {mode}",
                        [(None, u, u, rs("uint8", (0, 1), size, mode))], (0,)))
    w = cr.source("int16", (3, LIMIT), seed=72)
    out.append((f"(3, {LIMIT}) int16 -> (5, {LIMIT - 1}) float16",
                [(None, w, w, rs("int16", (0, 1), (5, LIMIT - 1), "bilinear", "float16"))], (0,)))
    f = cr.source("float32", (2, 3), seed=73)
    out.append((f"(2, 3) float32 -> ({LIMIT}, 2)",
                [(None, f, f, rs("float32", (0, 1), (LIMIT, 2), "bilinear"))], (4,)))
    for mode in MODES:
        out.append((f"({LIMIT}, 1) -> (1, 1) {mode}",
                    [(None, u, u[:, 1:2], rs("uint8", (0, 1), (1, 1), mode, "float32"))], (0,)))
    wide = cr.source("uint8", (2 * LIMIT, 3), seed=74)
    out.append((f"({LIMIT}, 3) cut with step 2 -> ({LIMIT - 1}, 2)",
                [(None, wide, wide[::2], rs("uint8", (0, 1), (LIMIT - 1, 2), "bilinear"))], (3,)))
    out.append((f"({LIMIT}, 3) cut with step -2 -> ({LIMIT - 1}, 2)",
                [(None, wide, wide[::-2], rs("uint8", (0, 1), (LIMIT - 1, 2), "bilinear"))], (0,)))
    for label, rows in WEIGHT_FRAMES:
        x = np.array(rows, np.float32)
        for o in WEIGHT_EXTENTS:
            out.append((f"{label} O={o}", [(None, x, x, rs("float32", (0, 1), (o, 1), "bilinear"))],
                        (0,)))
    return out


def weights_in_float64(n_in, n_out):
    """(w0, w1, where the last source element stands alone) of every output coordinate of a
    bilinear axis by the statement's integer formula,
    the division in float64 and rounded to float32 once.  That is the correctly rounded float32
    quotient: float64's 53 bits are at least 2 * 24 + 2, so rounding a quotient twice is
    innocuous."""
    o = np.arange(n_out, dtype=np.int64)
    d = 2 * n_out
    n = np.maximum((2 * o + 1) * n_in - n_out, 0)
    last = n // d >= n_in - 1
    r = np.where(last, 0, n % d)
    return (((d - r).astype(np.float64) / d).astype(np.float32),
            (r.astype(np.float64) / d).astype(np.float32), last)


def record(d0=2):
    """A resized batch of HWC thumbnails between a plain int64 field and a strided plain float32
    field, then a second resized field to float16 whose leading extent is a resized one."""
    stamp = np.arange(d0, dtype=np.int64) * 1000 + 7
    frames = cr.source("uint8", (d0, 5, 6, 3), seed=51)
    x = cr.source("float32", (d0, 4), seed=52)
    m = cr.source("int16", (3, 7), seed=53)
    return [("stamp", stamp, stamp, None),
            ("thumb", frames, frames, rs("uint8", (1, 2), (3, 4), "bilinear")),
            ("xy", x, x[:, 1:3], None),
            ("map", m, m, rs("int16", (0, 1), (d0, 3), "nearest", "float16"))]
