"""Argmax records for the tensor-argmax tests (dora_gpu_plan_tensor_reduce), shared by the CPU plan
test, the host tests, the sanitized host emulation of gather_reduce_kernel and the GPU tests: a
record is a list of (field name or None, base array, view of that base, reduction or None), a
reduction a dict {"src": source dtype name, "axis": int, "dtype": index dtype name}.  bfloat16
sources are held as their bits in uint16 arrays (numpy has no such dtype).  `want` is the statement
of record, `np.argmax(x32, axis).astype(dtype)`; the comparison is bit for bit.

`cases()` is the list every runner goes through: the smallest shapes at which each path of the two
bodies can go wrong."""
import functools
from ctypes import byref, c_int, c_int64, c_uint64, c_void_p

import numpy as np

from tests import cast_records as cr
from tests import struct_records as sr
from tests.gather_views import describe_view

SOURCES = cr.SOURCES
# index dtype name -> (DLPack code, bits, largest C)
INDEX = {"uint8": (1, 8, 256), "uint16": (1, 16, 65536), "int32": (0, 32, 2 ** 31),
         "int64": (0, 64, 2 ** 62)}
CS = (1, 2, 3, 63, 64, 65, 129, 256, 1000, 4097)
COUNTS = (1, 15, 16, 17, 63, 64, 65, 257)


def red(src, axis, dtype="int64"):
    return {"src": src, "axis": axis, "dtype": dtype}


def want(view, r):
    """The statement of record for `view` under reduction `r` (None: the view as it is)."""
    if r is None:
        return np.ascontiguousarray(view)
    return np.argmax(cr.to_f32(view, r["src"]), r["axis"]).astype(r["dtype"])


def same(got, expect, what=""):
    expect = np.ascontiguousarray(expect)
    assert len(got) == expect.nbytes, (what, len(got), expect.nbytes)
    if bytes(got) != expect.tobytes():
        g = np.frombuffer(bytes(got), expect.dtype).reshape(expect.shape)
        bad = np.argwhere(g != expect)
        raise AssertionError((what, bad[0].tolist(), int(g[tuple(bad[0])]),
                              int(expect[tuple(bad[0])]), len(bad)))


def describe(rec, ptr_of):
    """(dora_tensor_field array, dora_tensor_reduce array, n, keepalive) of `rec` over `ptr_of`."""
    from dora_amd import tensor
    from dora_amd._lib import REDUCE_ARGMAX, TensorReduce
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
    reds = (TensorReduce * len(rec))()
    for k, (_, _, v, r) in enumerate(rec):
        if r is None:
            continue
        reds[k].op = REDUCE_ARGMAX
        reds[k].axis = r["axis"] % v.ndim if -v.ndim <= r["axis"] < v.ndim else r["axis"]
        reds[k].dtype_code, reds[k].dtype_bits = INDEX[r["dtype"]][:2]
    return lst.fields, reds, len(rec), (lst, keep, keeps, rec)


def plan_reduce(rec, ptr_of, dev):
    """Plan `rec` with dora_gpu_plan_tensor_reduce; the Plan keeps the ctypes."""
    from dora_amd import _lib
    from dora_amd.arrow_utils import Plan
    fields, reds, n, keep = describe(rec, ptr_of)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_reduce", fields, n, reds, dev, byref(h))
    return Plan(h.value, (fields, reds, keep))


def plan_reduces(plan, n, dst=0):
    """The per-field reduce descriptors of a device plan of `n` fields
    (dora_gpu_test_plan_reduce) for a sample at address `dst`."""
    from dora_amd import _lib
    out = []
    for i in range(n):
        op, bits, body = c_int(), c_int(), c_int()
        c, count, vec, elem, stride = c_uint64(), c_uint64(), c_uint64(), c_uint64(), c_int64()
        _lib.call("dora_gpu_test_plan_reduce", plan.handle, i, dst, byref(op), byref(c),
                  byref(stride), byref(count), byref(bits), byref(body), byref(vec), byref(elem))
        out.append({"op": op.value, "c": c.value, "cstride": stride.value, "count": count.value,
                    "bits": bits.value, "body": body.value, "vector_units": vec.value,
                    "element_units": elem.value})
    return out


def oracle(rec):
    """(sample bytes, ArrowTypeInfo, [(offset, length) of each field's leaf]) of the reference
    packing of the materialised record: the nested array of a bare index tensor, else the
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


def reach(v, axis):
    """[lo, hi] in bytes from the view's first element over every dimension, `axis` included."""
    lo = sum((n - 1) * s for n, s in zip(v.shape, v.strides) if s < 0)
    hi = sum((n - 1) * s for n, s in zip(v.shape, v.strides) if s > 0) + v.itemsize - 1
    return lo, hi


def bases_of(rec):
    return sr.bases_of([(n, b, v) for n, b, v, _ in rec])


def dst_offsets(dtype):
    """Every multiple of the index element size mod 16."""
    return range(0, 16, INDEX[dtype][1] // 8)


def index_for(c, k=0):
    """An index dtype that holds C - 1, a different one for different k."""
    ok = [d for d in INDEX if c <= INDEX[d][2]]
    return ok[k % len(ok)]


# ---------------------------------------------------------------------------------------------
# Values
# ---------------------------------------------------------------------------------------------
def from_f32(x, src):
    """float32 values (exactly representable in `src`) as the array that holds them."""
    x = np.asarray(x, np.float32)
    if src == "bfloat16":
        return (x.view(np.uint32) >> 16).astype(np.uint16)
    return x.astype(SOURCES[src][0])


def value_rows(src, c):
    """[(label, C values)]: where the maximum sits and what it ties with."""
    dt = np.dtype(SOURCES[src][0])
    flt = src in ("float16", "bfloat16", "float32")
    lo, hi = (-4.0, 9.0) if flt or dt.kind == "i" else (1.0, 9.0)
    if not flt:
        info = np.iinfo(dt)
        lo, hi = float(info.min), float(info.max)
    mid = 3.0

    def row(fill, **at):
        x = np.full(c, fill, np.float32)
        for k, v in at.items():
            x[int(k[1:]) % c] = v
        return x
    rows = [("all equal", row(mid)), ("max first", row(mid, _0=hi)),
            ("max last", row(mid, **{f"_{c - 1}": hi})),
            ("max first and last", row(mid, _0=hi, **{f"_{c - 1}": hi})),
            ("min everywhere but last", row(lo, **{f"_{c - 1}": mid})),
            ("extremes", row(mid, **{f"_{c // 2}": hi, f"_{c // 3}": lo}))]
    if c == 129:
        for p in (0, 1, 63, 64, 65, 127, 128):
            rows.append((f"max at {p}", row(mid, **{f"_{p}": hi})))
        rows.append(("equal maxima in two lanes", row(mid, _5=hi, _70=hi)))
        rows.append(("equal maxima in two passes of a lane", row(mid, _69=hi, _5=hi)))
        rows.append(("equal maxima in two passes, later lane first", row(mid, _64=hi, _3=hi)))
    if flt:
        nan, inf = np.float32(np.nan), np.float32(np.inf)
        rows += [("nan first", row(mid, _0=nan, **{f"_{c - 1}": hi})),
                 ("nan last", row(mid, _0=hi, **{f"_{c - 1}": nan})),
                 ("nan alone", row(nan)), ("all -inf", row(-inf)),
                 ("nan beside +inf", row(mid, **{f"_{c // 2}": inf, f"_{(c // 2 + 1)}": nan})),
                 ("two nans", row(mid, **{f"_{c // 3}": nan, f"_{c - 1}": nan})),
                 ("-0 before +0", row(-1.0, **{f"_{c // 3}": -0.0, f"_{c - 1}": 0.0})),
                 ("+0 before -0", row(-1.0, **{f"_{c // 3}": 0.0, f"_{c - 1}": -0.0}))]
    return rows


def value_block(src, c):
    """(labels, array of shape (rows, C)) of value_rows as `src`."""
    rows = value_rows(src, c)
    out = np.stack([from_f32(x, src) for _, x in rows])
    return [label for label, _ in rows], out


def bf16_last_bit():
    """(rows, C = 4) bfloat16 bits that differ only in the last kept bit."""
    return np.array([[0x3F80, 0x3F81, 0x3F80, 0x3F81], [0x3F81, 0x3F80, 0x3F80, 0x3F80],
                     [0xBF81, 0xBF80, 0xBF81, 0xBF80], [0x4000, 0x4000, 0x4001, 0x4000]], np.uint16)


# ---------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases():
    """[(label, record, destination offsets mod 16)]."""
    out = []
    srcs = list(SOURCES)
    k = 0
    # every C against an output count, the reduced axis first (a contiguous span a step) and last
    # (the source-contiguous dimension), sources and index dtypes taking turns
    for i, c in enumerate(CS):
        for last in (False, True):
            n = COUNTS[(i + (3 if last else 0)) % len(COUNTS)]
            src, dt = srcs[k % len(srcs)], index_for(c, k)
            k += 1
            b = cr.source(src, (n, c) if last else (c, n), seed=c)
            out.append((f"C={c} n={n} {'last' if last else 'first'} {src}->{dt}",
                        [(None, b, b, red(src, 1 if last else 0, dt))], (0,)))
    # every output count at a small and a wave-sized C, every source once more
    for i, n in enumerate(COUNTS):
        src = srcs[i % len(srcs)]
        b = cr.source(src, (5, n), seed=n)
        out.append((f"n={n} C=5 first {src}", [(None, b, b, red(src, 0, "uint8"))], (0,)))
        b = cr.source(src, (n, 129), seed=n + 1)
        out.append((f"n={n} C=129 last {src}", [(None, b, b, red(src, 1, "uint16"))], (0,)))
    # destinations: every multiple of the index size mod 16, on the vector path, the element path
    # and the wave body
    for dt in INDEX:
        b = cr.source("float16", (6, 70), seed=11)
        out.append((f"dst {dt} vector", [(None, b, b, red("float16", 0, dt))], tuple(dst_offsets(dt))))
        b = cr.source("float32", (37, 7), seed=12)
        out.append((f"dst {dt} element", [(None, b, b, red("float32", 1, dt))], tuple(dst_offsets(dt))))
        b = cr.source("int16", (21, 130), seed=13)
        out.append((f"dst {dt} wave", [(None, b, b, red("int16", 1, dt))], tuple(dst_offsets(dt))))
    # views
    b = cr.source("float32", (6, 9, 20), seed=21)
    for ax in (0, 1, 2):
        out.append((f"3-D axis {ax}", [(None, b, b, red("float32", ax, "int32"))], (0, 4)))
    b = cr.source("uint8", (5, 7, 3), seed=22)
    for ax in (0, 1, 2):
        out.append((f"image permuted axis {ax}",
                    [(None, b, b.transpose(2, 0, 1), red("uint8", ax, "uint8"))], (0, 3)))
    b = cr.source("float16", (9, 40), seed=23)
    out.append(("negative stride on the reduced axis, first", [(None, b, b[::-1], red("float16", 0, "uint8"))], (0,)))
    out.append(("negative stride on the reduced axis, last", [(None, b, b[:, ::-1], red("float16", 1, "int64"))], (0, 8)))
    z = cr.source("int8", (1, 37), seed=24)
    out.append(("zero stride on the reduced axis", [(None, z, np.broadcast_to(z, (6, 37)), red("int8", 0, "uint16"))], (0,)))
    out.append(("zero stride on a kept axis", [(None, z, np.broadcast_to(z, (6, 37)), red("int8", 1, "uint8"))], (0,)))
    z = cr.source("float32", (200, 1), seed=25)
    out.append(("zero stride on a kept axis, wave", [(None, z, np.broadcast_to(z, (200, 3)).T, red("float32", 1, "int32"))], (0,)))
    for src in ("uint8", "float16", "float32"):
        b = cr.source(src, (7, 70), seed=26)
        out.append((f"cut from a wider base {src}", [(None, b, b[:, 1:66], red(src, 0, "uint8"))], (0, 5)))
        b = cr.source(src, (19, 140), seed=27)
        out.append((f"cut from a wider base {src}, wave", [(None, b, b[:, 3:135], red(src, 1, "uint8"))], (0,)))
    # values
    for src in SOURCES:
        for c in (3, 129):
            _, block = value_block(src, c)
            out.append((f"values {src} C={c} last", [(None, block, block, red(src, 1, "uint8"))], (0,)))
            t = np.ascontiguousarray(block.T)
            out.append((f"values {src} C={c} first", [(None, t, t, red(src, 0, "int32"))], (0,)))
    bits = bf16_last_bit()
    out.append(("bfloat16 last kept bit", [(None, bits, bits, red("bfloat16", 1, "uint8"))], (0,)))
    t = np.ascontiguousarray(np.tile(bits.T, (1, 5)))
    out.append(("bfloat16 last kept bit, first", [(None, t, t, red("bfloat16", 0, "uint8"))], (0,)))
    # a record: two argmax fields and a strided plain one, the fields starting 2 and 4 mod 16
    for d0 in (9, 33):
        out.append((f"record d0={d0}", record(d0), (0, 2, 4)))
    return out


def record(d0=9):
    """Two argmax fields and a strided plain float32 field: with uint16 indices of (d0, 3) first,
    d0 odd, the plain field is padded to 4 and the last field starts 2 or 4 mod 16 at some of the
    destinations used (checked by the callers)."""
    a = cr.source("float16", (d0, 21, 3), seed=31)
    x = cr.source("float32", (d0, 4), seed=32)
    w = cr.source("bfloat16", (150, d0, 2), seed=33)
    return [("cls", a, a, red("float16", 1, "uint16")),
            ("depth", x, x[:, 1:3], None),
            ("top", w, w, red("bfloat16", 0, "uint16"))]
