"""Cast records for the tensor-cast tests (dora_gpu_plan_tensor_cast), shared by the CPU plan test,
the host tests, the sanitized host emulation of gather_cast_kernel and the GPU tests: a record is a
list of (field name or None, base array, view of that base, cast or None), a cast a dict
{"src": source dtype name, "dst": "float16" | "float32", "scale": float or None}.  bfloat16 sources
are held as their bits in uint16 arrays (numpy has no such dtype).  `want` is the statement of
record, `(x.astype(float32) * float32(scale)).astype(dst)`; `same` compares with it bit for bit
except where it is a NaN."""
import functools
from ctypes import byref, c_float, c_int, c_size_t, c_uint64, c_void_p

import numpy as np

from tests import struct_records as sr
from tests.gather_views import describe_view

# source dtype name -> (numpy dtype that holds it, DLPack type code)
SOURCES = {"uint8": (np.uint8, 1), "int8": (np.int8, 0), "uint16": (np.uint16, 1),
           "int16": (np.int16, 0), "float16": (np.float16, 2), "bfloat16": (np.uint16, 4),
           "float32": (np.float32, 2)}
DESTS = ("float16", "float32")
PAIRS = [(s, d) for s in SOURCES for d in DESTS]
SCALES = (1 / 255, 1 / 32768, 2.0 ** -20)


def cast(src, dst, scale=None):
    return {"src": src, "dst": dst, "scale": scale}


def source(src, shape, seed=0):
    """A base array of `src` with distinct-looking values: small and large ones, both signs, for
    the float types fractions too (all finite)."""
    rng = np.random.default_rng(seed + len(src))
    n = int(np.prod(shape))
    dt = SOURCES[src][0]
    if src == "bfloat16":
        f = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
        return (f.view(np.uint32) >> 16).astype(np.uint16).reshape(shape)
    if np.dtype(dt).kind == "f":
        return (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(dt).reshape(shape)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max + 1, n).astype(dt).reshape(shape)


def to_f32(x, src):
    x = np.asarray(x)
    if src == "bfloat16":
        return (np.ascontiguousarray(x).astype(np.uint32) << 16).view(np.float32)
    return x.astype(np.float32)


def want(view, c):
    """The statement of record for `view` under cast `c` (None: the view as it is)."""
    if c is None:
        return np.ascontiguousarray(view)
    y = to_f32(view, c["src"])
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if c["scale"] is not None:
            y = y * np.float32(c["scale"])
        return y.astype(c["dst"])


def same(got, expect, what=""):
    """`got` (bytes) equals array `expect` bit for bit, NaN for NaN."""
    expect = np.ascontiguousarray(expect)
    assert len(got) == expect.nbytes, (what, len(got), expect.nbytes)
    if expect.dtype.kind != "f":
        assert bytes(got) == expect.tobytes(), what
        return
    g = np.frombuffer(bytes(got), expect.dtype).reshape(expect.shape)
    nan = np.isnan(expect)
    assert np.isnan(g[nan]).all(), (what, "a NaN expected")
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[expect.dtype.itemsize]
    a, b = g[~nan].view(u), expect[~nan].view(u)
    bad = np.flatnonzero(a != b)
    assert len(bad) == 0, (what, int(bad[0]), hex(int(a[bad[0]])), hex(int(b[bad[0]])))


def describe(rec, ptr_of):
    """(dora_tensor_field array, dora_tensor_cast array, n, keepalive) of `rec` over `ptr_of`."""
    from dora_amd import tensor
    from dora_amd._lib import TensorCast
    tensors, keeps = [], []
    for _, b, v, c in rec:
        shape, strides, dtype, off = describe_view(b, v, None)
        t, keep = tensor._describe(ptr_of(b), shape, strides, dtype, off)
        if c is not None and c["src"] == "bfloat16":
            t.dtype_code = SOURCES["bfloat16"][1]  # (every other code is the numpy dtype's own)
        tensors.append(t)
        keeps.append(keep)
    names = None if len(rec) == 1 and rec[0][0] is None else [r[0] for r in rec]
    lst, keep = tensor._describe_list(names, tensors, tensors[0], 0, 0)
    casts = (TensorCast * len(rec))()
    for k, (_, _, _, c) in enumerate(rec):
        if c is None:
            continue
        casts[k].dtype_code, casts[k].dtype_bits = 2, 16 if c["dst"] == "float16" else 32
        casts[k].has_scale = 0 if c["scale"] is None else 1
        casts[k].scale = 0.0 if c["scale"] is None else c["scale"]
    return lst.fields, casts, len(rec), (lst, keep, keeps, rec)


def plan_cast(rec, ptr_of, dev):
    """Plan `rec` with dora_gpu_plan_tensor_cast; the Plan keeps the ctypes."""
    from dora_amd import _lib
    from dora_amd.arrow_utils import Plan
    fields, casts, n, keep = describe(rec, ptr_of)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_cast", fields, n, casts, dev, byref(h))
    return Plan(h.value, (fields, casts, keep))


def plan_casts(plan):
    """The per-field cast descriptors of a device plan (dora_gpu_test_plan_cast)."""
    from dora_amd import _lib
    out, i = [], 0
    while True:
        n, on, sc, sb, dc, db, hs = c_size_t(), c_int(), c_int(), c_int(), c_int(), c_int(), c_int()
        scale, count, sbytes, dbytes = c_float(), c_uint64(), c_uint64(), c_uint64()
        _lib.call("dora_gpu_test_plan_cast", plan.handle, i, byref(n), byref(on), byref(sc),
                  byref(sb), byref(dc), byref(db), byref(hs), byref(scale), byref(count),
                  byref(sbytes), byref(dbytes))
        out.append({"cast": bool(on.value), "src_code": sc.value, "src_bits": sb.value,
                    "dst_code": dc.value, "dst_bits": db.value, "has_scale": bool(hs.value),
                    "scale": scale.value, "count": count.value, "src_bytes": sbytes.value,
                    "dst_bytes": dbytes.value})
        i += 1
        if i >= n.value:
            return out


def oracle(rec):
    """(sample bytes, ArrowTypeInfo, [(offset, length) of each field's leaf]) of the reference
    packing of the materialised converted record: the nested array of a bare tensor, else the
    StructArray of the fields."""
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


def reach(b, v):
    """[lo, hi] in bytes from the view's first element, from its strides and itemsize alone."""
    lo = sum((n - 1) * s for n, s in zip(v.shape, v.strides) if s < 0)
    hi = sum((n - 1) * s for n, s in zip(v.shape, v.strides) if s > 0) + v.itemsize - 1
    return lo, hi


# ---------------------------------------------------------------------------------------------
# Value sets: what the conversions are checked on, the hardware's and the integer routines alike.
# ---------------------------------------------------------------------------------------------
def f16_rounding_inputs():
    """float32 inputs around every float16: for each finite float16 bit pattern its exact value,
    the midpoint to the next float16 away from zero (65520 past the largest) and that midpoint
    -1 and +1 ulp; then +-0, +-inf, the largest and smallest float32 subnormals, 65504, 65519.996,
    65520 and NaNs."""
    bits = np.arange(65536, dtype=np.uint32)
    h = bits.astype(np.uint16).view(np.float16)
    fin = np.isfinite(h)
    bits, x = bits[fin], h[fin].astype(np.float64)
    nxt = (bits + 1).astype(np.uint16).view(np.float16).astype(np.float64)
    nxt = np.where(np.isinf(nxt), np.sign(nxt) * 65536.0, nxt)
    mid = ((x + nxt) / 2).astype(np.float32)  # exact: 12 significant bits
    assert (mid.astype(np.float64) == (x + nxt) / 2).all()
    away = np.where(np.signbit(mid), -np.inf, np.inf).astype(np.float32)
    extra = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x007fffff, 0x807fffff,
                      0x00000001, 0x80000001, 0x7fc00000, 0x7f800001, 0xffc00000, 0xff8fffff],
                     np.uint32).view(np.float32)
    named = np.array([65504.0, 65519.996, 65520.0, -65504.0, -65519.996, -65520.0], np.float32)
    return np.concatenate([x.astype(np.float32), mid, np.nextafter(mid, -away),
                           np.nextafter(mid, away), extra, named])


def all_patterns(src):
    """Every value of an 8- or 16-bit source type, as its holding dtype."""
    dt = np.dtype(SOURCES[src][0])
    n = 1 << (8 * dt.itemsize)
    return np.arange(n, dtype=np.uint32).astype({1: np.uint8, 2: np.uint16}[dt.itemsize]).view(dt)


# scales of the float16 and bfloat16 sources: products in the float16 subnormals, far below the
# float32 normals, inexact, negated, and exactly zero of either sign
FLOAT_SCALES = (2.0 ** -14, 2.0 ** -120, 1 / 255, 3.0, -1.0, 0.0, -0.0)
# scales of float32 -> float32 over the float16 values: products rounded inside the float32
# subnormal range, overflow to infinity, a scale that is itself subnormal
F32_SCALES = (float(np.float32(2.0 ** -118 / 255)), 2.0 ** 114, 2.0 ** -140)
# len(value_sets()), for parametrising without computing them at collection time
N_VALUE_SETS = 3 + 4 * 2 * 3 + 2 * 2 * len(FLOAT_SCALES) + 3 + len(F32_SCALES)


@functools.lru_cache(maxsize=None)
def value_sets():
    """[(label, 1-D source array, cast)]: the conversions' whole domain where it is small
    (computed once; the callers leave the arrays as they are)."""
    out = [("f32->f16 rounding", f16_rounding_inputs(), cast("float32", "float16")),
           ("f16->f32 all", all_patterns("float16"), cast("float16", "float32")),
           ("bf16->f32 all", all_patterns("bfloat16"), cast("bfloat16", "float32"))]
    for src in ("uint8", "int8", "uint16", "int16"):
        for dst in DESTS:
            for s in SCALES:
                out.append((f"{src}->{dst} * {s!r}", all_patterns(src), cast(src, dst, s)))
    # float sources under a scale, the multiplication over its domain: products that land in the
    # float16 and the float32 subnormals, that underflow to a signed zero and that overflow;
    # signed zeros, infinities and NaNs through the multiply; scales that are negative, +-0 and
    # themselves subnormal
    for src in ("float16", "bfloat16"):
        for dst in DESTS:
            for s in FLOAT_SCALES:
                out.append((f"{src}->{dst} * {s!r}", all_patterns(src), cast(src, dst, s)))
    for s in (2.0 ** 8, 2.0 ** -8, 3.0):  # (the first two are exact: the boundaries move)
        out.append((f"f32->f16 rounding * {s!r}", f16_rounding_inputs(), cast("float32", "float16", s)))
    widened = all_patterns("float16").astype(np.float32)
    for s in F32_SCALES:
        out.append((f"f32->f32 f16 values * {s!r}", widened, cast("float32", "float32", s)))
    return out


def cut_from_wider(x, run=67):
    """(base, view) holding the 1-D value set `x` as rows of `run` elements cut from rows 3 wider:
    an odd run, so units straddle rows and a row's first element meets every alignment.  The last
    row is padded with x[0] (+0 in every set), which so sits at many places of a 16-byte unit."""
    rows = -(-len(x) // run)
    b = np.full((rows, run + 3), x[0], x.dtype)
    v = b[:, 1:run + 1]
    v[...] = np.resize(np.concatenate([x, np.full(rows * run - len(x), x[0], x.dtype)]), (rows, run))
    return b, v


# ---------------------------------------------------------------------------------------------
# Shapes: what the address computations are checked on (the emulation and the GPU alike).
# ---------------------------------------------------------------------------------------------
RUNS = (1, 3, 7, 8, 9, 17, 1024)
D0 = (1, 63, 64, 65, 257)


def run_view(src, run, dense, d0=5):
    """(base, view): d0 rows of `run` contiguous elements, dense or cut from rows 3 wider."""
    b = source(src, (d0, run if dense else run + 3), seed=run)
    return b, (b if dense else b[:, 1:run + 1])


def image_view(src):
    """A 5 x 7 x 3 image permuted to 3 x 5 x 7."""
    b = source(src, (5, 7, 3), seed=7)
    return b, b.transpose(2, 0, 1)


def strided_views(src):
    """[(label, base, view)]: a negative and a zero stride in dimension 0."""
    b, z = source(src, (9, 11), seed=3), source(src, (1, 13), seed=4)
    return [("negative", b, b[::-1, :10]), ("zero", z, np.broadcast_to(z, (6, 13)))]


def three_fields(d0=9):
    """A cast from uint8, a plain float32 field and a cast from float32 to float16: with a
    uint8 -> float16 field of d0 * 3 elements first, the float32 field is padded to 4 and the
    last field starts 2 or 4 mod 16 for the d0 used (checked by the callers)."""
    img, x, w = source("uint8", (d0, 4), 1), source("float32", (d0, 2), 2), source("float32", (d0, 6), 3)
    return [("rgb", img, img[:, :3], cast("uint8", "float16", 1 / 255)),
            ("xy", x, x, None),
            ("w", w, w[:, 1:6], cast("float32", "float16"))]


def tiled_plain_and_cast():
    """A cast from uint8 in front of a plain permuted float32 field that the library's own
    selection tiles (output rows of 260 bytes, 70 elements along the source-contiguous dimension):
    the tile body and the cast body in one launch of gather_cast_kernel."""
    from tests.gather_views import base
    img, b = source("uint8", (9, 5), 5), base(np.float32, (65, 9, 70))
    return [("u", img, img, cast("uint8", "float16", 1 / 255)), ("planes", b, b.transpose(1, 2, 0), None)]


def dst_offsets(dst):
    """Every multiple of the destination element size mod 16."""
    return range(0, 16, 2 if dst == "float16" else 4)


def bases_of(rec):
    return sr.bases_of([(n, b, v) for n, b, v, _ in rec])
