"""Crop records for the tensor-crops tests (dora_gpu_plan_tensor_crop), shared by the CPU plan test,
the host tests, the sanitized host emulation of gather_crop_kernel and the GPU tests: a record is a
list of (field name or None, base array, view of that base, crop or None), a crop a resize of
tests/resize_records.py ({"src", "axes", "size", "mode", "dst"}) with "boxes", a [K, 4] int32 view
of the 1-D int32 array "boxes_base" — one more base of the record, uploaded and addressed like the
frames'.  `want` is the statement of record, `tensor.from_numpy_crops`' values; `same` compares
with it bit for bit except where it is a NaN.

`cases()` is the list every runner goes through: the smallest shapes at which each path of the body
can go wrong."""
import functools
from ctypes import byref, c_int, c_int64, c_uint64, c_void_p, pointer

import numpy as np

from tests import cast_records as cr
from tests import resize_records as rr
from tests import struct_records as sr
from tests.gather_views import describe_view

SOURCES, DESTS, MODES, same = rr.SOURCES, rr.DESTS, rr.MODES, rr.same
dst_name, dests_of, dst_offsets = rr.dst_name, rr.dests_of, rr.dst_offsets
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def boxes_at(rows, mis=0):
    """(base, view): `rows` as a [K, 4] int32 view that starts `mis` bytes (a multiple of 4) into
    a 1-D int32 base."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    base = np.zeros(mis // 4 + rows.size, np.int32)
    view = base[mis // 4:].reshape(-1, 4)
    view[...] = rows
    return base, view


def crop(src, axes, size, rows, mode="bilinear", dst=None, mis=0):
    c = rr.rs(src, axes, size, mode, dst)
    c["boxes_base"], c["boxes"] = boxes_at(rows, mis)
    return c


def want(view, c):
    """The statement of record for `view` under crop `c` (None: the view as it is)."""
    if c is None:
        return np.ascontiguousarray(view)
    from dora_amd import tensor
    return tensor._numpy_crops(view, c["boxes"], c["size"], c["axes"], c["mode"], c["dst"],
                               c["src"] == "bfloat16")


def bases_of(rec):
    """The distinct bases of `rec`, the boxes' among them."""
    return sr.bases_of(triples(rec))


def triples(rec):
    """`rec` as (name, base, view) triples, every crop's boxes one more."""
    out = [(n, b, v) for n, b, v, _ in rec]
    return out + [(f"boxes of {n}", c["boxes_base"], c["boxes"]) for n, _, _, c in rec if c]


def describe(rec, ptr_of):
    """(dora_tensor_field array, dora_tensor_crop array, n, keepalive) of `rec` over `ptr_of`."""
    from dora_amd import tensor
    from dora_amd._lib import TensorCrop
    tensors, keeps = [], []
    for _, b, v, c in rec:
        shape, strides, dtype, off = describe_view(b, v, None)
        t, keep = tensor._describe(ptr_of(b), shape, strides, dtype, off)
        if c is not None and c["src"] == "bfloat16":
            t.dtype_code = SOURCES["bfloat16"][1]
        tensors.append(t)
        keeps.append(keep)
    names = None if len(rec) == 1 and rec[0][0] is None else [x[0] for x in rec]
    lst, keep = tensor._describe_list(names, tensors, tensors[0], 0, 0)
    arr = (TensorCrop * len(rec))()
    for k, (_, _, v, c) in enumerate(rec):
        if c is None:
            continue
        arr[k].mode = MODES[c["mode"]]
        for j in range(2):
            a = c["axes"][j]
            arr[k].axis[j] = a % v.ndim if -v.ndim <= a < v.ndim else a
            arr[k].size[j] = c["size"][j]
        if c["dst"] is not None:
            arr[k].dtype_code, arr[k].dtype_bits = DESTS[c["dst"]]
        bb, bv = c["boxes_base"], c["boxes"]
        shape, strides, dtype, off = describe_view(bb, bv, None)
        bt, bkeep = tensor._describe(ptr_of(bb), shape, strides, dtype, off)
        arr[k].boxes = pointer(bt)
        keeps.append((bt, bkeep))
    return lst.fields, arr, len(rec), (lst, keep, keeps, rec)


def plan_crop(rec, ptr_of, dev):
    """Plan `rec` with dora_gpu_plan_tensor_crop; the Plan keeps the ctypes."""
    from dora_amd import _lib
    from dora_amd.arrow_utils import Plan
    fields, arr, n, keep = describe(rec, ptr_of)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_crop", fields, n, arr, dev, byref(h))
    return Plan(h.value, (fields, arr, keep))


def plan_crops(plan, n, dst=0):
    """The per-field crop descriptors of a device plan of `n` fields (dora_gpu_test_plan_crop) for
    a sample at address `dst`."""
    from dora_amd import _lib
    out = []
    for i in range(n):
        mode, device = c_int(), c_int()
        k, head, units, tail = c_uint64(), c_uint64(), c_uint64(), c_uint64()
        boxes, lo, hi = c_void_p(), c_int64(), c_int64()
        _lib.call("dora_gpu_test_plan_crop", plan.handle, i, dst, byref(mode), byref(k),
                  byref(boxes), byref(device), byref(lo), byref(hi), byref(head), byref(units),
                  byref(tail))
        out.append({"mode": mode.value, "k": k.value, "boxes": boxes.value or 0,
                    "device": device.value, "lo": lo.value, "hi": hi.value, "head": head.value,
                    "units": units.value, "tail": tail.value})
    return out


def oracle(rec):
    """(sample bytes, ArrowTypeInfo, [(offset, length) of each field's leaf]) of the reference
    packing of the materialised record: the nested array of bare crops, else the StructArray of
    the fields."""
    import pyarrow as pa
    from dora_amd import tensor
    from oracle.pack_ref import pack
    cols = [tensor.from_numpy(want(v, c)) for _, _, v, c in rec]
    bare = len(rec) == 1 and rec[0][0] is None
    arr = cols[0] if bare else pa.StructArray.from_arrays(cols, names=[x[0] for x in rec])
    sample, info = pack(arr)
    ranges = []
    for c in ([info] if bare else info.child_data):
        while c.child_data:
            c = c.child_data[0]
        ranges.append((c.buffer_offsets[0].offset, c.buffer_offsets[0].len))
    return sample, info, ranges


# ---------------------------------------------------------------------------------------------
# Boxes
# ---------------------------------------------------------------------------------------------
def box_kinds(ia, ib, size):
    """[(label, row)] over a frame of extents (ia, ib) cropped to `size`: every kind of box the
    statement speaks of."""
    sa, sb = min(size[0], ia), min(size[1], ib)
    return [
        ("whole frame", (0, 0, ia, ib)),
        ("identity extent", (ia - sa, ib - sb, ia, ib)),
        ("1x1", (ia // 2, ib // 2, ia // 2 + 1, ib // 2 + 1)),
        ("over the top", (-3, 1, 3, ib - 1)),
        ("over the bottom", (ia - 2, 1, ia + 5, ib - 1)),
        ("over the left", (1, -4, ia - 1, 2)),
        ("over the right", (1, ib - 3, ia - 1, ib + 100)),
        ("outside above", (-9, 0, -1, ib)),
        ("outside below", (ia, 0, ia + 4, ib)),
        ("outside left", (0, -7, ia, 0)),
        ("outside right", (0, ib + 1, ia, ib + 9)),
        ("inverted a", (ia - 1, 0, 1, ib)),
        ("inverted b", (0, ib - 1, ia, 1)),
        ("zero area a", (2, 0, 2, ib)),
        ("zero area b", (0, 3, ia, 3)),
        ("all zero", (0, 0, 0, 0)),
        ("int32 extremes: the whole frame", (I32_MIN, I32_MIN, I32_MAX, I32_MAX)),
        ("int32 extremes: inverted", (I32_MAX, I32_MAX, I32_MIN, I32_MIN)),
        ("int32 extremes: one row", (I32_MIN, 1, 1, I32_MAX)),
        ("int32 extremes: empty at the far edge", (I32_MAX, 0, I32_MAX, ib)),
    ]


THREE = [(1, 2, 5, 7), (-2, 5, 4, 12), (3, 4, 4, 5)]  # interior, overhanging, 1x1 of a (7, 9) frame

# (label, base shape, view of the base, axes, size): resize_records.GEOMETRY's views under boxes
GEOMETRY = [g for g in rr.GEOMETRY if g[0] in (
    "HWC down coprime", "CHW up coprime", "axes reversed", "permuted HWC -> CHW", "cut",
    "reversed rows", "reversed columns", "broadcast on a resized axis")] + [
    ("7-D", (2, 1, 2, 3, 1, 4, 2), None, (3, 5), (5, 3))]


def boxes_for(ia, ib, seed, k=3):
    """`k` seeded boxes over extents (ia, ib): interior, overhanging and now and then empty."""
    rng = np.random.default_rng(seed)
    lo = np.stack([rng.integers(-3, ia, k), rng.integers(-3, ib, k)], 1)
    ext = np.stack([rng.integers(0, ia + 3, k), rng.integers(0, ib + 3, k)], 1)
    return np.concatenate([lo, lo + ext], 1)


@functools.lru_cache(maxsize=None)
def cases():
    """[(label, record, destination offsets mod 16)]."""
    out = []
    srcs = list(SOURCES)
    # all seven sources x the destinations allowed x both modes: one frame, three boxes
    for i, src in enumerate(srcs):
        b = cr.source(src, (7, 9, 3), seed=i)
        for dst in dests_of(src):
            for mode in MODES:
                out.append((f"{src}->{dst} {mode}",
                            [(None, b, b, crop(src, (0, 1), (5, 4), THREE, mode, dst))], (0,)))
    # geometry and views, both modes, sources and destinations taking turns
    k = 0
    for label, shape, view, axes, size in GEOMETRY:
        for mode in MODES:
            src = srcs[k % len(srcs)]
            dst = dests_of(src)[k % len(dests_of(src))]
            k += 1
            b = cr.source(src, shape, seed=k)
            v = b if view is None else view(b)
            ia, ib = (v.shape[a] for a in axes)
            c = crop(src, axes, size, boxes_for(ia, ib, k), mode, dst)
            out.append((f"{label} {mode} {src}->{dst}", [(None, b, v, c)],
                        (0, 3 * DESTS[dst_name(c)][1] // 8)))
    # every kind of box, each in a message of its own and all of them in one
    b = cr.source("uint8", (8, 10, 3), seed=31)
    f = cr.source("float32", (8, 10), seed=32)
    kinds = box_kinds(8, 10, (4, 6))
    for label, row in kinds:
        out.append((f"box {label}", [(None, b, b, crop("uint8", (0, 1), (4, 6), [row]))], (0,)))
    rows = [row for _, row in kinds]
    out.append(("every box uint8", [(None, b, b, crop("uint8", (0, 1), (4, 6), rows))], (0, 9)))
    out.append(("every box float32->float16 nearest",
                [(None, f, f, crop("float32", (0, 1), (4, 6), rows, "nearest", "float16"))], (0, 6)))
    # K = 1 and K = 0
    out.append(("K = 1", [(None, b, b, crop("uint8", (0, 1), (3, 3), [(1, 1, 6, 8)]))], (0, 5)))
    out.append(("K = 0", [(None, b, b, crop("uint8", (0, 1), (3, 3), []))], (0,)))
    # units across crops: crops of 15 uint8 elements, so units straddle crops — into an empty one
    # (the second) and out of it again
    g = cr.source("uint8", (6, 7), seed=33)
    five = [(0, 0, 6, 7), (2, 2, 2, 5), (1, 1, 5, 6), (-1, 3, 2, 9), (4, 0, 9, 3)]
    for mode in MODES:
        out.append((f"units across crops {mode}",
                    [(None, g, g, crop("uint8", (0, 1), (3, 5), five, mode))], (0, 1, 15)))
    # destinations: every multiple of the destination element size mod 16
    for dst in ("uint8", "int16", "float16", "float32"):
        out.append((f"dst {dst} every misalignment",
                    [(None, b, b, crop("uint8", (0, 1), (3, 5), THREE, "bilinear", dst))],
                    tuple(dst_offsets(dst))))
    # boxes at every multiple of 4 mod 16
    for mis in (0, 4, 8, 12):
        out.append((f"boxes at {mis} mod 16",
                    [(None, b, b, crop("uint8", (0, 1), (2, 3), THREE, "nearest", mis=mis))], (0,)))
    # values: non-finite and subnormal floats, the .5 ties and saturation, through one box each
    for src in ("float16", "bfloat16", "float32"):
        x = rr.special_floats(src)
        for dst in dests_of(src)[:4]:
            for mode in MODES:
                out.append((f"special values {src}->{dst} {mode}",
                            [(None, x, x, crop(src, (0, 1), (7, 9), [(0, 0, 4, 5)], mode, dst))], (0,)))
    t = rr.ties_u8()
    out.append(("ties to even uint8", [(None, t, t, crop("uint8", (0, 1), (2, 4), [(0, 0, 2, 8)]))], (0,)))
    out.append(("ties to even uint8, a box of two pairs",
                [(None, t, t, crop("uint8", (0, 1), (2, 2), [(0, 4, 2, 8)]))], (0,)))
    w = np.array([[300, -5, 70000 // 3, -32768], [255, 256, -129, 127]], np.int16)
    for dst in ("uint8", "int8", "uint16"):
        out.append((f"saturation int16->{dst}",
                    [(None, w, w, crop("int16", (0, 1), (3, 7), [(0, 0, 2, 4)], "bilinear", dst))], (0,)))
    e = np.array([[1e9, -1e9, np.nan], [40000.0, -40000.0, 0.5]], np.float32)
    for dst in ("int16", "uint16", "float16"):
        out.append((f"saturation float32->{dst}",
                    [(None, e, e, crop("float32", (0, 1), (2, 3), [(0, 0, 2, 3)], "nearest", dst))], (0,)))
    out.append(("record", record(), (0, 2, 8)))
    return out


@functools.lru_cache(maxsize=None)
def limit_cases():
    """[(label, record, destination offsets mod 16)] at the edge of the contract, beside `cases()`:
    a frame with an axis of 32768 steps cut by boxes over all of it, its last row, all but its
    first and last row, and the int32 extremes, to crops of 32768 x 1 and of 7 x 2.  None has more
    than 100 000 output elements."""
    n = rr.LIMIT
    b = cr.source("uint8", (n, 3), seed=71)
    inside = [(0, 0, n, 3), (n - 1, 0, n, 3), (1, 0, n - 1, 2)]
    extremes = [(I32_MIN, I32_MIN, I32_MAX, I32_MAX), (I32_MAX, I32_MAX, I32_MIN, I32_MIN),
                (I32_MIN, 1, n - 1, I32_MAX)]
    out = []
    for label, rows in (("boxes over the long axis", inside), ("int32 extremes", extremes)):
        out.append((f"{label} -> ({n}, 1) bilinear",
                    [(None, b, b, crop("uint8", (0, 1), (n, 1), rows, "bilinear"))], (0,)))
    out.append((f"boxes over the long axis -> ({n}, 1) nearest to float16",
                [(None, b, b, crop("uint8", (0, 1), (n, 1), inside, "nearest", "float16"))], (2,)))
    for mode in MODES:
        out.append((f"all six boxes -> (7, 2) {mode}",
                    [(None, b, b, crop("uint8", (0, 1), (7, 2), inside + extremes, mode, mis=4))],
                    (0, 5)))
    return out


def many():
    """[(label, record)]: K = 40 crops of 32 x 32 x 3 uint8 — 7680 units, 30 workgroups — from a
    (70, 90, 3) view cut from a wider base, both modes, by seeded boxes of which 30 overhang the
    frame and 6 are empty."""
    rng = np.random.default_rng(71)
    lo = np.stack([rng.integers(-20, 70, 40), rng.integers(-20, 90, 40)], 1)
    ext = np.stack([rng.integers(-4, 60, 40), rng.integers(-4, 60, 40)], 1)
    rows = np.concatenate([lo, lo + ext], 1)
    b = cr.source("uint8", (72, 96, 3), seed=61)
    return [(f"40 crops {mode}", [(None, b, b[1:71, 2:92], crop("uint8", (0, 1), (32, 32), rows, mode))])
            for mode in MODES]


def record(k=3):
    """A plain int64 field of K rows, the crops, the boxes themselves as a plain field, and a
    second crops field to float16 from another frame by boxes of its own."""
    stamp = np.arange(k, dtype=np.int64) * 1000 + 7
    frame = cr.source("uint8", (9, 11, 3), seed=51)
    c = crop("uint8", (0, 1), (4, 3), boxes_for(9, 11, 5, k))
    other = cr.source("int16", (3, 6, 7), seed=52)
    c2 = crop("int16", (-2, -1), (2, 5), boxes_for(6, 7, 6, k), "nearest", "float16", mis=4)
    return [("stamp", stamp, stamp, None),
            ("crop", frame, frame, c),
            ("box", c["boxes_base"], c["boxes"], None),
            ("map", other, other, c2)]
