"""Model-input records for the tensor-prep tests (dora_gpu_plan_tensor_prep), shared by the CPU plan
test, the host tests, the sanitized host emulation of gather_resize_prep_kernel and
gather_crop_prep_kernel and the GPU tests: a record is a list of (field name or None, base array,
view of that base, op or None), an op a resize of tests/resize_records.py or a crop of
tests/crop_records.py (it has "boxes") with one more key, "prep": None or a dict {"scale", "bias":
None, a number or a (base, view) pair of float32 arrays — a per-channel table, one more base of the
record; "axis"; "inner", "lead": None or two integers each; "fill"}.  `want` is the statement of
record, `tensor.from_numpy_resize`'s or `tensor.from_numpy_crops`' values; `same` compares with it
bit for bit except where it is a NaN.

`cases()` is the list every runner goes through: the smallest shapes at which each path of the body
can go wrong."""
import functools
from ctypes import byref, c_float, c_int, c_int64, c_uint64, c_void_p, pointer

import numpy as np

from tests import cast_records as cr
from tests import crop_records as kr
from tests import resize_records as rr
from tests import struct_records as sr
from tests.gather_views import describe_view

SOURCES, DESTS, MODES, same = rr.SOURCES, rr.DESTS, rr.MODES, rr.same
dst_name = rr.dst_name
LIMIT = 32768
# destination element size -> the offsets mod 16 a case of that size is packed at: 0 and two
# others, so that heads of different lengths, whole units and tails all run
OFFSETS = {1: (0, 5, 11), 2: (0, 6, 14), 4: (0, 4, 12)}


def table(values, lead=1):
    """(base, view): `values` as a float32 table that starts `lead` words into its base and ends
    with it — tight against the end of its allocation."""
    values = np.asarray(values, np.float32).reshape(-1)
    base = np.zeros(lead + values.size, np.float32)
    base[lead:] = values
    return base, base[lead:]


def prep(scale=None, bias=None, axis=None, inner=None, lead=None, fill=0.0):
    return {"scale": scale, "bias": bias, "axis": axis, "inner": inner, "lead": lead, "fill": fill}


def resized(src, axes, size, mode="bilinear", dst=None, **kw):
    op = rr.rs(src, axes, size, mode, dst)
    op["prep"] = prep(**kw) if kw else None
    return op


def cropped(src, axes, size, rows, mode="bilinear", dst=None, mis=0, **kw):
    op = kr.crop(src, axes, size, rows, mode, dst, mis)
    op["prep"] = prep(**kw) if kw else None
    return op


def is_table(v):
    return isinstance(v, tuple)


def term(v):
    """A scale or a bias as the statement takes it."""
    return v[1] if is_table(v) else v


def offsets_of(op):
    return OFFSETS[DESTS[dst_name(op)][1] // 8]


def statement_kwargs(op):
    """The keyword arguments of `tensor.resize` / `from_numpy_resize` (`crops` / `.._crops`) that
    `op`'s prep stands for."""
    p = op.get("prep")
    if not p:
        return {}
    kw = {"scale": term(p["scale"]), "bias": term(p["bias"]), "axis": p["axis"]}
    if p["inner"] is not None:
        kw.update(inner=p["inner"], lead=p["lead"] or (0, 0), fill=p["fill"])
    return kw


def want(view, op):
    """The statement of record for `view` under `op` (None: the view as it is)."""
    if op is None:
        return np.ascontiguousarray(view)
    from dora_amd import tensor
    kw = statement_kwargs(op)
    if "boxes" in op:
        return tensor._numpy_crops(view, op["boxes"], op["size"], op["axes"], op["mode"],
                                   op["dst"], op["src"] == "bfloat16", **kw)
    return tensor._numpy_resize(view, op["size"], op["axes"], op["mode"], op["dst"],
                                op["src"] == "bfloat16", **kw)


def oracle(rec):
    """(sample bytes, ArrowTypeInfo, [(offset, length) of each field's leaf]) of the reference
    packing of the materialised record: the nested array of a bare tensor, else the StructArray of
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


def tables_of(op):
    """[(what, base, view)] of the tables of `op`."""
    p = (op or {}).get("prep") or {}
    return [(w, *p[w]) for w in ("scale", "bias") if is_table(p.get(w))]


def triples(rec):
    """`rec` as (name, base, view) triples, every crop's boxes and every table one more."""
    out = [(n, b, v) for n, b, v, _ in rec]
    out += [(f"boxes of {n}", c["boxes_base"], c["boxes"]) for n, _, _, c in rec
            if c and "boxes" in c]
    return out + [(f"{w} of {n}", b, v) for n, _, _, c in rec for w, b, v in tables_of(c)]


def bases_of(rec):
    """The distinct bases of `rec`, the boxes' and the tables' among them."""
    return sr.bases_of(triples(rec))


def describe(rec, ptr_of):
    """(dora_tensor_field array, dora_tensor_resize array or None, dora_tensor_crop array or None,
    dora_tensor_prep array, n, keepalive) of `rec` over `ptr_of`."""
    from dora_amd import tensor
    from dora_amd._lib import TensorCrop, TensorPrep, TensorResize
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
    crops = any(c and "boxes" in c for _, _, _, c in rec)
    arr = ((TensorCrop if crops else TensorResize) * len(rec))()
    parr = (TensorPrep * len(rec))()

    def pointer_to(base, view):
        shape, strides, dtype, off = describe_view(base, view, None)
        t, tkeep = tensor._describe(ptr_of(base), shape, strides, dtype, off)
        keeps.append((t, tkeep))
        return pointer(t)
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
        if crops:
            arr[k].boxes = pointer_to(c["boxes_base"], c["boxes"])
        p = c.get("prep")
        if not p:
            continue
        a = parr[k]
        if is_table(p["scale"]):
            a.scale = pointer_to(*p["scale"])
        elif p["scale"] is not None:
            a.has_scale, a.scale_value = 1, p["scale"]
        if is_table(p["bias"]):
            a.bias = pointer_to(*p["bias"])
        elif p["bias"] is not None:
            a.has_bias, a.bias_value = 1, p["bias"]
        if p["axis"] is not None:
            a.axis = p["axis"] % v.ndim if -v.ndim <= p["axis"] < v.ndim else p["axis"]
        if p["inner"] is not None:
            a.inner[0], a.inner[1] = p["inner"]
            a.lead[0], a.lead[1] = p["lead"] or (0, 0)
            a.fill = p["fill"]
    return (lst.fields, None if crops else arr, arr if crops else None, parr, len(rec),
            (lst, keep, keeps, rec))


def plan_prep(rec, ptr_of, dev):
    """Plan `rec` with dora_gpu_plan_tensor_prep; the Plan keeps the ctypes."""
    from dora_amd import _lib
    from dora_amd.arrow_utils import Plan
    fields, rarr, carr, parr, n, keep = describe(rec, ptr_of)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_prep", fields, n, rarr, carr, parr, dev, byref(h))
    return Plan(h.value, (fields, rarr, carr, parr, keep))


def plan_preps(plan, n):
    """The per-field prep descriptors of a device plan of `n` fields (dora_gpu_test_plan_prep)."""
    from dora_amd import _lib
    out = []
    for i in range(n):
        on, axis = c_int(), c_int()
        st, bt, ch = c_void_p(), c_void_p(), c_uint64()
        inner, lead, fill = (c_int64 * 2)(), (c_int64 * 2)(), c_float()
        lo, hi = c_int64(), c_int64()
        _lib.call("dora_gpu_test_plan_prep", plan.handle, i, byref(on), byref(st), byref(bt),
                  byref(ch), byref(axis), inner, lead, byref(fill), byref(lo), byref(hi))
        out.append({"on": on.value, "scale_table": st.value or 0, "bias_table": bt.value or 0,
                    "channels": ch.value, "axis": axis.value, "inner": tuple(inner),
                    "lead": tuple(lead), "fill": fill.value, "lo": lo.value, "hi": hi.value})
    return out


def plan_launch(plan):
    """dora_gpu_test_plan_launch's launch kind: 9 gather_resize_prep_kernel, 10
    gather_crop_prep_kernel."""
    from dora_amd import _lib
    launch, scan, checked = c_int(), c_int(), c_int()
    _lib.call("dora_gpu_test_plan_launch", plan.handle, byref(launch), byref(scan), byref(checked))
    return launch.value


# ---------------------------------------------------------------------------------------------
# Cases
# ---------------------------------------------------------------------------------------------
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)


def norm_tables():
    """(scale, bias) tables of (x / 255 - mean[c]) / std[c] as x * S[c] + B[c]."""
    s = [1.0 / (255.0 * d) for d in STD]
    b = [-m / d for m, d in zip(MEAN, STD)]
    return table(s), table(b, lead=3)


def letterboxed(view, axes, size):
    from dora_amd import tensor
    return tensor.letterbox(tuple(view.shape[a] for a in axes), size)


FOUR = [(1, 2, 5, 7), (2, 3, 2, 9), (-2, 5, 4, 14), (7, 0, 1, 10)]  # interior, empty, overhanging, inverted


@functools.lru_cache(maxsize=None)
def cases():
    """[(label, record, destination offsets mod 16)]."""
    out = []

    def add(label, rec):
        op = next(c for _, _, _, c in rec if c is not None)
        out.append((label, rec, offsets_of(op)))
    srcs, dsts = list(SOURCES), list(DESTS)
    # all seven sources, all six destinations, both modes: an HWC image, table scale + scalar bias
    for i, src in enumerate(srcs):
        b = cr.source(src, (7, 9, 3), seed=i)
        for j, mode in enumerate(MODES):
            dst = dsts[(i + 3 * j) % len(dsts)]
            add(f"{src}->{dst} {mode}",
                [(None, b, b, resized(src, (0, 1), (5, 4), mode, dst, scale=table([0.5, -1.25, 2.0]),
                                      bias=0.75, axis=2))])
    # normalise into the source's own integer dtype (the quantised conversion)
    u = cr.source("uint8", (7, 9, 3), seed=11)
    add("uint8 -> its own dtype", [(None, u, u, resized("uint8", (0, 1), (5, 4), scale=0.5, bias=3.0))])
    # the forms of scale and bias
    s3, b3 = norm_tables()
    for label, kw in (("scalar scale only", dict(scale=1 / 255)),
                      ("scalar bias only", dict(bias=-7.5)),
                      ("table scale + scalar bias", dict(scale=s3, bias=-0.5, axis=2)),
                      ("scalar scale + table bias", dict(scale=0.25, bias=b3, axis=-1)),
                      ("both tables", dict(scale=s3, bias=b3, axis=2))):
        for mode in MODES:
            add(f"{label} {mode}", [(None, u, u, resized("uint8", (0, 1), (5, 4), mode, "float16", **kw))])
    # where the tables' axis lies: leading (a permuted view of HWC), in the middle, last
    add("axis leading", [(None, u, u.transpose(2, 0, 1),
                          resized("uint8", (-2, -1), (5, 4), "bilinear", "float16", scale=s3, bias=b3, axis=0))])
    m = cr.source("int16", (5, 3, 6), seed=12)
    add("axis in the middle", [(None, m, m, resized("int16", (0, 2), (3, 8), "bilinear", "float32",
                                                     scale=table([2.0, -1.0, 0.5]), bias=b3, axis=1))])
    add("axis last", [(None, u, u, resized("uint8", (0, 1), (6, 11), "nearest", "float32",
                                           scale=s3, bias=b3, axis=-1))])
    # letterbox: a view tight against the end of its base, the border inside a 16-byte unit
    base = cr.source("uint8", (13, 20, 3), seed=13)
    cut = base[2:, 3:]
    inner, lead = letterboxed(cut, (0, 1), (16, 16))
    assert (inner, lead) == ((10, 16), (3, 0))
    for mode in MODES:
        add(f"letterbox HWC uint8 {mode}",
            [(None, base, cut, resized("uint8", (0, 1), (16, 16), mode, None, inner=inner, lead=lead,
                                       fill=114.0, scale=0.5, bias=1.0))])
    chw = cut.transpose(2, 0, 1)
    inner, lead = letterboxed(chw, (-2, -1), (16, 15))
    for mode in MODES:
        add(f"letterbox CHW float16 odd rows {mode}",
            [(None, base, chw, resized("uint8", (-2, -1), (16, 15), mode, "float16", inner=inner,
                                       lead=lead, fill=114.0, scale=s3, bias=b3, axis=0))])
    # explicit placement: padding on all four sides; the image filling the output; a placement
    # with no affine step at all
    add("padding on four sides", [(None, u, u, resized("uint8", (0, 1), (12, 14), "bilinear", "float32",
                                                       inner=(6, 7), lead=(2, 3), fill=-2.5, scale=s3,
                                                       bias=b3, axis=2))])
    add("inner == size", [(None, u, u, resized("uint8", (0, 1), (5, 4), "bilinear", "float16",
                                               inner=(5, 4), lead=(0, 0), fill=9.0, bias=0.5))])
    add("placement alone", [(None, u, u, resized("uint8", (1, 0), (6, 8), "nearest", "int16",
                                                 inner=(1, 8), lead=(5, 0), fill=-7.0))])
    # fills: saturating an integer destination, and -0.0 whose sign the product keeps
    add("fill saturates uint8", [(None, u, u, resized("uint8", (0, 1), (8, 6), "bilinear", "uint8",
                                                      inner=(5, 4), lead=(1, 2), fill=300.0, scale=2.0))])
    add("fill saturates int16", [(None, m, m, resized("int16", (0, 2), (7, 8), "nearest", "int16",
                                                      inner=(3, 8), lead=(4, 0), fill=-1e6, bias=1.0))])
    for dst in ("float16", "float32"):
        add(f"fill -0.0 -> {dst}", [(None, u, u, resized("uint8", (0, 1), (8, 6), "nearest", dst,
                                                         inner=(5, 4), lead=(3, 1), fill=-0.0, scale=3.0))])
    # values: non-finite and subnormal floats through both terms; exact .5 ties after the step
    for i, src in enumerate(("float16", "bfloat16", "float32")):
        x = rr.special_floats(src)
        x = np.stack([x, x[::-1, ::-1], x[:, ::-1], x[::-1]])  # (4, 4, 5): four channels of them
        for j, mode in enumerate(MODES):
            dst = ("float16", "float32", "int16", "uint8")[(2 * i + j) % 4]
            add(f"special values {src}->{dst} {mode}",
                [(None, x, x, resized(src, (1, 2), (7, 9), mode, dst, scale=table([1.0, -0.0, 0.5, 2.0 ** -20]),
                                      bias=table([0.0, -0.0, 1e-40, -3.0], lead=2), axis=0,
                                      inner=(6, 7), lead=(1, 1), fill=-0.0))])
    odd = np.arange(1, 65, dtype=np.uint8).reshape(8, 8)
    for dst in ("uint8", "int8", "int16"):
        add(f"ties to even after the step -> {dst}",
            [(None, odd, odd, resized("uint8", (0, 1), (8, 8), "nearest", dst, scale=0.5))])
    add("ties to even after the bias",
        [(None, odd, odd, resized("uint8", (0, 1), (4, 8), "nearest", "uint8", bias=-0.5))])
    # crops: K = 4 — interior, empty (zeros despite a bias), overhanging, inverted — with tables
    f = cr.source("uint8", (8, 10, 3), seed=14)
    for mode in MODES:
        for dst in ("float16", "uint8"):
            add(f"four crops {mode} -> {dst}",
                [(None, f, f, cropped("uint8", (0, 1), (4, 6), FOUR, mode, dst, scale=s3, bias=b3, axis=2))])
    add("four crops, axis leading", [(None, f, f.transpose(2, 0, 1),
                                      cropped("uint8", (-2, -1), (3, 5), FOUR, "bilinear", "float32", mis=4,
                                              scale=table([1.0, 2.0, 3.0]), bias=100.0, axis=0))])
    # a unit that spans two crops: crops of 15 uint8 elements, the second empty, a scalar bias
    g = cr.source("uint8", (6, 7), seed=15)
    five = [(0, 0, 6, 7), (2, 2, 2, 5), (1, 1, 5, 6), (-1, 3, 2, 9), (4, 0, 9, 3)]
    for mode in MODES:
        out.append((f"units across crops {mode}",
                    [(None, g, g, cropped("uint8", (0, 1), (3, 5), five, mode, scale=0.5, bias=9.0))],
                    (0, 1, 15)))
    out.append(("record of a resize", resize_record(), (0, 2, 8)))
    out.append(("record of crops", crops_record(), (0, 2, 8)))
    return out


def resize_record():
    """A prepped field between plain fields, and a resized field without a prep entry behind
    them: leading extent 5."""
    s3, b3 = norm_tables()
    stamp = np.arange(5, dtype=np.int64) * 1000 + 7
    frame = cr.source("uint8", (9, 11, 3), seed=51)
    inner, lead = letterboxed(frame, (0, 1), (5, 8))
    wide = cr.source("int16", (6, 4), seed=52)
    other = cr.source("float32", (3, 6), seed=53)
    return [("stamp", stamp, stamp, None),
            ("image", frame, frame, resized("uint8", (0, 1), (5, 8), "bilinear", "float16", inner=inner,
                                            lead=lead, fill=114.0, scale=s3, bias=b3, axis=2)),
            ("tail", wide, wide[:5, ::2], None),
            ("map", other, other, resized("float32", (0, 1), (5, 2), "nearest", "int8"))]


def crops_record(k=3):
    """The crops normalised through `permute(2, 0, 1)` next to the boxes themselves as a plain
    field and a stamp: leading extent K."""
    stamp = np.arange(k, dtype=np.int64) * 1000 + 7
    frame = cr.source("uint8", (9, 11, 3), seed=54)
    c = cropped("uint8", (-2, -1), (4, 3), kr.boxes_for(9, 11, 5, k), "bilinear", "float16",
                scale=table([0.5, 0.25, 2.0]), bias=table([-1.0, 0.0, 1.0], lead=2), axis=0)
    return [("stamp", stamp, stamp, None),
            ("crop", frame, frame.transpose(2, 0, 1), c),
            ("box", c["boxes_base"], c["boxes"], None)]


@functools.lru_cache(maxsize=None)
def limit_cases():
    """[(label, record, destination offsets mod 16)] at the edge of the contract: an output axis of
    32768 steps whose image ends with it, lead + inner == 32768."""
    b = cr.source("uint8", (5, 3), seed=71)
    out = []
    for mode, inner, lead in (("bilinear", (LIMIT - 768, 1), (768, 1)), ("nearest", (1, 2), (LIMIT - 1, 0))):
        out.append((f"({LIMIT}, 2) {mode}, the image from {lead[0]} to the end",
                    [(None, b, b, resized("uint8", (0, 1), (LIMIT, 2), mode, "uint8", inner=inner,
                                          lead=lead, fill=114.0, scale=0.5, bias=1.0))], (0, 3)))
    return out


def many():
    """[(label, record)]: a (70, 90, 3) uint8 frame letterboxed into 300 x 300 with tables — 16875
    units, 66 workgroups — HWC to uint8 and through `permute(2, 0, 1)` to float16."""
    s3, b3 = norm_tables()
    b = cr.source("uint8", (72, 96, 3), seed=61)
    v = b[1:71, 2:92]
    inner, lead = letterboxed(v, (0, 1), (300, 300))
    return [("letterbox 300 x 300 HWC uint8",
             [(None, b, v, resized("uint8", (0, 1), (300, 300), "bilinear", "uint8", inner=inner, lead=lead,
                                   fill=114.0, scale=table([0.5, 1.0, 0.25]), bias=b3, axis=2))]),
            ("letterbox 300 x 300 CHW float16",
             [(None, b, v.transpose(2, 0, 1),
               resized("uint8", (-2, -1), (300, 300), "bilinear", "float16", inner=inner, lead=lead,
                       fill=114.0, scale=s3, bias=b3, axis=0))])]
