"""Affine records for the tensor-affine tests (dora_gpu_plan_tensor_affine), shared by the CPU plan
and host tests, the sanitized host emulation of gather_affine_kernel's body and the GPU tests.  A
record is a list of (field name or None, base array, view of that base, conversion or None, affine
or None): the first four as in tests/quant_records.py (a cast, a quantise or a plain field, the
conversion's "scale" the scalar scale), the affine a dict {"scale": 1-D float32 table or None,
"bias": 1-D float32 table or None, "axis": int or None, "bias_value": float or None}.  `want` is
the statement of record, `tensor.from_numpy_cast` / `tensor.from_numpy_quantize` with `bias` and
`axis`; `same` compares with it bit for bit, nothing exempt but the payload of a NaN in a float
destination."""
from ctypes import byref, c_float, c_int, c_int64, c_uint64, c_void_p, pointer

import numpy as np

from tests import cast_records as cr
from tests import quant_records as qr

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


def imagenet():
    """(scale, bias) of (x / 255 - mean) / std as x * s + b, float32."""
    mean, std = np.array(IMAGENET_MEAN, np.float64), np.array(IMAGENET_STD, np.float64)
    return (1 / (255 * std)).astype(np.float32), (-mean / std).astype(np.float32)


def affine(scale=None, bias=None, axis=None, bias_value=None):
    f = lambda t: None if t is None else np.ascontiguousarray(t, dtype=np.float32)  # noqa: E731
    return {"scale": f(scale), "bias": f(bias), "axis": axis, "bias_value": bias_value}


def table(c, seed, kind="scale"):
    """A table of `c` finite float32 values: inexact factors of both signs, or biases with
    fractions."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal(c) * (3.0 if kind == "bias" else 1.0) + (0.0 if kind == "bias" else 0.37)
    return t.astype(np.float32)


def want(view, c, a):
    """The statement of record for `view` under conversion `c` and affine `a`."""
    if a is None:
        return qr.want(view, c)
    import pyarrow as pa
    from dora_amd import tensor
    view = np.asarray(view)
    scale = a["scale"] if a["scale"] is not None else c["scale"]
    bias = a["bias"] if a["bias"] is not None else a["bias_value"]
    bf = c["src"] == "bfloat16"
    if qr.is_quant(c):
        arr = tensor.from_numpy_quantize(view, c["dst"], scale, c["zp"], bfloat16=bf, bias=bias,
                                         axis=a["axis"])
    else:
        arr = tensor.from_numpy_cast(view, c["dst"], scale, bfloat16=bf, bias=bias, axis=a["axis"])
    while isinstance(arr, pa.FixedSizeListArray):
        arr = arr.flatten()
    return arr.to_numpy(zero_copy_only=False).reshape(view.shape)


same = qr.same


def tables_of(rec):
    """The distinct tables of a record, in order."""
    out = []
    for r in rec:
        for t in ((r[4]["scale"], r[4]["bias"]) if r[4] is not None else ()):
            if t is not None and not any(t is x for x in out):
                out.append(t)
    return out


def describe(rec, ptr_of, tab_ptr_of=None):
    """(fields, casts, quants, affines, n, keepalive) of `rec`: quant_records.describe of its
    first four columns and the dora_tensor_affine entries, a table described over
    `tab_ptr_of(table)` (default: the array's own memory)."""
    from dora_amd import tensor
    from dora_amd._lib import TensorAffine
    fields, casts, quants, n, keep = qr.describe([r[:4] for r in rec], ptr_of)
    affs = (TensorAffine * len(rec))()
    keeps = []
    for k, r in enumerate(rec):
        a = r[4]
        if a is None:
            continue
        for name in ("scale", "bias"):
            t = a[name]
            if t is None:
                continue
            ptr = tab_ptr_of(t) if tab_ptr_of else t.__array_interface__["data"][0]
            d, kp = tensor._describe(ptr, t.shape, [s // t.itemsize for s in t.strides], t.dtype)
            setattr(affs[k], name, pointer(d))
            keeps.append((d, kp, t))
        # (the C entry counts from the front; Python's negative axes are dora_amd.tensor's)
        affs[k].axis = (a["axis"] or 0) % np.asarray(r[2]).ndim if a.get("wrap", True) \
            else a["axis"]
        if a["bias_value"] is not None:
            affs[k].has_bias, affs[k].bias_value = 1, a["bias_value"]
    return fields, casts, quants, affs, n, (keep, keeps)


def plan_affine(rec, ptr_of, dev, tab_ptr_of=None):
    """Plan `rec` with dora_gpu_plan_tensor_affine; the Plan (a context manager) keeps the
    ctypes."""
    from dora_amd import _lib
    from dora_amd.arrow_utils import Plan
    fields, casts, quants, affs, n, keep = describe(rec, ptr_of, tab_ptr_of)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_affine", fields, n, casts, quants, affs, dev, byref(h))
    return Plan(h.value, (fields, casts, quants, affs, keep))


def plan_affines(plan, n):
    """What dora_gpu_test_plan_affine reports of each of the `n` fields of a device plan."""
    from dora_amd import _lib
    out = []
    for i in range(n):
        on, hb = c_int(), c_int()
        st, bt = c_void_p(), c_void_p()
        inner, ch = c_uint64(), c_uint64()
        bias, lo, hi = c_float(), c_int64(), c_int64()
        _lib.call("dora_gpu_test_plan_affine", plan.handle, i, byref(on), byref(st), byref(bt),
                  byref(inner), byref(ch), byref(hb), byref(bias), byref(lo), byref(hi))
        out.append({"affine": bool(on.value), "scale": st.value or 0, "bias": bt.value or 0,
                    "inner": inner.value, "channels": ch.value, "has_bias": bool(hb.value),
                    "bias_value": bias.value, "lo": lo.value, "hi": hi.value})
    return out


def oracle(rec):
    """(sample bytes, ArrowTypeInfo, [(offset, length) of each field's leaf]) of the reference
    packing of the materialised converted record."""
    import pyarrow as pa
    from dora_amd import tensor
    from oracle.pack_ref import pack
    cols = [tensor.from_numpy(want(v, c, a)) for _, _, v, c, a in rec]
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
# Shapes: the smallest at which the channel stepping can go wrong.
# ---------------------------------------------------------------------------------------------
CHANNELS = (1, 3, 4, 5, 17)
INNERS = (3, 7, 16, 17, 35)
CONVS = (cr.cast("uint8", "float16"), cr.cast("float32", "float32"), cr.cast("float16", "float32"),
         qr.quant("float32", "int8", None, -7), qr.quant("uint8", "uint8", None, 3),
         qr.quant("int16", "uint16", None, 100))


def conv_label(c):
    return f"{c['src']}->{c['dst']}"


def dst_offsets(c):
    """Every multiple of the destination element size mod 16."""
    return range(0, 16, np.dtype(c["dst"]).itemsize)


def _bare(b, v, c, a):
    return [(None, b, v, c, a)]


def both(c, axis, seed=0):
    return affine(table(c, seed), table(c, seed + 1, "bias"), axis)


def shape_cases(conv):
    """[(label, record)] of bare tensors of conv's source under `conv` with per-channel tables."""
    src = conv["src"]
    out = []
    for c in CHANNELS:
        # axis innermost: inner = 1, a 16-element unit wraps C several times
        for dense in (True, False):
            b = cr.source(src, (6, c if dense else c + 3), seed=c)
            v = b if dense else b[:, 1:c + 1]
            out.append((f"innermost C={c} dense={dense}", _bare(b, v, conv, both(c, -1, c))))
    for inner in INNERS:
        # axis outermost: units that cross one or several channel boundaries, and ones that cross none
        for dense in (True, False):
            b = cr.source(src, (4, inner if dense else inner + 3), seed=inner)
            v = b if dense else b[:, 1:inner + 1]
            out.append((f"outermost inner={inner} dense={dense}", _bare(b, v, conv, both(4, 0, inner))))
    b = cr.source(src, (3, 5, 2, 3), seed=21)
    out.append(("middle axis of 4-D", _bare(b, b, conv, both(5, 1, 5))))
    out.append(("middle axis of 4-D, cut", _bare(b, b[:, :, :, 1:], conv, both(2, 2, 6))))
    b, v = cr.image_view(src)  # 5 x 7 x 3 permuted to 3 x 5 x 7
    out.append(("image chw axis=0", _bare(b, v, conv, both(3, 0, 7))))
    out.append(("image hwc axis=-1", _bare(b, b, conv, both(3, -1, 8))))
    for label, b, v in cr.strided_views(src):
        out.append((f"{label} stride", _bare(b, v, conv, both(v.shape[1], 1, 9))))
        out.append((f"{label} stride, axis 0", _bare(b, v, conv, both(v.shape[0], 0, 10))))
    return out


def mode_cases(conv):
    """Scale table only, bias table only, both, and a table with a scalar of the other kind."""
    src = conv["src"]
    b = cr.source(src, (5, 3, 7), seed=31)
    v = b[:, :, 1:6]
    s, t = table(3, 40), table(3, 41, "bias")
    scaled = dict(conv, scale=0.5)
    return [("scale table only", _bare(b, v, conv, affine(s, None, 1))),
            ("bias table only", _bare(b, v, conv, affine(None, t, 1))),
            ("bias table, scalar scale", _bare(b, v, scaled, affine(None, t, 1))),
            ("scale table, scalar bias", _bare(b, v, conv, affine(s, None, 1, 0.75))),
            ("both", _bare(b, v, conv, affine(s, t, 1))),
            ("scalar bias alone", _bare(b, v, scaled, affine(bias_value=-1.25)))]


def short_totals(conv):
    """3 elements (fewer than the head) at the last element slots of a 16-byte line, C = 3."""
    b = cr.source(conv["src"], (3,), seed=5)
    ds = np.dtype(conv["dst"]).itemsize
    return 16 - ds, _bare(b, b, conv, both(3, 0, 11))


def mixed_record(d0=9):
    """An affine cast, an affine quantise, a plain field and a scalar cast in one record."""
    img, f, x, w = (cr.source("uint8", (d0, 5, 3), 1), cr.source("float16", (d0, 17), 2),
                    cr.source("float32", (d0, 2), 3), cr.source("float32", (d0, 6), 4))
    s, b = imagenet()
    return [("image", img, img[:, 1:4], cr.cast("uint8", "float16"), affine(s, b, -1)),
            ("act", f, f, qr.quant("float16", "int8", None, 0), affine(table(17, 50), None, 1)),
            ("xy", x, x, None, None),
            ("w", w, w[:, 1:6], cr.cast("float32", "float16", 0.5), None)]
