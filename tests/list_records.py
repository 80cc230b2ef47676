"""Ragged batches for the tensor-list tests (dora_gpu_plan_tensor_list), shared by the CPU plan
test, the host dataflow test and the GPU tests: each record is a list of (field name, base array,
view of that base) as in tests/struct_records.py — a name of None marks the one bare tensor — and
the helpers cut its N rows into lists, describe values and partition over any memory, plan them,
and give the reference packing of pa.ListArray.from_arrays(offsets, child)."""
from ctypes import byref, c_int, c_int64, c_uint64, c_void_p

import numpy as np

from tests import struct_records as sr
from tests.gather_views import base, describe_view


def bare(n):
    """A bare tensor child: (n, 4) float32 cut from (n, 6)."""
    b = base(np.float32, (n, 6))
    return [(None, b, b[:, :4])]


def clouds(n):
    """The C3-shaped record: x, y, z columns of one (n, 3) float32 base (element-strided) and a
    dense uint8 intensity."""
    p, i = base(np.float32, (n, 3)), base(np.uint8, (n,))
    return [("x", p, p[:, 0]), ("y", p, p[:, 1]), ("z", p, p[:, 2]), ("intensity", i, i)]


def f64_first(n):
    """A record whose first leaf is float64: behind an offsets buffer of 4 * odd bytes it starts
    after 4 bytes of padding."""
    t, k = base(np.float64, (n, 2)), base(np.int16, (n, 3))
    return [("t", t, t[:, 1]), ("k", k, k)]


def detector(n):
    return sr.detector(n, cls=True)


RECORDS = {"bare": bare, "clouds": clouds, "f64_first": f64_first, "detector": detector}


def partitions(n):
    """Lengths that cut n rows: B in {1, 2, 16} with empty lists at the front, in the middle and
    at the end; for n == 0 also B == 0 and B == 3."""
    if n == 0:
        return [[], [0], [0, 0, 0]]
    assert n >= 13
    sixteen = [0, 0, 1, 2, 3, 0, 0, 4, 1, 1, 0, 1, 0, 0, 0, 0]
    sixteen[7] += n - sum(sixteen)
    sixteen[15] = 0
    return [[n], [0, n], [n, 0], [n // 2, n - n // 2], sixteen]


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))]).astype(np.int64)


def child_of(rec):
    import pyarrow as pa
    from dora_amd import tensor
    if rec[0][0] is None:
        return tensor.from_numpy(rec[0][2])
    return pa.StructArray.from_arrays([tensor.from_numpy(v) for _, _, v in rec],
                                      names=[name for name, _, _ in rec])


def oracle(rec, offsets):
    """(sample bytes, ArrowTypeInfo, [(offset, length) of each field's leaf]) of the reference
    packing of the ListArray of `rec` cut at `offsets`."""
    import pyarrow as pa
    from oracle.pack_ref import pack
    arr = pa.ListArray.from_arrays(pa.array(np.asarray(offsets), pa.int32()), child_of(rec))
    sample, info = pack(arr)
    kids = [info.child_data[0]] if rec[0][0] is None else info.child_data[0].child_data
    ranges = []
    for c in kids:
        while c.child_data:
            c = c.child_data[0]
        ranges.append((c.buffer_offsets[0].offset, c.buffer_offsets[0].len))
    return sample, info, ranges


def describe_values(rec, ptr_of):
    from dora_amd import tensor
    tensors, keeps = [], []
    for _, b, v in rec:
        shape, strides, dtype, off = describe_view(b, v, None)
        t, keep = tensor._describe(ptr_of(b), shape, strides, dtype, off)
        tensors.append(t)
        keeps.append(keep)
    names = None if rec[0][0] is None else [name for name, _, _ in rec]
    return names, tensors, keeps


def plan_list(rec, ptr_of, dev, part, form, part_dev, part_ptr=None):
    """Plan `rec` (fields over `ptr_of(base)`) cut by the numpy array `part` (lengths or offsets
    as `form` says), which lives at `part_ptr` (default: where numpy holds it) on `part_dev`."""
    from dora_amd import _lib, tensor
    from dora_amd.arrow_utils import Plan
    names, tensors, keeps = describe_values(rec, ptr_of)
    part = np.ascontiguousarray(part)
    ptr = part.__array_interface__["data"][0] if part_ptr is None else part_ptr
    pt, pkeep = tensor._describe(ptr, part.shape, None, part.dtype)
    lst, keep = tensor._describe_list(names, tensors, pt, form, part_dev)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_list", byref(lst), dev, byref(h))
    return Plan(h.value, (lst, keep, keeps, pkeep, part, rec))


def plan_scan(plan):
    """dora_gpu_test_plan_list of a ragged-batch plan."""
    from dora_amd import _lib
    scan, wide, form = c_int(), c_int(), c_int()
    src, count, rows, prefix = c_void_p(), c_uint64(), c_uint64(), c_uint64()
    lo, hi = c_int64(), c_int64()
    _lib.call("dora_gpu_test_plan_list", plan.handle, byref(scan), byref(src), byref(count),
              byref(wide), byref(form), byref(rows), byref(lo), byref(hi), byref(prefix))
    return {"scan": bool(scan.value), "src": src.value or 0, "count": count.value,
            "wide": bool(wide.value), "offsets": bool(form.value), "rows": rows.value,
            "lo": lo.value, "hi": hi.value, "prefix": prefix.value}


def clamped_offsets(words, offsets_form, n):
    """What the scan share writes for device words, stated in numpy: from lengths
    o[i] = min(n, sum_{j<i} max(len_j, 0)), from offsets o[i] = min(n, max(0, max_{j<=i} in_j))."""
    w = np.asarray(words).astype(object)  # exact integers: no wrap-around in the statement
    if offsets_form:
        run, out = 0, []
        for v in w:
            run = max(run, v)
            out.append(min(n, max(0, run)))
        return np.array(out, dtype=np.int32)
    total, out = 0, [0]
    for v in w:
        total += max(v, 0)
        out.append(min(n, total))
    return np.array(out, dtype=np.int32)
