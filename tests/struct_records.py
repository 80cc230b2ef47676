"""Records of tensors for the struct-of-tensors tests (dora_gpu_plan_tensor_struct), shared by
the CPU plan test, the sanitized host emulation of gather_struct_kernel and the GPU tests: each
record is a list of (field name, base array, view of that base) whose views share shape[0], and
the helpers describe it over any memory holding the bases' bytes, plan it, and read the plan's
per-field descriptors back through the testing library."""
from ctypes import byref, c_int, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

import numpy as np

from tests.gather_views import base, describe_view


def detector(n, cls=False):
    """The detector record: `bbox` rows of 16 bytes cut from a (n, 6) float32 base (a strided rows
    field), `conf` every twelfth float16 of the same base (element-strided), `label` a dense int64
    column, `rgb` (n, 3) cut from a (n, 4) uint8 base; with `cls`, the bytes left over in that
    base as a fifth field, whose offset in the sample is odd when n is."""
    out, img, lab = base(np.float32, (n, 6)), base(np.uint8, (n, 4)), base(np.int64, (n,))
    rec = [("bbox", out, out[:, :4]), ("conf", out, out.view(np.float16)[:, 8]),
           ("label", lab, lab), ("rgb", img, img[:, :3])]
    if cls:
        rec.append(("cls", img, img[:, 3]))
    return rec


def permuted_and_bytes():
    """A permuted field the tile body applies to (a partial tile on every edge: its 33 x 40 merge,
    a 67 x 1320 (c, j) plane) next to 67 single bytes, a field with no whole 16-byte unit at the
    misaligned destinations.  The library's own selection takes the rows body for the first
    (its output rows are 160 bytes, below the tile's threshold); forced, it is tiled."""
    b, u = base(np.float32, (33, 40, 67)), base(np.uint8, (67,))
    return [("chw", b, b.transpose(2, 0, 1)), ("tag", u, u)]


def tile_selected():
    """A permuted field the library's own selection tiles (output rows of 260 bytes, 70 elements
    along the source-contiguous dimension) next to a dense float64 column: two kinds of body in
    one launch without forcing either."""
    b, d = base(np.float32, (65, 9, 70)), base(np.float64, (9,))
    return [("planes", b, b.transpose(1, 2, 0)), ("t", d, d)]


def eight_fields():
    """The maximum field count: element sizes 1, 2, 4 and 8 twice over, field k of shape
    (9, k + 1), the even ones cut from a wider base and the odd ones dense; every field's share
    of the grid is one workgroup."""
    rec = []
    for k, dt in enumerate([np.uint8, np.int16, np.float32, np.float64, np.int8, np.uint16,
                            np.int32, np.int64]):
        b = base(dt, (9, k + 2 if k % 2 == 0 else k + 1))
        rec.append((f"f{k}", b, b[:, :k + 1]))
    return rec


def negative_and_broadcast():
    """A field with negative and stepped strides and a broadcast (zero-stride) one, d0 = 9."""
    b, f = base(np.int16, (9, 10)), base(np.float32, (1, 5))
    return [("rev", b, b[::-1, ::2]), ("same", f, np.broadcast_to(f, (9, 5)))]


RECORDS = {
    "detector_67": lambda: detector(67, cls=True),
    "permuted_and_bytes": permuted_and_bytes,
    "tile_selected": tile_selected,
    "eight_fields": eight_fields,
    "negative_and_broadcast": negative_and_broadcast,
}


def bases_of(rec):
    """The distinct base arrays of a record, by identity, in first-use order."""
    out = []
    for _, b, _ in rec:
        if not any(b is x for x in out):
            out.append(b)
    return out


def plan_record(rec, ptr_of, dev):
    """Plan `rec` with each field described over `ptr_of(base)`; the Plan keeps the ctypes."""
    from dora_amd import _lib, tensor
    from dora_amd.arrow_utils import Plan
    tensors, keeps = [], []
    for _, b, v in rec:
        shape, strides, dtype, off = describe_view(b, v, None)
        t, keep = tensor._describe(ptr_of(b), shape, strides, dtype, off)
        tensors.append(t)
        keeps.append(keep)
    fields, keep = tensor._describe_fields([name for name, _, _ in rec], tensors)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_struct", fields, len(rec), dev, byref(h))
    return Plan(h.value, (fields, keep, keeps, rec))


def plan_fields(plan, dst=0):
    """The per-field descriptors of a device struct plan (dora_gpu_test_plan_field), `kind` as
    the current selection gives it for a sample at address `dst`."""
    from dora_amd import _lib
    out, i = [], 0
    while True:
        n, g, off, nbytes, kind = c_size_t(), c_int(), c_uint64(), c_uint64(), c_int()
        src, nd, row, elem = c_void_p(), c_int(), c_uint64(), c_uint32()
        shp, std, lo, hi = (c_int64 * 8)(), (c_int64 * 8)(), c_int64(), c_int64()
        _lib.call("dora_gpu_test_plan_field", plan.handle, i, dst, byref(n), byref(g), byref(off),
                  byref(nbytes), byref(kind), byref(src), byref(nd), byref(row), byref(elem), shp,
                  std, byref(lo), byref(hi))
        out.append({"gather": bool(g.value), "off": off.value, "bytes": nbytes.value,
                    "kind": kind.value, "src": src.value or 0, "nd": nd.value, "row": row.value,
                    "elem": elem.value, "shape": list(shp)[:nd.value],
                    "stride": list(std)[:nd.value], "lo": lo.value, "hi": hi.value})
        i += 1
        if i >= n.value:
            return out


def oracle(rec):
    """(sample bytes, ArrowTypeInfo, [(offset, length) of each field's leaf]) of the reference
    packing of the record's StructArray."""
    import pyarrow as pa
    from dora_amd import tensor
    from oracle.pack_ref import pack
    arr = pa.StructArray.from_arrays([tensor.from_numpy(v) for _, _, v in rec],
                                     names=[name for name, _, _ in rec])
    sample, info = pack(arr)
    ranges = []
    for c in info.child_data:
        while c.child_data:
            c = c.child_data[0]
        ranges.append((c.buffer_offsets[0].offset, c.buffer_offsets[0].len))
    return sample, info, ranges
