"""Takes for the tensor-take tests (dora_gpu_plan_tensor_take), shared by the CPU plan test, the
sanitized host emulation of the taken body, the host dataflow test and the GPU tests: records are
lists of (field name, base array, view of that base) as in tests/struct_records.py and
tests/list_records.py (a name of None marks the one bare tensor), and the helpers here make the
indices the tests take rows by, describe values, index and partition over any memory, plan them,
read the plan's index back through the testing library, and state in numpy what a take writes:
`values[index]`, a row of zeros where a word is not a row."""
from ctypes import byref, c_int, c_int64, c_uint64, c_void_p

import numpy as np

from tests import list_records as lr
from tests.gather_views import base

KS = (0, 1, 63, 64, 65, 257, 1025)
DSTS = (0, 3, 4, 8, 12)  # destination mod 16
ROWS = (1, 2, 4, 12, 16, 20, 24, 4096)  # bytes per taken row
# views of tests/gather_views.py whose dimension 0 differs in kind: a positive stride, a negative
# one, dimension 0 the contiguous one (rows of one element), stride 0, a misaligned source (the
# funnel path), a permuted image
VIEWS = ("f32_drop_first_column", "i16_reversed_step2", "f32_67x129_T", "f32_broadcast",
         "u8_byte_offset_3", "u8_hwc_to_chw_37x53x3")


def rows_view(n, row, dense):
    """(base, view) of `n` rows of `row` uint8: the base itself, or cut from a base 5 wider."""
    b = base(np.uint8, (n, row if dense else row + 5))
    return b, b if dense else b[:, :row]


def indices(k, n, wide):
    """(label, K words) over N rows: identity (cycled when K > N), reversed, one row repeated,
    random with repeats, and random mixed with words that are no row: -1, N, the type's minimum
    and maximum, and for int64 2^32 + 1 (whose low half alone would be a row) and -2^33."""
    dt = np.int64 if wide else np.int32
    rng = np.random.default_rng(7 * k + 3 * n + wide)
    ident = (np.arange(k) % n).astype(dt)
    info = np.iinfo(dt)
    bad = [-1, n, info.min, info.max] + ([(1 << 32) + 1, -(1 << 33)] if wide else [])
    mixed = rng.integers(0, n, k).astype(dt)
    where = rng.random(k) < 0.3
    if k:
        where[rng.integers(0, k)] = True
    mixed[where] = rng.choice(np.array(bad, dtype=dt), int(where.sum()))
    return [("identity", ident), ("reversed", ident[::-1].copy()),
            ("one row repeated", np.full(k, n - 1, dt)),
            ("random with repeats", rng.integers(0, n, k).astype(dt)),
            ("mixed with invalid words", mixed)]


def sweep(v, ks=KS):
    """(label, index, destination mod 16) for every K of `ks`, both widths and every kind of
    index over view `v`, the destinations in turn so that every kind meets every alignment."""
    n, turn = v.shape[0], 0
    for k in ks:
        for wide in (0, 1):
            for label, index in indices(k, n, wide):
                mis = DSTS[turn % len(DSTS)]
                turn += 1
                yield f"K={k} int{64 if wide else 32} {label} dst%16={mis}", index, mis
            turn += 1  # (five kinds, five destinations: shift the pairing with every round)


def three_fields(n=97):
    """A record of three fields of different row sizes — 16 bytes cut from 24, one float64 of
    three, 3 bytes cut from 7 — and the takes of it the tests run behind a ragged batch's 20 bytes
    of offsets (4 lists), where the first field starts at 4 mod 16 in a sample on a 16-byte
    boundary: (record, [(label, index, lengths, destination mod 16)])."""
    out, t, u = base(np.float32, (n, 6)), base(np.float64, (n, 3)), base(np.uint8, (n, 7))
    rec = [("bbox", out, out[:, :4]), ("t", t, t[:, 1]), ("rgb", u, u[:, 2:5])]
    cases = []
    for k in (1, 65, 257):
        for wide in (0, 1):
            for label, index in indices(k, n, wide):
                for mis in (0, 8):
                    cases.append((f"record K={k} int{64 if wide else 32} {label} dst%16={mis}", index,
                                  np.array([0, k // 2, k - k // 2, 0], np.int32), mis))
    return rec, cases


def taken(v, index):
    """What a take of view `v` by `index` holds: v[index], zero rows where a word is no row."""
    index = np.asarray(index)
    out = np.zeros((len(index),) + v.shape[1:], v.dtype)
    ok = (index >= 0) & (index < v.shape[0])
    out[ok] = v[index[ok].astype(np.int64)]
    return out


def taken_record(rec, index):
    """The record of materialised takes: every view replaced by `taken(view, index)`."""
    return [(name, None, taken(v, index)) for name, _, v in rec]


def oracle(rec, index, offsets=None):
    """(sample bytes, ArrowTypeInfo, [(offset, length) of each field's leaf]) of the reference
    packing of the message `values[index]` is today: tests/struct_records.py's or
    tests/list_records.py's oracle of the materialised record (zero rows where a word is no row,
    which is what a device take writes; a host take refuses such an index)."""
    from oracle.pack_ref import pack
    from dora_amd import tensor
    from tests import struct_records as sr
    mat = taken_record(rec, index)
    if offsets is not None:
        return lr.oracle(mat, offsets)
    if rec[0][0] is not None:
        return sr.oracle(mat)
    sample, info = pack(tensor.from_numpy(mat[0][2]))
    c = info
    while c.child_data:
        c = c.child_data[0]
    return sample, info, [(c.buffer_offsets[0].offset, c.buffer_offsets[0].len)]


def plan_take(rec, ptr_of, dev, index, index_dev, index_ptr=None, part=None,
              form=0, part_dev=1, part_ptr=None):
    """Plan the take of `rec` (fields over `ptr_of(base)`) by the numpy array `index`, which
    lives at `index_ptr` (default: where numpy holds it) on `index_dev`; with `part`, the ragged
    batch over the taken rows cut by it (lengths or offsets as `form` says, at `part_ptr` on
    `part_dev`)."""
    from dora_amd import _lib, tensor
    from dora_amd.arrow_utils import Plan
    names, tensors, keeps = lr.describe_values(rec, ptr_of)
    index = np.ascontiguousarray(index)
    iptr = index.__array_interface__["data"][0] if index_ptr is None else index_ptr
    it, ikeep = tensor._describe(iptr, index.shape, None, index.dtype)
    pt = pkeep = None
    if part is not None:
        part = np.ascontiguousarray(part)
        pptr = part.__array_interface__["data"][0] if part_ptr is None else part_ptr
        pt, pkeep = tensor._describe(pptr, part.shape, None, part.dtype)
    tk, keep = tensor._describe_take(names, tensors, it, index_dev, pt, form, part_dev)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_take", byref(tk), dev, byref(h))
    return Plan(h.value, (tk, keep, keeps, ikeep, pkeep, index, part, rec))


def plan_index(plan):
    """dora_gpu_test_plan_take of a take plan."""
    from dora_amd import _lib
    dev, wide = c_int(), c_int()
    src, k, n, lo, hi = c_void_p(), c_uint64(), c_uint64(), c_int64(), c_int64()
    stride0 = (c_int64 * 8)()
    _lib.call("dora_gpu_test_plan_take", plan.handle, byref(dev), byref(src), byref(k), byref(n),
              byref(wide), byref(lo), byref(hi), stride0)
    return {"device": bool(dev.value), "index": src.value or 0, "k": k.value, "n": n.value,
            "wide": bool(wide.value), "lo": lo.value, "hi": hi.value, "stride0": list(stride0)}
