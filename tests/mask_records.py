"""Masks for the tensor-mask tests (dora_gpu_plan_tensor_mask), shared by the CPU plan test, the
sanitized host emulation of the two compaction kernels, the host dataflow test and the GPU tests:
records are lists of (field name, base array, view of that base) as in tests/list_records.py (a
name of None marks the one bare tensor), and the helpers here make the masks the tests select
rows by, describe values, mask and partition over any memory, plan them, read the plan back
through the testing library, and state in numpy what a masked message holds: N rows, the K
selected ones in source order in front and zero rows behind, under offsets C[p]."""
from ctypes import byref, c_int, c_int64, c_uint64, c_void_p

import numpy as np

from tests import list_records as lr

TILE = 4096  # gather_device.h mask::kTile
SIZES = (0, 1, 15, 16, 17, 255, 256, 257, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 3 * TILE + 5)
MANY_TILES = 257 * TILE + 3  # more tiles than threads take part in the sum of the totals
SHIFTS = (0, 1, 3, 13)  # the mask's address mod 16
DSTS = (0, 4, 8, 12)  # destination mod 16
MAX_ROWS = 1 << 24


def masks(n):
    """(label, N uint8 bytes): all zero, all set, alternating, random at 0.5, only the first row,
    only the last row, and random with the set bytes 2, 0x80 and 0xFF."""
    rng = np.random.default_rng(11 * n + 5)
    first, last = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    first[:1] = 1
    last[n - 1:] = 1
    odd = rng.choice(np.array([0, 0, 0, 2, 0x80, 0xFF], np.uint8), n)
    return [("all zero", np.zeros(n, np.uint8)), ("all set", np.ones(n, np.uint8)),
            ("alternating", (np.arange(n) % 2).astype(np.uint8)),
            ("random at 0.5", (rng.random(n) < 0.5).astype(np.uint8)),
            ("only the first row", first), ("only the last row", last),
            ("set bytes of 2, 0x80 and 0xFF", odd)]


def the_67_row_mask():
    """The mask of the 67-row case: 13 of rows [0, 31) and 16 of rows [31, 67) are set, so that
    under offsets [0, 31, 67] the message's offsets are [0, 13, 29]."""
    m = np.zeros(67, np.bool_)
    m[np.arange(0, 26, 2)] = True      # 13 rows below 31
    m[np.arange(31, 63, 2)] = True     # 16 rows from 31 on
    return m


def counts(mask):
    """C[0..N]: C[i] the number of selected rows among rows [0, i)."""
    return np.concatenate([[0], np.cumsum(np.asarray(mask) != 0)]).astype(np.int32)


def compacted(v, mask):
    """What a masked message holds of view `v`: the selected rows in front, zero rows behind."""
    keep = np.asarray(mask) != 0
    out = np.zeros(v.shape, v.dtype)
    out[:int(keep.sum())] = v[keep]
    return out


def masked_record(rec, mask):
    return [(name, None, compacted(v, mask)) for name, _, v in rec]


def oracle(rec, mask, offsets=None):
    """(sample bytes, ArrowTypeInfo, [(offset, length) of each field's leaf]) of the reference
    packing of the masked message: the ListArray of the compacted, zero-padded record under
    offsets C[p], `offsets` the partition p of the N source rows ([0, N] without one)."""
    n = len(mask)
    p = np.array([0, n], np.int64) if offsets is None else np.asarray(offsets, dtype=np.int64)
    return lr.oracle(masked_record(rec, mask), counts(mask)[p])


def values_of(rec):
    """The numpy values `tensor.from_numpy_masked` takes for `rec`."""
    return rec[0][2] if rec[0][0] is None else {name: v for name, _, v in rec}


def plan_mask(rec, ptr_of, dev, mask, mask_dev, mask_ptr=None, part=None, form=0, part_dev=1,
              part_ptr=None, mask_desc=None):
    """Plan the rows of `rec` (fields over `ptr_of(base)`) that the numpy array `mask` selects,
    which lives at `mask_ptr` (default: where numpy holds it) on `mask_dev`; with `part`, the
    partition of the N source rows (lengths or offsets as `form` says, at `part_ptr` on
    `part_dev`).  `mask_desc`: (shape, strides, dtype) the mask is described with instead of its
    own."""
    from dora_amd import _lib, tensor
    from dora_amd.arrow_utils import Plan
    names, tensors, keeps = lr.describe_values(rec, ptr_of)
    mask = np.ascontiguousarray(mask)
    mptr = mask.__array_interface__["data"][0] if mask_ptr is None else mask_ptr
    shape, strides, dtype = mask_desc or (mask.shape, None, mask.dtype)
    mt, mkeep = tensor._describe(mptr, shape, strides, dtype)
    pt = pkeep = None
    if part is not None:
        part = np.ascontiguousarray(part)
        pptr = part.__array_interface__["data"][0] if part_ptr is None else part_ptr
        pt, pkeep = tensor._describe(pptr, part.shape, None, part.dtype)
    mk, keep = tensor._describe_mask(names, tensors, mt, mask_dev, pt, form, part_dev)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_mask", byref(mk), dev, byref(h))
    return Plan(h.value, (mk, keep, keeps, mkeep, pkeep, mask, part, rec))


def workspace_size(plan):
    from dora_amd import _lib
    return int(_lib.load().dora_gpu_plan_workspace_size(plan.handle))


def plan_info(plan):
    """dora_gpu_test_plan_mask of a mask plan."""
    from dora_amd import _lib
    dev = c_int()
    src, n, lo, hi, part = c_void_p(), c_uint64(), c_int64(), c_int64(), c_uint64()
    ws, stride0 = (c_uint64 * 5)(), (c_int64 * 8)()
    _lib.call("dora_gpu_test_plan_mask", plan.handle, byref(dev), byref(src), byref(n), byref(lo),
              byref(hi), ws, byref(part), stride0)
    return {"device": bool(dev.value), "mask": src.value or 0, "n": n.value, "lo": lo.value,
            "hi": hi.value, "index": ws[0], "counts": ws[1], "totals": ws[2], "part": ws[3],
            "end": ws[4], "part_words": part.value, "stride0": list(stride0)}
