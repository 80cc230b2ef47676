"""Seeded random Arrow arrays for the two plans of an Arrow `send_output` (plan.cpp walk and
walk_compact) and for transform_kernel, with their two references.

`array(seed)` builds one pyarrow array that passes `validate(full=True)`, every node through
`from_buffers` so that each decision is the generator's own:

* types: every class of plan.cpp's layout_of — fixed widths 1, 2, 4, 8, 16 and 32 (decimal128,
  month_day_nano, decimal256), fixed_size_binary down to width 0,
  bool, null, string / binary and their large forms, list, large_list, map, fixed_size_list down
  to width 1, struct of 1-4 fields, dictionary with int8 / int16 / int32 indices — nested to
  depth 3;
* slicing at every level: every node is built over `pre + n + post` elements and given the offset
  `pre`, so children have offsets of their own, list offsets do not start at 0 and dictionary
  values are slices; the top level is then sliced again, `n == 0` and `lo == len` included;
* validity per node: no bitmap, nulls inside the node's window, a bitmap whose nulls all lie
  outside the window (present, and dropped by both plans), or all null;
* sizes: at most 64 top-level elements, except that the seeds 7 mod 10 hold a Boolean column of
  more than 32768 values or an offsets buffer of more than 4096 entries (more than one workgroup
  of transform_kernel).

The references are both oracle/pack_ref.py's `pack`: of the array itself (reference layout) and
of `rebuilt(arr)` (compact layout), a deep copy with offset 0 at every level.  `compare` holds a
sample against either under the rules of the sweep: every byte of every region exact, but for
the bits past `len` in the last byte of a Boolean column's bitmap, where the kernel carries the
source's bits; every byte outside the regions still the poison.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pyarrow as pa

from oracle.arrow_ffi import Exported, layout
from oracle.pack_ref import pack

POISON = 0xC7
SLACK = 48
SMALL = 64          # most seeds: top-level elements at most
LETTERS = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz", np.uint8)

FIXED = [pa.int8(), pa.uint8(), pa.int16(), pa.float16(), pa.int32(), pa.float32(), pa.date32(),
         pa.int64(), pa.float64(), pa.timestamp("us"), pa.decimal128(38, 3),
         pa.month_day_nano_interval(), pa.decimal256(76, 5), pa.binary(0), pa.binary(3),
         pa.binary(16)]
VAR = [pa.string(), pa.binary(), pa.large_string(), pa.large_binary()]
LEAVES = FIXED + VAR + VAR + [pa.bool_()] * 8 + [pa.null()]


def _bits(rng, total, mode, pre, n):
    """Validity of `total` elements whose window is [pre, pre + n), or None."""
    if mode == "none":
        return None
    if mode == "all":
        v = np.zeros(total, bool)
    elif mode == "outside":
        v = np.ones(total, bool)
        out = [i for i in range(total) if not pre <= i < pre + n]
        if not out:
            return None
        v[rng.choice(out, size=max(1, len(out) // 2), replace=False)] = False
    else:
        v = rng.random(total) < 0.7
        if n:
            v[pre + int(rng.integers(0, n))] = False
    return v


def _bitmap(v):
    return pa.py_buffer(np.packbits(v, bitorder="little").tobytes())


class _Gen:
    def __init__(self, seed):
        self.rng = np.random.default_rng([0xA77A, seed])

    # ---- types --------------------------------------------------------------------------------
    def pick_type(self, depth):
        rng = self.rng
        if depth >= 3 or rng.random() < 0.35:
            return LEAVES[int(rng.integers(len(LEAVES)))]
        k = int(rng.integers(7))
        if k == 0:
            return pa.list_(self.pick_type(depth + 1))
        if k == 1:
            return pa.large_list(self.pick_type(depth + 1))
        if k == 2:
            key = [pa.int32(), pa.string(), pa.int8()][int(rng.integers(3))]
            return pa.map_(key, self.pick_type(depth + 2))
        if k == 3:
            return pa.list_(self.pick_type(depth + 1), int(rng.integers(1, 4)))
        if k == 4:
            nf = int(rng.integers(1, 5))
            return pa.struct([pa.field(f"f{i}", self.pick_type(depth + 1)) for i in range(nf)])
        if k == 5:
            idx = [pa.int8(), pa.int16(), pa.int32()][int(rng.integers(3))]
            val = [pa.string(), pa.int32(), pa.float64(), pa.large_string(), pa.bool_(),
                   pa.binary(2)][int(rng.integers(6))]
            return pa.dictionary(idx, val, ordered=bool(rng.integers(2)))
        return pa.list_(pa.list_(self.pick_type(depth + 2)))

    # ---- nodes --------------------------------------------------------------------------------
    def window(self, n):
        """(pre, post): what a node's buffers hold before and after its n elements."""
        rng = self.rng
        if rng.random() < 0.3:
            return 0, 0
        return int(rng.integers(0, 12)), int(rng.integers(0, 5))

    def validity(self, total, pre, n, allow=True):
        rng = self.rng
        if not allow:
            return None
        mode = ["none", "some", "outside", "all", "some"][int(rng.integers(5))]
        if mode == "all" and rng.random() < 0.5:
            mode = "some"
        return _bits(rng, total, mode, pre, n)

    def node(self, t, n, nullable=True):
        """An array of type `t` and length `n`, with an offset of its own more often than not."""
        rng = self.rng
        if pa.types.is_null(t):
            pre, post = self.window(n)
            return pa.nulls(pre + n + post).slice(pre, n)
        pre, post = self.window(n)
        total = pre + n + post
        v = self.validity(total, pre, n, nullable)
        vb = None if v is None else _bitmap(v)
        mk = lambda bufs, children=None: pa.Array.from_buffers(  # noqa: E731
            t, n, [vb] + bufs, -1, pre, children)
        if pa.types.is_boolean(t):
            return mk([_bitmap(rng.random(total) < 0.5)])
        if pa.types.is_decimal(t):
            w = t.byte_width
            lim = 10 ** (t.precision - 1)
            raw = b"".join((int(rng.integers(-10 ** 18, 10 ** 18)) * (lim // 10 ** 18 - 1))
                           .to_bytes(w, "little", signed=True) for _ in range(total))
            return mk([pa.py_buffer(raw)])
        if pa.types.is_floating(t):
            x = rng.standard_normal(total).astype({16: np.float16, 32: np.float32,
                                                   64: np.float64}[t.bit_width])
            return mk([pa.py_buffer(x.tobytes())])
        if pa.types.is_fixed_size_binary(t) or pa.types.is_primitive(t):
            w = t.byte_width
            return mk([pa.py_buffer(rng.integers(0, 256, total * w, dtype=np.uint8).tobytes())])
        if (pa.types.is_string(t) or pa.types.is_binary(t) or pa.types.is_large_string(t)
                or pa.types.is_large_binary(t)):
            odt = np.int64 if (pa.types.is_large_string(t) or pa.types.is_large_binary(t)) \
                else np.int32
            lens = rng.integers(0, 6, total)
            lead = int(rng.integers(0, 4))       # data bytes before the first string
            off = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(odt)
            data = LETTERS[rng.integers(0, 26, int(off[-1]) + int(rng.integers(0, 3)))]
            return mk([pa.py_buffer(off.tobytes()), pa.py_buffer(data.tobytes())])
        if pa.types.is_dictionary(t):
            nd = int(rng.integers(1, 9))
            d = self.node(t.value_type, nd)
            idx = rng.integers(0, nd, total).astype(t.index_type.to_pandas_dtype())
            return pa.DictionaryArray.from_buffers(t, n, [vb, pa.py_buffer(idx.tobytes())], d, -1,
                                                   pre)
        if pa.types.is_struct(t):
            return mk([], [self.node(f.type, total, f.nullable) for f in t])
        if pa.types.is_fixed_size_list(t):
            return mk([], [self.node(t.value_type, total * t.list_size)])
        if pa.types.is_map(t) or pa.types.is_list(t) or pa.types.is_large_list(t):
            odt = np.int64 if pa.types.is_large_list(t) else np.int32
            lens = rng.integers(0, 4, total)
            lead = int(rng.integers(0, 4))       # child elements before the first list
            off = (lead + np.concatenate([[0], np.cumsum(lens)])).astype(odt)
            nchild = int(off[-1]) + int(rng.integers(0, 3))
            if pa.types.is_map(t):
                et = pa.struct([t.key_field, t.item_field])
                keys = self.node(t.key_type, nchild, nullable=False)
                items = self.node(t.item_type, nchild)
                child = pa.Array.from_buffers(et, nchild, [None], 0, 0, [keys, items])
            else:
                child = self.node(t.value_type, nchild)
            return mk([pa.py_buffer(off.tobytes())], [child])
        raise NotImplementedError(str(t))

    # ---- a whole array ------------------------------------------------------------------------
    def big(self):
        """More than kXElems = 4096 elements of one transformed buffer."""
        rng = self.rng
        kind = int(rng.integers(5))
        if kind == 0:
            t, n = pa.bool_(), int(rng.integers(32769 + 11, 3 * 32768))
        elif kind == 1:
            t, n = pa.string(), int(rng.integers(4100, 9000))
        elif kind == 2:
            t, n = pa.large_string(), int(rng.integers(4100, 9000))
        elif kind == 3:
            t, n = pa.list_(pa.int8()), int(rng.integers(4100, 9000))
        else:
            t = pa.struct([pa.field("b", pa.bool_()), pa.field("s", pa.large_list(pa.bool_())),
                           pa.field("k", pa.int16())])
            n = int(rng.integers(32769 + 11, 40000))
        return self.node(t, n)

    def top(self, seed):
        rng = self.rng
        if seed % 10 == 7:
            arr = self.big()
            lo = int(rng.integers(0, 9))
            return arr.slice(lo, len(arr) - lo - int(rng.integers(0, 3)))
        arr = self.node(self.pick_type(0), int(rng.integers(0, SMALL + 1)))
        mode = rng.random()
        n = len(arr)
        if mode < 0.25:
            return arr
        if mode < 0.35:
            return arr.slice(int(rng.integers(0, n + 1)), 0)
        if mode < 0.45:
            return arr.slice(n)
        lo = int(rng.integers(0, n + 1))
        return arr.slice(lo, int(rng.integers(0, n - lo + 1)))


def array(seed: int) -> pa.Array:
    arr = _Gen(seed).top(seed)
    arr.validate(full=True)
    return arr


# ---------------------------------------------------------------------------------------------
# What an array is, read from its C export as the plans read it
# ---------------------------------------------------------------------------------------------
def _count_nulls(ptr, off, n):
    raw = np.frombuffer(ctypes.string_at(ptr, (off + n + 7) // 8), np.uint8)
    return n - int(np.unpackbits(raw, bitorder="little")[off:off + n].sum())


def _walk(a, s, depth, out, in_list, is_dict_values=False):
    fmt = s.format.decode()
    can_null = layout(fmt)[1]
    bitmap = bool(can_null and a.n_buffers > 0 and a.buffers[0])
    nulls = 0
    if bitmap:
        nulls = a.null_count if a.null_count >= 0 else _count_nulls(a.buffers[0], a.offset, a.length)
    out.append({"fmt": fmt, "depth": depth, "offset": a.offset, "length": a.length,
                "bitmap": bitmap, "nulls": nulls, "dict_values": is_dict_values,
                "list_in_list": in_list and fmt in ("+l", "+L", "+m") and not s.dictionary})
    if s.dictionary:
        _walk(a.dictionary.contents, s.dictionary.contents, depth + 1, out, False, True)
        return
    lst = in_list or fmt in ("+l", "+L", "+m")
    for i in range(a.n_children):
        _walk(a.children[i].contents, s.children[i].contents, depth + 1, out, lst)


def nodes(arr):
    """One record per node of `arr` in walk order: format, depth, offset, length, whether a
    validity bitmap is present and the nulls of [offset, offset + length)."""
    out = []
    with Exported(arr) as ex:
        _walk(ex.array, ex.schema, 0, out, False)
    return out


def facts(arr):
    """The conditions of the sweep that the array alone decides."""
    ns = nodes(arr)
    return {
        "top_offset": ns[0]["offset"] > 0,
        "child_offset": any(x["offset"] > 0 for x in ns[1:]),
        "empty": ns[0]["length"] == 0,
        "dict_sliced_values": any(x["dict_values"] and x["offset"] > 0 for x in ns),
        "list_in_list": any(x["list_in_list"] for x in ns),
        "validity_kept": any(x["bitmap"] and x["nulls"] > 0 for x in ns),
        "validity_dropped": any(x["bitmap"] and x["nulls"] == 0 for x in ns),
        "no_nulls": not any(x["bitmap"] for x in ns),
        "all_null": any(x["bitmap"] and x["length"] and x["nulls"] == x["length"] for x in ns),
    }


# ---------------------------------------------------------------------------------------------
# References
# ---------------------------------------------------------------------------------------------
def _own_children(c):
    t = c.type
    if pa.types.is_struct(t):
        return [c.field(i) for i in range(t.num_fields)]
    return [c.values]


def _fix_dictionaries(c):
    """`c` (fresh buffers, offset 0 but for dictionary values) with every dictionary's values
    rebuilt as well."""
    t = c.type
    if pa.types.is_dictionary(t):
        return pa.DictionaryArray.from_arrays(c.indices, rebuilt(c.dictionary), ordered=t.ordered)
    if not pa.types.is_nested(t):
        return c
    assert c.offset == 0
    own = 1 if (pa.types.is_struct(t) or pa.types.is_fixed_size_list(t)) else 2
    return pa.Array.from_buffers(t, len(c), c.buffers()[:own], c.null_count, 0,
                                 [_fix_dictionaries(x) for x in _own_children(c)])


def rebuilt(arr):
    """A deep copy of `arr` with offset 0 at every level: pyarrow's concatenation copies a slice
    into fresh buffers at every node but a dictionary's values, which it keeps whole; those are
    rebuilt on their own."""
    out = _fix_dictionaries(pa.concat_arrays([arr]))
    assert out.type == arr.type and len(out) == len(arr)
    assert all(x["offset"] == 0 for x in nodes(out)), "a node of the rebuilt array has an offset"
    return out


def reference(arr, compact):
    """(sample bytes, ArrowTypeInfo) of the layout: oracle.pack_ref.pack of the array, or of its
    rebuilt copy."""
    return pack(rebuilt(arr) if compact else arr)


def mask_validity(ti):
    """Type info as JSON with the bits past `len` dropped from every validity bitmap (they are
    not part of the logical array; tests/test_compact_host.py)."""
    j = ti.to_json() if hasattr(ti, "to_json") else ti

    def walk(t):
        if t["validity"] is not None:
            b = bytearray(bytes.fromhex(t["validity"]))
            n = t["len"]
            if n % 8 and b:
                b[-1] &= (1 << (n % 8)) - 1
            t["validity"] = bytes(b).hex()
        for c in t["child_data"]:
            walk(c)
    walk(j)
    return j


def regions(info):
    """[(offset, len, bits)] of every buffer of a type info, in walk order; `bits` is the element
    count of a Boolean column's bitmap (whose last byte is compared under a mask), else None."""
    out = []
    for k, b in enumerate(info.buffer_offsets):
        out.append((b.offset, b.len, info.len if info.data_type == "b" and k == 0 else None))
    for c in info.child_data:
        out += regions(c)
    return out


def compare(got, want, info, compact, label=""):
    """`got`: the packed buffer, sample plus slack, poisoned before the pack.  Every region equals
    the reference's — in the compact layout but for the bits past `len` of a shifted bitmap's last
    byte — and every other byte keeps the poison."""
    got = bytes(got)
    assert len(got) >= len(want), (label, len(got), len(want))
    covered = np.zeros(len(got), bool)
    for off, ln, bits in regions(info):
        g, w = got[off:off + ln], want[off:off + ln]
        if compact and bits is not None and bits % 8 and ln:
            m = (1 << (bits % 8)) - 1
            g = g[:-1] + bytes([g[-1] & m])
            w = w[:-1] + bytes([w[-1] & m])
        if g != w:
            bad = [i for i in range(ln) if g[i] != w[i]]
            raise AssertionError((label, "region", off, ln, "first bad bytes", bad[:8]))
        covered[off:off + ln] = True
    stale = np.flatnonzero(~covered & (np.frombuffer(got, np.uint8) != POISON))
    assert stale.size == 0, (label, "bytes outside the regions written", stale[:16].tolist())


# ---------------------------------------------------------------------------------------------
# Limit cases that are real arrays (CPU emulation and GPU alike)
# ---------------------------------------------------------------------------------------------
X_ELEMS = 4096      # transform_device.h kXElems: output elements per workgroup
X_MAX_SEGS = 32     # transform_device.h kXMaxSegs: transform segments per launch
EDGES = (X_ELEMS - 1, X_ELEMS, X_ELEMS + 1, 2 * X_ELEMS + 1)


def _exact_bool(rng, lo, n, validity=None):
    """A Boolean column of n values `lo` bits into a bitmap of exactly ceil((lo + n) / 8) bytes."""
    return pa.Array.from_buffers(pa.bool_(), n, [validity, _bitmap(rng.random(lo + n) < 0.5)],
                                 -1 if validity is not None else 0, lo)


def _strings(rng, t, total):
    odt = np.int64 if t in (pa.large_string(), pa.large_binary()) else np.int32
    off = (3 + np.concatenate([[0], np.cumsum(rng.integers(0, 3, total))])).astype(odt)
    data = LETTERS[rng.integers(0, 26, int(off[-1]))]
    return pa.Array.from_buffers(t, total, [None, pa.py_buffer(off.tobytes()),
                                            pa.py_buffer(data.tobytes())], 0, 0)


def limit_arrays():
    """[(label, array)]: each op at the edges of a workgroup's share, every (bit offset,
    len mod 8) at 1-3 output bytes, more transform segments than one launch holds, and a first
    transform segment of three blocks before segments of one."""
    rng = np.random.default_rng(0x11A1)
    out = []
    for e in EDGES:
        # e output bytes of a shifted bitmap; e offsets of 4 and of 8 bytes
        out.append((f"bitshift {e} B", _exact_bool(rng, 3, 8 * e - 5)))
        out.append((f"rebase32 {e} offsets", _strings(rng, pa.string(), e + 4).slice(2, e - 1)))
        out.append((f"rebase64 {e} offsets", _strings(rng, pa.large_string(), e + 4).slice(2, e - 1)))
    for nbytes in (1, 2, 3):
        for r in range(1, 9):                       # len mod 8 = r mod 8
            n = 8 * (nbytes - 1) + r
            cols = [_exact_bool(rng, b, n) for b in range(8)]
            out.append((f"bit offsets 0-7, {n} bits", pa.StructArray.from_arrays(
                cols, names=[f"b{b}" for b in range(8)])))
    # 40 string and Boolean columns of a sliced struct: 40 transform segments, two launches
    n = 21
    cols = [(_strings(rng, pa.string(), n) if k % 2 else _exact_bool(rng, 0, n)) for k in range(40)]
    out.append(("40 transformed columns", pa.StructArray.from_arrays(
        cols, names=[f"c{k}" for k in range(40)]).slice(5, 13)))
    # list<struct<s: string, b: bool>>: 2 * 4096 + 1 list offsets (three blocks), then the string
    # offsets and the bitmap of the few entries (one block each)
    nl = 2 * X_ELEMS + 3
    lens = np.zeros(nl, np.int64)
    lens[rng.choice(nl, 300, replace=False)] = rng.integers(1, 4, 300)
    off = (2 + np.concatenate([[0], np.cumsum(lens)])).astype(np.int32)
    nc = int(off[-1]) + 1
    entries = pa.StructArray.from_arrays([_strings(rng, pa.string(), nc), _exact_bool(rng, 0, nc)],
                                         names=["s", "b"])
    lst = pa.Array.from_buffers(pa.list_(entries.type), nl, [None, pa.py_buffer(off.tobytes())],
                                0, 0, [entries])
    out.append(("three blocks, then one each", lst.slice(1, 2 * X_ELEMS)))
    for _, a in out:
        a.validate(full=True)
    return out
