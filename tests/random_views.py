"""Seeded random views, records, indices, masks and partitions for the sweeps of
tests/test_random_views_host.py (the sanitized emulations) and tests/test_gpu_random_views.py (the
kernels): plain functions of a numpy.random.Generator, so that one integer names a case —
`rng(seed)` and the same calls in the same order reproduce it, and every failure message of the
sweeps prints `seed=`.  No test lives here.

A view has 1 to 6 dimensions (8 for an occasional seed) with extents from a pool around the edges
of the 16-byte unit and the 16-, 32- and 64-element tiles, a step of 1, 2, 3, -1 or -2 and up to
two elements of slack on either side in every dimension of its base, the dimensions permuted,
sometimes one of them broadcast (stride 0: dimension 0 and the innermost one each get their
turn), and sometimes a base whose first byte is not a multiple of the element size.

The op bodies (quantise, affine, argmax, resize, crops) get records of such views in the form of
their tests/*_records.py: `quant_record`, `affine_record`, `argmax_record`, `resize_record`,
`crop_record`, and `misaligned_op` for the refusals.  What a sweep must see in known numbers it
deals along its seeds and hands in (`narrow`: 8-bit destinations only, so that a record goes to odd
addresses; `dense` for argmax); left out, the same things are drawn.  Values are shaped where the
plain ones would test little: quantised sources are brought to about the destination's span, float
sources that go to integers are grown, argmax sources are sprinkled with NaN, infinities, zeros of
both signs and repeats.  The two model-input bodies (gather_resize_prep_kernel,
gather_crop_prep_kernel) get `prep_resize_record` and `prep_crop_record`: the resize's and the
crops' records with a step of `prep_step` on their op fields.  To reproduce a case of a sweep call its `*_case(seed)` in
tests/test_random_views_host.py."""
import numpy as np

from tests import affine_records as ar
from tests import argmax_records as am
from tests import cast_records as cr
from tests import crop_records as kr
from tests import mask_records as mr
from tests import prep_records as pr
from tests import quant_records as qr
from tests import resize_records as rr
from tests import take_records as tr

EXTENTS = (1, 2, 3, 5, 7, 15, 16, 17, 31, 32, 33, 63, 64, 65)
STEPS = (1, 1, 1, 2, 3, -1, -2)
DTYPES = (np.uint8, np.int16, np.float32, np.float64, np.int8, np.float16, np.uint32, np.int64)
MAX_ELEMS = 24000


def rng(seed):
    return np.random.default_rng(seed)


def fill(dtype, shape, raw_shift=0, src=None, seed=0):
    """A base of `shape`: tests/gather_views.py's values (neighbouring elements differ), or
    tests/cast_records.py's for a cast source `src`; with `raw_shift`, over memory that starts that
    many bytes past an aligned address."""
    n = int(np.prod(shape))
    if src is not None:
        vals = cr.source(src, (n,), seed)
        dtype = vals.dtype
    else:
        vals = ((np.arange(n, dtype=np.int64) * 37 + 11) % 2039).astype(dtype)
    if not raw_shift:
        return vals.reshape(shape)
    raw = np.zeros(n * vals.itemsize + 16, np.uint8)
    assert raw.ctypes.data % 16 == 0
    b = np.frombuffer(raw, dtype, count=n, offset=raw_shift).reshape(shape)
    b[...] = vals.reshape(shape)
    return b


def view(r, dtype, d0=None, max_elems=MAX_ELEMS, src=None, shift=None, nd_min=1, nd_max=8):
    """(base, view) of `dtype` (or of cast source `src`); with `d0`, dimension 0 of the view has
    that extent and stays in front, whichever dimension of the base it is.  `shift`: the bytes
    the base starts past a multiple of its element size (default: 0 for most seeds, 1 or 3 for a
    tenth of those whose elements are wider than a byte).  `nd_min`, `nd_max`: the fewest and
    the most dimensions an op takes."""
    nd = min(8 if r.random() < 0.12 else int(r.integers(nd_min, 7)), nd_max)
    lead = int(r.integers(0, nd))  # the base dimension that becomes dimension 0 when d0 is given
    shape, slices, room = [], [], 1  # (room: the base's elements so far)
    order, ext = list(r.permutation(nd)), {}  # (extents are dealt in random order, a given one first)
    if d0 is not None:
        order.remove(lead)
        order.insert(0, lead)
    for i, k in enumerate(order):
        step = int(r.choice(STEPS))
        before, after = int(r.integers(0, 3)), int(r.integers(0, 3))
        if nd == 8 and r.random() < 0.7:  # (or no room is left for the last dimensions)
            step, before, after = (1 if step > 0 else -1), 0, 0
        left = nd - i
        cap = max(2.0, (max_elems / room) ** (1.0 / left) * float(r.uniform(1.0, 4.0)))
        if d0 is not None and k == lead:
            e = d0
        else:
            fit = [e for e in EXTENTS
                   if (e - 1) * abs(step) + 1 + before + after <= cap
                   and room * ((e - 1) * abs(step) + 1 + before + after) <= max_elems]
            # (where room is short, as in 8 dimensions, an extent of 1 is most of what fits:
            # mostly pass it over, or the view has few dimensions left once they are dropped)
            more = [e for e in fit if e > 1]
            e = int(r.choice(more if more and r.random() < 0.8 else fit)) if fit else 1
        span = (e - 1) * abs(step) + 1
        if room * (span + before + after) > max_elems:  # no room for slack, or for the step
            before = after = 0
            if room * span > max_elems:
                step, span = 1, e
        room *= span + before + after
        ext[k] = (e, step, before, after, span)
    for k in range(nd):
        e, step, before, after, span = ext[k]
        shape.append(span + before + after)
        if step > 0:
            slices.append(slice(before, before + span, step))
        else:
            stop = before + step
            slices.append(slice(before + span - 1, stop if stop >= 0 else None, step))
    size = np.dtype(cr.SOURCES[src][0] if src else dtype).itemsize
    if shift is None:
        shift = int(r.choice([1, 3])) if size > 1 and r.random() < 0.1 else 0
    b = fill(dtype, tuple(shape), shift, src, seed=int(r.integers(0, 1 << 16)))
    v = b[tuple(slices)]
    assert v.shape == tuple(ext[k][0] for k in range(nd))
    perm = list(r.permutation(nd))
    if d0 is not None:
        perm.remove(lead)
        perm.insert(0, lead)
    v = v.transpose(perm)
    if r.random() < 0.15 and v.size > 1:
        # one dimension broadcast: dimension 0, the innermost, or any
        which = int(r.choice([0, nd - 1, int(r.integers(0, nd))]))
        if v.shape[which] > 1:
            one = tuple(slice(0, 1) if k == which else slice(None) for k in range(nd))
            v = np.broadcast_to(v[one], v.shape)
    return b, v


def inside(b, v):
    """Every element of `v` lies inside `b`: what a test checks before it hands a view's
    description to a kernel."""
    off = v.__array_interface__["data"][0] - b.__array_interface__["data"][0]
    lo, hi = cr.reach(b, v)
    return v.size == 0 or (0 <= off + lo and off + hi < b.nbytes)


def bare(r, max_elems=MAX_ELEMS):
    dtype = DTYPES[int(r.integers(0, len(DTYPES)))]
    return view(r, dtype, max_elems=max_elems)


def record(r, n_fields=None, max_elems=MAX_ELEMS, d0=None):
    """[(name, base, view)] of `n_fields` (default: 1 to 8, 8 more often than its turn) random
    views over one d0."""
    if n_fields is None:
        n_fields = 8 if r.random() < 0.1 else int(r.integers(1, 9))
    if d0 is None:
        d0 = int(r.choice(EXTENTS))
    rec = []
    for k in range(n_fields):
        dtype = DTYPES[int(r.integers(0, len(DTYPES)))]
        b, v = view(r, dtype, d0=d0, max_elems=max(max_elems // n_fields, 4 * d0))
        rec.append((f"f{k}", b, v))
    return rec


def cast_record(r, n_fields=None, max_elems=MAX_ELEMS):
    """[(name or None, base, view, cast or None)]: every field a cast of a random pair of
    tests/cast_records.py's under no scale, 1/255 or 3.0 (3.0 where the pair is the identity),
    except that the fields behind the first are sometimes plain."""
    if n_fields is None:
        n_fields = int(r.integers(1, 5))
    d0 = int(r.choice(EXTENTS))
    rec = []
    for k in range(n_fields):
        if k > 0 and r.random() < 0.3:
            dtype = DTYPES[int(r.integers(0, len(DTYPES)))]
            b, v = view(r, dtype, d0=d0, max_elems=max(max_elems // n_fields, 4 * d0))
            rec.append((f"f{k}", b, v, None))
            continue
        src, dst = cr.PAIRS[int(r.integers(0, len(cr.PAIRS)))]
        scale = [None, 1 / 255, 3.0][int(r.integers(0, 3))]
        if src == dst and scale is None:
            scale = 3.0
        b, v = view(r, None, d0=d0, max_elems=max(max_elems // n_fields, 4 * d0), src=src,
                    shift=0)
        rec.append((f"f{k}" if n_fields > 1 else None, b, v, cr.cast(src, dst, scale)))
    return rec


def index(r, k, n, wide):
    """(label, K words over N rows): one of tests/take_records.py's kinds, or words of this seed's
    own, a third of them no row."""
    kinds = tr.indices(k, n, wide)
    which = int(r.integers(0, len(kinds) + 1))
    if which < len(kinds):
        return kinds[which]
    dt = np.int64 if wide else np.int32
    info = np.iinfo(dt)
    words = r.integers(0, n, k).astype(dt)
    bad = np.array([-1, n, info.min, info.max] + ([(1 << 32) + 1, -(1 << 33)] if wide else []), dt)
    where = r.random(k) < 0.3
    words[where] = r.choice(bad, int(where.sum()))
    return "random words of the seed", words


def mask(r, n):
    """(label, N uint8 bytes): one of tests/mask_records.py's, or random at a random density."""
    kinds = mr.masks(n)
    which = int(r.integers(0, len(kinds) + 1))
    if which < len(kinds):
        return kinds[which]
    p = float(r.random())
    return f"random at {p:.2f}", (r.random(n) < p).astype(np.uint8)


def partition(r, n, garbage=False):
    """(words, offsets form?, the offsets they mean): 1 to 6 lists over n rows with empty ones
    among them, as lengths or offsets in int32 or int64.  With `garbage` (partitions in HBM, which
    no one checks before the launch) the words are anything: negative, past n, not monotone; the
    offsets are then the clamped formula's (tests/list_records.py)."""
    from tests import list_records as lr
    lists = int(r.integers(1, 7))
    cuts = np.sort(r.integers(0, n + 1, lists - 1))
    offs = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    form = bool(r.integers(0, 2))
    dt = np.int64 if r.integers(0, 2) else np.int32
    words = offs if form else np.diff(offs)
    if garbage:
        info = np.iinfo(dt)
        words = words.copy()
        bad = np.array([-1, -7, n + 1, 2 * n + 3, info.max, info.min, 1 << 30], np.int64)
        where = r.random(len(words)) < 0.4
        words[where] = r.choice(bad, int(where.sum()))
        words = words.astype(dt)
        return words, form, lr.clamped_offsets(words, form, n)
    return words.astype(dt), form, offs.astype(np.int32)


def misaligned_cast(r):
    """[(name, base, view, cast)]: an aligned plain field in front of a cast whose 2- or 4-byte
    source starts 1 or 3 bytes past a multiple of its element size: no kernel runs it."""
    d0 = int(r.choice(EXTENTS))
    src = ["uint16", "int16", "float16", "bfloat16", "float32"][int(r.integers(0, 5))]
    a, va = view(r, np.uint8, d0=d0, max_elems=2000)
    b, vb = view(r, None, d0=d0, max_elems=2000, src=src, shift=int(r.choice([1, 3])))
    return [("f0", a, va, None), ("f1", b, vb, cr.cast(src, "float32", 1 / 255))]


# ---------------------------------------------------------------------------------------------
# The op bodies: quantise, affine, argmax, resize, crops.  A record is the op's own
# (tests/*_records.py): (name or None, base, view, op or None), for affine with a fifth column.
# ---------------------------------------------------------------------------------------------
FLOATS = ("float16", "bfloat16", "float32")
ARGMAX_EXTENTS = EXTENTS + (129, 256, 257)
CROP_COUNTS = (0, 1, 2, 3, 5, 17)


def share(r, p, given=None):
    """True for a share `p` of the seeds; `given` (a sweep deals it along its seeds, so that what
    depends on it comes in known numbers) in its place, the draw made all the same."""
    drawn = bool(r.random() < p)
    return drawn if given is None else given


def plain(r, d0, room, width=3):
    """A plain field (name, base, view, None ..) of `width` columns over `d0`."""
    dtype = DTYPES[int(r.integers(0, len(DTYPES)))]
    b, v = view(r, dtype, d0=d0, max_elems=max(room, 4 * d0))
    return (b, v) + (None,) * (width - 2)


def planes(d0, width=3):
    """The permuted float32 field that the library's own selection tiles (output rows of 280 bytes
    along the source-contiguous dimension), as tests/test_random_views_host.py's cast_case has it."""
    from tests.gather_views import base
    b = base(np.float32, (65, d0, 70))
    return ("planes", b, b.transpose(1, 2, 0)) + (None,) * (width - 2)


def with_planes(r, rec, d0, share=0.8):
    """`rec` with the `planes` field at a seeded place, for a seeded share of the records whose
    leading extent `d0` is 1 to 7; a bare tensor gets a name beside it."""
    if not 1 <= d0 <= 7 or r.random() >= share:
        return rec
    rec = [((x[0] or "f0"),) + tuple(x[1:]) for x in rec]
    rec.insert(int(r.integers(0, len(rec) + 1)), planes(d0, len(rec[0]) - 1))
    return rec


def names(rec):
    """Fields named f0.., a single one bare."""
    if len(rec) == 1:
        return [(None,) + tuple(rec[0])]
    return [(f"f{k}",) + tuple(x) for k, x in enumerate(rec)]


def grow(b, src, factor):
    """The values of float base `b` of source `src` times `factor`, in place."""
    if src == "bfloat16":
        f = (b.astype(np.uint32) << 16).view(np.float32) * np.float32(factor)
        b[...] = (f.view(np.uint32) >> 16).astype(np.uint16)
    else:
        with np.errstate(over="ignore"):
            b *= b.dtype.type(factor)


def for_integers(b, op):
    """A float source's values times 300 where the destination is an integer, which would round
    most of them to zero as they are."""
    if op["src"] in FLOATS and rr.dst_name(op)[0] in "ui":
        grow(b, op["src"], 300.0)


def quant_conv(r, narrow=False):
    """A quantise of a random pair (`narrow`: to 8 bits, so that a record of such fields goes to
    odd destinations too) under a scale its source allows and one of the destination's zero
    points."""
    pairs = [p for p in qr.PAIRS if p[1] in ("uint8", "int8")] if narrow else qr.PAIRS
    src, dst = pairs[int(r.integers(0, len(pairs)))]
    scales = qr.FLOAT_SCALES if src in FLOATS else qr.INT_SCALES
    zps = qr.zero_points(dst)
    info = np.iinfo(qr.DESTS[dst][0])
    # (a zero point on a bound of the destination half as often as one inside it)
    w = np.array([1.0 if z in (info.min, info.max) else 2.0 for z in zps])
    return qr.quant(src, dst, scales[int(r.integers(0, len(scales)))], int(r.choice(zps, p=w / w.sum())))


def float_cast(r):
    src, dst = cr.PAIRS[int(r.integers(0, len(cr.PAIRS)))]
    scale = [None, 1 / 255, 3.0][int(r.integers(0, 3))]
    return cr.cast(src, dst, 3.0 if src == dst and scale is None else scale)


def quant_record(r, n_fields=None, max_elems=MAX_ELEMS, narrow=None):
    """[(name or None, base, view, conversion or None)]: the first field quantised, the ones behind
    it quantised, plain or a float cast."""
    if n_fields is None:
        n_fields = int(r.integers(1, 4))
    d0 = int(r.choice(EXTENTS))
    room = max(max_elems // n_fields, 4 * d0)
    narrow = share(r, 0.7, narrow)
    rec = []
    for k in range(n_fields):
        kind = int(r.integers(0, 4)) if k else 0
        if kind == 1:
            rec.append(plain(r, d0, room))
            continue
        c = float_cast(r) if kind == 2 and not narrow else quant_conv(r, narrow)
        b, v = view(r, None, d0=d0, max_elems=room, src=c["src"], shift=0)
        if qr.is_quant(c) and r.random() < 0.75:
            # values brought to about the destination's span under the scale, so that a part of
            # the outputs saturates and not nearly all of them, nor nearly all are the zero point
            span = float(np.iinfo(qr.DESTS[c["dst"]][0]).max) - np.iinfo(qr.DESTS[c["dst"]][0]).min
            if c["src"] in FLOATS:
                grow(b, c["src"], span / 8 / max(abs(c["scale"] or 1.0), 1e-3))
            else:
                most = int(np.iinfo(b.dtype).max)
                b //= min(most, max(1, int(np.ceil(abs(c["scale"] or 1.0) * most * 2 / span))))
        rec.append((b, v, c))
    return with_planes(r, names(rec), d0)


AFFINE_TERMS = ("none", "scalar", "table")


def affine_field(r, d0, room, first, narrow=False):
    """(base, view, conversion, affine or None, (scale term, bias term)): an entry of
    affine_records.CONVS or a quantise of a random pair, under a scale and a bias that are each
    absent, one number or a table along a random dimension of the view."""
    if narrow or r.random() < 0.3:
        c = dict(quant_conv(r, narrow), scale=None)
    else:
        c = dict(ar.CONVS[int(r.integers(0, len(ar.CONVS)))])
    while True:
        st, bt = (AFFINE_TERMS[int(r.integers(0, 3))] for _ in range(2))
        if not first or bt != "none" or st == "table":  # (the first field runs the affine step)
            break
    b, v = view(r, None, d0=d0, max_elems=room, src=c["src"], shift=0)
    axis = int(r.choice([0, v.ndim - 1, int(r.integers(0, v.ndim))]))
    seed = int(r.integers(0, 1 << 16))
    if st == "scalar":
        c["scale"] = [0.5, 1 / 255, 3.0, -1.0][int(r.integers(0, 4))]
    if st != "table" and bt == "none":  # (no affine entry: a conversion as it was)
        if st == "none" and not qr.is_quant(c) and c["src"] == c["dst"]:
            st, c["scale"] = "scalar", 3.0  # (without a scale it would be no cast)
        return b, v, c, None, (st, bt)
    a = ar.affine(ar.table(v.shape[axis], seed) if st == "table" else None,
                  ar.table(v.shape[axis], seed + 1, "bias") if bt == "table" else None,
                  axis if "table" in (st, bt) else None,
                  [0.75, -1.25, 100.5][int(r.integers(0, 3))] if bt == "scalar" else None)
    return b, v, c, a, (st, bt)


def affine_record(r, n_fields=None, max_elems=MAX_ELEMS, narrow=None):
    """([(name or None, base, view, conversion or None, affine or None)], [(scale term, bias term)
    of every converted field])."""
    if n_fields is None:
        n_fields = int(r.integers(1, 4))
    d0 = int(r.choice(EXTENTS))
    room = max(max_elems // n_fields, 4 * d0)
    narrow = share(r, 0.7, narrow)
    rec, terms = [], []
    for k in range(n_fields):
        if k and r.random() < 0.3:
            rec.append(plain(r, d0, room, 4))
            continue
        *f, t = affine_field(r, d0, room, k == 0, narrow)
        rec.append(tuple(f))
        terms.append(t)
    return with_planes(r, names(rec), d0), terms


def sprinkle(r, b, src):
    """Overwrite a seeded share of base `b` with draws from a small alphabet, so that the argmax
    rule matters: NaN, +-inf, +-0.0 and one repeated finite value for a float source, the minimum,
    the maximum and one repeated value for an integer one."""
    if src in FLOATS:
        alphabet = am.from_f32([np.nan, np.inf, -np.inf, 0.0, -0.0, 2.5], src)
    else:
        info = np.iinfo(b.dtype)
        alphabet = np.array([info.min, info.max, 7], b.dtype)
    # (NaN ends every contest it is in: a rarer letter than the others)
    p = np.array([0.3] + [1.0] * (len(alphabet) - 1)) if src in FLOATS else np.ones(len(alphabet))
    where = r.random(b.shape) < float(r.choice([0.01, 0.03, 0.1, 0.3]))
    b[where] = r.choice(alphabet, int(where.sum()), p=p / p.sum())


DENSE = ("no", "first", "last")


def argmax_field(r, room, d0=None, narrow=False, dense=None):
    """(base, view, reduction): without `d0` the reduced axis is any dimension and C from the
    widened pool; with it the view's leading extent is d0 and the reduced axis lies behind it.
    `dense` (one of DENSE, default: "no" for half of the seeds): the field is a dense (C, n) or
    (n, C) base whose rows start on multiples of 16 bytes, reduced along its first or its last
    dimension, which is what the lane body's vector path and the wave body ask for; the first
    under int64 indices from a 2- or 4-byte source, so that a unit's two sources are aligned
    wherever its index pair is."""
    src = list(cr.SOURCES)[int(r.integers(0, len(cr.SOURCES)))]
    drawn = DENSE[int(r.choice(3, p=[0.5, 0.35, 0.15]))]
    dense = "no" if d0 is not None else drawn if dense is None else dense
    if dense != "no":
        c, n = int(r.choice(ARGMAX_EXTENTS)), int(r.choice([16, 32, 48, 64]))
        axis = int(dense == "last")
        if axis == 0 and src in ("uint8", "int8"):
            src = ["uint16", "int16", "float16", "bfloat16", "float32"][int(r.integers(0, 5))]
        b = fill(None, (c, n) if axis == 0 else (n, c), 0, src, seed=int(r.integers(0, 1 << 16)))
        v = np.flip(b, axis) if r.random() < 0.3 else b
        if axis == 0:
            sprinkle(r, b, src)
            return b, v, am.red(src, axis, "int64")
    elif d0 is None:
        c = int(r.choice(ARGMAX_EXTENTS))
        # (a short axis leaves many outputs, most of them index 0: less room for those)
        few = room if c > 3 else room // (8 * (4 - c))
        b, v = view(r, None, d0=c, max_elems=max(few, 4 * c), src=src, shift=0, nd_min=2)
        axis = int(r.choice([0, v.ndim - 1, int(r.integers(0, v.ndim))]))
        v = np.moveaxis(v, 0, axis)
    else:
        b, v = view(r, None, d0=d0, max_elems=max(room, 4 * d0), src=src, shift=0, nd_min=2)
        # (an extent of 1, which many dimensions of a view have, only now and then)
        longer = [k for k in range(1, v.ndim) if v.shape[k] > 1]
        axis = int(r.choice(longer)) if longer and r.random() < 0.9 else int(r.integers(1, v.ndim))
    sprinkle(r, b, src)
    # (`narrow`: the narrowest index that holds C - 1, for destinations at odd addresses)
    return b, v, am.red(src, axis, am.index_for(v.shape[axis], 0 if narrow else int(r.integers(0, 4))))


def argmax_record(r, n_fields=None, max_elems=MAX_ELEMS, narrow=None, dense=None):
    """[(name or None, base, view, reduction or None)]: the first field reduced along any of its
    dimensions, the ones behind it plain or reduced along a dimension behind the first."""
    if n_fields is None:
        n_fields = int(r.integers(1, 4))
    room = max_elems // n_fields
    narrow = share(r, 0.7, narrow)
    b, v, red = argmax_field(r, room, None, narrow, dense)
    d0 = [n for k, n in enumerate(v.shape) if k != red["axis"]][0]
    rec = [(b, v, red)]
    for k in range(1, n_fields):
        rec.append(plain(r, d0, room) if r.random() < 0.6 else argmax_field(r, room, d0, narrow))
    return with_planes(r, names(rec), d0)


def resize_op(r, v, src, keep0=None, narrow=False):
    """A resize of view `v`: any ordered pair of distinct dimensions, each output extent from
    EXTENTS, the identity or 1, both modes, a destination the source allows; the output capped at
    MAX_ELEMS elements.  `keep0`: the extent dimension 0 keeps or gets."""
    a, b = (int(x) for x in r.choice(v.ndim, 2, replace=False))
    size = []
    for ax in (a, b):
        u = r.random()
        size.append(v.shape[ax] if u < 0.12 else 1 if u < 0.22 else int(r.choice(EXTENTS)))
    if keep0 is not None:
        size = [keep0 if ax == 0 else s for ax, s in zip((a, b), size)]
    rest = v.size // (v.shape[a] * v.shape[b])
    free = [j for j in (0, 1) if keep0 is None or (a, b)[j] != 0]  # (dimension 0 stays as given)
    while size[0] * size[1] * rest > MAX_ELEMS and any(size[j] > 1 for j in free):
        j = max(free, key=lambda j: size[j])
        size[j] = max(e for e in EXTENTS if e < size[j])
    dests = rr.dests_of(src)
    if narrow:  # (8-bit destinations, for records at odd addresses)
        dests = ["uint8", "int8"] + [None] * (src in ("uint8", "int8"))
    elif r.random() < 0.6:  # (and the others mostly to the wider ones)
        dests = ["float16", "float32", "uint16", "int16"]
    return rr.rs(src, (a, b), size, ["nearest", "bilinear"][int(r.integers(0, 2))],
                 dests[int(r.integers(0, len(dests)))])


def resize_field(r, room, d0=None, narrow=False):
    src = list(cr.SOURCES)[int(r.integers(0, len(cr.SOURCES)))]
    b, v = view(r, None, d0=d0, max_elems=max(room, 4 * (d0 or 1)), src=src, shift=0, nd_min=2)
    op = resize_op(r, v, src, d0, narrow)
    for_integers(b, op)
    return b, v, op


def out_shape(v, op):
    shape = list(v.shape)
    for ax, s in zip(op["axes"], op["size"]):
        shape[ax] = s
    return shape


def resize_record(r, n_fields=None, max_elems=MAX_ELEMS, narrow=None):
    """[(name or None, base, view, resize or None)]: a resized field between plain ones, sometimes
    two resized fields."""
    if n_fields is None:
        n_fields = int(r.integers(1, 4))
    room = max_elems // n_fields
    narrow = share(r, 0.7, narrow)
    b, v, op = resize_field(r, room, None, narrow)
    d0 = out_shape(v, op)[0]
    rec = [(b, v, op)]
    for k in range(1, n_fields):
        rec.append(plain(r, d0, room) if r.random() < 0.65 else resize_field(r, room, d0, narrow))
    if len(rec) > 1 and r.random() < 0.5:  # (the resized field between the plain ones)
        rec[0], rec[1] = rec[1], rec[0]
    return with_planes(r, names(rec), d0)


def boxes(r, ia, ib, size, k):
    """K rows: a kind of crop_records.box_kinds, an interior or overhanging box in the manner of
    crop_records.boxes_for, or four words of anything in int32 range; with K >= 1 at least one box
    whose clamped area is not empty."""
    kinds = kr.box_kinds(ia, ib, size)
    rows = []
    for _ in range(k):
        u = r.random()
        if u < 0.2:
            rows.append(kinds[int(r.integers(0, len(kinds)))][1])
        elif u < 0.9:
            lo = [int(r.integers(-3, ia)), int(r.integers(-3, ib))]
            hi = [int(r.integers(max(lo[0], 0) + 1, ia + 4)), int(r.integers(max(lo[1], 0) + 1, ib + 4))]
            rows.append((lo[0], lo[1], hi[0], hi[1]))
        else:
            rows.append(tuple(int(x) for x in r.integers(kr.I32_MIN, kr.I32_MAX + 1, 4)))

    def area(row):
        a0, a1 = (min(max(row[j], 0), ia) for j in (0, 2))
        b0, b1 = (min(max(row[j], 0), ib) for j in (1, 3))
        return max(a1 - a0, 0) * max(b1 - b0, 0)
    if k and not any(area(row) for row in rows):
        rows[int(r.integers(0, k))] = (int(r.integers(-2, 1)), 0, ia, ib + int(r.integers(0, 3)))
    return rows


def crop_field(r, room, k, narrow=False):
    """(base, view, crop) of K boxes of a frame of 2 to 7 dimensions, the output capped at
    MAX_ELEMS elements, the boxes at 0, 4, 8 or 12 mod 16."""
    src = list(cr.SOURCES)[int(r.integers(0, len(cr.SOURCES)))]
    b, v = view(r, None, max_elems=max(room, 4), src=src, shift=0, nd_min=2, nd_max=7)
    op = resize_op(r, v, src, None, narrow)
    for_integers(b, op)
    a, bx = op["axes"]
    size = list(op["size"])
    rest = v.size // (v.shape[a] * v.shape[bx])
    while max(k, 1) * size[0] * size[1] * rest > room and max(size) > 1:
        j = int(np.argmax(size))
        size[j] = max(e for e in EXTENTS if e < size[j])
    rows = boxes(r, v.shape[a], v.shape[bx], size, k)
    return b, v, kr.crop(src, (a, bx), size, rows, op["mode"], op["dst"], mis=4 * int(r.integers(0, 4)))


def crop_record(r, n_fields=None, max_elems=MAX_ELEMS, narrow=None):
    """[(name or None, base, view, crop or None)] over K boxes: K = 0 a bare field of crops; else
    crops beside plain fields of K rows, sometimes a second field of crops by boxes of its own."""
    k = int(r.choice(CROP_COUNTS, p=[0.06, 0.2, 0.2, 0.2, 0.2, 0.14]))  # (K = 0 launches nothing)
    if n_fields is None:
        n_fields = int(r.integers(1, 4)) if k else 1
    room = max_elems // n_fields
    narrow = share(r, 0.7, narrow)
    rec = [crop_field(r, room, k, narrow)]
    for _ in range(1, n_fields):
        rec.append(plain(r, k, room) if r.random() < 0.7 else crop_field(r, room, k, narrow))
    return with_planes(r, names(rec), k)


PREP_FILLS = (114.0, 0.0, -0.0, -2.5, 300.0, -1e6)
PLACEMENTS = ("none", "letterbox", "free")


def prep_reach(v, op):
    """(the largest finite magnitude among the view's values, the magnitude the destination
    holds): their ratio is the scale that brings the one to the other.  A float destination is
    given the source's own reach, held well inside float16."""
    x = np.abs(cr.to_f32(v, op["src"]))
    x = x[np.isfinite(x)]
    most = float(x.max()) if x.size and x.max() > 0 else 1.0
    dst = rr.dst_name(op)
    if dst[0] in "ui":
        return most, float(np.iinfo(np.dtype(dst)).max)
    return most, min(most, 20000.0)


def prep_term(r, form, n, about, unsigned, lead):
    """A scale or a bias of `form`: None, a number of magnitude about `about`, or a table of `n`
    such numbers that starts `lead` words into its base — mostly positive for an unsigned
    destination, now and then with an exact 0.0, -0.0 or 1.0 in one entry."""
    if form == "none":
        return None
    vals = about * r.uniform(0.2, 0.9, n if form == "table" else 1)
    vals = np.where(r.random(len(vals)) < (0.1 if unsigned else 0.5), -vals, vals).astype(np.float32)
    if form == "scalar":
        return float(vals[0])
    if r.random() < 0.3:
        vals[int(r.integers(0, n))] = [0.0, -0.0, 1.0][int(r.integers(0, 3))]
    return pr.table(vals, lead)


def prep_step(r, v, op, crops):
    """The model-input step of `op` (a resize, or with `crops` a crop) over view `v`, never an
    empty one.  Scale and bias are each absent, a number or a table; a table where the view has a
    dimension that is not resized, both along one axis — a broadcast or a reversed dimension more
    often than its turn, negative a third of the time — and 0 to 3 words into their bases.  Their
    magnitudes come from the ratio of the destination's reach to the source's, so that an integer
    destination is filled and not overrun; the bias of an unsigned destination lies inside it.  A
    resize is placed by nothing, by `tensor.letterbox` or by a free `inner` of at least three
    quarters of the output at any `lead`, over a `fill` of PREP_FILLS."""
    from dora_amd import tensor
    nd = v.ndim
    taken = {a % nd for a in op["axes"]}
    free = [k for k in range(nd) if k not in taken]
    still = [k for k in free if v.strides[k] == 0 and v.shape[k] > 1]
    back = [k for k in free if v.strides[k] < 0]
    forms = AFFINE_TERMS if free else AFFINE_TERMS[:2]
    st, bt = (forms[int(r.integers(0, len(forms)))] for _ in range(2))
    if (still or back) and "table" not in (st, bt) and r.random() < 0.8:
        # (a table along a broadcast or a reversed dimension, which few views have)
        st, bt = [("table", bt), (st, "table"), ("table", "table")][int(r.integers(0, 3))]
    place = "none" if crops else PLACEMENTS[int(r.choice(3, p=[0.3, 0.3, 0.4]))]
    if (st, bt, place) == ("none", "none", "none"):
        st = "scalar"  # (an empty step would plan as the plain kernel)
    axis = None
    if "table" in (st, bt):
        if still and r.random() < 0.8:
            axis = int(r.choice(still))
        elif back and r.random() < 0.5:
            axis = int(r.choice(back))
        else:
            axis = int(r.choice([free[0], free[-1], free[int(r.integers(0, len(free)))]]))
    n = v.shape[axis] if axis is not None else 1
    most, reach = prep_reach(v, op)
    unsigned = rr.dst_name(op)[0] == "u"
    signed_src = op["src"] not in ("uint8", "uint16")
    # an unsigned destination of a signed source: half the span each way, the bias in the middle
    half = unsigned and signed_src and st != "none"
    scale = prep_term(r, st, n, reach / most / (2 if half else 1), unsigned, int(r.integers(0, 4)))
    bias = prep_term(r, bt, n, reach * (0.7 if half else 0.4), unsigned, int(r.integers(0, 4)))
    step = pr.prep(scale, bias, None if axis is None else axis - nd if r.random() < 1 / 3 else axis)
    if place != "none":
        size = op["size"]
        if place == "letterbox":
            inner, lead = tensor.letterbox(tuple(v.shape[a % nd] for a in op["axes"]), size)
        else:
            inner = tuple(int(r.integers(-(-3 * s // 4), s + 1)) for s in size)
            lead = tuple(int(r.integers(0, s - i + 1)) for s, i in zip(size, inner))
        fill = PREP_FILLS[int(r.integers(0, len(PREP_FILLS)))]
        if rr.dst_name(op)[0] == "f" and r.random() < 0.5:
            fill = -0.0  # (few destinations are floats: the zero whose sign the product keeps)
        step.update(inner=tuple(inner), lead=tuple(lead), fill=fill)
    return step


def with_steps(r, rec, crops):
    """`rec` with a model-input step on its first op field and on about 0.6 of the others."""
    first = True
    for _, _, v, op in rec:
        if op is None:
            continue
        op["prep"] = prep_step(r, v, op, crops) if first or r.random() < 0.6 else None
        first = False
    return rec


def prep_resize_record(r, n_fields=None, max_elems=MAX_ELEMS, narrow=None):
    """`resize_record`'s record as tests/prep_records.py takes it: every resize with one more key,
    "prep", the first one's a step, the others' a step or None."""
    return with_steps(r, resize_record(r, n_fields, max_elems, narrow), False)


def prep_crop_record(r, n_fields=None, max_elems=MAX_ELEMS, narrow=None):
    """`crop_record`'s record with steps in the same way (no placement: crops have none)."""
    return with_steps(r, crop_record(r, n_fields, max_elems, narrow), True)


def misaligned_op(r, op):
    """The record of `op` ("quant", "affine", "argmax", "resize", "crop", "prep_resize",
    "prep_crop"): an aligned plain field in front of an op field whose 2- or 4-byte source starts 1
    or 3 bytes past a multiple of its element size: no kernel runs it.  The last two are the
    resize's and the crops' record with a scalar scale and bias on `f1`."""
    if op.startswith("prep_"):
        rec = misaligned_op(r, op[len("prep_"):])
        rec[1][3]["prep"] = pr.prep(scale=0.5, bias=1.0)
        return rec
    d0 = int(r.choice(EXTENTS[:8]))
    src = ["uint16", "int16", "float16", "bfloat16", "float32"][int(r.integers(0, 5))]
    a, va = view(r, np.uint8, d0=d0, max_elems=2000)
    b, vb = view(r, None, d0=None if op == "crop" else d0, max_elems=2000, src=src,
                 shift=int(r.choice([1, 3])), nd_min=2, nd_max=7)
    if op == "quant":
        return [("f0", a, va, None), ("f1", b, vb, qr.quant(src, "uint8", 0.5, 128))]
    if op == "affine":
        return [("f0", a, va, None, None),
                ("f1", b, vb, cr.cast(src, "float32"), ar.both(vb.shape[1], 1, 3))]
    if op == "argmax":
        return [("f0", a, va, None), ("f1", b, vb, am.red(src, 1, "int64"))]
    if op == "resize":
        return [("f0", a, va, None), ("f1", b, vb, rr.rs(src, (0, 1), (d0, 3), "bilinear", "float32"))]
    rows = boxes(r, vb.shape[0], vb.shape[1], (2, 3), d0)
    return [("f0", a, va, None), ("f1", b, vb, kr.crop(src, (0, 1), (2, 3), rows, "nearest", "float32"))]
