"""Seeded random views, records, indices, masks and partitions for the sweeps of
tests/test_random_views_host.py (the sanitized emulations) and tests/test_gpu_random_views.py (the
kernels): plain functions of a numpy.random.Generator, so that one integer names a case —
`rng(seed)` and the same calls in the same order reproduce it, and every failure message of the
sweeps prints `seed=`.  No test lives here.

A view has 1 to 6 dimensions (8 for an occasional seed) with extents from a pool around the edges
of the 16-byte unit and the 16-, 32- and 64-element tiles, a step of 1, 2, 3, -1 or -2 and up to
two elements of slack on either side in every dimension of its base, the dimensions permuted,
sometimes one of them broadcast (stride 0: dimension 0 and the innermost one each get their
turn), and sometimes a base whose first byte is not a multiple of the element size."""
import numpy as np

from tests import cast_records as cr
from tests import mask_records as mr
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


def view(r, dtype, d0=None, max_elems=MAX_ELEMS, src=None, shift=None):
    """(base, view) of `dtype` (or of cast source `src`); with `d0`, dimension 0 of the view has
    that extent and stays in front, whichever dimension of the base it is.  `shift`: the bytes
    the base starts past a multiple of its element size (default: 0 for most seeds, 1 or 3 for a
    tenth of those whose elements are wider than a byte)."""
    nd = 8 if r.random() < 0.12 else int(r.integers(1, 7))
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
