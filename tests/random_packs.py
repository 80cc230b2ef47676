"""Seeded random segment layouts for the pack bodies (dora_amd/csrc/pack_device.h `pack_chunk` /
`pack_body`), the numpy reference of a pack and a Python statement of the rules the host builders
and the kernel share (`segment_chunks`, `edge_mask`, chunk windows, head / tail paths), for
tests/test_random_packs_host.py (argument blocks and generator coverage, on the CPU) and
tests/test_gpu_random_packs.py (the kernels).  One integer names a case: `case(body, seed)` and
the same calls in the same order reproduce it, and every failure message prints `seed=`.  No test
lives here.

Bodies (include/dora_gpu_testing.h dora_gpu_test_pack_segments): 0 the product's launch_pack,
1 the write-through body over PackArgs, 2 the coherent-load body over AqlPackArgs, 3 the batch body
over AqlBatchArgs.

A case is one or (body 3) several messages, each a destination inside one destination allocation
and sorted, disjoint segments (source position, destination offset, length).  All positions are
offsets from the two allocations' starts, which are taken to be 256-byte aligned."""
import ctypes
import struct

import numpy as np

from dora_amd import _lib

LINE = 128
GRAIN = 8192
GUARD = 256
SIGNAL_GRID = 1024
DST_BYTES = 1 << 20
SRC_BYTES = (1 << 20) + (1 << 18)
BUDGET = 640 << 10            # bytes of all segments of a case
MAX_SEGS = {0: 40, 1: 32, 2: 8, 3: 8}
BODIES = (0, 1, 2, 3)


def rng(seed):
    return np.random.default_rng(seed)


def splitmix_bytes(seed, n):
    """n bytes of the splitmix64 stream of `seed` (little-endian words)."""
    words = (n + 7) // 8
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * np.arange(1, words + 1, dtype=np.uint64)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    return z.view(np.uint8)[:n].copy()


def source_bytes():
    return splitmix_bytes(0x5EED5, SRC_BYTES)


def background_bytes():
    return splitmix_bytes(0xBAC6, DST_BYTES)


# ----------------------------------------------------------------------------------------------
# The rules, stated once in Python (pack_device.h segment_chunks / pack_chunk, kernels.hip
# edge_mask / pack_grid).  Addresses are absolute.
# ----------------------------------------------------------------------------------------------
def segment_chunks(d0, length, chunk):
    a0 = (d0 + 15) & ~15
    a1 = (d0 + length) & ~15
    if a1 <= a0:
        return 1
    o = a0 & ~(LINE - 1)
    return (a1 - o + chunk - 1) // chunk


def edge_mask(segs, dst, cap):
    """segs: (src, dst_off, len) of one message at address `dst` with `cap` writable bytes."""
    if not cap or len(segs) > 32:
        return 0
    for k in range(1, len(segs)):
        if segs[k][1] < segs[k - 1][1] + segs[k - 1][2]:
            return 0

    def inside(u):
        return u >= dst and u + 16 <= dst + cap

    def hidden(k, unit):
        """The kernel leaves a stitched head unit to the lowest segment holding a byte of it, which
        takes it only if seg[j - 1] ends before the unit: an empty seg[j - 1] inside the unit hides
        the owner, and no head in that unit is stitched."""
        j = k
        for p in range(k - 1, -1, -1):
            if not segs[p][2]:
                continue
            if dst + segs[p][1] + segs[p][2] <= unit:
                break
            j = p
        return (dst + segs[j][1] > unit and j > 0 and segs[j - 1][2] == 0
                and dst + segs[j - 1][1] > unit)
    m = 0
    for k, (_, off, n) in enumerate(segs):
        d0, d1 = dst + off, dst + off + n
        if d1 == d0:
            continue
        a0 = (d0 + 15) & ~15
        if a0 > d0 and inside(a0 - 16) and not hidden(k, a0 - 16):
            m |= 1 << (2 * k)
        if a0 < d1 and (d1 & 15) and inside(d1 & ~15):
            m |= 2 << (2 * k)
    return m


def windows(d0, length, chunk):
    """Chunk windows of the body of segment [d0, d0 + length): [(lo, hi)] per chunk, empty list
    without a body."""
    a0 = (d0 + 15) & ~15
    a1 = (d0 + length) & ~15
    if a1 <= a0:
        return []
    o = a0 & ~(LINE - 1)
    out = []
    for c in range(segment_chunks(d0, length, chunk)):
        lo, hi = o + c * chunk, o + (c + 1) * chunk
        out.append((max(lo, a0), min(hi, a1)))
    return out


class Case:
    """body, seed, msgs [(dst position, cap, [(src position, dst_off, len)])], chunk, grid_pick."""

    def __init__(self, body, seed, msgs, chunk, grid_pick):
        self.body, self.seed, self.msgs, self.chunk, self.grid_pick = body, seed, msgs, chunk, grid_pick

    @property
    def chunk_eff(self):
        return self.chunk or GRAIN   # every case is far below the size at which chunks grow

    def flat(self, dst0=0, src0=0):
        """The launch's segments as the argument block has them: (src, dst, len, edge bits, msg),
        absolute, sorted by destination for a batch."""
        out = []
        for m, (pos, cap, segs) in enumerate(self.msgs):
            em = edge_mask(segs, dst0 + pos, cap)
            for k, (s, off, n) in enumerate(segs):
                out.append((src0 + s, dst0 + pos + off, n, (em >> (2 * k)) & 3, m))
        if self.body == 3:
            out.sort(key=lambda x: x[1])
        return out

    def launches(self, dst0=0, src0=0):
        """Body 0 packs more than 32 segments in launches of 32, none of them stitched."""
        f = self.flat(dst0, src0)
        if len(f) <= 32:
            return [f]
        return [[(s, d, n, 0, m) for (s, d, n, _, m) in f[i:i + 32]] for i in range(0, len(f), 32)]

    def n_chunks(self, dst0=0):
        return sum(segment_chunks(d, n, self.chunk_eff) for _, d, n, _, _ in self.flat(dst0))

    def grid(self, dst0=0):
        """The grid override handed to the hook (0: the product's choice)."""
        if self.body == 0 or self.grid_pick == 0:
            return 0
        n = self.n_chunks(dst0)
        return n if self.grid_pick < 0 else min(self.grid_pick, n)

    def grid_expected(self, dst0=0):
        n = self.n_chunks(dst0)
        return self.grid(dst0) or (n if self.body == 0 else min(n, SIGNAL_GRID))

    def reference(self, bg, src):
        out = bg.copy()
        for pos, _, segs in self.msgs:
            for s, off, n in segs:
                out[pos + off:pos + off + n] = src[s:s + n]
        return out

    def __repr__(self):
        return (f"body={self.body} seed={self.seed} chunk={self.chunk} grid_pick={self.grid_pick} "
                f"msgs={self.msgs}")


def facts(c, dst0=0, src0=0):
    """What the kernel does with every segment of case `c`, by the rules of pack_chunk: a list of
    dicts per launch segment (head / tail path, ownership, residue class, skip, chunks)."""
    out = []
    for launch in c.launches(dst0, src0):
        for s, (src, d0, n, em, _) in enumerate(launch):
            d1 = d0 + n
            a0, a1 = (d0 + 15) & ~15, d1 & ~15
            body = a1 > a0
            has_head = n > 0 and a0 > d0
            has_tail = a0 < d1 and (d1 & 15) != 0
            st_head, st_tail = has_head and bool(em & 1), has_tail and bool(em & 2)
            h = a0 - 16
            own = st_head and (s == 0 or launch[s - 1][1] + launch[s - 1][2] <= h)
            # bytes of other segments in this segment's head unit
            sharers = sum(1 for (_, e0, en, _, _) in launch if en and e0 < h + 16 and e0 + en > h) \
                if has_head else 0
            earlier = any(en and e0 + en > h for (_, e0, en, _, _) in launch[:s]) if has_head else False
            hidden = (has_head and s > 0 and launch[s - 1][2] == 0 and launch[s - 1][1] > h
                      and not earlier)
            out.append(dict(
                n=n, body=body, chunks=segment_chunks(d0, n, c.chunk_eff),
                residue=(src - d0) & 15, skip=((a0 & (LINE - 1)) >> 4) if body else None,
                head="none" if not has_head else "bytes" if not st_head else "own" if own else "left",
                tail="none" if not has_tail else "bytes" if not st_tail else "stitched",
                sharers=sharers, hidden=hidden))
    return out


def emulate(c, bg, src):
    """The pack of case `c` by pack_chunk's own rules, byte for byte: heads and tails stored by
    bytes or as whole stitched units gathered from the launch's segments (a head unit only by the
    segment the ownership rule names), bodies chunk window by chunk window.  Equal to
    `c.reference` exactly if the rules and the edge bits write every segment byte and nothing
    else."""
    out = bg.copy()
    for launch in c.launches():
        def unit(u):
            v = out[u:u + 16].copy()
            for (sp, e0, en, _, _) in launch:
                lo, hi = max(u, e0), min(u + 16, e0 + en)
                if lo < hi:
                    v[lo - u:hi - u] = src[sp + lo - e0:sp + hi - e0]
            return v
        for s, (sp, d0, n, em, _) in enumerate(launch):
            d1 = d0 + n
            a0, a1 = (d0 + 15) & ~15, d1 & ~15
            has_head = n > 0 and a0 > d0
            has_tail = a0 < d1 and (d1 & 15) != 0
            if has_head and not em & 1:
                hend = min(a0, d1)
                out[d0:hend] = src[sp:sp + hend - d0]
            if has_tail and not em & 2:
                t0 = max(a1, a0)
                out[t0:d1] = src[sp + t0 - d0:sp + n]
            if has_head and em & 1 and (s == 0 or launch[s - 1][1] + launch[s - 1][2] <= a0 - 16):
                out[a0 - 16:a0] = unit(a0 - 16)
            if has_tail and em & 2:
                out[d1 & ~15:(d1 & ~15) + 16] = unit(d1 & ~15)
            for lo, hi in windows(d0, n, c.chunk_eff):
                out[lo:hi] = src[sp + lo - d0:sp + hi - d0]
    return out


def owner(c, offset):
    """(message, segment, chunk or None, (src - dst) mod 16) of the byte at `offset` of the
    destination allocation, or None for a byte no segment holds."""
    for m, (pos, _, segs) in enumerate(c.msgs):
        for k, (s, off, n) in enumerate(segs):
            if pos + off <= offset < pos + off + n:
                chunk = None
                for i, (lo, hi) in enumerate(windows(pos + off, n, c.chunk_eff)):
                    if lo <= offset < hi:
                        chunk = i
                return m, k, chunk, (s - pos - off) & 15
    return None


# ----------------------------------------------------------------------------------------------
# The generator
# ----------------------------------------------------------------------------------------------
def _gap(r):
    k = r.choice(4, p=(0.55, 0.15, 0.15, 0.15))
    return 0 if k == 0 else int(r.integers(1, 4)) if k == 1 else int(r.integers(4, 16)) if k == 2 \
        else int(r.integers(16, 201))


def _length(r, start, chunk, room):
    """(extra gap, length) of a segment whose first byte would lie at absolute `start`."""
    small = room < 2 * chunk + 64
    k = int(r.choice(6, p=(0.10, 0.15, 0.15, 0.20, 0.20, 0.20)))
    if small and k >= 4:
        k = int(r.integers(0, 4))
    res = start & 15
    if k == 0:
        return 0, 0
    if k == 1:    # wholly inside one unit
        return 0, int(r.integers(1, min(15, 16 - res) + 1))
    if k == 2:    # a head and a tail, no body
        extra = 0 if res else int(r.integers(1, 16))
        return extra, (16 - ((start + extra) & 15)) + int(r.integers(1, 16))
    if k == 3:
        return 0, int(r.integers(16, 49))
    if k == 4:
        return 0, chunk + int(r.integers(-17, 18))
    hi = min(5 * chunk, room - 64)
    return 0, int(r.integers(2 * chunk, hi + 1))


def _message(r, base, nseg, chunk, budget, deal):
    """Segments (dst_off, len) of one message at absolute address `base`.  `deal`: a layout the
    sweep must see in known numbers — 1 three segments in one unit, 2 an empty segment inside its
    follower's head unit with no earlier owner, 3 a segment of whole units."""
    segs = []
    off = 0
    forced = {}
    if deal == 1 and nseg >= 3:
        j = int(r.integers(0, nseg - 2))
        forced = {j: "tiny0", j + 1: "tiny", j + 2: "join"}
    elif deal == 2 and nseg >= 2:
        j = int(r.integers(0, nseg - 1))
        forced = {j: "hole", j + 1: "after"}
    elif deal == 3:
        forced = {int(r.integers(0, nseg)): "aligned"}
    k = 0
    while k < nseg:
        f = forced.get(k)
        gap = _gap(r)
        if f == "tiny0":     # starts early in a unit, two more segments follow inside it
            start = base + off + gap
            gap += (16 - (start & 15)) & 15 if (start & 15) > 6 else 0
            n = int(r.integers(1, 4))
        elif f == "aligned":   # whole units: neither head nor tail
            gap += (16 - ((base + off + gap) & 15)) & 15
            n = 16 * int(r.integers(1, 4)) if r.random() < 0.5 or budget < 3 * chunk else \
                chunk + 16 * int(r.integers(0, 3))
        elif f == "tiny":
            gap, n = int(r.integers(0, 2)), int(r.integers(1, 4))
        elif f == "join":
            gap, (extra, n) = 0, _length(r, base + off, chunk, budget)
            if n == 0 or extra:
                gap, n = 0, int(r.integers(1, 40))
        elif f == "hole":
            # the unit before holds no byte: the empty segment lies 1-15 bytes into a fresh unit
            start = (base + off + gap + 15) & ~15
            if segs and start - 16 < base + off:
                start += 16
            inner = int(r.integers(1, 16))
            at = start + int(r.integers(1, inner + 1))
            segs.append((at - base, 0))
            off = start + inner - base
            k += 1
            n = int(r.integers(1, 16)) if r.random() < 0.3 else int(r.choice((40, chunk + 5)))
            n = min(n, max(1, budget - 64))
            segs.append((off, n))
            off += n
            budget -= n
            k += 1
            continue
        else:
            extra, n = _length(r, base + off + gap, chunk, budget)
            gap += extra
        segs.append((off + gap, n))
        off += gap + n
        budget -= n
        k += 1
    return segs, budget


def case(body, seed):
    r = rng([body, seed])
    chunk = int(r.choice((0, GRAIN, 2 * GRAIN))) if body else 0
    grid_pick = int(r.choice((0, 1, 2, 3, -1))) if body else 0
    cap_case = int(r.integers(0, 3))
    if body == 0:
        nseg = int(r.integers(33, 41)) if seed % 4 == 3 else \
            int(r.integers(9, 33)) if seed % 4 == 1 else int(r.integers(1, 9))
    elif body == 1:
        nseg = int(r.integers(9, 33)) if seed % 2 else int(r.integers(1, 9))
    else:
        nseg = int(r.integers(1, 9))
    deal = {1: 1, 2: 2, 3: 3, 5: 1, 6: 2}.get(seed % 8, 0)
    nmsg = int(r.integers(1, nseg + 1)) if body == 3 else 1
    cuts = sorted(r.choice(np.arange(1, nseg), nmsg - 1, replace=False).tolist()) if nmsg > 1 else []
    counts = [b - a for a, b in zip([0] + cuts, cuts + [nseg])]
    eff = chunk or GRAIN
    budget = BUDGET
    msgs = []
    pos = GUARD
    spos = GUARD
    order = r.permutation(nmsg)
    placed = {}
    # destinations in shuffled order through the allocation, so message order is not address order
    for m in order:
        start = ((pos + LINE - 1) & ~(LINE - 1)) + int(r.integers(0, LINE))
        segs, budget = _message(r, start, counts[m], eff, budget, deal if m == order[0] else 0)
        extent = max([o + n for o, n in segs] + [0])
        ccase = cap_case if nmsg == 1 else int(r.integers(0, 3))
        cap = extent if ccase == 0 else extent + 64 if ccase == 1 else 0
        full = []
        for off, n in segs:
            s = ((spos + 15) & ~15) + int(r.integers(0, 16))
            full.append((s, off, n))
            spos = s + n + 48
        placed[m] = (start, cap, full)
        pos = start + max(cap, extent) + GUARD + int(r.integers(0, 64))
    msgs = [placed[m] for m in range(nmsg)]
    assert pos + GUARD <= DST_BYTES and spos + GUARD <= SRC_BYTES, (body, seed)
    return Case(body, seed, msgs, chunk, grid_pick)


def empty_hole_case(body):
    """The layout built by hand: a base at 4 mod 16, a 12-byte segment ending on a unit boundary, an
    empty segment at offset 16 (inside the next unit) and a segment at offset 16 whose head unit
    nobody else holds.  Generous capacity, so the head would be stitched."""
    start = GUARD + 4
    segs = [(GUARD, 0, 12), (GUARD + 64, 16, 0), (GUARD + 131, 16, 8192 + 40)]
    return Case(body, -1, [(start, 16 + 8192 + 40 + 64, segs)], 0, 0)


# ----------------------------------------------------------------------------------------------
# The hooks
# ----------------------------------------------------------------------------------------------
def _marshal(c, dst0, src0):
    n = len(c.msgs)
    counts = (ctypes.c_size_t * n)(*[len(m[2]) for m in c.msgs])
    flat = [x for pos, _, segs in c.msgs for (s, off, ln) in segs for x in (src0 + s, off, ln)]
    segs = (ctypes.c_uint64 * max(1, len(flat)))(*flat)
    dsts = (ctypes.c_uint64 * n)(*[dst0 + m[0] for m in c.msgs])
    caps = (ctypes.c_uint64 * n)(*[m[1] for m in c.msgs])
    return n, counts, segs, dsts, caps


def pack_args(c, dst0, src0):
    """(rc, parsed argument block) of case `c` from dora_gpu_test_pack_args: nothing is launched."""
    lib = _lib.load_testing()
    n, counts, segs, dsts, caps = _marshal(c, dst0, src0)
    out = ctypes.create_string_buffer(1024)
    got = ctypes.c_size_t()
    rc = lib.dora_gpu_test_pack_args(c.body, n, counts, segs, dsts, caps, c.chunk, c.grid(dst0),
                                     out, len(out), ctypes.byref(got))
    return rc, (parse(c.body, out.raw[:got.value]) if rc == 0 else None)


def pack(c, dst0, src0, stream=None):
    """Run case `c` on the GPU; returns the bit mask of messages whose flag holds its epoch."""
    lib = _lib.load_testing()
    n, counts, segs, dsts, caps = _marshal(c, dst0, src0)
    ok = ctypes.c_uint32()
    rc = lib.dora_gpu_test_pack_segments(c.body, n, counts, segs, dsts, caps, c.chunk,
                                         c.grid(dst0), stream, ctypes.byref(ok))
    assert rc == 0, (_lib.load().dora_gpu_last_error(), c)
    return ok.value


def parse(body, raw):
    """The argument block of a body: PackArgs (952 bytes), AqlPackArgs (280), AqlBatchArgs (640)."""
    dst, flag, done, epoch = struct.unpack_from("<4Q", raw, 0)
    n_chunks, nseg, chunk, grid = struct.unpack_from("<4I", raw, 32)
    edge, = struct.unpack_from("<Q", raw, 48)
    slots, ce, sg = {0: (32, 56, 184), 1: (32, 56, 184), 2: (8, 56, 88), 3: (16, 64, 128)}[body]
    assert len(raw) == {0: 952, 1: 952, 2: 280, 3: 640}[body], len(raw)
    chunk_end = struct.unpack_from(f"<{slots}I", raw, ce)
    seg = [struct.unpack_from("<3Q", raw, sg + 24 * k) for k in range(slots)]
    p = dict(dst=dst, flag=flag, done=done, epoch=epoch, n_chunks=n_chunks, nseg=nseg, chunk=chunk,
             grid=grid, edge=edge, chunk_end=chunk_end, seg=seg)
    if body == 3:
        p["nmsg"], = struct.unpack_from("<I", raw, 56)
        p["msg"] = [struct.unpack_from("<2Q", raw, 512 + 16 * k) for k in range(8)]
    return p
