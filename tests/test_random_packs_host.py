"""The seeded pack sweep on the CPU (tests/random_packs.py): for every seed of every body the
argument block that dora_gpu_test_pack_args fills through the product's builders (kernels.hip
finish_args / edge_mask / build_aql_batch_args, pack_device.h chunk_layout) against the Python
statement of the same rules; the chunk windows under that chunk count; and the generator's
coverage, as counts of seeds that show each path of pack_chunk.  tests/test_gpu_random_packs.py runs
the same seeds through the kernels.  To reproduce a case call `random_packs.case(body, seed)`."""
import collections

import pytest

from dora_amd import _lib
from tests import random_packs as rp

SEEDS = 200
DST0 = 0x7F0000000000   # the two allocations, as 256-byte aligned addresses no one dereferences
SRC0 = 0x7E0000000000
MIN_SEEDS = 5


@pytest.mark.parametrize("body", rp.BODIES)
def test_argument_blocks_match_the_stated_rules(body):
    for seed in range(SEEDS):
        c = rp.case(body, seed)
        rc, p = rp.pack_args(c, DST0, SRC0)
        assert rc == 0, (_lib.load().dora_gpu_last_error(), c)
        want = c.launches(DST0, SRC0)[0]
        chunk = c.chunk_eff
        assert p["chunk"] == chunk and p["nseg"] == len(want), c
        assert p["dst"] == (0 if body == 3 else DST0 + c.msgs[0][0]), c
        base = 0 if body == 3 else p["dst"]
        total = 0
        for k, (src, d, n, e, _) in enumerate(want):
            assert p["seg"][k] == (src, d - base, n), (k, c)
            total += rp.segment_chunks(d, n, chunk)
            assert p["chunk_end"][k] == total, (k, c)
            assert (p["edge"] >> (2 * k)) & 3 == e, (k, c)
        assert p["edge"] >> (2 * len(want)) == 0, c
        assert p["n_chunks"] == total, c
        if len(c.launches()) == 1:
            assert total == c.n_chunks(DST0)
            assert p["grid"] == c.grid_expected(DST0), c
        else:   # launch_pack's first launch of several: one workgroup per chunk
            assert p["grid"] == total and p["edge"] == 0, c
        if body == 3:
            assert p["nmsg"] == len(c.msgs), c
            epochs = [e for _, e in p["msg"][:len(c.msgs)]]
            assert len(set(epochs)) == len(epochs) and p["epoch"] == epochs[0], c
            assert len({f for f, _ in p["msg"][:len(c.msgs)]}) == len(c.msgs), c
        assert (p["flag"] != 0) == (body != 0), c


@pytest.mark.parametrize("body", rp.BODIES)
def test_chunk_windows_tile_every_body(body):
    for seed in range(SEEDS):
        c = rp.case(body, seed)
        for _, d0, n, _, _ in c.flat(DST0, SRC0):
            w = rp.windows(d0, n, c.chunk_eff)
            a0, a1 = (d0 + 15) & ~15, (d0 + n) & ~15
            if a1 <= a0:
                assert w == []
                continue
            # consecutive, inside the body, covering it once; the last one is not empty
            assert w[0][0] == a0 and w[-1][1] == a1 and w[-1][1] > w[-1][0], (seed, d0, n)
            for (l0, h0), (l1, h1) in zip(w, w[1:]):
                assert h0 == l1 and h0 > l0, (seed, d0, n)
            assert sum(h - l for l, h in w) == a1 - a0


@pytest.mark.parametrize("body", rp.BODIES)
def test_the_stated_rules_write_every_segment_byte_and_nothing_else(body):
    """pack_chunk's head, tail, ownership and chunk rules, restated byte for byte over the edge
    bits the host builders give (held to the product's above), against the plain reference: a
    stitched unit that the ownership rule leaves to a segment that does not write it shows here,
    without a GPU."""
    import numpy as np
    bg, src = rp.background_bytes(), rp.source_bytes()
    for c in [rp.case(body, seed) for seed in range(SEEDS)] + [rp.empty_hole_case(body)]:
        got, want = rp.emulate(c, bg, src), c.reference(bg, src)
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            pytest.fail(f"seed={c.seed} body={body}: offset {i}, owner {rp.owner(c, i)}; {c!r}")


def _coverage(body):
    """Seeds of `body` that show each condition."""
    cov = collections.Counter()
    for seed in range(SEEDS):
        c = rp.case(body, seed)
        f = rp.facts(c, DST0, SRC0)
        seen = set()
        for x in f:
            if x["body"] and x["chunks"] >= 2:
                seen.add(("residue", x["residue"]))
            if x["body"]:
                seen.add(("skip", x["skip"]))
            seen.add(("head", x["head"]))
            seen.add(("tail", x["tail"]))
            if x["sharers"] >= 3:
                seen.add("three segments in one unit")
            if x["n"] and x["head"] == "none" and x["tail"] == "none":
                seen.add("neither head nor tail")
            if x["hidden"]:
                seen.add("empty segment hides the head unit's owner")
        if c.grid_expected(DST0) < c.n_chunks(DST0):
            seen.add("grid < n_chunks")
        if len(c.launches()) == 1 and sum(1 for x in f if x["chunks"] > 1) >= 3:
            seen.add("three segments of several chunks")
        if len(f) >= 33:
            seen.add("33 or more segments")
        cov.update(seen)
    return cov


def _wanted(body):
    want = [("residue", r) for r in range(16)] + [("skip", k) for k in range(8)]
    want += [("head", "bytes"), ("tail", "bytes"), "three segments in one unit",
             "neither head nor tail", "three segments of several chunks",
             "empty segment hides the head unit's owner"]
    want += [("head", "own"), ("head", "left"), ("tail", "stitched")]
    if body != 0:
        want.append("grid < n_chunks")   # launch_pack takes one workgroup per chunk
    else:
        want.append("33 or more segments")
    return want


@pytest.mark.parametrize("body", rp.BODIES)
def test_generator_shows_every_path(body):
    cov = _coverage(body)
    want = _wanted(body)
    report = ", ".join(f"{k}: {cov[k]}" for k in want)
    print(f"body {body}: {report}")
    low = [k for k in want if cov[k] < MIN_SEEDS]
    assert not low, f"body {body}: fewer than {MIN_SEEDS} seeds show {low}; counts: {report}"


def test_hand_built_empty_hole_layout_is_stored_by_bytes():
    """An empty segment inside its follower's head unit, no earlier segment in that unit: the
    kernel's ownership rule would leave the unit to the empty segment, so edge_mask does not stitch
    that head."""
    for body in rp.BODIES:
        c = rp.empty_hole_case(body)
        rc, p = rp.pack_args(c, DST0, SRC0)
        assert rc == 0
        f = rp.facts(c, DST0, SRC0)
        assert f[2]["hidden"] and f[2]["head"] == "bytes" and f[2]["tail"] == "stitched"
        assert (p["edge"] >> 4) & 3 == 2, hex(p["edge"])


def test_hook_refuses_what_the_product_never_chooses():
    c = rp.case(1, 0)
    lib = _lib.load_testing()
    for body, chunk, grid, word in ((1, 4096, 0, b"8192"), (1, (4 << 20) + 8192, 0, b"8192"),
                                    (1, 0, 1 << 20, b"grid"), (0, 8192, 0, b"body 0"),
                                    (0, 0, 1, b"body 0"), (4, 0, 0, b"body")):
        n, counts, segs, dsts, caps = rp._marshal(c, DST0, SRC0)
        out = (rp.ctypes.c_char * 1024)()
        got = rp.ctypes.c_size_t()
        rc = lib.dora_gpu_test_pack_args(body, n, counts, segs, dsts, caps, chunk, grid, out, 1024,
                                         rp.ctypes.byref(got))
        assert rc == -1 and word in _lib.load().dora_gpu_last_error(), (body, chunk, grid)
