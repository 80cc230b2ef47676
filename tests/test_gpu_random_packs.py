"""The seeded pack sweep of tests/random_packs.py on the GPU: 200 seeds per body through
dora_gpu_test_pack_segments — the product's launch_pack (0), the write-through body over PackArgs
(1), the coherent-load body over AqlPackArgs (2) and the batch body over AqlBatchArgs (3) — each
into one destination allocation refilled with seeded bytes before every pack and compared whole,
byte for byte, with the numpy reference: the segments' bytes and nothing else, guards of 256 bytes
and more around every destination included.  Signalling bodies must leave every message's flag at
exactly its epoch.  A mismatch names the seed, the first differing offset, the message, segment and
chunk that own it and its (src - dst) mod 16 class; `random_packs.case(body, seed)` reproduces it.
Every source and destination range lies inside the two buffers a test allocates, and the hook
checks them against their allocations before it launches.

One layout is built by hand for every body: an empty segment inside its follower's head unit.  The
struct planner refuses a field without values unless the whole record is empty, so through the
plan API the nearest layout is a record of dense fields packed to dst + 4.

The last test sends device bytes through the real AQL code object (one dataflow, two nodes on GPU
0): every source residue at sizes around the unit, the chunk and the read-signalled threshold,
then a held backlog of eight ragged messages that leaves as a batch pack; the received bytes are
downloaded and compared with the source's."""
import ctypes
import threading
import time

import numpy as np
import pytest

from tests import random_packs as rp

pytestmark = pytest.mark.gpu

SEEDS = 200


@pytest.fixture(scope="module")
def dev():
    from dora_amd import device
    assert device.device_count() >= 1
    device.set_device(0)
    s = device.Stream()
    yield s
    s.close()


class Buffers:
    """The source, the destination and the destination's seeded background in device memory, with
    their host copies, allocated once per module."""

    def __init__(self, stream):
        from dora_amd.device import DeviceBuffer
        self.stream = stream
        self.src_host = rp.source_bytes()
        self.bg_host = rp.background_bytes()
        self.src = DeviceBuffer.from_bytes(self.src_host.tobytes(), stream)
        self.bg = DeviceBuffer.from_bytes(self.bg_host.tobytes(), stream)
        self.dst = DeviceBuffer(rp.DST_BYTES)
        assert self.src.ptr % 256 == 0 and self.dst.ptr % 256 == 0
        self.got = np.empty(rp.DST_BYTES, np.uint8)

    def run(self, c):
        """Pack case `c` into the refilled destination; (flag bits, the whole allocation)."""
        from dora_amd._lib import call
        h = self.stream.handle
        call("dora_gpu_memcpy_async", self.dst.ptr, self.bg.ptr, rp.DST_BYTES, h)
        ok = rp.pack(c, self.dst.ptr, self.src.ptr, h)
        call("dora_gpu_memcpy_async", self.got.ctypes.data, self.dst.ptr, rp.DST_BYTES, h)
        self.stream.sync()
        return ok, self.got

    def free(self):
        for b in (self.src, self.bg, self.dst):
            b.free()


@pytest.fixture(scope="module")
def bufs(dev):
    b = Buffers(dev)
    yield b
    b.free()


def verdict(c, ok, got, want):
    """None if case `c` arrived, else what went wrong."""
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        return (f"seed={c.seed} body={c.body}: first differing offset {i} (got {got[i]:#04x}, want "
                f"{want[i]:#04x}); owner (message, segment, chunk, (src - dst) mod 16) = "
                f"{rp.owner(c, i)}; {c!r}")
    flags = (1 << len(c.msgs)) - 1 if c.body else 0
    if ok != flags:
        return f"seed={c.seed} body={c.body}: flags at their epoch {ok:#x}, expected {flags:#x}; {c!r}"
    return None


@pytest.mark.parametrize("body", rp.BODIES)
def test_seeded_layouts_arrive_byte_exact(bufs, body):
    t0 = time.perf_counter()
    failed = []
    for seed in range(SEEDS):
        c = rp.case(body, seed)
        ok, got = bufs.run(c)
        v = verdict(c, ok, got, c.reference(bufs.bg_host, bufs.src_host))
        if v:
            failed.append(v)
    print(f"body {body}: {SEEDS} seeds in {time.perf_counter() - t0:.2f} s, {len(failed)} failed")
    assert not failed, f"{len(failed)} of {SEEDS} seeds failed; the first: {failed[0]}"


@pytest.mark.parametrize("body", rp.BODIES)
def test_empty_segment_inside_its_followers_head_unit(bufs, body):
    c = rp.empty_hole_case(body)
    ok, got = bufs.run(c)
    v = verdict(c, ok, got, c.reference(bufs.bg_host, bufs.src_host))
    assert v is None, v


def test_dense_record_packed_four_bytes_past_a_unit(dev):
    """Through the plan API: a field without values is refused by name (only a whole record may be
    empty), so no plan holds an empty segment before a head unit; the dense record with a 12-byte
    first field arrives at dst + 4 byte for byte, its padding and guards untouched."""
    from dora_amd._lib import ARROW_DEVICE_ROCM, DoraGpuError
    from tests import struct_records as sr
    from tests.gather_views import base
    from tests.test_gpu_tensor_struct_device import Uploaded, check_sample, pack_guarded
    a, e, b = base(np.float32, (3,)), base(np.float64, (3, 0)), base(np.uint8, (3, 2811))
    up = Uploaded([("a", a, a), ("b", b, b)], dev)
    try:
        with pytest.raises(DoraGpuError, match="field 1 `e`"):
            sr.plan_record([("a", a, a), ("e", e, e), ("b", b, b)],
                           lambda x: up.ptr_of(a if x is e else x), ARROW_DEVICE_ROCM)
        rec = [("a", a, a), ("b", b, b)]
        sample, info, ranges = sr.oracle(rec)
        assert ranges[0] == (0, 12)
        with sr.plan_record(rec, up.ptr_of, ARROW_DEVICE_ROCM) as p:
            assert len(p.segments()) == 2 and p.type_info().to_json() == info.to_json()
            got, intact = pack_guarded(p, dev, 4)
            assert intact
            check_sample(got, sample, ranges, "destination 4 mod 16")
    finally:
        up.free()


def _nodes(df, spec):
    from dora_amd.node import Node
    out = {}

    def mk(i, d):
        out[i] = Node(i, dataflow=df.shm, device=d)
    ts = [threading.Thread(target=mk, args=(i, d)) for i, d in spec.items()]
    [t.start() for t in ts]
    [t.join(90) for t in ts]
    assert set(out) == set(spec)
    return out


CHUNK = 8192
SMALL = list(range(1, 48)) + [CHUNK - 17, CHUNK, CHUNK + 17, 3 * CHUNK + 5]
READ = [(1 << 20) + k for k in (0, 1, 15)]


def test_device_bytes_through_the_aql_code_object(launcher, dev):
    from dora_amd import device
    from dora_amd._lib import call
    from dora_amd.dataflow import Dataflow
    from dora_amd.device import DeviceBuffer
    desc = {"nodes": [
        {"id": "src", "path": "dynamic", "outputs": ["x"]},
        {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 16}}},
    ]}
    t0 = time.perf_counter()
    n_src = (1 << 20) + 64
    src_host = rp.splitmix_bytes(0xA91, n_src)
    buf = DeviceBuffer.from_bytes(src_host.tobytes(), dev)
    assert buf.ptr % 16 == 0
    got = np.empty(n_src, np.uint8)

    def receive(rx, k, r, z):
        ev = rx.next(timeout=60)
        assert ev is not None and ev["metadata"] == {"k": k}, (k, r, z)
        assert ev["data_len"] == z and ev["on_device"], (k, r, z)
        call("dora_gpu_memcpy_async", got.ctypes.data, ev["data_ptr"], z, dev.handle)
        dev.sync()
        if not np.array_equal(got[:z], src_host[r:r + z]):
            i = int(np.flatnonzero(got[:z] != src_host[r:r + z])[0])
            pytest.fail(f"message {k}: {z} bytes from source residue {r}: first differing byte {i}")
        del ev

    def pack1r():
        return device.aql_dispatch_counts(0).get("dora_aql_pack1r_u4", 0)

    with Dataflow(desc, launcher=launcher) as df:
        n = _nodes(df, {"src": 0, "dst": 0})
        tx, rx = n["src"], n["dst"]
        k = 0
        for r in range(16):
            for z in SMALL:
                for asy in (True, False):
                    tx.send_output_device_bytes("x", buf.ptr + r, z, {"k": k}, asynchronous=asy)
                    receive(rx, k, r, z)
                    k += 1
            for z in READ:   # synchronous, >= 1 MiB: read-signalled when source and slot are aligned
                r0 = pack1r()
                tx.send_output_device_bytes("x", buf.ptr + r, z, {"k": k})
                assert pack1r() - r0 == int(r == 0), (r, z)
                receive(rx, k, r, z)
                k += 1
        tx.sync()
        # a held backlog: eight messages of distinct residues and ragged lengths leave as a batch
        held = [(2 * j + 1, 3 * CHUNK + 1000 * j + 7 * j + 1) for j in range(8)]
        b0 = device.aql_batch_stats(0)
        device.aql_hold(0, True)
        try:
            for j, (r, z) in enumerate(held):
                tx.send_output_device_bytes("x", buf.ptr + r, z, {"k": k + j}, asynchronous=True)
        finally:
            device.aql_hold(0, False)
        tx.sync()
        b1 = device.aql_batch_stats(0)
        assert b1["batched_msgs"] - b0["batched_msgs"] == len(held), (b0, b1)
        for j, (r, z) in enumerate(held):
            receive(rx, k + j, r, z)
        tx.close()
        rx.close()
        df.wait(60)
    buf.free()
    print(f"AQL object: {k + len(held)} messages in {time.perf_counter() - t0:.2f} s")
