"""Samples published by the producer's own kernel (dora_sample_fill_ticket +
include/dora_gpu_device.h): allocate_data_sample -> ticket -> ONE kernel that writes the sample
in place and raises the slot's fill flag itself -> send_output_sample, with no stream operation
of the send and no pack.

The shapes are the smallest at which the signal can still go wrong: the one-workgroup short
path, two workgroups, 257 (more done words than one poll round of a 64-lane workgroup covers
with one load per lane), the 4096 done-word limit, and payloads that end inside a 16-byte unit
(12,289 B and 4 MiB + 5 B).  Every send has its own seed, so a slot that kept an earlier
message's bytes cannot pass.
"""
import ctypes
import json
import threading
import time
from ctypes import byref, c_uint64, c_void_p

import pytest

pytestmark = pytest.mark.gpu

WT, PLAIN = 0, 1  # DORA_FILL_WRITE_THROUGH, DORA_FILL_PLAIN
LENGTHS = [4096, 12289, (4 << 20) + 5]
WORKGROUPS = [1, 2, 257, 4096]
SEED0 = 0x71C4E700000


def _nodes(df, spec):
    from dora_amd.node import Node
    out = {}

    def mk(i, dev):
        out[i] = Node(i, dataflow=df.shm, device=dev)
    ts = [threading.Thread(target=mk, args=(i, d)) for i, d in spec.items()]
    [t.start() for t in ts]
    [t.join(90) for t in ts]
    assert set(out) == set(spec)
    return out


def _device_bytes(ptr, n, stream):
    from dora_amd._lib import call
    out = ctypes.create_string_buffer(max(n, 1))
    call("dora_gpu_memcpy_async", out, ptr, n, stream.handle)
    stream.sync()
    return out.raw[:n]


class _Sender:
    """allocate -> ticket -> kernel on a caller stream (never the node stream) -> send."""

    def __init__(self, lib, tx, stream):
        self.lib, self.tx, self.stream, self.tis = lib, tx, stream, {}

    def type_info(self, ptr, z):
        from dora_amd.arrow_utils import Plan
        if z not in self.tis:  # ArrowTypeInfo::byte_array(z)
            with Plan.of_bytes(ptr, z, True) as p:
                self.tis[z] = p.type_info_bytes()
        return self.tis[z]

    def allocate(self, z):
        from dora_amd._lib import call
        smp = c_void_p()
        call("dora_node_allocate_data_sample", self.tx.handle, z, byref(smp))
        return smp, self.lib.dora_sample_data(smp)

    def launch(self, ptr, z, seed, ticket, threads):
        """threads None: the product's ticket kernel (256 threads, write-through); else the test
        hook with that workgroup size, storing as the ticket's mode says."""
        from dora_amd._lib import call
        if threads is None:
            call("dora_gpu_fill_splitmix_ticket", ptr, z, seed, byref(ticket), self.stream.handle)
        else:
            call("dora_gpu_test_publish_kernel", ptr, z, seed, byref(ticket), threads,
                 1 if ticket.mode == PLAIN else 0, self.stream.handle)

    def send(self, out, smp, ptr, z, params=b""):
        from dora_amd._lib import call
        ti = self.type_info(ptr, z)
        call("dora_node_send_output_sample", self.tx.handle, out.encode(), ti, len(ti),
             params, len(params), smp)

    def ticketed(self, out, z, seed, wgs, mode, threads=None, params=b""):
        smp, ptr = self.allocate(z)
        t = self.tx.sample_fill_ticket(smp, wgs, mode)
        self.launch(ptr, z, seed, t, threads)
        self.send(out, smp, ptr, z, params)
        return smp, t


def _paths(tx):
    from dora_amd._lib import call
    a, b = c_uint64(), c_uint64()
    call("dora_node_sample_paths", tx.handle, byref(a), byref(b))
    return {"stream_ordered": a.value, "self_published": b.value}


@pytest.fixture(scope="module")
def flow(launcher, lib):
    """One dataflow, sender and receiver on GPU 0 in this process, for the tests that only send
    and receive."""
    from dora_amd import device
    from dora_amd.dataflow import Dataflow
    desc = {"nodes": [
        {"id": "src", "path": "dynamic", "outputs": ["x"]},
        {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 10}}},
    ]}
    s = device.Stream()
    with Dataflow(desc, launcher=launcher) as df:
        n = _nodes(df, {"src": 0, "dst": 0})
        yield _Sender(lib, n["src"], s), n["dst"], s
        n["src"].close()
        n["dst"].close()
        df.wait(30)
    s.close()


def test_bit_exact_every_shape_mode_and_workgroup_size(flow, lib):
    """Lengths 4096 / 12,289 / 4 MiB + 5 x workgroups 1 / 2 / 257 / 4096 x both modes x workgroup
    sizes 64 / 256 / 1024 (test hook), and the product's ticket kernel at every length and
    workgroup count: the receiver's bytes equal the oracle's, byte for byte.  Every one of those
    sends is counted as self-published, none as stream-ordered.  4097 workgroups, a second
    ticket and a second send are refused."""
    from dora_amd import device
    from dora_amd._lib import DoraGpuError, call
    from oracle.checksum_ref import csum64, splitmix_bytes
    tx, rx, s = flow
    before = _paths(tx.tx)
    cases = [(z, w, m, th) for z in LENGTHS for w in WORKGROUPS for m in (WT, PLAIN)
             for th in (64, 256, 1024)]
    cases += [(z, w, WT, None) for z in LENGTHS for w in WORKGROUPS]
    for k, (z, wgs, mode, threads) in enumerate(cases):
        seed = SEED0 + k
        smp, t = tx.ticketed("x", z, seed, wgs, mode, threads)
        assert (t.workgroups, t.mode) == (wgs, mode) and t.flag and t.done and t.epoch
        ev = rx.next(timeout=60)
        case = (z, wgs, mode, threads)
        assert ev["type"] == "INPUT", (case, ev.get("error"))
        assert ev["on_device"] and ev["data_len"] == z, case
        want = splitmix_bytes(z, seed)
        if z > (1 << 20):
            assert device.csum64(ev["data_ptr"], z, s) == csum64(want), case
        got = _device_bytes(ev["data_ptr"], z, s)
        if got != want:
            bad = next(i for i in range(z) if got[i] != want[i])
            raise AssertionError(f"{case}: first wrong byte at {bad} of {z}")
        del ev
    after = _paths(tx.tx)
    assert after["self_published"] - before["self_published"] == len(cases)
    assert after["stream_ordered"] == before["stream_ordered"]
    # refusals: too many workgroups, a second ticket, a second send
    smp, ptr = tx.allocate(4096)
    with pytest.raises(DoraGpuError, match="workgroups"):
        tx.tx.sample_fill_ticket(smp, 4097, WT)
    with pytest.raises(DoraGpuError, match="workgroups"):
        tx.tx.sample_fill_ticket(smp, 0, WT)
    with pytest.raises(DoraGpuError, match="mode"):
        tx.tx.sample_fill_ticket(smp, 1, 2)
    t = tx.tx.sample_fill_ticket(smp, 1, WT)
    with pytest.raises(DoraGpuError, match="already has a ticket"):
        tx.tx.sample_fill_ticket(smp, 1, WT)
    seed = SEED0 + 0x1000
    tx.launch(ptr, 4096, seed, t, None)
    tx.send("x", smp, ptr, 4096)
    with pytest.raises(DoraGpuError, match="already sent or discarded"):
        tx.send("x", smp, ptr, 4096)
    with pytest.raises(DoraGpuError, match="not live"):
        tx.tx.sample_fill_ticket(smp, 1, WT)
    ev = rx.next(timeout=60)
    assert _device_bytes(ev["data_ptr"], 4096, s) == splitmix_bytes(4096, seed)
    del ev
    # the hook refuses the invalid form (ordinary stores, nothing to write them back)
    smp, ptr = tx.allocate(4096)
    t = tx.tx.sample_fill_ticket(smp, 1, WT)
    with pytest.raises(DoraGpuError, match="DORA_FILL_PLAIN"):
        call("dora_gpu_test_publish_kernel", ptr, 4096, 1, byref(t), 64, 1, s.handle)
    lib.dora_sample_discard(tx.tx.handle, smp)


def test_kernel_queued_after_the_send(flow):
    """The kernel may be queued after send_output_sample: the receiver waits on the flag."""
    from oracle.checksum_ref import splitmix_bytes
    tx, rx, s = flow
    z, seed = 12289, SEED0 + 0x2000
    smp, ptr = tx.allocate(z)
    t = tx.tx.sample_fill_ticket(smp, 2, WT)
    tx.send("x", smp, ptr, z)
    tx.launch(ptr, z, seed, t, None)
    ev = rx.next(timeout=60)
    assert ev["type"] == "INPUT", ev.get("error")
    assert _device_bytes(ev["data_ptr"], z, s) == splitmix_bytes(z, seed)
    del ev


def test_stream_ordered_path_is_unchanged(flow):
    """A sample written on the node stream and sent without a ticket is still ordered by the
    send's stream operation, counted as such, and arrives equal."""
    from dora_amd._lib import call
    from oracle.checksum_ref import splitmix_bytes
    tx, rx, s = flow
    before = _paths(tx.tx)
    nst = tx.tx.stream  # dora_node_stream
    for k, z in enumerate(LENGTHS):
        seed = SEED0 + 0x3000 + k
        smp, ptr = tx.allocate(z)
        call("dora_gpu_fill_splitmix", ptr, z, seed, nst)
        tx.send("x", smp, ptr, z)
        ev = rx.next(timeout=60)
        assert ev["type"] == "INPUT", ev.get("error")
        assert _device_bytes(ev["data_ptr"], z, s) == splitmix_bytes(z, seed), z
        del ev
    # and a ticketed sample after the node stream was handed out still queues nothing on it
    seed = SEED0 + 0x3100
    tx.ticketed("x", 4096, seed, 1, PLAIN, 64)
    ev = rx.next(timeout=60)
    assert _device_bytes(ev["data_ptr"], 4096, s) == splitmix_bytes(4096, seed)
    del ev
    after = _paths(tx.tx)
    assert after["stream_ordered"] - before["stream_ordered"] == len(LENGTHS)
    assert after["self_published"] - before["self_published"] == 1


def test_flag_line_stamps(flow):
    """Workgroup 0 stamps the flag line before it raises the flag: after a ticketed fill the
    line reads (the ticket's epoch, start, signal) with 0 < start <= signal (DORA_GPU_TRACE's
    GPU side relies on them)."""
    tx, rx, s = flow
    for wgs, mode, threads in ((1, WT, None), (257, WT, None), (2, PLAIN, 64)):
        smp, t = tx.ticketed("x", 1 << 20, SEED0 + 0x4000 + wgs, wgs, mode, threads)
        ev = rx.next(timeout=60)  # the fill is complete
        assert ev["type"] == "INPUT", ev.get("error")
        line = (c_uint64 * 3).from_buffer_copy(_device_bytes(t.flag, 24, s))
        assert line[0] == t.epoch, (wgs, list(line), t.epoch)
        assert 0 < line[1] <= line[2], (wgs, list(line))
        # s_memrealtime ticks at 100 MHz: a 1 MiB fill takes far less than a second
        assert line[2] - line[1] < 100_000_000, (wgs, list(line))
        del ev


def test_rewritten_slots_second_process_zero_stale(launcher, tmp_path):
    """600 messages of 64 KiB alternating between two outputs, each with its own seed, the modes
    alternating, the kernels on a caller stream that is not the node stream; the receiver is a
    second process (the bench sink, which checksums every sample on its GPU against the oracle
    checksum the message carries).  Slots recycle: none is created after the first round."""
    from dora_amd import device
    from dora_amd._lib import load
    from dora_amd.dataflow import Dataflow
    from dora_amd.node import Node, encode_parameters
    from dora_amd.verify import to_i64
    from oracle.checksum_ref import csum64, splitmix_bytes
    res = str(tmp_path / "sink.json")
    desc = {"nodes": [
        {"id": "node", "path": "dynamic", "outputs": ["a", "b"], "inputs": {"ack": "sink/ack"}},
        {"id": "sink", "path": "dora-gpu-bench-sink", "outputs": ["ack"],
         "inputs": {"a": {"source": "node/a", "queue_size": 1000},
                    "b": {"source": "node/b", "queue_size": 1000}},
         "env": {"DORA_BENCH_RESULT": res}},
    ]}
    z, n_msgs, rounds = 64 << 10, 600, 3
    sums = [to_i64(csum64(splitmix_bytes(z, SEED0 + 0x5000 + k))) for k in range(n_msgs)]
    assert len(set(sums)) == n_msgs
    s = device.Stream()
    created = []
    with Dataflow(desc, launcher=launcher) as df:
        node = Node("node", dataflow=df.shm, device=0)
        tx = _Sender(load(), node, s)
        for k in range(n_msgs):
            params = encode_parameters({"seq": k, "csum": sums[k], "verify": True})
            mode = (WT, PLAIN)[k % 2]
            tx.ticketed("ab"[k % 2], z, SEED0 + 0x5000 + k, 8, mode,
                        None if mode == WT else (64, 256, 1024)[(k // 2) % 3], params)
            if (k + 1) % (n_msgs // rounds) == 0:
                node.send_output("a", b"", {"seq": n_msgs + k, "ack": True})
                node.wait_input("ack", "seq", n_msgs + k, 60.0)
                created.append(node.stats()["slots_created"])
        paths = _paths(node)
        node.close()
        codes = df.wait(60)
        log = df.log("sink")
    s.close()
    assert codes["sink"] == 0, log
    out = json.load(open(res))
    assert out["errors"] == 0, out
    series = [x for x in out["series"] if x["size"] == z]
    assert sum(x["verified"] for x in series) == n_msgs, out
    assert sum(x["mismatches"] for x in out["series"]) == 0, out
    assert paths == {"stream_ordered": 0, "self_published": n_msgs}
    assert created[0] == created[1] == created[2], created


def test_receiver_without_a_gpu(launcher, lib):
    """A receiver with DORA_GPU_DEVICE=-1 stages a ticketed 4096 B and a ticketed 1 MiB sample to
    host memory behind the same flag: host data equal to the oracle's bytes."""
    from dora_amd import device
    from dora_amd.dataflow import Dataflow
    from oracle.checksum_ref import splitmix_bytes
    desc = {"nodes": [
        {"id": "src", "path": "dynamic", "outputs": ["x"]},
        {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 10}},
         "_unstable_deploy": {"gpu": -1}},
    ]}
    s = device.Stream()
    with Dataflow(desc, launcher=launcher) as df:
        n = _nodes(df, {"src": 0, "dst": -1})
        tx, rx = _Sender(lib, n["src"], s), n["dst"]
        k = 0
        for z in (4096, 1 << 20):
            for wgs, mode, threads in ((1, WT, None), (2, PLAIN, 1024), (257, WT, 64)):
                seed = SEED0 + 0x6000 + k
                k += 1
                tx.ticketed("x", z, seed, wgs, mode, threads)
                ev = rx.next(timeout=60)
                assert ev["type"] == "INPUT", ev.get("error")
                assert not ev["on_device"] and ev["data_len"] == z
                assert ctypes.string_at(ev["data_ptr"], z) == splitmix_bytes(z, seed), (z, wgs)
                del ev
        assert rx.host_paths()["staged"] == k
        n["src"].close()
        n["dst"].close()
        df.wait(30)
    s.close()


def test_abandoned_ticket_leaves_no_slot_waiting(launcher, lib):
    """allocate, take a ticket, launch nothing, discard: the discard returns at once (it raises
    the flag to the ticket's epoch itself), the next allocation of that size reuses the slot
    without waiting and its ticketed send arrives equal, and closing the node with another
    abandoned ticket still live returns normally."""
    from dora_amd import device
    from dora_amd.dataflow import Dataflow
    from oracle.checksum_ref import splitmix_bytes
    desc = {"nodes": [
        {"id": "src", "path": "dynamic", "outputs": ["x"]},
        {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 10}}},
    ]}
    z = 1 << 20
    s = device.Stream()
    with Dataflow(desc, launcher=launcher) as df:
        n = _nodes(df, {"src": 0, "dst": 0})
        tx, rx = _Sender(lib, n["src"], s), n["dst"]
        smp, ptr = tx.allocate(z)
        t = tx.tx.sample_fill_ticket(smp, 257, WT)
        t0 = time.perf_counter()
        lib.dora_sample_discard(tx.tx.handle, smp)
        # the host's own store is visible through the flag's device address
        assert c_uint64.from_buffer_copy(_device_bytes(t.flag, 8, s)).value == t.epoch
        st0 = tx.tx.stats()
        seed = SEED0 + 0x7000
        smp2, t2 = tx.ticketed("x", z, seed, 257, WT)
        took = time.perf_counter() - t0
        st1 = tx.tx.stats()
        assert st1["slots_created"] == st0["slots_created"] == 1, (st0, st1)
        assert st1["cache_hits"] == st0["cache_hits"] + 1, (st0, st1)
        assert t2.flag == t.flag and t2.epoch > t.epoch
        ev = rx.next(timeout=60)
        assert ev["type"] == "INPUT", ev.get("error")
        assert _device_bytes(ev["data_ptr"], z, s) == splitmix_bytes(z, seed)
        del ev
        # slot reuse waits up to 10 s for a fill nobody completes: far from it
        assert took < 2.0, took
        t0 = time.perf_counter()
        tx.tx.sync()  # the abandoned ticket left nothing for dora_node_sync to wait on
        assert time.perf_counter() - t0 < 2.0
        # a ticket still live at close, its kernel never launched
        smp3, _ = tx.allocate(z)
        tx.tx.sample_fill_ticket(smp3, 2, PLAIN)
        t0 = time.perf_counter()
        n["src"].close()
        assert time.perf_counter() - t0 < 5.0
        n["dst"].close()
        df.wait(30)
    s.close()
