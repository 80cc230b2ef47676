"""Child process of test_gpu_tensor_dataflow.py: torch tensors in HBM sent by a node of the same
process (the relay scenario starts one more process, tensor_relay_child.py).  torch is imported before dora_amd loads its library, so that both use one HIP runtime
(torch's wheel carries its own; the node refuses device tensors while two are loaded).  Every
scenario's outcome goes into the JSON report named on the command line; the test asserts on it.

    python tests/tensor_torch_child.py REPORT.json
"""
import json
import os
import sys
import threading
import traceback

import torch  # first: see above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from dora_amd import launcher as launcher_mod  # noqa: E402

DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["x", "y", "r"]},
    {"id": "rly", "path": "dynamic", "inputs": {"r": {"source": "src/r", "queue_size": 10}},
     "outputs": ["z"]},
    {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 10},
                                                "z": {"source": "rly/z", "queue_size": 10}}},
    {"id": "hst", "path": "dynamic", "inputs": {"y": {"source": "src/y", "queue_size": 10}},
     "_unstable_deploy": {"gpu": -1}},
]}


RELAY_HW = (96, 70)


def nodes(df, spec):
    from dora_amd.node import Node
    out = {}

    def mk(i, d):
        out[i] = Node(i, dataflow=df.shm, device=d)
    ts = [threading.Thread(target=mk, args=(i, d)) for i, d in spec.items()]
    [t.start() for t in ts]
    [t.join(90) for t in ts]
    assert set(out) == set(spec), sorted(out)
    return out


def received(ev):
    """(numpy array, type info JSON) of an input event, downloaded through to_pyarrow."""
    from dora_amd import tensor
    assert ev["type"] == "INPUT", ev["type"]
    v = ev["value"].to_pyarrow() if ev["on_device"] else ev["value"]
    return tensor.to_numpy(v).copy(), ev["type_info"].to_json()


def oracle(x):
    from dora_amd import tensor
    from oracle.pack_ref import pack
    want, info = pack(tensor.from_numpy(np.ascontiguousarray(x)))
    return bytes(want), info.to_json()


def scenario_views(n):
    dev = torch.device("cuda", 0)
    f = (torch.arange(67 * 129, device=dev, dtype=torch.float32) * 0.5).reshape(67, 129)
    img = (torch.arange(37 * 53 * 3, device=dev) % 251).to(torch.uint8).reshape(37, 53, 3)
    big = (torch.arange(130 * 200, device=dev) % 253).to(torch.uint8).reshape(130, 200)
    dense = torch.arange(6 * 1024, device=dev, dtype=torch.float32).reshape(6, 1024)
    flat = torch.arange(1000, device=dev, dtype=torch.int32)
    views = {"T": f.T, "permute": img.permute(2, 0, 1), "crop": big[3:120, 5:190], "dense": dense,
             "1d": flat, "1d_step": flat[::3], "small_T": f[:5, :7].T}
    for k, (name, t) in enumerate(views.items()):
        x = t.cpu().numpy()
        assert x.shape == tuple(t.shape)
        n["src"].send_output("x", t, {"k": k})
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"k": k}, (name, ev["metadata"])
        got, info = received(ev)
        del ev
        want, winfo = oracle(x)
        assert got.dtype == x.dtype and got.shape == x.shape, (name, got.dtype, got.shape)
        assert got.tobytes() == want, name
        assert info == winfo, name
    return {"views": len(views)}


def overwrite_rounds(n, asynchronous):
    """200 messages: t.mul_(k) on torch's stream right before each send, t.fill_(-1) right after
    it returns (after sync() for asynchronous sends): the receiver sees every value k."""
    dev = torch.device("cuda", 0)
    t = torch.empty((512, 384), device=dev, dtype=torch.float32)
    view = t.T
    bad = []
    for k in range(1, 201):
        t.fill_(1.0)
        t.mul_(float(k))
        n["src"].send_output("x", view, {"k": k}, asynchronous=asynchronous)
        if asynchronous:
            n["src"].sync()
        t.fill_(-1.0)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"k": k}, ev["metadata"]
        got, _ = received(ev)
        del ev
        if got.shape != (384, 512) or not np.all(got == float(k)):
            bad.append((k, float(got.min()), float(got.max())))
    torch.cuda.synchronize()
    assert not bad, bad[:5]
    return {"messages": 200}


def scenario_host_receiver(n):
    dev = torch.device("cuda", 0)
    img = (torch.arange(37 * 53 * 3, device=dev) % 251).to(torch.uint8).reshape(37, 53, 3)
    t = img.permute(2, 0, 1)
    n["src"].send_output("y", t, {"k": 1})
    ev = n["hst"].next(timeout=60)
    assert ev["type"] == "INPUT" and ev["metadata"] == {"k": 1} and not ev["on_device"]
    import pyarrow as pa
    from dora_amd import tensor
    v = ev["value"]
    assert isinstance(v, pa.Array) and v.type == tensor.tensor_type(np.uint8, (3, 37, 53)), v.type
    x = t.cpu().numpy()
    assert np.array_equal(tensor.to_numpy(v), x)
    assert ev["type_info"].to_json() == oracle(x)[1]
    del ev, v
    return {}


def scenario_relay(n):
    """The relay is a process of its own (tests/tensor_relay_child.py): the sample it receives is
    a slot of this process that hipIpcOpenMemHandle mapped there, and it sends a transposed view
    of torch.from_dlpack of it."""
    import time
    dev = torch.device("cuda", 0)
    h, w = RELAY_HW
    rep_path, pid = n["relay_report"], n["relay_pid"]

    def relay_report():
        try:
            with open(rep_path) as f:
                return json.load(f)
        except (OSError, ValueError):
            return {}

    def log():
        try:
            return open(rep_path + ".log").read()[-2000:]
        except OSError:
            return ""
    deadline = time.monotonic() + 120
    try:
        while not relay_report().get("ready"):
            assert n["launcher"].poll(pid) is None and time.monotonic() < deadline, \
                ("the relay did not start", relay_report(), log())
            time.sleep(0.05)
        flat = torch.arange(h * w, device=dev, dtype=torch.float32)
        n["src"].send_output("r", flat, {"k": 7})
        while "sent" not in relay_report():
            assert n["launcher"].poll(pid) is None and time.monotonic() < deadline, \
                ("the relay did not answer", relay_report(), log())
            time.sleep(0.05)
        rr = relay_report()
        out = {"relay": rr}
        assert rr["ipc_opens"] >= 1, rr  # the slot was opened through IPC there
        assert rr["sent"], rr
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"k": 8}
        y, info = received(ev)
        del ev
        x = np.arange(h * w, dtype=np.float32).reshape(h, w).T
        assert np.array_equal(y, x) and info == oracle(x)[1]
        return out
    finally:
        if n["launcher"].poll(pid) is None:
            n["src"].send_output("r", b"", {"quit": 1})
            while n["launcher"].poll(pid) is None and time.monotonic() < deadline:
                time.sleep(0.05)
            if n["launcher"].poll(pid) is None:
                n["launcher"].kill(pid)


def scenario_async_bound(n):
    """Asynchronous sends hold their tensors on the node, at most _ASYNC_TENSORS_MAX of them: the
    send past that syncs first.  Temporaries are sent (the caller keeps nothing), and every one
    arrives intact."""
    dev = torch.device("cuda", 0)
    tx = n["src"]
    cap = tx._ASYNC_TENSORS_MAX
    held = []
    for k in range(cap + 6):
        tx.send_output("x", torch.full((48, 40), float(k), device=dev).T, {"k": k},
                       asynchronous=True)
        held.append(len(tx._async_tensors))
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"k": k}
        got, _ = received(ev)
        del ev
        assert got.shape == (40, 48) and np.all(got == float(k)), k
    assert held[:cap] == list(range(1, cap + 1)) and held[cap] == 1, held
    tx.sync()
    assert tx._async_tensors == []
    return {"held_max": max(held)}


def scenario_timing(n):
    """A gather send inside a timed region gives the region a device span, and with profiling on
    its kernel is stamped like a pack's (one interval of its own bytes)."""
    dev = torch.device("cuda", 0)
    tx, rx = n["src"], n["dst"]
    t = torch.arange(512 * 384, device=dev, dtype=torch.float32).reshape(512, 384)
    nbytes = t.numel() * 4
    torch.cuda.synchronize()
    tx.region_begin()
    tx.send_output("x", t.T, {"k": "region"})
    tx.region_mark()
    ev = rx.next(timeout=60)
    assert ev["metadata"] == {"k": "region"}
    del ev
    region = tx.region_end()
    assert region["packs"] == 1 and region["bytes"] == nbytes, region
    assert 0.0 < region["span_ms"] < 1000.0, region
    tx.set_profiling(True)
    tx.set_timing_period(1)
    try:
        before = tx.pack_stats()
        tx.send_output("x", t.T, {"k": "profiled"})
        ev = rx.next(timeout=60)
        assert ev["metadata"] == {"k": "profiled"}
        del ev
        tx.sync()
        after = tx.pack_stats()
    finally:
        tx.set_profiling(False)
    assert after["count"] == before["count"] + 1, (before, after)
    assert after["bytes"] == before["bytes"] + nbytes, (before, after)
    assert 0.0 < after["total_ms"] - before["total_ms"] < 1000.0, (before, after)
    return {"region": region}


def scenario_refusals(n):
    from ctypes import byref

    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM, DoraGpuError
    from dora_amd.node import encode_parameters
    dev = torch.device("cuda", 0)
    t = torch.arange(64 * 64, device=dev, dtype=torch.float32).reshape(64, 64)

    class Elsewhere:  # a producer that reports another GPU; never asked for its capsule
        def __dlpack_device__(self):
            return (10, 1)

        def __dlpack__(self, **kw):
            raise AssertionError("the capsule of a tensor on another GPU was requested")
    try:
        n["src"].send_output("x", Elsewhere())
        raise AssertionError("a tensor on another GPU was sent")
    except TypeError as e:
        assert "GPU 1" in str(e) and "GPU 0" in str(e), str(e)
    # a view reaching far beyond the allocation its pointer lies in (64 rows 2^30 elements apart)
    d, keep = tensor._describe(t.data_ptr(), (64, 16), (2 ** 30, 1), np.float32)
    params = encode_parameters({"k": 0})
    rc = _lib.load().dora_node_send_output_tensor(n["src"].handle, b"x", byref(d), ARROW_DEVICE_ROCM,
                                                   params, len(params), 0)
    try:
        _lib.check(rc)
        raise AssertionError("a view beyond its allocation was sent")
    except DoraGpuError as e:
        assert e.code == -1 and "allocation" in str(e), str(e)
    del keep
    n["src"].send_output("x", t.T, {"k": 99})
    ev = n["dst"].next(timeout=60)
    assert ev["type"] == "INPUT" and ev["metadata"] == {"k": 99}, ev.get("metadata")
    y, _ = received(ev)
    del ev
    assert np.array_equal(y, t.cpu().numpy().T)
    return {}


def main(report_path):
    report = {}
    lch = launcher_mod.Launcher()  # before HIP is initialised in this process
    try:
        from dora_amd.dataflow import Dataflow
        torch.cuda.set_device(0)
        with Dataflow(DESC, launcher=lch) as df:
            # the relay joins from a process of its own (every node attaches before any starts)
            relay_report = report_path + ".relay"
            relay_pid = lch.spawn([sys.executable, os.path.join(ROOT, "tests", "tensor_relay_child.py"),
                                   df.shm, relay_report, str(RELAY_HW[0]), str(RELAY_HW[1])],
                                  out=relay_report + ".log")
            try:
                n = nodes(df, {"src": 0, "dst": 0, "hst": -1})
            except BaseException:
                lch.kill(relay_pid)
                raise
            live = list(n.values())
            n.update(launcher=lch, relay_report=relay_report, relay_pid=relay_pid)
            try:
                for name, fn in [("views", scenario_views),
                                 ("sync_overwrite", lambda n: overwrite_rounds(n, False)),
                                 ("async_overwrite", lambda n: overwrite_rounds(n, True)),
                                 ("host_receiver", scenario_host_receiver),
                                 ("async_bound", scenario_async_bound),
                                 ("timing", scenario_timing),
                                 ("refusals", scenario_refusals),
                                 ("relay", scenario_relay)]:  # last: the relay's exit closes z
                    try:
                        report[name] = {"ok": True, **(fn(n) or {})}
                    except Exception:
                        report[name] = {"ok": False, "error": traceback.format_exc()[-3000:]}
                    with open(report_path, "w") as f:
                        json.dump(report, f)
                    if not report[name]["ok"]:
                        break  # nothing more on the GPU after a failure
            finally:
                if lch.poll(relay_pid) is None:
                    try:
                        n["src"].send_output("r", b"", {"quit": 1})
                    except Exception:
                        pass
                for k in live:
                    k.close()
                import time
                t_end = time.monotonic() + 20
                while lch.poll(relay_pid) is None and time.monotonic() < t_end:
                    time.sleep(0.05)
                if lch.poll(relay_pid) is None:
                    lch.kill(relay_pid)
    except Exception:
        report["setup"] = {"ok": False, "error": traceback.format_exc()[-3000:]}
    finally:
        lch.close()
    with open(report_path, "w") as f:
        json.dump(report, f)
    return 0 if all(v.get("ok") for v in report.values()) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
