"""Child process of test_gpu_tensor_list_dataflow.py: ragged batches of torch tensors in HBM sent
as one List message by a node of the same process.  torch is imported before dora_amd loads its
library, so that both use one HIP runtime.  Every scenario's outcome goes into the JSON report
named on the command line; the test asserts on it.

    python tests/tensor_list_child.py REPORT.json
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
    {"id": "src", "path": "dynamic", "outputs": ["x", "y"]},
    {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 10}}},
    {"id": "hst", "path": "dynamic", "inputs": {"y": {"source": "src/y", "queue_size": 10}},
     "_unstable_deploy": {"gpu": -1}},
]}
N = 67


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


def values(k):
    """The (N, 6) points of message k, exact in float32."""
    return (np.arange(N * 6, dtype=np.float32).reshape(N, 6) * 0.25 + float(k)).astype(np.float32)


def lengths(k):
    """Five lengths that sum to N, different for every message, with empty lists."""
    a = (7 * k) % 30
    return [a, 0, 30 - a, N - 30, 0]


def cloud(p, inten):
    return {"x": p[:, 0], "y": p[:, 1], "z": p[:, 2], "intensity": inten}


def oracle(vals, ln):
    from dora_amd import tensor
    from oracle.pack_ref import pack
    arr = tensor.from_numpy_ragged(vals, lengths=ln)
    return arr, pack(arr)[1].to_json()


def inside(t, ev):
    return ev["data_ptr"] <= t.data_ptr() and \
        t.data_ptr() + t.numel() * t.element_size() <= ev["data_ptr"] + ev["data_len"]


def check_device_ragged(ev, want, ln, what):
    """to_torch of a device receiver's value: Ragged of kDLROCM tensors over the one sample."""
    from dora_amd import tensor
    assert ev["type"] == "INPUT" and ev["on_device"], (what, ev["type"])
    r = tensor.to_torch(ev["value"])
    assert isinstance(r, tensor.Ragged) and len(r) == len(ln), what
    off = r.offsets
    assert off.is_cuda and off.dtype == torch.int32 and inside(off, ev), what
    assert off.cpu().tolist() == np.concatenate([[0], np.cumsum(ln)]).tolist(), (what, off.cpu().tolist())
    assert r.lengths().cpu().tolist() == list(ln), what
    got = r.values if isinstance(want, dict) else {"": r.values}
    for name, w in (want if isinstance(want, dict) else {"": want}).items():
        g = got[name]
        assert g.is_cuda and g.device.index == 0 and inside(g, ev), (what, name)  # zero-copy
        assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), (what, name)
    assert ev["type_info"].to_json() == oracle(want, ln)[1], what
    rows = r.unbind()
    assert len(rows) == len(ln)
    first = rows[0] if not isinstance(want, dict) else rows[0]["x"]
    assert first.shape[0] == ln[0], what
    return r


def scenario_sync_rewrite(n):
    """50 messages from one (67, 6) tensor rewritten on torch's stream right before each
    synchronous send and poisoned right after it returns, the partition rewritten with it:
    in turn a record cut by int64 lengths in HBM, a bare tensor cut by int32 offsets in HBM (as
    torch's jagged layout holds them), and a record cut by a host list."""
    dev = torch.device("cuda", 0)
    pts = torch.empty((N, 6), device=dev, dtype=torch.float32)
    inten = torch.arange(N, device=dev, dtype=torch.uint8)
    inten_np = np.arange(N, dtype=np.uint8)
    counts = torch.zeros(5, device=dev, dtype=torch.int64)
    offs = torch.zeros(6, device=dev, dtype=torch.int32)
    for k in range(50):
        ln = lengths(k)
        pts.copy_(torch.from_numpy(values(k)))
        from dora_amd import tensor
        if k % 3 == 0:
            counts.copy_(torch.tensor(ln, dtype=torch.int64))
            msg, want = tensor.ragged(cloud(pts, inten), lengths=counts), cloud(values(k), inten_np)
        elif k % 3 == 1:
            offs.copy_(torch.tensor(np.concatenate([[0], np.cumsum(ln)]), dtype=torch.int32))
            msg, want = tensor.ragged(pts[:, :4], offsets=offs), values(k)[:, :4]
        else:
            msg, want = tensor.ragged(cloud(pts, inten), lengths=ln), cloud(values(k), inten_np)
        n["src"].send_output("x", msg, {"k": k})
        pts.fill_(-1.0)
        counts.fill_(-5)
        offs.fill_(99)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"k": k}, ev["metadata"]
        r = check_device_ragged(ev, want, ln, f"message {k}")
        del ev, r
    torch.cuda.synchronize()
    return {"messages": 50}


def scenario_host_receiver(n):
    """A receiver without a GPU gets the staged pyarrow ListArray of from_numpy_ragged."""
    import pyarrow as pa
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    pts = torch.from_numpy(values(7)).to(dev)
    inten = torch.arange(N, device=dev, dtype=torch.uint8)
    sent = 0
    for ln, part in ((lengths(3), torch.tensor(lengths(3), device=dev, dtype=torch.int32)),
                     (lengths(4), lengths(4))):
        n["src"].send_output("y", tensor.ragged(cloud(pts, inten), lengths=part), {"k": sent})
        ev = n["hst"].next(timeout=60)
        assert ev["type"] == "INPUT" and ev["metadata"] == {"k": sent} and not ev["on_device"]
        want, info = oracle(cloud(values(7), np.arange(N, dtype=np.uint8)), ln)
        v = ev["value"]
        assert isinstance(v, pa.ListArray) and v.type == want.type and v.equals(want), str(v.type)
        v.validate(full=True)
        assert ev["type_info"].to_json() == info
        r = tensor.to_numpy(v)
        assert r.lengths().tolist() == ln
        del ev, v
        sent += 1
    return {"messages": sent}


def scenario_async(n):
    """One asynchronous send: the node holds every field and the device partition until sync()."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    tx = n["src"]
    pts = torch.from_numpy(values(11)).to(dev)
    inten = torch.arange(N, device=dev, dtype=torch.uint8)
    ln = lengths(11)
    counts = torch.tensor(ln, device=dev, dtype=torch.int64)
    tx.sync()
    tx.send_output("x", tensor.ragged(cloud(pts, inten), lengths=counts), {"k": "async"},
                   asynchronous=True)
    held = len(tx._async_tensors)
    tx.sync()
    assert held == 5 and tx._async_tensors == [], held
    pts.fill_(-1.0)
    counts.fill_(-1)
    ev = n["dst"].next(timeout=60)
    assert ev["metadata"] == {"k": "async"}
    r = check_device_ragged(ev, cloud(values(11), np.arange(N, dtype=np.uint8)), ln, "async")
    del ev, r
    torch.cuda.synchronize()
    return {"held": held}


def scenario_clamped(n):
    """Device words that do not describe the rows arrive as the clamped formula's offsets."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    pts = torch.from_numpy(values(2)).to(dev)
    words = [40, -7, 60, 3]
    n["src"].send_output("x", tensor.ragged(pts[:, :4], lengths=torch.tensor(words, device=dev)),
                         {"k": "clamped"})
    ev = n["dst"].next(timeout=60)
    r = tensor.to_torch(ev["value"])
    assert r.offsets.cpu().tolist() == [0, 40, 40, N, N], r.offsets.cpu().tolist()
    host = ev["value"].to_pyarrow()
    host.validate(full=True)
    del ev, r
    return {}


def scenario_refusals(n):
    from dora_amd import tensor
    from dora_amd._lib import DoraGpuError
    dev = torch.device("cuda", 0)
    pts = torch.from_numpy(values(0)).to(dev)
    counts = torch.tensor([N], device=dev)
    try:
        n["src"].send_output("x", tensor.ragged(values(0), lengths=counts))
        raise AssertionError("a device partition with host values was sent")
    except TypeError as e:
        assert ".tolist()" in str(e), str(e)
    try:
        n["src"].send_output("x", tensor.ragged(pts, lengths=[N - 1]))
        raise AssertionError("a host partition short of N was sent")
    except DoraGpuError as e:
        assert e.code == -1 and "sum to 66" in str(e), str(e)
    try:
        n["src"].send_output("x", tensor.ragged({"a": pts[:, 0], "b": values(0)[:, 1]}, lengths=[N]))
        raise AssertionError("a record mixing a device tensor and a numpy array was sent")
    except TypeError as e:
        assert "`a`" in str(e) and "`b`" in str(e), str(e)
    # nothing was sent: the next valid batch is the next message; N == 0 with B > 0 and B == 0
    n["src"].send_output("x", tensor.ragged(pts, lengths=[N]), {"k": "next"})
    ev = n["dst"].next(timeout=60)
    assert ev["metadata"] == {"k": "next"}, ev.get("metadata")
    check_device_ragged(ev, values(0), [N], "after refusals")
    del ev
    for ln in ([0, 0, 0], []):
        n["src"].send_output("x", tensor.ragged(pts[:0], lengths=ln), {"k": len(ln)})
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"k": len(ln)}
        r = tensor.to_numpy(ev["value"] if not ev.get("on_device") else ev["value"].to_pyarrow())
        assert r.offsets.tolist() == [0] * (len(ln) + 1) and r.values.shape == (0, 6)
        del ev
    return {}


def main(report_path):
    report = {}
    lch = launcher_mod.Launcher()  # before HIP is initialised in this process
    try:
        from dora_amd.dataflow import Dataflow
        torch.cuda.set_device(0)
        with Dataflow(DESC, launcher=lch) as df:
            n = nodes(df, {"src": 0, "dst": 0, "hst": -1})
            try:
                for name, fn in [("sync_rewrite", scenario_sync_rewrite),
                                 ("host_receiver", scenario_host_receiver),
                                 ("async", scenario_async),
                                 ("clamped", scenario_clamped),
                                 ("refusals", scenario_refusals)]:
                    try:
                        report[name] = {"ok": True, **(fn(n) or {})}
                    except Exception:
                        report[name] = {"ok": False, "error": traceback.format_exc()[-3000:]}
                    with open(report_path, "w") as f:
                        json.dump(report, f)
                    if not report[name]["ok"]:
                        break  # nothing more on the GPU after a failure
            finally:
                for k in n.values():
                    k.close()
    except Exception:
        report["setup"] = {"ok": False, "error": traceback.format_exc()[-3000:]}
    finally:
        lch.close()
    with open(report_path, "w") as f:
        json.dump(report, f)
    return 0 if all(v.get("ok") for v in report.values()) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
