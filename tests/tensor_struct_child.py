"""Child process of test_gpu_tensor_struct_dataflow.py: dicts of torch tensors in HBM sent as one
Struct message by a node of the same process.  torch is imported before dora_amd loads its
library, so that both use one HIP runtime (torch's wheel carries its own; the node refuses device
tensors while two are loaded).  Every scenario's outcome goes into the JSON report named on the
command line; the test asserts on it.

    python tests/tensor_struct_child.py REPORT.json
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
    """The (N, 6) detector output of message k, exact in float32."""
    return (np.arange(N * 6, dtype=np.float32).reshape(N, 6) * 0.25 + float(k)).astype(np.float32)


def record(out, ids):
    """The detector record over a (N, 6) base: three strided views of it and a dense column."""
    return {"bbox": out[:, :4], "conf": out[:, 4], "cls": out[:, 5], "ids": ids}


def oracle(rec):
    from dora_amd import tensor
    from oracle.pack_ref import pack
    arr = tensor.from_numpy_struct(rec)
    return arr, pack(arr)[1].to_json()


def check_device_dict(ev, want, what):
    from dora_amd import tensor
    assert ev["type"] == "INPUT" and ev["on_device"], (what, ev["type"])
    got = tensor.to_torch(ev["value"])
    assert list(got) == list(want), (what, list(got))
    for name, w in want.items():
        g = got[name]
        assert g.is_cuda and g.device.index == 0, (what, name, str(g.device))
        assert tuple(g.shape) == w.shape and g.dtype == torch.from_numpy(w[:0].copy()).dtype, \
            (what, name, tuple(g.shape), str(g.dtype))
        assert np.array_equal(g.cpu().numpy(), w), (what, name)
    assert ev["type_info"].to_json() == oracle(want)[1], what
    return got


def scenario_sync_rewrite(n):
    """20 messages from the views of one (67, 6) tensor, the base rewritten on torch's stream
    right before each synchronous send and poisoned right after it returns."""
    dev = torch.device("cuda", 0)
    out = torch.empty((N, 6), device=dev, dtype=torch.float32)
    ids = torch.arange(N, device=dev, dtype=torch.int64)
    ids_np = np.arange(N, dtype=np.int64)
    for k in range(20):
        out.copy_(torch.from_numpy(values(k)))
        n["src"].send_output("x", record(out, ids), {"k": k})
        out.fill_(-1.0)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"k": k}, ev["metadata"]
        got = check_device_dict(ev, record(values(k), ids_np), f"message {k}")
        del ev, got
    torch.cuda.synchronize()
    return {"messages": 20}


def scenario_fields(n):
    """DeviceArray.field by name and by index: child views over the one sample."""
    dev = torch.device("cuda", 0)
    out = torch.from_numpy(values(3)).to(dev)
    ids = torch.arange(N, device=dev, dtype=torch.int64)
    n["src"].send_output("x", record(out, ids), {"k": "fields"})
    ev = n["dst"].next(timeout=60)
    v = ev["value"]
    conf, bbox = v.field("conf"), v.field(0)
    assert conf.length == N and bbox.length == N
    a, b = torch.from_dlpack(conf), torch.from_dlpack(bbox)
    assert np.array_equal(a.cpu().numpy(), values(3)[:, 4])
    assert np.array_equal(b.cpu().numpy(), values(3)[:, :4])
    try:
        v.field("nope")
        raise AssertionError("an unknown field was returned")
    except KeyError:
        pass
    del ev, v, a, b, conf, bbox
    return {}


def scenario_host_receiver(n):
    import pyarrow as pa
    dev = torch.device("cuda", 0)
    out = torch.from_numpy(values(7)).to(dev)
    ids = torch.arange(N, device=dev, dtype=torch.int64)
    n["src"].send_output("y", record(out, ids), {"k": 1})
    ev = n["hst"].next(timeout=60)
    assert ev["type"] == "INPUT" and ev["metadata"] == {"k": 1} and not ev["on_device"]
    want, info = oracle(record(values(7), np.arange(N, dtype=np.int64)))
    v = ev["value"]
    assert isinstance(v, pa.StructArray) and v.type == want.type and v.equals(want), str(v.type)
    assert ev["type_info"].to_json() == info
    del ev, v
    return {}


def scenario_async(n):
    """One asynchronous send: the node holds every field until sync()."""
    dev = torch.device("cuda", 0)
    tx = n["src"]
    out = torch.from_numpy(values(11)).to(dev)
    ids = torch.arange(N, device=dev, dtype=torch.int64)
    tx.sync()
    tx.send_output("x", record(out, ids), {"k": "async"}, asynchronous=True)
    held = len(tx._async_tensors)
    tx.sync()
    assert held == 4 and tx._async_tensors == [], held
    out.fill_(-1.0)
    ev = n["dst"].next(timeout=60)
    assert ev["metadata"] == {"k": "async"}
    got = check_device_dict(ev, record(values(11), np.arange(N, dtype=np.int64)), "async")
    del ev, got
    torch.cuda.synchronize()
    return {"held": held}


def scenario_refusals(n):
    dev = torch.device("cuda", 0)
    out = torch.from_numpy(values(0)).to(dev)
    try:
        n["src"].send_output("x", {"host": values(0)[:, 0], "hbm": out[:, 1]})
        raise AssertionError("a dict mixing a numpy array and a device tensor was sent")
    except TypeError as e:
        assert "`host`" in str(e) and "`hbm`" in str(e), str(e)
    from dora_amd._lib import DoraGpuError
    try:
        n["src"].send_output("x", {"a": out[:, :4], "b": out[:5, 4]})
        raise AssertionError("fields of different leading extents were sent")
    except DoraGpuError as e:
        assert e.code == -1 and "field 1 `b`" in str(e), str(e)
    # nothing was sent: the next valid record is the next message
    n["src"].send_output("x", {"only": out.T[:, None]}, {"k": "next"})
    ev = n["dst"].next(timeout=60)
    assert ev["metadata"] == {"k": "next"}, ev.get("metadata")
    check_device_dict(ev, {"only": values(0).T[:, None]}, "after refusals")
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
                                 ("fields", scenario_fields),
                                 ("host_receiver", scenario_host_receiver),
                                 ("async", scenario_async),
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
