"""Child process of test_gpu_tensor_take_dataflow.py: rows of torch tensors in HBM taken by an
index in HBM and sent as one message by a node of the same process.  torch is imported before
dora_amd loads its library, so that both use one HIP runtime.  Every scenario's outcome goes into
the JSON report named on the command line; the test asserts on it.

    python tests/tensor_take_child.py REPORT.json
"""
import ctypes
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
N = 100
KS = (0, 1, 37)
KINDS = ("bare", "dict", "ragged")


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


def values(m):
    """The (100, 6) detector output of message m, exact in float32."""
    return (np.arange(N * 6, dtype=np.float32).reshape(N, 6) * 0.5 + float(m)).astype(np.float32)


def keep_of(m, k):
    """K row numbers of message m, with repeats, different for every message."""
    return ((np.arange(k, dtype=np.int64) * 7 + 3 * m) % N).astype(np.int64)


def counts_of(k):
    """Per-image counts over the K kept rows: three images, the middle one empty."""
    return [k // 2, 0, k - k // 2]


def fields(out):
    return {"bbox": out[:, :4], "conf": out[:, 4], "cls": out[:, 5]}


def message(kind, out, keep, counts):
    """(what send_output takes, from_numpy_take's arguments for the same message)."""
    from dora_amd import tensor
    if kind == "bare":
        return tensor.take(out[:, :4], keep)
    if kind == "dict":
        return tensor.take(fields(out), keep)
    return tensor.ragged(tensor.take(fields(out), keep), lengths=counts)


def expected(kind, out_np, keep_np, k):
    """(the pyarrow array of the message, its oracle sample and type info)."""
    from dora_amd import tensor
    from oracle.pack_ref import pack
    vals = out_np[:, :4] if kind == "bare" else fields(out_np)
    arr = tensor.from_numpy_take(vals, keep_np, **({"lengths": counts_of(k)} if kind == "ragged" else {}))
    sample, info = pack(arr)
    return arr, sample, info


def inside(t, ev):
    """`t` (not empty: a tensor of no element has no bytes to place) lies in the event's sample."""
    return t.numel() == 0 or (ev["data_ptr"] <= t.data_ptr() and
                              t.data_ptr() + t.numel() * t.element_size() <= ev["data_ptr"] + ev["data_len"])


def check_device(ev, kind, out_np, keep_np, what):
    """A device receiver's event: to_torch equals out[keep] zero-copy over the one sample, the
    type info is the oracle's and the sample byte-equal to the oracle's packing in every region."""
    from dora_amd import _lib, tensor
    from oracle.pack_ref import sample_regions
    k = len(keep_np)
    arr, sample, info = expected(kind, out_np, keep_np, k)
    assert ev["type"] == "INPUT", (what, ev["type"])
    assert ev["type_info"].to_json() == info.to_json(), what
    if not ev["on_device"]:  # K == 0: no row to gather, so at most the offsets travel, inline
        assert k == 0 and ev["value"].equals(arr), what
        return
    assert ev["data_len"] >= len(sample), what
    host = ctypes.create_string_buffer(max(ev["data_len"], 1))
    _lib.call("dora_gpu_memcpy_async", host, ev["data_ptr"], ev["data_len"], None)
    _lib.call("dora_gpu_device_sync")
    assert sample_regions(host.raw[:ev["data_len"]], info) == sample_regions(sample, info), what
    got = tensor.to_torch(ev["value"])
    if kind == "ragged":
        assert isinstance(got, tensor.Ragged), what
        off = got.offsets
        assert off.is_cuda and off.dtype == torch.int32 and inside(off, ev), what
        assert off.cpu().tolist() == np.concatenate([[0], np.cumsum(counts_of(k))]).tolist(), what
        got = got.values
    want = {"": out_np[keep_np, :4]} if kind == "bare" else {n: v[keep_np] for n, v in fields(out_np).items()}
    got = {"": got} if kind == "bare" else got
    assert list(got) == list(want), what
    for name, w in want.items():
        g = got[name]
        assert g.is_cuda and g.device.index == 0 and inside(g, ev), (what, name)  # zero-copy
        assert tuple(g.shape) == w.shape and np.array_equal(g.cpu().numpy(), w), (what, name)


def scenario_sync_rewrite(n):
    """50 synchronous sends from one (100, 6) tensor and one index, both rewritten on torch's
    stream right before each send and poisoned right after it returns, as is the tensor of
    per-image counts: in turn a bare take, a dict and a ragged batch cut by int64 lengths in HBM,
    K in turn 0, 1 and 37.  No message shows a stale or torn row."""
    dev = torch.device("cuda", 0)
    out = torch.empty((N, 6), device=dev, dtype=torch.float32)
    keep = torch.zeros(max(KS), device=dev, dtype=torch.int64)
    counts = torch.zeros(3, device=dev, dtype=torch.int64)
    seen = set()
    for m in range(50):
        kind, k = KINDS[m % 3], KS[(m // 3) % 3]
        seen.add((kind, k))
        out.copy_(torch.from_numpy(values(m)))
        keep[:k].copy_(torch.from_numpy(keep_of(m, k)))
        counts.copy_(torch.tensor(counts_of(k), dtype=torch.int64))
        n["src"].send_output("x", message(kind, out, keep[:k], counts), {"m": m})
        out.fill_(-1.0)
        keep.fill_(N - 1)
        counts.fill_(-5)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check_device(ev, kind, values(m), keep_of(m, k), f"message {m} ({kind}, K={k})")
        del ev
    torch.cuda.synchronize()
    assert len(seen) == 9, sorted(seen)
    return {"messages": 50}


def scenario_async(n):
    """Every kind and K sent with asynchronous=True and followed by sync(): the node holds every
    field, the index and the device partition until then."""
    dev = torch.device("cuda", 0)
    tx = n["src"]
    held = {}
    for kind in KINDS:
        for k in KS:
            out = torch.from_numpy(values(60 + k)).to(dev)
            keep = torch.from_numpy(keep_of(5, k)).to(dev)
            counts = torch.tensor(counts_of(k), device=dev, dtype=torch.int64)
            tx.sync()
            tx.send_output("x", message(kind, out, keep, counts), {"m": f"{kind} {k}"}, asynchronous=True)
            held[kind] = len(tx._async_tensors)
            tx.sync()
            assert tx._async_tensors == []
            out.fill_(-1.0)
            keep.fill_(0)
            counts.fill_(-1)
            ev = n["dst"].next(timeout=60)
            assert ev["metadata"] == {"m": f"{kind} {k}"}, ev["metadata"]
            check_device(ev, kind, values(60 + k), keep_of(5, k), f"async {kind} K={k}")
            del ev
    torch.cuda.synchronize()
    return {"held": held}


def scenario_host_receiver(n):
    """A receiver without a GPU gets the staged pyarrow array of from_numpy_take."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    out = torch.from_numpy(values(7)).to(dev)
    sent = 0
    for kind in KINDS:
        for k in KS:
            keep = torch.from_numpy(keep_of(9, k)).to(dev)
            counts = torch.tensor(counts_of(k), device=dev, dtype=torch.int64)
            n["src"].send_output("y", message(kind, out, keep, counts), {"m": sent})
            ev = n["hst"].next(timeout=60)
            assert ev["type"] == "INPUT" and ev["metadata"] == {"m": sent} and not ev["on_device"]
            want, _, info = expected(kind, values(7), keep_of(9, k), k)
            v = ev["value"]
            assert v.type == want.type and v.equals(want), (kind, k, str(v.type))
            v.validate(full=True)
            assert ev["type_info"].to_json() == info.to_json(), (kind, k)
            r = tensor.to_numpy(v)
            r = r.values if kind == "ragged" else r
            first = r if kind == "bare" else r["bbox"]
            assert np.array_equal(first, values(7)[keep_of(9, k), :4]), (kind, k)
            del ev, v
            sent += 1
    return {"messages": sent}


def scenario_zero_rows(n):
    """Words that are no row — -1, N, 2^32 + 1 — arrive as rows of zeros between the taken ones,
    in a well-formed message; the partition in HBM is clamped to K."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    out = torch.from_numpy(values(3)).to(dev)
    words = [5, -1, 99, N, (1 << 32) + 1, 0]
    keep = torch.tensor(words, device=dev, dtype=torch.int64)
    n["src"].send_output("x", tensor.ragged(tensor.take(fields(out), keep),
                                            lengths=torch.tensor([4, 50], device=dev)), {"m": "zero"})
    ev = n["dst"].next(timeout=60)
    r = tensor.to_torch(ev["value"])
    assert r.offsets.cpu().tolist() == [0, 4, 6], r.offsets.cpu().tolist()
    want = np.zeros((6, 4), np.float32)
    for i, w in enumerate(words):
        if 0 <= w < N:
            want[i] = values(3)[w, :4]
    assert np.array_equal(r.values["bbox"].cpu().numpy(), want)
    assert r.values["conf"].cpu().tolist()[1] == 0.0 and r.values["cls"].cpu().tolist()[3] == 0.0
    ev["value"].to_pyarrow().validate(full=True)
    del ev, r
    return {}


def scenario_refusals(n):
    from dora_amd import tensor
    from dora_amd._lib import DoraGpuError
    dev = torch.device("cuda", 0)
    out = torch.from_numpy(values(0)).to(dev)
    keep = torch.tensor([1, 2, 3], device=dev)
    for data in (tensor.take(out, [1, 2, 3]), tensor.take(values(0), keep),
                 tensor.ragged(tensor.take(fields(out), np.array([1, 2])), lengths=[2])):
        try:
            n["src"].send_output("x", data)
            raise AssertionError("an index away from its values was sent")
        except TypeError as e:
            assert "move the index next to the values" in str(e), str(e)
    try:
        n["src"].send_output("x", tensor.ragged(tensor.take(out, keep), lengths=[N]))
        raise AssertionError("a host partition of the N source rows was sent")
    except DoraGpuError as e:
        assert e.code == -1 and "3 rows" in str(e), str(e)
    try:
        n["src"].send_output("x", tensor.take(out, keep.to(torch.float32)))
        raise AssertionError("a float index was sent")
    except DoraGpuError as e:
        assert e.code == -1 and "int32 or int64" in str(e), str(e)
    # nothing was sent: the next valid take is the next message (an int32 index this time)
    n["src"].send_output("x", tensor.take(out[:, :4], keep.to(torch.int32)), {"m": "next"})
    ev = n["dst"].next(timeout=60)
    assert ev["metadata"] == {"m": "next"}, ev.get("metadata")
    check_device(ev, "bare", values(0), np.array([1, 2, 3]), "after refusals")
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
                                 ("async", scenario_async),
                                 ("host_receiver", scenario_host_receiver),
                                 ("zero_rows", scenario_zero_rows),
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
