"""Child process of test_gpu_tensor_mask_dataflow.py: rows of torch tensors in HBM selected by a
bool mask in HBM and sent as one message by a node of the same process.  torch is imported before
dora_amd loads its library, so that both use one HIP runtime.  Every scenario's outcome goes into
the JSON report named on the command line; the test asserts on it.

    python tests/tensor_mask_child.py REPORT.json
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
N = 300
KINDS = ("tensor", "record", "ragged")
COUNTS = [120, 0, 180]  # candidates per image over the N source rows


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
    """The (300, 6) detector output of message m, exact in float32."""
    return (np.arange(N * 6, dtype=np.float32).reshape(N, 6) * 0.5 + float(m)).astype(np.float32)


def mask_of(m):
    """The mask of message m, different for every message: none, all, or a third of the rows."""
    if m % 7 == 5:
        return np.zeros(N, np.bool_)
    if m % 7 == 6:
        return np.ones(N, np.bool_)
    return ((np.arange(N) * 11 + 3 * m) % 97) < 33


def fields(out):
    return {"bbox": out[:, :4], "conf": out[:, 4], "cls": out[:, 5]}


def message(kind, out, keep, counts):
    from dora_amd import tensor
    if kind == "tensor":
        return tensor.masked(out[:, :4], keep)
    if kind == "record":
        return tensor.masked(fields(out), keep)
    return tensor.ragged(tensor.masked(fields(out), keep), lengths=counts)


def expected(kind, out_np, keep_np):
    """(the pyarrow array of the message, its oracle sample and type info)."""
    from dora_amd import tensor
    from oracle.pack_ref import pack
    vals = out_np[:, :4] if kind == "tensor" else fields(out_np)
    arr = tensor.from_numpy_masked(vals, keep_np, **({"lengths": COUNTS} if kind == "ragged" else {}))
    sample, info = pack(arr)
    return arr, sample, info


def inside(t, ev):
    return t.numel() == 0 or (ev["data_ptr"] <= t.data_ptr() and
                              t.data_ptr() + t.numel() * t.element_size() <= ev["data_ptr"] + ev["data_len"])


def check_device(ev, kind, out_np, keep_np, what):
    """A device receiver's event: the type info is the oracle's, the sample byte-equal to the
    oracle's packing of from_numpy_masked in every region — and no longer than it: the workspace
    does not travel — and to_torch gives the N-row values zero-copy over the one sample, the first
    offsets[-1] of them the selected rows."""
    from dora_amd import _lib, tensor
    from oracle.pack_ref import sample_regions
    arr, sample, info = expected(kind, out_np, keep_np)
    assert ev["type"] == "INPUT", (what, ev["type"])
    assert ev["type_info"].to_json() == info.to_json(), what
    assert ev["on_device"] and ev["data_len"] == len(sample), (what, ev["data_len"], len(sample))
    host = ctypes.create_string_buffer(max(ev["data_len"], 1))
    _lib.call("dora_gpu_memcpy_async", host, ev["data_ptr"], ev["data_len"], None)
    _lib.call("dora_gpu_device_sync")
    assert sample_regions(host.raw[:ev["data_len"]], info) == sample_regions(sample, info), what
    got = tensor.to_torch(ev["value"])
    assert isinstance(got, tensor.Ragged), what
    off = got.offsets
    assert off.is_cuda and off.dtype == torch.int32 and inside(off, ev), what
    assert off.cpu().tolist() == arr.offsets.to_pylist(), (what, off.cpu().tolist())
    k = int(keep_np.sum())
    assert off.cpu().tolist()[-1] == k, what
    src = {"": out_np[:, :4]} if kind == "tensor" else fields(out_np)
    got = {"": got.values} if kind == "tensor" else got.values
    assert list(got) == list(src), what
    for name, v in src.items():
        g = got[name]
        assert g.is_cuda and g.device.index == 0 and inside(g, ev), (what, name)  # zero-copy
        assert g.shape[0] == N and tuple(g.shape[1:]) == v.shape[1:], (what, name)
        h = g.cpu().numpy()
        assert np.array_equal(h[:k], v[keep_np]) and not h[k:].any(), (what, name)


def scenario_sync_rewrite(n):
    """42 synchronous sends from one (300, 6) tensor, one bool mask and one tensor of per-image
    counts, all rewritten on torch's stream right before each send and poisoned right after it
    returns: in turn a bare tensor, a record and a record under a ragged batch cut by int64
    lengths in HBM, the mask in turn a third of the rows, none and all.  No message shows a stale
    or torn row."""
    dev = torch.device("cuda", 0)
    out = torch.empty((N, 6), device=dev, dtype=torch.float32)
    keep = torch.zeros(N + 3, device=dev, dtype=torch.bool)[3:]  # 3 mod 16: mask[3:] is dense
    counts = torch.zeros(3, device=dev, dtype=torch.int64)
    seen = set()
    for m in range(42):
        kind = KINDS[m % 3]
        seen.add((kind, m % 7))
        out.copy_(torch.from_numpy(values(m)))
        keep.copy_(torch.from_numpy(mask_of(m)))
        counts.copy_(torch.tensor(COUNTS, dtype=torch.int64))
        n["src"].send_output("x", message(kind, out, keep, counts), {"m": m})
        out.fill_(-1.0)
        keep.fill_(m % 2 == 0)
        counts.fill_(-5)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check_device(ev, kind, values(m), mask_of(m), f"message {m} ({kind})")
        del ev
    torch.cuda.synchronize()
    assert len(seen) == 21, sorted(seen)
    return {"messages": 42}


def scenario_async_bursts(n):
    """Bursts of 8 sends with asynchronous=True, each from tensors of its own, then sync(): the
    node holds every field, the mask and the device partition until then, and the eight samples
    in flight — each with its own workspace behind it — do not disturb one another."""
    dev = torch.device("cuda", 0)
    tx = n["src"]
    held = {}
    for burst, kind in enumerate(KINDS):
        tx.sync()
        live = []
        for i in range(8):
            m = 100 + 8 * burst + i
            out = torch.from_numpy(values(m)).to(dev)
            keep = torch.from_numpy(mask_of(m)).to(dev)
            counts = torch.tensor(COUNTS, device=dev, dtype=torch.int64)
            live.append((out, keep, counts))
            tx.send_output("x", message(kind, out, keep, counts), {"m": m}, asynchronous=True)
            if i == 0:
                held[kind] = len(tx._async_tensors)
        tx.sync()
        assert tx._async_tensors == []
        for out, keep, counts in live:
            out.fill_(-1.0)
            keep.fill_(False)
            counts.fill_(-1)
        for i in range(8):
            m = 100 + 8 * burst + i
            ev = n["dst"].next(timeout=60)
            assert ev["metadata"] == {"m": m}, ev["metadata"]
            check_device(ev, kind, values(m), mask_of(m), f"async {kind} message {m}")
            del ev
    torch.cuda.synchronize()
    return {"held": held, "messages": 24}


def scenario_host_receiver(n):
    """A receiver without a GPU gets the staged pyarrow array of from_numpy_masked: the sample
    alone is staged, not the workspace behind it."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    sent = 0
    for kind in KINDS:
        for m in (1, 5, 6):
            out = torch.from_numpy(values(m)).to(dev)
            keep = torch.from_numpy(mask_of(m)).to(dev)
            counts = torch.tensor(COUNTS, device=dev, dtype=torch.int64)
            n["src"].send_output("y", message(kind, out, keep, counts), {"m": sent})
            ev = n["hst"].next(timeout=60)
            assert ev["type"] == "INPUT" and ev["metadata"] == {"m": sent} and not ev["on_device"]
            want, _, info = expected(kind, values(m), mask_of(m))
            v = ev["value"]
            assert v.type == want.type and v.equals(want), (kind, m, str(v.type))
            v.validate(full=True)
            assert ev["type_info"].to_json() == info.to_json(), (kind, m)
            r = tensor.to_numpy(v)
            assert isinstance(r, tensor.Ragged), (kind, m)
            lists = r.unbind()
            first = np.concatenate([x if kind == "tensor" else x["bbox"] for x in lists])
            assert np.array_equal(first, values(m)[mask_of(m), :4]), (kind, m)
            del ev, v
            sent += 1
    return {"messages": sent}


def scenario_garbage_partition(n):
    """A partition in HBM that does not describe the N rows: the offsets follow the clamped
    formula through C, a well-formed List whatever the words hold; a uint8 mask with set bytes of
    2 and 0x80 selects like a bool one."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    out = torch.from_numpy(values(3)).to(dev)
    keep_np = mask_of(3)
    keep = torch.from_numpy(keep_np.astype(np.uint8) * np.where(np.arange(N) % 2, 2, 0x80).astype(np.uint8)).to(dev)
    words = [50, -7, 1 << 40, 3]
    n["src"].send_output("x", tensor.ragged(tensor.masked(fields(out), keep),
                                            lengths=torch.tensor(words, device=dev)), {"m": "garbage"})
    ev = n["dst"].next(timeout=60)
    r = tensor.to_torch(ev["value"])
    c = np.concatenate([[0], np.cumsum(keep_np)])
    assert r.offsets.cpu().tolist() == [0, int(c[50]), int(c[50]), int(c[N]), int(c[N])], \
        r.offsets.cpu().tolist()
    k = int(keep_np.sum())
    assert np.array_equal(r.values["bbox"].cpu().numpy()[:k], values(3)[keep_np, :4])
    ev["value"].to_pyarrow().validate(full=True)
    del ev, r
    return {}


def scenario_refusals(n):
    from dora_amd import tensor
    from dora_amd._lib import DoraGpuError
    dev = torch.device("cuda", 0)
    out = torch.from_numpy(values(0)).to(dev)
    keep = torch.from_numpy(mask_of(0)).to(dev)
    for data in (tensor.masked(out, mask_of(0)), tensor.masked(values(0), keep),
                 tensor.ragged(tensor.masked(fields(out), mask_of(0).tolist()), lengths=[N])):
        try:
            n["src"].send_output("x", data)
            raise AssertionError("a mask away from its values was sent")
        except TypeError as e:
            assert "move the mask next to the values" in str(e), str(e)
    for data, word in ((tensor.ragged(tensor.masked(out, keep), lengths=[int(mask_of(0).sum())]),
                        f"{N} rows"),
                       (tensor.masked(out, keep.to(torch.int32)), "is not bool or uint8"),
                       (tensor.masked(out, keep[:N - 1]), f"mask has {N - 1} elements"),
                       (tensor.masked(out, torch.zeros(2 * N, device=dev, dtype=torch.bool)[::2]),
                        "the mask is dense")):
        try:
            n["src"].send_output("x", data)
            raise AssertionError("sent: " + word)
        except DoraGpuError as e:
            assert e.code == -1 and word in str(e), str(e)
    # nothing was sent: the next valid mask is the next message
    n["src"].send_output("x", tensor.masked(out[:, :4], keep), {"m": "next"})
    ev = n["dst"].next(timeout=60)
    assert ev["metadata"] == {"m": "next"}, ev.get("metadata")
    check_device(ev, "tensor", values(0), mask_of(0), "after refusals")
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
                                 ("async_bursts", scenario_async_bursts),
                                 ("host_receiver", scenario_host_receiver),
                                 ("garbage_partition", scenario_garbage_partition),
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
