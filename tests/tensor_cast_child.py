"""Child process of test_gpu_tensor_cast_dataflow.py: torch tensors in HBM converted on send by a
node of the same process.  torch is imported before dora_amd loads its library, so that both use
one HIP runtime.  Every scenario's outcome goes into the JSON report named on the command line;
the test asserts on it.

    python tests/tensor_cast_child.py REPORT.json
"""
import json
import os
import sys
import threading
import traceback

import torch  # first: see above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dora_amd import launcher as launcher_mod  # noqa: E402

DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["x", "y"]},
    {"id": "dst", "path": "dynamic", "inputs": {"x": {"source": "src/x", "queue_size": 10}}},
    {"id": "hst", "path": "dynamic", "inputs": {"y": {"source": "src/y", "queue_size": 10}},
     "_unstable_deploy": {"gpu": -1}},
]}
S255 = 1 / 255


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


def frame_of(m):
    """The 6 x 8 x 3 uint8 frame of message m (CPU)."""
    g = torch.Generator().manual_seed(m)
    return torch.randint(0, 256, (6, 8, 3), dtype=torch.uint8, generator=g)


def logits_of(m):
    g = torch.Generator().manual_seed(100 + m)
    return (torch.randn(33, 7, generator=g) * 50).to(torch.bfloat16)


def conf_of(m):
    g = torch.Generator().manual_seed(200 + m)
    return torch.rand(6, generator=g)


def torch_cast(x, dst, scale=None):
    """torch's own statement on the CPU: x.float().mul(s).to(dst)."""
    y = x.float()
    if scale is not None:
        y = y.mul(torch.tensor(scale, dtype=torch.float32))
    return y.to(dst)


def inside(t, ev):
    return ev["data_ptr"] <= t.data_ptr() and \
        t.data_ptr() + t.numel() * t.element_size() <= ev["data_ptr"] + ev["data_len"]


def check(ev, want, what):
    """A device receiver's event: tensor.to_torch is zero-copy over the one sample and equal to
    `want` (a CPU tensor, or a dict of them)."""
    from dora_amd import tensor
    assert ev["type"] == "INPUT" and ev["on_device"], (what, ev["type"])
    got = tensor.to_torch(ev["value"])
    record = isinstance(want, dict)
    got, want = (got, want) if record else ({"": got}, {"": want})
    assert list(got) == list(want), what
    for name, w in want.items():
        g = got[name]
        assert g.is_cuda and g.device.index == 0 and inside(g, ev), (what, name)
        assert g.dtype == w.dtype and tuple(g.shape) == tuple(w.shape), (what, name, g.dtype)
        assert torch.equal(g.cpu(), w), (what, name)


def scenario_frame(n):
    """A uint8 HWC frame in HBM sent as float16 CHW in [0, 1], rewritten before and poisoned
    after every synchronous send."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    frame = torch.empty((6, 8, 3), device=dev, dtype=torch.uint8)
    for m in range(6):
        frame.copy_(frame_of(m))
        n["src"].send_output("x", tensor.cast(frame.permute(2, 0, 1), torch.float16, scale=S255),
                             {"m": m})
        frame.fill_(77)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, torch_cast(frame_of(m).permute(2, 0, 1), torch.float16, S255), f"frame {m}")
        del ev
    torch.cuda.synchronize()
    return {"messages": 6}


def scenario_bfloat16(n):
    """A bfloat16 tensor in HBM sent as float32, dense and as a strided view; on its own it is
    still no tensor message."""
    from dora_amd import tensor
    from dora_amd._lib import DoraGpuError
    dev = torch.device("cuda", 0)
    x = logits_of(0).to(dev)
    for m, view in enumerate((x, x[:, 1:6], x.t())):
        n["src"].send_output("x", tensor.cast(view, torch.float32), {"m": m})
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, torch_cast(view.cpu(), torch.float32), f"bfloat16 view {m}")
        del ev
    try:
        n["src"].send_output("x", x)
        raise AssertionError("a bfloat16 tensor was sent as it is")
    except DoraGpuError as e:
        assert e.code == -4 and "bfloat16" in str(e), str(e)
    return {"messages": 3}


def scenario_record(n):
    """The mixed record: a converted image next to a field sent as it is, synchronously and with
    asynchronous=True followed by sync()."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    held = None
    for m, asynchronous in enumerate((False, True)):
        img, conf = frame_of(10 + m).to(dev), conf_of(m).to(dev)
        n["src"].sync()
        n["src"].send_output("x", {"image": tensor.cast(img, "float16", scale=S255), "conf": conf},
                             {"m": m}, asynchronous=asynchronous)
        if asynchronous:
            held = len(n["src"]._async_tensors)
            n["src"].sync()
            assert n["src"]._async_tensors == []
        img.fill_(1)
        conf.fill_(-1.0)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, {"image": torch_cast(frame_of(10 + m), torch.float16, S255), "conf": conf_of(m)},
              f"record {m}")
        del ev
    torch.cuda.synchronize()
    return {"held": held}


def scenario_host_receiver(n):
    """A receiver without a GPU gets the staged pyarrow array of from_numpy_cast."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    frame = frame_of(3)
    n["src"].send_output("y", tensor.cast(frame.to(dev).permute(2, 0, 1), "float32", scale=S255),
                         {"m": "host"})
    ev = n["hst"].next(timeout=60)
    assert ev["type"] == "INPUT" and ev["metadata"] == {"m": "host"} and not ev["on_device"]
    want = tensor.from_numpy_cast(frame.permute(2, 0, 1).numpy(), "float32", S255)
    v = ev["value"]
    assert v.type == want.type and v.equals(want), str(v.type)
    v.validate(full=True)
    del ev, v
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
                for name, fn in [("frame", scenario_frame), ("bfloat16", scenario_bfloat16),
                                 ("record", scenario_record),
                                 ("host_receiver", scenario_host_receiver)]:
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
