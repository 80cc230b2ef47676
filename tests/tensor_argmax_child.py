"""Child process of test_gpu_tensor_argmax_dataflow.py: torch logits in HBM reduced to class maps
on send by a node of the same process.  torch is imported before dora_amd loads its library, so
that both use one HIP runtime.  Every scenario's outcome goes into the JSON report named on the
command line; the test asserts on it.

    python tests/tensor_argmax_child.py REPORT.json
"""
import json
import os
import sys
import traceback

import torch  # first: see above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dora_amd import launcher as launcher_mod  # noqa: E402
from tests.tensor_cast_child import DESC, inside, nodes  # noqa: E402


def logits_of(m, shape, dtype):
    g = torch.Generator().manual_seed(m)
    return (torch.randn(*shape, generator=g) * 8).to(dtype)


def check(ev, want, what):
    """A device receiver's event: tensor.to_torch is zero-copy over the one sample and equal to
    `want` (a CPU torch tensor, or a dict of them), dtype and shape included."""
    from dora_amd import tensor
    assert ev["type"] == "INPUT" and ev["on_device"], (what, ev["type"])
    got = tensor.to_torch(ev["value"])
    record = isinstance(want, dict)
    got, want = (got, want) if record else ({"": got}, {"": want})
    assert list(got) == list(want), what
    for name, w in want.items():
        g = got[name]
        assert g.is_cuda and g.device.index == 0 and inside(g, ev), (what, name)
        h = g.cpu()
        assert h.dtype == w.dtype and h.shape == w.shape, (what, name, h.dtype, h.shape)
        assert torch.equal(h, w), (what, name)


def scenario_segmentation(n):
    """float16 (19, 64, 96) logits along 0 to uint8, rewritten before and poisoned after every
    synchronous send."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    x = torch.empty((19, 64, 96), device=dev, dtype=torch.float16)
    for m in range(3):
        src = logits_of(m, (19, 64, 96), torch.float16)
        x.copy_(src)
        n["src"].send_output("x", tensor.argmax(x, 0, torch.uint8), {"m": m})
        x.fill_(float("nan"))
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, torch.argmax(src.float(), 0).to(torch.uint8), f"segmentation {m}")
        del ev
    torch.cuda.synchronize()
    return {"messages": 3}


def scenario_classifier(n):
    """bfloat16 (33, 1000) logits along -1 to int32: the wave body."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    for m in range(2):
        src = logits_of(10 + m, (33, 1000), torch.bfloat16)
        x = src.to(dev)
        n["src"].send_output("x", tensor.argmax(x, -1, "int32"), {"m": m})
        x.fill_(0)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, torch.argmax(src.float(), -1).to(torch.int32), f"classifier {m}")
        del ev
    torch.cuda.synchronize()
    return {"messages": 2}


def scenario_record(n):
    """A dict of a class map and a strided float32 field, synchronously and with
    asynchronous=True followed by sync(): the asynchronous send holds both tensors."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    held = None
    for m, asynchronous in enumerate((False, True)):
        src = logits_of(20 + m, (48, 21, 40), torch.float16)
        depth = torch.rand(48, 80, generator=torch.Generator().manual_seed(m))
        x, d = src.to(dev), depth.to(dev)
        n["src"].sync()
        n["src"].send_output("x", {"cls": tensor.argmax(x, 1, "uint8"), "depth": d[:, ::2]},
                             {"m": m}, asynchronous=asynchronous)
        if asynchronous:
            held = len(n["src"]._async_tensors)
            n["src"].sync()
            assert n["src"]._async_tensors == []
        x.fill_(1)
        d.fill_(-1.0)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, {"cls": torch.argmax(src.float(), 1).to(torch.uint8),
                   "depth": depth[:, ::2].contiguous()}, f"record {m}")
        del ev
    torch.cuda.synchronize()
    return {"held": held}


def scenario_host_receiver(n):
    """A receiver without a GPU gets the staged pyarrow array of from_numpy_argmax."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    src = logits_of(30, (7, 9, 130), torch.float32)
    n["src"].send_output("y", tensor.argmax(src.to(dev), 2, "uint16"), {"m": "host"})
    ev = n["hst"].next(timeout=60)
    assert ev["type"] == "INPUT" and ev["metadata"] == {"m": "host"} and not ev["on_device"]
    want = tensor.from_numpy_argmax(src.numpy(), 2, "uint16")
    v = ev["value"]
    assert v.type == want.type and v.equals(want), str(v.type)
    v.validate(full=True)
    del ev, v
    return {}


def scenario_refused(n):
    """What the send refuses raises in the producer; the next send goes through."""
    from dora_amd import tensor
    from dora_amd._lib import DoraGpuError
    dev = torch.device("cuda", 0)
    src = logits_of(40, (5, 300), torch.float16)
    x = src.to(dev)
    errors = []
    for data in (tensor.argmax(x, 1, "uint8"), tensor.argmax(x, 2), tensor.argmax(x[0], 0),
                 tensor.argmax(x.double(), 1),
                 {"a": tensor.argmax(x, 1), "b": tensor.cast(x, "float32")}):
        try:
            n["src"].send_output("x", data)
            raise AssertionError("a refused argmax was sent")
        except DoraGpuError as e:
            errors.append(e.code)
    assert errors == [-1, -1, -1, -4, -4], errors
    n["src"].send_output("x", tensor.argmax(x, 1, "int64"), {"m": "after"})
    ev = n["dst"].next(timeout=60)
    assert ev["metadata"] == {"m": "after"}, ev["metadata"]
    check(ev, torch.argmax(src.float(), 1), "after")
    del ev
    return {"refused": len(errors)}


def main(report_path):
    report = {}
    lch = launcher_mod.Launcher()  # before HIP is initialised in this process
    try:
        from dora_amd.dataflow import Dataflow
        torch.cuda.set_device(0)
        with Dataflow(DESC, launcher=lch) as df:
            n = nodes(df, {"src": 0, "dst": 0, "hst": -1})
            try:
                for name, fn in [("segmentation", scenario_segmentation),
                                 ("classifier", scenario_classifier), ("record", scenario_record),
                                 ("host_receiver", scenario_host_receiver),
                                 ("refused", scenario_refused)]:
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
