"""Child process of test_gpu_tensor_quant_dataflow.py: torch tensors in HBM quantised on send by a
node of the same process.  torch is imported before dora_amd loads its library, so that both use
one HIP runtime.  Every scenario's outcome goes into the JSON report named on the command line;
the test asserts on it.

    python tests/tensor_quant_child.py REPORT.json
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


def prob_of(m):
    """The (3, 48, 64) float16 map in [0, 1] of message m (CPU)."""
    g = torch.Generator().manual_seed(m)
    return torch.rand(3, 48, 64, generator=g).to(torch.float16)


def depth_of(m):
    """A (48, 64) float32 depth map in metres, some of it past 65.535 m, one NaN and one inf."""
    g = torch.Generator().manual_seed(100 + m)
    d = torch.rand(48, 64, generator=g) * 80.0
    d[0, 0], d[0, 1], d[0, 2] = float("nan"), float("inf"), -1.0
    return d


def feat_of(m):
    g = torch.Generator().manual_seed(200 + m)
    return (torch.randn(48, 5, generator=g) * 50).to(torch.bfloat16)


def quantized(x, dst, scale=None, zp=0, bfloat16=False):
    """tensor.from_numpy_quantize of the CPU tensor `x`, as a torch tensor."""
    import numpy as np
    from dora_amd import tensor
    a = x.view(torch.int16).numpy().view(np.uint16) if bfloat16 else x.numpy()
    arr = tensor.from_numpy_quantize(a, dst, scale, zp, bfloat16=bfloat16)
    return torch.from_numpy(np.ascontiguousarray(tensor.to_numpy(arr)))


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
        assert tuple(g.shape) == tuple(w.shape) and g.element_size() == w.element_size(), (what, name)
        # (torch may lack uint16 arithmetic: compare the bytes)
        assert g.cpu().contiguous().view(torch.uint8).equal(w.contiguous().view(torch.uint8)), (what, name)


def scenario_mask(n):
    """A (3, 48, 64) float16 map in [0, 1], permuted to HWC, arrives as uint8 * 255."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    x = torch.empty((3, 48, 64), device=dev, dtype=torch.float16)
    for m in range(3):
        x.copy_(prob_of(m))
        n["src"].send_output("x", tensor.quantize(x.permute(1, 2, 0), torch.uint8, scale=255), {"m": m})
        x.fill_(0.5)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, quantized(prob_of(m).permute(1, 2, 0), "uint8", 255), f"mask {m}")
        del ev
    torch.cuda.synchronize()
    return {"messages": 3}


def scenario_depth(n):
    """A (48, 64) float32 depth map arrives as uint16 * 1000, saturated past 65.535 m."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    for m in range(2):
        d = depth_of(m).to(dev)
        n["src"].send_output("x", tensor.quantize(d, "uint16", scale=1000), {"m": m})
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        want = quantized(depth_of(m), "uint16", 1000)
        assert int(want[0, 0]) == 0 and int(want[0, 1]) == 65535 and int(want[0, 2]) == 0
        check(ev, want, f"depth {m}")
        del ev
    torch.cuda.synchronize()
    return {"messages": 2}


def scenario_record(n):
    """The mixed record: a quantised, a cast and a plain field, synchronously and with
    asynchronous=True followed by sync()."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    held = None
    for m, asynchronous in enumerate((False, True)):
        mask = prob_of(m)[0].float()[:, :7].contiguous()
        feat, ids = feat_of(m), torch.arange(48, dtype=torch.int64) * 3 + m
        dm, df, di = mask.to(dev), feat.to(dev), ids.to(dev)
        n["src"].sync()
        n["src"].send_output("x", {"mask": tensor.quantize(dm, "uint8", 255),
                                   "feat": tensor.cast(df, "float32"), "ids": di},
                             {"m": m}, asynchronous=asynchronous)
        if asynchronous:
            held = len(n["src"]._async_tensors)
            n["src"].sync()
            assert n["src"]._async_tensors == []
        dm.fill_(1)
        df.fill_(1)
        di.fill_(-1)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, {"mask": quantized(mask, "uint8", 255), "feat": feat.float(), "ids": ids},
              f"record {m}")
        del ev
    torch.cuda.synchronize()
    return {"held": held}


def scenario_host_receiver(n):
    """A receiver without a GPU gets the pyarrow array of from_numpy_quantize; a host producer's
    numpy array, quantised by the CPU inside the send, gives the same message."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    x = prob_of(7)
    want = tensor.from_numpy_quantize(x.permute(1, 2, 0).numpy(), "int8", 255, -128)
    for m, src in enumerate((x.to(dev), x.numpy())):
        view = src.permute(1, 2, 0) if m == 0 else src.transpose(1, 2, 0)
        n["src"].send_output("y", tensor.quantize(view, "int8", scale=255, zero_point=-128), {"m": m})
        ev = n["hst"].next(timeout=60)
        assert ev["type"] == "INPUT" and ev["metadata"] == {"m": m} and not ev["on_device"]
        v = ev["value"]
        assert v.type == want.type and v.equals(want), (m, str(v.type))
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
                for name, fn in [("mask", scenario_mask), ("depth", scenario_depth),
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
