"""Child process of test_gpu_tensor_affine_dataflow.py: torch tensors in HBM normalised and
quantised per channel on send by a node of the same process, the tables float32 tensors in HBM.
torch is imported before dora_amd loads its library, so that both use one HIP runtime.  Every
scenario's outcome goes into the JSON report named on the command line; the test asserts on it.

    python tests/tensor_affine_child.py REPORT.json
"""
import json
import os
import sys
import traceback

import numpy as np
import torch  # first: see above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dora_amd import launcher as launcher_mod  # noqa: E402
from tests.tensor_cast_child import DESC, inside, nodes  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def tables():
    """(scale, bias) of (x / 255 - mean) / std as x * s + b: float32 numpy."""
    mean, std = np.array(MEAN, np.float64), np.array(STD, np.float64)
    return (1 / (255 * std)).astype(np.float32), (-mean / std).astype(np.float32)


def frame_of(m):
    g = torch.Generator().manual_seed(m)
    return torch.randint(0, 256, (37, 53, 3), dtype=torch.uint8, generator=g)


def feat_of(m):
    g = torch.Generator().manual_seed(100 + m)
    return (torch.randn(5, 17, 9, generator=g) * 40).to(torch.float16)


def per_channel():
    return (np.random.default_rng(3).random(17) * 2 + 0.25).astype(np.float32)


def oracle(arr):
    """The numpy array (or dict of them) of a statement-of-record pyarrow array."""
    from dora_amd import tensor
    return tensor.to_numpy(arr)


def check(ev, want, what):
    """A device receiver's event: tensor.to_torch is zero-copy over the one sample and equal bit
    for bit to `want` (a numpy array without NaNs, or a dict of them)."""
    from dora_amd import tensor
    assert ev["type"] == "INPUT" and ev["on_device"], (what, ev["type"])
    got = tensor.to_torch(ev["value"])
    record = isinstance(want, dict)
    got, want = (got, want) if record else ({"": got}, {"": want})
    assert list(got) == list(want), what
    for name, w in want.items():
        g = got[name]
        assert g.is_cuda and g.device.index == 0 and inside(g, ev), (what, name)
        h = g.cpu().numpy()
        assert h.dtype == w.dtype and h.shape == w.shape, (what, name, h.dtype, h.shape)
        assert h.tobytes() == np.ascontiguousarray(w).tobytes(), (what, name)


def scenario_frame(n):
    """A 37 x 53 x 3 uint8 frame in HBM sent as normalised CHW float16, rewritten before and
    poisoned after every synchronous send; the tables are made once on the device."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    s, b = tables()
    sd, bd = torch.from_numpy(s).to(dev), torch.from_numpy(b).to(dev)
    frame = torch.empty((37, 53, 3), device=dev, dtype=torch.uint8)
    for m in range(4):
        frame.copy_(frame_of(m))
        n["src"].send_output("x", tensor.cast(frame.permute(2, 0, 1), "float16", scale=sd, bias=bd,
                                              axis=0), {"m": m})
        frame.fill_(77)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        want = tensor.from_numpy_cast(frame_of(m).permute(2, 0, 1).numpy(), "float16", s, bias=b,
                                      axis=0)
        check(ev, oracle(want), f"frame {m}")
        del ev
    torch.cuda.synchronize()
    return {"messages": 4}


def scenario_quantise(n):
    """A float16 (5, 17, 9) tensor quantised to int8 with one scale per channel along axis 1."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    per = per_channel()
    pd = torch.from_numpy(per).to(dev)
    for m in range(2):
        feat = feat_of(m).to(dev)
        n["src"].send_output("x", tensor.quantize(feat, "int8", scale=pd, axis=1), {"m": m})
        feat.fill_(1)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        want = tensor.from_numpy_quantize(feat_of(m).numpy(), "int8", per, axis=1)
        check(ev, oracle(want), f"quantise {m}")
        del ev
    torch.cuda.synchronize()
    return {"messages": 2}


def scenario_record(n):
    """A dict mixing both with a plain field, synchronously and with asynchronous=True followed by
    sync(): the asynchronous send holds the three fields and the three tables."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    s, b = tables()
    per = per_channel()
    sd, bd, pd = (torch.from_numpy(t).to(dev) for t in (s, b, per))
    held = None
    for m, asynchronous in enumerate((False, True)):
        img = frame_of(10 + m)[:5].to(dev)          # 5 x 53 x 3: the leading extent of `feat`
        feat = feat_of(10 + m).to(dev)
        conf = torch.rand(5, generator=torch.Generator().manual_seed(m))
        confd = conf.to(dev)
        n["src"].sync()
        n["src"].send_output("x", {"image": tensor.cast(img, "float16", scale=sd, bias=bd, axis=-1),
                                   "act": tensor.quantize(feat, "int8", scale=pd, axis=1),
                                   "conf": confd}, {"m": m}, asynchronous=asynchronous)
        if asynchronous:
            held = len(n["src"]._async_tensors)
            n["src"].sync()
            assert n["src"]._async_tensors == []
        img.fill_(1)
        feat.fill_(1)
        confd.fill_(-1.0)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        want = {"image": oracle(tensor.from_numpy_cast(frame_of(10 + m)[:5].numpy(), "float16", s,
                                                       bias=b, axis=-1)),
                "act": oracle(tensor.from_numpy_quantize(feat_of(10 + m).numpy(), "int8", per, axis=1)),
                "conf": conf.numpy()}
        check(ev, want, f"record {m}")
        del ev
    torch.cuda.synchronize()
    return {"held": held}


def scenario_host_receiver(n):
    """A receiver without a GPU gets the staged pyarrow array of from_numpy_cast."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    s, b = tables()
    frame = frame_of(3)
    n["src"].send_output("y", tensor.cast(frame.to(dev).permute(2, 0, 1), "float32",
                                          scale=torch.from_numpy(s).to(dev),
                                          bias=torch.from_numpy(b).to(dev), axis=0), {"m": "host"})
    ev = n["hst"].next(timeout=60)
    assert ev["type"] == "INPUT" and ev["metadata"] == {"m": "host"} and not ev["on_device"]
    want = tensor.from_numpy_cast(frame.permute(2, 0, 1).numpy(), "float32", s, bias=b, axis=0)
    v = ev["value"]
    assert v.type == want.type and v.equals(want), str(v.type)
    v.validate(full=True)
    del ev, v
    return {}


def scenario_host_table(n):
    """A host table over device values raises in the producer, and so does a device table over
    host values; the next send goes through."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    s, b = tables()
    frame = frame_of(4).to(dev)
    errors = []
    for data in (tensor.cast(frame, "float16", scale=s, axis=2),
                 tensor.cast(frame, "float16", scale=torch.from_numpy(s).to(dev), bias=b.tolist(), axis=2),
                 tensor.cast(frame.cpu(), "float16", scale=torch.from_numpy(s).to(dev), axis=2)):
        try:
            n["src"].send_output("x", data)
            raise AssertionError("a table away from its values was sent")
        except TypeError as e:
            errors.append(str(e))
    assert "once on the device" in errors[0] and "once on the device" in errors[1], errors
    assert "next to the values" in errors[2], errors
    n["src"].send_output("x", tensor.cast(frame, "float16", scale=torch.from_numpy(s).to(dev), axis=2),
                         {"m": "after"})
    ev = n["dst"].next(timeout=60)
    assert ev["metadata"] == {"m": "after"}, ev["metadata"]
    check(ev, oracle(tensor.from_numpy_cast(frame_of(4).numpy(), "float16", s, axis=2)), "after")
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
                for name, fn in [("frame", scenario_frame), ("quantise", scenario_quantise),
                                 ("record", scenario_record),
                                 ("host_receiver", scenario_host_receiver),
                                 ("host_table", scenario_host_table)]:
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
