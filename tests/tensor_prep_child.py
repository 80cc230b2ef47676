"""Child process of test_gpu_tensor_prep_dataflow.py: a torch frame in HBM letterboxed and
normalised on send, and crops of it normalised by tables in HBM, by a node of the same process.
torch is imported before dora_amd loads its library, so that both use one HIP runtime.  Every
scenario's outcome goes into the JSON report named on the command line; the test asserts on it.

    python tests/tensor_prep_child.py REPORT.json
"""
import json
import os
import sys
import traceback

import torch  # first: see above

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dora_amd import launcher as launcher_mod  # noqa: E402
from tests.tensor_argmax_child import check  # noqa: E402
from tests.tensor_cast_child import DESC, nodes  # noqa: E402
from tests.tensor_crops_child import BOXES, never_read_on_the_host  # noqa: E402
from tests.tensor_resize_child import frame_of  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SCALE = [1.0 / (255.0 * d) for d in STD]
BIAS = [-m / d for m, d in zip(MEAN, STD)]


def scenario_letterbox(n):
    """A (54, 96, 3) uint8 frame through permute(2, 0, 1) letterboxed into 3 x 64 x 64 float16 with
    per-channel tables in HBM; frame and tables rewritten before and poisoned after every
    synchronous send, the tables never read on the host."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    x = torch.empty((54, 96, 3), device=dev, dtype=torch.uint8)
    s = torch.empty(3, device=dev, dtype=torch.float32)
    b = torch.empty(3, device=dev, dtype=torch.float32)
    inner, lead = tensor.letterbox((54, 96), (64, 64))
    assert (inner, lead) == ((36, 64), (14, 0)), (inner, lead)
    for m in range(3):
        src = frame_of(m)
        sv = [v * (m + 1) for v in SCALE]
        x.copy_(src)
        s.copy_(torch.tensor(sv))
        b.copy_(torch.tensor(BIAS))
        with never_read_on_the_host(s), never_read_on_the_host(b):
            n["src"].send_output("x", tensor.resize(x.permute(2, 0, 1), (64, 64), mode="bilinear",
                                                    dtype=torch.float16, scale=s, bias=b, axis=0,
                                                    fit="letterbox", fill=114), {"m": m})
        x.fill_(255)
        s.fill_(float("nan"))
        b.fill_(7.0)
        want = torch.from_numpy(tensor._numpy_resize(
            src.permute(2, 0, 1).numpy(), (64, 64), mode="bilinear", dtype="float16", scale=sv,
            bias=BIAS, axis=0, inner=inner, lead=lead, fill=114.0))
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, want, f"letterbox {m}")
        del ev
    torch.cuda.synchronize()
    return {"messages": 3}


def scenario_record(n):
    """{"crop": crops normalised along axis 2, "box": the boxes themselves} as one Struct message,
    synchronously and with asynchronous=True followed by sync(): the asynchronous send holds the
    two fields, the boxes once more as the crops' own and the two tables."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    held = None
    for m, asynchronous in enumerate((False, True)):
        src = frame_of(20 + m)
        rows = BOXES[m:] + BOXES[:m]
        x, bx = src.to(dev), torch.tensor(rows, dtype=torch.int32).to(dev)
        s, b = torch.tensor(SCALE).to(dev), torch.tensor(BIAS).to(dev)
        n["src"].sync()
        with never_read_on_the_host(bx), never_read_on_the_host(s):
            n["src"].send_output("x", {"crop": tensor.crops(x, bx, (16, 8), axes=(0, 1), dtype="float16",
                                                            scale=s, bias=b, axis=2), "box": bx},
                                 {"m": m}, asynchronous=asynchronous)
        if asynchronous:
            held = len(n["src"]._async_tensors)
            n["src"].sync()
            assert n["src"]._async_tensors == []
        x.fill_(1)
        bx.fill_(-1)
        s.fill_(0.0)
        b.fill_(float("inf"))
        want = torch.from_numpy(tensor._numpy_crops(src.numpy(), rows, (16, 8), axes=(0, 1), dtype="float16",
                                                    scale=SCALE, bias=BIAS, axis=2))
        assert not want[rows.index((0, 0, 0, 0))].any()  # an empty box: zeros despite the bias
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, {"crop": want, "box": torch.tensor(rows, dtype=torch.int32)}, f"record {m}")
        del ev
    torch.cuda.synchronize()
    return {"held": held}


def scenario_host_receiver(n):
    """A receiver without a GPU gets the staged pyarrow array of from_numpy_resize from a device
    source; frame and tables in host memory take the CPU path of the same send."""
    from dora_amd import tensor
    src = frame_of(30)
    dev = torch.device("cuda", 0)
    kw = dict(axes=(0, 1), mode="bilinear", dtype="float32", axis=2, fill=114.0)
    inner, lead = tensor.letterbox((54, 96), (20, 20))
    for m, (f, s, b) in enumerate(((src.to(dev), torch.tensor(SCALE).to(dev), torch.tensor(BIAS).to(dev)),
                                   (src, SCALE, torch.tensor(BIAS)))):
        n["src"].send_output("y", tensor.resize(f, (20, 20), fit="letterbox", scale=s, bias=b, **kw), {"m": m})
        ev = n["hst"].next(timeout=60)
        assert ev["type"] == "INPUT" and ev["metadata"] == {"m": m} and not ev["on_device"]
        want = tensor.from_numpy_resize(src.numpy(), (20, 20), inner=inner, lead=lead, scale=SCALE,
                                        bias=BIAS, **kw)
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
    src = frame_of(40)
    x = src.to(dev)
    s = torch.tensor(SCALE).to(dev)
    errors = []
    for data in (tensor.resize(x, (8, 8), axes=(0, 1), scale=s, axis=1),
                 tensor.resize(x, (8, 8), axes=(0, 1), scale=s[:2], axis=2),
                 tensor.resize(x, (8, 8), axes=(0, 1), scale=s.double(), axis=2),
                 tensor.resize(x, (8, 8), axes=(0, 1), inner=(9, 8)),
                 tensor.resize(x, (8, 8), axes=(0, 1), bias=float("inf"))):
        try:
            n["src"].send_output("x", data)
            raise AssertionError("a refused model input was sent")
        except DoraGpuError as e:
            errors.append(e.code)
    assert errors == [-1, -1, -4, -1, -1], errors
    sides = 0
    for data in (tensor.resize(x, (8, 8), axes=(0, 1), scale=SCALE, axis=2),
                 tensor.resize(src, (8, 8), axes=(0, 1), scale=s, axis=2)):
        try:
            n["src"].send_output("x", data)
            raise AssertionError("a table on the other side from the values was sent")
        except TypeError as e:
            assert "per-channel table" in str(e), str(e)
            sides += 1
    n["src"].send_output("x", tensor.resize(x, (8, 8), axes=(0, 1), scale=s, axis=2, dtype="float32"),
                         {"m": "after"})
    ev = n["dst"].next(timeout=60)
    assert ev["metadata"] == {"m": "after"}, ev["metadata"]
    check(ev, torch.from_numpy(tensor._numpy_resize(src.numpy(), (8, 8), axes=(0, 1), scale=SCALE, axis=2,
                                                    dtype="float32")), "after")
    del ev
    return {"refused": len(errors), "sides": sides}


def main(report_path):
    report = {}
    lch = launcher_mod.Launcher()  # before HIP is initialised in this process
    try:
        from dora_amd.dataflow import Dataflow
        torch.cuda.set_device(0)
        with Dataflow(DESC, launcher=lch) as df:
            n = nodes(df, {"src": 0, "dst": 0, "hst": -1})
            try:
                for name, fn in [("letterbox", scenario_letterbox), ("record", scenario_record),
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
