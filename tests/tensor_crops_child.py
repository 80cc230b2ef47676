"""Child process of test_gpu_tensor_crops_dataflow.py: boxes in HBM cut from a torch frame in HBM
and resized on send by a node of the same process.  torch is imported before dora_amd loads its
library, so that both use one HIP runtime.  Every scenario's outcome goes into the JSON report named
on the command line; the test asserts on it.

    python tests/tensor_crops_child.py REPORT.json
"""
import contextlib
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
from tests.tensor_resize_child import frame_of  # noqa: E402

BOXES = [(3, 5, 40, 60), (-6, 70, 20, 120), (10, 10, 11, 11), (30, 30, 30, 50), (50, 0, 54, 96),
         (0, 0, 0, 0)]


def stated(x, boxes, size, **kw):
    """The statement of record on the CPU, as a torch tensor."""
    from dora_amd import tensor
    return torch.from_numpy(tensor._numpy_crops(x.numpy(), boxes, size, **kw))


@contextlib.contextmanager
def never_read_on_the_host(t):
    """While this holds, `.cpu()`, `.item()`, `.tolist()` and `.numpy()` of tensor `t` raise."""
    saved = {name: getattr(torch.Tensor, name) for name in ("cpu", "item", "tolist", "numpy")}

    def guard(name):
        def method(self, *args, **kw):
            if self.is_cuda and self.data_ptr() == t.data_ptr():
                raise AssertionError(f"the sender called .{name}() on the boxes")
            return saved[name](self, *args, **kw)
        return method
    for name in saved:
        setattr(torch.Tensor, name, guard(name))
    try:
        yield
    finally:
        for name, fn in saved.items():
            setattr(torch.Tensor, name, fn)


def scenario_bare(n):
    """Six boxes of a (54, 96, 3) uint8 frame to (16, 8, 3) uint8, bilinear, frame and boxes
    rewritten before and poisoned after every synchronous send; then the same through
    permute(2, 0, 1) to float16."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    x = torch.empty((54, 96, 3), device=dev, dtype=torch.uint8)
    bx = torch.empty((6, 4), device=dev, dtype=torch.int32)
    for m in range(3):
        src = frame_of(m)
        rows = BOXES[m:] + BOXES[:m]
        x.copy_(src)
        bx.copy_(torch.tensor(rows, dtype=torch.int32))
        with never_read_on_the_host(bx):
            if m < 2:
                n["src"].send_output("x", tensor.crops(x, bx, (16, 8), axes=(0, 1)), {"m": m})
                want = stated(src, rows, (16, 8), axes=(0, 1))
            else:
                n["src"].send_output("x", tensor.crops(x.permute(2, 0, 1), bx, (12, 20),
                                                       dtype="float16"), {"m": m})
                want = stated(src.permute(2, 0, 1), rows, (12, 20), dtype="float16")
        x.fill_(255)
        bx.fill_(7)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, want, f"bare {m}")
        del ev
    torch.cuda.synchronize()
    return {"messages": 3}


def scenario_record(n):
    """{"crop": crops, "box": the boxes themselves, "cls": int64} as one Struct message,
    synchronously and with asynchronous=True followed by sync(): the asynchronous send holds the
    three tensors and the boxes once more as the crops' own."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    held = None
    for m, asynchronous in enumerate((False, True)):
        src = frame_of(20 + m)
        rows = BOXES[m:] + BOXES[:m]
        cls = torch.arange(6, dtype=torch.int64) * 10 + m
        x, bx, c = src.to(dev), torch.tensor(rows, dtype=torch.int32).to(dev), cls.to(dev)
        n["src"].sync()
        with never_read_on_the_host(bx):
            n["src"].send_output("x", {"crop": tensor.crops(x, bx, (16, 8), axes=(0, 1),
                                                            mode="nearest"), "box": bx, "cls": c},
                                 {"m": m}, asynchronous=asynchronous)
        if asynchronous:
            held = len(n["src"]._async_tensors)
            n["src"].sync()
            assert n["src"]._async_tensors == []
        x.fill_(1)
        bx.fill_(-1)
        c.fill_(-1)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, {"crop": stated(src, rows, (16, 8), axes=(0, 1), mode="nearest"),
                   "box": torch.tensor(rows, dtype=torch.int32), "cls": cls}, f"record {m}")
        del ev
    torch.cuda.synchronize()
    return {"held": held}


def scenario_host_receiver(n):
    """A receiver without a GPU gets the staged pyarrow array of from_numpy_crops from a device
    source; frame and boxes in host memory take the CPU path of the same send."""
    from dora_amd import tensor
    src = frame_of(30)
    x = src.to(torch.device("cuda", 0))
    bx = torch.tensor(BOXES, dtype=torch.int32).to(torch.device("cuda", 0))
    for m, (f, b) in enumerate(((x, bx), (src, torch.tensor(BOXES, dtype=torch.int32)))):
        n["src"].send_output("y", tensor.crops(f, b, (5, 7), axes=(0, 1), dtype="float32"), {"m": m})
        ev = n["hst"].next(timeout=60)
        assert ev["type"] == "INPUT" and ev["metadata"] == {"m": m} and not ev["on_device"]
        want = tensor.from_numpy_crops(src.numpy(), BOXES, (5, 7), axes=(0, 1), dtype="float32")
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
    bx = torch.tensor(BOXES, dtype=torch.int32).to(dev)
    errors = []
    for data in (tensor.crops(x, bx, (4, 4), axes=(0, 0)), tensor.crops(x, bx, (4, 4), axes=(0, 3)),
                 tensor.crops(x, bx, (0, 4), axes=(0, 1)), tensor.crops(x, bx.long(), (4, 4), axes=(0, 1)),
                 tensor.crops(x, bx[:, :3], (4, 4), axes=(0, 1)),
                 tensor.crops(x, bx.t().contiguous().t(), (4, 4), axes=(0, 1)),
                 tensor.crops(x.double(), bx, (4, 4)), tensor.crops(x, bx, (4, 4), dtype="int32"),
                 {"a": tensor.crops(x, bx, (4, 4), axes=(0, 1)), "b": tensor.cast(x, "float32")},
                 {"a": tensor.crops(x, bx, (4, 4), axes=(0, 1)), "b": bx[:5]}):
        try:
            n["src"].send_output("x", data)
            raise AssertionError("refused crops were sent")
        except DoraGpuError as e:
            errors.append(e.code)
    assert errors == [-1, -1, -1, -1, -1, -1, -4, -4, -4, -1], errors
    sides = 0
    for data in (tensor.crops(x, bx.cpu(), (4, 4), axes=(0, 1)), tensor.crops(src, bx, (4, 4), axes=(0, 1)),
                 tensor.crops(x, BOXES, (4, 4), axes=(0, 1))):
        try:
            n["src"].send_output("x", data)
            raise AssertionError("boxes on the other side from the frame were sent")
        except TypeError as e:
            assert "boxes live where the frame lives" in str(e), str(e)
            sides += 1
    n["src"].send_output("x", tensor.crops(x, bx, (8, 8), axes=(0, 1)), {"m": "after"})
    ev = n["dst"].next(timeout=60)
    assert ev["metadata"] == {"m": "after"}, ev["metadata"]
    check(ev, stated(src, BOXES, (8, 8), axes=(0, 1)), "after")
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
                for name, fn in [("bare", scenario_bare), ("record", scenario_record),
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
