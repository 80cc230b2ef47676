"""Child process of test_gpu_tensor_resize_dataflow.py: torch frames in HBM resized on send by a
node of the same process.  torch is imported before dora_amd loads its library, so that both use
one HIP runtime.  Every scenario's outcome goes into the JSON report named on the command line;
the test asserts on it.

    python tests/tensor_resize_child.py REPORT.json
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


def frame_of(m, shape=(54, 96, 3)):
    g = torch.Generator().manual_seed(m)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def stated(x, size, **kw):
    """The statement of record on the CPU, as a torch tensor."""
    from dora_amd import tensor
    return torch.from_numpy(tensor._numpy_resize(x.numpy(), size, **kw))


def scenario_hwc(n):
    """A (54, 96, 3) uint8 frame to (32, 32, 3) uint8, bilinear, rewritten before and poisoned
    after every synchronous send."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    x = torch.empty((54, 96, 3), device=dev, dtype=torch.uint8)
    for m in range(3):
        src = frame_of(m)
        x.copy_(src)
        n["src"].send_output("x", tensor.resize(x, (32, 32), axes=(0, 1), mode="bilinear"), {"m": m})
        x.fill_(255)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, stated(src, (32, 32), axes=(0, 1), mode="bilinear"), f"hwc {m}")
        del ev
    torch.cuda.synchronize()
    return {"messages": 3}


def scenario_chw(n):
    """The same frame through permute(2, 0, 1) to (3, 20, 28) float16, bilinear."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    for m in range(2):
        src = frame_of(10 + m)
        x = src.to(dev)
        n["src"].send_output("x", tensor.resize(x.permute(2, 0, 1), (20, 28), mode="bilinear",
                                                dtype="float16"), {"m": m})
        x.fill_(0)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, stated(src.permute(2, 0, 1), (20, 28), mode="bilinear", dtype="float16"),
              f"chw {m}")
        del ev
    torch.cuda.synchronize()
    return {"messages": 2}


def scenario_record(n):
    """A dict of nearest thumbnails of a batch and a plain int64 field, synchronously and with
    asynchronous=True followed by sync(): the asynchronous send holds both tensors."""
    from dora_amd import tensor
    dev = torch.device("cuda", 0)
    held = None
    for m, asynchronous in enumerate((False, True)):
        src = frame_of(20 + m, (4, 36, 64, 3))
        stamps = torch.arange(4, dtype=torch.int64) * 1000 + m
        x, s = src.to(dev), stamps.to(dev)
        n["src"].sync()
        n["src"].send_output("x", {"thumb": tensor.resize(x, (9, 16), axes=(1, 2)), "stamp": s},
                             {"m": m}, asynchronous=asynchronous)
        if asynchronous:
            held = len(n["src"]._async_tensors)
            n["src"].sync()
            assert n["src"]._async_tensors == []
        x.fill_(1)
        s.fill_(-1)
        ev = n["dst"].next(timeout=60)
        assert ev["metadata"] == {"m": m}, ev["metadata"]
        check(ev, {"thumb": stated(src, (9, 16), axes=(1, 2)), "stamp": stamps}, f"record {m}")
        del ev
    torch.cuda.synchronize()
    return {"held": held}


def scenario_host_source(n):
    """A frame in host memory takes the CPU path of the same send; a receiver without a GPU gets
    the staged pyarrow array of from_numpy_resize from a host and from a device source."""
    from dora_amd import tensor
    src = frame_of(30)
    n["src"].send_output("y", tensor.resize(src, (17, 23), axes=(0, 1), mode="bilinear",
                                            dtype="float32"), {"m": "host"})
    ev = n["hst"].next(timeout=60)
    assert ev["type"] == "INPUT" and ev["metadata"] == {"m": "host"}, ev["metadata"]
    want = tensor.from_numpy_resize(src.numpy(), (17, 23), axes=(0, 1), mode="bilinear",
                                    dtype="float32")
    assert ev["value"].type == want.type and ev["value"].equals(want)
    del ev
    x = src.to(torch.device("cuda", 0))
    n["src"].send_output("y", tensor.resize(x, (5, 7), axes=(0, 1), mode="bilinear"), {"m": "hst"})
    ev = n["hst"].next(timeout=60)
    assert ev["type"] == "INPUT" and ev["metadata"] == {"m": "hst"} and not ev["on_device"]
    want = tensor.from_numpy_resize(src.numpy(), (5, 7), axes=(0, 1), mode="bilinear")
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
    errors = []
    for data in (tensor.resize(x, (4, 4), axes=(0, 0)), tensor.resize(x, (4, 4), axes=(0, 3)),
                 tensor.resize(x[0, 0], (4, 4), axes=(0, 0)), tensor.resize(x, (0, 4)),
                 tensor.resize(x.double(), (4, 4)), tensor.resize(x, (4, 4), dtype="int32"),
                 {"a": tensor.resize(x, (54, 4), axes=(0, 1)), "b": tensor.cast(x, "float32")}):
        try:
            n["src"].send_output("x", data)
            raise AssertionError("a refused resize was sent")
        except DoraGpuError as e:
            errors.append(e.code)
    assert errors == [-1, -1, -1, -1, -4, -4, -4], errors
    n["src"].send_output("x", tensor.resize(x, (8, 8), axes=(0, 1)), {"m": "after"})
    ev = n["dst"].next(timeout=60)
    assert ev["metadata"] == {"m": "after"}, ev["metadata"]
    check(ev, stated(src, (8, 8), axes=(0, 1)), "after")
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
                for name, fn in [("hwc", scenario_hwc), ("chw", scenario_chw),
                                 ("record", scenario_record), ("host_source", scenario_host_source),
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
