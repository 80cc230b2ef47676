"""Probe: what sending a class map costs against what a producer does without the argmax send —
`x.argmax(dim).to(dtype)` into fresh tensors, then the plain send of the result.

Cases, src and sink on GPU 0 of one process:

  seg19     (19, 1024, 2048) float16 along 0 to uint8
  seg150    (150, 512, 512) float16 along 0 to uint8
  hwc21     (512, 512, 21) float16 along -1 to uint8
  cls1000   (4096, 1000) float32 along -1 to int32

Sends: `--messages` synchronous sends in every one of `--rounds` rounds, the two modes alternating
within the round in `--blocks` blocks, so that a change of the machine's state during a run falls
on both alike; compare them round by round:

  torch_then_send   x.argmax(dim).to(dtype), then send_output of its result: the yardstick, its
                    torch kernels inside the clock
  argmax_send       send_output("s", tensor.argmax(x, dim, dtype))

each as the time of the synchronous call of one message (p10 / p50 / p90 us over the round's blocks
of the mode; the sink drains after the clock stops).

Launches (`kind: "launch"`): the plan of each case packed `--launches` times back to back on one
stream, per round, as us per launch and source bytes per second, beside a dense copy plan of as
many source bytes on the same stream (`copy_gbs`, the measured ceiling of one read of the logits).

Crossover (`kind: "crossover"`): (4096, C) float32 along -1 to int32 for C in 8 .. 1000 with the
lane body and with the wave body forced (dora_gpu_test_reduce_body), us per launch each, and
(512, 512, 21)-like float16 (65536, C) to uint8 the same way.

One JSON line per measurement goes to `--out`.

    python scripts/tensor_argmax_probe.py --out profiles/tensor_argmax_probe.jsonl
"""
import argparse
import json
import os
import sys
import threading
import time
from ctypes import byref, c_void_p

CASES = {"seg19": ((19, 1024, 2048), "float16", 0, "uint8"),
         "seg150": ((150, 512, 512), "float16", 0, "uint8"),
         "hwc21": ((512, 512, 21), "float16", -1, "uint8"),
         "cls1000": ((4096, 1000), "float32", -1, "int32")}
MODES = ("torch_then_send", "argmax_send")
SWEEP = (8, 16, 32, 64, 96, 128, 192, 256, 512, 1000)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["s"]},
    {"id": "dst", "path": "dynamic", "inputs": {"s": {"source": "src/s", "queue_size": 10}}},
]}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] / 1e3


def reduce_plan(x, axis, dtype):
    """The device reduce plan of torch tensor `x` (dora_gpu_plan_tensor_reduce)."""
    import numpy as np
    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM, REDUCE_ARGMAX, TensorReduce
    from dora_amd.arrow_utils import Plan
    np_dtype = {2: np.float16, 4: np.float32}[x.element_size()]
    t, keep = tensor._describe(x.data_ptr(), tuple(x.shape), list(x.stride()), np_dtype)
    lst, keep2 = tensor._describe_list(None, [t], t, 0, 0)
    reds = (TensorReduce * 1)()
    code, bits, _ = tensor._cast_dtype(dtype)
    reds[0].op, reds[0].axis = REDUCE_ARGMAX, axis % x.dim()
    reds[0].dtype_code, reds[0].dtype_bits = code, bits
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_reduce", lst.fields, 1, reds, ARROW_DEVICE_ROCM, byref(h))
    return Plan(h.value, (lst, keep, keep2, reds, x))


def copy_plan(x):
    """The dense copy plan of the bytes of torch tensor `x` (dora_gpu_plan_tensor)."""
    import numpy as np
    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from dora_amd.arrow_utils import Plan
    t, keep = tensor._describe(x.data_ptr(), (x.numel() * x.element_size(),), None, np.uint8)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor", byref(t), ARROW_DEVICE_ROCM, byref(h))
    return Plan(h.value, (keep, x))


def launches(plan, dst, stream, n):
    """us per launch of `plan` packed `n` times back to back into `dst`."""
    plan.pack(dst.ptr, dst.size, stream)
    stream.sync()
    t0 = time.perf_counter_ns()
    for _ in range(n):
        plan.pack(dst.ptr, dst.size, stream)
    stream.sync()
    return (time.perf_counter_ns() - t0) / n / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_argmax_probe.jsonl"))
    ap.add_argument("--messages", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    names = [c for c in a.cases.split(",") if c]
    rows = []

    def row(**r):
        rows.append(r)
        print(json.dumps(r), flush=True)

    import torch  # before dora_amd: one HIP runtime for both (dora_amd/node.py)
    sys.path.insert(0, ROOT)
    from dora_amd import launcher as launcher_mod
    lch = launcher_mod.Launcher()  # before HIP is initialised here
    from dora_amd import _lib, device, tensor
    from dora_amd.dataflow import Dataflow
    from dora_amd.device import DeviceBuffer
    from dora_amd.node import Node
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    made = {}
    for name in names:
        shape, dt, axis, idx = CASES[name]
        made[name] = (torch.randn(shape, dtype=getattr(torch, dt), device=dev), axis, idx)
    torch.cuda.synchronize()
    try:
        # the launches on their own, and the crossover sweep
        stream = device.Stream()
        dst = DeviceBuffer(96 << 20)
        try:
            for name in names:
                x, axis, idx = made[name]
                nbytes = x.numel() * x.element_size()
                with reduce_plan(x, axis, idx) as p, copy_plan(x) as c:
                    for rnd in range(a.rounds):
                        us, cus = launches(p, dst, stream, a.launches), launches(c, dst, stream, a.launches)
                        row(kind="launch", case=name, round=rnd, launch_us=us,
                            source_gbs=nbytes / us / 1e3, copy_us=cus, copy_gbs=nbytes / cus / 1e3)
            for rows_, dt, idx, label in ((4096, torch.float32, "int32", "f32_4096xC"),
                                          (65536, torch.float16, "uint8", "f16_65536xC")):
                for c in SWEEP:
                    if idx == "uint8" and c > 256:
                        continue
                    x = torch.randn((rows_, c), dtype=dt, device=dev)
                    torch.cuda.synchronize()
                    with reduce_plan(x, -1, idx) as p:
                        for rnd in range(a.rounds):
                            got = {}
                            for mode, body in ((1, "lane"), (2, "wave")):
                                _lib.call("dora_gpu_test_reduce_body", mode)
                                got[body] = launches(p, dst, stream, a.launches)
                            _lib.call("dora_gpu_test_reduce_body", 0)
                            row(kind="crossover", case=label, c=c, round=rnd, lane_us=got["lane"],
                                wave_us=got["wave"])
        finally:
            _lib.call("dora_gpu_test_reduce_body", 0)
            dst.free()
            stream.close()
        # the sends
        with Dataflow(DESC, launcher=lch) as df:
            n = {}
            ts = [threading.Thread(target=lambda i=i: n.__setitem__(i, Node(i, dataflow=df.shm, device=0)))
                  for i in ("src", "dst")]
            [t.start() for t in ts]
            [t.join(90) for t in ts]
            tx, rx = n["src"], n["dst"]

            def one(make):
                """One message; ns of the synchronous call, the message's making included."""
                t0 = time.perf_counter_ns()
                tx.send_output("s", make())
                dt = time.perf_counter_ns() - t0
                ev = rx.next(timeout=60)
                assert ev["type"] == "INPUT"
                del ev
                return dt

            try:
                for name in names:
                    x, axis, idx = made[name]
                    tdt = getattr(torch, idx)
                    make = {"torch_then_send": lambda x=x, axis=axis, tdt=tdt: x.argmax(axis).to(tdt),
                            "argmax_send": lambda x=x, axis=axis, idx=idx: tensor.argmax(x, axis, idx)}
                    for mode in MODES:  # warm up: slots, streams, code objects, the allocator
                        for _ in range(a.warmup):
                            one(make[mode])
                    for rnd in range(a.rounds):
                        per = {mode: [] for mode in MODES}
                        for _ in range(a.blocks):
                            for mode in MODES:
                                per[mode] += [one(make[mode]) for _ in range(a.messages // a.blocks)]
                        for mode in MODES:
                            row(kind="send", case=name, mode=mode, round=rnd,
                                messages=len(per[mode]), blocks=a.blocks,
                                sync_us_p10=pct(per[mode], 0.1), sync_us_p50=pct(per[mode], 0.5),
                                sync_us_p90=pct(per[mode], 0.9))
            finally:
                for node in n.values():
                    node.close()
    finally:
        lch.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
