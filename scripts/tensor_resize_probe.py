"""Probe: what sending a resized frame costs against what a producer does without the resize send —
the torch chain around `F.interpolate` into fresh tensors, then the plain send of its result
(DESIGN §4).

Cases, src and sink on GPU 0 of one process:

  hwc_u8     (1080, 1920, 3) uint8 to (640, 640, 3) uint8, bilinear, axes (0, 1)
  chw_f16    the same frame through permute(2, 0, 1) to (3, 640, 640) float16, bilinear
  batch_f16  (8, 3, 720, 1280) float16 to (8, 3, 224, 224) float16, nearest

Sends: `--messages` synchronous sends in every one of `--rounds` rounds, the two modes alternating
within the round in `--blocks` blocks, so that a change of the machine's state during a run falls
on both alike; compare them round by round:

  torch_then_send   the torch chain (permute, float, interpolate, round, clamp, to, permute,
                    contiguous as the case needs them), then send_output of its result: the
                    yardstick, its torch kernels inside the clock
  resize_send       send_output("s", tensor.resize(x, size, ...))

each as the time of the synchronous call of one message (p10 / p50 / p90 us over the round's blocks
of the mode; the sink drains after the clock stops).

Launches (`kind: "launch"`): the plan of each case packed `--launches` times back to back on one
stream, per round, as us per launch and output bytes per second.

One JSON line per measurement goes to `--out`.

    python scripts/tensor_resize_probe.py --out profiles/tensor_resize_probe.jsonl
"""
import argparse
import json
import os
import sys
import threading
import time
from ctypes import byref, c_void_p

# name -> (shape, dtype, permute or None, size, axes, mode, destination)
CASES = {"hwc_u8": ((1080, 1920, 3), "uint8", None, (640, 640), (0, 1), "bilinear", "uint8"),
         "chw_f16": ((1080, 1920, 3), "uint8", (2, 0, 1), (640, 640), (-2, -1), "bilinear", "float16"),
         "batch_f16": ((8, 3, 720, 1280), "float16", None, (224, 224), (-2, -1), "nearest", "float16")}
MODES = ("torch_then_send", "resize_send")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["s"]},
    {"id": "dst", "path": "dynamic", "inputs": {"s": {"source": "src/s", "queue_size": 10}}},
]}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] / 1e3


def resize_plan(x, size, axes, mode, dtype):
    """The device resize plan of torch tensor `x` (dora_gpu_plan_tensor_resize)."""
    import numpy as np
    from dora_amd import _lib, tensor
    from dora_amd._lib import ARROW_DEVICE_ROCM
    from dora_amd.arrow_utils import Plan
    np_dtype = {1: np.uint8, 2: np.float16, 4: np.float32}[x.element_size()]
    t, keep = tensor._describe(x.data_ptr(), tuple(x.shape), list(x.stride()), np_dtype)
    lst, keep2 = tensor._describe_list(None, [t], t, 0, 0)
    arr = tensor._describe_entries([tensor.resize(x, size, axes=axes, mode=mode, dtype=dtype)],
                                    tensor.Resized)
    h = c_void_p()
    _lib.call("dora_gpu_plan_tensor_resize", lst.fields, 1, arr, ARROW_DEVICE_ROCM, byref(h))
    return Plan(h.value, (lst, keep, keep2, arr, x))


def launches(plan, dst, stream, n):
    """us per launch of `plan` packed `n` times back to back into `dst`."""
    plan.pack(dst.ptr, dst.size, stream)
    stream.sync()
    t0 = time.perf_counter_ns()
    for _ in range(n):
        plan.pack(dst.ptr, dst.size, stream)
    stream.sync()
    return (time.perf_counter_ns() - t0) / n / 1e3


def torch_chain(name, x):
    """What a producer runs in place of the resize send, on the tensor it holds."""
    import torch
    import torch.nn.functional as F
    _, _, _, size, _, mode, _ = CASES[name]
    if name == "hwc_u8":
        y = F.interpolate(x.permute(2, 0, 1).unsqueeze(0).float(), size, mode=mode, align_corners=False)
        return y.round().clamp(0, 255).to(torch.uint8).squeeze(0).permute(1, 2, 0).contiguous()
    if name == "chw_f16":
        y = F.interpolate(x.unsqueeze(0).float(), size, mode=mode, align_corners=False)
        return y.to(torch.float16).squeeze(0)
    return F.interpolate(x, size, mode=mode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_resize_probe.jsonl"))
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
    from dora_amd import device, tensor
    from dora_amd.dataflow import Dataflow
    from dora_amd.device import DeviceBuffer
    from dora_amd.node import Node
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    made = {}
    for name in names:
        shape, dt, perm, size, axes, mode, dst = CASES[name]
        if dt == "uint8":
            x = torch.randint(0, 256, shape, dtype=torch.uint8, device=dev)
        else:
            x = torch.randn(shape, dtype=getattr(torch, dt), device=dev)
        made[name] = x if perm is None else x.permute(*perm)
    torch.cuda.synchronize()
    try:
        stream = device.Stream()
        dst = DeviceBuffer(16 << 20)
        try:
            for name in names:
                _, _, _, size, axes, mode, dt = CASES[name]
                with resize_plan(made[name], size, axes, mode, dt) as p:
                    for rnd in range(a.rounds):
                        us = launches(p, dst, stream, a.launches)
                        row(kind="launch", case=name, round=rnd, launch_us=us, output_bytes=p.size,
                            output_gbs=p.size / us / 1e3)
        finally:
            dst.free()
            stream.close()
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
                    _, _, _, size, axes, mode, dt = CASES[name]
                    x = made[name]
                    make = {"torch_then_send": lambda x=x, name=name: torch_chain(name, x),
                            "resize_send": lambda x=x, size=size, axes=axes, mode=mode, dt=dt:
                                tensor.resize(x, size, axes=axes, mode=mode, dtype=dt)}
                    for m in MODES:  # warm up: slots, streams, code objects, the allocator
                        for _ in range(a.warmup):
                            one(make[m])
                    for rnd in range(a.rounds):
                        per = {m: [] for m in MODES}
                        for _ in range(a.blocks):
                            for m in MODES:
                                per[m] += [one(make[m]) for _ in range(a.messages // a.blocks)]
                        for m in MODES:
                            row(kind="send", case=name, mode=m, round=rnd, messages=len(per[m]),
                                blocks=a.blocks, sync_us_p10=pct(per[m], 0.1),
                                sync_us_p50=pct(per[m], 0.5), sync_us_p90=pct(per[m], 0.9))
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
