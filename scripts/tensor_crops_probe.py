"""Probe: what sending crops costs against what a producer does without the crops send — the boxes
read back to the host, K slices of the frame, K `F.interpolate` calls and a `stack` into fresh
tensors, then the plain send of the result.

Cases, src and sink on GPU 0 of one process, all from one (1080, 1920, 3) uint8 frame and seeded
boxes inside it:

  k16_u8    K = 16 boxes to (16, 128, 64, 3) uint8, bilinear, axes (0, 1)
  k64_f16   K = 64 boxes through permute(2, 0, 1) to (64, 3, 224, 224) float16, bilinear
  whole_u8  K = 1 box, the whole frame, to (1, 640, 640, 3) uint8, bilinear — also against
            `tensor.resize` of the frame to (640, 640, 3): what the per-box path costs

Sends: `--messages` synchronous sends in every one of `--rounds` rounds, the modes alternating
within the round in `--blocks` blocks, so that a change of the machine's state during a run falls
on all alike; compare them round by round:

  torch_then_send   boxes.tolist(), the slices, interpolate, round, clamp, to, stack as the case
                    needs them, then send_output of the result: the yardstick, its torch kernels
                    and its host read inside the clock
  crops_send        send_output("s", tensor.crops(x, boxes, size, ...))
  resize_send       (whole_u8 only) send_output("s", tensor.resize(x, size, ...))

each as the time of the synchronous call of one message (p10 / p50 / p90 us over the round's blocks
of the mode; the sink drains after the clock stops).

One JSON line per measurement goes to `--out`.

    python scripts/tensor_crops_probe.py --out profiles/tensor_crops_probe.jsonl
"""
import argparse
import json
import os
import sys
import threading
import time

FRAME = (1080, 1920, 3)
# name -> (K, permute or None, size, axes, destination)
CASES = {"k16_u8": (16, None, (128, 64), (0, 1), "uint8"),
         "k64_f16": (64, (2, 0, 1), (224, 224), (-2, -1), "float16"),
         "whole_u8": (1, None, (640, 640), (0, 1), "uint8")}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["s"]},
    {"id": "dst", "path": "dynamic", "inputs": {"s": {"source": "src/s", "queue_size": 10}}},
]}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] / 1e3


def boxes_of(name):
    """The case's K boxes as rows (a_lo, b_lo, a_hi, b_hi), every one inside the frame."""
    import numpy as np
    k = CASES[name][0]
    if name == "whole_u8":
        return [(0, 0, FRAME[0], FRAME[1])]
    rng = np.random.default_rng(k)
    h, w = rng.integers(64, 480, k), rng.integers(32, 320, k)
    a, b = rng.integers(0, FRAME[0] - h), rng.integers(0, FRAME[1] - w)
    return np.stack([a, b, a + h, b + w], 1).tolist()


def torch_chain(name, frame, boxes):
    """What a producer runs in place of the crops send, on the tensors it holds: `frame` the
    (1080, 1920, 3) uint8 frame, `boxes` the [K, 4] int32 tensor, both in HBM."""
    import torch
    import torch.nn.functional as F
    _, perm, size, _, dst = CASES[name]
    chw = frame.permute(2, 0, 1)
    out = []
    for a0, b0, a1, b1 in boxes.tolist():  # the host read: a synchronisation with the GPU
        y = F.interpolate(chw[:, a0:a1, b0:b1].unsqueeze(0).float(), size, mode="bilinear",
                          align_corners=False).squeeze(0)
        if dst == "uint8":
            y = y.round().clamp(0, 255).to(torch.uint8)
            out.append(y if perm else y.permute(1, 2, 0))
        else:
            out.append(y.to(torch.float16))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_crops_probe.jsonl"))
    ap.add_argument("--messages", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
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
    from dora_amd import tensor
    from dora_amd.dataflow import Dataflow
    from dora_amd.node import Node
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    frame = torch.randint(0, 256, FRAME, dtype=torch.uint8, device=dev)
    boxes = {name: torch.tensor(boxes_of(name), dtype=torch.int32, device=dev) for name in names}
    torch.cuda.synchronize()
    try:
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
                    _, perm, size, axes, dt = CASES[name]
                    x = frame if perm is None else frame.permute(*perm)
                    bx = boxes[name]
                    make = {"torch_then_send": lambda name=name, bx=bx: torch_chain(name, frame, bx),
                            "crops_send": lambda x=x, bx=bx, size=size, axes=axes, dt=dt:
                                tensor.crops(x, bx, size, axes=axes, dtype=dt)}
                    if name == "whole_u8":
                        make["resize_send"] = lambda x=x, size=size, axes=axes, dt=dt: \
                            tensor.resize(x, size, axes=axes, mode="bilinear", dtype=dt)
                    modes = tuple(make)
                    for m in modes:  # warm up: slots, streams, code objects, the allocator
                        for _ in range(a.warmup):
                            one(make[m])
                    for rnd in range(a.rounds):
                        per = {m: [] for m in modes}
                        for _ in range(a.blocks):
                            for m in modes:
                                per[m] += [one(make[m]) for _ in range(a.messages // a.blocks)]
                        for m in modes:
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
