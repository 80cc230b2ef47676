"""Probe: what sending a model input costs against what a producer does without it — the whole
torch preprocessing chain (`F.interpolate` and its casts, `F.pad`, `mul`, `sub`, `div`, `half`,
for crops the boxes read back to the host and K slices) into fresh tensors, then the plain send of
the result.

Cases, src and sink on GPU 0 of one process, all from one (1080, 1920, 3) uint8 frame, normalised
as (x / 255 - mean[c]) / std[c] by per-channel tables in HBM:

  letterbox_f16   through permute(2, 0, 1) letterboxed into (3, 640, 640) float16, grey 114
  stretch_f16     the same stretched to (3, 640, 640) float16
  k64_f16         64 seeded boxes through permute(2, 0, 1) to (64, 3, 224, 224) float16

Sends: `--messages` synchronous sends in every one of `--rounds` rounds, the modes alternating
within the round in `--blocks` blocks, so that a change of the machine's state during a run falls
on all alike; compare them round by round:

  torch_then_send   the torch chain, then send_output of the result: the yardstick, its torch
                    kernels (and for crops its host read) inside the clock
  prep_send         send_output("s", tensor.resize(.., scale=s, bias=b, axis=0, fit=..)) or
                    tensor.crops(.., scale=s, bias=b, axis=0): one launch
  plain_send        the same resize or crops to float16 without scale, bias and placement: the
                    launch the step rides on (tensor_resize_probe.py / tensor_crops_probe.py)

each as the time of the synchronous call of one message (p10 / p50 / p90 us over the round's blocks
of the mode; the sink drains after the clock stops).

One JSON line per measurement goes to `--out`.

    python scripts/tensor_prep_probe.py --out profiles/tensor_prep_probe.jsonl
"""
import argparse
import json
import os
import sys
import threading
import time

FRAME = (1080, 1920, 3)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# name -> (K or 0, size, fit)
CASES = {"letterbox_f16": (0, (640, 640), "letterbox"),
         "stretch_f16": (0, (640, 640), "stretch"),
         "k64_f16": (64, (224, 224), None)}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["s"]},
    {"id": "dst", "path": "dynamic", "inputs": {"s": {"source": "src/s", "queue_size": 10}}},
]}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] / 1e3


def boxes_of(k):
    """K boxes as rows (a_lo, b_lo, a_hi, b_hi), every one inside the frame."""
    import numpy as np
    rng = np.random.default_rng(k)
    h, w = rng.integers(64, 480, k), rng.integers(32, 320, k)
    a, b = rng.integers(0, FRAME[0] - h), rng.integers(0, FRAME[1] - w)
    return np.stack([a, b, a + h, b + w], 1).tolist()


def torch_chain(name, frame, boxes, mean, std, geometry):
    """What a producer runs in place of the prep send, on the tensors it holds: `frame` the
    (1080, 1920, 3) uint8 frame, `boxes` the [K, 4] int32 tensor, `mean` and `std` (3, 1, 1)
    float32, all in HBM."""
    import torch
    import torch.nn.functional as F
    k, size, fit = CASES[name]
    chw = frame.permute(2, 0, 1)
    if k:
        out = []
        for a0, b0, a1, b1 in boxes.tolist():  # the host read: a synchronisation with the GPU
            y = F.interpolate(chw[:, a0:a1, b0:b1].unsqueeze(0).float(), size, mode="bilinear",
                              align_corners=False).squeeze(0)
            out.append(y)
        return torch.stack(out).div(255.0).sub(mean).div(std).half()
    if fit == "letterbox":
        (ra, rb), (pa, pb) = geometry
        y = F.interpolate(chw.unsqueeze(0).float(), (ra, rb), mode="bilinear", align_corners=False)
        y = F.pad(y, (pb, size[1] - rb - pb, pa, size[0] - ra - pa), value=114.0).squeeze(0)
    else:
        y = F.interpolate(chw.unsqueeze(0).float(), size, mode="bilinear",
                          align_corners=False).squeeze(0)
    return y.div(255.0).sub(mean).div(std).half()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_prep_probe.jsonl"))
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
    x = frame.permute(2, 0, 1)
    mean = torch.tensor(MEAN, device=dev).reshape(3, 1, 1)
    std = torch.tensor(STD, device=dev).reshape(3, 1, 1)
    s = torch.tensor([1.0 / (255.0 * d) for d in STD], device=dev)
    b = torch.tensor([-m / d for m, d in zip(MEAN, STD)], device=dev)
    boxes = torch.tensor(boxes_of(64), dtype=torch.int32, device=dev)
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
                    k, size, fit = CASES[name]
                    geometry = tensor.letterbox(FRAME[:2], size)
                    kw = dict(mode="bilinear", dtype="float16")
                    norm = dict(scale=s, bias=b, axis=0)
                    make = {"torch_then_send": lambda name=name, geometry=geometry:
                            torch_chain(name, frame, boxes, mean, std, geometry)}
                    if k:
                        make["prep_send"] = lambda size=size: tensor.crops(x, boxes, size, **kw, **norm)
                        make["plain_send"] = lambda size=size: tensor.crops(x, boxes, size, **kw)
                    else:
                        make["prep_send"] = lambda size=size, fit=fit: tensor.resize(
                            x, size, fit=fit, fill=114.0, **kw, **norm)
                        make["plain_send"] = lambda size=size: tensor.resize(x, size, **kw)
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
