"""Probe: what sending a normalised or per-channel quantised tensor costs against what a producer
does without the affine send — the torch chain (`.float()`, multiply, add, `.to(dtype)` or round
and clamp) into a fresh tensor, then the plain send of the result — and against the same view as a
scalar-scale cast or quantise, which isolates what the channel stepping and the table loads cost
over the existing body.

Cases, src and sink on GPU 0 of one process, the tables float32 tensors in HBM made once:

  frame_chw     a 1080 x 1920 x 3 uint8 frame permuted to CHW, normalised to float16 (axis 0)
  frame_hwc     the same frame as it lies, normalised to float16 (axis -1)
  act_int8      1 Mi float32 as (16384, 64) to int8, one scale per channel (axis 1)

Modes, `--messages` synchronous sends each in every one of `--rounds` rounds, alternating within
the round in `--blocks` blocks, so that a change of the machine's state during a run falls on all
modes alike; compare the modes round by round:

  torch_then_send   the torch chain, then send_output of its result: the yardstick, its torch
                    kernels inside the clock
  affine_send       send_output("s", tensor.cast / tensor.quantize(.., scale=table, bias=table, axis=..))
  scalar_send       the same view with one scalar scale and no bias (gather_cast_kernel /
                    gather_quant_kernel)

each as the time of the synchronous call of one message (p10 / p50 / p90 us over the round's blocks
of the mode; the sink drains after the clock stops).  One JSON line per (case, mode, round) goes
to `--out`.

    python scripts/tensor_affine_probe.py --out profiles/tensor_affine_probe.jsonl
"""
import argparse
import json
import os
import sys
import threading
import time

CASES = ("frame_chw", "frame_hwc", "act_int8")
MODES = ("torch_then_send", "affine_send", "scalar_send")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["s"]},
    {"id": "dst", "path": "dynamic", "inputs": {"s": {"source": "src/s", "queue_size": 10}}},
]}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] / 1e3


def cases(torch, tensor, names):
    """name -> {mode: callable making the message}."""
    dev = torch.device("cuda", 0)
    mean = torch.tensor([0.485, 0.456, 0.406], dtype=torch.float64)
    std = torch.tensor([0.229, 0.224, 0.225], dtype=torch.float64)
    s = (1 / (255 * std)).float().to(dev)
    b = (-mean / std).float().to(dev)
    out = {}
    for name in names:
        if name.startswith("frame"):
            f = torch.randint(0, 256, (1080, 1920, 3), dtype=torch.uint8, device=dev)
            chw = name == "frame_chw"
            v = f.permute(2, 0, 1) if chw else f
            axis = 0 if chw else -1
            sv, bv = (s.view(3, 1, 1), b.view(3, 1, 1)) if chw else (s, b)
            out[name] = {
                "torch_then_send": lambda v=v, sv=sv, bv=bv: v.float().mul(sv).add(bv).half(),
                "affine_send": lambda v=v, axis=axis: tensor.cast(v, "float16", scale=s, bias=b, axis=axis),
                "scalar_send": lambda v=v: tensor.cast(v, "float16", scale=1 / 255)}
        else:
            x = torch.randn((16384, 64), dtype=torch.float32, device=dev)
            per = (torch.rand(64, dtype=torch.float32) * 50 + 10).to(dev)
            out[name] = {
                "torch_then_send": lambda x=x, per=per: x.mul(per).round().clamp(-128, 127).to(torch.int8),
                "affine_send": lambda x=x, per=per: tensor.quantize(x, "int8", scale=per, axis=1),
                "scalar_send": lambda x=x: tensor.quantize(x, "int8", scale=32.0)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_affine_probe.jsonl"))
    ap.add_argument("--messages", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--cases", default=",".join(CASES))
    a = ap.parse_args()
    names = [c for c in a.cases.split(",") if c]
    rows = []
    import torch  # before dora_amd: one HIP runtime for both (dora_amd/node.py)
    sys.path.insert(0, ROOT)
    from dora_amd import launcher as launcher_mod
    lch = launcher_mod.Launcher()  # before HIP is initialised here
    from dora_amd import tensor
    from dora_amd.dataflow import Dataflow
    from dora_amd.node import Node
    torch.cuda.set_device(0)
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
                made = cases(torch, tensor, names)
                torch.cuda.synchronize()
                for name in names:
                    make = made[name]
                    for mode in MODES:  # warm up: slots, streams, code objects, the allocator
                        for _ in range(a.warmup):
                            one(make[mode])
                    for rnd in range(a.rounds):
                        per = {mode: [] for mode in MODES}
                        for _ in range(a.blocks):
                            for mode in MODES:
                                per[mode] += [one(make[mode]) for _ in range(a.messages // a.blocks)]
                        for mode in MODES:
                            rows.append({"case": name, "mode": mode, "round": rnd,
                                         "messages": len(per[mode]), "blocks": a.blocks,
                                         "sync_us_p10": pct(per[mode], 0.1),
                                         "sync_us_p50": pct(per[mode], 0.5),
                                         "sync_us_p90": pct(per[mode], 0.9)})
                            print(json.dumps(rows[-1]), flush=True)
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
