"""Probe: what sending a quantised tensor costs against what a producer does without
`tensor.quantize`: `x.float().mul(s).round().clamp(lo - zp, hi - zp).add(zp).to(dtype)` in torch
into fresh tensors, then the plain tensor or struct send of the result.

Cases, src and sink on GPU 0 of one process:

  frame_dense     a 1080 x 1920 x 3 float16 frame in [0, 1], as it lies, to uint8 with scale 255
  frame_hwc       the same values held as 3 x 1080 x 1920 and permuted to HWC (the element path)
  depth_u16       1 Mi float32 to uint16 with scale 1000
  act_i8          1 Mi float32 to int8 (no scale)
  detector_300    {bbox: out[:, :4] float32, conf: out[:, 4] quantised to uint8 * 255, cls: int64}
                  of a (300, 6) float32

Modes, `--messages` synchronous sends each in every one of `--rounds` rounds, alternating within
the round in `--blocks` blocks (two-step, fused, two-step, ..), so that a change of the machine's
state during a run falls on both modes alike; compare the modes round by round:

  torch_then_send   the yardstick above, its torch kernels inside the clock
  quant_send        send_output("s", tensor.quantize(x, dtype, scale))

each as the time of the synchronous call of one message (p10 / p50 / p90 us over the round's
blocks of the mode; the sink drains after the clock stops).  One JSON line per (case, mode,
round) goes to `--out`, with the algorithmic bytes of the mode: the fused send reads S source
bytes and writes D; the two-step path reads S, writes D, reads D and writes D (its float32
intermediates not counted).

    python scripts/tensor_quant_probe.py --out profiles/tensor_quant_probe.jsonl
"""
import argparse
import json
import os
import sys
import threading
import time

CASES = ("frame_dense", "frame_hwc", "depth_u16", "act_i8", "detector_300")
MODES = ("torch_then_send", "quant_send")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["s"]},
    {"id": "dst", "path": "dynamic", "inputs": {"s": {"source": "src/s", "queue_size": 10}}},
]}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] / 1e3


def two_step(torch, x, dtype, scale, zp=0):
    info = torch.iinfo(dtype)
    y = x.float()
    if scale is not None:
        y = y.mul(scale)
    return y.round().clamp(info.min - zp, info.max - zp).add(zp).to(dtype)


def cases(torch, tensor, names):
    """name -> ({mode: callable making the message}, source bytes S, destination bytes D)."""
    dev = torch.device("cuda", 0)
    out = {}
    for name in names:
        if name.startswith("frame"):
            if name == "frame_dense":
                v = torch.rand((1080, 1920, 3), device=dev).to(torch.float16)
            else:
                v = torch.rand((3, 1080, 1920), device=dev).to(torch.float16).permute(1, 2, 0)
            out[name] = ({"torch_then_send": lambda v=v: two_step(torch, v, torch.uint8, 255.0),
                          "quant_send": lambda v=v: tensor.quantize(v, torch.uint8, scale=255)},
                         2 * v.numel(), v.numel())
        elif name == "depth_u16":
            x = torch.rand(1 << 20, dtype=torch.float32, device=dev) * 80
            out[name] = ({"torch_then_send": lambda x=x: two_step(torch, x, torch.uint16, 1000.0),
                          "quant_send": lambda x=x: tensor.quantize(x, torch.uint16, scale=1000)},
                         4 * x.numel(), 2 * x.numel())
        elif name == "act_i8":
            x = torch.randn(1 << 20, dtype=torch.float32, device=dev) * 40
            out[name] = ({"torch_then_send": lambda x=x: two_step(torch, x, torch.int8, None),
                          "quant_send": lambda x=x: tensor.quantize(x, torch.int8)},
                         4 * x.numel(), x.numel())
        else:
            o = torch.rand((300, 6), dtype=torch.float32, device=dev)
            cls = torch.randint(0, 80, (300,), dtype=torch.int64, device=dev)
            out[name] = ({"torch_then_send": lambda o=o, cls=cls: {
                              "bbox": o[:, :4], "conf": two_step(torch, o[:, 4], torch.uint8, 255.0),
                              "cls": cls},
                          "quant_send": lambda o=o, cls=cls: {
                              "bbox": o[:, :4], "conf": tensor.quantize(o[:, 4], torch.uint8, 255),
                              "cls": cls}},
                         300 * 5 * 4 + 300 * 8, 300 * 4 * 4 + 300 + 300 * 8)
    return out


def algorithmic_bytes(s, d, mode):
    if mode == "quant_send":
        return {"read": s, "written": d}
    return {"read": s + d, "written": 2 * d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_quant_probe.jsonl"))
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
                    make, s, d = made[name]
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
                                         "algorithmic_bytes": algorithmic_bytes(s, d, mode),
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
