"""Probe: what sending a converted tensor costs against what a producer does without
`tensor.cast`: `x.to(dtype)` (and `.mul(scale)`) in torch into a fresh tensor, then the plain
tensor or struct send of the result.

Cases, src and sink on GPU 0 of one process:

  frame_dense     a 1080 x 1920 x 3 uint8 frame, as it lies, to float16 with scale 1/255
  frame_chw       the same frame permuted to CHW (the cast's element path)
  f32_to_f16      1 Mi float32 to float16
  bf16_to_f32     1 Mi bfloat16 to float32
  detector_300    {bbox: out[:, :4], conf: out[:, 4] of a (300, 6) float16 to float32, cls: int64}

Modes, `--messages` synchronous sends each in every one of `--rounds` rounds, alternating within
the round in `--blocks` blocks (two-step, fused, two-step, ..), so that a change of the machine's
state during a run falls on both modes alike; compare the modes round by round:

  torch_then_send   send_output("s", x.float().mul(s).to(dst)) (x.to(dst) without a scale; a bf16
                    source can be sent no other way): the yardstick, its torch kernels inside the
                    clock
  cast_send         send_output("s", tensor.cast(x, dst, scale))

each as the time of the synchronous call of one message (p10 / p50 / p90 us over the round's
blocks of the mode; the sink drains after the clock stops).  One JSON line per (case, mode,
round) goes to `--out`, with the algorithmic bytes of the mode: the fused send reads S source
bytes and writes D; the two-step path reads S, writes D, reads D and writes D (its intermediate
float32, where it has one, not counted).

    python scripts/tensor_cast_probe.py --out profiles/tensor_cast_probe.jsonl
"""
import argparse
import json
import os
import sys
import threading
import time

CASES = ("frame_dense", "frame_chw", "f32_to_f16", "bf16_to_f32", "detector_300")
MODES = ("torch_then_send", "cast_send")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESC = {"nodes": [
    {"id": "src", "path": "dynamic", "outputs": ["s"]},
    {"id": "dst", "path": "dynamic", "inputs": {"s": {"source": "src/s", "queue_size": 10}}},
]}


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))] / 1e3


def cases(torch, tensor, names):
    """name -> ({mode: callable making the message}, source bytes S, destination bytes D)."""
    dev = torch.device("cuda", 0)
    s255 = 1 / 255
    out = {}
    for name in names:
        if name.startswith("frame"):
            f = torch.randint(0, 256, (1080, 1920, 3), dtype=torch.uint8, device=dev)
            v = f if name == "frame_dense" else f.permute(2, 0, 1)
            out[name] = ({"torch_then_send": lambda v=v: v.float().mul(s255).to(torch.float16),
                          "cast_send": lambda v=v: tensor.cast(v, torch.float16, scale=s255)},
                         v.numel(), 2 * v.numel())
        elif name == "f32_to_f16":
            x = torch.randn(1 << 20, dtype=torch.float32, device=dev)
            out[name] = ({"torch_then_send": lambda x=x: x.to(torch.float16),
                          "cast_send": lambda x=x: tensor.cast(x, torch.float16)},
                         4 * x.numel(), 2 * x.numel())
        elif name == "bf16_to_f32":
            x = torch.randn(1 << 20, dtype=torch.float32, device=dev).to(torch.bfloat16)
            out[name] = ({"torch_then_send": lambda x=x: x.to(torch.float32),
                          "cast_send": lambda x=x: tensor.cast(x, torch.float32)},
                         2 * x.numel(), 4 * x.numel())
        else:
            o = torch.randn((300, 6), dtype=torch.float32, device=dev).to(torch.float16)
            cls = torch.randint(0, 80, (300,), dtype=torch.int64, device=dev)
            out[name] = ({"torch_then_send": lambda o=o, cls=cls: {"bbox": o[:, :4].float(),
                                                                   "conf": o[:, 4].float(), "cls": cls},
                          "cast_send": lambda o=o, cls=cls: {"bbox": tensor.cast(o[:, :4], torch.float32),
                                                             "conf": tensor.cast(o[:, 4], torch.float32),
                                                             "cls": cls}},
                         300 * 5 * 2 + 300 * 8, 300 * 5 * 4 + 300 * 8)
    return out


def algorithmic_bytes(s, d, mode):
    if mode == "cast_send":
        return {"read": s, "written": d}
    return {"read": s + d, "written": 2 * d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_cast_probe.jsonl"))
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
